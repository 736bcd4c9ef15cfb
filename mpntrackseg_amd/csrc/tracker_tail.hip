// The tail of the sliding-window inference, after the averaged directed edge scores:
//   overall_node_preds / overall_num_node_preds   reference tracker/mpn_tracker.py:132,162-165,199-200,209-210
//   to_undirected_graph                           reference utils/graph.py:165-186
//   to_lightweight_graph (the edge pruning)       reference utils/graph.py:204-207
// The reference sorts the two rows of edge_index, calls torch.unique(dim=1, return_inverse=True) and scatter_mean.  Here
// every directed edge gets the key (min << 32) | max; ONE stable radix sort of (key, edge id) puts the copies of a pair
// next to each other in ascending edge id, the run heads are the unique pairs in torch.unique's column order, and each
// run is summed front to back and divided by its length -- no atomics, the same bits on every call, and for the normal
// run of two exactly the reference's (a + b) / 2.
// The node-mask accumulators are plain streams over contiguous rows (16-byte accesses, grid-stride, one launch per
// window: windows overlap in nodes, the stream orders them).
#include "common.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace mpnhip {
namespace {

__global__ void k_pair_keys(const int64_t* __restrict__ ei, int64_t E, unsigned long long* __restrict__ keys, int* __restrict__ vals) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const unsigned r = (unsigned)ei[e], c = (unsigned)ei[E + e];
    const unsigned lo = r < c ? r : c, hi = r < c ? c : r;
    keys[e] = ((unsigned long long)lo << 32) | hi;
    vals[e] = (int)e;
}

__global__ void k_run_heads(const unsigned long long* __restrict__ skeys, int64_t E, int* __restrict__ heads) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= E) return;
    heads[i] = (i == 0 || skeys[i] != skeys[i - 1]) ? 1 : 0;
}

// run_no[i] = (number of heads in [0, i]) - 1 = column of the pair in the unique list; inverse = torch.unique's inverse map
__global__ void k_inverse(const int* __restrict__ svals, const int* __restrict__ run_no, int64_t E, int* __restrict__ inverse,
                          int* __restrict__ n_unique) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= E) return;
    const int u = run_no[i] - 1;
    inverse[svals[i]] = u;
    if (i == E - 1) n_unique[0] = u + 1;
}

// one thread per run head: the pair's end points, and the run's mean in ascending original edge id (the sort is stable)
__global__ void k_merge_fill(const unsigned long long* __restrict__ skeys, const int* __restrict__ svals, const int* __restrict__ run_no,
                             int64_t E, int64_t U, int64_t* __restrict__ ei_u, const float* __restrict__ attr,
                             float* __restrict__ attr_u) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= E) return;
    const int u = run_no[i] - 1;
    if (i > 0 && run_no[i - 1] - 1 == u) return;   // not a head
    if (u < 0 || u >= U) return;                   // (a count that is not this sort's: write nothing)
    if (ei_u) {
        ei_u[u] = (int64_t)(skeys[i] >> 32);
        ei_u[U + u] = (int64_t)(skeys[i] & 0xFFFFFFFFull);
    }
    if (attr) {
        float sum = 0.f;
        int64_t j = i;
        for (; j < E && run_no[j] - 1 == u; ++j) sum += attr[svals[j]];
        attr_u[u] = sum / (float)(j - i);
    }
}

// edges_mask = edge_preds >= threshold (utils/graph.py:205); NaN compares false, as in torch
__global__ void k_threshold(const float* __restrict__ preds, int64_t n, float thr, unsigned char* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    flags[i] = preds[i] >= thr ? 1 : 0;
}

__device__ __forceinline__ float sigmoidf(float v) { return 1.f / (1.f + expf(-v)); }

// overall[0 : n * row_len] += sigmoid(logits), count[0 : n] += 1; both already offset to the window's first node.
// VEC: the block of rows as float4 (total % 4 == 0, both pointers 16-byte aligned)
template <bool VEC>
__global__ __launch_bounds__(256) void k_node_accumulate(const float* __restrict__ logits, int64_t n_rows, int64_t total,
                                                         float* __restrict__ overall, float* __restrict__ count) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = tid; r < n_rows; r += stride) count[r] += 1.f;
    if (VEC) {
        const float4* src = reinterpret_cast<const float4*>(logits);
        float4* dst = reinterpret_cast<float4*>(overall);
        for (int64_t i = tid; i < total / 4; i += stride) {
            const float4 l = src[i];
            float4 o = dst[i];
            o.x += sigmoidf(l.x); o.y += sigmoidf(l.y); o.z += sigmoidf(l.z); o.w += sigmoidf(l.w);
            dst[i] = o;
        }
    } else {
        for (int64_t i = tid; i < total; i += stride) overall[i] += sigmoidf(logits[i]);
    }
}

// out[r, :] = overall[r, :] / count[r]  (torch.div, mpn_tracker.py:209): count 0 gives 0 / 0 = NaN and stays NaN
template <bool VEC>
__global__ __launch_bounds__(256) void k_node_average(const float* __restrict__ overall, const float* __restrict__ count, int64_t total,
                                                      int64_t row_len, float* __restrict__ out) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    if (VEC) {   // row_len % 4 == 0: a float4 never straddles two rows
        const float4* src = reinterpret_cast<const float4*>(overall);
        float4* dst = reinterpret_cast<float4*>(out);
        for (int64_t i = tid; i < total / 4; i += stride) {
            const float c = count[(i * 4) / row_len];
            float4 o = src[i];
            o.x /= c; o.y /= c; o.z /= c; o.w /= c;
            dst[i] = o;
        }
    } else {
        for (int64_t i = tid; i < total; i += stride) out[i] = overall[i] / count[i / row_len];
    }
}

static size_t sort_temp(int64_t n) {
    size_t bytes = 0;
    unsigned long long* k = nullptr;
    int* v = nullptr;
    (void)rocprim::radix_sort_pairs(nullptr, bytes, k, k, v, v, (size_t)(n > 0 ? n : 1), 0, 64, (hipStream_t)0);
    return bytes;
}
static size_t scan_temp(int64_t n) {
    size_t bytes = 0;
    int* p = nullptr;
    (void)rocprim::inclusive_scan(nullptr, bytes, p, p, (size_t)(n > 0 ? n : 1), rocprim::plus<int>(), (hipStream_t)0);
    return bytes;
}

// what mpnhip_undirected_merge_sort leaves at the head of the workspace for mpnhip_undirected_merge_fill
struct MergeView {
    unsigned long long* skeys;
    int* svals;
    int* run_no;
    char* rest;
};
static MergeView merge_view(void* workspace, int64_t E) {
    char* w = static_cast<char*>(workspace);
    MergeView v;
    v.skeys = reinterpret_cast<unsigned long long*>(w); w += align_up((size_t)E * 8, 256);
    v.svals = reinterpret_cast<int*>(w); w += align_up((size_t)E * 4, 256);
    v.run_no = reinterpret_cast<int*>(w); w += align_up((size_t)E * 4, 256);
    v.rest = w;
    return v;
}

// blocks of 256 threads for a grid-stride stream over `items` work items: enough to fill the chip, never more than the work
static unsigned stream_blocks(int64_t items) {
    static int cus = 0;
    if (cus == 0) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0)
            cus = n;
        else
            cus = 256;
    }
    const int64_t need = (items + 255) / 256, cap = (int64_t)cus * 8;
    return (unsigned)(need < 1 ? 1 : (need < cap ? need : cap));
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
}  // namespace mpnhip

using namespace mpnhip;

extern "C" size_t mpnhip_undirected_merge_workspace_bytes(int64_t n_edges) {
    if (n_edges <= 0) return 0;
    const size_t E = (size_t)n_edges;
    const size_t tmp = sort_temp(n_edges) > scan_temp(n_edges) ? sort_temp(n_edges) : scan_temp(n_edges);
    // sorted keys / ids / run numbers (kept for the fill), unsorted keys / ids / head flags, rocprim's scratch
    return 2 * align_up(E * 8, 256) + 4 * align_up(E * 4, 256) + align_up(tmp, 256) + 256;
}

extern "C" int mpnhip_undirected_merge_sort(const int64_t* edge_index, int64_t n_edges, int64_t n_nodes, int32_t* inverse,
                                            int32_t* n_unique, void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(n_edges >= 0 && n_edges < (1LL << 30) && n_nodes >= 0 && n_nodes <= (1LL << 32), "undirected_merge_sort: bad sizes");
    MPN_CHECK_ARG(n_unique, "undirected_merge_sort: null n_unique");
    if (n_edges == 0) {
        MPN_HIP(hipMemsetAsync(n_unique, 0, 4, stream));
        return MPNHIP_OK;
    }
    MPN_CHECK_ARG(edge_index && inverse, "undirected_merge_sort: null pointer");
    if (!workspace || workspace_bytes < mpnhip_undirected_merge_workspace_bytes(n_edges)) {
        set_error("undirected_merge_sort: workspace %zu < %zu", workspace_bytes, mpnhip_undirected_merge_workspace_bytes(n_edges));
        return MPNHIP_ERR_WORKSPACE;
    }
    const int64_t E = n_edges;
    MergeView v = merge_view(workspace, E);
    char* w = v.rest;
    auto take = [&](size_t bytes) { char* p = w; w += align_up(bytes, 256); return p; };
    auto* keys = reinterpret_cast<unsigned long long*>(take((size_t)E * 8));
    int* vals = reinterpret_cast<int*>(take((size_t)E * 4));
    int* heads = reinterpret_cast<int*>(take((size_t)E * 4));
    void* tmp = w;
    // the key's low word holds max(r, c) < n_nodes and its high word min(r, c): only the bits a node id needs are sorted
    unsigned id_bits = 32;
    if (n_nodes > 0) {
        id_bits = 1;
        while (id_bits < 32 && (1LL << id_bits) < n_nodes) ++id_bits;
    }
    const unsigned blocks = (unsigned)((E + 255) / 256);
    hipLaunchKernelGGL(k_pair_keys, dim3(blocks), dim3(256), 0, stream, edge_index, E, keys, vals);
    MPN_LAUNCH_CHECK();
    size_t tmp_bytes = sort_temp(E);
    MPN_HIP(rocprim::radix_sort_pairs(tmp, tmp_bytes, keys, v.skeys, vals, v.svals, (size_t)E, 0, 32 + id_bits, stream));
    hipLaunchKernelGGL(k_run_heads, dim3(blocks), dim3(256), 0, stream, v.skeys, E, heads);
    MPN_LAUNCH_CHECK();
    tmp_bytes = scan_temp(E);
    MPN_HIP(rocprim::inclusive_scan(tmp, tmp_bytes, heads, v.run_no, (size_t)E, rocprim::plus<int>(), stream));
    hipLaunchKernelGGL(k_inverse, dim3(blocks), dim3(256), 0, stream, v.svals, v.run_no, E, inverse, n_unique);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}

extern "C" int mpnhip_undirected_merge_fill(int64_t n_edges, int64_t n_unique, const void* workspace, size_t workspace_bytes,
                                            int64_t* edge_index_u, const float* attr, float* attr_u, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(n_edges >= 0 && n_edges < (1LL << 30) && n_unique >= 0 && n_unique <= n_edges, "undirected_merge_fill: bad sizes");
    if (n_edges == 0 || n_unique == 0) return MPNHIP_OK;
    MPN_CHECK_ARG((attr == nullptr) == (attr_u == nullptr), "undirected_merge_fill: attr and attr_u go together");
    if (!edge_index_u && !attr) return MPNHIP_OK;
    if (!workspace || workspace_bytes < mpnhip_undirected_merge_workspace_bytes(n_edges)) {
        set_error("undirected_merge_fill: workspace %zu < %zu", workspace_bytes, mpnhip_undirected_merge_workspace_bytes(n_edges));
        return MPNHIP_ERR_WORKSPACE;
    }
    MergeView v = merge_view(const_cast<void*>(workspace), n_edges);
    hipLaunchKernelGGL(k_merge_fill, dim3((unsigned)((n_edges + 255) / 256)), dim3(256), 0, stream, v.skeys, v.svals, v.run_no, n_edges,
                       n_unique, edge_index_u, attr, attr_u);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}

extern "C" int mpnhip_threshold_flags(const float* preds, int64_t n, float threshold, unsigned char* flags, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(n >= 0, "threshold_flags: bad size");
    if (n == 0) return MPNHIP_OK;
    MPN_CHECK_ARG(preds && flags, "threshold_flags: null pointer");
    hipLaunchKernelGGL(k_threshold, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, preds, n, threshold, flags);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}

extern "C" int mpnhip_node_mask_accumulate(const float* mask_logits, int64_t n_rows, int64_t row_len, int64_t node_begin,
                                           int64_t n_nodes, float* overall_node_preds, float* overall_num_node_preds, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(n_rows >= 0 && row_len >= 0 && n_nodes >= 0, "node_mask_accumulate: bad sizes");
    MPN_CHECK_ARG(node_begin >= 0 && n_rows <= n_nodes && node_begin <= n_nodes - n_rows,
                  "node_mask_accumulate: rows [%lld, %lld) leave the %lld nodes", (long long)node_begin, (long long)(node_begin + n_rows),
                  (long long)n_nodes);
    if (n_rows == 0) return MPNHIP_OK;
    MPN_CHECK_ARG(overall_num_node_preds && (row_len == 0 || (mask_logits && overall_node_preds)), "node_mask_accumulate: null pointer");
    const int64_t total = n_rows * row_len;
    float* dst = overall_node_preds ? overall_node_preds + node_begin * row_len : nullptr;
    float* cnt = overall_num_node_preds + node_begin;
    if (total % 4 == 0 && aligned16(mask_logits) && aligned16(dst)) {
        hipLaunchKernelGGL(k_node_accumulate<true>, dim3(stream_blocks(total / 4 > n_rows ? total / 4 : n_rows)), dim3(256), 0, stream,
                           mask_logits, n_rows, total, dst, cnt);
    } else {
        hipLaunchKernelGGL(k_node_accumulate<false>, dim3(stream_blocks(total > n_rows ? total : n_rows)), dim3(256), 0, stream,
                           mask_logits, n_rows, total, dst, cnt);
    }
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}

extern "C" int mpnhip_node_mask_average(const float* overall_node_preds, const float* overall_num_node_preds, int64_t n_nodes,
                                        int64_t row_len, float* node_preds, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(n_nodes >= 0 && row_len >= 0, "node_mask_average: bad sizes");
    if (n_nodes == 0 || row_len == 0) return MPNHIP_OK;
    MPN_CHECK_ARG(overall_node_preds && overall_num_node_preds && node_preds, "node_mask_average: null pointer");
    const int64_t total = n_nodes * row_len;
    if (row_len % 4 == 0 && aligned16(overall_node_preds) && aligned16(node_preds)) {
        hipLaunchKernelGGL(k_node_average<true>, dim3(stream_blocks(total / 4)), dim3(256), 0, stream, overall_node_preds,
                           overall_num_node_preds, total, row_len, node_preds);
    } else {
        hipLaunchKernelGGL(k_node_average<false>, dim3(stream_blocks(total)), dim3(256), 0, stream, overall_node_preds,
                           overall_num_node_preds, total, row_len, node_preds);
    }
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}
