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
#include "device_prims.h"

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

// The merge workspace.  Its head -- sorted keys, sorted edge ids, run numbers -- is what mpnhip_undirected_merge_sort leaves for
// mpnhip_undirected_merge_fill; behind it the sort's own: unsorted keys and ids, head flags, rocprim's scratch.
struct MergeView {
    unsigned long long* skeys; int* svals; int* run_no;
    unsigned long long* keys; int* vals; int* heads;
    void* tmp;
    size_t tmp_bytes, bytes;
};
static MergeView merge_view(void* workspace, int64_t n_edges) {
    Carver c(workspace);
    const size_t E = (size_t)n_edges, a = sort_pairs_temp<unsigned long long>(n_edges), b = inclusive_scan_temp<int>(n_edges);
    MergeView v = {c.take<unsigned long long>(E), c.take<int>(E), c.take<int>(E), c.take<unsigned long long>(E), c.take<int>(E), c.take<int>(E),
                   nullptr, a > b ? a : b, 0};
    v.tmp = c.take<char>(v.tmp_bytes);
    v.bytes = c.bytes() + 256;
    return v;
}

}  // namespace
}  // namespace mpnhip

using namespace mpnhip;

extern "C" size_t mpnhip_undirected_merge_workspace_bytes(int64_t n_edges) {
    if (n_edges <= 0) return 0;
    return merge_view(nullptr, n_edges).bytes;
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
    const int64_t E = n_edges;
    MergeView v = merge_view(workspace, E);
    MPN_CHECK_WORKSPACE("undirected_merge_sort", workspace, workspace_bytes, v.bytes);
    // the key's low word holds max(r, c) < n_nodes and its high word min(r, c): only the bits a node id needs are sorted
    const unsigned id_bits = n_nodes > 0 ? key_bits((uint64_t)n_nodes - 1) : 32;
    const unsigned blocks = blocks_for(E);
    hipLaunchKernelGGL(k_pair_keys, dim3(blocks), dim3(256), 0, stream, edge_index, E, v.keys, v.vals);
    MPN_LAUNCH_CHECK();
    MPN_HIP(rocprim::radix_sort_pairs(v.tmp, v.tmp_bytes, v.keys, v.skeys, v.vals, v.svals, (size_t)E, 0, 32 + id_bits, stream));
    hipLaunchKernelGGL(k_run_heads, dim3(blocks), dim3(256), 0, stream, v.skeys, E, v.heads);
    MPN_LAUNCH_CHECK();
    MPN_HIP(rocprim::inclusive_scan(v.tmp, v.tmp_bytes, v.heads, v.run_no, (size_t)E, rocprim::plus<int>(), stream));
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
    const MergeView v = merge_view(const_cast<void*>(workspace), n_edges);
    MPN_CHECK_WORKSPACE("undirected_merge_fill", workspace, workspace_bytes, v.bytes);
    hipLaunchKernelGGL(k_merge_fill, dim3(blocks_for(n_edges)), dim3(256), 0, stream, v.skeys, v.svals, v.run_no, n_edges,
                       n_unique, edge_index_u, attr, attr_u);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}

extern "C" int mpnhip_threshold_flags(const float* preds, int64_t n, float threshold, unsigned char* flags, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(n >= 0, "threshold_flags: bad size");
    if (n == 0) return MPNHIP_OK;
    MPN_CHECK_ARG(preds && flags, "threshold_flags: null pointer");
    hipLaunchKernelGGL(k_threshold, dim3(blocks_for(n)), dim3(256), 0, stream, preds, n, threshold, flags);
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
