// Training targets on the device, without host synchronisation:
//   * MOTGraph.assign_edge_labels (data/mot_graph.py:223-262), modes 'all' and 'closest': the reference minimises |row - col|
//     over the same-id edges of every row with torch_scatter.scatter_min, once over the future edges (col > row) and once over
//     the past ones.  For a fixed row distinct cols have distinct distances, so the active future edge of a row is the one
//     with the SMALLEST col > row and the active past edge the one with the LARGEST col < row: two integer atomics per edge
//     (order-independent: the same bits on every call), then one comparison per edge;
//   * the segmentation term of MOTNeuralSolver._compute_loss (pl_module/pl_module.py:108-118): for every classified step the
//     mean over the valid rows of binary_cross_entropy_with_logits(pred[valid], gt[valid]) times the segmentation weight, and
//     its gradient w.r.t. every step's mask predictions (zero rows where the reference leaves no gradient) -- all steps in
//     one launch, a thread loading its ground-truth values once.
#include <limits.h>

#include "common.h"

namespace mpnhip {
namespace {

constexpr int MASK_MAX_STEPS = 16;

// ------------------------------------------------------------------------------------------------ edge labels
__global__ __launch_bounds__(256) void k_labels_init(int* __restrict__ fut, int* __restrict__ past, int64_t N) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n < N) {
        fut[n] = INT_MAX;
        past[n] = -1;
    }
}

// true: both endpoints in [0, N) and the same real id at both
__device__ __forceinline__ bool same_track(const int64_t* __restrict__ ids, int64_t N, int64_t r, int64_t c, bool* in_range) {
    *in_range = r >= 0 && r < N && c >= 0 && c < N;
    if (!*in_range) return false;
    const int64_t a = ids[r];
    return a != -1 && a == ids[c];
}

// pass 1 of 'closest': fut[row] = min col > row, past[row] = max col < row over the same-id edges of the row
__global__ __launch_bounds__(256) void k_labels_closest(const int64_t* __restrict__ ei, int64_t E, const int64_t* __restrict__ ids,
                                                        int64_t N, int* __restrict__ fut, int* __restrict__ past) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const int64_t r = ei[e], c = ei[E + e];
    bool in_range;
    if (!same_track(ids, N, r, c, &in_range)) return;
    if (c > r) atomicMin(&fut[r], (int)c);
    else if (c < r) atomicMax(&past[r], (int)c);
}

// pass 2 (mode 1), or the whole of mode 0 ('all'); an endpoint outside [0, N): label 0 and the flag
__global__ __launch_bounds__(256) void k_labels_write(const int64_t* __restrict__ ei, int64_t E, const int64_t* __restrict__ ids, int64_t N,
                                                      int mode, const int* __restrict__ fut, const int* __restrict__ past,
                                                      float* __restrict__ labels, int* __restrict__ flag) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const int64_t r = ei[e], c = ei[E + e];
    bool in_range;
    bool on = same_track(ids, N, r, c, &in_range);
    if (!in_range) atomicOr(flag, 1);
    if (on && mode == 1) on = c > r ? fut[r] == (int)c : (c < r ? past[r] == (int)c : false);
    labels[e] = on ? 1.f : 0.f;
}

// ------------------------------------------------------------------------------------------------ segmentation loss
struct MaskPtrs {
    const float* pred[MASK_MAX_STEPS];
    float* grad[MASK_MAX_STEPS];
};

// counts[g] = valid rows of graph g (exact integers whatever the order); K <= 1024
__global__ __launch_bounds__(256) void k_mask_counts(const unsigned char* __restrict__ valid, const int* __restrict__ node_graph, int64_t N,
                                                     int K, int* __restrict__ counts) {
    extern __shared__ int sc[];   // [K]
    for (int i = threadIdx.x; i < K; i += 256) sc[i] = 0;
    __syncthreads();
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n < N && valid[n]) {
        const int g = node_graph ? node_graph[n] : 0;
        if (g >= 0 && g < K) atomicAdd(&sc[g], 1);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < K; j += 256)
        if (sc[j]) atomicAdd(&counts[j], sc[j]);
}

template <int V> struct Pack;
template <> struct Pack<4> { using T = float4; };
template <> struct Pack<1> { using T = float; };
__device__ __forceinline__ float lane(const float4& v, int i) { return i == 0 ? v.x : (i == 1 ? v.y : (i == 2 ? v.z : v.w)); }
__device__ __forceinline__ float lane(const float& v, int) { return v; }
__device__ __forceinline__ void set_lane(float4& v, int i, float x) { if (i == 0) v.x = x; else if (i == 1) v.y = x; else if (i == 2) v.z = x; else v.w = x; }
__device__ __forceinline__ void set_lane(float& v, int, float x) { v = x; }

// a unit of V floats at unit index i of `base`: one 16-byte access (WIDE: V == 4 and the base on a 16-byte boundary) or V 4-byte ones
template <int V, bool WIDE>
__device__ __forceinline__ typename Pack<V>::T load_unit(const float* __restrict__ base, int64_t i) {
    using T = typename Pack<V>::T;
    if constexpr (WIDE || V == 1) return reinterpret_cast<const T*>(base)[i];
    T v;
#pragma unroll
    for (int j = 0; j < V; ++j) set_lane(v, j, base[i * V + j]);
    return v;
}
template <int V, bool WIDE>
__device__ __forceinline__ void store_unit(float* __restrict__ base, int64_t i, const typename Pack<V>::T& v) {
    using T = typename Pack<V>::T;
    if constexpr (WIDE || V == 1) { reinterpret_cast<T*>(base)[i] = v; return; }
#pragma unroll
    for (int j = 0; j < V; ++j) base[i * V + j] = lane(v, j);
}

// One block = one chunk of one node's row ([N, P] rows in units of V floats: 4 when P is a multiple of 4, else 1; WIDE: every base
// allows 16-byte accesses.  Which element a thread takes and the order of every sum depend on V alone, so the loss of a row shape
// does not depend on where the allocator put the tensors: bit-equal results with and without WIDE).
// block b: node b / cpr, units [(b % cpr) * chunk, ...) of the row's P / V units.  partial[s][b] = the block's sum of the BCE terms
// of step s divided by the valid rows of the node's graph (0 for a row that is not valid).
template <int V, bool WIDE>
__global__ __launch_bounds__(256) void k_mask_bce(MaskPtrs p, int k, const float* __restrict__ labels, const unsigned char* __restrict__ valid,
                                                  const int* __restrict__ node_graph, int K, const int* __restrict__ counts, int64_t P,
                                                  int cpr, int chunk, float weight, float* __restrict__ partial) {
    using T = typename Pack<V>::T;
    const int64_t node = blockIdx.x / cpr;
    const int64_t units = P / V;
    const int64_t u0 = (int64_t)(blockIdx.x % cpr) * chunk;
    const int64_t u1 = u0 + chunk < units ? u0 + chunk : units;
    const int g = node_graph ? node_graph[node] : 0;
    const bool ok = valid[node] != 0 && g >= 0 && g < K;
    const int64_t row = node * units;
    if (!ok) {   // the reference leaves no gradient here: zeros (block-uniform branch)
        T zero;
#pragma unroll
        for (int j = 0; j < V; ++j) set_lane(zero, j, 0.f);
        for (int64_t u = u0 + threadIdx.x; u < u1; u += 256) {
#pragma unroll
            for (int s = 0; s < MASK_MAX_STEPS; ++s)
                if (s < k) store_unit<V, WIDE>(p.grad[s], row + u, zero);
        }
        if ((int)threadIdx.x < k) partial[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] = 0.f;
        return;
    }
    const float cnt = (float)counts[g];
    const float gs = weight / (cnt * (float)P * (float)K);
    float acc[MASK_MAX_STEPS];
#pragma unroll
    for (int s = 0; s < MASK_MAX_STEPS; ++s) acc[s] = 0.f;
    for (int64_t u = u0 + threadIdx.x; u < u1; u += 256) {
        const T y = load_unit<V, WIDE>(labels, row + u);
#pragma unroll
        for (int s = 0; s < MASK_MAX_STEPS; ++s) {
            if (s < k) {
                const T z = load_unit<V, WIDE>(p.pred[s], row + u);
                T gr;
                float t = 0.f;
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const float zj = lane(z, j), yj = lane(y, j);
                    // aten's stable form: (1 - y) z + log1p(exp(-|z|)) + max(-z, 0)
                    t += (1.f - yj) * zj + (log1pf(expf(-fabsf(zj))) + fmaxf(-zj, 0.f));
                    const float sg = zj >= 0.f ? 1.f / (1.f + expf(-zj)) : expf(zj) / (1.f + expf(zj));
                    set_lane(gr, j, (sg - yj) * gs);
                }
                acc[s] += t;
                store_unit<V, WIDE>(p.grad[s], row + u, gr);
            }
        }
    }
    // wave64 sums, then the four waves in a fixed order
    __shared__ float red[MASK_MAX_STEPS][4];
    const int wave = threadIdx.x >> 6, ln = threadIdx.x & 63;
#pragma unroll
    for (int s = 0; s < MASK_MAX_STEPS; ++s) {
        if (s < k) {
            float v = acc[s];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
            if (ln == 0) red[s][wave] = v;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < k) {
        const int s = threadIdx.x;
        partial[(int64_t)s * gridDim.x + blockIdx.x] = ((red[s][0] + red[s][1]) + (red[s][2] + red[s][3])) / cnt;
    }
}

// one block; loss_out[1 + s] = scale * sum of partial[s][:] (double, fixed order), loss_out[0] = their sum
__global__ __launch_bounds__(256) void k_mask_loss_reduce(const float* __restrict__ partial, int64_t nblk, int k, double scale,
                                                          float* __restrict__ loss_out) {
    __shared__ double red[256];
    double total = 0.0;
    for (int s = 0; s < k; ++s) {
        double acc = 0.0;
        for (int64_t b = threadIdx.x; b < nblk; b += 256) acc += (double)partial[(int64_t)s * nblk + b];
        red[threadIdx.x] = acc;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
            __syncthreads();
        }
        const double ls = red[0] * scale;
        if (threadIdx.x == 0) loss_out[1 + s] = (float)ls;
        total += ls;
        __syncthreads();
    }
    if (threadIdx.x == 0) loss_out[0] = (float)total;
}

// chunks per row and units per chunk: at most two accesses per thread and chunk, the chunks of a row equally long up to the
// rounding of the division (cpr * chunk >= units: for very long rows the last chunks can start past the row's end -- their blocks
// find u0 >= u1, touch nothing and write a partial of 0)
void mask_plan(int64_t units, int* cpr, int* chunk) {
    const int64_t c = (units + 511) / 512;
    *cpr = (int)(c > 0 ? c : 1);
    *chunk = (int)((units + *cpr - 1) / *cpr);
}

// edge_labels' workspace ('closest' mode): fut[N] then past[N] as ONE block of 2 max(N, 1) ints
struct LabelsView { int* fut; int* past; size_t bytes; };
LabelsView labels_view(void* workspace, int64_t n_nodes) {
    Carver c(workspace);
    int* fut = c.take<int>((size_t)2 * (size_t)(n_nodes > 0 ? n_nodes : 1));
    return {fut, fut ? fut + n_nodes : nullptr, c.bytes()};
}

// mask_loss' workspace: the graphs' valid-row counts, then the blocks' partial sums [steps][blocks] (sized for the scalar
// path's plan: never fewer blocks than the vector path's)
struct MaskLossView { int* counts; float* partial; size_t bytes; };
MaskLossView mask_loss_view(void* workspace, int n_steps, int64_t n_nodes, int64_t row_floats, int n_graphs) {
    int cpr, chunk;
    mask_plan(row_floats > 0 ? row_floats : 1, &cpr, &chunk);
    const size_t nblk = (size_t)(n_nodes > 0 ? n_nodes : 1) * (size_t)cpr;
    Carver c(workspace);
    MaskLossView v = {c.take<int>((size_t)(n_graphs > 0 ? n_graphs : 1)), c.take<float>((size_t)(n_steps > 0 ? n_steps : 1) * nblk), 0};
    v.bytes = c.bytes();
    return v;
}

}  // namespace
}  // namespace mpnhip

using namespace mpnhip;

extern "C" size_t mpnhip_edge_labels_workspace_bytes(int64_t n_nodes) {
    return labels_view(nullptr, n_nodes).bytes;
}

extern "C" int mpnhip_edge_labels(const int64_t* edge_index, int64_t n_edges, const int64_t* ids, int64_t n_nodes, int mode, float* labels,
                                  int32_t* status, void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t s = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(n_edges >= 0 && n_nodes >= 0 && n_nodes < (int64_t)INT_MAX && n_edges < ((int64_t)INT_MAX - 255) * 256,
                  "edge_labels: bad sizes (%lld edges, %lld nodes)", (long long)n_edges, (long long)n_nodes);
    MPN_CHECK_ARG(mode == MPNHIP_LABELS_ALL || mode == MPNHIP_LABELS_CLOSEST, "edge_labels: unknown mode %d (0 'all', 1 'closest')", mode);
    if (n_edges == 0) {
        if (status) MPN_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
        return MPNHIP_OK;
    }
    MPN_CHECK_ARG(edge_index && labels && status, "edge_labels: null tensor");
    MPN_CHECK_ARG(ids || n_nodes == 0, "edge_labels: null ids");
    const unsigned nblk = blocks_for(n_edges);
    LabelsView v = {};   // 'all' reads neither
    if (mode == MPNHIP_LABELS_CLOSEST && n_nodes > 0) {
        v = labels_view(workspace, n_nodes);
        MPN_CHECK_WORKSPACE("edge_labels", workspace, workspace_bytes, v.bytes);
    }
    MPN_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    if (mode == MPNHIP_LABELS_CLOSEST && n_nodes > 0) {
        hipLaunchKernelGGL(k_labels_init, dim3(blocks_for(n_nodes)), dim3(256), 0, s, v.fut, v.past, n_nodes);
        MPN_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_labels_closest, dim3(nblk), dim3(256), 0, s, edge_index, n_edges, ids, n_nodes, v.fut, v.past);
        MPN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_labels_write, dim3(nblk), dim3(256), 0, s, edge_index, n_edges, ids, n_nodes, mode, v.fut, v.past, labels, status);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}

extern "C" size_t mpnhip_mask_loss_workspace_bytes(int n_steps, int64_t n_nodes, int64_t row_floats, int n_graphs) {
    return mask_loss_view(nullptr, n_steps, n_nodes, row_floats, n_graphs).bytes;
}

extern "C" int mpnhip_mask_loss(const float* const* preds, int n_steps, const float* labels, const uint8_t* valid, const int32_t* node_graph,
                                int n_graphs, int64_t n_nodes, int64_t row_floats, float weight, float* loss_out, float* const* grads,
                                void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t s = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(n_steps >= 0 && n_nodes >= 0 && row_floats >= 0, "mask_loss: bad sizes");
    MPN_CHECK_ARG(n_steps <= MASK_MAX_STEPS, "mask_loss: %d steps in one call (at most %d: split the steps)", n_steps, MASK_MAX_STEPS);
    MPN_CHECK_ARG(n_graphs >= 1 && n_graphs <= 1024, "mask_loss: %d graphs (1 .. 1024)", n_graphs);
    MPN_CHECK_ARG(node_graph || n_graphs == 1, "mask_loss: %d graphs without node_graph", n_graphs);
    if (n_steps == 0 || n_nodes == 0 || row_floats == 0) {
        if (loss_out) MPN_HIP(hipMemsetAsync(loss_out, 0, (size_t)(1 + n_steps) * sizeof(float), s));
        return MPNHIP_OK;
    }
    MPN_CHECK_ARG(preds && grads && labels && valid && loss_out, "mask_loss: null tensor");
    MaskPtrs p = {};
    const bool quad = (row_floats & 3) == 0;   // units of 4 floats; with every base on a 16-byte boundary one access each
    bool wide = quad && aligned16(labels);
    for (int i = 0; i < n_steps; ++i) {
        MPN_CHECK_ARG(preds[i] && grads[i], "mask_loss: null tensor of step %d", i);
        p.pred[i] = preds[i];
        p.grad[i] = grads[i];
        wide = wide && aligned16(preds[i]) && aligned16(grads[i]);
    }
    int cpr, chunk;
    mask_plan(quad ? row_floats / 4 : row_floats, &cpr, &chunk);
    MPN_CHECK_ARG(n_nodes <= (int64_t)INT_MAX / cpr, "mask_loss: %lld rows of %lld floats exceed one launch", (long long)n_nodes,
                  (long long)row_floats);
    const MaskLossView v = mask_loss_view(workspace, n_steps, n_nodes, row_floats, n_graphs);
    MPN_CHECK_WORKSPACE("mask_loss", workspace, workspace_bytes, v.bytes);
    const int64_t nblk = n_nodes * cpr;
    MPN_HIP(hipMemsetAsync(v.counts, 0, (size_t)n_graphs * sizeof(int), s));
    hipLaunchKernelGGL(k_mask_counts, dim3(blocks_for(n_nodes)), dim3(256), (size_t)n_graphs * sizeof(int), s, valid,
                       node_graph, n_nodes, n_graphs, v.counts);
    MPN_LAUNCH_CHECK();
    auto* kernel = wide ? k_mask_bce<4, true> : (quad ? k_mask_bce<4, false> : k_mask_bce<1, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)nblk), dim3(256), 0, s, p, n_steps, labels, valid, node_graph, n_graphs, v.counts,
                       row_floats, cpr, chunk, weight, v.partial);
    MPN_LAUNCH_CHECK();
    // (the block sums were divided by their graph's valid rows; the mean over a row's elements and over the graphs goes here)
    const double scale = (double)weight / ((double)row_floats * (double)n_graphs);
    hipLaunchKernelGGL(k_mask_loss_reduce, dim3(1), dim3(256), 0, s, v.partial, nblk, n_steps, scale, loss_out);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}
