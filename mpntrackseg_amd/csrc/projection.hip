// From edge scores to track ids (the three lines of MPNTracker.track after the windows):
//   GreedyProjector.project / ExactProjector.project    reference tracker/projectors.py:19-67, :82-98
//   compute_constr_satisfaction_rate(undirected_edges=False, return_flow_vals=True)   utils/evaluation.py:370-414
//   MPNTracker._assign_ped_ids                          tracker/mpn_tracker.py:231-248
//   Postprocessor.drop_short_trajectories               tracker/postprocessing.py:14-18
// The input is an undirected edge list [2, K] with row < col (what tracker.evaluate_sequence returns), in any edge order.
//
// Greedy rounding.  The reference walks the violated constraints, all flow-out ones before any flow-in one.  The out-constraint of
// node n touches the edges with row == n only, the in-constraint the edges with col == n only, so within one type the constraints
// are independent and the loop is two edge-parallel passes: per violated node keep the active edge with the largest score (lowest
// edge id on a tie: Python's max returns the first maximum) and zero the node's other edges; pass B works on pass A's result and
// only where the in-count is STILL above 1.  The arg-max is one 64-bit atomicMax per node on (score bits << 32) | ~edge id -- active
// scores are > 0.5, so their bit patterns order as unsigned integers -- and a second edge-parallel kernel keeps an edge iff it is
// the winner.  No sort, no CSR; integer and compare-only arithmetic, so the result has the same bits whatever the scheduling.
//
// Connected components.  Lock-free union-find: every active edge finds both roots and links the LARGER under the smaller with a
// compare-and-swap, retrying from the value it lost to.  parent[v] <= v always holds, so there is no cycle and the root of a
// component is its smallest node; one launch, no host loop, no flag read.  Then root[v] = find(v), the roots are flagged, an
// exclusive scan ranks them, and label[v] = rank[root[v]] -- scipy's connected_components(directed=False) labels.
#include "device_prims.h"
#include "projection_common.h"

namespace mpnhip {
namespace {

// counters of mpnhip_project_round_count (int32 [8])
enum { CNT_VIOL_OUT = 0, CNT_VIOL_IN = 1, CNT_CONSTRAINTS = 2, CNT_BAD_IDS = 3 };

// round_preds = edge_preds > 0.5 (NaN -> 0 as in torch); flow_out[row] / flow_in[col] += 1 per active edge; seen_* mark the nodes
// that have an outgoing / incoming edge at all (every writer stores the same 1)
__global__ void k_round_count(const int64_t* __restrict__ ei, int64_t K, int64_t N, const float* __restrict__ preds,
                              float* __restrict__ round_preds, int* __restrict__ flow_out, int* __restrict__ flow_in,
                              unsigned char* __restrict__ seen_out, unsigned char* __restrict__ seen_in, int* __restrict__ counters) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= K) return;
    const bool active = preds[e] > 0.5f;
    round_preds[e] = active ? 1.f : 0.f;
    const int64_t r = ei[e], c = ei[K + e];
    if (!ids_ok(r, c, N)) {
        atomicAdd(&counters[CNT_BAD_IDS], 1);
        return;
    }
    seen_out[r] = 1;
    seen_in[c] = 1;
    if (active) {
        atomicAdd(&flow_out[r], 1);
        atomicAdd(&flow_in[c], 1);
    }
}

__device__ __forceinline__ int wave_sum(int v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// violated = #(flow_out > 1) and #(flow_in > 1); num_constraints = distinct rows + distinct cols
__global__ __launch_bounds__(256) void k_constraint_counts(const int* __restrict__ flow_out, const int* __restrict__ flow_in,
                                                           const unsigned char* __restrict__ seen_out,
                                                           const unsigned char* __restrict__ seen_in, int64_t N,
                                                           int* __restrict__ counters) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int vo = 0, vi = 0, nc = 0;
    for (int64_t v = tid; v < N; v += stride) {
        vo += flow_out[v] > 1;
        vi += flow_in[v] > 1;
        nc += (int)seen_out[v] + (int)seen_in[v];
    }
    vo = wave_sum(vo); vi = wave_sum(vi); nc = wave_sum(nc);
    if ((threadIdx.x & 63) == 0) {
        if (vo) atomicAdd(&counters[CNT_VIOL_OUT], vo);
        if (vi) atomicAdd(&counters[CNT_VIOL_IN], vi);
        if (nc) atomicAdd(&counters[CNT_CONSTRAINTS], nc);
    }
}

// SIDE 0: the out-constraints (node = row), 1: the in-constraints (node = col).  count[node] is the number of active edges of
// the node on that side NOW; only nodes with count > 1 take part.
template <int SIDE>
__global__ void k_argmax(const int64_t* __restrict__ ei, int64_t K, int64_t N, const float* __restrict__ preds,
                         const float* __restrict__ round_preds, const int* __restrict__ count, unsigned long long* __restrict__ best) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= K) return;
    if (round_preds[e] != 1.f) return;
    const int64_t r = ei[e], c = ei[K + e];
    if (!ids_ok(r, c, N)) return;
    const int64_t n = SIDE == 0 ? r : c;
    if (count[n] <= 1) return;
    const unsigned long long key = pack_key(preds[e], e);
    // (best only grows: a key that is not above what is already there cannot win, and the plain read spares the hub's atomics)
    if (key > __atomic_load_n(&best[n], __ATOMIC_RELAXED)) atomicMax(&best[n], key);
}

// keep the winner, zero the violated node's other active edges; pass A also takes the zeroed edges out of the in-counts
template <int SIDE>
__global__ void k_keep_winner(const int64_t* __restrict__ ei, int64_t K, int64_t N, const float* __restrict__ preds,
                              float* __restrict__ round_preds, const int* __restrict__ count,
                              const unsigned long long* __restrict__ best, int* __restrict__ other_count) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= K) return;
    if (round_preds[e] != 1.f) return;
    const int64_t r = ei[e], c = ei[K + e];
    if (!ids_ok(r, c, N)) return;
    const int64_t n = SIDE == 0 ? r : c;
    if (count[n] <= 1) return;
    if (pack_key(preds[e], e) == best[n]) return;
    round_preds[e] = 0.f;
    if (SIDE == 0) atomicSub(&other_count[c], 1);
}

__global__ void k_nodes_mask(const int* __restrict__ flow_out, const int* __restrict__ flow_in, int64_t N,
                             unsigned char* __restrict__ nodes_mask) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= N) return;
    nodes_mask[v] = (flow_in[v] > 1 || flow_out[v] > 1) ? 1 : 0;
}

__global__ void k_edges_mask(const int64_t* __restrict__ ei, int64_t K, int64_t N, const unsigned char* __restrict__ nodes_mask,
                             unsigned char* __restrict__ edges_mask) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= K) return;
    const int64_t r = ei[e], c = ei[K + e];
    edges_mask[e] = (ids_ok(r, c, N) && (nodes_mask[r] | nodes_mask[c])) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------ connected components
// (the union-find itself: projection_common.h)
__global__ void k_cc_union(const int64_t* __restrict__ ei, int64_t K, int64_t N, const float* __restrict__ preds, int* parent) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= K) return;
    if (preds[e] != 1.f) return;
    const int64_t r = ei[e], c = ei[K + e];
    if (!ids_ok(r, c, N)) return;
    cc_link(parent, (int)r, (int)c);
}

__global__ void k_cc_labels(const int* __restrict__ root, const int* __restrict__ is_root, const int* __restrict__ rank, int64_t N,
                            int64_t* __restrict__ labels, int* __restrict__ n_components) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= N) return;
    labels[v] = (int64_t)rank[root[v]];
    if (v == N - 1 && n_components) n_components[0] = rank[v] + is_root[v];
}

__global__ void k_label_count(const int64_t* __restrict__ labels, int64_t N, int* __restrict__ counts) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= N) return;
    const int64_t l = labels[v];
    if (l >= 0 && l < N) atomicAdd(&counts[l], 1);
}

__global__ void k_label_keep(const int64_t* __restrict__ labels, int64_t N, const int* __restrict__ counts, int64_t min_len,
                             unsigned char* __restrict__ keep) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= N) return;
    const int64_t l = labels[v];
    keep[v] = (l >= 0 && l < N && (int64_t)counts[l] >= min_len) ? 1 : 0;
}

// project_round_count's workspace: the "has an outgoing / incoming edge" marks, one byte per node (zeroed as one block)
struct RoundView { unsigned char* seen_out; unsigned char* seen_in; size_t bytes; };
static RoundView round_view(void* workspace, int64_t n_nodes) {
    if (n_nodes <= 0) return {};
    Carver c(workspace);
    RoundView v = {c.take<unsigned char>((size_t)n_nodes), c.take<unsigned char>((size_t)n_nodes), 0};
    v.bytes = c.bytes();
    return v;
}

// project_greedy's workspace: the arg-max keys and the in-counts as pass A leaves them, per node
struct GreedyView { unsigned long long* best; int* in_now; size_t bytes; };
static GreedyView greedy_view(void* workspace, int64_t n_nodes) {
    if (n_nodes <= 0) return {};
    Carver c(workspace);
    GreedyView v = {c.take<unsigned long long>((size_t)n_nodes), c.take<int>((size_t)n_nodes), 0};
    v.bytes = c.bytes();
    return v;
}

// connected_components' workspace: parent, root, root flags, ranks per node, rocprim's scratch
struct CcView { int* parent; int* root; int* is_root; int* rank; void* tmp; size_t tmp_bytes, bytes; };
static CcView cc_view(void* workspace, int64_t n_nodes) {
    if (n_nodes <= 0) return {};
    Carver c(workspace);
    const size_t n = (size_t)n_nodes;
    CcView v = {c.take<int>(n), c.take<int>(n), c.take<int>(n), c.take<int>(n), nullptr, exclusive_scan_temp<int>(n_nodes), 0};
    v.tmp = c.take<char>(v.tmp_bytes);
    v.bytes = c.bytes() + 256;
    return v;
}

static const int64_t MAX_IDS = 1LL << 30;   // node ids are kept as int32, edge ids as the low word of the arg-max key

}  // namespace
}  // namespace mpnhip

using namespace mpnhip;

extern "C" size_t mpnhip_project_round_count_workspace_bytes(int64_t n_nodes) {
    return round_view(nullptr, n_nodes).bytes;
}

extern "C" int mpnhip_project_round_count(const int64_t* edge_index, int64_t n_edges, int64_t n_nodes, const float* edge_preds,
                                          float* round_preds, int32_t* flow_out, int32_t* flow_in, int32_t* counters, void* workspace,
                                          size_t workspace_bytes, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(n_edges >= 0 && n_edges < MAX_IDS && n_nodes >= 0 && n_nodes < MAX_IDS, "project_round_count: bad sizes");
    if (n_edges == 0 && n_nodes == 0) return MPNHIP_OK;
    MPN_CHECK_ARG(counters, "project_round_count: null counters");
    MPN_CHECK_ARG(n_nodes == 0 || (flow_out && flow_in), "project_round_count: null flow pointer");
    MPN_CHECK_ARG(n_edges == 0 || (edge_index && edge_preds && round_preds), "project_round_count: null pointer");
    const RoundView v = round_view(workspace, n_nodes);
    if (n_nodes > 0) MPN_CHECK_WORKSPACE("project_round_count", workspace, workspace_bytes, v.bytes);
    MPN_HIP(hipMemsetAsync(counters, 0, 8 * sizeof(int32_t), stream));
    // (every edge of a graph without nodes has ids out of range: counted in counters[3], nothing else touched)
    if (n_nodes > 0) {
        MPN_HIP(hipMemsetAsync(flow_out, 0, (size_t)n_nodes * 4, stream));
        MPN_HIP(hipMemsetAsync(flow_in, 0, (size_t)n_nodes * 4, stream));
        MPN_HIP(hipMemsetAsync(workspace, 0, v.bytes, stream));
    }
    if (n_edges > 0) {
        hipLaunchKernelGGL(k_round_count, dim3(blocks_for(n_edges)), dim3(256), 0, stream, edge_index, n_edges, n_nodes, edge_preds,
                           round_preds, flow_out, flow_in, v.seen_out, v.seen_in, counters);
        MPN_LAUNCH_CHECK();
    }
    if (n_nodes > 0 && n_edges > 0) {
        const unsigned blocks = blocks_for(n_nodes) < 1024 ? blocks_for(n_nodes) : 1024;
        hipLaunchKernelGGL(k_constraint_counts, dim3(blocks), dim3(256), 0, stream, flow_out, flow_in, v.seen_out, v.seen_in, n_nodes, counters);
        MPN_LAUNCH_CHECK();
    }
    return MPNHIP_OK;
}

extern "C" size_t mpnhip_project_greedy_workspace_bytes(int64_t n_nodes) {
    return greedy_view(nullptr, n_nodes).bytes;
}

extern "C" int mpnhip_project_greedy(const int64_t* edge_index, int64_t n_edges, int64_t n_nodes, const float* edge_preds,
                                     float* round_preds, const int32_t* flow_out, const int32_t* flow_in, void* workspace,
                                     size_t workspace_bytes, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(n_edges >= 0 && n_edges < MAX_IDS && n_nodes >= 0 && n_nodes < MAX_IDS, "project_greedy: bad sizes");
    if (n_edges == 0 || n_nodes == 0) return MPNHIP_OK;
    MPN_CHECK_ARG(edge_index && edge_preds && round_preds && flow_out && flow_in, "project_greedy: null pointer");
    const GreedyView v = greedy_view(workspace, n_nodes);
    MPN_CHECK_WORKSPACE("project_greedy", workspace, workspace_bytes, v.bytes);
    const unsigned blocks = blocks_for(n_edges);
    // pass A: the out-constraints; the in-counts follow the edges it zeroes
    MPN_HIP(hipMemsetAsync(v.best, 0, (size_t)n_nodes * 8, stream));
    MPN_HIP(hipMemcpyAsync(v.in_now, flow_in, (size_t)n_nodes * 4, hipMemcpyDeviceToDevice, stream));
    hipLaunchKernelGGL(k_argmax<0>, dim3(blocks), dim3(256), 0, stream, edge_index, n_edges, n_nodes, edge_preds, round_preds, flow_out, v.best);
    MPN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_keep_winner<0>, dim3(blocks), dim3(256), 0, stream, edge_index, n_edges, n_nodes, edge_preds, round_preds,
                       flow_out, v.best, v.in_now);
    MPN_LAUNCH_CHECK();
    // pass B: the in-constraints that are still violated
    MPN_HIP(hipMemsetAsync(v.best, 0, (size_t)n_nodes * 8, stream));
    hipLaunchKernelGGL(k_argmax<1>, dim3(blocks), dim3(256), 0, stream, edge_index, n_edges, n_nodes, edge_preds, round_preds, v.in_now, v.best);
    MPN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_keep_winner<1>, dim3(blocks), dim3(256), 0, stream, edge_index, n_edges, n_nodes, edge_preds, round_preds,
                       v.in_now, v.best, (int*)nullptr);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}

extern "C" int mpnhip_project_violated_masks(const int64_t* edge_index, int64_t n_edges, int64_t n_nodes, const int32_t* flow_out,
                                             const int32_t* flow_in, unsigned char* nodes_mask, unsigned char* edges_mask,
                                             void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(n_edges >= 0 && n_edges < MAX_IDS && n_nodes >= 0 && n_nodes < MAX_IDS, "project_violated_masks: bad sizes");
    MPN_CHECK_ARG(n_nodes == 0 || (flow_out && flow_in && nodes_mask), "project_violated_masks: null node pointer");
    MPN_CHECK_ARG(n_edges == 0 || (edge_index && edges_mask), "project_violated_masks: null edge pointer");
    if (n_nodes > 0) {
        hipLaunchKernelGGL(k_nodes_mask, dim3(blocks_for(n_nodes)), dim3(256), 0, stream, flow_out, flow_in, n_nodes, nodes_mask);
        MPN_LAUNCH_CHECK();
    }
    if (n_edges > 0) {
        hipLaunchKernelGGL(k_edges_mask, dim3(blocks_for(n_edges)), dim3(256), 0, stream, edge_index, n_edges, n_nodes, nodes_mask, edges_mask);
        MPN_LAUNCH_CHECK();
    }
    return MPNHIP_OK;
}

extern "C" size_t mpnhip_connected_components_workspace_bytes(int64_t n_nodes) {
    return cc_view(nullptr, n_nodes).bytes;
}

extern "C" int mpnhip_connected_components(const int64_t* edge_index, int64_t n_edges, int64_t n_nodes, const float* edge_preds,
                                           int64_t* labels, int32_t* n_components, void* workspace, size_t workspace_bytes,
                                           void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(n_edges >= 0 && n_edges < MAX_IDS && n_nodes >= 0 && n_nodes < MAX_IDS, "connected_components: bad sizes");
    if (n_nodes == 0) {
        if (n_components) MPN_HIP(hipMemsetAsync(n_components, 0, 4, stream));
        return MPNHIP_OK;
    }
    MPN_CHECK_ARG(labels && (n_edges == 0 || (edge_index && edge_preds)), "connected_components: null pointer");
    CcView v = cc_view(workspace, n_nodes);
    MPN_CHECK_WORKSPACE("connected_components", workspace, workspace_bytes, v.bytes);
    const unsigned nb = blocks_for(n_nodes);
    hipLaunchKernelGGL(k_cc_init, dim3(nb), dim3(256), 0, stream, v.parent, n_nodes);
    MPN_LAUNCH_CHECK();
    if (n_edges > 0) {
        hipLaunchKernelGGL(k_cc_union, dim3(blocks_for(n_edges)), dim3(256), 0, stream, edge_index, n_edges, n_nodes, edge_preds, v.parent);
        MPN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_cc_roots, dim3(nb), dim3(256), 0, stream, v.parent, n_nodes, v.root, v.is_root);
    MPN_LAUNCH_CHECK();
    MPN_HIP(rocprim::exclusive_scan(v.tmp, v.tmp_bytes, v.is_root, v.rank, 0, (size_t)n_nodes, rocprim::plus<int>(), stream));
    hipLaunchKernelGGL(k_cc_labels, dim3(nb), dim3(256), 0, stream, v.root, v.is_root, v.rank, n_nodes, labels, n_components);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}

extern "C" int mpnhip_track_lengths(const int64_t* labels, int64_t n_nodes, int64_t min_track_len, int32_t* counts,
                                    unsigned char* keep, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(n_nodes >= 0 && n_nodes < MAX_IDS, "track_lengths: bad size");
    if (n_nodes == 0) return MPNHIP_OK;
    MPN_CHECK_ARG(labels && counts && keep, "track_lengths: null pointer");
    MPN_HIP(hipMemsetAsync(counts, 0, (size_t)n_nodes * 4, stream));
    hipLaunchKernelGGL(k_label_count, dim3(blocks_for(n_nodes)), dim3(256), 0, stream, labels, n_nodes, counts);
    MPN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_label_keep, dim3(blocks_for(n_nodes)), dim3(256), 0, stream, labels, n_nodes, counts, min_track_len, keep);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}
