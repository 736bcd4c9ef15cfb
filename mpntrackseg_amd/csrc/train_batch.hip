// Training batches on the device: what MOTGraphDataset.__getitem__ (reference data/mot_graph_dataset.py:185-247) and the
// DataLoader's collation do per sample on the host, for ALL graphs of a batch at once:
//   MOTGraphAugmentor._wiggle_boxes   data/augmentation.py:41-86   box sides shifted by eps, the IoU check (utils/iou.py:33-59)
//   get_time_valid_conn_ixs           utils/graph.py:6-37          pairs inside each graph, batch-global node indices
//   compute_edge_feats_dict           utils/graph.py:90-124        with the fps of each pair's own sequence, + F.pairwise_distance
//   construct_graph_object            data/mot_graph.py:311-312    pairs then flipped pairs per graph, in the order of a PyG Batch
// A batch is N nodes in graph order, graph_ptr [B + 1] and one row of a sequence table per node (node_src).  The random numbers
// (eps) and the rows come from the host (mpntrackseg_amd/dataset.py); nothing here draws anything.
// Contraction is off for the whole file: the float64 boxes equal numpy's bit for bit, and the float32 features equal those of
// mpnhip_edge_features / mpnhip_pairwise_distance on one graph alone.  No float atomics: the minimum is taken on ordered keys.
#pragma clang fp contract(off)

#include "device_prims.h"

namespace mpnhip {
namespace {

constexpr int BOX_COLS = MPNHIP_BOX_COLS;   // bb_left, bb_top, bb_right, bb_bot, bb_width, bb_height, feet_x, feet_y
enum { C_LEFT = 0, C_TOP, C_RIGHT, C_BOT, C_W, C_H, C_FX, C_FY };

// a double as a key whose unsigned order is the doubles' order; NaN -> 0, below every number (numpy's min returns NaN)
__device__ __forceinline__ unsigned long long ordered_key(double v) {
    if (v != v) return 0ull;
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double key_value(unsigned long long k) {
    if (k == 0ull) return __longlong_as_double(0x7ff8000000000000ll);
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

__device__ __forceinline__ double np_max(double a, double b) { return (a > b || a != a) ? a : b; }   // np.maximum: NaN wins
__device__ __forceinline__ double np_min(double a, double b) { return (a < b || a != a) ? a : b; }

// the graph of node i: largest g in [0, n_graphs) with ptr[g] <= i (graphs without nodes are skipped over)
__device__ __forceinline__ int graph_of_node(const int32_t* __restrict__ ptr, int n_graphs, int i) {
    int lo = 0, hi = n_graphs;   // first g with ptr[g] > i
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ptr[mid] <= i) lo = mid + 1; else hi = mid;
    }
    return lo - 1 < 0 ? 0 : lo - 1;
}

// One thread per node: the row node_src[i] of the table, wiggled (eps != nullptr) in the reference's order, its float32 feature
// columns, frame, id and graph, and the IoU of the new box with the old one; the block's smallest IoU goes to min_key.
__global__ __launch_bounds__(256) void k_augment_boxes(const double* __restrict__ boxes, const int64_t* __restrict__ frame,
                                                       const int64_t* __restrict__ ids, int64_t n_rows, const int32_t* __restrict__ node_src,
                                                       const int32_t* __restrict__ graph_ptr, int n_graphs, const double* __restrict__ eps,
                                                       int n_nodes, double* __restrict__ out_boxes, float* __restrict__ out_cols,
                                                       int64_t* __restrict__ out_frame, int64_t* __restrict__ out_id,
                                                       int32_t* __restrict__ node_graph, unsigned long long* __restrict__ min_key,
                                                       int32_t* __restrict__ bad_rows) {
    __shared__ unsigned long long s_min[4];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long key = ~0ull;
    if (i < n_nodes) {
        const int64_t r = node_src[i];
        const bool ok = r >= 0 && r < n_rows;
        double b[BOX_COLS];
#pragma unroll
        for (int c = 0; c < BOX_COLS; ++c) b[c] = ok ? boxes[r * BOX_COLS + c] : 0.0;
        if (!ok) atomicAdd(bad_rows, 1);
        if (eps && ok) {
            const double e0 = eps[(int64_t)i * 4 + 0], e1 = eps[(int64_t)i * 4 + 1], e2 = eps[(int64_t)i * 4 + 2], e3 = eps[(int64_t)i * 4 + 3];
            const double h = b[C_H], w = b[C_W];
            const double top = b[C_TOP] + h * e0, bot = b[C_BOT] + h * e1;        // augmentation.py:71-78
            const double left = b[C_LEFT] + w * e2, right = b[C_RIGHT] + w * e3;
            // iou_pairs(new, old) over (left, top, right, bot), utils/iou.py:45-57
            const double xA = np_max(left, b[C_LEFT]), yA = np_max(top, b[C_TOP]);
            const double xB = np_min(right, b[C_RIGHT]), yB = np_min(bot, b[C_BOT]);
            const double inter = np_max(0.0, (xB - xA) + 1.0) * np_max(0.0, (yB - yA) + 1.0);
            const double area_a = ((right - left) + 1.0) * ((bot - top) + 1.0);
            const double area_b = ((b[C_RIGHT] - b[C_LEFT]) + 1.0) * ((b[C_BOT] - b[C_TOP]) + 1.0);
            key = ordered_key(inter / ((area_a + area_b) - inter));
            b[C_TOP] = top; b[C_BOT] = bot; b[C_LEFT] = left; b[C_RIGHT] = right;
            b[C_H] = bot - top;                                                    // :79-80 (feet_x / feet_y stay: the code, not the docstring)
            b[C_W] = right - left;
        }
#pragma unroll
        for (int c = 0; c < BOX_COLS; ++c) out_boxes[(int64_t)i * BOX_COLS + c] = b[c];
        float* __restrict__ o = out_cols + (int64_t)i * 4;                         // .float(): round to nearest even
        o[0] = (float)b[C_H]; o[1] = (float)b[C_W]; o[2] = (float)b[C_FX]; o[3] = (float)b[C_FY];
        out_frame[i] = ok ? frame[r] : 0;
        out_id[i] = ok ? ids[r] : -1;
        node_graph[i] = graph_of_node(graph_ptr, n_graphs, i);
    }
    if (!eps) return;   // (uniform: no minimum to take)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long other = __shfl_xor(key, off, 64);
        key = other < key ? other : key;
    }
    if ((threadIdx.x & 63) == 0) s_min[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) key = s_min[w] < key ? s_min[w] : key;
        atomicMin(min_key, key);
    }
}

__global__ void k_min_iou_value(const unsigned long long* __restrict__ min_key, double* __restrict__ min_iou) {
    // no node at all: + inf (the key's initial value); the reference's min() of nothing raises, the caller decides
    const unsigned long long k = *min_key;
    *min_iou = k == ~0ull ? __longlong_as_double(0x7ff0000000000000ll) : key_value(k);
}

// pairs (i, j), i < j, of ONE graph with 0 < |frame[i] - frame[j]| <= max_dist (max_dist < 0: no upper limit): k_time_pairs of
// graph_build.hip with the row's scan ending where its graph ends.  One wavefront per row; pass 0 counts, pass 1 writes at offs[i].
template <bool FILL>
__global__ __launch_bounds__(256) void k_batch_pairs(const int64_t* __restrict__ frame, const int32_t* __restrict__ node_graph,
                                                     const int32_t* __restrict__ graph_ptr, int n_graphs, int n, int64_t max_dist,
                                                     int64_t* __restrict__ counts, const int64_t* __restrict__ offs,
                                                     int64_t* __restrict__ out_row, int64_t* __restrict__ out_col) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    int g = node_graph[i];
    g = g < 0 ? 0 : (g >= n_graphs ? n_graphs - 1 : g);
    int end = graph_ptr[g + 1];
    end = end > n ? n : end;       // (a table that is not the batch's never sends a lane past the nodes)
    const int64_t fi = frame[i];
    int64_t base = FILL ? offs[i] : 0;
    int64_t total = 0;
    for (int j0 = i + 1; j0 < end; j0 += 64) {
        const int j = j0 + lane;
        bool ok = false;
        if (j < end) {
            int64_t d = frame[j] - fi;
            d = d < 0 ? -d : d;
            ok = d > 0 && (max_dist < 0 || d <= max_dist);
        }
        const unsigned long long m = __ballot(ok);
        if (FILL && ok) {
            const int64_t pos = base + __popcll(m & ((1ull << lane) - 1ull));
            out_row[pos] = i;
            out_col[pos] = j;
        }
        const int c = __popcll(m);
        base += c;
        total += c;
    }
    if (!FILL && lane == 0) counts[i] = total;
}

// utils/graph.py:104-122 with the fps of the pair's graph, and || a - b + eps ||_2 of the embeddings (mot_graph.py:211, :301):
// one wavefront per pair, k_edge_feats and k_pairwise_dist of graph_build.hip operation for operation
__global__ __launch_bounds__(256) void k_batch_edge_feats(const int64_t* __restrict__ ei, int64_t E, int n_nodes,
                                                          const int64_t* __restrict__ frame, const int32_t* __restrict__ node_graph,
                                                          const float* __restrict__ fps, int n_graphs, const float* __restrict__ cols,
                                                          const float* __restrict__ emb, int64_t ld, int dim, float eps,
                                                          float* __restrict__ feats, float* __restrict__ dist) {
    const int lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= E) return;
    int64_t r = ei[e], c = ei[E + e];
    if (r < 0 || r >= n_nodes || c < 0 || c >= n_nodes) r = c = 0;   // (not a pair of this batch: a defined value, no wild read)
    const float* a = emb + r * ld;
    const float* b = emb + c * ld;
    float acc = 0.f;
    if (dim % 4 == 0 && ld % 4 == 0 && (((uintptr_t)emb) & 15) == 0) {
        for (int k = lane * 4; k < dim; k += 256) {
            const float4 x = *reinterpret_cast<const float4*>(a + k);
            const float4 y = *reinterpret_cast<const float4*>(b + k);
            float d;
            d = x.x - y.x + eps; acc = fmaf(d, d, acc);
            d = x.y - y.y + eps; acc = fmaf(d, d, acc);
            d = x.z - y.z + eps; acc = fmaf(d, d, acc);
            d = x.w - y.w + eps; acc = fmaf(d, d, acc);
        }
    } else {
        for (int k = lane; k < dim; k += 64) {
            const float d = a[k] - b[k] + eps;
            acc = fmaf(d, d, acc);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane != 0) return;
    dist[e] = sqrtf(acc);
    int g = node_graph[r];
    g = g < 0 ? 0 : (g >= n_graphs ? n_graphs - 1 : g);
    const float f = fps[g];
    const float tr = (float)frame[r] / f, tc = (float)frame[c] / f;       // .float() / fps per node, then the difference (graph.py:106, :116)
    const float hr = cols[r * 4 + 0], hc = cols[c * 4 + 0];
    const float mean_h = (hr + hc) / 2.f;
    float* o = feats + e * 5;
    o[0] = tc - tr;
    o[1] = (cols[c * 4 + 2] - cols[r * 4 + 2]) / mean_h;
    o[2] = (cols[c * 4 + 3] - cols[r * 4 + 3]) / mean_h;
    o[3] = logf(hc / hr);
    o[4] = logf(cols[c * 4 + 1] / cols[r * 4 + 1]);
}

// the graph of kept pair k (its row's); pairs are listed by ascending row, so this never decreases with k
__device__ __forceinline__ int graph_of_kept(const int64_t* __restrict__ pairs, int64_t n_pairs, const int32_t* __restrict__ kept, int64_t k,
                                             const int32_t* __restrict__ node_graph, int n_nodes, int n_graphs) {
    int64_t p = kept ? (int64_t)kept[k] : k;
    p = p < 0 ? 0 : (p >= n_pairs ? n_pairs - 1 : p);
    int64_t r = pairs[p];
    r = r < 0 ? 0 : (r >= n_nodes ? n_nodes - 1 : r);
    const int g = node_graph[r];
    return g < 0 ? 0 : (g >= n_graphs ? n_graphs - 1 : g);
}

// pair_ptr[g] = first kept pair of a graph >= g (g = 0 .. n_graphs; pair_ptr[n_graphs] = n_kept): one thread per entry
__global__ void k_pair_ptr(const int64_t* __restrict__ pairs, int64_t n_pairs, const int32_t* __restrict__ kept, int64_t n_kept,
                           const int32_t* __restrict__ node_graph, int n_nodes, int n_graphs, int64_t* __restrict__ pair_ptr) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g > n_graphs) return;
    int64_t lo = 0, hi = n_kept;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (graph_of_kept(pairs, n_pairs, kept, mid, node_graph, n_nodes, n_graphs) < g) lo = mid + 1; else hi = mid;
    }
    pair_ptr[g] = lo;
}

// kept pair k of graph g, the a-th of its graph's m: edge 2 * pair_ptr[g] + a = (row, col), edge ... + m + a = (col, row); the
// chosen feature columns are copied to both (mot_graph.py:311-312: duplicated, not sign-flipped)
struct LayoutCols { int n; int col[MPNHIP_EDGE_ATTR_COLS]; };
__global__ void k_edge_layout(const int64_t* __restrict__ pairs, int64_t n_pairs, const int32_t* __restrict__ kept, int64_t n_kept,
                              const int32_t* __restrict__ node_graph, int n_nodes, int n_graphs, const int64_t* __restrict__ pair_ptr,
                              const float* __restrict__ feats, const float* __restrict__ dist, LayoutCols lc,
                              int64_t* __restrict__ edge_index, float* __restrict__ edge_attr, int32_t* __restrict__ edge_graph) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_kept) return;
    const int64_t p = kept ? (int64_t)kept[k] : k;
    const bool ok = p >= 0 && p < n_pairs;
    const int g = graph_of_kept(pairs, n_pairs, kept, k, node_graph, n_nodes, n_graphs);
    int64_t first = pair_ptr[g], m = pair_ptr[g + 1] - first;
    if (first < 0 || first > k || m <= k - first || first + m > n_kept) { first = k; m = 1; }   // (a list not sorted by graph: stay inside)
    const int64_t fwd = 2 * first + (k - first), bwd = fwd + m, E = 2 * n_kept;
    const int64_t r = ok ? pairs[p] : 0, c = ok ? pairs[n_pairs + p] : 0;
    edge_index[fwd] = r; edge_index[E + fwd] = c;
    edge_index[bwd] = c; edge_index[E + bwd] = r;
    edge_graph[fwd] = g; edge_graph[bwd] = g;
    for (int q = 0; q < lc.n; ++q) {
        const float v = !ok ? 0.f : (lc.col[q] < 5 ? feats[p * 5 + lc.col[q]] : dist[p]);
        edge_attr[fwd * lc.n + q] = v;
        edge_attr[bwd * lc.n + q] = v;
    }
}

// mpnhip_augment_boxes' workspace: the minimum's key, the count of rows outside the table
struct AugmentView { unsigned long long* min_key; int32_t* bad_rows; size_t bytes; };
static AugmentView augment_view(void* workspace) {
    Carver c(workspace);
    AugmentView v = {c.take<unsigned long long>(1), c.take<int32_t>(1), 0};
    v.bytes = c.bytes();
    return v;
}

// mpnhip_batch_pairs_count's workspace: the rows' pair counts [N + 1] (the last one 0), rocprim's scratch
struct BatchPairsView { int64_t* counts; void* tmp; size_t tmp_bytes; size_t bytes; };
static BatchPairsView batch_pairs_view(void* workspace, int64_t n_nodes) {
    Carver c(workspace);
    BatchPairsView v = {c.take<int64_t>((size_t)n_nodes + 1), nullptr, exclusive_scan_temp<int64_t>(n_nodes + 1), 0};
    v.tmp = c.take<char>(v.tmp_bytes);
    v.bytes = c.bytes() + 256;
    return v;
}

// mpnhip_batch_edge_layout's workspace: pair_ptr [B + 1]
struct LayoutView { int64_t* pair_ptr; size_t bytes; };
static LayoutView layout_view(void* workspace, int64_t n_graphs) {
    Carver c(workspace);
    LayoutView v = {c.take<int64_t>((size_t)n_graphs + 1), 0};
    v.bytes = c.bytes();
    return v;
}

static bool batch_sizes_ok(int64_t n_nodes, int64_t n_graphs) {
    return n_nodes >= 0 && n_nodes < (1LL << 31) - 64 && n_graphs >= 0 && n_graphs < (1LL << 31) - 1;
}

}  // namespace
}  // namespace mpnhip

using namespace mpnhip;

extern "C" size_t mpnhip_augment_boxes_workspace_bytes(void) { return augment_view(nullptr).bytes; }

extern "C" int mpnhip_augment_boxes(const double* boxes, const int64_t* frame, const int64_t* ids, int64_t n_rows, const int32_t* node_src,
                                    const int32_t* graph_ptr_host, int64_t n_graphs, const double* eps, int64_t n_nodes, double* out_boxes,
                                    float* out_cols, int64_t* out_frame, int64_t* out_id, int32_t* node_graph, int32_t* graph_ptr,
                                    double* min_iou, int32_t* bad_rows, void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(batch_sizes_ok(n_nodes, n_graphs) && n_rows >= 0, "augment_boxes: bad sizes");
    MPN_CHECK_ARG(n_graphs > 0 || n_nodes == 0, "augment_boxes: nodes without a graph");
    if (n_graphs == 0) return MPNHIP_OK;
    MPN_CHECK_ARG(graph_ptr_host && graph_ptr, "augment_boxes: null graph_ptr");
    MPN_CHECK_ARG(graph_ptr_host[0] == 0 && graph_ptr_host[n_graphs] == n_nodes, "augment_boxes: graph_ptr must run from 0 to the node count");
    for (int64_t g = 0; g < n_graphs; ++g)
        MPN_CHECK_ARG(graph_ptr_host[g] <= graph_ptr_host[g + 1], "augment_boxes: graph_ptr is not ascending at graph %lld", (long long)g);
    MPN_CHECK_ARG(min_iou && bad_rows, "augment_boxes: null min_iou or bad_rows");
    MPN_CHECK_ARG(n_nodes == 0 || (boxes && frame && ids && node_src && out_boxes && out_cols && out_frame && out_id && node_graph),
                  "augment_boxes: null table, node_src or results");
    AugmentView v = augment_view(workspace);
    MPN_CHECK_WORKSPACE("augment_boxes", workspace, workspace_bytes, v.bytes);
    MPN_HIP(hipMemcpyAsync(graph_ptr, graph_ptr_host, ((size_t)n_graphs + 1) * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    MPN_HIP(hipMemsetAsync(v.min_key, 0xff, sizeof(unsigned long long), stream));
    MPN_HIP(hipMemsetAsync(bad_rows, 0, sizeof(int32_t), stream));
    if (n_nodes > 0) {
        hipLaunchKernelGGL(k_augment_boxes, dim3(blocks_for(n_nodes)), dim3(256), 0, stream, boxes, frame, ids, n_rows, node_src, graph_ptr,
                           (int)n_graphs, eps, (int)n_nodes, out_boxes, out_cols, out_frame, out_id, node_graph, v.min_key, bad_rows);
        MPN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_min_iou_value, dim3(1), dim3(1), 0, stream, v.min_key, min_iou);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}

extern "C" size_t mpnhip_batch_pairs_workspace_bytes(int64_t n_nodes) {
    return n_nodes < 0 ? 0 : batch_pairs_view(nullptr, n_nodes).bytes;
}

extern "C" int mpnhip_batch_pairs_count(const int64_t* frame_num, const int32_t* node_graph, const int32_t* graph_ptr, int64_t n_graphs,
                                        int64_t n_nodes, int64_t max_frame_dist, int64_t* offsets, void* workspace, size_t workspace_bytes,
                                        void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(batch_sizes_ok(n_nodes, n_graphs), "batch_pairs: bad sizes");
    if (n_nodes == 0) return MPNHIP_OK;   // (no pairs; offsets is not written)
    MPN_CHECK_ARG(n_graphs > 0 && frame_num && node_graph && graph_ptr && offsets, "batch_pairs: nodes without graphs / null pointer");
    BatchPairsView v = batch_pairs_view(workspace, n_nodes);
    MPN_CHECK_WORKSPACE("batch_pairs", workspace, workspace_bytes, v.bytes);
    MPN_HIP(hipMemsetAsync(v.counts, 0, ((size_t)n_nodes + 1) * 8, stream));
    hipLaunchKernelGGL((k_batch_pairs<false>), dim3((unsigned)((n_nodes + 3) / 4)), dim3(256), 0, stream, frame_num, node_graph, graph_ptr,
                       (int)n_graphs, (int)n_nodes, max_frame_dist, v.counts, nullptr, nullptr, nullptr);
    MPN_LAUNCH_CHECK();
    MPN_HIP(rocprim::exclusive_scan(v.tmp, v.tmp_bytes, v.counts, offsets, (int64_t)0, (size_t)n_nodes + 1, rocprim::plus<int64_t>(), stream));
    return MPNHIP_OK;
}

extern "C" int mpnhip_batch_pairs_fill(const int64_t* frame_num, const int32_t* node_graph, const int32_t* graph_ptr, int64_t n_graphs,
                                       int64_t n_nodes, int64_t max_frame_dist, const int64_t* offsets, int64_t n_pairs, int64_t* edge_ixs,
                                       void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(batch_sizes_ok(n_nodes, n_graphs) && n_pairs >= 0, "batch_pairs: bad sizes");
    if (n_nodes == 0 || n_pairs == 0) return MPNHIP_OK;
    MPN_CHECK_ARG(n_graphs > 0 && frame_num && node_graph && graph_ptr && offsets && edge_ixs, "batch_pairs: nodes without graphs / null pointer");
    hipLaunchKernelGGL((k_batch_pairs<true>), dim3((unsigned)((n_nodes + 3) / 4)), dim3(256), 0, stream, frame_num, node_graph, graph_ptr,
                       (int)n_graphs, (int)n_nodes, max_frame_dist, nullptr, offsets, edge_ixs, edge_ixs + n_pairs);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}

extern "C" int mpnhip_batch_edge_features(const int64_t* edge_ixs, int64_t n_edges, int64_t n_nodes, const int64_t* frame_num,
                                          const int32_t* node_graph, const float* fps, int64_t n_graphs, const float* node_cols,
                                          const float* emb, int64_t ld, int dim, float eps, float* edge_feats, float* emb_dist,
                                          void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(n_edges >= 0 && batch_sizes_ok(n_nodes, n_graphs) && dim >= 0 && ld >= dim, "batch_edge_features: bad sizes");
    if (n_edges == 0) return MPNHIP_OK;
    MPN_CHECK_ARG(n_nodes > 0 && n_graphs > 0, "batch_edge_features: edges without nodes or graphs");
    MPN_CHECK_ARG(edge_ixs && frame_num && node_graph && fps && node_cols && edge_feats && emb_dist && (emb || dim == 0),
                  "batch_edge_features: null pointer");
    hipLaunchKernelGGL(k_batch_edge_feats, dim3((unsigned)((n_edges + 3) / 4)), dim3(256), 0, stream, edge_ixs, n_edges, (int)n_nodes,
                       frame_num, node_graph, fps, (int)n_graphs, node_cols, emb, ld, dim, eps, edge_feats, emb_dist);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}

extern "C" size_t mpnhip_batch_edge_layout_workspace_bytes(int64_t n_graphs) {
    return n_graphs < 0 ? 0 : layout_view(nullptr, n_graphs).bytes;
}

extern "C" int mpnhip_batch_edge_layout(const int64_t* pairs, int64_t n_pairs, const int32_t* kept, int64_t n_kept, const int32_t* node_graph,
                                        int64_t n_nodes, int64_t n_graphs, const float* edge_feats, const float* emb_dist,
                                        const int32_t* attr_cols, int n_attr_cols, int64_t* edge_index, float* edge_attr,
                                        int32_t* edge_graph, void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(n_pairs >= 0 && n_kept >= 0 && n_kept <= n_pairs && n_pairs < (1LL << 31) && batch_sizes_ok(n_nodes, n_graphs),
                  "batch_edge_layout: bad sizes (at most 2^31 - 1 pairs, no more kept than there are)");
    MPN_CHECK_ARG(n_attr_cols >= 0 && n_attr_cols <= MPNHIP_EDGE_ATTR_COLS && (attr_cols || n_attr_cols == 0),
                  "batch_edge_layout: 0 .. %d attribute columns", MPNHIP_EDGE_ATTR_COLS);
    LayoutCols lc = {n_attr_cols, {0}};
    for (int q = 0; q < n_attr_cols; ++q) {
        MPN_CHECK_ARG(attr_cols[q] >= 0 && attr_cols[q] < MPNHIP_EDGE_ATTR_COLS, "batch_edge_layout: attribute column %d is not one of 0 .. %d",
                      attr_cols[q], MPNHIP_EDGE_ATTR_COLS - 1);
        lc.col[q] = attr_cols[q];
    }
    if (n_kept == 0) return MPNHIP_OK;
    MPN_CHECK_ARG(n_nodes > 0 && n_graphs > 0, "batch_edge_layout: pairs without nodes or graphs");
    MPN_CHECK_ARG(pairs && node_graph && edge_index && edge_graph && (n_attr_cols == 0 || (edge_feats && emb_dist && edge_attr)),
                  "batch_edge_layout: null pointer");
    LayoutView v = layout_view(workspace, n_graphs);
    MPN_CHECK_WORKSPACE("batch_edge_layout", workspace, workspace_bytes, v.bytes);
    hipLaunchKernelGGL(k_pair_ptr, dim3(blocks_for(n_graphs + 1)), dim3(256), 0, stream, pairs, n_pairs, kept, n_kept, node_graph, (int)n_nodes,
                       (int)n_graphs, v.pair_ptr);
    MPN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_edge_layout, dim3(blocks_for(n_kept)), dim3(256), 0, stream, pairs, n_pairs, kept, n_kept, node_graph, (int)n_nodes,
                       (int)n_graphs, v.pair_ptr, edge_feats, emb_dist, lc, edge_index, edge_attr, edge_graph);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}
