// The rounding LP of ExactProjector (reference tracker/projectors.py:92-113, :129-160) as batched linear assignment.
//
// The reference minimises sum x_e (1 - 2 p_e) over 0 <= x <= 1 with in-flow <= 1 and out-flow <= 1 per node, on the edges that
// touch a violated node (edges_mask of mpnhip_project_violated_masks).  Every edge joins the OUT-copy of its row to the IN-copy
// of its column, so the constraint matrix is the incidence matrix of a bipartite graph and the LP is a maximum-weight matching:
//   - an edge with p <= 0.5 (or NaN) has a cost >= 0 and is 0 in an optimum: only the ACTIVE edges (masked, ids in range,
//     p > 0.5) take part;
//   - the active edges split into connected components of the bipartite graph on 2 n_nodes vertices (u: out-copy of u,
//     n_nodes + v: in-copy of v), and every component is one small dense assignment: rows = its out-copies, columns = its
//     in-copies, cell = 1 - 2 p for an active edge and 0 elsewhere.  A complete assignment of such a matrix pays 0 for a pair
//     that is no edge, which is "the row stays unmatched" of the LP; a pair that is an edge costs < 0.
// Where the LP's optimum is unique the assignment's is the same; among ties (scores of exactly 0.5 never take part, equal totals
// of different matchings do) mpnhip_lsa_batched picks by its own rule (include/mpnhip.h).
//
// Three calls around mpnhip_lsa_batched, which is used as it is:
//   plan   union-find (projection_common.h) over the active edges; a problem = a component with an active edge.  Its root is its
//          smallest vertex, always an out-copy, so problems are ranked by a scan over the root flags of the first n_nodes
//          vertices.  Rows and columns are put in (problem, node id) order by one stable radix sort per side; counts per problem
//          and two scans give a_ptr / b_ptr / cell_ptr.
//   fill   cost cells.  Duplicate active edges of one pair: the largest score wins, the lowest edge id among equals -- the
//          64-bit arg-max key of mpnhip_project_greedy, atomicMax'ed INTO the zeroed cost cell (8 bytes either way); a second
//          pass marks the winners, a third lets each winner write 1 - 2 p over its key.  Cells without an edge keep the zero bits.
//   apply  a masked edge is 1 iff it is its cell's winner and the assignment matched its row to its column.
// Integer and compare-only arithmetic apart from the one float64 expression per cell; integer atomics only; the loops are the
// union-find's walks (strictly falling ids) and a binary search.  The same bits whatever the edge order, up to the edge-id tie of
// duplicate pairs.
#include "device_prims.h"
#include "label_tables.h"
#include "projection_common.h"

namespace mpnhip {
namespace {

enum { SZ_PROBLEMS = 0, SZ_A = 1, SZ_B = 2, SZ_MAX_SIDE = 3, SZ_CELLS = 4, SZ_SKIPPED = 5, SZ_COUNT = 6 };

static const int64_t XP_MAX_IDS = 1LL << 30;   // 2 n_nodes vertices as int32; edge ids as the low word of the arg-max key

__device__ __forceinline__ bool xp_active(const int64_t* __restrict__ ei, int64_t e, int64_t K, int64_t N,
                                          const float* __restrict__ preds, const unsigned char* __restrict__ mask, int64_t& r,
                                          int64_t& c) {
    r = ei[e];
    c = ei[K + e];
    return ids_ok(r, c, N) && mask[e] && preds[e] > 0.5f;   // (NaN > 0.5 is false)
}

// has[vertex] = 1 for the end points of the active edges (every writer stores the same 1); skipped edges are counted
__global__ void k_xp_union(const int64_t* __restrict__ ei, int64_t K, int64_t N, const float* __restrict__ preds,
                           const unsigned char* __restrict__ mask, int* parent, unsigned char* __restrict__ has,
                           unsigned long long* __restrict__ sizes) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= K) return;
    int64_t r, c;
    if (!xp_active(ei, e, K, N, preds, mask, r, c)) {
        if (!ids_ok(r, c, N)) atomicAdd(&sizes[SZ_SKIPPED], 1ull);
        return;
    }
    has[r] = 1;
    has[N + c] = 1;
    cc_link(parent, (int)r, (int)(N + c));
}

// the root of a problem: a root among the out-copies that has an active edge (an in-copy is never the smallest of a component)
__global__ void k_xp_root_flags(const int* __restrict__ root, const unsigned char* __restrict__ has, int64_t N,
                                int* __restrict__ is_root) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v < N) is_root[v] = (root[v] == (int)v && has[v]) ? 1 : 0;
}

// SIDE 0: out-copies (rows), 1: in-copies (columns).  key[v] = the problem of the copy of node v, N for a copy without an
// active edge (sorted behind every problem); cnt[problem] += 1
template <int SIDE>
__global__ void k_xp_keys(const int* __restrict__ root, const unsigned char* __restrict__ has, const int* __restrict__ rank,
                          int64_t N, unsigned* __restrict__ key, int* __restrict__ iota, int* __restrict__ cnt) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= N) return;
    iota[v] = (int)v;
    const int64_t vert = SIDE == 0 ? v : N + v;
    unsigned k = (unsigned)N;
    if (has[vert]) {
        const int rt = root[vert];
        if (rt >= 0 && rt < N) {
            const int f = rank[rt];
            if (f >= 0 && f < N) {
                k = (unsigned)f;
                atomicAdd(&cnt[f], 1);
            }
        }
    }
    key[v] = k;
}

__global__ void k_xp_slots(const unsigned* __restrict__ key_sorted, const int* __restrict__ node_sorted, int64_t N,
                           int* __restrict__ slot) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int v = node_sorted[i];
    if (key_sorted[i] < (unsigned)N && v >= 0 && v < N) slot[v] = (int)i;
}

// f in [0, N]: cells of problem f (0 behind the last problem) and the largest side
__global__ void k_xp_cells(const int* __restrict__ cnt_a, const int* __restrict__ cnt_b, int64_t N, int64_t* __restrict__ prod,
                           unsigned long long* __restrict__ sizes) {
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f > N) return;
    const int na = cnt_a[f], nb = cnt_b[f];
    prod[f] = (int64_t)na * nb;
    const int side = na > nb ? na : nb;
    if (side > 0) atomicMax(&sizes[SZ_MAX_SIDE], (unsigned long long)side);
}

__global__ void k_xp_sizes(const int* __restrict__ rank, const int* __restrict__ is_root, const int* __restrict__ a_ptr,
                           const int* __restrict__ b_ptr, const int64_t* __restrict__ cell_ptr, int64_t N,
                           unsigned long long* __restrict__ sizes) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    sizes[SZ_PROBLEMS] = (unsigned long long)(rank[N - 1] + is_root[N - 1]);
    sizes[SZ_A] = (unsigned long long)a_ptr[N];
    sizes[SZ_B] = (unsigned long long)b_ptr[N];
    sizes[SZ_CELLS] = (unsigned long long)cell_ptr[N];
}

struct XpLists {
    const int* a_slot; const int* b_slot; const int* a_ptr; const int* b_ptr; const int64_t* cell_ptr;
    int n_problems, n_a, n_b;
    int64_t cells;
};

// the cost cell of an active edge, or -1; every index read from an array is checked before it is used
__device__ __forceinline__ int64_t xp_cell(const XpLists& L, int64_t r, int64_t c) {
    const int sa = L.a_slot[r], sb = L.b_slot[c];
    if (sa < 0 || sa >= L.n_a || sb < 0 || sb >= L.n_b) return -1;
    const int f = frame_of(L.a_ptr, L.n_problems, sa);
    if (f < 0) return -1;
    const int b0 = L.b_ptr[f], nb = L.b_ptr[f + 1] - b0, la = sa - L.a_ptr[f], lb = sb - b0;
    if (lb < 0 || lb >= nb) return -1;
    const int64_t cell = L.cell_ptr[f] + (int64_t)la * nb + lb;
    return (cell >= 0 && cell < L.cells) ? cell : -1;
}

// PASS 0: arg-max keys into the zeroed cells; 1: win[e] = the edge holds its cell's key; 2: the winners write their cost
template <int PASS>
__global__ void k_xp_fill(const int64_t* __restrict__ ei, int64_t K, int64_t N, const float* __restrict__ preds,
                          const unsigned char* __restrict__ mask, XpLists L, unsigned long long* cell_keys, double* cost,
                          unsigned char* __restrict__ win) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= K) return;
    if (PASS == 2 && !win[e]) return;
    int64_t r, c;
    const int64_t cell = xp_active(ei, e, K, N, preds, mask, r, c) ? xp_cell(L, r, c) : -1;
    if (PASS == 1) win[e] = (cell >= 0 && cell_keys[cell] == pack_key(preds[e], e)) ? 1 : 0;
    if (cell < 0) return;
    if (PASS == 0) {
        const unsigned long long key = pack_key(preds[e], e);
        if (key > __atomic_load_n(&cell_keys[cell], __ATOMIC_RELAXED)) atomicMax(&cell_keys[cell], key);
    }
    if (PASS == 2) cost[cell] = 1.0 - 2.0 * (double)preds[e];
}

__global__ void k_xp_apply(const int64_t* __restrict__ ei, int64_t K, int64_t N, const unsigned char* __restrict__ mask,
                           const float* __restrict__ round_preds, const int* __restrict__ a_slot, const int* __restrict__ b_slot,
                           const int* __restrict__ match_b, int n_a, const unsigned char* __restrict__ win, float* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= K) return;
    if (!mask[e]) {
        out[e] = round_preds[e];
        return;
    }
    float x = 0.f;
    const int64_t r = ei[e], c = ei[K + e];
    if (win[e] && ids_ok(r, c, N)) {
        const int sa = a_slot[r];
        if (sa >= 0 && sa < n_a && match_b[sa] == b_slot[c]) x = 1.f;
    }
    out[e] = x;
}

// ONE workspace for the three calls: the winner flags the fill leaves for the apply at its head, then the plan's scratch
struct XpView {
    unsigned char* win;       // [K]
    int* parent;              // [2 N]
    int* root;                // [2 N]
    unsigned char* has;       // [2 N]
    int* is_root;             // [N]
    int* rank;                // [N]
    int* cnt_a;               // [N + 1]
    int* cnt_b;               // [N + 1]
    int64_t* prod;            // [N + 1]
    unsigned* key;            // [N]
    unsigned* key_sorted;     // [N]
    int* iota;                // [N]
    int* node_sorted;         // [N]
    void* tmp;
    size_t tmp_bytes, bytes;
};
static XpView xp_view(void* workspace, int64_t n_nodes, int64_t n_edges) {
    if (n_nodes <= 0 && n_edges <= 0) return {};
    Carver c(workspace);
    const size_t n = (size_t)(n_nodes > 0 ? n_nodes : 0), k = (size_t)(n_edges > 0 ? n_edges : 0);
    XpView v = {};
    v.win = c.take<unsigned char>(k);
    v.parent = c.take<int>(2 * n);
    v.root = c.take<int>(2 * n);
    v.has = c.take<unsigned char>(2 * n);
    v.is_root = c.take<int>(n);
    v.rank = c.take<int>(n);
    v.cnt_a = c.take<int>(n + 1);
    v.cnt_b = c.take<int>(n + 1);
    v.prod = c.take<int64_t>(n + 1);
    v.key = c.take<unsigned>(n);
    v.key_sorted = c.take<unsigned>(n);
    v.iota = c.take<int>(n);
    v.node_sorted = c.take<int>(n);
    const size_t t0 = sort_pairs_temp<unsigned>(n_nodes), t1 = exclusive_scan_temp<int>(n_nodes + 1),
                 t2 = exclusive_scan_temp<int64_t>(n_nodes + 1);
    v.tmp_bytes = t0 > t1 ? (t0 > t2 ? t0 : t2) : (t1 > t2 ? t1 : t2);
    v.tmp = c.take<char>(v.tmp_bytes);
    v.bytes = c.bytes();
    return v;
}

static bool xp_sizes_ok(int64_t n_edges, int64_t n_nodes) {
    return n_edges >= 0 && n_edges < XP_MAX_IDS && n_nodes >= 0 && n_nodes < XP_MAX_IDS;
}

}  // namespace
}  // namespace mpnhip

using namespace mpnhip;

extern "C" size_t mpnhip_project_exact_workspace_bytes(int64_t n_nodes, int64_t n_edges) {
    return xp_sizes_ok(n_edges, n_nodes) ? xp_view(nullptr, n_nodes, n_edges).bytes : 0;
}

extern "C" int mpnhip_project_exact_plan(const int64_t* edge_index, int64_t n_edges, int64_t n_nodes, const float* edge_preds,
                                         const unsigned char* edges_mask, int32_t* a_slot, int32_t* b_slot, int32_t* a_ptr,
                                         int32_t* b_ptr, int64_t* cell_ptr, int64_t* sizes, void* workspace, size_t workspace_bytes,
                                         void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(xp_sizes_ok(n_edges, n_nodes), "project_exact_plan: bad sizes");
    MPN_CHECK_ARG(sizes && a_ptr && b_ptr && cell_ptr, "project_exact_plan: null sizes or prefix list");
    MPN_CHECK_ARG(n_nodes == 0 || (a_slot && b_slot), "project_exact_plan: null slot pointer");
    MPN_CHECK_ARG(n_edges == 0 || (edge_index && edge_preds && edges_mask), "project_exact_plan: null edge pointer");
    XpView v = xp_view(workspace, n_nodes, n_edges);
    if (v.bytes) MPN_CHECK_WORKSPACE("project_exact_plan", workspace, workspace_bytes, v.bytes);
    const size_t n = (size_t)n_nodes;
    unsigned long long* sz = reinterpret_cast<unsigned long long*>(sizes);
    MPN_HIP(hipMemsetAsync(sizes, 0, SZ_COUNT * sizeof(int64_t), stream));
    const unsigned nb = blocks_for(n_nodes), nb2 = blocks_for(2 * n_nodes);
    if (n_nodes == 0) {   // (no problem; every edge has ids out of range and is counted below)
        MPN_HIP(hipMemsetAsync(a_ptr, 0, 4, stream));
        MPN_HIP(hipMemsetAsync(b_ptr, 0, 4, stream));
        MPN_HIP(hipMemsetAsync(cell_ptr, 0, 8, stream));
    } else {
        MPN_HIP(hipMemsetAsync(a_slot, 0xFF, n * 4, stream));
        MPN_HIP(hipMemsetAsync(b_slot, 0xFF, n * 4, stream));
        MPN_HIP(hipMemsetAsync(v.has, 0, 2 * n, stream));
        MPN_HIP(hipMemsetAsync(v.cnt_a, 0, (n + 1) * 4, stream));
        MPN_HIP(hipMemsetAsync(v.cnt_b, 0, (n + 1) * 4, stream));
        hipLaunchKernelGGL(k_cc_init, dim3(nb2), dim3(256), 0, stream, v.parent, 2 * n_nodes);
        MPN_LAUNCH_CHECK();
    }
    if (n_edges > 0) {
        hipLaunchKernelGGL(k_xp_union, dim3(blocks_for(n_edges)), dim3(256), 0, stream, edge_index, n_edges, n_nodes, edge_preds,
                           edges_mask, v.parent, v.has, sz);
        MPN_LAUNCH_CHECK();
    }
    if (n_nodes == 0) return MPNHIP_OK;
    hipLaunchKernelGGL(k_cc_roots, dim3(nb2), dim3(256), 0, stream, v.parent, 2 * n_nodes, v.root, (int*)nullptr);
    MPN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_xp_root_flags, dim3(nb), dim3(256), 0, stream, v.root, v.has, n_nodes, v.is_root);
    MPN_LAUNCH_CHECK();
    MPN_HIP(rocprim::exclusive_scan(v.tmp, v.tmp_bytes, v.is_root, v.rank, 0, n, rocprim::plus<int>(), stream));
    const unsigned bits = key_bits((uint64_t)n_nodes);
    // rows, then columns: keys, a stable sort by problem (node ids ascending within one), slots, the prefix list
    hipLaunchKernelGGL(k_xp_keys<0>, dim3(nb), dim3(256), 0, stream, v.root, v.has, v.rank, n_nodes, v.key, v.iota, v.cnt_a);
    MPN_LAUNCH_CHECK();
    MPN_HIP(rocprim::radix_sort_pairs(v.tmp, v.tmp_bytes, v.key, v.key_sorted, v.iota, v.node_sorted, n, 0, bits, stream));
    hipLaunchKernelGGL(k_xp_slots, dim3(nb), dim3(256), 0, stream, v.key_sorted, v.node_sorted, n_nodes, a_slot);
    MPN_LAUNCH_CHECK();
    MPN_HIP(rocprim::exclusive_scan(v.tmp, v.tmp_bytes, v.cnt_a, a_ptr, 0, n + 1, rocprim::plus<int>(), stream));
    hipLaunchKernelGGL(k_xp_keys<1>, dim3(nb), dim3(256), 0, stream, v.root, v.has, v.rank, n_nodes, v.key, v.iota, v.cnt_b);
    MPN_LAUNCH_CHECK();
    MPN_HIP(rocprim::radix_sort_pairs(v.tmp, v.tmp_bytes, v.key, v.key_sorted, v.iota, v.node_sorted, n, 0, bits, stream));
    hipLaunchKernelGGL(k_xp_slots, dim3(nb), dim3(256), 0, stream, v.key_sorted, v.node_sorted, n_nodes, b_slot);
    MPN_LAUNCH_CHECK();
    MPN_HIP(rocprim::exclusive_scan(v.tmp, v.tmp_bytes, v.cnt_b, b_ptr, 0, n + 1, rocprim::plus<int>(), stream));
    hipLaunchKernelGGL(k_xp_cells, dim3(blocks_for(n_nodes + 1)), dim3(256), 0, stream, v.cnt_a, v.cnt_b, n_nodes, v.prod, sz);
    MPN_LAUNCH_CHECK();
    MPN_HIP(rocprim::exclusive_scan(v.tmp, v.tmp_bytes, v.prod, cell_ptr, (int64_t)0, n + 1, rocprim::plus<int64_t>(), stream));
    hipLaunchKernelGGL(k_xp_sizes, dim3(1), dim3(64), 0, stream, v.rank, v.is_root, a_ptr, b_ptr, cell_ptr, n_nodes, sz);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}

// the checks the fill and the apply share
static int xp_edge_args(const char* name, int64_t n_edges, int64_t n_nodes, bool edge_ptrs, bool node_ptrs) {
    MPN_CHECK_ARG(xp_sizes_ok(n_edges, n_nodes), "%s: bad sizes", name);
    MPN_CHECK_ARG(n_edges == 0 || edge_ptrs, "%s: null edge pointer", name);
    MPN_CHECK_ARG(n_edges == 0 || n_nodes == 0 || node_ptrs, "%s: null slot or list pointer", name);
    return MPNHIP_OK;
}

extern "C" int mpnhip_project_exact_fill(const int64_t* edge_index, int64_t n_edges, int64_t n_nodes, const float* edge_preds,
                                         const unsigned char* edges_mask, const int32_t* a_slot, const int32_t* b_slot,
                                         const int32_t* a_ptr, const int32_t* b_ptr, const int64_t* cell_ptr, int64_t n_problems,
                                         int64_t n_a, int64_t n_b, double* cost, int64_t cells, void* workspace,
                                         size_t workspace_bytes, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_TRY(xp_edge_args("project_exact_fill", n_edges, n_nodes, edge_index && edge_preds && edges_mask,
                         a_slot && b_slot && a_ptr && b_ptr && cell_ptr));
    MPN_CHECK_ARG(n_problems >= 0 && n_problems <= n_nodes && n_a >= 0 && n_a <= n_nodes && n_b >= 0 && n_b <= n_nodes && cells >= 0,
                  "project_exact_fill: bad plan sizes");
    MPN_CHECK_ARG(cells == 0 || cost, "project_exact_fill: null cost");
    const XpView v = xp_view(workspace, n_nodes, n_edges);
    if (v.bytes) MPN_CHECK_WORKSPACE("project_exact_fill", workspace, workspace_bytes, v.bytes);
    if (cells > 0) MPN_HIP(hipMemsetAsync(cost, 0, (size_t)cells * 8, stream));
    if (n_edges == 0) return MPNHIP_OK;
    if (n_nodes == 0) {   // (no edge is in range: no winner)
        MPN_HIP(hipMemsetAsync(v.win, 0, (size_t)n_edges, stream));
        return MPNHIP_OK;
    }
    const XpLists L = {a_slot, b_slot, a_ptr, b_ptr, cell_ptr, (int)n_problems, (int)n_a, (int)n_b, cells};
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(cost);
    const unsigned blocks = blocks_for(n_edges);
    hipLaunchKernelGGL(k_xp_fill<0>, dim3(blocks), dim3(256), 0, stream, edge_index, n_edges, n_nodes, edge_preds, edges_mask, L, keys, cost, v.win);
    MPN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_xp_fill<1>, dim3(blocks), dim3(256), 0, stream, edge_index, n_edges, n_nodes, edge_preds, edges_mask, L, keys, cost, v.win);
    MPN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_xp_fill<2>, dim3(blocks), dim3(256), 0, stream, edge_index, n_edges, n_nodes, edge_preds, edges_mask, L, keys, cost, v.win);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}

extern "C" int mpnhip_project_exact_apply(const int64_t* edge_index, int64_t n_edges, int64_t n_nodes, const unsigned char* edges_mask,
                                          const float* round_preds, const int32_t* a_slot, const int32_t* b_slot,
                                          const int32_t* match_b, int64_t n_a, float* out, const void* workspace,
                                          size_t workspace_bytes, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_TRY(xp_edge_args("project_exact_apply", n_edges, n_nodes, edge_index && edges_mask && round_preds && out, a_slot && b_slot));
    MPN_CHECK_ARG(n_a >= 0 && n_a <= n_nodes && (n_a == 0 || n_edges == 0 || match_b), "project_exact_apply: bad n_a or null match_b");
    const XpView v = xp_view(const_cast<void*>(workspace), n_nodes, n_edges);
    if (v.bytes) MPN_CHECK_WORKSPACE("project_exact_apply", workspace, workspace_bytes, v.bytes);
    if (n_edges == 0) return MPNHIP_OK;
    hipLaunchKernelGGL(k_xp_apply, dim3(blocks_for(n_edges)), dim3(256), 0, stream, edge_index, n_edges, n_nodes, edges_mask, round_preds,
                       a_slot, b_slot, match_b, (int)n_a, v.win, out);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}
