// Graph preparation: one stable sort of the edges by (direction, row) replaces the per-step boolean
// masks / nonzero() syncs of TimeAwareNodeModel.forward (reference models/mpn.py:85-87,91-93) and
// gives every scatter of the path (torch_scatter calls at mpn.py:266-273, index_put_ in autograd) a
// CSR form that needs no atomics and fixes the summation order to the reference CPU order
// (ascending edge id inside a segment).
#include <cstring>

#include "device_prims.h"

namespace mpnhip {

size_t graph_layout(int N, int64_t E, GraphView* v, void* base) {
    Carver c(base);
    GraphView g;
    g.N = N;
    g.E = E;
    g.header = c.take<int>(8);
    g.perm = c.take<int>((size_t)E);
    g.srow = c.take<int>((size_t)E);
    g.scol = c.take<int>((size_t)E);
    g.seg_ptr = c.take<int>(3 * (size_t)N + 1);
    g.cperm = c.take<int>((size_t)E);
    g.cseg_ptr = c.take<int>(3 * (size_t)N + 1);
    g.rperm = c.take<int>((size_t)E);
    g.rseg_ptr = c.take<int>((size_t)N + 1);
    g.cperm_all = c.take<int>((size_t)E);
    g.cseg_all = c.take<int>((size_t)N + 1);
    if (v) *v = g;
    return c.bytes();
}

__global__ void k_make_keys(const int64_t* __restrict__ ei, int64_t E, int N, unsigned* __restrict__ keys,
                            int* __restrict__ vals, int* __restrict__ header) {
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    int64_t r = ei[e], c = ei[E + e];
    if (r < 0 || r >= N || c < 0 || c >= N) {
        header[0] = 1;  // benign race: every writer stores the same value
        r = r < 0 ? 0 : (r >= N ? N - 1 : r);
        c = c < 0 ? 0 : (c >= N ? N - 1 : c);
    }
    unsigned dir = r < c ? 0u : (r > c ? 1u : 2u);
    keys[e] = dir * (unsigned)N + (unsigned)r;
    vals[e] = (int)e;
}

__global__ void k_gather_rc(const int64_t* __restrict__ ei, int64_t E, int N, const int* __restrict__ perm,
                            int* __restrict__ srow, int* __restrict__ scol) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= E) return;
    int64_t e = perm[i];
    int64_t r = ei[e], c = ei[E + e];
    r = r < 0 ? 0 : (r >= N ? N - 1 : r);
    c = c < 0 ? 0 : (c >= N ? N - 1 : c);
    srow[i] = (int)r;
    scol[i] = (int)c;
}

// ptr[k] = first position whose sorted key is >= k, k = 0..nkeys (ptr[nkeys] = E)
__global__ void k_lower_bound(const unsigned* __restrict__ skeys, int64_t E, int nkeys, int* __restrict__ ptr) {
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k > nkeys) return;
    int64_t lo = 0, hi = E;
    while (lo < hi) {
        int64_t mid = (lo + hi) >> 1;
        if (skeys[mid] < (unsigned)k) lo = mid + 1; else hi = mid;
    }
    ptr[k] = (int)lo;
}

__global__ void k_header(const int* __restrict__ seg_ptr, int N, int64_t E, int* __restrict__ header) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        int e_out = seg_ptr[N], e_in = seg_ptr[2 * N] - seg_ptr[N];
        header[1] = e_out;
        header[2] = e_in;
        header[3] = (int)E - e_out - e_in;
        header[4] = e_out;         // row_end of the flow_out group / row_begin of the flow_in group
        header[5] = e_out + e_in;  // row_end of the flow_in group
        header[6] = 0;
        header[7] = (int)E;
    }
}

// keys for the secondary (backward) orders, over SORTED positions
__global__ void k_keys2(const int* __restrict__ srow, const int* __restrict__ scol, int64_t E, int N, int mode,
                        unsigned* __restrict__ keys, int* __restrict__ vals) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= E) return;
    int r = srow[i], c = scol[i];
    unsigned dir = r < c ? 0u : (r > c ? 1u : 2u);
    unsigned k = mode == 0 ? dir * (unsigned)N + (unsigned)c : (mode == 1 ? (unsigned)r : (unsigned)c);
    keys[i] = k;
    vals[i] = (int)i;
}

// the sort's workspace: unsorted keys, sorted keys, unsorted values [max(E, 1)] each, rocprim's scratch
struct PrepView { unsigned* keys_in; unsigned* keys_out; int* vals_in; void* tmp; size_t tmp_bytes; size_t bytes; };
static PrepView prep_view(void* workspace, int64_t E) {
    Carver c(workspace);
    const size_t e = (size_t)(E > 0 ? E : 1);
    PrepView v = {c.take<unsigned>(e), c.take<unsigned>(e), c.take<int>(e), nullptr, sort_pairs_temp<unsigned>(E), 0};
    v.tmp = c.take<char>(v.tmp_bytes);
    v.bytes = c.bytes() + 256;
    return v;
}

}  // namespace mpnhip

using namespace mpnhip;

extern "C" size_t mpnhip_graph_bytes(int n_nodes, int64_t n_edges) {
    return graph_layout(n_nodes, n_edges, nullptr, nullptr);
}

extern "C" size_t mpnhip_graph_prep_workspace_bytes(int n_nodes, int64_t n_edges) {
    return prep_view(nullptr, n_edges).bytes;
}

static int graph_prep_impl(const int64_t* edge_index, int n_nodes, int64_t n_edges, void* graph_buf, size_t graph_bytes,
                           void* workspace, size_t workspace_bytes, bool secondary, void* stream_);

extern "C" int mpnhip_graph_prep(const int64_t* edge_index, int n_nodes, int64_t n_edges, void* graph_buf,
                                 size_t graph_bytes, void* workspace, size_t workspace_bytes, void* stream_) {
    return graph_prep_impl(edge_index, n_nodes, n_edges, graph_buf, graph_bytes, workspace, workspace_bytes, true, stream_);
}

extern "C" int mpnhip_graph_prep_forward(const int64_t* edge_index, int n_nodes, int64_t n_edges, void* graph_buf,
                                         size_t graph_bytes, void* workspace, size_t workspace_bytes, void* stream_) {
    return graph_prep_impl(edge_index, n_nodes, n_edges, graph_buf, graph_bytes, workspace, workspace_bytes, false, stream_);
}

static int graph_prep_impl(const int64_t* edge_index, int n_nodes, int64_t n_edges, void* graph_buf, size_t graph_bytes,
                           void* workspace, size_t workspace_bytes, bool secondary, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int N = n_nodes;
    const int64_t E = n_edges;
    MPN_CHECK_ARG(N >= 0 && E >= 0, "graph_prep: negative sizes");
    MPN_CHECK_ARG((int64_t)3 * N + 1 < 2147483647LL && E < 2147483647LL, "graph_prep: graph too large for int32 indices");
    MPN_CHECK_ARG(graph_buf && (E == 0 || edge_index), "graph_prep: null pointer");
    if (graph_bytes < mpnhip_graph_bytes(N, E)) {
        set_error("graph_prep: graph buffer %zu < %zu", graph_bytes, mpnhip_graph_bytes(N, E));
        return MPNHIP_ERR_WORKSPACE;
    }
    PrepView w = prep_view(workspace, E);
    if (E > 0 || workspace_bytes < w.bytes) MPN_CHECK_WORKSPACE("graph_prep", workspace, workspace_bytes, w.bytes);   // (no edges: may be null)
    GraphView g;
    graph_layout(N, E, &g, graph_buf);
    MPN_HIP(hipMemsetAsync(g.header, 0, 8 * sizeof(int), stream));
    const int T = 256;
    const unsigned nbE = blocks_for(E);
    if (E == 0) {
        MPN_HIP(hipMemsetAsync(g.seg_ptr, 0, (3 * (size_t)N + 1) * sizeof(int), stream));
        MPN_HIP(hipMemsetAsync(g.cseg_ptr, 0, (3 * (size_t)N + 1) * sizeof(int), stream));
        MPN_HIP(hipMemsetAsync(g.rseg_ptr, 0, ((size_t)N + 1) * sizeof(int), stream));
        MPN_HIP(hipMemsetAsync(g.cseg_all, 0, ((size_t)N + 1) * sizeof(int), stream));
        return MPNHIP_OK;
    }
    // primary order: (direction, row), stable
    hipLaunchKernelGGL(k_make_keys, dim3(nbE), dim3(T), 0, stream, edge_index, E, N, w.keys_in, w.vals_in, g.header);
    MPN_LAUNCH_CHECK();
    MPN_HIP(rocprim::radix_sort_pairs(w.tmp, w.tmp_bytes, w.keys_in, w.keys_out, w.vals_in, g.perm, (size_t)E, 0,
                                      key_bits(3u * (unsigned)N), stream));
    hipLaunchKernelGGL(k_gather_rc, dim3(nbE), dim3(T), 0, stream, edge_index, E, N, g.perm, g.srow, g.scol);
    MPN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_lower_bound, dim3((3 * N + 1 + T) / T), dim3(T), 0, stream, w.keys_out, E, 3 * N, g.seg_ptr);
    MPN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_header, dim3(1), dim3(64), 0, stream, g.seg_ptr, N, E, g.header);
    MPN_LAUNCH_CHECK();

    if (!secondary) return MPNHIP_OK;  // inference: mpnhip_forward reads the primary order only
    // secondary orders for the backward scatter-adds (index_put_ of x[row], x[col])
    struct { int mode; int* perm; int* ptr; int nkeys; } sec[3] = {
        {0, g.cperm, g.cseg_ptr, 3 * N}, {1, g.rperm, g.rseg_ptr, N}, {2, g.cperm_all, g.cseg_all, N}};
    for (auto& s : sec) {
        hipLaunchKernelGGL(k_keys2, dim3(nbE), dim3(T), 0, stream, g.srow, g.scol, E, N, s.mode, w.keys_in, w.vals_in);
        MPN_LAUNCH_CHECK();
        MPN_HIP(rocprim::radix_sort_pairs(w.tmp, w.tmp_bytes, w.keys_in, w.keys_out, w.vals_in, s.perm, (size_t)E, 0,
                                          key_bits((unsigned)s.nkeys), stream));
        hipLaunchKernelGGL(k_lower_bound, dim3((s.nkeys + 1 + T) / T), dim3(T), 0, stream, w.keys_out, E, s.nkeys, s.ptr);
        MPN_LAUNCH_CHECK();
    }
    return MPNHIP_OK;
}

extern "C" int mpnhip_graph_status(const void* graph_buf, int n_nodes, int64_t n_edges, int32_t status[4], void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(graph_buf && status, "graph_status: null pointer");
    GraphView g;
    graph_layout(n_nodes, n_edges, &g, const_cast<void*>(graph_buf));
    MPN_HIP(hipMemcpyAsync(status, g.header, 4 * sizeof(int), hipMemcpyDeviceToHost, stream));
    MPN_HIP(hipStreamSynchronize(stream));
    return MPNHIP_OK;
}
