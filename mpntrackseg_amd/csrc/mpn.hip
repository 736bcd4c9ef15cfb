// Host-side orchestration of the MPN hot path on one MI355X: MOTMPNet.forward restricted to the
// encoder -> L x {reattach, MetaLayer, classifier} loop (reference models/mpn.py:349-392), expressed
// as fused-epilogue MFMA GEMMs + one segmented aggregation per step.  No allocation, no host sync.
//
// Re-association used (fp32 throughout, only the summation order differs from the reference):
//   EdgeModel  (mpn.py:67-69):  W1 [x[row] | x[col] | e] = (W1r x)[row] + (W1c x)[col] + W1e e
//   flow MLPs  (mpn.py:87-88):  Wf [x[col] | e']         = (Wfx x)[col] + Wfe e'
// The node-side products are computed once per node per step by ONE GEMM against the row-stacked
// weight block [W1r; W1c; Wfo_x; Wfi_x] (biases folded in) and added per edge in the epilogue of the
// per-edge GEMMs; torch.cat([x0, x]) / torch.cat([e0, e]) (mpn.py:369-373) are never materialised --
// the GEMM's A operand is read from two K segments.
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "common.h"
#include "edge_chain.h"
#include "plan.h"

namespace mpnhip {

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ------------------------------------------------------------------------------------ path counters (common.h)
static std::atomic<long long> g_path_counts[PC_COUNT];
static const char* const g_path_names[PC_COUNT] = {
    "edge_chain_fwd", "edge_chain_fwd_split", "edge_chain_bwd", "edge_chain_bwd_split", "aggregate", "aggregate_block",
    "node_step32", "node_step32_bwd", "segment_reduce", "segment_reduce_block", "segment_reduce_block3", "edge_encoder",
    "edge_encoder_bwd", "gemm_tn_mfma", "gemm_tn_small", "gemm_tn_generic", "gemm_fp32", "gemm_split", "gemm_bf16", "weight_pack", "segment_reduce3", "gemm_splitk", "edge_chain_fwd_bf16", "gemm_tn_panel", "wgrad_panel_launches", "node_chain", "wgrad_panel_fallback", "edge_chain_bwd_bf16", "node_chain_bwd", "gemm_bf16_tiled", "gemm_bf16_ring", "wgrad_rows16", "wgrad_rows16_launches", "wgrad_panel_narrow_launches", "label_overlap_lds", "label_overlap_global", "conv_tile", "conv_small_cout",
    "conv_transpose", "layer_norm", "conv_bwd_gate", "conv_wgrad", "conv_wgrad_plain", "conv_affine_tile", "conv_affine_grouped", "conv_affine_small_grid", "conv_affine_wide", "maxpool", "conv_affine_up",
    "box_predict", "nms_batched", "roi_mask_finish",
    "conv_transpose_bwd",
    "layer_norm_bwd"};
void count_path(int id) {
    if (id >= 0 && id < PC_COUNT) g_path_counts[id].fetch_add(1, std::memory_order_relaxed);
}

// ------------------------------------------------------------------------------------ event profiling
namespace {
constexpr int PROF_MAX = 2048;
struct ProfState {
    bool on = false;
    hipEvent_t ev[PROF_KINDS][PROF_MAX][2];
    double work[PROF_KINDS][PROF_MAX];
    bool made[PROF_KINDS] = {};
    int n[PROF_KINDS] = {};
    int open_kind = -1;
    bool taken = false;
    hipStream_t stream = nullptr;
    int stride = 1;        // time every stride-th launch of each kind
    int seen[PROF_KINDS] = {};
    double open_work = 0.0;
} g_prof;
}  // namespace

void prof_begin(int kind, hipStream_t s, double work) {
    if (!g_prof.on || g_prof.n[kind] >= PROF_MAX - 64) return;
    if (g_prof.seen[kind]++ % g_prof.stride != 0) return;  // sampled: the attached events are not free (~0.5 us each)
    if (!g_prof.made[kind]) {
        for (int i = 0; i < PROF_MAX; ++i) {
            (void)hipEventCreate(&g_prof.ev[kind][i][0]);
            (void)hipEventCreate(&g_prof.ev[kind][i][1]);
        }
        g_prof.made[kind] = true;
    }
    // The designated kernel's launch site picks the pair up with prof_launch_events() and hands it to
    // hipExtLaunchKernelGGL, which stamps the events with the dispatch's own begin / end times -- no record packets
    // before and after the kernel inflate a 7 us measurement.  A site that does not pick them up falls back to records.
    g_prof.open_kind = kind;
    g_prof.taken = false;
    g_prof.stream = s;
    g_prof.open_work = work;
}

bool prof_launch_events(hipEvent_t* start, hipEvent_t* stop) {
    if (!g_prof.on || g_prof.open_kind < 0 || g_prof.taken) return false;
    const int kind = g_prof.open_kind;
    *start = g_prof.ev[kind][g_prof.n[kind]][0];
    *stop = g_prof.ev[kind][g_prof.n[kind]][1];
    g_prof.taken = true;
    return true;
}

void prof_end(int kind, hipStream_t s) {
    if (!g_prof.on || g_prof.open_kind != kind || g_prof.n[kind] >= PROF_MAX - 64) return;
    if (g_prof.taken) {  // (a bracket nobody launched into is dropped)
        g_prof.work[kind][g_prof.n[kind]] = g_prof.open_work;
        g_prof.n[kind]++;
    }
    g_prof.open_kind = -1;
}

// ------------------------------------------------------------------------------------ small kernels
// dst[r][c] = src[r][c0 + c] for r < rows, c < cols  (weight sub-block copy)
__global__ void k_copy_block(const float* __restrict__ src, int64_t lds, int c0, float* __restrict__ dst, int64_t ldd,
                             int rows, int cols) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)rows * cols) return;
    int r = (int)(i / cols), c = (int)(i % cols);
    dst[(int64_t)r * ldd + c] = src[(int64_t)r * lds + c0 + c];
}

__global__ void k_copy_vec(const float* __restrict__ src, float* __restrict__ dst, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src ? src[i] : 0.f;
}

// dst[idx ? idx[r] : r][:] = src[r][:]
__global__ void k_scatter_rows(const float* __restrict__ src, const int* __restrict__ idx, float* __restrict__ dst,
                               int64_t rows, int cols) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * cols) return;
    int64_t r = i / cols;
    int c = (int)(i % cols);
    dst[(int64_t)(idx ? idx[r] : r) * cols + c] = src[i];
}

// y[r] = mean(x[r][0:hw]); `sub` lanes (power of two) share one row and reduce with shuffles
__global__ void k_avgpool(const float* __restrict__ x, int64_t rows, int hw, float* __restrict__ y, int sub) {
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t r = t / sub;
    int l = (int)(t % sub);
    float acc = 0.f;
    if (r < rows) {
        const float* p = x + r * hw;
        for (int i = l; i < hw; i += sub) acc += p[i];
    }
    for (int o = sub >> 1; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if (r < rows && l == 0) y[r] = acc / (float)hw;
}

// ------------------------------------------------------------------------------------ deferred packing (common.h)
__device__ __forceinline__ void pack_one(const PackOp& o, int64_t i) {
    const int64_t n = (int64_t)o.rows_pad * o.cols_pad;
    if (i >= n) return;
    const int r = (int)(i / o.cols_pad), c = (int)(i % o.cols_pad);
    const bool in = o.src && r < o.rows && c < o.cols;
    if (o.transposed) o.dst[i] = in ? o.src[(int64_t)c * o.lds + o.c0 + r] : 0.f;
    else o.dst[(int64_t)r * o.ldd + o.dst_c0 + c] = in ? o.src[(int64_t)r * o.lds + o.c0 + c] : 0.f;
}

// blockIdx.y = op (static indices into the by-value argument: a dynamic one would move the whole table to scratch memory)
__global__ __launch_bounds__(256) void k_pack_multi(PackBatch b) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    switch (blockIdx.y) {
#define MPN_PACK_CASE(k) case k: pack_one(b.op[k], i); break;
        MPN_PACK_CASE(0) MPN_PACK_CASE(1) MPN_PACK_CASE(2) MPN_PACK_CASE(3) MPN_PACK_CASE(4) MPN_PACK_CASE(5) MPN_PACK_CASE(6) MPN_PACK_CASE(7)
        MPN_PACK_CASE(8) MPN_PACK_CASE(9) MPN_PACK_CASE(10) MPN_PACK_CASE(11) MPN_PACK_CASE(12) MPN_PACK_CASE(13) MPN_PACK_CASE(14) MPN_PACK_CASE(15)
        MPN_PACK_CASE(16) MPN_PACK_CASE(17) MPN_PACK_CASE(18) MPN_PACK_CASE(19) MPN_PACK_CASE(20) MPN_PACK_CASE(21) MPN_PACK_CASE(22) MPN_PACK_CASE(23)
        MPN_PACK_CASE(24) MPN_PACK_CASE(25) MPN_PACK_CASE(26) MPN_PACK_CASE(27) MPN_PACK_CASE(28) MPN_PACK_CASE(29) MPN_PACK_CASE(30) MPN_PACK_CASE(31)
#undef MPN_PACK_CASE
        default: break;
    }
}

bool pack_batch_add(PackBatch* b, const PackOp& op) {
    if (!b || b->n >= PackBatch::MAX) return false;
    if ((int64_t)op.rows_pad * op.cols_pad > 0) b->op[b->n++] = op;
    return true;
}

int pack_batch_flush(const PackBatch* b, hipStream_t s) {
    if (b->n == 0) return MPNHIP_OK;
    int64_t mx = 0;
    for (int i = 0; i < b->n; ++i) {
        const int64_t n = (int64_t)b->op[i].rows_pad * b->op[i].cols_pad;
        mx = n > mx ? n : mx;
    }
    hipLaunchKernelGGL(k_pack_multi, dim3((unsigned)((mx + 255) / 256), b->n), dim3(256), 0, s, *b);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}

static int copy_block(const float* src, int64_t lds, int c0, float* dst, int64_t ldd, int rows, int cols, PackBatch* batch, hipStream_t s) {
    int64_t n = (int64_t)rows * cols;
    if (n <= 0) return MPNHIP_OK;
    if (pack_batch_add(batch, {src, dst, lds, c0, rows, cols, rows, cols, (int)ldd, 0, 0})) return MPNHIP_OK;
    hipLaunchKernelGGL(k_copy_block, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, lds, c0, dst, ldd, rows, cols);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}
static int copy_vec(const float* src, float* dst, int n, PackBatch* batch, hipStream_t s) {
    if (n <= 0) return MPNHIP_OK;
    if (pack_batch_add(batch, {src, dst, n, 0, 1, n, 1, n, n, 0, 0})) return MPNHIP_OK;
    hipLaunchKernelGGL(k_copy_vec, dim3((n + 255) / 256), dim3(256), 0, s, src, dst, n);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}
static int scatter_rows(const float* src, const int* idx, float* dst, int64_t rows, int cols, hipStream_t s) {
    int64_t n = rows * cols;
    if (n <= 0) return MPNHIP_OK;
    hipLaunchKernelGGL(k_scatter_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, idx, dst, rows, cols);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}

// ------------------------------------------------------------------------------------ building blocks

// hidden / output layers i >= 1 of an MLP on [rows, :] activations; `two` = direction-grouped run
// of the flow MLPs (group 0: flow_out weights on rows [0, E_out), group 1: flow_in on [E_out, E_out+E_in)).
static int mlp_tail(const mpnhip_mlp& m0, const mpnhip_mlp* m1, const GraphView* g, float* const* hidden,
                    float* out_last, int64_t ld_last, const int* c_idx_last, int64_t rows, int prec, hipStream_t s) {
    for (int i = 1; i < m0.n_layers; ++i) {
        GemmArgs a = {};
        a.ngroups = m1 ? 2 : 1;
        a.N = m0.out_dims[i];
        a.K = m0.out_dims[i - 1];
        a.ksplit = a.K;
        a.relu = m0.out_dims[i] != 1;  // mlp.py:17
        a.m_upper = rows;
        bool last = i == m0.n_layers - 1;
        for (int q = 0; q < a.ngroups; ++q) {
            const mpnhip_mlp& m = q == 0 ? m0 : *m1;
            GemmGroup& G = a.g[q];
            init_group(G);
            G.A = hidden[i - 1];
            G.lda = a.K;
            G.B = m.weight[i];
            G.ldb = a.K;
            G.bias = m.bias[i];
            G.C = last ? out_last : hidden[i];
            G.ldc = last ? ld_last : a.N;
            G.c_idx = last ? c_idx_last : nullptr;
            G.m_static = rows;
            if (m1) {
                G.row_begin = q == 0 ? nullptr : g->header + 4;
                G.row_end = q == 0 ? g->header + 4 : g->header + 5;
            }
        }
        MPN_TRY(launch_gemm(a, A_KCONTIG, B_KCONTIG, prec, s));
    }
    return MPNHIP_OK;
}

static int pack_node_weights(const mpnhip_model& m, const Dims& d, float* Wnode, float* bnode, PackBatch* batch, hipStream_t s) {
    const int he = d.he, hn = d.hn, kx = d.kx;
    MPN_TRY(copy_block(m.edge.weight[0], m.edge.in_dim, 0, Wnode, kx, he, kx, batch, s));                         // W1 row part
    MPN_TRY(copy_block(m.edge.weight[0], m.edge.in_dim, kx, Wnode + (size_t)he * kx, kx, he, kx, batch, s));      // W1 col part
    MPN_TRY(copy_block(m.flow_out.weight[0], m.flow_out.in_dim, 0, Wnode + (size_t)2 * he * kx, kx, hn, kx, batch, s));
    MPN_TRY(copy_block(m.flow_in.weight[0], m.flow_in.in_dim, 0, Wnode + (size_t)(2 * he + hn) * kx, kx, hn, kx, batch, s));
    MPN_TRY(copy_vec(m.edge.bias[0], bnode, he, batch, s));
    MPN_TRY(copy_vec(nullptr, bnode + he, he, batch, s));
    MPN_TRY(copy_vec(m.flow_out.bias[0], bnode + 2 * he, hn, batch, s));
    MPN_TRY(copy_vec(m.flow_in.bias[0], bnode + 2 * he + hn, hn, batch, s));
    return MPNHIP_OK;
}

static int pack_chain_weights(const mpnhip_model& m, const Dims& d, const ChainWeights& cw, bool split, PackBatch* batch, SplitBatch* split_batch, hipStream_t s) {
    const float* f0[2] = {m.flow_out.weight[0], m.flow_in.weight[0]};
    const float* f1[2] = {m.flow_out.weight[1], m.flow_in.weight[1]};
    return pack_edge_chain(m.edge.weight[0], m.edge.in_dim, 2 * d.kx, d.ke, m.edge.weight[1], m.classifier.weight[0], f0, m.flow_out.in_dim, d.kx,
                           f1, d.he, d.de, d.hn, d.dn, m.classifier.out_dims[0], cw, split, batch, split_batch, s);
}

// Q0 = e0 W1[:, e0 columns]^T, [E, he]: the re-attached initial edge features' share of the edge MLP's first layer, the same in every
// step (ForwardRun::hoist_edge_share; mpnhip_debug_edge_chain_forward)
static int edge_share_q0(const mpnhip_model& m, const Dims& d, const float* e0, float* Q0, int64_t E, int prec, hipStream_t s) {
    GemmArgs a = {};
    a.ngroups = 1; a.N = d.he; a.K = d.de; a.ksplit = d.de; a.m_upper = E;
    GemmGroup& G = a.g[0];
    init_group(G);
    G.A = e0; G.lda = d.de; G.B = m.edge.weight[0] + 2 * d.kx; G.ldb = m.edge.in_dim; G.C = Q0; G.ldc = d.he; G.m_static = E;
    return launch_gemm(a, A_KCONTIG, B_KCONTIG, prec, s);
}

// What one launch of the fp32 / split forward chain kernel reads and writes besides the model and the graph: [ea | eb] the first
// layer's input segments (eb == nullptr: ea alone, all ke columns), the saves all four or none
struct ChainFwdIO {
    const float* ea; int64_t ldea; int kea; const float* eb; int64_t ldeb;
    const float* P;
    float* e_new; float* msg; float* logits;
    float* save_h1; float* save_hc; float* save_hf; unsigned* save_mask;
};
// The kernel's arguments for one step (ForwardRun::edge_side_chain; mpnhip_debug_edge_chain_forward).  Q0 (or nullptr): ea = the
// re-attached initial edge features, whose product with W1's e0 columns is Q0 -- the kernel multiplies the current features only
// (rows kea .. of the [k][n] weight image)
static EdgeChainArgs chain_fwd_args(const mpnhip_model& m, const Dims& d, const GraphView& g, int64_t N, int64_t E, const ChainWeights& cw,
                                    bool split, const float* Q0, const ChainFwdIO& io) {
    EdgeChainArgs a = {};
    a.E = (int)E; a.N = (int)N; a.header = g.header; a.srow = g.srow; a.scol = g.scol; a.perm = g.perm; a.split = split ? 1 : 0;
    a.he = d.he; a.de = d.de; a.hn = d.hn; a.dn = d.dn; a.hc = m.classifier.out_dims[0];
    a.xa = io.ea; a.ldxa = io.ldea; a.k1a = io.eb ? io.kea : d.ke;
    a.xb = io.eb; a.ldxb = io.ldeb; a.k1b = io.eb ? d.ke - io.kea : 0;
    a.P = io.P; a.pw = d.pw;
    a.w1T = cw.w1T; a.w2T = cw.w2T; a.b2 = m.edge.bias[1];
    if (Q0) {
        a.Q0 = Q0;
        a.xa = io.eb; a.ldxa = io.ldeb; a.k1a = d.ke - io.kea;
        a.xb = nullptr; a.ldxb = 0; a.k1b = 0;
        a.w1T = cw.w1T + chain_row_off(io.kea, pad32(d.he), split);
    }
    a.wc1T = cw.wc1T; a.bc1 = m.classifier.bias[0]; a.wc2 = m.classifier.weight[1]; a.bc2 = m.classifier.bias[1];
    a.wf1T_out = cw.wf1T[0]; a.wf1T_in = cw.wf1T[1]; a.wf2T_out = cw.wf2T[0]; a.wf2T_in = cw.wf2T[1];
    a.bf2_out = m.flow_out.bias[1]; a.bf2_in = m.flow_in.bias[1];
    a.e_new = io.e_new; a.msg = io.msg; a.logits = io.logits;
    a.save_h1 = io.save_h1; a.save_hc = io.save_hc; a.save_hf = io.save_hf; a.save_mask = io.save_mask;
    return a;
}

static int pack_chain_bf16_weights(const mpnhip_model& m, const Dims& d, const ChainBf16& cb, hipStream_t s) {
    const float* f0[2] = {m.flow_out.weight[0], m.flow_in.weight[0]};
    const float* f1[2] = {m.flow_out.weight[1], m.flow_in.weight[1]};
    return pack_chain_bf16(m.edge.weight[0], m.edge.in_dim, 2 * d.kx, d.ef, m.edge.weight[1], m.classifier.weight[0], f0, m.flow_out.in_dim,
                           d.kx, f1, d.he, d.de, d.hn, d.dn, m.classifier.out_dims[0], cb.img, s);
}

// What one launch of the bf16-operand forward chain kernel reads and writes besides the model and the graph: the first-layer input
// [ea | eb] as fp32 rows or (ea16 / eb16) as bf16 rows; the saves all four or none; agg_out: the kernel aggregates (msg is not written)
struct ChainBf16FwdIO {
    const float* ea; int64_t ldea; const float* eb; int64_t ldeb;
    const unsigned short* ea16; const unsigned short* eb16;
    const float* P;
    float* e_new; unsigned short* e16_out; float* msg; float* logits;
    unsigned short* save_h1; unsigned short* save_hc; unsigned short* save_hf; unsigned* save_mask;
    float* agg_out; float* piece; int* start_row;
    int plain_barriers;
};
// The kernel's arguments for one step (ForwardRun::edge_side_bf16; mpnhip_debug_edge_chain_bf16_forward)
static EdgeChainBf16Args chain_bf16_fwd_args(const mpnhip_model& m, const Dims& d, const GraphView& g, int64_t N, int64_t E, const ChainBf16& cb,
                                             const ChainBf16FwdIO& io) {
    EdgeChainBf16Args a = {};
    a.E = (int)E; a.N = (int)N; a.header = g.header; a.srow = g.srow; a.scol = g.scol; a.perm = g.perm;
    a.he = d.he; a.de = d.de; a.hn = d.hn; a.dn = d.dn; a.hc = m.classifier.out_dims[0];
    a.xa = io.ea; a.ldxa = io.ldea; a.xb = io.eb; a.ldxb = io.ldeb;
    a.P = io.P; a.pw = d.pw;
    a.img_edge = cb.img; a.img_cls = cb.img + cb.off_cls; a.img_flow[0] = cb.img + cb.off_flow[0]; a.img_flow[1] = cb.img + cb.off_flow[1];
    a.b2 = m.edge.bias[1]; a.bc1 = m.classifier.bias[0]; a.wc2 = m.classifier.weight[1]; a.bc2 = m.classifier.bias[1];
    a.bf2_out = m.flow_out.bias[1]; a.bf2_in = m.flow_in.bias[1];
    a.e_new = io.e_new; a.msg = io.msg; a.logits = io.logits;
    a.xa16 = io.ea16; a.xb16 = io.eb16; a.e16_out = io.e16_out;
    if (io.save_mask) { a.save_h1 = io.save_h1; a.save_hc = io.save_hc; a.save_hf = io.save_hf; a.save_eb = io.e16_out; a.save_mask = io.save_mask; }
    if (io.agg_out) { a.seg_ptr = g.seg_ptr; a.agg_out = io.agg_out; a.piece = io.piece; a.start_row = io.start_row; a.agg = m.agg; }
    a.plain_barriers = io.plain_barriers;
    return a;
}

// Reference widths, few nodes: the hoisted projections P0 = x0 Wnode[:, :dn]^T + bnode AND the first step's P = P0 + x0 Wnode[:, dn:]^T
// (x_0 IS the re-attached x0 there) in one launch, one thread per output -- two 5 us GEMM launches for 140 x 272 outputs otherwise.
__global__ __launch_bounds__(256) void k_proj_hoist32(const float* __restrict__ x0, const float* __restrict__ Wnode,
                                                     const float* __restrict__ bnode, float* __restrict__ P0, float* __restrict__ P,
                                                     int64_t total, int pw, int dn) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t n = i / pw;
    const int p = (int)(i - n * pw);
    const float* w = Wnode + (int64_t)p * 2 * dn;
    const float* x = x0 + n * dn;
    float s0 = bnode[p], s1 = 0.f;
    for (int k = 0; k < dn; k += 4) {
        const float4 xv = *reinterpret_cast<const float4*>(x + k);
        const float4 wa = *reinterpret_cast<const float4*>(w + k);
        const float4 wb = *reinterpret_cast<const float4*>(w + dn + k);
        s0 = fmaf(xv.x, wa.x, s0); s0 = fmaf(xv.y, wa.y, s0); s0 = fmaf(xv.z, wa.z, s0); s0 = fmaf(xv.w, wa.w, s0);
        s1 = fmaf(xv.x, wb.x, s1); s1 = fmaf(xv.y, wb.y, s1); s1 = fmaf(xv.z, wb.z, s1); s1 = fmaf(xv.w, wb.w, s1);
    }
    P0[i] = s0;
    P[i] = s0 + s1;
}

// what one MetaLayer step reads and writes (which kernels run it is the route's matter: plan.h FwdRoute)
struct StepIO {
    // node features as one or two K segments (x0 | x) -- together kx columns
    const float* xa; int64_t ldxa; const float* xb; int64_t ldxb; int kxa;
    // edge features (e0 | e) -- together ke columns; optional row indirection (original-order input)
    const float* ea; int64_t ldea; const float* eb; int64_t ldeb; int kea; const int* e_idx;
    float* e_new; const int* e_new_idx;   // [E, de]; row scatter when the caller wants original order
    const int* e_new_read_idx;            // how the flow MLPs must index e_new (nullptr = sorted order)
    float* x_new;                         // [N, dn]
    float* logits;                        // [E] original order, or nullptr (operator-level call)
    // FwdRoute::rows16 (gemm_bf16.hip reads bf16 rows): mirrors of xa / xb, and where the mirror of x_new goes
    const unsigned short* xa16; const unsigned short* xb16; unsigned short* x_new16;
    // FwdRoute::e16_on (FwdPlan::eb_hist): mirrors of ea / eb, and where the mirror of e_new goes
    const unsigned short* ea16; const unsigned short* eb16; unsigned short* e_new16;
};

// ---- the reference's edge encoder (6 -> 18 -> 18 -> 16, ReLU after every layer; tracking_cfg.yaml:136-139) in one launch ----
// Three Linear layers this narrow are three launches of the any-shape GEMM kernel (one thread per OUTPUT element, ~25 us each at
// 78k edges): here one thread carries one edge through all three layers (720 FMAs), the weights sit in LDS and are read as
// broadcasts, the hidden activations stay in registers (written out only when the backward pass needs them).
template <int IN, int H1, int H2, int OUT>
__global__ __launch_bounds__(256) void k_edge_encoder(const float* __restrict__ x, const int* __restrict__ idx, int64_t rows,
                                                      const float* __restrict__ w0, const float* __restrict__ b0,
                                                      const float* __restrict__ w1, const float* __restrict__ b1,
                                                      const float* __restrict__ w2, const float* __restrict__ b2,
                                                      float* __restrict__ h1_out, float* __restrict__ h2_out, float* __restrict__ y) {
    __shared__ float sw0[H1 * IN], sb0[H1], sw1[H2 * H1], sb1[H2], sw2[OUT * H2], sb2[OUT];
    for (int i = threadIdx.x; i < H1 * IN; i += 256) sw0[i] = w0[i];
    for (int i = threadIdx.x; i < H2 * H1; i += 256) sw1[i] = w1[i];
    for (int i = threadIdx.x; i < OUT * H2; i += 256) sw2[i] = w2[i];
    if (threadIdx.x < H1) sb0[threadIdx.x] = b0[threadIdx.x];
    if (threadIdx.x < H2) sb1[threadIdx.x] = b1[threadIdx.x];
    if (threadIdx.x < OUT) sb2[threadIdx.x] = b2[threadIdx.x];
    __syncthreads();
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const float* xr = x + (int64_t)(idx ? idx[r] : r) * IN;
    float a[IN], h1[H1], h2[H2];
#pragma unroll
    for (int k = 0; k < IN; ++k) a[k] = xr[k];
#pragma unroll
    for (int o = 0; o < H1; ++o) {
        float s = sb0[o];
#pragma unroll
        for (int k = 0; k < IN; ++k) s = fmaf(a[k], sw0[o * IN + k], s);
        h1[o] = fmaxf(s, 0.f);
    }
#pragma unroll
    for (int o = 0; o < H2; ++o) {
        float s = sb1[o];
#pragma unroll
        for (int k = 0; k < H1; ++k) s = fmaf(h1[k], sw1[o * H1 + k], s);
        h2[o] = fmaxf(s, 0.f);
    }
    if (h1_out) {
#pragma unroll
        for (int o = 0; o < H1; ++o) h1_out[r * H1 + o] = h1[o];
#pragma unroll
        for (int o = 0; o < H2; ++o) h2_out[r * H2 + o] = h2[o];
    }
#pragma unroll
    for (int o = 0; o < OUT; ++o) {
        float s = sb2[o];
#pragma unroll
        for (int k = 0; k < H2; ++k) s = fmaf(h2[k], sw2[o * H2 + k], s);
        y[r * OUT + o] = fmaxf(s, 0.f);
    }
}

// (tried where FwdRoute::enc_fused holds)  true (and launched) when `m` is exactly that encoder; hidden[0..1] = where the backward wants the activations, or nullptr
static bool edge_encoder_fused(const mpnhip_mlp& m, const float* x, const int* idx, float* const* hidden, bool keep_hidden, float* y,
                               int64_t rows, hipStream_t s, int* status) {
    *status = MPNHIP_OK;
    if (m.n_layers == 3 && rows > 0 && !(m.in_dim == 6 && m.out_dims[0] == 18 && m.out_dims[1] == 18 && m.out_dims[2] == 16)) {
        // the wider models' encoder (e.g. 6 -> 72 -> 72 -> 64 at d = 128): the MFMA form (edge_chain.hip, k_edge_encoder_mfma)
        const float* w[3] = {m.weight[0], m.weight[1], m.weight[2]};
        const float* b[3] = {m.bias[0], m.bias[1], m.bias[2]};
        const int dims[3] = {m.out_dims[0], m.out_dims[1], m.out_dims[2]};
        const int r = launch_edge_encoder_mfma(x, idx, rows, m.in_dim, w, b, dims, keep_hidden ? hidden[0] : nullptr, keep_hidden ? hidden[1] : nullptr, y, s);
        if (r < 0) *status = r;
        if (r != 0) count_path(PC_EDGE_ENCODER);
        return r != 0;
    }
    if (m.n_layers != 3 || m.in_dim != 6 || m.out_dims[0] != 18 || m.out_dims[1] != 18 || m.out_dims[2] != 16 || rows <= 0) return false;
    count_path(PC_EDGE_ENCODER);
    hipLaunchKernelGGL((k_edge_encoder<6, 18, 18, 16>), dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, x, idx, rows, m.weight[0],
                       m.bias[0], m.weight[1], m.bias[1], m.weight[2], m.bias[2], keep_hidden ? hidden[0] : nullptr,
                       keep_hidden ? hidden[1] : nullptr, y);
    if (hipGetLastError() != hipSuccess) { set_error("edge encoder: launch failed"); *status = MPNHIP_ERR_HIP; }
    return true;
}

// full MLP (all layers) with ping-pong or per-layer hidden buffers; a_idx permutes the input rows
static int mlp_forward(const mpnhip_mlp& m, const float* x, int64_t ldx, const int* a_idx, float* const* hidden, float* y,
                       int64_t rows, int prec, hipStream_t s, float* splitk = nullptr, size_t splitk_floats = 0) {
    for (int i = 0; i < m.n_layers; ++i) {
        if (splitk && !a_idx) {
            int st = MPNHIP_OK;
            const int k_in = layer_in(m, i);
            // (the layer after it rides along when it is the MLP's last and narrow: the reference's 2048 -> 128 -> 32 node encoder)
            SplitkNext nx = {};
            const bool has_next = i + 2 == m.n_layers;
            if (has_next) nx = {m.weight[i + 1], m.bias[i + 1], m.out_dims[i + 1], m.out_dims[i + 1] != 1, y, m.out_dims[i + 1], false};
            if (linear_splitk(i == 0 ? x : hidden[i - 1], i == 0 ? ldx : k_in, m.weight[i], m.bias[i], i == m.n_layers - 1 ? y : hidden[i],
                              m.out_dims[i], rows, m.out_dims[i], k_in, m.out_dims[i] != 1, prec, splitk, splitk_floats, s, &st,
                              has_next ? &nx : nullptr)) {
                if (st != MPNHIP_OK) return st;
                if (nx.done) ++i;   // both layers are evaluated
                continue;
            }
        }
        GemmArgs a = {};
        a.ngroups = 1;
        a.N = m.out_dims[i];
        a.K = layer_in(m, i);
        a.ksplit = a.K;
        a.relu = m.out_dims[i] != 1;
        a.m_upper = rows;
        GemmGroup& G = a.g[0];
        init_group(G);
        G.A = i == 0 ? x : hidden[i - 1];
        G.lda = i == 0 ? ldx : a.K;
        G.a_idx = i == 0 ? a_idx : nullptr;
        G.B = m.weight[i];
        G.ldb = a.K;
        G.bias = m.bias[i];
        G.C = i == m.n_layers - 1 ? y : hidden[i];
        G.ldc = a.N;
        G.m_static = rows;
        MPN_TRY(launch_gemm(a, A_KCONTIG, B_KCONTIG, prec, s));
    }
    return MPNHIP_OK;
}

// One mpnhip_forward call: the object lives in that call's frame (no allocation), the route (plan.h FwdRoute) is decided once in
// init(), and the phases are the methods below in the order mpnhip_forward calls them.  mpnhip_meta_layer_forward runs the same
// step code on the all-off route with the caller's row indirections.
struct ForwardRun {
    const mpnhip_model& m;
    const EnvSwitches sw;
    const hipStream_t s;
    Dims d;
    FwdPlan p;
    GraphView g;
    FwdRoute r = {};
    int prec = MPNHIP_PREC_FP32;
    int64_t N = 0, E = 0;
    float *x0 = nullptr, *e0 = nullptr;   // the encoder's outputs (x_hist[0], e_hist[0])
    size_t xs = 0, es = 0;                // floats of one [N, dn] / [E, de] block
    int prev = 0, cur = 0;   // history slots of the step's inputs / outputs: advanced by step()

    ForwardRun(const mpnhip_model& model, const EnvSwitches& switches, hipStream_t stream) : m(model), sw(switches), s(stream) {}
    ForwardRun(const ForwardRun&) = delete;
    ForwardRun& operator=(const ForwardRun&) = delete;

    // ---- checks, the plan, the route (host only: nothing is launched) -----------------------------------------------------------
    int init(const void* graph_buf, int n_nodes, int64_t n_edges, const float* x, const float* edge_attr, const float* logits, void* workspace,
             size_t workspace_bytes, int save) {
        MPN_TRY(check_full(m, &d));
        N = n_nodes; E = n_edges;
        MPN_CHECK_ARG(N >= 0 && E >= 0, "forward: negative sizes");
        MPN_CHECK_ARG((x || N == 0) && (edge_attr || E == 0) && (logits || E == 0), "forward: null tensor");
        r = fwd_route(m, d, save, sw);
        const size_t need = plan_forward(m, d, r, N, E, workspace, &p);
        MPN_CHECK_WORKSPACE("forward", workspace, workspace_bytes, need);
        graph_layout(n_nodes, n_edges, &g, const_cast<void*>(graph_buf));
        MPN_CHECK_ARG(m.precision == MPNHIP_PREC_FP32 || m.precision == MPNHIP_PREC_BF16 || m.precision == MPNHIP_PREC_FP32_SPLIT ||
                      m.precision == MPNHIP_PREC_FP32_WGSPLIT, "forward: unknown precision %d", m.precision);
        // every product of this call rounds its operands as the model asks (FP32_SPLIT: the fused chain kernels, and the larger
        // K-contiguous GEMMs -- gemm.hip; FP32_WGSPLIT differs from FP32 in the backward's weight gradients only)
        prec = m.precision == MPNHIP_PREC_FP32_WGSPLIT ? MPNHIP_PREC_FP32 : m.precision;
        x0 = p.x_hist; e0 = p.e_hist;
        xs = (size_t)N * d.dn; es = (size_t)E * d.de;
        decide();
        return MPNHIP_OK;
    }

    // the run part of the route: what needs N, E and the carved pointers
    void decide() {
        auto al = [](const void* a, const void* b = nullptr) { return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0; };
        // the node side runs over bf16 rows (plan.h: the backward applies the same test before it reads xb_hist)
        r.rows16 = node_rows16_runtime(p, m, d);
        // P0 = x0 Wnode[:, :dn]^T + bnode, once per forward, is the re-attached x0's share of every step's projections
        // (bf16 rows: the projections multiply [x0 | x] whole -- twice the MFMAs, which this product has to spare, instead of streaming
        // the [N, pw] fp32 table P0 back in every step)
        r.hoist = d.nf == 2 && d.L > 1 && !r.rows16;
        // the same for the edge side of the fused chain: Q0 = e0 W1[:, e0 columns]^T, [E, he] (64 MB at cfg-B), saves a
        // quarter of the chain's first-layer MFMAs in every step
        // (measured: pays from de = 32 up; at the reference's de = 16 the extra C-in loads cost more than the one chunk saved)
        // (FP32_SPLIT: the chain kernel is bound by its row traffic, not by MFMA cycles -- re-reading 4 he bytes per edge and step
        // costs more than the k blocks it saves: measured 1.59 -> 1.55 ms per cfg-B forward without the hoist)
        r.hoist_e = r.chain && !r.split && d.ef == 2 && d.L > 1 && E > 0 && d.de >= 32 && (d.ke - d.de) % 16 == 0 && d.de % 16 == 0;
        // The reference's node width, few nodes: ONE gate for k_proj_hoist32 and node_step32 (segment.hip: the three node-side kernels
        // of a step in one launch); both need the hoisted P0 form and 16-byte aligned images.  (Every 2-node block re-reads the 43 KB of
        // node-side weights from L2: beyond a few thousand nodes the GEMMs win again.)
        const bool node32 = r.hoist && d.dn == 32 && N > 0 && N <= 4096 && m.precision != MPNHIP_PREC_BF16 && al(p.Wnode, p.P0) && !sw.no_node_fusion;
        // each adds what its own kernel reads: k_proj_hoist32 loads x0 as float4 (kx == 2 dn follows from hoist); node_step32 loads the
        // node update's weight as float4, needs edges, and does not record the arg max a training forward with max keeps
        r.proj_small = node32 && al(x0);   // P0 AND the first step's projections in one launch
        r.fuse_node32 = node32 && !r.save_arg && d.pw % 4 == 0 && E > 0 && al(m.node.weight[0]);
        // wider models in the split precision: the same three launches as one (node_chain.hip)
        r.fuse_node_chain = !r.save_arg && r.hoist && p.nc_img && m.precision == MPNHIP_PREC_FP32_SPLIT && E > 0 && N > 0 && m.node.n_layers == 1 &&
                            al(m.node.bias[0]);
        // (training on the bf16 chain kernel: only with the bf16 saves of FwdRoute::b16; without edges no chain kernel runs, nothing mirrors)
        r.edge_bf16 = r.chain_bf16 && (!r.save || r.b16) && E > 0;   // the edge side of a step: the bf16 chain kernel,
        r.edge_chain = r.chain && E > 0;                             // the fp32 one, or (neither) one launch per product
        // the edge features travel between the steps as bf16 rows (eb_hist is planned only where edge_bf16 can hold: fwd_route)
        r.e16_on = r.eb_hist && E > 0;
        // the bf16 chain kernel aggregates the messages itself: they never reach HBM (MPNHIP_NO_AGG_FUSION=1: k_aggregate); training with
        // max keeps k_aggregate, which records the arg max.  (No fused node kernel stands beside this arm: they refuse MPNHIP_PREC_BF16.)
        r.agg_in_kernel = r.edge_bf16 && !r.save_arg && !sw.no_agg_fusion;
        // the edge encoder may run as one fused launch (bf16-operand mode: every Linear product rounds its operands -- the GEMM path
        // does that, the fused encoder is fp32)
        r.enc_fused = m.precision != MPNHIP_PREC_BF16 && !sw.no_encoder_fusion;
    }

    // ---- weight images at the head of the workspace ------------------------------------------------------------------------------
    int pack_weights() {
        if (m.weights_prepacked && !r.save) return MPNHIP_OK;   // the caller kept them from an earlier call
        count_path(PC_WEIGHT_PACK);
        PackBatch pb;   // (the fp32 images' copies / transposes are recorded and run as one launch,
        SplitBatch sb;  //  the split images as another)
        int rc = pack_node_weights(m, d, p.Wnode, p.bnode, &pb, s);
        if (rc == MPNHIP_OK && r.chain) rc = pack_chain_weights(m, d, p.cw, r.split, &pb, &sb, s);
        if (rc == MPNHIP_OK && r.chain_bf16) rc = pack_chain_bf16_weights(m, d, p.cb, s);
        const int rf = pack_batch_flush(&pb, s);
        const int rs = split_batch_flush(&sb, s);
        MPN_TRY(rc);
        MPN_TRY(rf);
        MPN_TRY(rs);
        // (after the flush: the unit images of the fused node-side kernel read the packed projection weights)
        if (p.nc_img && m.precision == MPNHIP_PREC_FP32_SPLIT)
            MPN_TRY(pack_node_chain(m.node.weight[0], p.Wnode, d.dn, d.pw, d.kx, p.nc_img, s));
        // ... and so do the bf16 images of the node-side weights (what to_bf16_rows needs; FwdRoute::rows16 adds the GEMM's conditions)
        if (p.Wnode16 && ((size_t)d.pw * d.kx) % 4 == 0 && ((size_t)d.dn * 2 * d.dn) % 4 == 0 && (((uintptr_t)m.node.weight[0]) & 15) == 0) {
            MPN_TRY(to_bf16_rows(p.Wnode, p.Wnode16, (int64_t)d.pw * d.kx, s));
            MPN_TRY(to_bf16_rows(m.node.weight[0], p.Wu16, (int64_t)d.dn * 2 * d.dn, s));
        }
        return MPNHIP_OK;
    }

    // ---- encoder (mpn.py:355 -> :164-178); the edge encoder reads edge_attr through the sort permutation: per-edge tensors are sorted
    int encode(const float* x, const float* edge_attr) {
        float* hid[MPNHIP_MAX_LAYERS];
        hidden_ptrs(m.enc_node, p.enc_n, N, r.save, hid);
        MPN_TRY(mlp_forward(m.enc_node, x, m.enc_node.in_dim, nullptr, hid, x0, N, prec, s, p.splitk, p.splitk_floats));
        hidden_ptrs(m.enc_edge, p.enc_e, E, r.save, hid);
        int st = MPNHIP_OK;
        if (!r.enc_fused || !edge_encoder_fused(m.enc_edge, edge_attr, g.perm, hid, r.save, e0, E, s, &st))
            return mlp_forward(m.enc_edge, edge_attr, m.enc_edge.in_dim, g.perm, hid, e0, E, prec, s);
        return st;
    }

    // ---- the encoder outputs as slot 0 of the bf16 mirrors ---------------------------------------------------------------------------
    int mirror_encoder_outputs() {
        if (r.e16_on && d.L > 0) MPN_TRY(to_bf16_rows(e0, p.eb_hist, (int64_t)es, s));
        if (r.rows16 && xs && d.L > 0) MPN_TRY(to_bf16_rows(x0, p.xb_hist, (int64_t)xs, s));
        return MPNHIP_OK;
    }

    // ---- P0 = x0 Wnode[:, :dn]^T + bnode, once per forward (the GEMM form; the small form: hoist_projections32) -----------------------
    int hoist_projections() {
        if (!r.hoist || r.proj_small) return MPNHIP_OK;
        GemmArgs a = {};
        a.ngroups = 1; a.N = d.pw; a.K = d.dn; a.ksplit = d.dn; a.m_upper = N;
        GemmGroup& G = a.g[0];
        init_group(G);
        G.A = x0; G.lda = d.dn; G.B = p.Wnode; G.ldb = d.kx; G.bias = p.bnode; G.C = p.P0; G.ldc = d.pw; G.m_static = N;
        return launch_gemm(a, A_KCONTIG, B_KCONTIG, prec, s);
    }

    // ---- Q0 = e0 W1[:, e0 columns]^T ---------------------------------------------------------------------------------------------------
    int hoist_edge_share() {
        if (!r.hoist_e) return MPNHIP_OK;
        return edge_share_q0(m, d, e0, p.Q0, E, prec, s);
    }

    // ---- P0 AND the first step's projections by k_proj_hoist32 (its place in the launch order: behind Q0) ------------------------------
    int hoist_projections32() {
        if (!r.proj_small) return MPNHIP_OK;
        const int64_t total = N * d.pw;
        hipLaunchKernelGGL(k_proj_hoist32, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x0, p.Wnode, p.bnode, p.P0, step_at(p, 0).P,
                           total, d.pw, d.dn);
        MPN_LAUNCH_CHECK();
        return MPNHIP_OK;
    }

    // ---- message-passing step i (0-based) between the history slots -------------------------------------------------------------------
    int step(int i, float* logits) {
        cur = r.save ? i + 1 : 1 + (i & 1);
        StepIO io = {};
        const float* xp = p.x_hist + xs * prev;
        const float* ep = p.e_hist + es * prev;
        if (d.nf == 2) { io.xa = x0; io.ldxa = d.dn; io.xb = xp; io.ldxb = d.dn; io.kxa = d.dn; }
        else { io.xa = xp; io.ldxa = d.dn; }
        if (d.ef == 2) { io.ea = e0; io.ldea = d.de; io.eb = ep; io.ldeb = d.de; io.kea = d.de; }
        else { io.ea = ep; io.ldea = d.de; }
        io.e_new = p.e_hist + es * cur;
        io.x_new = p.x_hist + xs * cur;
        io.logits = logits + (size_t)i * E;
        if (r.rows16) {
            io.xa16 = d.nf == 2 ? p.xb_hist : p.xb_hist + xs * prev;
            io.xb16 = d.nf == 2 ? p.xb_hist + xs * prev : nullptr;
            io.x_new16 = p.xb_hist + xs * cur;
        }
        // (bf16-operand chain: the edge features travel between the steps as bf16 rows; the fp32 ones only where they are returned)
        if (r.e16_on) { io.ea16 = p.eb_hist; io.eb16 = p.eb_hist + es * prev; io.e_new16 = p.eb_hist + es * cur; }
        MPN_TRY(meta_layer(io, step_at(p, i), i));
        prev = cur;
        return MPNHIP_OK;
    }

    // One MetaLayer.forward (mpn.py:33-54) (+ classifier, mpn.py:114) on prepared weights
    int meta_layer(const StepIO& io, const StepBufs& b, int i) {
        MPN_TRY(projections(io, b, i));
        if (r.edge_bf16) MPN_TRY(edge_side_bf16(io, b, i));
        else if (r.edge_chain) MPN_TRY(edge_side_chain(io, b));
        else if (E > 0) MPN_TRY(edge_side_unfused(io, b));
        return node_side(io, b, i);
    }

    // (1) per-node projections P = [xa | xb] Wnode^T + bnode
    int projections(const StepIO& io, const StepBufs& b, int i) {
        // (the previous step's fused node kernel, or k_proj_hoist32 ahead of the first step, already wrote them into b.P)
        if (((r.fuse_node32 || r.fuse_node_chain) && i > 0) || (r.proj_small && i == 0)) return MPNHIP_OK;
        GemmArgs a = {};
        a.ngroups = 1; a.N = d.pw; a.relu = 0; a.m_upper = N;
        GemmGroup& G = a.g[0];
        init_group(G);
        if (r.rows16) {
            // bf16 rows in memory, the whole K (both segments), biases in the epilogue: the LDS-DMA ring kernel
            a.K = d.kx; a.ksplit = io.xb16 ? io.kxa : d.kx;
            G.A = reinterpret_cast<const float*>(io.xa16); G.lda = io.ldxa; G.a16 = 1;
            G.A2 = reinterpret_cast<const float*>(io.xb16); G.lda2 = io.ldxb;
            G.B = reinterpret_cast<const float*>(p.Wnode16); G.ldb = d.kx; G.b16 = 1; G.bias = p.bnode;
        } else if (r.hoist) {
            // xa (the re-attached initial features) does not change from step to step: its product is P0
            a.K = d.kx - io.kxa; a.ksplit = a.K;
            G.A = io.xb; G.lda = io.ldxb;
            G.B = p.Wnode + io.kxa; G.ldb = d.kx;
            G.G1 = p.P0; G.ldg1 = d.pw;
        } else {
            a.K = d.kx; a.ksplit = io.xb ? io.kxa : d.kx;
            G.A = io.xa; G.lda = io.ldxa; G.A2 = io.xb; G.lda2 = io.ldxb;
            G.B = p.Wnode; G.ldb = d.kx; G.bias = p.bnode;
        }
        G.C = b.P; G.ldc = d.pw; G.m_static = N;
        return launch_gemm(a, A_KCONTIG, B_KCONTIG, prec, s);
    }

    // (2)-(4) fused, bf16 operands / fp32 accumulation (edge_chain_bf16.hip)
    int edge_side_bf16(const StepIO& io, const StepBufs& b, int i) {
        ChainBf16FwdIO c = {};
        c.ea = io.ea; c.ldea = io.ldea; c.eb = io.eb; c.ldeb = io.ldeb; c.P = b.P;
        c.e_new = io.e_new; c.msg = b.M; c.logits = io.logits;
        if (r.e16_on) {
            c.ea16 = io.ea16; c.eb16 = io.eb16; c.e16_out = io.e_new16;
            if (i + 1 != d.L) c.e_new = nullptr;   // (the fp32 features of the last step only: they are returned / kept)
        }
        if (r.save) {
            c.save_h1 = reinterpret_cast<unsigned short*>(b.HE[0]); c.save_hc = reinterpret_cast<unsigned short*>(b.HC[0]);
            c.save_hf = reinterpret_cast<unsigned short*>(b.HF[0]); c.e16_out = io.e_new16; c.save_mask = reinterpret_cast<unsigned*>(b.MK);
        }
        if (r.agg_in_kernel) {
            c.agg_out = b.AGG; c.piece = p.cb.piece; c.start_row = p.cb.start_row;
            MPN_HIP(hipMemsetAsync(b.AGG, 0, (size_t)N * 2 * d.dn * sizeof(float), s));   // (empty segments)
        }
        const EdgeChainBf16Args a = chain_bf16_fwd_args(m, d, g, N, E, p.cb, c);
        prof_begin(PROF_GEMM, s);
        MPN_TRY(launch_edge_chain_bf16(a, s));
        prof_end(PROF_GEMM, s);
        return MPNHIP_OK;
    }

    // (2)-(4) fused: edge MLP, classifier and both flow MLPs in one kernel (edge_chain.hip)
    int edge_side_chain(const StepIO& io, const StepBufs& b) {
        ChainFwdIO c = {};
        c.ea = io.ea; c.ldea = io.ldea; c.kea = io.kea; c.eb = io.eb; c.ldeb = io.ldeb; c.P = b.P;
        c.e_new = io.e_new; c.msg = b.M; c.logits = io.logits;
        if (r.save) { c.save_h1 = b.HE[0]; c.save_hc = b.HC[0]; c.save_hf = b.HF[0]; c.save_mask = reinterpret_cast<unsigned*>(b.MK); }
        const EdgeChainArgs a = chain_fwd_args(m, d, g, N, E, p.cw, r.split, r.hoist_e ? p.Q0 : nullptr, c);
        prof_begin(PROF_GEMM, s);
        MPN_TRY(launch_edge_chain(a, s));
        prof_end(PROF_GEMM, s);
        return MPNHIP_OK;
    }

    // (2)-(4) one launch per product
    int edge_side_unfused(const StepIO& io, const StepBufs& b) {
        const int he = d.he, hn = d.hn;
        // (2) edge MLP layer 0: relu([ea | eb] W1e^T + P_r[row] + P_c[col])      (EdgeModel, mpn.py:67-69)
        {
            GemmArgs a = {};
            a.ngroups = 1; a.N = he; a.K = d.ke; a.ksplit = io.eb ? io.kea : d.ke; a.m_upper = E;
            a.relu = he != 1;
            GemmGroup& G = a.g[0];
            init_group(G);
            G.A = io.ea; G.lda = io.ldea; G.A2 = io.eb; G.lda2 = io.ldeb; G.a_idx = io.e_idx;
            G.B = m.edge.weight[0] + 2 * d.kx; G.ldb = m.edge.in_dim;
            G.G1 = b.P; G.g1_idx = g.srow; G.ldg1 = d.pw;
            G.G2 = b.P + he; G.g2_idx = g.scol; G.ldg2 = d.pw;
            bool last = m.edge.n_layers == 1;
            G.C = last ? io.e_new : b.HE[0]; G.ldc = last ? d.de : he; G.c_idx = last ? io.e_new_idx : nullptr;
            G.m_static = E;
            prof_begin(PROF_GEMM, s);
            MPN_TRY(launch_gemm(a, A_KCONTIG, B_KCONTIG, prec, s));
            prof_end(PROF_GEMM, s);
        }
        MPN_TRY(mlp_tail(m.edge, nullptr, nullptr, b.HE, io.e_new, d.de, io.e_new_idx, E, prec, s));
        // (3) classifier on the NEW edge features (mpn.py:377 -> :114)
        if (io.logits) {
            const mpnhip_mlp& c = m.classifier;
            GemmArgs a = {};
            a.ngroups = 1; a.N = c.out_dims[0]; a.K = d.de; a.ksplit = d.de; a.relu = c.out_dims[0] != 1; a.m_upper = E;
            GemmGroup& G = a.g[0];
            init_group(G);
            G.A = io.e_new; G.lda = d.de; G.a_idx = io.e_new_read_idx; G.B = c.weight[0]; G.ldb = d.de; G.bias = c.bias[0];
            bool last = c.n_layers == 1;
            G.C = last ? io.logits : b.HC[0]; G.ldc = last ? 1 : a.N; G.c_idx = last ? g.perm : nullptr; G.m_static = E;
            MPN_TRY(launch_gemm(a, A_KCONTIG, B_KCONTIG, prec, s));
            MPN_TRY(mlp_tail(c, nullptr, nullptr, b.HC, io.logits, 1, g.perm, E, prec, s));
        }
        // (4) flow MLP layer 0, both directions in one grouped launch (TimeAwareNodeModel, mpn.py:85-94)
        {
            GemmArgs a = {};
            a.ngroups = 2; a.N = hn; a.K = d.de; a.ksplit = d.de; a.relu = hn != 1; a.m_upper = E;
            bool last = m.flow_in.n_layers == 1;
            for (int q = 0; q < 2; ++q) {
                const mpnhip_mlp& f = q == 0 ? m.flow_out : m.flow_in;
                GemmGroup& G = a.g[q];
                init_group(G);
                G.A = io.e_new; G.lda = d.de; G.a_idx = io.e_new_read_idx;
                G.B = f.weight[0] + d.kx; G.ldb = f.in_dim;
                G.G1 = b.P + 2 * he + q * hn; G.g1_idx = g.scol; G.ldg1 = d.pw;
                G.C = last ? b.M : b.HF[0]; G.ldc = last ? d.dn : hn;
                G.m_static = E;
                G.row_begin = q == 0 ? nullptr : g.header + 4;
                G.row_end = q == 0 ? g.header + 4 : g.header + 5;
            }
            MPN_TRY(launch_gemm(a, A_KCONTIG, B_KCONTIG, prec, s));
        }
        return mlp_tail(m.flow_out, &m.flow_in, &g, b.HF, b.M, d.dn, nullptr, E, prec, s);
    }

    // (5) aggregation (mpn.py:89,96) and node update (mpn.py:97-99); the fused kernels also write the NEXT step's projections
    int node_side(const StepIO& io, const StepBufs& b, int i) {
        float* const P_next = i + 1 == d.L ? nullptr : step_at(p, i + 1).P;
        if (r.fuse_node_chain) {
            size_t off_wx = 0;
            node_chain_image_shorts(d.dn, d.pw, &off_wx);
            NodeChainArgs a = {(int)N, d.dn, d.pw, m.agg, g.seg_ptr, b.M, p.nc_img, m.node.bias[0], p.nc_img + off_wx, p.P0,
                               P_next, io.x_new, r.save ? b.AGG : nullptr};
            // (profiled under the aggregation's kind: node_agg_fn runs inside this launch)
            prof_begin(PROF_AGG, s);
            const int st_nc = launch_node_chain(a, s);
            prof_end(PROF_AGG, s);
            return st_nc;
        }
        if (r.fuse_node32)
            return node_step32(g, b.M, m.agg, m.node.weight[0], m.node.bias[0], io.x_new, r.save ? b.AGG : nullptr, p.Wnode + io.kxa, d.kx,
                               p.P0, P_next, d.pw, s);
        if (!r.agg_in_kernel) {
            prof_begin(PROF_AGG, s);
            MPN_TRY(aggregate(g, b.M, d.dn, m.agg, b.AGG, r.save_arg ? b.ARG : nullptr, s));
            prof_end(PROF_AGG, s);
        }
        if (r.rows16 && N > 0) {
            // bf16 weight image; the bf16 mirror of the new node features (the next step's projections read it) leaves with the result
            GemmArgs a = {};
            a.ngroups = 1; a.N = d.dn; a.K = 2 * d.dn; a.ksplit = a.K; a.relu = 1; a.m_upper = N;
            GemmGroup& G = a.g[0];
            init_group(G);
            G.A = b.AGG; G.lda = 2 * d.dn; G.B = reinterpret_cast<const float*>(p.Wu16); G.ldb = 2 * d.dn; G.b16 = 1;
            G.bias = m.node.bias[0]; G.C = io.x_new; G.ldc = d.dn; G.C16 = io.x_new16; G.ldc16 = d.dn; G.m_static = N;
            return launch_gemm(a, A_KCONTIG, B_KCONTIG, prec, s);
        }
        return linear(b.AGG, 2 * d.dn, m.node.weight[0], m.node.bias[0], io.x_new, d.dn, N, d.dn, 2 * d.dn, 1, prec, s);
    }

    // ---- mpn.py:387-389: no message-passing step -- classify the encoder output once ---------------------------------------------------
    int classify_encoder_output(float* logits) {
        if (d.L != 0 || E <= 0) return MPNHIP_OK;
        const mpnhip_mlp& c = m.classifier;
        if (c.n_layers == 1) {
            GemmArgs a = {};
            a.ngroups = 1; a.N = 1; a.K = d.de; a.ksplit = d.de; a.relu = 0; a.m_upper = E;
            GemmGroup& G = a.g[0];
            init_group(G);
            G.A = e0; G.lda = d.de; G.B = c.weight[0]; G.ldb = d.de; G.bias = c.bias[0];
            G.C = logits; G.ldc = 1; G.c_idx = g.perm; G.m_static = E;
            return launch_gemm(a, A_KCONTIG, B_KCONTIG, prec, s);
        }
        MPN_TRY(linear(e0, d.de, c.weight[0], c.bias[0], p.step0.HC[0], c.out_dims[0], E, c.out_dims[0], d.de, c.out_dims[0] != 1, prec, s));
        return mlp_tail(c, nullptr, nullptr, p.step0.HC, logits, 1, g.perm, E, prec, s);
    }

    // ---- the final features, edges back in original order ----------------------------------------------------------------------------
    int write_outputs(float* x_out, float* e_out) {
        if (x_out && N > 0) MPN_HIP(hipMemcpyAsync(x_out, p.x_hist + xs * prev, xs * sizeof(float), hipMemcpyDeviceToDevice, s));
        if (e_out) MPN_TRY(scatter_rows(p.e_hist + es * prev, g.perm, e_out, E, d.de, s));
        return MPNHIP_OK;
    }
};

}  // namespace mpnhip

using namespace mpnhip;

extern "C" const char* mpnhip_version(void) { return "mpnhip 0.1 (gfx950)"; }
extern "C" const char* mpnhip_last_error(void) { return g_err; }

extern "C" int mpnhip_debug_counters(int64_t* counts, int capacity, int reset) {
    for (int i = 0; i < PC_COUNT; ++i) {
        if (counts && i < capacity) counts[i] = (int64_t)g_path_counts[i].load(std::memory_order_relaxed);
        if (reset) g_path_counts[i].store(0, std::memory_order_relaxed);
    }
    return PC_COUNT;
}
extern "C" const char* mpnhip_debug_counter_name(int index) { return index >= 0 && index < PC_COUNT ? g_path_names[index] : ""; }

extern "C" size_t mpnhip_forward_workspace_bytes(const mpnhip_model* model, int n_nodes, int64_t n_edges, int save) {
    Dims d;
    if (!model || check_full(*model, &d, false) != MPNHIP_OK) return 0;
    return plan_forward(*model, d, fwd_route(*model, d, save, read_switches()), n_nodes, n_edges, nullptr, nullptr);
}

extern "C" int mpnhip_forward(const mpnhip_model* model, const void* graph_buf, int n_nodes, int64_t n_edges,
                              const float* x, const float* edge_attr, float* logits, float* x_out, float* e_out,
                              void* workspace, size_t workspace_bytes, int save, void* stream_) {
    MPN_CHECK_ARG(model && graph_buf, "forward: null model / graph");
    ForwardRun run(*model, read_switches(), static_cast<hipStream_t>(stream_));
    MPN_TRY(run.init(graph_buf, n_nodes, n_edges, x, edge_attr, logits, workspace, workspace_bytes, save));
    MPN_TRY(run.pack_weights());
    MPN_TRY(run.encode(x, edge_attr));
    MPN_TRY(run.mirror_encoder_outputs());
    MPN_TRY(run.hoist_projections());
    MPN_TRY(run.hoist_edge_share());
    MPN_TRY(run.hoist_projections32());
    for (int i = 0; i < run.d.L; ++i) MPN_TRY(run.step(i, logits));
    MPN_TRY(run.classify_encoder_output(logits));   // (L == 0)
    return run.write_outputs(x_out, e_out);
}

// ------------------------------------------------------------------------------------ test instrumentation: the forward chain kernel
// (workspace of mpnhip_debug_edge_chain_forward: the weight images, then Q0)
static size_t plan_debug_chain_fwd(const Dims& d, int64_t E, void* base, ChainWeights* cw, float** Q0) {
    Carver a(base);
    ChainWeights w;
    carve_chain_weights(a, d, &w);
    float* q = a.take<float>((size_t)E * d.he);
    if (cw) *cw = w;
    if (Q0) *Q0 = q;
    return a.bytes();
}
// model and precision checks shared by the size queries and the entry: MPNHIP_OK with *d filled, or the refusal
static int debug_chain_fwd_model(const mpnhip_model* model, Dims* d) {
    MPN_CHECK_ARG(model, "debug_edge_chain_forward: null model");
    MPN_TRY(check_chain_model(*model, d));
    if (model->precision != MPNHIP_PREC_FP32 && model->precision != MPNHIP_PREC_FP32_SPLIT) {
        set_error("debug_edge_chain_forward: precision %d (the entry runs edge_chain_kernel: MPNHIP_PREC_FP32 / _FP32_SPLIT)", model->precision);
        return MPNHIP_ERR_UNSUPPORTED;
    }
    if (!edge_chain_supported(d->he, d->de, d->hn, d->dn, model->classifier.out_dims[0], d->de, d->ef == 2 ? d->de : 0)) {
        set_error("debug_edge_chain_forward: widths he %d de %d hn %d dn %d hc %d are not the kernel's", d->he, d->de, d->hn, d->dn,
                  model->classifier.out_dims[0]);
        return MPNHIP_ERR_UNSUPPORTED;
    }
    return MPNHIP_OK;
}

extern "C" size_t mpnhip_debug_edge_chain_mask_ints(const mpnhip_model* model, int64_t n_edges) {
    Dims d;
    if (n_edges < 0 || debug_chain_fwd_model(model, &d) != MPNHIP_OK) return 0;
    return chain_mask_ints(n_edges, d.he, d.de, d.hn, d.dn);
}

extern "C" size_t mpnhip_debug_edge_chain_forward_workspace_bytes(const mpnhip_model* model, int64_t n_edges) {
    Dims d;
    if (n_edges < 0 || debug_chain_fwd_model(model, &d) != MPNHIP_OK) return 0;
    return plan_debug_chain_fwd(d, n_edges, nullptr, nullptr, nullptr);
}

extern "C" int mpnhip_debug_edge_chain_forward(const mpnhip_model* model, const void* graph_buf, int n_nodes, int64_t n_edges,
                                               const mpnhip_debug_edge_chain_fwd* io, void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t s = static_cast<hipStream_t>(stream_);
    Dims d;
    MPN_TRY(debug_chain_fwd_model(model, &d));
    const mpnhip_model& m = *model;
    MPN_CHECK_ARG(graph_buf && io, "debug_edge_chain_forward: null graph / io");
    MPN_CHECK_ARG(n_nodes >= 0 && n_edges >= 0 && n_edges <= INT32_MAX, "debug_edge_chain_forward: bad sizes");
    const bool split = m.precision == MPNHIP_PREC_FP32_SPLIT;
    // (the conditions of the forward's own route, ForwardRun::decide, but for its L > 1)
    MPN_CHECK_ARG(!io->hoist_e0 || (d.ef == 2 && !split && d.de >= 32 && d.de % 16 == 0),
                  "debug_edge_chain_forward: hoist_e0 needs re-attached edge features, MPNHIP_PREC_FP32 and de >= 32, a multiple of 16");
    if (n_edges == 0) return MPNHIP_OK;
    MPN_CHECK_ARG(n_nodes > 0, "debug_edge_chain_forward: edges without nodes");
    MPN_CHECK_ARG(io->P && io->e_prev && (io->e0 || d.ef == 1) && io->e_new && io->msg && io->logits, "debug_edge_chain_forward: null tensor");
    MPN_CHECK_ARG(!io->save || (io->h1 && io->hc && io->hf && io->mask), "debug_edge_chain_forward: save without h1 / hc / hf / mask");
    MPN_CHECK_ARG(aligned16(io->P) && aligned16(io->e0) && aligned16(io->e_prev) && aligned16(io->e_new) && aligned16(io->msg) &&
                  aligned16(io->h1) && aligned16(io->hc) && aligned16(io->hf) && aligned16(workspace),
                  "debug_edge_chain_forward: the feature matrices and the workspace must be 16-byte aligned");
    MPN_CHECK_WORKSPACE("debug_edge_chain_forward", workspace, workspace_bytes, plan_debug_chain_fwd(d, n_edges, nullptr, nullptr, nullptr));
    GraphView g;
    graph_layout(n_nodes, n_edges, &g, const_cast<void*>(graph_buf));
    ChainWeights cw;
    float* Q0 = nullptr;
    plan_debug_chain_fwd(d, n_edges, workspace, &cw, &Q0);
    {
        PackBatch pb;
        SplitBatch sb;
        const int rc = pack_chain_weights(m, d, cw, split, &pb, &sb, s);
        const int rf = pack_batch_flush(&pb, s);
        const int rs = split_batch_flush(&sb, s);
        MPN_TRY(rc);
        MPN_TRY(rf);
        MPN_TRY(rs);
    }
    if (io->hoist_e0) MPN_TRY(edge_share_q0(m, d, io->e0, Q0, n_edges, MPNHIP_PREC_FP32, s));
    ChainFwdIO c = {};
    if (d.ef == 2) { c.ea = io->e0; c.ldea = d.de; c.kea = d.de; c.eb = io->e_prev; c.ldeb = d.de; }
    else { c.ea = io->e_prev; c.ldea = d.de; }
    c.P = io->P; c.e_new = io->e_new; c.msg = io->msg; c.logits = io->logits;
    if (io->save) { c.save_h1 = io->h1; c.save_hc = io->hc; c.save_hf = io->hf; c.save_mask = io->mask; }
    const EdgeChainArgs a = chain_fwd_args(m, d, g, n_nodes, n_edges, cw, split, io->hoist_e0 ? Q0 : nullptr, c);
    return launch_edge_chain(a, s);
}

// ---- ... and the bf16-operand forward chain kernel -----------------------------------------------------------------------------------
struct DebugChainBf16Plan {
    ChainBf16 cb;
    unsigned short* x16[2];                      // rows16: the first-layer input as bf16 rows
    unsigned short* e16; unsigned short* h1; unsigned short* hc; unsigned short* hf;   // raw bf16 rows the kernel writes
};
static size_t plan_debug_chain_bf16(const mpnhip_model& m, const Dims& d, int64_t E, void* base, DebugChainBf16Plan* out) {
    Carver a(base);
    DebugChainBf16Plan p = {};
    const int hc = m.classifier.out_dims[0];
    p.cb.img = a.take<char>(chain_bf16_image_bytes(d.he, d.de, d.hn, d.dn, hc, d.ef, &p.cb.off_cls, &p.cb.off_flow[0], &p.cb.off_flow[1]));
    size_t pieces = 0;
    const size_t fl = chain_bf16_agg_scratch_floats(E, d.dn, &pieces);
    p.cb.piece = a.take<float>(pieces);
    p.cb.start_row = a.take<int>(fl - pieces);
    for (int i = 0; i < 2; ++i) p.x16[i] = a.take<unsigned short>((size_t)E * d.de);
    p.e16 = a.take<unsigned short>((size_t)E * d.de);
    p.h1 = a.take<unsigned short>((size_t)E * d.he);
    p.hc = a.take<unsigned short>((size_t)E * hc);
    p.hf = a.take<unsigned short>((size_t)E * d.hn);
    if (out) *out = p;
    return a.bytes();
}
static int debug_chain_bf16_model(const mpnhip_model* model, Dims* d) {
    MPN_CHECK_ARG(model, "debug_edge_chain_bf16_forward: null model");
    MPN_TRY(check_chain_model(*model, d));
    if (model->precision != MPNHIP_PREC_BF16) {
        set_error("debug_edge_chain_bf16_forward: precision %d (the entry runs edge_chain_bf16_kernel: MPNHIP_PREC_BF16)", model->precision);
        return MPNHIP_ERR_UNSUPPORTED;
    }
    if (!edge_chain_bf16_supported(d->he, d->de, d->hn, d->dn, model->classifier.out_dims[0], d->ef)) {
        set_error("debug_edge_chain_bf16_forward: widths he %d de %d hn %d dn %d hc %d (re-attached edges: %d) are not the kernel's", d->he, d->de,
                  d->hn, d->dn, model->classifier.out_dims[0], d->ef - 1);
        return MPNHIP_ERR_UNSUPPORTED;
    }
    return MPNHIP_OK;
}

extern "C" size_t mpnhip_debug_edge_chain_bf16_mask_ints(const mpnhip_model* model, int64_t n_edges) {
    Dims d;
    if (n_edges < 0 || debug_chain_bf16_model(model, &d) != MPNHIP_OK) return 0;
    return chain_bf16_mask_ints(n_edges, d.he, d.de, d.hn, d.dn, model->classifier.out_dims[0]);
}

extern "C" size_t mpnhip_debug_edge_chain_bf16_forward_workspace_bytes(const mpnhip_model* model, int64_t n_edges) {
    Dims d;
    if (n_edges < 0 || debug_chain_bf16_model(model, &d) != MPNHIP_OK) return 0;
    return plan_debug_chain_bf16(*model, d, n_edges, nullptr, nullptr);
}

extern "C" void mpnhip_debug_edge_chain_bf16_geometry(const mpnhip_model* model, int32_t* edges_per_block, int32_t* waves_per_block) {
    Dims d;
    int epb = 0, nw = 0;
    if (debug_chain_bf16_model(model, &d) == MPNHIP_OK) chain_bf16_geometry(d.he, d.de, d.hn, d.dn, model->classifier.out_dims[0], &epb, &nw);
    if (edges_per_block) *edges_per_block = epb;
    if (waves_per_block) *waves_per_block = nw;
}

extern "C" int mpnhip_debug_edge_chain_bf16_forward(const mpnhip_model* model, const void* graph_buf, int n_nodes, int64_t n_edges,
                                                    const mpnhip_debug_edge_chain_bf16_fwd* io, void* workspace, size_t workspace_bytes,
                                                    void* stream_) {
    hipStream_t s = static_cast<hipStream_t>(stream_);
    Dims d;
    MPN_TRY(debug_chain_bf16_model(model, &d));
    const mpnhip_model& m = *model;
    const int hc = m.classifier.out_dims[0];
    MPN_CHECK_ARG(graph_buf && io, "debug_edge_chain_bf16_forward: null graph / io");
    MPN_CHECK_ARG(n_nodes >= 0 && n_edges >= 0 && n_edges <= INT32_MAX, "debug_edge_chain_bf16_forward: bad sizes");
    if (io->save && !(d.he % 8 == 0 && d.de % 8 == 0 && d.hn % 8 == 0 && d.dn % 8 == 0 && hc % 8 == 0 &&
                      edge_chain_bf16_bwd_supported(d.he, d.de, d.hn, d.dn, hc))) {
        set_error("debug_edge_chain_bf16_forward: the SAVE variant needs widths that are multiples of 8 and that the backward kernel takes");
        return MPNHIP_ERR_UNSUPPORTED;
    }
    if (io->rows16 && d.de % 8 != 0) {
        set_error("debug_edge_chain_bf16_forward: rows16 needs de a multiple of 8");
        return MPNHIP_ERR_UNSUPPORTED;
    }
    if (n_edges == 0) return MPNHIP_OK;
    MPN_CHECK_ARG(n_nodes > 0, "debug_edge_chain_bf16_forward: edges without nodes");
    MPN_CHECK_ARG(io->P && io->e0 && io->e_prev && io->e_new && io->logits && (io->fused_agg ? io->agg_out != nullptr : io->msg != nullptr),
                  "debug_edge_chain_bf16_forward: null tensor");
    MPN_CHECK_ARG(!io->save || (io->h1 && io->hc && io->hf && io->e16 && io->mask && io->dec_h1 && io->dec_e && io->dec_hc && io->dec_hf && io->dec_m),
                  "debug_edge_chain_bf16_forward: save without its buffers");
    MPN_CHECK_ARG(!io->rows16 || io->e16, "debug_edge_chain_bf16_forward: rows16 without e16");
    MPN_CHECK_ARG(aligned16(io->P) && aligned16(io->e0) && aligned16(io->e_prev) && aligned16(io->e_new) && aligned16(io->msg) &&
                  aligned16(io->agg_out) && aligned16(io->mask) && aligned16(workspace),
                  "debug_edge_chain_bf16_forward: the matrices and the workspace must be 16-byte aligned");
    MPN_CHECK_WORKSPACE("debug_edge_chain_bf16_forward", workspace, workspace_bytes, plan_debug_chain_bf16(m, d, n_edges, nullptr, nullptr));
    GraphView g;
    graph_layout(n_nodes, n_edges, &g, const_cast<void*>(graph_buf));
    DebugChainBf16Plan p;
    plan_debug_chain_bf16(m, d, n_edges, workspace, &p);
    MPN_TRY(pack_chain_bf16_weights(m, d, p.cb, s));
    ChainBf16FwdIO c = {};
    c.ea = io->e0; c.ldea = d.de; c.eb = io->e_prev; c.ldeb = d.de; c.P = io->P;
    c.e_new = io->e_new; c.msg = io->fused_agg ? nullptr : io->msg; c.logits = io->logits;
    if (io->rows16) {
        MPN_TRY(to_bf16_rows(io->e0, p.x16[0], n_edges * d.de, s));
        MPN_TRY(to_bf16_rows(io->e_prev, p.x16[1], n_edges * d.de, s));
        c.ea16 = p.x16[0]; c.eb16 = p.x16[1]; c.e16_out = p.e16;
    }
    if (io->save) { c.save_h1 = p.h1; c.save_hc = p.hc; c.save_hf = p.hf; c.e16_out = p.e16; c.save_mask = io->mask; }
    if (io->fused_agg) {
        c.agg_out = io->agg_out; c.piece = p.cb.piece; c.start_row = p.cb.start_row;
        MPN_HIP(hipMemsetAsync(io->agg_out, 0, (size_t)n_nodes * 2 * d.dn * sizeof(float), s));   // (empty segments, as the forward does)
    }
    c.plain_barriers = io->plain_barriers ? 1 : 0;
    const EdgeChainBf16Args a = chain_bf16_fwd_args(m, d, g, n_nodes, n_edges, p.cb, c);
    MPN_TRY(launch_edge_chain_bf16(a, s));
    // the bf16 rows and the decision bits, decoded with the readers of mpnhip_debug_saved (ORIGINAL edge order)
    if (c.e16_out && io->e16) MPN_TRY(chain_bf16_debug_rows(p.e16, g.perm, n_edges, d.de, io->e16, s));
    if (io->save) {
        MPN_TRY(chain_bf16_debug_rows(p.h1, g.perm, n_edges, d.he, io->h1, s));
        MPN_TRY(chain_bf16_debug_rows(p.hc, g.perm, n_edges, hc, io->hc, s));
        MPN_TRY(chain_bf16_debug_rows(p.hf, g.perm, n_edges, d.hn, io->hf, s));
        float* const dec[5] = {io->dec_h1, io->dec_e, io->dec_hc, io->dec_hf, io->dec_m};
        for (int sec = 0; sec < 5; ++sec)
            MPN_TRY(chain_bf16_debug_mask(io->mask, sec, g.header, g.perm, n_edges, d.he, d.de, d.hn, d.dn, hc, dec[sec], s));
    }
    return MPNHIP_OK;
}

// ------------------------------------------------------------------------------------ MetaLayer op
// (the part of a FwdPlan one step reads on the all-off route: the packed node weights and one block of step buffers)
static size_t plan_meta(const mpnhip_model& m, const Dims& d, int64_t N, int64_t E, void* base, FwdPlan* out) {
    Carver a(base);
    FwdPlan p = {};
    p.Wnode = a.take<float>((size_t)d.pw * d.kx);
    p.bnode = a.take<float>((size_t)d.pw);
    carve_step(a, m, d, N, E, false, false, &p.step0);
    if (out) *out = p;
    return a.bytes();
}

extern "C" size_t mpnhip_meta_layer_workspace_bytes(const mpnhip_model* model, int n_nodes, int64_t n_edges) {
    Dims d;
    if (!model || check_core(*model, &d, false) != MPNHIP_OK) return 0;
    return plan_meta(*model, d, n_nodes, n_edges, nullptr, nullptr);
}

extern "C" int mpnhip_meta_layer_forward(const mpnhip_model* model, const void* graph_buf, int n_nodes, int64_t n_edges,
                                         const float* x, const float* e, float* x_new, float* e_new, void* workspace,
                                         size_t workspace_bytes, void* stream_) {
    MPN_CHECK_ARG(model && graph_buf, "meta_layer: null model / graph");
    // the full forward's step code on the all-off route (fp32, one launch per product): the operator takes [initial | current] features
    // whole, in original edge order, so the edge side goes through row indirections no fused kernel reads
    ForwardRun run(*model, read_switches(), static_cast<hipStream_t>(stream_));
    const Dims& d = run.d;
    MPN_TRY(check_core(*model, &run.d));
    run.N = n_nodes; run.E = n_edges;
    MPN_CHECK_ARG((x && x_new) || run.N == 0, "meta_layer: null node tensors");
    MPN_CHECK_ARG((e && e_new) || run.E == 0, "meta_layer: null edge tensors");
    const size_t need = plan_meta(*model, d, run.N, run.E, workspace, &run.p);
    MPN_CHECK_WORKSPACE("meta_layer", workspace, workspace_bytes, need);
    graph_layout(n_nodes, n_edges, &run.g, const_cast<void*>(graph_buf));
    MPN_TRY(pack_node_weights(*model, d, run.p.Wnode, run.p.bnode, nullptr, run.s));
    StepIO io = {};
    io.xa = x; io.ldxa = d.kx;
    io.ea = e; io.ldea = d.ke; io.e_idx = run.g.perm;
    io.e_new = e_new; io.e_new_idx = run.g.perm; io.e_new_read_idx = run.g.perm;
    io.x_new = x_new;
    io.logits = nullptr;
    return run.meta_layer(io, run.p.step0, 0);
}

// ------------------------------------------------------------------------------------ Linear / MLP ops
extern "C" int mpnhip_linear(const float* x, int64_t ldx, const float* w, const float* b, float* y, int64_t ldy,
                             int64_t m, int n, int k, int relu, void* stream_) {
    MPN_CHECK_ARG(m >= 0 && n >= 1 && k >= 1, "linear: bad sizes");
    if (m == 0) return MPNHIP_OK;
    MPN_CHECK_ARG(x && w && y, "linear: null pointer");
    return linear(x, ldx, w, b, y, ldy, m, n, k, relu, MPNHIP_PREC_FP32, static_cast<hipStream_t>(stream_));
}

// the two ping-pong buffers of the hidden activations, [m, widest hidden layer] each
static size_t mlp_layout(const mpnhip_mlp& mlp, int64_t m, void* workspace, float* two[2]) {
    Carver c(workspace);
    const int h = max_hidden(mlp);
    for (int i = 0; i < 2; ++i) two[i] = c.take<float>((size_t)(m > 0 ? m : 1) * (h > 0 ? h : 1));
    return c.bytes();
}

extern "C" size_t mpnhip_mlp_workspace_bytes(const mpnhip_mlp* mlp, int64_t m) {
    float* two[2];
    return mlp ? mlp_layout(*mlp, m, nullptr, two) : 0;
}

extern "C" int mpnhip_mlp_forward(const mpnhip_mlp* mlp, const float* x, float* y, int64_t m, void* workspace,
                                  size_t workspace_bytes, void* stream_) {
    MPN_CHECK_ARG(mlp, "mlp_forward: null mlp");
    MPN_TRY(mlp_ok(*mlp, "mlp", true));
    if (m == 0) return MPNHIP_OK;
    MPN_CHECK_ARG(x && y && m > 0, "mlp_forward: null pointer");
    float* two[2];
    const size_t need = mlp_layout(*mlp, m, workspace, two);
    if (mlp->n_layers > 1) MPN_CHECK_WORKSPACE("mlp_forward", workspace, workspace_bytes, need);   // (one layer: no hidden activation)
    float* hid[MPNHIP_MAX_LAYERS];
    hidden_ptrs(*mlp, two, m, false, hid);
    return mlp_forward(*mlp, x, mlp->in_dim, nullptr, hid, y, m, MPNHIP_PREC_FP32, static_cast<hipStream_t>(stream_));
}

extern "C" int mpnhip_avgpool(const float* x, int64_t rows, int hw, float* y, void* stream_) {
    MPN_CHECK_ARG(rows >= 0 && hw >= 1, "avgpool: bad sizes");
    if (rows == 0) return MPNHIP_OK;
    MPN_CHECK_ARG(x && y, "avgpool: null pointer");
    int sub = 1;
    while (sub < hw && sub < 64) sub <<= 1;
    int64_t threads = rows * sub;
    hipLaunchKernelGGL(k_avgpool, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream_),
                       x, rows, hw, y, sub);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}

// ------------------------------------------------------------------------------------ test instrumentation
// argmax entries are positions in SORTED edge order (or -1): as floats holding the ORIGINAL edge id
__global__ void k_arg_to_original(const int* __restrict__ arg, const int* __restrict__ perm, float* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int j = arg[i];
    out[i] = j >= 0 ? (float)perm[j] : -1.f;
}

extern "C" int mpnhip_debug_saved(const mpnhip_model* model, const void* graph_buf, int n_nodes, int64_t n_edges,
                                  const void* fwd_workspace, size_t fwd_workspace_bytes, int what, int step, int layer, float* out,
                                  int64_t* rows_out, int* width_out, void* stream_) {
    hipStream_t s = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(model && graph_buf && fwd_workspace, "debug_saved: null argument");
    const mpnhip_model& m = *model;
    Dims d;
    MPN_TRY(check_full(m, &d));
    const int64_t N = n_nodes, E = n_edges;
    const FwdRoute r = fwd_route(m, d, 1, read_switches());   // (what was saved, and in which form, is the route's to say)
    FwdPlan p;
    const size_t need = plan_forward(m, d, r, N, E, const_cast<void*>(fwd_workspace), &p);
    // (a null buffer was refused above as a bad argument: only the size test of the macro is live here)
    MPN_CHECK_WORKSPACE_MSG("debug_saved: workspace", " (must be a save_for_backward buffer)", fwd_workspace, fwd_workspace_bytes, need);
    GraphView g;
    graph_layout(n_nodes, n_edges, &g, const_cast<void*>(graph_buf));
    const size_t xs = (size_t)N * d.dn, es = (size_t)E * d.de;
    const float* src = nullptr;
    int64_t rows = 0;
    int width = 0;
    bool per_edge = false;
    auto enc_layer = [&](const mpnhip_mlp& e, float* base, int64_t r) -> const float* {
        if (layer < 0 || layer + 1 >= e.n_layers) return nullptr;
        size_t off = 0;
        for (int i = 0; i < layer; ++i) off += (size_t)r * e.out_dims[i];
        width = e.out_dims[layer];
        return base + off;
    };
    const bool step_ok = step >= 1 && step <= d.L;
    const StepBufs b = step_ok ? step_at(p, step - 1) : p.step0;
    switch (what) {
        case MPNHIP_SAVED_ENC_NODE: src = enc_layer(m.enc_node, p.enc_n[0], N); rows = N; break;
        case MPNHIP_SAVED_ENC_EDGE: src = enc_layer(m.enc_edge, p.enc_e[0], E); rows = E; per_edge = true; break;
        case MPNHIP_SAVED_X: if (step >= 0 && step <= d.L) { src = p.x_hist + xs * step; rows = N; width = d.dn; } break;
        case MPNHIP_SAVED_E: if (step >= 0 && step <= d.L) { src = p.e_hist + es * step; rows = E; width = d.de; per_edge = true; } break;
        case MPNHIP_SAVED_EDGE_HIDDEN:
            if (step_ok && layer >= 0 && layer + 1 < m.edge.n_layers) { src = b.HE[layer]; rows = E; width = m.edge.out_dims[layer]; per_edge = true; }
            break;
        case MPNHIP_SAVED_CLS_HIDDEN:
            if (step_ok && layer >= 0 && layer + 1 < m.classifier.n_layers) { src = b.HC[layer]; rows = E; width = m.classifier.out_dims[layer]; per_edge = true; }
            break;
        case MPNHIP_SAVED_FLOW_HIDDEN:
            if (step_ok && layer >= 0 && layer + 1 < m.flow_in.n_layers) { src = b.HF[layer]; rows = E; width = m.flow_in.out_dims[layer]; per_edge = true; }
            break;
        case MPNHIP_SAVED_MSG: if (step_ok) { src = b.M; rows = E; width = d.dn; per_edge = true; } break;
        case MPNHIP_SAVED_AGG: if (step_ok) { src = b.AGG; rows = N; width = 2 * d.dn; } break;
        case MPNHIP_SAVED_ARGMAX: if (step_ok && b.ARG) { src = reinterpret_cast<const float*>(b.ARG); rows = N; width = 2 * d.dn; } break;
        default: break;
    }
    if (!src) {
        set_error("debug_saved: nothing saved for what = %d, step = %d, layer = %d", what, step, layer);
        return MPNHIP_ERR_ARG;
    }
    if (rows_out) *rows_out = rows;
    if (width_out) *width_out = width;
    if (!out || rows * width == 0) return MPNHIP_OK;
    if (r.b16 && step_ok && E > 0) {
        // bf16-operand training on the fused kernels: the hidden activations are bf16 rows (returned as floats), and for sum / mean
        // the messages themselves are never stored -- their ReLU decisions are (returned as 1.0 / 0.0: what a test reads them for)
        if (what == MPNHIP_SAVED_EDGE_HIDDEN || what == MPNHIP_SAVED_CLS_HIDDEN || what == MPNHIP_SAVED_FLOW_HIDDEN)
            return chain_bf16_debug_rows(reinterpret_cast<const unsigned short*>(src), g.perm, E, width, out, s);
        if (what == MPNHIP_SAVED_E && step >= 1 && step < d.L)   // (only the last step's fp32 features are written)
            return chain_bf16_debug_rows(p.eb_hist + es * step, g.perm, E, width, out, s);
        if (what == MPNHIP_SAVED_MSG && m.agg != MPNHIP_AGG_MAX)
            return chain_bf16_debug_mask(reinterpret_cast<const unsigned*>(b.MK), 4, g.header, g.perm, E, d.he, d.de, d.hn, d.dn,
                                         m.classifier.out_dims[0], out, s);
    }
    if (what == MPNHIP_SAVED_ARGMAX) {
        const int64_t n = rows * width;
        hipLaunchKernelGGL(k_arg_to_original, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const int*>(src), g.perm, out, n);
        MPN_LAUNCH_CHECK();
        return MPNHIP_OK;
    }
    if (per_edge) return scatter_rows(src, g.perm, out, rows, width, s);   // sorted -> original edge order
    MPN_HIP(hipMemcpyAsync(out, src, (size_t)rows * width * sizeof(float), hipMemcpyDeviceToDevice, s));
    return MPNHIP_OK;
}

extern "C" int mpnhip_edge_chain_active(const mpnhip_model* model) {
    Dims d;
    if (!model || check_full(*model, &d, false) != MPNHIP_OK) return 0;
    const FwdRoute r = fwd_route(*model, d, 0, read_switches());
    return r.chain ? 1 : (r.chain_bf16 ? 2 : 0);
}

extern "C" int mpnhip_profile_enable(int on) {
    g_prof.on = on != 0;
    g_prof.stride = on > 1 ? on : 1;
    for (int k = 0; k < PROF_KINDS; ++k) g_prof.seen[k] = g_prof.n[k] = 0;
    g_prof.open_kind = -1;
    return MPNHIP_OK;
}

extern "C" int mpnhip_profile_read_kind(int kind, float* avg_us, int* launches, double* avg_work) {
    MPN_CHECK_ARG(kind >= 0 && kind < PROF_KINDS, "profile_read_kind: kind %d", kind);
    MPN_HIP(hipDeviceSynchronize());
    double tot = 0.0, work = 0.0;
    for (int i = 0; i < g_prof.n[kind]; ++i) {
        float ms = 0.f;
        MPN_HIP(hipEventElapsedTime(&ms, g_prof.ev[kind][i][0], g_prof.ev[kind][i][1]));
        tot += ms;
        work += g_prof.work[kind][i];
    }
    const int n = g_prof.n[kind];
    if (avg_us) *avg_us = n ? (float)(tot * 1000.0 / n) : 0.f;
    if (launches) *launches = n;
    if (avg_work) *avg_work = n ? work / n : 0.0;
    g_prof.n[kind] = 0;
    return MPNHIP_OK;
}

extern "C" int mpnhip_profile_read(float* gemm_avg_us, int* gemm_launches, float* agg_avg_us, int* agg_launches,
                                   float* empty_pair_us) {
    MPN_HIP(hipDeviceSynchronize());
    if (empty_pair_us) {
        // what a begin/end event pair costs with NO kernel between them (same stream, same API calls)
        *empty_pair_us = 0.f;
        if (g_prof.made[PROF_AGG] || g_prof.made[PROF_GEMM]) {
            const int k = g_prof.made[PROF_AGG] ? PROF_AGG : PROF_GEMM;
            const int reps = 64;
            for (int i = 0; i < reps; ++i) {
                MPN_HIP(hipEventRecord(g_prof.ev[k][PROF_MAX - 1 - i][0], 0));
                MPN_HIP(hipEventRecord(g_prof.ev[k][PROF_MAX - 1 - i][1], 0));
            }
            MPN_HIP(hipDeviceSynchronize());
            double tot = 0.0;
            for (int i = 0; i < reps; ++i) {
                float ms = 0.f;
                MPN_HIP(hipEventElapsedTime(&ms, g_prof.ev[k][PROF_MAX - 1 - i][0], g_prof.ev[k][PROF_MAX - 1 - i][1]));
                tot += ms;
            }
            *empty_pair_us = (float)(tot * 1000.0 / reps);
        }
    }
    float* outs[2] = {gemm_avg_us, agg_avg_us};
    int* cnts[2] = {gemm_launches, agg_launches};
    for (int k = 0; k < 2; ++k) {
        double tot = 0.0;
        for (int i = 0; i < g_prof.n[k]; ++i) {
            float ms = 0.f;
            MPN_HIP(hipEventElapsedTime(&ms, g_prof.ev[k][i][0], g_prof.ev[k][i][1]));
            tot += ms;
        }
        if (outs[k]) *outs[k] = g_prof.n[k] ? (float)(tot * 1000.0 / g_prof.n[k]) : 0.f;
        if (cnts[k]) *cnts[k] = g_prof.n[k];
        g_prof.n[k] = 0;
    }
    return MPNHIP_OK;
}

extern "C" int mpnhip_time_linear(const float* x, const float* w, const float* b, float* y, int64_t m, int n, int k,
                                  int iters, float* avg_us, void* stream_) {
    hipStream_t s = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(x && w && y && avg_us && iters > 0, "time_linear: bad argument");
    hipEvent_t t0, t1;
    MPN_HIP(hipEventCreate(&t0));
    MPN_HIP(hipEventCreate(&t1));
    MPN_TRY(linear(x, k, w, b, y, n, m, n, k, 1, MPNHIP_PREC_FP32, s));
    MPN_HIP(hipEventRecord(t0, s));
    for (int i = 0; i < iters; ++i) MPN_TRY(linear(x, k, w, b, y, n, m, n, k, 1, MPNHIP_PREC_FP32, s));
    MPN_HIP(hipEventRecord(t1, s));
    MPN_HIP(hipEventSynchronize(t1));
    float ms = 0.f;
    MPN_HIP(hipEventElapsedTime(&ms, t0, t1));
    *avg_us = ms * 1000.f / iters;
    (void)hipEventDestroy(t0);
    (void)hipEventDestroy(t1);
    return MPNHIP_OK;
}
