// Hand-written backward pass of the MPN hot path (what torch.autograd derives for the reference's
// models/mpn.py:349-392), mirroring the forward's project-then-gather structure:
//
//   activation gradients   dH_{i-1} = (dZ_i W_i) (.) [H_{i-1} > 0]       -> gemm_kernel (B N-contiguous,
//                                                                          ReLU mask fused in the epilogue)
//   weight / bias gradients dW_i += dZ_i^T H_{i-1}, db_i += colsum(dZ_i)   -> gemm_tn_kernel (split over edges)
//   index_put_(accumulate) of the reference's x[row] / x[col] gathers      -> segmented sums over the
//       row- and col-sorted CSR lists built by graph prep (no atomics, fixed order)
//   scatter_{add,mean,max} backward                                        -> one gather kernel (k_agg_bwd)
//
// Every per-step activation was saved by the forward (288 GB of HBM: nothing is recomputed).
#include <cstdlib>
#include <mutex>

#include "backward_plan.h"
#include "common.h"
#include "edge_chain.h"
#include "plan.h"

namespace mpnhip {

// ------------------------------------------------------------------------------------ small kernels
// out = (g (+ g2)) (.) [act > 0]   (ReLU backward), float4; g2: optional second addend (the other K half of a split product)
__global__ void k_relu_mask(const float* __restrict__ g, const float* __restrict__ g2, const float* __restrict__ act,
                            float* __restrict__ out, int64_t n) {
    int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i + 3 < n) {
        float4 a = *reinterpret_cast<const float4*>(act + i), v = *reinterpret_cast<const float4*>(g + i);
        if (g2) {
            const float4 w = *reinterpret_cast<const float4*>(g2 + i);
            v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w;
        }
        v.x = a.x > 0.f ? v.x : 0.f; v.y = a.y > 0.f ? v.y : 0.f; v.z = a.z > 0.f ? v.z : 0.f; v.w = a.w > 0.f ? v.w : 0.f;
        *reinterpret_cast<float4*>(out + i) = v;
    } else {
        for (; i < n; ++i) out[i] = act[i] > 0.f ? g[i] + (g2 ? g2[i] : 0.f) : 0.f;
    }
}

// Backward of node_agg_fn followed by the ReLU of the last flow layer:
//   dZM[j][c] = [M[j][c] > 0] * dAGG[srow[j]][half(j) + c] (* 1/cnt for mean) (* [ARG == j] for max)
// j in sorted order; half = dn for flow_out rows (j < E_out), 0 for flow_in rows; self-loop rows -> 0.
// One thread per 4 columns (dn % 4 == 0) or per column.
__global__ void k_agg_bwd(const float* __restrict__ dagg, const float* __restrict__ msg, const int* __restrict__ arg,
                          const int* __restrict__ srow, const int* __restrict__ seg_ptr, const int* __restrict__ header,
                          int N, int64_t E, int dn, int agg, int has_relu, float* __restrict__ out) {
    const bool vec = (dn & 3) == 0;
    const int per = vec ? dn >> 2 : dn;
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t j = t / per;
    int c = (int)(t % per) * (vec ? 4 : 1);
    if (j >= E) return;
    const int e_out = header[1], e_in = header[2];
    const int w = vec ? 4 : 1;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (j < e_out + e_in) {
        const int dir = j < e_out ? 0 : 1;
        const int row = srow[j];
        const int64_t o = (int64_t)row * 2 * dn + (dir == 0 ? dn : 0) + c;
        float scale = 1.f;
        if (agg == MPNHIP_AGG_MEAN) {
            const int key = dir * N + row;
            const int cnt = seg_ptr[key + 1] - seg_ptr[key];
            scale = (float)(cnt > 0 ? cnt : 1);
        }
        for (int q = 0; q < w; ++q) {
            float x = dagg[o + q];
            if (agg == MPNHIP_AGG_MEAN) x = x / scale;
            else if (agg == MPNHIP_AGG_MAX) x = arg[o + q] == (int)j ? x : 0.f;
            if (has_relu) x = msg[j * dn + c + q] > 0.f ? x : 0.f;
            v[q] = x;
        }
    }
    if (vec) *reinterpret_cast<float4*>(out + j * dn + c) = make_float4(v[0], v[1], v[2], v[3]);
    else out[j * dn + c] = v[0];
}

// dst[r][c0 + c] += src[r][c]
__global__ void k_add_block(const float* __restrict__ src, int64_t lds, float* __restrict__ dst, int64_t ldd, int c0,
                            int rows, int cols) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)rows * cols) return;
    int r = (int)(i / cols), c = (int)(i % cols);
    dst[(int64_t)r * ldd + c0 + c] += src[(int64_t)r * lds + c];
}

// the same for four row blocks of one source in one launch (the packed node-projection gradient back into its layers' gradients)
struct AddParts { float* dst[4]; int64_t ldd[4]; int c0[4]; int r0[4]; int rows[4]; };
__global__ void k_add_block4(const float* __restrict__ src, int64_t lds, int cols, AddParts P) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int q = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int64_t n = (int64_t)P.rows[k] * cols;
        if (q == k && i >= n) { i -= n; q = k + 1; }
    }
    if (i >= (int64_t)P.rows[q] * cols) return;
    const int r = (int)(i / cols), c = (int)(i % cols);
    P.dst[q][(int64_t)r * P.ldd[q] + P.c0[q] + c] += src[(int64_t)(P.r0[q] + r) * lds + c];
}

// src [rows, 2d] (or [rows, d] when !two): acc[r][c] += src[r][c]; other[r][c] (=|+=) src[r][d + c]
__global__ void k_split_cat(const float* __restrict__ src, int64_t rows, int d, int two, float* __restrict__ acc,
                            float* __restrict__ other, int other_accumulate) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * d) return;
    int64_t r = i / d;
    int c = (int)(i % d);
    if (two) {
        acc[i] += src[r * 2 * d + c];
        float v = src[r * 2 * d + d + c];
        other[i] = other_accumulate ? other[i] + v : v;
    } else {
        float v = src[i];
        other[i] = other_accumulate ? other[i] + v : v;
    }
}

// out[i] = sum_b src[b * stride + i]   (n4 float4 elements, ascending b: deterministic)
__global__ void k_sum_blocks(const float* __restrict__ src, int64_t stride, int nb, int64_t n4, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    float4 acc = *reinterpret_cast<const float4*>(src + 4 * i);
    for (int b = 1; b < nb; ++b) {
        const float4 v = *reinterpret_cast<const float4*>(src + (int64_t)b * stride + 4 * i);
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    *reinterpret_cast<float4*>(out + 4 * i) = acc;
}

// out[i] = sum_b src[b * stride + i] over bf16 blocks (n8 groups of eight elements, ascending b), fp32 result; up to 12 blocks'
// 16-byte loads are in flight per lane at once (a serial chain of 8-byte loads ran at 1.9 TB/s at cfg-E)
// OUT16: the sum leaves as bf16 (RNE) -- where every consumer rounds it to bf16 as an operand anyway (the hoisted e0 share: a bf16
// GEMM's A operand and a one-piece weight-gradient product), the same values at half the bytes written and read twice
template <bool OUT16>
__global__ __launch_bounds__(256) void k_sum_blocks_bf16(const unsigned short* __restrict__ src, int64_t stride, int nb, int64_t n8,
                                                         float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n8) return;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int b0 = 0; b0 < nb; b0 += 12) {
        uint4 v[12];
#pragma unroll
        for (int u = 0; u < 12; ++u) {
            const int b = b0 + u < nb ? b0 + u : nb - 1;   // clamped, unconditional loads (summed in ascending b below)
            v[u] = *reinterpret_cast<const uint4*>(src + (int64_t)b * stride + 8 * i);
        }
#pragma unroll
        for (int u = 0; u < 12; ++u) {
            if (b0 + u < nb) {
                const unsigned w[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    acc[2 * q] += __uint_as_float(w[q] << 16);
                    acc[2 * q + 1] += __uint_as_float(w[q] & 0xffff0000u);
                }
            }
        }
    }
    if (OUT16) {
        typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
        const bf16x8 o = {(__bf16)acc[0], (__bf16)acc[1], (__bf16)acc[2], (__bf16)acc[3], (__bf16)acc[4], (__bf16)acc[5], (__bf16)acc[6], (__bf16)acc[7]};
        *reinterpret_cast<uint4*>(reinterpret_cast<unsigned short*>(out) + 8 * i) = __builtin_bit_cast(uint4, o);
    } else {
        *reinterpret_cast<float4*>(out + 8 * i) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        *reinterpret_cast<float4*>(out + 8 * i + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
    }
}

__global__ void k_bf16_to_f32(const unsigned short* __restrict__ src, float* __restrict__ dst, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = __uint_as_float((unsigned)src[i] << 16);
}

// dst[i][:] = src[idx[i]][:]
__global__ void k_gather_rows(const float* __restrict__ src, const int* __restrict__ idx, float* __restrict__ dst,
                              int64_t rows, int cols) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * cols) return;
    int64_t r = i / cols;
    int c = (int)(i % cols);
    dst[i] = src[(int64_t)idx[r] * cols + c];
}

// 16-byte zeros over two regions (grid-stride)
__global__ __launch_bounds__(256) void k_zero_pair(uint4* __restrict__ a, int64_t na, uint4* __restrict__ b, int64_t nb) {
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < na + nb; i += (int64_t)gridDim.x * 256) {
        if (i < na) a[i] = z;
        else b[i - na] = z;
    }
}

static int relu_mask(const float* g, const float* act, float* out, int64_t n, hipStream_t s, const float* g2 = nullptr) {
    if (n <= 0) return MPNHIP_OK;
    hipLaunchKernelGGL(k_relu_mask, dim3((unsigned)((n / 4 + 256) / 256)), dim3(256), 0, s, g, g2, act, out, n);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}

// ------------------------------------------------------------------------------------ side stream
// One internal stream + two events per process (one process per GPU), created on the first backward call:
// the weight-gradient products of the later steps run there, concurrently with the earlier steps' chains.
struct SideStream {
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;   // the tail batch (hoisted shares, encoder layers): beside the last group of steps, not behind it
    hipEvent_t ready = nullptr, done = nullptr, done2 = nullptr;
};
// one per device, created on first use; g_side_mu serialises the ENQUEUE phase of concurrent mpnhip_backward calls (threads /
// caller streams of one process): each call's event record -> wait pairs are then issued as a unit, and a wait refers to the
// record made just before it.  (Device work of different caller streams still overlaps; their slab buffers are per call.)
constexpr int MAX_DEVICES = 64;
static SideStream g_side_dev[MAX_DEVICES];
static std::mutex g_side_mu;

static int side_stream_ready(SideStream** out) {
    int dev = -1;
    MPN_HIP(hipGetDevice(&dev));
    MPN_CHECK_ARG(dev >= 0 && dev < MAX_DEVICES, "backward: device ordinal %d", dev);
    SideStream& ss = g_side_dev[dev];
    if (!ss.stream) {
        // lowest priority: the caller's stream carries the critical path (the step loop); when both have workgroups pending, the
        // dispatcher should place the loop's first
        int least = 0, greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
        MPN_HIP(hipStreamCreateWithPriority(&ss.stream, hipStreamNonBlocking, least));
        MPN_HIP(hipStreamCreateWithPriority(&ss.stream2, hipStreamNonBlocking, least));
        MPN_HIP(hipEventCreateWithFlags(&ss.ready, hipEventDisableTiming));
        MPN_HIP(hipEventCreateWithFlags(&ss.done, hipEventDisableTiming));
        MPN_HIP(hipEventCreateWithFlags(&ss.done2, hipEventDisableTiming));
    }
    *out = &ss;
    return MPNHIP_OK;
}

// Once work has been forked to the side stream the caller's stream must wait for it on EVERY exit path -- also when a later
// launch fails and the function returns early: the side stream still reads the forward / backward workspaces and adds into
// the gradient buffers, all of which the caller is free to release as soon as this call returns.
struct SideJoin {
    SideStream* ss = nullptr;
    hipStream_t caller = nullptr;
    bool forked = false, joined = false;
    ~SideJoin() {
        if (forked && !joined && ss) {
            if (hipEventRecord(ss->done2, ss->stream2) != hipSuccess || hipStreamWaitEvent(caller, ss->done2, 0) != hipSuccess)
                (void)hipStreamSynchronize(ss->stream2);
            if (hipEventRecord(ss->done, ss->stream) != hipSuccess || hipStreamWaitEvent(caller, ss->done, 0) != hipSuccess)
                (void)hipStreamSynchronize(ss->stream);   // last resort: block the host rather than leave the work unordered
        }
    }
};

// ------------------------------------------------------------------------------------ helpers
// (BwdPlan, plan_backward: backward_plan.h)
// (RowRange, Operand, WgProduct: common.h)
// ... two weight blocks that are KEPT transposed for the whole backward: the node update's and the per-node projections' weights are the
// operands of an activation-gradient product in every step (22 transpositions of the same two blocks per cfg-E step before round 4,
// 25 - 30 us each)
struct WtKeep { float* wt; size_t floats; bool valid; unsigned short* wt16; };
// what the helpers of one mpnhip_backward_flags call share (BackwardRun::c: built once, in init() after plan_backward; it lives in that call's frame)
struct BwdCtx {
    const BwdPlan* p;
    // a model in MPNHIP_PREC_FP32_SPLIT / _WGSPLIT / _BF16: weight gradients in the three-piece operand form (wgrad_panel.hip)
    bool wgrad_split;
    // MPNHIP_PREC_BF16 (training): every product of the backward rounds its operands to bf16 like the forward's -- the activation
    // gradients dH = dZ W through the K-contiguous bf16 GEMM (the weight block transposed into p->wt_scratch first: the kernel takes
    // nn.Linear-style [out][in] operands), the weight gradients through the row-panel kernel with ONE bf16 piece per operand
    bool bf16;
    WtKeep wt_keep[2];  // (valid only inside this call: the blocks live in this call's workspace)
};

// batch: where the product is recorded (all products of a group of steps: one product launch + one slab-sum launch); nullptr: run now,
// as a batch of its own on slab_base
static int weight_grad(const BwdCtx& c, float* slab_base, WpBatch* batch, const WgProduct& w, hipStream_t s) {
    const int rc = weight_grad_route({c.wgrad_split, c.bf16}, wg_two_group_slabs(slab_base, c.p->slab_floats_per_group), batch, w, s);
    if (rc == MPNHIP_ERR_UNSUPPORTED) set_error("backward (bf16): a product over bf16 rows [%d x %d] is not covered by the row-panel kernel", w.n_out, w.k_in);
    return rc;
}

// C = mask( A B (+ C) ) with B given as weight rows: B[k][n] = W[k * ldw + n]  (dH = dZ W)
// a16: A is bf16 rows in memory (unsigned shorts behind the pointer, lda counts them; MPNHIP_PREC_BF16 only: gemm_bf16.hip reads them)
static int act_grad(BwdCtx& c, int ngroups, const float* A, int64_t lda, const int* a_idx, const float* const W[2], int64_t ldw, int K,
                    int N, float* C, int64_t ldc, const int* c_idx, const float* mask, int64_t ldmask, int accumulate,
                    const RowRange rr[2], int64_t rows, hipStream_t s, int keep = -1, bool a16 = false) {
    GemmArgs a = {};
    a.ngroups = ngroups;
    a.N = N;
    a.K = K;
    a.ksplit = K;
    a.relu = 0;
    a.accumulate = accumulate;
    a.m_upper = rows;
    const bool bf16 = c.bf16 && rows > 0 && (size_t)ngroups * K * N <= c.p->wt_scratch_floats;
    if (c.bf16 && !bf16 && rows > 0) { set_error("backward (bf16): weight block %d x %d exceeds the transposition scratch", K, N); return MPNHIP_ERR_WORKSPACE; }
    for (int q = 0; q < ngroups; ++q) {
        GemmGroup& g = a.g[q];
        init_group(g);
        g.A = A;
        g.lda = lda;
        g.a16 = a16 ? 1 : 0;
        g.a_idx = a_idx;
        g.B = W[q];
        g.ldb = ldw;
        if (bf16) {
            // WT[n][k] = W[k][n]: the block as an nn.Linear weight of the product C = A WT^T (bf16 operands, K-contiguous)
            float* wt = c.p->wt_scratch + (size_t)q * K * N;
            WtKeep* kp = (keep >= 0 && ngroups == 1 && c.wt_keep[keep].wt && (size_t)K * N <= c.wt_keep[keep].floats) ? &c.wt_keep[keep] : nullptr;
            if (kp) wt = kp->wt;
            // (launched now, not recorded: the product below reads the block)
            if (!kp || !kp->valid) MPN_TRY(transpose_padded(W[q], ldw, 0, K, N, wt, K, N, nullptr, s));
            // the kept blocks also as bf16 rows (rounded once per backward instead of in every block of every step's product)
            // (N % 4: launch_gemm's bf16-row path needs whole 16-byte result vectors; otherwise the fp32 image on the register-staged path)
            const bool img16 = kp && kp->wt16 && K % 8 == 0 && N % 4 == 0 && ((size_t)K * N) % 4 == 0;
            if (img16 && !kp->valid) MPN_TRY(to_bf16_rows(wt, kp->wt16, (int64_t)K * N, s));
            if (kp) kp->valid = true;   // (one stream: the later steps' products are ordered behind this transposition)
            g.B = img16 ? reinterpret_cast<const float*>(kp->wt16) : wt;
            g.b16 = img16 ? 1 : 0;
            g.ldb = K;
        }
        g.C = C;
        g.ldc = ldc;
        g.c_idx = c_idx;
        g.mask = mask;
        g.ldmask = ldmask;
        g.m_static = rows;
        g.row_begin = rr ? rr[q].begin : nullptr;
        g.row_end = rr ? rr[q].end : nullptr;
    }
    if (bf16) return launch_gemm(a, A_KCONTIG, B_KCONTIG, MPNHIP_PREC_BF16, s);
    return launch_gemm(a, A_KCONTIG, B_NCONTIG, MPNHIP_PREC_FP32, s);
}

// dZ_{i-1} = (dZ_i W_i) (.) [H_{i-1} > 0] for i = n-1 .. 1.  dz[i] / hidden[i]: this step's blocks.
static int mlp_chain_backward(BwdCtx& c, const mpnhip_mlp& m0, const mpnhip_mlp* m1, float* const* dz, float* const* hidden,
                              const RowRange* rr, int64_t rows, hipStream_t s) {
    const int ng = m1 ? 2 : 1;
    for (int i = m0.n_layers - 1; i >= 1; --i) {
        const int n_out = m0.out_dims[i], k_in = m0.out_dims[i - 1];
        const float* Wq[2] = {m0.weight[i], m1 ? m1->weight[i] : nullptr};
        MPN_TRY(act_grad(c, ng, dz[i], n_out, nullptr, Wq, k_in, n_out, k_in, dz[i - 1], k_in, nullptr,
                         k_in != 1 ? hidden[i - 1] : nullptr, k_in, 0, rr, rows, s));
    }
    return MPNHIP_OK;
}

// batched weight gradients of layers >= 1 of an MLP whose dZ / hidden blocks repeat every step
static int mlp_weight_grads(const BwdCtx& c, float* slab_base, WpBatch* batch, const mpnhip_mlp& m0, const mpnhip_mlp* m1,
                            float* const* dz_all, float* const* hidden0, int64_t hidden_bstride, const RowRange* rr, int64_t rows,
                            int nbatch, hipStream_t s) {
    for (int i = m0.n_layers - 1; i >= 1; --i) {
        const int n_out = m0.out_dims[i], k_in = m0.out_dims[i - 1];
        WgProduct w = {.dZ = {dz_all[i], n_out, rows * n_out}, .H = {hidden0[i - 1], k_in, hidden_bstride}, .n_out = n_out, .k_in = k_in,
                       .ldw = k_in, .rows = rows, .nbatch = nbatch, .g = {{m0.grad_weight[i], m0.grad_bias[i], rr ? rr[0] : RowRange{}}}};
        if (m1) w.g[1] = {m1->grad_weight[i], m1->grad_bias[i], rr[1]};
        MPN_TRY(weight_grad(c, slab_base, batch, w, s));
    }
    return MPNHIP_OK;
}

// ---- the reference's edge encoder (6 -> 18 -> 18 -> 16) backwards: the three activation gradients of an edge in one thread ------
//   dz2 = dE0 (.) [e0 > 0];   dz1 = (dz2 W2) (.) [H2 > 0];   dz0 = (dz1 W1) (.) [H1 > 0]
// (instead of a ReLU-mask kernel and two launches of the any-shape GEMM kernel; the weight-gradient products read dz2 / dz1 / dz0)
template <int H1W, int H2W, int OUTW>
__global__ __launch_bounds__(256) void k_edge_encoder_bwd(const float* __restrict__ dE0, const float* __restrict__ e0,
                                                          const float* __restrict__ h2, const float* __restrict__ h1,
                                                          const float* __restrict__ w2, const float* __restrict__ w1, int64_t rows,
                                                          float* __restrict__ dz2, float* __restrict__ dz1, float* __restrict__ dz0) {
    __shared__ float sw2[OUTW * H2W], sw1[H2W * H1W];
    for (int i = threadIdx.x; i < OUTW * H2W; i += 256) sw2[i] = w2[i];
    for (int i = threadIdx.x; i < H2W * H1W; i += 256) sw1[i] = w1[i];
    __syncthreads();
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    float g2[OUTW], g1[H2W];
#pragma unroll
    for (int o = 0; o < OUTW; ++o) {
        g2[o] = e0[r * OUTW + o] > 0.f ? dE0[r * OUTW + o] : 0.f;
        dz2[r * OUTW + o] = g2[o];
    }
#pragma unroll
    for (int k = 0; k < H2W; ++k) {
        float s = 0.f;
#pragma unroll
        for (int o = 0; o < OUTW; ++o) s = fmaf(g2[o], sw2[o * H2W + k], s);
        g1[k] = h2[r * H2W + k] > 0.f ? s : 0.f;
        dz1[r * H2W + k] = g1[k];
    }
#pragma unroll
    for (int k = 0; k < H1W; ++k) {
        float s = 0.f;
#pragma unroll
        for (int o = 0; o < H2W; ++o) s = fmaf(g1[o], sw1[o * H1W + k], s);
        dz0[r * H1W + k] = h1[r * H1W + k] > 0.f ? s : 0.f;
    }
}

// bf16-operand training, deferred tail batch: the GEMM-shaped weight-gradient products of the node encoder ([1024 x 2048] over 20,000 rows
// at cfg-E: 128 output tiles of the row-panel kernel, every block walking all rows) read bf16 ROWS on the LDS-DMA kernel's 256 x 256
// tiles instead.  Their operands are fp32 blocks that stay put until the batch runs (BwdPlan::Tn, the saved hidden activations, the
// input features): the roundings are RECORDED here and launched on the tail's own stream just before its products.
struct Rows16Later {
    struct Item { const float* src; unsigned short* dst; int64_t n; };
    Item item[2 * MPNHIP_MAX_LAYERS];
    int n = 0;
    unsigned short* pool = nullptr;
    size_t pool_elems = 0, used = 0;
    unsigned short* take(const float* src, int64_t elems) {
        if (n >= 2 * MPNHIP_MAX_LAYERS || used + (size_t)elems > pool_elems || elems % 8 != 0 || (((uintptr_t)src) & 15) != 0) return nullptr;
        unsigned short* d = pool + used;
        item[n++] = {src, d, elems};
        used += (size_t)elems;
        return d;
    }
};

// one weight-gradient product of an encoder layer, recorded into the tail batch (or nullptr: run now): over bf16 rows when a
// Rows16Later is given (with the batch its roundings run ahead of) and the shape is one of the tiled ones
static int encoder_weight_grad(const BwdCtx& c, WpBatch* batch, Rows16Later* L16, const float* dz, const float* h, int n_out, int k_in,
                               float* gw, float* gb, int64_t rows, hipStream_t s) {
    WgProduct w = {.dZ = {dz, n_out, 0}, .H = {h, k_in, 0}, .n_out = n_out, .k_in = k_in, .ldw = k_in, .rows = rows, .nbatch = 1, .g = {{gw, gb}}};
    int to = 1, tc = 1;
    if (L16 && batch && (int64_t)n_out * k_in >= 65536 && r16_variant(n_out, k_in, &to, &tc) >= 16 && L16->n + 2 <= 2 * MPNHIP_MAX_LAYERS &&
        L16->used + (size_t)rows * (n_out + k_in) <= L16->pool_elems) {
        const unsigned short* z16 = L16->take(dz, rows * n_out);
        const unsigned short* h16 = z16 ? L16->take(h, rows * k_in) : nullptr;
        if (z16 && h16) {
            w.dZ.p = reinterpret_cast<const float*>(z16);
            w.H.p = reinterpret_cast<const float*>(h16);
            w.src16 = true;
        } else if (z16) {   // (the partner did not qualify: fp32 rows for both)
            --L16->n;
            L16->used -= (size_t)rows * n_out;
        }
    }
    return weight_grad(c, c.p->slab, batch, w, s);
}

// encoder-style chain with ping-pong scratch (one batch): returns dZ of layer 0 in *dz
static int mlp_tail_backward(BwdCtx& c, WpBatch* batch, Rows16Later* L16, float* const* T, const mpnhip_mlp& m0, float* const* hidden,
                             const float** dz, int* cur_buf, int64_t rows, hipStream_t s) {
    for (int i = m0.n_layers - 1; i >= 1; --i) {
        const int n_out = m0.out_dims[i], k_in = m0.out_dims[i - 1];
        MPN_TRY(encoder_weight_grad(c, batch, L16, *dz, hidden[i - 1], n_out, k_in, m0.grad_weight[i], m0.grad_bias[i], rows, s));
        const float* Wq[2] = {m0.weight[i], nullptr};
        float* dst = T[(*cur_buf + 1) % 3];
        MPN_TRY(act_grad(c, 1, *dz, n_out, nullptr, Wq, k_in, n_out, k_in, dst, k_in, nullptr,
                         k_in != 1 ? hidden[i - 1] : nullptr, k_in, 0, nullptr, rows, s));
        *cur_buf = (*cur_buf + 1) % 3;
        *dz = dst;
    }
    return MPNHIP_OK;
}

// ------------------------------------------------------------------------------------ one backward call
// bf16 rows: pointer `elems` unsigned shorts into a buffer the plans type as float*
static inline const float* u16(const float* p0, int64_t elems) {
    return reinterpret_cast<const float*>(reinterpret_cast<const unsigned short*>(p0) + elems);
}
static inline unsigned short* w16(float* p0, int64_t elems) { return reinterpret_cast<unsigned short*>(p0) + elems; }

static bool backward_forks(const mpnhip_model& m) { return m.num_enc_steps >= 4; }

// The weight images of edge_chain_bwd_kernel (caller's stream): one launch for the eight of them
int pack_chain_bwd_weights(const mpnhip_model& m, const Dims& d, const ChainBwdImages& p, bool bwd_split, hipStream_t s) {
    const float* f0[2] = {m.flow_out.weight[0], m.flow_in.weight[0]};
    const float* f1[2] = {m.flow_out.weight[1], m.flow_in.weight[1]};
    return pack_edge_chain_bwd(m.edge.weight[0], m.edge.in_dim, 2 * d.kx, d.ef, m.edge.weight[1], m.classifier.weight[0], f0, m.flow_out.in_dim,
                               d.kx, f1, d.he, d.de, d.hn, d.dn, m.classifier.out_dims[0], p, bwd_split, s);
}

// The pair images of edge_chain_bf16_bwd_kernel (caller's stream)
int pack_chain_bf16_bwd_weights(const mpnhip_model& m, const Dims& d, const ChainBf16BwdImages& im, hipStream_t s) {
    const float* f0[2] = {m.flow_out.weight[0], m.flow_in.weight[0]};
    const float* f1[2] = {m.flow_out.weight[1], m.flow_in.weight[1]};
    return pack_chain_bf16_bwd(m.edge.weight[0], m.edge.in_dim, 2 * d.kx + d.de, m.edge.weight[1], m.classifier.weight[0], f0, m.flow_out.in_dim,
                               d.kx, f1, d.he, d.de, d.hn, d.dn, m.classifier.out_dims[0], im.img, s);
}

// What one launch of a backward chain kernel reads and writes besides the model, the graph and the weight images (fp32 / split:
// dE_io in and out, dZ2 unused; bf16: dE_io is read only, the five dZ blocks are bf16 rows behind the float pointers)
struct ChainBwdIO {
    const float* dAGG; const unsigned* mask; const int* ARG; const float* dlog;
    float* dE_io; float* dZM; float* dZF; float* dZc; float* dZ2; float* dZ1; float* dE0; float* dEprev;
    int first_step, skip_e0, plain_barriers;
};
// The arguments of edge_chain_bwd_kernel for one step (BackwardRun::edge_side_chain; mpnhip_debug_edge_chain_backward)
static EdgeChainBwdArgs chain_bwd_args(const mpnhip_model& m, const Dims& d, const GraphView& g, int64_t N, int64_t E, const ChainBwdImages& im,
                                       bool split, const ChainBwdIO& io) {
    EdgeChainBwdArgs a = {};
    a.E = (int)E; a.N = (int)N; a.agg = m.agg; a.first_step = io.first_step ? 1 : 0; a.cat_two = d.ef == 2 ? 1 : 0; a.split = split ? 1 : 0;
    a.skip_e0 = io.skip_e0 ? 1 : 0;
    a.he = d.he; a.de = d.de; a.hn = d.hn; a.dn = d.dn; a.hc = m.classifier.out_dims[0];
    a.header = g.header; a.srow = g.srow; a.perm = g.perm; a.seg_ptr = g.seg_ptr;
    a.dAGG = io.dAGG; a.mask = io.mask; a.ARG = io.ARG; a.dlog = io.dlog;
    a.dE_io = io.dE_io; a.dZM = io.dZM; a.dZF = io.dZF; a.dZc = io.dZc; a.dZ1 = io.dZ1;
    a.dE0 = io.dE0; a.dEprev = io.first_step ? io.dE0 : io.dEprev;   // (the first step's e_{s-1} IS the re-attached e0)
    a.wf2_out = im.wf2p[0]; a.wf2_in = im.wf2p[1]; a.wfe_out = im.wfep[0]; a.wfe_in = im.wfep[1];
    a.wc1 = im.wc1p; a.wc2 = m.classifier.weight[1]; a.w2 = im.w2p; a.w1e = im.w1ep;
    return a;
}
// ... and of edge_chain_bf16_bwd_kernel (BackwardRun::edge_side_bf16; mpnhip_debug_edge_chain_backward in MPNHIP_PREC_BF16)
static EdgeChainBf16BwdArgs chain_bf16_bwd_args(const mpnhip_model& m, const Dims& d, const GraphView& g, int64_t N, int64_t E,
                                                const ChainBf16BwdImages& im, const ChainBwdIO& io) {
    auto r16 = [](float* q) { return reinterpret_cast<unsigned short*>(q); };
    EdgeChainBf16BwdArgs a = {};
    a.E = (int)E; a.N = (int)N; a.agg = m.agg; a.first_step = io.first_step ? 1 : 0;
    a.he = d.he; a.de = d.de; a.hn = d.hn; a.dn = d.dn; a.hc = m.classifier.out_dims[0];
    a.plain_barriers = io.plain_barriers ? 1 : 0;
    a.header = g.header; a.srow = g.srow; a.perm = g.perm; a.seg_ptr = g.seg_ptr;
    a.dAGG = io.dAGG; a.mask = io.mask; a.ARG = io.ARG; a.dlog = io.dlog;
    a.dE_in = io.dE_io;
    a.dZM = r16(io.dZM); a.dZF = r16(io.dZF); a.dZc = r16(io.dZc); a.dZ2 = r16(io.dZ2); a.dZ1 = r16(io.dZ1);
    a.dE0 = io.dE0; a.dEprev = io.dEprev;
    a.img_edge = im.img; a.img_cls = im.img + im.off_cls; a.img_flow[0] = im.img + im.off_flow[0]; a.img_flow[1] = im.img + im.off_flow[1];
    a.wc2 = m.classifier.weight[1];
    return a;
}

// One call of mpnhip_backward_flags: constructed in that call's frame, its methods are the phases of the backward in the order
// mpnhip_backward_flags calls them.  Every method returns an MPNHIP_* status; after a failure the object is only destroyed (which
// orders the caller's stream behind whatever was forked: SideJoin).
struct BackwardRun {
    // ---- what the caller gave
    const mpnhip_model& m;
    const float* const x;
    const float* const edge_attr;
    const float* const grad_logits;
    const float* const grad_x_out;
    const float* const grad_e_out;
    float* const grad_x;
    float* const grad_edge_attr;
    const int flags;
    const hipStream_t s;   // the caller's stream: the step loop, the hoisted shares' sums and the encoder chains run here
    // ---- init(): plans, widths, modes
    const EnvSwitches sw;   // read once by the entry point (tests flip the switches between calls)
    Dims d;
    FwdRoute fr;            // the route of the forward that left the saves: how to read them
    FwdPlan f;
    BwdPlan p;
    GraphView g;
    // the ONE BwdCtx of the call: act_grad flips wt_keep[].valid in it -- a copy per phase would transpose the kept blocks again
    BwdCtx c;
    int64_t N = 0, E = 0;
    int he = 0, hn = 0, dn = 0, de = 0, kx = 0, ke = 0, pw = 0, L = 0;
    size_t xs = 0, es = 0;          // floats of one [N, dn] / [E, de] block
    RowRange dir_rr[2];             // device-side row ranges of the two flow directions
    int ne = 0, nfl = 0, nc = 0;    // layers of the edge MLP, the flow MLPs, the classifier
    int64_t sstride = 0;            // floats between two steps' saved activations
    const float* x0 = nullptr;      // the encoder's outputs (x_hist[0], e_hist[0])
    const float* e0 = nullptr;
    bool use_b16 = false;       // bf16-operand training on the fused kernels (plan.h: FwdRoute::b16)
    bool use_chain = false;     // the fused fp32 edge chain (edge_chain.hip)
    bool bwd_split = false;     // ... on split images
    bool hoist_x = false;       // the re-attached x0's share of dX / gWnode: once, from the sum of the steps' dP (hoisted_shares)
    bool hoist_e0 = false;      // the same for the re-attached e0 on the edge side
    bool node16 = false;        // bf16-operand training: the node-level weight-gradient products over bf16 rows
    bool fuse_node_chain_bwd = false;   // F + the next step's A as one MFMA kernel (node_chain.hip)
    bool fuse_node_bwd = false;         // the same at the reference's node width (segment.hip, node_step32_bwd)
    size_t ncb_off_wu = 0;      // set by pack_weights: offset of the node update's units in p.ncb_img
    // ---- schedule_groups(): the side stream and the groups of steps
    SideStream* side = nullptr;
    // g_side_mu is locked (schedule_groups) before the first hipEventRecord(side->ready, ...) and held until the call returns.
    // Members are destroyed in reverse order of declaration: side_lock stands BEFORE join, so ~SideJoin runs under the lock on
    // every exit path.
    std::unique_lock<std::mutex> side_lock{g_side_mu, std::defer_lock};
    // join.forked becomes true (fork_group_if_due) BEFORE the first mp_weight_grads on the side stream: a failure inside that call
    // must still order the caller's stream behind the side stream.  join.joined: set at the join -- under tail_inline that is ahead
    // of the unpacking (flush_tail_and_unpack), and join() finds it true.
    SideJoin join;
    int gsize[3] = {0, 0, 0};   // group sizes in steps, first-finished group first
    int ngroups = 1;
    // ---- loop state
    int cx = 0;                 // p.dX[cx] holds the gradient w.r.t. x_s: flipped at the end of step(); read by node_update_bwd, projection_bwd
    int ce = 0;                 // p.dEpp[ce] holds the gradient w.r.t. e_s (bf16 chain): flipped and read by edge_side_bf16
    bool dx_split = false;      // set by projection_bwd (the gradient w.r.t. x_s arrived as two K halves, p.dX[cx] + p.dXh); read and
                                // cleared by the next step's node_update_bwd
    bool node_a_done = false;   // set by projection_bwd (its fused kernel already produced dZn / dAGG of the coming step); read and
                                // cleared by the next step's node_update_bwd
    int next_group = 0;         // the next group to fork: advanced and read by fork_group_if_due
    // ---- the tail batch (plan_tail)
    // tailb is initialised only when defer_tail holds; tail_hoist / tail_enc are null otherwise.  later16 is drained only in
    // flush_tail, on the tail's stream.
    WpBatch tailb;
    Rows16Later later16;
    bool defer_tail = false, defer_encoder = false, tail_beside = false, tail_inline = false;
    WpBatch* tail_hoist = nullptr;   // where the hoisted shares' products are recorded (nullptr: run now)
    WpBatch* tail_enc = nullptr;     // ... and the encoder's: only when the batch stays to the end
    bool unpack_pending = false;     // set by finish_message_passing (the unpacking waits for the tail batch); read by flush_tail_and_unpack

    // (model and the graph buffer are not null: mpnhip_backward_flags checks both before it constructs the object)
    BackwardRun(const mpnhip_model& model, const float* x_, const float* edge_attr_, const float* grad_logits_, const float* grad_x_out_,
                const float* grad_e_out_, float* grad_x_, float* grad_edge_attr_, int flags_, hipStream_t stream, const EnvSwitches& switches)
        : m(model), x(x_), edge_attr(edge_attr_), grad_logits(grad_logits_), grad_x_out(grad_x_out_), grad_e_out(grad_e_out_),
          grad_x(grad_x_), grad_edge_attr(grad_edge_attr_), flags(flags_), s(stream), sw(switches) {}
    BackwardRun(const BackwardRun&) = delete;
    BackwardRun& operator=(const BackwardRun&) = delete;

    // the blocks of one step (batch index b_ = step - 1) in the forward's saves and in the kept dZ arrays
    struct StepView {
        int step, b_;
        StepBufs b;
        const float* x_s;
        const float* e_s;
        float* dZn;
        float* dP;
        float* dzfl[MPNHIP_MAX_LAYERS];
        float* dzed[MPNHIP_MAX_LAYERS];
        float* dzcl[MPNHIP_MAX_LAYERS];
        float* dEc;   // gradient w.r.t. e_s (seeded by the later step / the caller)
    };

    // ---- checks, both plans, the modes (host only: nothing is launched) --------------------------------------------------------
    int init(const void* graph_buf, int n_nodes, int64_t n_edges, void* fwd_workspace, size_t fwd_workspace_bytes, void* bwd_workspace,
             size_t bwd_workspace_bytes) {
        MPN_TRY(check_full(m, &d));
        N = n_nodes;
        E = n_edges;
        MPN_CHECK_ARG(N >= 0 && E >= 0, "backward: negative sizes");
        MPN_CHECK_ARG((x || N == 0) && (edge_attr || E == 0) && (grad_logits || E == 0), "backward: null tensor");
        {
            const mpnhip_mlp* all[] = {&m.enc_node, &m.enc_edge, &m.edge, &m.flow_in, &m.flow_out, &m.node, &m.classifier};
            for (const mpnhip_mlp* q : all)
                for (int i = 0; i < q->n_layers; ++i)
                    MPN_CHECK_ARG(q->grad_weight[i] && q->grad_bias[i], "backward: null gradient buffer");
        }
        fr = fwd_route(m, d, 1, sw);
        const size_t fneed = plan_forward(m, d, fr, N, E, fwd_workspace, &f);
        MPN_CHECK_WORKSPACE_MSG("backward: forward workspace", " (must be the save_for_backward buffer)", fwd_workspace, fwd_workspace_bytes, fneed);
        const size_t need = plan_backward(m, d, fr, N, E, bwd_workspace, &p);
        MPN_CHECK_WORKSPACE("backward", bwd_workspace, bwd_workspace_bytes, need);
        c = {&p, m.precision == MPNHIP_PREC_FP32_SPLIT || m.precision == MPNHIP_PREC_FP32_WGSPLIT || m.precision == MPNHIP_PREC_BF16,
             m.precision == MPNHIP_PREC_BF16, {}};
        for (int i = 0; i < 2; ++i) c.wt_keep[i] = {p.wt_keep_floats[i] ? p.wt_keep[i] : nullptr, p.wt_keep_floats[i], false, p.wt_keep_floats[i] ? p.wt_keep16[i] : nullptr};
        graph_layout(n_nodes, n_edges, &g, const_cast<void*>(graph_buf));
        he = d.he; hn = d.hn; dn = d.dn; de = d.de; kx = d.kx; ke = d.ke; pw = d.pw; L = d.L;
        xs = (size_t)N * dn;
        es = (size_t)E * de;
        dir_rr[0] = {nullptr, g.header + 4};
        dir_rr[1] = {g.header + 4, g.header + 5};
        ne = m.edge.n_layers;
        nfl = m.flow_in.n_layers;
        nc = m.classifier.n_layers;
        sstride = (int64_t)(f.step_stride_bytes / sizeof(float));
        x0 = f.x_hist;
        e0 = f.e_hist;
        use_b16 = fr.b16 && E > 0 && L > 0;
        use_chain = fr.chain && E > 0 && L > 0;
        bwd_split = use_chain && fr.split;
        // The re-attached x0 does not change from step to step: its share of dX (and of the packed projection weight's gradient)
        // comes from the SUM of the steps' dP, once, after the loop
        hoist_x = d.nf == 2 && L > 1 && N > 0 && pw % 4 == 0 && dn % 4 == 0;
        // The same for the re-attached e0 on the edge side (fused chain, whole 64-column passes: 32 < de <= 64): the gradient w.r.t. e0
        // through the edge MLP's first layer and the e0 columns of that layer's weight gradient are ONE product each with
        // S = sum_s dZ1_s after the loop -- 2 E he de MACs less in every step's backward chain and in every step's weight gradient
        // (2 x 2.05 of ~31 GFLOP per step at cfg-B), for one pass over the kept dZ1 blocks.
        // (the bf16 backward chain kernel never contracts the e0 columns: always hoisted there, also at L = 1)
        hoist_e0 = use_b16 || (use_chain && d.ef == 2 && L > 1 && chain_e0_half_is_one_pass(pad32(de)) && he % 4 == 0 && de % 4 == 0);
        // bf16-operand training: the per-node projections' weight gradient over bf16 ROWS -- dP_s rounded once by the scatter-add kernel that
        // produces it, x_{s-1} from the forward's bf16 mirror -- on the LDS-DMA kernel in 256 x 256 output tiles (wgrad_rows16.hip)
        // (f.xb_hist is filled under the forward's own run-time test: plan.h node_rows16_runtime, the one definition both sides use)
        node16 = use_b16 && hoist_x && p.dP16 && node_rows16_runtime(f, m, d) && !sw.no_node_rows16;
        // (k_node_step32_bwd stages the weights in LDS: 128 pw + 8 KB + ... <= 64 KB, 16-byte aligned rows)
        // wider models in the split precision: the same three launches as one MFMA kernel (node_chain.hip, node_chain_bwd_kernel)
        fuse_node_chain_bwd = p.ncb_img && !c.bf16 && N > 0 && L > 1 && d.nf == 2;
        fuse_node_bwd = !c.bf16 && dn == 32 && N <= 4096 && pw <= 384 && kx % 4 == 0 &&
                        ((((uintptr_t)f.Wnode) | ((uintptr_t)m.node.weight[0])) & 15) == 0 && !sw.no_node_fusion;
        return MPNHIP_OK;
    }

    // ---- seeds (caller's stream) -------------------------------------------------------------------------------------------------
    int seed() {
        // zeros: dX[0] (unless the caller seeds it) | dX0 | dE0 | gWnode, contiguous in the plan -- and, below, the seed of the gradient
        // w.r.t. e_L: ONE launch of a plain kernel for both (hipMemsetAsync's fill was preceded by ~18 us of idle queue in every step
        // of the cfg-D timeline; two of them opened every backward)
        char* const z0 = reinterpret_cast<char*>(grad_x_out ? p.dX0 : p.dX[0]);
        const size_t z0_bytes = (size_t)(reinterpret_cast<char*>(p.zero_end) - z0);
        if (grad_x_out) MPN_HIP(hipMemcpyAsync(p.dX[0], grad_x_out, xs * 4, hipMemcpyDeviceToDevice, s));
        // the gradient w.r.t. e_s lives in the LAST edge-layer dZ block of step s (it becomes that dZ once masked); bf16 chain: it
        // travels in p.dEpp[ce].  (L == 0: dE_last aliases p.dE0)
        float* dE_last = use_b16 ? p.dEpp[0] : (L > 0 ? p.dZed[ne - 1] + (size_t)(L - 1) * es : p.dE0);
        {
            bool zero_e = !(grad_e_out && es) && es && L > 0;
            if (zero_e && ((((uintptr_t)dE_last) & 15) != 0 || (es * 4) % 16 != 0)) {   // (odd E de: a block inside the dZ array is not 16-byte aligned)
                MPN_HIP(hipMemsetAsync(dE_last, 0, es * 4, s));
                zero_e = false;
            }
            const int64_t n0 = (int64_t)(z0_bytes / 16), n1 = zero_e ? (int64_t)(es * 4 / 16) : 0;   // (arena blocks: 256-byte multiples)
            if (n0 + n1 > 0) {
                int64_t blocks = (n0 + n1 + 255) / 256;
                blocks = blocks > 4096 ? 4096 : blocks;
                hipLaunchKernelGGL(k_zero_pair, dim3((unsigned)blocks), dim3(256), 0, s, reinterpret_cast<uint4*>(z0), n0, reinterpret_cast<uint4*>(dE_last), n1);
                MPN_LAUNCH_CHECK();
            }
        }
        if (grad_e_out && es) {
            hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)((es + 255) / 256)), dim3(256), 0, s, grad_e_out, g.perm, dE_last, E, de);
            MPN_LAUNCH_CHECK();
        }
        return MPNHIP_OK;
    }

    // ---- weight images of the chain kernels (caller's stream): bf16 pair images, the split or padded fp32 images, the node chain's ---
    int pack_weights() {
        if (use_b16) {
            const ChainBf16BwdImages im = {p.cb16_img, p.cb16_off_cls, {p.cb16_off_flow[0], p.cb16_off_flow[1]}};
            MPN_TRY(pack_chain_bf16_bwd_weights(m, d, im, s));
        }
        if (use_chain) {
            const ChainBwdImages im = {{p.wf2p[0], p.wf2p[1]}, {p.wfep[0], p.wfep[1]}, p.wc1p, p.w2p, p.w1ep};
            MPN_TRY(pack_chain_bwd_weights(m, d, im, bwd_split, s));
        }
        if (fuse_node_chain_bwd) {
            node_chain_bwd_image_shorts(dn, pw, &ncb_off_wu);
            MPN_TRY(pack_node_chain_bwd(m.node.weight[0], f.Wnode, dn, pw, kx, p.ncb_img, s));
        }
        return MPNHIP_OK;
    }

    // ---- the side stream and the groups of steps (host only) ---------------------------------------------------------------------
    // The steps are finished from L down to 1.  Their weight gradients go in groups: as soon as a group's steps are done
    // its batched products run on a side stream UNDER the remaining steps' chain kernels (which leave 120 of the 256
    // CUs idle for the last third of their run at cfg-B); only the last group runs after the loop.  Groups are issued
    // to ONE side stream in order, so they can share its slab buffer and their "+=" into the gradients stay ordered.
    int schedule_groups() {
        const bool want_fork = backward_forks(m) && side_stream_ready(&side) == MPNHIP_OK;
        if (want_fork) side_lock.lock();
        join.ss = side;
        join.caller = s;
        // Group sizes (in steps, first-finished group first).  The side stream is serial, so the last group should be the
        // smallest: it starts only when the loop is over and what it has not finished when the encoder's backward ends is
        // exposed.  Default for L = 12: 5 + 4 + 3; in general three groups with sizes ~ (5 : 4 : 3), two below six steps or when
        // the products are small.
        if (want_fork) {
            if (L >= 6 && (double)E * dn * dn >= 3e8 && !c.wgrad_split) {
                // (enough work per group to pay for a third round of ~30 launches: cfg-B 8e8; the reference's 32-d widths, 8e7 at
                // cfg-C, do better with two groups -- measured 2.59 -> 2.48 ms.  The row-panel products of MPNHIP_PREC_FP32_SPLIT are
                // two launches per group whatever its size, and a larger group needs fewer slabs per row: two groups there,
                // cfg-B 5.27 -> 5.23 ms)
                ngroups = 3;
                gsize[0] = (int)((5 * L + 6) / 12);
                gsize[2] = (int)(L / 4);
                gsize[1] = (int)L - gsize[0] - gsize[2];
            } else {
                ngroups = 2;
                gsize[0] = (int)(L - L / 2);
                gsize[1] = (int)(L / 2);
            }
        } else {
            gsize[0] = (int)L;
        }
        return MPNHIP_OK;
    }
    // group g (g = 0 is finished first) covers batches [group_lo(g), group_lo(g - 1)); group_lo(-1) = L
    int group_lo(int g) const {
        int lo = (int)L;
        for (int i = 0; i <= g && i < ngroups; ++i) lo -= gsize[i];
        return g < 0 ? (int)L : lo;
    }
    // steps of the last group (the one that runs after the loop): batches [0, last_group_steps())
    int last_group_steps() const { return group_lo(ngroups - 2 < 0 ? -1 : ngroups - 2); }

    // ---- one step of the loop, step = L .. 1 (caller's stream) -------------------------------------------------------------------
    int step(int step_no) {
        StepView v;
        v.step = step_no;
        v.b_ = step_no - 1;  // batch (block) index of this step
        v.b = step_at(f, v.b_);
        v.x_s = f.x_hist + xs * step_no;
        v.e_s = f.e_hist + es * step_no;
        v.dZn = p.dZn + (size_t)v.b_ * xs;
        v.dP = p.dP + (size_t)v.b_ * N * pw;
        for (int i = 0; i < nfl; ++i) v.dzfl[i] = p.dZfl[i] + (size_t)v.b_ * E * m.flow_in.out_dims[i];
        for (int i = 0; i < ne; ++i) v.dzed[i] = p.dZed[i] + (size_t)v.b_ * E * m.edge.out_dims[i];
        for (int i = 0; i + 1 < nc; ++i) v.dzcl[i] = p.dZcl[i] + (size_t)v.b_ * E * m.classifier.out_dims[i];
        v.dEc = v.dzed[ne - 1];
        MPN_TRY(node_update_bwd(v));
        if (use_b16) MPN_TRY(edge_side_bf16(v));
        else if (use_chain) MPN_TRY(edge_side_chain(v));
        else if (E > 0) MPN_TRY(edge_side_unfused(v));
        else MPN_HIP(hipMemsetAsync(v.dP, 0, (size_t)N * pw * 4, s));
        MPN_TRY(projection_bwd(v));
        cx ^= 1;
        return MPNHIP_OK;
    }

    // A. node update  x_s = relu(AGG W^T + b)  (mpn.py:97-99)
    int node_update_bwd(const StepView& v) {
        if (!node_a_done) {
            MPN_TRY(relu_mask(p.dX[cx], v.x_s, v.dZn, (int64_t)xs, s, dx_split ? p.dXh : nullptr));
            const float* Wq[2] = {m.node.weight[0], nullptr};
            MPN_TRY(act_grad(c, 1, v.dZn, dn, nullptr, Wq, 2 * dn, dn, 2 * dn, p.dAGG, 2 * dn, nullptr, nullptr, 0, 0, nullptr, N, s, 0));
        }
        dx_split = false;
        node_a_done = false;
        return MPNHIP_OK;
    }

    // B-E fused, bf16 operands: the mirror of the forward chain kernel (edge_chain_bf16_bwd.hip)
    int edge_side_bf16(const StepView& v) {
        const int b_ = v.b_;
        const int hcw = m.classifier.out_dims[0];
        auto f16 = [](unsigned short* q) { return reinterpret_cast<float*>(q); };
        ChainBwdIO c = {};
        c.dAGG = p.dAGG; c.mask = reinterpret_cast<const unsigned*>(v.b.MK); c.ARG = v.b.ARG; c.dlog = grad_logits + (size_t)b_ * E;
        c.dE_io = p.dEpp[ce];
        c.dZM = f16(w16(p.dZfl[1], (int64_t)b_ * E * dn)); c.dZF = f16(w16(p.dZfl[0], (int64_t)b_ * E * hn));
        c.dZc = f16(w16(p.dZcl[0], (int64_t)b_ * E * hcw)); c.dZ2 = f16(w16(p.dZed[1], (int64_t)b_ * E * de));
        c.dZ1 = f16(w16(p.dZed[0], (int64_t)b_ * E * he));
        c.dE0 = p.dE0; c.dEprev = p.dEpp[ce ^ 1];
        c.first_step = v.step == 1 ? 1 : 0;
        const ChainBf16BwdImages im = {p.cb16_img, p.cb16_off_cls, {p.cb16_off_flow[0], p.cb16_off_flow[1]}};
        const EdgeChainBf16BwdArgs a = chain_bf16_bwd_args(m, d, g, N, E, im, c);
        prof_begin(PROF_CHAIN_BWD, s);
        MPN_TRY(launch_edge_chain_bf16_bwd(a, s));
        prof_end(PROF_CHAIN_BWD, s);
        ce ^= 1;
        // index_put_(accumulate) of the gathers x[flow_col] (mpn.py:87,93) and x[row], x[col] (mpn.py:69) over the bf16 dZ rows
        const float* zf = reinterpret_cast<const float*>(a.dZF);
        const float* z1 = reinterpret_cast<const float*>(a.dZ1);
        float* const dP = v.dP;
        unsigned short* const dP16 = node16 ? p.dP16 + (size_t)b_ * N * pw : nullptr;
        const SegReduce2 c3[3] = {{zf, hn, g.cperm, g.cseg_ptr, 2 * (int)N, hn, dP, pw, (int)N, 2 * he, 2 * he + hn, 0, 0, dP16, pw},
                                  {z1, he, nullptr, g.seg_ptr, (int)N, he, dP, pw, (int)N, 0, 0, 3, (int)N, dP16, pw},
                                  {z1, he, g.cperm_all, g.cseg_all, (int)N, he, dP, pw, (int)N, he, he, 0, 0, dP16, pw}};
        return segment_reduce_csr2_x3_bf16(c3, s);
    }

    // B-E fused: every activation-gradient product of the per-edge modules in one kernel
    int edge_side_chain(const StepView& v) {
        const int b_ = v.b_;
        float* const dP = v.dP;
        ChainBwdIO c = {};
        c.dAGG = p.dAGG; c.mask = reinterpret_cast<const unsigned*>(v.b.MK); c.ARG = v.b.ARG; c.dlog = grad_logits + (size_t)b_ * E;
        c.dE_io = v.dzed[1]; c.dZM = v.dzfl[1]; c.dZF = v.dzfl[0]; c.dZc = v.dzcl[0]; c.dZ1 = v.dzed[0];
        c.dE0 = p.dE0; c.dEprev = v.step == 1 ? p.dE0 : p.dZed[ne - 1] + (size_t)(b_ - 1) * es;
        c.first_step = v.step == 1 ? 1 : 0; c.skip_e0 = hoist_e0 ? 1 : 0;
        const ChainBwdImages im = {{p.wf2p[0], p.wf2p[1]}, {p.wfep[0], p.wfep[1]}, p.wc1p, p.w2p, p.w1ep};
        const EdgeChainBwdArgs a = chain_bwd_args(m, d, g, N, E, im, bwd_split, c);
        prof_begin(PROF_CHAIN_BWD, s);
        MPN_TRY(launch_edge_chain_bwd(a, s));
        prof_end(PROF_CHAIN_BWD, s);
        // index_put_(accumulate) of the gathers x[flow_col] (mpn.py:87,93) and x[row], x[col] (mpn.py:69)
        if (E >= 48 * N) {
            // dense graphs (long segments): the three reductions as ONE launch of the block-per-segment kernel
            const SegReduce2 c3[3] = {{v.dzfl[0], hn, g.cperm, g.cseg_ptr, 2 * (int)N, hn, dP, pw, (int)N, 2 * he, 2 * he + hn, 0, 0},
                                      {v.dzed[0], he, g.rperm, g.rseg_ptr, (int)N, he, dP, pw, (int)N, 0, 0, 0, 0},
                                      {v.dzed[0], he, g.cperm_all, g.cseg_all, (int)N, he, dP, pw, (int)N, he, he, 0, 0}};
            MPN_TRY(segment_reduce_csr2_x3(c3, E, s));
        } else {
            // sparse graphs: ONE launch of the short-segment kernel for the three (segment.hip, k_segment_reduce3).
            // (by row: the sorted order IS (direction, row), so a node's rows are three contiguous runs of the CSR -- no list)
            const SegReduce2 c3[3] = {{v.dzfl[0], hn, g.cperm, g.cseg_ptr, 2 * (int)N, hn, dP, pw, (int)N, 2 * he, 2 * he + hn, 0, 0},
                                      {v.dzed[0], he, nullptr, g.seg_ptr, (int)N, he, dP, pw, (int)N, 0, 0, 3, (int)N},
                                      {v.dzed[0], he, g.cperm_all, g.cseg_all, (int)N, he, dP, pw, (int)N, he, he, 0, 0}};
            MPN_TRY(segment_reduce_csr2_x3(c3, E, s));
        }
        return MPNHIP_OK;
    }

    // B-E one launch per product (any depth, any width)
    int edge_side_unfused(const StepView& v) {
        const int b_ = v.b_;
        float* const dP = v.dP;
        // ---- B. aggregation backward + ReLU of the last flow layer ---------------------------
        {
            int64_t tot = E * (dn / 4 > 0 && dn % 4 == 0 ? dn / 4 : dn);
            hipLaunchKernelGGL(k_agg_bwd, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, p.dAGG, v.b.M, v.b.ARG,
                               g.srow, g.seg_ptr, g.header, (int)N, E, dn, m.agg, dn != 1 ? 1 : 0, v.dzfl[nfl - 1]);
            MPN_LAUNCH_CHECK();
        }
        // ---- C. flow MLPs (both directions grouped) -------------------------------------------
        MPN_TRY(mlp_chain_backward(c, m.flow_out, &m.flow_in, v.dzfl, v.b.HF, dir_rr, E, s));
        {
            // layer 0:  Z = e_s Wfe^T + Pf[col];  dPf[n] = sum over the direction's edges with col == n
            // (index_put_ of x[flow_col], mpn.py:87,93)
            MPN_TRY(segment_reduce_csr2(v.dzfl[0], hn, g.cperm, g.cseg_ptr, 2 * (int)N, hn, dP, pw, (int)N, 2 * he, 2 * he + hn, s, E));
            const float* Wq[2] = {m.flow_out.weight[0] + kx, m.flow_in.weight[0] + kx};
            MPN_TRY(act_grad(c, 2, v.dzfl[0], hn, nullptr, Wq, m.flow_out.in_dim, hn, de, v.dEc, de, nullptr, nullptr, 0, 1, dir_rr, E, s));
        }
        // ---- D. classifier (mpn.py:377 -> :114); also applies the ReLU mask of e_s -------------
        MPN_TRY(classifier_chain(v.b.HC, v.dzcl, grad_logits + (size_t)b_ * E, v.dEc, de != 1 ? v.e_s : nullptr));
        // ---- E. edge MLP (EdgeModel, mpn.py:67-69) ----------------------------------------------
        MPN_TRY(mlp_chain_backward(c, m.edge, nullptr, v.dzed, v.b.HE, nullptr, E, s));
        {
            // dPr / dPc: index_put_(accumulate) of x[row], x[col] (mpn.py:69)
            MPN_TRY(segment_reduce_csr2(v.dzed[0], he, g.rperm, g.rseg_ptr, (int)N, he, dP, pw, (int)N, 0, 0, s, E));
            MPN_TRY(segment_reduce_csr2(v.dzed[0], he, g.cperm_all, g.cseg_all, (int)N, he, dP, pw, (int)N, he, he, s, E));
            // gradient w.r.t. [e0 | e_{s-1}]: one product, then split (e_0 IS e0 at step 1)
            const float* Wa[2] = {m.edge.weight[0] + 2 * kx, nullptr};
            MPN_TRY(act_grad(c, 1, v.dzed[0], he, nullptr, Wa, m.edge.in_dim, he, ke, p.dCat, ke, nullptr, nullptr, 0, 0, nullptr, E, s));
            float* dEp = v.step == 1 ? p.dE0 : p.dZed[ne - 1] + (size_t)(b_ - 1) * es;
            hipLaunchKernelGGL(k_split_cat, dim3((unsigned)((es + 255) / 256)), dim3(256), 0, s, p.dCat, E, de, d.ef == 2 ? 1 : 0,
                               p.dE0, dEp, v.step == 1 ? 1 : 0);
            MPN_LAUNCH_CHECK();
        }
        return MPNHIP_OK;
    }

    // activation-gradient chain of the classifier for one step: dz chain blocks in dzc[], final product
    // accumulated into dEdst and masked by `mask` (ReLU of the edge layer that produced ef)
    int classifier_chain(float* const* HC, float* const* dzc, const float* dlog, float* dEdst, const float* mask) {
        if (E == 0) return MPNHIP_OK;
        const mpnhip_mlp& cls = m.classifier;
        for (int i = nc - 1; i >= 0; --i) {
            const int n_out = cls.out_dims[i], k_in = layer_in(cls, i);
            const bool top = i == nc - 1;  // dZ of the last layer is grad_logits, [E, 1] in ORIGINAL order
            const float* A = top ? dlog : dzc[i];
            const float* Wq[2] = {cls.weight[i], nullptr};
            if (i == 0)
                MPN_TRY(act_grad(c, 1, A, top ? 1 : n_out, top ? g.perm : nullptr, Wq, k_in, n_out, k_in, dEdst, de, nullptr, mask, de,
                                 1, nullptr, E, s));
            else
                MPN_TRY(act_grad(c, 1, A, top ? 1 : n_out, top ? g.perm : nullptr, Wq, k_in, n_out, k_in, dzc[i - 1], k_in, nullptr,
                                 k_in != 1 ? HC[i - 1] : nullptr, k_in, 0, nullptr, E, s));
        }
        return MPNHIP_OK;
    }

    // F. per-node projections  P = [x0 | x_{s-1}] Wnode^T
    int projection_bwd(const StepView& v) {
        const int step = v.step, b_ = v.b_;
        float* const dP = v.dP;
        float* dXp = p.dX[cx ^ 1];
        if (hoist_x && step > 1 && fuse_node_bwd) {
            // the reference's node width: this product, the previous step's ReLU mask and its node-update activation gradient
            // in one launch (segment.hip, node_step32_bwd); the next iteration starts at the chain kernel
            MPN_TRY(node_step32_bwd(dP, (int)N, pw, f.Wnode + dn, kx, f.x_hist + xs * (step - 1), m.node.weight[0],
                                    p.dZn + (size_t)(b_ - 1) * xs, p.dAGG, s));
            node_a_done = true;
        } else if (hoist_x && step > 1 && fuse_node_chain_bwd) {
            NodeChainBwdArgs a = {(int)N, dn, pw, dP, p.ncb_img, f.x_hist + xs * (step - 1), p.ncb_img + ncb_off_wu,
                                  p.dZn + (size_t)(b_ - 1) * xs, p.dAGG};
            MPN_TRY(launch_node_chain_bwd(a, s));
            node_a_done = true;
        } else if (hoist_x && step > 1 && pw % 8 == 0 && N * 2 < 2000000000 && !c.bf16) {
            // [N, pw] x [pw, dn] is 157 tiles of 64 x 64 at cfg-B -- not enough blocks for 256 CUs and 34 K steps each: the two K
            // halves run as the two groups of ONE grouped launch into dXp / dXh; the next step's ReLU-mask kernel adds them
            GemmArgs a = {};
            a.ngroups = 2; a.N = dn; a.K = pw / 2; a.ksplit = pw / 2; a.m_upper = 2 * N; a.small_tiles = 1;
            for (int q = 0; q < 2; ++q) {
                GemmGroup& G = a.g[q];
                init_group(G);
                G.A = dP + q * (pw / 2); G.lda = pw;
                G.B = f.Wnode + dn + (size_t)q * (pw / 2) * kx; G.ldb = kx;
                G.C = q == 0 ? dXp : p.dXh; G.ldc = dn;
                G.m_static = N;
            }
            MPN_TRY(launch_gemm(a, A_KCONTIG, B_NCONTIG, MPNHIP_PREC_FP32, s));
            dx_split = true;
        } else if (hoist_x) {
            // only the x_{s-1} columns here (at step 1 x_0 IS x0); the re-attached x0's columns take the SUM of the steps'
            // dP after the loop: one product instead of L
            const float* Wa[2] = {f.Wnode + dn, nullptr};
            MPN_TRY(act_grad(c, 1, dP, pw, nullptr, Wa, kx, pw, dn, step == 1 ? p.dX0 : dXp, dn, nullptr, nullptr, 0, step == 1 ? 1 : 0,
                             nullptr, N, s, 1));
        } else {
            const float* Wa[2] = {f.Wnode, nullptr};
            MPN_TRY(act_grad(c, 1, dP, pw, nullptr, Wa, kx, pw, kx, p.dCat, kx, nullptr, nullptr, 0, 0, nullptr, N, s));
            if (xs) {
                hipLaunchKernelGGL(k_split_cat, dim3((unsigned)((xs + 255) / 256)), dim3(256), 0, s, p.dCat, N, dn, d.nf == 2 ? 1 : 0,
                                   p.dX0, step == 1 ? p.dX0 : dXp, step == 1 ? 1 : 0);
                MPN_LAUNCH_CHECK();
            }
        }
        return MPNHIP_OK;
    }

    // ---- after step b + 1: a group of steps is complete -> its weight gradients to the side stream ------------------------------
    int fork_group_if_due(int b) {
        if (next_group < ngroups - 1 && b == group_lo(next_group)) {
            MPN_HIP(hipEventRecord(side->ready, s));
            MPN_HIP(hipStreamWaitEvent(side->stream, side->ready, 0));
            join.forked = true;
            MPN_TRY(mp_weight_grads(group_lo(next_group), group_lo(next_group - 1) - group_lo(next_group), side->stream, p.slab_side));
            ++next_group;
        }
        return MPNHIP_OK;
    }

    // ---- weight gradients of the message-passing modules for steps b0+1 .. b0+nb: ONE batched split-row product per weight ------
    // (batch index = step - 1).  Issued on `st` with the slab buffer `slab`.
    int mp_weight_grads(int b0, int nb, hipStream_t st, float* slab) {
        if (nb <= 0) return MPNHIP_OK;
        const int64_t zb = b0;  // first batch
        // MPNHIP_PREC_FP32_SPLIT: the products below are recorded and run as ONE product launch + ONE slab-sum launch at the end
        // (calls are serialised on `st`, so successive groups may share the slab region)
        WpBatch wpb;
        if (c.wgrad_split) wp_batch_init(&wpb, p.slab_wp, p.slab_wp_floats, true, &st);
        WpBatch* const batch = c.wgrad_split ? &wpb : nullptr;
        {   // node update Linear
            WgProduct w = {.dZ = {p.dZn + zb * xs, dn, (int64_t)xs}, .H = {f.step0.AGG + zb * sstride, 2 * dn, sstride}, .n_out = dn, .k_in = 2 * dn,
                           .ldw = 2 * dn, .rows = N, .nbatch = nb, .g = {{m.node.grad_weight[0], m.node.grad_bias[0]}}};
            if (node16 && p.dZn16 && sstride % 4 == 0) {
                // bf16 rows (rounded here, on the products' own stream, ahead of the recorded batch): [dn x 2 dn] = two column tiles of
                // the LDS-DMA kernel instead of 2 x 4 tiles of the row-panel kernel over fp32 rows
                MPN_TRY(to_bf16_rows(p.dZn + zb * xs, p.dZn16 + zb * xs, (int64_t)nb * xs, st));
                for (int q = 0; q < nb; ++q)
                    MPN_TRY(to_bf16_rows(f.step0.AGG + (zb + q) * sstride, p.AGG16 + (zb + q) * N * 2 * dn, N * 2 * dn, st));
                w.dZ = {reinterpret_cast<const float*>(p.dZn16 + zb * xs), dn, (int64_t)xs};
                w.H = {reinterpret_cast<const float*>(p.AGG16 + zb * N * 2 * dn), 2 * dn, N * 2 * dn};
                w.src16 = true;
            }
            MPN_TRY(weight_grad(c, slab, batch, w, st));
        }
        if (use_b16) MPN_TRY(edge_weight_grads_bf16(zb, nb, st, slab, batch));
        else if (E > 0) MPN_TRY(edge_weight_grads_fp32(zb, nb, st, slab, batch));
        // per-node projections (packed), accumulated into gWnode
        if (hoist_x) {
            // columns [dn, 2 dn) (the current features) here; the x0 columns are one product with the summed dP after the loop
            WgProduct w = {.dZ = {p.dP + zb * N * pw, pw, (int64_t)N * pw}, .H = {f.x_hist + xs * zb, dn, (int64_t)xs}, .n_out = pw, .k_in = dn,
                           .ldw = kx, .rows = N, .nbatch = nb, .g = {{p.gWnode + dn, nullptr}}};
            if (node16) {
                w.dZ.p = reinterpret_cast<const float*>(p.dP16 + zb * N * pw);
                w.H.p = reinterpret_cast<const float*>(f.xb_hist + xs * zb);
                w.src16 = true;
            }
            MPN_TRY(weight_grad(c, slab, batch, w, st));
        } else {
            const bool two = d.nf == 2;
            Operand h1 = two ? Operand{x0, dn, 0} : Operand{f.x_hist + xs * zb, dn, (int64_t)xs};
            Operand h2 = two ? Operand{f.x_hist + xs * zb, dn, (int64_t)xs} : Operand{nullptr, 0, 0};
            MPN_TRY(weight_grad(c, slab, batch, {.dZ = {p.dP + zb * N * pw, pw, (int64_t)N * pw}, .H = h1, .H2 = h2, .csplit = dn, .n_out = pw, .k_in = kx,
                                                 .ldw = kx, .rows = N, .nbatch = nb, .g = {{p.gWnode, nullptr}}}, st));
        }
        // the one flush of the recorded batch, whichever form the projection product took
        return batch ? wp_batch_flush(batch, st) : MPNHIP_OK;
    }

    // the per-edge modules' products of mp_weight_grads, bf16 chain: every operand of these products is a bf16 row block -- the backward
    // chain kernel's dZ outputs, the forward chain kernel's saved activations and the bf16 mirror of e_hist (WgProduct::src16: loaded
    // as they are, one product per k block)
    int edge_weight_grads_bf16(int64_t zb, int nb, hipStream_t st, float* slab, WpBatch* batch) {
        const mpnhip_mlp& cls = m.classifier;
        const int hcw = cls.out_dims[0];
        const int64_t ss16 = 2 * sstride;   // unsigned shorts between two steps' saved activations
        const float* dZF = u16(p.dZfl[0], zb * E * hn); const float* dZM = u16(p.dZfl[1], zb * E * dn);
        const float* dZ1 = u16(p.dZed[0], zb * E * he); const float* dZ2 = u16(p.dZed[1], zb * E * de);
        const float* dZc = u16(p.dZcl[0], zb * E * hcw);
        const float* H1 = u16(f.step0.HE[0], zb * ss16); const float* HFb = u16(f.step0.HF[0], zb * ss16);
        const float* HCb = u16(f.step0.HC[0], zb * ss16);
        const float* eb_new = reinterpret_cast<const float*>(f.eb_hist + es * (zb + 1));
        const float* eb_prev = reinterpret_cast<const float*>(f.eb_hist + es * zb);
        // flow layer 1, both directions
        MPN_TRY(weight_grad(c, slab, batch, {.dZ = {dZM, dn, (int64_t)E * dn}, .H = {HFb, hn, ss16}, .n_out = dn, .k_in = hn, .ldw = hn, .rows = E,
                                             .nbatch = nb, .src16 = true,
                                             .g = {{m.flow_out.grad_weight[1], m.flow_out.grad_bias[1], dir_rr[0]},
                                                   {m.flow_in.grad_weight[1], m.flow_in.grad_bias[1], dir_rr[1]}}}, st));
        // flow layer 0: e' columns [kx, kx + de) and the bias (folded into P in the forward)
        MPN_TRY(weight_grad(c, slab, batch, {.dZ = {dZF, hn, (int64_t)E * hn}, .H = {eb_new, de, (int64_t)es}, .n_out = hn, .k_in = de,
                                             .ldw = m.flow_out.in_dim, .rows = E, .nbatch = nb, .src16 = true,
                                             .g = {{m.flow_out.grad_weight[0] + kx, m.flow_out.grad_bias[0], dir_rr[0]},
                                                   {m.flow_in.grad_weight[0] + kx, m.flow_in.grad_bias[0], dir_rr[1]}}}, st));
        // classifier output layer [1 x hc]: dZ = grad_logits (fp32, original order -> perm), H = HC rows (bf16)
        MPN_TRY(weight_grad(c, slab, batch, {.dZ = {grad_logits + zb * E, 1, (int64_t)E}, .dz_idx = g.perm, .H = {HCb, hcw, ss16}, .n_out = 1, .k_in = hcw,
                                             .ldw = hcw, .rows = E, .nbatch = nb, .src16 = true, .g = {{cls.grad_weight[1], cls.grad_bias[1]}}}, st));
        // classifier layer 0
        MPN_TRY(weight_grad(c, slab, batch, {.dZ = {dZc, hcw, (int64_t)E * hcw}, .H = {eb_new, de, (int64_t)es}, .n_out = hcw, .k_in = de, .ldw = de,
                                             .rows = E, .nbatch = nb, .src16 = true, .g = {{cls.grad_weight[0], cls.grad_bias[0]}}}, st));
        // edge layer 1
        MPN_TRY(weight_grad(c, slab, batch, {.dZ = {dZ2, de, (int64_t)E * de}, .H = {H1, he, ss16}, .n_out = de, .k_in = he, .ldw = he, .rows = E,
                                             .nbatch = nb, .src16 = true, .g = {{m.edge.grad_weight[1], m.edge.grad_bias[1]}}}, st));
        // edge layer 0: the e_{s-1} columns and the bias (the e0 columns: one product with the summed dZ1 after the loop)
        MPN_TRY(weight_grad(c, slab, batch, {.dZ = {dZ1, he, (int64_t)E * he}, .H = {eb_prev, de, (int64_t)es}, .n_out = he, .k_in = de,
                                             .ldw = m.edge.in_dim, .rows = E, .nbatch = nb, .src16 = true,
                                             .g = {{m.edge.grad_weight[0] + 2 * kx + de, m.edge.grad_bias[0]}}}, st));
        return MPNHIP_OK;
    }

    // ... and over fp32 blocks (E > 0)
    int edge_weight_grads_fp32(int64_t zb, int nb, hipStream_t st, float* slab, WpBatch* batch) {
        const mpnhip_mlp& cls = m.classifier;
        float* dzfl_b[MPNHIP_MAX_LAYERS];
        float* dzed_b[MPNHIP_MAX_LAYERS];
        float* hf_b[MPNHIP_MAX_LAYERS];
        float* he_b[MPNHIP_MAX_LAYERS];
        for (int i = 0; i < nfl; ++i) { dzfl_b[i] = p.dZfl[i] + zb * E * m.flow_in.out_dims[i]; hf_b[i] = f.step0.HF[i] ? f.step0.HF[i] + zb * sstride : nullptr; }
        for (int i = 0; i < ne; ++i) { dzed_b[i] = p.dZed[i] + zb * E * m.edge.out_dims[i]; he_b[i] = f.step0.HE[i] ? f.step0.HE[i] + zb * sstride : nullptr; }
        MPN_TRY(mlp_weight_grads(c, slab, batch, m.flow_out, &m.flow_in, dzfl_b, hf_b, sstride, dir_rr, E, nb, st));
        // flow layer 0: e-part columns [kx, kx + de) and the bias (folded into P in the forward)
        MPN_TRY(weight_grad(c, slab, batch, {.dZ = {dzfl_b[0], hn, (int64_t)E * hn}, .H = {f.e_hist + es * (zb + 1), de, (int64_t)es}, .n_out = hn,
                                             .k_in = de, .ldw = m.flow_out.in_dim, .rows = E, .nbatch = nb,
                                             .g = {{m.flow_out.grad_weight[0] + kx, m.flow_out.grad_bias[0], dir_rr[0]},
                                                   {m.flow_in.grad_weight[0] + kx, m.flow_in.grad_bias[0], dir_rr[1]}}}, st));
        // classifier: dZ of the last layer is grad_logits ([L, E], original order -> perm)
        for (int i = nc - 1; i >= 0; --i) {
            const int n_out = cls.out_dims[i], k_in = layer_in(cls, i);
            const bool top = i == nc - 1;
            Operand dz = top ? Operand{grad_logits + zb * E, 1, (int64_t)E} : Operand{p.dZcl[i] + zb * E * n_out, n_out, (int64_t)E * n_out};
            Operand h = i == 0 ? Operand{f.e_hist + es * (zb + 1), de, (int64_t)es} : Operand{f.step0.HC[i - 1] + zb * sstride, k_in, sstride};
            MPN_TRY(weight_grad(c, slab, batch, {.dZ = dz, .dz_idx = top ? g.perm : nullptr, .H = h, .n_out = n_out, .k_in = k_in, .ldw = k_in, .rows = E,
                                                 .nbatch = nb, .g = {{cls.grad_weight[i], cls.grad_bias[i]}}}, st));
        }
        MPN_TRY(mlp_weight_grads(c, slab, batch, m.edge, nullptr, dzed_b, he_b, sstride, nullptr, E, nb, st));
        if (hoist_e0) {
            // edge layer 0: the e_{s-1} columns [2kx + de, 2kx + 2 de) and the bias; the e0 columns follow after the loop
            MPN_TRY(weight_grad(c, slab, batch, {.dZ = {dzed_b[0], he, (int64_t)E * he}, .H = {f.e_hist + es * zb, de, (int64_t)es}, .n_out = he,
                                                 .k_in = de, .ldw = m.edge.in_dim, .rows = E, .nbatch = nb,
                                                 .g = {{m.edge.grad_weight[0] + 2 * kx + de, m.edge.grad_bias[0]}}}, st));
        } else {   // edge layer 0: e-part columns [2kx, 2kx + ke) = [e0 | e_{s-1}], and the bias
            const bool two = d.ef == 2;
            Operand h1 = two ? Operand{e0, de, 0} : Operand{f.e_hist + es * zb, de, (int64_t)es};
            Operand h2 = two ? Operand{f.e_hist + es * zb, de, (int64_t)es} : Operand{nullptr, 0, 0};
            MPN_TRY(weight_grad(c, slab, batch, {.dZ = {dzed_b[0], he, (int64_t)E * he}, .H = h1, .H2 = h2, .csplit = de, .n_out = he, .k_in = ke,
                                                 .ldw = m.edge.in_dim, .rows = E, .nbatch = nb,
                                                 .g = {{m.edge.grad_weight[0] + 2 * kx, m.edge.grad_bias[0]}}}, st));
        }
        return MPNHIP_OK;
    }

    // ---- after the loop: the last group of steps goes to the side stream (in order behind the earlier groups), under the sums /
    // products of the hoisted shares and the encoder's backward that follow on the caller's stream
    int fork_last_group() {
        if (L > 0 && join.forked) {
            MPN_HIP(hipEventRecord(side->ready, s));
            MPN_HIP(hipStreamWaitEvent(side->stream, side->ready, 0));
            MPN_TRY(mp_weight_grads(0, last_group_steps(), side->stream, p.slab_side));
        }
        return MPNHIP_OK;
    }

    // ---- where the tail's products (hoisted shares, encoder layers) are recorded and where the batch will run (host only) --------
    // MPNHIP_PREC_FP32_SPLIT with a side stream: the weight-gradient products of this tail (hoisted shares, encoder layers) are
    // leaves -- nothing on the caller's stream reads their results -- so they are RECORDED here and run as ONE batch at the end
    // (flush_tail), while the caller's stream goes on with the activation-gradient chain (the encoder chains keep every dZ
    // block of <= 3 layers: BwdPlan::T / Tn).  With MPNHIP_BWD_DEFER_SIDE_JOIN the encoder's products stay on the caller's stream
    // as separate launches and only the hoisted shares are batched: there the side stream's order must end with the
    // message-passing modules' gradients (a trainer puts their all-reduce behind it while the encoder's backward still runs).
    int plan_tail() {
        defer_tail = c.wgrad_split && L > 0 && join.forked;
        defer_encoder = defer_tail && !(flags & MPNHIP_BWD_DEFER_SIDE_JOIN) && m.enc_node.n_layers <= 3 && m.enc_edge.n_layers <= 3;
        if (defer_tail) wp_batch_init(&tailb, p.slab_tail, p.slab_tail_floats, true, nullptr);   // (no stream yet: a full tail batch is not rolled)
        // where the tail's products are recorded: the hoisted shares' while the batch exists, the encoder's only when it stays to the end
        tail_hoist = defer_tail ? &tailb : nullptr;
        tail_enc = defer_encoder ? &tailb : nullptr;
        // flush_tail runs what was recorded (its "+=" go to gradient columns disjoint from the groups': it may run
        // beside the last group of steps).  Where it runs.  With the encoder's products deferred to the end anyway (no MPNHIP_BWD_DEFER_SIDE_JOIN) it runs on the
        // CALLER's stream itself, then the join, the unpacking and whatever the caller enqueues next: no hop ahead of the batch (event
        // record -> wait: 10 - 18 us each) and one instead of two behind it.  Same-box A-B, three runs each, second side stream / caller's
        // stream / first side stream: cfg-B 4.94 - 5.00 / 4.90 - 4.93 / 4.92 - 4.97 ms, cfg-C 1.76 - 1.78 / 1.72 - 1.74 / 1.80 - 1.82, cfg-E 33.5 - 33.6 /
        // 33.6 / 34.0, cfg-D 0.494 / 0.444 / 0.470 -- the second stream was round 4's answer to a tail of ~0.3 ms behind the last group; with
        // the launches' blocks dispatched longest first it no longer pays.  A trainer's path (MPNHIP_BWD_DEFER_SIDE_JOIN: the hoisted
        // shares' products run early, the message-passing gradients' collective follows on the first side stream) keeps the second stream
        // on large graphs -- the first side stream is ordered behind it, so the unpacking and the collective that follow there see both.
        tail_beside = (flags & MPNHIP_BWD_DEFER_SIDE_JOIN) && (double)E * dn >= 1e6;
        tail_inline = defer_encoder && !tail_beside;
        later16.pool = p.enc16;
        later16.pool_elems = p.enc16_elems;
        return MPNHIP_OK;
    }

    // runs the tail batch: on the caller's stream (tail_inline), on the second side stream (tail_beside) or on the first
    int flush_tail() {
        if (!defer_tail) return MPNHIP_OK;
        hipStream_t st = tail_inline ? s : tail_beside ? side->stream2 : side->stream;
        if (!tail_inline) {
            MPN_HIP(hipEventRecord(side->ready, s));
            MPN_HIP(hipStreamWaitEvent(st, side->ready, 0));
        }
        for (int i = 0; i < later16.n; ++i) MPN_TRY(to_bf16_rows(later16.item[i].src, later16.item[i].dst, later16.item[i].n, st));
        later16.n = 0;
        MPN_TRY(wp_batch_flush(&tailb, st));
        if (tail_beside) {
            MPN_HIP(hipEventRecord(side->done2, side->stream2));
            MPN_HIP(hipStreamWaitEvent(side->stream, side->done2, 0));
        }
        return MPNHIP_OK;
    }

    // ---- the re-attached x0 / e0 shares, once, from the sums over the steps (caller's stream; their weight-gradient products go
    // to the tail batch when there is one) -----------------------------------------------------------------------------------------
    int hoisted_shares() {
        if (hoist_x) {
            const int64_t n4 = N * pw / 4;
            hipLaunchKernelGGL(k_sum_blocks, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, p.dP, N * pw, (int)L, n4, p.dPsum);
            MPN_LAUNCH_CHECK();
            const float* Wa[2] = {f.Wnode, nullptr};
            MPN_TRY(act_grad(c, 1, p.dPsum, pw, nullptr, Wa, kx, pw, dn, p.dX0, dn, nullptr, nullptr, 0, 1, nullptr, N, s));
            // ... and the x0 columns [0, dn) of the packed projection weight's gradient: (sum of dP)^T x0 (disjoint from the columns the
            // side stream accumulates; main-stream slab buffer)
            WgProduct w = {.dZ = {p.dPsum, pw, 0}, .H = {x0, dn, 0}, .n_out = pw, .k_in = dn, .ldw = kx, .rows = N, .nbatch = 1, .g = {{p.gWnode, nullptr}}};
            if (node16) {
                MPN_TRY(to_bf16_rows(p.dPsum, p.dPsum16, N * pw, s));
                w.dZ.p = reinterpret_cast<const float*>(p.dPsum16);
                w.H.p = reinterpret_cast<const float*>(f.xb_hist);
                w.src16 = true;
            }
            MPN_TRY(weight_grad(c, p.slab, tail_hoist, w, s));
        }
        if (hoist_e0) {
            // S = sum_s dZ1_s (the blocks are all kept for the weight gradients);  dE0 += S W1[:, e0 columns];  dW1[:, e0 columns] += S^T e0
            const int64_t n4 = E * he / 4;
            // bf16-operand training: both consumers of S round it to bf16 as they stage it, so S itself is kept as bf16 rows (rounded once,
            // the same values) and its partner e0 is the forward's bf16 mirror: half the bytes written and read twice, the GEMM reads
            // bf16 rows, the weight-gradient product runs on the bf16-row kernels
            const bool s16 = use_b16 && f.eb_hist && he % 8 == 0 && de % 8 == 0;
            if (s16) hipLaunchKernelGGL(k_sum_blocks_bf16<true>, dim3((unsigned)((n4 / 2 + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const unsigned short*>(p.dZed[0]),
                                        E * he, (int)L, n4 / 2, p.dZ1sum);
            else if (use_b16) hipLaunchKernelGGL(k_sum_blocks_bf16<false>, dim3((unsigned)((n4 / 2 + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const unsigned short*>(p.dZed[0]),
                                                 E * he, (int)L, n4 / 2, p.dZ1sum);   // (he % 8 == 0: chain_bf16_train_ok)
            else hipLaunchKernelGGL(k_sum_blocks, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, p.dZed[0], E * he, (int)L, n4, p.dZ1sum);
            MPN_LAUNCH_CHECK();
            const float* Wa[2] = {m.edge.weight[0] + 2 * kx, nullptr};
            MPN_TRY(act_grad(c, 1, p.dZ1sum, he, nullptr, Wa, m.edge.in_dim, he, de, p.dE0, de, nullptr, nullptr, 0, 1, nullptr, E, s, -1, s16));
            MPN_TRY(weight_grad(c, p.slab, tail_hoist, {.dZ = {p.dZ1sum, he, 0}, .H = {s16 ? reinterpret_cast<const float*>(f.eb_hist) : e0, de, 0}, .n_out = he,
                                                        .k_in = de, .ldw = m.edge.in_dim, .rows = E, .nbatch = 1, .src16 = s16,
                                                        .g = {{m.edge.grad_weight[0] + 2 * kx, nullptr}}}, s));
        }
        return MPNHIP_OK;
    }

    // the packed node-projection gradient [W1r; W1c; Wfo_x; Wfi_x] back into the layers' grads (their biases were handled above)
    int unpack_node_grads(hipStream_t us) {
        struct { float* dst; int64_t ld; int c0; int r0; int rows; } parts[4] = {
            {m.edge.grad_weight[0], m.edge.in_dim, 0, 0, he},
            {m.edge.grad_weight[0], m.edge.in_dim, kx, he, he},
            {m.flow_out.grad_weight[0], m.flow_out.in_dim, 0, 2 * he, hn},
            {m.flow_in.grad_weight[0], m.flow_in.in_dim, 0, 2 * he + hn, hn}};
        AddParts P;
        int64_t tot = 0;
        for (int i = 0; i < 4; ++i) {
            P.dst[i] = parts[i].dst; P.ldd[i] = parts[i].ld; P.c0[i] = parts[i].c0; P.r0[i] = parts[i].r0; P.rows[i] = parts[i].rows;
            tot += (int64_t)parts[i].rows * kx;
        }
        if (tot > 0) {   // (one launch for the four blocks: they are disjoint destinations)
            hipLaunchKernelGGL(k_add_block4, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, us, p.gWnode, (int64_t)kx, kx, P);
            MPN_LAUNCH_CHECK();
        }
        return MPNHIP_OK;
    }

    // ---- the end of the message-passing modules' gradients: the unpacking -- now, or pending behind the tail batch -----------------
    int finish_message_passing() {
        if (L == 0) return classifier_only();
        if (join.forked) {
            // (the unpacking follows on the side stream as well: with it every gradient of the message-passing modules and of
            // the classifier is final IN SIDE-STREAM ORDER, while the caller's stream still runs the encoder's backward)
            if (defer_encoder) {
                unpack_pending = true;   // after the tail batch (the hoisted x0 product adds into gWnode), at the end
            } else {
                // the hoisted products: recorded -> run them now on the side stream; run on the caller's stream -> order the
                // unpacking behind them
                if (defer_tail) MPN_TRY(flush_tail());
                else {
                    MPN_HIP(hipEventRecord(side->ready, s));
                    MPN_HIP(hipStreamWaitEvent(side->stream, side->ready, 0));
                }
                MPN_TRY(unpack_node_grads(side->stream));
            }
        } else {
            MPN_TRY(mp_weight_grads(0, last_group_steps(), s, p.slab));
            MPN_TRY(unpack_node_grads(s));
        }
        return MPNHIP_OK;
    }

    // L == 0 (mpn.py:387-389): only the classifier sits between the encoder output and the logits
    int classifier_only() {
        const mpnhip_mlp& cls = m.classifier;
        StepBufs b = f.step0;
        float* dzc[MPNHIP_MAX_LAYERS];
        for (int i = 0; i + 1 < nc; ++i) dzc[i] = p.dZcl[i];
        MPN_TRY(classifier_chain(b.HC, dzc, grad_logits, p.dE0, nullptr));
        for (int i = nc - 1; i >= 0 && E > 0; --i) {
            const int n_out = cls.out_dims[i], k_in = layer_in(cls, i);
            const bool top = i == nc - 1;
            Operand dz = top ? Operand{grad_logits, 1, 0} : Operand{p.dZcl[i], n_out, 0};
            Operand h = i == 0 ? Operand{e0, de, 0} : Operand{b.HC[i - 1], k_in, 0};
            // (L == 0: nothing was forked, no tail batch)
            MPN_TRY(weight_grad(c, p.slab, nullptr, {.dZ = dz, .dz_idx = top ? g.perm : nullptr, .H = h, .n_out = n_out, .k_in = k_in, .ldw = k_in, .rows = E,
                                                     .nbatch = 1, .g = {{cls.grad_weight[i], cls.grad_bias[i]}}}, s));
        }
        // incoming gradients of the final latents ARE gradients of the encoder outputs
        if (xs) {
            hipLaunchKernelGGL(k_add_block, dim3((unsigned)((xs + 255) / 256)), dim3(256), 0, s, p.dX[0], dn, p.dX0, dn, 0, (int)N, dn);
            MPN_LAUNCH_CHECK();
        }
        // (grad_e_out: dE0 was seeded with the gathered grad_e_out -- seed()'s dE_last aliases dE0 when L == 0: nothing to add)
        return MPNHIP_OK;
    }

    // ---- encoder (MLPGraphIndependent, mpn.py:355), caller's stream; the products go to the tail batch when it stays to the end -----
    int encoder_node_bwd() {
        float* two[2] = {f.enc_n[0], nullptr};
        float* hid[MPNHIP_MAX_LAYERS];
        hidden_ptrs(m.enc_node, two, N, true, hid);
        const mpnhip_mlp& en = m.enc_node;
        const float* dz = p.dX0;
        int cur = 0;
        if (N > 0) {
            if (en.out_dims[en.n_layers - 1] != 1) {
                MPN_TRY(relu_mask(p.dX0, x0, p.Tn[0], (int64_t)xs, s));
                dz = p.Tn[0];
            }
            // (bf16-operand training with the deferred tail batch: the wide layers' products over bf16 rows, rounded on the tail's stream)
            Rows16Later* const later = defer_encoder && node16 && p.enc16 ? &later16 : nullptr;
            MPN_TRY(mlp_tail_backward(c, tail_enc, later, p.Tn, en, hid, &dz, &cur, N, s));
            MPN_TRY(encoder_weight_grad(c, tail_enc, later, dz, x, en.out_dims[0], en.in_dim, en.grad_weight[0], en.grad_bias[0], N, s));
            if (grad_x) {
                const float* Wq[2] = {en.weight[0], nullptr};
                MPN_TRY(act_grad(c, 1, dz, en.out_dims[0], nullptr, Wq, en.in_dim, en.out_dims[0], en.in_dim, grad_x, en.in_dim,
                                 nullptr, nullptr, 0, 0, nullptr, N, s));
            }
        }
        return MPNHIP_OK;
    }

    int encoder_edge_bwd() {
        float* two[2] = {f.enc_e[0], nullptr};
        float* hid[MPNHIP_MAX_LAYERS];
        hidden_ptrs(m.enc_edge, two, E, true, hid);
        const mpnhip_mlp& ee = m.enc_edge;
        const float* dz = p.dE0;
        int cur = 0;
        const bool ref_encoder = !c.bf16 && ee.n_layers == 3 && ee.in_dim == 6 && ee.out_dims[0] == 18 && ee.out_dims[1] == 18 && ee.out_dims[2] == 16 &&
                                 p.t_width >= 52 && !sw.no_encoder_fusion;
        if (E > 0 && ref_encoder) {
            // the reference's edge encoder: all three activation gradients in one launch (dz2 | dz1 | dz0 side by side in T[0]),
            // then the weight-gradient products as before
            float* dz2 = p.T[0];
            float* dz1 = dz2 + (size_t)E * 16;
            float* dz0 = dz1 + (size_t)E * 18;
            count_path(PC_EDGE_ENCODER_BWD);
            hipLaunchKernelGGL((k_edge_encoder_bwd<18, 18, 16>), dim3((unsigned)((E + 255) / 256)), dim3(256), 0, s, p.dE0, e0, hid[1], hid[0],
                               ee.weight[2], ee.weight[1], E, dz2, dz1, dz0);
            MPN_LAUNCH_CHECK();
            MPN_TRY(weight_grad(c, p.slab, tail_enc, {.dZ = {dz2, 16, 0}, .H = {hid[1], 18, 0}, .n_out = 16, .k_in = 18, .ldw = 18, .rows = E, .nbatch = 1,
                                                      .g = {{ee.grad_weight[2], ee.grad_bias[2]}}}, s));
            MPN_TRY(weight_grad(c, p.slab, tail_enc, {.dZ = {dz1, 18, 0}, .H = {hid[0], 18, 0}, .n_out = 18, .k_in = 18, .ldw = 18, .rows = E, .nbatch = 1,
                                                      .g = {{ee.grad_weight[1], ee.grad_bias[1]}}}, s));
            dz = dz0;
        } else if (E > 0) {
            if (ee.out_dims[ee.n_layers - 1] != 1) {
                MPN_TRY(relu_mask(p.dE0, e0, p.T[0], (int64_t)es, s));
                dz = p.T[0];
            }
            MPN_TRY(mlp_tail_backward(c, tail_enc, nullptr, p.T, ee, hid, &dz, &cur, E, s));
        }
        if (E > 0) {
            // layer 0 read edge_attr through the sort permutation
            MPN_TRY(weight_grad(c, p.slab, tail_enc, {.dZ = {dz, ee.out_dims[0], 0}, .H = {edge_attr, ee.in_dim, 0}, .h_idx = g.perm, .n_out = ee.out_dims[0],
                                                      .k_in = ee.in_dim, .ldw = ee.in_dim, .rows = E, .nbatch = 1,
                                                      .g = {{ee.grad_weight[0], ee.grad_bias[0]}}}, s));
            if (grad_edge_attr) {
                const float* Wq[2] = {ee.weight[0], nullptr};
                MPN_TRY(act_grad(c, 1, dz, ee.out_dims[0], nullptr, Wq, ee.in_dim, ee.out_dims[0], ee.in_dim, grad_edge_attr,
                                 ee.in_dim, g.perm, nullptr, 0, 0, nullptr, E, s));
            }
        }
        return MPNHIP_OK;
    }

    // ---- the tail batch that stayed to the end, and the unpacking behind it ----------------------------------------------------------
    int flush_tail_and_unpack() {
        if (!unpack_pending) return MPNHIP_OK;
        MPN_TRY(flush_tail());
        if (tail_inline) {
            // the groups' "+=" first (side stream), then the unpacking on the caller's stream
            MPN_HIP(hipEventRecord(side->done, side->stream));
            MPN_HIP(hipStreamWaitEvent(s, side->done, 0));
            join.joined = true;
            MPN_TRY(unpack_node_grads(s));
        } else {
            MPN_TRY(unpack_node_grads(side->stream));
        }
        return MPNHIP_OK;
    }

    // ---- the caller's stream behind the side stream (or, MPNHIP_BWD_DEFER_SIDE_JOIN, the promise that the caller will do it) -------
    int join_side() {
        if ((flags & MPNHIP_BWD_DEFER_SIDE_JOIN) && !join.forked && side) {
            // nothing was forked (no side stream work: few steps, or the fork was not possible), but the caller was promised that the
            // side stream's order ends with the message-passing modules' gradients: order it behind the caller's stream
            MPN_HIP(hipEventRecord(side->ready, s));
            MPN_HIP(hipStreamWaitEvent(side->stream, side->ready, 0));
        }
        if (L > 0 && join.forked) {
            // join: every "+=" of the side stream's groups (and the unpacking) is in.  MPNHIP_BWD_DEFER_SIDE_JOIN leaves it to the
            // caller (mpnhip_side_stream_join): a data-parallel trainer first puts the all-reduce of the message-passing modules'
            // gradients on the side stream, where it overlaps the encoder's backward still running on the caller's stream.
            if (flags & MPNHIP_BWD_DEFER_SIDE_JOIN) {
                join.joined = true;
            } else if (!join.joined) {   // (tail_inline: joined ahead of the unpacking)
                MPN_HIP(hipEventRecord(side->done, side->stream));
                MPN_HIP(hipStreamWaitEvent(s, side->done, 0));
                join.joined = true;
            }
        }
        return MPNHIP_OK;
    }
};

}  // namespace mpnhip

using namespace mpnhip;

extern "C" size_t mpnhip_backward_workspace_bytes(const mpnhip_model* model, int n_nodes, int64_t n_edges) {
    Dims d;
    if (!model) return 256;  // non-zero: "the backward pass is built into this library"
    if (check_full(*model, &d, false) != MPNHIP_OK) return 0;
    return plan_backward(*model, d, fwd_route(*model, d, 1, read_switches()), n_nodes, n_edges, nullptr, nullptr);
}

extern "C" int mpnhip_backward_uses_side_stream(const mpnhip_model* model) { return model && backward_forks(*model) ? 1 : 0; }

extern "C" void* mpnhip_side_stream(void) {
    SideStream* side = nullptr;
    std::lock_guard<std::mutex> lock(g_side_mu);
    return side_stream_ready(&side) == MPNHIP_OK ? static_cast<void*>(side->stream) : nullptr;
}

extern "C" int mpnhip_side_stream_join(void* stream_) {
    SideStream* side = nullptr;
    std::lock_guard<std::mutex> lock(g_side_mu);
    MPN_TRY(side_stream_ready(&side));
    MPN_HIP(hipEventRecord(side->done, side->stream));
    MPN_HIP(hipStreamWaitEvent(static_cast<hipStream_t>(stream_), side->done, 0));
    return MPNHIP_OK;
}

extern "C" int mpnhip_backward(const mpnhip_model* model, const void* graph_buf, int n_nodes, int64_t n_edges,
                               const float* x, const float* edge_attr, const float* grad_logits, const float* grad_x_out,
                               const float* grad_e_out, float* grad_x, float* grad_edge_attr, void* fwd_workspace,
                               size_t fwd_workspace_bytes, void* bwd_workspace, size_t bwd_workspace_bytes, void* stream_) {
    return mpnhip_backward_flags(model, graph_buf, n_nodes, n_edges, x, edge_attr, grad_logits, grad_x_out, grad_e_out, grad_x,
                                 grad_edge_attr, fwd_workspace, fwd_workspace_bytes, bwd_workspace, bwd_workspace_bytes, 0, stream_);
}

extern "C" int mpnhip_backward_flags(const mpnhip_model* model, const void* graph_buf, int n_nodes, int64_t n_edges,
                                     const float* x, const float* edge_attr, const float* grad_logits, const float* grad_x_out,
                                     const float* grad_e_out, float* grad_x, float* grad_edge_attr, void* fwd_workspace,
                                     size_t fwd_workspace_bytes, void* bwd_workspace, size_t bwd_workspace_bytes, int flags,
                                     void* stream_) {
    MPN_CHECK_ARG(model && graph_buf, "backward: null model / graph");
    BackwardRun run(*model, x, edge_attr, grad_logits, grad_x_out, grad_e_out, grad_x, grad_edge_attr, flags, static_cast<hipStream_t>(stream_), read_switches());
    MPN_TRY(run.init(graph_buf, n_nodes, n_edges, fwd_workspace, fwd_workspace_bytes, bwd_workspace, bwd_workspace_bytes));
    // caller's stream: the seeds and the weight images
    MPN_TRY(run.seed());
    MPN_TRY(run.pack_weights());
    // the step loop on the caller's stream; each complete group of steps forks its weight gradients to the side stream
    MPN_TRY(run.schedule_groups());
    for (int step = run.L; step >= 1; --step) {
        MPN_TRY(run.step(step));
        MPN_TRY(run.fork_group_if_due(step - 1));
    }
    // the last group to the side stream FIRST: it runs under everything the caller's stream does from here on
    MPN_TRY(run.fork_last_group());
    MPN_TRY(run.plan_tail());
    MPN_TRY(run.hoisted_shares());
    MPN_TRY(run.finish_message_passing());   // (L == 0: classifier_only)
    MPN_TRY(run.encoder_node_bwd());
    MPN_TRY(run.encoder_edge_bwd());
    MPN_TRY(run.flush_tail_and_unpack());
    return run.join_side();
}

// ---- test instrumentation: ONE launch of a backward chain kernel (include/mpnhip.h) ----------------------------------------------
static int debug_chain_bwd_model(const mpnhip_model* model, Dims* d) {
    MPN_CHECK_ARG(model, "debug_edge_chain_backward: null model");
    MPN_TRY(check_chain_model(*model, d));
    const int hc = model->classifier.out_dims[0];
    bool ok;
    if (model->precision == MPNHIP_PREC_BF16)   // (what the forward's plan asks before it saves in the bf16-row form: chain_bf16_train_ok)
        ok = edge_chain_bf16_supported(d->he, d->de, d->hn, d->dn, hc, d->ef) && d->he % 8 == 0 && d->de % 8 == 0 && d->hn % 8 == 0 &&
             d->dn % 8 == 0 && hc % 8 == 0 && edge_chain_bf16_bwd_supported(d->he, d->de, d->hn, d->dn, hc);
    else if (model->precision == MPNHIP_PREC_FP32 || model->precision == MPNHIP_PREC_FP32_SPLIT)
        ok = edge_chain_supported(d->he, d->de, d->hn, d->dn, hc, d->de, d->ef == 2 ? d->de : 0);
    else {
        set_error("debug_edge_chain_backward: precision %d (MPNHIP_PREC_FP32 / _FP32_SPLIT / _BF16)", model->precision);
        return MPNHIP_ERR_UNSUPPORTED;
    }
    if (!ok) {
        set_error("debug_edge_chain_backward: widths he %d de %d hn %d dn %d hc %d (re-attached edges: %d) are not the kernel's", d->he, d->de,
                  d->hn, d->dn, hc, d->ef - 1);
        return MPNHIP_ERR_UNSUPPORTED;
    }
    return MPNHIP_OK;
}

extern "C" size_t mpnhip_debug_edge_chain_backward_workspace_bytes(const mpnhip_model* model) {
    Dims d;
    if (debug_chain_bwd_model(model, &d) != MPNHIP_OK) return 0;
    Carver a(nullptr);
    if (model->precision == MPNHIP_PREC_BF16) {
        ChainBf16BwdImages im;
        carve_chain_bf16_bwd_images(a, *model, d, &im);
    } else {
        ChainBwdImages im;
        carve_chain_bwd_images(a, d, &im);
    }
    return a.bytes();
}

extern "C" int mpnhip_debug_edge_chain_backward(const mpnhip_model* model, const void* graph_buf, int n_nodes, int64_t n_edges,
                                                const mpnhip_debug_edge_chain_bwd* io, void* workspace, size_t workspace_bytes,
                                                void* stream_) {
    hipStream_t s = static_cast<hipStream_t>(stream_);
    Dims d;
    MPN_TRY(debug_chain_bwd_model(model, &d));
    const mpnhip_model& m = *model;
    const bool bf16 = m.precision == MPNHIP_PREC_BF16;
    MPN_CHECK_ARG(graph_buf && io, "debug_edge_chain_backward: null graph / io");
    MPN_CHECK_ARG(n_nodes >= 0 && n_edges >= 0 && n_edges <= INT32_MAX, "debug_edge_chain_backward: bad sizes");
    MPN_CHECK_ARG(!io->skip_e0 || bf16 || (d.ef == 2 && chain_e0_half_is_one_pass(pad32(d.de))),
                  "debug_edge_chain_backward: skip_e0 needs re-attached edge features and 32 < de <= 64 (whole column passes)");
    if (n_edges == 0) return MPNHIP_OK;
    MPN_CHECK_ARG(n_nodes > 0, "debug_edge_chain_backward: edges without nodes");
    MPN_CHECK_ARG(io->dAGG && io->dlog && io->mask && io->dE_io && io->dZM && io->dZF && io->dZc && io->dZ1 && io->dE0 && (io->dZ2 || !bf16) &&
                  (io->dEprev || io->first_step) && (io->ARG || m.agg != MPNHIP_AGG_MAX), "debug_edge_chain_backward: null tensor");
    MPN_CHECK_ARG(aligned16(io->dAGG) && aligned16(io->ARG) && aligned16(io->dE_io) && aligned16(io->dZM) && aligned16(io->dZF) &&
                  aligned16(io->dZc) && aligned16(io->dZ2) && aligned16(io->dZ1) && aligned16(io->dE0) && aligned16(io->dEprev) &&
                  aligned16(io->mask) && aligned16(workspace),
                  "debug_edge_chain_backward: the matrices and the workspace must be 16-byte aligned");
    MPN_CHECK_WORKSPACE("debug_edge_chain_backward", workspace, workspace_bytes, mpnhip_debug_edge_chain_backward_workspace_bytes(model));
    GraphView g;
    graph_layout(n_nodes, n_edges, &g, const_cast<void*>(graph_buf));
    Carver c(workspace);
    auto fp = [](void* q) { return static_cast<float*>(q); };
    ChainBwdIO b = {};
    b.dAGG = io->dAGG; b.mask = io->mask; b.ARG = io->ARG; b.dlog = io->dlog;
    b.dE_io = io->dE_io; b.dZM = fp(io->dZM); b.dZF = fp(io->dZF); b.dZc = fp(io->dZc); b.dZ2 = fp(io->dZ2); b.dZ1 = fp(io->dZ1);
    b.dE0 = io->dE0; b.dEprev = io->dEprev;
    b.first_step = io->first_step; b.skip_e0 = io->skip_e0; b.plain_barriers = io->plain_barriers;
    if (bf16) {
        ChainBf16BwdImages im;
        carve_chain_bf16_bwd_images(c, m, d, &im);
        MPN_TRY(pack_chain_bf16_bwd_weights(m, d, im, s));
        return launch_edge_chain_bf16_bwd(chain_bf16_bwd_args(m, d, g, n_nodes, n_edges, im, b), s);
    }
    ChainBwdImages im;
    carve_chain_bwd_images(c, d, &im);
    const bool split = m.precision == MPNHIP_PREC_FP32_SPLIT;
    MPN_TRY(pack_chain_bwd_weights(m, d, im, split, s));
    return launch_edge_chain_bwd(chain_bwd_args(m, d, g, n_nodes, n_edges, im, split, b), s);
}

// Test / diagnosis instrumentation: one block of pre-activation gradients mpnhip_backward left in its workspace (sorted edge
// order / node order as stored; include/mpnhip.h).
extern "C" int mpnhip_debug_backward_saved(const mpnhip_model* model, int n_nodes, int64_t n_edges, const void* bwd_workspace,
                                           size_t bwd_workspace_bytes, int what, int step, int layer, float* out, int64_t* rows_out,
                                           int* width_out, void* stream_) {
    hipStream_t s = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(model && bwd_workspace, "debug_backward_saved: null argument");
    const mpnhip_model& m = *model;
    Dims d;
    MPN_TRY(check_full(m, &d));
    const int64_t N = n_nodes, E = n_edges;
    BwdPlan p;
    const size_t need = plan_backward(m, d, fwd_route(m, d, 1, read_switches()), N, E, const_cast<void*>(bwd_workspace), &p);
    // (a null buffer was refused above as a bad argument: only the size test of the macro is live here)
    MPN_CHECK_WORKSPACE("debug_backward_saved", bwd_workspace, bwd_workspace_bytes, need);
    MPN_CHECK_ARG(step >= 1 && step <= (d.L > 0 ? d.L : 1), "debug_backward_saved: step %d", step);
    const size_t b = (size_t)(step - 1);
    const float* src = nullptr;
    int64_t rows = 0;
    int width = 0;
    switch (what) {
        case MPNHIP_BWD_SAVED_DZ_NODE: src = p.dZn + b * N * d.dn; rows = N; width = d.dn; break;
        case MPNHIP_BWD_SAVED_DP: src = p.dP + b * N * d.pw; rows = N; width = d.pw; break;
        case MPNHIP_BWD_SAVED_DZ_FLOW:
            if (layer >= 0 && layer < m.flow_in.n_layers) { width = m.flow_in.out_dims[layer]; src = p.dZfl[layer] + b * E * width; rows = E; }
            break;
        case MPNHIP_BWD_SAVED_DZ_EDGE:
            if (layer >= 0 && layer < m.edge.n_layers) { width = m.edge.out_dims[layer]; src = p.dZed[layer] + b * E * width; rows = E; }
            break;
        case MPNHIP_BWD_SAVED_DZ_CLS:
            if (layer >= 0 && layer + 1 < m.classifier.n_layers) { width = m.classifier.out_dims[layer]; src = p.dZcl[layer] + b * E * width; rows = E; }
            break;
        default: break;
    }
    if (!src) {
        set_error("debug_backward_saved: nothing kept for what = %d, step = %d, layer = %d", what, step, layer);
        return MPNHIP_ERR_ARG;
    }
    if (rows_out) *rows_out = rows;
    if (width_out) *width_out = width;
    if (out && rows > 0 && p.b16 && (what == MPNHIP_BWD_SAVED_DZ_FLOW || what == MPNHIP_BWD_SAVED_DZ_EDGE || what == MPNHIP_BWD_SAVED_DZ_CLS)) {
        // bf16-operand training on the fused kernels: the per-edge dZ blocks are bf16 rows (block b at b * E * width shorts)
        const float* base = what == MPNHIP_BWD_SAVED_DZ_FLOW ? p.dZfl[layer] : (what == MPNHIP_BWD_SAVED_DZ_EDGE ? p.dZed[layer] : p.dZcl[layer]);
        const unsigned short* s16 = reinterpret_cast<const unsigned short*>(base) + b * E * width;
        const int64_t n = rows * width;
        hipLaunchKernelGGL(k_bf16_to_f32, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, s16, out, n);
        MPN_LAUNCH_CHECK();
        return MPNHIP_OK;
    }
    if (out && rows > 0) MPN_HIP(hipMemcpyAsync(out, src, (size_t)rows * width * sizeof(float), hipMemcpyDeviceToDevice, s));
    return MPNHIP_OK;
}
