/*
 * mpnhip.h -- C ABI of the MI355X-native MPNTrackSeg message-passing hot path.
 *
 * The reference (ocetintas/MPNTrackSeg) has no FFI: the path sits behind a Python nn.Module API.
 * Each entry point below names the reference interface it replaces (paths relative to
 * /root/reference/src/mot_neural_solver/); INTEGRATION.md shows the ctypes binding a maintainer
 * would add.  All pointers are DEVICE pointers (HIP) unless stated otherwise; buffers are caller
 * owned; `stream` is a hipStream_t passed as void*; nothing here allocates, frees or synchronises,
 * so every call can be captured in a HIP graph.  Return value: 0 on success, negative MPNHIP_ERR_*
 * otherwise (mpnhip_last_error() gives a host string).  Feature matrices are dense row-major fp32.
 */
#ifndef MPNHIP_H
#define MPNHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPNHIP_OK 0
#define MPNHIP_ERR_ARG (-1)         /* bad argument (null pointer, inconsistent dims, misalignment) */
#define MPNHIP_ERR_HIP (-2)         /* a HIP runtime call / kernel launch failed */
#define MPNHIP_ERR_WORKSPACE (-3)   /* caller buffer too small */
#define MPNHIP_ERR_UNSUPPORTED (-4) /* valid reference configuration this build does not cover */

#define MPNHIP_MAX_LAYERS 8

/* Operand precision of every Linear layer's product.  FP32 (default): fp32 operands and accumulation, the reference's
 * arithmetic.  BF16: activations and weights are rounded to bf16 (round to nearest even) as they enter the product,
 * accumulation, biases, gather-adds and aggregation stay fp32 -- BASELINE.json's "bf16 MLP GEMMs on MFMA"
 * configuration (SURVEY.md section 8d cfg-E).  mpnhip_backward rounds the operands of its products the same way (round 3).
 * Round 4: at the fused chain's widths (edge dim 16 ... 128) mpnhip_forward_saved keeps the hidden activations of the per-edge
 * modules as bf16 rows -- the values the backward's products would round them to anyway -- and the ReLU decisions as bits, and
 * mpnhip_backward runs one fused chain kernel per step over them; the workspaces of the two calls belong together as before. */
#define MPNHIP_PREC_FP32 0
#define MPNHIP_PREC_BF16 1
/* FP32_SPLIT: fp32 results from bf16 matrix instructions.  In the fused per-edge chain kernels (forward and backward) every
 * fp32 operand is taken as the exact sum of three bfloat16 pieces (x = h + m + l, each the RNE rounding of the remainder)
 * and a product is accumulated in fp32 from the six piece products whose weight is at least 2^-16 of the leading one; the
 * three dropped products are below 2^-26 |a b|.  Nothing is rounded to bf16: measured against float64 the logits' error is the
 * FP32 mode's (3 ... 7e-7 relative at cfg-B, 12 steps) and every gradient's is too (decision-pinned comparison, tests/
 * test_gpu_pinned.py: <= 5e-6, the FP32 mode's bound), at 3/8 of the fp32 MFMA's cycles.  One hardware property is handled in the
 * backward kernel: v_mfma_f32_32x32x16_bf16 adds its products to the accumulator with a small bias toward -infinity (mean error
 * -0.06 ... -0.11 of the rms error of a six-product result; tools/micro/mfma_bias.hip), which the backward's sums over edges
 * and steps would add up coherently -- the kernel keeps the gradients of every other edge negated in its registers, so the
 * bias cancels in every sum.  (The forward keeps it: a common offset of ~4e-7 of the logits' scale.)  The larger K-contiguous
 * GEMMs (node projections, encoders) use the same six products; the remaining products (small GEMMs, weight gradients) stay
 * fp32 MFMAs.  Forward and backward.  Operands must be finite and below 3.3e38 in magnitude: an infinite operand gives NaN
 * (inf - inf in the split) where the FP32 mode gives +-inf; pieces below the bf16 normal range (|x| < 1e-33) may be flushed. */
#define MPNHIP_PREC_FP32_SPLIT 2
/* FP32_WGSPLIT: MPNHIP_PREC_FP32 in every product of the forward and of the backward's activation-gradient chain (fp32 MFMAs), and
 * the FP32_SPLIT form for the WEIGHT-GRADIENT products only: there it is the batched row-panel kernel (csrc/wgrad_panel.hip: all
 * products of a group of steps in one launch) that pays -- at the reference's graph sizes (configs[2] / configs[3]: a few hundred
 * nodes) a training step is bound by its ~50 small weight-gradient launches, while the chain kernels, one wave per SIMD, are
 * faster on fp32 MFMAs.  Same accuracy class as the other two fp32 modes; what 'auto' selects for small graphs. */
#define MPNHIP_PREC_FP32_WGSPLIT 3

#define MPNHIP_AGG_SUM 0  /* torch_scatter.scatter_add  (models/mpn.py:273) */
#define MPNHIP_AGG_MEAN 1 /* torch_scatter.scatter_mean (models/mpn.py:267) */
#define MPNHIP_AGG_MAX 2  /* torch_scatter.scatter_max  (models/mpn.py:270), empty segment -> 0 */

/* One reference `MLP` (models/mlp.py:4-28) with dropout_p = 0 and use_batchnorm = False:
 * n_layers Linear layers, weight[i] is nn.Linear layout [out_dims[i], in] row-major, ReLU after every
 * layer whose out dim != 1 (mlp.py:17).  grad pointers (same shapes) are used by mpnhip_backward only
 * and may be NULL otherwise; gradients are ACCUMULATED into them (+=), like autograd's .grad. */
typedef struct {
    int n_layers;
    int in_dim;
    int out_dims[MPNHIP_MAX_LAYERS];
    const float* weight[MPNHIP_MAX_LAYERS];
    const float* bias[MPNHIP_MAX_LAYERS];
    float* grad_weight[MPNHIP_MAX_LAYERS];
    float* grad_bias[MPNHIP_MAX_LAYERS];
} mpnhip_mlp;

/* The hot-path sub-modules of MOTMPNet (models/mpn.py:220-317) -- what
 * `MOTMPNet.__init__(model_params)` builds from `graph_model_params` (configs/tracking_cfg.yaml:134-168). */
typedef struct {
    int dn;               /* encoder_feats_dict.node_out_dim */
    int de;               /* encoder_feats_dict.edge_out_dim */
    int reattach_nodes;   /* reattach_initial_nodes (mpn.py:276) */
    int reattach_edges;   /* reattach_initial_edges (mpn.py:277) */
    int agg;              /* node_agg_fn: MPNHIP_AGG_*  (mpn.py:263-273) */
    int num_enc_steps;    /* mpn.py:249 */
    mpnhip_mlp enc_node;  /* encoder.node_model       (mpn.py:153,237) */
    mpnhip_mlp enc_edge;  /* encoder.edge_model       (mpn.py:159,237) */
    mpnhip_mlp edge;      /* MPNet.edge_model.edge_model, in = nf*2*dn + ef*de (mpn.py:282-283,294) */
    mpnhip_mlp flow_in;   /* MPNet.node_model.flow_in_model,  in = nf*dn + de (mpn.py:285,299) */
    mpnhip_mlp flow_out;  /* MPNet.node_model.flow_out_model (mpn.py:304) */
    mpnhip_mlp node;      /* MPNet.node_model.node_model: ONE Linear(2dn -> dn) + ReLU (mpn.py:309-310) */
    mpnhip_mlp classifier;/* classifier.edge_model    (mpn.py:238) */
    int precision;        /* MPNHIP_PREC_*: operand precision of the Linear layers' products (forward and backward) */
    int weights_prepacked;/* != 0: the head of `workspace` still holds the weight images a previous mpnhip_forward
                           * (save_for_backward = 0) of THIS model wrote there and no weight has changed since: skip
                           * re-packing them (about 20 small launches).  The caller vouches for it; 0 is always safe. */
} mpnhip_model;

const char* mpnhip_version(void);
/* Host string describing the last error raised on the calling thread ("" if none). */
const char* mpnhip_last_error(void);

/* Test instrumentation: host-side counters of the kernel variants launched by this process (which code path a call took:
 * fused chain or GEMMs, block-per-segment or short-segment reductions, ...).  Copies min(capacity, count) values into
 * counts (may be NULL), zeroes them when reset != 0, returns the number of counters; mpnhip_debug_counter_name(i) names
 * counter i ("" past the end).  No reference counterpart: the parity tests use it to prove that the kernel they mean to
 * check is the one that ran. */
int mpnhip_debug_counters(int64_t* counts, int capacity, int reset);
const char* mpnhip_debug_counter_name(int index);

/* Test instrumentation: one activation that mpnhip_forward(save_for_backward = 1) left in its workspace, copied to `out`
 * [rows, width] fp32 in ORIGINAL node / edge order (the workspace keeps per-edge tensors in sorted order).  The parity tests
 * read the forward's ReLU / arg-max DECISIONS from these (value > 0) and differentiate the oracle on the same branch of the
 * piecewise-linear function, so that a gradient comparison is not at the mercy of a pre-activation that sits within fp32
 * noise of zero (tests/test_gpu_pinned.py).  out == NULL: only rows / width are reported.
 *   what                         step        layer   contents (reference line)
 *   MPNHIP_SAVED_ENC_NODE / EDGE -           i       encoder hidden layer i, post-ReLU (mpn.py:355)
 *   MPNHIP_SAVED_X / _E          0..L        -       latent node / edge features after `step` steps (0 = encoder output)
 *   MPNHIP_SAVED_EDGE_HIDDEN     1..L        i       EdgeModel MLP hidden layer i (mpn.py:69)
 *   MPNHIP_SAVED_CLS_HIDDEN      1..L        i       classifier hidden layer i (mpn.py:114)
 *   MPNHIP_SAVED_FLOW_HIDDEN     1..L        i       flow_out / flow_in MLP hidden layer i of each edge's direction (mpn.py:88,95)
 *   MPNHIP_SAVED_MSG             1..L        -       the messages the aggregation reads (mpn.py:89,96)
 *   MPNHIP_SAVED_AGG             1..L        -       [flow_in | flow_out] (mpn.py:97)
 *   MPNHIP_SAVED_ARGMAX          1..L        -       max aggregation: original edge id chosen per (node, column), -1 = none */
#define MPNHIP_SAVED_ENC_NODE 0
#define MPNHIP_SAVED_ENC_EDGE 1
#define MPNHIP_SAVED_X 2
#define MPNHIP_SAVED_E 3
#define MPNHIP_SAVED_EDGE_HIDDEN 4
#define MPNHIP_SAVED_CLS_HIDDEN 5
#define MPNHIP_SAVED_FLOW_HIDDEN 6
#define MPNHIP_SAVED_MSG 7
#define MPNHIP_SAVED_AGG 8
#define MPNHIP_SAVED_ARGMAX 9
int mpnhip_debug_saved(const mpnhip_model* model, const void* graph_buf, int n_nodes, int64_t n_edges, const void* fwd_workspace,
                       size_t fwd_workspace_bytes, int what, int step, int layer, float* out, int64_t* rows, int* width,
                       void* stream);
/* The same for mpnhip_backward: one [rows, width] block of the pre-activation gradients it keeps per step in its workspace
 * (for the batched weight-gradient products), in the order it is stored (edges: sorted order).  step = 1 .. num_enc_steps. */
#define MPNHIP_BWD_SAVED_DZ_NODE 0 /* [N, dn]   gradient of the node update's pre-activation */
#define MPNHIP_BWD_SAVED_DP 1      /* [N, pw]   gradient of the per-node projections */
#define MPNHIP_BWD_SAVED_DZ_FLOW 2 /* layer i of the flow MLPs (last layer: the masked message gradient) */
#define MPNHIP_BWD_SAVED_DZ_EDGE 3 /* layer i of the edge MLP */
#define MPNHIP_BWD_SAVED_DZ_CLS 4  /* hidden layer i of the classifier */
int mpnhip_debug_backward_saved(const mpnhip_model* model, int n_nodes, int64_t n_edges, const void* bwd_workspace,
                                size_t bwd_workspace_bytes, int what, int step, int layer, float* out, int64_t* rows,
                                int* width, void* stream);

/* Test instrumentation: ONE call of the forward neighbour aggregation of a message-passing step on a prepared graph
 * (mpnhip_time_aggregate without its timing loop): src [E, dim] in SORTED edge order, out [N, 2 * dim] = [flow_in | flow_out],
 * argmax (optional, int32, same geometry as out): for MAX the sorted position of the row chosen (first maximum, -1 for empty
 * segments).  Reaches k_segment_reduce_block (E >= 48 * 2N, dim % 4 == 0, dim <= 256), else k_aggregate (dim % 4 == 0), else
 * the scalar short-segment kernel. */
int mpnhip_debug_aggregate(const void* graph_buf, int n_nodes, int64_t n_edges, const float* src, int dim, int agg, float* out,
                           int32_t* argmax, void* stream);

/* Test instrumentation: the three segmented sums of a backward step (the index_put_(accumulate) of the gathers x[flow_col],
 * x[row], x[col]) as mpnhip_backward issues them.  One job sums, for every segment s < nseg, the rows
 * src[list ? list[j] : j] (j in [ptr[s], ptr[s + 1]); with runs > 1 and no list: the union of the runs
 * [ptr[s + r * run_stride], ptr[s + r * run_stride + 1]), r < runs) into out[(s % nmod) * ldo + (s / nmod == 0 ? off0 : off1)
 * + 0 .. dim).  total_rows is the number of source rows the dispatch compares with 48 * nseg to choose between the
 * block-per-segment and the short-segment kernels.  bf16_rows != 0: src holds bf16 rows (lds counts bf16 elements), always the
 * short-segment kernel, and out16 (optional, leading dimension ldo16) receives the sums rounded to nearest-even bf16 as well;
 * out16 / ldo16 are ignored for fp32 rows.  Arguments are checked on the host before any launch (MPNHIP_ERR_ARG): null jobs,
 * negative nseg / dim, null src / ptr / out with nseg > 0 and dim > 0, runs > 1 together with a list, nmod <= 0 with nseg > 0. */
typedef struct mpnhip_seg_job {
    const void* src; int64_t lds; const int32_t* list; const int32_t* ptr; int nseg; int dim; float* out; int64_t ldo;
    int nmod; int off0; int off1; int runs; int run_stride; uint16_t* out16; int64_t ldo16;
} mpnhip_seg_job;
int mpnhip_debug_segment_reduce3(const mpnhip_seg_job jobs[3], int64_t total_rows, int bf16_rows, void* stream);

/* Test instrumentation: ONE call of the dense product every MLP layer of the forward and every activation-gradient product of the
 * fp32 backward goes through (csrc/gemm.hip: launch_gemm), with every term of its prologue and epilogue reachable.  For each of
 * up to two row groups g (rows [*row_begin, *row_end) read from DEVICE memory; row_begin == NULL: 0, row_end == NULL: m_static),
 * for every row m of the group and every column n < N:
 *   v = sum_k a[k] * B(k, n)            a = A[i][0 .. ksplit) followed by A2[i][0 .. K - ksplit), i = a_idx ? a_idx[m] : m;
 *                                       B(k, n) = B[n * ldb + k] (MPNHIP_GEMM_B_KCONTIG: nn.Linear weights) or B[k * ldb + n]
 *   v += bias[n] + G1[(g1_idx ? g1_idx[m] : m) * ldg1 + n] + G2[(g2_idx ? g2_idx[m] : m) * ldg2 + n]     (each optional)
 *   v = relu ? max(v, 0) : v
 *   v += accumulate ? C[c * ldc + n] : 0                                                     c = c_idx ? c_idx[m] : m
 *   C[c * ldc + n] = mask ? (mask[m * ldmask + n] > 0 ? v : 0) : v
 * The groups share N, K, ksplit, relu and accumulate; ksplit == K when A2 is unused.  m_upper: host-side upper bound of the rows of
 * both groups together (sizes the grid; 0: nothing is launched).  small_tiles != 0: the 64 x 64 tile whatever m_upper says.
 * precision: MPNHIP_PREC_FP32 / _BF16 (operands rounded to bf16 as they are staged) / _FP32_SPLIT (three bf16 pieces per operand).
 * chosen (optional) reports what ran: chosen[0] = kernel | form << 8 with kernel 0 = the MFMA strip / tile kernel (chosen[1 .. 3] =
 * its WM, WN, TN: block tile 32 WM x 32 TN WN), 1 = the one-thread-per-output kernel, 2 = the K <= 8 kernel, 3 = the tiled bf16
 * kernel of csrc/gemm_bf16.hip (chosen[1 .. 3] = 0 for 1 .. 3), and form the MPNHIP_PREC_* operand form actually used (the split form
 * is demoted to fp32 unless K >= 128 and N >= 256); chosen[0] = -1 when nothing was launched.  Refused on the host before any launch
 * (MPNHIP_ERR_ARG): null args, ngroups outside 1 .. 2, an unknown b_layout or precision, MPNHIP_GEMM_B_NCONTIG with a precision
 * other than fp32; then the checks of launch_gemm itself (null A / B / C, ksplit without A2, operands beyond 32-bit offsets). */
#define MPNHIP_GEMM_B_KCONTIG 0
#define MPNHIP_GEMM_B_NCONTIG 1
typedef struct mpnhip_debug_gemm_group {
    const float* A; const float* A2; const int32_t* a_idx; const float* B; const float* bias; const float* G1; const int32_t* g1_idx;
    const float* G2; const int32_t* g2_idx; const float* mask; float* C; const int32_t* c_idx; const int32_t* row_begin;
    const int32_t* row_end; int64_t lda; int64_t lda2; int64_t ldb; int64_t ldg1; int64_t ldg2; int64_t ldmask; int64_t ldc;
    int64_t m_static;
} mpnhip_debug_gemm_group;
typedef struct mpnhip_debug_gemm_args {
    mpnhip_debug_gemm_group g[2]; int ngroups; int N; int K; int ksplit; int relu; int accumulate; int64_t m_upper; int small_tiles;
    int b_layout; int precision;
} mpnhip_debug_gemm_args;
int mpnhip_debug_gemm(const mpnhip_debug_gemm_args* args, int32_t chosen[4], void* stream);

/* Test instrumentation: the split-K form of y = act(x W^T + b) for few rows and long K (csrc/gemm.hip: linear_splitk; the node
 * encoder's first layer in mpnhip_forward), optionally with the next, narrow Linear layer y2 = act2(y W2^T + b2) evaluated in the
 * summing launch (w2 != NULL; W2 is [n2, n] row-major).  x [m, k] (leading dimension ldx), w [n, k], y [m, n] (ldy), y2 [m, n2]
 * (ldy2); scratch: scratch_floats floats of device memory, mpnhip_debug_linear_splitk_scratch_floats(m, n, k) suffice (0: not a
 * shape of this path).  taken_and_fused[0] = 1 when the path was taken (0: not a shape of this path -- k < 512, k or ldx not a
 * multiple of 4, more than 8192 rows, 320 or more 64 x 64 tiles, the bf16 precision, too little scratch: nothing is launched and
 * MPNHIP_OK is returned); taken_and_fused[1] = 1 when the next layer ran in the same launch (n % 4 == 0, n <= 256, ldy == n,
 * n2 <= 64), 0: y2 is untouched.  Null x / w / y, an unknown precision or w2 without y2 are refused (MPNHIP_ERR_ARG). */
size_t mpnhip_debug_linear_splitk_scratch_floats(int64_t m, int n, int k);
int mpnhip_debug_linear_splitk(const float* x, int64_t ldx, const float* w, const float* b, float* y, int64_t ldy, int64_t m, int n,
                               int k, int relu, int precision, const float* w2, const float* b2, int n2, int relu2, float* y2,
                               int64_t ldy2, float* scratch, size_t scratch_floats, int32_t taken_and_fused[2], void* stream);

/* Test instrumentation: the weight-gradient products of mpnhip_backward, through the backward's own routing (csrc/gemm_tn.hip:
 * weight_grad_route, the function every product of the backward goes through).  Each of the n_products (1 .. 16) descriptions is, for
 * each of one or two groups g (g[1].grad_w == NULL: one group), every batch b < nbatch and every row
 * r in [*row_begin, *row_end) (read from DEVICE memory; NULL: 0 / rows) intersected with [0, rows):
 *   z[o] = dZ[b * z_bstride + (dz_idx ? dz_idx[r] : r) * ldz + o]                                                 o < n_out
 *   h[c] = c < csplit ? H[b * h_bstride + i * ldh + c] : H2[b * h2_bstride + i * ldh2 + c - csplit]    i = h_idx ? h_idx[r] : r
 *   grad_w[o * ldw + c] += z[o] * h[c]       (c < k_in;  H2 == NULL: csplit = k_in)
 *   grad_b[o] += z[o]                        (grad_b may be NULL)
 * dz_idx / h_idx are the same for every batch.  src16 != 0: dZ and H are bf16 rows (leading dimensions and batch strides count bf16
 * elements; the [1 x k] form keeps an fp32 dZ).  precision: MPNHIP_PREC_FP32 -> the fp32 kernels (launch_gemm_tn);
 * MPNHIP_PREC_FP32_SPLIT -> the row-panel kernels with three bf16 pieces per operand; MPNHIP_PREC_BF16 -> one piece (both operands of a
 * product rounded to nearest-even bf16; the bias sum is not rounded).  one_launch != 0: all products are recorded into one batch on
 * `stream` and flushed once (batched: with the chunk plan of a job that shares its launch); one_launch == 0: batched != 0 -> every
 * product is a batch of its own with that chunk plan, batched == 0 -> every product is run at once, as the backward's unbatched
 * products are.  MPNHIP_PREC_FP32 records nothing: there is no batch, every product is launched at once and one_launch, batched and
 * batch_slab_floats are ignored.  batch_slab_floats > 0 caps the slab region of the batch (a batch that runs out of it is flushed and refilled);
 * 0: room for all products.  Workspace: mpnhip_debug_weight_grad_batch_workspace_bytes with the same arguments.
 * chosen (optional, n_products x 2 x 10 ints) reports per product and group what ran:
 *   [0] path: 0 row-panel kernel, 1 LDS-DMA kernel over bf16 rows (wgrad_rows16.hip), 2 gemm_tn_kernel (MFMA), 3 gemm_tn_narrowk_kernel,
 *       4 gemm_tn_small_kernel, 5 gemm_tn_generic_kernel, -1 nothing ran
 *   [1] variant: the block variant after any narrow re-tiling (row-panel: 0 <5,1>, 1 <1,5>, 2 <4,1>, 3 <1,1>, 5 <2,2>, 6 [1 x k], 7 small
 *       shapes, 8 .. 15 bf16 rows; 16 .. 19 the LDS-DMA kernel's), or the column tile (64 / 128) of gemm_tn_kernel, else 0
 *   [2] tiles_o  [3] tiles_c  [4] chunk (rows per chunk)  [5] nsplit (chunks per batch)
 *   [6] narrow: the job ran in the four-blocks-per-CU launch     [7] rolled: the batch was flushed to make room for this product
 *   [8] xcd_map, [9] red_ny: the fp32 path's XCD-aware block mapping and the partial sums of its two-stage slab sum (1: one stage)
 * Refused on the host before any launch (MPNHIP_ERR_ARG): null products, n_products outside 1 .. 16, an unknown precision, src16 with
 * a precision other than bf16, csplit outside (0, k_in) when H2 is given, bad sizes / null operands; a workspace that is too small
 * (MPNHIP_ERR_WORKSPACE).  A product over bf16 rows that the row-panel kernels do not cover returns MPNHIP_ERR_UNSUPPORTED. */
typedef struct mpnhip_wgrad_group { float* grad_w; float* grad_b; const int32_t* row_begin; const int32_t* row_end; } mpnhip_wgrad_group;
typedef struct mpnhip_wgrad_product {
    const void* dZ; int64_t ldz; int64_t z_bstride; const int32_t* dz_idx;
    const void* H; int64_t ldh; int64_t h_bstride; const int32_t* h_idx;
    const void* H2; int64_t ldh2; int64_t h2_bstride;
    int64_t ldw; int64_t rows; int csplit; int n_out; int k_in; int nbatch; int src16;
    mpnhip_wgrad_group g[2];
} mpnhip_wgrad_product;
size_t mpnhip_debug_weight_grad_batch_workspace_bytes(const mpnhip_wgrad_product* products, int n_products, int precision, int batched,
                                                      int64_t batch_slab_floats);
int mpnhip_debug_weight_grad_batch(const mpnhip_wgrad_product* products, int n_products, int precision, int batched, int one_launch,
                                   int64_t batch_slab_floats, void* workspace, size_t workspace_bytes, int32_t* chosen, void* stream);

/* Test instrumentation: ONE launch of the fused per-edge chain kernel of a message-passing step (csrc/edge_chain.hip:
 * edge_chain_kernel, what mpnhip_forward runs per step in MPNHIP_PREC_FP32 and MPNHIP_PREC_FP32_SPLIT) on caller-given tensors, through
 * the forward's own packer and launcher (pack_chain_weights, launch_edge_chain; with hoist_e0 the forward's Q0 product as well).
 * Of the model only edge, flow_in, flow_out, classifier (two Linear layers each, with weights and biases), dn, de, agg,
 * reattach_edges and precision are read; kx, the node columns in front of the edge columns of edge.weight[0] (twice) and of
 * flow_*.weight[0] (once), is (edge.in_dim - ke) / 2 with ke = (reattach_edges ? 2 : 1) de.  Widths: he = edge.out_dims[0],
 * hn = flow_*.out_dims[0], hc = classifier.out_dims[0], pw = 2 he + 2 hn.  The entries take flags for what the forward's route would
 * decide and read none of its MPNHIP_* switches; two switches that the shared LAUNCHERS read themselves still act:
 * MPNHIP_CHAIN_BF16_PLAIN_BARRIERS (launch_edge_chain_bf16 / _bwd: overrides the plain_barriers flag) and MPNHIP_NO_NODE_CHAIN_BWD
 * (node_chain_bwd_supported: mpnhip_debug_node_chain_backward then returns MPNHIP_ERR_UNSUPPORTED).
 * Per-edge tensors cross the ABI in SORTED edge order (position i holds edge perm[i] of the prepared graph: the edges with
 * row < col first -- group 0, flow_out --, then row > col -- group 1, flow_in --, then the self loops, each group by row); logits is in
 * ORIGINAL order.  With W1 = edge.weight[0], W2 = edge.weight[1], Wc* = classifier.weight[*], Wf* = the weights of flow_out (group
 * 0) or flow_in (group 1), r = srow[i], c = scol[i], for every sorted position i < n_edges:
 *   H1[i]  = relu( [e0[i] | e_prev[i]] W1[:, 2 kx :]^T + P[r][0 .. he) + P[c][he .. 2 he) )       (without re-attachment: e_prev alone)
 *   e_new[i] = relu( H1[i] W2^T + edge.bias[1] )
 *   HC[i]  = relu( e_new[i] Wc0^T + classifier.bias[0] );   logits[perm[i]] = HC[i] . Wc1[0] + classifier.bias[1][0]
 *   and for the edges of groups 0 and 1 only (q = the group):
 *   HF[i]  = relu( e_new[i] Wf0[:, kx :]^T + P[c][2 he + q hn .. 2 he + (q + 1) hn) )
 *   msg[i] = relu( HF[i] Wf1^T + flow.bias[1] )
 * (the first layers' biases and node columns are inside P: the per-node projections, P [N, pw] = [Pr | Pc | Pf_out | Pf_in]).  The rows
 * of msg and hf at self loops are never written.  Every value that is stored is the fp32 value the next product consumes; nothing
 * is rounded between the stages.  MPNHIP_PREC_FP32: fp32 MFMAs; _FP32_SPLIT: three bf16 pieces per operand, six products.
 * save != 0 (training): h1 [E, he], hc [E, hc], hf [E, hn] receive H1, HC, HF as fp32 rows and mask receives the ReLU decisions
 * of H1 | e_new | HC | HF | msg as bits in the kernels' private layout, mpnhip_debug_edge_chain_mask_ints(model, n_edges) words of
 * which none past that count is written: the buffer mpnhip_debug_edge_chain_backward reads.  save == 0: the four are ignored.
 * hoist_e0 != 0 (MPNHIP_PREC_FP32 with re-attachment, de >= 32 and de % 16 == 0 only -- where mpnhip_forward takes this form): Q0 = e0 W1[:, 2 kx : 2 kx + de]^T is computed first
 * (one GEMM launch, counted as such) and the kernel starts H1 from P[r] + Q0[i] and multiplies e_prev only -- the same H1.
 * workspace: mpnhip_debug_edge_chain_forward_workspace_bytes(model, n_edges) (weight images and Q0).
 * Checked on the host before any launch: a null model / graph / io, inconsistent model dims, negative sizes, hoist_e0 where it
 * does not apply (MPNHIP_ERR_ARG); MLP depths other than two, MPNHIP_PREC_BF16, widths edge_chain_supported refuses -- tiles of
 * 32 other than (he, de, hn, dn) = (10, 2, 7, 4), (5, 1, 4, 2), (3, 1, 2, 1), hc > 32, a width that is no multiple of 4, de no multiple
 * of 16 -- (MPNHIP_ERR_UNSUPPORTED; the size queries then return 0); then, with edges (n_edges == 0 is a successful no-op): null
 * tensors, save without its four buffers, a matrix or workspace that is not 16-byte aligned (MPNHIP_ERR_ARG), a short workspace
 * (MPNHIP_ERR_WORKSPACE).  A successful call with edges adds 1 to "edge_chain_fwd" (FP32) or "edge_chain_fwd_split". */
typedef struct mpnhip_debug_edge_chain_fwd {
    const float* P; const float* e0; const float* e_prev;      /* e0: NULL without re-attachment */
    float* e_new; float* msg; float* logits;                   /* [E, de], [E, dn], [E] */
    float* h1; float* hc; float* hf; uint32_t* mask;           /* save != 0 */
    int save; int hoist_e0;
} mpnhip_debug_edge_chain_fwd;
size_t mpnhip_debug_edge_chain_mask_ints(const mpnhip_model* model, int64_t n_edges);
size_t mpnhip_debug_edge_chain_forward_workspace_bytes(const mpnhip_model* model, int64_t n_edges);
int mpnhip_debug_edge_chain_forward(const mpnhip_model* model, const void* graph_buf, int n_nodes, int64_t n_edges,
                                    const mpnhip_debug_edge_chain_fwd* io, void* workspace, size_t workspace_bytes, void* stream);

/* Test instrumentation: ONE launch of the backward of the same chain (csrc/edge_chain.hip: edge_chain_bwd_kernel, steps B1 - B6),
 * through the backward's packer and launcher (pack_chain_bwd_weights, launch_edge_chain_bwd), on the mask buffer a call of
 * mpnhip_debug_edge_chain_forward (save != 0, same model and graph) left.  Model, orders and names as above; [X > 0] are the
 * decisions in the mask buffer.  For every sorted position i, with r = srow[i]:
 *   B1 (groups 0, 1)  g = dAGG[r][dn .. 2 dn) (group 0) or dAGG[r][0 .. dn) (group 1);
 *                     MEAN: g /= max(count of r's segment in the group, 1);  MAX: g[k] = ARG[r][that column] == i ? g[k] : 0
 *                     dZM[i] = g (.) [msg[i] > 0]
 *   B2                dZF[i] = (dZM[i] Wf1) (.) [HF[i] > 0]
 *   B3                dE' = dE_io[i] + dZF[i] Wf0[:, kx :]                            (self loops: dE' = dE_io[i])
 *   B4                dZc[i] = dlog[perm[i]] Wc1[0] (.) [HC[i] > 0];  dE' += dZc[i] Wc0;  dZ2[i] = dE' (.) [e_new[i] > 0]
 *   B5                dZ1[i] = (dZ2[i] W2) (.) [H1[i] > 0]
 *   B6                [d0 | dp] = dZ1[i] W1[:, 2 kx :]     (without re-attachment: dp alone)
 *                     dE0[i] += d0  (not with skip_e0);   first_step ? dE0[i] += dp : dEprev[i] = dp
 * dAGG [N, 2 dn] = [flow_in | flow_out]; ARG (MAX only) [N, 2 dn] int32: the SORTED position the forward's maximum took, -1 for none;
 * dlog [E] in ORIGINAL order; dE_io [E, de]: in, the gradient with respect to e_new arriving from the later step; out, dZ2 (written
 * in place).  Outputs dZM [E, dn], dZF [E, hn] (rows of self loops are never written), dZc [E, hc], dZ1 [E, he]; dE0 [E, de] is
 * accumulated into what the caller put there; dEprev [E, de] (may be NULL with first_step).  skip_e0 != 0 (re-attachment and
 * 32 < de <= 64 only): the e0 half of B6 is left to the caller (mpnhip_backward takes it as one product over the sum of the steps'
 * dZ1), dE0 then receives only the first step's dp.  Every stage consumes the fp32 value it stores.
 * workspace: mpnhip_debug_edge_chain_backward_workspace_bytes(model) (the weight images).
 * Host-side refusals as for the forward (skip_e0 where it does not apply: MPNHIP_ERR_ARG; ARG is required for MAX).  A successful
 * call with edges adds 1 to "edge_chain_bwd" (FP32), "edge_chain_bwd_split" or "edge_chain_bwd_bf16" and to no other counter.
 * MPNHIP_PREC_BF16 (csrc/edge_chain_bf16_bwd.hip: edge_chain_bf16_bwd_kernel through pack_chain_bf16_bwd_weights and
 * launch_edge_chain_bf16_bwd; re-attached edge features and widths that are multiples of 8 which edge_chain_bf16_bwd_supported
 * takes, else MPNHIP_ERR_UNSUPPORTED), on the mask buffer mpnhip_debug_edge_chain_bf16_forward (save != 0) left.  The same steps
 * with bf(.) = nearest-even bfloat16 on BOTH operands of every product, fp32 sums:
 *   dZM = bf(g (.) [msg > 0]);  dZF = bf((dZM bf(Wf1)) (.) [HF > 0]);  dZc = bf(dlog[perm[i]] bf(Wc1[0]) (.) [HC > 0])   (dlog unrounded)
 *   dZ2 = bf((dE_io[i] + dZF bf(Wf0e) + dZc bf(Wc0)) (.) [e_new > 0]);  dZ1 = bf((dZ2 bf(W2)) (.) [H1 > 0])
 *   dp = dZ1 bf(W1[:, 2 kx + de :])  (fp32);  first_step ? dE0[i] += dp : dEprev[i] = dp
 * Every dZ is rounded once and the rounded value is both stored and fed.  The five dZ blocks are bf16 ROWS (uint16 [E, width] behind the
 * void pointers, dZ2 a buffer of its own); dE_io is read only; the e0 half of B6 is never computed (skip_e0 is ignored: mpnhip_backward
 * always takes it as one product after the step loop), so dE0 is touched at the first step only and dEprev at the others only.
 * plain_barriers: passed to the launcher (the fp32 kernels ignore it). */
typedef struct mpnhip_debug_edge_chain_bwd {
    const float* dAGG; const int32_t* ARG; const float* dlog; const uint32_t* mask;
    float* dE_io; void* dZM; void* dZF; void* dZc; void* dZ1; float* dE0; float* dEprev;
    void* dZ2;                                                  /* MPNHIP_PREC_BF16 only */
    int first_step; int skip_e0; int plain_barriers;
} mpnhip_debug_edge_chain_bwd;
size_t mpnhip_debug_edge_chain_backward_workspace_bytes(const mpnhip_model* model);
int mpnhip_debug_edge_chain_backward(const mpnhip_model* model, const void* graph_buf, int n_nodes, int64_t n_edges,
                                     const mpnhip_debug_edge_chain_bwd* io, void* workspace, size_t workspace_bytes, void* stream);

/* Test instrumentation: ONE launch of the bf16-operand forward chain kernel (csrc/edge_chain_bf16.hip: edge_chain_bf16_kernel, what
 * mpnhip_forward runs per step in MPNHIP_PREC_BF16), through pack_chain_bf16_weights and launch_edge_chain_bf16.  Model, orders and
 * formulas as for mpnhip_debug_edge_chain_forward (re-attached edge features are required), with bf(.) = round to nearest-even
 * bfloat16 applied to BOTH operands of every product and everything else in fp32:
 *   H1 = relu(bf([e0 | e_prev]) bf(W1e)^T + P[r] + P[c]);  the kernel keeps and feeds bf(H1)
 *   e_new = relu(bf(H1) bf(W2)^T + b2)  (fp32, stored);     e16 = bf(e_new) is what the classifier and the flow MLPs consume
 *   HC = relu(e16 bf(Wc0)^T + bc0);  logits[perm[i]] = sum_k bf(Wc1[0][k]) bf(HC[k]) + bc1   (an fp32 fma chain)
 *   HF = relu(e16 bf(Wf0e)^T + Pf[c]);  msg = relu(bf(HF) bf(Wf1)^T + bf2)  (fp32)                 (groups 0 and 1 only)
 * The ReLU decisions are taken on the ROUNDED values (bf(H1) > 0, e16 > 0, bf(HC) > 0, bf(HF) > 0) and on the fp32 msg.
 * Flags: save (the SAVE variant: widths multiples of 8 that edge_chain_bf16_bwd_supported takes); rows16 (de % 8 == 0: the entry rounds
 * e0 / e_prev to bf16 rows with the forward's own to_bf16_rows and the kernel reads those -- the same values -- and writes e16);
 * fused_agg (the kernel aggregates: agg_out [N, 2 dn] = [flow_in | flow_out] of msg by model.agg, zero-filled first, msg is not written);
 * plain_barriers (__syncthreads at the weight-chunk ends instead of the counted waits).
 * Outputs: e_new [E, de], msg [E, dn] (or agg_out), in SORTED order; logits [E] in ORIGINAL order.  With save or rows16: e16 [E, de], the
 * bf16 mirror decoded to floats; with save also h1 [E, he], hc [E, hc], hf [E, hn] (the bf16 rows the kernel keeps, decoded) and the five
 * decision sections dec_h1 | dec_e | dec_hc | dec_hf | dec_m as 1.0 / 0.0 floats (self loops: 0 in dec_hf / dec_m) -- ALL decoded
 * tensors come back in ORIGINAL edge order, as mpnhip_debug_saved gives them (chain_bf16_debug_rows / chain_bf16_debug_mask); the raw
 * bits stay in mask, mpnhip_debug_edge_chain_bf16_mask_ints(model, n_edges) words of which none past that count is written.
 * mpnhip_debug_edge_chain_bf16_geometry reports the edges and waves per block of the launch (0: widths the kernel does not take).
 * workspace: mpnhip_debug_edge_chain_bf16_forward_workspace_bytes(model, n_edges).  Host-side refusals as for the fp32 entry; any other
 * precision, widths edge_chain_bf16_supported refuses, save / rows16 at widths they do not take: MPNHIP_ERR_UNSUPPORTED.  A successful
 * call with edges adds 1 to "edge_chain_fwd_bf16" and to no other counter. */
typedef struct mpnhip_debug_edge_chain_bf16_fwd {
    const float* P; const float* e0; const float* e_prev;
    float* e_new; float* msg; float* agg_out; float* logits;
    float* e16; float* h1; float* hc; float* hf;
    float* dec_h1; float* dec_e; float* dec_hc; float* dec_hf; float* dec_m;
    uint32_t* mask;
    int save; int rows16; int fused_agg; int plain_barriers;
} mpnhip_debug_edge_chain_bf16_fwd;
size_t mpnhip_debug_edge_chain_bf16_mask_ints(const mpnhip_model* model, int64_t n_edges);
size_t mpnhip_debug_edge_chain_bf16_forward_workspace_bytes(const mpnhip_model* model, int64_t n_edges);
void mpnhip_debug_edge_chain_bf16_geometry(const mpnhip_model* model, int32_t* edges_per_block, int32_t* waves_per_block);
int mpnhip_debug_edge_chain_bf16_forward(const mpnhip_model* model, const void* graph_buf, int n_nodes, int64_t n_edges,
                                         const mpnhip_debug_edge_chain_bf16_fwd* io, void* workspace, size_t workspace_bytes, void* stream);

/* Test instrumentation: ONE launch of the fused node-side kernel of a message-passing step (csrc/node_chain.hip:
 * node_chain_kernel, what mpnhip_forward runs per step in MPNHIP_PREC_FP32_SPLIT at dn = 64 / 128), on caller-given tensors, through
 * the forward's own packer and launcher (pack_node_chain, launch_node_chain).  On a prepared graph (mpnhip_graph_prep) with
 * seg_ptr the CSR over the keys dir * N + row of the SORTED edge order (dir 0: row < col, flow_out; 1: row > col, flow_in; self
 * loops are in neither), for every node n < n_nodes:
 *   AGG[n][0 .. dn)      = agg over j in [seg_ptr[N + n], seg_ptr[N + n + 1]) of M[j][:]          (flow_in)
 *   AGG[n][dn .. 2 dn)   = agg over j in [seg_ptr[n], seg_ptr[n + 1]) of M[j][:]                  (flow_out)
 *       agg = MPNHIP_AGG_SUM: the sum in ascending j; _MEAN: that sum times 1 / max(count, 1); _MAX: the maximum; an empty segment
 *       gives 0 with all three
 *   x_new[n][o]          = max(sum_{k < 2 dn} Wu[o][k] AGG[n][k] + bu[o], 0)                       o < dn
 *   P_next[n][p]         = P0[n][p] + sum_{k < dn} Wnode[p][dn + k] x_new[n][k]                    p < pw
 * M [E, dn] in SORTED edge order; Wu [dn, 2 dn], bu [dn]; Wnode [pw, 2 dn]: the packed projection weights, of which only the
 * current-feature columns [dn, 2 dn) are read; P0, P_next [N, pw]; x_new [N, dn]; agg_out [N, 2 dn] receives AGG.  P_next (the last
 * step has none; P0 may then be NULL too) and agg_out (inference) may each be NULL.  Both products take their fp32 operands as three
 * bf16 pieces (MPNHIP_PREC_FP32_SPLIT): nothing is rounded to bf16; AGG is stored as the fp32 value that is multiplied, and
 * P_next is computed from the fp32 x_new that is stored.  Nothing but rows [0, N) of the three outputs is written.
 * workspace: mpnhip_debug_node_chain_workspace_bytes(dn, pw) bytes (the weight images; 0: widths the kernel does not take).
 * Checked on the host before any launch: negative sizes, an unknown agg, a null graph (MPNHIP_ERR_ARG); widths other than
 * dn in {64, 128} with pw a positive multiple of 32 (MPNHIP_ERR_UNSUPPORTED); then, with n_nodes > 0 (n_nodes == 0 is a successful
 * no-op): null Wu / bu / Wnode / x_new, null M with edges, P_next without P0, a pointer among M, bu, P0, x_new, P_next, agg_out or
 * the workspace that is not 16-byte aligned (MPNHIP_ERR_ARG); a null or short workspace (MPNHIP_ERR_WORKSPACE).  A successful call
 * with nodes adds 1 to the path counter "node_chain" and to no other. */
size_t mpnhip_debug_node_chain_workspace_bytes(int dn, int pw);
int mpnhip_debug_node_chain(const void* graph_buf, int n_nodes, int64_t n_edges, const float* M, int dn, int pw, int agg,
                            const float* Wu, const float* bu, const float* Wnode, const float* P0, float* x_new, float* P_next,
                            float* agg_out, void* workspace, size_t workspace_bytes, void* stream);

/* Test instrumentation: ONE launch of the node side of a backward step (csrc/node_chain.hip: node_chain_bwd_kernel; what
 * mpnhip_backward runs between two steps in MPNHIP_PREC_FP32_SPLIT at dn = 64 / 128), through pack_node_chain_bwd and
 * launch_node_chain_bwd.  For every node n < n_nodes:
 *   dX[n][k]    = sum_{p < pw} dP[n][p] Wnode[p][dn + k]                                           k < dn
 *   dZn[n][k]   = x_prev[n][k] > 0 ? dX[n][k] : 0
 *   dAGG[n][c]  = sum_{k < dn} dZn[n][k] Wu[k][c]                                                  c < 2 dn
 * dP [N, pw]: the gradient of a step's projections; x_prev [N, dn]: the output of the previous step's node update, read only for
 * its sign (a NaN counts as not positive); Wnode [pw, 2 dn] and Wu [dn, 2 dn] as above; outputs dZn [N, dn] and dAGG [N, 2 dn], rows
 * [0, N) only.  Three-piece operands as above; dAGG is computed from the fp32 dZn that is stored.
 * workspace: mpnhip_debug_node_chain_backward_workspace_bytes(dn, pw) bytes (0: widths the kernel does not take).
 * Checked on the host before any launch: negative sizes (MPNHIP_ERR_ARG); widths other than dn in {64, 128} with pw >= 64 a multiple
 * of 16 (MPNHIP_ERR_UNSUPPORTED); then, with n_nodes > 0: a null pointer, a pointer among dP, x_prev, dZn, dAGG or the workspace
 * that is not 16-byte aligned (MPNHIP_ERR_ARG); a null or short workspace (MPNHIP_ERR_WORKSPACE).  A successful call with nodes adds
 * 1 to the path counter "node_chain_bwd" and to no other. */
size_t mpnhip_debug_node_chain_backward_workspace_bytes(int dn, int pw);
int mpnhip_debug_node_chain_backward(int n_nodes, const float* dP, int dn, int pw, const float* x_prev, const float* Wnode,
                                     const float* Wu, float* dZn, float* dAGG, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Graph preparation -- replaces the six boolean-mask indexings per step of
 * TimeAwareNodeModel.forward (models/mpn.py:85-87,91-93) and the implicit index structures behind
 * torch_scatter / index_put_.  Done once per edge_index, reused by all steps, forward and backward.
 *
 * edge_index: int64 [2,E] row-major (row = edge_index[0], col = edge_index[1]), as the reference's
 * Graph.edge_index (data/mot_graph.py:312).  Edges are stably sorted by (direction, row) with
 * direction 0 = row<col (flow_out), 1 = row>col (flow_in), 2 = row==col (in neither aggregate,
 * mpn.py:85,91).  The prepared graph lives in `graph_buf` (mpnhip_graph_bytes) and is opaque.
 * Out-of-range indices set an error flag readable with mpnhip_graph_status (which synchronises).
 * ------------------------------------------------------------------------------------------- */
size_t mpnhip_graph_bytes(int n_nodes, int64_t n_edges);
size_t mpnhip_graph_prep_workspace_bytes(int n_nodes, int64_t n_edges);
int mpnhip_graph_prep(const int64_t* edge_index, int n_nodes, int64_t n_edges, void* graph_buf, size_t graph_bytes,
                      void* workspace, size_t workspace_bytes, void* stream);
/* The primary (direction, row) order only -- all that mpnhip_forward / mpnhip_meta_layer_forward / the forward of
 * mpnhip_attention_aggregate read (a quarter of the sorting work; sliding-window inference prepares a graph per window).
 * mpnhip_backward, mpnhip_attention_aggregate_backward and mpnhip_step_metrics need mpnhip_graph_prep. */
int mpnhip_graph_prep_forward(const int64_t* edge_index, int n_nodes, int64_t n_edges, void* graph_buf, size_t graph_bytes,
                              void* workspace, size_t workspace_bytes, void* stream);
/* Synchronising debug helper: host copy of {error_flag, E_flow_out, E_flow_in, E_self}. */
int mpnhip_graph_status(const void* graph_buf, int n_nodes, int64_t n_edges, int32_t status[4], void* stream);

/* ---------------------------------------------------------------------------------------------
 * MOTMPNet.forward hot path (models/mpn.py:349-392 minus the x_ext / mask lines): encoder, then
 * num_enc_steps x { reattach (:369-373), MetaLayer (:376 -> :33-54), classifier (:377 -> :114) }.
 *
 * x         [N, enc_node.in_dim]   node inputs after the avg-pool of mpn.py:351-352
 * edge_attr [E, enc_edge.in_dim]   in edge_index order
 * logits    [max(L,1), E]          OUT: classifier output of EVERY step, edge_index order (the
 *                                  reference's classified_edges are the last num_class_steps rows)
 * x_out [N,dn], e_out [E,de]       OUT, optional (NULL): final latent node / edge features
 * save_for_backward != 0 keeps every step's activations in `workspace` for mpnhip_backward.
 * ------------------------------------------------------------------------------------------- */
size_t mpnhip_forward_workspace_bytes(const mpnhip_model* model, int n_nodes, int64_t n_edges, int save_for_backward);
int mpnhip_forward(const mpnhip_model* model, const void* graph_buf, int n_nodes, int64_t n_edges, const float* x,
                   const float* edge_attr, float* logits, float* x_out, float* e_out, void* workspace,
                   size_t workspace_bytes, int save_for_backward, void* stream);

/* Autograd of the above (what torch.autograd derives for mpn.py:349-392).
 * grad_logits [max(L,1), E] incoming gradient for every step's logits (zeros where unused);
 * grad_x_out / grad_e_out optional incoming gradients for the final latents (NULL = 0);
 * grad_x [N, enc_node.in_dim], grad_edge_attr [E, enc_edge.in_dim]: OUT, optional (overwritten).
 * Parameter gradients are accumulated into model->*.grad_weight / grad_bias.
 * `workspace` must be the buffer the matching forward ran with save_for_backward = 1. */
size_t mpnhip_backward_workspace_bytes(const mpnhip_model* model, int n_nodes, int64_t n_edges);
int mpnhip_backward(const mpnhip_model* model, const void* graph_buf, int n_nodes, int64_t n_edges, const float* x,
                    const float* edge_attr, const float* grad_logits, const float* grad_x_out,
                    const float* grad_e_out, float* grad_x, float* grad_edge_attr, void* fwd_workspace,
                    size_t fwd_workspace_bytes, void* bwd_workspace, size_t bwd_workspace_bytes, void* stream);

/* Data-parallel training: the same backward with flags.  MPNHIP_BWD_DEFER_SIDE_JOIN: when the
 * backward runs its weight-gradient groups on the library's side stream (mpnhip_backward_uses_side_stream(model) == 1: four
 * or more steps), do NOT make `stream` wait for that stream before returning.  On return the gradients of the message-passing
 * modules and of the classifier are complete in SIDE-stream order, the encoder's gradients and grad_x / grad_edge_attr in
 * `stream` order: the trainer enqueues the all-reduce of the first bucket on mpnhip_side_stream() -- it then overlaps the
 * encoder's backward -- and joins with mpnhip_side_stream_join(stream) (or its collective's own wait) before it reads them. */
#define MPNHIP_BWD_DEFER_SIDE_JOIN 1
int mpnhip_backward_flags(const mpnhip_model* model, const void* graph_buf, int n_nodes, int64_t n_edges, const float* x,
                          const float* edge_attr, const float* grad_logits, const float* grad_x_out, const float* grad_e_out,
                          float* grad_x, float* grad_edge_attr, void* fwd_workspace, size_t fwd_workspace_bytes,
                          void* bwd_workspace, size_t bwd_workspace_bytes, int flags, void* stream);
int mpnhip_backward_uses_side_stream(const mpnhip_model* model);
void* mpnhip_side_stream(void);              /* hipStream_t of the current device's side stream (created on first use) */
int mpnhip_side_stream_join(void* stream);   /* `stream` waits for everything enqueued on the side stream so far */

/* ---------------------------------------------------------------------------------------------
 * Operator level.
 * ------------------------------------------------------------------------------------------- */

/* MetaLayer.forward(x, edge_index, edge_attr) -> (x', e')  (models/mpn.py:33-54) with
 * x [N, nf*dn], e [E, ef*de] (already re-attached, edge_index order); x_new [N,dn], e_new [E,de].
 * Only model->edge / flow_in / flow_out / node and dn, de, agg, reattach_* are read. */
size_t mpnhip_meta_layer_workspace_bytes(const mpnhip_model* model, int n_nodes, int64_t n_edges);
int mpnhip_meta_layer_forward(const mpnhip_model* model, const void* graph_buf, int n_nodes, int64_t n_edges,
                              const float* x, const float* e, float* x_new, float* e_new, void* workspace,
                              size_t workspace_bytes, void* stream);

/* node_agg_fn(out, row, x_size) (models/mpn.py:266-273): out[i] = AGG over {j : row[j] == i} src[j];
 * src [M, dim], row int64 [M] (any order), out [x_size, dim]; empty -> 0; max returns values only.
 * argmax (optional, int32 [x_size, dim]): for MAX the source row chosen (first maximum in index
 * order, -1 for empty segments), as torch_scatter's CPU kernel picks it. */
size_t mpnhip_segment_reduce_workspace_bytes(int64_t m, int x_size);
int mpnhip_segment_reduce(const float* src, const int64_t* row, int64_t m, int dim, int x_size, int agg, float* out,
                          int32_t* argmax, void* workspace, size_t workspace_bytes, void* stream);

/* y = act(x W^T + b): one layer of models/mlp.py (nn.Linear + optional ReLU).
 * x [M,K] (row stride ldx), w [N,K], b [N] or NULL, y [M,N] (row stride ldy). */
int mpnhip_linear(const float* x, int64_t ldx, const float* w, const float* b, float* y, int64_t ldy, int64_t m, int n,
                  int k, int relu, void* stream);

/* One nn.Linear (+ ReLU) of models/mlp.py:27 in BASELINE.json's configs[4] arithmetic -- what mpnhip_forward / mpnhip_backward run
 * for the node-side products of models/mpn.py:69,87,93,97-99 when mpnhip_model.precision == MPNHIP_PREC_BF16 (round 5: the 128 x 128
 * tiled kernel, csrc/gemm_bf16.hip):
 *     y[m][n] = mask( act( sum_k bf16(xcat[m][k]) * bf16(w[n][k]) + b[n] + c_in[m][n] ) (+ y[m][n]) ),  fp32 accumulation,
 * xcat = [x | x2] (torch.cat of the re-attached initial and the current features, mpn.py:369-373, never materialised).
 * Operands are fp32 rows rounded to bf16 (RNE) as they are staged, or ALREADY bf16 rows in memory (x_bf16 / w_bf16 != 0: the
 * pointers are bfloat16 bit patterns, leading dims count elements; K, ksplit and the leading dims multiples of 8, 16-byte bases).
 * b, c_in, mask (value kept where mask > 0), x2 and y16 (a bf16 mirror of the result) may be NULL.  n % 4 == 0, k % 4 == 0. */
typedef struct mpnhip_linear_bf16_args {
    const void* x;  int64_t ldx;        /* [m, ksplit] */
    const void* x2; int64_t ldx2;       /* [m, k - ksplit] or NULL (then ksplit == k) */
    const void* w;  int64_t ldw;        /* [n, k] */
    const float* b;                     /* [n] */
    const float* c_in; int64_t ldc_in;  /* [m, n] added before the activation */
    const float* mask; int64_t ldmask;  /* [m, n] */
    float* y; int64_t ldy;              /* [m, n] */
    uint16_t* y16; int64_t ldy16;       /* [m, n] bf16 mirror of y */
    int64_t m;
    int n, k, ksplit;
    int x_bf16, w_bf16, relu, accumulate;
} mpnhip_linear_bf16_args;
int mpnhip_linear_bf16(const mpnhip_linear_bf16_args* args, void* stream);
/* dst[i] = bf16(src[i]) (round to nearest even; NaN stays NaN): the packed weight images / feature mirrors of that mode. n % 4 == 0. */
int mpnhip_to_bf16(const float* src, uint16_t* dst, int64_t n, void* stream);

/* The weight / bias gradient autograd derives for one nn.Linear of models/mlp.py, batched over the
 * message-passing steps that share the weight:  grad_w[o][c] += sum_b sum_m dZ[b][m][o] * H[b][m][c],  grad_b[o] += sum dZ[b][m][o].
 * dZ [nbatch][rows][n_out] (gradient at the layer's pre-activation), H [nbatch][rows][k_in] (the layer's input), both dense
 * row-major; grad_w [n_out][k_in], grad_b [n_out] or NULL.  Fixed summation order (no float atomics): bitwise reproducible. */
size_t mpnhip_weight_grad_workspace_bytes(int n_out, int k_in, int64_t rows, int nbatch);
int mpnhip_weight_grad(const float* dZ, const float* H, int64_t rows, int n_out, int k_in, int nbatch, float* grad_w, float* grad_b,
                       void* workspace, size_t workspace_bytes, void* stream);
/* The same with the operand form chosen: MPNHIP_PREC_FP32 (fp32 MFMAs; what mpnhip_weight_grad does) or MPNHIP_PREC_FP32_SPLIT
 * (every fp32 operand as the exact sum of three bf16 pieces, six piece products with fp32 accumulate: the same accuracy class;
 * what mpnhip_backward uses for a model in that precision). */
int mpnhip_weight_grad_prec(const float* dZ, const float* H, int64_t rows, int n_out, int k_in, int nbatch, int precision, float* grad_w,
                            float* grad_b, void* workspace, size_t workspace_bytes, void* stream);
/* The same product over operands that are ALREADY bf16 rows in memory (round 4: what the bf16-operand training path keeps -- the
 * backward chain kernel's dZ blocks, the forward chain kernel's saved activations; mlp.py:27-28 under autograd in BASELINE.json's
 * configs[4] arithmetic): dZ [nbatch][rows][n_out], H [nbatch][rows][k_in] as bfloat16 bit patterns, n_out and k_in multiples of 4
 * (or a narrow shape, k_in <= 32 and n_out <= 32), fp32 accumulation; grad_w / grad_b fp32, "+=". */
size_t mpnhip_weight_grad_bf16_rows_workspace_bytes(int n_out, int k_in, int64_t rows, int nbatch);
int mpnhip_weight_grad_bf16_rows(const uint16_t* dZ, const uint16_t* H, int64_t rows, int n_out, int k_in, int nbatch, float* grad_w,
                                 float* grad_b, void* workspace, size_t workspace_bytes, void* stream);

/* The gradient of node_agg_fn (models/mpn.py:266-273; torch_scatter's scatter_add / scatter_mean / scatter_max backward), gather
 * form: grad_src[j] = grad_out[row[j]] (sum), / count[row[j]] (mean; count int32 [x_size]), or only where argmax[row[j]][d] == j
 * (max; `argmax` as mpnhip_segment_reduce returned it).  grad_out [x_size, dim], grad_src [M, dim].  A row[j] outside
 * [0, x_size) contributed nothing to the forward (mpnhip_segment_reduce parks it behind the last segment): its grad_src row
 * is written as 0 and grad_out / count / argmax are not read for it. */
int mpnhip_segment_reduce_backward(const float* grad_out, const int64_t* row, const int32_t* argmax, const int32_t* count, int64_t m,
                                   int dim, int x_size, int agg, float* grad_src, void* stream);

/* nn.BatchNorm1d (TRAINING mode: batch statistics) -> nn.ReLU -> nn.Dropout as models/mlp.py:12-23 stacks them behind each
 * nn.Linear, and their gradients -- the layer-by-layer training path of a model built with use_batchnorm / dropout_p
 * (mpntrackseg_amd/modular.py; no shipped configuration enables them, configs/tracking_cfg.yaml:150-167; in eval mode BatchNorm
 * folds into the Linear layers and the fused path runs).  z [M, N] dense = the Linear's output.
 *   forward : use_bn: mean / biased variance over the M rows (two passes), y = relu(gamma (z - mean) invstd + beta) keep / (1 - p);
 *             running_mean / running_var (may be NULL) updated like nn.BatchNorm1d (momentum, unbiased variance); save_mean /
 *             save_invstd [N] receive the batch statistics for the backward.  M == 1 with use_bn is refused like torch does.
 *             keep(r, c) = hash(seed, r N + c) >= p: the backward regenerates it from the same seed, nothing is stored.
 *   backward: dz [M, N], dgamma / dbeta [N] (may be NULL; written, not accumulated).
 * Column sums in a fixed order (no float atomics): bitwise reproducible.  workspace: mpnhip_bn_dropout_workspace_bytes. */
size_t mpnhip_bn_dropout_workspace_bytes(int64_t m, int n);
int mpnhip_bn_relu_dropout_forward(const float* z, int64_t m, int n, int use_bn, const float* gamma, const float* beta,
                                   float* running_mean, float* running_var, float momentum, float eps, int relu, float dropout_p,
                                   uint64_t seed, float* y, float* save_mean, float* save_invstd, void* workspace,
                                   size_t workspace_bytes, void* stream);
int mpnhip_bn_relu_dropout_backward(const float* dy, const float* z, int64_t m, int n, int use_bn, const float* gamma,
                                    const float* beta, const float* save_mean, const float* save_invstd, int relu, float dropout_p,
                                    uint64_t seed, float* dz, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes,
                                    void* stream);

/* MLP.forward (models/mlp.py:27-28): all layers; scratch [2, M, max(out_dims)] floats. */
size_t mpnhip_mlp_workspace_bytes(const mpnhip_mlp* mlp, int64_t m);
int mpnhip_mlp_forward(const mpnhip_mlp* mlp, const float* x, float* y, int64_t m, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The callers' next step, device side, no host sync.
 * ------------------------------------------------------------------------------------------- */

/* Tracking term of MOTNeuralSolver._compute_loss (pl_module/pl_module.py:88-107):
 *   loss = weight * sum_{s >= first_step} BCEWithLogits(logits[s], labels, pos_weight = #neg / #pos), mean over edges.
 * logits [n_steps, E] (every step, as mpnhip_forward returns them), labels [E] in {0,1} (edge_index order),
 * first_step = num_enc_steps - num_class_steps (steps before it carry no loss).
 * loss_out [1 + n_steps] (device): total, then per step.  grad_logits [n_steps, E]: d loss / d logits (zeros for
 * the unclassified steps) -- exactly the grad_logits argument of mpnhip_backward. */
size_t mpnhip_tracking_loss_workspace_bytes(int n_steps, int64_t n_edges);
int mpnhip_tracking_loss(const float* logits, const float* labels, int n_steps, int64_t n_edges, int first_step,
                         float weight, float* loss_out, float* grad_logits, void* workspace, size_t workspace_bytes,
                         void* stream);

/* The same loss over the n_graphs graphs of ONE block-diagonal batch (torch_geometric's Batch; edge_graph[e] = graph of edge e, int32,
 * edge_index order): every graph its own pos_weight and its own mean, as the reference computes them graph by graph with
 * batch_size 1, and the n_graphs losses AVERAGED -- what accumulate_grad_batches = n_graphs backward passes add up to
 * (configs/tracking_cfg.yaml:3-4, pl_module.py:88-107).  loss_out [1 + n_steps]; grad_logits [n_steps, E]. */
size_t mpnhip_tracking_loss_graphs_workspace_bytes(int n_steps, int64_t n_edges, int n_graphs);
int mpnhip_tracking_loss_graphs(const float* logits, const float* labels, const int32_t* edge_graph, int n_graphs, int n_steps,
                                int64_t n_edges, int first_step, float weight, float* loss_out, float* grad_logits, void* workspace,
                                size_t workspace_bytes, void* stream);

/* compute_perform_metrics (utils/evaluation.py:416-437) on the last step's logits [E] (edge_index order):
 * counts[0..3] = TP, FP, TN, FN of (logit > 0) vs labels (fast_compute_class_metric, :340-366);
 * counts[4..5] = nodes whose outgoing / incoming flow exceeds 1, counts[6..7] = nodes that have an outgoing /
 * incoming constraint (compute_constr_satisfaction_rate, :370-414, undirected_edges = True).
 * counts: int32[8] on the device; the caller reads them back when it wants the ratios. */
int mpnhip_step_metrics(const void* graph_buf, int n_nodes, int64_t n_edges, const float* logits, const float* labels,
                        int32_t* counts, void* stream);

/* The same eight counts for each graph of ONE block-diagonal batch (a batch is n_graphs reference steps executed in space, so
 * validation_epoch_end's means need them graph by graph): counts [n_graphs, 8] int32, row g = {TP, FP, TN, FN, viol_out, viol_in,
 * constr_out, constr_in} as above, over the edges with edge_graph[e] == g and the nodes with node_graph[n] == g (int32, edge_index /
 * node order).  n_graphs in [1, 1024]; with n_graphs == 1 both id arrays may be NULL (every edge and node is graph 0).  An id outside
 * [0, n_graphs) is counted nowhere and writes nowhere; labels other than 0 / 1 fall in no confusion cell.  Integer counts: exact and
 * independent of the order.  No workspace, nothing read back. */
int mpnhip_step_metrics_graphs(const void* graph_buf, int n_nodes, int64_t n_edges, const float* logits, const float* labels,
                               const int32_t* edge_graph, const int32_t* node_graph, int n_graphs, int32_t* counts /* [n_graphs, 8] */,
                               void* stream);

/* MOTGraph.assign_edge_labels (data/mot_graph.py:223-262): labels [E] float32 in {0, 1} from edge_index (int64 [2, E]) and the
 * track id of every node (ids, int64 [N]; -1 = no track).  same_id = ids[row] == ids[col] && ids[row] != -1.
 *   MPNHIP_LABELS_ALL:      label = same_id;
 *   MPNHIP_LABELS_CLOSEST:  label = same_id && (col is the smallest col > row, or the largest col < row, over the same-id EDGES of
 *                           that row) -- what the reference's scatter_min over |row - col| selects; stored duplicates of the active
 *                           edge are all labelled, a self loop never is.
 * Integer atomics only: the same bits on every call.  An endpoint outside [0, N) is never used as an index: its edge gets label 0
 * and *status (one device int32, overwritten) becomes non-zero -- the reference's gather raises IndexError there.
 * workspace: 2 N ints ('closest' only).  Nothing is read back; n_edges == 0 is a successful no-op. */
#define MPNHIP_LABELS_ALL 0
#define MPNHIP_LABELS_CLOSEST 1
size_t mpnhip_edge_labels_workspace_bytes(int64_t n_nodes);
int mpnhip_edge_labels(const int64_t* edge_index, int64_t n_edges, const int64_t* ids, int64_t n_nodes, int mode, float* labels,
                       int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* Segmentation term of MOTNeuralSolver._compute_loss (pl_module/pl_module.py:108-118):
 *   loss = weight * sum_s mean over the valid rows and their row_floats elements of BCEWithLogits(preds[s], labels).
 * preds / grads: HOST arrays of n_steps device pointers (n_steps <= 16; the kernel takes them by value), each [N, row_floats]
 * contiguous; labels [N, row_floats] (any float in [0, 1]); valid [N] bytes (non-zero = the row has a ground-truth mask).
 * grads[s] is written in full: (sigmoid(z) - y) * weight / (n_valid * row_floats) on valid rows, 0 on the others.
 * loss_out [1 + n_steps] (device): total, then per step.  No valid row: loss 0, gradients 0.
 * node_graph (int32 [N], optional) with n_graphs (1 .. 1024): the rows belong to the graphs of one block-diagonal batch -- every
 * graph its own mean over its own valid rows, a graph without one contributes nothing, the n_graphs losses averaged (as
 * mpnhip_tracking_loss_graphs).  Without it n_graphs must be 1.
 * All steps run in ONE launch; 16-byte accesses when every base pointer and row_floats allow them, 4-byte ones otherwise.
 * Per-block partial sums are added in double in a fixed order, and which elements a thread sums depends on row_floats alone:
 * the loss is bitwise reproducible, also between differently aligned copies of the same tensors.  No host read. */
size_t mpnhip_mask_loss_workspace_bytes(int n_steps, int64_t n_nodes, int64_t row_floats, int n_graphs);
int mpnhip_mask_loss(const float* const* preds, int n_steps, const float* labels, const uint8_t* valid, const int32_t* node_graph,
                     int n_graphs, int64_t n_nodes, int64_t row_floats, float weight, float* loss_out, float* const* grads,
                     void* workspace, size_t workspace_bytes, void* stream);

/* Mask branch: the neighbour aggregation of TimeAwareAttentionModel.forward
 * (models/mpn.py:117-134): per (node, direction) segment w = scatter_softmax(logits) and
 * out_dir[n] = sum_j w_j x[col_j], x [N, feat] with feat = C*H*W (64*14*14).  logits [E] in edge_index order (the
 * classifier output of this step); out_in / out_out [N, feat] (flow_in: row > col, flow_out: row < col);
 * weights [E] (sorted edge order, optional) keeps w for the backward. */
int mpnhip_attention_aggregate(const void* graph_buf, int n_nodes, int64_t n_edges, const float* x, int64_t feat,
                               const float* logits, float* out_in, float* out_out, float* weights, void* stream);
/* Its autograd: grad_x [N, feat] (overwritten, or += when accumulate_grad_x) and grad_logits [E] (+=, edge_index
 * order) from grad_in / grad_out [N, feat]; workspace_dw: E floats. */
int mpnhip_attention_aggregate_backward(const void* graph_buf, int n_nodes, int64_t n_edges, const float* x, int64_t feat,
                                        const float* weights, const float* grad_in, const float* grad_out, float* grad_x,
                                        int accumulate_grad_x, float* grad_logits, float* workspace_dw, void* stream);

/* nn.AdaptiveAvgPool2d((1,1)) + view (models/mpn.py:252,351-352): x [rows, hw] -> y [rows] = mean over
 * the hw contiguous spatial positions (rows = N * C). */
int mpnhip_avgpool(const float* x, int64_t rows, int hw, float* y, void* stream);

/* Mask branch, inference: the convolution-type layers of models/cnn.py and MaskModel (models/mpn.py:180-206) without autograd.
 * Everything is NCHW fp32; products are exact fp32 with fp32 accumulation in a fixed k order (input channel, then tap), one
 * block per (image, output tile, output-channel group): a pixel's value does not depend on how many images the call holds or
 * where its image sits among them.  No workspace.
 *
 * The input is the channel-wise concatenation of n_segments (1 .. MPNHIP_CONV_MAX_SEGMENTS) tensors that is never
 * materialised: segment s holds seg_channels[s] channels of every image, image i at seg_data[s] + i * seg_stride[s] (floats),
 * channels and pixels dense behind it ([channels][H][W]).  The output image i starts at out + i * out_stride (floats) and is
 * dense [cout][Hout][Wout]: a stride wider than that writes a channel slice of a wider tensor and leaves the rest alone.
 *
 *   transposed == 0: nn.Conv2d(cin, cout, ksize, stride 1, padding ksize / 2), ksize 1 or 3; weight [cout][cin][ksize][ksize];
 *                    Hout = H, Wout = W.  cout <= 8 takes a plain (non-MFMA) kernel with the same summation order.
 *   transposed != 0: nn.ConvTranspose2d(cin, cout, 2, stride 2, padding 0), ksize must be 2; weight [cin][cout][2][2];
 *                    Hout = 2 H, Wout = 2 W.
 * bias [cout] or NULL (no bias); relu != 0: max(., 0) at the end.
 *
 * Checked on the host before any launch (MPNHIP_ERR_ARG): null args; n_images < 0; (n_images == 0 is a successful no-op, nothing
 * else is looked at;) n_segments outside 1 .. 4; a segment with a null pointer, no channels or a negative stride; H, W or
 * cout < 1; a kernel size other than the ones above; null weight or out; and any stride, image size (cin * H * W,
 * cout * Hout * Wout) or weight count beyond INT32_MAX -- the kernels index inside an image with 32 bits. */
#define MPNHIP_CONV_MAX_SEGMENTS 4
typedef struct mpnhip_conv_args {
    const float* seg_data[4]; int64_t seg_stride[4]; int seg_channels[4]; int n_segments;
    int H; int W; int cout; int ksize; int transposed; int relu;
    int64_t n_images; const float* weight; const float* bias; float* out; int64_t out_stride;
} mpnhip_conv_args;
int mpnhip_conv2d_forward(const mpnhip_conv_args* args, void* stream);

/* Mask branch, training: the backward of ONE nn.Conv2d(cin, cout, ksize, stride 1, padding ksize / 2), ksize 1 or 3, with the
 * ReLU that mpnhip_conv2d_forward fuses behind it (relu != 0).  Exact fp32 products, fp32 accumulation, no float atomics: every
 * sum has a fixed order that depends on the layer and on n_images alone, so two calls on the same inputs agree bit for bit.
 *
 * Inputs: the segment list of the forward (the layer's input), weight [cout][cin][ksize][ksize], the layer's output y (image i at
 * y + i * y_stride, dense [cout][H][W]; read only when relu != 0) and grad_out (image i at grad_out + i * grad_out_stride,
 * dense [cout][H][W]).  Outputs, each may be NULL ("not needed") and each is OVERWRITTEN, never accumulated into:
 *   grad_in     [n_images][cin][H][W], dense: the gradient of the channel concatenation; segment s owns the channel slice behind
 *               the channels of segments 0 .. s - 1.
 *   grad_weight [cout][cin][ksize][ksize]
 *   grad_bias   [cout]
 *
 *   g = grad_out * [y > 0] (relu; torch's ReLU backward: nothing at y == 0), else g = grad_out.  A pre-pass writes g once into the
 *       workspace and sums it per (block of 8 images, channel); grad_bias adds those partial sums in block order.
 *   grad_in = conv2d(g, W') with W'[c][m][ky][kx] = W[m][c][k-1-ky][k-1-kx], built in the workspace, through
 *       mpnhip_conv2d_forward itself (its small-cout kernel when cin <= 8): an image's bits do not depend on the batch.
 *       Skipped when grad_in is NULL.
 *   grad_weight[m][c][tap] = sum over images and pixels of g[m][n][p] * x[c][n][p + tap offset]: one block per (<= 128 rows of
 *       cout, 32 input channels, 8 images) on v_mfma_f32_32x32x2_f32 with the pixel as k, partial sums [split][cout][cin * taps]
 *       in the workspace, added in split order by a second kernel.  cout <= 8: a plain kernel, the same two stages.
 *
 * MPNHIP_ERR_ARG before any launch: everything mpnhip_conv2d_forward refuses (with grad_in's image in the place of out),
 * transposed != 0, relu with a null y, a null grad_out, all three outputs NULL, y_stride / grad_out_stride outside the 32-bit
 * range, a null workspace or one smaller than mpnhip_conv2d_backward_workspace_bytes(args), more images than one launch holds.
 * n_images == 0 (checked like any other call) zero-fills grad_weight / grad_bias where given and touches nothing else.
 * mpnhip_conv2d_backward_workspace_bytes: 0 for arguments the operator refuses. */
typedef struct mpnhip_conv_bwd_args {
    const float* seg_data[4]; int64_t seg_stride[4]; int seg_channels[4]; int n_segments;
    int H; int W; int cout; int ksize; int transposed; int relu;
    int64_t n_images; const float* weight; const float* y; int64_t y_stride; const float* grad_out; int64_t grad_out_stride;
    float* grad_in; float* grad_weight; float* grad_bias;
} mpnhip_conv_bwd_args;
size_t mpnhip_conv2d_backward_workspace_bytes(const mpnhip_conv_bwd_args* args);
int mpnhip_conv2d_backward(const mpnhip_conv_bwd_args* args, void* workspace, size_t workspace_bytes, void* stream);

/* Mask branch, training: the backward of ONE nn.ConvTranspose2d(cin, cout, 2, stride 2, padding 0) with the ReLU that
 * mpnhip_conv2d_forward (transposed != 0) fuses behind it.  The same args struct as mpnhip_conv2d_backward, read as follows:
 * transposed must be non-zero and ksize 2; H, W are the INPUT size; the segment list is the layer's input ([channels][H][W] per
 * image); weight and grad_weight are [cin][cout][2][2]; y and grad_out are dense [cout][2 H][2 W] per image at y_stride /
 * grad_out_stride; grad_in is dense [n_images][cin][H][W] over the channel concatenation of the segments; grad_bias [cout].
 * Outputs may be NULL and are overwritten, never accumulated into.  Exact fp32 products, fp32 accumulation, no float atomics:
 * every sum has an order fixed by the layer's shape and n_images alone.
 *
 * Stride equals kernel size, so no two taps meet in one output pixel and the layer is a 1 x 1 product in a space-to-depth layout:
 *   pre-pass    g = grad_out * [y > 0] (relu) or grad_out, written once into the workspace as g'[n][4 m + 2 dy + dx][h][w] =
 *               g[n][m][2 h + dy][2 w + dx]: 4 cout channels at H x W.  The same kernel sums g per (block of 8 images, channel m);
 *               grad_bias adds those partial sums in block order.
 *   grad_in     [n][c][h][w] = sum over (m, dy, dx) of g'[n][(m, dy, dx)][h][w] * W[c][m][dy][dx]: the weight as stored is the
 *               weight [cin][4 cout] of a 1 x 1 Conv2d from g' to the input, so this is mpnhip_conv2d_forward (ksize 1) on g'
 *               with the weight pointer itself -- an image's bits do not depend on the batch.  Skipped when grad_in is NULL.
 *   grad_weight [c][(m, dy, dx)] = sum over images and pixels of x[n][c][p] * g'[n][(m, dy, dx)][p]: a 1 x 1 weight-gradient
 *               product with its rows from the layer's input and its columns from g', so its output layout is this weight's: one
 *               block per (32 rows, 64 columns, 8 images) on v_mfma_f32_32x32x2_f32 with the pixel as k (cin <= 8: the plain
 *               kernel of mpnhip_conv2d_backward with the roles swapped); partial sums added in split order.  The row operand is
 *               one dense tensor: more than one input segment is first gathered into the workspace.
 *
 * Workspace (floats, every region padded to 256 bytes), with splits = ceil(n_images / 8):
 *   g' [n_images][4 cout][H W] | the gathered input [n_images][cin][H W] (only when n_segments > 1) |
 *   weight partial sums [splits][cin][4 cout] | bias partial sums [splits][cout]
 *
 * MPNHIP_ERR_ARG before any launch, the message starting with the entry point's name: what mpnhip_conv2d_backward refuses, with
 * transposed == 0 and ksize != 2 in the place of its kernel-size rules.  n_images == 0 zero-fills grad_weight / grad_bias where
 * given and touches nothing else.  mpnhip_conv_transpose2d_backward_workspace_bytes: 0 for arguments the operator refuses. */
size_t mpnhip_conv_transpose2d_backward_workspace_bytes(const mpnhip_conv_bwd_args* args);
int mpnhip_conv_transpose2d_backward(const mpnhip_conv_bwd_args* args, void* workspace, size_t workspace_bytes, void* stream);

/* nn.LayerNorm over the trailing [C][H][W] of every image (MaskModel.layer_norm), elementwise affine of that same shape:
 * out = (x - mean) / sqrt(var + eps) * weight + bias with the biased variance of the centred values (two passes: the mean first).
 * The input is a segment list as above (C = the sum of seg_channels, hw = H * W), weight / bias [C * hw] (both or neither may
 * be NULL: no affine), out image i at out + i * out_stride.  Refusals as for the convolution: null lists, n_segments outside
 * 1 .. 4, null / empty segments, hw < 1, eps < 0 or not finite, null out, sizes or strides beyond INT32_MAX; n_images == 0 is
 * a successful no-op. */
int mpnhip_layer_norm_forward(const float* const* seg_data, const int64_t* seg_stride, const int* seg_channels, int n_segments,
                              int64_t n_images, int64_t hw, const float* weight, const float* bias, float eps, float* out,
                              int64_t out_stride, void* stream);

/* The backward of mpnhip_layer_norm_forward over the same segment list.  weight [C * hw] or NULL (no affine: gamma = 1; the call
 * computes grad_in only, and a grad_weight or grad_bias handed to it is refused); grad_out image i at grad_out + i *
 * grad_out_stride, dense [C * hw].  Outputs, each may be NULL (all three NULL is refused), each overwritten:
 *   grad_in     [n_images][C * hw], dense: segment s owns the channel slice behind the channels of segments 0 .. s - 1
 *   grad_weight [C * hw], grad_bias [C * hw]
 * Per image (one block, like the forward): mean and rstd are recomputed with the forward's own two passes and block sums -- the
 * same order, hence the same bits --, then a = sum g_i gamma_i and b = sum g_i gamma_i xhat_i as fixed-order block sums and
 * grad_in_i = rstd * (g_i gamma_i - a / F - xhat_i * b / F), F = C * hw: an image's grad_in does not depend on the batch.
 * Per element: grad_weight_i = sum_n g[n][i] * xhat[n][i], grad_bias_i = sum_n g[n][i] as partial sums over blocks of 8 images
 * (threads along i), added in block order by a second kernel: a function of the inputs and n_images alone.  No float atomics.
 *
 * Workspace (floats, every region padded to 256 bytes), with splits = ceil(n_images / 8):
 *   (mean, rstd) [n_images][2] | with a weight: grad_weight partial sums [splits][C * hw] | grad_bias partial sums [splits][C * hw]
 *
 * MPNHIP_ERR_ARG before any launch, the message starting with the entry point's name: what the forward refuses (null lists,
 * n_segments outside 1 .. 4, null / empty segments, hw < 1, eps < 0 or not finite, sizes or strides beyond INT32_MAX), a null
 * grad_out, no output wanted, grad_weight / grad_bias with a NULL weight, a null workspace or one smaller than
 * mpnhip_layer_norm_backward_workspace_bytes (which is 0 for arguments the operator refuses).  n_images == 0 zero-fills
 * grad_weight / grad_bias where given and touches nothing else. */
size_t mpnhip_layer_norm_backward_workspace_bytes(const float* const* seg_data, const int64_t* seg_stride, const int* seg_channels,
                                                  int n_segments, int64_t n_images, int64_t hw, const float* weight, float eps,
                                                  const float* grad_out, int64_t grad_out_stride, float* grad_in, float* grad_weight,
                                                  float* grad_bias);
int mpnhip_layer_norm_backward(const float* const* seg_data, const int64_t* seg_stride, const int* seg_channels, int n_segments,
                               int64_t n_images, int64_t hw, const float* weight, float eps, const float* grad_out,
                               int64_t grad_out_stride, float* grad_in, float* grad_weight, float* grad_bias, void* workspace,
                               size_t workspace_bytes, void* stream);

/* ReID ResNet50 (models/resnet.py), inference: ONE nn.Conv2d(cin, cout, ksize, stride, padding ksize / 2, bias=False) with the
 * eval-mode BatchNorm, the residual add and the ReLU behind it.  ksize 1, 3 or 7; stride 1 or 2; Hout = (H - 1) / stride + 1,
 * Wout likewise.  Everything is NCHW fp32.
 *   x         image i at x + i * x_stride (floats), dense [cin][H][W]
 *   weight    [cout][cin][ksize][ksize], as the module stores it
 *   scale, shift   [cout] each or NULL (1 and 0 stand in): the folded BatchNorm, gamma / sqrt(var + eps) and beta - mean * scale
 *   residual  NULL, or image i at residual + i * residual_stride, dense [cout][Hout][Wout]
 *   out       image i at out + i * out_stride, dense [cout][Hout][Wout]: a stride wider than that writes a channel slice of a
 *             wider tensor and leaves the rest alone.  out must not overlap x or residual (not checked).
 * Result, in this float32 order: v = fmaf(acc, scale[m], shift[m]); v += residual; relu != 0: v = max(v, 0).
 *
 * acc is an implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulation): M = cout, N = n_images * Hout * Wout
 * -- the output pixels of ALL images packed into one column index, so a small map fills the 32-column tiles --, K = cin * ksize^2
 * walked in (channel, then tap) order, one chain per output, no split of K across blocks, no float atomics: an output's bits are
 * a function of the layer and of its image alone, not of n_images and not of the image's position in the batch.  No workspace.
 * K > 2048 (the 3 x 3 layers of 256 and 512 channels): the chain is cut into groups of four K chunks (a chunk: 32 channels of a
 * 1 x 1, 4 channels of a 3 x 3) -- every group is summed from zero and added to the running total, groups in order; one chain of
 * K = 4608 measured 2.5e-6 of the largest output against float64, above the 2e-6 the shorter chains are held to.  The grouping is
 * a function of the layer alone as well.  The block shape (128 x 128; 64 rows x 256 columns for cout <= 64; 64 x 64 when fewer than
 * 512 of the large blocks would be launched) does depend on n_images, and does not show in the bits: the chain is the same in all
 * three.  Path counters: conv_affine_tile (every launch), conv_affine_grouped (K > 2048), conv_affine_small_grid (64 x 64 blocks),
 * conv_affine_wide (64 x 256 blocks); a launch counted by neither of the last two ran 128 x 128 blocks.
 *
 * MPNHIP_ERR_ARG before any launch, the message starting with the entry point's name: null args; n_images < 0; (n_images == 0 is
 * a successful no-op, nothing else is looked at;) null x, weight or out; a ksize other than 1, 3, 7; a stride other than 1, 2;
 * H, W, cin or cout < 1; and any stride, image size (cin * H * W, cout * Hout * Wout) or weight count beyond INT32_MAX,
 * n_images * Hout * Wout beyond INT32_MAX - 256 (a block's column indices run past the last column), or more blocks than a
 * launch holds. */
typedef struct mpnhip_conv_affine_args {
    const float* x; int64_t x_stride; const float* weight; const float* scale; const float* shift;
    const float* residual; int64_t residual_stride; int relu; float* out; int64_t out_stride;
    int64_t n_images; int cin; int cout; int H; int W; int ksize; int stride;
} mpnhip_conv_affine_args;
int mpnhip_conv2d_affine_forward(const mpnhip_conv_affine_args* args, void* stream);

/* The lateral convolution of a feature pyramid's top-down path (torchvision's FeaturePyramidNetwork), inner = conv(x) + bias +
 * F.interpolate(coarser_inner, size=inner.shape[-2:], mode='nearest'): mpnhip_conv2d_affine_forward -- the same kernel, the same
 * chain, every field as above -- whose residual is a COARSER map, image i at residual + i * residual_stride, dense
 * [cout][residual_H][residual_W].  Output pixel (oy, ox) adds residual[m][sy][sx] with aten's nearest-neighbour source index in
 * float32: sy = min((int)floorf(oy * ((float)residual_H / Hout)), residual_H - 1), sx likewise from ox, residual_W and Wout; the
 * index is computed once per output pixel, not per channel.  The convolution's bias goes in as shift with a NULL scale
 * (fmaf(acc, 1, bias) is acc + bias rounded once).  With residual_H == Hout and residual_W == Wout the result equals
 * mpnhip_conv2d_affine_forward's bit for bit.  Path counters: conv_affine_up, beside those of mpnhip_conv2d_affine_forward.
 * MPNHIP_ERR_ARG before any launch: everything mpnhip_conv2d_affine_forward refuses, a null residual, residual_H or residual_W < 1
 * and a residual image (cout * residual_H * residual_W) beyond INT32_MAX.  n_images == 0 is a successful no-op. */
typedef struct mpnhip_conv_affine_up_args {
    const float* x; int64_t x_stride; const float* weight; const float* scale; const float* shift;
    const float* residual; int64_t residual_stride; int relu; float* out; int64_t out_stride;
    int64_t n_images; int cin; int cout; int H; int W; int ksize; int stride;
    int residual_H; int residual_W;
} mpnhip_conv_affine_up_args;
int mpnhip_conv2d_affine_up_forward(const mpnhip_conv_affine_up_args* args, void* stream);

/* nn.MaxPool2d(3, stride 2, padding 1) (the ReID ResNet50's stem): image i at x + i * x_stride, dense [C][H][W], to out + i *
 * out_stride, dense [C][Hout][Wout] with Hout = (H - 1) / 2 + 1, Wout likewise.  Padded cells do not take part: a window of
 * negative values yields the largest of them, never 0.  One thread per output element.  MPNHIP_ERR_ARG before any launch:
 * n_images < 0 (0 is a successful no-op), null x or out, C, H or W < 1, a stride or an input image beyond INT32_MAX, more
 * elements than a launch holds. */
int mpnhip_maxpool2d_forward(const float* x, int64_t x_stride, int64_t n_images, int C, int H, int W, float* out, int64_t out_stride,
                             void* stream);

/* torch.optim.Adam(lr, betas, eps, weight_decay).step() (the optimizer of pl_module.py:76-77, configs/tracking_cfg.yaml:6-10)
 * over FLAT fp32 buffers of n elements: parameters, gradients (as the backward / all-reduce left them) and the two
 * moment buffers (zero before step 1); step = 1, 2, ... counts the calls. */
int mpnhip_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                     float beta2, float eps, float weight_decay, int step, void* stream);
/* The same, skipped as a whole when *skip_flag (device float, may be NULL) is non-zero.  Data-parallel training (one graph per
 * rank, scripts/train.py:65-77 executed in space): every rank adds "my graph's edge_index left [0, N)" (the reference's
 * IndexError, mpn.py:69) to one spare element of the gradient all-reduce; with the reduced element as skip_flag no rank steps
 * on gradients of a clamped graph, without a host read on the ranks whose own graph is fine. */
int mpnhip_adam_step_guarded(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                             float beta2, float eps, float weight_decay, int step, const float* skip_flag, void* stream);
/* The same with the step count kept where the skip decision is made: `calls` = 1, 2, ... counts the CALLS, *skipped_calls (device
 * int, zero before the first call, may be NULL) the calls that were skipped; a skipped call adds one to it and an applied update uses
 * the bias corrections of step calls - *skipped_calls -- torch.optim.Adam's count of applied steps -- so a skipped step followed by a
 * good one equals ONE reference step (pl_module.py:76-77).  skipped_calls == NULL: mpnhip_adam_step_guarded. */
int mpnhip_adam_step_counted(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                             float beta2, float eps, float weight_decay, int calls, const float* skip_flag, int* skipped_calls,
                             void* stream);

/* ---------------------------------------------------------------------------------------------
 * Graph construction on the device: what MOTGraph.construct_graph_object
 * (data/mot_graph.py:283-317) computes before the model runs.  All indices int64 like the reference's tensors.
 * ------------------------------------------------------------------------------------------- */
/* get_time_valid_conn_ixs(frame_num, max_frame_dist, return_undirected=True) (utils/graph.py:6-37): the pairs
 * (i, j), i < j, whose frames differ and are at most max_frame_dist apart (max_frame_dist < 0 = the reference's
 * 'max'), in the reference's order (ascending i, then j).  Two calls, because the caller allocates the result:
 *   count: offsets [N + 1] (device) <- exclusive scan of the per-node pair counts; offsets[N] = number of pairs
 *   fill : edge_ixs [2, n_pairs] row-major, n_pairs = offsets[N] read back by the caller. */
size_t mpnhip_time_valid_conn_workspace_bytes(int n_nodes);
int mpnhip_time_valid_conn_count(const int64_t* frame_num, int n_nodes, int64_t max_frame_dist, int64_t* offsets,
                                 void* workspace, size_t workspace_bytes, void* stream);
int mpnhip_time_valid_conn_fill(const int64_t* frame_num, int n_nodes, int64_t max_frame_dist, const int64_t* offsets,
                                int64_t n_pairs, int64_t* edge_ixs, void* stream);
/* return_undirected=False (utils/graph.py:30-32): ALL ordered pairs (row, col), both directions of every pair, in the row-major
 * order of torch.where on the dense condition.  Same two calls, same workspace size; edge_ixs [2, n_pairs] = row then col. */
int mpnhip_time_valid_conn_directed_count(const int64_t* frame_num, int n_nodes, int64_t max_frame_dist, int64_t* offsets,
                                          void* workspace, size_t workspace_bytes, void* stream);
int mpnhip_time_valid_conn_directed_fill(const int64_t* frame_num, int n_nodes, int64_t max_frame_dist, const int64_t* offsets,
                                         int64_t n_pairs, int64_t* edge_ixs, void* stream);
/* compute_edge_feats_dict (utils/graph.py:90-124): edge_feats [E, 5] = secs_time_dists, norm_feet_x_dists,
 * norm_feet_y_dists, bb_height_dists, bb_width_dists (the dict's order) for edge_ixs [2, E]; per-node columns of
 * the detection frame: frame_num int64 [N], bb_height / bb_width / feet_x / feet_y float32 [N]. */
int mpnhip_edge_features(const int64_t* edge_ixs, int64_t n_edges, int n_nodes, const int64_t* frame_num, float fps,
                         const float* bb_height, const float* bb_width, const float* feet_x, const float* feet_y,
                         float* edge_feats, void* stream);
/* F.pairwise_distance(emb[edge_ixs[0]], emb[edge_ixs[1]]) (data/mot_graph.py:298-301; p = 2, eps as given, the
 * reference uses torch's default 1e-6): dist [E]; emb [N, dim] with row stride ld. */
int mpnhip_pairwise_distance(const float* emb, int64_t ld, int dim, const int64_t* edge_ixs, int64_t n_edges, float eps,
                             float* dist, void* stream);

/* load_precomputed_embeddings (utils/rgb.py:150-188) once the per-frame files are in device memory: stored [n_stored, ld]
 * fp32 rows whose element 0 carries the detection id (1D files: column 0; 3D files [n, 1 + C, H, W]: element [0, 0, 0], i.e.
 * ld = (1 + C) H W).  keep [n_stored] = 1 iff that id occurs in det_ids_sorted [n_det] (int32 ascending): the np.isin
 * filter of rgb.py:179 / :185.  The kept rows without their id column / channel are then one mpnhip_gather_rows. */
int mpnhip_embedding_keep(const float* stored, int64_t ld, int64_t n_stored, const int32_t* det_ids_sorted, int64_t n_det,
                          unsigned char* keep, void* stream);
/* the order assertion of rgb.py:180 / :186: mismatch[0] (device int32) = number of j < n with id(stored[rows[j]]) != det_ids[j] */
int mpnhip_embedding_check(const float* stored, int64_t ld, const int32_t* rows, int64_t n, const int32_t* det_ids,
                           int32_t* mismatch, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Sliding-window inference: MPNTracker._predict_edges_and_masks /
 * _evaluate_graph_in_batches (tracker/mpn_tracker.py:96-210) around mpnhip_forward.
 * ------------------------------------------------------------------------------------------- */
/* get_knn_mask (utils/graph.py:40-87): pruned_mask [E] (1 = keep) for edge_ixs [2, E] with distances pwise_dist [E].
 * symmetric_edges != 0: edge_ixs lists both directions of every pair (inference); 0: one direction (training).
 * Ties in distance rank by column index (stable argsort); the reference leaves them to torch.argsort. */
size_t mpnhip_knn_mask_workspace_bytes(int64_t n_edges, int symmetric_edges);
int mpnhip_knn_mask(const float* pwise_dist, const int64_t* edge_ixs, int n_nodes, int64_t n_edges, int top_k_nns,
                    int reciprocal_k_nns, int symmetric_edges, unsigned char* pruned_mask, void* workspace,
                    size_t workspace_bytes, void* stream);
/* edges_mask of a window (mpn_tracker.py:171-173): flags [E] = both end points in [node_begin, node_end). */
int mpnhip_window_flags(const int64_t* edge_index, int64_t n_edges, int64_t node_begin, int64_t node_end,
                        unsigned char* flags, void* stream);
/* torch.where(flags)[0] as int32 ids (ascending) + their number (device int32), e.g. tensor[mask] selections. */
size_t mpnhip_compact_workspace_bytes(int64_t n);
int mpnhip_compact(const unsigned char* flags, int64_t n, int32_t* ids, int32_t* count, void* workspace,
                   size_t workspace_bytes, void* stream);
/* out [n, dim] = src[ids] (rows of stride ld);  out [2, n] = edge_index[:, ids] - node_begin. */
int mpnhip_gather_rows(const float* src, int64_t ld, const int32_t* ids, int64_t n, int dim, float* out, void* stream);
int mpnhip_gather_edges(const int64_t* edge_index, int64_t n_edges, const int32_t* ids, int64_t n, int64_t node_begin,
                        int64_t* out, void* stream);
/* mpn_tracker.py:126-141,188-190: overall_edge_preds[full id] += sigmoid(logit) for the window's kept edges and
 * overall_num_preds += 1 for the kept edges (or, with set_pruned_edges_to_inactive, for every edge of the window).
 * logits [n_kept]; kept_ids [n_kept] index the window's edge list (NULL = identity); window_ids [n_window] index
 * the full sequence graph's edges. */
int mpnhip_window_accumulate(const float* logits, const int32_t* kept_ids, int64_t n_kept, const int32_t* window_ids,
                             int64_t n_window, int set_pruned_edges_to_inactive, float* overall_edge_preds,
                             float* overall_num_preds, void* stream);
/* final_edge_preds = overall_edge_preds / overall_num_preds, NaN -> 0 (mpn_tracker.py:195-197). */
int mpnhip_average_preds(const float* overall_preds, const float* overall_num, int64_t n, float* final_preds, void* stream);

/* The rest of _evaluate_graph_in_batches (mpn_tracker.py:199-210): node masks, undirected merge, edge pruning.
 *
 * Node masks.  accumulate: overall_node_preds[node_begin + i, :] += sigmoid(mask_logits[i, :]) and
 * overall_num_node_preds[node_begin + i] += 1 for the n_rows nodes of ONE window (mask_logits [n_rows, row_len] =
 * mask_predictions[-1] of the window, row_len = H * W; the accumulators cover all n_nodes of the sequence).  Windows overlap in
 * nodes: one call per window, in window order on one stream -- no atomics, a fixed summation order.  16-byte accesses when the
 * window's block is 16-byte aligned and a multiple of 4 floats, a scalar path otherwise.
 * average: node_preds [n_nodes, row_len] = overall_node_preds / overall_num_node_preds per row.  A node that was in no window
 * gives 0 / 0 = NaN, as the reference's torch.div does (the reference zeroes NaN for EDGES only, mpn_tracker.py:204). */
int mpnhip_node_mask_accumulate(const float* mask_logits, int64_t n_rows, int64_t row_len, int64_t node_begin, int64_t n_nodes,
                                float* overall_node_preds, float* overall_num_node_preds, void* stream);
int mpnhip_node_mask_average(const float* overall_node_preds, const float* overall_num_node_preds, int64_t n_nodes, int64_t row_len,
                             float* node_preds, void* stream);
/* to_undirected_graph (utils/graph.py:165-186) in two calls, because the caller allocates the results:
 *   sort: keys (min(r, c) << 32) | max(r, c) of edge_index [2, E], one stable radix sort with the edge ids; inverse [E] (int32) =
 *         column of every directed edge in the unique list (torch.unique's return_inverse), n_unique (device int32) = U.  n_nodes
 *         > 0 promises every id < n_nodes and limits the sorted bits to what such ids need; 0 = ids up to 2^32 - 1.
 *   fill: edge_index_u [2, U] (pairs with row < col in lexicographic order = torch.unique(dim=1)'s columns; NULL: skip) and, for
 *         one attribute attr [E] (NULL: skip), attr_u [U] = mean over the pair's directed copies, summed in ascending edge id
 *         and divided by their number (scatter_mean; for the normal two copies exactly (a + b) / 2).  One call per attribute;
 *         `workspace` is the sort's, untouched in between.  The reference's assertion is the caller's E == 2 U. */
size_t mpnhip_undirected_merge_workspace_bytes(int64_t n_edges);
int mpnhip_undirected_merge_sort(const int64_t* edge_index, int64_t n_edges, int64_t n_nodes, int32_t* inverse, int32_t* n_unique,
                                 void* workspace, size_t workspace_bytes, void* stream);
int mpnhip_undirected_merge_fill(int64_t n_edges, int64_t n_unique, const void* workspace, size_t workspace_bytes,
                                 int64_t* edge_index_u, const float* attr, float* attr_u, void* stream);
/* flags [n] = preds[i] >= threshold (utils/graph.py:205; NaN -> 0 as in torch); the selection itself is mpnhip_compact +
 * mpnhip_gather_edges / mpnhip_gather_rows. */
int mpnhip_threshold_flags(const float* preds, int64_t n, float threshold, unsigned char* flags, void* stream);

/* ---------------------------------------------------------------------------------------------
 * From edge scores to track ids: the projectors (tracker/projectors.py), MPNTracker._assign_ped_ids
 * (tracker/mpn_tracker.py:231-248) and Postprocessor.drop_short_trajectories (tracker/postprocessing.py:14-18).
 * edge_index [2, K] int64 is an undirected list with row < col per edge (mpnhip_undirected_merge_fill's, pruned or not), in any
 * edge order; n_nodes, n_edges < 2^30.  An edge with an id outside [0, n_nodes) is never followed: it is counted
 * (counters[3]) and otherwise skipped.  Integer and compare-only arithmetic throughout: the same bits on every call.
 * ------------------------------------------------------------------------------------------- */
/* compute_constr_satisfaction_rate(undirected_edges=False, return_flow_vals=True) (utils/evaluation.py:370-414) up to its last
 * division: round_preds [K] = edge_preds > 0.5 as 0 / 1 (NaN -> 0), flow_out / flow_in [n_nodes] (int32) = active edges per row /
 * column, counters (device int32 [8]) = { #(flow_out > 1), #(flow_in > 1), num_constraints = distinct rows + distinct cols,
 * edges with an id out of range, 0 ... }.  constr_sat_rate = 1 - (counters[0] + counters[1]) / counters[2] is the caller's.
 * With n_edges == 0 and n_nodes == 0 nothing is written. */
size_t mpnhip_project_round_count_workspace_bytes(int64_t n_nodes);
int mpnhip_project_round_count(const int64_t* edge_index, int64_t n_edges, int64_t n_nodes, const float* edge_preds,
                               float* round_preds, int32_t* flow_out, int32_t* flow_in, int32_t* counters, void* workspace,
                               size_t workspace_bytes, void* stream);
/* The loop of GreedyProjector.project (projectors.py:41-60) as two edge-parallel passes, in place on round_preds (as
 * mpnhip_project_round_count left it, with its flow counts): A. every node with flow_out > 1 keeps its active outgoing edge with
 * the largest edge_preds -- the lowest edge id on a tie -- and loses the others; B. the same over the incoming edges of every
 * node whose in-count is still above 1 after A.  Per node one 64-bit atomicMax on (score bits << 32) | ~edge id. */
size_t mpnhip_project_greedy_workspace_bytes(int64_t n_nodes);
int mpnhip_project_greedy(const int64_t* edge_index, int64_t n_edges, int64_t n_nodes, const float* edge_preds, float* round_preds,
                          const int32_t* flow_out, const int32_t* flow_in, void* workspace, size_t workspace_bytes, void* stream);
/* The sub-problem of ExactProjector.project (projectors.py:92-93): nodes_mask [n_nodes] = flow_in > 1 | flow_out > 1,
 * edges_mask [K] = nodes_mask[row] | nodes_mask[col]; the selection itself is mpnhip_compact + the gathers. */
int mpnhip_project_violated_masks(const int64_t* edge_index, int64_t n_edges, int64_t n_nodes, const int32_t* flow_out,
                                  const int32_t* flow_in, unsigned char* nodes_mask, unsigned char* edges_mask, void* stream);
/* scipy.sparse.csgraph.connected_components(directed=False) over the edges with edge_preds == 1 (_assign_ped_ids): labels
 * [n_nodes] (int64) = rank of the component's smallest node among all components' smallest nodes, n_components (device int32,
 * may be NULL).  Lock-free union-find in one launch (the larger root goes under the smaller by compare-and-swap), one pass
 * that resolves every node's root, a scan over the root flags.  Any undirected graph: cycles, duplicate edges, isolated nodes. */
size_t mpnhip_connected_components_workspace_bytes(int64_t n_nodes);
int mpnhip_connected_components(const int64_t* edge_index, int64_t n_edges, int64_t n_nodes, const float* edge_preds, int64_t* labels,
                                int32_t* n_components, void* workspace, size_t workspace_bytes, void* stream);
/* drop_short_trajectories: counts [n_nodes] (int32) = nodes per label (labels in [0, n_nodes)), keep [n_nodes] =
 * counts[labels[v]] >= min_track_len.  Labels are not renumbered. */
int mpnhip_track_lengths(const int64_t* labels, int64_t n_nodes, int64_t min_track_len, int32_t* counts, unsigned char* keep,
                         void* stream);

/* ---------------------------------------------------------------------------------------------
 * The linear program of ExactProjector (projectors.py:92-113, PuLPMinCostFlowSolver :129-160) on the device, as batched linear
 * assignment.  The LP -- minimise sum x_e (1 - 2 p_e), 0 <= x <= 1, in-flow <= 1 and out-flow <= 1 per node, over the edges of
 * edges_mask (mpnhip_project_violated_masks) -- is a maximum-weight matching of out-copies against in-copies of the nodes: an
 * edge with p <= 0.5 costs >= 0 and is 0 in an optimum, the ACTIVE edges (edges_mask set, ids in [0, n_nodes), p > 0.5; NaN is
 * not active) split into connected components of that bipartite graph, and each component is one dense assignment whose cells
 * are 1 - 2 p for an edge and 0 for "unmatched".  Where the LP's optimum is unique, so is the assignment's and they agree; among
 * optima of equal total mpnhip_lsa_batched decides by its own tie rule (below); the total is the LP's either way.
 *
 *   mpnhip_project_exact_plan     the problems and their layout
 *   mpnhip_project_exact_fill     the cost cells
 *   mpnhip_lsa_batched(cost, cells, cell_ptr, a_ptr, n_a, b_ptr, n_b, n_problems, NULL, NULL, maximize = 0, match_b, ...)
 *   mpnhip_project_exact_apply    the edge values
 * The names follow the greedy family (mpnhip_project_*).  The three calls take ONE workspace of
 * mpnhip_project_exact_workspace_bytes(n_nodes, n_edges) bytes (0 for sizes the calls refuse); the fill leaves one winner flag
 * per edge at its head, which the apply reads: hand both the same buffer.  edge_index as above ([2, K], row < col, any order;
 * n_nodes, n_edges < 2^30); an edge with an id outside [0, n_nodes) is skipped and counted (sizes[5]).  Integer and compare-only
 * arithmetic apart from the float64 cost cells, integer atomics only, sorts and scans by rocprim: the same bits on every call
 * and for every order of the edge list (duplicate pairs excepted: their tie goes by edge id).
 * ------------------------------------------------------------------------------------------- */
size_t mpnhip_project_exact_workspace_bytes(int64_t n_nodes, int64_t n_edges);
/* The bipartite graph has the vertices u (out-copy) and n_nodes + v (in-copy) of every active edge (u, v); its components come
 * from the union-find of mpnhip_connected_components over 2 n_nodes vertices.  A PROBLEM is a component with an active edge;
 * problems are ordered by their smallest vertex, a problem's rows are its out-copies and its columns its in-copies, both by
 * ascending node id.  Outputs (device):
 *   a_slot, b_slot [n_nodes] (int32)  position of the node's out-copy in the list of all rows / of its in-copy in the list of
 *                                     all columns (problem after problem), or -1
 *   a_ptr, b_ptr (int32), cell_ptr (int64)  prefix lists over the problems, CAPACITY n_nodes + 1 each: entry f for f <=
 *                                     n_problems, and the totals in every entry behind; problem f owns the rows a_ptr[f] ..
 *                                     a_ptr[f + 1], the columns b_ptr[f] .. b_ptr[f + 1] and na_f x nb_f cells at cell_ptr[f]
 *   sizes [6] (int64)                 { n_problems, n_a (rows), n_b (columns), max_side (the longest side of a problem),
 *                                       cells, skipped_edges }
 * n_nodes == 0: no problem, one zero in each prefix list. */
int mpnhip_project_exact_plan(const int64_t* edge_index, int64_t n_edges, int64_t n_nodes, const float* edge_preds,
                              const unsigned char* edges_mask, int32_t* a_slot, int32_t* b_slot, int32_t* a_ptr, int32_t* b_ptr,
                              int64_t* cell_ptr, int64_t* sizes, void* workspace, size_t workspace_bytes, void* stream);
/* cost [cells] (float64; n_problems, n_a, n_b, cells: the plan's sizes): cell (a, b) of problem f, cost[cell_ptr[f] + a * nb_f
 * + b], is 1.0 - 2.0 * (double)p_e for the active edge between that row and that column and 0.0 for every other pair.  Several
 * active edges of one pair: the one with the largest score is the cell's WINNER, the lowest edge id among equal scores (the tie
 * order of mpnhip_project_greedy); the others count as 0.  An edge whose slots or cell do not lie inside the lists (a plan of
 * other inputs) is left out. */
int mpnhip_project_exact_fill(const int64_t* edge_index, int64_t n_edges, int64_t n_nodes, const float* edge_preds,
                              const unsigned char* edges_mask, const int32_t* a_slot, const int32_t* b_slot, const int32_t* a_ptr,
                              const int32_t* b_ptr, const int64_t* cell_ptr, int64_t n_problems, int64_t n_a, int64_t n_b,
                              double* cost, int64_t cells, void* workspace, size_t workspace_bytes, void* stream);
/* out [K] (float32): round_preds[e] for an edge outside edges_mask; for a masked edge 1.0 iff it is active, its cell's winner and
 * match_b[a_slot[u]] == b_slot[v] (match_b [n_a]: mpnhip_lsa_batched's, entries of the whole lists), else 0.0. */
int mpnhip_project_exact_apply(const int64_t* edge_index, int64_t n_edges, int64_t n_nodes, const unsigned char* edges_mask,
                               const float* round_preds, const int32_t* a_slot, const int32_t* b_slot, const int32_t* match_b,
                               int64_t n_a, float* out, const void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * From RoI masks to MOTS run-length masks: MPNTracker._to_full_masks (tracker/mpn_tracker.py:267-298) =
 * torchvision's paste_masks_in_image(padding = 1), ensure_unique_masks (utils/mots.py:5-25), >= mask_threshold and the run
 * boundaries of COCO's RLE.  One launch covers n_frames frames of one image size (img_h * img_w < 2^31, at most 65535 frames);
 * its detections are a list of n_dets entries grouped by frame: frame_ptr [n_frames + 1] (device int32, ascending, frame f owns
 * the entries [frame_ptr[f], frame_ptr[f + 1])), det_ids [n_dets] (device int32; NULL = identity) = row of masks [n_rows, mh, mw]
 * (float32) and boxes [n_rows, 4] (float64: left, top, right, bottom) of every entry.  An entry whose row leaves [0, n_rows) or
 * whose box is not finite pastes nothing; expanded coordinates are clamped to +-2^29.  Unfused IEEE arithmetic in a fixed order,
 * integer counts, a stable sort: the same bits on every call (tests/full_masks_ref.py restates them in numpy).
 * ------------------------------------------------------------------------------------------- */
/* Bytes that any of the three calls below needs for these sizes (hw = img_h * img_w; n_events = 0 while it is not known: enough
 * for mpnhip_paste_unique_masks and mpnhip_mask_run_events_count).  0 for sizes the calls refuse. */
size_t mpnhip_full_masks_workspace_bytes(int64_t n_dets, int64_t n_frames, int64_t hw, int64_t n_events);
/* labels [n_frames, img_w, img_h] (int32, column-major images: position p = x * img_h + y): the list entry that owns the pixel, or
 * -1.  Per pixel the entries of the frame are walked in list order; an entry's value is the bilinear sample (align_corners =
 * False, no antialiasing) of its zero-padded mask resized to its expanded box, 0 outside the box; an entry replaces the winner
 * iff its value is greater, or is NaN while the winner's is not (np.argmax); the label is the winner if its value >=
 * mask_threshold (> 0; NaN compares false).  values (NULL: skip), same shape, float32: the winner's value. */
int mpnhip_paste_unique_masks(const float* masks, int64_t n_rows, int mh, int mw, const double* boxes, const int32_t* det_ids,
                              int64_t n_dets, const int32_t* frame_ptr, int64_t n_frames, int img_h, int img_w, float mask_threshold,
                              int32_t* labels, float* values, void* workspace, size_t workspace_bytes, void* stream);
/* The run boundaries of every entry's mask (labels == entry) in two calls, because the caller allocates the result.  Position p
 * of a frame is an event of entry d when exactly one of labels[p - 1], labels[p] is d (labels[-1] = -1; a run continues across
 * column ends; nothing at p = hw; labels outside [0, n_dets) count as -1).
 *   count: det_counts [n_dets] (device int32) = events per entry, n_events (device int32) = their sum.
 *   fill:  event_pos [n_events] (int32) = the positions, sorted by (entry, position): entry d owns the det_counts[d] positions
 *          after those of the entries before it.  n_events is the count's.  COCO's counts for d are the differences of
 *          (0, its positions ..., hw). */
int mpnhip_mask_run_events_count(const int32_t* labels, int64_t n_frames, int64_t hw, int64_t n_dets, int32_t* det_counts,
                                 int32_t* n_events, void* workspace, size_t workspace_bytes, void* stream);
int mpnhip_mask_run_events(const int32_t* labels, int64_t n_frames, int64_t hw, int64_t n_dets, int64_t n_events, int32_t* event_pos,
                           void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * COCO's compressed run-length strings for a batch of masks: rleToString / rleFrString of the COCO API (common/maskApi.c), as
 * masks.rle_string, masks.rle_counts and mots_eval.counts_to_runs restate them on the host.  A string holds a mask's counts
 * (alternating run lengths, zeros first, summing to hw); count i >= 3 is stored as its difference to count i - 2; a value is
 * written in 5-bit groups, low bits first, as the characters 48 + group + 32 * more.  Integers only (int64, wrapping as numpy's):
 * the bytes and numbers of the host codec on every call.
 * ------------------------------------------------------------------------------------------- */
/* Bytes mpnhip_rle_encode needs for these sizes (no device needed).  0 for sizes the call refuses, and when nothing is needed. */
size_t mpnhip_rle_encode_workspace_bytes(int64_t n_dets, int64_t n_events);
/* The strings of n_dets masks from what mpnhip_mask_run_events_count / mpnhip_mask_run_events leave on the device: det_counts
 * [n_dets] and event_pos [n_events] (int32, sorted by (entry, position); n_events and hw < 2^31).  The counts of entry d are the
 * differences of (0, its positions ..., hw): det_counts[d] + 1 of them -- the one count hw for an entry without events, a leading 0
 * for a first position of 0.  bytes [bytes_capacity] (uint8): the strings one behind the other in entry order, no separator;
 * str_ptr [n_dets + 1] (int64): string d is bytes[str_ptr[d] .. str_ptr[d + 1]).  No host read sizes the output: a value takes at
 * most 7 characters, and a bytes_capacity below 7 * (n_events + n_dets) is refused before any launch.  Lists that are not those
 * two calls' own (unsorted positions, counts that do not sum to n_events) give strings of no meaning and no access outside the
 * buffers. */
int mpnhip_rle_encode(const int32_t* event_pos, const int32_t* det_counts, int64_t n_dets, int64_t n_events, int64_t hw,
                      unsigned char* bytes, int64_t bytes_capacity, int64_t* str_ptr, void* workspace, size_t workspace_bytes,
                      void* stream);
/* Bytes mpnhip_rle_decode_runs needs for n strings (mpnhip_rle_decode_scan needs none). */
size_t mpnhip_rle_decode_workspace_bytes(int64_t n);
/* The runs of set pixels of n strings in two calls, because the caller allocates the result.  bytes [n_bytes] (uint8, n_bytes <
 * 2^31) and str_ptr [n + 1] (int64) as above (offsets are clamped into the buffer); hw_per_string [n] (int64): the pixels every
 * string must describe.
 *   scan: per string n_counts (int32), n_runs (int32: the non-empty runs of set pixels, i.e. the odd counts > 0), area (int64:
 *         their total length) and status (int32), the refusals of the host path as bits: 1 = a character outside '0' .. 'o',
 *         2 = truncated (the last character announces another group), 4 = a count of more than 12 groups, 8 = a negative
 *         count, 16 = the counts do not sum to hw_per_string, or a position leaves [0, 2^31).  With one of 1 / 2 / 4 there are
 *         no counts to judge and 8 / 16 stay clear.  A string with a status has n_runs = area = 0.  The empty string has no
 *         counts: status 0 for hw = 0, else 16.
 *   runs: run_ptr [n + 1] (int64) = exclusive scan of n_runs (the scan's, with status; total_runs = their sum, read by the
 *         caller); run_row, run_begin, run_end [total_runs] (int32): string, first position and position behind the run, ordered
 *         by string, then position.  Empty runs are left out, adjacent runs are not merged ([3, 2, 0, 4] gives [3, 5) and
 *         [5, 9)).  A string with a status writes nothing.
 * Malformed input of any kind ends in a status, never in an access outside the buffers. */
int mpnhip_rle_decode_scan(const unsigned char* bytes, int64_t n_bytes, const int64_t* str_ptr, const int64_t* hw_per_string, int64_t n,
                           int32_t* n_counts, int32_t* n_runs, int64_t* area, int32_t* status, void* stream);
int mpnhip_rle_decode_runs(const unsigned char* bytes, int64_t n_bytes, const int64_t* str_ptr, const int64_t* hw_per_string, int64_t n,
                           const int32_t* n_runs, const int32_t* status, int64_t total_runs, int64_t* run_ptr, int32_t* run_row,
                           int32_t* run_begin, int32_t* run_end, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The pixel work of the MOTS metrics (sMOTSA, IDF1, ...): compute_mots_metrics (utils/evaluation.py:87-102) =
 * MOTChallengeEvalKit/MOTS/MOTS_metrics.py.  Masks of one MOTS frame are disjoint (mots_common/io.py:57-62), so a frame is one
 * label image per side, as above: [n_frames, img_w, img_h] int32, position p = x * img_h + y, hw = img_h * img_w < 2^31, at most
 * 65535 frames per call.  A side's objects are a list grouped by frame (a_ptr / b_ptr [n_frames + 1], device int32, ascending:
 * side a = ground truth, side b = prediction); a label is the list entry that owns the pixel, a label outside its frame's
 * entry range counts as -1.  Integer atomics and integer compares only: the same bits on every call
 * (tests/mots_metrics_ref.py restates the three operators in numpy).
 * ------------------------------------------------------------------------------------------- */
/* Bytes that any of the three calls below needs for these sizes (mpnhip_label_overlap needs none).  0 for sizes the calls
 * refuse, and when nothing is needed. */
size_t mpnhip_mots_workspace_bytes(int64_t n_runs, int64_t n_a, int64_t n_b, int64_t n_frames, int64_t hw);
/* The inverse of mpnhip_mask_run_events: labels [n_frames, hw] = -1, then entry run_entry[r] over the positions
 * [run_begin[r], run_end[r]) of its frame (run_* [n_runs], device int32; 0 <= begin < end <= hw; frame_ptr [n_frames + 1] of
 * the list of n_entries entries).  A run continues across column ends, as COCO's do.  A run whose entry leaves the list or
 * whose range leaves [0, hw] paints nothing.  Overlapping runs of different entries are the caller's error: which one a pixel
 * keeps is unspecified.  The work is spread by painted pixel, not by run. */
int mpnhip_paint_label_runs(const int32_t* run_entry, const int32_t* run_begin, const int32_t* run_end, int64_t n_runs,
                            const int32_t* frame_ptr, int64_t n_entries, int64_t n_frames, int64_t hw, int32_t* labels, void* workspace,
                            size_t workspace_bytes, void* stream);
/* The joint histogram of two label images of the same frames (both starting on a 16-byte boundary).  table [table_cells]
 * (int32, zeroed by the call); table_ptr [n_frames + 1] (device int64): frame f owns the (na_f + 1) x (nb_f + 1) cells at
 * table_ptr[f], cell [(ia + 1) * (nb_f + 1) + (ib + 1)] = number of pixels whose labels are the frame's entries (ia, ib); row 0
 * and column 0 stand for "no object".  A frame's cells sum to hw, its row sums are the areas of the a-entries, its column sums
 * those of the b-entries.  A frame whose cells would leave the table is skipped.  table_ptr_host: the same numbers in host
 * memory, or NULL; read only to count per frame which form of the kernel it takes (mpnhip_debug_counters: label_overlap_lds
 * for a table of at most 4096 cells, label_overlap_global beyond).  MPNHIP_ERR_UNSUPPORTED for table_cells >= 2^31. */
int mpnhip_label_overlap(const int32_t* labels_a, const int32_t* labels_b, const int32_t* a_ptr, int64_t n_a, const int32_t* b_ptr,
                         int64_t n_b, const int64_t* table_ptr, const int64_t* table_ptr_host, int64_t n_frames, int64_t hw,
                         int32_t* table, int64_t table_cells, void* stream);
/* The kit's decisions from the table, in exact integer form.  a_ignore [n_a] (uint8, 1 = part of the frame's ignore region),
 * a_traj [n_a] / b_traj [n_b] (int32): trajectory index of every entry, -1 = none.  With i = cell, A = row sum, B = column
 * sum, u = A + B - i:
 *   per a-entry that is not ignore: match_b = the b-entry (index into the list) with 2 i > u (c > 0.5, MOTS_metrics.py:253-254;
 *       at most one among disjoint masks) or -1, inter = its i, uni = its u (0 without a match).  Ignore entries: -1, 0, 0.
 *   per b-entry: b_matched (uint8) = some a-entry matched it, b_ignored (uint8) = 2 * (sum of i over the ignore a-entries) > B
 *       (:272-273, intersection over the prediction's own area), b_area = B.
 *   id_match [n_a_traj, n_b_traj] (int32, zeroed by the call): + 1 for every pair of an a-entry that is not ignore and a b-entry
 *       of one frame with 2 i >= u and u > 0 (the complement of overlap < 0.5, :529-535) whose trajectory indices are in range.
 * A pair of two EMPTY masks (u = 0) matches nowhere; the kit's 0 / 0 = NaN there counts as matched in its IDF1 part.
 * MPNHIP_ERR_UNSUPPORTED for table_cells or n_a_traj * n_b_traj >= 2^31. */
int mpnhip_mots_frame_match(const int32_t* table, int64_t table_cells, const int64_t* table_ptr, const int32_t* a_ptr, int64_t n_a,
                            const int32_t* b_ptr, int64_t n_b, int64_t n_frames, const unsigned char* a_ignore, const int32_t* a_traj,
                            const int32_t* b_traj, int64_t n_a_traj, int64_t n_b_traj, int32_t* match_b, int32_t* inter, int32_t* uni,
                            unsigned char* b_matched, unsigned char* b_ignored, int32_t* b_area, int32_t* id_match, void* workspace,
                            size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * HOTA of a KITTI-MOTS sequence: eval_kitti_mots (utils/evaluation.py:127-135) = TrackEval's KittiMOTS preprocessing
 * (datasets/kitti_mots.py:299-387) and HOTA.eval_sequence (metrics/hota.py:25-117) for one class, from the tables of
 * mpnhip_label_overlap.  Lists, a_ptr / b_ptr and the table as above.  A launch's similarities are one block of float64:
 * frame f owns na_f x nb_f cells at sim_ptr[f] (device int64 [n_frames + 1]), cell [ia * nb_f + ib]; sim_cells is their
 * number (< 2^31).  a_traj [n_a] / b_traj [n_b] (int32): index of the entry's id among the n_gt_ids / n_tr_ids ids of the
 * sequence; an entry whose index is outside its range (-1: an ignore row, a prediction of another class) takes no part.  A
 * b-entry is KEPT when its index is in range and b_removed is 0; an a-entry when its index is in range.  The accumulators
 * (potential, gt_count, tr_count, tp, loca, matches_count) belong to the caller, who zeroes them before the first launch of a
 * sequence; the launches are issued in frame order.  No floating-point atomics: a float64 sum is one thread adding in frame
 * order, or a tree whose shape depends on the sizes alone -- the same bits on every call (tests/hota_ref.py restates the five
 * operators in numpy).  Every index read from a caller's array is clamped or checked before it is used.
 * MPNHIP_ERR_UNSUPPORTED for n_gt_ids * n_tr_ids * MPNHIP_HOTA_ALPHAS >= 2^31 or n_frames * (n_gt_ids + n_tr_ids) >= 2^31.
 * ------------------------------------------------------------------------------------------- */
#define MPNHIP_HOTA_ALPHAS 19   /* np.arange(0.05, 0.99, 0.05), hota.py:17 */
/* Bytes that any of the five calls below needs for these sizes.  0 for sizes the calls refuse. */
size_t mpnhip_hota_workspace_bytes(int64_t n_a, int64_t n_b, int64_t n_frames, int64_t n_gt_ids, int64_t n_tr_ids);
/* a_ignore [n_a] (uint8, 1 = part of the frame's ignore region), b_scored [n_b] (uint8, 1 = a prediction of the evaluated class).
 * With i = cell, A = row sum, B = column sum (both with the "no object" cells), u = A + B - i:
 *   sim [sim_cells] (zeroed by the call) = double(i) / double(u) for an a-entry that is not ignore and a scored b-entry with
 *       i > 0, else 0: an empty mask has similarity 0 with everything.
 *   b_removed [n_b] (uint8) = scored, unmatched and 2 * (sum of i over the frame's ignore rows) > B (kitti_mots.py:336-344).
 *       A scored b-entry is matched iff it is the FIRST column some object row is eligible with, eligible = i > 0 and
 *       2 i >= u (the complement of "< 0.5 - eps", :329).  Masks of one side are disjoint, so the kit's assignment (:330) is
 *       that, except for an object split exactly in half by two predictions: there the kit's choice follows scipy's tie order,
 *       here the prediction earlier in the list is the matched one.
 *   row_sum [n_a] / col_sum [n_b] (float64): the sums of sim over the kept entries of the other side (similarity.sum(1) /
 *       .sum(0) of hota.py:57 after the removal); 0 for an ignore row, a removed or an unscored column. */
int mpnhip_hota_frame_similarity(const int32_t* table, int64_t table_cells, const int64_t* table_ptr, const int32_t* a_ptr, int64_t n_a,
                                 const int32_t* b_ptr, int64_t n_b, int64_t n_frames, const unsigned char* a_ignore,
                                 const unsigned char* b_scored, const int64_t* sim_ptr, int64_t sim_cells, double* sim,
                                 unsigned char* b_removed, double* row_sum, double* col_sum, void* workspace, size_t workspace_bytes,
                                 void* stream);
/* hota.py:53-65 for one launch: potential [n_gt_ids, n_tr_ids] (float64) += sim / (row_sum + col_sum - sim) of every kept pair
 * of a frame where that denominator exceeds eps, frames in order; gt_count [n_gt_ids] / tr_count [n_tr_ids] (int32) += 1 per
 * kept entry.  Two kept entries of one id in a frame are the caller's error: one of them is the id's entry. */
int mpnhip_hota_accumulate_alignment(const double* sim, int64_t sim_cells, const int64_t* sim_ptr, const int32_t* a_ptr, int64_t n_a,
                                     const int32_t* b_ptr, int64_t n_b, int64_t n_frames, const int32_t* a_traj, const int32_t* b_traj,
                                     const unsigned char* b_removed, const double* row_sum, const double* col_sum, int64_t n_gt_ids,
                                     int64_t n_tr_ids, double* potential, int32_t* gt_count, int32_t* tr_count, void* workspace,
                                     size_t workspace_bytes, void* stream);
/* hota.py:68, :85, once all launches are accumulated: score [sim_cells] (the layout of sim; zeroed by the call) = potential /
 * (gt_count + tr_count - potential) * sim for a kept pair, 0 elsewhere -- the cells of the host's assignment problems. */
int mpnhip_hota_frame_scores(const double* sim, int64_t sim_cells, const int64_t* sim_ptr, const int32_t* a_ptr, int64_t n_a,
                             const int32_t* b_ptr, int64_t n_b, int64_t n_frames, const int32_t* a_traj, const int32_t* b_traj,
                             const unsigned char* b_removed, int64_t n_gt_ids, int64_t n_tr_ids, const double* potential,
                             const int32_t* gt_count, const int32_t* tr_count, double* score, void* stream);
/* hota.py:91-101 for one launch.  match_b [n_a] (int32): the b-entry (index into the list) the host's assignment gave the
 * a-entry, or -1; a pair counts when both are kept entries of one frame.  alphas: MPNHIP_HOTA_ALPHAS float64 in HOST memory.
 * For every alpha with sim >= alpha - eps: tp [alphas] (int64) += 1, loca [alphas] (float64) += sim (a frame's terms through a
 * fixed tree, the frames in order), matches_count [alphas, n_gt_ids, n_tr_ids] (int32) += 1 at the pair's ids. */
int mpnhip_hota_alpha_accumulate(const double* sim, int64_t sim_cells, const int64_t* sim_ptr, const int32_t* a_ptr, int64_t n_a,
                                 const int32_t* b_ptr, int64_t n_b, int64_t n_frames, const int32_t* a_traj, const int32_t* b_traj,
                                 const unsigned char* b_removed, const int32_t* match_b, const double* alphas, int64_t n_gt_ids,
                                 int64_t n_tr_ids, int64_t* tp, double* loca, int32_t* matches_count, void* workspace,
                                 size_t workspace_bytes, void* stream);
/* hota.py:105-112 without the division by max(1, TP): out [alphas, 3] (float64) = the sums over (g, t) of mc * (mc / max(1,
 * gt_count + tr_count - mc)), mc * (mc / max(1, gt_count)) and mc * (mc / max(1, tr_count)) with mc = matches_count[alpha, g, t]
 * (the AssA, AssRe and AssPr numerators). */
int mpnhip_hota_association(const int32_t* matches_count, const int32_t* gt_count, const int32_t* tr_count, int64_t n_gt_ids,
                            int64_t n_tr_ids, double* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * TrackEval's Identity and CLEAR metrics of a KITTI-MOTS sequence (metrics/identity.py:32-89, metrics/clear.py:37-128) for one
 * class, from what mpnhip_hota_frame_similarity left on the device for a launch: sim, sim_ptr, the lists, b_removed and the
 * trajectory indices, all as in the HOTA calls above (an entry is KEPT in the same way).  The accumulators and the scan's state
 * belong to the caller, who initialises them before the first launch of a sequence; the launches are issued in frame order and
 * the result does not depend on how the frames are split into launches.  Integer atomics only; the one float64 sum (MOTP_sum)
 * is one thread adding in the kit's order: the same bits on every call (tests/clear_identity_ref.py restates the operators in
 * numpy).  Every index read from a caller's array is clamped or checked before it is used.  MPNHIP_ERR_UNSUPPORTED from the
 * two Identity calls for n_gt_ids * n_tr_ids >= 2^31 (the table is one problem of mpnhip_lsa_batched).
 * ------------------------------------------------------------------------------------------- */
/* Bytes that any of the calls below needs for these sizes.  0 for sizes the calls refuse. */
size_t mpnhip_clear_identity_workspace_bytes(int64_t n_a, int64_t n_b, int64_t n_frames, int64_t n_gt_ids, int64_t n_tr_ids);
/* identity.py:55-57 for one launch: potential_count [n_gt_ids, n_tr_ids] (int32) += 1 at the ids of every kept pair with
 * sim >= 0.5 (the kit's np.greater_equal on the double of mpnhip_hota_frame_similarity).  gt_id_count / tracker_id_count of
 * :60-61 are gt_count / tr_count of mpnhip_hota_accumulate_alignment. */
int mpnhip_identity_accumulate(const double* sim, int64_t sim_cells, const int64_t* sim_ptr, const int32_t* a_ptr, int64_t n_a,
                               const int32_t* b_ptr, int64_t n_b, int64_t n_frames, const int32_t* a_traj, const int32_t* b_traj,
                               const unsigned char* b_removed, int64_t n_gt_ids, int64_t n_tr_ids, int32_t* potential_count, void* stream);
/* idtp [1] (int64, written by the call) = the sum of potential_count[g, match_b[g]] over the ids g with match_b[g] (int32
 * [n_gt_ids]) in [0, n_tr_ids): IDTP for the complete assignment of min(n_gt_ids, n_tr_ids) pairs that maximises that sum, which
 * is what identity.py:63-85 computes (IDFN = sum(gt_count) - IDTP, IDFP = sum(tr_count) - IDTP).  match_b is that of
 * mpnhip_lsa_batched for the one problem a_ptr = {0, n_gt_ids}, b_ptr = {0, n_tr_ids}. */
int mpnhip_identity_sums(const int32_t* potential_count, const int32_t* match_b, int64_t n_gt_ids, int64_t n_tr_ids, int64_t* idtp,
                         void* stream);
/* clear.py:81 for one launch, all frames in parallel.  A cell is eligible iff sim >= 0.5 - eps (compared as doubles; for a mask:
 * 2 i >= u).  a_cand [n_a, 2] / b_cand [n_b, 2] (int32): the first two kept entries of the other list (indices into it, list
 * order) a kept entry is eligible with, -1 for none and for an entry that is not kept.  status [1] (int32, written by the
 * call): bit 0 an entry has three or more, bit 1 an a-entry with two has one that itself has two -- among the disjoint masks
 * of label images neither can happen, and a component of eligible cells is a single pair or a star of three entries. */
int mpnhip_clear_frame_candidates(const double* sim, int64_t sim_cells, const int64_t* sim_ptr, const int32_t* a_ptr, int64_t n_a,
                                  const int32_t* b_ptr, int64_t n_b, int64_t n_frames, const int32_t* a_traj, const int32_t* b_traj,
                                  const unsigned char* b_removed, int64_t n_gt_ids, int64_t n_tr_ids, int32_t* a_cand, int32_t* b_cand,
                                  int32_t* status, void* stream);
/* clear.py:67-114 for one launch, its frames in ascending order (one wavefront).  State of the sequence, all [n_gt_ids] int32:
 * prev_tracker_id and prev_timestep_tracker_id (trajectory indices; the caller starts them at -1, the kit's NaN), gt_id_count,
 * gt_matched_count, gt_frag_count (from 0); counters [4] (int64, from 0): CLR_TP, CLR_FN, CLR_FP, IDSW; motp_sum [1] (float64).
 * A frame without kept a-entries only adds its kept b-entries to CLR_FP; one without kept b-entries adds to CLR_FN and
 * gt_id_count; both leave prev_timestep_tracker_id alone.  Otherwise a single pair of candidates is a match; in a star the arm
 * whose tracker id equals prev_timestep_tracker_id of its object wins, without one the entry earlier in the list (the kit:
 * scipy's tie order).  match_b [n_a] (int32, written by the call): the b-entry matched with every a-entry, or -1. */
int mpnhip_clear_sequence_scan(const double* sim, int64_t sim_cells, const int64_t* sim_ptr, const int32_t* a_ptr, int64_t n_a,
                               const int32_t* b_ptr, int64_t n_b, int64_t n_frames, const int32_t* a_traj, const int32_t* b_traj,
                               const unsigned char* b_removed, const int32_t* a_cand, const int32_t* b_cand, int64_t n_gt_ids,
                               int64_t n_tr_ids, int32_t* prev_tracker_id, int32_t* prev_timestep_tracker_id, int32_t* gt_id_count,
                               int32_t* gt_matched_count, int32_t* gt_frag_count, int64_t* counters, double* motp_sum, int32_t* match_b,
                               void* workspace, size_t workspace_bytes, void* stream);
/* clear.py:117-121: out [4] (int64, written by the call) = MT, PT, ML, Frag from the three per-id counts: over the ids with
 * gt_id_count > 0, matched / count > 0.8 is MT and >= 0.2 is MT + PT (decided in integers: 5 m > 4 c, 5 m >= c);
 * ML = n_gt_ids - MT - PT; Frag = the sum of gt_frag_count - 1 over the ids where it is positive. */
int mpnhip_clear_track_summary(const int32_t* gt_id_count, const int32_t* gt_matched_count, const int32_t* gt_frag_count, int64_t n_gt_ids,
                               int64_t* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Batched rectangular linear sum assignment: scipy.optimize.linear_sum_assignment(cost, maximize) for n_problems problems in
 * one launch, in the layout of the HOTA calls above (a score block goes in as it is).  Problem f owns the a-entries a_ptr[f] ..
 * a_ptr[f + 1] and the b-entries b_ptr[f] .. b_ptr[f + 1] of two lists (device int32 [n_problems + 1]) and na_f x nb_f float64
 * cells at cell_ptr[f] (device int64 [n_problems + 1]), cell [ia * nb_f + ib]; cells is their number (< 2^31).  a_keep [n_a] /
 * b_keep [n_b] (uint8, 1 = the entry takes part; NULL = all of them).
 *   match_b [n_a] (int32): the b-entry (index into the whole list, b_ptr[f] + ib) assigned to the a-entry, or -1;
 *   match_a [n_b] (int32; may be NULL): its inverse.  Both are filled with -1 by the call first.
 * Over its kept rows and columns a problem gets a complete assignment of min(kept rows, kept columns) pairs of optimal total
 * cost; a problem with no kept row or no kept column gets nothing and status 0.
 *   status [n_problems] (int32): 0 solved; 1 the costs are not finite -- a NaN among the kept cells, or a search that finds no
 *   column at a finite distance (-inf, or only +inf left); 2 more than MPNHIP_LSA_MAX_SIDE kept rows or kept columns (the lists
 *   are device arrays, so this refusal happens on the device); 3 the problem's cells do not lie inside cost.  A problem with a
 *   status other than 0 gets only -1; the other problems of the launch are not affected.
 * The algorithm is the shortest augmenting path of Crouse 2016 (scipy's) in float64 on c = maximize ? -cost : cost, with more
 * kept rows than kept columns on the transpose (by index, nothing is copied): rows in list order, r = ((minval + c[i][j]) - u[i])
 * - v[j] taken only if r < shortest[j], the next column the unscanned one of lowest shortest -- among equals an unassigned one,
 * lowest index first, otherwise the lowest index.  Where the optimum is unique the pairs are scipy's; among ties they need not
 * be (the total is).  One wavefront per problem, no floating-point atomics, no sums in a tree: the same bits on every call
 * (tests/lsa_ref.py restates it in numpy).  Every loop is bounded by a counter: at most kept rows x kept columns column scans
 * per problem.  Every index read from a caller's array is clamped or checked before it is used.
 * n_problems == 0, or n_a == 0 and n_b == 0: a successful no-op (status is not written).  MPNHIP_ERR_UNSUPPORTED for
 * cells >= 2^31.
 * ------------------------------------------------------------------------------------------- */
/* largest number of kept rows, or of kept columns, of one problem: its state (u, v, shortest, path, col4row, row4col, the two
 * lists of kept entries, the two scanned sets: 46 B per row or column) stays in the LDS of one workgroup, 160 KiB on gfx950 */
#define MPNHIP_LSA_MAX_SIDE 2048
/* Bytes mpnhip_lsa_batched needs for these sizes (a small constant: the state lives in LDS).  0 for sizes the call refuses. */
size_t mpnhip_lsa_workspace_bytes(int64_t n_a, int64_t n_b, int64_t n_problems);
int mpnhip_lsa_batched(const double* cost, int64_t cells, const int64_t* cell_ptr, const int32_t* a_ptr, int64_t n_a,
                       const int32_t* b_ptr, int64_t n_b, int64_t n_problems, const unsigned char* a_keep, const unsigned char* b_keep,
                       int maximize, int32_t* match_b, int32_t* match_a, int32_t* status, void* workspace, size_t workspace_bytes,
                       void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training inputs from a detections file and a ground-truth file: MOTSeqProcessor._assign_gt and _store_gt_masks
 * (data/seq_processing/seq_processor.py:203-237, :289-393).  Side a = the detections, side b = the ground-truth rows, both lists
 * grouped by frame (a_ptr / b_ptr [n_frames + 1], device int32, ascending, at most 65535 frames per call); a launch's pairs are
 * one block of cells in the layout of mpnhip_lsa_batched: frame f owns na_f x nb_f cells at cell_ptr[f] (device int64
 * [n_frames + 1]), cell [ia * nb_f + ib]; cells is their number (< 2^31).  Per cell the two cost calls write
 *   iou     (float64) the pair's intersection over union;
 *   allowed (uint8)   !(iou < min_iou): the pairs the reference does not overwrite with NaN (:223);
 *   cost    (float64) allowed ? 1 - iou : min(na_f, nb_f) + 1.
 * Solved with mpnhip_lsa_batched (minimising), a forbidden cell costs more than any complete assignment of allowed ones, so the
 * allowed pairs of the solution are: among the matchings of allowed pairs one with the most pairs, and among those one of the
 * smallest total 1 - iou -- what solve_dense(1 - iou) with NaN for the forbidden pairs is taken to return.  A cell that belongs
 * to no frame (cell_ptr not ascending, a frame whose cells leave the block) gets 0, 0, 0.  Float64 arithmetic, one rounded
 * operation at a time, no atomics: the same bits on every call (tests/gt_assign_ref.py restates the operators in numpy).  Every
 * index read from a caller's array is clamped or checked before it is used.  MPNHIP_ERR_UNSUPPORTED for cells >= 2^31.
 * ------------------------------------------------------------------------------------------- */
/* a_boxes [n_a, 4] / b_boxes [n_b, 4] (float64: top, left, bottom, right).  iou = utils/iou.py:4-31: the extents of the
 * intersection and of both boxes with + 1, inter / (area_a + area_b - inter); NaN where numpy's is (allowed, cost NaN: the
 * solver then reports status 1 for the frame). */
int mpnhip_box_iou_costs(const double* a_boxes, int64_t n_a, const double* b_boxes, int64_t n_b, const int32_t* a_ptr,
                         const int32_t* b_ptr, const int64_t* cell_ptr, int64_t n_frames, int64_t cells, double min_iou, double* iou,
                         unsigned char* allowed, double* cost, void* stream);
/* The same from the table of mpnhip_label_overlap(labels of the detections, labels of the ground truth) -- masks that are
 * disjoint within a side of a frame: with i = cell, A = row sum, B = column sum, u = A + B - i, iou = double(i) / double(u)
 * (pycocotools' iou with iscrowd = False, utils/iou.py:62-76).  A pair with u = 0 has iou 0 and is not allowed. */
int mpnhip_overlap_iou_costs(const int32_t* table, int64_t table_cells, const int64_t* table_ptr, const int32_t* a_ptr, int64_t n_a,
                             const int32_t* b_ptr, int64_t n_b, const int64_t* cell_ptr, int64_t n_frames, int64_t cells,
                             double min_iou, double* iou, unsigned char* allowed, double* cost, void* stream);
/* seq_processor.py:226-234 from the solver's match_b [n_a] (the b-entry of every a-entry, or -1): a pair counts when both are
 * entries of one frame and its cell is allowed.  gt_ids [n_b] (int64): the id column; gt_row [n_b] / det_row [n_a] (int32; NULL =
 * identity): the row of either file an entry stands for.  Per a-entry, at row o = det_row[a] of the two results [n_out] (skipped
 * when o is outside): det_gt_entry (int32) = gt_row of its b-entry or -1, det_id (int64) = that entry's id or -1 (a false
 * positive). */
int mpnhip_gt_assign_finish(const int32_t* match_b, const unsigned char* allowed, int64_t cells, const int64_t* cell_ptr,
                            const int32_t* a_ptr, int64_t n_a, const int32_t* b_ptr, int64_t n_b, int64_t n_frames,
                            const int64_t* gt_ids, const int32_t* gt_row, const int32_t* det_row, int64_t n_out, int32_t* det_gt_entry,
                            int64_t* det_id, void* stream);
/* largest number of samples per output pixel and axis mpnhip_roi_align_labels takes: a box of up to 256 * ph x 256 * pw pixels */
#define MPNHIP_ROI_MAX_GRID 256
/* torchvision 0.6.0's roi_align(input [K, 1, H, W], rois, (ph, pw), spatial_scale = 1, sampling_ratio = -1, aligned = False) on
 * the CPU in float32 (seq_processor.py:344-355), where input[k] = "the pixel belongs to the ground-truth mask detection k was
 * assigned" is never materialised: labels [n_frames, img_w, img_h] (int32, position x * img_h + y) is the ground truth's label
 * image of mpnhip_paint_label_runs, one per frame for all its detections.  The n_dets detections of the launch are a list
 * grouped by frame (det_ptr [n_frames + 1]) with boxes [n_dets, 4] (float32: left, top, right, bottom) and det_row [n_dets]
 * (int32; NULL = identity), their row o of det_gt_entry (int32), masks ([n_out, ph, pw] float32) and valid ([n_out] uint8); a
 * row outside [0, n_out) is skipped.  e = det_gt_entry[o] is a row of the ground-truth file (n_gt rows): gt_ids [n_gt] (int64)
 * its id, gt_label [n_gt] (int32) the label its pixels have in this launch, which must be an entry of the detection's frame in
 * gt_ptr [n_frames + 1].
 *   valid = e in [0, n_gt), the label in the frame's range, and the id none of ignore_ids [n_ignore] (int64; :329).  Where it is
 *   0 the row of masks is 0, and so it is for a box that is not finite or needs more than MPNHIP_ROI_MAX_GRID samples per axis.
 *   Else, in float32 and unfused: roi = max(x2 - x1, 1), bin = roi / p, grid = ceil(roi / p) per axis; sample (iy, ix) of pixel
 *   (py, px) lies at start + p * bin + (i + 0.5) * bin / grid; outside [-1, size] it adds 0, else it is clamped at 0, low =
 *   int(v), at low >= size - 1: low = high = size - 1 and v = low; l = v - low, h = 1 - l; it adds hy hx t(ylow, xlow) +
 *   hy lx t(ylow, xhigh) + ly hx t(yhigh, xlow) + ly lx t(yhigh, xhigh), t = 1 where the label is the detection's.  Samples are
 *   added in (iy, ix) order and the sum is divided by max(grid_h * grid_w, 1).
 * One block per detection, no atomics: the same bits on every call, and those of tests/gt_assign_ref.py in float32. */
int mpnhip_roi_align_labels(const int32_t* labels, int64_t n_frames, int img_h, int img_w, const int32_t* det_ptr, const int32_t* gt_ptr,
                            const float* boxes, int64_t n_dets, const int32_t* det_row, const int32_t* det_gt_entry, int64_t n_out,
                            const int32_t* gt_label, const int64_t* gt_ids, int64_t n_gt, const int64_t* ignore_ids, int n_ignore,
                            int ph, int pw, float* masks, unsigned char* valid, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The inputs of the two embedding CNNs: MOTSeqProcessor._store_embeddings (data/seq_processing/seq_processor.py:395-562) around
 * its stock modules.  No atomics, no sums in a tree: the same bits on every call, and those of tests/embed_inputs_ref.py.  Every
 * index read from a caller's array is checked before it is used.
 * ------------------------------------------------------------------------------------------- */
/* largest side of a padded crop and of the output of mpnhip_reid_crops */
#define MPNHIP_CROP_MAX_SIDE 8192
/* Bytes mpnhip_reid_crops needs for n boxes whose padded crops are at most max_ph x max_pw (both passes' coefficients and the
 * pad's means, per box).  0 for sizes the call refuses. */
size_t mpnhip_reid_crops_workspace_bytes(int64_t n, int max_ph, int max_pw, int oh, int ow);
/* BoundingBoxDataset.__getitem__ (utils/rgb.py:40-69) for n boxes in one launch sequence: the crop, np.pad(mode='mean'),
 * PIL.Image.resize((ow, oh), BILINEAR), ToTensor, Normalize.
 *   frames [n_frames, H, W, 3] (uint8, as imread returns them); box_frame [n] (int32) the frame of every box;
 *   geom [n, 8] (int32) what the reference's expressions give for the box: y0, y1, x0, x1 -- the crop is rows [y0, y1) and
 *   columns [x0, x1) of the frame -- and pt, pb, pl, pr, the pads above, below, left and right of it; the padded crop has
 *   ph = pt + (y1 - y0) + pb rows and pw = pl + (x1 - x0) + pr columns, at most max_ph and max_pw (<= MPNHIP_CROP_MAX_SIDE);
 *   mean_std (HOST, 6 floats): Normalize's mean and std per channel;
 *   out [n, 3, oh, ow] (float32); out_u8 [n, oh, ow, 3] (uint8; may be NULL): the resized patch before ToTensor.
 * A box whose frame, crop or pads do not fit (frame outside [0, n_frames), an empty crop or one outside the frame, a negative
 * pad, a padded side above max_ph / max_pw) gets zeros.
 *   The pad, never materialised: a padded row above or below the crop holds per column and channel m(sum of that column over
 *   the crop's rows, rows), m(s, c) = s / c rounded half to even in integer arithmetic (numpy's mean of uint8 and its round());
 *   then every row, the padded ones included, is continued left and right by m(sum of the row over the crop's columns, columns).
 *   The resize is Pillow's ImagingResample for 8-bit images, the horizontal pass first, a pass skipped when its size does not
 *   change.  Per output index xx of an axis in -> out, in float64 and unfused: scale = in / out, filterscale = support =
 *   max(scale, 1), center = (xx + 0.5) * scale, xmin = max(int(center - support + 0.5), 0), xmax = min(int(center + support +
 *   0.5), in); tap x of xmax - xmin has w = max(0, 1 - |(x + xmin - center + 0.5) * (1 / filterscale)|), the weights are divided
 *   by their sum (added in tap order) and each becomes int(0.5 + w * 2^22).  A pixel of a pass is
 *   clip8((2^21 + sum coef * pixel) >> 22) in int32, stored as uint8 between the passes.
 *   out = (float(v) / 255f - mean[c]) / std[c] in float32, one rounded operation at a time.
 * A block takes a box and a band of output rows: the horizontal pass of the input rows the band's vertical taps reach goes to
 * LDS, the vertical pass reads it there.  MPNHIP_ERR_UNSUPPORTED when not even one output row's input rows fit (60 KiB);
 * n == 0: a successful no-op. */
int mpnhip_reid_crops(const unsigned char* frames, int64_t n_frames, int H, int W, const int32_t* geom, const int32_t* box_frame,
                      int64_t n, int max_ph, int max_pw, int oh, int ow, const float* mean_std, float* out, unsigned char* out_u8,
                      void* workspace, size_t workspace_bytes, void* stream);

/* GeneralizedRCNNTransform.forward of torchvision 0.6.0 under torch 1.5.0 (tracktor_masked/maskrcnn_fpn.py:81-92) for n_frames
 * frames of one size, in one launch: ToTensor, Normalize, the bilinear resize to oh x ow and the zero padding of the batch to
 * Hp x Wp.  The caller computes the sizes (embed_inputs.transform_sizes).
 *   frames [n_frames, H, W, 3] (uint8, as imread returns them); mean_std (HOST, 6 floats): Normalize's mean and std per channel;
 *   out [n_frames, 3, Hp, Wp] (float32).
 * A tap of channel c is t(v) = (float(v) / 255f - mean[c]) / std[c] in float32, one rounded operation at a time: the image is
 * normalised first and interpolated after, the reference's order.  Per axis in -> out, aten's upsample_bilinear2d with
 * align_corners=False and no antialiasing in float32, unfused: scale = (float)in / out -- from the OUTPUT SIZE, as torch 1.5.0
 * recomputes it for a float scale_factor, which is F.interpolate(size=(oh, ow)) in later releases --, src = max(scale * (dst +
 * 0.5f) - 0.5f, 0), i0 = min((int)src, in - 1), i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1.  An output inside oh x ow is
 *   ly0 * (lx0 * t(y0, x0) + lx1 * t(y0, x1)) + ly1 * (lx0 * t(y1, x0) + lx1 * t(y1, x1));
 * every output outside it is 0.  One thread per output pixel: the indices and weights of both axes are computed once and serve
 * the three channels; the 3 x 256 values of t sit in LDS.  No sums across threads: the same bits on every call, and a frame's
 * bits do not depend on the batch.  MPNHIP_ERR_ARG before any launch: n_frames < 0 (0 is a successful no-op), a null pointer,
 * a size below 1, oh > Hp or ow > Wp, a frame (3 * H * W) or an output image (3 * Hp * Wp) beyond INT32_MAX, more elements than a
 * launch holds. */
int mpnhip_rcnn_transform(const unsigned char* frames, int64_t n_frames, int H, int W, int oh, int ow, int Hp, int Wp,
                          const float* mean_std, float* out, void* stream);

#define MPNHIP_FPN_LEVELS 4
/* largest output_size * sampling_ratio of mpnhip_fpn_roi_align: the samples of one axis, kept in LDS */
#define MPNHIP_FPN_MAX_SAMPLES 1024
/* the four levels of one feature pyramid (a HOST struct): data[l] [n_frames, channels, h[l], w[l]] (float32, device), scale[l]
 * the level's cells per pixel of the network's image */
typedef struct mpnhip_fpn_levels {
    const float* data[MPNHIP_FPN_LEVELS];
    int h[MPNHIP_FPN_LEVELS];
    int w[MPNHIP_FPN_LEVELS];
    float scale[MPNHIP_FPN_LEVELS];
} mpnhip_fpn_levels;
/* MultiScaleRoIAlign(['0', '1', '2', '3'], output_size, sampling_ratio) of torchvision 0.6.0 (maskrcnn_fpn.py:108-115,
 * seq_processor.py:493-495) with the level of every box chosen by the caller: box k = boxes [k, 4] (float32: left, top, right,
 * bottom in the network's image) is pooled from frame box_frame[k] (int32) of level box_level[k] (int32) into
 * out [n, channels (+ 1), S, S] (float32), S = output_size; a box whose frame or level is outside gets zeros.
 *   Per axis, in float32 and unfused, with scale and size the level's: roi_start = v1 * scale, extent = max(v2 * scale -
 *   roi_start, 1), bin = extent / S, grid = sampling_ratio; sample i of output p lies at (roi_start + p * bin) + ((i + 0.5) * bin)
 *   / grid; outside [-1, size] it adds 0, else it is clamped at 0, low = int(v), at low >= size - 1: low = high = size - 1 and
 *   v = low; l = v - low, h = float(1 - double(l)).  A sample adds ((hy hx t(ylow, xlow) + hy lx t(ylow, xhigh)) + ly hx
 *   t(yhigh, xlow)) + ly lx t(yhigh, xhigh), t the channel's plane; samples are added in (iy, ix) order and the sum is divided
 *   by float(grid * grid).  The same for every channel.
 *   detection_id [n] (int32, values in [0, 2^24); may be NULL): when given, channel 0 of out holds float(detection_id[k]) and
 *   the features follow from channel 1 -- the stored format of seq_processor.py:545-548 without the torch.cat.
 * n == 0: a successful no-op. */
int mpnhip_fpn_roi_align(const mpnhip_fpn_levels* levels, int64_t n_frames, int channels, const float* boxes, const int32_t* box_frame,
                         const int32_t* box_level, int64_t n, int output_size, int sampling_ratio, const int32_t* detection_id,
                         float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The Mask R-CNN RoI heads on given boxes (tracktor_masked/frcnn_fpn.py:29-64, maskrcnn_fpn.py:31-79, data/preprocessing.py:19-42),
 * inference: what follows the dense and convolution-type layers (mpnhip_fpn_roi_align, mpnhip_linear,
 * mpnhip_conv2d_affine_forward, mpnhip_conv2d_forward).  Everything is float32; every operation a decision or a coordinate
 * depends on is rounded on its own, never contracted into an FMA.  No float atomics: the same bits on every call.
 * ------------------------------------------------------------------------------------------- */
#define MPNHIP_BOX_MAX_CLASSES 91
/* FastRCNNPredictor + F.softmax(class_logits, -1)[:, label] + BoxCoder(weights).decode(...)[:, label] + resize_boxes back to the
 * original image (torchvision 0.6.0), for one class, in one launch.
 *   h [n, K] (row stride ldh) the box head's output; w_cls [C, K], b_cls [C]; w_box [4 C, K], b_box [4 C]; proposals [n, 4]
 *   (x1, y1, x2, y2 in the network's image); weights (HOST, 4 floats): the coder's (wx, wy, ww, wh), (10, 10, 5, 5) in RoIHeads;
 *   clip: float32(log(1000 / 16)); ratio_h, ratio_w: resize_boxes' Python-float ratios original / network size, rounded to
 *   float32 (1 and 1: the boxes stay in the network's image).
 *   boxes [n, 4], scores [n]; logits [n, C] and deltas [n, 4] (the four rows 4 label .. 4 label + 3 of the regression, before
 *   the weights) may be NULL.
 * One wavefront per box computes the C + 4 dot products it needs: a lane adds the products of the float4s lane, lane + 64, ... of
 * a row in that order (fmaf), a butterfly adds the 64 partial sums, the bias is added last -- an order that is a function of K
 * alone, so a box's bits depend neither on n nor on its position.  Softmax: e_c = expf(logit_c - max), the sum in class order,
 * score = e_label / sum.  Decoding per axis (decode_single): w = v2 - v1, c = v1 + 0.5f * w, d = delta / weight, the size delta
 * d > clip ? clip : d, pc = d * w + c, pw = expf(dsize) * w, lo = (pc - 0.5f * pw) * ratio, hi = (pc + 0.5f * pw) * ratio.
 * No clip_boxes_to_image: predict_boxes and predict do not clip.
 * MPNHIP_ERR_ARG before any launch, the message starting with the entry point's name: n < 0 (n == 0 is a successful no-op,
 * nothing else is looked at); a null h, weight, bias, proposals, weights, boxes or scores; C outside 2 .. MPNHIP_BOX_MAX_CLASSES;
 * K < 4 or K % 4 != 0; label outside [0, C); ldh < K or ldh % 4 != 0; h, w_cls or w_box not 16-byte aligned; a weight that is 0
 * or not finite; n beyond INT32_MAX.  Path counter: box_predict. */
int mpnhip_box_predict(const float* h, int64_t ldh, const float* w_cls, const float* b_cls, const float* w_box, const float* b_box,
                       const float* proposals, int64_t n, int k, int num_classes, int label, const float* weights, float clip,
                       float ratio_h, float ratio_w, float* boxes, float* scores, float* logits, float* deltas, void* stream);

/* the most boxes of one frame mpnhip_nms_batched takes: 64 lanes x 64 bits of one wavefront's "removed" set */
#define MPNHIP_NMS_MAX_PER_FRAME 4096
/* scores >= score_threshold followed by torchvision.ops.nms(boxes, scores, iou_threshold) (data/preprocessing.py:26-31) for
 * every frame of a batch at once.
 *   boxes [n, 4] (x1, y1, x2, y2), scores [n]; ptr [n_frames + 1] (int32, device): the boxes of frame f are the rows ptr[f] ..
 *   ptr[f + 1]; it must start at 0 and never descend; max_per_frame (host): an upper bound of a frame's row count;
 *   score_threshold: -INFINITY switches the filter off.
 *   keep [n] (uint8) 1 for a kept row; order [n] (int32): from ptr[f] the kept rows of frame f in the order they were visited,
 *   -1 behind them (and for rows of no frame); count [n_frames] (int32).
 * Within a frame the candidates -- rows with score >= score_threshold, which a NaN score never is -- are visited by decreasing
 * score, equal scores (-0 equals +0) by increasing row.  A candidate i is kept unless an earlier KEPT box j of the frame has
 * iou(j, i) > iou_threshold (strict); a suppressed box suppresses nobody.  iou = inter / ((area_i + area_j) - inter), inter =
 * max(min(x2) - max(x1), 0) * max(min(y2) - max(y1), 0), area = (x2 - x1) * (y2 - y1); 0 / 0 is NaN and suppresses nothing.
 * A frame's result depends neither on n_frames nor on the frame's position.
 * Three steps: a stable radix sort of (frame, descending score) keys over all rows (rocprim); one wavefront per 64 x 64 tile of
 * every frame's upper triangle builds 64-bit suppression words with ballots, all frames in one launch of n_frames *
 * ceil(max_per_frame / 64)^2 blocks; ONE wavefront per frame scans them, lane l holding word l of the removed set.
 * A frame whose OWN range ptr does not describe (negative, descending, beyond n, more rows than max_per_frame; every frame
 * when ptr[0] != 0) gets count -1 and keeps nothing.  Only a frame's own range is checked: where ptr descends, the results of the
 * other frames whose rows overlap the bad range are unspecified.  Every access stays inside the buffers whatever ptr holds.
 * Workspace (every region padded to 256 bytes), W = ceil(max_per_frame / 64):
 *   keys [n] (8 bytes) | sorted keys [n] | row ids [n] (int32) | sorted row ids [n] | suppression words [n][W] (8 bytes) | rocprim
 * MPNHIP_ERR_ARG before any launch, the message starting with the entry point's name: n or n_frames < 0 (n == 0 is a successful
 * no-op: nothing else is looked at and nothing is written, count included); max_per_frame outside 1 .. MPNHIP_NMS_MAX_PER_FRAME;
 * n above 2^30; n_frames < 1; a null boxes, scores, ptr, keep, order or count; boxes not 16-byte aligned; a NaN threshold; more
 * tiles than a launch holds.  MPNHIP_ERR_WORKSPACE: a null workspace or one smaller than mpnhip_nms_batched_workspace_bytes (0 for
 * sizes the operator refuses and for n == 0).  Path counter: nms_batched. */
size_t mpnhip_nms_batched_workspace_bytes(int64_t n, int max_per_frame);
int mpnhip_nms_batched(const float* boxes, const float* scores, const int32_t* ptr, int64_t n, int64_t n_frames, int max_per_frame,
                       float score_threshold, float iou_threshold, unsigned char* keep, int32_t* order, int32_t* count,
                       void* workspace, size_t workspace_bytes, void* stream);

#define MPNHIP_ROI_MASK_MAX_SIZE 1024
/* maskrcnn_inference for one label (maskrcnn_fpn.py:68-75), optionally followed by the tracker's nn.Upsample(scale_factor=2,
 * mode='bilinear') (tracker/mpn_tracker.py:300-341): out [n, S * up, S * up] = bilinear_up(1 / (1 + expf(-logits[:, label]))).
 *   logits: image i at logits + i * ld (floats), dense [num_channels][S][S] -- num_channels may be 1 when the caller computed
 *   only the label's channel (label 0); S = size; up 1 or 2.
 * The sigmoid comes first, one rounded operation at a time.  up == 2, per axis, aten's float32 arithmetic for
 * align_corners=False: src = max((dst + 0.5f) * 0.5f - 0.5f, 0), i0 = (int)src, i1 = min(i0 + 1, S - 1), l1 = src - i0,
 * l0 = 1 - l1; out = ly0 * (lx0 * t(y0, x0) + lx1 * t(y0, x1)) + ly1 * (lx0 * t(y1, x0) + lx1 * t(y1, x1)).  One thread per output.
 * MPNHIP_ERR_ARG before any launch, the message starting with the entry point's name: n < 0 (n == 0 is a successful no-op,
 * nothing else is looked at); null logits or out; size outside 1 .. MPNHIP_ROI_MASK_MAX_SIZE; up other than 1, 2; num_channels < 1
 * or an image beyond INT32_MAX; label outside [0, num_channels); ld smaller than an image; more outputs than a launch holds.
 * Path counter: roi_mask_finish. */
int mpnhip_roi_mask_finish(const float* logits, int64_t ld, int64_t n, int num_channels, int label, int size, int up, float* out,
                           void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training batches: MOTGraphDataset.get_from_frame_and_seq (data/mot_graph_dataset.py:185-234) and the DataLoader's collation
 * for all graphs of a batch at once.  A batch is n_nodes nodes in graph order (graph g owns the nodes graph_ptr[g] ..
 * graph_ptr[g + 1]), every node a row of a sequence table that stays on the device.  Which rows, and the random shifts, come
 * from the host (mpntrackseg_amd/dataset.py).  Node indices are batch-global everywhere.  No float atomics and no sums in a
 * tree: the same bits on every call -- those of numpy in float64, and in float32 those of mpnhip_edge_features /
 * mpnhip_pairwise_distance on each graph alone.  kNN pruning, edge labels and the row gathers of x / x_ext / the mask
 * targets are the existing mpnhip_knn_mask (it ranks per node, so the batch graph is the same problem), mpnhip_edge_labels
 * and mpnhip_gather_rows over the batch.
 * ------------------------------------------------------------------------------------------- */
/* columns of a box table, float64: bb_left, bb_top, bb_right, bb_bot, bb_width, bb_height, feet_x, feet_y */
#define MPNHIP_BOX_COLS 8
/* columns an edge attribute can be made of: the five of mpnhip_edge_features, then the embedding distance */
#define MPNHIP_EDGE_ATTR_COLS 6
size_t mpnhip_augment_boxes_workspace_bytes(void);
/* Gather and MOTGraphAugmentor._wiggle_boxes (data/augmentation.py:41-86).
 *   boxes [n_rows, MPNHIP_BOX_COLS] (float64), frame [n_rows], ids [n_rows] (int64): the table; node_src [n_nodes] (int32) the
 *   row of every node; graph_ptr_host [n_graphs + 1] (int32, HOST): must start at 0, never descend and end at n_nodes -- it is
 *   checked here and copied to graph_ptr [n_graphs + 1] (device), which the later calls take; eps [n_nodes, 4] (float64; NULL
 *   = no augmentation, the rows are copied) the relative shift of the top, bottom, left and right side.
 *   In float64 and unfused, in the reference's order (:71-80): top += h * e0, bot += h * e1, left += w * e2, right += w * e3 with
 *   the table's h and w, then h = bot - top, w = right - left.  feet_x / feet_y are NOT touched (the reference's code, against
 *   its docstring).
 *   out_boxes [n_nodes, MPNHIP_BOX_COLS] (float64); out_cols [n_nodes, 4] (float32) = bb_height, bb_width, feet_x, feet_y cast
 *   as .float() casts; out_frame, out_id [n_nodes] (int64); node_graph [n_nodes] (int32).
 *   min_iou (device double) = min over the nodes of iou_pairs(new box, old box) (utils/iou.py:33-59, the + 1 convention), NaN if
 *   any is NaN, + inf without eps or without nodes: the caller compares it with min_iou_bb_wiggling (:86).
 *   bad_rows (device int32) = the nodes whose row lies outside [0, n_rows); they get zeros and id -1.
 * n_graphs == 0 (then n_nodes must be 0): a successful no-op. */
int mpnhip_augment_boxes(const double* boxes, const int64_t* frame, const int64_t* ids, int64_t n_rows, const int32_t* node_src,
                         const int32_t* graph_ptr_host, int64_t n_graphs, const double* eps, int64_t n_nodes, double* out_boxes,
                         float* out_cols, int64_t* out_frame, int64_t* out_id, int32_t* node_graph, int32_t* graph_ptr,
                         double* min_iou, int32_t* bad_rows, void* workspace, size_t workspace_bytes, void* stream);
/* get_time_valid_conn_ixs (utils/graph.py:6-37) inside every graph of the batch: the pairs (i, j), i < j, of ONE graph whose
 * frames differ and are at most max_frame_dist apart (< 0 = 'max'), by ascending i, then j -- the concatenation of the graphs'
 * own lists with their node offsets added.  frame_num [n_nodes] (int64); node_graph, graph_ptr: device, as mpnhip_augment_boxes
 * wrote them.  count / fill as mpnhip_time_valid_conn_count / _fill: two launches and a scan, however many graphs.
 * n_nodes == 0: a successful no-op that writes nothing. */
size_t mpnhip_batch_pairs_workspace_bytes(int64_t n_nodes);
int mpnhip_batch_pairs_count(const int64_t* frame_num, const int32_t* node_graph, const int32_t* graph_ptr, int64_t n_graphs,
                             int64_t n_nodes, int64_t max_frame_dist, int64_t* offsets, void* workspace, size_t workspace_bytes,
                             void* stream);
int mpnhip_batch_pairs_fill(const int64_t* frame_num, const int32_t* node_graph, const int32_t* graph_ptr, int64_t n_graphs,
                            int64_t n_nodes, int64_t max_frame_dist, const int64_t* offsets, int64_t n_pairs, int64_t* edge_ixs,
                            void* stream);
/* compute_edge_feats_dict (utils/graph.py:90-124) with fps [n_graphs] (float32, device) -- float32(frame) / fps is formed per
 * node with the fps of the node's graph, then subtracted -- and F.pairwise_distance of emb [n_nodes, dim] (row stride ld).
 * node_cols [n_nodes, 4] = out_cols of mpnhip_augment_boxes.  edge_feats [n_edges, 5], emb_dist [n_edges]. */
int mpnhip_batch_edge_features(const int64_t* edge_ixs, int64_t n_edges, int64_t n_nodes, const int64_t* frame_num,
                               const int32_t* node_graph, const float* fps, int64_t n_graphs, const float* node_cols,
                               const float* emb, int64_t ld, int dim, float eps, float* edge_feats, float* emb_dist, void* stream);
/* From the kept pairs to the layout of a PyG Batch of reference graphs (data/mot_graph.py:311-312): kept [n_kept] (int32,
 * ascending; NULL = all, n_kept == n_pairs) selects of pairs [2, n_pairs]; a graph with m kept pairs, the first of them kept
 * pair number s, owns the edges 2 s .. 2 s + 2 m: its pairs, then its flipped pairs.  attr_cols [n_attr_cols] (HOST, each in
 * 0 .. MPNHIP_EDGE_ATTR_COLS - 1) names the columns of edge_attr [2 n_kept, n_attr_cols]: 0 .. 4 of edge_feats, 5 = emb_dist;
 * values are duplicated, not sign-flipped.  edge_index [2, 2 n_kept] (int64), edge_graph [2 n_kept] (int32). */
size_t mpnhip_batch_edge_layout_workspace_bytes(int64_t n_graphs);
int mpnhip_batch_edge_layout(const int64_t* pairs, int64_t n_pairs, const int32_t* kept, int64_t n_kept, const int32_t* node_graph,
                             int64_t n_nodes, int64_t n_graphs, const float* edge_feats, const float* emb_dist,
                             const int32_t* attr_cols, int n_attr_cols, int64_t* edge_index, float* edge_attr, int32_t* edge_graph,
                             void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Measurement helpers used by bench.py (HIP events on the launch stream; these synchronise).
 * ------------------------------------------------------------------------------------------- */
/* In-stream kernel timing of the real hot path: while enabled, mpnhip_forward brackets (a) the first-layer
 * edge-MLP GEMM (the dominant MFMA kernel) and (b) the aggregation kernel (the HBM-bound one) of every
 * message-passing step with HIP events on the launch stream.  mpnhip_profile_read synchronises, returns
 * the average duration (us) and launch count of each since the last read, and resets the counters.
 * The empty-pair cost applies to the default (NULL) stream the calibration pairs are recorded on. */
int mpnhip_profile_enable(int on);   /* 0 = off, 1 = time every launch of the two kernels, n > 1 = every n-th launch */
/* 1 when mpnhip_forward evaluates the per-edge chain (edge MLP + classifier + flow MLPs) of this model with the
 * fused edge_chain kernel (then THAT kernel is the one bracketed as "gemm" by the profile hooks), 2 when it does so with
 * the bf16-operand chain kernel (MPNHIP_PREC_BF16, edge_chain_bf16.hip), else 0. */
int mpnhip_edge_chain_active(const mpnhip_model* model);
int mpnhip_profile_read(float* gemm_avg_us, int* gemm_launches, float* agg_avg_us, int* agg_launches,
                        float* empty_pair_us /* cost of an event pair with nothing between, for calibration */);

/* The same hooks, one kernel kind at a time: MPNHIP_PROF_CHAIN = the kernel mpnhip_profile_read reports as "gemm" (forward),
 * _AGG = the aggregation kernel, _CHAIN_BWD = the fused backward chain of mpnhip_backward, _WEIGHT_GRAD = the MFMA
 * weight-gradient product kernel (gemm_tn_kernel; launched on the library's side stream as well as on the caller's -- the events
 * are attached to each dispatch on whatever stream it goes to).  avg_work: average algorithmic flops per timed launch (only
 * _WEIGHT_GRAD reports it: its launches differ in shape).  Synchronises and resets the kind's counters. */
#define MPNHIP_PROF_CHAIN 0
#define MPNHIP_PROF_AGG 1
#define MPNHIP_PROF_CHAIN_BWD 2
#define MPNHIP_PROF_WEIGHT_GRAD 3
int mpnhip_profile_read_kind(int kind, float* avg_us, int* launches, double* avg_work);

/* Average duration in microseconds of `iters` back-to-back launches of the aggregation kernel on
 * a prepared graph: src [E, dim] in SORTED edge order, out [N, 2*dim]. */
int mpnhip_time_aggregate(const void* graph_buf, int n_nodes, int64_t n_edges, const float* src, int dim, int agg,
                          float* out, int iters, float* avg_us, void* stream);
/* Average duration (us) of `iters` back-to-back mpnhip_weight_grad calls (product + slab sum). */
int mpnhip_time_weight_grad(const float* dZ, const float* H, int64_t rows, int n_out, int k_in, int nbatch, float* grad_w, float* grad_b,
                            void* workspace, size_t workspace_bytes, int iters, float* avg_us, void* stream);
int mpnhip_time_weight_grad_prec(const float* dZ, const float* H, int64_t rows, int n_out, int k_in, int nbatch, int precision, float* grad_w,
                                 float* grad_b, void* workspace, size_t workspace_bytes, int iters, float* avg_us, void* stream);
/* Average duration (us) of `iters` launches of y = relu(x W^T + b). */
int mpnhip_time_linear(const float* x, const float* w, const float* b, float* y, int64_t m, int n, int k, int iters,
                       float* avg_us, void* stream);

/* Average duration (us) of `iters` launches of mpnhip_linear_bf16. */
int mpnhip_time_linear_bf16(const mpnhip_linear_bf16_args* args, int iters, float* avg_us, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MPNHIP_H */
