// Weight-gradient products, host side: the ONE route from a product's description (WgProduct, common.h) to the kernels, and the C-ABI
// entries that go through it.  No kernel lives here.
//   weight_grad_route   row-panel kernels (wgrad_panel.hip / wgrad_rows16.hip) for a split / bf16 product of their shapes -- recorded
//                       into the caller's batch or run as a batch of its own -- else the fp32 kernels (gemm_tn.hip)
//   callers             the backward (backward.hip: weight_grad), mpnhip_weight_grad / _prec / _bf16_rows and their timing forms,
//                       the test entry mpnhip_debug_weight_grad_batch
// The two device-facing forms are each filled from a WgProduct in one place: TnArgs in tn_args_of below, WpJob in wp_batch_add.
#include <algorithm>
#include <cstring>

#include "common.h"

namespace mpnhip {

// the product as the fp32 kernels see it: group q's slab at slabs.base + q * slabs.group_stride
static TnArgs tn_args_of(const WgProduct& w, const WgSlabs& slabs) {
    const bool ranged = w.g[0].rr.begin || w.g[0].rr.end;
    TnArgs a = {};
    a.ngroups = wg_ngroups(w);
    a.n_out = w.n_out; a.k_in = w.k_in; a.csplit = w.H2.p ? w.csplit : w.k_in;
    a.m_upper = w.rows; a.nbatch = w.nbatch;
    // (with device-side row ranges the groups partition the `rows` rows between them; without, each group covers all of them)
    a.flops = 2.0 * (double)w.rows * (ranged ? 1 : a.ngroups) * w.nbatch * w.n_out * w.k_in;
    for (int q = 0; q < a.ngroups; ++q) {
        TnGroup& g = a.g[q];
        g.dZ = w.dZ.p; g.ldz = w.dZ.ld; g.z_bstride = w.dZ.bstride; g.dz_idx = w.dz_idx;
        g.H = w.H.p; g.ldh = w.H.ld; g.h_bstride = w.H.bstride; g.h_idx = w.h_idx;
        g.H2 = w.H2.p; g.ldh2 = w.H2.ld; g.h2_bstride = w.H2.bstride;
        g.row_begin = w.g[q].rr.begin; g.row_end = w.g[q].rr.end; g.m_static = w.rows;
        g.grad_w = w.g[q].grad_w; g.ldw = w.ldw; g.grad_b = w.g[q].grad_b;
        g.slab = slabs.base + q * slabs.group_stride;
    }
    return a;
}

int weight_grad_route(const WgRouting& c, const WgSlabs& slabs, WpBatch* batch, const WgProduct& w, hipStream_t s, WgChosen* chosen) {
    const int ngroups = wg_ngroups(w);
    if (chosen)
        for (int q = 0; q < 2; ++q) chosen[q] = {WG_PATH_NONE, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (c.wgrad_split && w.rows > 0) {
        // MPNHIP_PREC_FP32_SPLIT / _BF16: the row-panel kernels (wgrad_panel.hip)
        const int pieces = c.bf16 ? 1 : 3;
        if (batch) {
            if (wp_batch_add(batch, w, pieces, chosen)) return MPNHIP_OK;
            if (wp_eligible(w, pieces)) {
                // the batch is full (more than WP_MAX_JOBS jobs in a group of steps: deeper MLPs; or its slab region): run it
                // and go on in a fresh one rather than switch kernels in the middle of a group
                int st = MPNHIP_OK;
                if (wp_batch_roll(batch, &st) && wp_batch_add(batch, w, pieces, chosen)) {
                    if (chosen)
                        for (int q = 0; q < ngroups; ++q) chosen[q].rolled = 1;
                    return MPNHIP_OK;
                }
                MPN_TRY(st);
            }
        } else {
            WpBatch own;
            wp_batch_init(&own, slabs.base, slabs.own_floats, false, nullptr);
            if (wp_batch_add(&own, w, pieces, chosen)) return wp_batch_flush(&own, s);
        }
        // not a shape / alignment of the row-panel kernel (or the batch cannot be rolled): the fp32 kernel below, counted
        count_path(PC_TN_PANEL_FALLBACK);
        if (w.src16) return MPNHIP_ERR_UNSUPPORTED;   // (no fp32 kernel reads bf16 rows: the caller words the refusal)
    }
    return launch_gemm_tn(tn_args_of(w, slabs), s, chosen);
}

}  // namespace mpnhip

using namespace mpnhip;

// ---- the public entries: one group, contiguous blocks (ld = width, batch stride = rows * width) ------------------------------------
// One slab -- the larger of the split-row and the row-panel form's (MPNHIP_PREC_FP32_SPLIT / _BF16); rows16: the row-panel form over
// bf16 rows only -- behind a base the operator rounds up to 256 itself (callers may pass unaligned buffers): 256 bytes to spare.
static size_t weight_grad_layout(int n_out, int k_in, int64_t rows, int nbatch, bool rows16, void* workspace, float** slab) {
    const int nb = nbatch < 1 ? 1 : nbatch;
    const size_t tn = rows16 ? 0 : tn_slab_floats(n_out, k_in, rows, nb), wp = rows > 0 ? wp_slab_floats(n_out, k_in, rows, nb, false, false, rows16) : 0;
    const uintptr_t w = reinterpret_cast<uintptr_t>(workspace);
    Carver c(workspace ? static_cast<char*>(workspace) + (align_up(w, 256) - w) : nullptr);
    *slab = c.take<float>(tn > wp ? tn : wp);
    return c.bytes() + 256;
}

static WgProduct contiguous_product(const void* dZ, const void* H, int64_t rows, int n_out, int k_in, int nbatch, bool src16, float* grad_w,
                                    float* grad_b) {
    WgProduct w = {};
    w.dZ = {static_cast<const float*>(dZ), n_out, rows * n_out};
    w.H = {static_cast<const float*>(H), k_in, rows * k_in};
    w.n_out = n_out; w.k_in = k_in; w.ldw = k_in; w.rows = rows; w.nbatch = nbatch; w.src16 = src16;
    w.g[0] = {grad_w, grad_b, {}};
    return w;
}
// (a batch of its own may use all of the caller's buffer, as far as it is known to reach behind the rounded-up base)
static WgSlabs caller_slabs(float* slab, size_t workspace_bytes) { return {slab, (workspace_bytes - 256) / sizeof(float), 0}; }

extern "C" size_t mpnhip_weight_grad_workspace_bytes(int n_out, int k_in, int64_t rows, int nbatch) {
    float* slab;
    return n_out < 1 || k_in < 1 || rows < 0 ? 0 : weight_grad_layout(n_out, k_in, rows, nbatch, false, nullptr, &slab);
}

struct WgCall { WgRouting r; WgSlabs slabs; WgProduct w; };   // what a checked public call hands to the route
static int weight_grad_checked(const char* name, const float* dZ, const float* H, int64_t rows, int n_out, int k_in, int nbatch, int precision,
                               float* grad_w, float* grad_b, void* workspace, size_t workspace_bytes, WgCall* call) {
    MPN_CHECK_ARG(precision == MPNHIP_PREC_FP32 || precision == MPNHIP_PREC_FP32_SPLIT || precision == MPNHIP_PREC_BF16, "%s: precision %d", name, precision);
    MPN_CHECK_ARG(n_out >= 1 && k_in >= 1 && rows >= 0 && nbatch >= 1, "weight_grad: bad sizes");
    MPN_CHECK_ARG((dZ && H && grad_w) || rows == 0, "weight_grad: null pointer");
    float* slab;
    const size_t need = weight_grad_layout(n_out, k_in, rows, nbatch, false, workspace, &slab);
    if (rows > 0) MPN_CHECK_WORKSPACE("weight_grad", workspace, workspace_bytes, need);
    *call = {{precision != MPNHIP_PREC_FP32, precision == MPNHIP_PREC_BF16}, caller_slabs(slab, workspace_bytes),
             contiguous_product(dZ, H, rows, n_out, k_in, nbatch, false, grad_w, grad_b)};
    return MPNHIP_OK;
}

// precision MPNHIP_PREC_FP32_SPLIT / _BF16: the row-panel kernels (three-piece / rounded bf16 operands) where the shape allows it
extern "C" int mpnhip_weight_grad_prec(const float* dZ, const float* H, int64_t rows, int n_out, int k_in, int nbatch, int precision,
                                       float* grad_w, float* grad_b, void* workspace, size_t workspace_bytes, void* stream) {
    WgCall c;
    MPN_TRY(weight_grad_checked("weight_grad", dZ, H, rows, n_out, k_in, nbatch, precision, grad_w, grad_b, workspace, workspace_bytes, &c));
    if (rows == 0) return MPNHIP_OK;
    return weight_grad_route(c.r, c.slabs, nullptr, c.w, static_cast<hipStream_t>(stream));
}

extern "C" int mpnhip_weight_grad_bf16_rows(const uint16_t* dZ, const uint16_t* H, int64_t rows, int n_out, int k_in, int nbatch,
                                            float* grad_w, float* grad_b, void* workspace, size_t workspace_bytes, void* stream) {
    MPN_CHECK_ARG(n_out >= 1 && k_in >= 1 && rows >= 0 && nbatch >= 1, "weight_grad_bf16_rows: bad sizes");
    if (rows == 0) return MPNHIP_OK;
    MPN_CHECK_ARG(dZ && H && grad_w, "weight_grad_bf16_rows: null pointer");
    float* slab;
    const size_t need = weight_grad_layout(n_out, k_in, rows, nbatch, true, workspace, &slab);
    MPN_CHECK_WORKSPACE("weight_grad_bf16_rows", workspace, workspace_bytes, need);
    const int rc = weight_grad_route({true, true}, caller_slabs(slab, workspace_bytes), nullptr,
                                     contiguous_product(dZ, H, rows, n_out, k_in, nbatch, true, grad_w, grad_b), static_cast<hipStream_t>(stream));
    if (rc == MPNHIP_ERR_UNSUPPORTED)
        set_error("weight_grad_bf16_rows: [%d x %d] over bf16 rows is not a shape of the row-panel kernel (multiples of 4, 8-byte aligned rows)", n_out, k_in);
    return rc;
}

extern "C" size_t mpnhip_weight_grad_bf16_rows_workspace_bytes(int n_out, int k_in, int64_t rows, int nbatch) {
    float* slab;
    return n_out < 1 || k_in < 1 || rows < 0 ? 0 : weight_grad_layout(n_out, k_in, rows, nbatch, true, nullptr, &slab);
}

extern "C" int mpnhip_weight_grad(const float* dZ, const float* H, int64_t rows, int n_out, int k_in, int nbatch, float* grad_w,
                                  float* grad_b, void* workspace, size_t workspace_bytes, void* stream) {
    return mpnhip_weight_grad_prec(dZ, H, rows, n_out, k_in, nbatch, MPNHIP_PREC_FP32, grad_w, grad_b, workspace, workspace_bytes, stream);
}

extern "C" int mpnhip_time_weight_grad_prec(const float* dZ, const float* H, int64_t rows, int n_out, int k_in, int nbatch, int precision,
                                            float* grad_w, float* grad_b, void* workspace, size_t workspace_bytes, int iters, float* avg_us,
                                            void* stream_) {
    hipStream_t s = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(avg_us && iters > 0 && rows > 0, "time_weight_grad: bad argument");
    WgCall c;
    MPN_TRY(weight_grad_checked("time_weight_grad", dZ, H, rows, n_out, k_in, nbatch, precision, grad_w, grad_b, workspace, workspace_bytes, &c));
    hipEvent_t t0, t1;
    MPN_HIP(hipEventCreate(&t0));
    MPN_HIP(hipEventCreate(&t1));
    MPN_TRY(weight_grad_route(c.r, c.slabs, nullptr, c.w, s));
    MPN_HIP(hipEventRecord(t0, s));
    for (int i = 0; i < iters; ++i) MPN_TRY(weight_grad_route(c.r, c.slabs, nullptr, c.w, s));
    MPN_HIP(hipEventRecord(t1, s));
    MPN_HIP(hipEventSynchronize(t1));
    float ms = 0.f;
    MPN_HIP(hipEventElapsedTime(&ms, t0, t1));
    *avg_us = ms * 1000.f / iters;
    (void)hipEventDestroy(t0);
    (void)hipEventDestroy(t1);
    return MPNHIP_OK;
}

extern "C" int mpnhip_time_weight_grad(const float* dZ, const float* H, int64_t rows, int n_out, int k_in, int nbatch, float* grad_w,
                                       float* grad_b, void* workspace, size_t workspace_bytes, int iters, float* avg_us, void* stream_) {
    return mpnhip_time_weight_grad_prec(dZ, H, rows, n_out, k_in, nbatch, MPNHIP_PREC_FP32, grad_w, grad_b, workspace, workspace_bytes, iters,
                                        avg_us, stream_);
}

// ---- test instrumentation: the backward's weight-gradient routing (weight_grad_route) behind the C ABI ---------------------------
// Workspace: [ two groups' slabs for a product that runs on its own (and the fp32 kernels) | the slab region of the batch ]
namespace {
struct WgDebugLayout { float* own; size_t per_group; float* batch; size_t batch_floats; };
bool wg_ranged(const mpnhip_wgrad_product& p) { return p.g[0].row_begin || p.g[0].row_end; }
size_t wg_debug_layout(const mpnhip_wgrad_product* ps, int n, int precision, int batched, int64_t batch_slab_floats, void* workspace,
                       WgDebugLayout* out) {
    size_t per_group = 0, sum = 0;
    for (int i = 0; i < n; ++i) {
        const mpnhip_wgrad_product& p = ps[i];
        if (p.rows <= 0 || p.n_out < 1 || p.k_in < 1 || p.nbatch < 1) continue;
        const size_t tn = p.src16 ? 0 : tn_slab_floats(p.n_out, p.k_in, p.rows, p.nbatch);
        const size_t own = wp_slab_floats(p.n_out, p.k_in, p.rows, p.nbatch, wg_ranged(p), false, p.src16 != 0);
        per_group = std::max(per_group, std::max(tn, own));
        sum += (p.g[1].grad_w ? 2 : 1) * wp_slab_floats(p.n_out, p.k_in, p.rows, p.nbatch, wg_ranged(p), batched != 0, p.src16 != 0);
    }
    per_group = (per_group + 63) / 64 * 64;
    const uintptr_t w = reinterpret_cast<uintptr_t>(workspace);
    Carver c(workspace ? static_cast<char*>(workspace) + (align_up(w, 256) - w) : nullptr);
    out->per_group = per_group;
    out->own = c.take<float>(2 * per_group);
    out->batch_floats = precision == MPNHIP_PREC_FP32 ? 0 : (batch_slab_floats > 0 ? (size_t)batch_slab_floats : sum);
    out->batch = c.take<float>(out->batch_floats);
    return c.bytes() + 256;
}
int wg_debug_check(const mpnhip_wgrad_product* ps, int n, int precision) {
    MPN_CHECK_ARG(ps, "debug_weight_grad_batch: null products");
    MPN_CHECK_ARG(n >= 1 && n <= WP_MAX_JOBS, "debug_weight_grad_batch: %d products (1 .. %d)", n, WP_MAX_JOBS);
    MPN_CHECK_ARG(precision == MPNHIP_PREC_FP32 || precision == MPNHIP_PREC_FP32_SPLIT || precision == MPNHIP_PREC_BF16,
                  "debug_weight_grad_batch: unknown precision %d", precision);
    for (int i = 0; i < n; ++i) {
        const mpnhip_wgrad_product& p = ps[i];
        MPN_CHECK_ARG(p.n_out >= 1 && p.k_in >= 1 && p.rows >= 0 && p.nbatch >= 1 && p.ldw >= p.k_in, "debug_weight_grad_batch: product %d: bad sizes", i);
        MPN_CHECK_ARG(p.rows == 0 || (p.dZ && p.H && p.g[0].grad_w), "debug_weight_grad_batch: product %d: null dZ / H / grad_w", i);
        MPN_CHECK_ARG(!p.src16 || precision == MPNHIP_PREC_BF16, "debug_weight_grad_batch: product %d: src16 needs the bf16 precision", i);
        MPN_CHECK_ARG(!p.H2 || (p.csplit > 0 && p.csplit < p.k_in), "debug_weight_grad_batch: product %d: csplit %d outside (0, %d)", i, p.csplit,
                      p.k_in);
    }
    return MPNHIP_OK;
}
}  // namespace

extern "C" size_t mpnhip_debug_weight_grad_batch_workspace_bytes(const mpnhip_wgrad_product* products, int n_products, int precision,
                                                                 int batched, int64_t batch_slab_floats) {
    if (wg_debug_check(products, n_products, precision) != MPNHIP_OK) return 0;
    WgDebugLayout L;
    return wg_debug_layout(products, n_products, precision, batched, batch_slab_floats, nullptr, &L);
}

extern "C" int mpnhip_debug_weight_grad_batch(const mpnhip_wgrad_product* products, int n_products, int precision, int batched, int one_launch,
                                              int64_t batch_slab_floats, void* workspace, size_t workspace_bytes, int32_t* chosen,
                                              void* stream_) {
    MPN_TRY(wg_debug_check(products, n_products, precision));
    WgDebugLayout L;
    const size_t need = wg_debug_layout(products, n_products, precision, batched, batch_slab_floats, workspace, &L);
    MPN_CHECK_WORKSPACE("debug_weight_grad_batch", workspace, workspace_bytes, need);
    hipStream_t s = static_cast<hipStream_t>(stream_);
    const WgRouting r = {precision != MPNHIP_PREC_FP32, precision == MPNHIP_PREC_BF16};
    static_assert(sizeof(WgChosen) == 10 * sizeof(int32_t), "the chosen report is ten ints per group");
    WgChosen ch[WP_MAX_JOBS][2];
    for (int i = 0; i < n_products; ++i)
        for (int q = 0; q < 2; ++q) ch[i][q] = {WG_PATH_NONE, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    // one_launch: one batch for all products; else batched: a batch per product (a job with the batched chunk plan, alone in its
    // launch); else: no batch -- the routing runs the product now, on a batch of its own
    WpBatch wpb;
    const bool use_batch = r.wgrad_split && (one_launch || batched);
    if (use_batch) wp_batch_init(&wpb, L.batch, L.batch_floats, batched != 0, &s);
    int rc = MPNHIP_OK;
    for (int i = 0; i < n_products && rc == MPNHIP_OK; ++i) {
        const mpnhip_wgrad_product& p = products[i];
        WgProduct w = {};   // (the ABI boundary: the flat mirror, field by field)
        w.dZ = {static_cast<const float*>(p.dZ), p.ldz, p.z_bstride};
        w.dz_idx = p.dz_idx;
        w.H = {static_cast<const float*>(p.H), p.ldh, p.h_bstride};
        w.H2 = {static_cast<const float*>(p.H2), p.ldh2, p.h2_bstride};
        w.csplit = p.csplit;
        w.h_idx = p.h_idx;
        w.n_out = p.n_out; w.k_in = p.k_in; w.ldw = p.ldw; w.rows = p.rows; w.nbatch = p.nbatch; w.src16 = p.src16 != 0;
        for (int q = 0; q < 2; ++q) w.g[q] = {p.g[q].grad_w, p.g[q].grad_b, {p.g[q].row_begin, p.g[q].row_end}};
        rc = weight_grad_route(r, wg_two_group_slabs(L.own, L.per_group), use_batch ? &wpb : nullptr, w, s, ch[i]);
        if (rc == MPNHIP_ERR_UNSUPPORTED)
            set_error("debug_weight_grad_batch: product %d over bf16 rows [%d x %d] is not covered by the row-panel kernel", i, p.n_out, p.k_in);
        if (rc == MPNHIP_OK && use_batch && !one_launch) {
            rc = wp_batch_flush(&wpb, s);
            wp_batch_init(&wpb, L.batch, L.batch_floats, batched != 0, &s);
        }
    }
    if (rc == MPNHIP_OK && use_batch && one_launch) rc = wp_batch_flush(&wpb, s);
    if (chosen) memcpy(chosen, ch, sizeof(WgChosen) * 2 * (size_t)n_products);
    return rc;
}
