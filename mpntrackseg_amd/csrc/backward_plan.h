// Workspace planning of the backward (backward.hip): the forward's plan is in plan.h.  Everything here is host code; offsets and
// sizes are a pure function of (model dims, N, E).
#pragma once
#include "common.h"
#include "edge_chain.h"
#include "plan.h"

namespace mpnhip {

// zero-padded copies of the per-edge weights for the fused backward chain kernel (edge_chain.hip: native [n][k] orientation, or the
// same logical images as three-piece split images): ONE layout and ONE packer for the backward's plan and for
// mpnhip_debug_edge_chain_backward (edge_chain.h: ChainBwdImages; each sized for either operand form)
static inline void carve_chain_bwd_images(Carver& a, const Dims& d, ChainBwdImages* im) {
    const size_t HE = pad32(d.he), DE = pad32(d.de), HN = pad32(d.hn), DN = pad32(d.dn);
    for (int q = 0; q < 2; ++q) { im->wf2p[q] = a.take<float>(chain_image_capacity(DN * HN)); im->wfep[q] = a.take<float>(chain_image_capacity(HN * DE)); }
    im->wc1p = a.take<float>(chain_image_capacity(CHAIN_HC * DE));
    im->w2p = a.take<float>(chain_image_capacity(DE * HE));
    im->w1ep = a.take<float>(chain_image_capacity(HE * 2 * DE));
}
// ... and the pair images of the bf16-operand backward chain kernel (edge_chain_bf16_bwd.hip): edge | classifier | flow_out | flow_in
struct ChainBf16BwdImages { char* img; size_t off_cls, off_flow[2]; };
static inline void carve_chain_bf16_bwd_images(Carver& a, const mpnhip_model& m, const Dims& d, ChainBf16BwdImages* im) {
    im->img = a.take<char>(chain_bf16_bwd_image_bytes(d.he, d.de, d.hn, d.dn, m.classifier.out_dims[0], &im->off_cls, &im->off_flow[0],
                                                      &im->off_flow[1]));
}
// (backward.hip)
int pack_chain_bwd_weights(const mpnhip_model& m, const Dims& d, const ChainBwdImages& im, bool split, hipStream_t s);
int pack_chain_bf16_bwd_weights(const mpnhip_model& m, const Dims& d, const ChainBf16BwdImages& im, hipStream_t s);

// ------------------------------------------------------------------------------------ plan
// Pre-activation gradients (dZ) of EVERY step are kept ([L][rows][width] blocks): the activation-gradient
// chain of a step reads its predecessor's block, and after the step loop each weight's gradient is ONE
// batched split-row product over all L steps (12x fewer launches and slab reductions than per step).
struct BwdPlan {
    float* dX[2];                       // [N, dn] ping-pong: gradient w.r.t. x_s
    float* dXh;                         // [N, dn] second K half of the per-node projection's activation gradient (split product)
    float* dX0;                         // [N, dn] gradient w.r.t. the encoder's node output
    float* dE0;                         // [E, de]
    float* dAGG;                        // [N, 2dn]
    float* dCat;                        // [max(E ke, N kx)] gradient w.r.t. the concatenated [initial | current] features
    float* dPsum;                       // [N, pw] sum over the steps of dP (the re-attached x0's share is one product)
    float* dZ1sum;                      // [E, he] sum over the steps of the edge MLP's first-layer dZ (the re-attached e0's share)
    float* dZn;                         // [L][N, dn]
    float* dP;                          // [L][N, pw]
    unsigned short* dP16;               // bf16-operand training: the same blocks rounded to bf16 rows (the node-level weight-gradient
    unsigned short* dPsum16;            // products over bf16 rows, wgrad_rows16.hip), and the rounded sum over the steps [N, pw]
    unsigned short* dZn16;              // ... and the node update's operands: [L][N, dn] pre-activation gradients, [L][N, 2 dn] aggregated
    unsigned short* AGG16;              // messages, rounded on the side stream just before the group's products
    unsigned short* enc16;              // ... and the node encoder's dZ / input blocks [N, sum of (out_i + in_i)] (rounded on the tail's stream)
    size_t enc16_elems;
    float* dZfl[MPNHIP_MAX_LAYERS];     // flow MLP layer i:   [L][E, out_i]
    float* dZed[MPNHIP_MAX_LAYERS];     // edge MLP layer i:   [L][E, out_i]  (last layer: the masked dE_s)
    float* dZcl[MPNHIP_MAX_LAYERS];     // classifier layer i: [L][E, out_i]  (i < n-1; the last one is grad_logits)
    float* T[3];                        // edge-encoder chain scratch [E, max encoder width], rotating (layer i -> buffer (n - 1 - i) % 3)
    float* Tn[3];                       // node-encoder chain scratch [N, max encoder width]: chains of <= 3 layers never overwrite a
                                        // dZ block, so their weight-gradient products may run later, on another stream
    int t_width;                        // that width (floats per row)
    // zero-padded copies of the per-edge weights for the fused backward chain (native [n][k] orientation)
    float* wf2p[2]; float* wfep[2]; float* wc1p; float* w2p; float* w1ep;
    float* gWnode;                      // [pw, kx] gradient of the packed node-projection weights
    float* zero_end;                    // end of the run dX[0] | dX0 | dE0 | gWnode that a backward zero-fills at once
    unsigned short* ncb_img;            // unit images of the fused node-side backward kernel (node_chain.hip) or nullptr
    float* wt_scratch;                  // MPNHIP_PREC_BF16: transposed weight blocks of the activation-gradient products
    size_t wt_scratch_floats;
    float* wt_keep[2];                  // ... the node update's (0) and the projections' (1) blocks, transposed once per backward
    size_t wt_keep_floats[2];
    unsigned short* wt_keep16[2];       // ... and their bf16 images: the B operand of the tiled bf16 GEMM as bf16 rows (gemm_bf16.hip)
    // bf16-operand training on the fused kernels (FwdPlan::b16): the dZ blocks above are bf16 rows (half the floats), the gradient
    // w.r.t. e_s travels between the steps in two fp32 buffers, and the backward chain kernel has its own pair images
    bool b16;
    float* dEpp[2];                     // [E, de] fp32 ping-pong
    char* cb16_img;                     // backward pair images (edge | classifier | flow_out | flow_in)
    size_t cb16_off_cls, cb16_off_flow[2];
    float* slab;                        // split partials of the weight-gradient products (2 groups)
    float* slab_side;                   // the same for the products issued on the side stream
    size_t slab_floats_per_group;
    float* slab_wp;                     // slabs of a batch of row-panel products (all jobs of one group of steps)
    size_t slab_wp_floats;
    float* slab_tail;                   // slabs of the tail batch (hoisted shares + encoder layers)
    size_t slab_tail_floats;
    size_t total;
};

static inline int enc_maxw(const mpnhip_model& m, const Dims& d) {
    int w = d.dn > d.de ? d.dn : d.de;
    const mpnhip_mlp* all[] = {&m.enc_node, &m.enc_edge};
    for (const mpnhip_mlp* p : all)
        for (int i = 0; i < p->n_layers; ++i) w = p->out_dims[i] > w ? p->out_dims[i] : w;
    return w;
}

// slab floats of the weight-gradient products of an MLP's layers (layer 0's k_in given: the share of the input it is taken over)
static inline size_t mlp_slab(const mpnhip_mlp& m, int k_in0, int64_t rows, int nbatch) {
    size_t mx = 0;
    for (int i = 0; i < m.n_layers; ++i) {
        size_t f = tn_slab_floats(m.out_dims[i], i == 0 ? k_in0 : m.out_dims[i - 1], rows, nbatch);
        mx = f > mx ? f : mx;
    }
    return mx;
}

// slab floats of one row-panel product inside a batch: its fp32-row form or, where the operands may be bf16 rows, the larger of the two
static inline size_t wp_slab_either(int n_out, int k_in, int64_t rows, int nb, bool ranged, bool rows16) {
    if (rows <= 0) return 0;
    const size_t f32 = wp_slab_floats(n_out, k_in, rows, nb, ranged, true), f16 = rows16 ? wp_slab_floats(n_out, k_in, rows, nb, ranged, true, true) : 0;
    return f32 > f16 ? f32 : f16;
}

// The slabs of the weight-gradient products, in three parts.  Each lists exactly the products mpnhip_backward launches in that form
// (the slab size depends on the shape through tn_plan / the row-panel chunking); node16: the node-level products run over bf16 rows.
// The methods of BackwardRun (backward.hip) that issue them: BackwardRun::mp_weight_grads (the groups of steps),
// BackwardRun::hoisted_shares, BackwardRun::classifier_only and the encoder methods (encoder_node_bwd, encoder_edge_bwd) -- a
// product added to one of them is added here, and the other way round.
// 1. one product alone on a stream: floats of the LARGEST one (BwdPlan::slab and slab_side hold two direction groups of it)
static inline size_t slab_per_group(const mpnhip_model& m, const Dims& d, int64_t N, int64_t E, int L, bool b16, bool node16) {
    size_t sl = 0;
    auto upd = [&](size_t f) { sl = f > sl ? f : sl; };
    upd(mlp_slab(m.enc_node, m.enc_node.in_dim, N, 1));
    upd(mlp_slab(m.enc_edge, m.enc_edge.in_dim, E, 1));
    upd(mlp_slab(m.edge, d.ke, E, L));
    for (int nb = 1; nb <= L; ++nb) upd(tn_slab_floats(d.he, d.de, E, nb));   // (the e0-hoisted forms of the edge layer-0 product)
    upd(mlp_slab(m.flow_in, d.de, E, L));
    upd(mlp_slab(m.classifier, d.de, E, L));
    upd(tn_slab_floats(d.dn, 2 * d.dn, N, L));
    upd(tn_slab_floats(d.pw, d.kx, N, L));
    // the same products in the row-panel form (MPNHIP_PREC_FP32_SPLIT), each a batch of its own over both groups' shares (common.h)
    auto updw = [&](int n_out, int k_in, int64_t rows, bool rows16) { if (rows > 0) upd(wg_group_share(wp_slab_floats(n_out, k_in, rows, 1, false, false, rows16))); };
    for (int i = 0; i < m.enc_node.n_layers; ++i) updw(m.enc_node.out_dims[i], layer_in(m.enc_node, i), N, false);
    for (int i = 0; i < m.enc_edge.n_layers; ++i) updw(m.enc_edge.out_dims[i], layer_in(m.enc_edge, i), E, false);
    updw(d.he, d.de, E, false);
    if (b16) updw(d.he, d.de, E, true);      // (the hoisted e0 share over bf16 rows)
    updw(d.pw, d.dn, N, false);
    if (node16) updw(d.pw, d.dn, N, true);   // (the hoisted x0 share over bf16 rows)
    for (int i = 0; i < m.classifier.n_layers; ++i) updw(m.classifier.out_dims[i], layer_in(m.classifier, i), E, false);
    return sl;
}

// 2. all products of a group of nb steps in one batch (BackwardRun::mp_weight_grads): every job has its own slabs, so their SUM
static inline size_t slab_batched(const mpnhip_model& m, const Dims& d, int64_t N, int64_t E, int nb, bool b16) {
    size_t t = 0;
    auto wp = [&](int n_out, int k_in, int64_t rows, bool ranged) { return wp_slab_either(n_out, k_in, rows, nb, ranged, b16); };
    t += wp(d.dn, 2 * d.dn, N, false);
    for (int i = 1; i < m.flow_in.n_layers; ++i) t += 2 * wp(m.flow_in.out_dims[i], layer_in(m.flow_in, i), E, true);   // (flow_in and flow_out)
    t += 2 * wp(d.hn, d.de, E, true);
    for (int i = 0; i < m.classifier.n_layers; ++i) t += wp(m.classifier.out_dims[i], layer_in(m.classifier, i), E, false);
    for (int i = 1; i < m.edge.n_layers; ++i) t += wp(m.edge.out_dims[i], layer_in(m.edge, i), E, false);
    // (a product that runs in one of two forms -- the first-layer inputs whole or with the re-attached share hoisted -- reserves
    // the larger of the two: a narrower k_in can mean MORE row chunks, i.e. more slabs)
    auto larger = [](size_t x, size_t y) { return x > y ? x : y; };
    t += larger(wp(d.he, d.ke, E, false), wp(d.he, d.de, E, false));
    t += larger(wp(d.pw, d.kx, N, false), wp(d.pw, d.dn, N, false));
    return t;
}

// 3. the tail batch (BackwardRun::hoisted_shares and the encoder methods record into it): hoisted shares + encoder layers, their sum
static inline size_t slab_tail(const mpnhip_model& m, const Dims& d, int64_t N, int64_t E, bool b16, bool node16) {
    size_t t = 0;
    t += wp_slab_either(d.pw, d.dn, N, 1, false, node16);
    t += wp_slab_either(d.he, d.de, E, 1, false, b16);   // (bf16-operand training keeps S = sum_s dZ1_s as bf16 rows: the bf16-row kernels' chunking)
    for (int i = 0; i < m.enc_node.n_layers; ++i) t += wp_slab_either(m.enc_node.out_dims[i], layer_in(m.enc_node, i), N, 1, false, node16);
    for (int i = 0; i < m.enc_edge.n_layers; ++i) t += wp_slab_either(m.enc_edge.out_dims[i], layer_in(m.enc_edge, i), E, 1, false, false);
    return t;
}

// fr: the route of the training forward whose saves this backward reads (plan.h fwd_route with save = 1)
static inline size_t plan_backward(const mpnhip_model& m, const Dims& d, const FwdRoute& fr, int64_t N, int64_t E, void* base, BwdPlan* out) {
    Carver a(base);
    BwdPlan p = {};
    const size_t L = d.L > 0 ? d.L : 1;
    // (what every backward starts from as zeros lies side by side -- dX[0] | dX0 | dE0 | gWnode: ONE fill instead of four, ~12 us of
    // the 0.5 ms step of a KITTIMOTS-size graph)
    p.dX[0] = a.take<float>((size_t)N * d.dn);
    p.dX0 = a.take<float>((size_t)N * d.dn);
    p.dE0 = a.take<float>((size_t)E * d.de);
    p.gWnode = a.take<float>((size_t)d.pw * d.kx);
    p.zero_end = a.take<float>(0);
    p.dX[1] = a.take<float>((size_t)N * d.dn);
    p.dXh = a.take<float>((size_t)N * d.dn);
    p.dPsum = a.take<float>((size_t)N * d.pw);
    p.dZ1sum = a.take<float>((size_t)E * d.he);
    p.dAGG = a.take<float>((size_t)N * 2 * d.dn);
    {
        size_t a1 = (size_t)E * d.ke, a2 = (size_t)N * d.kx;
        p.dCat = a.take<float>(a1 > a2 ? a1 : a2);
    }
    p.dZn = a.take<float>(L * N * d.dn);
    p.dP = a.take<float>(L * N * d.pw);
    p.b16 = fr.b16;
    p.dP16 = p.dPsum16 = p.dZn16 = p.AGG16 = p.enc16 = nullptr;
    p.enc16_elems = 0;
    const bool node16 = p.b16 && d.pw % 8 == 0 && d.dn % 8 == 0;   // (not `p.dP16 != nullptr`: a size query plans without a base)
    if (node16) {
        p.dP16 = a.take<unsigned short>(L * N * d.pw);
        p.dPsum16 = a.take<unsigned short>((size_t)N * d.pw);
        p.dZn16 = a.take<unsigned short>(L * N * d.dn);
        p.AGG16 = a.take<unsigned short>(L * N * 2 * d.dn);
        size_t w = 0;
        for (int i = 0; i < m.enc_node.n_layers; ++i) w += (size_t)m.enc_node.out_dims[i] + layer_in(m.enc_node, i);
        p.enc16_elems = (size_t)N * w;
        p.enc16 = a.take<unsigned short>(p.enc16_elems);
    }
    // (b16: the dZ blocks are bf16 rows)
    auto dzb = [&](int width) { return a.take_as<float>(L * E * width, p.b16 ? sizeof(unsigned short) : sizeof(float)); };
    for (int i = 0; i < m.flow_in.n_layers; ++i) p.dZfl[i] = dzb(m.flow_in.out_dims[i]);
    for (int i = 0; i < m.edge.n_layers; ++i) p.dZed[i] = dzb(m.edge.out_dims[i]);
    for (int i = 0; i + 1 < m.classifier.n_layers; ++i) p.dZcl[i] = dzb(m.classifier.out_dims[i]);
    p.dEpp[0] = p.dEpp[1] = nullptr;
    p.cb16_img = nullptr;
    if (p.b16) {
        for (int i = 0; i < 2; ++i) p.dEpp[i] = a.take<float>((size_t)E * d.de);
        ChainBf16BwdImages im;
        carve_chain_bf16_bwd_images(a, m, d, &im);
        p.cb16_img = im.img; p.cb16_off_cls = im.off_cls; p.cb16_off_flow[0] = im.off_flow[0]; p.cb16_off_flow[1] = im.off_flow[1];
    }
    int mw = enc_maxw(m, d);
    if (mw < 52) mw = 52;   // (the fused reference edge encoder keeps dz2 | dz1 | dz0 side by side in T[0])
    for (int i = 0; i < 3; ++i) p.T[i] = a.take<float>((size_t)E * mw);
    for (int i = 0; i < 3; ++i) p.Tn[i] = a.take<float>((size_t)N * mw);
    p.t_width = (int)mw;
    {
        ChainBwdImages im;
        carve_chain_bwd_images(a, d, &im);
        for (int q = 0; q < 2; ++q) { p.wf2p[q] = im.wf2p[q]; p.wfep[q] = im.wfep[q]; }
        p.wc1p = im.wc1p; p.w2p = im.w2p; p.w1ep = im.w1ep;
    }
    p.ncb_img = nullptr;
    if (node_chain_bwd_supported(d.dn, d.pw, d.kx) && m.node.n_layers == 1 && m.precision == MPNHIP_PREC_FP32_SPLIT)
        p.ncb_img = a.take<unsigned short>(node_chain_bwd_image_shorts(d.dn, d.pw, nullptr));
    {   // MPNHIP_PREC_BF16: transposition scratch of the activation-gradient products (two direction groups of the largest weight)
        size_t mx = (size_t)d.pw * d.kx;
        const mpnhip_mlp* all[] = {&m.enc_node, &m.enc_edge, &m.edge, &m.flow_in, &m.flow_out, &m.node, &m.classifier};
        for (const mpnhip_mlp* q : all)
            for (int i = 0; i < q->n_layers; ++i) {
                const size_t w = (size_t)q->out_dims[i] * layer_in(*q, i);
                mx = w > mx ? w : mx;
            }
        p.wt_scratch_floats = m.precision == MPNHIP_PREC_BF16 ? 2 * mx : 0;
        p.wt_scratch = a.take<float>(p.wt_scratch_floats);
        p.wt_keep_floats[0] = m.precision == MPNHIP_PREC_BF16 && m.node.n_layers >= 1 ? (size_t)d.dn * m.node.in_dim : 0;
        p.wt_keep_floats[1] = m.precision == MPNHIP_PREC_BF16 ? (size_t)d.pw * d.dn : 0;
        for (int i = 0; i < 2; ++i) p.wt_keep[i] = a.take<float>(p.wt_keep_floats[i]);
        for (int i = 0; i < 2; ++i) p.wt_keep16[i] = a.take<unsigned short>(p.wt_keep_floats[i]);
    }
    p.slab_floats_per_group = slab_per_group(m, d, N, E, (int)L, p.b16, node16);
    p.slab = a.take<float>(2 * p.slab_floats_per_group);
    p.slab_side = a.take<float>(2 * p.slab_floats_per_group);
    p.slab_wp_floats = 0;
    for (int nb = 1; nb <= (int)L; ++nb) {
        const size_t t = slab_batched(m, d, N, E, nb, p.b16);
        p.slab_wp_floats = t > p.slab_wp_floats ? t : p.slab_wp_floats;
    }
    p.slab_wp = a.take<float>(p.slab_wp_floats);
    p.slab_tail_floats = slab_tail(m, d, N, E, p.b16, node16);
    p.slab_tail = a.take<float>(p.slab_tail_floats);
    p.total = a.bytes();
    if (out) *out = p;
    return p.total;
}

}  // namespace mpnhip
