// Inference forward of the convolution-type layers of the two ResNet50s (the ReID network, the Mask R-CNN FPN backbone;
// include/mpnhip.h: mpnhip_conv2d_affine_forward, mpnhip_conv2d_affine_up_forward, mpnhip_maxpool2d_forward): implicit-GEMM convolution (1x1 / 3x3 / 7x7, stride 1 or 2, padding k / 2, no bias) on the fp32-input
// MFMA with the eval-mode BatchNorm (one fmaf per output), the residual add and the ReLU in its epilogue, and MaxPool2d(3, 2, 1).
//
// GEMM view of conv_affine_tile_kernel: M = output channels (rows of the weight), N = the output pixels of ALL images packed into
// one column index (n = image * Hout * Wout + oy * Wout + ox), K = input channels x taps.  conv.hip's kernel tiles ONE image into
// 14 x 14 output tiles; an 8 x 4 map of this network would fill 32 of its 224 columns.  Here a 32-column MFMA tile may straddle
// images: every column carries its own (image, oy, ox).  One block per (BN columns, BM rows); K is walked in chunks of CK input
// channels: the chunk's weight columns [k][m] and its im2col operand [k][n] -- built on the fly from
// (image, oy * s + ky - k / 2, ox * s + kx - k / 2), cells outside the image written as zeros -- are staged in LDS, then every
// wave runs v_mfma_f32_32x32x2_f32 over the chunk on its tiles of 32 x 32 (2 x 2, or one).  The chunk after the one being multiplied
// travels in registers (conv_tile_kernel's prefetch).  The summation order (channel, then tap; one chain per output) is a function
// of the layer alone: no split of K across blocks, no atomics, so an output's bits depend on the layer and on its image only --
// not on n_images, not on where the image sits in the batch.  (K > 2048: the chain is cut into groups, see GROUPED below.)
// UP (mpnhip_conv2d_affine_up_forward, the FPN's top-down path): the residual is a coarser map [cout][res_H][res_W] read at the
// nearest-neighbour source cell of every output pixel; nothing else of the kernel changes.
#include "common.h"

#include <math.h>

namespace mpnhip {
namespace {

constexpr int CA_THREADS = 256;

using f32x16 = __attribute__((ext_vector_type(16))) float;

struct ConvAffine {
    const float* x;
    const float* weight;
    const float* scale;
    const float* shift;
    const float* residual;
    float* out;
    int64_t x_stride, residual_stride, out_stride;
    int cin, cout, H, W, Hout, Wout, stride, relu;
    int ntotal;                                   // n_images * Hout * Wout
    int res_H, res_W;                             // UP only: the residual's own size, and (float)res_H / Hout, (float)res_W / Wout
    float up_sy, up_sx;
};

constexpr int CA_GROUP_CHUNKS = 4;               // GROUPED: chunks per partial sum
constexpr int CA_GROUP_MIN_K = 2048;             // K above this takes the grouped summation

// KS: 1, 3 or 7.  WM: waves along M; TW: every wave owns TW x TW tiles of 32 x 32.  (WM, TW) = (2, 2): the 128 x 128 block;
// (1, 2): 64 rows x 256 columns for cout <= 64; (2, 1): a 64 x 64 block for launches whose larger blocks would not fill the chip
// (few images on the 8 x 4 maps).  The chain of an output is the same in all three, so which one runs does not show in the bits.
// GROUPED (K > CA_GROUP_MIN_K): the chain of an output is cut every CA_GROUP_CHUNKS chunks -- the chunks of a group are summed
// from zero in a second accumulator, and the group's sum is added to the running total, groups in order.  Still (channel, then
// tap) order, fixed by the layer alone; it keeps the rounding of a K = 4608 chain (measured 2.5e-6 of the largest output as ONE
// chain, against 1.5e-6 at K = 2048) below what the project holds the short chains to.
// UP: the epilogue adds residual[m][sy][sx] with aten's nearest-neighbour source index, sy = min((int)floorf(oy * up_sy), res_H - 1)
// and sx likewise, computed once per column; with res_H == Hout and res_W == Wout that is the cell (oy, ox) itself.
template <int KS, int WM, int TW, bool GROUPED, bool UP>
__global__ __launch_bounds__(CA_THREADS) void conv_affine_tile_kernel(ConvAffine p) {
    constexpr int TAPS = KS * KS, PAD = KS / 2;
    constexpr int CK = KS == 1 ? 32 : (KS == 3 ? 4 : 1);   // input channels per chunk
    constexpr int KV = CK * TAPS;                  // k per chunk in use
    constexpr int KC = (KV + 1) & ~1;              // ... padded to even (7 x 7: 49 -> 50, the pad row is zeros on both sides)
    constexpr int WN = 4 / WM, BM = 32 * TW * WM, BN = 32 * TW * WN;
    constexpr int PW = BM + 1;                     // row pitch of the weight image [k][m]: conflict-free transposing stores
    constexpr int PB = BN + 32;                    // row pitch of the im2col image [k][n]: rows k, k + 1 in disjoint bank halves
    constexpr int WREGS = (BM * KC + CA_THREADS - 1) / CA_THREADS;   // weight elements per thread and chunk
    constexpr int KROWS = CA_THREADS / BN;         // k rows of the im2col image the block stages at once (1, 2 or 4)
    constexpr int BREGS = KC / KROWS;              // im2col elements per thread and chunk: one column, every KROWS-th row
    static_assert(KC % KROWS == 0, "the im2col chunk must divide among the threads");
    __shared__ float wl[KC * PW];
    __shared__ float bl[KC * PB];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 31, lh = lane >> 5;
    const int wm = wave % WM, wn = wave / WM;
    const int n0 = blockIdx.x * BN, m0 = blockIdx.y * BM;
    const int hw = p.H * p.W, hwo = p.Hout * p.Wout, ktotal = p.cin * TAPS;

    // the column of the im2col image this thread stages for every chunk
    const int sc = t % BN, kr0 = t / BN;
    const bool col_ok = n0 + sc < p.ntotal;
    int iy0 = 0, ix0 = 0;
    const float* __restrict__ xi = p.x;
    if (col_ok) {
        const int n = n0 + sc, img = n / hwo, pix = n % hwo;
        iy0 = (pix / p.Wout) * p.stride - PAD;
        ix0 = (pix % p.Wout) * p.stride - PAD;
        xi = p.x + (int64_t)img * p.x_stride;
    }

    f32x16 acc[TW][TW], part[GROUPED ? TW : 1][GROUPED ? TW : 1];
#pragma unroll
    for (int i = 0; i < TW; ++i)
#pragma unroll
        for (int j = 0; j < TW; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                acc[i][j][r] = 0.f;
                if constexpr (GROUPED) part[i][j][r] = 0.f;
            }

    // The chunk after the one being multiplied travels in registers: its global loads are issued before the MFMA loop and
    // land in LDS after it, so their latency hides behind the products instead of standing between two barriers.
    float pv[BREGS], wv[WREGS];
    auto fetch = [&](int c0) {
#pragma unroll
        for (int q = 0; q < BREGS; ++q) {
            const int k = kr0 + q * KROWS, c = c0 + k / TAPS, tap = k % TAPS;
            const int iy = iy0 + tap / KS, ix = ix0 + tap % KS;
            const bool ok = col_ok && k < KV && c < p.cin && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
            pv[q] = ok ? xi[c * hw + iy * p.W + ix] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < WREGS; ++q) {          // weight[m][c0 * TAPS + k]: k contiguous in memory
            const int idx = t + q * CA_THREADS, k = idx % KC, m = idx / KC;
            const bool ok = idx < BM * KC && m0 + m < p.cout && k < KV && c0 + k / TAPS < p.cin;
            wv[q] = ok ? p.weight[(m0 + m) * ktotal + c0 * TAPS + k] : 0.f;
        }
    };
    fetch(0);
    for (int c0 = 0; c0 < p.cin; c0 += CK) {
#pragma unroll
        for (int q = 0; q < BREGS; ++q) bl[(kr0 + q * KROWS) * PB + sc] = pv[q];
#pragma unroll
        for (int q = 0; q < WREGS; ++q) {
            const int idx = t + q * CA_THREADS;
            if (idx < BM * KC) wl[(idx % KC) * PW + idx / KC] = wv[q];
        }
        __syncthreads();
        if (c0 + CK < p.cin) fetch(c0 + CK);
#pragma unroll
        for (int kk = 0; kk < KC; kk += 2) {
            float a[TW], b[TW];
#pragma unroll
            for (int i = 0; i < TW; ++i) a[i] = wl[(kk + lh) * PW + (wm * TW + i) * 32 + li];
#pragma unroll
            for (int j = 0; j < TW; ++j) b[j] = bl[(kk + lh) * PB + (wn * TW + j) * 32 + li];
#pragma unroll
            for (int i = 0; i < TW; ++i)
#pragma unroll
                for (int j = 0; j < TW; ++j) {
                    if constexpr (GROUPED) part[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], part[i][j], 0, 0, 0);
                    else acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
                }
        }
        if constexpr (GROUPED) {
            if ((c0 / CK) % CA_GROUP_CHUNKS == CA_GROUP_CHUNKS - 1 || c0 + CK >= p.cin) {   // the group ends (uniform over the block)
#pragma unroll
                for (int i = 0; i < TW; ++i)
#pragma unroll
                    for (int j = 0; j < TW; ++j)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            acc[i][j][r] += part[i][j][r];
                            part[i][j][r] = 0.f;
                        }
            }
        }
        __syncthreads();
    }

    // D[i][j] of a 32 x 32 tile: j = lane & 31 (pixel column), i = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) (row of M)
#pragma unroll
    for (int j = 0; j < TW; ++j) {
        const int n = n0 + (wn * TW + j) * 32 + li;
        if (n >= p.ntotal) continue;
        const int img = n / hwo, pix = n % hwo;
        float* __restrict__ o = p.out + (int64_t)img * p.out_stride + pix;
        int rpix = pix;
        if constexpr (UP) {
            const int sy = min((int)floorf((float)(pix / p.Wout) * p.up_sy), p.res_H - 1);
            const int sx = min((int)floorf((float)(pix % p.Wout) * p.up_sx), p.res_W - 1);
            rpix = sy * p.res_W + sx;
        }
        const int rplane = UP ? p.res_H * p.res_W : hwo;
        const float* __restrict__ res = p.residual ? p.residual + (int64_t)img * p.residual_stride + rpix : nullptr;
#pragma unroll
        for (int i = 0; i < TW; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + (wm * TW + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (m >= p.cout) continue;
                float v = fmaf(acc[i][j][r], p.scale ? p.scale[m] : 1.f, p.shift ? p.shift[m] : 0.f);
                if (res) v += res[m * rplane];
                if (p.relu) v = fmaxf(v, 0.f);
                o[m * hwo] = v;
            }
        }
    }
}

// nn.MaxPool2d(3, stride 2, padding 1): one thread per output element, the pixel index fastest.  Padded cells do not take part
// (the centre cell of every window lies inside the image, so no window is empty); a NaN wins, as in torch.
__global__ __launch_bounds__(CA_THREADS) void maxpool3s2_kernel(const float* __restrict__ x, int64_t x_stride, int C, int H, int W,
                                                                int Hout, int Wout, float* __restrict__ out, int64_t out_stride,
                                                                int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * CA_THREADS + threadIdx.x;
    if (idx >= total) return;
    const int hwo = Hout * Wout;
    const int64_t per_image = (int64_t)C * hwo, img = idx / per_image;
    const int e = (int)(idx % per_image), c = e / hwo, pix = e % hwo, oy = pix / Wout, ox = pix % Wout;
    const float* __restrict__ xc = x + img * x_stride + c * (H * W);
    float m = -INFINITY;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
        const int iy = 2 * oy + dy - 1;
        if (iy < 0 || iy >= H) continue;
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int ix = 2 * ox + dx - 1;
            if (ix < 0 || ix >= W) continue;
            const float v = xc[iy * W + ix];
            if (v > m || v != v) m = v;
        }
    }
    out[img * out_stride + e] = m;
}

bool conv_affine_grouped(const ConvAffine& p, int ksize) { return (int64_t)p.cin * ksize * ksize > CA_GROUP_MIN_K; }

constexpr int64_t CA_SMALL_GRID = 512;            // fewer blocks than this (two per CU of an MI355X): the 64 x 64 block

template <int KS, bool UP>
void launch_conv_affine(const ConvAffine& p, hipStream_t stream) {
    const bool grouped = conv_affine_grouped(p, KS);
    const int64_t n = p.ntotal;
#define MPN_CA_LAUNCH(WM, TW, BM, BN)                                                                                   \
    do {                                                                                                                \
        const dim3 grid((unsigned)((n + BN - 1) / BN), (unsigned)((p.cout + BM - 1) / BM));                             \
        if (grouped) conv_affine_tile_kernel<KS, WM, TW, true, UP><<<grid, CA_THREADS, 0, stream>>>(p);                     \
        else conv_affine_tile_kernel<KS, WM, TW, false, UP><<<grid, CA_THREADS, 0, stream>>>(p);                            \
    } while (0)
    if constexpr (KS != 7) {            // (the 7 x 7 chunk is no multiple of four rows, and with 256 columns it would not fit 64 KB of LDS)
        const int64_t blocks = p.cout <= 64 ? (n + 255) / 256 : ((n + 127) / 128) * ((p.cout + 127) / 128);
        if (blocks < CA_SMALL_GRID) {
            MPN_CA_LAUNCH(2, 1, 64, 64);
            count_path(PC_CONV_AFFINE_SMALL_GRID);
            return;
        }
        if (p.cout <= 64) {
            MPN_CA_LAUNCH(1, 2, 64, 256);
            count_path(PC_CONV_AFFINE_WIDE);
            return;
        }
    }
    MPN_CA_LAUNCH(2, 2, 128, 128);
#undef MPN_CA_LAUNCH
}

}  // namespace
}  // namespace mpnhip

using namespace mpnhip;

// The argument checks both convolution entry points share, then the launch.  up: the residual is [cout][res_H][res_W] per image.
static int conv_affine_run(const char* name, const mpnhip_conv_affine_args& a, bool up, int res_H, int res_W, hipStream_t stream) {
    MPN_CHECK_ARG(a.n_images >= 0, "%s: negative n_images", name);
    if (a.n_images == 0) return MPNHIP_OK;
    MPN_CHECK_ARG(a.x != nullptr && a.weight != nullptr && a.out != nullptr, "%s: null x, weight or out", name);
    MPN_CHECK_ARG(a.ksize == 1 || a.ksize == 3 || a.ksize == 7, "%s: kernel size %d is none of 1, 3, 7", name, a.ksize);
    MPN_CHECK_ARG(a.stride == 1 || a.stride == 2, "%s: stride %d is neither 1 nor 2", name, a.stride);
    MPN_CHECK_ARG(a.H >= 1 && a.W >= 1 && a.cin >= 1 && a.cout >= 1, "%s: H %d, W %d, cin %d, cout %d must be positive", name, a.H, a.W,
                  a.cin, a.cout);
    MPN_CHECK_ARG(a.x_stride >= 0 && a.x_stride <= INT32_MAX, "%s: x_stride %lld outside the 32-bit range", name, (long long)a.x_stride);
    MPN_CHECK_ARG(a.out_stride >= 0 && a.out_stride <= INT32_MAX, "%s: out_stride %lld outside the 32-bit range", name,
                  (long long)a.out_stride);
    MPN_CHECK_ARG(a.residual == nullptr || (a.residual_stride >= 0 && a.residual_stride <= INT32_MAX),
                  "%s: residual_stride %lld outside the 32-bit range", name, (long long)a.residual_stride);
    const int64_t Hout = (a.H - 1) / a.stride + 1, Wout = (a.W - 1) / a.stride + 1, hwo = Hout * Wout;
    MPN_CHECK_ARG((int64_t)a.cin * a.H * a.W <= INT32_MAX, "%s: an input image of %d x %lld floats is beyond the 32-bit offsets", name, a.cin,
                  (long long)a.H * a.W);
    MPN_CHECK_ARG((int64_t)a.cout * hwo <= INT32_MAX, "%s: an output image of %d x %lld floats is beyond the 32-bit offsets", name, a.cout,
                  (long long)hwo);
    MPN_CHECK_ARG((int64_t)a.cin * a.cout * a.ksize * a.ksize <= INT32_MAX, "%s: the weight is beyond the 32-bit offsets", name);
    // (a block's column indices run up to 255 past the last column: they must stay ints as well)
    MPN_CHECK_ARG(a.n_images <= (INT32_MAX - 256) / hwo, "%s: %lld images of %lld output pixels are beyond the 32-bit column index", name,
                  (long long)a.n_images, (long long)hwo);
    MPN_CHECK_ARG((a.cout + 63) / 64 <= 65535, "%s: cout %d is more than one launch holds", name, a.cout);
    if (up) {
        MPN_CHECK_ARG(a.residual != nullptr, "%s: null residual", name);
        MPN_CHECK_ARG(res_H >= 1 && res_W >= 1, "%s: residual_H %d, residual_W %d must be positive", name, res_H, res_W);
        MPN_CHECK_ARG((int64_t)a.cout * res_H * res_W <= INT32_MAX, "%s: a residual image of %d x %lld floats is beyond the 32-bit offsets",
                      name, a.cout, (long long)res_H * res_W);
    }

    ConvAffine p;
    p.x = a.x, p.weight = a.weight, p.scale = a.scale, p.shift = a.shift, p.residual = a.residual, p.out = a.out;
    p.x_stride = a.x_stride, p.residual_stride = a.residual_stride, p.out_stride = a.out_stride;
    p.cin = a.cin, p.cout = a.cout, p.H = a.H, p.W = a.W, p.Hout = (int)Hout, p.Wout = (int)Wout, p.stride = a.stride, p.relu = a.relu;
    p.ntotal = (int)(a.n_images * hwo);
    p.res_H = up ? res_H : (int)Hout, p.res_W = up ? res_W : (int)Wout;
    p.up_sy = (float)p.res_H / (float)Hout, p.up_sx = (float)p.res_W / (float)Wout;
    if (up) {
        if (a.ksize == 1) launch_conv_affine<1, true>(p, stream);
        else if (a.ksize == 3) launch_conv_affine<3, true>(p, stream);
        else launch_conv_affine<7, true>(p, stream);
        count_path(PC_CONV_AFFINE_UP);
    } else {
        if (a.ksize == 1) launch_conv_affine<1, false>(p, stream);
        else if (a.ksize == 3) launch_conv_affine<3, false>(p, stream);
        else launch_conv_affine<7, false>(p, stream);
    }
    count_path(PC_CONV_AFFINE_TILE);
    if (conv_affine_grouped(p, a.ksize)) count_path(PC_CONV_AFFINE_GROUPED);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}

extern "C" int mpnhip_conv2d_affine_forward(const mpnhip_conv_affine_args* args, void* stream_) {
    static const char* const name = "mpnhip_conv2d_affine_forward";
    MPN_CHECK_ARG(args != nullptr, "%s: null args", name);
    return conv_affine_run(name, *args, false, 0, 0, (hipStream_t)stream_);
}

extern "C" int mpnhip_conv2d_affine_up_forward(const mpnhip_conv_affine_up_args* args, void* stream_) {
    static const char* const name = "mpnhip_conv2d_affine_up_forward";
    MPN_CHECK_ARG(args != nullptr, "%s: null args", name);
    const mpnhip_conv_affine_up_args& u = *args;
    mpnhip_conv_affine_args a;
    a.x = u.x, a.x_stride = u.x_stride, a.weight = u.weight, a.scale = u.scale, a.shift = u.shift;
    a.residual = u.residual, a.residual_stride = u.residual_stride, a.relu = u.relu, a.out = u.out, a.out_stride = u.out_stride;
    a.n_images = u.n_images, a.cin = u.cin, a.cout = u.cout, a.H = u.H, a.W = u.W, a.ksize = u.ksize, a.stride = u.stride;
    return conv_affine_run(name, a, true, u.residual_H, u.residual_W, (hipStream_t)stream_);
}

extern "C" int mpnhip_maxpool2d_forward(const float* x, int64_t x_stride, int64_t n_images, int C, int H, int W, float* out,
                                        int64_t out_stride, void* stream_) {
    static const char* const name = "mpnhip_maxpool2d_forward";
    hipStream_t stream = (hipStream_t)stream_;
    MPN_CHECK_ARG(n_images >= 0, "%s: negative n_images", name);
    if (n_images == 0) return MPNHIP_OK;
    MPN_CHECK_ARG(x != nullptr && out != nullptr, "%s: null x or out", name);
    MPN_CHECK_ARG(C >= 1 && H >= 1 && W >= 1, "%s: C %d, H %d, W %d must be positive", name, C, H, W);
    MPN_CHECK_ARG(x_stride >= 0 && x_stride <= INT32_MAX, "%s: x_stride %lld outside the 32-bit range", name, (long long)x_stride);
    MPN_CHECK_ARG(out_stride >= 0 && out_stride <= INT32_MAX, "%s: out_stride %lld outside the 32-bit range", name, (long long)out_stride);
    MPN_CHECK_ARG((int64_t)C * H * W <= INT32_MAX, "%s: an input image of %d x %lld floats is beyond the 32-bit offsets", name, C,
                  (long long)H * W);
    const int Hout = (H - 1) / 2 + 1, Wout = (W - 1) / 2 + 1;
    const int64_t per_image = (int64_t)C * Hout * Wout;
    MPN_CHECK_ARG(n_images <= ((int64_t)INT32_MAX * CA_THREADS) / per_image, "%s: %lld images of %d x %d x %d are more than one launch holds",
                  name, (long long)n_images, C, H, W);
    const int64_t total = n_images * per_image;
    maxpool3s2_kernel<<<(unsigned)((total + CA_THREADS - 1) / CA_THREADS), CA_THREADS, 0, stream>>>(x, x_stride, C, H, W, Hout, Wout, out,
                                                                                                   out_stride, total);
    count_path(PC_MAXPOOL);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}
