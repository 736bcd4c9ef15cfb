// Backward of the mask branch's Conv2d layers (include/mpnhip.h: mpnhip_conv2d_backward): 1x1 / 3x3, stride 1, padding k / 2, with
// the ReLU the forward fuses.  Four steps, every sum in a fixed order that depends on the layer and the image count alone (no
// atomics, no split that looks at the device):
//
//   conv_bwd_gate_kernel    g = grad_out * [y > 0] written once into the workspace (relu only), and the sum of g per (block of
//                           WG_IMAGES images, output channel): the bias gradient's partial sums.
//   data gradient           W'[c][m][tap] = W[m][c][taps - 1 - tap] (conv_bwd_flip_kernel), then mpnhip_conv2d_forward on g with W':
//                           the forward's own kernels and launcher, so an image's bits do not depend on the batch.
//   conv_wgrad_kernel       GEMM view: M = output channels, N = input channels x taps, K = every pixel of every image.  One block
//                           per (32 MT rows of M, WG_CK input channels, WG_IMAGES images).  Per (image, 14 x 14 tile) the block
//                           stages the 16 x 16 zero-halo input patches of its channels in LDS as the forward does, then the g tile
//                           two pixel rows at a time (pixels outside the image as zeros), and every wave runs
//                           v_mfma_f32_32x32x2_f32 with the pixel index as k: A = g[m][pixel], B = patch[channel][pixel + tap], one
//                           32 x 32 accumulator per (32 rows, tap) -- its columns are the 32 channels.  The accumulators live
//                           across the block's images and are written once, to partial[split][cout][cin * taps].
//   conv_bwd_sum_kernel     adds the partial sums in split order (weight and bias).
//
// cout <= CONV_SMALL_COUT: conv_wgrad_plain_kernel, one block per (m, c, split), the pixels strided over the threads and summed
// over the block in a fixed order; the same partial layout and second stage.
//
// Backward of ConvTranspose2d(2, stride 2, padding 0) (mpnhip_conv_transpose2d_backward): stride = kernel size, so the layer is a
// 1 x 1 product in a space-to-depth layout.  convt_bwd_gate_kernel writes g as g'[n][4 m + 2 dy + dx][h][w] (4 cout channels at the
// INPUT size) and takes the bias partial sums as the gate kernel does; the data gradient is mpnhip_conv2d_forward (ksize 1) on g'
// with the weight [cin][4 cout] as it stands; the weight gradient is convt_wgrad_kernel, a tap-less product of two pixel-contiguous
// row operands (rows of M from the layer's input, columns from g') whose partial layout [split][cin][4 cout] is the weight's, and at
// cin <= CONV_SMALL_COUT the plain 1 x 1 kernel with the roles swapped.
#include "common.h"

namespace mpnhip {
namespace {

constexpr int CB_THREADS = 256;
constexpr int WG_IMAGES = 8;                          // images per block: the split of K is a function of n_images alone
constexpr int WG_CK = 32;                             // input channels per block = the columns of one MFMA tile
constexpr int WG_PP = CONV_PATCH_CELLS + 1;           // channel pitch of the patches: odd, lanes that differ in the channel hit different banks
constexpr int WG_ROWS = 2;                            // tile rows of g staged at a time
constexpr int WG_GPX = WG_ROWS * CONV_TILE;           // ... their pixels (even: k advances in pairs)
constexpr int WG_GP = WG_GPX + 1;                     // row pitch of the g stage: odd, lanes that differ in the row of M hit different banks
static_assert(CONV_TILE % 2 == 0 && CONV_TILE % WG_ROWS == 0, "a k pair stays inside one tile row; whole stages");

using f32x16 = __attribute__((ext_vector_type(16))) float;

// sum over the block in a fixed order: a shuffle tree inside every wave, then the wave sums one after the other
__device__ __forceinline__ float cb_block_sum(float v, float* red) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    __syncthreads();                            // red may still be read from the previous sum
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < CB_THREADS / 64; ++w) s += red[w];
    return s;
}

// grid (cout, splits).  g_out: dense [n_images][cout][hw] or nullptr (no ReLU: g is grad_out itself); bias_partial [splits][cout] or nullptr
__global__ __launch_bounds__(CB_THREADS) void conv_bwd_gate_kernel(const float* __restrict__ grad_out, int64_t go_stride,
                                                                   const float* __restrict__ y, int64_t y_stride, int cout, int hw,
                                                                   int64_t n_images, float* __restrict__ g_out,
                                                                   float* __restrict__ bias_partial) {
    __shared__ float red[CB_THREADS / 64];
    const int m = blockIdx.x, t = threadIdx.x;
    const int64_t img0 = (int64_t)blockIdx.y * WG_IMAGES;
    const int64_t img1 = img0 + WG_IMAGES < n_images ? img0 + WG_IMAGES : n_images;
    float s = 0.f;
    for (int64_t img = img0; img < img1; ++img) {
        const float* __restrict__ go = grad_out + img * go_stride + (int64_t)m * hw;
        const float* __restrict__ yy = y ? y + img * y_stride + (int64_t)m * hw : nullptr;
        float* __restrict__ gw = g_out ? g_out + (img * cout + m) * hw : nullptr;
        for (int p = t; p < hw; p += CB_THREADS) {
            float v = go[p];
            if (yy && !(yy[p] > 0.f)) v = 0.f;
            if (gw) gw[p] = v;
            s += v;
        }
    }
    s = cb_block_sum(s, red);
    if (bias_partial && t == 0) bias_partial[(int64_t)blockIdx.y * cout + m] = s;
}

// wT[c][m][tap] = w[m][c][taps - 1 - tap]
__global__ __launch_bounds__(CB_THREADS) void conv_bwd_flip_kernel(const float* __restrict__ w, int cout, int cin, int taps,
                                                                   float* __restrict__ wT) {
    const int idx = blockIdx.x * CB_THREADS + threadIdx.x;
    if (idx >= cout * cin * taps) return;
    const int tap = idx % taps, m = (idx / taps) % cout, c = idx / (taps * cout);
    wT[idx] = w[(m * cin + c) * taps + taps - 1 - tap];
}

// out[i] = partial[0][i] + partial[1][i] + ... in that order
__global__ __launch_bounds__(CB_THREADS) void conv_bwd_sum_kernel(const float* __restrict__ partial, int splits, int count,
                                                                  float* __restrict__ out) {
    const int idx = blockIdx.x * CB_THREADS + threadIdx.x;
    if (idx >= count) return;
    float s = 0.f;
    for (int sp = 0; sp < splits; ++sp) s += partial[(int64_t)sp * count + idx];
    out[idx] = s;
}

// ConvTranspose2d(2, stride 2): grid (cout, splits).  grad_out / y: [cout][2 H][2 W] per image.  g_out: dense [n_images][4 cout][hw]
// with channel 4 m + 2 dy + dx holding g[m][2 h + dy][2 w + dx], or nullptr; bias_partial [splits][cout] or nullptr.  The sum runs
// over the output pixels in the gate kernel's order.
__global__ __launch_bounds__(CB_THREADS) void convt_bwd_gate_kernel(const float* __restrict__ grad_out, int64_t go_stride,
                                                                    const float* __restrict__ y, int64_t y_stride, int cout, int H,
                                                                    int W, int64_t n_images, float* __restrict__ g_out,
                                                                    float* __restrict__ bias_partial) {
    __shared__ float red[CB_THREADS / 64];
    const int m = blockIdx.x, t = threadIdx.x;
    const int hw = H * W, ohw = 4 * hw, ow = 2 * W;
    const int64_t img0 = (int64_t)blockIdx.y * WG_IMAGES;
    const int64_t img1 = img0 + WG_IMAGES < n_images ? img0 + WG_IMAGES : n_images;
    float s = 0.f;
    for (int64_t img = img0; img < img1; ++img) {
        const float* __restrict__ go = grad_out + img * go_stride + (int64_t)m * ohw;
        const float* __restrict__ yy = y ? y + img * y_stride + (int64_t)m * ohw : nullptr;
        float* __restrict__ gw = g_out ? g_out + (img * cout + m) * (int64_t)ohw : nullptr;   // the four channels of m
        for (int p = t; p < ohw; p += CB_THREADS) {
            float v = go[p];
            if (yy && !(yy[p] > 0.f)) v = 0.f;
            if (gw) {
                const int oy = p / ow, ox = p % ow;
                gw[(2 * (oy & 1) + (ox & 1)) * hw + (oy >> 1) * W + (ox >> 1)] = v;
            }
            s += v;
        }
    }
    s = cb_block_sum(s, red);
    if (bias_partial && t == 0) bias_partial[(int64_t)blockIdx.y * cout + m] = s;
}

// out[img][c0 + c][p] = the segments' channels one behind the other: the dense row operand of the transposed layer's weight gradient
__global__ __launch_bounds__(CB_THREADS) void conv_bwd_gather_kernel(ConvSegs segs, int cin, int hw, int64_t total,
                                                                     float* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * CB_THREADS + threadIdx.x;
    if (idx >= total) return;
    const int p = (int)(idx % hw);
    const int c = (int)((idx / hw) % cin);
    const int64_t img = idx / ((int64_t)hw * cin);
    int seg = 0, seg_c0 = 0;
    while (c >= seg_c0 + segs.ch[seg]) {
        seg_c0 += segs.ch[seg];
        ++seg;
    }
    out[idx] = segs.p[seg][img * segs.stride[seg] + (int64_t)(c - seg_c0) * hw + p];
}

// Weight gradient of the transposed layer: partial[split][c][j] = sum over the split's images and all pixels of x[c][p] * g'[j][p]
// -- both operands are rows with the pixel contiguous, no patch and no tap.  GEMM view: M = cin (rows, from x), N = 4 cout (columns,
// from g'), K = pixels.  One block per (32 rows, 64 columns, WG_IMAGES images): K is walked image by image in stages of 32 pixels
// (the tail of an image as zeros); a stage's 32 + 64 rows are staged in LDS on an odd pitch, the next stage travels in registers
// across the products.  The four waves are 2 column tiles x 2 halves of a stage's k range; the two halves' accumulators are added
// once, at the end (first half + second half).  grid (row tiles x col_tiles, splits).  x: image i at x + i * x_stride, dense
// [cin][hw]; g: dense [n_images][m4][hw].
constexpr int CTW_KC = 32;                    // pixels per stage
constexpr int CTW_P = CTW_KC + 1;             // row pitch of the stages: odd, lanes that differ in the row hit different banks
constexpr int CTW_ROWS = 32, CTW_COLS = 64;   // block tile
__global__ __launch_bounds__(CB_THREADS) void convt_wgrad_kernel(const float* __restrict__ x, int64_t x_stride, int cin,
                                                                 const float* __restrict__ g, int m4, int hw, int64_t n_images,
                                                                 float* __restrict__ partial, int col_tiles) {
    constexpr int XREGS = CTW_ROWS * CTW_KC / CB_THREADS, GREGS = CTW_COLS * CTW_KC / CB_THREADS;
    __shared__ float xs[CTW_ROWS * CTW_P];
    __shared__ float gs[CTW_COLS * CTW_P];
    __shared__ float red[2 * 16 * 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 31, lh = lane >> 5;
    const int ct = wave & 1, kh = wave >> 1;
    const int c0 = (blockIdx.x / col_tiles) * CTW_ROWS, j0 = (blockIdx.x % col_tiles) * CTW_COLS;
    const int64_t img0 = (int64_t)blockIdx.y * WG_IMAGES;
    const int64_t img1 = img0 + WG_IMAGES < n_images ? img0 + WG_IMAGES : n_images;
    const int kk_t = t & (CTW_KC - 1), r_t = t / CTW_KC;      // this thread's pixel of a stage, and its first row (then every 8th)

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    float xv[XREGS], gv[GREGS];
    auto fetch = [&](int64_t img, int k0) {
        const bool k_ok = k0 + kk_t < hw;
#pragma unroll
        for (int q = 0; q < XREGS; ++q) {
            const int c = c0 + r_t + q * (CB_THREADS / CTW_KC);
            xv[q] = (k_ok && c < cin) ? x[img * x_stride + (int64_t)c * hw + k0 + kk_t] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < GREGS; ++q) {
            const int j = j0 + r_t + q * (CB_THREADS / CTW_KC);
            gv[q] = (k_ok && j < m4) ? g[(img * m4 + j) * (int64_t)hw + k0 + kk_t] : 0.f;
        }
    };
    int64_t img = img0;
    int k0 = 0;
    fetch(img, k0);
    while (img < img1) {
#pragma unroll
        for (int q = 0; q < XREGS; ++q) xs[(r_t + q * (CB_THREADS / CTW_KC)) * CTW_P + kk_t] = xv[q];
#pragma unroll
        for (int q = 0; q < GREGS; ++q) gs[(r_t + q * (CB_THREADS / CTW_KC)) * CTW_P + kk_t] = gv[q];
        __syncthreads();
        k0 += CTW_KC;
        if (k0 >= hw) {
            k0 = 0;
            ++img;
        }
        if (img < img1) fetch(img, k0);
        const float* __restrict__ xa = xs + li * CTW_P + (CTW_KC / 2) * kh + lh;
        const float* __restrict__ gb = gs + (32 * ct + li) * CTW_P + (CTW_KC / 2) * kh + lh;
#pragma unroll
        for (int kk = 0; kk < CTW_KC / 2; kk += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[kk], gb[kk], acc, 0, 0, 0);
        __syncthreads();                       // the next stage overwrites xs / gs
    }

    // the second half of every stage's k range joins the first, then D[i][j]: j = lane & 31 (column), i = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    if (kh == 1) {
#pragma unroll
        for (int r = 0; r < 16; ++r) red[(ct * 16 + r) * 64 + lane] = acc[r];
    }
    __syncthreads();
    if (kh == 1) return;
    const int j = j0 + 32 * ct + li;
    if (j >= m4) return;
    float* __restrict__ o = partial + (int64_t)blockIdx.y * cin * m4;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int c = c0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (c < cin) o[(int64_t)c * m4 + j] = acc[r] + red[(ct * 16 + r) * 64 + lane];
    }
}

// KS: 1 or 3.  MT: 32-row tiles of M per block (1, 2, 4); the four waves are MT row tiles x 4 / MT tap groups.
// grid (row groups x channel chunks, splits).  g: image i at g + i * g_stride, dense [cout][H][W].
template <int KS, int MT>
__global__ __launch_bounds__(CB_THREADS) void conv_wgrad_kernel(ConvSegs segs, int cin, int H, int W, int cout,
                                                                const float* __restrict__ g, int64_t g_stride, int64_t n_images,
                                                                float* __restrict__ partial, int tiles_x, int tiles_per_image,
                                                                int cchunks) {
    constexpr int TAPS = KS * KS, PAD = KS / 2;
    constexpr int EDGE = CONV_TILE + 2 * PAD;  // patch cells in use per row / column
    constexpr int NG = 4 / MT;                 // tap groups
    constexpr int TPW = (TAPS + NG - 1) / NG;  // taps per wave: tap = group + j NG
    constexpr int MG = 32 * MT;
    constexpr int GREGS = (MG * WG_GPX + CB_THREADS - 1) / CB_THREADS;
    __shared__ float patch[WG_CK * WG_PP];
    __shared__ float gl[MG * WG_GP];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 31, lh = lane >> 5;
    const int rt = wave % MT, tg = wave / MT;
    const int m0 = (blockIdx.x / cchunks) * MG, c0 = (blockIdx.x % cchunks) * WG_CK;
    const int64_t img0 = (int64_t)blockIdx.y * WG_IMAGES;
    const int64_t img1 = img0 + WG_IMAGES < n_images ? img0 + WG_IMAGES : n_images;
    const int hw = H * W;
    const bool wave_rows = m0 + 32 * rt < cout;   // (wave-uniform) this wave's rows of M exist

    f32x16 acc[TPW];
#pragma unroll
    for (int j = 0; j < TPW; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

    int toff[TPW];                              // patch offset of this wave's taps
#pragma unroll
    for (int j = 0; j < TPW; ++j) toff[j] = ((tg + j * NG) / KS) * CONV_PATCH + (tg + j * NG) % KS;
    const int pr = t >> 4, pc = t & 15;        // the patch cell this thread stages for every channel of the chunk
    for (int64_t img = img0; img < img1; ++img) {
        for (int tile = 0; tile < tiles_per_image; ++tile) {
            const int y0 = (tile / tiles_x) * CONV_TILE, x0 = (tile % tiles_x) * CONV_TILE;
            const int gy = y0 + pr - PAD, gx = x0 + pc - PAD;
            const bool cell_ok = pr < EDGE && pc < EDGE && gy >= 0 && gy < H && gx >= 0 && gx < W;
            const int cell_off = gy * W + gx;
#pragma unroll 1
            for (int sub = 0; sub * WG_ROWS < CONV_TILE; ++sub) {
                const int r0 = sub * WG_ROWS;
                __syncthreads();               // the products of the previous stage have read patch / gl
                if (sub == 0) {
                    int seg = 0, seg_c0 = 0;   // the segment that holds channel c0 + ch (channels only go up)
                    for (int ch = 0; ch < WG_CK; ++ch) {
                        const int c = c0 + ch;
                        float v = 0.f;
                        if (c < cin) {
                            while (c >= seg_c0 + segs.ch[seg]) {
                                seg_c0 += segs.ch[seg];
                                ++seg;
                            }
                            if (cell_ok) v = segs.p[seg][img * segs.stride[seg] + (int64_t)(c - seg_c0) * hw + cell_off];
                        }
                        patch[ch * WG_PP + t] = v;
                    }
                }
#pragma unroll
                for (int q = 0; q < GREGS; ++q) {
                    const int idx = t + q * CB_THREADS;
                    if (idx >= MG * WG_GPX) break;
                    const int m = idx / WG_GPX, px = idx % WG_GPX;
                    const int oy = y0 + r0 + px / CONV_TILE, ox = x0 + px % CONV_TILE;
                    float v = 0.f;
                    if (m0 + m < cout && oy < H && ox < W) v = g[img * g_stride + (int64_t)(m0 + m) * hw + oy * W + ox];
                    gl[m * WG_GP + px] = v;
                }
                __syncthreads();
                if (wave_rows && tg < TAPS) {
                    const float* __restrict__ ga = gl + (32 * rt + li) * WG_GP + lh;
                    const float* __restrict__ pb = patch + li * WG_PP + r0 * CONV_PATCH + lh;
                    // k = the pixel, in pairs (kk, kk + 1) that share a tile row
#pragma unroll
                    for (int kk = 0; kk < WG_GPX; kk += 2) {
                        const float a = ga[kk];
                        const int poff = (kk / CONV_TILE) * CONV_PATCH + kk % CONV_TILE;
#pragma unroll
                        for (int j = 0; j < TPW; ++j)
                            if (tg + j * NG < TAPS) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, pb[poff + toff[j]], acc[j], 0, 0, 0);
                    }
                }
            }
        }
    }

    // D[i][j] of a 32 x 32 tile: j = lane & 31 (channel), i = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) (row of M)
    if (!wave_rows) return;
    const int c = c0 + li;
    if (c >= cin) return;
    const int ktotal = cin * TAPS;
    float* __restrict__ o = partial + (int64_t)blockIdx.y * cout * ktotal;
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
        const int tap = tg + j * NG;
        if (tap >= TAPS) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + 32 * rt + (r & 3) + 8 * (r >> 2) + 4 * lh;
            if (m < cout) o[(int64_t)m * ktotal + c * TAPS + tap] = acc[j][r];
        }
    }
}

// cout <= CONV_SMALL_COUT: grid (cout x cin, splits), one block per (m, c, split)
template <int KS>
__global__ __launch_bounds__(CB_THREADS) void conv_wgrad_plain_kernel(ConvSegs segs, int cin, int H, int W, int cout,
                                                                      const float* __restrict__ g, int64_t g_stride,
                                                                      int64_t n_images, float* __restrict__ partial) {
    constexpr int TAPS = KS * KS, PAD = KS / 2;
    __shared__ float red[CB_THREADS / 64];
    const int t = threadIdx.x, m = blockIdx.x / cin, c = blockIdx.x % cin;
    const int64_t img0 = (int64_t)blockIdx.y * WG_IMAGES;
    const int64_t img1 = img0 + WG_IMAGES < n_images ? img0 + WG_IMAGES : n_images;
    const int hw = H * W;
    int seg = 0, seg_c0 = 0;
    while (c >= seg_c0 + segs.ch[seg]) {
        seg_c0 += segs.ch[seg];
        ++seg;
    }
    float acc[TAPS];
#pragma unroll
    for (int tap = 0; tap < TAPS; ++tap) acc[tap] = 0.f;
    for (int64_t img = img0; img < img1; ++img) {
        const float* __restrict__ x = segs.p[seg] + img * segs.stride[seg] + (int64_t)(c - seg_c0) * hw;
        const float* __restrict__ gp = g + img * g_stride + (int64_t)m * hw;
        for (int p = t; p < hw; p += CB_THREADS) {
            const float gv = gp[p];
            const int oy = p / W, ox = p % W;
#pragma unroll
            for (int tap = 0; tap < TAPS; ++tap) {
                const int iy = oy + tap / KS - PAD, ix = ox + tap % KS - PAD;
                const float v = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? x[iy * W + ix] : 0.f;
                acc[tap] = fmaf(gv, v, acc[tap]);
            }
        }
    }
    float* __restrict__ o = partial + ((int64_t)blockIdx.y * cout + m) * cin * TAPS + c * TAPS;
#pragma unroll
    for (int tap = 0; tap < TAPS; ++tap) {
        const float s = cb_block_sum(acc[tap], red);
        if (t == 0) o[tap] = s;
    }
}

template <int KS>
void launch_conv_wgrad(const ConvSegs& segs, int cin, const mpnhip_conv_bwd_args& a, const float* g, int64_t g_stride, int splits,
                       float* partial, hipStream_t stream) {
    if (a.cout <= CONV_SMALL_COUT) {
        conv_wgrad_plain_kernel<KS><<<dim3((unsigned)(a.cout * cin), (unsigned)splits), CB_THREADS, 0, stream>>>(
            segs, cin, a.H, a.W, a.cout, g, g_stride, a.n_images, partial);
        count_path(PC_CONV_WGRAD_PLAIN);
        return;
    }
    const int tiles_x = (a.W + CONV_TILE - 1) / CONV_TILE, tiles = tiles_x * ((a.H + CONV_TILE - 1) / CONV_TILE);
    const int mt = a.cout <= 32 ? 1 : a.cout <= 64 ? 2 : 4;
    const int cchunks = (cin + WG_CK - 1) / WG_CK;
    const dim3 grid((unsigned)((a.cout + 32 * mt - 1) / (32 * mt) * cchunks), (unsigned)splits);
#define MPN_WGRAD_LAUNCH(MT)                                                                                                     \
    conv_wgrad_kernel<KS, MT><<<grid, CB_THREADS, 0, stream>>>(segs, cin, a.H, a.W, a.cout, g, g_stride, a.n_images, partial, tiles_x, \
                                                               tiles, cchunks)
    if (mt == 1) MPN_WGRAD_LAUNCH(1);
    else if (mt == 2) MPN_WGRAD_LAUNCH(2);
    else MPN_WGRAD_LAUNCH(4);
#undef MPN_WGRAD_LAUNCH
    count_path(PC_CONV_WGRAD);
}

int64_t conv_bwd_splits(int64_t n_images) { return (n_images + WG_IMAGES - 1) / WG_IMAGES; }

// The regions of the workspace; sized by the layer's shape alone (whichever outputs the call wants)
struct ConvBwdWs {
    float* g;             // [n_images][cout][hw]
    float* wT;            // [cin][cout][taps]
    float* w_partial;     // [splits][cout][cin * taps]
    float* b_partial;     // [splits][cout]
};
size_t conv_bwd_layout(const mpnhip_conv_bwd_args& a, int64_t cin, void* workspace, ConvBwdWs* ws) {
    Carver c(workspace);
    const size_t hw = (size_t)a.H * a.W, taps = (size_t)a.ksize * a.ksize, splits = (size_t)conv_bwd_splits(a.n_images);
    ws->g = c.take<float>((size_t)a.n_images * a.cout * hw);
    ws->wT = c.take<float>(a.n_images > 0 ? (size_t)cin * a.cout * taps : 0);
    ws->w_partial = c.take<float>(splits * a.cout * cin * taps);
    ws->b_partial = c.take<float>(splits * a.cout);
    return c.bytes();
}

// every refusal that does not concern the workspace
int conv_bwd_check(const char* name, const mpnhip_conv_bwd_args* args, ConvSegs* segs, int64_t* cin_out) {
    MPN_CHECK_ARG(args != nullptr, "%s: null args", name);
    const mpnhip_conv_bwd_args& a = *args;
    MPN_CHECK_ARG(a.n_images >= 0, "%s: negative n_images", name);
    MPN_CHECK_ARG(a.H >= 1 && a.W >= 1 && a.cout >= 1, "%s: H %d, W %d, cout %d must be positive", name, a.H, a.W, a.cout);
    MPN_CHECK_ARG(a.transposed == 0, "%s: a transposed convolution has no native backward", name);
    MPN_CHECK_ARG(a.ksize == 1 || a.ksize == 3, "%s: kernel size %d is neither 1 nor 3", name, a.ksize);
    const int64_t hw = (int64_t)a.H * a.W;
    int64_t cin = 0;
    MPN_TRY(check_segments(name, a.seg_data, a.seg_stride, a.seg_channels, a.n_segments, hw, segs, &cin));
    MPN_CHECK_ARG(a.weight != nullptr, "%s: null weight", name);
    MPN_CHECK_ARG(a.grad_out != nullptr, "%s: null grad_out", name);
    MPN_CHECK_ARG(!a.relu || a.y != nullptr, "%s: relu needs the layer's output y", name);
    MPN_CHECK_ARG(a.grad_in != nullptr || a.grad_weight != nullptr || a.grad_bias != nullptr, "%s: no output wanted (all three are null)",
                  name);
    MPN_CHECK_ARG((int64_t)a.cout * hw <= INT32_MAX, "%s: an output image of %lld floats is beyond the 32-bit offsets", name,
                  (long long)((int64_t)a.cout * hw));
    MPN_CHECK_ARG(a.grad_out_stride >= 0 && a.grad_out_stride <= INT32_MAX, "%s: grad_out_stride %lld outside the 32-bit range", name,
                  (long long)a.grad_out_stride);
    MPN_CHECK_ARG(a.y_stride >= 0 && a.y_stride <= INT32_MAX, "%s: y_stride %lld outside the 32-bit range", name, (long long)a.y_stride);
    MPN_CHECK_ARG(cin * a.cout * a.ksize * a.ksize <= INT32_MAX, "%s: the weight is beyond the 32-bit offsets", name);
    const int64_t tiles = (int64_t)((a.W + CONV_TILE - 1) / CONV_TILE) * ((a.H + CONV_TILE - 1) / CONV_TILE);
    MPN_CHECK_ARG(a.n_images * tiles <= INT32_MAX && a.n_images * hw <= (int64_t)INT32_MAX * CB_THREADS &&
                      conv_bwd_splits(a.n_images) <= 65535,
                  "%s: %lld images of %d x %d are more than one launch holds", name, (long long)a.n_images, a.H, a.W);
    MPN_CHECK_ARG(a.cout <= 65535 * 16 && cin <= 65535 * 16, "%s: %d x %lld channels are more than one launch holds", name, a.cout,
                  (long long)cin);
    *cin_out = cin;
    return MPNHIP_OK;
}

// ---- ConvTranspose2d(2, stride 2): the regions of its workspace, sized by the layer's shape alone
struct ConvtBwdWs {
    float* g;             // [n_images][4 cout][hw]
    float* x;             // [n_images][cin][hw], only with more than one segment
    float* w_partial;     // [splits][cin][4 cout]
    float* b_partial;     // [splits][cout]
};
size_t convt_bwd_layout(const mpnhip_conv_bwd_args& a, int64_t cin, void* workspace, ConvtBwdWs* ws) {
    Carver c(workspace);
    const size_t hw = (size_t)a.H * a.W, splits = (size_t)conv_bwd_splits(a.n_images);
    ws->g = c.take<float>((size_t)a.n_images * 4 * a.cout * hw);
    ws->x = c.take<float>(a.n_segments > 1 ? (size_t)a.n_images * cin * hw : 0);
    ws->w_partial = c.take<float>(splits * cin * 4 * a.cout);
    ws->b_partial = c.take<float>(splits * a.cout);
    return c.bytes();
}

// every refusal that does not concern the workspace
int convt_bwd_check(const char* name, const mpnhip_conv_bwd_args* args, ConvSegs* segs, int64_t* cin_out) {
    MPN_CHECK_ARG(args != nullptr, "%s: null args", name);
    const mpnhip_conv_bwd_args& a = *args;
    MPN_CHECK_ARG(a.n_images >= 0, "%s: negative n_images", name);
    MPN_CHECK_ARG(a.H >= 1 && a.W >= 1 && a.cout >= 1, "%s: H %d, W %d, cout %d must be positive", name, a.H, a.W, a.cout);
    MPN_CHECK_ARG(a.transposed != 0, "%s: transposed is 0: a Conv2d's backward is mpnhip_conv2d_backward", name);
    MPN_CHECK_ARG(a.ksize == 2, "%s: a transposed convolution needs kernel size 2 (stride 2, padding 0), not %d", name, a.ksize);
    const int64_t hw = (int64_t)a.H * a.W;
    int64_t cin = 0;
    MPN_TRY(check_segments(name, a.seg_data, a.seg_stride, a.seg_channels, a.n_segments, hw, segs, &cin));
    MPN_CHECK_ARG(a.weight != nullptr, "%s: null weight", name);
    MPN_CHECK_ARG(a.grad_out != nullptr, "%s: null grad_out", name);
    MPN_CHECK_ARG(!a.relu || a.y != nullptr, "%s: relu needs the layer's output y", name);
    MPN_CHECK_ARG(a.grad_in != nullptr || a.grad_weight != nullptr || a.grad_bias != nullptr, "%s: no output wanted (all three are null)",
                  name);
    MPN_CHECK_ARG((int64_t)a.cout * 4 * hw <= INT32_MAX, "%s: an output image of %lld floats is beyond the 32-bit offsets", name,
                  (long long)((int64_t)a.cout * 4 * hw));
    MPN_CHECK_ARG(a.grad_out_stride >= 0 && a.grad_out_stride <= INT32_MAX, "%s: grad_out_stride %lld outside the 32-bit range", name,
                  (long long)a.grad_out_stride);
    MPN_CHECK_ARG(a.y_stride >= 0 && a.y_stride <= INT32_MAX, "%s: y_stride %lld outside the 32-bit range", name, (long long)a.y_stride);
    MPN_CHECK_ARG(cin * a.cout * 4 <= INT32_MAX, "%s: the weight is beyond the 32-bit offsets", name);
    const int64_t tiles = (int64_t)((a.W + CONV_TILE - 1) / CONV_TILE) * ((a.H + CONV_TILE - 1) / CONV_TILE);
    MPN_CHECK_ARG(a.n_images * tiles <= INT32_MAX && a.n_images * hw <= (int64_t)INT32_MAX * CB_THREADS / 4 &&
                      (a.n_segments == 1 || a.n_images * cin * hw <= (int64_t)INT32_MAX * CB_THREADS) && conv_bwd_splits(a.n_images) <= 65535,
                  "%s: %lld images of %d x %d are more than one launch holds", name, (long long)a.n_images, a.H, a.W);
    MPN_CHECK_ARG(a.cout < 65535 * 4 && cin < 65535 * 16, "%s: %d x %lld channels are more than one launch holds", name, a.cout,
                  (long long)cin);
    *cin_out = cin;
    return MPNHIP_OK;
}

}  // namespace
}  // namespace mpnhip

using namespace mpnhip;

extern "C" size_t mpnhip_conv2d_backward_workspace_bytes(const mpnhip_conv_bwd_args* args) {
    ConvSegs segs;
    int64_t cin = 0;
    if (conv_bwd_check("mpnhip_conv2d_backward_workspace_bytes", args, &segs, &cin) != MPNHIP_OK) return 0;
    ConvBwdWs ws;
    return conv_bwd_layout(*args, cin, nullptr, &ws);
}

extern "C" int mpnhip_conv2d_backward(const mpnhip_conv_bwd_args* args, void* workspace, size_t workspace_bytes, void* stream_) {
    static const char* const name = "mpnhip_conv2d_backward";
    hipStream_t stream = (hipStream_t)stream_;
    ConvSegs segs;
    int64_t cin64 = 0;
    MPN_TRY(conv_bwd_check(name, args, &segs, &cin64));
    const mpnhip_conv_bwd_args& a = *args;
    const int cin = (int)cin64, taps = a.ksize * a.ksize, hw = a.H * a.W;
    const int wcount = a.cout * cin * taps;
    if (a.n_images == 0) {
        if (a.grad_weight) MPN_HIP(hipMemsetAsync(a.grad_weight, 0, sizeof(float) * wcount, stream));
        if (a.grad_bias) MPN_HIP(hipMemsetAsync(a.grad_bias, 0, sizeof(float) * a.cout, stream));
        return MPNHIP_OK;
    }
    ConvBwdWs ws;
    const size_t need = conv_bwd_layout(a, cin, nullptr, &ws);
    MPN_CHECK_ARG(workspace != nullptr && workspace_bytes >= need, "%s: workspace %zu < %zu", name, workspace ? workspace_bytes : (size_t)0,
                  need);
    conv_bwd_layout(a, cin, workspace, &ws);
    const int splits = (int)conv_bwd_splits(a.n_images);

    // gate and bias partial sums; without a ReLU g is grad_out as it stands
    const float* g = a.relu ? ws.g : a.grad_out;
    const int64_t g_stride = a.relu ? (int64_t)a.cout * hw : a.grad_out_stride;
    if (a.relu || a.grad_bias) {
        conv_bwd_gate_kernel<<<dim3((unsigned)a.cout, (unsigned)splits), CB_THREADS, 0, stream>>>(
            a.grad_out, a.grad_out_stride, a.relu ? a.y : nullptr, a.y_stride, a.cout, hw, a.n_images, a.relu ? ws.g : nullptr,
            a.grad_bias ? ws.b_partial : nullptr);
        count_path(PC_CONV_BWD_GATE);
        if (a.grad_bias) conv_bwd_sum_kernel<<<blocks_for(a.cout), CB_THREADS, 0, stream>>>(ws.b_partial, splits, a.cout, a.grad_bias);
        MPN_LAUNCH_CHECK();
    }

    if (a.grad_in) {
        conv_bwd_flip_kernel<<<blocks_for(wcount), CB_THREADS, 0, stream>>>(a.weight, a.cout, cin, taps, ws.wT);
        MPN_LAUNCH_CHECK();
        mpnhip_conv_args f = {};
        f.seg_data[0] = g;
        f.seg_stride[0] = g_stride;
        f.seg_channels[0] = a.cout;
        f.n_segments = 1;
        f.H = a.H;
        f.W = a.W;
        f.cout = cin;
        f.ksize = a.ksize;
        f.n_images = a.n_images;
        f.weight = ws.wT;
        f.out = a.grad_in;
        f.out_stride = (int64_t)cin * hw;
        MPN_TRY(mpnhip_conv2d_forward(&f, stream_));
    }

    if (a.grad_weight) {
        if (a.ksize == 1) launch_conv_wgrad<1>(segs, cin, a, g, g_stride, splits, ws.w_partial, stream);
        else launch_conv_wgrad<3>(segs, cin, a, g, g_stride, splits, ws.w_partial, stream);
        conv_bwd_sum_kernel<<<blocks_for(wcount), CB_THREADS, 0, stream>>>(ws.w_partial, splits, wcount, a.grad_weight);
        MPN_LAUNCH_CHECK();
    }
    return MPNHIP_OK;
}

extern "C" size_t mpnhip_conv_transpose2d_backward_workspace_bytes(const mpnhip_conv_bwd_args* args) {
    ConvSegs segs;
    int64_t cin = 0;
    if (convt_bwd_check("mpnhip_conv_transpose2d_backward_workspace_bytes", args, &segs, &cin) != MPNHIP_OK) return 0;
    ConvtBwdWs ws;
    return convt_bwd_layout(*args, cin, nullptr, &ws);
}

extern "C" int mpnhip_conv_transpose2d_backward(const mpnhip_conv_bwd_args* args, void* workspace, size_t workspace_bytes,
                                                void* stream_) {
    static const char* const name = "mpnhip_conv_transpose2d_backward";
    hipStream_t stream = (hipStream_t)stream_;
    ConvSegs segs;
    int64_t cin64 = 0;
    MPN_TRY(convt_bwd_check(name, args, &segs, &cin64));
    const mpnhip_conv_bwd_args& a = *args;
    const int cin = (int)cin64, hw = a.H * a.W, m4 = 4 * a.cout;
    const int wcount = cin * m4;
    if (a.n_images == 0) {
        if (a.grad_weight) MPN_HIP(hipMemsetAsync(a.grad_weight, 0, sizeof(float) * wcount, stream));
        if (a.grad_bias) MPN_HIP(hipMemsetAsync(a.grad_bias, 0, sizeof(float) * a.cout, stream));
        return MPNHIP_OK;
    }
    ConvtBwdWs ws;
    const size_t need = convt_bwd_layout(a, cin, nullptr, &ws);
    MPN_CHECK_ARG(workspace != nullptr && workspace_bytes >= need, "%s: workspace %zu < %zu", name, workspace ? workspace_bytes : (size_t)0,
                  need);
    convt_bwd_layout(a, cin, workspace, &ws);
    const int splits = (int)conv_bwd_splits(a.n_images);
    count_path(PC_CONV_TRANSPOSE_BWD);

    // gate, space-to-depth and the bias partial sums in one pass over grad_out
    const bool need_g = a.grad_in || a.grad_weight;
    convt_bwd_gate_kernel<<<dim3((unsigned)a.cout, (unsigned)splits), CB_THREADS, 0, stream>>>(
        a.grad_out, a.grad_out_stride, a.relu ? a.y : nullptr, a.y_stride, a.cout, a.H, a.W, a.n_images, need_g ? ws.g : nullptr,
        a.grad_bias ? ws.b_partial : nullptr);
    if (a.grad_bias) conv_bwd_sum_kernel<<<blocks_for(a.cout), CB_THREADS, 0, stream>>>(ws.b_partial, splits, a.cout, a.grad_bias);
    MPN_LAUNCH_CHECK();
    const int64_t g_stride = (int64_t)m4 * hw;

    if (a.grad_in) {   // a 1 x 1 Conv2d from the 4 cout channels of g' to the cin input channels: its weight is this layer's, as stored
        mpnhip_conv_args f = {};
        f.seg_data[0] = ws.g;
        f.seg_stride[0] = g_stride;
        f.seg_channels[0] = m4;
        f.n_segments = 1;
        f.H = a.H;
        f.W = a.W;
        f.cout = cin;
        f.ksize = 1;
        f.n_images = a.n_images;
        f.weight = a.weight;
        f.out = a.grad_in;
        f.out_stride = (int64_t)cin * hw;
        MPN_TRY(mpnhip_conv2d_forward(&f, stream_));
    }

    if (a.grad_weight) {
        // rows from the layer's input x (one dense tensor), columns from g': partial[split][cin][4 cout], the weight's own layout
        const float* x = segs.p[0];
        int64_t x_stride = segs.stride[0];
        if (segs.n > 1) {
            const int64_t total = a.n_images * cin * hw;
            conv_bwd_gather_kernel<<<blocks_for(total), CB_THREADS, 0, stream>>>(segs, cin, hw, total, ws.x);
            MPN_LAUNCH_CHECK();
            x = ws.x;
            x_stride = (int64_t)cin * hw;
        }
        if (cin <= CONV_SMALL_COUT) {   // the plain 1 x 1 kernel with the roles swapped: "cout" = the layer's input channels, segments = g'
            ConvSegs gs = {};
            gs.p[0] = ws.g;
            gs.stride[0] = g_stride;
            gs.ch[0] = m4;
            gs.n = 1;
            mpnhip_conv_bwd_args r = a;
            r.cout = cin;
            launch_conv_wgrad<1>(gs, m4, r, x, x_stride, splits, ws.w_partial, stream);
        } else {
            const int col_tiles = (m4 + CTW_COLS - 1) / CTW_COLS;
            const dim3 grid((unsigned)((cin + CTW_ROWS - 1) / CTW_ROWS * col_tiles), (unsigned)splits);
            convt_wgrad_kernel<<<grid, CB_THREADS, 0, stream>>>(x, x_stride, cin, ws.g, m4, hw, a.n_images, ws.w_partial, col_tiles);
        }
        conv_bwd_sum_kernel<<<blocks_for(wcount), CB_THREADS, 0, stream>>>(ws.w_partial, splits, wcount, a.grad_weight);
        MPN_LAUNCH_CHECK();
    }
    return MPNHIP_OK;
}
