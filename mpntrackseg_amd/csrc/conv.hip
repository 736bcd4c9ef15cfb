// Inference forward of the mask branch's convolution-type layers (include/mpnhip.h: mpnhip_conv2d_forward,
// mpnhip_layer_norm_forward): implicit-GEMM convolution (1x1 / 3x3, stride 1, padding k / 2) and ConvTranspose2d(2, stride 2)
// on the fp32-input MFMA, a plain variant for very few output channels, and LayerNorm over [C, H, W].
//
// GEMM view of conv_tile_kernel: M = output channels (rows of the weight), N = the pixels of one 14 x 14 output tile of one
// image (196, padded to 7 x 32 columns), K = input channels x taps.  One block per (image, tile, group of MT x 32 rows).  K is
// walked in chunks of CK input channels: the chunk's 16 x 16 input patches (halo cells outside the image written as zeros) and
// the chunk's weight columns are staged in LDS, then every wave runs v_mfma_f32_32x32x2_f32 over the chunk.  The summation
// order (channel, then tap; one chain per output) is a function of the layer alone: no split of K across blocks, no atomics,
// so a pixel's bits do not depend on the number of images in the launch.
//
// ConvTranspose2d(2, stride 2, padding 0) is the same kernel with TRANSPOSED: a tap-less product whose M index is
// (cout, dy, dx) -- the weight [cin][cout][2][2] is [K][M] as it stands -- and whose epilogue scatters row (co, dy, dx) of input
// pixel (y, x) to out[co][2 y + dy][2 x + dx].
#include "common.h"

#include <math.h>

namespace mpnhip {
namespace {

constexpr int CONV_NT = 7;                    // 32-pixel column tiles per block: 7 * 32 >= 196
constexpr int CONV_THREADS = 256;

using f32x16 = __attribute__((ext_vector_type(16))) float;

// the patch offset of k index `k` of a chunk: k = channel * taps + tap
template <int KS>
__device__ __forceinline__ constexpr int patch_k_offset(int k) {
    return (k / (KS * KS)) * CONV_PATCH_CELLS + ((k % (KS * KS)) / KS) * CONV_PATCH + (k % (KS * KS)) % KS;
}

// KS: 1 or 3 (TRANSPOSED: 1).  MT: 32-row tiles of M per block.  M: rows of the product (cout, or 4 cout when TRANSPOSED).
template <int KS, int MT, bool TRANSPOSED>
__global__ __launch_bounds__(CONV_THREADS) void conv_tile_kernel(ConvSegs segs, int cin, int H, int W, int M,
                                                                 const float* __restrict__ weight, const float* __restrict__ bias,
                                                                 int relu, float* __restrict__ out, int64_t out_stride, int tiles_x,
                                                                 int tiles_per_image) {
    constexpr int TAPS = KS * KS;
    constexpr int CK = KS == 3 ? 8 : 32;       // input channels per chunk
    constexpr int KC = CK * TAPS;              // k per chunk (even)
    constexpr int MG = 32 * MT;                // rows per block
    constexpr int PW = MG + 1;                 // row pitch of the weight image [k][m]: conflict-free transposing stores
    constexpr int PAD = KS / 2;
    constexpr int EDGE = CONV_TILE + 2 * PAD;  // patch cells in use per row / column
    __shared__ float patch[CK * CONV_PATCH_CELLS];
    __shared__ float wl[KC * PW];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 31, lh = lane >> 5;
    const int img = blockIdx.x / tiles_per_image, tile = blockIdx.x % tiles_per_image;
    const int y0 = (tile / tiles_x) * CONV_TILE, x0 = (tile % tiles_x) * CONV_TILE;
    const int m0 = blockIdx.y * MG;
    const int hw = H * W;

    // this wave's pixel columns: tiles wave and wave + 4 (the latter exists for waves 0 .. 2)
    const bool second = wave + 4 < CONV_NT;
    int poff[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int p = (wave + 4 * j) * 32 + li;
        poff[j] = p < CONV_TILE * CONV_TILE ? (p / CONV_TILE) * CONV_PATCH + p % CONV_TILE : 0;
    }

    f32x16 acc[MT][2];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // the cell of the patch this thread stages for every channel of a chunk
    const int pr = t >> 4, pc = t & 15;
    const int gy = y0 + pr - PAD, gx = x0 + pc - PAD;
    const bool cell_ok = pr < EDGE && pc < EDGE && gy >= 0 && gy < H && gx >= 0 && gx < W;
    const int cell_off = gy * W + gx;
    const int ktotal = cin * TAPS;

    // The chunk after the one being multiplied travels in registers: its global loads are issued before the MFMA loop and
    // land in LDS after it, so their latency hides behind the products instead of standing between two barriers.
    constexpr int WREGS = MG * KC / CONV_THREADS;   // weight elements per thread and chunk (32 * KC is a multiple of 256)
    static_assert(MG * KC % CONV_THREADS == 0, "weight chunk must divide among the threads");
    float pv[CK], wv[WREGS];
    int seg = 0, seg_c0 = 0;                    // the segment that holds channel c0 + ch (channels only go up)
    auto fetch = [&](int c0) {
#pragma unroll
        for (int ch = 0; ch < CK; ++ch) {
            const int c = c0 + ch;
            float v = 0.f;
            if (c < cin) {
                while (c >= seg_c0 + segs.ch[seg]) {
                    seg_c0 += segs.ch[seg];
                    ++seg;
                }
                if (cell_ok) v = segs.p[seg][(int64_t)img * segs.stride[seg] + (c - seg_c0) * hw + cell_off];
            }
            pv[ch] = v;
        }
#pragma unroll
        for (int q = 0; q < WREGS; ++q) {
            const int idx = t + q * CONV_THREADS;
            if (!TRANSPOSED) {                  // weight[m][c0 * TAPS + k]: k contiguous in memory
                const int k = idx % KC, m = idx / KC;
                const int gk = c0 * TAPS + k;
                wv[q] = (m0 + m < M && gk < ktotal) ? weight[(m0 + m) * ktotal + gk] : 0.f;
            } else {                            // weight[c0 + k][m]: m contiguous in memory
                const int m = idx % MG, k = idx / MG;
                wv[q] = (m0 + m < M && c0 + k < cin) ? weight[(c0 + k) * M + m0 + m] : 0.f;
            }
        }
    };
    fetch(0);
    for (int c0 = 0; c0 < cin; c0 += CK) {
#pragma unroll
        for (int ch = 0; ch < CK; ++ch) patch[ch * CONV_PATCH_CELLS + t] = pv[ch];
#pragma unroll
        for (int q = 0; q < WREGS; ++q) {
            const int idx = t + q * CONV_THREADS;
            if (!TRANSPOSED) wl[(idx % KC) * PW + idx / KC] = wv[q];
            else wl[(idx / MG) * PW + idx % MG] = wv[q];
        }
        __syncthreads();
        if (c0 + CK < cin) fetch(c0 + CK);
#pragma unroll
        for (int kk = 0; kk < KC; kk += 2) {
            const int koff = lh ? patch_k_offset<KS>(kk + 1) : patch_k_offset<KS>(kk);
            float a[MT];
#pragma unroll
            for (int i = 0; i < MT; ++i) a[i] = wl[(kk + lh) * PW + 32 * i + li];
            const float b0 = patch[koff + poff[0]];
#pragma unroll
            for (int i = 0; i < MT; ++i) acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b0, acc[i][0], 0, 0, 0);
            if (second) {
                const float b1 = patch[koff + poff[1]];
#pragma unroll
                for (int i = 0; i < MT; ++i) acc[i][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b1, acc[i][1], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // D[i][j] of a 32 x 32 tile: j = lane & 31 (pixel), i = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) (row of M)
    float* __restrict__ o = out + (int64_t)img * out_stride;
    // (TRANSPOSED) every pair (dx = 0, 1) is 8-byte aligned: the offset inside an image is even, the image bases are too
    const bool pair_stores = (reinterpret_cast<uintptr_t>(out) & 7) == 0 && (out_stride & 1) == 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (j == 1 && !second) break;
        const int p = (wave + 4 * j) * 32 + li;
        const int oy = y0 + p / CONV_TILE, ox = x0 + p % CONV_TILE;
        if (p >= CONV_TILE * CONV_TILE || oy >= H || ox >= W) continue;
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            if (!TRANSPOSED) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = m0 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    if (m >= M) continue;
                    float v = acc[i][j][r];
                    if (bias) v += bias[m];
                    if (relu) v = fmaxf(v, 0.f);
                    o[m * hw + oy * W + ox] = v;
                }
            } else {
                // rows m = 4 co + 2 dy + dx: registers r, r + 1 (r even) are dx = 0, 1 of one (co, dy), neighbours in memory
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                    const int m = m0 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lh;   // even; M = 4 cout: m + 1 < M with it
                    if (m >= M) continue;
                    const int co = m >> 2, dy = (m >> 1) & 1;
                    const float bv = bias ? bias[co] : 0.f;
                    float v0 = acc[i][j][r] + bv, v1 = acc[i][j][r + 1] + bv;
                    if (relu) {
                        v0 = fmaxf(v0, 0.f);
                        v1 = fmaxf(v1, 0.f);
                    }
                    float* dst = o + co * (4 * hw) + (2 * oy + dy) * (2 * W) + 2 * ox;
                    if (pair_stores) {
                        *reinterpret_cast<float2*>(dst) = make_float2(v0, v1);
                    } else {
                        dst[0] = v0;
                        dst[1] = v1;
                    }
                }
            }
        }
    }
}

// cout <= CONV_SMALL_COUT: one thread per output pixel, every output channel in registers; the same summation order
// (channel, then tap) as the tile kernel.  The weight index is uniform over the block.
template <int KS>
__global__ __launch_bounds__(CONV_THREADS) void conv_small_cout_kernel(ConvSegs segs, int cin, int H, int W, int cout,
                                                                       const float* __restrict__ weight,
                                                                       const float* __restrict__ bias, int relu,
                                                                       float* __restrict__ out, int64_t out_stride, int64_t total) {
    constexpr int TAPS = KS * KS, PAD = KS / 2;
    const int64_t idx = (int64_t)blockIdx.x * CONV_THREADS + threadIdx.x;
    if (idx >= total) return;
    const int hw = H * W;
    const int64_t img = idx / hw;
    const int pix = (int)(idx % hw), oy = pix / W, ox = pix % W;
    float acc[CONV_SMALL_COUT];
#pragma unroll
    for (int co = 0; co < CONV_SMALL_COUT; ++co) acc[co] = 0.f;
    int c = 0;
    for (int s = 0; s < segs.n; ++s) {
        const float* __restrict__ x = segs.p[s] + img * segs.stride[s];
        for (int lc = 0; lc < segs.ch[s]; ++lc, ++c) {
#pragma unroll
            for (int tap = 0; tap < TAPS; ++tap) {
                const int iy = oy + tap / KS - PAD, ix = ox + tap % KS - PAD;
                const float v = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? x[lc * hw + iy * W + ix] : 0.f;
#pragma unroll
                for (int co = 0; co < CONV_SMALL_COUT; ++co)
                    if (co < cout) acc[co] = fmaf(weight[(co * cin + c) * TAPS + tap], v, acc[co]);
            }
        }
    }
    float* __restrict__ o = out + img * out_stride;
#pragma unroll
    for (int co = 0; co < CONV_SMALL_COUT; ++co) {
        if (co >= cout) break;
        float v = acc[co] + (bias ? bias[co] : 0.f);
        if (relu) v = fmaxf(v, 0.f);
        o[co * hw + pix] = v;
    }
}

// ------------------------------------------------------------------------------------ LayerNorm over [C, H, W]
constexpr int LN_THREADS = 512;

// sum over the block in a fixed order: a shuffle tree inside every wave, then the eight wave sums one after the other
__device__ __forceinline__ float ln_block_sum(float v, float* red) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    __syncthreads();                            // red may still be read from the previous sum
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < LN_THREADS / 64; ++w) s += red[w];
    return s;
}

__global__ __launch_bounds__(LN_THREADS) void layer_norm_kernel(ConvSegs segs, int hw, int feat, const float* __restrict__ weight,
                                                                const float* __restrict__ bias, float eps,
                                                                float* __restrict__ out, int64_t out_stride) {
    __shared__ float red[LN_THREADS / 64];
    const int64_t img = blockIdx.x;
    const int t = threadIdx.x;
    float s = 0.f;
    for (int sg = 0; sg < segs.n; ++sg) {
        const float* __restrict__ x = segs.p[sg] + img * segs.stride[sg];
        const int n = segs.ch[sg] * hw;
        for (int i = t; i < n; i += LN_THREADS) s += x[i];
    }
    const float mean = ln_block_sum(s, red) / (float)feat;
    float q = 0.f;
    for (int sg = 0; sg < segs.n; ++sg) {
        const float* __restrict__ x = segs.p[sg] + img * segs.stride[sg];
        const int n = segs.ch[sg] * hw;
        for (int i = t; i < n; i += LN_THREADS) {
            const float d = x[i] - mean;
            q = fmaf(d, d, q);
        }
    }
    const float rstd = 1.f / sqrtf(ln_block_sum(q, red) / (float)feat + eps);
    float* __restrict__ o = out + img * out_stride;
    int base = 0;
    for (int sg = 0; sg < segs.n; ++sg) {
        const float* __restrict__ x = segs.p[sg] + img * segs.stride[sg];
        const int n = segs.ch[sg] * hw;
        for (int i = t; i < n; i += LN_THREADS) {
            float v = (x[i] - mean) * rstd;
            if (weight) v = fmaf(v, weight[base + i], bias[base + i]);
            o[base + i] = v;
        }
        base += n;
    }
}

// ---- backward (mpnhip_layer_norm_backward)
constexpr int LNB_IMAGES = 8;                 // images per block of the affine gradients: the split is a function of n_images alone
constexpr int LNB_THREADS = 256;

// One block per image.  mean / rstd: layer_norm_kernel's own two passes and block sums (same order, same bits), written to
// stats[img] = (mean, rstd); then (grad_in given) a = sum g gamma, b = sum g gamma xhat and grad_in = rstd (g gamma - a / F - xhat b / F).
__global__ __launch_bounds__(LN_THREADS) void layer_norm_bwd_image_kernel(ConvSegs segs, int hw, int feat,
                                                                          const float* __restrict__ weight, float eps,
                                                                          const float* __restrict__ grad_out, int64_t go_stride,
                                                                          float* __restrict__ grad_in, float* __restrict__ stats) {
    __shared__ float red[LN_THREADS / 64];
    const int64_t img = blockIdx.x;
    const int t = threadIdx.x;
    float s = 0.f;
    for (int sg = 0; sg < segs.n; ++sg) {
        const float* __restrict__ x = segs.p[sg] + img * segs.stride[sg];
        const int n = segs.ch[sg] * hw;
        for (int i = t; i < n; i += LN_THREADS) s += x[i];
    }
    const float mean = ln_block_sum(s, red) / (float)feat;
    float q = 0.f;
    for (int sg = 0; sg < segs.n; ++sg) {
        const float* __restrict__ x = segs.p[sg] + img * segs.stride[sg];
        const int n = segs.ch[sg] * hw;
        for (int i = t; i < n; i += LN_THREADS) {
            const float d = x[i] - mean;
            q = fmaf(d, d, q);
        }
    }
    const float rstd = 1.f / sqrtf(ln_block_sum(q, red) / (float)feat + eps);
    if (t == 0) {
        stats[2 * img] = mean;
        stats[2 * img + 1] = rstd;
    }
    if (!grad_in) return;
    const float* __restrict__ go = grad_out + img * go_stride;
    float a = 0.f, b = 0.f;
    int base = 0;
    for (int sg = 0; sg < segs.n; ++sg) {
        const float* __restrict__ x = segs.p[sg] + img * segs.stride[sg];
        const int n = segs.ch[sg] * hw;
        for (int i = t; i < n; i += LN_THREADS) {
            const float gg = weight ? go[base + i] * weight[base + i] : go[base + i];
            a += gg;
            b = fmaf(gg, (x[i] - mean) * rstd, b);
        }
        base += n;
    }
    a = ln_block_sum(a, red) / (float)feat;
    b = ln_block_sum(b, red) / (float)feat;
    float* __restrict__ gi = grad_in + img * (int64_t)feat;
    base = 0;
    for (int sg = 0; sg < segs.n; ++sg) {
        const float* __restrict__ x = segs.p[sg] + img * segs.stride[sg];
        const int n = segs.ch[sg] * hw;
        for (int i = t; i < n; i += LN_THREADS) {
            const float gg = weight ? go[base + i] * weight[base + i] : go[base + i];
            gi[base + i] = rstd * (gg - a - (x[i] - mean) * rstd * b);
        }
        base += n;
    }
}

// grid (blocks along i, splits): one thread per element i, the block's LNB_IMAGES images one after the other.
// w_partial / b_partial: [splits][feat], either may be nullptr
__global__ __launch_bounds__(LNB_THREADS) void layer_norm_bwd_affine_kernel(ConvSegs segs, int hw, int feat,
                                                                            const float* __restrict__ grad_out, int64_t go_stride,
                                                                            const float* __restrict__ stats, int64_t n_images,
                                                                            float* __restrict__ w_partial,
                                                                            float* __restrict__ b_partial) {
    const int i = blockIdx.x * LNB_THREADS + threadIdx.x;
    if (i >= feat) return;
    int sg = 0, base = 0;
    while (i >= base + segs.ch[sg] * hw) {
        base += segs.ch[sg] * hw;
        ++sg;
    }
    const float* __restrict__ x = segs.p[sg] + (i - base);
    const int64_t xs = segs.stride[sg];
    const int64_t img0 = (int64_t)blockIdx.y * LNB_IMAGES;
    const int64_t img1 = img0 + LNB_IMAGES < n_images ? img0 + LNB_IMAGES : n_images;
    float sw = 0.f, sb = 0.f;
    for (int64_t img = img0; img < img1; ++img) {
        const float g = grad_out[img * go_stride + i];
        sb += g;
        if (w_partial) sw = fmaf(g, (x[img * xs] - stats[2 * img]) * stats[2 * img + 1], sw);
    }
    if (w_partial) w_partial[(int64_t)blockIdx.y * feat + i] = sw;
    if (b_partial) b_partial[(int64_t)blockIdx.y * feat + i] = sb;
}

// out[i] = partial[0][i] + partial[1][i] + ... in that order, for the weight and the bias gradient (either may be nullptr)
__global__ __launch_bounds__(LNB_THREADS) void layer_norm_bwd_sum_kernel(const float* __restrict__ w_partial,
                                                                         const float* __restrict__ b_partial, int splits, int feat,
                                                                         float* __restrict__ grad_weight,
                                                                         float* __restrict__ grad_bias) {
    const int i = blockIdx.x * LNB_THREADS + threadIdx.x;
    if (i >= feat) return;
    if (grad_weight) {
        float s = 0.f;
        for (int sp = 0; sp < splits; ++sp) s += w_partial[(int64_t)sp * feat + i];
        grad_weight[i] = s;
    }
    if (grad_bias) {
        float s = 0.f;
        for (int sp = 0; sp < splits; ++sp) s += b_partial[(int64_t)sp * feat + i];
        grad_bias[i] = s;
    }
}

}  // namespace

// the checks the entry points share (common.h); *cin: the channel total.  name: the entry point, for the message
int check_segments(const char* name, const float* const* data, const int64_t* stride, const int* channels, int n_segments,
                   int64_t hw, ConvSegs* segs, int64_t* cin) {
    MPN_CHECK_ARG(n_segments >= 1 && n_segments <= MPNHIP_CONV_MAX_SEGMENTS, "%s: n_segments %d outside 1 .. %d", name, n_segments,
                  MPNHIP_CONV_MAX_SEGMENTS);
    int64_t c = 0;
    for (int s = 0; s < MPNHIP_CONV_MAX_SEGMENTS; ++s) {
        segs->p[s] = nullptr;
        segs->stride[s] = 0;
        segs->ch[s] = 0;
    }
    for (int s = 0; s < n_segments; ++s) {
        MPN_CHECK_ARG(data[s] != nullptr, "%s: segment %d: null pointer", name, s);
        MPN_CHECK_ARG(channels[s] >= 1, "%s: segment %d: %d channels", name, s, channels[s]);
        MPN_CHECK_ARG(stride[s] >= 0 && stride[s] <= INT32_MAX, "%s: segment %d: image stride %lld outside the 32-bit range", name, s,
                      (long long)stride[s]);
        segs->p[s] = data[s];
        segs->stride[s] = stride[s];
        segs->ch[s] = channels[s];
        c += channels[s];
    }
    segs->n = n_segments;
    MPN_CHECK_ARG(c * hw <= INT32_MAX, "%s: an input image of %lld x %lld floats is beyond the 32-bit offsets", name, (long long)c,
                  (long long)hw);
    *cin = c;
    return MPNHIP_OK;
}

namespace {

template <int KS, bool TRANSPOSED>
void launch_conv_tile(const ConvSegs& segs, int cin, const mpnhip_conv_args& a, int M, hipStream_t stream) {
    const int tiles_x = (a.W + CONV_TILE - 1) / CONV_TILE, tiles = tiles_x * ((a.H + CONV_TILE - 1) / CONV_TILE);
    const int mt = M <= 32 ? 1 : (M > 64 && M <= 96) ? 3 : 2;
    const dim3 grid((unsigned)(a.n_images * tiles), (unsigned)((M + 32 * mt - 1) / (32 * mt)));
#define MPN_CONV_LAUNCH(MT)                                                                                                          \
    conv_tile_kernel<KS, MT, TRANSPOSED><<<grid, CONV_THREADS, 0, stream>>>(segs, cin, a.H, a.W, M, a.weight, a.bias, a.relu, a.out, \
                                                                            a.out_stride, tiles_x, tiles)
    if (mt == 1) MPN_CONV_LAUNCH(1);
    else if (mt == 2) MPN_CONV_LAUNCH(2);
    else MPN_CONV_LAUNCH(3);
#undef MPN_CONV_LAUNCH
}

}  // namespace
}  // namespace mpnhip

using namespace mpnhip;

extern "C" int mpnhip_conv2d_forward(const mpnhip_conv_args* args, void* stream_) {
    static const char* const name = "mpnhip_conv2d_forward";
    hipStream_t stream = (hipStream_t)stream_;
    MPN_CHECK_ARG(args != nullptr, "%s: null args", name);
    const mpnhip_conv_args& a = *args;
    MPN_CHECK_ARG(a.n_images >= 0, "%s: negative n_images", name);
    if (a.n_images == 0) return MPNHIP_OK;
    MPN_CHECK_ARG(a.H >= 1 && a.W >= 1 && a.cout >= 1, "%s: H %d, W %d, cout %d must be positive", name, a.H, a.W, a.cout);
    if (a.transposed)
        MPN_CHECK_ARG(a.ksize == 2, "%s: a transposed convolution needs kernel size 2 (stride 2, padding 0), not %d", name, a.ksize);
    else
        MPN_CHECK_ARG(a.ksize == 1 || a.ksize == 3, "%s: kernel size %d is neither 1 nor 3", name, a.ksize);
    const int64_t hw = (int64_t)a.H * a.W;
    ConvSegs segs;
    int64_t cin = 0;
    MPN_TRY(check_segments(name, a.seg_data, a.seg_stride, a.seg_channels, a.n_segments, hw, &segs, &cin));
    MPN_CHECK_ARG(a.weight != nullptr && a.out != nullptr, "%s: null weight or out", name);
    const int64_t out_floats = (int64_t)a.cout * hw * (a.transposed ? 4 : 1);
    MPN_CHECK_ARG(out_floats <= INT32_MAX, "%s: an output image of %lld floats is beyond the 32-bit offsets", name, (long long)out_floats);
    MPN_CHECK_ARG(a.out_stride >= 0 && a.out_stride <= INT32_MAX, "%s: out_stride %lld outside the 32-bit range", name,
                  (long long)a.out_stride);
    MPN_CHECK_ARG(cin * a.cout * a.ksize * a.ksize <= INT32_MAX, "%s: the weight is beyond the 32-bit offsets", name);
    const int64_t tiles = (int64_t)((a.W + CONV_TILE - 1) / CONV_TILE) * ((a.H + CONV_TILE - 1) / CONV_TILE);
    MPN_CHECK_ARG(a.n_images * tiles <= INT32_MAX && a.n_images * hw <= (int64_t)INT32_MAX * CONV_THREADS,
                  "%s: %lld images of %d x %d are more than one launch holds", name, (long long)a.n_images, a.H, a.W);
    MPN_CHECK_ARG((int64_t)a.cout * 4 / 64 < 65535, "%s: cout %d is more than one launch holds", name, a.cout);

    if (a.transposed) {
        launch_conv_tile<1, true>(segs, (int)cin, a, 4 * a.cout, stream);
        count_path(PC_CONV_TRANSPOSE);
    } else if (a.cout <= CONV_SMALL_COUT) {
        const int64_t total = a.n_images * hw;
        const unsigned blocks = (unsigned)((total + CONV_THREADS - 1) / CONV_THREADS);
        if (a.ksize == 1)
            conv_small_cout_kernel<1><<<blocks, CONV_THREADS, 0, stream>>>(segs, (int)cin, a.H, a.W, a.cout, a.weight, a.bias, a.relu,
                                                                           a.out, a.out_stride, total);
        else
            conv_small_cout_kernel<3><<<blocks, CONV_THREADS, 0, stream>>>(segs, (int)cin, a.H, a.W, a.cout, a.weight, a.bias, a.relu,
                                                                           a.out, a.out_stride, total);
        count_path(PC_CONV_SMALL_COUT);
    } else {
        if (a.ksize == 1) launch_conv_tile<1, false>(segs, (int)cin, a, a.cout, stream);
        else launch_conv_tile<3, false>(segs, (int)cin, a, a.cout, stream);
        count_path(PC_CONV_TILE);
    }
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}

extern "C" int mpnhip_layer_norm_forward(const float* const* seg_data, const int64_t* seg_stride, const int* seg_channels,
                                         int n_segments, int64_t n_images, int64_t hw, const float* weight, const float* bias,
                                         float eps, float* out, int64_t out_stride, void* stream_) {
    static const char* const name = "mpnhip_layer_norm_forward";
    hipStream_t stream = (hipStream_t)stream_;
    MPN_CHECK_ARG(n_images >= 0, "%s: negative n_images", name);
    if (n_images == 0) return MPNHIP_OK;
    MPN_CHECK_ARG(seg_data != nullptr && seg_stride != nullptr && seg_channels != nullptr, "%s: null segment lists", name);
    MPN_CHECK_ARG(hw >= 1 && hw <= INT32_MAX, "%s: hw %lld must be positive and within 32 bits", name, (long long)hw);
    MPN_CHECK_ARG(eps >= 0.f && isfinite(eps), "%s: eps %g", name, (double)eps);
    ConvSegs segs;
    int64_t c = 0;
    MPN_TRY(check_segments(name, seg_data, seg_stride, seg_channels, n_segments, hw, &segs, &c));
    MPN_CHECK_ARG(out != nullptr, "%s: null out", name);
    MPN_CHECK_ARG((weight == nullptr) == (bias == nullptr), "%s: weight and bias must both be given or both be null", name);
    MPN_CHECK_ARG(out_stride >= 0 && out_stride <= INT32_MAX, "%s: out_stride %lld outside the 32-bit range", name,
                  (long long)out_stride);
    MPN_CHECK_ARG(n_images <= INT32_MAX, "%s: %lld images are more than one launch holds", name, (long long)n_images);
    layer_norm_kernel<<<(unsigned)n_images, LN_THREADS, 0, stream>>>(segs, (int)hw, (int)(c * hw), weight, bias, eps, out, out_stride);
    count_path(PC_LAYER_NORM);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}

namespace mpnhip {
namespace {

int64_t ln_bwd_splits(int64_t n_images) { return (n_images + LNB_IMAGES - 1) / LNB_IMAGES; }

// The regions of the backward's workspace; sized by the shape and by whether there is an affine
struct LnBwdWs {
    float* stats;         // [n_images][2]: mean, rstd
    float* w_partial;     // [splits][feat]
    float* b_partial;     // [splits][feat]
};
size_t ln_bwd_layout(int64_t n_images, int64_t feat, bool affine, void* workspace, LnBwdWs* ws) {
    Carver c(workspace);
    const size_t splits = (size_t)ln_bwd_splits(n_images);
    ws->stats = c.take<float>((size_t)n_images * 2);
    ws->w_partial = c.take<float>(affine ? splits * feat : 0);
    ws->b_partial = c.take<float>(affine ? splits * feat : 0);
    return c.bytes();
}

// every refusal that does not concern the workspace
int ln_bwd_check(const char* name, const float* const* seg_data, const int64_t* seg_stride, const int* seg_channels, int n_segments,
                 int64_t n_images, int64_t hw, const float* weight, float eps, const float* grad_out, int64_t grad_out_stride,
                 const float* grad_in, const float* grad_weight, const float* grad_bias, ConvSegs* segs, int64_t* feat) {
    MPN_CHECK_ARG(n_images >= 0, "%s: negative n_images", name);
    MPN_CHECK_ARG(seg_data != nullptr && seg_stride != nullptr && seg_channels != nullptr, "%s: null segment lists", name);
    MPN_CHECK_ARG(hw >= 1 && hw <= INT32_MAX, "%s: hw %lld must be positive and within 32 bits", name, (long long)hw);
    MPN_CHECK_ARG(eps >= 0.f && isfinite(eps), "%s: eps %g", name, (double)eps);
    int64_t c = 0;
    MPN_TRY(check_segments(name, seg_data, seg_stride, seg_channels, n_segments, hw, segs, &c));
    MPN_CHECK_ARG(grad_out != nullptr, "%s: null grad_out", name);
    MPN_CHECK_ARG(grad_in != nullptr || grad_weight != nullptr || grad_bias != nullptr, "%s: no output wanted (all three are null)", name);
    MPN_CHECK_ARG(weight != nullptr || (grad_weight == nullptr && grad_bias == nullptr),
                  "%s: grad_weight / grad_bias without a weight (no affine: grad_in only)", name);
    MPN_CHECK_ARG(grad_out_stride >= 0 && grad_out_stride <= INT32_MAX, "%s: grad_out_stride %lld outside the 32-bit range", name,
                  (long long)grad_out_stride);
    MPN_CHECK_ARG(n_images <= INT32_MAX && ln_bwd_splits(n_images) <= 65535, "%s: %lld images are more than one launch holds", name,
                  (long long)n_images);
    *feat = c * hw;
    return MPNHIP_OK;
}

}  // namespace
}  // namespace mpnhip

extern "C" size_t mpnhip_layer_norm_backward_workspace_bytes(const float* const* seg_data, const int64_t* seg_stride,
                                                             const int* seg_channels, int n_segments, int64_t n_images, int64_t hw,
                                                             const float* weight, float eps, const float* grad_out,
                                                             int64_t grad_out_stride, float* grad_in, float* grad_weight,
                                                             float* grad_bias) {
    ConvSegs segs;
    int64_t feat = 0;
    if (ln_bwd_check("mpnhip_layer_norm_backward_workspace_bytes", seg_data, seg_stride, seg_channels, n_segments, n_images, hw, weight, eps,
                     grad_out, grad_out_stride, grad_in, grad_weight, grad_bias, &segs, &feat) != MPNHIP_OK)
        return 0;
    if (n_images == 0) return 0;
    LnBwdWs ws;
    return ln_bwd_layout(n_images, feat, weight != nullptr, nullptr, &ws);
}

extern "C" int mpnhip_layer_norm_backward(const float* const* seg_data, const int64_t* seg_stride, const int* seg_channels,
                                          int n_segments, int64_t n_images, int64_t hw, const float* weight, float eps,
                                          const float* grad_out, int64_t grad_out_stride, float* grad_in, float* grad_weight,
                                          float* grad_bias, void* workspace, size_t workspace_bytes, void* stream_) {
    static const char* const name = "mpnhip_layer_norm_backward";
    hipStream_t stream = (hipStream_t)stream_;
    ConvSegs segs;
    int64_t feat64 = 0;
    MPN_TRY(ln_bwd_check(name, seg_data, seg_stride, seg_channels, n_segments, n_images, hw, weight, eps, grad_out, grad_out_stride, grad_in,
                         grad_weight, grad_bias, &segs, &feat64));
    const int feat = (int)feat64;
    if (n_images == 0) {
        if (grad_weight) MPN_HIP(hipMemsetAsync(grad_weight, 0, sizeof(float) * feat, stream));
        if (grad_bias) MPN_HIP(hipMemsetAsync(grad_bias, 0, sizeof(float) * feat, stream));
        return MPNHIP_OK;
    }
    LnBwdWs ws;
    const size_t need = ln_bwd_layout(n_images, feat, weight != nullptr, nullptr, &ws);
    MPN_CHECK_ARG(workspace != nullptr && workspace_bytes >= need, "%s: workspace %zu < %zu", name, workspace ? workspace_bytes : (size_t)0,
                  need);
    ln_bwd_layout(n_images, feat, weight != nullptr, workspace, &ws);
    count_path(PC_LAYER_NORM_BWD);

    if (grad_in || grad_weight)     // (the bias gradient alone needs no statistics)
        layer_norm_bwd_image_kernel<<<(unsigned)n_images, LN_THREADS, 0, stream>>>(segs, (int)hw, feat, weight, eps, grad_out,
                                                                                   grad_out_stride, grad_in, ws.stats);
    if (grad_weight || grad_bias) {
        const int splits = (int)ln_bwd_splits(n_images);
        const unsigned bx = (unsigned)((feat + LNB_THREADS - 1) / LNB_THREADS);
        layer_norm_bwd_affine_kernel<<<dim3(bx, (unsigned)splits), LNB_THREADS, 0, stream>>>(
            segs, (int)hw, feat, grad_out, grad_out_stride, ws.stats, n_images, grad_weight ? ws.w_partial : nullptr,
            grad_bias ? ws.b_partial : nullptr);
        layer_norm_bwd_sum_kernel<<<bx, LNB_THREADS, 0, stream>>>(ws.w_partial, ws.b_partial, splits, feat, grad_weight, grad_bias);
    }
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}
