// The inputs of the two embedding CNNs (reference data/seq_processing/seq_processor.py:395-562, _store_embeddings):
//   ReID patches    utils/rgb.py:40-69     crop, np.pad(mode='mean'), PIL resize (bilinear), ToTensor, Normalize
//   node_ext        tracktor-mots/src/tracktor_masked/maskrcnn_fpn.py:108-115   MultiScaleRoIAlign over the four FPN levels
// The CNNs themselves are stock modules.  Patches: the padded crop is never materialised -- after one pass over the crop for its
// column and row means it is a function of (y, x) -- and the two resampling passes of a band of output rows meet in LDS: a block
// owns a box and a band, runs the horizontal pass over the input rows the band's vertical taps reach into LDS as uint8, and the
// vertical pass from there.  RoIAlign: the sample table of a box (S * grid positions per axis) is built once per block in LDS
// and shared by all channels; a block writes one contiguous range of the box's [C, S, S] output.
// Contraction is off for the whole file: an FMA in a resampling coefficient moves its fixed-point rounding, one in a sample
// position a tap.
#pragma clang fp contract(off)

#include "common.h"

namespace mpnhip {
namespace {

constexpr int CROP_THREADS = 256, CROP_WAVES = CROP_THREADS / 64;
constexpr int CROP_MAX_BAND = 8;              // output rows per block at most
constexpr int CROP_LDS_BYTES = 60 * 1024;     // of the horizontal result one block keeps
constexpr int PRECISION_BITS = 22;            // Pillow's, 8 bits per channel
constexpr int FPN_THREADS = 256, FPN_CHANNELS = 16;   // threads = output positions at a time; channels per block

// ------------------------------------------------------------------------------------------------ patches: geometry
// A box as the host describes it (geom [n, 8]: y0, y1, x0, x1 = the crop's rows and columns in the frame; pt, pb, pl, pr = the
// pads), checked against the frame and the launch's largest padded sides before anything is indexed with it.
struct CropBox { int f, y0, x0, ch, cw, pt, pl, ph, pw; bool ok, padded; };
__device__ __forceinline__ CropBox crop_box(const int32_t* __restrict__ geom, const int32_t* __restrict__ box_frame, int64_t k, int n_frames,
                                            int H, int W, int max_ph, int max_pw) {
    const int32_t* __restrict__ g = geom + k * 8;
    const int y0 = g[0], y1 = g[1], x0 = g[2], x1 = g[3], pt = g[4], pb = g[5], pl = g[6], pr = g[7];
    CropBox b = {box_frame[k], y0, x0, 0, 0, pt, pl, 0, 0, false, false};
    const int M = MPNHIP_CROP_MAX_SIDE;
    if (b.f < 0 || b.f >= n_frames || y0 < 0 || y1 <= y0 || y1 > H || x0 < 0 || x1 <= x0 || x1 > W) return b;
    if (pt < 0 || pt > M || pb < 0 || pb > M || pl < 0 || pl > M || pr < 0 || pr > M || y1 - y0 > M || x1 - x0 > M) return b;
    b.ch = y1 - y0;
    b.cw = x1 - x0;
    b.ph = pt + b.ch + pb;
    b.pw = pl + b.cw + pr;
    b.padded = (pt | pb | pl | pr) != 0;
    b.ok = b.ph <= max_ph && b.pw <= max_pw;
    return b;
}

// taps of one output index at most: Pillow's ksize for the bilinear filter (support 1)
__host__ __device__ inline int resample_taps(int in_size, int out_size) {
    const double scale = (double)in_size / (double)out_size;
    const double support = scale < 1.0 ? 1.0 : scale;
    return (int)ceil(support) * 2 + 1;
}

// The workspace of one launch: per box the fixed-point coefficients of both passes (hcoef [ow][ksh], vcoef [oh][ksv]) with their
// bounds ((first input index, taps) per output index) and the means of np.pad: per crop column, per crop row, and of the padded
// rows over the crop's columns.  One layout for the size query and the operator.
struct CropPlan {
    int ksh, ksv;
    int32_t *hcoef, *hbound, *vcoef, *vbound;
    unsigned char *colmean, *rowmean, *corner;
    size_t mean_stride_w, mean_stride_h, total;
};
CropPlan plan_crops(int64_t n, int max_ph, int max_pw, int oh, int ow, void* base) {
    Carver a(base);
    CropPlan p = {};
    const size_t nn = (size_t)(n > 0 ? n : 0);
    p.ksh = resample_taps(max_pw, ow);
    p.ksv = resample_taps(max_ph, oh);
    p.hcoef = a.take<int32_t>(nn * ow * p.ksh);
    p.hbound = a.take<int32_t>(nn * ow * 2);
    p.vcoef = a.take<int32_t>(nn * oh * p.ksv);
    p.vbound = a.take<int32_t>(nn * oh * 2);
    p.mean_stride_w = (size_t)max_pw * 3;
    p.mean_stride_h = (size_t)max_ph * 3;
    p.colmean = a.take<unsigned char>(nn * p.mean_stride_w);
    p.rowmean = a.take<unsigned char>(nn * p.mean_stride_h);
    p.corner = a.take<unsigned char>(nn * 4);
    p.total = a.bytes();
    return p;
}

// rows of the horizontal result a band of `band` output rows reaches at most, for any box of the launch: its first tap lies at
// center(r0) - support - 0.5 or above, its last below center(r0 + band - 1) + support + 0.5, support = max(scale, 1), and the
// scale of a box is at most max_ph / oh
int band_rows_bound(int band, int max_ph, int oh) {
    const double s = (double)max_ph / (double)oh, support = s < 1.0 ? 1.0 : s;
    return (int)ceil((band - 1) * s + 2.0 * support) + 3;
}

struct Norm { float mean[3], std[3]; };

// ------------------------------------------------------------------------------------------------ patches: coefficients
// Pillow's precompute_coeffs and normalize_coeffs_8bpc (src/libImaging/Resample.c) for the bilinear filter in float64, one
// thread per (box, output index of either pass).  A pass whose size does not change is skipped by Pillow: one tap of 2^22.
__global__ void k_crop_coeffs(const int32_t* __restrict__ geom, const int32_t* __restrict__ box_frame, int64_t n, int n_frames, int H, int W,
                              int max_ph, int max_pw, int oh, int ow, int ksh, int ksv, int32_t* __restrict__ hcoef,
                              int32_t* __restrict__ hbound, int32_t* __restrict__ vcoef, int32_t* __restrict__ vbound) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int per_box = ow + oh;
    if (i >= n * per_box) return;
    const int64_t k = i / per_box;
    const int j = (int)(i - k * per_box);
    const bool vertical = j >= ow;
    const int xx = vertical ? j - ow : j;
    const CropBox b = crop_box(geom, box_frame, k, n_frames, H, W, max_ph, max_pw);
    const int in_size = vertical ? b.ph : b.pw, out_size = vertical ? oh : ow, ks = vertical ? ksv : ksh;
    int32_t* __restrict__ coef = vertical ? vcoef + (k * oh + xx) * ksv : hcoef + (k * ow + xx) * ksh;
    int32_t* __restrict__ bound = vertical ? vbound + (k * oh + xx) * 2 : hbound + (k * ow + xx) * 2;
    if (!b.ok) { bound[0] = 0; bound[1] = 0; return; }
    if (in_size == out_size) {
        bound[0] = xx;
        bound[1] = 1;
        coef[0] = 1 << PRECISION_BITS;
        return;
    }
    const double scale = (double)in_size / (double)out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = filterscale;   // (bilinear: 1.0 * filterscale)
    const double center = ((double)xx + 0.5) * scale;
    const double ss = 1.0 / filterscale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    int count = xmax - xmin;
    count = count < 0 ? 0 : (count > ks ? ks : count);   // (never more than ks: ksize is Pillow's own bound)
    auto weight = [&](int x) {
        double v = ((double)(x + xmin) - center + 0.5) * ss;
        if (v < 0.0) v = -v;
        return v < 1.0 ? 1.0 - v : 0.0;
    };
    double ww = 0.0;
    for (int x = 0; x < count; ++x) ww += weight(x);
    for (int x = 0; x < count; ++x) {
        double w = weight(x);
        if (ww != 0.0) w /= ww;
        coef[x] = (int)(0.5 + w * (double)(1 << PRECISION_BITS));
    }
    bound[0] = xmin;
    bound[1] = count;
}

// ------------------------------------------------------------------------------------------------ patches: means
// round(total / count) half to even: numpy's mean of uint8 (an exact sum over the count, in float64) and its round()
__device__ __forceinline__ unsigned char mean_u8(unsigned total, unsigned count) {
    const unsigned q = total / count, r = total - q * count;
    return (unsigned char)(q + ((2 * r > count || (2 * r == count && (q & 1))) ? 1 : 0));
}

// np.pad(mode='mean') over axis 0, then axis 1: one block per box with a pad.  Column means over the crop's rows (threads over
// the 3 cw bytes of a row), row means over the crop's columns (a wavefront per row), and the mean of the padded rows -- which
// hold the column means -- over the crop's columns.
__global__ __launch_bounds__(CROP_THREADS) void k_crop_means(const unsigned char* __restrict__ frames, const int32_t* __restrict__ geom,
                                                             const int32_t* __restrict__ box_frame, int n_frames, int H, int W, int max_ph,
                                                             int max_pw, unsigned char* __restrict__ colmean, unsigned char* __restrict__ rowmean,
                                                             unsigned char* __restrict__ corner) {
    const int64_t k = blockIdx.x;
    const CropBox b = crop_box(geom, box_frame, k, n_frames, H, W, max_ph, max_pw);
    if (!b.ok || !b.padded) return;   // (block-uniform)
    const int64_t pitch = (int64_t)W * 3;
    const unsigned char* __restrict__ src = frames + ((int64_t)b.f * H + b.y0) * pitch + (int64_t)b.x0 * 3;
    unsigned char* cm = colmean + k * ((int64_t)max_pw * 3);   // (read back below: no restrict)
    unsigned char* __restrict__ rm = rowmean + k * ((int64_t)max_ph * 3);
    const int row_bytes = b.cw * 3;   // (<= 3 max_pw)
    for (int j = threadIdx.x; j < row_bytes; j += CROP_THREADS) {
        unsigned s = 0;
        for (int y = 0; y < b.ch; ++y) s += src[y * pitch + j];
        cm[j] = mean_u8(s, (unsigned)b.ch);
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    auto row_mean = [&](const unsigned char* row, unsigned char* dst) {   // (wave-uniform call)
        unsigned s[3] = {0, 0, 0};
        for (int j = lane; j < row_bytes; j += 64) {
            const unsigned v = row[j];
            const int c = j % 3;
            s[0] += c == 0 ? v : 0;
            s[1] += c == 1 ? v : 0;
            s[2] += c == 2 ? v : 0;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s[c] += __shfl_xor(s[c], o);
        }
        if (lane < 3) dst[lane] = mean_u8(lane == 0 ? s[0] : (lane == 1 ? s[1] : s[2]), (unsigned)b.cw);
    };
    for (int y = wave; y < b.ch; y += CROP_WAVES) row_mean(src + y * pitch, rm + y * 3);
    __syncthreads();   // (the column means of this block's own threads)
    if (wave == 0) row_mean(cm, corner + k * 4);
}

// ------------------------------------------------------------------------------------------------ patches: resize + normalise
// One block per (box, band of output rows).  Phase 1: the horizontal pass of the rows [ylo, yhi) the band's vertical taps reach,
// into LDS as uint8 [row][xo][c]; a pixel of the padded crop is the frame's inside the crop, the row mean beside it, the column
// mean above and below it and the padded rows' mean in the corners.  Phase 2: the vertical pass, ToTensor and Normalize; the
// float stores of a block are whole output rows.
__global__ __launch_bounds__(CROP_THREADS) void k_crop_resize(const unsigned char* __restrict__ frames, const int32_t* __restrict__ geom,
                                                              const int32_t* __restrict__ box_frame, int n_frames, int H, int W, int max_ph,
                                                              int max_pw, int oh, int ow, int band, int bands, int lds_bytes, CropPlan p,
                                                              Norm norm, float* __restrict__ out, unsigned char* __restrict__ out_u8) {
    extern __shared__ unsigned char hres[];
    const int64_t k = blockIdx.x / bands;
    const int r0 = (int)(blockIdx.x % bands) * band, r1 = r0 + band < oh ? r0 + band : oh;
    const CropBox b = crop_box(geom, box_frame, k, n_frames, H, W, max_ph, max_pw);
    const int32_t* __restrict__ vb = p.vbound + k * oh * 2;
    const int32_t* __restrict__ hb = p.hbound + k * ow * 2;
    const int ylo = vb[r0 * 2], yhi = vb[(r1 - 1) * 2] + vb[(r1 - 1) * 2 + 1], nrows = yhi - ylo;
    const int row_items = ow * 3, out_items = (r1 - r0) * row_items;
    float* __restrict__ out_k = out + k * ((int64_t)3 * oh * ow);
    unsigned char* __restrict__ u8_k = out_u8 ? out_u8 + k * ((int64_t)oh * ow * 3) : nullptr;
    if (!b.ok || ylo < 0 || nrows <= 0 || yhi > b.ph || (int64_t)nrows * row_items > lds_bytes) {   // (block-uniform) a refused box: zeros
        for (int i = threadIdx.x; i < out_items; i += CROP_THREADS) {
            const int c = i / ((r1 - r0) * ow), rest = i - c * ((r1 - r0) * ow), r = r0 + rest / ow, xo = rest - (r - r0) * ow;
            out_k[((int64_t)c * oh + r) * ow + xo] = 0.f;
            if (u8_k) u8_k[((int64_t)r * ow + xo) * 3 + c] = 0;
        }
        return;
    }
    const int64_t pitch = (int64_t)W * 3;
    const unsigned char* __restrict__ src = frames + ((int64_t)b.f * H + b.y0) * pitch + (int64_t)b.x0 * 3;
    const unsigned char* __restrict__ cm = p.colmean + k * (int64_t)p.mean_stride_w;
    const unsigned char* __restrict__ rm = p.rowmean + k * (int64_t)p.mean_stride_h;
    const unsigned char* __restrict__ cn = p.corner + k * 4;
    const int32_t* __restrict__ hc = p.hcoef + k * ow * p.ksh;
    for (int i = threadIdx.x; i < nrows * row_items; i += CROP_THREADS) {
        const int row = i / row_items, rest = i - row * row_items, xo = rest / 3, c = rest - xo * 3;
        const int cy = ylo + row - b.pt;
        const bool in_y = cy >= 0 && cy < b.ch;
        const unsigned char* __restrict__ line = in_y ? src + cy * pitch + c : cm + c;       // inside the crop's columns
        const int beside = in_y ? rm[cy * 3 + c] : cn[c];                                    // left and right of them
        const int xmin = hb[xo * 2], count = hb[xo * 2 + 1];
        const int32_t* __restrict__ coef = hc + xo * p.ksh;
        int acc = 1 << (PRECISION_BITS - 1);
        for (int t = 0; t < count; ++t) {
            const int cx = xmin + t - b.pl;
            const int v = (cx >= 0 && cx < b.cw) ? line[cx * 3] : beside;
            acc += coef[t] * v;
        }
        acc >>= PRECISION_BITS;
        hres[i] = (unsigned char)(acc < 0 ? 0 : (acc > 255 ? 255 : acc));
    }
    __syncthreads();
    const int32_t* __restrict__ vc = p.vcoef + k * oh * p.ksv;
    for (int i = threadIdx.x; i < out_items; i += CROP_THREADS) {
        const int c = i / ((r1 - r0) * ow), rest = i - c * ((r1 - r0) * ow), r = r0 + rest / ow, xo = rest - (r - r0) * ow;
        const int ymin = vb[r * 2] - ylo, count = vb[r * 2 + 1];
        const int32_t* __restrict__ coef = vc + r * p.ksv;
        int acc = 1 << (PRECISION_BITS - 1);
        for (int t = 0; t < count; ++t) {
            int row = ymin + t;
            row = row < 0 ? 0 : (row >= nrows ? nrows - 1 : row);   // (inside [0, nrows) already: the bounds ascend with r)
            acc += coef[t] * hres[(row * ow + xo) * 3 + c];
        }
        acc >>= PRECISION_BITS;
        const int v = acc < 0 ? 0 : (acc > 255 ? 255 : acc);
        out_k[((int64_t)c * oh + r) * ow + xo] = ((float)v / 255.f - norm.mean[c]) / norm.std[c];
        if (u8_k) u8_k[((int64_t)r * ow + xo) * 3 + c] = (unsigned char)v;
    }
}

// ------------------------------------------------------------------------------------------------ FPN RoIAlign
// One block per (box, FPN_CHANNELS output channels of its [C (+ 1), S, S] block), one thread per output position (py, px).  The
// sample table -- per axis S * grid positions: low, high, l, h (torchvision's pre_calc_for_bilinear_interpolate; a sample outside
// [-1, size] has all four 0, so it adds + 0 like torchvision's) -- is built once per block in LDS.  G > 0: the grid is a
// compile-time constant and a thread keeps the 4 G^2 offsets and weights of its position in registers over its channels, so a
// channel costs 4 G^2 loads, as many products and sums, and one store; the 64 stores of a wavefront are consecutive floats of one
// channel.  G = 0: any grid, the table is read again for every channel.  (Copying the box's footprint into LDS first and reading
// the taps there was tried and took the same time: what a box costs is fetching its short row segments from 256 planes.)
template <int G>
__device__ __forceinline__ float roi_sum(const float* __restrict__ base, const int (&off)[G * G][4], const float (&w)[G * G][4]) {
    float sum = 0.f;
#pragma unroll
    for (int s = 0; s < G * G; ++s)
        sum += ((w[s][0] * base[off[s][0]] + w[s][1] * base[off[s][1]]) + w[s][2] * base[off[s][2]]) + w[s][3] * base[off[s][3]];
    return sum;
}

template <int G>
__global__ __launch_bounds__(FPN_THREADS) void k_fpn_roi_align(mpnhip_fpn_levels lv, int n_frames, int channels, const float* __restrict__ boxes,
                                                               const int32_t* __restrict__ box_frame, const int32_t* __restrict__ box_level,
                                                               int S, int grid_rt, const int32_t* __restrict__ detection_id,
                                                               int blocks_per_box, float* __restrict__ out) {
    extern __shared__ int table[];
    const int grid = G > 0 ? G : grid_rt;
    const int SG = S * grid;
    int* __restrict__ t_low = table;                 // [2][SG]: axis 0 = x, 1 = y
    int* __restrict__ t_high = table + 2 * SG;
    float* __restrict__ t_l = reinterpret_cast<float*>(table + 4 * SG);
    float* __restrict__ t_h = reinterpret_cast<float*>(table + 6 * SG);
    const int64_t k = blockIdx.x / blocks_per_box;
    const int chunk = blockIdx.x % blocks_per_box;
    const int f = box_frame[k], level = box_level[k];
    const bool ok = f >= 0 && f < n_frames && level >= 0 && level < MPNHIP_FPN_LEVELS;   // (block-uniform)
    const int lvl = ok ? level : 0;
    const int fh = lv.h[lvl], fw = lv.w[lvl];
    const float scale = lv.scale[lvl];
    for (int i = threadIdx.x; i < 2 * SG; i += FPN_THREADS) {
        const int axis = i >= SG ? 1 : 0, j = i - axis * SG, pi = j / grid, gi = j - pi * grid;
        const float v1 = boxes[k * 4 + axis], v2 = boxes[k * 4 + 2 + axis];
        const int size = axis ? fh : fw;
        const float start = v1 * scale;
        float extent = v2 * scale - start;
        extent = extent < 1.f ? 1.f : extent;   // std::max(extent, 1.f); a NaN extent leaves NaN positions: outside
        const float bin = extent / (float)S;
        float v = (start + (float)pi * bin) + (((float)gi + .5f) * bin) / (float)grid;
        int low = 0, high = 0;
        float l = 0.f, h = 0.f;
        if (ok && !(v < -1.0f || v > (float)size || v != v)) {
            if (v <= 0.f) v = 0.f;
            low = (int)v;
            if (low >= size - 1) {
                high = low = size - 1;
                v = (float)low;
            } else {
                high = low + 1;
            }
            l = v - (float)low;
            h = (float)(1.0 - (double)l);   // (T hy = 1. - ly: the subtraction is a double's)
        }
        t_low[i] = low;
        t_high[i] = high;
        t_l[i] = l;
        t_h[i] = h;
    }
    __syncthreads();
    const int SS = S * S, has_id = detection_id ? 1 : 0;
    const int c_total = channels + has_id;
    const int c_begin = chunk * FPN_CHANNELS, c_end = c_begin + FPN_CHANNELS < c_total ? c_begin + FPN_CHANNELS : c_total;
    float* __restrict__ out_k = out + k * ((int64_t)c_total * SS);
    const float id = has_id ? (float)detection_id[k] : 0.f;
    const float count = (float)(grid * grid);
    const int64_t plane_size = (int64_t)fh * fw;
    // (a box whose frame or level is outside reads frame 0 of level 0 through an all-zero table: zeros)
    const float* __restrict__ feat = lv.data[lvl] + (int64_t)(ok ? f : 0) * channels * plane_size;
    for (int pp = threadIdx.x; pp < SS; pp += FPN_THREADS) {
        const int py = pp / S, px = pp - py * S;
        if constexpr (G > 0) {
            int off[G * G][4];
            float w[G * G][4];
#pragma unroll
            for (int iy = 0; iy < G; ++iy) {
                const int yi = SG + py * G + iy;
                const int ylow = t_low[yi] * fw, yhigh = t_high[yi] * fw;
                const float ly = t_l[yi], hy = t_h[yi];
#pragma unroll
                for (int ix = 0; ix < G; ++ix) {
                    const int xi = px * G + ix, s = iy * G + ix;
                    const int xlow = t_low[xi], xhigh = t_high[xi];
                    const float lx = t_l[xi], hx = t_h[xi];
                    off[s][0] = ylow + xlow; off[s][1] = ylow + xhigh; off[s][2] = yhigh + xlow; off[s][3] = yhigh + xhigh;
                    w[s][0] = hy * hx; w[s][1] = hy * lx; w[s][2] = ly * hx; w[s][3] = ly * lx;
                }
            }
            for (int c = c_begin; c < c_end; ++c) {
                if (c < has_id) { out_k[(int64_t)c * SS + pp] = id; continue; }
                out_k[(int64_t)c * SS + pp] = roi_sum<G>(feat + (int64_t)(c - has_id) * plane_size, off, w) / count;
            }
        } else {
            for (int c = c_begin; c < c_end; ++c) {
                if (c < has_id) { out_k[(int64_t)c * SS + pp] = id; continue; }
                const float* __restrict__ plane = feat + (int64_t)(c - has_id) * plane_size;
                float sum = 0.f;
                for (int iy = 0; iy < grid; ++iy) {
                    const int yi = SG + py * grid + iy;
                    const int ylow = t_low[yi] * fw, yhigh = t_high[yi] * fw;
                    const float ly = t_l[yi], hy = t_h[yi];
                    for (int ix = 0; ix < grid; ++ix) {
                        const int xi = px * grid + ix;
                        const int xlow = t_low[xi], xhigh = t_high[xi];
                        const float lx = t_l[xi], hx = t_h[xi];
                        const float w1 = hy * hx, w2 = hy * lx, w3 = ly * hx, w4 = ly * lx;
                        sum += ((w1 * plane[ylow + xlow] + w2 * plane[ylow + xhigh]) + w3 * plane[yhigh + xlow]) + w4 * plane[yhigh + xhigh];
                    }
                }
                out_k[(int64_t)c * SS + pp] = sum / count;
            }
        }
    }
}

static bool crop_sizes_ok(int64_t n, int max_ph, int max_pw, int oh, int ow) {
    const int M = MPNHIP_CROP_MAX_SIDE;
    return n >= 0 && n < (1LL << 24) && max_ph >= 1 && max_ph <= M && max_pw >= 1 && max_pw <= M && oh >= 1 && oh <= M && ow >= 1 && ow <= M;
}

// the band of output rows a block takes: the largest up to CROP_MAX_BAND whose horizontal result fits; 0: not even one row does
static int crop_band(int max_ph, int oh, int ow, int* lds_bytes) {
    for (int band = oh < CROP_MAX_BAND ? oh : CROP_MAX_BAND; band >= 1; --band) {
        const int64_t bytes = (int64_t)band_rows_bound(band, max_ph, oh) * ow * 3;
        if (bytes <= CROP_LDS_BYTES) {
            *lds_bytes = (int)align_up((size_t)bytes, 16);
            return band;
        }
    }
    return 0;
}

}  // namespace
}  // namespace mpnhip

using namespace mpnhip;

extern "C" size_t mpnhip_reid_crops_workspace_bytes(int64_t n, int max_ph, int max_pw, int oh, int ow) {
    if (!crop_sizes_ok(n, max_ph, max_pw, oh, ow)) return 0;
    return plan_crops(n, max_ph, max_pw, oh, ow, nullptr).total;
}

extern "C" int mpnhip_reid_crops(const unsigned char* frames, int64_t n_frames, int H, int W, const int32_t* geom, const int32_t* box_frame,
                                 int64_t n, int max_ph, int max_pw, int oh, int ow, const float* mean_std, float* out, unsigned char* out_u8,
                                 void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(crop_sizes_ok(n, max_ph, max_pw, oh, ow),
                  "reid_crops: bad sizes (fewer than 2^24 boxes per call, output and padded sides in [1, %d])", MPNHIP_CROP_MAX_SIDE);
    MPN_CHECK_ARG(n_frames >= 0 && n_frames < (1LL << 31) && H >= 0 && W >= 0 && (int64_t)H * W < (1LL << 31) / 3 &&
                  n_frames * ((int64_t)H * W * 3) < (1LL << 46), "reid_crops: bad frame sizes (3 H W must stay below 2^31)");
    MPN_CHECK_ARG(mean_std, "reid_crops: null mean_std");
    for (int c = 0; c < 3; ++c)
        MPN_CHECK_ARG(mean_std[c] - mean_std[c] == 0.f && mean_std[3 + c] - mean_std[3 + c] == 0.f && mean_std[3 + c] != 0.f,
                      "reid_crops: mean and std must be finite, std not 0");
    if (n == 0) return MPNHIP_OK;
    MPN_CHECK_ARG(frames && n_frames > 0 && H > 0 && W > 0, "reid_crops: boxes without frames");
    MPN_CHECK_ARG(geom && box_frame && out, "reid_crops: null geom, box_frame or out");
    int lds_bytes = 0;
    const int band = crop_band(max_ph, oh, ow, &lds_bytes);
    if (band == 0) {
        set_error("reid_crops: one output row of %d pixels from crops of up to %d rows does not fit the block's %d bytes of LDS", ow, max_ph,
                  CROP_LDS_BYTES);
        return MPNHIP_ERR_UNSUPPORTED;
    }
    const CropPlan p = plan_crops(n, max_ph, max_pw, oh, ow, workspace);
    MPN_CHECK_WORKSPACE("reid_crops", workspace, workspace_bytes, p.total);
    const int bands = (oh + band - 1) / band;
    MPN_CHECK_ARG(n * bands < (1LL << 31), "reid_crops: too many blocks: fewer boxes per call");
    Norm norm;
    for (int c = 0; c < 3; ++c) { norm.mean[c] = mean_std[c]; norm.std[c] = mean_std[3 + c]; }
    hipLaunchKernelGGL(k_crop_coeffs, dim3(blocks_for(n * (ow + oh))), dim3(256), 0, stream, geom, box_frame, n, (int)n_frames, H, W, max_ph,
                       max_pw, oh, ow, p.ksh, p.ksv, p.hcoef, p.hbound, p.vcoef, p.vbound);
    MPN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_crop_means, dim3((unsigned)n), dim3(CROP_THREADS), 0, stream, frames, geom, box_frame, (int)n_frames, H, W, max_ph,
                       max_pw, p.colmean, p.rowmean, p.corner);
    MPN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_crop_resize, dim3((unsigned)(n * bands)), dim3(CROP_THREADS), (size_t)lds_bytes, stream, frames, geom, box_frame,
                       (int)n_frames, H, W, max_ph, max_pw, oh, ow, band, bands, lds_bytes, p, norm, out, out_u8);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}

extern "C" int mpnhip_fpn_roi_align(const mpnhip_fpn_levels* levels, int64_t n_frames, int channels, const float* boxes,
                                    const int32_t* box_frame, const int32_t* box_level, int64_t n, int output_size, int sampling_ratio,
                                    const int32_t* detection_id, float* out, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(levels, "fpn_roi_align: null levels");
    MPN_CHECK_ARG(n >= 0 && n < (1LL << 24) && n_frames >= 0 && n_frames < (1LL << 31) && channels >= 1 && channels < (1 << 20),
                  "fpn_roi_align: bad sizes (fewer than 2^24 boxes per call)");
    MPN_CHECK_ARG(output_size >= 1 && sampling_ratio >= 1 && (int64_t)output_size * sampling_ratio <= MPNHIP_FPN_MAX_SAMPLES,
                  "fpn_roi_align: output_size and sampling_ratio must be positive, their product at most %d", MPNHIP_FPN_MAX_SAMPLES);
    const int64_t total = ((int64_t)channels + 1) * output_size * output_size;
    MPN_CHECK_ARG(total < (1LL << 31), "fpn_roi_align: (channels + 1) x output_size^2 must stay below 2^31");
    const mpnhip_fpn_levels lv = *levels;
    for (int l = 0; l < MPNHIP_FPN_LEVELS; ++l)
        MPN_CHECK_ARG(lv.h[l] >= 1 && lv.w[l] >= 1 && (int64_t)lv.h[l] * lv.w[l] < (1LL << 31) && lv.scale[l] > 0.f &&
                      lv.scale[l] - lv.scale[l] == 0.f, "fpn_roi_align: level %d: bad shape or scale", l);
    if (n == 0) return MPNHIP_OK;
    MPN_CHECK_ARG(n_frames > 0 && boxes && box_frame && box_level && out, "fpn_roi_align: boxes without frames / null boxes, box_frame, box_level or out");
    for (int l = 0; l < MPNHIP_FPN_LEVELS; ++l) MPN_CHECK_ARG(lv.data[l], "fpn_roi_align: level %d: null features", l);
    const int c_total = channels + (detection_id ? 1 : 0);
    const int blocks_per_box = (c_total + FPN_CHANNELS - 1) / FPN_CHANNELS;
    MPN_CHECK_ARG(n * blocks_per_box < (1LL << 31), "fpn_roi_align: too many blocks: fewer boxes per call");
    const size_t lds = (size_t)8 * output_size * sampling_ratio * sizeof(int);
    const dim3 blocks((unsigned)(n * blocks_per_box)), threads(FPN_THREADS);
    if (sampling_ratio == 2)   // (the reference's)
        hipLaunchKernelGGL(k_fpn_roi_align<2>, blocks, threads, lds, stream, lv, (int)n_frames, channels, boxes, box_frame, box_level, output_size,
                           sampling_ratio, detection_id, blocks_per_box, out);
    else
        hipLaunchKernelGGL(k_fpn_roi_align<0>, blocks, threads, lds, stream, lv, (int)n_frames, channels, boxes, box_frame, box_level, output_size,
                           sampling_ratio, detection_id, blocks_per_box, out);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}
