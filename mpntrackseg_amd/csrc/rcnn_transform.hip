// The image transform in front of the Mask R-CNN FPN backbone (include/mpnhip.h: mpnhip_rcnn_transform):
// GeneralizedRCNNTransform.forward for a batch of equally sized uint8 frames in one launch -- ToTensor, Normalize, the bilinear
// resize (align_corners=False, no antialiasing, the scale taken from the output size) and the zero padding of the batch.
//
// One thread per output pixel (image, y, x) of the padded [Hp][Wp] plane, x fastest: the two source rows, the two source columns
// and their weights are computed once and serve the three channels; the stores of a wave are 256 contiguous bytes per channel.
// ToTensor and Normalize have 256 possible results per channel: a block computes the 768 of them once into LDS, in the reference's
// float32 operations, and a tap is one LDS read.  Every float operation is an explicitly rounded one (no contraction into FMAs),
// so the bits are those of the arithmetic the header states.
#include "common.h"

#include <math.h>

namespace mpnhip {
namespace {

constexpr int RT_THREADS = 256;

struct RcnnNorm {
    float mean[3], std[3];
};

// aten's area_pixel_compute_source_index + guard_index_and_lambda for align_corners=False, in float32
__device__ __forceinline__ void bilinear_axis(int dst, float scale, int in, int* i0, int* i1, float* l0, float* l1) {
    float src = __fsub_rn(__fmul_rn(scale, __fadd_rn((float)dst, 0.5f)), 0.5f);
    src = src < 0.f ? 0.f : src;
    const int i = min((int)src, in - 1);
    *i0 = i;
    *i1 = i + (i < in - 1 ? 1 : 0);
    const float l = fminf(fmaxf(__fsub_rn(src, (float)i), 0.f), 1.f);
    *l1 = l;
    *l0 = __fsub_rn(1.f, l);
}

__global__ __launch_bounds__(RT_THREADS) void rcnn_transform_kernel(const unsigned char* __restrict__ frames, int H, int W, int oh, int ow,
                                                                    int Hp, int Wp, float scale_y, float scale_x, RcnnNorm norm,
                                                                    float* __restrict__ out, int64_t total) {
    __shared__ float lut[3][256];
    for (int e = threadIdx.x; e < 3 * 256; e += RT_THREADS) {
        const int c = e >> 8, v = e & 255;
        lut[c][v] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)v, 255.f), norm.mean[c]), norm.std[c]);
    }
    __syncthreads();
    const int64_t idx = (int64_t)blockIdx.x * RT_THREADS + threadIdx.x;
    if (idx >= total) return;
    const int plane = Hp * Wp;
    const int64_t img = idx / plane;
    const int pix = (int)(idx % plane), y = pix / Wp, x = pix % Wp;
    float* __restrict__ o = out + img * 3 * (int64_t)plane + pix;
    if (y >= oh || x >= ow) {                     // the batch padding
        o[0] = 0.f, o[plane] = 0.f, o[2 * plane] = 0.f;
        return;
    }
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    bilinear_axis(y, scale_y, H, &y0, &y1, &ly0, &ly1);
    bilinear_axis(x, scale_x, W, &x0, &x1, &lx0, &lx1);
    const unsigned char* __restrict__ f = frames + img * 3 * (int64_t)H * W;
    const unsigned char* __restrict__ p00 = f + (y0 * W + x0) * 3;
    const unsigned char* __restrict__ p01 = f + (y0 * W + x1) * 3;
    const unsigned char* __restrict__ p10 = f + (y1 * W + x0) * 3;
    const unsigned char* __restrict__ p11 = f + (y1 * W + x1) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float top = __fadd_rn(__fmul_rn(lx0, lut[c][p00[c]]), __fmul_rn(lx1, lut[c][p01[c]]));
        const float bot = __fadd_rn(__fmul_rn(lx0, lut[c][p10[c]]), __fmul_rn(lx1, lut[c][p11[c]]));
        o[c * plane] = __fadd_rn(__fmul_rn(ly0, top), __fmul_rn(ly1, bot));
    }
}

}  // namespace
}  // namespace mpnhip

using namespace mpnhip;

extern "C" int mpnhip_rcnn_transform(const unsigned char* frames, int64_t n_frames, int H, int W, int oh, int ow, int Hp, int Wp,
                                     const float* mean_std, float* out, void* stream_) {
    static const char* const name = "mpnhip_rcnn_transform";
    hipStream_t stream = (hipStream_t)stream_;
    MPN_CHECK_ARG(n_frames >= 0, "%s: negative n_frames", name);
    if (n_frames == 0) return MPNHIP_OK;
    MPN_CHECK_ARG(frames != nullptr && out != nullptr && mean_std != nullptr, "%s: null frames, mean_std or out", name);
    MPN_CHECK_ARG(H >= 1 && W >= 1 && oh >= 1 && ow >= 1 && Hp >= 1 && Wp >= 1, "%s: H %d, W %d, oh %d, ow %d, Hp %d, Wp %d must be positive",
                  name, H, W, oh, ow, Hp, Wp);
    MPN_CHECK_ARG(oh <= Hp && ow <= Wp, "%s: the resized image %d x %d does not fit the padded %d x %d", name, oh, ow, Hp, Wp);
    for (int c = 0; c < 3; ++c)
        MPN_CHECK_ARG(mean_std[c] - mean_std[c] == 0.f && mean_std[3 + c] - mean_std[3 + c] == 0.f && mean_std[3 + c] != 0.f,
                      "%s: mean and std must be finite, std not 0", name);
    MPN_CHECK_ARG((int64_t)3 * H * W <= INT32_MAX, "%s: a frame of 3 x %lld bytes is beyond the 32-bit offsets", name, (long long)H * W);
    MPN_CHECK_ARG((int64_t)3 * Hp * Wp <= INT32_MAX, "%s: an output image of 3 x %lld floats is beyond the 32-bit offsets", name,
                  (long long)Hp * Wp);
    const int64_t plane = (int64_t)Hp * Wp;
    MPN_CHECK_ARG(n_frames <= ((int64_t)INT32_MAX * RT_THREADS) / plane, "%s: %lld frames of %d x %d are more than one launch holds", name,
                  (long long)n_frames, Hp, Wp);
    RcnnNorm norm;
    for (int c = 0; c < 3; ++c) { norm.mean[c] = mean_std[c]; norm.std[c] = mean_std[3 + c]; }
    const int64_t total = n_frames * plane;
    rcnn_transform_kernel<<<(unsigned)((total + RT_THREADS - 1) / RT_THREADS), RT_THREADS, 0, stream>>>(
        frames, H, W, oh, ow, Hp, Wp, (float)H / (float)oh, (float)W / (float)ow, norm, out, total);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}
