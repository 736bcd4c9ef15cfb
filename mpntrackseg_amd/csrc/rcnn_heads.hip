// The tail of the Mask R-CNN RoI heads on given boxes (include/mpnhip.h: mpnhip_box_predict, mpnhip_nms_batched,
// mpnhip_roi_mask_finish).  The dense and convolution-type layers in front of them are mpnhip_linear, mpnhip_conv2d_affine_forward
// and mpnhip_conv2d_forward; what is here is what follows them:
//
//   box_predict_kernel     FastRCNNPredictor + softmax + BoxCoder.decode + resize_boxes for one class.  One wavefront per box: the
//                          C class rows and the four box rows of `label` are C + 4 dot products of length K; a lane sums the
//                          float4s lane, lane + 64, ... of a row in that order, a butterfly adds the 64 partial sums -- an order
//                          that is a function of K alone.  Softmax and decoding are one explicitly rounded operation at a time.
//   nms_*                  score filter + greedy NMS of every frame of a batch: a stable radix sort of (frame, descending score)
//                          keys, an upper-triangular matrix of 64-bit suppression words built with ballots (one wavefront per
//                          64 x 64 tile, all frames in one launch), and a scan by ONE wavefront per frame whose lane l holds word
//                          l of the "removed" set -- 64 lanes x 64 bits is the cap of 4096 boxes per frame.
//   roi_mask_finish_kernel sigmoid of the label's logit plane and the optional bilinear x 2 (aten, align_corners=False).
//
// Every float operation a decision or a coordinate depends on is an explicitly rounded one (no contraction into FMAs).
#include "device_prims.h"

#include <math.h>

namespace mpnhip {
namespace {

// ------------------------------------------------------------------------------------------------ box predictor
constexpr int BP_WAVES = 4;
constexpr int BP_MAX_CLASSES = MPNHIP_BOX_MAX_CLASSES;

struct BoxPredictArgs {
    const float* h; int64_t ldh;
    const float* w_cls; const float* b_cls; const float* w_box; const float* b_box;
    const float* proposals;
    int64_t n;
    int K, C, label;
    float weight[4];
    float clip, ratio_h, ratio_w;
    float* boxes; float* scores; float* logits; float* deltas;
};

// sum_k h[k] w[k] over the whole wavefront: every lane returns the same bits
__device__ __forceinline__ float wave_dot(const float* __restrict__ h, const float* __restrict__ w, int K, int lane) {
    float acc = 0.f;
    for (int k = lane * 4; k < K; k += 256) {
        const float4 a = *reinterpret_cast<const float4*>(h + k);
        const float4 b = *reinterpret_cast<const float4*>(w + k);
        acc = fmaf(a.x, b.x, acc);
        acc = fmaf(a.y, b.y, acc);
        acc = fmaf(a.z, b.z, acc);
        acc = fmaf(a.w, b.w, acc);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc = __fadd_rn(acc, __shfl_xor(acc, o));
    return acc;
}

// one axis of torchvision 0.6.0's BoxCoder.decode_single, then resize_boxes
__device__ __forceinline__ void decode_axis(float v1, float v2, float dctr, float dsize, float ratio, float* lo, float* hi) {
    const float w = __fsub_rn(v2, v1);
    const float c = __fadd_rn(v1, __fmul_rn(0.5f, w));
    const float pc = __fadd_rn(__fmul_rn(dctr, w), c);
    const float pw = __fmul_rn(expf(dsize), w);
    const float half = __fmul_rn(0.5f, pw);
    *lo = __fmul_rn(__fsub_rn(pc, half), ratio);
    *hi = __fmul_rn(__fadd_rn(pc, half), ratio);
}

__global__ __launch_bounds__(BP_WAVES * 64) void box_predict_kernel(BoxPredictArgs a) {
    __shared__ float s_logit[BP_WAVES][BP_MAX_CLASSES + 5];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t box = (int64_t)blockIdx.x * BP_WAVES + wave;
    if (box >= a.n) return;                       // (no barrier below: a wavefront works alone)
    const float* __restrict__ h = a.h + box * a.ldh;
    float* sl = s_logit[wave];
    for (int c = 0; c < a.C; ++c) {
        const float v = __fadd_rn(wave_dot(h, a.w_cls + (int64_t)c * a.K, a.K, lane), a.b_cls[c]);
        if (lane == 0) sl[c] = v;
    }
    for (int i = 0; i < 4; ++i) {
        const int r = 4 * a.label + i;
        const float v = __fadd_rn(wave_dot(h, a.w_box + (int64_t)r * a.K, a.K, lane), a.b_box[r]);
        if (lane == 0) sl[a.C + i] = v;
    }
    if (lane != 0) return;                        // lane 0 wrote sl and is the only one to read it
    if (a.logits)
        for (int c = 0; c < a.C; ++c) a.logits[box * a.C + c] = sl[c];
    // softmax of the label: subtract the maximum, expf, the sum in class order, one division
    float mx = sl[0];
    for (int c = 1; c < a.C; ++c) mx = sl[c] > mx ? sl[c] : mx;
    float sum = 0.f, mine = 0.f;
    for (int c = 0; c < a.C; ++c) {
        const float e = expf(__fsub_rn(sl[c], mx));
        sum = __fadd_rn(sum, e);
        if (c == a.label) mine = e;
    }
    a.scores[box] = __fdiv_rn(mine, sum);
    float d[4];
    for (int i = 0; i < 4; ++i) {
        d[i] = sl[a.C + i];
        if (a.deltas) a.deltas[box * 4 + i] = d[i];
        d[i] = __fdiv_rn(d[i], a.weight[i]);
    }
    d[2] = d[2] > a.clip ? a.clip : d[2];         // torch.clamp(max=clip): a NaN stays one
    d[3] = d[3] > a.clip ? a.clip : d[3];
    const float* __restrict__ p = a.proposals + box * 4;
    float x1, y1, x2, y2;
    decode_axis(p[0], p[2], d[0], d[2], a.ratio_w, &x1, &x2);
    decode_axis(p[1], p[3], d[1], d[3], a.ratio_h, &y1, &y2);
    float* __restrict__ o = a.boxes + box * 4;
    o[0] = x1, o[1] = y1, o[2] = x2, o[3] = y2;
}

// ------------------------------------------------------------------------------------------------ batched NMS
constexpr unsigned NMS_NOT_A_CANDIDATE = 0xFFFFFFFFu;   // low key word of a row that never takes part; no score maps to it

// The NMS workspace: sort keys and row ids before and after the sort, the suppression words, rocprim's scratch.
struct NmsView {
    unsigned long long* keys; unsigned long long* skeys; int* vals; int* svals;
    unsigned long long* words;
    void* tmp;
    size_t tmp_bytes, bytes;
};
static int nms_words_per_row(int max_per_frame) { return (max_per_frame + 63) / 64; }
static NmsView nms_view(void* workspace, int64_t n, int max_per_frame) {
    Carver c(workspace);
    const size_t N = (size_t)n;
    NmsView v = {c.take<unsigned long long>(N), c.take<unsigned long long>(N), c.take<int>(N), c.take<int>(N),
                 c.take<unsigned long long>(N * (size_t)nms_words_per_row(max_per_frame)), nullptr, sort_pairs_temp<unsigned long long>(n), 0};
    v.tmp = c.take<char>(v.tmp_bytes);
    v.bytes = c.bytes();
    return v;
}

// the rows of frame f, or false: ptr does not describe a frame this call can take (count[f] = -1)
__device__ __forceinline__ bool nms_frame(const int* __restrict__ ptr, int f, int64_t n, int max_per_frame, int* base, int* rows) {
    const int b = ptr[f], e = ptr[f + 1];
    *base = b, *rows = e - b;
    return ptr[0] == 0 && b >= 0 && e >= b && (int64_t)e <= n && e - b <= max_per_frame;
}

// key of row i: (frame, descending score); a stable ascending sort then visits equal scores by increasing row
__global__ __launch_bounds__(256) void nms_keys_kernel(const float* __restrict__ scores, const int* __restrict__ ptr, int64_t n, int F,
                                                        float score_threshold, unsigned long long* __restrict__ keys,
                                                        int* __restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    // the last f in [0, F] with ptr[f] <= i; f == F (or a frame that ends before i): the row belongs to no frame
    int lo = 0, hi = F;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((int64_t)ptr[mid] <= i) lo = mid; else hi = mid - 1;
    }
    unsigned frame = (unsigned)lo;
    if (lo >= F || (int64_t)ptr[lo] > i || (int64_t)ptr[lo + 1] <= i) frame = (unsigned)F;
    float s = scores[i];
    unsigned low = NMS_NOT_A_CANDIDATE;
    if (s >= score_threshold) {                   // false for a NaN score
        if (s == 0.f) s = 0.f;                    // -0 and +0 are equal scores
        const unsigned u = __float_as_uint(s);
        const unsigned asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
        low = ~asc;
    }
    keys[i] = ((unsigned long long)frame << 32) | low;
    vals[i] = (int)i;
}

struct NmsBox { float x1, y1, x2, y2; };

__device__ __forceinline__ bool nms_suppresses(const NmsBox& a, const NmsBox& b, float thr) {
    const float area_a = __fmul_rn(__fsub_rn(a.x2, a.x1), __fsub_rn(a.y2, a.y1));
    const float area_b = __fmul_rn(__fsub_rn(b.x2, b.x1), __fsub_rn(b.y2, b.y1));
    const float iw = fmaxf(__fsub_rn(fminf(a.x2, b.x2), fmaxf(a.x1, b.x1)), 0.f);
    const float ih = fmaxf(__fsub_rn(fminf(a.y2, b.y2), fmaxf(a.y1, b.y1)), 0.f);
    const float inter = __fmul_rn(iw, ih);
    const float iou = __fdiv_rn(inter, __fsub_rn(__fadd_rn(area_a, area_b), inter));
    return iou > thr;                             // 0 / 0 = NaN suppresses nothing
}

// One wavefront per (frame, row tile, column tile) of the upper triangle: bit b of words[(base + i) * W + ct] says that the box
// at sorted position i of the frame suppresses the one at position 64 ct + b > i.
__global__ __launch_bounds__(64) void nms_words_kernel(const float* __restrict__ boxes, const int* __restrict__ ptr,
                                                       const int* __restrict__ svals, int64_t n, int max_per_frame, int W, float iou_threshold,
                                                       unsigned long long* __restrict__ words) {
    const int tiles = W * W;
    const int f = blockIdx.x / tiles, rt = (blockIdx.x % tiles) / W, ct = blockIdx.x % W;
    if (ct < rt) return;
    int base, rows;
    if (!nms_frame(ptr, f, n, max_per_frame, &base, &rows)) return;
    if (rt * 64 >= rows || ct * 64 >= rows) return;
    __shared__ NmsBox rb[64];
    const int lane = threadIdx.x;
    const int i = rt * 64 + lane, j = ct * 64 + lane;
    NmsBox mine = {0.f, 0.f, 0.f, 0.f};
    if (i < rows) {
        const float4 v = *reinterpret_cast<const float4*>(boxes + (int64_t)svals[base + i] * 4);
        rb[lane] = {v.x, v.y, v.z, v.w};
    }
    if (j < rows) {
        const float4 v = *reinterpret_cast<const float4*>(boxes + (int64_t)svals[base + j] * 4);
        mine = {v.x, v.y, v.z, v.w};
    }
    __syncthreads();
    const int nr = min(64, rows - rt * 64);
    unsigned long long word = 0;
    for (int r = 0; r < nr; ++r) {
        const NmsBox a = rb[r];
        const bool hit = j < rows && j > rt * 64 + r && nms_suppresses(a, mine, iou_threshold);
        const unsigned long long m = __ballot(hit);
        if (lane == r) word = m;
    }
    if (i < rows) words[(int64_t)(base + i) * W + ct] = word;
}

__device__ __forceinline__ unsigned long long read_lane64(unsigned long long v, int l) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
    return ((unsigned long long)hi << 32) | lo;
}

// One wavefront per frame.  Lane l holds word l of the removed set (sorted positions 64 l .. 64 l + 63).  A chunk of 64 positions
// is resolved serially on wave-uniform values -- position b is kept unless removed, and then removes what its diagonal word says
// --, after which the rows of the chunk's kept boxes are OR-ed into the lanes behind it.
__global__ __launch_bounds__(64) void nms_scan_kernel(const int* __restrict__ ptr, const unsigned long long* __restrict__ skeys,
                                                      const int* __restrict__ svals, const unsigned long long* __restrict__ words, int64_t n,
                                                      int max_per_frame, int W, unsigned char* __restrict__ keep, int* __restrict__ order,
                                                      int* __restrict__ count) {
    const int f = blockIdx.x, lane = threadIdx.x;
    int base, rows;
    if (!nms_frame(ptr, f, n, max_per_frame, &base, &rows)) {
        if (lane == 0) count[f] = -1;
        return;
    }
    unsigned long long removed = 0;
    int kept_total = 0;
    const int chunks = (rows + 63) >> 6;
    for (int c = 0; c < chunks; ++c) {
        const int p = c * 64 + lane;
        const bool cand = p < rows && (unsigned)(skeys[base + p] & 0xFFFFFFFFull) != NMS_NOT_A_CANDIDATE;
        const unsigned long long valid = __ballot(cand);
        if (valid == 0) break;                    // candidates come first in a frame's sorted slice
        const unsigned long long diag = cand ? words[(int64_t)(base + p) * W + c] : 0ull;
        unsigned long long cur = read_lane64(removed, c) | ~valid;
        unsigned long long kept = 0;
#pragma unroll
        for (int b = 0; b < 64; ++b) {
            if (!((cur >> b) & 1ull)) {
                kept |= 1ull << b;
                cur |= read_lane64(diag, b);
            }
        }
        if ((kept >> lane) & 1ull) {
            const int row = svals[base + p];
            order[base + kept_total + __popcll(kept & ((1ull << lane) - 1ull))] = row;
            keep[row] = 1;
        }
        kept_total += __popcll(kept);
        if (lane > c && lane < chunks) {          // (the column tiles the words kernel wrote; chunks <= W)
            unsigned long long k = kept;
            while (k) {
                const int b = __ffsll((long long)k) - 1;
                k &= k - 1;
                removed |= words[(int64_t)(base + c * 64 + b) * W + lane];
            }
        }
    }
    if (lane == 0) count[f] = kept_total;
}

// ------------------------------------------------------------------------------------------------ mask tail
// aten's area_pixel_compute_source_index for align_corners=False and a scale factor of 2, in float32
__device__ __forceinline__ void up2_axis(int dst, int S, int* i0, int* i1, float* l0, float* l1) {
    float src = __fsub_rn(__fmul_rn(__fadd_rn((float)dst, 0.5f), 0.5f), 0.5f);
    src = src < 0.f ? 0.f : src;
    const int i = (int)src;
    *i0 = i;
    *i1 = min(i + 1, S - 1);
    *l1 = __fsub_rn(src, (float)i);
    *l0 = __fsub_rn(1.f, *l1);
}

__device__ __forceinline__ float sigmoid_rn(float x) { return __fdiv_rn(1.f, __fadd_rn(1.f, expf(-x))); }

__global__ __launch_bounds__(256) void roi_mask_finish_kernel(const float* __restrict__ logits, int64_t ld, int S, int up, int label,
                                                              float* __restrict__ out, int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int So = S * up, plane = So * So;
    const int64_t img = idx / plane;
    const int pix = (int)(idx % plane), y = pix / So, x = pix % So;
    const float* __restrict__ src = logits + img * ld + (int64_t)label * S * S;
    if (up == 1) {
        out[idx] = sigmoid_rn(src[y * S + x]);
        return;
    }
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    up2_axis(y, S, &y0, &y1, &ly0, &ly1);
    up2_axis(x, S, &x0, &x1, &lx0, &lx1);
    const float t00 = sigmoid_rn(src[y0 * S + x0]), t01 = sigmoid_rn(src[y0 * S + x1]);
    const float t10 = sigmoid_rn(src[y1 * S + x0]), t11 = sigmoid_rn(src[y1 * S + x1]);
    const float top = __fadd_rn(__fmul_rn(lx0, t00), __fmul_rn(lx1, t01));
    const float bot = __fadd_rn(__fmul_rn(lx0, t10), __fmul_rn(lx1, t11));
    out[idx] = __fadd_rn(__fmul_rn(ly0, top), __fmul_rn(ly1, bot));
}

static bool finite_f(float v) { return v - v == 0.f; }

}  // namespace
}  // namespace mpnhip

using namespace mpnhip;

extern "C" int mpnhip_box_predict(const float* h, int64_t ldh, const float* w_cls, const float* b_cls, const float* w_box, const float* b_box,
                                  const float* proposals, int64_t n, int k, int num_classes, int label, const float* weights, float clip,
                                  float ratio_h, float ratio_w, float* boxes, float* scores, float* logits, float* deltas, void* stream_) {
    static const char* const name = "mpnhip_box_predict";
    hipStream_t stream = (hipStream_t)stream_;
    MPN_CHECK_ARG(n >= 0, "%s: negative n", name);
    if (n == 0) return MPNHIP_OK;
    MPN_CHECK_ARG(h && w_cls && b_cls && w_box && b_box && proposals, "%s: null h, weights, biases or proposals", name);
    MPN_CHECK_ARG(boxes && scores, "%s: null boxes or scores", name);
    MPN_CHECK_ARG(weights, "%s: null weights[4]", name);
    MPN_CHECK_ARG(num_classes >= 2 && num_classes <= BP_MAX_CLASSES, "%s: %d classes (2 .. %d)", name, num_classes, BP_MAX_CLASSES);
    MPN_CHECK_ARG(k >= 4 && k % 4 == 0, "%s: K = %d must be a positive multiple of 4", name, k);
    MPN_CHECK_ARG(label >= 0 && label < num_classes, "%s: label %d outside [0, %d)", name, label, num_classes);
    MPN_CHECK_ARG(ldh >= k && ldh % 4 == 0, "%s: ldh %lld must be a multiple of 4 and at least K = %d", name, (long long)ldh, k);
    MPN_CHECK_ARG(aligned16(h) && aligned16(w_cls) && aligned16(w_box), "%s: h, w_cls and w_box must be 16-byte aligned", name);
    for (int i = 0; i < 4; ++i)
        MPN_CHECK_ARG(finite_f(weights[i]) && weights[i] != 0.f, "%s: weights must be finite and not 0", name);
    MPN_CHECK_ARG(n <= (int64_t)INT32_MAX, "%s: %lld boxes are more than one launch holds", name, (long long)n);
    BoxPredictArgs a;
    a.h = h, a.ldh = ldh, a.w_cls = w_cls, a.b_cls = b_cls, a.w_box = w_box, a.b_box = b_box, a.proposals = proposals;
    a.n = n, a.K = k, a.C = num_classes, a.label = label;
    for (int i = 0; i < 4; ++i) a.weight[i] = weights[i];
    a.clip = clip, a.ratio_h = ratio_h, a.ratio_w = ratio_w;
    a.boxes = boxes, a.scores = scores, a.logits = logits, a.deltas = deltas;
    box_predict_kernel<<<(unsigned)((n + BP_WAVES - 1) / BP_WAVES), BP_WAVES * 64, 0, stream>>>(a);
    MPN_LAUNCH_CHECK();
    count_path(PC_BOX_PREDICT);
    return MPNHIP_OK;
}

static bool nms_sizes_ok(int64_t n, int max_per_frame) {
    return n >= 0 && n <= (1LL << 30) && max_per_frame >= 1 && max_per_frame <= MPNHIP_NMS_MAX_PER_FRAME;
}

extern "C" size_t mpnhip_nms_batched_workspace_bytes(int64_t n, int max_per_frame) {
    if (!nms_sizes_ok(n, max_per_frame) || n == 0) return 0;
    return nms_view(nullptr, n, max_per_frame).bytes;
}

extern "C" int mpnhip_nms_batched(const float* boxes, const float* scores, const int32_t* ptr, int64_t n, int64_t n_frames,
                                  int max_per_frame, float score_threshold, float iou_threshold, unsigned char* keep, int32_t* order,
                                  int32_t* count, void* workspace, size_t workspace_bytes, void* stream_) {
    static const char* const name = "mpnhip_nms_batched";
    hipStream_t stream = (hipStream_t)stream_;
    MPN_CHECK_ARG(n >= 0 && n_frames >= 0, "%s: negative n or n_frames", name);
    if (n == 0) return MPNHIP_OK;
    MPN_CHECK_ARG(max_per_frame >= 1 && max_per_frame <= MPNHIP_NMS_MAX_PER_FRAME, "%s: max_per_frame %d outside 1 .. %d", name,
                  max_per_frame, MPNHIP_NMS_MAX_PER_FRAME);
    MPN_CHECK_ARG(n <= (1LL << 30), "%s: %lld boxes are more than the 32-bit row ids hold", name, (long long)n);
    MPN_CHECK_ARG(n_frames >= 1, "%s: boxes without frames", name);
    MPN_CHECK_ARG(boxes && scores && ptr, "%s: null boxes, scores or ptr", name);
    MPN_CHECK_ARG(keep && order && count, "%s: null keep, order or count", name);
    MPN_CHECK_ARG(aligned16(boxes), "%s: boxes must be 16-byte aligned", name);
    MPN_CHECK_ARG(iou_threshold == iou_threshold && score_threshold == score_threshold, "%s: a threshold is NaN", name);
    const int W = nms_words_per_row(max_per_frame);
    MPN_CHECK_ARG(n_frames <= (int64_t)INT32_MAX / ((int64_t)W * W), "%s: %lld frames of %d x %d tiles are more than one launch holds", name,
                  (long long)n_frames, W, W);
    NmsView v = nms_view(workspace, n, max_per_frame);
    MPN_CHECK_WORKSPACE("mpnhip_nms_batched", workspace, workspace_bytes, v.bytes);
    const int F = (int)n_frames;
    MPN_HIP(hipMemsetAsync(keep, 0, (size_t)n, stream));
    MPN_HIP(hipMemsetAsync(order, 0xFF, (size_t)n * sizeof(int32_t), stream));
    nms_keys_kernel<<<blocks_for(n), 256, 0, stream>>>(scores, ptr, n, F, score_threshold, v.keys, v.vals);
    MPN_LAUNCH_CHECK();
    MPN_HIP(rocprim::radix_sort_pairs(v.tmp, v.tmp_bytes, v.keys, v.skeys, v.vals, v.svals, (size_t)n, 0, 32 + key_bits((uint64_t)F), stream));
    nms_words_kernel<<<(unsigned)(F * W * W), 64, 0, stream>>>(boxes, ptr, v.svals, n, max_per_frame, W, iou_threshold, v.words);
    MPN_LAUNCH_CHECK();
    nms_scan_kernel<<<(unsigned)F, 64, 0, stream>>>(ptr, v.skeys, v.svals, v.words, n, max_per_frame, W, keep, order, count);
    MPN_LAUNCH_CHECK();
    count_path(PC_NMS_BATCHED);
    return MPNHIP_OK;
}

extern "C" int mpnhip_roi_mask_finish(const float* logits, int64_t ld, int64_t n, int num_channels, int label, int size, int up, float* out,
                                      void* stream_) {
    static const char* const name = "mpnhip_roi_mask_finish";
    hipStream_t stream = (hipStream_t)stream_;
    MPN_CHECK_ARG(n >= 0, "%s: negative n", name);
    if (n == 0) return MPNHIP_OK;
    MPN_CHECK_ARG(logits && out, "%s: null logits or out", name);
    MPN_CHECK_ARG(size >= 1 && size <= MPNHIP_ROI_MASK_MAX_SIZE, "%s: size %d outside 1 .. %d", name, size, MPNHIP_ROI_MASK_MAX_SIZE);
    MPN_CHECK_ARG(up == 1 || up == 2, "%s: up %d is neither 1 nor 2", name, up);
    MPN_CHECK_ARG(num_channels >= 1 && (int64_t)num_channels * size * size <= INT32_MAX, "%s: %d channels of %d x %d", name, num_channels,
                  size, size);
    MPN_CHECK_ARG(label >= 0 && label < num_channels, "%s: label %d outside [0, %d)", name, label, num_channels);
    MPN_CHECK_ARG(ld >= (int64_t)num_channels * size * size, "%s: ld %lld is smaller than an image of %d x %d x %d", name, (long long)ld,
                  num_channels, size, size);
    const int64_t plane = (int64_t)size * up * size * up;
    MPN_CHECK_ARG(n <= ((int64_t)INT32_MAX * 256) / plane, "%s: %lld masks of %d x %d are more than one launch holds", name, (long long)n,
                  size * up, size * up);
    const int64_t total = n * plane;
    roi_mask_finish_kernel<<<blocks_for(total), 256, 0, stream>>>(logits, ld, size, up, label, out, total);
    MPN_LAUNCH_CHECK();
    count_path(PC_ROI_MASK_FINISH);
    return MPNHIP_OK;
}
