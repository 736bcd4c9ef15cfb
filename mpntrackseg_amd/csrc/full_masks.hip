// From RoI masks to MOTS run-length masks (the end of MPNTracker.track):
//   paste_masks_in_image (torchvision.models.detection.roi_heads)   reference tracker/mpn_tracker.py:285
//   ensure_unique_masks                                             reference utils/mots.py:5-25
//   >= mask_threshold, rletools.encode                              reference tracker/mpn_tracker.py:292-297
// The reference materialises n full images per frame, takes the arg-max over them and encodes each.  Here a frame is ONE label
// per pixel: every pixel walks the detections whose expanded box meets its tile, in ascending order, evaluates the bilinear
// sample of the (virtually zero-padded) RoI mask directly and keeps the running winner -- the n-deep stack never exists.  The
// label image is column-major ([frame][x][y], COCO's flattening), so a detection's RLE is the list of positions where "label ==
// detection" flips: a count pass, a scan over the block counts, an ordered fill and one stable radix sort by detection.
// Integer, compare-only and unfused IEEE arithmetic throughout: the same bits on every call, and the bits of the numpy
// restatement in tests/full_masks_ref.py.  Contraction is off for the whole file: an FMA in the box expansion can move a
// truncated coordinate, one in the interpolation a thresholded pixel.
#pragma clang fp contract(off)

#include "device_prims.h"

#include <rocprim/block/block_scan.hpp>

namespace mpnhip {
namespace {

constexpr int BOX_INTS = 6;        // x0, y0, x1, y1 (inclusive corners of the expanded box), w, h (size of the resize)
constexpr double COORD_MAX = 536870912.0;   // 2^29: x1 - x0 + 1 stays inside int32
constexpr int TILE_Y = 64, TILE_X = 16, PASTE_THREADS = 256, PX = TILE_X / (PASTE_THREADS / TILE_Y);   // 4 pixels per thread
constexpr int EV_THREADS = 256, EV_PER_THREAD = 4, EV_PER_BLOCK = EV_THREADS * EV_PER_THREAD;

// expand_boxes + .to(torch.int64) of roi_heads.py in float64, one operation at a time.  A detection whose row id leaves
// [0, n_rows) or whose box is not finite gets the empty box (x1 < x0): it pastes nothing.
__global__ void k_expand_boxes(const double* __restrict__ boxes, const int* __restrict__ det_ids, int64_t n_dets, int64_t n_rows, int mw,
                               int* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_dets) return;
    const int64_t r = det_ids ? (int64_t)det_ids[j] : j;
    int* o = out + j * BOX_INTS;
    o[0] = 0; o[1] = 0; o[2] = -1; o[3] = -1; o[4] = 1; o[5] = 1;
    if (r < 0 || r >= n_rows) return;
    const double l = boxes[r * 4 + 0], t = boxes[r * 4 + 1], rr = boxes[r * 4 + 2], b = boxes[r * 4 + 3];
    const double scale = (double)(mw + 2) / (double)mw;
    double w_half = (rr - l) * 0.5;
    double h_half = (b - t) * 0.5;
    const double xc = (rr + l) * 0.5;
    const double yc = (b + t) * 0.5;
    w_half = w_half * scale;
    h_half = h_half * scale;
    double e[4] = {xc - w_half, yc - h_half, xc + w_half, yc + h_half};
    int c[4];
    for (int i = 0; i < 4; ++i) {
        if (!(e[i] == e[i]) || e[i] - e[i] != 0.0) return;   // NaN or infinite
        const double v = e[i] > COORD_MAX ? COORD_MAX : (e[i] < -COORD_MAX ? -COORD_MAX : e[i]);
        c[i] = (int)v;                                        // truncation toward zero
    }
    const int w = c[2] - c[0] + 1, h = c[3] - c[1] + 1;
    o[0] = c[0]; o[1] = c[1]; o[2] = c[2]; o[3] = c[3];
    o[4] = w > 1 ? w : 1;
    o[5] = h > 1 ? h : 1;
}

// one axis of F.interpolate(mode='bilinear', align_corners=False) from the padded size `in` (= m + 2) to `out`
struct Axis { int i0, i1; float l0, l1; };
__device__ __forceinline__ Axis axis_of(int j, float scale, int in) {
    float src = scale * ((float)j + 0.5f) - 0.5f;
    src = src > 0.f ? src : 0.f;
    Axis a;
    a.i0 = (int)src;
    a.i0 = a.i0 < in - 1 ? a.i0 : in - 1;        // (never taken for 0 <= j < out; keeps the reads inside the mask whatever comes)
    a.i1 = a.i0 + 1 < in - 1 ? a.i0 + 1 : in - 1;
    a.l1 = src - (float)a.i0;
    a.l0 = 1.f - a.l1;
    return a;
}
// padded index ip in [0, m + 1]: 0 at both ends, m[ip - 1] between
__device__ __forceinline__ float padded(const float* __restrict__ row, int ip, int m) { return (ip >= 1 && ip <= m) ? row[ip - 1] : 0.f; }

// Grid (pixel tiles, frames).  A tile is TILE_Y rows by TILE_X columns; the threads of a wavefront are 64 consecutive y of one
// column, so the stores to the column-major images are contiguous.  Every thread owns PX pixels of one row (columns
// tx0 + q + 4 k): the y half of the interpolation is shared between them.
template <bool VALUES>
__global__ __launch_bounds__(PASTE_THREADS) void k_paste_unique(const float* __restrict__ masks, int mh, int mw, const int* __restrict__ det_ids,
                                                                const int* __restrict__ boxes, const int* __restrict__ frame_ptr,
                                                                int64_t n_dets, int H, int W, float thr, int tiles_y,
                                                                int* __restrict__ labels, float* __restrict__ values) {
    __shared__ int s_box[PASTE_THREADS][BOX_INTS];
    __shared__ int s_det[PASTE_THREADS];
    __shared__ int s_wave[PASTE_THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int f = blockIdx.y;
    const int ty0 = (int)(blockIdx.x % tiles_y) * TILE_Y, tx0 = (int)(blockIdx.x / tiles_y) * TILE_X;
    const int y = ty0 + lane;
    int64_t d0 = frame_ptr[f], d1 = frame_ptr[f + 1];
    d0 = d0 < 0 ? 0 : (d0 > n_dets ? n_dets : d0);
    d1 = d1 < d0 ? d0 : (d1 > n_dets ? n_dets : d1);

    float best[PX];
    int besti[PX];
#pragma unroll
    for (int k = 0; k < PX; ++k) { best[k] = -INFINITY; besti[k] = -1; }
    int64_t walked = 0;

    for (int64_t c0 = d0; c0 < d1; c0 += PASTE_THREADS) {
        // cull this chunk of the frame's boxes against the tile, keeping their order
        const int64_t j = c0 + t;
        int bx[BOX_INTS] = {0, 0, -1, -1, 1, 1};
        if (j < d1) {
#pragma unroll
            for (int i = 0; i < BOX_INTS; ++i) bx[i] = boxes[j * BOX_INTS + i];
        }
        const bool hit = bx[2] >= bx[0] && bx[3] >= bx[1] && bx[0] < tx0 + TILE_X && bx[2] >= tx0 && bx[1] < ty0 + TILE_Y && bx[3] >= ty0;
        const unsigned long long m = __ballot(hit);
        __syncthreads();   // the previous chunk's walk is over
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int base = 0, cnt = 0;
#pragma unroll
        for (int wv = 0; wv < PASTE_THREADS / 64; ++wv) {
            base += wv < wave ? s_wave[wv] : 0;
            cnt += s_wave[wv];
        }
        if (hit) {
            const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
#pragma unroll
            for (int i = 0; i < BOX_INTS; ++i) s_box[pos][i] = bx[i];
            s_det[pos] = (int)j;
        }
        __syncthreads();
        walked += cnt;

        for (int c = 0; c < cnt; ++c) {
            const int x0 = s_box[c][0], y0 = s_box[c][1], x1 = s_box[c][2], y1 = s_box[c][3], w = s_box[c][4], h = s_box[c][5];
            const int det = s_det[c];
            const int64_t row_id = det_ids ? (int64_t)det_ids[det] : (int64_t)det;
            const float* __restrict__ mk = masks + row_id * ((int64_t)mh * mw);
            const bool in_y = y >= y0 && y <= y1;
            const float scale_y = __fdiv_rn((float)(mh + 2), (float)h), scale_x = __fdiv_rn((float)(mw + 2), (float)w);
            Axis ay = axis_of(in_y ? y - y0 : 0, scale_y, mh + 2);
            const bool r0 = ay.i0 >= 1 && ay.i0 <= mh, r1 = ay.i1 >= 1 && ay.i1 <= mh;
            const float* __restrict__ row0 = mk + (int64_t)(r0 ? ay.i0 - 1 : 0) * mw;
            const float* __restrict__ row1 = mk + (int64_t)(r1 ? ay.i1 - 1 : 0) * mw;
#pragma unroll
            for (int k = 0; k < PX; ++k) {
                const int x = tx0 + wave + (PASTE_THREADS / 64) * k;
                float v = 0.f;
                if (in_y && x >= x0 && x <= x1) {
                    const Axis ax = axis_of(x - x0, scale_x, mw + 2);
                    const float a = r0 ? padded(row0, ax.i0, mw) : 0.f, b = r0 ? padded(row0, ax.i1, mw) : 0.f;
                    const float cc = r1 ? padded(row1, ax.i0, mw) : 0.f, d = r1 ? padded(row1, ax.i1, mw) : 0.f;
                    v = ay.l0 * (ax.l0 * a + ax.l1 * b) + ay.l1 * (ax.l0 * cc + ax.l1 * d);
                }
                // np.argmax: the first maximum wins, a NaN is the maximum and the first NaN wins
                if (v > best[k] || (v != v && best[k] == best[k])) { best[k] = v; besti[k] = det; }
            }
        }
    }
    if (y >= H) return;
#pragma unroll
    for (int k = 0; k < PX; ++k) {
        const int x = tx0 + wave + (PASTE_THREADS / 64) * k;
        if (x >= W) continue;
        float b = best[k];
        // the detections that were culled (or an empty frame) are zeros at this pixel: they beat a negative winner, and the label
        // is -1 either way because the threshold is positive
        if (walked < d1 - d0 || d1 == d0) b = b < 0.f ? 0.f : b;
        const int64_t p = ((int64_t)f * W + x) * H + y;
        labels[p] = b >= thr ? besti[k] : -1;
        if (VALUES) values[p] = b;
    }
}

// ---- run boundaries.  Position q = frame * hw + p over the whole launch; the label before p = 0 is -1.
__device__ __forceinline__ int label_at(const int* __restrict__ labels, int64_t q, int n_dets) {
    const int v = labels[q];
    return (v >= 0 && v < n_dets) ? v : -1;
}

// the events of a thread's EV_PER_THREAD consecutive positions, in order (up to two per position): emit(detection, position)
template <class Emit>
__device__ __forceinline__ void thread_events(const int* __restrict__ labels, int64_t total, int64_t hw, int n_dets, Emit emit) {
    const int64_t q0 = ((int64_t)blockIdx.x * EV_THREADS + threadIdx.x) * EV_PER_THREAD;
    if (q0 >= total) return;
    int64_t p = q0 % hw;
    int prev = p == 0 ? -1 : label_at(labels, q0 - 1, n_dets);
#pragma unroll
    for (int i = 0; i < EV_PER_THREAD; ++i) {
        if (q0 + i < total) {
            if (p >= hw) p = 0;   // the next frame begins
            if (p == 0) prev = -1;
            const int cur = label_at(labels, q0 + i, n_dets);
            if (cur != prev) {
                if (prev >= 0) emit(prev, (int)p);
                if (cur >= 0) emit(cur, (int)p);
            }
            prev = cur;
            ++p;
        }
    }
}

using EvScan = rocprim::block_scan<int, EV_THREADS>;

__global__ __launch_bounds__(EV_THREADS) void k_event_count(const int* __restrict__ labels, int64_t total, int64_t hw, int n_dets,
                                                            int* __restrict__ block_counts, int* __restrict__ det_counts) {
    __shared__ typename EvScan::storage_type storage;
    int n = 0;
    thread_events(labels, total, hw, n_dets, [&](int det, int) {
        ++n;
        if (det_counts) atomicAdd(&det_counts[det], 1);   // integer counts: the same whatever the order
    });
    int offset = 0, sum = 0;
    EvScan().exclusive_scan(n, offset, 0, sum, storage);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = sum;
}

__global__ void k_event_total(const int* __restrict__ block_offsets, int64_t n_blocks, int* __restrict__ total) {
    if (blockIdx.x == 0 && threadIdx.x == 0) total[0] = block_offsets[n_blocks];
}

__global__ __launch_bounds__(EV_THREADS) void k_event_fill(const int* __restrict__ labels, int64_t total, int64_t hw, int n_dets,
                                                           const int* __restrict__ block_offsets, int64_t n_events,
                                                           unsigned* __restrict__ keys, int* __restrict__ vals) {
    __shared__ typename EvScan::storage_type storage;
    int n = 0;
    thread_events(labels, total, hw, n_dets, [&](int, int) { ++n; });
    int offset = 0, sum = 0;
    EvScan().exclusive_scan(n, offset, 0, sum, storage);
    int64_t slot = (int64_t)block_offsets[blockIdx.x] + offset;
    thread_events(labels, total, hw, n_dets, [&](int det, int pos) {
        if (slot < n_events) {   // (a count that is not this image's: never write past the buffers)
            keys[slot] = (unsigned)det;
            vals[slot] = pos;
        }
        ++slot;
    });
}

static int64_t ev_blocks(int64_t n_frames, int64_t hw) { return (n_frames * hw + EV_PER_BLOCK - 1) / EV_PER_BLOCK; }

// the event workspace: block counts and offsets [blocks + 1] each, rocprim's scratch, then (fill only) the unsorted keys and
// positions and the sorted keys
struct EvView { int* counts; int* offsets; void* tmp; size_t tmp_bytes; unsigned* keys; int* vals; unsigned* skeys; size_t bytes; };
static EvView ev_view(void* workspace, int64_t n_frames, int64_t hw, int64_t n_events) {
    Carver c(workspace);
    const int64_t nb = ev_blocks(n_frames, hw);
    const size_t a = exclusive_scan_temp<int>(nb + 1), b = sort_pairs_temp<unsigned>(n_events), tmp_bytes = a > b ? a : b, n = (size_t)n_events;
    EvView v = {c.take<int>((size_t)(nb + 1)), c.take<int>((size_t)(nb + 1)), c.take<char>(tmp_bytes), tmp_bytes,
                c.take<unsigned>(n), c.take<int>(n), c.take<unsigned>(n), 0};
    v.bytes = c.bytes();
    return v;
}

// the paste workspace: the detections' expanded boxes
struct PasteView { int* boxes; size_t bytes; };
static PasteView paste_view(void* workspace, int64_t n_dets) {
    Carver c(workspace);
    PasteView v = {c.take<int>((size_t)n_dets * BOX_INTS), 0};
    v.bytes = c.bytes();
    return v;
}

static bool sizes_ok(int64_t n_dets, int64_t n_frames, int64_t hw) {
    return n_dets >= 0 && n_dets < (1LL << 30) && n_frames >= 0 && n_frames <= 65535 && hw >= 0 && hw < (1LL << 31) &&
           n_frames * hw < (1LL << 40);
}

// block counts -> exclusive offsets, offsets[blocks] = number of events
static int count_and_scan(const int* labels, int64_t n_frames, int64_t hw, int64_t n_dets, EvView& v, int* det_counts,
                          hipStream_t stream) {
    const int64_t total = n_frames * hw, nb = ev_blocks(n_frames, hw);
    MPN_HIP(hipMemsetAsync(v.counts + nb, 0, 4, stream));
    hipLaunchKernelGGL(k_event_count, dim3((unsigned)nb), dim3(EV_THREADS), 0, stream, labels, total, hw, (int)n_dets, v.counts, det_counts);
    MPN_LAUNCH_CHECK();
    MPN_HIP(rocprim::exclusive_scan(v.tmp, v.tmp_bytes, v.counts, v.offsets, 0, (size_t)(nb + 1), rocprim::plus<int>(), stream));
    return MPNHIP_OK;
}

}  // namespace
}  // namespace mpnhip

using namespace mpnhip;

extern "C" size_t mpnhip_full_masks_workspace_bytes(int64_t n_dets, int64_t n_frames, int64_t hw, int64_t n_events) {
    if (!sizes_ok(n_dets, n_frames, hw) || n_events < 0 || n_events >= (1LL << 31)) return 0;
    const size_t paste = paste_view(nullptr, n_dets).bytes;
    const size_t events = (n_frames == 0 || hw == 0) ? 0 : ev_view(nullptr, n_frames, hw, n_events).bytes;
    const size_t need = paste > events ? paste : events;
    return need ? need + 256 : 0;
}

extern "C" int mpnhip_paste_unique_masks(const float* masks, int64_t n_rows, int mh, int mw, const double* boxes, const int32_t* det_ids,
                                         int64_t n_dets, const int32_t* frame_ptr, int64_t n_frames, int img_h, int img_w,
                                         float mask_threshold, int32_t* labels, float* values, void* workspace, size_t workspace_bytes,
                                         void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(n_rows >= 0 && img_h >= 0 && img_w >= 0 && sizes_ok(n_dets, n_frames, (int64_t)img_h * img_w),
                  "paste_unique_masks: bad sizes (H * W must stay below 2^31, at most 65535 frames per call)");
    MPN_CHECK_ARG(mask_threshold > 0.f, "paste_unique_masks: mask_threshold must be positive (with a threshold <= 0 the reference "
                  "hands every pixel no mask covers to the frame's first detection)");
    if (n_frames == 0 || img_h == 0 || img_w == 0) return MPNHIP_OK;
    MPN_CHECK_ARG(mh >= 1 && mw >= 1, "paste_unique_masks: the RoI masks need mh, mw >= 1");
    MPN_CHECK_ARG(labels && frame_ptr, "paste_unique_masks: null labels / frame_ptr");
    MPN_CHECK_ARG(n_dets == 0 || (masks && boxes), "paste_unique_masks: null masks / boxes");
    const PasteView pv = paste_view(workspace, n_dets);
    if (n_dets > 0) MPN_CHECK_WORKSPACE("paste_unique_masks", workspace, workspace_bytes, pv.bytes);
    int* bx = pv.boxes;
    if (n_dets > 0) {
        hipLaunchKernelGGL(k_expand_boxes, dim3(blocks_for(n_dets)), dim3(256), 0, stream, boxes, det_ids, n_dets, n_rows, mw, bx);
        MPN_LAUNCH_CHECK();
    }
    const int tiles_y = (img_h + TILE_Y - 1) / TILE_Y, tiles_x = (img_w + TILE_X - 1) / TILE_X;
    const dim3 grid((unsigned)((int64_t)tiles_y * tiles_x), (unsigned)n_frames);
    if (values)
        hipLaunchKernelGGL(k_paste_unique<true>, grid, dim3(PASTE_THREADS), 0, stream, masks, mh, mw, det_ids, bx, frame_ptr, n_dets, img_h,
                           img_w, mask_threshold, tiles_y, labels, values);
    else
        hipLaunchKernelGGL(k_paste_unique<false>, grid, dim3(PASTE_THREADS), 0, stream, masks, mh, mw, det_ids, bx, frame_ptr, n_dets, img_h,
                           img_w, mask_threshold, tiles_y, labels, values);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}

extern "C" int mpnhip_mask_run_events_count(const int32_t* labels, int64_t n_frames, int64_t hw, int64_t n_dets, int32_t* det_counts,
                                            int32_t* n_events, void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(sizes_ok(n_dets, n_frames, hw), "mask_run_events_count: bad sizes (H * W must stay below 2^31)");
    if (n_frames == 0 || hw == 0 || n_dets == 0) {   // no event: zero what the caller gave
        if (n_dets > 0 && det_counts) MPN_HIP(hipMemsetAsync(det_counts, 0, (size_t)n_dets * 4, stream));
        if (n_events) MPN_HIP(hipMemsetAsync(n_events, 0, 4, stream));
        return MPNHIP_OK;
    }
    MPN_CHECK_ARG(labels && det_counts && n_events, "mask_run_events_count: null pointer");
    EvView v = ev_view(workspace, n_frames, hw, 0);
    MPN_CHECK_WORKSPACE("mask_run_events_count", workspace, workspace_bytes, v.bytes);
    MPN_HIP(hipMemsetAsync(det_counts, 0, (size_t)n_dets * 4, stream));
    MPN_TRY(count_and_scan(labels, n_frames, hw, n_dets, v, det_counts, stream));
    hipLaunchKernelGGL(k_event_total, dim3(1), dim3(64), 0, stream, v.offsets, ev_blocks(n_frames, hw), n_events);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}

extern "C" int mpnhip_mask_run_events(const int32_t* labels, int64_t n_frames, int64_t hw, int64_t n_dets, int64_t n_events,
                                      int32_t* event_pos, void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(sizes_ok(n_dets, n_frames, hw) && n_events >= 0 && n_events < (1LL << 31),
                  "mask_run_events: bad sizes (H * W and the number of events must stay below 2^31)");
    if (n_events == 0 || n_frames == 0 || hw == 0 || n_dets == 0) return MPNHIP_OK;
    MPN_CHECK_ARG(labels && event_pos, "mask_run_events: null pointer");
    EvView v = ev_view(workspace, n_frames, hw, n_events);
    MPN_CHECK_WORKSPACE("mask_run_events", workspace, workspace_bytes, v.bytes);
    MPN_TRY(count_and_scan(labels, n_frames, hw, n_dets, v, nullptr, stream));
    // (slots the image does not fill -- a count that is not its own -- sort behind every detection)
    MPN_HIP(hipMemsetAsync(v.keys, 0xFF, (size_t)n_events * 4, stream));
    MPN_HIP(hipMemsetAsync(v.vals, 0, (size_t)n_events * 4, stream));
    hipLaunchKernelGGL(k_event_fill, dim3((unsigned)ev_blocks(n_frames, hw)), dim3(EV_THREADS), 0, stream, labels, n_frames * hw, hw,
                       (int)n_dets, v.offsets, n_events, v.keys, v.vals);
    MPN_LAUNCH_CHECK();
    // the fill is in position order inside a frame and a detection belongs to one frame: a STABLE sort by detection alone leaves
    // every detection's positions ascending; only the bits a detection index needs are sorted (the filler key has them all set)
    MPN_HIP(rocprim::radix_sort_pairs(v.tmp, v.tmp_bytes, v.keys, v.skeys, v.vals, event_pos, (size_t)n_events, 0, key_bits((uint64_t)n_dets), stream));
    return MPNHIP_OK;
}
