// Training inputs from a detections file and a ground-truth file (reference data/seq_processing/seq_processor.py):
//   _assign_gt        :203-237   per-frame IoU matrix, a threshold, lapsolver.solve_dense
//   _store_gt_masks   :289-393   pycocotools decode of every matched mask, torchvision.ops.roi_align over the detection's box
// The solver is mpnhip_lsa_batched; here are the cells it is given (box IoU, or mask IoU from the table of mpnhip_label_overlap),
// what is made of its answer, and RoIAlign.  The reference decodes one full-frame float image per matched detection; here the
// ground truth of a frame is ONE int32 label image (mpnhip_paint_label_runs) that every detection of the frame samples, a tap
// being "label == the detection's entry".
// Contraction is off for the whole file: an FMA in the IoU can move a pair across min_iou, one in a sample position a tap.
#pragma clang fp contract(off)

#include "label_tables.h"

namespace mpnhip {
namespace {

constexpr int ROI_THREADS = 256;

// largest f in [0, n_frames) with ptr[f] <= c < ptr[f + 1], or -1 (the int64 form of frame_of)
__device__ __forceinline__ int frame_of_cell(const int64_t* __restrict__ ptr, int n_frames, int64_t c) {
    int lo = 0, hi = n_frames;   // first f with ptr[f] > c
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ptr[mid] <= c) lo = mid + 1; else hi = mid;
    }
    const int f = lo - 1;
    return (f >= 0 && c < ptr[f + 1]) ? f : -1;
}

// The pair a cell stands for: entries ia, ib of frame f.  ok = false: the cell belongs to no frame.
struct CellPair { int f, a0, na, b0, nb, ia, ib; bool ok; };
__device__ __forceinline__ CellPair cell_pair(const int32_t* __restrict__ a_ptr, const int32_t* __restrict__ b_ptr,
                                              const int64_t* __restrict__ cell_ptr, int n_frames, int n_a, int n_b, int64_t cells, int64_t c) {
    CellPair p = {-1, 0, 0, 0, 0, 0, 0, false};
    p.f = frame_of_cell(cell_ptr, n_frames, c);
    if (p.f < 0) return p;
    clamp_range(a_ptr, p.f, n_a, p.a0, p.na);
    clamp_range(b_ptr, p.f, n_b, p.b0, p.nb);
    const int64_t base = cell_ptr[p.f], local = c - base, count = (int64_t)p.na * p.nb;
    if (base < 0 || count > cells - base || local >= count) return p;   // (local >= 0: cell_ptr[f] <= c)
    p.ia = (int)(local / p.nb);
    p.ib = (int)(local % p.nb);
    p.ok = true;
    return p;
}

__device__ __forceinline__ void write_cell(double v, bool union_ok, int na, int nb, double min_iou, int64_t c, double* __restrict__ iou,
                                           unsigned char* __restrict__ allowed, double* __restrict__ cost) {
    const bool ok = union_ok && !(v < min_iou);
    iou[c] = v;
    allowed[c] = ok ? 1 : 0;
    cost[c] = ok ? 1.0 - v : (double)((na < nb ? na : nb) + 1);
}

__device__ __forceinline__ double np_maximum0(double v) { return (v > 0.0 || v != v) ? v : 0.0; }   // np.maximum(v, 0): NaN stays

// ------------------------------------------------------------------------------------------------ costs
// utils/iou.py:4-31, one thread per cell
__global__ void k_box_iou_costs(const double* __restrict__ a_boxes, const double* __restrict__ b_boxes, const int32_t* __restrict__ a_ptr,
                                const int32_t* __restrict__ b_ptr, const int64_t* __restrict__ cell_ptr, int n_frames, int n_a, int n_b,
                                int64_t cells, double min_iou, double* __restrict__ iou, unsigned char* __restrict__ allowed,
                                double* __restrict__ cost) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= cells) return;
    const CellPair p = cell_pair(a_ptr, b_ptr, cell_ptr, n_frames, n_a, n_b, cells, c);
    if (!p.ok) { iou[c] = 0.0; allowed[c] = 0; cost[c] = 0.0; return; }
    const double* __restrict__ A = a_boxes + (int64_t)(p.a0 + p.ia) * 4;
    const double* __restrict__ B = b_boxes + (int64_t)(p.b0 + p.ib) * 4;
    const double x11 = A[0], y11 = A[1], x12 = A[2], y12 = A[3], x21 = B[0], y21 = B[1], x22 = B[2], y22 = B[3];
    const double xA = x11 > x21 || x11 != x11 ? x11 : x21, yA = y11 > y21 || y11 != y11 ? y11 : y21;   // np.maximum / np.minimum
    const double xB = x12 < x22 || x12 != x12 ? x12 : x22, yB = y12 < y22 || y12 != y12 ? y12 : y22;
    const double inter = np_maximum0((xB - xA) + 1.0) * np_maximum0((yB - yA) + 1.0);
    const double area_a = ((x12 - x11) + 1.0) * ((y12 - y11) + 1.0);
    const double area_b = ((x22 - x21) + 1.0) * ((y22 - y21) + 1.0);
    write_cell(inter / ((area_a + area_b) - inter), true, p.na, p.nb, min_iou, c, iou, allowed, cost);
}

// pycocotools' iou from the joint histogram of the two label images, one thread per cell: a frame has a handful of objects, so
// the row and the column of a cell are summed where they are needed
__global__ void k_overlap_iou_costs(const int32_t* __restrict__ table, const int64_t* __restrict__ table_ptr, int64_t table_cells,
                                    const int32_t* __restrict__ a_ptr, const int32_t* __restrict__ b_ptr,
                                    const int64_t* __restrict__ cell_ptr, int n_frames, int n_a, int n_b, int64_t cells, double min_iou,
                                    double* __restrict__ iou, unsigned char* __restrict__ allowed, double* __restrict__ cost) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= cells) return;
    const CellPair p = cell_pair(a_ptr, b_ptr, cell_ptr, n_frames, n_a, n_b, cells, c);
    if (!p.ok) { iou[c] = 0.0; allowed[c] = 0; cost[c] = 0.0; return; }
    const FrameTab ft = frame_tab(a_ptr, b_ptr, table_ptr, p.f, n_a, n_b, table_cells);   // (the same clamped na, nb)
    long long i = 0, A = 0, B = 0;
    if (ft.ok) {
        const int nb1 = ft.nb + 1;
        const int32_t* __restrict__ tab = table + ft.base;
        const int32_t* __restrict__ row = tab + (int64_t)(p.ia + 1) * nb1;
        i = row[p.ib + 1];
        for (int k = 0; k <= ft.nb; ++k) A += row[k];
        for (int r = 0; r <= ft.na; ++r) B += tab[(int64_t)r * nb1 + p.ib + 1];
    }
    const long long u = A + B - i;
    write_cell(u > 0 ? (double)i / (double)u : 0.0, u > 0, p.na, p.nb, min_iou, c, iou, allowed, cost);
}

// ------------------------------------------------------------------------------------------------ finish
__global__ void k_gt_assign_finish(const int32_t* __restrict__ match_b, const unsigned char* __restrict__ allowed, int64_t cells,
                                   const int64_t* __restrict__ cell_ptr, const int32_t* __restrict__ a_ptr, int n_a,
                                   const int32_t* __restrict__ b_ptr, int n_b, int n_frames, const int64_t* __restrict__ gt_ids,
                                   const int32_t* __restrict__ gt_row, const int32_t* __restrict__ det_row, int64_t n_out,
                                   int32_t* __restrict__ det_gt_entry, int64_t* __restrict__ det_id) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n_a) return;
    const int64_t o = det_row ? (int64_t)det_row[a] : (int64_t)a;
    if (o < 0 || o >= n_out) return;
    int entry = -1;
    int64_t id = -1;
    const int f = frame_of(a_ptr, n_frames, a);
    if (f >= 0) {
        int a0, na, b0, nb;
        clamp_range(a_ptr, f, n_a, a0, na);
        clamp_range(b_ptr, f, n_b, b0, nb);
        const int ia = a - a0, ib = match_b[a] - b0;   // (match_b = -1: ib < 0)
        const int64_t base = cell_ptr[f], count = (int64_t)na * nb;
        if (ia >= 0 && ia < na && ib >= 0 && ib < nb && base >= 0 && count <= cells - base && allowed[base + (int64_t)ia * nb + ib]) {
            entry = gt_row ? gt_row[b0 + ib] : b0 + ib;
            id = gt_ids[b0 + ib];
        }
    }
    det_gt_entry[o] = entry;
    det_id[o] = id;
}

// ------------------------------------------------------------------------------------------------ RoIAlign
// One axis of torchvision's pre_calc_for_bilinear_interpolate (ROIAlign_cpu.cpp) for T = float: the sample at v
struct Tap { int low, high; float l, h; bool in; };
__device__ __forceinline__ Tap tap_of(float v, int size) {
    Tap t = {0, 0, 0.f, 0.f, false};
    if (v < -1.0f || v > (float)size || v != v) return t;
    t.in = true;
    if (v <= 0.f) v = 0.f;
    t.low = (int)v;
    if (t.low >= size - 1) {
        t.high = t.low = size - 1;
        v = (float)t.low;
    } else {
        t.high = t.low + 1;
    }
    t.l = v - (float)t.low;
    t.h = (float)(1.0 - (double)t.l);   // (T hy = 1. - ly: the subtraction is a double's)
    return t;
}

struct RoiAxis { float start, bin; int grid; bool ok; };
__device__ __forceinline__ RoiAxis roi_axis(float v1, float v2, int p) {
    RoiAxis r = {v1, 0.f, 0, false};
    float extent = v2 - v1;
    extent = extent < 1.f ? 1.f : extent;   // std::max(extent, 1.f)
    r.bin = extent / (float)p;
    const float g = ceilf(extent / (float)p);
    if (!(v1 - v1 == 0.f) || !(g <= (float)MPNHIP_ROI_MAX_GRID)) return r;   // not finite (a NaN extent fails the second test) or too large
    r.grid = (int)g;
    r.ok = true;
    return r;
}

// One block per detection, the output pixels over its threads.  The taps of neighbouring pixels are neighbours in the label
// image, which (a few hundred KB) stays in L2 for all detections of the frame.
__global__ __launch_bounds__(ROI_THREADS) void k_roi_align_labels(const int32_t* __restrict__ labels, int n_frames, int img_h, int img_w,
                                                                   const int32_t* __restrict__ det_ptr, const int32_t* __restrict__ gt_ptr,
                                                                   const float* __restrict__ boxes, int n_dets, const int32_t* __restrict__ det_row,
                                                                   const int32_t* __restrict__ det_gt_entry, int64_t n_out,
                                                                   const int32_t* __restrict__ gt_label, const int64_t* __restrict__ gt_ids,
                                                                   int64_t n_gt, const int64_t* __restrict__ ignore_ids, int n_ignore, int ph,
                                                                   int pw, float* __restrict__ masks, unsigned char* __restrict__ valid) {
    const int k = blockIdx.x;   // (< n_dets: the grid)
    const int64_t o = det_row ? (int64_t)det_row[k] : (int64_t)k;
    if (o < 0 || o >= n_out) return;   // (block-uniform, like everything up to the pixel loop)
    const int f = frame_of(det_ptr, n_frames, k);
    const int64_t e = det_gt_entry[o];
    int want = -1;
    if (f >= 0 && e >= 0 && e < n_gt) {
        const int label = gt_label[e], g0 = gt_ptr[f], g1 = gt_ptr[f + 1];
        bool ok = label >= 0 && label >= g0 && label < g1;
        const int64_t id = gt_ids[e];
        for (int j = 0; j < n_ignore; ++j) ok = ok && id != ignore_ids[j];
        if (ok) want = label;
    }
    if (threadIdx.x == 0) valid[o] = want >= 0 ? 1 : 0;
    const RoiAxis ax = roi_axis(boxes[(int64_t)k * 4 + 0], boxes[(int64_t)k * 4 + 2], pw);
    const RoiAxis ay = roi_axis(boxes[(int64_t)k * 4 + 1], boxes[(int64_t)k * 4 + 3], ph);
    float* __restrict__ out = masks + o * ((int64_t)ph * pw);
    const int n_px = ph * pw;
    if (want < 0 || !ax.ok || !ay.ok) {
        for (int p = threadIdx.x; p < n_px; p += ROI_THREADS) out[p] = 0.f;
        return;
    }
    const int32_t* __restrict__ img = labels + (int64_t)f * ((int64_t)img_h * img_w);
    const int n_samples = ay.grid * ax.grid;
    const float count = (float)(n_samples > 1 ? n_samples : 1);
    for (int p = threadIdx.x; p < n_px; p += ROI_THREADS) {
        const int py = p / pw, px = p % pw;
        const float y0 = ay.start + (float)py * ay.bin, x0 = ax.start + (float)px * ax.bin;
        float sum = 0.f;
        for (int iy = 0; iy < ay.grid; ++iy) {
            const Tap ty = tap_of(y0 + ((float)iy + .5f) * ay.bin / (float)ay.grid, img_h);
            for (int ix = 0; ix < ax.grid; ++ix) {
                const Tap tx = tap_of(x0 + ((float)ix + .5f) * ax.bin / (float)ax.grid, img_w);
                if (!ty.in || !tx.in) continue;   // (adds + 0.f)
                const int32_t* __restrict__ c_lo = img + (int64_t)tx.low * img_h;
                const int32_t* __restrict__ c_hi = img + (int64_t)tx.high * img_h;
                const float v1 = c_lo[ty.low] == want ? 1.f : 0.f, v2 = c_hi[ty.low] == want ? 1.f : 0.f;
                const float v3 = c_lo[ty.high] == want ? 1.f : 0.f, v4 = c_hi[ty.high] == want ? 1.f : 0.f;
                const float w1 = ty.h * tx.h, w2 = ty.h * tx.l, w3 = ty.l * tx.h, w4 = ty.l * tx.l;
                sum += ((w1 * v1 + w2 * v2) + w3 * v3) + w4 * v4;
            }
        }
        out[p] = sum / count;
    }
}

static bool cost_sizes_ok(int64_t n_a, int64_t n_b, int64_t n_frames, int64_t cells) {
    return list_sizes_ok(n_a, n_frames, 0) && list_sizes_ok(n_b, n_frames, 0) && cells >= 0;
}

}  // namespace
}  // namespace mpnhip

using namespace mpnhip;

extern "C" int mpnhip_box_iou_costs(const double* a_boxes, int64_t n_a, const double* b_boxes, int64_t n_b, const int32_t* a_ptr,
                                    const int32_t* b_ptr, const int64_t* cell_ptr, int64_t n_frames, int64_t cells, double min_iou,
                                    double* iou, unsigned char* allowed, double* cost, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(cost_sizes_ok(n_a, n_b, n_frames, cells), "box_iou_costs: bad sizes (at most 65535 frames per call)");
    if (cells >= (1LL << 31)) {
        set_error("box_iou_costs: %lld cells (2^31 or more) are not supported: fewer frames per call", (long long)cells);
        return MPNHIP_ERR_UNSUPPORTED;
    }
    if (cells == 0) return MPNHIP_OK;
    MPN_CHECK_ARG(n_frames > 0 && a_ptr && b_ptr && cell_ptr, "box_iou_costs: cells without frames / null lists");
    MPN_CHECK_ARG(a_boxes && b_boxes && iou && allowed && cost, "box_iou_costs: null boxes or results");
    hipLaunchKernelGGL(k_box_iou_costs, dim3(blocks_for(cells)), dim3(256), 0, stream, a_boxes, b_boxes, a_ptr, b_ptr, cell_ptr, (int)n_frames,
                       (int)n_a, (int)n_b, cells, min_iou, iou, allowed, cost);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}

extern "C" int mpnhip_overlap_iou_costs(const int32_t* table, int64_t table_cells, const int64_t* table_ptr, const int32_t* a_ptr, int64_t n_a,
                                        const int32_t* b_ptr, int64_t n_b, const int64_t* cell_ptr, int64_t n_frames, int64_t cells,
                                        double min_iou, double* iou, unsigned char* allowed, double* cost, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(cost_sizes_ok(n_a, n_b, n_frames, cells) && table_cells >= 0, "overlap_iou_costs: bad sizes (at most 65535 frames per call)");
    if (cells >= (1LL << 31) || table_cells >= (1LL << 31)) {
        set_error("overlap_iou_costs: %lld cells of a table of %lld (2^31 or more) are not supported: fewer frames per call", (long long)cells,
                  (long long)table_cells);
        return MPNHIP_ERR_UNSUPPORTED;
    }
    if (cells == 0) return MPNHIP_OK;
    MPN_CHECK_ARG(n_frames > 0 && a_ptr && b_ptr && cell_ptr, "overlap_iou_costs: cells without frames / null lists");
    MPN_CHECK_ARG(table && table_ptr && iou && allowed && cost, "overlap_iou_costs: null table or results");
    hipLaunchKernelGGL(k_overlap_iou_costs, dim3(blocks_for(cells)), dim3(256), 0, stream, table, table_ptr, table_cells, a_ptr, b_ptr, cell_ptr,
                       (int)n_frames, (int)n_a, (int)n_b, cells, min_iou, iou, allowed, cost);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}

extern "C" int mpnhip_gt_assign_finish(const int32_t* match_b, const unsigned char* allowed, int64_t cells, const int64_t* cell_ptr,
                                       const int32_t* a_ptr, int64_t n_a, const int32_t* b_ptr, int64_t n_b, int64_t n_frames,
                                       const int64_t* gt_ids, const int32_t* gt_row, const int32_t* det_row, int64_t n_out,
                                       int32_t* det_gt_entry, int64_t* det_id, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(cost_sizes_ok(n_a, n_b, n_frames, cells) && n_out >= 0, "gt_assign_finish: bad sizes (at most 65535 frames per call)");
    if (cells >= (1LL << 31)) {
        set_error("gt_assign_finish: %lld cells (2^31 or more) are not supported: fewer frames per call", (long long)cells);
        return MPNHIP_ERR_UNSUPPORTED;
    }
    if (n_a == 0 || n_out == 0) return MPNHIP_OK;
    MPN_CHECK_ARG(n_frames > 0 && a_ptr && b_ptr && cell_ptr, "gt_assign_finish: detections without frames / null lists");
    MPN_CHECK_ARG(match_b && det_gt_entry && det_id, "gt_assign_finish: null match_b or results");
    MPN_CHECK_ARG(cells == 0 || allowed, "gt_assign_finish: null allowed");
    MPN_CHECK_ARG(n_b == 0 || gt_ids, "gt_assign_finish: null gt_ids");
    hipLaunchKernelGGL(k_gt_assign_finish, dim3(blocks_for(n_a)), dim3(256), 0, stream, match_b, allowed, cells, cell_ptr, a_ptr, (int)n_a, b_ptr,
                       (int)n_b, (int)n_frames, gt_ids, gt_row, det_row, n_out, det_gt_entry, det_id);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}

extern "C" int mpnhip_roi_align_labels(const int32_t* labels, int64_t n_frames, int img_h, int img_w, const int32_t* det_ptr,
                                       const int32_t* gt_ptr, const float* boxes, int64_t n_dets, const int32_t* det_row,
                                       const int32_t* det_gt_entry, int64_t n_out, const int32_t* gt_label, const int64_t* gt_ids, int64_t n_gt,
                                       const int64_t* ignore_ids, int n_ignore, int ph, int pw, float* masks, unsigned char* valid,
                                       void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(img_h >= 0 && img_w >= 0 && list_sizes_ok(n_dets, n_frames, (int64_t)img_h * img_w) && n_out >= 0 && n_gt >= 0 &&
                  n_gt < (1LL << 31) && n_ignore >= 0, "roi_align_labels: bad sizes (H * W must stay below 2^31, at most 65535 frames per call)");
    MPN_CHECK_ARG(ph > 0 && pw > 0 && (int64_t)ph * pw < (1LL << 24), "roi_align_labels: the output size must be positive (and below 2^24 pixels)");
    if (n_dets == 0 || n_out == 0) return MPNHIP_OK;
    MPN_CHECK_ARG(n_frames > 0 && det_ptr && gt_ptr, "roi_align_labels: detections without frames / null lists");
    MPN_CHECK_ARG(boxes && det_gt_entry && masks && valid, "roi_align_labels: null boxes, det_gt_entry or results");
    MPN_CHECK_ARG(n_gt == 0 || (gt_label && gt_ids && labels && img_h > 0 && img_w > 0), "roi_align_labels: ground-truth rows without labels, ids or an image");
    MPN_CHECK_ARG(n_ignore == 0 || ignore_ids, "roi_align_labels: null ignore_ids");
    hipLaunchKernelGGL(k_roi_align_labels, dim3((unsigned)n_dets), dim3(ROI_THREADS), 0, stream, labels, (int)n_frames, img_h, img_w, det_ptr,
                       gt_ptr, boxes, (int)n_dets, det_row, det_gt_entry, n_out, gt_label, gt_ids, n_gt, ignore_ids, n_ignore, ph, pw, masks,
                       valid);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}
