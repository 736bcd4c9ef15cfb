// The per-frame tables of mpnhip_label_overlap as the metric kernels read them (mots_eval.hip, hota.hip): a launch's lists
// grouped by frame, the clamped view of one frame's cells, and the areas (row and column sums) of its entries.  Every index
// that comes from a caller's array is clamped or checked here before it is used.
#pragma once
#include "common.h"

namespace mpnhip {

constexpr int MT_THREADS = 256, MT_WAVES = MT_THREADS / 64;

// largest f in [0, n_frames) with ptr[f] <= e < ptr[f + 1], or -1 (whatever ptr holds, the result stays inside [-1, n_frames))
__device__ __forceinline__ int frame_of(const int* __restrict__ ptr, int n_frames, int e) {
    int lo = 0, hi = n_frames;   // first f with ptr[f] > e
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ptr[mid] <= e) lo = mid + 1; else hi = mid;
    }
    const int f = lo - 1;
    return (f >= 0 && e < ptr[f + 1]) ? f : -1;
}

// Frame f of a launch: its entries on either side (clamped into the lists) and its cells.  ok = false: the frame's cells do
// not lie inside the table -- nothing of it is read or written.
struct FrameTab { int a0, na, b0, nb; int64_t base; bool ok; };
__device__ __forceinline__ void clamp_range(const int* __restrict__ ptr, int f, int n, int& first, int& count) {
    int64_t d0 = ptr[f], d1 = ptr[f + 1];
    d0 = d0 < 0 ? 0 : (d0 > n ? n : d0);
    d1 = d1 < d0 ? d0 : (d1 > n ? n : d1);
    first = (int)d0;
    count = (int)(d1 - d0);
}
__device__ __forceinline__ FrameTab frame_tab(const int* __restrict__ a_ptr, const int* __restrict__ b_ptr,
                                              const int64_t* __restrict__ table_ptr, int f, int n_a, int n_b, int64_t table_cells) {
    FrameTab t;
    clamp_range(a_ptr, f, n_a, t.a0, t.na);
    clamp_range(b_ptr, f, n_b, t.b0, t.nb);
    t.base = table_ptr[f];
    const int64_t cells = (int64_t)(t.na + 1) * (t.nb + 1);
    t.ok = t.base >= 0 && t.base <= table_cells && cells <= table_cells - t.base;
    return t;
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// one wavefront per a-entry: its area (row sum, the "no object" column included)
static __global__ __launch_bounds__(MT_THREADS) void k_row_sums(const int* __restrict__ table, const int64_t* __restrict__ table_ptr,
                                                                const int* __restrict__ a_ptr, const int* __restrict__ b_ptr, int n_frames,
                                                                int n_a, int n_b, int64_t table_cells, int* __restrict__ a_area) {
    const int a = blockIdx.x * MT_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (a >= n_a) return;
    const int f = frame_of(a_ptr, n_frames, a);
    int sum = 0;
    if (f >= 0) {
        const FrameTab ft = frame_tab(a_ptr, b_ptr, table_ptr, f, n_a, n_b, table_cells);
        const int ia = a - ft.a0;
        if (ft.ok && ia >= 0 && ia < ft.na) {
            const int* __restrict__ row = table + ft.base + (int64_t)(ia + 1) * (ft.nb + 1);
            for (int c = lane; c <= ft.nb; c += 64) sum += row[c];
        }
    }
    sum = wave_sum(sum);
    if (lane == 0) a_area[a] = sum;
}

// one thread per b-entry (neighbouring threads read neighbouring columns): its area and its share inside the ignore region
static __global__ void k_col_sums(const int* __restrict__ table, const int64_t* __restrict__ table_ptr, const int* __restrict__ a_ptr,
                                  const int* __restrict__ b_ptr, int n_frames, int n_a, int n_b, int64_t table_cells,
                                  const unsigned char* __restrict__ a_ignore, int* __restrict__ b_area, unsigned char* __restrict__ b_ignored,
                                  unsigned char* __restrict__ b_matched) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_b) return;
    const int f = frame_of(b_ptr, n_frames, b);
    long long area = 0, ign = 0;
    if (f >= 0) {
        const FrameTab ft = frame_tab(a_ptr, b_ptr, table_ptr, f, n_a, n_b, table_cells);
        const int ib = b - ft.b0;
        if (ft.ok && ib >= 0 && ib < ft.nb) {
            const int* __restrict__ col = table + ft.base + (ib + 1);
            for (int r = 0; r <= ft.na; ++r) {
                const int n = col[(int64_t)r * (ft.nb + 1)];
                area += n;
                if (r > 0 && a_ignore[ft.a0 + r - 1]) ign += n;
            }
        }
    }
    b_area[b] = (int)area;
    b_ignored[b] = 2 * ign > area ? 1 : 0;   // intersection / the prediction's own area > 0.5 (MOTS_metrics.py:272-273, kitti_mots.py:341)
    b_matched[b] = 0;
}

static inline bool list_sizes_ok(int64_t n_entries, int64_t n_frames, int64_t hw) {
    return n_entries >= 0 && n_entries < (1LL << 30) && n_frames >= 0 && n_frames <= 65535 && hw >= 0 && hw < (1LL << 31) &&
           n_frames * hw < (1LL << 40);
}

}  // namespace mpnhip
