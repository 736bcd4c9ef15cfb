// A launch of the KITTI-MOTS metric kernels as hota.hip and clear_identity.hip read it: the two lists grouped by frame and
// the clamped view of one frame's cells of the similarity block that mpnhip_hota_frame_similarity wrote.  Every index that
// comes from a caller's array is clamped or checked here before it is used.
#pragma once
#include "label_tables.h"

namespace mpnhip {

// one launch's lists and the layout of its similarity block: frame f owns na_f x nb_f doubles at sim_ptr[f]
struct Lists {
    const int* a_ptr; const int* b_ptr; const int64_t* sim_ptr;
    int n_a, n_b, n_frames;
    int64_t sim_cells;
};
struct FrameSim { int a0, na, b0, nb; int64_t base; bool ok; };
__device__ __forceinline__ FrameSim frame_sim(const Lists& L, int f) {
    FrameSim s;
    clamp_range(L.a_ptr, f, L.n_a, s.a0, s.na);
    clamp_range(L.b_ptr, f, L.n_b, s.b0, s.nb);
    s.base = L.sim_ptr[f];
    const int64_t cells = (int64_t)s.na * s.nb;
    s.ok = s.base >= 0 && s.base <= L.sim_cells && cells <= L.sim_cells - s.base;
    return s;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ bool in_range(int v, int n) { return (unsigned)v < (unsigned)n; }

static inline bool sim_sizes_ok(int64_t n_a, int64_t n_b, int64_t n_frames, int64_t n_gt, int64_t n_tr) {
    return list_sizes_ok(n_a, n_frames, 0) && list_sizes_ok(n_b, n_frames, 0) && n_gt >= 0 && n_tr >= 0 && n_gt < (1LL << 31) && n_tr < (1LL << 31);
}
// blocks (of MT_THREADS threads) per frame for a stride loop over its cells: sized for the average frame, at most 64
static inline unsigned frame_blocks(int64_t sim_cells, int64_t n_frames) {
    const int64_t b = (sim_cells / n_frames + MT_THREADS - 1) / MT_THREADS;
    return (unsigned)(b < 1 ? 1 : (b > 64 ? 64 : b));
}
static inline Lists make_lists(const int32_t* a_ptr, int64_t n_a, const int32_t* b_ptr, int64_t n_b, const int64_t* sim_ptr, int64_t sim_cells,
                               int64_t n_frames) {
    Lists L = {a_ptr, b_ptr, sim_ptr, (int)n_a, (int)n_b, (int)n_frames, sim_cells};
    return L;
}

}  // namespace mpnhip
