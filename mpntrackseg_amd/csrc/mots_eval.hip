// The pixel work of the MOTS metrics (sMOTSA / IDF1, reference utils/evaluation.py:87-102 ->
// MOTChallengeEvalKit/MOTS/MOTS_metrics.py).  The kit decodes a run-length mask per object and intersects every
// ground-truth / prediction pair of a frame.  Masks of one MOTS frame are disjoint (mots_common/io.py:57-62 refuses anything
// else), so a frame is ONE label per pixel on either side -- the representation of full_masks.hip -- and every intersection of
// the frame is one cell of the joint histogram of the two label images:
//   paint_label_runs   runs -> label image (the inverse of mask_run_events)
//   label_overlap      two label images -> per-frame table [(na + 1) x (nb + 1)] of pixel counts
//   mots_frame_match   table -> the kit's per-object decisions (MOTS_metrics.py:251-273, :529-535) in exact integer form
// Integer atomics and integer compares only: the same bits on every call, and the bits of tests/mots_metrics_ref.py.
#include "device_prims.h"
#include "label_tables.h"

namespace mpnhip {
namespace {

constexpr int OV_THREADS = 256;
constexpr int OV_VEC_PER_THREAD = 8;   // 16-byte loads per thread (and image) a block is sized for
// a frame whose table has at most this many cells is counted in LDS: 16 KB a block, so eight blocks -- all 32 wavefronts --
// share a CU's 160 KB
constexpr int OV_LDS_CELLS = 4096;
constexpr int PAINT_THREADS = 256;

// ------------------------------------------------------------------------------------------------ paint
// length of every run (0 for a run that paints nothing) and the frame of its entry
__global__ void k_run_lengths(const int* __restrict__ run_entry, const int* __restrict__ run_begin, const int* __restrict__ run_end,
                              int64_t n_runs, const int* __restrict__ frame_ptr, int n_frames, int n_entries, int64_t hw,
                              int64_t* __restrict__ len, int* __restrict__ run_frame) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n_runs) return;
    if (r == n_runs) { len[r] = 0; return; }   // the scan's last slot: its offset is the total
    const int e = run_entry[r], b = run_begin[r], en = run_end[r];
    int f = -1;
    if (e >= 0 && e < n_entries && b >= 0 && b < en && (int64_t)en <= hw) f = frame_of(frame_ptr, n_frames, e);
    run_frame[r] = f;
    len[r] = f >= 0 ? (int64_t)(en - b) : 0;
}

// One painted pixel per thread and step: t counts the pixels of all runs in run order, its run is the last one whose
// offset is <= t (runs of length 0 own no t) -- one run of hw pixels and hw runs of one pixel cost the same.
__global__ __launch_bounds__(PAINT_THREADS) void k_paint_runs(const int* __restrict__ run_entry, const int* __restrict__ run_begin,
                                                               const int* __restrict__ run_frame, const int64_t* __restrict__ offsets,
                                                               int64_t n_runs, int64_t hw, int* __restrict__ labels) {
    const int64_t total = offsets[n_runs], stride = (int64_t)gridDim.x * PAINT_THREADS;
    for (int64_t t = (int64_t)blockIdx.x * PAINT_THREADS + threadIdx.x; t < total; t += stride) {
        int64_t lo = 0, hi = n_runs;   // first run with offsets[run] > t
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (offsets[mid] <= t) lo = mid + 1; else hi = mid;
        }
        const int64_t r = lo - 1;      // >= 0: offsets[0] = 0 <= t
        const int f = run_frame[r];
        const int64_t p = (int64_t)run_begin[r] + (t - offsets[r]);
        if (f >= 0 && p >= 0 && p < hw) labels[(int64_t)f * hw + p] = run_entry[r];
    }
}

struct PaintView { int64_t* len; int64_t* offsets; int* run_frame; void* tmp; size_t tmp_bytes; size_t bytes; };
static PaintView paint_view(void* workspace, int64_t n_runs) {
    Carver c(workspace);
    const size_t n = (size_t)n_runs + 1, tmp_bytes = exclusive_scan_temp<int64_t>(n_runs + 1);
    PaintView v = {c.take<int64_t>(n), c.take<int64_t>(n), c.take<int>(n), c.take<char>(tmp_bytes), tmp_bytes, 0};
    v.bytes = c.bytes();
    return v;
}

// ------------------------------------------------------------------------------------------------ overlap
// Grid (blocks of a frame, frames).  A frame is a scalar head (up to the first 16-byte boundary: f * hw need not be a multiple
// of 4), 16-byte vectors, a scalar tail.  The key of a pixel is its cell; key 0 -- no object on either side, the vast majority --
// is counted in a register.  Masks are runs along y, the direction of the memory: a thread's four pixels and the lanes next to
// it mostly share a key, so a wavefront first folds every maximal run of lanes whose four keys are all the same into ONE add
// (of 4 x the run's length, by its first lane); only the lanes on an object's border add pixel by pixel.  The adds go to the
// block's table in LDS where the frame's table fits (flushed once, non-zero cells only) and straight to memory where not;
// the choice depends on the frame alone, so it is the same for the whole block.
template <class Add>
__device__ __forceinline__ void add_pixel(int key, int& zeros, Add add) {
    if (key == 0) ++zeros; else add(key, 1);
}

__global__ __launch_bounds__(OV_THREADS) void k_label_overlap(const int* __restrict__ labels_a, const int* __restrict__ labels_b,
                                                              const int* __restrict__ a_ptr, const int* __restrict__ b_ptr,
                                                              const int64_t* __restrict__ table_ptr, int n_a, int n_b, int64_t hw,
                                                              int64_t table_cells, int* __restrict__ table) {
    __shared__ int s_tab[OV_LDS_CELLS];
    __shared__ int s_zeros;
    const int t = threadIdx.x, lane = t & 63, f = blockIdx.y;
    const FrameTab ft = frame_tab(a_ptr, b_ptr, table_ptr, f, n_a, n_b, table_cells);
    if (!ft.ok) return;   // (block-uniform)
    const int cells = (int)((int64_t)(ft.na + 1) * (ft.nb + 1)), nb1 = ft.nb + 1;   // cells <= table_cells < 2^31
    const bool lds = cells <= OV_LDS_CELLS;
    int* __restrict__ out = table + ft.base;
    if (lds)
        for (int c = t; c < cells; c += OV_THREADS) s_tab[c] = 0;
    if (t == 0) s_zeros = 0;
    __syncthreads();

    auto add = [&](int key, int n) {
        if (lds) atomicAdd(&s_tab[key], n); else atomicAdd(&out[key], n);
    };
    auto key_of = [&](int la, int lb) {
        const unsigned ia = (unsigned)(la - ft.a0), ib = (unsigned)(lb - ft.b0);   // one compare for both ends of the range
        const int ra = ia < (unsigned)ft.na ? (int)ia + 1 : 0, rb = ib < (unsigned)ft.nb ? (int)ib + 1 : 0;
        return ra * nb1 + rb;
    };

    const int64_t start = (int64_t)f * hw;
    const int* __restrict__ pa = labels_a + start;
    const int* __restrict__ pb = labels_b + start;
    int64_t head = (4 - (start & 3)) & 3;   // both images start on a 16-byte boundary (checked by the host)
    head = head < hw ? head : hw;
    const int64_t nvec = (hw - head) >> 2, tail0 = head + (nvec << 2);
    int zeros = 0;
    if (blockIdx.x == 0) {
        if (t < head) add_pixel(key_of(pa[t], pb[t]), zeros, add);
        if (t >= 64 && tail0 + (t - 64) < hw) add_pixel(key_of(pa[tail0 + (t - 64)], pb[tail0 + (t - 64)]), zeros, add);
    }

    const int4* __restrict__ va = reinterpret_cast<const int4*>(pa + head);
    const int4* __restrict__ vb = reinterpret_cast<const int4*>(pb + head);
    const int64_t step = (int64_t)gridDim.x * OV_THREADS;
    const int64_t iters = (nvec + step - 1) / step;   // the same for every thread: the ballots below see whole wavefronts
    int64_t v = (int64_t)blockIdx.x * OV_THREADS + t;
    const int4 none = make_int4(-1, -1, -1, -1);
    int4 a_next = none, b_next = none;
    if (iters > 0 && v < nvec) { a_next = va[v]; b_next = vb[v]; }
    for (int64_t it = 0; it < iters; ++it, v += step) {
        const int4 a = a_next, b = b_next;
        const bool active = v < nvec;
        if (it + 1 < iters && v + step < nvec) { a_next = va[v + step]; b_next = vb[v + step]; }
        const int k0 = key_of(a.x, b.x), k1 = key_of(a.y, b.y), k2 = key_of(a.z, b.z), k3 = key_of(a.w, b.w);
        const bool same = active && k0 == k1 && k0 == k2 && k0 == k3;
        const unsigned long long same_bits = __ballot(same);
        const int k_prev = __shfl_up(k0, 1);
        const bool prev_same = lane > 0 && ((same_bits >> (lane - 1)) & 1ull);
        const bool run_head = !same || !prev_same || k_prev != k0;
        const unsigned long long heads = __ballot(run_head);
        if (same) {
            if (run_head) {
                const unsigned long long later = lane < 63 ? (heads >> (lane + 1)) << (lane + 1) : 0ull;
                const int end = later ? __ffsll((long long)later) - 1 : 64;
                const int n = 4 * (end - lane);
                if (k0 == 0) zeros += n; else add(k0, n);
            }
        } else if (active) {
            add_pixel(k0, zeros, add);
            add_pixel(k1, zeros, add);
            add_pixel(k2, zeros, add);
            add_pixel(k3, zeros, add);
        }
    }

    // the pixels without an object: one add per wavefront to the block's counter, one per block to the table
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) zeros += __shfl_xor(zeros, o);
    if (lane == 0 && zeros) atomicAdd(&s_zeros, zeros);
    __syncthreads();
    if (t == 0 && s_zeros) atomicAdd(&out[0], s_zeros);
    if (lds)
        for (int c = t; c < cells; c += OV_THREADS) {
            const int n = s_tab[c];
            if (n) atomicAdd(&out[c], n);
        }
}

// ------------------------------------------------------------------------------------------------ match
// one wavefront per a-entry over the frame's b-entries.  i = cell, u = A + B - i:
//   2 i > u            c > 0.5 of MOTS_metrics.py:253-254: the CLEAR match (at most one b: the b-masks are disjoint)
//   2 i >= u, u > 0    not (overlap < 0.5) of :529-535: one more frame the two trajectories share
__global__ __launch_bounds__(MT_THREADS) void k_frame_match(const int* __restrict__ table, const int64_t* __restrict__ table_ptr,
                                                            const int* __restrict__ a_ptr, const int* __restrict__ b_ptr, int n_frames,
                                                            int n_a, int n_b, int64_t table_cells, const unsigned char* __restrict__ a_ignore,
                                                            const int* __restrict__ a_traj, const int* __restrict__ b_traj, int n_a_traj,
                                                            int n_b_traj, const int* __restrict__ a_area, const int* __restrict__ b_area,
                                                            int* __restrict__ match_b, int* __restrict__ inter, int* __restrict__ uni,
                                                            unsigned char* __restrict__ b_matched, int* __restrict__ id_match) {
    const int a = blockIdx.x * MT_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (a >= n_a) return;
    int best_b = -1, best_i = 0, best_u = 0;
    const int f = frame_of(a_ptr, n_frames, a);
    if (f >= 0 && !a_ignore[a]) {
        const FrameTab ft = frame_tab(a_ptr, b_ptr, table_ptr, f, n_a, n_b, table_cells);
        const int ia = a - ft.a0;
        if (ft.ok && ia >= 0 && ia < ft.na) {
            const int* __restrict__ row = table + ft.base + (int64_t)(ia + 1) * (ft.nb + 1);
            const long long A = a_area[a];
            const int ta = a_traj[a];
            for (int c = lane; c < ft.nb; c += 64) {
                const long long i = row[c + 1], u = A + (long long)b_area[ft.b0 + c] - i;
                if (2 * i > u && best_b < 0) { best_b = ft.b0 + c; best_i = (int)i; best_u = (int)u; }
                if (2 * i >= u && u > 0) {
                    const int tb = b_traj[ft.b0 + c];
                    if (ta >= 0 && ta < n_a_traj && tb >= 0 && tb < n_b_traj) atomicAdd(&id_match[(int64_t)ta * n_b_traj + tb], 1);
                }
            }
        }
    }
    // the first lane that found one (there is at most one among disjoint masks)
    const unsigned long long found = __ballot(best_b >= 0);
    const int src = found ? __ffsll((long long)found) - 1 : 0;
    best_b = __shfl(best_b, src);
    best_i = __shfl(best_i, src);
    best_u = __shfl(best_u, src);
    if (lane == 0) {
        match_b[a] = best_b;
        inter[a] = best_i;
        uni[a] = best_u;
        if (best_b >= 0) b_matched[best_b] = 1;
    }
}

struct MatchView { int* a_area; size_t bytes; };
static MatchView match_view(void* workspace, int64_t n_a) {
    Carver c(workspace);
    MatchView v = {c.take<int>((size_t)n_a), 0};
    v.bytes = c.bytes();
    return v;
}

}  // namespace
}  // namespace mpnhip

using namespace mpnhip;

extern "C" size_t mpnhip_mots_workspace_bytes(int64_t n_runs, int64_t n_a, int64_t n_b, int64_t n_frames, int64_t hw) {
    if (n_runs < 0 || n_runs >= (1LL << 30) || !list_sizes_ok(n_a, n_frames, hw) || !list_sizes_ok(n_b, n_frames, hw)) return 0;
    const size_t paint = n_runs > 0 ? paint_view(nullptr, n_runs).bytes : 0;
    const size_t match = n_a > 0 ? match_view(nullptr, n_a).bytes : 0;   // (label_overlap needs none)
    const size_t need = paint > match ? paint : match;
    return need ? need + 256 : 0;
}

extern "C" int mpnhip_paint_label_runs(const int32_t* run_entry, const int32_t* run_begin, const int32_t* run_end, int64_t n_runs,
                                       const int32_t* frame_ptr, int64_t n_entries, int64_t n_frames, int64_t hw, int32_t* labels,
                                       void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(n_runs >= 0 && n_runs < (1LL << 30) && list_sizes_ok(n_entries, n_frames, hw),
                  "paint_label_runs: bad sizes (H * W must stay below 2^31, at most 65535 frames per call)");
    if (n_frames == 0 || hw == 0) return MPNHIP_OK;
    MPN_CHECK_ARG(labels && frame_ptr, "paint_label_runs: null labels / frame_ptr");
    MPN_CHECK_ARG(n_runs == 0 || (run_entry && run_begin && run_end), "paint_label_runs: null runs");
    PaintView v = paint_view(workspace, n_runs);
    if (n_runs > 0) MPN_CHECK_WORKSPACE("paint_label_runs", workspace, workspace_bytes, v.bytes);
    MPN_HIP(hipMemsetAsync(labels, 0xFF, (size_t)(n_frames * hw) * 4, stream));
    if (n_runs == 0) return MPNHIP_OK;
    hipLaunchKernelGGL(k_run_lengths, dim3(blocks_for(n_runs + 1)), dim3(256), 0, stream, run_entry, run_begin, run_end, n_runs, frame_ptr,
                       (int)n_frames, (int)n_entries, hw, v.len, v.run_frame);
    MPN_LAUNCH_CHECK();
    MPN_HIP(rocprim::exclusive_scan(v.tmp, v.tmp_bytes, v.len, v.offsets, (int64_t)0, (size_t)(n_runs + 1), rocprim::plus<int64_t>(), stream));
    // the number of painted pixels stays on the device: a grid for an image without overlapping runs, and a stride loop
    hipLaunchKernelGGL(k_paint_runs, dim3(stream_blocks(n_frames * hw)), dim3(PAINT_THREADS), 0, stream, run_entry, run_begin, v.run_frame,
                       v.offsets, n_runs, hw, labels);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}

extern "C" int mpnhip_label_overlap(const int32_t* labels_a, const int32_t* labels_b, const int32_t* a_ptr, int64_t n_a,
                                    const int32_t* b_ptr, int64_t n_b, const int64_t* table_ptr, const int64_t* table_ptr_host,
                                    int64_t n_frames, int64_t hw, int32_t* table, int64_t table_cells, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(list_sizes_ok(n_a, n_frames, hw) && list_sizes_ok(n_b, n_frames, hw) && table_cells >= 0,
                  "label_overlap: bad sizes (H * W must stay below 2^31, at most 65535 frames per call)");
    if (table_cells >= (1LL << 31)) {
        set_error("label_overlap: a table of %lld cells (2^31 or more) is not supported: fewer frames per call", (long long)table_cells);
        return MPNHIP_ERR_UNSUPPORTED;
    }
    // (every check before the first HIP call)
    const bool work = n_frames > 0 && hw > 0 && table_cells > 0;
    MPN_CHECK_ARG(table_cells == 0 || table, "label_overlap: null table");
    MPN_CHECK_ARG(!work || (labels_a && labels_b && a_ptr && b_ptr && table_ptr), "label_overlap: null pointer");
    MPN_CHECK_ARG(!work || (aligned16(labels_a) && aligned16(labels_b)), "label_overlap: the label images must start on a 16-byte boundary");
    if (table_cells > 0) MPN_HIP(hipMemsetAsync(table, 0, (size_t)table_cells * 4, stream));
    if (!work) return MPNHIP_OK;
    if (table_ptr_host)
        for (int64_t f = 0; f < n_frames; ++f) {
            const int64_t cells = table_ptr_host[f + 1] - table_ptr_host[f];
            if (cells > 0) count_path(cells <= OV_LDS_CELLS ? PC_LABEL_OVERLAP_LDS : PC_LABEL_OVERLAP_GLOBAL);
        }
    const int64_t nvec = hw / 4, per_block = (int64_t)OV_THREADS * OV_VEC_PER_THREAD;
    int64_t bx = (nvec + per_block - 1) / per_block, cap = (int64_t)stream_blocks(1LL << 40) / n_frames;
    cap = cap < 1 ? 1 : cap;
    bx = bx < 1 ? 1 : (bx > cap ? cap : bx);
    hipLaunchKernelGGL(k_label_overlap, dim3((unsigned)bx, (unsigned)n_frames), dim3(OV_THREADS), 0, stream, labels_a, labels_b, a_ptr, b_ptr,
                       table_ptr, (int)n_a, (int)n_b, hw, table_cells, table);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}

extern "C" int mpnhip_mots_frame_match(const int32_t* table, int64_t table_cells, const int64_t* table_ptr, const int32_t* a_ptr, int64_t n_a,
                                       const int32_t* b_ptr, int64_t n_b, int64_t n_frames, const unsigned char* a_ignore,
                                       const int32_t* a_traj, const int32_t* b_traj, int64_t n_a_traj, int64_t n_b_traj, int32_t* match_b,
                                       int32_t* inter, int32_t* uni, unsigned char* b_matched, unsigned char* b_ignored, int32_t* b_area,
                                       int32_t* id_match, void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(list_sizes_ok(n_a, n_frames, 0) && list_sizes_ok(n_b, n_frames, 0) && table_cells >= 0 && n_a_traj >= 0 && n_b_traj >= 0 &&
                  n_a_traj < (1LL << 31) && n_b_traj < (1LL << 31), "mots_frame_match: bad sizes");
    if (table_cells >= (1LL << 31) || n_a_traj * n_b_traj >= (1LL << 31)) {
        set_error("mots_frame_match: a table of %lld cells or an id_match of %lld x %lld (2^31 or more) is not supported",
                  (long long)table_cells, (long long)n_a_traj, (long long)n_b_traj);
        return MPNHIP_ERR_UNSUPPORTED;
    }
    // (every check before the first HIP call)
    const bool work = n_a > 0 || n_b > 0;
    MPN_CHECK_ARG(n_a_traj * n_b_traj == 0 || id_match, "mots_frame_match: null id_match");
    MPN_CHECK_ARG(!work || (n_frames > 0 && a_ptr && b_ptr && table_ptr && table), "mots_frame_match: entries without frames / null table or lists");
    MPN_CHECK_ARG(n_a == 0 || (a_ignore && a_traj && match_b && inter && uni), "mots_frame_match: null a-side array");
    MPN_CHECK_ARG(n_b == 0 || (b_traj && b_matched && b_ignored && b_area), "mots_frame_match: null b-side array");
    MatchView v = match_view(workspace, n_a);
    if (n_a > 0) MPN_CHECK_WORKSPACE("mots_frame_match", workspace, workspace_bytes, v.bytes);
    if (n_a_traj * n_b_traj > 0) MPN_HIP(hipMemsetAsync(id_match, 0, (size_t)(n_a_traj * n_b_traj) * 4, stream));
    if (!work) return MPNHIP_OK;
    const unsigned a_blocks = (unsigned)((n_a + MT_WAVES - 1) / MT_WAVES);
    if (n_a > 0) {
        hipLaunchKernelGGL(k_row_sums, dim3(a_blocks), dim3(MT_THREADS), 0, stream, table, table_ptr, a_ptr, b_ptr, (int)n_frames, (int)n_a,
                           (int)n_b, table_cells, v.a_area);
        MPN_LAUNCH_CHECK();
    }
    if (n_b > 0) {
        hipLaunchKernelGGL(k_col_sums, dim3(blocks_for(n_b)), dim3(256), 0, stream, table, table_ptr, a_ptr, b_ptr, (int)n_frames, (int)n_a,
                           (int)n_b, table_cells, a_ignore, b_area, b_ignored, b_matched);
        MPN_LAUNCH_CHECK();
    }
    if (n_a > 0) {
        hipLaunchKernelGGL(k_frame_match, dim3(a_blocks), dim3(MT_THREADS), 0, stream, table, table_ptr, a_ptr, b_ptr, (int)n_frames,
                           (int)n_a, (int)n_b, table_cells, a_ignore, a_traj, b_traj, (int)n_a_traj, (int)n_b_traj, v.a_area, b_area, match_b,
                           inter, uni, b_matched, id_match);
        MPN_LAUNCH_CHECK();
    }
    return MPNHIP_OK;
}
