// HOTA of a KITTI-MOTS sequence (reference utils/evaluation.py:127-135 -> TrackEval: datasets/kitti_mots.py:299-387 and
// metrics/hota.py:25-117) from the per-frame tables of mpnhip_label_overlap.  What the kit does with three Python loops over
// frames and 19 dense [num_gt_ids, num_tracker_ids] matrices:
//   hota_frame_similarity      table -> the IoU block of every frame, the predictions the preprocessing removes, the kept sums
//   hota_accumulate_alignment  + one launch's sim_iou into potential[G, T], + its presence counts
//   hota_frame_scores          global alignment score x similarity: the cells of the host's assignment problems
//   hota_alpha_accumulate      the host's assignment -> TP, the LocA sums and matches_count per alpha
//   hota_association           matches_count -> the AssA / AssRe / AssPr numerators per alpha
// The same bits on every call: integer atomics only; a double sum is one thread walking the frames in order (potential, LocA)
// or a tree whose shape depends on the sizes alone.  An entry is KEPT when its trajectory index is in range (the host gives
// -1 to ignore rows and to predictions of another class) and, on the b-side, the preprocessing did not remove it.
#include <cfloat>
#include <climits>

#include "sim_lists.h"

namespace mpnhip {
namespace {

constexpr int N_ALPHA = MPNHIP_HOTA_ALPHAS;
constexpr int HT_THREADS = MT_THREADS, HT_WAVES = HT_THREADS / 64;
constexpr int AS_CELLS_PER_BLOCK = 1024, AS_MAX_BLOCKS = 256;   // association: blocks per alpha = f(G * T) alone
constexpr double EPS = DBL_EPSILON;                            // np.finfo('float').eps

struct Alphas { double v[N_ALPHA]; };

// ------------------------------------------------------------------------------------------------ similarity
// One wavefront per a-entry: its row of the similarity block (0 in the row of an ignore entry and in the column of a
// prediction that is not scored) and the first column it is eligible with -- i > 0 and 2 i >= u, the complement of
// kitti_mots.py:329's "< 0.5 - eps" -- which is the prediction the kit's assignment matches with it.
__global__ __launch_bounds__(HT_THREADS) void k_hota_rows(const int* __restrict__ table, const int64_t* __restrict__ table_ptr,
                                                          int64_t table_cells, Lists L, const unsigned char* __restrict__ a_ignore,
                                                          const unsigned char* __restrict__ b_scored, const int* __restrict__ a_area,
                                                          const int* __restrict__ b_area, double* __restrict__ sim,
                                                          unsigned char* __restrict__ b_matched) {
    const int a = blockIdx.x * HT_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (a >= L.n_a) return;
    const int f = frame_of(L.a_ptr, L.n_frames, a);
    if (f < 0) return;
    const FrameTab ft = frame_tab(L.a_ptr, L.b_ptr, table_ptr, f, L.n_a, L.n_b, table_cells);
    const FrameSim fs = frame_sim(L, f);
    const int ia = a - fs.a0;
    if (!ft.ok || !fs.ok || ia < 0 || ia >= fs.na) return;   // (wavefront-uniform)
    const int* __restrict__ row = table + ft.base + (int64_t)(ia + 1) * (ft.nb + 1);
    double* __restrict__ out = sim + fs.base + (int64_t)ia * fs.nb;
    const bool object = !a_ignore[a];
    const long long A = a_area[a];
    int first = INT_MAX;
    for (int c = lane; c < fs.nb; c += 64) {
        const long long i = row[c + 1], u = A + (long long)b_area[fs.b0 + c] - i;
        const bool pair = object && b_scored[fs.b0 + c] && i > 0;
        out[c] = pair ? (double)i / (double)u : 0.0;
        if (pair && 2 * i >= u && c < first) first = c;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o));
    if (lane == 0 && first != INT_MAX) b_matched[fs.b0 + first] = 1;   // (two rows may share it: both store 1)
}

// one thread per b-entry: removed (kitti_mots.py:336-344) iff scored, unmatched and more than half inside the ignore region;
// the column sum of a kept entry, rows in order
__global__ void k_hota_cols(Lists L, const unsigned char* __restrict__ b_scored, const unsigned char* __restrict__ b_matched,
                            const unsigned char* __restrict__ b_in_ignore, const double* __restrict__ sim,
                            unsigned char* __restrict__ b_removed, double* __restrict__ col_sum) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= L.n_b) return;
    const bool scored = b_scored[b] != 0, removed = scored && !b_matched[b] && b_in_ignore[b];
    double sum = 0.0;
    const int f = frame_of(L.b_ptr, L.n_frames, b);
    if (f >= 0 && scored && !removed) {
        const FrameSim fs = frame_sim(L, f);
        const int ib = b - fs.b0;
        if (fs.ok && ib >= 0 && ib < fs.nb)
            for (int r = 0; r < fs.na; ++r) sum += sim[fs.base + (int64_t)r * fs.nb + ib];
    }
    b_removed[b] = removed ? 1 : 0;
    col_sum[b] = sum;
}

// one wavefront per a-entry: the row sum over the kept columns (a lane's columns in order, then the wavefront's tree)
__global__ __launch_bounds__(HT_THREADS) void k_hota_row_sums(Lists L, const unsigned char* __restrict__ b_removed,
                                                              const double* __restrict__ sim, double* __restrict__ row_sum) {
    const int a = blockIdx.x * HT_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (a >= L.n_a) return;
    double sum = 0.0;
    const int f = frame_of(L.a_ptr, L.n_frames, a);
    if (f >= 0) {
        const FrameSim fs = frame_sim(L, f);
        const int ia = a - fs.a0;
        if (fs.ok && ia >= 0 && ia < fs.na) {
            const double* __restrict__ row = sim + fs.base + (int64_t)ia * fs.nb;
            for (int c = lane; c < fs.nb; c += 64)
                if (!b_removed[fs.b0 + c]) sum += row[c];
        }
    }
    sum = wave_sum_f64(sum);
    if (lane == 0) row_sum[a] = sum;
}

// ------------------------------------------------------------------------------------------------ alignment
// one thread per entry of either list: where its trajectory is in the frame (map [n_frames, n_traj], -1 elsewhere) and one
// more frame the trajectory is present in.  Two entries of one trajectory in a frame are the caller's error: one of them stays.
__global__ void k_hota_entry_maps(Lists L, const int* __restrict__ a_traj, const int* __restrict__ b_traj,
                                  const unsigned char* __restrict__ b_removed, int n_gt, int n_tr, int* __restrict__ map_a,
                                  int* __restrict__ map_b, int* __restrict__ gt_count, int* __restrict__ tr_count) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < L.n_a) {
        const int f = frame_of(L.a_ptr, L.n_frames, e), g = a_traj[e];
        if (f >= 0 && in_range(g, n_gt)) {
            map_a[(int64_t)f * n_gt + g] = e;
            atomicAdd(&gt_count[g], 1);
        }
    } else if (e - L.n_a < L.n_b) {
        const int b = e - L.n_a, f = frame_of(L.b_ptr, L.n_frames, b), t = b_traj[b];
        if (f >= 0 && in_range(t, n_tr) && !b_removed[b]) {
            map_b[(int64_t)f * n_tr + t] = b;
            atomicAdd(&tr_count[t], 1);
        }
    }
}

// One thread per (g, t): a cell receives at most one sim_iou per frame (hota.py:56-61), so the thread walks the launch's frames
// in order -- the sum has the same order whatever the launches are.
__global__ void k_hota_alignment(Lists L, const double* __restrict__ sim, const double* __restrict__ row_sum,
                                 const double* __restrict__ col_sum, const int* __restrict__ map_a, const int* __restrict__ map_b,
                                 int n_gt, int n_tr, double* __restrict__ potential) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= (int64_t)n_gt * n_tr) return;
    const int g = (int)(c / n_tr), t = (int)(c % n_tr);
    double pot = potential[c];
    for (int f = 0; f < L.n_frames; ++f) {
        const int a = map_a[(int64_t)f * n_gt + g], b = map_b[(int64_t)f * n_tr + t];
        if (a < 0 || b < 0) continue;
        const FrameSim fs = frame_sim(L, f);
        const int ia = a - fs.a0, ib = b - fs.b0;
        if (!fs.ok || !in_range(ia, fs.na) || !in_range(ib, fs.nb)) continue;
        const double s = sim[fs.base + (int64_t)ia * fs.nb + ib];
        const double den = (col_sum[b] + row_sum[a]) - s;
        if (den > 0 + EPS) pot += s / den;
    }
    potential[c] = pot;
}

// ------------------------------------------------------------------------------------------------ scores
// grid (blocks of a frame, frames): score = gas[g, t] * sim (hota.py:68, :85) for a kept pair, 0 elsewhere
__global__ __launch_bounds__(HT_THREADS) void k_hota_scores(Lists L, const double* __restrict__ sim, const int* __restrict__ a_traj,
                                                            const int* __restrict__ b_traj, const unsigned char* __restrict__ b_removed,
                                                            int n_gt, int n_tr, const double* __restrict__ potential,
                                                            const int* __restrict__ gt_count, const int* __restrict__ tr_count,
                                                            double* __restrict__ score) {
    const FrameSim fs = frame_sim(L, blockIdx.y);
    if (!fs.ok || fs.nb == 0) return;
    const int64_t cells = (int64_t)fs.na * fs.nb;
    for (int64_t c = (int64_t)blockIdx.x * HT_THREADS + threadIdx.x; c < cells; c += (int64_t)gridDim.x * HT_THREADS) {
        const int a = fs.a0 + (int)(c / fs.nb), b = fs.b0 + (int)(c % fs.nb);
        const int g = a_traj[a], t = b_traj[b];
        double v = 0.0;
        if (in_range(g, n_gt) && in_range(t, n_tr) && !b_removed[b]) {
            const double p = potential[(int64_t)g * n_tr + t];
            const double den = ((double)gt_count[g] + (double)tr_count[t]) - p;
            if (den > 0.0) v = (p / den) * sim[fs.base + c];
        }
        score[fs.base + c] = v;
    }
}

// ------------------------------------------------------------------------------------------------ alphas
// One block per frame.  A thread's a-entries: the matched pair's similarity against every alpha (hota.py:91-101).  The frame's
// LocA sums go through the block's tree into frame_loca [n_frames, N_ALPHA]; k_hota_fold adds them in frame order.
__global__ __launch_bounds__(HT_THREADS) void k_hota_alphas(Lists L, const double* __restrict__ sim, const int* __restrict__ a_traj,
                                                            const int* __restrict__ b_traj, const unsigned char* __restrict__ b_removed,
                                                            const int* __restrict__ match_b, int n_gt, int n_tr, Alphas alphas,
                                                            unsigned long long* __restrict__ tp, int* __restrict__ matches_count,
                                                            double* __restrict__ frame_loca) {
    __shared__ double s_loca[HT_WAVES][N_ALPHA];
    __shared__ int s_tp[HT_WAVES][N_ALPHA];
    const int f = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const FrameSim fs = frame_sim(L, f);
    double loca[N_ALPHA];
    int n[N_ALPHA];
#pragma unroll
    for (int k = 0; k < N_ALPHA; ++k) { loca[k] = 0.0; n[k] = 0; }
    if (fs.ok)
        for (int ia = threadIdx.x; ia < fs.na; ia += HT_THREADS) {
            const int a = fs.a0 + ia, g = a_traj[a], b = match_b[a];
            const unsigned ib = (unsigned)b - (unsigned)fs.b0;   // (whatever the host sent: inside the frame's entries or nothing)
            if (!in_range(g, n_gt) || ib >= (unsigned)fs.nb) continue;
            const int t = b_traj[b];
            if (!in_range(t, n_tr) || b_removed[b]) continue;
            const double s = sim[fs.base + (int64_t)ia * fs.nb + ib];
            int* __restrict__ mc = matches_count + (int64_t)g * n_tr + t;
#pragma unroll
            for (int k = 0; k < N_ALPHA; ++k)
                if (s >= alphas.v[k] - EPS) {
                    loca[k] += s;
                    ++n[k];
                    atomicAdd(mc + (int64_t)k * n_gt * n_tr, 1);
                }
        }
#pragma unroll
    for (int k = 0; k < N_ALPHA; ++k) {
        const double v = wave_sum_f64(loca[k]);
        const int m = wave_sum(n[k]);
        if (lane == 0) { s_loca[wave][k] = v; s_tp[wave][k] = m; }
    }
    __syncthreads();
    if (threadIdx.x < N_ALPHA) {
        const int k = threadIdx.x;
        double v = s_loca[0][k];
        int m = s_tp[0][k];
        for (int w = 1; w < HT_WAVES; ++w) { v += s_loca[w][k]; m += s_tp[w][k]; }
        frame_loca[(int64_t)f * N_ALPHA + k] = v;
        if (m) atomicAdd(&tp[k], (unsigned long long)m);
    }
}

__global__ void k_hota_fold(const double* __restrict__ frame_loca, int n_frames, double* __restrict__ loca) {
    const int k = threadIdx.x;
    if (k >= N_ALPHA) return;
    double v = loca[k];
    for (int f = 0; f < n_frames; ++f) v += frame_loca[(int64_t)f * N_ALPHA + k];
    loca[k] = v;
}

// ------------------------------------------------------------------------------------------------ association
// grid (blocks, alphas): a block's cells of matches_count[k] (stride = the grid) -> partial [N_ALPHA, blocks, 3]: the sums of
// mc * mc / max(1, gt_count + tr_count - mc), mc * mc / max(1, gt_count) and mc * mc / max(1, tr_count) (hota.py:105-112)
__global__ __launch_bounds__(HT_THREADS) void k_hota_association(const int* __restrict__ matches_count, const int* __restrict__ gt_count,
                                                                 const int* __restrict__ tr_count, int n_gt, int n_tr,
                                                                 double* __restrict__ partial) {
    __shared__ double s_sum[HT_WAVES][3];
    const int k = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t cells = (int64_t)n_gt * n_tr;
    const int* __restrict__ mc = matches_count + (int64_t)k * cells;
    double ass = 0.0, re = 0.0, pr = 0.0;
    for (int64_t c = (int64_t)blockIdx.x * HT_THREADS + threadIdx.x; c < cells; c += (int64_t)gridDim.x * HT_THREADS) {
        const int m_ = mc[c];
        if (m_ == 0) continue;
        const double m = (double)m_, gc = (double)gt_count[c / n_tr], tc = (double)tr_count[c % n_tr];
        ass += m * (m / fmax(1.0, (gc + tc) - m));
        re += m * (m / fmax(1.0, gc));
        pr += m * (m / fmax(1.0, tc));
    }
    ass = wave_sum_f64(ass);
    re = wave_sum_f64(re);
    pr = wave_sum_f64(pr);
    if (lane == 0) { s_sum[wave][0] = ass; s_sum[wave][1] = re; s_sum[wave][2] = pr; }
    __syncthreads();
    if (threadIdx.x < 3) {
        double v = s_sum[0][threadIdx.x];
        for (int w = 1; w < HT_WAVES; ++w) v += s_sum[w][threadIdx.x];
        partial[((int64_t)k * gridDim.x + blockIdx.x) * 3 + threadIdx.x] = v;
    }
}

// one wavefront per alpha: a lane's partials in order, then the wavefront's tree
__global__ __launch_bounds__(64) void k_hota_association_fold(const double* __restrict__ partial, int n_blocks, double* __restrict__ out) {
    const int k = blockIdx.x, lane = threadIdx.x;
    double v[3] = {0.0, 0.0, 0.0};
    for (int b = lane; b < n_blocks; b += 64)
        for (int j = 0; j < 3; ++j) v[j] += partial[((int64_t)k * n_blocks + b) * 3 + j];
    for (int j = 0; j < 3; ++j) {
        const double s = wave_sum_f64(v[j]);
        if (lane == 0) out[k * 3 + j] = s;
    }
}

// ------------------------------------------------------------------------------------------------ workspaces
static int association_blocks(int64_t cells) {
    const int64_t b = (cells + AS_CELLS_PER_BLOCK - 1) / AS_CELLS_PER_BLOCK;
    return (int)(b < 1 ? 1 : (b > AS_MAX_BLOCKS ? AS_MAX_BLOCKS : b));
}

struct SimView { int* a_area; int* b_area; unsigned char* b_in_ignore; unsigned char* b_matched; size_t bytes; };
static SimView sim_view(void* workspace, int64_t n_a, int64_t n_b) {
    Carver c(workspace);
    SimView v = {c.take<int>((size_t)n_a), c.take<int>((size_t)n_b), c.take<unsigned char>((size_t)n_b), c.take<unsigned char>((size_t)n_b), 0};
    v.bytes = c.bytes();
    return v;
}
struct MapView { int* map_a; int* map_b; size_t map_bytes; size_t bytes; };   // (the two maps are one stretch: one memset)
static MapView map_view(void* workspace, int64_t n_frames, int64_t n_gt, int64_t n_tr) {
    Carver c(workspace);
    MapView v = {c.take<int>((size_t)(n_frames * n_gt)), c.take<int>((size_t)(n_frames * n_tr)), 0, 0};
    v.map_bytes = v.bytes = c.bytes();
    return v;
}
struct AlphaView { double* frame_loca; size_t bytes; };
static AlphaView alpha_view(void* workspace, int64_t n_frames) {
    Carver c(workspace);
    AlphaView v = {c.take<double>((size_t)n_frames * N_ALPHA), 0};
    v.bytes = c.bytes();
    return v;
}
struct AssView { double* partial; size_t bytes; };
static AssView ass_view(void* workspace, int64_t cells) {
    Carver c(workspace);
    AssView v = {c.take<double>((size_t)N_ALPHA * association_blocks(cells) * 3), 0};
    v.bytes = c.bytes();
    return v;
}

// the int32 matches_count [N_ALPHA, G, T] and the per-frame maps [n_frames, G] / [n_frames, T] are indexed below 2^31
static bool hota_supported(int64_t n_frames, int64_t n_gt, int64_t n_tr) {
    return n_gt * n_tr * N_ALPHA < (1LL << 31) && n_frames * (n_gt + n_tr) < (1LL << 31);
}
static int refuse_unsupported(const char* name, int64_t n_frames, int64_t n_gt, int64_t n_tr) {
    set_error("%s: %lld x %lld trajectories x %d alphas, or %lld frames x %lld trajectories (2^31 cells or more) is not supported", name,
              (long long)n_gt, (long long)n_tr, N_ALPHA, (long long)n_frames, (long long)(n_gt + n_tr));
    return MPNHIP_ERR_UNSUPPORTED;
}

static unsigned wave_blocks(int64_t n) { return (unsigned)((n + HT_WAVES - 1) / HT_WAVES); }

}  // namespace
}  // namespace mpnhip

using namespace mpnhip;

extern "C" size_t mpnhip_hota_workspace_bytes(int64_t n_a, int64_t n_b, int64_t n_frames, int64_t n_gt_ids, int64_t n_tr_ids) {
    if (!sim_sizes_ok(n_a, n_b, n_frames, n_gt_ids, n_tr_ids) || !hota_supported(n_frames, n_gt_ids, n_tr_ids)) return 0;
    size_t need = sim_view(nullptr, n_a, n_b).bytes;
    const size_t others[3] = {map_view(nullptr, n_frames, n_gt_ids, n_tr_ids).bytes, alpha_view(nullptr, n_frames).bytes,
                              ass_view(nullptr, n_gt_ids * n_tr_ids).bytes};
    for (size_t o : others) need = o > need ? o : need;
    return need + 256;
}

extern "C" int mpnhip_hota_frame_similarity(const int32_t* table, int64_t table_cells, const int64_t* table_ptr, const int32_t* a_ptr,
                                            int64_t n_a, const int32_t* b_ptr, int64_t n_b, int64_t n_frames,
                                            const unsigned char* a_ignore, const unsigned char* b_scored, const int64_t* sim_ptr,
                                            int64_t sim_cells, double* sim, unsigned char* b_removed, double* row_sum, double* col_sum,
                                            void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(sim_sizes_ok(n_a, n_b, n_frames, 0, 0) && table_cells >= 0 && sim_cells >= 0, "hota_frame_similarity: bad sizes");
    if (table_cells >= (1LL << 31) || sim_cells >= (1LL << 31)) {
        set_error("hota_frame_similarity: a table of %lld cells (2^31 or more) is not supported: fewer frames per call", (long long)table_cells);
        return MPNHIP_ERR_UNSUPPORTED;
    }
    // (every check before the first HIP call)
    const bool work = n_a > 0 || n_b > 0;
    MPN_CHECK_ARG(sim_cells == 0 || sim, "hota_frame_similarity: null sim");
    MPN_CHECK_ARG(!work || (n_frames > 0 && a_ptr && b_ptr && table_ptr && sim_ptr && table),
                  "hota_frame_similarity: entries without frames / null table or lists");
    MPN_CHECK_ARG(n_a == 0 || (a_ignore && row_sum), "hota_frame_similarity: null a-side array");
    MPN_CHECK_ARG(n_b == 0 || (b_scored && b_removed && col_sum), "hota_frame_similarity: null b-side array");
    SimView v = sim_view(workspace, n_a, n_b);
    if (work) MPN_CHECK_WORKSPACE("hota_frame_similarity", workspace, workspace_bytes, v.bytes);
    if (sim_cells > 0) MPN_HIP(hipMemsetAsync(sim, 0, (size_t)sim_cells * 8, stream));
    if (!work) return MPNHIP_OK;
    const Lists L = make_lists(a_ptr, n_a, b_ptr, n_b, sim_ptr, sim_cells, n_frames);
    if (n_a > 0) {
        hipLaunchKernelGGL(k_row_sums, dim3(wave_blocks(n_a)), dim3(MT_THREADS), 0, stream, table, table_ptr, a_ptr, b_ptr, (int)n_frames,
                           (int)n_a, (int)n_b, table_cells, v.a_area);
        MPN_LAUNCH_CHECK();
    }
    if (n_b > 0) {
        hipLaunchKernelGGL(k_col_sums, dim3(blocks_for(n_b)), dim3(256), 0, stream, table, table_ptr, a_ptr, b_ptr, (int)n_frames, (int)n_a,
                           (int)n_b, table_cells, a_ignore, v.b_area, v.b_in_ignore, v.b_matched);
        MPN_LAUNCH_CHECK();
    }
    if (n_a > 0 && n_b > 0) {
        hipLaunchKernelGGL(k_hota_rows, dim3(wave_blocks(n_a)), dim3(HT_THREADS), 0, stream, table, table_ptr, table_cells, L, a_ignore,
                           b_scored, v.a_area, v.b_area, sim, v.b_matched);
        MPN_LAUNCH_CHECK();
    }
    if (n_b > 0) {
        hipLaunchKernelGGL(k_hota_cols, dim3(blocks_for(n_b)), dim3(256), 0, stream, L, b_scored, v.b_matched, v.b_in_ignore, sim, b_removed,
                           col_sum);
        MPN_LAUNCH_CHECK();
    }
    if (n_a > 0) {
        hipLaunchKernelGGL(k_hota_row_sums, dim3(wave_blocks(n_a)), dim3(HT_THREADS), 0, stream, L, b_removed, sim, row_sum);
        MPN_LAUNCH_CHECK();
    }
    return MPNHIP_OK;
}

extern "C" int mpnhip_hota_accumulate_alignment(const double* sim, int64_t sim_cells, const int64_t* sim_ptr, const int32_t* a_ptr,
                                                int64_t n_a, const int32_t* b_ptr, int64_t n_b, int64_t n_frames, const int32_t* a_traj,
                                                const int32_t* b_traj, const unsigned char* b_removed, const double* row_sum,
                                                const double* col_sum, int64_t n_gt_ids, int64_t n_tr_ids, double* potential,
                                                int32_t* gt_count, int32_t* tr_count, void* workspace, size_t workspace_bytes,
                                                void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(sim_sizes_ok(n_a, n_b, n_frames, n_gt_ids, n_tr_ids) && sim_cells >= 0 && sim_cells < (1LL << 31),
                  "hota_accumulate_alignment: bad sizes");
    if (!hota_supported(n_frames, n_gt_ids, n_tr_ids)) return refuse_unsupported("hota_accumulate_alignment", n_frames, n_gt_ids, n_tr_ids);
    if (n_a == 0 && n_b == 0) return MPNHIP_OK;
    MPN_CHECK_ARG(n_frames > 0 && a_ptr && b_ptr && sim_ptr, "hota_accumulate_alignment: entries without frames / null lists");
    MPN_CHECK_ARG(n_a == 0 || (a_traj && row_sum), "hota_accumulate_alignment: null a-side array");
    MPN_CHECK_ARG(n_b == 0 || (b_traj && b_removed && col_sum), "hota_accumulate_alignment: null b-side array");
    MPN_CHECK_ARG((n_gt_ids == 0 || gt_count) && (n_tr_ids == 0 || tr_count) && (n_gt_ids * n_tr_ids == 0 || potential),
                  "hota_accumulate_alignment: null accumulator");
    MPN_CHECK_ARG(sim_cells == 0 || sim, "hota_accumulate_alignment: null sim");
    if (n_gt_ids + n_tr_ids == 0) return MPNHIP_OK;
    MapView v = map_view(workspace, n_frames, n_gt_ids, n_tr_ids);
    MPN_CHECK_WORKSPACE("hota_accumulate_alignment", workspace, workspace_bytes, v.bytes);
    const Lists L = make_lists(a_ptr, n_a, b_ptr, n_b, sim_ptr, sim_cells, n_frames);
    MPN_HIP(hipMemsetAsync(v.map_a, 0xFF, v.map_bytes, stream));
    hipLaunchKernelGGL(k_hota_entry_maps, dim3(blocks_for(n_a + n_b)), dim3(256), 0, stream, L, a_traj, b_traj, b_removed, (int)n_gt_ids,
                       (int)n_tr_ids, v.map_a, v.map_b, gt_count, tr_count);
    MPN_LAUNCH_CHECK();
    if (n_gt_ids * n_tr_ids > 0 && sim_cells > 0) {
        hipLaunchKernelGGL(k_hota_alignment, dim3(blocks_for(n_gt_ids * n_tr_ids)), dim3(256), 0, stream, L, sim, row_sum, col_sum, v.map_a,
                           v.map_b, (int)n_gt_ids, (int)n_tr_ids, potential);
        MPN_LAUNCH_CHECK();
    }
    return MPNHIP_OK;
}

extern "C" int mpnhip_hota_frame_scores(const double* sim, int64_t sim_cells, const int64_t* sim_ptr, const int32_t* a_ptr, int64_t n_a,
                                        const int32_t* b_ptr, int64_t n_b, int64_t n_frames, const int32_t* a_traj, const int32_t* b_traj,
                                        const unsigned char* b_removed, int64_t n_gt_ids, int64_t n_tr_ids, const double* potential,
                                        const int32_t* gt_count, const int32_t* tr_count, double* score, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(sim_sizes_ok(n_a, n_b, n_frames, n_gt_ids, n_tr_ids) && sim_cells >= 0 && sim_cells < (1LL << 31),
                  "hota_frame_scores: bad sizes");
    if (!hota_supported(n_frames, n_gt_ids, n_tr_ids)) return refuse_unsupported("hota_frame_scores", n_frames, n_gt_ids, n_tr_ids);
    if (sim_cells == 0) return MPNHIP_OK;
    MPN_CHECK_ARG(sim && score && n_frames > 0 && a_ptr && b_ptr && sim_ptr && a_traj && b_traj && b_removed,
                  "hota_frame_scores: null sim, score or lists");
    MPN_HIP(hipMemsetAsync(score, 0, (size_t)sim_cells * 8, stream));
    if (n_gt_ids * n_tr_ids == 0) return MPNHIP_OK;
    MPN_CHECK_ARG(potential && gt_count && tr_count, "hota_frame_scores: null accumulator");
    const Lists L = make_lists(a_ptr, n_a, b_ptr, n_b, sim_ptr, sim_cells, n_frames);
    hipLaunchKernelGGL(k_hota_scores, dim3(frame_blocks(sim_cells, n_frames), (unsigned)n_frames), dim3(HT_THREADS), 0, stream, L, sim, a_traj,
                       b_traj, b_removed, (int)n_gt_ids, (int)n_tr_ids, potential, gt_count, tr_count, score);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}

extern "C" int mpnhip_hota_alpha_accumulate(const double* sim, int64_t sim_cells, const int64_t* sim_ptr, const int32_t* a_ptr, int64_t n_a,
                                            const int32_t* b_ptr, int64_t n_b, int64_t n_frames, const int32_t* a_traj,
                                            const int32_t* b_traj, const unsigned char* b_removed, const int32_t* match_b,
                                            const double* alphas, int64_t n_gt_ids, int64_t n_tr_ids, int64_t* tp, double* loca,
                                            int32_t* matches_count, void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(sim_sizes_ok(n_a, n_b, n_frames, n_gt_ids, n_tr_ids) && sim_cells >= 0 && sim_cells < (1LL << 31),
                  "hota_alpha_accumulate: bad sizes");
    if (!hota_supported(n_frames, n_gt_ids, n_tr_ids)) return refuse_unsupported("hota_alpha_accumulate", n_frames, n_gt_ids, n_tr_ids);
    MPN_CHECK_ARG(alphas && tp && loca, "hota_alpha_accumulate: null alphas, tp or loca");
    if (sim_cells == 0 || n_gt_ids * n_tr_ids == 0) return MPNHIP_OK;   // no pair to match
    MPN_CHECK_ARG(sim && matches_count && n_frames > 0 && a_ptr && b_ptr && sim_ptr && a_traj && b_traj && b_removed && match_b,
                  "hota_alpha_accumulate: null sim, matches_count or lists");
    AlphaView v = alpha_view(workspace, n_frames);
    MPN_CHECK_WORKSPACE("hota_alpha_accumulate", workspace, workspace_bytes, v.bytes);
    const Lists L = make_lists(a_ptr, n_a, b_ptr, n_b, sim_ptr, sim_cells, n_frames);
    Alphas al;
    for (int k = 0; k < N_ALPHA; ++k) al.v[k] = alphas[k];
    hipLaunchKernelGGL(k_hota_alphas, dim3((unsigned)n_frames), dim3(HT_THREADS), 0, stream, L, sim, a_traj, b_traj, b_removed, match_b,
                       (int)n_gt_ids, (int)n_tr_ids, al, reinterpret_cast<unsigned long long*>(tp), matches_count, v.frame_loca);
    MPN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_hota_fold, dim3(1), dim3(64), 0, stream, v.frame_loca, (int)n_frames, loca);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}

extern "C" int mpnhip_hota_association(const int32_t* matches_count, const int32_t* gt_count, const int32_t* tr_count, int64_t n_gt_ids,
                                       int64_t n_tr_ids, double* out, void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(sim_sizes_ok(0, 0, 0, n_gt_ids, n_tr_ids), "hota_association: bad sizes");
    if (!hota_supported(0, n_gt_ids, n_tr_ids)) return refuse_unsupported("hota_association", 0, n_gt_ids, n_tr_ids);
    MPN_CHECK_ARG(out, "hota_association: null out");
    const int64_t cells = n_gt_ids * n_tr_ids;
    MPN_CHECK_ARG(cells == 0 || (matches_count && gt_count && tr_count), "hota_association: null matches_count / counts");
    AssView v = ass_view(workspace, cells);
    if (cells > 0) MPN_CHECK_WORKSPACE("hota_association", workspace, workspace_bytes, v.bytes);
    if (cells == 0) {
        MPN_HIP(hipMemsetAsync(out, 0, (size_t)N_ALPHA * 3 * 8, stream));
        return MPNHIP_OK;
    }
    const int blocks = association_blocks(cells);
    hipLaunchKernelGGL(k_hota_association, dim3((unsigned)blocks, N_ALPHA), dim3(HT_THREADS), 0, stream, matches_count, gt_count, tr_count,
                       (int)n_gt_ids, (int)n_tr_ids, v.partial);
    MPN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_hota_association_fold, dim3(N_ALPHA), dim3(64), 0, stream, v.partial, blocks, out);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}
