// TrackEval's CLEAR and Identity metrics of a KITTI-MOTS sequence (metrics/clear.py:37-128, metrics/identity.py:32-89) from what
// mpnhip_hota_frame_similarity leaves on the device for a launch: the per-frame IoU blocks, the removed predictions and the
// entry-to-trajectory lists.  Two more consumers of HOTA's first pass:
//   identity_accumulate      kept cells with sim >= 0.5 -> potential_count[G, T]
//   identity_sums            the [G, T] assignment's match_b -> IDTP
//   clear_frame_candidates   per entry of either list its (at most two) eligible partners, all frames in parallel
//   clear_sequence_scan      the frames in order: matches, IDSW, Frag, the per-id counts and MOTP_sum, state carried over launches
//   clear_track_summary      the per-id counts -> MT, PT, ML, Frag
//
// Why CLEAR needs no assignment solver here.  clear.py:79-84 solves, per frame, an assignment over score = 1000 * (tracker id ==
// prev_timestep_tracker_id[gt id]) + similarity on the ELIGIBLE cells (similarity >= 0.5 - eps, the complement of :81) and 0
// elsewhere.  The frames are label images: one label per pixel, so the masks of either side are disjoint, and for a mask
// eligibility means 2 i >= u (i the intersection, u the union).
//   * Two predictions eligible with one object have disjoint intersections, each at least half the object (2 i >= u >= A): they
//     are two exact halves of it, each wholly inside it (u = A = 2 i, so B = i).  A third one has no pixel left: an object has at
//     most two eligible predictions, and then both at similarity exactly 0.5.
//   * In the same way a prediction has at most two eligible objects, and is then exactly the union of two objects of equal size.
//   * An entry with two eligible partners lies wholly inside / is wholly covered by them, so neither partner can be eligible with
//     anything else: a connected component of eligible cells is a single pair or a star of three entries.
//   * Components do not interact (every other cell scores 0), a single pair always beats leaving it (score > 0), and in a star the
//     two arms tie at 0.5 unless one carries the 1000 of continuity.  Only one can: an object has one previous tracker id and two
//     different predictions, and one tracker id was matched to at most one object in the previous frame.
// So a single pair is a match; in a star the arm with continuity wins, and without one the kit follows scipy's tie order --
// here the entry earlier in the list wins (the one deliberate difference; it never changes CLR_TP / CLR_FN / CLR_FP).  An entry
// with three candidates, or two stars that share an arm, cannot come from label images: the candidates kernel reports them in a
// status word and the host raises -- a guard, not a fallback.
//
// The same bits on every call and for every split into launches: integer atomics only; MOTP_sum is one thread adding a frame's
// matched similarities by ascending a-entry, then the frames in order (the kit's own order, clear.py:114).  An entry is KEPT as in
// hota.hip: its trajectory index is in range and, on the b-side, b_removed is 0.
#include <cfloat>

#include "sim_lists.h"

namespace mpnhip {
namespace {

constexpr int CI_THREADS = MT_THREADS;
constexpr double CLEAR_THRESHOLD = 0.5 - DBL_EPSILON;   // clear.py:81: eligible = not (similarity < 0.5 - np.finfo('float').eps)
constexpr double IDENTITY_THRESHOLD = 0.5;              // identity.py:55: np.greater_equal(similarity, 0.5)

__device__ __forceinline__ bool kept_b(const int* __restrict__ b_traj, const unsigned char* __restrict__ b_removed, int n_tr, int b) {
    return in_range(b_traj[b], n_tr) && !b_removed[b];
}

// ------------------------------------------------------------------------------------------------ Identity
// grid (blocks of a frame, frames): a kept cell at or above the threshold is one more potential match of its two ids
__global__ __launch_bounds__(CI_THREADS) void k_identity_cells(Lists L, const double* __restrict__ sim, const int* __restrict__ a_traj,
                                                               const int* __restrict__ b_traj, const unsigned char* __restrict__ b_removed,
                                                               int n_gt, int n_tr, int* __restrict__ potential_count) {
    const FrameSim fs = frame_sim(L, blockIdx.y);
    if (!fs.ok || fs.nb == 0) return;
    const int64_t cells = (int64_t)fs.na * fs.nb;
    for (int64_t c = (int64_t)blockIdx.x * CI_THREADS + threadIdx.x; c < cells; c += (int64_t)gridDim.x * CI_THREADS) {
        if (!(sim[fs.base + c] >= IDENTITY_THRESHOLD)) continue;
        const int b = fs.b0 + (int)(c % fs.nb), g = a_traj[fs.a0 + (int)(c / fs.nb)];
        if (in_range(g, n_gt) && kept_b(b_traj, b_removed, n_tr, b)) atomicAdd(&potential_count[(int64_t)g * n_tr + b_traj[b]], 1);
    }
}

// one thread per ground-truth id: the count of its chosen pair (match_b: a column of the table, or anything else for none)
__global__ void k_identity_sums(const int* __restrict__ potential_count, const int* __restrict__ match_b, int n_gt, int n_tr,
                                unsigned long long* __restrict__ idtp) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_gt) return;
    const int t = match_b[g];
    if (!in_range(t, n_tr)) return;
    const int v = potential_count[(int64_t)g * n_tr + t];
    if (v > 0) atomicAdd(idtp, (unsigned long long)v);
}

// ------------------------------------------------------------------------------------------------ CLEAR: candidates
// One thread per entry of either list: a kept a-entry walks its row, a kept b-entry its column, in list order; the first two
// eligible kept partners (indices into the launch's lists, -1 for none) are its candidates.  Status bit 0: a third one exists.
__global__ void k_clear_candidates(Lists L, const double* __restrict__ sim, const int* __restrict__ a_traj, const int* __restrict__ b_traj,
                                   const unsigned char* __restrict__ b_removed, int n_gt, int n_tr, int* __restrict__ a_cand,
                                   int* __restrict__ b_cand, int* __restrict__ status) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    int c[2] = {-1, -1}, n = 0;
    if (e < L.n_a) {
        const int a = e, f = frame_of(L.a_ptr, L.n_frames, a);
        if (f >= 0 && in_range(a_traj[a], n_gt)) {
            const FrameSim fs = frame_sim(L, f);
            const int ia = a - fs.a0;
            if (fs.ok && in_range(ia, fs.na)) {
                const double* __restrict__ row = sim + fs.base + (int64_t)ia * fs.nb;
                for (int ib = 0; ib < fs.nb; ++ib)
                    if (row[ib] >= CLEAR_THRESHOLD && kept_b(b_traj, b_removed, n_tr, fs.b0 + ib)) {
                        if (n < 2) c[n] = fs.b0 + ib;
                        ++n;
                    }
            }
        }
        a_cand[2 * (int64_t)a] = c[0];
        a_cand[2 * (int64_t)a + 1] = c[1];
    } else if (e - L.n_a < L.n_b) {
        const int b = e - L.n_a, f = frame_of(L.b_ptr, L.n_frames, b);
        if (f >= 0 && kept_b(b_traj, b_removed, n_tr, b)) {
            const FrameSim fs = frame_sim(L, f);
            const int ib = b - fs.b0;
            if (fs.ok && in_range(ib, fs.nb))
                for (int ia = 0; ia < fs.na; ++ia)
                    if (sim[fs.base + (int64_t)ia * fs.nb + ib] >= CLEAR_THRESHOLD && in_range(a_traj[fs.a0 + ia], n_gt)) {
                        if (n < 2) c[n] = fs.a0 + ia;
                        ++n;
                    }
        }
        b_cand[2 * (int64_t)b] = c[0];
        b_cand[2 * (int64_t)b + 1] = c[1];
    }
    if (n > 2) atomicOr(status, 1);
}

// one thread per a-entry: status bit 1 if an a-entry with two candidates has one that itself has two (a component larger than a
// star).  The candidates are the ones k_clear_candidates wrote: entries of the lists or -1.
__global__ void k_clear_check(int n_a, const int* __restrict__ a_cand, const int* __restrict__ b_cand, int* __restrict__ status) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n_a) return;
    const int c0 = a_cand[2 * (int64_t)a], c1 = a_cand[2 * (int64_t)a + 1];
    if (c0 >= 0 && c1 >= 0 && (b_cand[2 * (int64_t)c0 + 1] >= 0 || b_cand[2 * (int64_t)c1 + 1] >= 0)) atomicOr(status, 2);
}

// ------------------------------------------------------------------------------------------------ CLEAR: the scan
struct ClearState {
    int* prev_tracker; int* prev_timestep; int* id_count; int* matched_count; int* frag_count;
    long long* counters;   // CLR_TP, CLR_FN, CLR_FP, IDSW
    double* motp_sum;
};

// The b-entry matched with the kept a-entry a of frame fs, or -1 (the header's argument).  The candidates come from the caller:
// each is used only as an entry of this frame that is kept.
__device__ int clear_match(const FrameSim& fs, int a, const int* __restrict__ a_traj, const int* __restrict__ b_traj,
                           const unsigned char* __restrict__ b_removed, const int* __restrict__ a_cand, const int* __restrict__ b_cand,
                           int n_gt, int n_tr, const int* __restrict__ prev_timestep) {
    const int c0 = a_cand[2 * (int64_t)a], c1 = a_cand[2 * (int64_t)a + 1];
    auto b_ok = [&](int b) { return in_range(b - fs.b0, fs.nb) && kept_b(b_traj, b_removed, n_tr, b); };
    auto a_ok = [&](int x) { return in_range(x - fs.a0, fs.na) && in_range(a_traj[x], n_gt); };
    if (!b_ok(c0)) return -1;
    if (b_ok(c1))   // a row star: the later arm wins only by continuity
        return b_traj[c1] == prev_timestep[a_traj[a]] ? c1 : c0;
    const int d0 = b_cand[2 * (int64_t)c0], d1 = b_cand[2 * (int64_t)c0 + 1];
    if (!a_ok(d0)) return -1;
    if (!a_ok(d1)) return d0 == a ? c0 : -1;   // a single pair
    const int winner = prev_timestep[a_traj[d1]] == b_traj[c0] ? d1 : d0;   // a column star
    return winner == a ? c0 : -1;
}

// One wavefront for the sequence: the frames of the launch in ascending order, lanes over the frame's entries and over the ids
// (clear.py:67-114).  now [n_gt] is the workspace: the tracker id matched with every ground-truth id in the current frame.
__global__ __launch_bounds__(64) void k_clear_scan(Lists L, const double* __restrict__ sim, const int* __restrict__ a_traj,
                                                   const int* __restrict__ b_traj, const unsigned char* __restrict__ b_removed,
                                                   const int* __restrict__ a_cand, const int* __restrict__ b_cand, int n_gt, int n_tr,
                                                   ClearState st, int* __restrict__ now, int* __restrict__ match_b) {
    const int lane = threadIdx.x;
    long long tp = st.counters[0], fn = st.counters[1], fp = st.counters[2], idsw = st.counters[3];
    double motp = st.motp_sum[0];
    for (int f = 0; f < L.n_frames; ++f) {
        const FrameSim fs = frame_sim(L, f);
        if (!fs.ok) continue;   // (the frame's cells do not lie inside sim: nothing of it is read or written)
        int ka = 0, kb = 0;
        for (int ia = lane; ia < fs.na; ia += 64) ka += in_range(a_traj[fs.a0 + ia], n_gt) ? 1 : 0;
        for (int ib = lane; ib < fs.nb; ib += 64) kb += kept_b(b_traj, b_removed, n_tr, fs.b0 + ib) ? 1 : 0;
        ka = wave_sum(ka);
        kb = wave_sum(kb);
        if (ka == 0) {   // :69-71 (the branches below are uniform: ka and kb are the wavefront's sums)
            fp += kb;
            continue;
        }
        if (kb == 0) {   // :72-75: prev_timestep_tracker_id stays, so continuity survives the frame
            fn += ka;
            for (int ia = lane; ia < fs.na; ia += 64) {
                const int g = a_traj[fs.a0 + ia];
                if (in_range(g, n_gt)) atomicAdd(&st.id_count[g], 1);
            }
            continue;
        }
        for (int g = lane; g < n_gt; g += 64) now[g] = -1;
        __syncthreads();
        int nm = 0, sw = 0;
        for (int ia = lane; ia < fs.na; ia += 64) {
            const int a = fs.a0 + ia, g = a_traj[a];
            if (!in_range(g, n_gt)) continue;
            atomicAdd(&st.id_count[g], 1);
            const int m = clear_match(fs, a, a_traj, b_traj, b_removed, a_cand, b_cand, n_gt, n_tr, st.prev_timestep);
            if (m < 0) continue;
            const int t = b_traj[m], before = st.prev_tracker[g];
            match_b[a] = m;
            atomicAdd(&st.matched_count[g], 1);
            if (before >= 0 && before != t) ++sw;   // :93-96: against the last time the id was matched, however long ago
            st.prev_tracker[g] = t;
            now[g] = t;
            ++nm;
        }
        __syncthreads();
        for (int g = lane; g < n_gt; g += 64) {   // :101-106
            const int t = now[g];
            if (st.prev_timestep[g] < 0 && t >= 0) st.frag_count[g] += 1;
            st.prev_timestep[g] = t;
        }
        nm = wave_sum(nm);
        sw = wave_sum(sw);
        tp += nm;
        fn += ka - nm;
        fp += kb - nm;
        idsw += sw;
        if (lane == 0 && nm > 0) {   // :114: Python's sum over the matched rows in order, then += into the total
            double s = 0.0;
            for (int ia = 0; ia < fs.na; ++ia) {
                const int m = match_b[fs.a0 + ia];
                if (m >= 0) s += sim[fs.base + (int64_t)ia * fs.nb + (m - fs.b0)];
            }
            motp += s;
        }
        __syncthreads();
    }
    if (lane == 0) {
        st.counters[0] = tp; st.counters[1] = fn; st.counters[2] = fp; st.counters[3] = idsw;
        st.motp_sum[0] = motp;
    }
}

// ------------------------------------------------------------------------------------------------ CLEAR: the tracks
// One block: out = MT, PT, ML, Frag (clear.py:117-121).  The kit compares the double matched / count with 0.8 and 0.2; for
// integers 0 <= m <= c < 2^31 the integer predicates are the same decisions: if 5 m != 4 c the quotient differs from 4 / 5 by at
// least 1 / (5 c) > 2^-34, far more than the rounding of the division and of the literal 0.8, and if 5 m == 4 c the division
// rounds 4 / 5 to the very double the literal 0.8 is; likewise for 0.2 and 5 m >= c.
__global__ __launch_bounds__(CI_THREADS) void k_clear_tracks(const int* __restrict__ id_count, const int* __restrict__ matched_count,
                                                             const int* __restrict__ frag_count, int n_gt, long long* __restrict__ out) {
    __shared__ unsigned long long s_sum[3];   // MT, MT + PT, Frag
    if (threadIdx.x < 3) s_sum[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long mt = 0, ge = 0, frag = 0;
    for (int g = threadIdx.x; g < n_gt; g += CI_THREADS) {
        const long long c = id_count[g], m = matched_count[g], fr = frag_count[g];
        if (c > 0) {
            mt += 5 * m > 4 * c ? 1 : 0;
            ge += 5 * m >= c ? 1 : 0;
        }
        if (fr > 0) frag += (unsigned long long)(fr - 1);
    }
    if (mt) atomicAdd(&s_sum[0], mt);
    if (ge) atomicAdd(&s_sum[1], ge);
    if (frag) atomicAdd(&s_sum[2], frag);
    __syncthreads();
    if (threadIdx.x == 0) {
        const long long MT = (long long)s_sum[0], PT = (long long)s_sum[1] - MT;
        out[0] = MT; out[1] = PT; out[2] = n_gt - MT - PT; out[3] = (long long)s_sum[2];
    }
}

// ------------------------------------------------------------------------------------------------ workspaces
struct ScanView { int* now; size_t bytes; };
static ScanView scan_view(void* workspace, int64_t n_gt) {
    Carver c(workspace);
    ScanView v = {c.take<int>((size_t)n_gt), 0};
    v.bytes = c.bytes();
    return v;
}

// the int32 potential_count [G, T] is one problem of mpnhip_lsa_batched: fewer than 2^31 cells
static bool ci_supported(int64_t n_gt, int64_t n_tr) { return n_gt * n_tr < (1LL << 31); }
static int refuse_unsupported(const char* name, int64_t n_gt, int64_t n_tr) {
    set_error("%s: %lld x %lld trajectories (2^31 cells or more) is not supported", name, (long long)n_gt, (long long)n_tr);
    return MPNHIP_ERR_UNSUPPORTED;
}

}  // namespace
}  // namespace mpnhip

using namespace mpnhip;

extern "C" size_t mpnhip_clear_identity_workspace_bytes(int64_t n_a, int64_t n_b, int64_t n_frames, int64_t n_gt_ids, int64_t n_tr_ids) {
    if (!sim_sizes_ok(n_a, n_b, n_frames, n_gt_ids, n_tr_ids) || !ci_supported(n_gt_ids, n_tr_ids)) return 0;
    return scan_view(nullptr, n_gt_ids).bytes + 256;
}

extern "C" int mpnhip_identity_accumulate(const double* sim, int64_t sim_cells, const int64_t* sim_ptr, const int32_t* a_ptr, int64_t n_a,
                                          const int32_t* b_ptr, int64_t n_b, int64_t n_frames, const int32_t* a_traj,
                                          const int32_t* b_traj, const unsigned char* b_removed, int64_t n_gt_ids, int64_t n_tr_ids,
                                          int32_t* potential_count, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(sim_sizes_ok(n_a, n_b, n_frames, n_gt_ids, n_tr_ids) && sim_cells >= 0 && sim_cells < (1LL << 31),
                  "identity_accumulate: bad sizes");
    if (!ci_supported(n_gt_ids, n_tr_ids)) return refuse_unsupported("identity_accumulate", n_gt_ids, n_tr_ids);
    if (sim_cells == 0 || n_gt_ids * n_tr_ids == 0) return MPNHIP_OK;   // no pair
    MPN_CHECK_ARG(sim && potential_count && n_frames > 0 && a_ptr && b_ptr && sim_ptr && a_traj && b_traj && b_removed,
                  "identity_accumulate: null sim, potential_count or lists");
    const Lists L = make_lists(a_ptr, n_a, b_ptr, n_b, sim_ptr, sim_cells, n_frames);
    hipLaunchKernelGGL(k_identity_cells, dim3(frame_blocks(sim_cells, n_frames), (unsigned)n_frames), dim3(CI_THREADS), 0, stream, L, sim,
                       a_traj, b_traj, b_removed, (int)n_gt_ids, (int)n_tr_ids, potential_count);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}

extern "C" int mpnhip_identity_sums(const int32_t* potential_count, const int32_t* match_b, int64_t n_gt_ids, int64_t n_tr_ids, int64_t* idtp,
                                    void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(sim_sizes_ok(0, 0, 0, n_gt_ids, n_tr_ids), "identity_sums: bad sizes");
    if (!ci_supported(n_gt_ids, n_tr_ids)) return refuse_unsupported("identity_sums", n_gt_ids, n_tr_ids);
    MPN_CHECK_ARG(idtp, "identity_sums: null idtp");
    MPN_CHECK_ARG(n_gt_ids * n_tr_ids == 0 || (potential_count && match_b), "identity_sums: null potential_count or match_b");
    MPN_HIP(hipMemsetAsync(idtp, 0, 8, stream));
    if (n_gt_ids * n_tr_ids == 0) return MPNHIP_OK;
    hipLaunchKernelGGL(k_identity_sums, dim3(blocks_for(n_gt_ids)), dim3(256), 0, stream, potential_count, match_b, (int)n_gt_ids,
                       (int)n_tr_ids, reinterpret_cast<unsigned long long*>(idtp));
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}

extern "C" int mpnhip_clear_frame_candidates(const double* sim, int64_t sim_cells, const int64_t* sim_ptr, const int32_t* a_ptr, int64_t n_a,
                                             const int32_t* b_ptr, int64_t n_b, int64_t n_frames, const int32_t* a_traj,
                                             const int32_t* b_traj, const unsigned char* b_removed, int64_t n_gt_ids, int64_t n_tr_ids,
                                             int32_t* a_cand, int32_t* b_cand, int32_t* status, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(sim_sizes_ok(n_a, n_b, n_frames, n_gt_ids, n_tr_ids) && sim_cells >= 0 && sim_cells < (1LL << 31),
                  "clear_frame_candidates: bad sizes");
    MPN_CHECK_ARG(status, "clear_frame_candidates: null status");
    // (every check before the first HIP call)
    const bool work = n_a > 0 || n_b > 0;
    MPN_CHECK_ARG(!work || (n_frames > 0 && a_ptr && b_ptr && sim_ptr), "clear_frame_candidates: entries without frames / null lists");
    MPN_CHECK_ARG(n_a == 0 || (a_traj && a_cand), "clear_frame_candidates: null a-side array");
    MPN_CHECK_ARG(n_b == 0 || (b_traj && b_removed && b_cand), "clear_frame_candidates: null b-side array");
    MPN_CHECK_ARG(sim_cells == 0 || sim, "clear_frame_candidates: null sim");
    MPN_HIP(hipMemsetAsync(status, 0, 4, stream));
    if (!work) return MPNHIP_OK;
    const Lists L = make_lists(a_ptr, n_a, b_ptr, n_b, sim_ptr, sim_cells, n_frames);
    hipLaunchKernelGGL(k_clear_candidates, dim3(blocks_for(n_a + n_b)), dim3(256), 0, stream, L, sim, a_traj, b_traj, b_removed, (int)n_gt_ids,
                       (int)n_tr_ids, a_cand, b_cand, status);
    MPN_LAUNCH_CHECK();
    if (n_a > 0 && n_b > 0) {
        hipLaunchKernelGGL(k_clear_check, dim3(blocks_for(n_a)), dim3(256), 0, stream, (int)n_a, a_cand, b_cand, status);
        MPN_LAUNCH_CHECK();
    }
    return MPNHIP_OK;
}

extern "C" int mpnhip_clear_sequence_scan(const double* sim, int64_t sim_cells, const int64_t* sim_ptr, const int32_t* a_ptr, int64_t n_a,
                                          const int32_t* b_ptr, int64_t n_b, int64_t n_frames, const int32_t* a_traj,
                                          const int32_t* b_traj, const unsigned char* b_removed, const int32_t* a_cand,
                                          const int32_t* b_cand, int64_t n_gt_ids, int64_t n_tr_ids, int32_t* prev_tracker_id,
                                          int32_t* prev_timestep_tracker_id, int32_t* gt_id_count, int32_t* gt_matched_count,
                                          int32_t* gt_frag_count, int64_t* counters, double* motp_sum, int32_t* match_b, void* workspace,
                                          size_t workspace_bytes, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(sim_sizes_ok(n_a, n_b, n_frames, n_gt_ids, n_tr_ids) && sim_cells >= 0 && sim_cells < (1LL << 31),
                  "clear_sequence_scan: bad sizes");
    MPN_CHECK_ARG(counters && motp_sum, "clear_sequence_scan: null counters or motp_sum");
    if (n_a == 0 && n_b == 0) return MPNHIP_OK;
    MPN_CHECK_ARG(n_frames > 0 && a_ptr && b_ptr && sim_ptr, "clear_sequence_scan: entries without frames / null lists");
    MPN_CHECK_ARG(n_a == 0 || (a_traj && a_cand && match_b), "clear_sequence_scan: null a-side array");
    MPN_CHECK_ARG(n_b == 0 || (b_traj && b_removed && b_cand), "clear_sequence_scan: null b-side array");
    MPN_CHECK_ARG(sim_cells == 0 || sim, "clear_sequence_scan: null sim");
    MPN_CHECK_ARG(n_gt_ids == 0 || (prev_tracker_id && prev_timestep_tracker_id && gt_id_count && gt_matched_count && gt_frag_count),
                  "clear_sequence_scan: null state");
    ScanView v = scan_view(workspace, n_gt_ids);
    MPN_CHECK_WORKSPACE("clear_sequence_scan", workspace, workspace_bytes, v.bytes);
    if (n_a > 0) MPN_HIP(hipMemsetAsync(match_b, 0xFF, (size_t)n_a * 4, stream));
    const Lists L = make_lists(a_ptr, n_a, b_ptr, n_b, sim_ptr, sim_cells, n_frames);
    ClearState st = {prev_tracker_id, prev_timestep_tracker_id, gt_id_count, gt_matched_count, gt_frag_count,
                     reinterpret_cast<long long*>(counters), motp_sum};
    hipLaunchKernelGGL(k_clear_scan, dim3(1), dim3(64), 0, stream, L, sim, a_traj, b_traj, b_removed, a_cand, b_cand, (int)n_gt_ids,
                       (int)n_tr_ids, st, v.now, match_b);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}

extern "C" int mpnhip_clear_track_summary(const int32_t* gt_id_count, const int32_t* gt_matched_count, const int32_t* gt_frag_count,
                                          int64_t n_gt_ids, int64_t* out, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(sim_sizes_ok(0, 0, 0, n_gt_ids, 0), "clear_track_summary: bad sizes");
    MPN_CHECK_ARG(out, "clear_track_summary: null out");
    MPN_CHECK_ARG(n_gt_ids == 0 || (gt_id_count && gt_matched_count && gt_frag_count), "clear_track_summary: null counts");
    if (n_gt_ids == 0) {
        MPN_HIP(hipMemsetAsync(out, 0, 4 * 8, stream));
        return MPNHIP_OK;
    }
    hipLaunchKernelGGL(k_clear_tracks, dim3(1), dim3(CI_THREADS), 0, stream, gt_id_count, gt_matched_count, gt_frag_count, (int)n_gt_ids,
                       reinterpret_cast<long long*>(out));
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}
