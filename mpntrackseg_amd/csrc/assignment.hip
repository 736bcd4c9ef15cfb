// Batched rectangular linear sum assignment (scipy.optimize.linear_sum_assignment), one problem per frame, over the layout of
// hota.hip's similarity block: problem f owns na_f x nb_f float64 cells at cell_ptr[f], cell [ia * nb_f + ib], and the rows /
// columns that take part are picked by two keep masks -- a score block goes in as it is.
//
// The shortest augmenting path of Crouse 2016 (the algorithm scipy runs) with dual variables u, v in float64, stated so that
// tests/lsa_ref.py gives the same bits, ties included:
//   c = maximize ? -cost : cost; more kept rows than kept columns: the index roles are swapped (nothing is copied)
//   rows in list order; a search relaxes r = ((minval + c[i][j]) - u[i]) - v[j] and takes it only if r < shortest[j]
//   next column: the unscanned one of lowest shortest; among equals an unassigned one, then the lowest index
//   a NaN r, or no unscanned column with a finite shortest (a NaN, -inf, or only +inf cells): the problem stops, status 1
// One wavefront per problem, its whole state in LDS; a lane owns the columns j = lane (mod 64), reads the cost row straight from
// global memory and the wavefront agrees on the next column with a butterfly of (shortest, assigned, index).  Every loop is
// bounded by a counter: a search scans one new column per step (<= nc steps), a problem runs nr searches.
#include <climits>
#include <cmath>

#include "label_tables.h"

namespace mpnhip {
namespace {

constexpr int LSA_SIDE = MPNHIP_LSA_MAX_SIDE;
// per row or column of the larger side: u / v / shortest (8 B each), path, col4row, row4col, the two lists of kept entries
// (4 B each), the two scanned sets (1 B each)
constexpr int LSA_STATE_BYTES = 3 * 8 + 5 * 4 + 2 * 1;
constexpr int LSA_LDS_BYTES = 160 * 1024;   // what one workgroup may declare on gfx950
static_assert(LSA_SIDE * LSA_STATE_BYTES <= LSA_LDS_BYTES && 2 * LSA_SIDE * LSA_STATE_BYTES > LSA_LDS_BYTES,
              "MPNHIP_LSA_MAX_SIDE is the largest power of two whose state fits the LDS of one workgroup");
static_assert(LSA_SIDE <= (1 << 15), "the argmin key packs a column index into 16 bits");

enum { LSA_DONE = 0, LSA_NOT_FINITE = 1, LSA_TOO_LARGE = 2, LSA_BAD_CELLS = 3 };

// the wavefront's LDS writes are visible to all its lanes past this point (no block-wide barrier: the block IS the wavefront)
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// the kept entries of [first, first + count) of a list, in order, into idx (at most LSA_SIDE of them); returns their number
__device__ __forceinline__ int kept_entries(const unsigned char* __restrict__ keep, int first, int count, int lane, int* idx) {
    int n = 0;
    for (int e0 = 0; e0 < count; e0 += 64) {
        const int e = e0 + lane;
        const bool k = e < count && (!keep || keep[first + e]);
        const unsigned long long m = __ballot(k);
        const int at = n + __popcll(m & ((1ull << lane) - 1));
        if (k && at < LSA_SIDE) idx[at] = e;
        n += __popcll(m);
        if (n > LSA_SIDE) break;   // (wavefront-uniform)
    }
    return n;
}

struct Best { double v; int key; };   // key = assigned << 16 | column
__device__ __forceinline__ bool before(double v, int key, const Best& b) { return v < b.v || (v == b.v && key < b.key); }

__global__ __launch_bounds__(64) void k_lsa(const double* __restrict__ cost, int64_t cells, const int64_t* __restrict__ cell_ptr,
                                            const int* __restrict__ a_ptr, int n_a, const int* __restrict__ b_ptr, int n_b,
                                            const unsigned char* __restrict__ a_keep, const unsigned char* __restrict__ b_keep,
                                            int maximize, int* __restrict__ match_b, int* __restrict__ match_a,
                                            int* __restrict__ status) {
    __shared__ double s_u[LSA_SIDE], s_v[LSA_SIDE], s_shortest[LSA_SIDE];
    __shared__ int s_path[LSA_SIDE], s_col4row[LSA_SIDE], s_row4col[LSA_SIDE], s_a[LSA_SIDE], s_b[LSA_SIDE];
    __shared__ unsigned char s_sr[LSA_SIDE], s_sc[LSA_SIDE];
    const int f = blockIdx.x, lane = threadIdx.x;
    int a0, na, b0, nb;
    clamp_range(a_ptr, f, n_a, a0, na);
    clamp_range(b_ptr, f, n_b, b0, nb);
    const int64_t base = cell_ptr[f];
    if (!(base >= 0 && base <= cells && (int64_t)na * nb <= cells - base)) {   // (the match arrays hold -1 already)
        if (lane == 0) status[f] = LSA_BAD_CELLS;
        return;
    }
    const int nka = kept_entries(a_keep, a0, na, lane, s_a), nkb = kept_entries(b_keep, b0, nb, lane, s_b);
    if (nka > LSA_SIDE || nkb > LSA_SIDE) {
        if (lane == 0) status[f] = LSA_TOO_LARGE;
        return;
    }
    // rows: the side with fewer kept entries
    const bool swapped = nka > nkb;
    const int nr = swapped ? nkb : nka, nc = swapped ? nka : nkb;
    const int* __restrict__ rows = swapped ? s_b : s_a;
    const int* __restrict__ cols = swapped ? s_a : s_b;
    const int64_t row_stride = swapped ? 1 : nb, col_stride = swapped ? nb : 1;
    const double* __restrict__ c0 = cost + base;
    for (int j = lane; j < nc; j += 64) {
        s_v[j] = 0.0;
        s_row4col[j] = -1;
        if (j < nr) { s_u[j] = 0.0; s_col4row[j] = -1; }
    }
    wave_sync();
    int state = LSA_DONE;
    for (int cur = 0; cur < nr && state == LSA_DONE; ++cur) {
        for (int j = lane; j < nc; j += 64) {
            s_shortest[j] = INFINITY;
            s_sc[j] = 0;
            if (j < nr) s_sr[j] = 0;
        }
        wave_sync();
        double minval = 0.0;
        int i = cur, sink = -1;
        for (int step = 0; step < nc && sink < 0; ++step) {
            if (lane == 0) s_sr[i] = 1;
            const double ui = s_u[i];
            const double* __restrict__ crow = c0 + rows[i] * row_stride;
            Best best = {INFINITY, INT_MAX};
            bool nan = false;
            for (int j = lane; j < nc; j += 64) {   // (a lane's own columns: nothing another lane wrote in this search)
                if (s_sc[j]) continue;
                const double c = crow[cols[j] * col_stride];
                const double r = ((minval + (maximize ? -c : c)) - ui) - s_v[j];
                nan = nan || r != r;
                double s = s_shortest[j];
                if (r < s) {
                    s_shortest[j] = s = r;
                    s_path[j] = i;
                }
                const int key = (s_row4col[j] >= 0 ? 1 << 16 : 0) | j;
                if (before(s, key, best)) { best.v = s; best.key = key; }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double v = __shfl_xor(best.v, o);
                const int key = __shfl_xor(best.key, o);
                if (before(v, key, best)) { best.v = v; best.key = key; }
            }
            if (__any(nan) || !isfinite(best.v)) {   // (wavefront-uniform: every lane holds the same best)
                state = LSA_NOT_FINITE;
                break;
            }
            minval = best.v;
            const int j = best.key & 0xFFFF;
            if ((j & 63) == lane) s_sc[j] = 1;
            if (best.key >> 16) i = s_row4col[j]; else sink = j;
        }
        if (state == LSA_DONE && sink < 0) state = LSA_NOT_FINITE;   // (not reached: nc >= nr leaves an unassigned column)
        if (state != LSA_DONE) break;
        wave_sync();
        // the duals, then the augmentation along path
        for (int r = lane; r < nr; r += 64)
            if (r == cur) s_u[r] += minval;
            else if (s_sr[r]) s_u[r] += minval - s_shortest[s_col4row[r]];
        for (int j = lane; j < nc; j += 64)
            if (s_sc[j]) s_v[j] -= minval - s_shortest[j];
        wave_sync();
        if (lane == 0) {
            int j = sink;
            for (int k = 0; k < nr; ++k) {
                const int r = s_path[j];
                s_row4col[j] = r;
                const int next = s_col4row[r];
                s_col4row[r] = j;
                j = next;
                if (r == cur || j < 0) break;
            }
        }
        wave_sync();
    }
    if (state == LSA_DONE)
        for (int r = lane; r < nr; r += 64) {
            const int a = a0 + (swapped ? cols[s_col4row[r]] : rows[r]), b = b0 + (swapped ? rows[r] : cols[s_col4row[r]]);
            match_b[a] = b;
            if (match_a) match_a[b] = a;
        }
    if (lane == 0) status[f] = state;
}

static bool lsa_sizes_ok(int64_t n_a, int64_t n_b, int64_t n_problems) {
    return list_sizes_ok(n_a, n_problems, 0) && list_sizes_ok(n_b, n_problems, 0);
}

}  // namespace
}  // namespace mpnhip

using namespace mpnhip;

extern "C" size_t mpnhip_lsa_workspace_bytes(int64_t n_a, int64_t n_b, int64_t n_problems) {
    return lsa_sizes_ok(n_a, n_b, n_problems) ? 256 : 0;   // (the state lives in LDS; the buffer is reserved)
}

extern "C" int mpnhip_lsa_batched(const double* cost, int64_t cells, const int64_t* cell_ptr, const int32_t* a_ptr, int64_t n_a,
                                  const int32_t* b_ptr, int64_t n_b, int64_t n_problems, const unsigned char* a_keep,
                                  const unsigned char* b_keep, int maximize, int32_t* match_b, int32_t* match_a, int32_t* status,
                                  void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(lsa_sizes_ok(n_a, n_b, n_problems) && cells >= 0, "lsa_batched: bad sizes");
    if (cells >= (1LL << 31)) {
        set_error("lsa_batched: %lld cells (2^31 or more) are not supported: fewer problems per call", (long long)cells);
        return MPNHIP_ERR_UNSUPPORTED;
    }
    if (n_problems == 0 || (n_a == 0 && n_b == 0)) return MPNHIP_OK;
    MPN_CHECK_ARG(cell_ptr && a_ptr && b_ptr && status && (n_a == 0 || match_b) && (cells == 0 || cost),
                  "lsa_batched: null cost, lists, match_b or status");
    MPN_CHECK_WORKSPACE("lsa_batched", workspace, workspace_bytes, mpnhip_lsa_workspace_bytes(n_a, n_b, n_problems));
    if (n_a > 0) MPN_HIP(hipMemsetAsync(match_b, 0xFF, (size_t)n_a * 4, stream));
    if (n_b > 0 && match_a) MPN_HIP(hipMemsetAsync(match_a, 0xFF, (size_t)n_b * 4, stream));
    hipLaunchKernelGGL(k_lsa, dim3((unsigned)n_problems), dim3(64), 0, stream, cost, cells, cell_ptr, a_ptr, (int)n_a, b_ptr, (int)n_b, a_keep,
                       b_keep, maximize, match_b, match_a, status);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}
