// COCO's compressed run-length strings, both directions, for a batch of masks (SURVEY.md section 8 row f-3 and the text files of
// the evaluation):
//   rleToString   (cocoapi common/maskApi.c)  = masks.rle_string of the host codec             -> mpnhip_rle_encode
//   rleFrString   (cocoapi common/maskApi.c)  = masks.rle_counts + mots_eval.counts_to_runs    -> mpnhip_rle_decode_scan / _runs
// A string is a list of counts (alternating run lengths, zeros first).  Count i >= 3 is stored as its difference to count i - 2;
// a value is written in 5-bit groups, low bits first, as the characters 48 + group + 32 * more, where `more` is clear once the
// rest is all sign (the group's bit 4 is the sign the reader extends).
//
// Encode: the counts of an entry are the differences of (0, its run boundaries ..., hw), so a stored value depends on four
// neighbouring boundaries only: one thread per count, a code-length pass, ONE exclusive scan over all counts of all entries (the
// strings are concatenated in entry order) and a write pass.
// Decode: one wavefront per string, 64 characters at a time.  The lane at a count's first character assembles the value by
// reading forward (never past the string's end); the "+= count i - 2" recurrence over the odd and over the even places and the
// running position are wave scans with carries from chunk to chunk.  No LDS.  Integers only, int64 with wrap-around as numpy's:
// the same bits as the host codec on every call.
#include "device_prims.h"

namespace mpnhip {
namespace {

constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int MAX_GROUPS = 12;                 // masks.rle_counts: "count too long" beyond 12 groups (60 bits)
constexpr int64_t POS_END = 1LL << 31;         // positions are int32
enum { ST_CHAR = 1, ST_TRUNCATED = 2, ST_LONG = 4, ST_NEGATIVE = 8, ST_SUM = 16 };

static bool enc_sizes_ok(int64_t n_dets, int64_t n_events, int64_t hw) {
    return n_dets >= 0 && n_dets < (1LL << 30) && n_events >= 0 && n_events < (1LL << 31) && hw >= 0 && hw < (1LL << 31);
}
static bool dec_sizes_ok(int64_t n, int64_t n_bytes) { return n >= 0 && n < (1LL << 30) && n_bytes >= 0 && n_bytes < (1LL << 31); }

// ------------------------------------------------------------------------------------------------ encode
// events per entry (a negative count is none), [n_dets] and a zero behind
__global__ void k_enc_entry_counts(const int* __restrict__ det_counts, int64_t n_dets, int64_t* __restrict__ out) {
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d > n_dets) return;
    const int v = d < n_dets ? det_counts[d] : 0;
    out[d] = v > 0 ? v : 0;
}

// The stored value of count c of the launch.  Entry d owns the counts [ev_ptr[d] + d, ev_ptr[d + 1] + d + 1): one more than its
// events.  false: c lies behind the last entry's counts (a number of events that is not the lists' own).
__device__ __forceinline__ bool enc_value(int64_t c, const int64_t* __restrict__ ev_ptr, int64_t n_dets, const int* __restrict__ event_pos,
                                          int64_t n_events, int64_t hw, int64_t* value) {
    int64_t lo = 0, hi = n_dets;   // the largest d in [0, n_dets] with ev_ptr[d] + d <= c
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (ev_ptr[mid] + mid <= c) lo = mid; else hi = mid - 1;
    }
    if (lo >= n_dets) return false;
    const int64_t e0 = ev_ptr[lo], k = ev_ptr[lo + 1] - e0, i = c - (e0 + lo);
    // boundary j of the entry: 0, its positions, hw
    auto bound = [&](int64_t j) -> int64_t {
        if (j <= 0) return 0;
        if (j > k) return hw;
        const int64_t e = e0 + j - 1;
        return e < n_events ? (int64_t)event_pos[e] : hw;
    };
    int64_t x = bound(i + 1) - bound(i);
    if (i >= 3) x -= bound(i - 1) - bound(i - 2);
    *value = x;
    return true;
}

// rleToString's loop: the characters of one value, low groups first; returns their number
template <class Put>
__device__ __forceinline__ int enc_groups(int64_t x, Put put) {
    int n = 0;
    bool more = true;
    while (more) {
        int c = (int)(x & 0x1f);
        x >>= 5;   // arithmetic
        more = (c & 0x10) ? x != -1 : x != 0;
        if (more) c |= 0x20;
        put(n, (unsigned char)(c + 48));
        ++n;
    }
    return n;
}

__global__ __launch_bounds__(THREADS) void k_enc_lengths(const int64_t* __restrict__ ev_ptr, int64_t n_dets, const int* __restrict__ event_pos,
                                                         int64_t n_events, int64_t hw, int64_t n_counts, int64_t* __restrict__ len) {
    const int64_t c = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (c > n_counts) return;
    int64_t x = 0;
    int n = 0;
    if (c < n_counts && enc_value(c, ev_ptr, n_dets, event_pos, n_events, hw, &x)) n = enc_groups(x, [](int, unsigned char) {});
    len[c] = n;   // len[n_counts] = 0: the scan's last entry is the number of bytes
}

__global__ __launch_bounds__(THREADS) void k_enc_write(const int64_t* __restrict__ ev_ptr, int64_t n_dets, const int* __restrict__ event_pos,
                                                       int64_t n_events, int64_t hw, int64_t n_counts, const int64_t* __restrict__ off,
                                                       unsigned char* __restrict__ bytes, int64_t capacity, int64_t* __restrict__ str_ptr) {
    const int64_t c = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (c <= n_dets) {   // (n_dets <= n_counts) the string of entry c begins at its first count
        int64_t first = ev_ptr[c] + c;
        first = first < n_counts ? first : n_counts;
        str_ptr[c] = off[first];
    }
    if (c >= n_counts) return;
    int64_t x = 0;
    if (!enc_value(c, ev_ptr, n_dets, event_pos, n_events, hw, &x)) return;
    const int64_t at = off[c];
    // (positions that are not sorted give values of more than 7 characters: never write past the buffer)
    enc_groups(x, [&](int g, unsigned char ch) { if (at + g < capacity) bytes[at + g] = ch; });
}

struct EncView { int64_t* ev_cnt; int64_t* ev_ptr; int64_t* len; int64_t* off; void* tmp; size_t tmp_bytes; size_t bytes; };
static EncView enc_view(void* workspace, int64_t n_dets, int64_t n_events) {
    Carver c(workspace);
    const size_t nd = (size_t)n_dets + 1, nc = (size_t)(n_dets + n_events) + 1;
    const size_t tmp_bytes = exclusive_scan_temp<int64_t>((int64_t)nc);
    EncView v = {c.take<int64_t>(nd), c.take<int64_t>(nd), c.take<int64_t>(nc), c.take<int64_t>(nc), c.take<char>(tmp_bytes), tmp_bytes, 0};
    v.bytes = c.bytes();
    return v;
}

// ------------------------------------------------------------------------------------------------ decode
__device__ __forceinline__ uint64_t wave_inclusive_sum(uint64_t v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t o = (uint64_t)__shfl_up((unsigned long long)v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}
__device__ __forceinline__ uint64_t lane63(uint64_t v) { return (uint64_t)__shfl((unsigned long long)v, 63, 64); }

// One string by one wavefront.  WRITE false: its numbers (count pass); true: its runs at run_* [first, limit).
struct StringTotals { int n_counts, n_runs, status; int64_t area; };
template <bool WRITE>
__device__ __forceinline__ StringTotals walk_string(const unsigned char* __restrict__ s, int64_t len, int64_t hw, int lane, int row, int64_t first,
                                                    int64_t limit, int* __restrict__ run_row, int* __restrict__ run_begin,
                                                    int* __restrict__ run_end) {
    int n_counts = 0, n_runs = 0, status = 0;
    bool prev_end = true;                            // the character before the chunk ended a count (or the string begins)
    uint64_t c_odd = 0, c_even = 0, c_pos = 0, area = 0;   // carries: the sums over the odd / the even (>= 2) places, the position
    for (int64_t base = 0; base < len; base += 64) {
        const int64_t p = base + lane;
        const bool in = p < len;
        const int raw = in ? (int)s[p] - 48 : 0;
        const bool bad = in && (raw < 0 || raw > 63);
        const bool end = in && (raw & 0x20) == 0;
        const unsigned long long ends = __ballot(end);
        const bool before_ends = lane == 0 ? prev_end : ((ends >> (lane - 1)) & 1ull) != 0;
        bool start = in && before_ends;
        // the value: the groups from here to the first one that announces no other, inside the string
        uint64_t x = 0;
        bool too_long = false;
        if (start) {
            int g = 0, c = raw;
            int64_t q = p;
            for (;;) {
                x |= (uint64_t)(c & 0x1f) << (5 * g);
                ++g;
                if ((c & 0x20) == 0) break;
                if (g == MAX_GROUPS) { too_long = true; break; }
                if (++q >= len) break;
                c = (int)s[q] - 48;
            }
            if ((c & 0x20) != 0) { start = false; x = 0; }            // too long or cut off: no count
            else if (c & 0x10) x |= ~0ull << (5 * g);                  // sign extension (g <= 12)
        }
        if (__ballot(bad)) status |= ST_CHAR;
        if (__ballot(too_long)) status |= ST_LONG;
        if (__ballot(in && p == len - 1 && (raw & 0x20) != 0)) status |= ST_TRUNCATED;
        const unsigned long long starts = __ballot(start);
        const int ci = n_counts + __popcll(starts & ((1ull << lane) - 1ull));      // index of this lane's count
        const bool odd = (ci & 1) != 0;
        const uint64_t s_odd = wave_inclusive_sum(start && odd ? x : 0, lane);
        const uint64_t s_even = wave_inclusive_sum(start && !odd && ci >= 2 ? x : 0, lane);
        uint64_t out = 0;                                                         // the count itself
        if (start) out = ci == 0 ? x : (odd ? c_odd + s_odd : c_even + s_even);
        const uint64_t pos = c_pos + wave_inclusive_sum(out, lane);                // the position behind the count
        const bool negative = start && (int64_t)out < 0;
        const bool outside = start && ((int64_t)pos < 0 || (int64_t)pos >= POS_END);
        if (__ballot(negative)) status |= ST_NEGATIVE;
        if (__ballot(outside)) status |= ST_SUM;
        const bool run = start && odd && (int64_t)out > 0;
        const unsigned long long runs = __ballot(run);
        area += lane63(wave_inclusive_sum(start && odd ? out : 0, lane));
        if (WRITE) {
            const int64_t at = first + n_runs + __popcll(runs & ((1ull << lane) - 1ull));
            if (run && !negative && !outside && at < limit && (int64_t)(pos - out) >= 0) {
                run_row[at] = row;
                run_begin[at] = (int)(pos - out);
                run_end[at] = (int)pos;
            }
        }
        n_runs += __popcll(runs);
        n_counts += __popcll(starts);
        c_odd += lane63(s_odd);
        c_even += lane63(s_even);
        c_pos = lane63(pos);
        prev_end = ((ends >> 63) & 1ull) != 0;
    }
    if ((int64_t)c_pos != hw) status |= ST_SUM;
    if ((status & (ST_CHAR | ST_TRUNCATED | ST_LONG)) != 0) status &= ST_CHAR | ST_TRUNCATED | ST_LONG;   // no counts: nothing to say of them
    StringTotals t = {n_counts, n_runs, status, (int64_t)area};
    return t;
}

// the bytes of string i, inside the buffer whatever str_ptr holds
__device__ __forceinline__ void string_range(const int64_t* __restrict__ str_ptr, int64_t i, int64_t n_bytes, int64_t* b0, int64_t* b1) {
    int64_t a = str_ptr[i], b = str_ptr[i + 1];
    a = a < 0 ? 0 : (a > n_bytes ? n_bytes : a);
    b = b < a ? a : (b > n_bytes ? n_bytes : b);
    *b0 = a;
    *b1 = b;
}

__global__ __launch_bounds__(THREADS) void k_dec_scan(const unsigned char* __restrict__ bytes, int64_t n_bytes, const int64_t* __restrict__ str_ptr,
                                                      const int64_t* __restrict__ hw_per_string, int64_t n, int* __restrict__ n_counts,
                                                      int* __restrict__ n_runs, int64_t* __restrict__ area, int* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (i >= n) return;   // (the whole wavefront)
    int64_t b0, b1;
    string_range(str_ptr, i, n_bytes, &b0, &b1);
    const StringTotals t = walk_string<false>(bytes + b0, b1 - b0, hw_per_string[i], lane, (int)i, 0, 0, nullptr, nullptr, nullptr);
    if (lane == 0) {
        n_counts[i] = t.n_counts;
        n_runs[i] = t.status ? 0 : t.n_runs;   // a refused string has no runs: run_ptr has no gaps
        area[i] = t.status ? 0 : t.area;
        status[i] = t.status;
    }
}

// runs per string as int64, [n] and a zero behind; a string with a status has none
__global__ void k_dec_run_counts(const int* __restrict__ n_runs, const int* __restrict__ status, int64_t n, int64_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    const int v = (i < n && status[i] == 0) ? n_runs[i] : 0;
    out[i] = v > 0 ? v : 0;
}

__global__ __launch_bounds__(THREADS) void k_dec_runs(const unsigned char* __restrict__ bytes, int64_t n_bytes, const int64_t* __restrict__ str_ptr,
                                                      const int64_t* __restrict__ hw_per_string, int64_t n, const int* __restrict__ status,
                                                      const int64_t* __restrict__ run_ptr, int64_t total_runs, int* __restrict__ run_row,
                                                      int* __restrict__ run_begin, int* __restrict__ run_end) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (i >= n || status[i] != 0) return;   // (the whole wavefront)
    int64_t b0, b1;
    string_range(str_ptr, i, n_bytes, &b0, &b1);
    int64_t first = run_ptr[i], limit = run_ptr[i + 1];
    limit = limit < total_runs ? limit : total_runs;
    if (first < 0 || first >= limit) return;
    walk_string<true>(bytes + b0, b1 - b0, hw_per_string[i], lane, (int)i, first, limit, run_row, run_begin, run_end);
}

struct DecView { int64_t* runs64; void* tmp; size_t tmp_bytes; size_t bytes; };
static DecView dec_view(void* workspace, int64_t n) {
    Carver c(workspace);
    const size_t tmp_bytes = exclusive_scan_temp<int64_t>(n + 1);
    DecView v = {c.take<int64_t>((size_t)n + 1), c.take<char>(tmp_bytes), tmp_bytes, 0};
    v.bytes = c.bytes();
    return v;
}

static unsigned wave_blocks(int64_t n) { return (unsigned)((n + WAVES - 1) / WAVES); }

}  // namespace
}  // namespace mpnhip

using namespace mpnhip;

extern "C" size_t mpnhip_rle_encode_workspace_bytes(int64_t n_dets, int64_t n_events) {
    if (!enc_sizes_ok(n_dets, n_events, 0) || n_dets == 0) return 0;
    return enc_view(nullptr, n_dets, n_events).bytes + 256;
}

extern "C" int mpnhip_rle_encode(const int32_t* event_pos, const int32_t* det_counts, int64_t n_dets, int64_t n_events, int64_t hw,
                                 unsigned char* bytes, int64_t bytes_capacity, int64_t* str_ptr, void* workspace, size_t workspace_bytes,
                                 void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(enc_sizes_ok(n_dets, n_events, hw), "rle_encode: bad sizes (H * W and the number of events must stay below 2^31)");
    MPN_CHECK_ARG(bytes_capacity >= 7 * (n_events + n_dets),
                  "rle_encode: bytes_capacity %lld is less than 7 * (n_events + n_dets) = %lld", (long long)bytes_capacity,
                  (long long)(7 * (n_events + n_dets)));
    if (n_dets == 0) {   // no string: one offset, where the caller gave room for it
        if (str_ptr) MPN_HIP(hipMemsetAsync(str_ptr, 0, 8, stream));
        return MPNHIP_OK;
    }
    MPN_CHECK_ARG(str_ptr && det_counts && bytes && (n_events == 0 || event_pos), "rle_encode: null pointer");
    EncView v = enc_view(workspace, n_dets, n_events);
    MPN_CHECK_WORKSPACE("rle_encode", workspace, workspace_bytes, v.bytes);
    const int64_t n_counts = n_dets + n_events;
    hipLaunchKernelGGL(k_enc_entry_counts, dim3(blocks_for(n_dets + 1)), dim3(256), 0, stream, det_counts, n_dets, v.ev_cnt);
    MPN_LAUNCH_CHECK();
    MPN_HIP(rocprim::exclusive_scan(v.tmp, v.tmp_bytes, v.ev_cnt, v.ev_ptr, (int64_t)0, (size_t)(n_dets + 1), rocprim::plus<int64_t>(), stream));
    hipLaunchKernelGGL(k_enc_lengths, dim3(blocks_for(n_counts + 1)), dim3(THREADS), 0, stream, v.ev_ptr, n_dets, event_pos, n_events, hw,
                       n_counts, v.len);
    MPN_LAUNCH_CHECK();
    MPN_HIP(rocprim::exclusive_scan(v.tmp, v.tmp_bytes, v.len, v.off, (int64_t)0, (size_t)(n_counts + 1), rocprim::plus<int64_t>(), stream));
    hipLaunchKernelGGL(k_enc_write, dim3(blocks_for(n_counts + 1)), dim3(THREADS), 0, stream, v.ev_ptr, n_dets, event_pos, n_events, hw, n_counts,
                       v.off, bytes, bytes_capacity, str_ptr);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}

extern "C" size_t mpnhip_rle_decode_workspace_bytes(int64_t n) {
    if (!dec_sizes_ok(n, 0) || n == 0) return 0;
    return dec_view(nullptr, n).bytes + 256;
}

extern "C" int mpnhip_rle_decode_scan(const unsigned char* bytes, int64_t n_bytes, const int64_t* str_ptr, const int64_t* hw_per_string,
                                      int64_t n, int32_t* n_counts, int32_t* n_runs, int64_t* area, int32_t* status, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(dec_sizes_ok(n, n_bytes), "rle_decode_scan: bad sizes (at most 2^30 strings, their bytes below 2^31)");
    if (n == 0) return MPNHIP_OK;
    MPN_CHECK_ARG(str_ptr && hw_per_string && n_counts && n_runs && area && status && (n_bytes == 0 || bytes), "rle_decode_scan: null pointer");
    hipLaunchKernelGGL(k_dec_scan, dim3(wave_blocks(n)), dim3(THREADS), 0, stream, bytes, n_bytes, str_ptr, hw_per_string, n, n_counts, n_runs,
                       area, status);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}

extern "C" int mpnhip_rle_decode_runs(const unsigned char* bytes, int64_t n_bytes, const int64_t* str_ptr, const int64_t* hw_per_string,
                                      int64_t n, const int32_t* n_runs, const int32_t* status, int64_t total_runs, int64_t* run_ptr,
                                      int32_t* run_row, int32_t* run_begin, int32_t* run_end, void* workspace, size_t workspace_bytes,
                                      void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MPN_CHECK_ARG(dec_sizes_ok(n, n_bytes) && total_runs >= 0 && total_runs < (1LL << 31),
                  "rle_decode_runs: bad sizes (at most 2^30 strings, their bytes and their runs below 2^31)");
    if (n == 0) {   // no string: one offset, where the caller gave room for it
        if (run_ptr) MPN_HIP(hipMemsetAsync(run_ptr, 0, 8, stream));
        return MPNHIP_OK;
    }
    MPN_CHECK_ARG(run_ptr && str_ptr && hw_per_string && n_runs && status && (n_bytes == 0 || bytes), "rle_decode_runs: null pointer");
    MPN_CHECK_ARG(total_runs == 0 || (run_row && run_begin && run_end), "rle_decode_runs: null runs");
    DecView v = dec_view(workspace, n);
    MPN_CHECK_WORKSPACE("rle_decode_runs", workspace, workspace_bytes, v.bytes);
    hipLaunchKernelGGL(k_dec_run_counts, dim3(blocks_for(n + 1)), dim3(256), 0, stream, n_runs, status, n, v.runs64);
    MPN_LAUNCH_CHECK();
    MPN_HIP(rocprim::exclusive_scan(v.tmp, v.tmp_bytes, v.runs64, run_ptr, (int64_t)0, (size_t)(n + 1), rocprim::plus<int64_t>(), stream));
    if (total_runs == 0) return MPNHIP_OK;
    hipLaunchKernelGGL(k_dec_runs, dim3(wave_blocks(n)), dim3(THREADS), 0, stream, bytes, n_bytes, str_ptr, hw_per_string, n, status, run_ptr,
                       total_runs, run_row, run_begin, run_end);
    MPN_LAUNCH_CHECK();
    return MPNHIP_OK;
}
