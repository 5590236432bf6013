// What the threshold sweep's sources share (runs.hip, binarize.hip, score.hip, events.hip): the tile geometry and the limits of a
// call, the fixed load of a probability, run starts / ends of a tile's ballot words and their placement by rank, the workgroup scan,
// what the scorers do alike with a run-table row and the interval index (the scans in front, the table a row belongs to, the
// coverage look-up, the seven integers of a run (run_fields: score.hip and the dense pair), the wave sum and the sum over the lanes
// of a wave that share a table (add_group: score.hip, events.hip)), and the host checks whose messages differ only in the entry
// point's name and in what it calls its K axis ("thresholds" / "settings"): among them everything lad_score_runs and
// lad_score_events ask before they launch (check_scorer) and the largest number of events of one channel (most_events_of).
// lad_score_runs and lad_score_events read the workspace the other two wrote, so there is one definition of each.
// calibration.hip (the label histogram of a track) takes from here the fixed load, the index scan, the coverage look-up and the
// index's half of the host checks (check_index_intervals).
#pragma once
#include <cmath>

#include "lad_common.h"

namespace lad {
namespace sweep {
constexpr int WAVE = 64;
constexpr int WORDS = 8;                    // 64-frame words per tile
constexpr int TILE = WAVE * WORDS;          // frames per wave: lad_runs_tile_frames()
constexpr int WAVES = 4;                    // tiles per workgroup
constexpr int THREADS = WAVE * WAVES;
constexpr int MAX_K = 64;                   // thresholds / settings per call: lane k of a wave carries number k's count / first row
constexpr int64_t MAX_T = (int64_t)1 << 30; // frame indices and per-threshold run counts are int32
constexpr int MAX_C = 65535;                // grid.y
constexpr int CLASSES = 5;                  // of the interval index: INVALID, LAUGH, SPEECH, NOISE, SILENCE (enum lad_score_class)
constexpr int MAX_L = 8;                    // min_lengths per scoring call: lane l * 7 + f of a wave carries one sum
constexpr int64_t MAX_INTERVALS = (int64_t)1 << 30;
constexpr int64_t MAX_ROWS = (int64_t)1 << 38;     // grid.x of a kernel with one lane per run-table row
constexpr double MS = 1000.0;               // utils.to_frames: 1000 / frame_duration, frame_duration = 1 ms

struct MinLengths {
    double v[MAX_L];
};

// fix_over_underflow in float64 (the reference maps Python floats)
template <typename T>
__device__ inline double load_fixed(const T *__restrict__ p, int64_t i, int64_t n) {
    if (i < 0 || i >= n) return __builtin_nan("");   // beyond the track: off for every threshold (NaN > t is false)
    double v = (double)p[i];
    if (v > 1.0) v = 1.0;
    else if (v <= 0.0) v = 0.0000001;
    return v;
}

// a tile's frames: lane l of word j = frame tile0 + 64 j + l
template <typename T>
__device__ inline void load_tile(const T *__restrict__ chan, int64_t tile0, int64_t n, int lane, double (&v)[WORDS]) {
#pragma unroll
    for (int j = 0; j < WORDS; ++j) v[j] = load_fixed(chan, tile0 + j * WAVE + lane, n);
}

// run starts / ends inside word j of a tile's on/off mask; bit 0 of before / behind: the state of the frame across the tile's edge
__device__ inline unsigned long long starts_of(const unsigned long long (&m)[WORDS], int j, unsigned long long before) {
    const unsigned long long prev = j == 0 ? (before & 1ull) : (m[j - 1] >> 63);
    return m[j] & ~((m[j] << 1) | prev);
}
__device__ inline unsigned long long ends_of(const unsigned long long (&m)[WORDS], int j, unsigned long long behind) {
    const unsigned long long next = j == WORDS - 1 ? (behind & 1ull) : (m[j + 1] & 1ull);
    return m[j] & ~((m[j] >> 1) | (next << 63));
}

// the runs of one tile into the table whose row `row` takes the first run that starts in the tile: a start at frame i goes to row
// + (starts before i), the end at frame i closes the run of rank (starts at frames <= i) - 1, so the same count places both columns
__device__ inline void place_runs(const unsigned long long (&m)[WORDS], unsigned long long before, unsigned long long behind,
                                  int64_t tile0, int lane, long long row, int64_t capacity, int32_t *__restrict__ table) {
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int j = 0; j < WORDS; ++j) {
        const unsigned long long s = starts_of(m, j, before), e = ends_of(m, j, behind);
        const int32_t frame = (int32_t)(tile0 + j * WAVE + lane);
        const int upto = __popcll(s & below);                   // starts in this word below this lane
        const int is_start = (int)((s >> lane) & 1ull);
        if (is_start) {
            const long long at = row + upto;
            if (at >= 0 && at < capacity) table[2 * at] = frame;
        }
        if ((e >> lane) & 1ull) {
            const long long at = row + upto + is_start - 1;      // (starts at frames <= this one) - 1
            if (at >= 0 && at < capacity) table[2 * at + 1] = frame;
        }
        row += __popcll(s);
    }
}

// exclusive scan of load(i), i in [lo, hi), by one workgroup of THREADS: store(i, sum of load(j) for lo <= j < i); returns the
// total in every thread
template <typename Acc, typename Load, typename Store>
__device__ inline Acc block_scan(int64_t lo, int64_t hi, Load load, Store store) {
    __shared__ Acc wave_sum[WAVES];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    Acc carry = 0;
    for (int64_t base = lo; base < hi; base += THREADS) {
        const int64_t i = base + threadIdx.x;
        const Acc x = i < hi ? (Acc)load(i) : (Acc)0;
        Acc incl = x;
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) {
            const Acc y = __shfl_up(incl, d, WAVE);
            if (lane >= d) incl += y;
        }
        if (lane == WAVE - 1) wave_sum[wave] = incl;
        __syncthreads();
        Acc before = carry, all = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            if (w < wave) before += wave_sum[w];
            all += wave_sum[w];
        }
        if (i < hi) store(i, before + incl - x);
        carry += all;
        __syncthreads();
    }
    return carry;
}

// ---- the scorers (score.hip, events.hip) ----------------------------------------------------------------------------------------
// the scans in front of a scorer, one workgroup each: workgroup s < segments: cum[i] = total length of the intervals before i in the
// same (channel, class) s; workgroup `segments`: first_row[i] = rows of the run tables before table i (the counts lad_runs_count /
// lad_binarize_fill left at the start of their workspace)
__device__ inline void scan_index_and_counts(const int32_t *__restrict__ bounds, const int32_t *__restrict__ offsets, int64_t n_intervals,
                                             int32_t *__restrict__ cum, int64_t segments, const int32_t *__restrict__ counts, int64_t CK,
                                             int64_t *__restrict__ first_row) {
    if ((int64_t)blockIdx.x == segments) {
        block_scan<long long>(0, CK, [&](int64_t i) { return counts[i]; }, [&](int64_t i, long long v) { first_row[i] = v; });
        return;
    }
    int64_t o0 = offsets[blockIdx.x], o1 = offsets[blockIdx.x + 1];
    o0 = o0 < 0 ? 0 : (o0 > n_intervals ? n_intervals : o0);
    o1 = o1 < o0 ? o0 : (o1 > n_intervals ? n_intervals : o1);
    block_scan<long long>(o0, o1, [&](int64_t i) { return bounds[2 * i + 1] - bounds[2 * i]; },
                          [&](int64_t i, long long v) { cum[i] = (int32_t)v; });
}

__device__ inline long long wave_sum64(long long s) {
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) s += __shfl_xor(s, d, WAVE);
    return s;
}

// the table a row belongs to: the last (c, k) whose first row is <= row (an empty table shares its first row with the next one, so
// the last such table is the one that holds the row)
__device__ inline long long table_of_row(const int64_t *__restrict__ first_row, int64_t CK, int64_t row) {
    int64_t at = 0, n = CK;
    while (n > 1) {
        const int64_t half = n >> 1;
        if (first_row[at + half] <= row) at += half;
        n -= half;
    }
    return at;
}

// a run's seconds, its keep bits (bit l: end - start > min_length l) and its millisecond interval (x[0], x[1]]
__device__ inline unsigned run_ms(int32_t first, int32_t last, double fps, const MinLengths &ml, int L, int32_t (&x)[2]) {
    const double start = (double)first / fps, end = (double)last / fps;
    const double len = end - start;
    unsigned keep = 0;
#pragma unroll
    for (int l = 0; l < MAX_L; ++l)
        if (l < L && len > ml.v[l]) keep |= 1u << l;
    x[0] = (int32_t)rint(start * MS);
    x[1] = (int32_t)rint(end * MS);
    return keep;
}

// F[2 j + s] = coverage of class j of channel c in (0, x[s]], j < NC: 2 NC searches advanced together (as many independent loads per
// step), base[s] ending at the last interval with lo < x, if there is one.  size[j]: intervals of the class.  Every read is clamped
// to the index.
template <int NC>
__device__ inline void coverage_pairs(int64_t c, const int32_t (&x)[2], const int32_t *__restrict__ bounds, const int32_t *__restrict__ cum,
                                      const int32_t *__restrict__ offsets, int64_t n_intervals, int32_t (&F)[2 * NC], int32_t (&size)[NC]) {
    int32_t base[2 * NC], left[2 * NC];
    int32_t longest = 0;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        int64_t o0 = offsets[c * CLASSES + j], o1 = offsets[c * CLASSES + j + 1];
        o0 = o0 < 0 ? 0 : (o0 > n_intervals ? n_intervals : o0);
        o1 = o1 < o0 ? o0 : (o1 > n_intervals ? n_intervals : o1);
        size[j] = (int32_t)(o1 - o0);
        base[2 * j] = base[2 * j + 1] = (int32_t)o0;
        left[2 * j] = left[2 * j + 1] = size[j];
        longest = size[j] > longest ? size[j] : longest;
    }
    for (int32_t n = longest; n > 1; n -= n >> 1) {
#pragma unroll
        for (int s = 0; s < 2 * NC; ++s) {
            const int32_t half = left[s] >> 1;
            if (half > 0) {
                const int32_t mid = base[s] + half;
                if (bounds[2 * (int64_t)mid] < x[s & 1]) base[s] = mid;
                left[s] -= half;
            }
        }
    }
#pragma unroll
    for (int s = 0; s < 2 * NC; ++s) {
        F[s] = 0;
        if (size[s >> 1] > 0) {
            const int32_t lo = bounds[2 * (int64_t)base[s]], hi = bounds[2 * (int64_t)base[s] + 1];
            const int32_t xs = x[s & 1];
            if (lo < xs) F[s] = cum[base[s]] + (xs < hi ? xs : hi) - lo;
        }
    }
}

// the seven integers of lad_score_runs for the run (first, last) of channel c (enum lad_score_field) and its keep bits; a run of
// one frame is the empty interval (a, a]: it covers nothing, so no look-up is made for it
constexpr int SCORE_FIELDS = 7;
__device__ inline unsigned run_fields(int64_t c, int32_t first, int32_t last, double fps, const MinLengths &ml, int L,
                                      const int32_t *__restrict__ bounds, const int32_t *__restrict__ cum,
                                      const int32_t *__restrict__ offsets, int64_t n_intervals, int32_t (&v)[SCORE_FIELDS]) {
    int32_t x[2];
    const unsigned keep = run_ms(first, last, fps, ml, L, x);
#pragma unroll
    for (int f = 0; f < SCORE_FIELDS; ++f) v[f] = 0;
    v[0] = 1;
    if (first == last) {
        v[1] = offsets[c * CLASSES + 1] > offsets[c * CLASSES] ? 0 : 1;      // pred_ms = 0: valid iff there is no INVALID interval
        return keep;
    }
    int32_t F[2 * CLASSES], size[CLASSES];
    coverage_pairs<CLASSES>(c, x, bounds, cum, offsets, n_intervals, F, size);
    const int32_t pred = (x[1] - x[0]) - (F[1] - F[0]);                      // |(a, b] \ INVALID|
    v[1] = size[0] > 0 ? (pred > 0 ? 1 : 0) : 1;                              // analyse.py:185-187
    v[2] = pred;
#pragma unroll
    for (int j = 1; j < CLASSES; ++j) v[2 + j] = F[2 * j + 1] - F[2 * j];
    return keep;
}

// value(l, f) of the lanes `in` of a wave that share table g -> out[g][l][f] (FIELDS values per min_length), one lane per sum;
// Value::has(f): whether the caller sums field f at all
template <int FIELDS, typename Value>
__device__ inline void add_group(bool in, long long g, int64_t CK, int L, int lane, Value value, unsigned long long *__restrict__ out) {
    long long mine = 0;
#pragma unroll
    for (int l = 0; l < MAX_L; ++l) {
        if (l < L) {
#pragma unroll
            for (int f = 0; f < FIELDS; ++f) {
                if (!value.has(f)) continue;
                const long long s = wave_sum64(in ? value(l, f) : 0ll);
                if (lane == l * FIELDS + f) mine = s;
            }
        }
    }
    if (lane < L * FIELDS && mine != 0 && g >= 0 && g < CK) atomicAdd(out + (g * L * FIELDS + lane), (unsigned long long)mine);
}

// ---- host side: `who` is the entry point, `what` its name for the K axis -------------------------------------------------------
inline int check_sizes(const char *who, const char *what, int64_t channels, int64_t frames, int32_t K) {
    LAD_REQUIRE(channels >= 1 && channels <= MAX_C && frames >= 1 && frames <= MAX_T && K >= 1 && K <= MAX_K,
                "%s: channels 1..%d, frames 1..2^30, %s 1..%d (got %lld, %lld, %d)", who, MAX_C, what, MAX_K, (long long)channels,
                (long long)frames, K);
    return LAD_OK;
}

// the rows of the n run tables whose counts the caller read back, or -1 (reported) if one is no run count of a track of `frames`
inline int64_t total_runs(const char *who, const int32_t *counts_host, int64_t n, int64_t frames) {
    int64_t total = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (counts_host[i] < 0 || counts_host[i] > (frames + 1) / 2) {
            fail(LAD_ERR_INVALID, "%s: counts_host[%lld] = %d is not a run count of a %lld-frame track", who, (long long)i, counts_host[i],
                 (long long)frames);
            return -1;
        }
        total += counts_host[i];
    }
    return total;
}

inline int check_fps(const char *who, const double *fps_host, int64_t channels) {
    for (int64_t c = 0; c < channels; ++c)
        LAD_REQUIRE(fps_host[c] > 0.0 && std::isfinite(fps_host[c]), "%s: fps[%lld] = %g is not a positive finite number", who,
                    (long long)c, fps_host[c]);
    return LAD_OK;
}

// what a scorer asks of its sizes (message by the caller: the two name different things)
inline bool score_sizes_ok(int64_t C, int64_t n_intervals, int64_t K, int64_t L) {
    return C >= 1 && C <= MAX_C && n_intervals >= 0 && n_intervals <= MAX_INTERVALS && K >= 1 && K <= MAX_K && L >= 1 && L <= MAX_L;
}

// the min_lengths of a scoring call as a kernel argument
inline int load_min_lengths(const char *who, const double *min_lengths, int L, MinLengths &ml) {
    for (int l = 0; l < MAX_L; ++l) {
        ml.v[l] = l < L ? min_lengths[l] : 0.0;
        LAD_REQUIRE(ml.v[l] == ml.v[l], "%s: min_lengths[%d] is NaN", who, l);
    }
    return LAD_OK;
}

// what the scorers and lad_label_histogram ask of the interval index before they launch anything: offsets ascend from 0 to
// n_intervals; within a (channel, class) intervals are non-empty, sorted and disjoint
inline int check_index_intervals(const char *who, int64_t channels, const int32_t *offsets_host, const int32_t *bounds_host,
                                 int64_t n_intervals) {
    LAD_REQUIRE(offsets_host[0] == 0 && offsets_host[channels * CLASSES] == n_intervals,
                "%s: index offsets run from %d to %d, expected 0 to %lld", who, offsets_host[0], offsets_host[channels * CLASSES],
                (long long)n_intervals);
    for (int64_t s = 0; s < channels * CLASSES; ++s) {
        const int64_t o0 = offsets_host[s], o1 = offsets_host[s + 1];
        LAD_REQUIRE(o0 <= o1 && o1 <= n_intervals, "%s: index offsets do not ascend at channel %lld, class %lld (%lld, %lld)", who,
                    (long long)(s / CLASSES), (long long)(s % CLASSES), (long long)o0, (long long)o1);
        for (int64_t i = o0; i < o1; ++i) {
            const int32_t lo = bounds_host[2 * i], hi = bounds_host[2 * i + 1];
            LAD_REQUIRE(lo >= 0 && hi > lo, "%s: index interval %lld (%d, %d] of channel %lld, class %lld is empty or negative", who,
                        (long long)i, lo, hi, (long long)(s / CLASSES), (long long)(s % CLASSES));
            LAD_REQUIRE(i == o0 || lo >= bounds_host[2 * i - 1],
                        "%s: index interval %lld (%d, %d] of channel %lld, class %lld is unsorted or overlaps the one before it", who,
                        (long long)i, lo, hi, (long long)(s / CLASSES), (long long)(s % CLASSES));
        }
    }
    return LAD_OK;
}

// what a scorer asks of the time base and the interval index before it launches anything: millisecond values are int32
// (to_frames(frames / fps) < 2^31 for every channel), then check_index_intervals (lad_label_histogram checks the time base per
// channel length instead and then asks the same of the index)
inline int check_index(const char *who, int64_t channels, int64_t frames, const double *fps_host, const int32_t *offsets_host,
                       const int32_t *bounds_host, int64_t n_intervals) {
    if (int rc = check_fps(who, fps_host, channels)) return rc;
    for (int64_t c = 0; c < channels; ++c) {
        const double f = fps_host[c];
        const double ms = std::nearbyint((double)frames / f * MS);
        LAD_REQUIRE(ms < 2147483648.0, "%s: millisecond overflow: %lld frames at fps[%lld] = %g end at %.0f ms, int32 holds 2^31 - 1", who,
                    (long long)frames, (long long)c, f, ms);
    }
    return check_index_intervals(who, channels, offsets_host, bounds_host, n_intervals);
}

inline int check_dtype(const char *who, int32_t dtype) {
    LAD_REQUIRE(dtype == LAD_RUNS_F32 || dtype == LAD_RUNS_F64, "%s: dtype %d (LAD_RUNS_F32 or LAD_RUNS_F64)", who, dtype);
    return LAD_OK;
}
// f(float{}) or f(double{}) for a dtype that check_dtype has passed
template <typename F>
inline void with_track_type(int32_t dtype, F f) {
    if (dtype == LAD_RUNS_F32) f(float{});
    else f(double{});
}

// the event criteria of lad_score_events and lad_score_surface_events
inline int check_criteria(const char *who, int32_t min_overlap_ms, int32_t min_overlap_pct) {
    LAD_REQUIRE(min_overlap_ms >= 0 && min_overlap_pct >= 0 && min_overlap_pct <= 100,
                "%s: min_overlap_ms >= 0, min_overlap_pct 0..100 (got %d, %d)", who, min_overlap_ms, min_overlap_pct);
    return LAD_OK;
}

// the LAUGH intervals of the channel that has most, from an index that check_index has passed
inline int64_t most_events_of(const int32_t *offsets_host, int64_t channels) {
    int64_t most = 0;
    for (int64_t c = 0; c < channels; ++c) {
        const int64_t n = offsets_host[c * CLASSES + LAD_SCORE_LAUGH + 1] - offsets_host[c * CLASSES + LAD_SCORE_LAUGH];
        most = n > most ? n : most;
    }
    return most;
}

// what lad_score_runs and lad_score_events (criteria: its two values, null for the other) ask before they launch anything, in
// this order: sizes, criteria, null buffers, min_lengths, the index, the run counts.  out: the entry point's result array.
// Gives the min_lengths as a kernel argument and the rows of all run tables together.
inline int check_scorer(const char *who, const int32_t *criteria, const void *runs_workspace, const int32_t *table,
                        const int32_t *counts_host, int64_t channels, int64_t frames, int32_t K, const int32_t *bounds,
                        const int32_t *offsets, const int32_t *bounds_host, const int32_t *offsets_host, int64_t n_intervals,
                        const double *fps, const double *fps_host, const double *min_lengths, int32_t L, const void *workspace,
                        const void *out, MinLengths &ml, int64_t &rows) {
    LAD_REQUIRE(score_sizes_ok(channels, n_intervals, K, L) && frames >= 1 && frames <= MAX_T,
                "%s: channels 1..%d, frames 1..2^30, intervals 0..2^30, thresholds 1..%d, min_lengths 1..%d "
                "(got %lld, %lld, %lld, %d, %d)",
                who, MAX_C, MAX_K, MAX_L, (long long)channels, (long long)frames, (long long)n_intervals, K, L);
    if (int rc = criteria ? check_criteria(who, criteria[0], criteria[1]) : LAD_OK) return rc;
    LAD_REQUIRE(runs_workspace && counts_host && offsets && offsets_host && fps && fps_host && min_lengths && workspace && out,
                "%s: null buffer", who);
    LAD_REQUIRE(n_intervals == 0 || (bounds && bounds_host), "%s: null interval bounds", who);
    if (int rc = load_min_lengths(who, min_lengths, L, ml)) return rc;
    if (int rc = check_index(who, channels, frames, fps_host, offsets_host, bounds_host, n_intervals)) return rc;
    rows = total_runs(who, counts_host, channels * K, frames);
    if (rows < 0) return LAD_ERR_INVALID;
    LAD_REQUIRE(rows <= MAX_ROWS, "%s: %lld run-table rows, at most 2^38 per call", who, (long long)rows);
    LAD_REQUIRE(rows == 0 || table, "%s: null table", who);
    return LAD_OK;
}
}  // namespace sweep
}  // namespace lad
