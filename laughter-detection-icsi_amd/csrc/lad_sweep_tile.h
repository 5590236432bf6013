// What the threshold sweep's sources share (runs.hip, binarize.hip, score.hip): the tile geometry and the limits of a call, the fixed
// load of a probability, run starts / ends of a tile's ballot words and their placement by rank, the workgroup scan, and the host
// checks whose messages differ only in the entry point's name and in what it calls its K axis ("thresholds" / "settings").
// lad_score_runs reads the workspace the other two wrote, so there is one definition of each.
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
}  // namespace sweep
}  // namespace lad
