// Scores of the threshold sweep against transcript intervals: for every (channel, threshold, min_length) of a sweep whose run
// tables are already on the device (runs.hip), seven int64 counts -- kept runs, kept runs outside INVALID, and the milliseconds of
// the kept runs outside INVALID in total and inside LAUGH / SPEECH / NOISE / SILENCE.
//
// Replaces, for tracks in GPU memory, the evaluation of analysis/analyse.py: eval_preds :152-225 and laugh_match :120-149 (and with
// them the 87 TextGrid files per channel that segment_laughter.py writes and textgrid_to_df :49-61 reads back), on the interval
// index of analysis/preprocess.py:27-46, 49-120, 133-167 with the time base of analysis/utils.py:8-37.
//
// A run (first, last) of channel c is start = first / fps[c], end = last / fps[c] in float64, kept for min_length l iff
// end - start > l (laugh_segmenter.py:74-111), and the millisecond interval (a, b] = (rint(start * 1000), rint(end * 1000)]
// (utils.to_frames: Python's round, half to even).  IEEE division, no reciprocal, contraction off: the host computes the same bits.
//
// Index: per (channel, class) sorted, disjoint, non-empty intervals (lo, hi] (CSR: bounds[n][2], offsets[channels * 5 + 1];
// classes INVALID, LAUGH, SPEECH, NOISE, SILENCE), the last four with INVALID already subtracted by whoever built the index.
// Coverage F(x) = milliseconds of a class in (0, x] = cum[i] + min(x, hi_i) - lo_i for the last interval i with lo_i < x, where
// cum is the exclusive running length (score_scan_kernel: one scan per (channel, class): block_scan), so that
// |(a, b] n class| = F(b) - F(a): no set arithmetic here.
//
// Shape: two launches after one memset of the output.
//   score_scan_kernel  one workgroup per (channel, class): cum; one more: each run table's first row from the counts that
//                      lad_runs_count left at the start of its workspace
//   score_rows_kernel  one lane per run-table row: (c, k) by binary search in the first-row table, a, b and the
//                      keep bits in float64, ten coverage look-ups advanced together (ten independent loads per step), then a
//                      butterfly sum over the lanes of the wave that share (c, k) and one vector global atomic add on int64 per
//                      (min_length, field) -- integer sums: whatever order the waves arrive in, the bytes are the same.
// Every index read is clamped to the index, every row read to the caller's row count.  No LDS in the row kernel, no scratch.
#pragma clang fp contract(off)
// The limits of the sweep whose workspace this reads, and the scan, are lad_sweep_tile.h's.
#include "lad_sweep_tile.h"

namespace {
using namespace lad::sweep;
constexpr int CLASSES = 5;                         // INVALID, LAUGH, SPEECH, NOISE, SILENCE
constexpr int FIELDS = 7;                          // n_pred, n_valid, pred_ms, corr_ms, fp_speech_ms, fp_noise_ms, fp_silence_ms
constexpr int MAX_L = 8;                           // min_lengths per call: lane l * 7 + f of a wave carries one sum
constexpr int64_t MAX_INTERVALS = (int64_t)1 << 30;
constexpr int64_t MAX_ROWS = (int64_t)1 << 38;     // grid.x of the row kernel
constexpr double MS = 1000.0;                      // utils.to_frames: 1000 / frame_duration, frame_duration = 1 ms

struct MinLengths {
    double v[MAX_L];
};

// workgroup s < segments: cum[i] = total length of the intervals before i in the same (channel, class) s;
// workgroup `segments`: first_row[i] = rows of the run tables before table i (the counts lad_runs_count left in its workspace)
__global__ __launch_bounds__(THREADS) void score_scan_kernel(const int32_t *__restrict__ bounds, const int32_t *__restrict__ offsets,
                                                             int64_t n_intervals, int32_t *__restrict__ cum, int64_t segments,
                                                             const int32_t *__restrict__ counts, int64_t CK,
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

__global__ __launch_bounds__(THREADS) void score_rows_kernel(const int32_t *__restrict__ table, int64_t rows,
                                                             const int64_t *__restrict__ first_row, int64_t CK, int K,
                                                             const double *__restrict__ fps, MinLengths ml, int L,
                                                             const int32_t *__restrict__ bounds, const int32_t *__restrict__ cum,
                                                             const int32_t *__restrict__ offsets, int64_t n_intervals,
                                                             unsigned long long *__restrict__ scores) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t row = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    const bool valid = row < rows;
    long long g = 0;              // c * K + k of this row
    int32_t v[FIELDS];
#pragma unroll
    for (int f = 0; f < FIELDS; ++f) v[f] = 0;
    unsigned keep = 0;            // bit l: the run passes min_length l
    if (valid) {
        // the table this row belongs to: the last (c, k) whose first row is <= row (an empty table shares its first row with the
        // next one, so the last such table is the one that holds the row)
        {
            int64_t at = 0, n = CK;
            while (n > 1) {
                const int64_t half = n >> 1;
                if (first_row[at + half] <= row) at += half;
                n -= half;
            }
            g = at;
        }
        const int c = (int)(g / K);
        const double f = fps[c];
        const double start = (double)table[2 * row] / f, end = (double)table[2 * row + 1] / f;
        const double len = end - start;
#pragma unroll
        for (int l = 0; l < MAX_L; ++l)
            if (l < L && len > ml.v[l]) keep |= 1u << l;
        int32_t x[2];
        x[0] = (int32_t)rint(start * MS);
        x[1] = (int32_t)rint(end * MS);
        // ten searches (five classes x {a, b}) advanced together: base[s] ends at the last interval with lo < x, if there is one
        int32_t base[2 * CLASSES], left[2 * CLASSES], size[CLASSES];
        int32_t longest = 0;
#pragma unroll
        for (int j = 0; j < CLASSES; ++j) {
            int64_t o0 = offsets[(int64_t)c * CLASSES + j], o1 = offsets[(int64_t)c * CLASSES + j + 1];
            o0 = o0 < 0 ? 0 : (o0 > n_intervals ? n_intervals : o0);
            o1 = o1 < o0 ? o0 : (o1 > n_intervals ? n_intervals : o1);
            size[j] = (int32_t)(o1 - o0);
            base[2 * j] = base[2 * j + 1] = (int32_t)o0;
            left[2 * j] = left[2 * j + 1] = size[j];
            longest = size[j] > longest ? size[j] : longest;
        }
        for (int32_t n = longest; n > 1; n -= n >> 1) {
#pragma unroll
            for (int s = 0; s < 2 * CLASSES; ++s) {
                const int32_t half = left[s] >> 1;
                if (half > 0) {
                    const int32_t mid = base[s] + half;
                    if (bounds[2 * (int64_t)mid] < x[s & 1]) base[s] = mid;
                    left[s] -= half;
                }
            }
        }
        int32_t F[2 * CLASSES];
#pragma unroll
        for (int s = 0; s < 2 * CLASSES; ++s) {
            F[s] = 0;
            if (size[s >> 1] > 0) {
                const int32_t lo = bounds[2 * (int64_t)base[s]], hi = bounds[2 * (int64_t)base[s] + 1];
                const int32_t xs = x[s & 1];
                if (lo < xs) F[s] = cum[base[s]] + (xs < hi ? xs : hi) - lo;
            }
        }
        const int32_t pred = (x[1] - x[0]) - (F[1] - F[0]);      // |(a, b] \ INVALID|
        v[0] = 1;
        v[1] = size[0] > 0 ? (pred > 0 ? 1 : 0) : 1;              // analyse.py:185-187
        v[2] = pred;
#pragma unroll
        for (int j = 1; j < CLASSES; ++j) v[2 + j] = F[2 * j + 1] - F[2 * j];
    }
    // sums over the lanes that share (c, k), one (c, k) at a time (rows ascend with c * K + k: mostly one or two per wave)
    unsigned long long todo = __ballot(valid);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const long long gl = __shfl(g, leader, WAVE);
        const bool in = valid && g == gl;
        long long mine = 0;
#pragma unroll
        for (int l = 0; l < MAX_L; ++l) {
            if (l < L) {
                const bool on = in && ((keep >> l) & 1u);
#pragma unroll
                for (int f = 0; f < FIELDS; ++f) {
                    const long long s = wave_sum64(on ? (long long)v[f] : 0ll);
                    if (lane == l * FIELDS + f) mine = s;
                }
            }
        }
        if (lane < L * FIELDS && mine != 0 && gl >= 0 && gl < CK)
            atomicAdd(scores + (gl * L * FIELDS + lane), (unsigned long long)mine);
        todo &= ~__ballot(in);
    }
}

using lad::up256;

inline bool sizes_ok(int64_t C, int64_t n_intervals, int64_t K, int64_t L) {
    return C >= 1 && C <= MAX_C && n_intervals >= 0 && n_intervals <= MAX_INTERVALS && K >= 1 && K <= MAX_K && L >= 1 && L <= MAX_L;
}
}  // namespace

extern "C" int32_t lad_score_max_min_lengths(void) { return MAX_L; }

extern "C" int64_t lad_score_workspace_bytes(int64_t channels, int64_t n_intervals, int32_t n_thresholds, int32_t n_min_lengths) {
    if (!sizes_ok(channels, n_intervals, n_thresholds, n_min_lengths)) {
        lad::fail(LAD_ERR_INVALID,
                  "lad_score_workspace_bytes: channels 1..%d, intervals 0..2^30, thresholds 1..%d, min_lengths 1..%d (got %lld, %lld, %d, %d)",
                  MAX_C, MAX_K, MAX_L, (long long)channels, (long long)n_intervals, n_thresholds, n_min_lengths);
        return -1;
    }
    return up256(channels * n_thresholds * 8) + up256(n_intervals * 4) + 256;
}

extern "C" int lad_score_runs(const void *runs_workspace, const int32_t *table, const int32_t *counts_host, int64_t channels,
                              int64_t frames, int32_t n_thresholds, const int32_t *bounds, const int32_t *offsets,
                              const int32_t *bounds_host, const int32_t *offsets_host, int64_t n_intervals, const double *fps,
                              const double *fps_host, const double *min_lengths, int32_t n_min_lengths, void *workspace,
                              int64_t *scores, void *stream) {
    using namespace lad;
    LAD_REQUIRE(sizes_ok(channels, n_intervals, n_thresholds, n_min_lengths) && frames >= 1 && frames <= MAX_T,
                "lad_score_runs: channels 1..%d, frames 1..2^30, intervals 0..2^30, thresholds 1..%d, min_lengths 1..%d "
                "(got %lld, %lld, %lld, %d, %d)",
                MAX_C, MAX_K, MAX_L, (long long)channels, (long long)frames, (long long)n_intervals, n_thresholds, n_min_lengths);
    LAD_REQUIRE(runs_workspace && counts_host && offsets && offsets_host && fps && fps_host && min_lengths && workspace && scores,
                "lad_score_runs: null buffer");
    LAD_REQUIRE(n_intervals == 0 || (bounds && bounds_host), "lad_score_runs: null interval bounds");
    const int K = n_thresholds, L = n_min_lengths;
    const int64_t CK = channels * K;
    MinLengths ml;
    for (int l = 0; l < MAX_L; ++l) {
        ml.v[l] = l < L ? min_lengths[l] : 0.0;
        LAD_REQUIRE(ml.v[l] == ml.v[l], "lad_score_runs: min_lengths[%d] is NaN", l);
    }
    // millisecond values are int32: to_frames(frames / fps) < 2^31 for every channel
    if (int rc = check_fps("lad_score_runs", fps_host, channels)) return rc;
    for (int64_t c = 0; c < channels; ++c) {
        const double f = fps_host[c];
        const double ms = std::nearbyint((double)frames / f * MS);
        LAD_REQUIRE(ms < 2147483648.0,
                    "lad_score_runs: millisecond overflow: %lld frames at fps[%lld] = %g end at %.0f ms, int32 holds 2^31 - 1",
                    (long long)frames, (long long)c, f, ms);
    }
    // the index: offsets ascend from 0 to n_intervals; within a (channel, class) intervals are non-empty, sorted and disjoint
    LAD_REQUIRE(offsets_host[0] == 0 && offsets_host[channels * CLASSES] == n_intervals,
                "lad_score_runs: index offsets run from %d to %d, expected 0 to %lld", offsets_host[0],
                offsets_host[channels * CLASSES], (long long)n_intervals);
    for (int64_t s = 0; s < channels * CLASSES; ++s) {
        const int64_t o0 = offsets_host[s], o1 = offsets_host[s + 1];
        LAD_REQUIRE(o0 <= o1 && o1 <= n_intervals, "lad_score_runs: index offsets do not ascend at channel %lld, class %lld (%lld, %lld)",
                    (long long)(s / CLASSES), (long long)(s % CLASSES), (long long)o0, (long long)o1);
        for (int64_t i = o0; i < o1; ++i) {
            const int32_t lo = bounds_host[2 * i], hi = bounds_host[2 * i + 1];
            LAD_REQUIRE(lo >= 0 && hi > lo, "lad_score_runs: index interval %lld (%d, %d] of channel %lld, class %lld is empty or negative",
                        (long long)i, lo, hi, (long long)(s / CLASSES), (long long)(s % CLASSES));
            LAD_REQUIRE(i == o0 || lo >= bounds_host[2 * i - 1],
                        "lad_score_runs: index interval %lld (%d, %d] of channel %lld, class %lld is unsorted or overlaps the one before it",
                        (long long)i, lo, hi, (long long)(s / CLASSES), (long long)(s % CLASSES));
        }
    }
    const int64_t rows = total_runs("lad_score_runs", counts_host, CK, frames);
    if (rows < 0) return LAD_ERR_INVALID;
    LAD_REQUIRE(rows <= MAX_ROWS, "lad_score_runs: %lld run-table rows, at most 2^38 per call", (long long)rows);
    LAD_REQUIRE(rows == 0 || table, "lad_score_runs: null table");

    int64_t *first_row = (int64_t *)workspace;
    int32_t *cum = (int32_t *)((char *)workspace + up256(CK * 8));
    const hipStream_t st = (hipStream_t)stream;
    LAD_HIP_CHECK(hipMemsetAsync(scores, 0, (size_t)(CK * L * FIELDS) * sizeof(int64_t), st));
    if (rows == 0) return LAD_OK;
    const int64_t segments = channels * CLASSES;
    hipLaunchKernelGGL(score_scan_kernel, dim3((unsigned)(segments + 1)), dim3(THREADS), 0, st, bounds, offsets, n_intervals, cum, segments,
                       (const int32_t *)runs_workspace, CK, first_row);
    if (int rc = check_launch("score_scan_kernel")) return rc;
    hipLaunchKernelGGL(score_rows_kernel, dim3((unsigned)ceil_div(rows, THREADS)), dim3(THREADS), 0, st, table, rows, first_row, CK, K, fps,
                       ml, L, bounds, cum, offsets, n_intervals, (unsigned long long *)scores);
    return check_launch("score_rows_kernel");
}
