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
//   score_rows_kernel  one lane per run-table row: (c, k) by binary search in the first-row table, then run_fields (the arithmetic
//                      the dense sweep runs per node): a, b and the keep bits in float64, ten coverage look-ups advanced together
//                      (ten independent loads per step), then add_group: a butterfly sum over the lanes of the wave that share
//                      (c, k) and one vector global atomic add on int64 per (min_length, field) -- integer sums: whatever order
//                      the waves arrive in, the bytes are the same.
// Every index read is clamped to the index, every row read to the caller's row count.  No LDS in the row kernel, no scratch.
#pragma clang fp contract(off)
// The limits of the sweep whose workspace this reads, the scan, run_fields, add_group and the checks of the entry point
// (check_scorer, shared with lad_score_events) are lad_sweep_tile.h's.
#include "lad_sweep_tile.h"

namespace {
using namespace lad::sweep;
constexpr int FIELDS = SCORE_FIELDS;               // n_pred, n_valid, pred_ms, corr_ms, fp_speech_ms, fp_noise_ms, fp_silence_ms

// the scans of lad_sweep_tile.h: cum per (channel, class), and each run table's first row
__global__ __launch_bounds__(THREADS) void score_scan_kernel(const int32_t *__restrict__ bounds, const int32_t *__restrict__ offsets,
                                                             int64_t n_intervals, int32_t *__restrict__ cum, int64_t segments,
                                                             const int32_t *__restrict__ counts, int64_t CK,
                                                             int64_t *__restrict__ first_row) {
    scan_index_and_counts(bounds, offsets, n_intervals, cum, segments, counts, CK, first_row);
}

// the seven integers of a row and its keep bits, as add_group sums them: field f counts for min_length l iff the run is kept there
struct RunScores {
    int32_t v[FIELDS];
    unsigned keep;                // bit l: the run passes min_length l
    __device__ static constexpr bool has(int) { return true; }
    __device__ long long operator()(int l, int f) const { return ((keep >> l) & 1u) ? (long long)v[f] : 0ll; }
};

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
    RunScores r;
#pragma unroll
    for (int f = 0; f < FIELDS; ++f) r.v[f] = 0;
    r.keep = 0;
    if (valid) {
        g = table_of_row(first_row, CK, row);
        const int c = (int)(g / K);
        // run_fields is the arithmetic of the dense sweep's nodes.  A row of one frame (first == last) is the empty interval (a, a]:
        // pred_ms = 0 and every overlap is 0 whatever the look-ups say, and n_valid is 1 iff the channel has no INVALID interval, so
        // run_fields skips the look-ups there and reads that from the offsets themselves; lad_score_runs has checked them on the
        // host (check_index), so they equal the clamped ones coverage_pairs would use.  Any other row goes through the same expressions.
        r.keep = run_fields(c, table[2 * row], table[2 * row + 1], fps[c], ml, L, bounds, cum, offsets, n_intervals, r.v);
    }
    // sums over the lanes that share (c, k), one (c, k) at a time (rows ascend with c * K + k: mostly one or two per wave)
    unsigned long long todo = __ballot(valid);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const long long gl = __shfl(g, leader, WAVE);
        const bool in = valid && g == gl;
        add_group<FIELDS>(in, gl, CK, L, lane, r, scores);
        todo &= ~__ballot(in);
    }
}

using lad::up256;

}  // namespace

extern "C" int32_t lad_score_max_min_lengths(void) { return MAX_L; }

extern "C" int64_t lad_score_workspace_bytes(int64_t channels, int64_t n_intervals, int32_t n_thresholds, int32_t n_min_lengths) {
    if (!score_sizes_ok(channels, n_intervals, n_thresholds, n_min_lengths)) {
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
    const int K = n_thresholds, L = n_min_lengths;
    const int64_t CK = channels * K;
    MinLengths ml;
    int64_t rows;
    if (int rc = check_scorer("lad_score_runs", nullptr, runs_workspace, table, counts_host, channels, frames, K, bounds, offsets, bounds_host,
                              offsets_host, n_intervals, fps, fps_host, min_lengths, L, workspace, scores, ml, rows))
        return rc;

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
