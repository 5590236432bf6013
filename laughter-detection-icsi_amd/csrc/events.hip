// Event-level scores of the threshold sweep: for every (channel, threshold, min_length) of a sweep whose run tables are on the
// device (runs.hip, binarize.hip), seven int64 values -- reference events, those touched and hit, predictions hit, links, and the
// summed onset / offset errors of the hit events.  The convention is include/lad_hip.h's (above lad_score_events); the time base,
// the keep rule, the index and the coverage function F are those of score.hip, through lad_sweep_tile.h.
//
// The reference counts events on both sides (analysis/analyse.py:255-257: num_of_pred_laughs, valid_pred_laughs,
// num_of_transc_laughs) and never matches them; this does.
//
// Shape: three launches after one memset of the output (two if there is no run: the events are still counted).
//   events_scan_kernel     one workgroup per (channel, class): cum; one more: each run table's first row (as score_scan_kernel)
//   events_prepare_kernel  one lane per run-table row: (c, k), a, b and the keep bits, |(a, b] n LAUGH| and |(a, b] \ INVALID| by
//                          four coverage look-ups advanced together; writes a, b, keep per row and sums PRED_HIT
//   events_match_kernel    grid.y = channel, one lane per (event, k) of it, events fastest: the first row of table (c, k) with
//                          b > lo by binary search in the b column, then a walk over the rows with a < hi, all inside rows
//                          first_row[g] .. first_row[g + 1] of that table; cov, frag, first a and last b per min_length in
//                          registers; the other six fields
// Both sum with a butterfly over the lanes of the wave that share (c, k) and one vector global atomic add on int64 per
// (min_length, field) (lad_sweep_tile.h: add_group, as score.hip): integer sums, the same bytes whatever order the waves arrive in.
// Every index read is clamped to the index, every row read to the caller's row count.  The checks of the entry point are
// check_scorer's, shared with lad_score_runs.
#pragma clang fp contract(off)
#include "lad_sweep_tile.h"

namespace {
using namespace lad::sweep;
constexpr int FIELDS = LAD_EVENT_FIELDS;

__global__ __launch_bounds__(THREADS) void events_scan_kernel(const int32_t *__restrict__ bounds, const int32_t *__restrict__ offsets,
                                                              int64_t n_intervals, int32_t *__restrict__ cum, int64_t segments,
                                                              const int32_t *__restrict__ counts, int64_t CK,
                                                              int64_t *__restrict__ first_row) {
    scan_index_and_counts(bounds, offsets, n_intervals, cum, segments, counts, CK, first_row);
}

struct PredHit {
    unsigned hit;      // bit l: kept for min_length l and hit
    __device__ static constexpr bool has(int f) { return f == LAD_EVENT_PRED_HIT; }
    __device__ long long operator()(int l, int) const { return (hit >> l) & 1u; }
};

__global__ __launch_bounds__(THREADS) void events_prepare_kernel(const int32_t *__restrict__ table, int64_t rows,
                                                                 const int64_t *__restrict__ first_row, int64_t CK, int K,
                                                                 const double *__restrict__ fps, MinLengths ml, int L,
                                                                 const int32_t *__restrict__ bounds, const int32_t *__restrict__ cum,
                                                                 const int32_t *__restrict__ offsets, int64_t n_intervals,
                                                                 int32_t min_ms, int32_t min_pct, int32_t *__restrict__ col_a,
                                                                 int32_t *__restrict__ col_b, int32_t *__restrict__ col_keep,
                                                                 unsigned long long *__restrict__ events) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t row = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    const bool valid = row < rows;
    long long g = 0;              // c * K + k of this row
    PredHit p{0};
    if (valid) {
        g = table_of_row(first_row, CK, row);
        const int64_t c = g / K;
        int32_t x[2];
        const unsigned keep = run_ms(table[2 * row], table[2 * row + 1], fps[c], ml, L, x);
        int32_t F[4], size[2];
        coverage_pairs<2>(c, x, bounds, cum, offsets, n_intervals, F, size);      // INVALID, LAUGH
        const long long pred = (long long)(x[1] - x[0]) - (F[1] - F[0]);          // |(a, b] \ INVALID|
        const long long lov = F[3] - F[2];                                        // |(a, b] n LAUGH|
        if (lov >= (min_ms > 1 ? min_ms : 1) && 100ll * lov >= (long long)min_pct * pred) p.hit = keep;
        col_a[row] = x[0];
        col_b[row] = x[1];
        col_keep[row] = (int32_t)keep;
    }
    // sums over the lanes that share (c, k), one (c, k) at a time (rows ascend with c * K + k: mostly one or two per wave)
    unsigned long long todo = __ballot(valid);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const long long gl = __shfl(g, leader, WAVE);
        const bool in = valid && g == gl;
        add_group<FIELDS>(in, gl, CK, L, lane, p, events);
        todo &= ~__ballot(in);
    }
}

struct EventSums {
    int32_t frag[MAX_L], onset[MAX_L], offset[MAX_L];
    unsigned hit;
    __device__ static constexpr bool has(int f) { return f != LAD_EVENT_PRED_HIT; }
    __device__ long long operator()(int l, int f) const {
        const long long h = (hit >> l) & 1u;
        return f == LAD_EVENT_N_REF ? 1 : f == LAD_EVENT_REF_TOUCHED ? (frag[l] > 0) : f == LAD_EVENT_REF_HIT ? h
             : f == LAD_EVENT_LINKS ? frag[l] : f == LAD_EVENT_ONSET_ABS_MS ? (h ? onset[l] : 0) : (h ? offset[l] : 0);
    }
};

__global__ __launch_bounds__(THREADS) void events_match_kernel(const int32_t *__restrict__ col_a, const int32_t *__restrict__ col_b,
                                                               const int32_t *__restrict__ col_keep, int64_t rows,
                                                               const int64_t *__restrict__ first_row, int64_t CK, int K, int L,
                                                               const int32_t *__restrict__ bounds, const int32_t *__restrict__ offsets,
                                                               int64_t n_intervals, int32_t min_ms, int32_t min_pct,
                                                               unsigned long long *__restrict__ events) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t c = blockIdx.y;
    // the LAUGH segment of channel c
    int64_t o0 = offsets[c * CLASSES + LAD_SCORE_LAUGH], o1 = offsets[c * CLASSES + LAD_SCORE_LAUGH + 1];
    o0 = o0 < 0 ? 0 : (o0 > n_intervals ? n_intervals : o0);
    o1 = o1 < o0 ? o0 : (o1 > n_intervals ? n_intervals : o1);
    const int64_t n_events = o1 - o0;
    const int64_t at = (int64_t)blockIdx.x * THREADS + threadIdx.x;      // k * n_events + event
    const bool valid = at < n_events * K;
    long long g = 0;
    EventSums s;
#pragma unroll
    for (int l = 0; l < MAX_L; ++l) s.frag[l] = s.onset[l] = s.offset[l] = 0;
    s.hit = 0;
    if (valid) {
        const int k = (int)(at / n_events);
        const int64_t e = o0 + at % n_events;
        g = c * K + k;
        const int32_t lo = bounds[2 * e], hi = bounds[2 * e + 1];
        // table (c, k): rows r0 .. r1 - 1 (an empty table: r0 == r1), inside the caller's row count
        int64_t r0 = first_row[g], r1 = g + 1 < CK ? first_row[g + 1] : rows;
        r0 = r0 < 0 ? 0 : (r0 > rows ? rows : r0);
        r1 = r1 < r0 ? r0 : (r1 > rows ? rows : r1);
        // the first row of the table with b > lo (b does not decrease)
        int64_t r = r0, n = r1 - r0;
        while (n > 0) {
            const int64_t half = n >> 1;
            if (col_b[r + half] <= lo) {
                r += half + 1;
                n -= half + 1;
            } else {
                n = half;
            }
        }
        int32_t cov[MAX_L], first_a[MAX_L], last_b[MAX_L];
#pragma unroll
        for (int l = 0; l < MAX_L; ++l) cov[l] = first_a[l] = last_b[l] = 0;
        for (; r < r1; ++r) {
            const int32_t a = col_a[r];
            if (a >= hi) break;
            const int32_t b = col_b[r];
            const int32_t ov = (b < hi ? b : hi) - (a > lo ? a : lo);
            if (ov < 1) continue;                                          // a == b: a run that overlaps nothing
            const unsigned keep = (unsigned)col_keep[r];
#pragma unroll
            for (int l = 0; l < MAX_L; ++l) {
                if (l < L && ((keep >> l) & 1u)) {
                    if (s.frag[l] == 0) first_a[l] = a;
                    last_b[l] = b;
                    cov[l] += ov;
                    s.frag[l] += 1;
                }
            }
        }
#pragma unroll
        for (int l = 0; l < MAX_L; ++l) {
            if (l < L && cov[l] >= (min_ms > 1 ? min_ms : 1) && 100ll * cov[l] >= (long long)min_pct * (hi - lo)) s.hit |= 1u << l;
            s.onset[l] = first_a[l] > lo ? first_a[l] - lo : lo - first_a[l];
            s.offset[l] = last_b[l] > hi ? last_b[l] - hi : hi - last_b[l];
        }
    }
    // sums over the lanes that share k (events are fastest: mostly one k per wave)
    unsigned long long todo = __ballot(valid);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const long long gl = __shfl(g, leader, WAVE);
        const bool in = valid && g == gl;
        add_group<FIELDS>(in, gl, CK, L, lane, s, events);
        todo &= ~__ballot(in);
    }
}

using lad::up256;
}  // namespace

extern "C" int64_t lad_score_events_workspace_bytes(int64_t channels, int64_t n_intervals, int32_t n_thresholds, int32_t n_min_lengths,
                                                    int64_t total_runs) {
    if (!score_sizes_ok(channels, n_intervals, n_thresholds, n_min_lengths) || total_runs < 0 || total_runs > MAX_ROWS) {
        lad::fail(LAD_ERR_INVALID,
                  "lad_score_events_workspace_bytes: channels 1..%d, intervals 0..2^30, thresholds 1..%d, min_lengths 1..%d, runs 0..2^38 "
                  "(got %lld, %lld, %d, %d, %lld)",
                  MAX_C, MAX_K, MAX_L, (long long)channels, (long long)n_intervals, n_thresholds, n_min_lengths, (long long)total_runs);
        return -1;
    }
    return up256(channels * n_thresholds * 8) + up256(n_intervals * 4) + 3 * up256(total_runs * 4) + 256;
}

extern "C" int lad_score_events(const void *runs_workspace, const int32_t *table, const int32_t *counts_host, int64_t channels,
                                int64_t frames, int32_t n_thresholds, const int32_t *bounds, const int32_t *offsets,
                                const int32_t *bounds_host, const int32_t *offsets_host, int64_t n_intervals, const double *fps,
                                const double *fps_host, const double *min_lengths, int32_t n_min_lengths, int32_t min_overlap_ms,
                                int32_t min_overlap_pct, void *workspace, int64_t *events, void *stream) {
    using namespace lad;
    const int K = n_thresholds, L = n_min_lengths;
    const int64_t CK = channels * K;
    const int32_t criteria[2] = {min_overlap_ms, min_overlap_pct};
    MinLengths ml;
    int64_t rows;
    if (int rc = check_scorer("lad_score_events", criteria, runs_workspace, table, counts_host, channels, frames, K, bounds, offsets,
                              bounds_host, offsets_host, n_intervals, fps, fps_host, min_lengths, L, workspace, events, ml, rows))
        return rc;
    const int64_t most_events = most_events_of(offsets_host, channels);      // grid.x of the match kernel

    int64_t *first_row = (int64_t *)workspace;
    int32_t *cum = (int32_t *)((char *)workspace + up256(CK * 8));
    int32_t *col_a = (int32_t *)((char *)cum + up256(n_intervals * 4));
    int32_t *col_b = (int32_t *)((char *)col_a + up256(rows * 4));
    int32_t *col_keep = (int32_t *)((char *)col_b + up256(rows * 4));
    const hipStream_t st = (hipStream_t)stream;
    LAD_HIP_CHECK(hipMemsetAsync(events, 0, (size_t)(CK * L * FIELDS) * sizeof(int64_t), st));
    if (most_events == 0) return LAD_OK;      // no event, so no link, and no prediction overlaps LAUGH: seven zeros
    const int64_t segments = channels * CLASSES;
    hipLaunchKernelGGL(events_scan_kernel, dim3((unsigned)(segments + 1)), dim3(THREADS), 0, st, bounds, offsets, n_intervals, cum, segments,
                       (const int32_t *)runs_workspace, CK, first_row);
    if (int rc = check_launch("events_scan_kernel")) return rc;
    if (rows > 0) {
        hipLaunchKernelGGL(events_prepare_kernel, dim3((unsigned)ceil_div(rows, THREADS)), dim3(THREADS), 0, st, table, rows, first_row, CK,
                           K, fps, ml, L, bounds, cum, offsets, n_intervals, min_overlap_ms, min_overlap_pct, col_a, col_b, col_keep,
                           (unsigned long long *)events);
        if (int rc = check_launch("events_prepare_kernel")) return rc;
    }
    hipLaunchKernelGGL(events_match_kernel, dim3((unsigned)ceil_div(most_events * K, THREADS), (unsigned)channels), dim3(THREADS), 0, st,
                       col_a, col_b, col_keep, rows, first_row, CK, K, L, bounds, offsets, n_intervals, min_overlap_ms, min_overlap_pct,
                       (unsigned long long *)events);
    return check_launch("events_match_kernel");
}
