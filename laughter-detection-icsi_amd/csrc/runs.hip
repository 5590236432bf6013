// Threshold sweep of a probability track: for K thresholds at once, the table of maximal runs (first_frame, last_frame) of
// frames whose probability exceeds the threshold.
//
// Replaces the per-frame loop of get_laughter_instances (laugh_segmenter.py:74-111, with fix_over_underflow :57-71) -- 87 passes
// over a 360,000-frame track in the evaluation sweep (cluster_scripts/gen_eval_exp.py:30-36) -- up to the integer run table;
// first / fps, last / fps and the min_length filter stay with the caller (float64 on the compact table).
//
// Semantics: p > 1 -> 1, p <= 0 -> 1e-7, anything else (NaN included) unchanged; frame i is on for threshold t iff
// (double)p[i] > t with t a double, whatever the track's type (float32(t) > t for 16 of the 29 evaluation thresholds, so a
// float32 comparison accepts a probability equal to float32(t) that the reference rejects).
//
// Shape: one wave owns a TILE of 512 consecutive frames as 8 words of 64 frames (lane l of word j = frame tile0 + 64 j + l),
// read once, plus the two frames across the tile's edges.  For a threshold the 8 ballots of `p > t` ARE the on/off mask of the
// tile, held in scalar registers; starts = M & ~(M << 1 | carry-in), ends = M & ~(M >> 1 | carry-in from above), counted with
// popcounts -- all wave-uniform bit arithmetic, K times over the same registers.  A run's slot in the table is its rank:
//   lad_runs_count   (1) starts per (channel, threshold, tile)   (2) exclusive scan over tiles per (channel, threshold), whose
//                    total is the run count   (3) exclusive scan of the C * K run counts: each table's first row
//   lad_runs_fill    a start at frame i goes to row base + (starts before i); the end at frame i closes the run of rank
//                    (starts at frames <= i) - 1, so the same count places both columns.
// Four launches whatever K and C are.  No atomic anywhere: rows ascend with the frame index by construction and two calls write
// the same bytes.  Every store is guarded by the caller's capacity.  No LDS in the tile kernels, no scratch.
// The tile geometry, the limits, the fixed load, starts / ends and their placement by rank, and the scan are lad_sweep_tile.h's.
#include "lad_sweep_tile.h"

namespace {
using namespace lad::sweep;

struct Thresholds {
    double t[MAX_K];
};

template <typename T>
struct TileRegs {
    double v[WORDS];
    double edge;   // lane 0: the frame before the tile; lane 1: the frame after it
    __device__ inline void load(const T *__restrict__ chan, int64_t tile0, int64_t n, int lane) {
        load_tile(chan, tile0, n, lane, v);
        edge = __builtin_nan("");
        if (lane == 0) edge = load_fixed(chan, tile0 - 1, n);
        if (lane == 1) edge = load_fixed(chan, tile0 + TILE, n);
    }
    // on/off masks of the tile for threshold t; returns the two edge bits (bit 0: frame before, bit 1: frame after)
    __device__ inline unsigned long long masks(double t, unsigned long long (&m)[WORDS]) const {
#pragma unroll
        for (int j = 0; j < WORDS; ++j) m[j] = __ballot(v[j] > t);
        return __ballot(edge > t);
    }
};

// (1) tile_count[(c * K + k) * n_tiles + tile] = runs that start inside the tile
template <typename T>
__global__ __launch_bounds__(THREADS) void runs_count_kernel(const T *__restrict__ probs, int64_t n, int K, Thresholds thr,
                                                             int64_t n_tiles, int32_t *__restrict__ tile_count) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t tile = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (tile >= n_tiles) return;                      // (whole waves leave: the ballots below see full waves)
    const int c = blockIdx.y;
    TileRegs<T> r;
    r.load(probs + (int64_t)c * n, tile * TILE, n, lane);
    int mine = 0;
    for (int k = 0; k < K; ++k) {
        unsigned long long m[WORDS];
        const unsigned long long eb = r.masks(thr.t[k], m);
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < WORDS; ++j) cnt += __popcll(starts_of(m, j, eb));
        if (lane == k) mine = cnt;
    }
    if (lane < K) tile_count[((int64_t)c * K + lane) * n_tiles + tile] = mine;
}

// (2), (3) exclusive scan of each row of `in` (rows of `len` values, one workgroup per row) into `out` (in place allowed);
// the row's total goes to total[row] when total is given.
template <typename In, typename Out>
__global__ __launch_bounds__(THREADS) void runs_scan_kernel(const In *in, Out *out, int32_t *__restrict__ total, int64_t len) {
    const In *src = in + (int64_t)blockIdx.x * len;
    Out *dst = out + (int64_t)blockIdx.x * len;
    const Out all = block_scan<Out>(0, len, [&](int64_t i) { return src[i]; }, [&](int64_t i, Out v) { dst[i] = v; });
    if (total != nullptr && threadIdx.x == 0) total[blockIdx.x] = (int32_t)all;
}

// fill: row (first_row[c * K + k] + rank) of the table = (first_frame, last_frame) of the run of that rank
template <typename T>
__global__ __launch_bounds__(THREADS) void runs_fill_kernel(const T *__restrict__ probs, int64_t n, int K, Thresholds thr,
                                                            int64_t n_tiles, const int32_t *__restrict__ tile_first,
                                                            const int64_t *__restrict__ first_row, int64_t capacity,
                                                            int32_t *__restrict__ table) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t tile = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (tile >= n_tiles) return;
    const int c = blockIdx.y;
    const int64_t tile0 = tile * TILE;
    TileRegs<T> r;
    r.load(probs + (int64_t)c * n, tile0, n, lane);
    long long my_row = 0;                            // lane k: the row of the first run that starts in this tile, threshold k
    if (lane < K) my_row = first_row[(int64_t)c * K + lane] + tile_first[((int64_t)c * K + lane) * n_tiles + tile];
    for (int k = 0; k < K; ++k) {
        unsigned long long m[WORDS];
        const unsigned long long eb = r.masks(thr.t[k], m);
        place_runs(m, eb, eb >> 1, tile0, lane, __shfl(my_row, k, WAVE), capacity, table);
    }
}

struct Workspace {
    int64_t counts, first_row, tile_first, bytes, n_tiles;
};
inline Workspace layout(int64_t C, int64_t T, int64_t K) {   // of sizes that check_sizes has passed
    using lad::up256;
    const int64_t ck = C * K;
    Workspace w;
    w.n_tiles = lad::ceil_div(T, TILE);
    w.counts = 0;
    w.first_row = up256(ck * 4);
    w.tile_first = w.first_row + up256(ck * 8);
    w.bytes = w.tile_first + up256(ck * w.n_tiles * 4);
    return w;
}
inline void thresholds_from(const double *host, int K, Thresholds &t) {
    for (int k = 0; k < MAX_K; ++k) t.t[k] = k < K ? host[k] : 0.0;
}
}  // namespace

extern "C" int32_t lad_runs_tile_frames(void) { return TILE; }
extern "C" int32_t lad_runs_max_thresholds(void) { return MAX_K; }

extern "C" int64_t lad_runs_workspace_bytes(int64_t channels, int64_t frames, int32_t n_thresholds) {
    if (check_sizes("lad_runs_workspace_bytes", "thresholds", channels, frames, n_thresholds)) return -1;
    return layout(channels, frames, n_thresholds).bytes;
}

extern "C" int lad_runs_count(const void *probs, int32_t dtype, int64_t channels, int64_t frames, const double *thresholds,
                              int32_t n_thresholds, void *workspace, void *stream) {
    using namespace lad;
    LAD_REQUIRE(probs && thresholds && workspace, "lad_runs_count: null buffer");
    if (int rc = check_dtype("lad_runs_count", dtype)) return rc;
    if (int rc = check_sizes("lad_runs_count", "thresholds", channels, frames, n_thresholds)) return rc;
    const Workspace w = layout(channels, frames, n_thresholds);
    Thresholds thr;
    thresholds_from(thresholds, n_thresholds, thr);
    char *ws = (char *)workspace;
    int32_t *counts = (int32_t *)(ws + w.counts), *tile_first = (int32_t *)(ws + w.tile_first);
    int64_t *first_row = (int64_t *)(ws + w.first_row);
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)ceil_div(w.n_tiles, WAVES), (unsigned)channels);
    const int K = n_thresholds;
    with_track_type(dtype, [&](auto z) {
        using T = decltype(z);
        hipLaunchKernelGGL(runs_count_kernel<T>, grid, dim3(THREADS), 0, st, (const T *)probs, frames, K, thr, w.n_tiles, tile_first);
    });
    if (int rc = check_launch("runs_count_kernel")) return rc;
    hipLaunchKernelGGL((runs_scan_kernel<int32_t, int32_t>), dim3((unsigned)(channels * K)), dim3(THREADS), 0, st,
                       (const int32_t *)tile_first, tile_first, counts, w.n_tiles);
    if (int rc = check_launch("runs_scan_kernel (tiles)")) return rc;
    hipLaunchKernelGGL((runs_scan_kernel<int32_t, int64_t>), dim3(1), dim3(THREADS), 0, st, (const int32_t *)counts, first_row,
                       (int32_t *)nullptr, channels * K);
    return check_launch("runs_scan_kernel (tables)");
}

extern "C" int lad_runs_fill(const void *probs, int32_t dtype, int64_t channels, int64_t frames, const double *thresholds,
                             int32_t n_thresholds, const void *workspace, const int32_t *counts_host, int32_t *table,
                             int64_t capacity_runs, void *stream) {
    using namespace lad;
    LAD_REQUIRE(probs && thresholds && workspace && counts_host, "lad_runs_fill: null buffer");
    if (int rc = check_dtype("lad_runs_fill", dtype)) return rc;
    if (int rc = check_sizes("lad_runs_fill", "thresholds", channels, frames, n_thresholds)) return rc;
    const Workspace w = layout(channels, frames, n_thresholds);
    LAD_REQUIRE(capacity_runs >= 0, "lad_runs_fill: negative capacity");
    const int64_t total = total_runs("lad_runs_fill", counts_host, channels * n_thresholds, frames);
    if (total < 0) return LAD_ERR_INVALID;
    LAD_REQUIRE(total <= capacity_runs, "lad_runs_fill: the tables hold %lld runs, the buffer %lld (nothing was written)",
                (long long)total, (long long)capacity_runs);
    if (total == 0) return LAD_OK;
    LAD_REQUIRE(table, "lad_runs_fill: null table");
    Thresholds thr;
    thresholds_from(thresholds, n_thresholds, thr);
    const char *ws = (const char *)workspace;
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)ceil_div(w.n_tiles, WAVES), (unsigned)channels);
    const int K = n_thresholds;
    with_track_type(dtype, [&](auto z) {
        using T = decltype(z);
        hipLaunchKernelGGL(runs_fill_kernel<T>, grid, dim3(THREADS), 0, st, (const T *)probs, frames, K, thr, w.n_tiles,
                           (const int32_t *)(ws + w.tile_first), (const int64_t *)(ws + w.first_row), capacity_runs, table);
    });
    return check_launch("runs_fill_kernel");
}
