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
#include "lad_common.h"

namespace {
constexpr int WAVE = 64;
constexpr int WORDS = 8;                    // 64-frame words per tile
constexpr int TILE = WAVE * WORDS;          // frames per wave
constexpr int WAVES = 4;                    // tiles per workgroup
constexpr int THREADS = WAVE * WAVES;
constexpr int MAX_K = 64;                   // thresholds per call: lane k of a wave carries threshold k's count / first row
constexpr int64_t MAX_T = (int64_t)1 << 30; // frame indices and per-threshold run counts are int32
constexpr int MAX_C = 65535;                // grid.y

struct Thresholds {
    double t[MAX_K];
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

template <typename T>
struct TileRegs {
    double v[WORDS];
    double edge;   // lane 0: the frame before the tile; lane 1: the frame after it
    __device__ inline void load(const T *__restrict__ chan, int64_t tile0, int64_t n, int lane) {
#pragma unroll
        for (int j = 0; j < WORDS; ++j) v[j] = load_fixed(chan, tile0 + j * WAVE + lane, n);
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

__device__ inline unsigned long long starts_of(const unsigned long long (&m)[WORDS], int j, unsigned long long eb) {
    const unsigned long long prev = j == 0 ? (eb & 1ull) : (m[j - 1] >> 63);
    return m[j] & ~((m[j] << 1) | prev);
}
__device__ inline unsigned long long ends_of(const unsigned long long (&m)[WORDS], int j, unsigned long long eb) {
    const unsigned long long next = j == WORDS - 1 ? ((eb >> 1) & 1ull) : (m[j + 1] & 1ull);
    return m[j] & ~((m[j] >> 1) | (next << 63));
}

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
    __shared__ Out wave_sum[WAVES];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    const In *src = in + (int64_t)blockIdx.x * len;
    Out *dst = out + (int64_t)blockIdx.x * len;
    Out carry = 0;
    for (int64_t base = 0; base < len; base += THREADS) {
        const int64_t i = base + threadIdx.x;
        const Out x = i < len ? (Out)src[i] : (Out)0;
        Out incl = x;
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) {
            const Out y = __shfl_up(incl, d, WAVE);
            if (lane >= d) incl += y;
        }
        if (lane == WAVE - 1) wave_sum[wave] = incl;
        __syncthreads();
        Out before = carry, all = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            if (w < wave) before += wave_sum[w];
            all += wave_sum[w];
        }
        if (i < len) dst[i] = before + incl - x;
        carry += all;
        __syncthreads();
    }
    if (total != nullptr && threadIdx.x == 0) total[blockIdx.x] = (int32_t)carry;
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
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int k = 0; k < K; ++k) {
        unsigned long long m[WORDS];
        const unsigned long long eb = r.masks(thr.t[k], m);
        long long row = __shfl(my_row, k, WAVE);
#pragma unroll
        for (int j = 0; j < WORDS; ++j) {
            const unsigned long long s = starts_of(m, j, eb), e = ends_of(m, j, eb);
            const int32_t frame = (int32_t)(tile0 + j * WAVE + lane);
            const int before = __popcll(s & below);                 // starts in this word below this lane
            const int is_start = (int)((s >> lane) & 1ull);
            if (is_start) {
                const long long at = row + before;
                if (at >= 0 && at < capacity) table[2 * at] = frame;
            }
            if ((e >> lane) & 1ull) {
                const long long at = row + before + is_start - 1;    // (starts at frames <= this one) - 1
                if (at >= 0 && at < capacity) table[2 * at + 1] = frame;
            }
            row += __popcll(s);
        }
    }
}

struct Workspace {
    int64_t counts, first_row, tile_first, bytes, n_tiles;
};
inline bool layout(int64_t C, int64_t T, int64_t K, Workspace &w) {
    if (C < 1 || C > MAX_C || T < 1 || T > MAX_T || K < 1 || K > MAX_K) return false;
    const int64_t ck = C * K;
    auto up = [](int64_t b) { return (b + 255) / 256 * 256; };
    w.n_tiles = lad::ceil_div(T, TILE);
    w.counts = 0;
    w.first_row = up(ck * 4);
    w.tile_first = w.first_row + up(ck * 8);
    w.bytes = w.tile_first + up(ck * w.n_tiles * 4);
    return true;
}
inline void thresholds_from(const double *host, int K, Thresholds &t) {
    for (int k = 0; k < MAX_K; ++k) t.t[k] = k < K ? host[k] : 0.0;
}
}  // namespace

extern "C" int32_t lad_runs_tile_frames(void) { return TILE; }
extern "C" int32_t lad_runs_max_thresholds(void) { return MAX_K; }

extern "C" int64_t lad_runs_workspace_bytes(int64_t channels, int64_t frames, int32_t n_thresholds) {
    Workspace w;
    if (!layout(channels, frames, n_thresholds, w)) {
        lad::fail(LAD_ERR_INVALID, "lad_runs_workspace_bytes: channels 1..%d, frames 1..2^30, thresholds 1..%d (got %lld, %lld, %d)",
                  MAX_C, MAX_K, (long long)channels, (long long)frames, n_thresholds);
        return -1;
    }
    return w.bytes;
}

extern "C" int lad_runs_count(const void *probs, int32_t dtype, int64_t channels, int64_t frames, const double *thresholds,
                              int32_t n_thresholds, void *workspace, void *stream) {
    using namespace lad;
    Workspace w;
    LAD_REQUIRE(probs && thresholds && workspace, "lad_runs_count: null buffer");
    LAD_REQUIRE(dtype == LAD_RUNS_F32 || dtype == LAD_RUNS_F64, "lad_runs_count: dtype %d (LAD_RUNS_F32 or LAD_RUNS_F64)", dtype);
    LAD_REQUIRE(layout(channels, frames, n_thresholds, w),
                "lad_runs_count: channels 1..%d, frames 1..2^30, thresholds 1..%d (got %lld, %lld, %d)", MAX_C, MAX_K,
                (long long)channels, (long long)frames, n_thresholds);
    Thresholds thr;
    thresholds_from(thresholds, n_thresholds, thr);
    char *ws = (char *)workspace;
    int32_t *counts = (int32_t *)(ws + w.counts), *tile_first = (int32_t *)(ws + w.tile_first);
    int64_t *first_row = (int64_t *)(ws + w.first_row);
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)ceil_div(w.n_tiles, WAVES), (unsigned)channels);
    const int K = n_thresholds;
    if (dtype == LAD_RUNS_F32)
        hipLaunchKernelGGL(runs_count_kernel<float>, grid, dim3(THREADS), 0, st, (const float *)probs, frames, K, thr, w.n_tiles,
                           tile_first);
    else
        hipLaunchKernelGGL(runs_count_kernel<double>, grid, dim3(THREADS), 0, st, (const double *)probs, frames, K, thr, w.n_tiles,
                           tile_first);
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
    Workspace w;
    LAD_REQUIRE(probs && thresholds && workspace && counts_host, "lad_runs_fill: null buffer");
    LAD_REQUIRE(dtype == LAD_RUNS_F32 || dtype == LAD_RUNS_F64, "lad_runs_fill: dtype %d (LAD_RUNS_F32 or LAD_RUNS_F64)", dtype);
    LAD_REQUIRE(layout(channels, frames, n_thresholds, w),
                "lad_runs_fill: channels 1..%d, frames 1..2^30, thresholds 1..%d (got %lld, %lld, %d)", MAX_C, MAX_K,
                (long long)channels, (long long)frames, n_thresholds);
    LAD_REQUIRE(capacity_runs >= 0, "lad_runs_fill: negative capacity");
    int64_t total = 0;
    for (int64_t i = 0; i < channels * n_thresholds; ++i) {
        LAD_REQUIRE(counts_host[i] >= 0 && counts_host[i] <= (frames + 1) / 2,
                    "lad_runs_fill: counts_host[%lld] = %d is not a run count of a %lld-frame track", (long long)i, counts_host[i],
                    (long long)frames);
        total += counts_host[i];
    }
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
    if (dtype == LAD_RUNS_F32)
        hipLaunchKernelGGL(runs_fill_kernel<float>, grid, dim3(THREADS), 0, st, (const float *)probs, frames, K, thr, w.n_tiles,
                           (const int32_t *)(ws + w.tile_first), (const int64_t *)(ws + w.first_row), capacity_runs, table);
    else
        hipLaunchKernelGGL(runs_fill_kernel<double>, grid, dim3(THREADS), 0, st, (const double *)probs, frames, K, thr, w.n_tiles,
                           (const int32_t *)(ws + w.tile_first), (const int64_t *)(ws + w.first_row), capacity_runs, table);
    return check_launch("runs_fill_kernel");
}
