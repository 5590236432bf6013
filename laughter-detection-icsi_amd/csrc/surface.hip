// Dense threshold sweep: the scores of lad_score_runs for up to 4096 ascending levels from ONE pass over the track, through the
// component tree (max-tree) of the 1-D signal.
//
// The runs of {q > level j} over all j are nested: a maximal frame interval [first, last] whose frames all have at least `top`
// levels below them, and whose two outside neighbours have fewer (`base` = the larger of the two counts), is a row of the run table
// of exactly the levels base <= j < top.  A track of T frames has at most T such nodes whatever the number of levels, so each node
// is scored once (lad_sweep_tile.h: run_fields, the arithmetic of score.hip) and its seven integers go to a difference array over
// the levels: +w at row base, -w at row top; one prefix sum over the levels gives the array lad_score_runs returns level by level.
//
// Frame value and comparison, the bins, the tree of minima over them and the two nearest-smaller searches (at most
// 2 ceil(log2 T) reads each, whatever the track looks like) are lad_surface_tree.h's, shared with surface_events.hip.
// The node of an interval is found at its leftmost minimum r: the nearest frame left of r with bin <= bin[r] has bin < bin[r] (or
// there is none); that frame is first - 1, and the nearest frame right of r with bin < bin[r] is last + 1.  A frame whose left
// search ends at an equal bin is no representative and makes no second search.
//
// Shape: one copy (the levels), one memset (the difference array) and six launches whatever C, K and L are:
//   surface_bins_kernel    one workgroup per 2048 frames: bins by binary search in the levels held in LDS (level 0 of the tree) and
//                          the 11 levels of minima above them
//   surface_tree_kernel    twice: levels 12..22 from level 11, levels 23..33 from level 22 (a track of 2^30 frames ends at level 30)
//   surface_cum_kernel     the interval index's running lengths per (channel, class): scan_index_and_counts
//   surface_nodes_kernel   one lane per frame: the two searches, run_fields for a representative, then +w / -w per kept min_length:
//                          into a copy of the difference array in LDS when it fits (few levels: every node of the workgroup lands on
//                          the same few rows), flushed with one vector global atomic per non-zero cell; straight to global memory
//                          otherwise (many levels: the adds spread over many rows)
//   surface_prefix_kernel  one workgroup per (channel, min_length, field): block_scan over the levels
// Integer sums on int64 only: whatever order the waves arrive in, the bytes are the same.  Every read of the tree is below its
// level's node count, every index read is clamped to the index (coverage_pairs).  No scratch.
#pragma clang fp contract(off)
#include "lad_surface_tree.h"

namespace {
using namespace lad::sweep;
using namespace lad::surface;
using lad::ceil_div;
using lad::up256;

constexpr int MAX_PRIVATE_BYTES = 48 * 1024;     // the difference array of one channel in LDS, if it fits

__global__ __launch_bounds__(THREADS) void surface_nodes_kernel(const bin_t *__restrict__ trees, int64_t tree_pitch, int64_t T, int K,
                                                                const double *__restrict__ fps, MinLengths ml, int L,
                                                                const int32_t *__restrict__ bounds, const int32_t *__restrict__ cum,
                                                                const int32_t *__restrict__ offsets, int64_t n_intervals, int use_lds,
                                                                unsigned long long *__restrict__ diff) {
    extern __shared__ unsigned long long priv[];
    const int64_t c = blockIdx.y;
    const bin_t *tree = trees + c * tree_pitch;
    const int cells = (K + 1) * L * SCORE_FIELDS;
    unsigned long long *mine = diff + c * cells;
    if (use_lds) {
        for (int i = threadIdx.x; i < cells; i += THREADS) priv[i] = 0;
        __syncthreads();
    }
    const double f = fps[c];
    const int64_t chunk0 = (int64_t)blockIdx.x * CHUNK;
    for (int j = threadIdx.x; j < CHUNK; j += THREADS) {
        const int64_t i = chunk0 + j;
        if (i >= T) break;
        const int top = tree[i];
        if (top == 0 || top > K) continue;
        int lb, rb;
        const int64_t left = nearest_left_le(tree, T, i, top, lb);
        if (left >= 0 && lb == top) continue;        // an equal bin further left in the same interval: that frame speaks for it
        const int64_t right = nearest_right_lt(tree, T, i, top, rb);
        const int base = lb > rb ? lb : rb;
        if (base >= top) continue;                   // (cannot happen: both neighbours are smaller)
        int32_t v[SCORE_FIELDS];
        const unsigned keep = run_fields(c, (int32_t)(left + 1), (int32_t)(right - 1), f, ml, L, bounds, cum, offsets, n_intervals, v);
#pragma unroll
        for (int l = 0; l < MAX_L; ++l) {
            if (l < L && ((keep >> l) & 1u)) {
#pragma unroll
                for (int fd = 0; fd < SCORE_FIELDS; ++fd) {
                    if (v[fd] != 0) {
                        const unsigned long long w = (unsigned long long)(long long)v[fd];
                        const int up = (base * L + l) * SCORE_FIELDS + fd, down = (top * L + l) * SCORE_FIELDS + fd;
                        if (use_lds) {
                            atomicAdd(priv + up, w);
                            atomicAdd(priv + down, 0ull - w);
                        } else {
                            atomicAdd(mine + up, w);
                            atomicAdd(mine + down, 0ull - w);
                        }
                    }
                }
            }
        }
    }
    if (use_lds) {
        __syncthreads();
        for (int i = threadIdx.x; i < cells; i += THREADS) {
            const unsigned long long w = priv[i];
            if (w != 0) atomicAdd(mine + i, w);
        }
    }
}

// scores[c][j][l][f] = the sum of diff[c][0..j][l][f]; row K of diff is never read
__global__ __launch_bounds__(THREADS) void surface_prefix_kernel(const long long *__restrict__ diff, int K, int LF,
                                                                 long long *__restrict__ scores) {
    const int64_t c = blockIdx.x / LF, lf = blockIdx.x % LF;
    const long long *in = diff + c * (K + 1) * LF + lf;
    long long *out = scores + c * K * LF + lf;
    block_scan<long long>(0, K, [&](int64_t j) { return in[j * LF]; }, [&](int64_t j, long long v) { out[j * LF] = v + in[j * LF]; });
}

struct Workspace {
    int64_t levels, cum, diff, trees, tree_pitch, bytes;
};
Workspace layout(int64_t C, int64_t T, int64_t n_intervals, int64_t K, int64_t L) {   // of sizes that surface_sizes_ok has passed
    Workspace w;
    w.levels = 0;
    w.cum = up256(K * 8);
    w.diff = w.cum + up256(n_intervals * 4);
    w.trees = w.diff + up256(C * (K + 1) * L * SCORE_FIELDS * 8);
    w.tree_pitch = tree_pitch_of(T);
    w.bytes = w.trees + C * w.tree_pitch * (int64_t)sizeof(bin_t) + 256;
    return w;
}
}  // namespace

extern "C" int32_t lad_surface_max_levels(void) { return MAX_LEVELS; }
extern "C" int32_t lad_surface_tile_frames(void) { return CHUNK; }

extern "C" int64_t lad_surface_workspace_bytes(int64_t channels, int64_t frames, int64_t n_intervals, int32_t n_levels,
                                               int32_t n_min_lengths) {
    if (!surface_sizes_ok(channels, frames, n_intervals, n_levels, n_min_lengths)) {
        lad::fail(LAD_ERR_INVALID, SURFACE_SIZES_MESSAGE("lad_surface_workspace_bytes"));
        return -1;
    }
    return layout(channels, frames, n_intervals, n_levels, n_min_lengths).bytes;
}

extern "C" int lad_score_surface(const void *probs, int32_t dtype, int64_t channels, int64_t frames, const double *levels,
                                 int32_t n_levels, const int32_t *bounds, const int32_t *offsets, const int32_t *bounds_host,
                                 const int32_t *offsets_host, int64_t n_intervals, const double *fps, const double *fps_host,
                                 const double *min_lengths, int32_t n_min_lengths, void *workspace, int64_t *scores, void *stream) {
    using namespace lad;
    LAD_REQUIRE(surface_sizes_ok(channels, frames, n_intervals, n_levels, n_min_lengths), SURFACE_SIZES_MESSAGE("lad_score_surface"));
    LAD_REQUIRE(probs && levels && offsets && offsets_host && fps && fps_host && min_lengths && workspace && scores,
                "lad_score_surface: null buffer");
    LAD_REQUIRE(n_intervals == 0 || (bounds && bounds_host), "lad_score_surface: null interval bounds");
    if (int rc = check_dtype("lad_score_surface", dtype)) return rc;
    const int K = n_levels, L = n_min_lengths;
    if (int rc = check_levels("lad_score_surface", levels, K)) return rc;
    MinLengths ml;
    if (int rc = load_min_lengths("lad_score_surface", min_lengths, L, ml)) return rc;
    if (int rc = check_index("lad_score_surface", channels, frames, fps_host, offsets_host, bounds_host, n_intervals)) return rc;

    const Workspace w = layout(channels, frames, n_intervals, K, L);
    char *ws = (char *)workspace;
    double *levels_dev = (double *)(ws + w.levels);
    int32_t *cum = (int32_t *)(ws + w.cum);
    unsigned long long *diff = (unsigned long long *)(ws + w.diff);
    bin_t *trees = (bin_t *)(ws + w.trees);
    const hipStream_t st = (hipStream_t)stream;
    const int64_t cells = (int64_t)(K + 1) * L * SCORE_FIELDS;
    LAD_HIP_CHECK(hipMemsetAsync(diff, 0, (size_t)(channels * cells) * sizeof(long long), st));
    if (int rc = build_trees(probs, dtype, channels, frames, levels, K, levels_dev, trees, w.tree_pitch, bounds, offsets, n_intervals, cum, st))
        return rc;
    const dim3 grid((unsigned)ceil_div(frames, CHUNK), (unsigned)channels);
    const int64_t private_bytes = cells * (int64_t)sizeof(long long);
    const int use_lds = private_bytes <= MAX_PRIVATE_BYTES;
    hipLaunchKernelGGL(surface_nodes_kernel, grid, dim3(THREADS), use_lds ? (size_t)private_bytes : 0, st, (const bin_t *)trees, w.tree_pitch,
                       frames, K, fps, ml, L, bounds, (const int32_t *)cum, offsets, n_intervals, use_lds, diff);
    if (int rc = check_launch("surface_nodes_kernel")) return rc;
    hipLaunchKernelGGL(surface_prefix_kernel, dim3((unsigned)(channels * L * SCORE_FIELDS)), dim3(THREADS), 0, st, (const long long *)diff, K,
                       L * SCORE_FIELDS, (long long *)scores);
    return check_launch("surface_prefix_kernel");
}
