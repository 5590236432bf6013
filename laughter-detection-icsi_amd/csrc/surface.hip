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
// 2 ceil(log2 T) reads each, whatever the track looks like) are lad_surface_tree.h's, shared with surface_events.hip; so are the
// body of the nodes kernel (score_nodes), the prefix sum (prefix_levels), the workspace and the host half of the entry point up to
// and including the nodes launch (sweep_nodes): what stands here is the two __global__ names, the prefix launch and the C ABI.
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

__global__ __launch_bounds__(THREADS) void surface_nodes_kernel(const bin_t *__restrict__ trees, int64_t tree_pitch, int64_t T, int K,
                                                                const double *__restrict__ fps, MinLengths ml, int L,
                                                                const int32_t *__restrict__ bounds, const int32_t *__restrict__ cum,
                                                                const int32_t *__restrict__ offsets, int64_t n_intervals, int use_lds,
                                                                unsigned long long *__restrict__ diff) {
    score_nodes<SCORE_FIELDS>(trees, tree_pitch, T, K, fps, ml, L, bounds, cum, offsets, n_intervals, use_lds, diff,
                              [](int32_t, int32_t, double, const MinLengths &, int, int32_t (&)[SCORE_FIELDS]) {});      // no field of its own
}

// scores[c][j][l][f] = the sum of diff[c][0..j][l][f]
__global__ __launch_bounds__(THREADS) void surface_prefix_kernel(const long long *__restrict__ diff, int K, int LF,
                                                                 long long *__restrict__ scores) {
    const int64_t c = blockIdx.x / LF, lf = blockIdx.x % LF;
    prefix_levels(diff + c * (K + 1) * LF + lf, LF, scores + c * K * LF + lf, LF, K);
}
}  // namespace

extern "C" int32_t lad_surface_max_levels(void) { return MAX_LEVELS; }
extern "C" int32_t lad_surface_tile_frames(void) { return CHUNK; }

extern "C" int64_t lad_surface_workspace_bytes(int64_t channels, int64_t frames, int64_t n_intervals, int32_t n_levels,
                                               int32_t n_min_lengths) {
    return workspace_bytes("lad_surface_workspace_bytes", channels, frames, n_intervals, n_levels, n_min_lengths, SCORE_FIELDS);
}

extern "C" int lad_score_surface(const void *probs, int32_t dtype, int64_t channels, int64_t frames, const double *levels,
                                 int32_t n_levels, const int32_t *bounds, const int32_t *offsets, const int32_t *bounds_host,
                                 const int32_t *offsets_host, int64_t n_intervals, const double *fps, const double *fps_host,
                                 const double *min_lengths, int32_t n_min_lengths, void *workspace, int64_t *scores, void *stream) {
    using namespace lad;
    const int K = n_levels, L = n_min_lengths;
    Sweep s;
    const auto nodes = [&](dim3 grid, size_t lds_bytes, hipStream_t st, const bin_t *trees, int64_t tree_pitch, const MinLengths &ml,
                           const int32_t *cum, int use_lds, unsigned long long *diff) {
        hipLaunchKernelGGL(surface_nodes_kernel, grid, dim3(THREADS), lds_bytes, st, trees, tree_pitch, frames, K, fps, ml, L, bounds, cum,
                           offsets, n_intervals, use_lds, diff);
    };
    if (int rc = sweep_nodes<SCORE_FIELDS>("lad_score_surface", "surface_nodes_kernel", nullptr, probs, dtype, channels, frames, levels, K,
                                           bounds, offsets, bounds_host, offsets_host, n_intervals, fps, fps_host, min_lengths, L, workspace,
                                           scores != nullptr, stream, s, nodes))
        return rc;
    hipLaunchKernelGGL(surface_prefix_kernel, dim3((unsigned)(channels * L * SCORE_FIELDS)), dim3(THREADS), 0, s.st, s.diff, K,
                       L * SCORE_FIELDS, (long long *)scores);
    return check_launch("surface_prefix_kernel");
}
