// Event-level scores on the dense threshold sweep: for up to 4096 ascending levels of a track, the seven time fields of
// lad_score_surface AND the seven event fields of lad_score_events, from one set of bins and one tree of minima
// (lad_surface_tree.h).  The convention is include/lad_hip.h's (above lad_score_surface_events): the predictions of level j are the
// nodes of the component tree with base <= j < top, i.e. exactly the rows of level j's run table.
//
// Per node (surface_events_nodes_kernel, one lane per frame: lad_surface_tree.h's score_nodes, the body surface.hip runs, with nine
// fields): run_fields gives the seven time integers and with them lov = corr_ms and pred_ms, so the node's own hit bit; its links
// are the LAUGH intervals with lo < b minus those with hi <= a (two binary searches; 0 for a == b): HitAndLinks, which holds the
// criteria and the channel's LAUGH segment, found once per workgroup.  Nine integers go to the difference array over the levels,
// +w at row base and -w at row top.
//
// Per (event, level) (surface_events_match_kernel): ms(f) = rint(f / fps * 1000) does not decrease with f, so with F0 the first
// frame whose ms is > lo and F1 the last whose ms is < hi, the run [s, e] of level j is linked to the event (lo, hi] iff s <= F1,
// e >= F0 and a < b.  F0 <= F1 + 1 always; the frames min(F0, F1) .. max(F0, F1) are walked once, lane = level, so the 64 lanes of
// a workgroup read the same bin and the same frame time from LDS (a broadcast), tile after tile of 1024 frames: a window of any
// length is exact, the state of the walk staying in registers.  The run that is on at the first frame of the walk starts where the
// nearest frame to its left with bin <= j says, the one still on at the last frame ends where the nearest frame to its right with
// bin <= j says: two searches in the tree per (event, level) at most.  A workgroup takes `group` consecutive events of one channel
// and 64 adjacent levels, sums REF_TOUCHED, REF_HIT and the two error sums over its events in registers and issues one vector
// atomic add on int64 per non-zero (level, min_length, field).
//
// Shape: one copy (the levels), two memsets (the difference array, the event array) and SEVEN launches whatever C, K, L and the
// number of events are: bins, tree twice, cum, nodes (lad_surface_tree.h: sweep_nodes, the host half shared with
// lad_score_surface), match, prefix (prefix_levels per field, and N_REF).  No loop over levels or
// events on the host.  Integer sums on int64 only: identical bytes on every call.  Every read of the tree is below its level's node
// count (the two searches; the walk reads frames 0 .. T - 1 only), every index read is clamped to the index.  No scratch.
#pragma clang fp contract(off)
#include "lad_surface_tree.h"

namespace {
using namespace lad::sweep;
using namespace lad::surface;
using lad::ceil_div;

constexpr int EV_FIELDS = LAD_EVENT_FIELDS;
constexpr int DIFF_FIELDS = SCORE_FIELDS + 2;    // the seven time fields, PRED_HIT, LINKS
constexpr int WALK_TILE = 1024;                  // frames of a window in LDS at a time: 2 + 8 bytes each, 10 KB per workgroup of one wave
constexpr int MAX_GROUP = 64;                    // events per workgroup of the match kernel, at most

// the LAUGH segment of channel c, clamped to the index
__device__ inline void laugh_segment(int64_t c, const int32_t *__restrict__ offsets, int64_t n_intervals, int64_t &o0, int64_t &o1) {
    o0 = offsets[c * CLASSES + LAD_SCORE_LAUGH];
    o1 = offsets[c * CLASSES + LAD_SCORE_LAUGH + 1];
    o0 = o0 < 0 ? 0 : (o0 > n_intervals ? n_intervals : o0);
    o1 = o1 < o0 ? o0 : (o1 > n_intervals ? n_intervals : o1);
}

// intervals i of [o0, o1) with bounds[2 i + side] < x (the end points of a segment ascend)
__device__ inline int64_t count_below(const int32_t *__restrict__ bounds, int64_t o0, int64_t o1, int side, int32_t x) {
    int64_t at = o0, n = o1 - o0;
    while (n > 0) {
        const int64_t half = n >> 1;
        if (bounds[2 * (at + half) + side] < x) {
            at += half + 1;
            n -= half + 1;
        } else {
            n = half;
        }
    }
    return at - o0;
}

// the two fields behind run_fields' seven, for the nodes of one channel: PRED_HIT from lov = corr_ms and pred_ms, LINKS from the
// channel's LAUGH segment [o0, o1) of the index
struct HitAndLinks {
    int32_t min_ms, min_pct;
    const int32_t *__restrict__ bounds;
    int64_t o0, o1;
    __device__ void operator()(int32_t first, int32_t last, double f, const MinLengths &ml, int L, int32_t (&v)[DIFF_FIELDS]) const {
        const long long lov = v[3], pred = v[2];                             // |(a, b] n LAUGH|, |(a, b] \ INVALID|
        v[SCORE_FIELDS] = (lov >= (min_ms > 1 ? min_ms : 1) && 100ll * lov >= (long long)min_pct * pred) ? 1 : 0;
        int32_t x[2];
        run_ms(first, last, f, ml, L, x);
        v[SCORE_FIELDS + 1] = 0;
        if (x[1] > x[0])                                                     // events with lo < b, minus those with hi <= a
            v[SCORE_FIELDS + 1] = (int32_t)(count_below(bounds, o0, o1, 0, x[1]) - count_below(bounds, o0, o1, 1, x[0] + 1));
    }
};

__global__ __launch_bounds__(THREADS) void surface_events_nodes_kernel(const bin_t *__restrict__ trees, int64_t tree_pitch, int64_t T, int K,
                                                                       const double *__restrict__ fps, MinLengths ml, int L,
                                                                       const int32_t *__restrict__ bounds,
                                                                       const int32_t *__restrict__ cum,
                                                                       const int32_t *__restrict__ offsets, int64_t n_intervals,
                                                                       int32_t min_ms, int32_t min_pct, int use_lds,
                                                                       unsigned long long *__restrict__ diff) {
    HitAndLinks extra{min_ms, min_pct, bounds, 0, 0};
    laugh_segment(blockIdx.y, offsets, n_intervals, extra.o0, extra.o1);     // once per workgroup
    score_nodes<DIFF_FIELDS>(trees, tree_pitch, T, K, fps, ml, L, bounds, cum, offsets, n_intervals, use_lds, diff, extra);
}

// the first frame f of [0, T) with rint(f / fps * 1000) >= x, or T
__device__ inline int64_t first_frame_at(int64_t T, double fps, int32_t x) {
    int64_t at = 0, n = T;
    while (n > 0) {
        const int64_t half = n >> 1;
        if ((int32_t)rint((double)(at + half) / fps * MS) < x) {
            at += half + 1;
            n -= half + 1;
        } else {
            n = half;
        }
    }
    return at;
}

// what one event has met at one level, per min_length
struct Met {
    int32_t cov[MAX_L], frag[MAX_L], first_a[MAX_L], last_b[MAX_L];
};

// the run [s, e] of this lane's level (seconds start, end) against the event (lo, hi] with the frame window F0, F1
__device__ inline void meet(Met &m, int64_t s, int64_t e, double start, double end, int64_t F0, int64_t F1, int32_t lo, int32_t hi,
                            const MinLengths &ml, int L) {
    if (s > F1 || e < F0) return;
    const double len = end - start;
    const int32_t a = (int32_t)rint(start * MS), b = (int32_t)rint(end * MS);
    const int32_t ov = (b < hi ? b : hi) - (a > lo ? a : lo);
    if (b <= a || ov < 1) return;                    // a == b: a run that overlaps nothing
#pragma unroll
    for (int l = 0; l < MAX_L; ++l) {
        if (l < L && len > ml.v[l]) {
            if (m.frag[l] == 0) m.first_a[l] = a;
            m.last_b[l] = b;
            m.cov[l] += ov;
            m.frag[l] += 1;
        }
    }
}

// grid: x = groups of `group` events, y = 64 levels, z = channel; one wave per workgroup, lane = level
__global__ __launch_bounds__(WAVE) void surface_events_match_kernel(const bin_t *__restrict__ trees, int64_t tree_pitch, int64_t T, int K,
                                                                    const double *__restrict__ fps, MinLengths ml, int L,
                                                                    const int32_t *__restrict__ bounds,
                                                                    const int32_t *__restrict__ offsets, int64_t n_intervals, int group,
                                                                    int32_t min_ms, int32_t min_pct,
                                                                    unsigned long long *__restrict__ events) {
    __shared__ bin_t sbin[WALK_TILE];
    __shared__ double ssec[WALK_TILE];
    const int lane = threadIdx.x;
    const int64_t c = blockIdx.z;
    const int j = (int)blockIdx.y * WAVE + lane;
    const bool live = j < K;
    int64_t o0, o1;
    laugh_segment(c, offsets, n_intervals, o0, o1);
    const int64_t e0 = o0 + (int64_t)blockIdx.x * group;
    const int64_t e1 = e0 + group < o1 ? e0 + group : o1;
    if (e0 >= e1) return;                            // (the whole workgroup)
    const double f = fps[c];
    const bin_t *tree = trees + c * tree_pitch;
    const int32_t need = min_ms > 1 ? min_ms : 1;
    int32_t touched[MAX_L], hits[MAX_L];
    long long onset[MAX_L], offset[MAX_L];
#pragma unroll
    for (int l = 0; l < MAX_L; ++l) {
        touched[l] = hits[l] = 0;
        onset[l] = offset[l] = 0;
    }
    for (int64_t e = e0; e < e1; ++e) {              // every lane of the workgroup takes the same path up to the walk
        const int32_t lo = bounds[2 * e], hi = bounds[2 * e + 1];
        if (hi <= lo || lo > 2147483646) continue;
        const int64_t F0 = first_frame_at(T, f, lo + 1), F1 = first_frame_at(T, f, hi) - 1;
        if (F0 >= T || F1 < 0) continue;             // no frame behind lo, or none in front of hi: no run can be linked
        const int64_t W0 = F0 < F1 ? F0 : F1, W1 = F0 < F1 ? F1 : F0;
        Met m;
#pragma unroll
        for (int l = 0; l < MAX_L; ++l) m.cov[l] = m.frag[l] = m.first_a[l] = m.last_b[l] = 0;
        bool on = false;
        int64_t s = 0;
        double start = 0.0, before = 0.0;            // of the run that is on; the time of the frame before this one
        for (int64_t t0 = W0; t0 <= W1; t0 += WALK_TILE) {
            const int n = (int)(W1 - t0 + 1 < WALK_TILE ? W1 - t0 + 1 : WALK_TILE);
            __syncthreads();
            for (int i = lane; i < n; i += WAVE) {
                sbin[i] = tree[t0 + i];              // level 0 of the tree: t0 + i <= W1 < T
                ssec[i] = (double)(t0 + i) / f;
            }
            __syncthreads();
            for (int i = 0; i < n; ++i) {
                const int b = sbin[i];
                const double sec = ssec[i];
                const bool now = live && b > j;
                if (now && !on) {
                    s = t0 + i;
                    start = sec;
                    if (s == W0) {                   // the run may have begun in front of the window
                        int found;
                        s = nearest_left_le(tree, T, W0, j, found) + 1;
                        start = (double)s / f;
                    }
                } else if (on && !now) {
                    meet(m, s, t0 + i - 1, start, before, F0, F1, lo, hi, ml, L);
                }
                on = now;
                before = sec;
            }
        }
        if (on) {                                    // still on at the last frame of the window: it may go on behind it
            int found;
            const int64_t last = nearest_right_lt(tree, T, W1, j + 1, found) - 1;
            meet(m, s, last, start, (double)last / f, F0, F1, lo, hi, ml, L);
        }
#pragma unroll
        for (int l = 0; l < MAX_L; ++l) {
            if (l < L && m.frag[l] > 0) {
                touched[l] += 1;
                if (m.cov[l] >= need && 100ll * m.cov[l] >= (long long)min_pct * ((long long)hi - lo)) {
                    hits[l] += 1;
                    onset[l] += m.first_a[l] > lo ? m.first_a[l] - lo : lo - m.first_a[l];
                    offset[l] += m.last_b[l] > hi ? m.last_b[l] - hi : hi - m.last_b[l];
                }
            }
        }
    }
    if (!live) return;
    unsigned long long *out = events + ((c * K + j) * L) * EV_FIELDS;
#pragma unroll
    for (int l = 0; l < MAX_L; ++l) {
        if (l < L && touched[l] > 0) {
            atomicAdd(out + l * EV_FIELDS + LAD_EVENT_REF_TOUCHED, (unsigned long long)touched[l]);
            if (hits[l] > 0) atomicAdd(out + l * EV_FIELDS + LAD_EVENT_REF_HIT, (unsigned long long)hits[l]);
            if (onset[l] != 0) atomicAdd(out + l * EV_FIELDS + LAD_EVENT_ONSET_ABS_MS, (unsigned long long)onset[l]);
            if (offset[l] != 0) atomicAdd(out + l * EV_FIELDS + LAD_EVENT_OFFSET_ABS_MS, (unsigned long long)offset[l]);
        }
    }
}

// one workgroup per (channel, min_length, field of the difference array): the sum of diff[c][0..j][l][f] to scores[c][j][l][f] for
// a time field, to events[c][j][l][PRED_HIT / LINKS] for the other two (prefix_levels); the workgroup of PRED_HIT also writes N_REF.
__global__ __launch_bounds__(THREADS) void surface_events_prefix_kernel(const long long *__restrict__ diff, int K, int L,
                                                                        const int32_t *__restrict__ offsets, int64_t n_intervals,
                                                                        long long *__restrict__ scores, long long *__restrict__ events) {
    const int LF = L * DIFF_FIELDS;
    const int64_t c = blockIdx.x / LF;
    const int l = (int)(blockIdx.x % LF) / DIFF_FIELDS, fd = (int)(blockIdx.x % LF) % DIFF_FIELDS;
    const long long *in = diff + c * (K + 1) * LF + l * DIFF_FIELDS + fd;
    if (fd < SCORE_FIELDS) {
        prefix_levels(in, LF, scores + (c * K * L + l) * SCORE_FIELDS + fd, L * SCORE_FIELDS, K);
        return;
    }
    const bool hit = fd == SCORE_FIELDS;
    long long *out = events + (c * K * L + l) * EV_FIELDS;
    const int step = L * EV_FIELDS;
    prefix_levels(in, LF, out + (hit ? LAD_EVENT_PRED_HIT : LAD_EVENT_LINKS), step, K);
    if (hit) {
        int64_t o0, o1;
        laugh_segment(c, offsets, n_intervals, o0, o1);
        for (int j = threadIdx.x; j < K; j += THREADS) out[(int64_t)j * step + LAD_EVENT_N_REF] = o1 - o0;
    }
}
}  // namespace

extern "C" int64_t lad_surface_events_workspace_bytes(int64_t channels, int64_t frames, int64_t n_intervals, int32_t n_levels,
                                                      int32_t n_min_lengths) {
    return workspace_bytes("lad_surface_events_workspace_bytes", channels, frames, n_intervals, n_levels, n_min_lengths, DIFF_FIELDS);
}

extern "C" int lad_score_surface_events(const void *probs, int32_t dtype, int64_t channels, int64_t frames, const double *levels,
                                        int32_t n_levels, const int32_t *bounds, const int32_t *offsets, const int32_t *bounds_host,
                                        const int32_t *offsets_host, int64_t n_intervals, const double *fps, const double *fps_host,
                                        const double *min_lengths, int32_t n_min_lengths, int32_t min_overlap_ms,
                                        int32_t min_overlap_pct, void *workspace, int64_t *scores, int64_t *events, void *stream) {
    using namespace lad;
    const int K = n_levels, L = n_min_lengths;
    const int32_t criteria[2] = {min_overlap_ms, min_overlap_pct};
    Sweep s;
    const auto nodes = [&](dim3 grid, size_t lds_bytes, hipStream_t st, const bin_t *trees, int64_t tree_pitch, const MinLengths &ml,
                           const int32_t *cum, int use_lds, unsigned long long *diff) {
        hipLaunchKernelGGL(surface_events_nodes_kernel, grid, dim3(THREADS), lds_bytes, st, trees, tree_pitch, frames, K, fps, ml, L, bounds,
                           cum, offsets, n_intervals, min_overlap_ms, min_overlap_pct, use_lds, diff);
    };
    if (int rc = sweep_nodes<DIFF_FIELDS>("lad_score_surface_events", "surface_events_nodes_kernel", criteria, probs, dtype, channels, frames,
                                          levels, K, bounds, offsets, bounds_host, offsets_host, n_intervals, fps, fps_host, min_lengths, L,
                                          workspace, scores && events, stream, s, nodes))
        return rc;
    const int64_t most_events = most_events_of(offsets_host, channels);
    LAD_HIP_CHECK(hipMemsetAsync(events, 0, (size_t)(channels * K * L * EV_FIELDS) * sizeof(long long), s.st));
    // events per workgroup: as many as leave some 16384 workgroups to the device (fewer atomics, the same sums)
    const int64_t level_blocks = ceil_div(K, WAVE);
    int64_t group = most_events * level_blocks * channels / 16384;
    group = group < 1 ? 1 : (group > MAX_GROUP ? MAX_GROUP : group);
    const int64_t groups = most_events > 0 ? ceil_div(most_events, group) : 1;      // (no event: every workgroup returns at once)
    hipLaunchKernelGGL(surface_events_match_kernel, dim3((unsigned)groups, (unsigned)level_blocks, (unsigned)channels), dim3(WAVE), 0, s.st,
                       s.trees, s.tree_pitch, frames, K, fps, s.ml, L, bounds, offsets, n_intervals, (int)group, min_overlap_ms,
                       min_overlap_pct, (unsigned long long *)events);
    if (int rc = check_launch("surface_events_match_kernel")) return rc;
    hipLaunchKernelGGL(surface_events_prefix_kernel, dim3((unsigned)(channels * L * DIFF_FIELDS)), dim3(THREADS), 0, s.st, s.diff, K, L,
                       offsets, n_intervals, (long long *)scores, (long long *)events);
    return check_launch("surface_events_prefix_kernel");
}
