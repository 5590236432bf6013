// Event-level scores on the dense threshold sweep: for up to 4096 ascending levels of a track, the seven time fields of
// lad_score_surface AND the seven event fields of lad_score_events, from one set of bins and one tree of minima
// (lad_surface_tree.h).  The convention is include/lad_hip.h's (above lad_score_surface_events): the predictions of level j are the
// nodes of the component tree with base <= j < top, i.e. exactly the rows of level j's run table.
//
// Per node (surface_events_nodes_kernel, one lane per frame as surface.hip's): run_fields gives the seven time integers and with
// them lov = corr_ms and pred_ms, so the node's own hit bit; its links are the LAUGH intervals with lo < b minus those with hi <= a
// (two binary searches; 0 for a == b).  Nine integers go to the difference array over the levels, +w at row base and -w at row top.
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
// number of events are: bins, tree twice, cum (lad_surface_tree.h: build_trees), nodes, match, prefix.  No loop over levels or
// events on the host.  Integer sums on int64 only: identical bytes on every call.  Every read of the tree is below its level's node
// count (the two searches; the walk reads frames 0 .. T - 1 only), every index read is clamped to the index.  No scratch.
#pragma clang fp contract(off)
#include "lad_surface_tree.h"

namespace {
using namespace lad::sweep;
using namespace lad::surface;
using lad::ceil_div;
using lad::up256;

constexpr int EV_FIELDS = LAD_EVENT_FIELDS;
constexpr int DIFF_FIELDS = SCORE_FIELDS + 2;    // the seven time fields, PRED_HIT, LINKS
constexpr int MAX_PRIVATE_BYTES = 48 * 1024;     // the difference array of one channel in LDS, if it fits
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

__global__ __launch_bounds__(THREADS) void surface_events_nodes_kernel(const bin_t *__restrict__ trees, int64_t tree_pitch, int64_t T, int K,
                                                                       const double *__restrict__ fps, MinLengths ml, int L,
                                                                       const int32_t *__restrict__ bounds,
                                                                       const int32_t *__restrict__ cum,
                                                                       const int32_t *__restrict__ offsets, int64_t n_intervals,
                                                                       int32_t min_ms, int32_t min_pct, int use_lds,
                                                                       unsigned long long *__restrict__ diff) {
    extern __shared__ unsigned long long priv[];
    const int64_t c = blockIdx.y;
    const bin_t *tree = trees + c * tree_pitch;
    const int cells = (K + 1) * L * DIFF_FIELDS;
    unsigned long long *mine = diff + c * cells;
    if (use_lds) {
        for (int i = threadIdx.x; i < cells; i += THREADS) priv[i] = 0;
        __syncthreads();
    }
    const double f = fps[c];
    int64_t o0, o1;
    laugh_segment(c, offsets, n_intervals, o0, o1);
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
        int32_t v[DIFF_FIELDS];
        int32_t time[SCORE_FIELDS];
        const int32_t first = (int32_t)(left + 1), last = (int32_t)(right - 1);
        const unsigned keep = run_fields(c, first, last, f, ml, L, bounds, cum, offsets, n_intervals, time);
#pragma unroll
        for (int fd = 0; fd < SCORE_FIELDS; ++fd) v[fd] = time[fd];
        const long long lov = time[3], pred = time[2];                       // |(a, b] n LAUGH|, |(a, b] \ INVALID|
        v[SCORE_FIELDS] = (lov >= (min_ms > 1 ? min_ms : 1) && 100ll * lov >= (long long)min_pct * pred) ? 1 : 0;
        int32_t x[2];
        run_ms(first, last, f, ml, L, x);
        v[SCORE_FIELDS + 1] = 0;
        if (x[1] > x[0])                                                     // events with lo < b, minus those with hi <= a
            v[SCORE_FIELDS + 1] = (int32_t)(count_below(bounds, o0, o1, 0, x[1]) - count_below(bounds, o0, o1, 1, x[0] + 1));
#pragma unroll
        for (int l = 0; l < MAX_L; ++l) {
            if (l < L && ((keep >> l) & 1u)) {
#pragma unroll
                for (int fd = 0; fd < DIFF_FIELDS; ++fd) {
                    if (v[fd] != 0) {
                        const unsigned long long w = (unsigned long long)(long long)v[fd];
                        const int up = (base * L + l) * DIFF_FIELDS + fd, down = (top * L + l) * DIFF_FIELDS + fd;
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
// a time field, to events[c][j][l][PRED_HIT / LINKS] for the other two; the workgroup of PRED_HIT also writes N_REF.  Row K of diff
// is never read.
__global__ __launch_bounds__(THREADS) void surface_events_prefix_kernel(const long long *__restrict__ diff, int K, int L,
                                                                        const int32_t *__restrict__ offsets, int64_t n_intervals,
                                                                        long long *__restrict__ scores, long long *__restrict__ events) {
    const int LF = L * DIFF_FIELDS;
    const int64_t c = blockIdx.x / LF;
    const int l = (int)(blockIdx.x % LF) / DIFF_FIELDS, fd = (int)(blockIdx.x % LF) % DIFF_FIELDS;
    const long long *in = diff + c * (K + 1) * LF + l * DIFF_FIELDS + fd;
    if (fd < SCORE_FIELDS) {
        long long *out = scores + (c * K * L + l) * SCORE_FIELDS + fd;
        const int step = L * SCORE_FIELDS;
        block_scan<long long>(0, K, [&](int64_t j) { return in[j * LF]; }, [&](int64_t j, long long v) { out[j * step] = v + in[j * LF]; });
        return;
    }
    int64_t o0, o1;
    laugh_segment(c, offsets, n_intervals, o0, o1);
    const bool hit = fd == SCORE_FIELDS;
    long long *out = events + (c * K * L + l) * EV_FIELDS;
    const int step = L * EV_FIELDS;
    block_scan<long long>(0, K, [&](int64_t j) { return in[j * LF]; },
                          [&](int64_t j, long long v) {
                              out[j * step + (hit ? LAD_EVENT_PRED_HIT : LAD_EVENT_LINKS)] = v + in[j * LF];
                              if (hit) out[j * step + LAD_EVENT_N_REF] = o1 - o0;
                          });
}

struct Workspace {
    int64_t levels, cum, diff, trees, tree_pitch, bytes;
};
Workspace layout(int64_t C, int64_t T, int64_t n_intervals, int64_t K, int64_t L) {   // of sizes that surface_sizes_ok has passed
    Workspace w;
    w.levels = 0;
    w.cum = up256(K * 8);
    w.diff = w.cum + up256(n_intervals * 4);
    w.trees = w.diff + up256(C * (K + 1) * L * DIFF_FIELDS * 8);
    w.tree_pitch = tree_pitch_of(T);
    w.bytes = w.trees + C * w.tree_pitch * (int64_t)sizeof(bin_t) + 256;
    return w;
}
}  // namespace

extern "C" int64_t lad_surface_events_workspace_bytes(int64_t channels, int64_t frames, int64_t n_intervals, int32_t n_levels,
                                                      int32_t n_min_lengths) {
    if (!surface_sizes_ok(channels, frames, n_intervals, n_levels, n_min_lengths)) {
        lad::fail(LAD_ERR_INVALID, SURFACE_SIZES_MESSAGE("lad_surface_events_workspace_bytes"));
        return -1;
    }
    return layout(channels, frames, n_intervals, n_levels, n_min_lengths).bytes;
}

extern "C" int lad_score_surface_events(const void *probs, int32_t dtype, int64_t channels, int64_t frames, const double *levels,
                                        int32_t n_levels, const int32_t *bounds, const int32_t *offsets, const int32_t *bounds_host,
                                        const int32_t *offsets_host, int64_t n_intervals, const double *fps, const double *fps_host,
                                        const double *min_lengths, int32_t n_min_lengths, int32_t min_overlap_ms,
                                        int32_t min_overlap_pct, void *workspace, int64_t *scores, int64_t *events, void *stream) {
    using namespace lad;
    const char *who = "lad_score_surface_events";
    LAD_REQUIRE(surface_sizes_ok(channels, frames, n_intervals, n_levels, n_min_lengths), SURFACE_SIZES_MESSAGE("lad_score_surface_events"));
    LAD_REQUIRE(min_overlap_ms >= 0 && min_overlap_pct >= 0 && min_overlap_pct <= 100,
                "lad_score_surface_events: min_overlap_ms >= 0, min_overlap_pct 0..100 (got %d, %d)", min_overlap_ms, min_overlap_pct);
    LAD_REQUIRE(probs && levels && offsets && offsets_host && fps && fps_host && min_lengths && workspace && scores && events,
                "lad_score_surface_events: null buffer");
    LAD_REQUIRE(n_intervals == 0 || (bounds && bounds_host), "lad_score_surface_events: null interval bounds");
    if (int rc = check_dtype(who, dtype)) return rc;
    const int K = n_levels, L = n_min_lengths;
    if (int rc = check_levels(who, levels, K)) return rc;
    MinLengths ml;
    if (int rc = load_min_lengths(who, min_lengths, L, ml)) return rc;
    if (int rc = check_index(who, channels, frames, fps_host, offsets_host, bounds_host, n_intervals)) return rc;
    int64_t most_events = 0;      // of one channel
    for (int64_t c = 0; c < channels; ++c) {
        const int64_t n = offsets_host[c * CLASSES + LAD_SCORE_LAUGH + 1] - offsets_host[c * CLASSES + LAD_SCORE_LAUGH];
        most_events = n > most_events ? n : most_events;
    }

    const Workspace w = layout(channels, frames, n_intervals, K, L);
    char *ws = (char *)workspace;
    double *levels_dev = (double *)(ws + w.levels);
    int32_t *cum = (int32_t *)(ws + w.cum);
    unsigned long long *diff = (unsigned long long *)(ws + w.diff);
    bin_t *trees = (bin_t *)(ws + w.trees);
    const hipStream_t st = (hipStream_t)stream;
    const int64_t cells = (int64_t)(K + 1) * L * DIFF_FIELDS;
    LAD_HIP_CHECK(hipMemsetAsync(diff, 0, (size_t)(channels * cells) * sizeof(long long), st));
    LAD_HIP_CHECK(hipMemsetAsync(events, 0, (size_t)(channels * K * L * EV_FIELDS) * sizeof(long long), st));
    if (int rc = build_trees(probs, dtype, channels, frames, levels, K, levels_dev, trees, w.tree_pitch, bounds, offsets, n_intervals, cum, st))
        return rc;
    const int64_t private_bytes = cells * (int64_t)sizeof(long long);
    const int use_lds = private_bytes <= MAX_PRIVATE_BYTES;
    hipLaunchKernelGGL(surface_events_nodes_kernel, dim3((unsigned)ceil_div(frames, CHUNK), (unsigned)channels), dim3(THREADS),
                       use_lds ? (size_t)private_bytes : 0, st, (const bin_t *)trees, w.tree_pitch, frames, K, fps, ml, L, bounds,
                       (const int32_t *)cum, offsets, n_intervals, min_overlap_ms, min_overlap_pct, use_lds, diff);
    if (int rc = check_launch("surface_events_nodes_kernel")) return rc;
    // events per workgroup: as many as leave some 16384 workgroups to the device (fewer atomics, the same sums)
    const int64_t level_blocks = ceil_div(K, WAVE);
    int64_t group = most_events * level_blocks * channels / 16384;
    group = group < 1 ? 1 : (group > MAX_GROUP ? MAX_GROUP : group);
    const int64_t groups = most_events > 0 ? ceil_div(most_events, group) : 1;      // (no event: every workgroup returns at once)
    hipLaunchKernelGGL(surface_events_match_kernel, dim3((unsigned)groups, (unsigned)level_blocks, (unsigned)channels), dim3(WAVE), 0, st,
                       (const bin_t *)trees, w.tree_pitch, frames, K, fps, ml, L, bounds, offsets, n_intervals, (int)group, min_overlap_ms,
                       min_overlap_pct, (unsigned long long *)events);
    if (int rc = check_launch("surface_events_match_kernel")) return rc;
    hipLaunchKernelGGL(surface_events_prefix_kernel, dim3((unsigned)(channels * L * DIFF_FIELDS)), dim3(THREADS), 0, st,
                       (const long long *)diff, K, L, offsets, n_intervals, (long long *)scores, (long long *)events);
    return check_launch("surface_events_prefix_kernel");
}
