// What the dense sweep's sources share (surface.hip, surface_events.hip): the bins of a track, the binary tree of minima over them,
// the two nearest-smaller searches in it, the scan of the interval index, the body of the nodes kernel (score_nodes: templated on
// the fields of the difference array and on what fills those behind run_fields' seven), the prefix sum over the levels
// (prefix_levels), the workspace (Workspace, layout, workspace_bytes), and the host half of an entry point up to and including the
// nodes launch (sweep_nodes: the checks, the carving, the memset, build_trees' four launches, the decision between LDS and global
// adds).  Each source gets its own copy of the kernels below (anonymous namespace) and keeps a __global__ of its own name around
// each shared body.
//
// Frame value and comparison are lad_runs_count's: q = load_fixed(p) in float64, frame i is on at level j iff q > levels[j], i.e.
// iff j < bin[i], bin[i] = the number of levels strictly below q (0 for NaN and beyond the track).
//
// Nearest smaller values: a binary tree of minima over the bins, level h of it holding min(bin[p 2^h .. (p + 1) 2^h - 1]) at p,
// ceil(T / 2^h) nodes.  A search walks up from its frame, looking at the one sibling on its side of each ancestor, until a sibling's
// minimum qualifies, then down into that sibling, taking the child nearer to the frame whenever it qualifies.  At most
// ceil(log2 T) steps up and as many down, ONE read of the tree per step: at most 2 ceil(log2 T) (60 for the largest track, 38 for
// 360,000 frames) whatever the track looks like -- a monotone ramp, a constant track and a plateau with one dip included.
// Every read of the tree is below its level's node count.
#pragma once
#include "lad_sweep_tile.h"

namespace lad {
namespace surface {
namespace {
using namespace lad::sweep;

constexpr int MAX_LEVELS = 4096;                 // lad_surface_max_levels(): the levels of a call fill 32 KB of LDS
constexpr int CHUNK_BITS = 11;
constexpr int CHUNK = 1 << CHUNK_BITS;           // frames per workgroup: lad_surface_tile_frames(); tree levels per launch: 11
constexpr int TREE_LEVELS = 1 + 3 * CHUNK_BITS;  // levels 0..33 are written; a search never leaves level ceil(log2 T) <= 30
typedef unsigned short bin_t;                    // 0..4096
constexpr bin_t ABSENT = 0xffff;                 // beyond a level's last node: never a minimum
constexpr int MAX_PRIVATE_BYTES = 48 * 1024;     // the difference array of one channel in LDS, if it fits

// nodes of level h, and the entries a level occupies in a channel's tree (at least its nodes, whatever T)
__host__ __device__ inline int64_t nodes_at(int64_t T, int h) { return (T + ((int64_t)1 << h) - 1) >> h; }
__host__ __device__ inline int64_t pitch_at(int64_t T, int h) { return (T >> h) + 2; }
inline int64_t tree_entries(int64_t T) {
    int64_t n = 0;
    for (int h = 0; h < TREE_LEVELS; ++h) n += pitch_at(T, h);
    return n;
}
// entries between two channels' trees: every channel's tree starts at a multiple of 256 bytes
inline int64_t tree_pitch_of(int64_t T) { return up256(tree_entries(T) * (int64_t)sizeof(bin_t)) / (int64_t)sizeof(bin_t); }

// s holds 2048 entries of level h0 (chunk `chunk` of it, ABSENT beyond the level's nodes): levels h0 + 1 .. h0 + 11 of the chunk
// into the tree; t: a second buffer of 1024 entries
__device__ inline void reduce_chunk(bin_t *s, bin_t *t, bin_t *__restrict__ tree, int64_t T, int h0, int64_t chunk) {
    int64_t off = 0;
    for (int h = 0; h <= h0; ++h) off += pitch_at(T, h);
    bin_t *src = s, *dst = t;
    for (int d = 1; d <= CHUNK_BITS; ++d) {
        const int cnt = CHUNK >> d;
        const int64_t n = nodes_at(T, h0 + d), first = chunk * cnt;
        __syncthreads();
        for (int i = threadIdx.x; i < cnt; i += THREADS) {
            const bin_t a = src[2 * i], b = src[2 * i + 1];
            const bin_t m = a < b ? a : b;
            dst[i] = m;
            if (first + i < n) tree[off + first + i] = m;
        }
        off += pitch_at(T, h0 + d);
        bin_t *x = src;
        src = dst;
        dst = x;
    }
}

template <typename T>
__global__ __launch_bounds__(THREADS) void surface_bins_kernel(const T *__restrict__ probs, int64_t n, const double *__restrict__ levels,
                                                               int K, bin_t *__restrict__ trees, int64_t tree_pitch) {
    __shared__ double lev[MAX_LEVELS];
    __shared__ bin_t s[CHUNK], t[CHUNK / 2];
    for (int k = threadIdx.x; k < K; k += THREADS) lev[k] = levels[k];
    __syncthreads();
    const int64_t c = blockIdx.y, chunk0 = (int64_t)blockIdx.x * CHUNK;
    const T *chan = probs + c * n;
    bin_t *tree = trees + c * tree_pitch;
    for (int j = threadIdx.x; j < CHUNK; j += THREADS) {
        const int64_t i = chunk0 + j;
        bin_t b = ABSENT;
        if (i < n) {
            const double q = load_fixed(chan, i, n);
            int lo = 0, len = K;                     // levels strictly below q: NaN compares false and stays at 0
            while (len > 0) {
                const int half = len >> 1;
                if (lev[lo + half] < q) {
                    lo += half + 1;
                    len -= half + 1;
                } else {
                    len = half;
                }
            }
            b = (bin_t)lo;
            tree[i] = b;
        }
        s[j] = b;
    }
    reduce_chunk(s, t, tree, n, 0, blockIdx.x);
}

__global__ __launch_bounds__(THREADS) void surface_tree_kernel(bin_t *__restrict__ trees, int64_t tree_pitch, int64_t n, int h0) {
    __shared__ bin_t s[CHUNK], t[CHUNK / 2];
    bin_t *tree = trees + (int64_t)blockIdx.y * tree_pitch;
    int64_t off = 0;
    for (int h = 0; h < h0; ++h) off += pitch_at(n, h);
    const int64_t nodes = nodes_at(n, h0), chunk0 = (int64_t)blockIdx.x * CHUNK;
    for (int j = threadIdx.x; j < CHUNK; j += THREADS) s[j] = chunk0 + j < nodes ? tree[off + chunk0 + j] : ABSENT;
    reduce_chunk(s, t, tree, n, h0, blockIdx.x);
}

__global__ __launch_bounds__(THREADS) void surface_cum_kernel(const int32_t *__restrict__ bounds, const int32_t *__restrict__ offsets,
                                                              int64_t n_intervals, int32_t *__restrict__ cum, int64_t segments) {
    scan_index_and_counts(bounds, offsets, n_intervals, cum, segments, nullptr, 0, nullptr);     // (no workgroup `segments`)
}

// the nearest frame left of i whose bin is <= x, or -1; found: its bin (0 for -1)
__device__ inline int64_t nearest_left_le(const bin_t *__restrict__ tree, int64_t T, int64_t i, int x, int &found) {
    int64_t p = i, off = 0;
    int h = 0;
    found = 0;
    for (;;) {
        if (p == 0 || h >= TREE_LEVELS - 1) return -1;
        if ((p & 1) && tree[off + p - 1] <= x) {
            --p;
            break;
        }
        off += pitch_at(T, h);
        p >>= 1;
        ++h;
    }
    while (h > 0) {                                  // node p of level h lies wholly inside the track: both children exist
        --h;
        off -= pitch_at(T, h);
        const int64_t r = 2 * p + 1;
        p = (r < nodes_at(T, h) && tree[off + r] <= x) ? r : 2 * p;
    }
    found = tree[p];
    return p;
}

// the nearest frame right of i whose bin is < x (x > 0), or T: the frames beyond the track have bin 0; found: its bin (0 for T)
__device__ inline int64_t nearest_right_lt(const bin_t *__restrict__ tree, int64_t T, int64_t i, int x, int &found) {
    int64_t p = i, off = 0;
    int h = 0;
    found = 0;
    for (;;) {
        if (h >= TREE_LEVELS - 1) return T;
        if (!(p & 1)) {
            if (p + 1 >= nodes_at(T, h)) return T;   // the last node of its level, and so are its ancestors
            if (tree[off + p + 1] < x) {
                ++p;
                break;
            }
        }
        off += pitch_at(T, h);
        p >>= 1;
        ++h;
    }
    while (h > 0) {                                  // the last node of a level may lack its right child: then the left one qualifies
        --h;
        off -= pitch_at(T, h);
        const int64_t l = 2 * p;
        p = (tree[off + l] < x || l + 1 >= nodes_at(T, h)) ? l : l + 1;
    }
    found = tree[p];
    return p;
}

// The body of a nodes kernel, one lane per frame: the two searches, run_fields for a representative, the fields behind its seven
// from extra(first, last, fps, ml, L, v) (FIELDS in all), then +w at row base and -w at row top of the difference array per kept
// min_length: into a copy of the channel's array in LDS when the host found that it fits (use_lds), flushed with one vector global
// atomic per non-zero cell; straight to global memory otherwise.
template <int FIELDS, typename Extra>
__device__ inline void score_nodes(const bin_t *__restrict__ trees, int64_t tree_pitch, int64_t T, int K, const double *__restrict__ fps,
                                   const MinLengths &ml, int L, const int32_t *__restrict__ bounds, const int32_t *__restrict__ cum,
                                   const int32_t *__restrict__ offsets, int64_t n_intervals, int use_lds,
                                   unsigned long long *__restrict__ diff, Extra extra) {
    extern __shared__ unsigned long long priv[];
    const int64_t c = blockIdx.y;
    const bin_t *tree = trees + c * tree_pitch;
    const int cells = (K + 1) * L * FIELDS;
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
        int32_t v[FIELDS], time[SCORE_FIELDS];
        const int32_t first = (int32_t)(left + 1), last = (int32_t)(right - 1);
        const unsigned keep = run_fields(c, first, last, f, ml, L, bounds, cum, offsets, n_intervals, time);
#pragma unroll
        for (int fd = 0; fd < SCORE_FIELDS; ++fd) v[fd] = time[fd];
        extra(first, last, f, ml, L, v);
#pragma unroll
        for (int l = 0; l < MAX_L; ++l) {
            if (l < L && ((keep >> l) & 1u)) {
#pragma unroll
                for (int fd = 0; fd < FIELDS; ++fd) {
                    if (v[fd] != 0) {
                        const unsigned long long w = (unsigned long long)(long long)v[fd];
                        const int up = (base * L + l) * FIELDS + fd, down = (top * L + l) * FIELDS + fd;
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

// one workgroup, one (channel, min_length, field): out[j * out_step] = the sum of in[0 .. j] (in_step apart), j < K: block_scan
// over the levels.  Row K of a difference array is never read.
__device__ inline void prefix_levels(const long long *__restrict__ in, int64_t in_step, long long *__restrict__ out, int64_t out_step,
                                     int K) {
    block_scan<long long>(0, K, [&](int64_t j) { return in[j * in_step]; },
                          [&](int64_t j, long long v) { out[j * out_step] = v + in[j * in_step]; });
}

inline bool surface_sizes_ok(int64_t C, int64_t T, int64_t n_intervals, int64_t K, int64_t L) {
    return C >= 1 && C <= MAX_C && T >= 1 && T <= MAX_T && n_intervals >= 0 && n_intervals <= MAX_INTERVALS && K >= 1 &&
           K <= MAX_LEVELS && L >= 1 && L <= MAX_L;
}
inline int fail_sizes(const char *who, int64_t channels, int64_t frames, int64_t n_intervals, int32_t n_levels, int32_t n_min_lengths) {
    return fail(LAD_ERR_INVALID,
                "%s: channels 1..%d, frames 1..2^30, intervals 0..2^30, levels 1..%d, min_lengths 1..%d (got %lld, %lld, %lld, %d, %d)", who,
                MAX_C, MAX_LEVELS, MAX_L, (long long)channels, (long long)frames, (long long)n_intervals, n_levels, n_min_lengths);
}

// the workspace of a call whose difference array has `fields` fields per (level, min_length): byte offsets of its parts
struct Workspace {
    int64_t levels, cum, diff, trees, tree_pitch, bytes;
};
inline Workspace layout(int64_t C, int64_t T, int64_t n_intervals, int64_t K, int64_t L, int fields) {   // sizes surface_sizes_ok has passed
    Workspace w;
    w.levels = 0;
    w.cum = up256(K * 8);
    w.diff = w.cum + up256(n_intervals * 4);
    w.trees = w.diff + up256(C * (K + 1) * L * fields * 8);
    w.tree_pitch = tree_pitch_of(T);
    w.bytes = w.trees + C * w.tree_pitch * (int64_t)sizeof(bin_t) + 256;
    return w;
}
// the two *_workspace_bytes queries: -1 (reported) for sizes out of range
inline int64_t workspace_bytes(const char *who, int64_t channels, int64_t frames, int64_t n_intervals, int32_t n_levels,
                               int32_t n_min_lengths, int fields) {
    if (!surface_sizes_ok(channels, frames, n_intervals, n_levels, n_min_lengths)) {
        fail_sizes(who, channels, frames, n_intervals, n_levels, n_min_lengths);
        return -1;
    }
    return layout(channels, frames, n_intervals, n_levels, n_min_lengths, fields).bytes;
}

// what both entry points ask of their levels before anything is launched
inline int check_levels(const char *who, const double *levels, int K) {
    for (int k = 0; k < K; ++k) {
        LAD_REQUIRE(std::isfinite(levels[k]), "%s: levels[%d] = %g is not finite", who, k, levels[k]);
        LAD_REQUIRE(k == 0 || levels[k] > levels[k - 1], "%s: levels must ascend strictly: levels[%d] = %.17g, levels[%d] = %.17g", who,
                    k - 1, levels[k - 1], k, levels[k]);
    }
    return LAD_OK;
}

// one copy (the levels) and four launches: the bins and the tree of every channel, and the running lengths of the interval index
inline int build_trees(const void *probs, int32_t dtype, int64_t channels, int64_t frames, const double *levels, int K,
                       double *levels_dev, bin_t *trees, int64_t tree_pitch, const int32_t *bounds, const int32_t *offsets,
                       int64_t n_intervals, int32_t *cum, hipStream_t st) {
    LAD_HIP_CHECK(hipMemcpyAsync(levels_dev, levels, (size_t)K * sizeof(double), hipMemcpyHostToDevice, st));
    const dim3 grid((unsigned)ceil_div(frames, CHUNK), (unsigned)channels);
    with_track_type(dtype, [&](auto z) {
        using T = decltype(z);
        hipLaunchKernelGGL(surface_bins_kernel<T>, grid, dim3(THREADS), 0, st, (const T *)probs, frames, (const double *)levels_dev, K, trees,
                           tree_pitch);
    });
    if (int rc = check_launch("surface_bins_kernel")) return rc;
    for (int h0 = CHUNK_BITS; h0 < TREE_LEVELS - 1; h0 += CHUNK_BITS) {
        const int64_t nodes = (frames + ((int64_t)1 << h0) - 1) >> h0;
        hipLaunchKernelGGL(surface_tree_kernel, dim3((unsigned)ceil_div(nodes, CHUNK), (unsigned)channels), dim3(THREADS), 0, st, trees,
                           tree_pitch, frames, h0);
        if (int rc = check_launch("surface_tree_kernel")) return rc;
    }
    const int64_t segments = channels * CLASSES;
    hipLaunchKernelGGL(surface_cum_kernel, dim3((unsigned)segments), dim3(THREADS), 0, st, bounds, offsets, n_intervals, cum, segments);
    return check_launch("surface_cum_kernel");
}

// what the launches behind the nodes kernel need of a call
struct Sweep {
    MinLengths ml;
    const bin_t *trees;
    int64_t tree_pitch;
    const long long *diff;
    hipStream_t st;
};

// Everything lad_score_surface and lad_score_surface_events (criteria: its two values, null for the other) do alike, up to and
// including the nodes launch.  The checks, in this order: sizes, criteria, null buffers (results: the entry point's own test of its
// result arrays), interval bounds, dtype, levels, min_lengths, the index.  Then the workspace is carved, the difference array of
// FIELDS fields zeroed, the trees built, and launch_nodes(grid, lds_bytes, st, trees, tree_pitch, ml, cum, use_lds, diff) called:
// the difference array of one channel is kept in LDS iff it fits into MAX_PRIVATE_BYTES.
template <int FIELDS, typename Launch>
inline int sweep_nodes(const char *who, const char *nodes_name, const int32_t *criteria, const void *probs, int32_t dtype, int64_t channels,
                       int64_t frames, const double *levels, int32_t n_levels, const int32_t *bounds, const int32_t *offsets,
                       const int32_t *bounds_host, const int32_t *offsets_host, int64_t n_intervals, const double *fps,
                       const double *fps_host, const double *min_lengths, int32_t n_min_lengths, void *workspace, bool results,
                       void *stream, Sweep &s, Launch launch_nodes) {
    if (!surface_sizes_ok(channels, frames, n_intervals, n_levels, n_min_lengths))
        return fail_sizes(who, channels, frames, n_intervals, n_levels, n_min_lengths);
    if (int rc = criteria ? check_criteria(who, criteria[0], criteria[1]) : LAD_OK) return rc;
    LAD_REQUIRE(probs && levels && offsets && offsets_host && fps && fps_host && min_lengths && workspace && results, "%s: null buffer",
                who);
    LAD_REQUIRE(n_intervals == 0 || (bounds && bounds_host), "%s: null interval bounds", who);
    if (int rc = check_dtype(who, dtype)) return rc;
    const int K = n_levels, L = n_min_lengths;
    if (int rc = check_levels(who, levels, K)) return rc;
    if (int rc = load_min_lengths(who, min_lengths, L, s.ml)) return rc;
    if (int rc = check_index(who, channels, frames, fps_host, offsets_host, bounds_host, n_intervals)) return rc;

    const Workspace w = layout(channels, frames, n_intervals, K, L, FIELDS);
    char *ws = (char *)workspace;
    double *levels_dev = (double *)(ws + w.levels);
    int32_t *cum = (int32_t *)(ws + w.cum);
    unsigned long long *diff = (unsigned long long *)(ws + w.diff);
    bin_t *trees = (bin_t *)(ws + w.trees);
    s.trees = trees;
    s.tree_pitch = w.tree_pitch;
    s.diff = (const long long *)diff;
    s.st = (hipStream_t)stream;
    const int64_t private_bytes = (int64_t)(K + 1) * L * FIELDS * (int64_t)sizeof(long long);
    LAD_HIP_CHECK(hipMemsetAsync(diff, 0, (size_t)(channels * private_bytes), s.st));
    if (int rc = build_trees(probs, dtype, channels, frames, levels, K, levels_dev, trees, w.tree_pitch, bounds, offsets, n_intervals, cum,
                             s.st))
        return rc;
    const int use_lds = private_bytes <= MAX_PRIVATE_BYTES;
    launch_nodes(dim3((unsigned)ceil_div(frames, CHUNK), (unsigned)channels), use_lds ? (size_t)private_bytes : (size_t)0, s.st,
                 (const bin_t *)trees, w.tree_pitch, s.ml, (const int32_t *)cum, use_lds, diff);
    return check_launch(nodes_name);
}
}  // namespace
}  // namespace surface
}  // namespace lad
