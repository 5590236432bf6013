// What the dense sweep's sources share (surface.hip, surface_events.hip): the bins of a track, the binary tree of minima over them,
// the two nearest-smaller searches in it, the scan of the interval index, the size checks, and the host driver of the four launches
// that build all of this.  Each source gets its own copy of the kernels below (anonymous namespace).
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

inline bool surface_sizes_ok(int64_t C, int64_t T, int64_t n_intervals, int64_t K, int64_t L) {
    return C >= 1 && C <= MAX_C && T >= 1 && T <= MAX_T && n_intervals >= 0 && n_intervals <= MAX_INTERVALS && K >= 1 &&
           K <= MAX_LEVELS && L >= 1 && L <= MAX_L;
}
#define SURFACE_SIZES_MESSAGE(who)                                                                                                 \
    who ": channels 1..%d, frames 1..2^30, intervals 0..2^30, levels 1..%d, min_lengths 1..%d (got %lld, %lld, %lld, %d, %d)", MAX_C, \
        MAX_LEVELS, MAX_L, (long long)channels, (long long)frames, (long long)n_intervals, n_levels, n_min_lengths

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
}  // namespace
}  // namespace surface
}  // namespace lad
