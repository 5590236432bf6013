// Confidence of an instance: the sum and the earliest peak of the probability track over every row (first, last) of the span tables.
//
// Not in the reference, which returns bare (start, end).  The statistic is a segmented reduction over spans of any length, so it is
// not computed by walking them: lad_span_stats_prepare writes, once per track and independent of any setting,
//   prefix[c][i] = Q(0) + ... + Q(i), int64, Q(i) = rint(w(i) * 2^32)                  (the sum of a span: two reads)
//   a binary tree of maxima over w, level h holding max(w[p 2^h .. (p + 1) 2^h - 1]) at p (float64; level 0 is the track itself,
//   read through load_fixed, and is not stored)                                       (the peak of a span: O(log frames) reads)
// and lad_span_stats answers every row with one lane from the two.  include/lad_hip.h has the convention in full.
//
// Prepare, five launches whatever the sizes and whatever the data holds, no atomics, no workgroup waits for another:
//   span_chunk_kernel   (chunk of 2048 frames, channel): tree levels 1..11 of the chunk, and the chunk's sum of Q
//   span_offsets_kernel (channel): exclusive scan of the chunk sums, in place
//   span_prefix_kernel  (chunk, channel): the chunk again: prefix[i] = chunk offset + scan inside the chunk
//   span_tree_kernel    twice: levels 12..22 from level 11, levels 23..33 from level 22 (a search never leaves level 30)
// lad_span_stats: one copy (the first row of every channel, C + 1 int64, into the workspace's last part) and one launch.
//
// The peak of a row [first, last]: the row is cut into the at most 2 (ceil(log2 frames) + 1) maximal tree nodes inside it, the
// usual bottom-up walk of the two edges; the nodes of the left edge come in ascending frame order (a later one wins only if it is
// strictly larger), those of the right edge in descending order (a later one wins if it is at least as large), and every node of the
// left edge lies before every node of the right one (the left wins a tie).  From the winning node the walk goes down, into the left
// child iff its maximum equals the node's: one read per level.  At most 3 ceil(log2 frames) + 2 reads of the tree (level 0
// included): 92 for the largest track, 59 for 360,000 frames, whatever the spans and the track look like -- one span as long as a
// constant track included.  Every node read lies inside the row, so inside the track and below its level's node count.
// Integer sums and float64 compares only: two calls write identical bytes, and the host form computes the same integers.
#include <vector>

#include "lad_sweep_tile.h"

namespace {
using namespace lad::sweep;

constexpr int CHUNK_BITS = 11;
constexpr int CHUNK = 1 << CHUNK_BITS;           // frames per workgroup: lad_span_stats_tile_frames(); tree levels per launch: 11
constexpr int TREE_LEVELS = 1 + 3 * CHUNK_BITS;  // levels 1..33 are written; a search never leaves level ceil(log2 T) <= 30
constexpr double ABSENT = -1.0;                  // beyond a level's last node: never a maximum (w >= 0)
constexpr double TWO32 = 4294967296.0;

// nodes of level h, and the entries a level occupies in a channel's tree (at least its nodes, whatever T)
__host__ __device__ inline int64_t nodes_at(int64_t T, int h) { return (T + ((int64_t)1 << h) - 1) >> h; }
__host__ __device__ inline int64_t pitch_at(int64_t T, int h) { return (T >> h) + 2; }
// entries between two channels' trees (levels 1..33): every channel's tree starts at a multiple of 256 bytes
inline int64_t tree_pitch_of(int64_t T) {
    int64_t n = 0;
    for (int h = 1; h < TREE_LEVELS; ++h) n += pitch_at(T, h);
    return lad::up256(n * 8) / 8;
}
inline int64_t chunks_of(int64_t T) { return lad::ceil_div(T, CHUNK); }

// the parts of a workspace
struct Layout {
    int64_t prefix, tree, chunk_off, first_row, bytes;   // byte offsets, and the total
    int64_t tree_pitch, chunks;
};
inline Layout layout_of(int64_t C, int64_t T) {
    Layout l;
    l.tree_pitch = tree_pitch_of(T);
    l.chunks = chunks_of(T);
    l.prefix = 0;
    l.tree = l.prefix + lad::up256(C * T * 8);
    l.chunk_off = l.tree + lad::up256(C * l.tree_pitch * 8);
    l.first_row = l.chunk_off + lad::up256(C * l.chunks * 8);
    l.bytes = l.first_row + lad::up256((C + 1) * 8);
    return l;
}

// w(i): the decoders' frame value, 0.0 for a NaN frame (and beyond the track)
template <typename T>
__device__ inline double load_w(const T *__restrict__ chan, int64_t i, int64_t n) {
    const double v = load_fixed(chan, i, n);
    return v == v ? v : 0.0;
}
__device__ inline long long fixed_q(double w) { return (long long)rint(w * TWO32); }

// s holds 2048 entries of level h0 (chunk `chunk` of it, ABSENT beyond the level's nodes): levels h0 + 1 .. h0 + 11 of the chunk
// into the tree, whose level 1 stands at entry 0; t: a second buffer of 1024 entries
__device__ inline void reduce_chunk(double *s, double *t, double *__restrict__ tree, int64_t T, int h0, int64_t chunk) {
    int64_t off = 0;
    for (int h = 1; h <= h0; ++h) off += pitch_at(T, h);
    double *src = s, *dst = t;
    for (int d = 1; d <= CHUNK_BITS; ++d) {
        const int cnt = CHUNK >> d;
        const int64_t n = nodes_at(T, h0 + d), first = chunk * cnt;
        __syncthreads();
        for (int i = threadIdx.x; i < cnt; i += THREADS) {
            const double a = src[2 * i], b = src[2 * i + 1];
            const double m = a < b ? b : a;
            dst[i] = m;
            if (first + i < n) tree[off + first + i] = m;
        }
        off += pitch_at(T, h0 + d);
        double *x = src;
        src = dst;
        dst = x;
    }
}

template <typename T>
__global__ __launch_bounds__(THREADS) void span_chunk_kernel(const T *__restrict__ probs, int64_t n, double *__restrict__ trees,
                                                             int64_t tree_pitch, long long *__restrict__ chunk_sums, int64_t chunks) {
    __shared__ double s[CHUNK], t[CHUNK / 2];
    const int64_t c = blockIdx.y, chunk0 = (int64_t)blockIdx.x * CHUNK;
    const T *chan = probs + c * n;
    for (int j = threadIdx.x; j < CHUNK; j += THREADS) s[j] = chunk0 + j < n ? load_w(chan, chunk0 + j, n) : ABSENT;
    __syncthreads();
    const int64_t hi = chunk0 + CHUNK < n ? chunk0 + CHUNK : n;
    const long long sum = block_scan<long long>(chunk0, hi, [&](int64_t i) { return fixed_q(s[i - chunk0]); }, [](int64_t, long long) {});
    if (threadIdx.x == 0 && (int64_t)blockIdx.x < chunks) chunk_sums[c * chunks + blockIdx.x] = sum;
    reduce_chunk(s, t, trees + c * tree_pitch, n, 0, blockIdx.x);
}

__global__ __launch_bounds__(THREADS) void span_offsets_kernel(long long *__restrict__ chunk_sums, int64_t chunks) {
    long long *mine = chunk_sums + (int64_t)blockIdx.x * chunks;
    block_scan<long long>(0, chunks, [&](int64_t i) { return mine[i]; }, [&](int64_t i, long long v) { mine[i] = v; });
}

template <typename T>
__global__ __launch_bounds__(THREADS) void span_prefix_kernel(const T *__restrict__ probs, int64_t n, const long long *__restrict__ chunk_off,
                                                              int64_t chunks, long long *__restrict__ prefix) {
    const int64_t c = blockIdx.y, chunk0 = (int64_t)blockIdx.x * CHUNK;
    if (chunk0 >= n) return;                                 // (the whole workgroup)
    const T *chan = probs + c * n;
    long long *dst = prefix + c * n;
    const long long before = chunk_off[c * chunks + blockIdx.x];
    const int64_t hi = chunk0 + CHUNK < n ? chunk0 + CHUNK : n;
    block_scan<long long>(chunk0, hi, [&](int64_t i) { return fixed_q(load_w(chan, i, n)); },
                          [&](int64_t i, long long v) { dst[i] = before + v + fixed_q(load_w(chan, i, n)); });
}

__global__ __launch_bounds__(THREADS) void span_tree_kernel(double *__restrict__ trees, int64_t tree_pitch, int64_t n, int h0) {
    __shared__ double s[CHUNK], t[CHUNK / 2];
    double *tree = trees + (int64_t)blockIdx.y * tree_pitch;
    int64_t off = 0;
    for (int h = 1; h < h0; ++h) off += pitch_at(n, h);
    const int64_t nodes = nodes_at(n, h0), chunk0 = (int64_t)blockIdx.x * CHUNK;
    for (int j = threadIdx.x; j < CHUNK; j += THREADS) s[j] = chunk0 + j < nodes ? tree[off + chunk0 + j] : ABSENT;
    reduce_chunk(s, t, tree, n, h0, blockIdx.x);
}

// node p of level h of a channel's tree; off: the entries of levels 1..h-1
template <typename T>
__device__ inline double node(const T *__restrict__ chan, const double *__restrict__ tree, int64_t n, int h, int64_t off, int64_t p) {
    return h == 0 ? load_w(chan, p, n) : tree[off + p];
}

template <typename T>
__global__ __launch_bounds__(THREADS) void span_rows_kernel(const T *__restrict__ probs, int64_t n, const long long *__restrict__ prefix,
                                                            const double *__restrict__ trees, int64_t tree_pitch,
                                                            const int32_t *__restrict__ table, int64_t rows,
                                                            const int64_t *__restrict__ first_row, int64_t C, long long *__restrict__ sums,
                                                            int32_t *__restrict__ peaks, double *__restrict__ peak_values) {
    const int64_t row = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (row >= rows) return;
    const int64_t first = table[2 * row], last = table[2 * row + 1];
    long long sum = 0;
    int64_t peak = -1;
    double value = 0.0;
    if (first >= 0 && last < n && first <= last) {
        const int64_t c = table_of_row(first_row, C, row);
        const T *chan = probs + c * n;
        const long long *pre = prefix + c * n;
        const double *tree = trees + c * tree_pitch;
        sum = pre[last] - (first > 0 ? pre[first - 1] : 0);
        // up: the maximal nodes inside [l, r) of every level; best_*: the winner of each edge, (level, node, entries below the level)
        int64_t l = first, r = last + 1, off = 0;
        double lv = ABSENT, rv = ABSENT;
        int lh = 0, rh = 0;
        int64_t lp = 0, rp = 0, loff = 0, roff = 0;
        for (int h = 0; l < r && h < TREE_LEVELS; ++h) {
            if (l & 1) {
                const double v = node(chan, tree, n, h, off, l);
                if (v > lv) lv = v, lh = h, lp = l, loff = off;
                ++l;
            }
            if (r & 1) {
                --r;
                const double v = node(chan, tree, n, h, off, r);
                if (v >= rv) rv = v, rh = h, rp = r, roff = off;
            }
            l >>= 1;
            r >>= 1;
            if (h > 0) off += pitch_at(n, h);
        }
        int h = lh;
        int64_t p = lp;
        off = loff;
        value = lv;
        if (rv > lv) h = rh, p = rp, off = roff, value = rv;
        // down: node p of level h lies inside the row, so both children exist; the left one iff it holds the maximum
        while (h > 0) {
            --h;
            if (h > 0) off -= pitch_at(n, h);
            p = node(chan, tree, n, h, off, 2 * p) == value ? 2 * p : 2 * p + 1;
        }
        peak = p;
    }
    sums[row] = sum;
    peaks[row] = (int32_t)peak;
    peak_values[row] = value;
}

inline bool sizes_ok(int64_t C, int64_t T) { return C >= 1 && C <= MAX_C && T >= 1 && T <= MAX_T; }
inline bool overlap(const void *p, int64_t pn, const void *q, int64_t qn) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return pn > 0 && qn > 0 && a < b + (uintptr_t)qn && b < a + (uintptr_t)pn;
}
}  // namespace

extern "C" int32_t lad_span_stats_tile_frames(void) { return CHUNK; }

extern "C" int64_t lad_span_stats_workspace_bytes(int64_t channels, int64_t frames) {
    if (!sizes_ok(channels, frames)) {
        lad::fail(LAD_ERR_INVALID, "lad_span_stats_workspace_bytes: channels 1..%d, frames 1..2^30 (got %lld, %lld)", MAX_C,
                  (long long)channels, (long long)frames);
        return -1;
    }
    return layout_of(channels, frames).bytes;
}

extern "C" int lad_span_stats_prepare(const void *probs, int32_t dtype, int64_t channels, int64_t frames, void *workspace, void *stream) {
    using namespace lad;
    LAD_REQUIRE(probs && workspace, "lad_span_stats_prepare: null buffer");
    if (int rc = check_dtype("lad_span_stats_prepare", dtype)) return rc;
    LAD_REQUIRE(sizes_ok(channels, frames), "lad_span_stats_prepare: channels 1..%d, frames 1..2^30 (got %lld, %lld)", MAX_C,
                (long long)channels, (long long)frames);
    const Layout lay = layout_of(channels, frames);
    LAD_REQUIRE(!overlap(probs, channels * frames * (dtype == LAD_RUNS_F32 ? 4 : 8), workspace, lay.bytes),
                "lad_span_stats_prepare: probs overlaps the workspace");
    const hipStream_t st = (hipStream_t)stream;
    long long *prefix = (long long *)((char *)workspace + lay.prefix);
    double *trees = (double *)((char *)workspace + lay.tree);
    long long *chunk_off = (long long *)((char *)workspace + lay.chunk_off);
    const dim3 grid((unsigned)lay.chunks, (unsigned)channels);
    with_track_type(dtype, [&](auto z) {
        using T = decltype(z);
        hipLaunchKernelGGL(span_chunk_kernel<T>, grid, dim3(THREADS), 0, st, (const T *)probs, frames, trees, lay.tree_pitch, chunk_off,
                           lay.chunks);
    });
    if (int rc = check_launch("span_chunk_kernel")) return rc;
    hipLaunchKernelGGL(span_offsets_kernel, dim3((unsigned)channels), dim3(THREADS), 0, st, chunk_off, lay.chunks);
    if (int rc = check_launch("span_offsets_kernel")) return rc;
    with_track_type(dtype, [&](auto z) {
        using T = decltype(z);
        hipLaunchKernelGGL(span_prefix_kernel<T>, grid, dim3(THREADS), 0, st, (const T *)probs, frames, (const long long *)chunk_off,
                           lay.chunks, prefix);
    });
    if (int rc = check_launch("span_prefix_kernel")) return rc;
    for (int h0 = CHUNK_BITS; h0 < TREE_LEVELS - 1; h0 += CHUNK_BITS) {
        hipLaunchKernelGGL(span_tree_kernel, dim3((unsigned)ceil_div(nodes_at(frames, h0), CHUNK), (unsigned)channels), dim3(THREADS), 0, st,
                           trees, lay.tree_pitch, frames, h0);
        if (int rc = check_launch("span_tree_kernel")) return rc;
    }
    return LAD_OK;
}

extern "C" int lad_span_stats(const void *probs, int32_t dtype, int64_t channels, int64_t frames, const void *workspace,
                              const int32_t *table, const int32_t *counts_host, int32_t n_settings, int64_t *sums, int32_t *peaks,
                              double *peak_values, void *stream) {
    using namespace lad;
    LAD_REQUIRE(probs && workspace && counts_host && sums && peaks && peak_values, "lad_span_stats: null buffer");
    if (int rc = check_dtype("lad_span_stats", dtype)) return rc;
    LAD_REQUIRE(sizes_ok(channels, frames) && n_settings >= 1, "lad_span_stats: channels 1..%d, frames 1..2^30, settings >= 1 (got %lld, %lld, %d)",
                MAX_C, (long long)channels, (long long)frames, n_settings);
    const int64_t K = n_settings;
    int64_t rows = 0;
    for (int64_t i = 0; i < channels * K; ++i) {
        LAD_REQUIRE(counts_host[i] >= 0, "lad_span_stats: counts_host[%lld] = %d is negative", (long long)i, counts_host[i]);
        rows += counts_host[i];
    }
    LAD_REQUIRE(rows <= MAX_ROWS, "lad_span_stats: %lld table rows, at most 2^38 per call", (long long)rows);
    LAD_REQUIRE(rows == 0 || table, "lad_span_stats: null table");
    const Layout lay = layout_of(channels, frames);
    const int64_t track_bytes = channels * frames * (dtype == LAD_RUNS_F32 ? 4 : 8);
    const void *outs[3] = {sums, peaks, peak_values};
    const int64_t out_bytes[3] = {rows * 8, rows * 4, rows * 8};
    static const char *const names[3] = {"sums", "peaks", "peak_values"};
    for (int o = 0; o < 3; ++o) {
        LAD_REQUIRE(!overlap(outs[o], out_bytes[o], probs, track_bytes), "lad_span_stats: %s overlaps probs", names[o]);
        LAD_REQUIRE(!overlap(outs[o], out_bytes[o], table, rows * 8), "lad_span_stats: %s overlaps the table", names[o]);
        LAD_REQUIRE(!overlap(outs[o], out_bytes[o], workspace, lay.bytes), "lad_span_stats: %s overlaps the workspace", names[o]);
        for (int q = 0; q < o; ++q)
            LAD_REQUIRE(!overlap(outs[o], out_bytes[o], outs[q], out_bytes[q]), "lad_span_stats: %s overlaps %s", names[o], names[q]);
    }
    if (rows == 0) return LAD_OK;

    // the first row of every channel's tables: the one part of the workspace that this call writes (calls that share a workspace
    // are ordered by their stream)
    const hipStream_t st = (hipStream_t)stream;
    int64_t *first_row = (int64_t *)((char *)workspace + lay.first_row);
    {
        std::vector<int64_t> staged((size_t)channels + 1);
        int64_t *host = staged.data(), at = 0;
        for (int64_t c = 0; c < channels; ++c) {
            host[c] = at;
            for (int64_t k = 0; k < K; ++k) at += counts_host[c * K + k];
        }
        host[channels] = at;
        // (from pageable host memory: the copy has left `staged` when the call returns)
        LAD_HIP_CHECK(hipMemcpyAsync(first_row, host, (size_t)(channels + 1) * 8, hipMemcpyHostToDevice, st));
    }
    const long long *prefix = (const long long *)((const char *)workspace + lay.prefix);
    const double *trees = (const double *)((const char *)workspace + lay.tree);
    with_track_type(dtype, [&](auto z) {
        using T = decltype(z);
        hipLaunchKernelGGL(span_rows_kernel<T>, dim3((unsigned)ceil_div(rows, THREADS)), dim3(THREADS), 0, st, (const T *)probs, frames, prefix,
                           trees, lay.tree_pitch, table, rows, (const int64_t *)first_row, channels, (long long *)sums, peaks, peak_values);
    });
    return check_launch("span_rows_kernel");
}
