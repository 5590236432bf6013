// Calibration of the probability track against the transcript: the label histogram of a track (per bucket of the track's value, the
// milliseconds of every transcript class that the frames in the bucket own) and its inverse, a 65537-entry map applied to a track.
// Not in the reference, which never asks whether a frame at 0.9 is laughter nine times in ten.  The convention stands above
// lad_label_histogram in include/lad_hip.h; calibration.py derives every figure and every fit from the integers on the host.
//
// Frame i of channel c owns the milliseconds (m_i, m_{i+1}], m_j = rint((double)j / fps[c] * 1000): the expression of run_ms, IEEE
// division, contraction off, so that the host computes the same bits.  Its weight for class k is F_k(m_{i+1}) - F_k(m_i), F the
// coverage function of score.hip, its slot the bucket of lad_viterbi_count (NaN: slot 65537).
//
// Shape: two launches after one memset of the histogram (and one copy each of the lengths and the groups, where given).
//   label_scan_kernel       one workgroup per (channel, class): cum, the exclusive running length of the intervals (block_scan)
//   label_histogram_kernel  one workgroup per (channel, tile of TILE_FRAMES frames), FRAMES_PER_LANE frames per lane:
//     1. per frame one coverage_pairs<5> look-up for (m_i, m_{i+1}); the key (slot << 10 | place in the tile) and the five weights
//        go to LDS.  A place beyond the channel's length gets the slot behind the last one and five zeros.
//     2. a bitonic network sorts the TILE_FRAMES keys in LDS: equal slots become neighbours, and a key still names its frame.
//     3. per class an exclusive scan (block_scan) of the weights in sorted order.  A tile's weights of one class sum to at most
//        m_end - m_start < 2^31, so the sums are int32.
//     4. the last place of every run of equal slots finds the run's first place (a binary search for slot << 10 among the sorted
//        keys), takes the difference of the two prefix sums and adds it to hist[group][class][slot] with one vector atomic on
//        int64 -- where it is not zero.  So a workgroup issues at most one atomic per distinct (class, slot) it met: a constant
//        track costs five atomics a tile, not five a frame, and the adds of different tiles meet on five addresses, not on one.
//   Integer sums: whatever order the workgroups arrive in, the bytes are the same.
// Every index read is clamped to the index (coverage_pairs), every track read to the channel's length, every add to the histogram.
//
// lad_track_remap is one launch, one lane per frame: out = table[bucket], the table read through the cache (512 KiB: no LDS).
#pragma clang fp contract(off)
#include "lad_sweep_tile.h"

namespace {
using namespace lad::sweep;
constexpr int SLOTS = 65538;                        // lad_label_histogram_slots(): buckets 0..65536, then the NaN frames
constexpr int NAN_SLOT = 65537;
constexpr int NO_SLOT = 65538;                      // a place of the tile beyond the channel's length: sorts behind every real slot
constexpr int BUCKETS = 65537;                      // entries of a calibration table (lad_viterbi_table_entries())
constexpr int FRAMES_PER_LANE = 4;
constexpr int TILE_FRAMES = THREADS * FRAMES_PER_LANE;      // lad_label_histogram_tile_frames()
constexpr int PLACE_BITS = 10;
static_assert(TILE_FRAMES == 1 << PLACE_BITS, "a key is slot << PLACE_BITS | place");
static_assert(((int64_t)NO_SLOT << PLACE_BITS) + TILE_FRAMES < ((int64_t)1 << 31), "a key is a uint32");

// the bucket of lad_viterbi_count for a fixed value; NaN: the slot behind the buckets
__device__ inline int slot_of(double v) { return v != v ? NAN_SLOT : (int)floor(v * 65536.0); }

// m_j of channel c (run_ms' expression)
__device__ inline int32_t frame_ms(int64_t j, double fps) { return (int32_t)rint((double)j / fps * MS); }

__global__ __launch_bounds__(THREADS) void label_scan_kernel(const int32_t *__restrict__ bounds, const int32_t *__restrict__ offsets,
                                                             int64_t n_intervals, int32_t *__restrict__ cum, int64_t segments) {
    scan_index_and_counts(bounds, offsets, n_intervals, cum, segments, nullptr, 0, nullptr);      // (no workgroup `segments`: no counts)
}

template <typename T>
__global__ __launch_bounds__(THREADS) void label_histogram_kernel(const T *__restrict__ probs, int64_t frames,
                                                                  const int64_t *__restrict__ lengths, const int32_t *__restrict__ group,
                                                                  int n_groups, const double *__restrict__ fps,
                                                                  const int32_t *__restrict__ bounds, const int32_t *__restrict__ cum,
                                                                  const int32_t *__restrict__ offsets, int64_t n_intervals,
                                                                  unsigned long long *__restrict__ hist) {
    __shared__ uint32_t key[TILE_FRAMES];
    __shared__ int32_t weight[CLASSES][TILE_FRAMES];            // by place in the tile
    __shared__ int32_t before[CLASSES][TILE_FRAMES + 1];        // by sorted position: the weights of the positions in front of it
    const int64_t c = blockIdx.y;
    const int64_t g = group ? group[c] : c;
    int64_t n = lengths ? lengths[c] : frames;
    n = n < 0 ? 0 : (n > frames ? frames : n);
    const int64_t tile0 = (int64_t)blockIdx.x * TILE_FRAMES;
    if (g < 0 || g >= n_groups || tile0 >= n) return;           // (the same for every lane of the workgroup)
    const T *chan = probs + c * frames;
    const double f = fps[c];

    // 1. keys and weights
    for (int r = 0; r < FRAMES_PER_LANE; ++r) {
        const int place = r * THREADS + threadIdx.x;
        const int64_t i = tile0 + place;
        int slot = NO_SLOT;
        int32_t w[CLASSES] = {0, 0, 0, 0, 0};
        if (i < n) {
            slot = slot_of(load_fixed(chan, i, n));
            const int32_t x[2] = {frame_ms(i, f), frame_ms(i + 1, f)};
            int32_t F[2 * CLASSES], size[CLASSES];
            coverage_pairs<CLASSES>(c, x, bounds, cum, offsets, n_intervals, F, size);
#pragma unroll
            for (int k = 0; k < CLASSES; ++k) w[k] = F[2 * k + 1] - F[2 * k];
        }
        key[place] = ((uint32_t)slot << PLACE_BITS) | (uint32_t)place;
#pragma unroll
        for (int k = 0; k < CLASSES; ++k) weight[k][place] = w[k];
    }
    __syncthreads();

    // 2. the keys in ascending order (they are distinct: each holds its place)
    for (int size = 2; size <= TILE_FRAMES; size <<= 1) {
        for (int d = size >> 1; d > 0; d >>= 1) {
            for (int t = threadIdx.x; t < TILE_FRAMES / 2; t += THREADS) {
                const int lo = ((t & ~(d - 1)) << 1) | (t & (d - 1)), hi = lo | d;
                const bool ascending = (lo & size) == 0;
                const uint32_t a = key[lo], b = key[hi];
                if ((a > b) == ascending) {
                    key[lo] = b;
                    key[hi] = a;
                }
            }
            __syncthreads();
        }
    }

    // 3. per class the sums in front of every sorted position, and the tile's total behind the last
    for (int k = 0; k < CLASSES; ++k) {
        const int32_t all = block_scan<int32_t>(0, TILE_FRAMES, [&](int64_t p) { return weight[k][key[p] & (TILE_FRAMES - 1)]; },
                                                [&](int64_t p, int32_t v) { before[k][p] = v; });
        if (threadIdx.x == 0) before[k][TILE_FRAMES] = all;
    }
    __syncthreads();

    // 4. the last position of every run of one slot adds the run's sums
    for (int r = 0; r < FRAMES_PER_LANE; ++r) {
        const int p = r * THREADS + threadIdx.x;
        const uint32_t slot = key[p] >> PLACE_BITS;
        const bool last = p == TILE_FRAMES - 1 || (key[p + 1] >> PLACE_BITS) != slot;
        if (!last || slot >= (uint32_t)SLOTS) continue;
        int first = 0;                                          // the first position whose key is >= slot << PLACE_BITS
        for (int span = TILE_FRAMES; span > 0;) {
            const int half = span >> 1;
            if (key[first + half] < (slot << PLACE_BITS)) {
                first += half + 1;
                span -= half + 1;
            } else {
                span = half;
            }
        }
        unsigned long long *row = hist + (g * CLASSES) * SLOTS + slot;
#pragma unroll
        for (int k = 0; k < CLASSES; ++k) {
            const int32_t sum = before[k][p + 1] - before[k][first];
            if (sum != 0) atomicAdd(row + (int64_t)k * SLOTS, (unsigned long long)(long long)sum);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(THREADS) void track_remap_kernel(const T *__restrict__ probs, int64_t frames, const double *__restrict__ table,
                                                              double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= frames) return;
    const int64_t at = (int64_t)blockIdx.y * frames + i;
    const int slot = slot_of(load_fixed(probs, at, at + 1));
    out[at] = slot >= BUCKETS ? __builtin_nan("") : table[slot < 0 ? 0 : slot];
}

bool sizes_ok(int64_t channels, int64_t frames, int64_t n_intervals) {
    return channels >= 1 && channels <= MAX_C && frames >= 1 && frames <= MAX_T && n_intervals >= 0 && n_intervals <= MAX_INTERVALS;
}
bool overlap(const void *a, int64_t a_bytes, const void *b, int64_t b_bytes) {
    const char *x = (const char *)a, *y = (const char *)b;
    return x < y + b_bytes && y < x + a_bytes;
}

using lad::up256;
}  // namespace

extern "C" int32_t lad_label_histogram_slots(void) { return SLOTS; }
extern "C" int32_t lad_label_histogram_tile_frames(void) { return TILE_FRAMES; }

extern "C" int64_t lad_label_histogram_workspace_bytes(int64_t channels, int64_t frames, int64_t n_intervals) {
    if (!sizes_ok(channels, frames, n_intervals)) {
        lad::fail(LAD_ERR_INVALID, "lad_label_histogram_workspace_bytes: channels 1..%d, frames 1..2^30, intervals 0..2^30 (got %lld, %lld, %lld)",
                  MAX_C, (long long)channels, (long long)frames, (long long)n_intervals);
        return -1;
    }
    return up256(n_intervals * 4) + up256(channels * 8) + up256(channels * 4) + 256;      // cum, the lengths, the groups
}

extern "C" int lad_label_histogram(const void *probs, int32_t dtype, int64_t channels, int64_t frames, const int64_t *lengths_host,
                                   const int32_t *bounds, const int32_t *offsets, const int32_t *bounds_host, const int32_t *offsets_host,
                                   int64_t n_intervals, const double *fps, const double *fps_host, const int32_t *group_host,
                                   int32_t n_groups, void *workspace, int64_t *hist, void *stream) {
    using namespace lad;
    const char *who = "lad_label_histogram";
    LAD_REQUIRE(sizes_ok(channels, frames, n_intervals), "%s: channels 1..%d, frames 1..2^30, intervals 0..2^30 (got %lld, %lld, %lld)", who,
                MAX_C, (long long)channels, (long long)frames, (long long)n_intervals);
    LAD_REQUIRE(n_groups >= 1 && n_groups <= channels, "%s: n_groups %d is outside 1..channels = %lld", who, n_groups, (long long)channels);
    LAD_REQUIRE(group_host || n_groups == channels, "%s: without groups every channel is its own: n_groups %d must equal channels = %lld",
                who, n_groups, (long long)channels);
    if (int rc = check_dtype(who, dtype)) return rc;
    LAD_REQUIRE(probs && offsets && offsets_host && fps && fps_host && workspace && hist, "%s: null buffer", who);
    LAD_REQUIRE(n_intervals == 0 || (bounds && bounds_host), "%s: null interval bounds", who);
    if (int rc = check_fps(who, fps_host, channels)) return rc;
    for (int64_t c = 0; c < channels; ++c) {
        const int64_t n = lengths_host ? lengths_host[c] : frames;
        LAD_REQUIRE(n >= 1 && n <= frames, "%s: lengths[%lld] = %lld is outside 1..frames = %lld", who, (long long)c, (long long)n,
                    (long long)frames);
        const double ms = std::nearbyint((double)n / fps_host[c] * MS);               // m_n of the channel
        LAD_REQUIRE(ms < 2147483648.0, "%s: millisecond overflow: %lld frames at fps[%lld] = %g end at %.0f ms, int32 holds 2^31 - 1", who,
                    (long long)n, (long long)c, fps_host[c], ms);
        LAD_REQUIRE(!group_host || (group_host[c] >= -1 && group_host[c] < n_groups), "%s: group[%lld] = %d is outside -1..n_groups - 1 = %d",
                    who, (long long)c, group_host ? group_host[c] : 0, n_groups - 1);
    }
    if (int rc = check_index_intervals(who, channels, offsets_host, bounds_host, n_intervals)) return rc;
    const int64_t track_bytes = channels * frames * (dtype == LAD_RUNS_F32 ? 4 : 8), hist_bytes = (int64_t)n_groups * CLASSES * SLOTS * 8;
    const int64_t ws_bytes = lad_label_histogram_workspace_bytes(channels, frames, n_intervals);
    LAD_REQUIRE(!overlap(hist, hist_bytes, probs, track_bytes), "%s: hist overlaps probs", who);
    LAD_REQUIRE(!overlap(hist, hist_bytes, workspace, ws_bytes), "%s: hist overlaps the workspace", who);
    LAD_REQUIRE(!overlap(probs, track_bytes, workspace, ws_bytes), "%s: probs overlaps the workspace", who);

    int32_t *cum = (int32_t *)workspace;
    int64_t *lengths = (int64_t *)((char *)workspace + up256(n_intervals * 4));
    int32_t *group = (int32_t *)((char *)lengths + up256(channels * 8));
    const hipStream_t st = (hipStream_t)stream;
    LAD_HIP_CHECK(hipMemsetAsync(hist, 0, (size_t)hist_bytes, st));
    if (n_intervals == 0) return LAD_OK;          // five empty sets for every channel: nobody owns a millisecond
    // (from pageable host memory: the copies have left the host arrays when the call returns)
    if (lengths_host) LAD_HIP_CHECK(hipMemcpyAsync(lengths, lengths_host, (size_t)channels * 8, hipMemcpyHostToDevice, st));
    if (group_host) LAD_HIP_CHECK(hipMemcpyAsync(group, group_host, (size_t)channels * 4, hipMemcpyHostToDevice, st));
    const int64_t segments = channels * CLASSES;
    hipLaunchKernelGGL(label_scan_kernel, dim3((unsigned)segments), dim3(THREADS), 0, st, bounds, offsets, n_intervals, cum, segments);
    if (int rc = check_launch("label_scan_kernel")) return rc;
    const dim3 grid((unsigned)ceil_div(frames, TILE_FRAMES), (unsigned)channels);
    with_track_type(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(label_histogram_kernel<T>, grid, dim3(THREADS), 0, st, (const T *)probs, frames,
                           lengths_host ? (const int64_t *)lengths : nullptr, group_host ? (const int32_t *)group : nullptr, (int)n_groups, fps,
                           bounds, (const int32_t *)cum, offsets, n_intervals, (unsigned long long *)hist);
    });
    return check_launch("label_histogram_kernel");
}

extern "C" int lad_track_remap(const void *probs, int32_t dtype, int64_t channels, int64_t frames, const double *table, double *out,
                               void *stream) {
    using namespace lad;
    const char *who = "lad_track_remap";
    LAD_REQUIRE(sizes_ok(channels, frames, 0), "%s: channels 1..%d, frames 1..2^30 (got %lld, %lld)", who, MAX_C, (long long)channels,
                (long long)frames);
    if (int rc = check_dtype(who, dtype)) return rc;
    LAD_REQUIRE(probs && table && out, "%s: null buffer", who);
    const int64_t track_bytes = channels * frames * (dtype == LAD_RUNS_F32 ? 4 : 8), out_bytes = channels * frames * 8;
    LAD_REQUIRE(!overlap(out, out_bytes, probs, track_bytes), "%s: out overlaps probs", who);
    LAD_REQUIRE(!overlap(out, out_bytes, table, (int64_t)BUCKETS * 8), "%s: out overlaps the table", who);
    const dim3 grid((unsigned)ceil_div(frames, THREADS), (unsigned)channels);
    with_track_type(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(track_remap_kernel<T>, grid, dim3(THREADS), 0, (hipStream_t)stream, (const T *)probs, frames, table, out);
    });
    return check_launch("track_remap_kernel");
}
