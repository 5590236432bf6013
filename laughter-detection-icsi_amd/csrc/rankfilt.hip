// Rank filter (median, minimum, maximum, any order statistic) of a probability track over a sliding window of `window` frames.
//
// Not in the reference: its only smoother is lowpass (laugh_segmenter.py:49-55).  This is the non-linear one in front of the
// thresholds, for tracks that are already in GPU memory, several channels of different lengths at once.
//
// Semantics (include/lad_hip.h has them in full): with n the channel's own length and h = (window - 1) / 2,
//   out[c][i] = sort_ascending(probs[c][clamp(i - h + j, 0, n - 1)] for j in 0 .. window-1)[rank]   for 0 <= i < n
//   out[c][i] = NaN                                                                                 for n <= i < frames
// The result is one of the window's values, bit for bit: no arithmetic touches it.
//
// Shape: one workgroup per (channel, TILE output frames), one lane per output frame.  The tile and its 2 h halo are staged
// into LDS as order-preserving unsigned keys (IEEE bits with the sign-flip map: negative values inverted, the others with the
// top bit set), clamped to the channel's ends while staging, so the search itself never tests an index.  Every lane then finds
// its order statistic by a bitwise binary search on the key: from the top bit down it proposes prefix | bit, counts the
// window's keys below the proposal and keeps the bit iff that count is <= rank.  After the last bit the prefix is the largest
// key with at most `rank` keys below it, which is the rank-th smallest key of the window.  keybits passes of `window` LDS
// reads per frame (32 or 64 of them), whatever the data holds; consecutive lanes read consecutive LDS words (no bank
// conflicts, the window's reads of one wave are one row of the LDS each).  The NaN tail is filled by the same launch.
// One launch whatever the sizes, no workgroup waits for another, no atomics: two calls write identical bytes.  Every store is
// guarded by the row stride; the input is only read.
#include "lad_common.h"

namespace {
constexpr int TILE = 256;                    // output frames per workgroup = its threads
constexpr int MAX_WINDOW = 1023;
constexpr int64_t MAX_T = (int64_t)1 << 30;
constexpr int MAX_C = 65535;                 // grid.y

template <typename T>
struct Key;
template <>
struct Key<float> {
    using type = uint32_t;
    static constexpr int bits = 32;
    static __device__ inline type of(float v) {
        const type u = __float_as_uint(v);
        return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
    }
    static __device__ inline float back(type k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }
    static __device__ inline float nan() { return __uint_as_float(0x7fc00000u); }
};
template <>
struct Key<double> {
    using type = uint64_t;
    static constexpr int bits = 64;
    static __device__ inline type of(double v) {
        const type u = (type)__double_as_longlong(v);
        return u ^ ((u >> 63) ? ~(type)0 : (type)1 << 63);
    }
    static __device__ inline double back(type k) { return __longlong_as_double((long long)(k ^ ((k >> 63) ? (type)1 << 63 : ~(type)0))); }
    static __device__ inline double nan() { return __longlong_as_double(0x7ff8000000000000ll); }
};

struct Job {
    const void *probs;       // [channels][frames]
    const int64_t *lengths;  // device, or nullptr: every channel has `frames`
    void *out;               // [channels][frames]
    int64_t frames;
    int window, rank;
};

template <typename T>
__global__ __launch_bounds__(TILE) void rank_filter_kernel(Job job) {
    using K = Key<T>;
    using key_t = typename K::type;
    __shared__ key_t keys[TILE + MAX_WINDOW - 1];
    const int tid = threadIdx.x, c = blockIdx.y;
    const int64_t tile0 = (int64_t)blockIdx.x * TILE, i = tile0 + tid;
    const int64_t n = job.lengths ? job.lengths[c] : job.frames;
    T *dst = (T *)job.out + (int64_t)c * job.frames;
    if (tile0 >= n) {                                        // (the whole workgroup: nobody is left at a barrier)
        if (i < job.frames) dst[i] = K::nan();
        return;
    }
    const T *src = (const T *)job.probs + (int64_t)c * job.frames;
    const int h = (job.window - 1) / 2;
    // keys[s] = frame tile0 - h + s, clamped to the channel: s in [0, TILE + window - 1)
    for (int s = tid; s < TILE + job.window - 1; s += TILE) {
        int64_t f = tile0 - h + s;
        f = f < 0 ? 0 : (f > n - 1 ? n - 1 : f);
        keys[s] = K::of(src[f]);
    }
    __syncthreads();
    if (i >= n) {
        if (i < job.frames) dst[i] = K::nan();
        return;
    }
    const key_t *win = keys + tid;                           // the window of frame i: win[0 .. window)
    key_t prefix = 0;
    for (int b = K::bits - 1; b >= 0; --b) {
        const key_t cand = prefix | ((key_t)1 << b);
        int below = 0;
#pragma unroll 8
        for (int j = 0; j < job.window; ++j) below += win[j] < cand ? 1 : 0;
        if (below <= job.rank) prefix = cand;
    }
    dst[i] = K::back(prefix);
}

inline bool sizes_ok(int64_t C, int64_t T, int32_t window) {
    return C >= 1 && C <= MAX_C && T >= 1 && T <= MAX_T && window >= 1 && window <= MAX_WINDOW && (window & 1);
}
inline bool overlap(const void *p, int64_t pn, const void *q, int64_t qn) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + (uintptr_t)qn && b < a + (uintptr_t)pn;
}
}  // namespace

extern "C" int32_t lad_rank_filter_tile_frames(void) { return TILE; }
extern "C" int32_t lad_rank_filter_max_window(void) { return MAX_WINDOW; }

extern "C" int64_t lad_rank_filter_workspace_bytes(int64_t channels, int64_t frames, int32_t window) {
    if (!sizes_ok(channels, frames, window)) {
        lad::fail(LAD_ERR_INVALID, "lad_rank_filter_workspace_bytes: channels 1..%d, frames 1..2^30, window odd in 1..%d (got %lld, %lld, %d)",
                  MAX_C, MAX_WINDOW, (long long)channels, (long long)frames, window);
        return -1;
    }
    return lad::up256(channels * 8);         // the lengths on the device
}

extern "C" int lad_rank_filter(const void *probs, int32_t dtype, int64_t channels, int64_t frames, const int64_t *lengths_host,
                               int32_t window, int32_t rank, void *out, void *workspace, void *stream) {
    using namespace lad;
    LAD_REQUIRE(probs && out && workspace, "lad_rank_filter: null buffer");
    LAD_REQUIRE(dtype == LAD_RUNS_F32 || dtype == LAD_RUNS_F64, "lad_rank_filter: dtype %d (LAD_RUNS_F32 or LAD_RUNS_F64)", dtype);
    LAD_REQUIRE(sizes_ok(channels, frames, window),
                "lad_rank_filter: channels 1..%d, frames 1..2^30, window odd in 1..%d (got %lld, %lld, %d)", MAX_C, MAX_WINDOW,
                (long long)channels, (long long)frames, window);
    LAD_REQUIRE(rank >= 0 && rank < window, "lad_rank_filter: rank %d is outside 0..window - 1 = %d", rank, window - 1);
    if (lengths_host)
        for (int64_t c = 0; c < channels; ++c)
            LAD_REQUIRE(lengths_host[c] >= 1 && lengths_host[c] <= frames, "lad_rank_filter: lengths[%lld] = %lld is outside 1..frames = %lld",
                        (long long)c, (long long)lengths_host[c], (long long)frames);
    const int64_t bytes = channels * frames * (dtype == LAD_RUNS_F32 ? 4 : 8), ws_bytes = up256(channels * 8);
    LAD_REQUIRE(!overlap(out, bytes, probs, bytes), "lad_rank_filter: out overlaps probs");
    LAD_REQUIRE(!overlap(out, bytes, workspace, ws_bytes), "lad_rank_filter: out overlaps the workspace");
    LAD_REQUIRE(!overlap(probs, bytes, workspace, ws_bytes), "lad_rank_filter: probs overlaps the workspace");

    const hipStream_t st = (hipStream_t)stream;
    Job job;
    job.probs = probs;
    job.lengths = nullptr;
    job.out = out;
    job.frames = frames;
    job.window = window;
    job.rank = rank;
    if (lengths_host) {
        // (from pageable host memory: the copy has left lengths_host when the call returns)
        LAD_HIP_CHECK(hipMemcpyAsync(workspace, lengths_host, (size_t)channels * 8, hipMemcpyHostToDevice, st));
        job.lengths = (const int64_t *)workspace;
    }
    const dim3 grid((unsigned)ceil_div(frames, TILE), (unsigned)channels);
    if (dtype == LAD_RUNS_F32)
        hipLaunchKernelGGL(rank_filter_kernel<float>, grid, dim3(TILE), 0, st, job);
    else
        hipLaunchKernelGGL(rank_filter_kernel<double>, grid, dim3(TILE), 0, st, job);
    return check_launch("rank_filter_kernel");
}
