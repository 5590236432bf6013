// Micro-benchmark behind csrc/viterbi.hip's thread layout: the max-plus product of a 512-frame tile for K settings, two ways.
//   hipcc -O3 --offload-arch=gfx950 -o viterbi_layouts viterbi_layouts.hip && ./viterbi_layouts
//   lane = setting   lane k walks the tile's 512 frames for its own (bias, penalty); the frame scores come from LDS as broadcasts
//                    (what the library does)
//   lane = frame     lane l owns frames 8 l .. 8 l + 7; for each setting in turn it multiplies its eight frame matrices and the
//                    wave reduces the 64 products in order with six shuffle-down steps of four int64 values
// Both read the same staged int32 scores and must write the same four int64 values per (setting, tile).  Prints one line per K
// with the median of 20 launches of each after a warm-up, by device events.  lane = setting is timed twice: with the lanes >= K
// leaving before the walk, and with every lane walking and only the stores guarded by K (what the library does: a wave with
// eight or fewer lanes left takes three times as long, at the same shader clock), with one wave's own cycle count beside it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

constexpr int WAVE = 64, TILE = 512, WAVES = 4, THREADS = WAVE * WAVES, MAX_K = 64;
struct Settings {
    int32_t bias[MAX_K], penalty[MAX_K];
};
#define CHECK(x)                                                                  \
    do {                                                                          \
        hipError_t e_ = (x);                                                      \
        if (e_ != hipSuccess) {                                                   \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));               \
            exit(1);                                                              \
        }                                                                         \
    } while (0)

__device__ inline void step(long long &d0, long long &d1, long long s, long long P) {
    const long long enter = d0 - P;
    const long long n0 = d1 > d0 ? d1 : d0;
    const long long n1 = (enter > d1 ? enter : d1) + s;
    d0 = n0;
    d1 = n1;
}

template <bool ALL>   // ALL: every lane walks (lanes >= K with a setting of their own too) and only the store is guarded by K
__global__ __launch_bounds__(THREADS) void lane_is_setting(const int32_t *__restrict__ e, int64_t n, int K, Settings set, int64_t n_tiles,
                                                           long long *__restrict__ rec, long long *__restrict__ ticks) {
    __shared__ int32_t staged[WAVES][TILE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long c0 = clock64(), w0 = wall_clock64();   // shader cycles, and the constant 100 MHz counter
    const int64_t tile = (int64_t)blockIdx.x * WAVES + wave;
    const bool valid = tile < n_tiles;
    const int64_t tile0 = tile * TILE;
    const int count = !valid ? 0 : (n - tile0 < TILE ? (int)(n - tile0) : TILE);
    for (int j = 0; j < TILE / WAVE; ++j) staged[wave][j * WAVE + lane] = j * WAVE + lane < count ? e[tile0 + j * WAVE + lane] : 0;
    __syncthreads();
    if (!valid || (!ALL && lane >= K)) return;
    const long long bias = set.bias[lane], P = set.penalty[lane];
    const long long s0 = staged[wave][0] - bias;
    long long a0 = 0, a1 = s0 - P, b0 = 0, b1 = s0;
    for (int i = 1; i < count; ++i) {
        const long long s = staged[wave][i] - bias;
        step(a0, a1, s, P);
        step(b0, b1, s, P);
    }
    if (lane < K) {
        long long *out = rec + ((int64_t)lane * n_tiles + tile) * 4;
        out[0] = a0, out[1] = b0, out[2] = a1, out[3] = b1;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ticks[0] = clock64() - c0;
        ticks[1] = wall_clock64() - w0;
    }
}

struct Mat {
    long long a00, a01, a10, a11;
};
__device__ inline long long mx(long long a, long long b) { return a > b ? a : b; }
__device__ inline Mat compose(const Mat &a, const Mat &b) {   // a first, then b
    return Mat{mx(b.a00 + a.a00, b.a01 + a.a10), mx(b.a00 + a.a01, b.a01 + a.a11), mx(b.a10 + a.a00, b.a11 + a.a10),
               mx(b.a10 + a.a01, b.a11 + a.a11)};
}

__global__ __launch_bounds__(THREADS) void lane_is_frame(const int32_t *__restrict__ e, int64_t n, int K, Settings set, int64_t n_tiles,
                                                         long long *__restrict__ rec) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t tile = (int64_t)blockIdx.x * WAVES + wave;
    if (tile >= n_tiles) return;
    const int64_t tile0 = tile * TILE;
    const int count = n - tile0 < TILE ? (int)(n - tile0) : TILE;
    int32_t mine[8];
    const int lanes = (count + 7) / 8;                      // lanes that own a frame
    const int own = lane * 8 >= count ? 0 : (count - lane * 8 < 8 ? count - lane * 8 : 8);
#pragma unroll
    for (int i = 0; i < 8; ++i) mine[i] = i < own ? e[tile0 + lane * 8 + i] : 0;
    for (int k = 0; k < K; ++k) {
        const long long bias = set.bias[k], P = set.penalty[k];
        const long long s0 = mine[0] - bias;
        long long a0 = 0, a1 = s0 - P, b0 = 0, b1 = s0;
#pragma unroll
        for (int i = 1; i < 8; ++i)
            if (i < own) {
                const long long s = mine[i] - bias;
                step(a0, a1, s, P);
                step(b0, b1, s, P);
            }
        Mat m{a0, b0, a1, b1};
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) {
            const Mat y{__shfl_down(m.a00, d, WAVE), __shfl_down(m.a01, d, WAVE), __shfl_down(m.a10, d, WAVE), __shfl_down(m.a11, d, WAVE)};
            if ((lane & (2 * d - 1)) == 0 && lane + d < lanes) m = compose(m, y);
        }
        if (lane == 0) {
            long long *out = rec + ((int64_t)k * n_tiles + tile) * 4;
            out[0] = m.a00, out[1] = m.a01, out[2] = m.a10, out[3] = m.a11;
        }
    }
}

int main() {
    const int64_t n = 360000, n_tiles = (n + TILE - 1) / TILE;
    std::vector<int32_t> e(n);
    uint32_t x = 12345;
    for (auto &v : e) {
        x = x * 1664525u + 1013904223u;
        v = (int32_t)(x >> 16) % 4000 - 2100;
    }
    Settings set;
    for (int k = 0; k < MAX_K; ++k) {
        set.bias[k] = 37 * k - 900;
        set.penalty[k] = 1024 * (k % 7);
    }
    int32_t *de;
    long long *ra, *rb, *ticks;
    CHECK(hipMalloc(&ticks, 2 * sizeof(long long)));
    const size_t bytes = (size_t)MAX_K * n_tiles * 4 * sizeof(long long);
    CHECK(hipMalloc(&de, n * sizeof(int32_t)));
    CHECK(hipMalloc(&ra, bytes));
    CHECK(hipMalloc(&rb, bytes));
    CHECK(hipMemcpy(de, e.data(), n * sizeof(int32_t), hipMemcpyHostToDevice));
    hipEvent_t t0, t1;
    CHECK(hipEventCreate(&t0));
    CHECK(hipEventCreate(&t1));
    const dim3 grid((unsigned)((n_tiles + WAVES - 1) / WAVES));
    std::vector<long long> ha(bytes / 8), hb(bytes / 8);
    for (int i = 0; i < 300; ++i)                           // (the clocks ramp up over the first few milliseconds of work)
        hipLaunchKernelGGL(lane_is_frame, grid, dim3(THREADS), 0, 0, de, n, MAX_K, set, n_tiles, rb);
    CHECK(hipDeviceSynchronize());
    for (int K : {1, 4, 8, 16, 23, 32, 64}) {
        double med[3];
        long long tk[3][2] = {};
        for (int which = 0; which < 3; ++which) {
            std::vector<float> ms;
            for (int i = 0; i < 23; ++i) {
                CHECK(hipEventRecord(t0));
                if (which == 0) hipLaunchKernelGGL(lane_is_setting<false>, grid, dim3(THREADS), 0, 0, de, n, K, set, n_tiles, ra, ticks);
                else if (which == 2) hipLaunchKernelGGL(lane_is_setting<true>, grid, dim3(THREADS), 0, 0, de, n, K, set, n_tiles, ra, ticks);
                else hipLaunchKernelGGL(lane_is_frame, grid, dim3(THREADS), 0, 0, de, n, K, set, n_tiles, rb);
                CHECK(hipEventRecord(t1));
                CHECK(hipEventSynchronize(t1));
                float t;
                CHECK(hipEventElapsedTime(&t, t0, t1));
                if (i >= 3) ms.push_back(t);
            }
            std::sort(ms.begin(), ms.end());
            med[which] = ms[ms.size() / 2];
            if (which != 1) CHECK(hipMemcpy(tk[which], ticks, sizeof(tk[which]), hipMemcpyDeviceToHost));
        }
        CHECK(hipMemcpy(ha.data(), ra, bytes, hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(hb.data(), rb, bytes, hipMemcpyDeviceToHost));
        const size_t used = (size_t)K * n_tiles * 4;
        const bool same = std::equal(ha.begin(), ha.begin() + used, hb.begin());
        printf("K=%2d  lane=setting %.4f ms (a wave: %lld shader cycles in %.1f us), all lanes walking %.4f ms (%lld cycles in %.1f us)  "
               "lane=frame %.4f ms  same=%d\n",
               K, med[0], tk[0][0], tk[0][1] / 100.0, med[2], tk[2][0], tk[2][1] / 100.0, med[1], (int)same);
        if (!same) return 1;
    }
    return 0;
}
