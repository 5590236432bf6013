// Rational sampling-rate conversion of one channel (polyphase FIR): y = resample(x, up / down), float32 out, float32 or
// int16 PCM in.  The step in front of the featuriser for audio that is not at 16 kHz, and the 44.1 kHz re-read of the
// reference's wav cuts (segment_laughter.py:134, librosa.load(sr=44100); laugh_segmenter.py:157-185, librosa.load(sr=8000)).
//
// Convention (scipy.signal.resample_poly with its defaults; the prototype h, 2 * half + 1 taps, is designed on the host):
//   y[n] = sum_j x[j] * h[half + n * down - j * up],   x zero-extended at both ends, n in [0, ceil(n_in * up / down)).
// With q = n * down = c * up + p (0 <= p < up) the taps of output n are row p of the table the caller passes (layout in
// include/lad_hip.h): y[n] = sum_{t < K} table[p][t] * x[c - L + t], L = (K - 1) / 2.
//
// Shape (resample_kernel, any ratio): a workgroup of 256 lanes stages the table once ([up][K] -> LDS rows of odd stride Ks, row p
// skewed by p / 32 floats: lanes of a wave walk the phases in steps of down mod up, and an even step would otherwise keep all of
// them on one bank), then loops over TILE-output tiles (tile = blockIdx.x, += gridDim.x).  Per tile it stages the input span
// [c0 - L, c_last - L + K) as float32 in LDS -- 16-byte global loads on an 8-sample grid, element loads with zeros outside
// [0, n_in) at the two ends of the signal, int16 scaled by 1 / 32768 here -- and each lane walks the K taps of 4 outputs
// (tile0 + lane + 256 k) side by side: two LDS reads per tap and output.  Single-phase ratios with enough taps (up == 1: 48 k,
// 32 k, 96 k -> 16 k) take resample_one_phase_kernel below: taps through wave-uniform loads, 4 consecutive outputs per lane.
//
// Order of summation: t = 0 .. K - 1, one fmaf each, zero taps and zero-extended samples included (they leave the sum as it is).  It
// depends on nothing but the output's phase, so a chunk [out_first, out_first + n_out) equals the same outputs of a whole call bit
// for bit, whatever the grid.  Indices: n, n * down and positions in x are int64; inside a tile everything is relative to the
// tile's first output (below 2^31 by the limits).  Plain stores, no atomics, no scratch.
#include "lad_common.h"

namespace {
constexpr int THREADS = 256;
constexpr int PER_LANE = 4;
constexpr int TILE = THREADS * PER_LANE;     // outputs per tile
constexpr int CHUNK = 8;                     // samples per staging step (16 bytes of int16, 32 of float32)
constexpr int MAX_UP = 1024;
constexpr int MAX_DOWN = 1024;
constexpr int MAX_K = 1024;
constexpr int64_t MAX_LDS = 64 * 1024;       // table + input span of one tile
constexpr int MAX_GRID = 512;                // 256 CUs x 2 workgroups at the largest table

struct Layout {
    bool blocked;      // single-phase kernel (up == 1, down >= 2, K >= 3 * down)
    int Ks;            // row stride of the table in LDS (odd)
    int tab_floats;    // table region (multiple of 4: the span behind it stays 16-byte aligned)
    int span_floats;   // input span of one tile, CHUNK-aligned start included
    int64_t bytes;
};

bool layout(int up, int down, int K, Layout &l) {
    if (up < 1 || down < 1 || K < 1 || up > MAX_UP || down > MAX_DOWN || K > MAX_K) return false;
    l.Ks = K | 1;
    l.blocked = up == 1 && down >= 2 && K >= (PER_LANE - 1) * down;
    const int64_t tab = l.blocked ? 0 : (int64_t)up * l.Ks + (up >> 5);
    l.tab_floats = (int)((tab + 3) & ~(int64_t)3);
    int64_t span = ((int64_t)(TILE - 1) * down) / up + 1 + K + (CHUNK - 1);
    if (l.blocked) span += span / (PER_LANE * down) + 1;      // one pad float per lane window
    l.span_floats = (int)((span + CHUNK - 1) & ~(int64_t)(CHUNK - 1));
    l.bytes = ((int64_t)l.tab_floats + l.span_floats) * 4;
    return l.bytes <= MAX_LDS;
}

__device__ inline float to_f32(float v) { return v; }
__device__ inline float to_f32(int16_t v) { return (float)v * (1.0f / 32768.0f); }

// 8 samples from g (g a multiple of 8, the whole chunk inside the signal, x 16-byte aligned)
__device__ inline void load_chunk(const float *__restrict__ x, int64_t g, float (&v)[CHUNK]) {
    const float4 a = *reinterpret_cast<const float4 *>(x + g), b = *reinterpret_cast<const float4 *>(x + g + 4);
    v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
}
__device__ inline void load_chunk(const int16_t *__restrict__ x, int64_t g, float (&v)[CHUNK]) {
    const uint4 a = *reinterpret_cast<const uint4 *>(x + g);
    const unsigned w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[2 * i] = to_f32((int16_t)(w[i] & 0xffffu));
        v[2 * i + 1] = to_f32((int16_t)(w[i] >> 16));
    }
}

template <typename T>
__global__ __launch_bounds__(THREADS) void resample_kernel(const T *__restrict__ x, int64_t n_in, const float *__restrict__ table,
                                                           int up, int down, int K, int Ks, int tab_floats, int64_t out_first,
                                                           int64_t n_out, int64_t n_tiles, int vec_ok, float *__restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *tab = reinterpret_cast<float *>(smem);
    float *xs = tab + tab_floats;
    const int tid = threadIdx.x;
    const int L = (K - 1) >> 1;

    // one wave per row: consecutive lanes copy consecutive taps
    for (int p = tid >> 6; p < up; p += THREADS / 64) {
        float *row = tab + p * Ks + (p >> 5);
        for (int t = tid & 63; t < K; t += 64) row[t] = table[(int64_t)p * K + t];
    }

    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t t0 = tile * TILE;                                   // relative to out_first
        const int cnt = (int)(n_out - t0 < TILE ? n_out - t0 : TILE);
        const int64_t q0 = (out_first + t0) * (int64_t)down;
        const int64_t c0 = q0 / up;
        const unsigned p0 = (unsigned)(q0 - c0 * up);
        const int span = (int)((p0 + (unsigned)(cnt - 1) * (unsigned)down) / (unsigned)up) + K;
        const int64_t first = c0 - L;
        const int64_t s0 = first & ~(int64_t)(CHUNK - 1);                 // floor, also below zero
        const int lead = (int)(first - s0);
        const int chunks = (lead + span + CHUNK - 1) / CHUNK;

        __syncthreads();                                                  // the tile before has been read (and the table written)
        for (int ch = tid; ch < chunks; ch += THREADS) {
            const int64_t g = s0 + (int64_t)ch * CHUNK;
            float v[CHUNK];
            if (vec_ok && g >= 0 && g + CHUNK <= n_in) {
                load_chunk(x, g, v);
            } else {
#pragma unroll
                for (int i = 0; i < CHUNK; ++i) v[i] = (g + i >= 0 && g + i < n_in) ? to_f32(x[g + i]) : 0.0f;
            }
            float4 *dst = reinterpret_cast<float4 *>(xs + ch * CHUNK);
            dst[0] = make_float4(v[0], v[1], v[2], v[3]);
            dst[1] = make_float4(v[4], v[5], v[6], v[7]);
        }
        __syncthreads();

        int xo[PER_LANE], ho[PER_LANE];
        float acc[PER_LANE];
#pragma unroll
        for (int k = 0; k < PER_LANE; ++k) {
            int i = tid + k * THREADS;
            i = i < cnt ? i : cnt - 1;                                    // idle lanes repeat the tile's last output, unstored
            const unsigned q = p0 + (unsigned)i * (unsigned)down;
            const unsigned c = q / (unsigned)up, p = q - c * (unsigned)up;
            xo[k] = lead + (int)c;
            ho[k] = (int)(p * Ks + (p >> 5));
            acc[k] = 0.0f;
        }
        for (int t = 0; t < K; ++t) {
#pragma unroll
            for (int k = 0; k < PER_LANE; ++k) acc[k] = fmaf(xs[xo[k] + t], tab[ho[k] + t], acc[k]);
        }
#pragma unroll
        for (int k = 0; k < PER_LANE; ++k) {
            const int i = tid + k * THREADS;
            if (i < cnt) y[t0 + i] = acc[k];
        }
    }
}

// Single-phase ratios (up == 1: 48 k, 32 k, 96 k -> 16 k): every output has the same taps, so they come through wave-uniform loads
// from the table in memory, and a lane takes PER_LANE CONSECUTIVE outputs: sample w of its window serves output r with tap
// w - r * down, i.e. one LDS read per (PER_LANE - 1) * down + K samples instead of one per tap and output.  Per output the taps
// still run t = 0 .. K - 1 with one fmaf each: the same sums as resample_kernel.  The staged span starts at the tile's first
// sample (position 0) and carries one pad float after every PER_LANE * down samples, so lane windows start an odd number of
// floats apart (no bank conflict between lanes) and sample w of a lane's window sits at lane * (PER_LANE * down + 1) + w +
// w / (PER_LANE * down), the last two terms wave-uniform.
template <typename T>
__global__ __launch_bounds__(THREADS) void resample_one_phase_kernel(const T *__restrict__ x, int64_t n_in, const float *__restrict__ table,
                                                                     int down, int K, int64_t out_first, int64_t n_out, int64_t n_tiles,
                                                                     int vec_ok, int y_vec_ok, float *__restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *xs = reinterpret_cast<float *>(smem);
    const int tid = threadIdx.x;
    const int L = (K - 1) >> 1;
    const int D = PER_LANE * down;                                        // samples between the windows of two lanes (>= 8)

    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t t0 = tile * TILE;
        const int cnt = (int)(n_out - t0 < TILE ? n_out - t0 : TILE);
        const int64_t first = (out_first + t0) * (int64_t)down - L;
        const int span = (cnt - 1) * down + K;
        const int64_t s0 = first & ~(int64_t)(CHUNK - 1);
        const int lead = (int)(first - s0);
        const int chunks = (lead + span + CHUNK - 1) / CHUNK;

        __syncthreads();
        for (int ch = tid; ch < chunks; ch += THREADS) {
            const int64_t g = s0 + (int64_t)ch * CHUNK;
            float v[CHUNK];
            if (vec_ok && g >= 0 && g + CHUNK <= n_in) {
                load_chunk(x, g, v);
            } else {
#pragma unroll
                for (int i = 0; i < CHUNK; ++i) v[i] = (g + i >= 0 && g + i < n_in) ? to_f32(x[g + i]) : 0.0f;
            }
            const int sb = ch * CHUNK - lead;                             // span position of v[0]; below zero in chunk 0 only
            const int qd = sb > 0 ? sb / D : 0, rem = sb - qd * D;
#pragma unroll
            for (int i = 0; i < CHUNK; ++i)
                if (sb + i >= 0) xs[sb + i + qd + (rem + i >= D ? 1 : 0)] = v[i];
        }
        __syncthreads();

        const float *xw = xs + tid * (D + 1);
        float acc[PER_LANE];
#pragma unroll
        for (int r = 0; r < PER_LANE; ++r) acc[r] = 0.0f;
        const int W0 = (PER_LANE - 1) * down;
        int o = 0, rem = 0;                                               // o = w + w / D
        for (int w = 0; w < W0; ++w) {                                    // head: the later outputs have not begun
            const float xv = xw[o];
#pragma unroll
            for (int r = 0; r < PER_LANE; ++r)
                if (w - r * down >= 0) acc[r] = fmaf(xv, table[w - r * down], acc[r]);
            ++o;
            if (++rem == D) rem = 0, ++o;
        }
#pragma unroll 4
        for (int w = W0; w < K; ++w) {                                    // body: every output takes the sample
            const float xv = xw[o];
#pragma unroll
            for (int r = 0; r < PER_LANE; ++r) acc[r] = fmaf(xv, table[w - r * down], acc[r]);
            ++o;
            if (++rem == D) rem = 0, ++o;
        }
        for (int w = K; w < K + W0; ++w) {                                // tail: the earlier outputs are complete
            const float xv = xw[o];
#pragma unroll
            for (int r = 0; r < PER_LANE; ++r)
                if (w - r * down < K) acc[r] = fmaf(xv, table[w - r * down], acc[r]);
            ++o;
            if (++rem == D) rem = 0, ++o;
        }
        const int i0 = tid * PER_LANE;
        if (y_vec_ok && i0 + PER_LANE <= cnt) {
            *reinterpret_cast<float4 *>(y + t0 + i0) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        } else {
#pragma unroll
            for (int r = 0; r < PER_LANE; ++r)
                if (i0 + r < cnt) y[t0 + i0 + r] = acc[r];
        }
    }
}

template <typename T>
int launch(const void *x, int64_t n_in, const float *table, int up, int down, int K, const Layout &l, int64_t out_first,
           int64_t n_out, float *y, hipStream_t st) {
    const int64_t n_tiles = lad::ceil_div(n_out, TILE);
    const dim3 grid((unsigned)(n_tiles < MAX_GRID ? n_tiles : MAX_GRID));
    const int vec_ok = ((uintptr_t)x & 15) == 0;
    if (l.blocked) {
        const int y_vec_ok = ((uintptr_t)y & 15) == 0;
        hipLaunchKernelGGL(resample_one_phase_kernel<T>, grid, dim3(THREADS), (size_t)l.bytes, st, (const T *)x, n_in, table, down, K,
                           out_first, n_out, n_tiles, vec_ok, y_vec_ok, y);
        return lad::check_launch("resample_one_phase_kernel");
    }
    hipLaunchKernelGGL(resample_kernel<T>, grid, dim3(THREADS), (size_t)l.bytes, st, (const T *)x, n_in, table, up, down, K, l.Ks,
                       l.tab_floats, out_first, n_out, n_tiles, vec_ok, y);
    return lad::check_launch("resample_kernel");
}
}  // namespace

extern "C" int32_t lad_resample_tile_outputs(void) { return TILE; }
extern "C" int32_t lad_resample_max_up(void) { return MAX_UP; }
extern "C" int32_t lad_resample_max_down(void) { return MAX_DOWN; }
extern "C" int32_t lad_resample_max_taps(void) { return MAX_K; }
extern "C" int64_t lad_resample_max_lds_bytes(void) { return MAX_LDS; }

extern "C" int64_t lad_resample_lds_bytes(int32_t up, int32_t down, int32_t K) {
    Layout l;
    if (up < 1 || down < 1 || K < 1 || up > MAX_UP || down > MAX_DOWN || K > MAX_K) {
        lad::fail(LAD_ERR_INVALID, "lad_resample_lds_bytes: up 1..%d, down 1..%d, K 1..%d (got %d, %d, %d)", MAX_UP, MAX_DOWN, MAX_K, up,
                  down, K);
        return -1;
    }
    layout(up, down, K, l);
    return l.bytes;
}

extern "C" int64_t lad_resample_out_len(int64_t n_in, int32_t up, int32_t down) {
    if (n_in < 0 || up < 1 || down < 1 || n_in > INT64_MAX / up - 1) {
        lad::fail(LAD_ERR_INVALID, "lad_resample_out_len: n_in >= 0, up, down >= 1, n_in * up below 2^63 (got %lld, %d, %d)",
                  (long long)n_in, up, down);
        return -1;
    }
    return (n_in * up + down - 1) / down;
}

extern "C" int lad_resample(const void *x, int32_t x_dtype, int64_t n_in, const float *table, int32_t up, int32_t down, int32_t K,
                            int64_t out_first, int64_t n_out, float *y, void *stream) {
    using namespace lad;
    LAD_REQUIRE(x_dtype == LAD_RESAMPLE_F32 || x_dtype == LAD_RESAMPLE_I16, "lad_resample: x_dtype %d is neither float32 nor int16",
                x_dtype);
    LAD_REQUIRE(up >= 1 && down >= 1 && K >= 1, "lad_resample: up, down, K must be >= 1 (got %d, %d, %d)", up, down, K);
    Layout l;
    LAD_REQUIRE(layout(up, down, K, l),
                "lad_resample: ratio %d/%d with %d taps per output is beyond the kernel's limits (up <= %d, down <= %d, K <= %d, table + "
                "tile span <= %lld bytes of LDS)",
                up, down, K, MAX_UP, MAX_DOWN, MAX_K, (long long)MAX_LDS);
    const int64_t total = lad_resample_out_len(n_in, up, down);
    LAD_REQUIRE(total >= 0, "lad_resample: n_in %lld out of range", (long long)n_in);
    LAD_REQUIRE(total <= INT64_MAX / down, "lad_resample: n_out * down overflows 64 bits");
    LAD_REQUIRE(out_first >= 0 && n_out >= 0 && out_first <= total && n_out <= total - out_first,
                "lad_resample: outputs [%lld, %lld + %lld) outside the %lld the signal has", (long long)out_first, (long long)out_first,
                (long long)n_out, (long long)total);
    if (n_out == 0) return LAD_OK;
    LAD_REQUIRE(x && table && y, "lad_resample: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (x_dtype == LAD_RESAMPLE_I16) return launch<int16_t>(x, n_in, table, up, down, K, l, out_first, n_out, y, st);
    return launch<float>(x, n_in, table, up, down, K, l, out_first, n_out, y, st);
}
