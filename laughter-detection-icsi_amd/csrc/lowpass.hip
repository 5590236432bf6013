// Zero-phase low-pass of a probability track: scipy.signal.filtfilt(b, a, x) with its defaults for one biquad, float64.
//
// Replaces lowpass (laugh_segmenter.py:49-55: a second-order Butterworth run forwards and backwards over the track before the
// thresholds, called from :170 and :195) for tracks that are already in GPU memory, several channels of different lengths at once.
//
// Semantics: the track is extended by an odd extension of PAD = 9 frames at both ends (ext[e] = 2 x[0] - x[9 - e],
// ext[T + 9 + j] = 2 x[T-1] - x[T-2-j]); forward pass in direct form II transposed
//   y = b0 x + z0;  z0 = b1 x + z1 - a1 y;  z1 = b2 x - a2 y
// from z = zi * ext[0]; the same recurrence over the reversed forward result from zi * (its first element); the middle T frames.
//
// Shape: the recurrence is serial, its state transition over m frames is the affine map z -> A^m z + c with
// A = [[-a1, 1], [-a2, 0]], and affine maps compose associatively.  A lane owns SEG = 64 consecutive frames of the extended
// track, a wave (one workgroup) a TILE of 64 * SEG of them, staged through LDS with coalesced loads (row stride SEG + 1 doubles:
// the lanes' stride-SEG reads fall on 64 different bank pairs).
//   local   every lane runs its segment from zero state; a wave scan with the host-computed powers A^(SEG 2^j) composes the 64
//           end states into the tile's own constant C (state at the tile's end from zero state at its start)
//   carry   one wave per channel walks the tiles 64 at a time with the powers A^(TILE 2^j), from zi * ext[0]: every tile's
//           true start state
//   apply   lane 0 starts from the tile's true state, the others from zero; the same scan now gives every lane's true start
//           state; each lane runs its segment again, writing y into its LDS row, and the tile is stored coalesced
// once forwards (into the workspace) and once over the reversed forward result (into `out`): six launches whatever the sizes.
// All arithmetic is float64 with explicit fused multiply-adds.  No workgroup waits for another, no atomics: two calls write
// identical bytes.  Every store is guarded by the channel's length and the row stride; the input is only read.
#include <cmath>

#include "lad_common.h"

namespace {
constexpr int WAVE = 64;
constexpr int SEG = 64;                      // frames one lane runs serially
constexpr int TILE = WAVE * SEG;             // frames per wave
constexpr int ROW = SEG + 1;                 // LDS row stride in doubles
constexpr int PAD = 9;                       // scipy's padlen = 3 * max(len(a), len(b))
constexpr int64_t MIN_T = PAD + 1;
constexpr int64_t MAX_T = (int64_t)1 << 30;
constexpr int MAX_C = 65535;                 // grid.y
constexpr int STEPS = 6;                     // log2(WAVE)

struct Filter {
    double b0, b1, b2, a1, a2, zi0, zi1;
    double seg[STEPS][4];                    // A^(SEG 2^j) as m00, m01, m10, m11
    double tile[STEPS][4];                   // A^(TILE 2^j)
};

struct State {
    double z0, z1;
};

__device__ inline double step(const Filter &f, State &s, double x) {
    const double y = fma(f.b0, x, s.z0);
    s.z0 = fma(-f.a1, y, fma(f.b1, x, s.z1));
    s.z1 = fma(-f.a2, y, f.b2 * x);
    return y;
}

__device__ inline State apply(const double (&m)[4], State u, State add) {
    return {fma(m[0], u.z0, fma(m[1], u.z1, add.z0)), fma(m[2], u.z0, fma(m[3], u.z1, add.z1))};
}

// in: lane l holds the map constant of its own span (state at its end from zero state at its start), pw[j] = A^(span 2^j).
// out: the constant of spans 0..l composed, i.e. the state at the end of span l from zero state at the start of span 0.
__device__ inline State wave_scan(State s, const double (&pw)[STEPS][4], int lane) {
#pragma unroll
    for (int j = 0; j < STEPS; ++j) {
        const int d = 1 << j;
        const State u = {__shfl_up(s.z0, d, WAVE), __shfl_up(s.z1, d, WAVE)};
        if (lane >= d) s = apply(pw[j], u, s);
    }
    return s;
}

// frame i of the extended track of one channel, i in [0, len + 2 PAD); zero beyond it
template <typename T>
struct Forward {
    const T *x;
    int64_t len;
    __device__ inline double operator()(int64_t i) const {
        if (i >= len + 2 * PAD) return 0.0;
        if (i < PAD) return 2.0 * (double)x[0] - (double)x[PAD - i];
        if (i < len + PAD) return (double)x[i - PAD];
        return 2.0 * (double)x[len - 1] - (double)x[2 * len + PAD - 2 - i];   // j = i - (len + PAD): x[len - 2 - j]
    }
};
// frame r of the reversed forward result
struct Backward {
    const double *y;
    int64_t len;
    __device__ inline double operator()(int64_t r) const {
        const int64_t ext = len + 2 * PAD;
        return r < ext ? y[ext - 1 - r] : 0.0;
    }
};

struct Job {
    const void *probs;       // [channels][frames]
    const int64_t *lengths;  // device, or nullptr: every channel has `frames`
    double *fwd;             // [channels][frames + 2 PAD]: the forward result over the extended track
    State *states;           // [channels][n_tiles]: the tiles' constants after `local`, their start states after `carry`
    double *out;             // [channels][frames]
    int64_t frames, n_tiles;
};

__device__ inline int64_t length_of(const Job &job, int c) {
    return job.lengths ? job.lengths[c] : job.frames;
}
template <typename Src>
__device__ inline Src source(const Job &job, int c, int64_t len);
template <>
__device__ inline Forward<float> source(const Job &job, int c, int64_t len) {
    return {(const float *)job.probs + (int64_t)c * job.frames, len};
}
template <>
__device__ inline Forward<double> source(const Job &job, int c, int64_t len) {
    return {(const double *)job.probs + (int64_t)c * job.frames, len};
}
template <>
__device__ inline Backward source(const Job &job, int c, int64_t len) {
    return {job.fwd + (int64_t)c * (job.frames + 2 * PAD), len};
}

template <typename Src>
__device__ inline void stage(double *lds, const Src &src, int64_t tile0, int lane) {
#pragma unroll 8
    for (int k = 0; k < SEG; ++k) lds[k * ROW + lane] = src(tile0 + k * WAVE + lane);   // frame k * 64 + lane: row k, column lane
    __syncthreads();
}

// the state at the end of the lane's segment from `s` at its start
__device__ inline State run(const Filter &f, const double *row, State s) {
#pragma unroll 8
    for (int j = 0; j < SEG; ++j) step(f, s, row[j]);
    return s;
}

template <typename Src>
__global__ __launch_bounds__(WAVE) void lowpass_local_kernel(Job job, Filter f) {
    __shared__ double lds[WAVE * ROW];
    const int lane = threadIdx.x, c = blockIdx.y;
    const int64_t tile = blockIdx.x, len = length_of(job, c);
    if (tile * TILE >= len + 2 * PAD) return;
    stage(lds, source<Src>(job, c, len), tile * TILE, lane);
    const State s = wave_scan(run(f, lds + lane * ROW, {0.0, 0.0}), f.seg, lane);
    if (lane == WAVE - 1) job.states[(int64_t)c * job.n_tiles + tile] = s;
}

// states[c][t]: the constant of tile t  ->  the state at the start of tile t
template <typename Src>
__global__ __launch_bounds__(WAVE) void lowpass_carry_kernel(Job job, Filter f) {
    const int lane = threadIdx.x, c = blockIdx.x;
    const int64_t len = length_of(job, c);
    const int64_t tiles = (len + 2 * PAD + TILE - 1) / TILE;
    State *st = job.states + (int64_t)c * job.n_tiles;
    const double first = source<Src>(job, c, len)(0);
    State carry = {f.zi0 * first, f.zi1 * first};
    for (int64_t base = 0; base < tiles; base += WAVE) {
        const int64_t t = base + lane;
        State s = t < tiles ? st[t] : State{0.0, 0.0};
        if (lane == 0) s = apply(f.tile[0], carry, s);            // the state at the end of tile `base`
        s = wave_scan(s, f.tile, lane);                           // ... at the end of tile base + lane
        State before = {__shfl_up(s.z0, 1, WAVE), __shfl_up(s.z1, 1, WAVE)};
        if (lane == 0) before = carry;
        if (t < tiles) st[t] = before;
        carry = {__shfl(s.z0, WAVE - 1, WAVE), __shfl(s.z1, WAVE - 1, WAVE)};
    }
}

// BACK = false: fwd[c][i] = forward result, i over the extended track.
// BACK = true:  out[c][t] = backward result at reversed frame r = len + PAD - 1 - t... t in [0, len), and NaN for t in [len, frames).
template <typename Src, bool BACK>
__global__ __launch_bounds__(WAVE) void lowpass_apply_kernel(Job job, Filter f) {
    __shared__ double lds[WAVE * ROW];
    const int lane = threadIdx.x, c = blockIdx.y;
    const int64_t tile = blockIdx.x, tile0 = tile * TILE, len = length_of(job, c), ext = len + 2 * PAD;
    if (BACK) {
        double *dst = job.out + (int64_t)c * job.frames;
        for (int k = 0; k < SEG; ++k) {
            const int64_t t = tile0 + k * WAVE + lane;
            if (t >= len && t < job.frames) dst[t] = __builtin_nan("");
        }
    }
    if (tile0 >= ext) return;
    stage(lds, source<Src>(job, c, len), tile0, lane);
    double *row = lds + lane * ROW;
    State s = {0.0, 0.0};
    if (lane == 0) s = job.states[(int64_t)c * job.n_tiles + tile];
    s = wave_scan(run(f, row, s), f.seg, lane);                    // the true state at the end of the lane's segment
    s = {__shfl_up(s.z0, 1, WAVE), __shfl_up(s.z1, 1, WAVE)};      // ... at its start
    if (lane == 0) s = job.states[(int64_t)c * job.n_tiles + tile];
#pragma unroll 8
    for (int j = 0; j < SEG; ++j) row[j] = step(f, s, row[j]);
    __syncthreads();
    for (int k = 0; k < SEG; ++k) {
        const int64_t i = tile0 + k * WAVE + lane;
        const double y = lds[k * ROW + lane];
        if (!BACK) {
            if (i < ext) job.fwd[(int64_t)c * (job.frames + 2 * PAD) + i] = y;
        } else {
            const int64_t t = len + PAD - 1 - i;                   // reversed frame i is extended frame ext - 1 - i
            if (t >= 0 && t < len) job.out[(int64_t)c * job.frames + t] = y;
        }
    }
}

struct Workspace {
    int64_t fwd, states, lengths, bytes, n_tiles;
};
inline bool layout(int64_t C, int64_t T, Workspace &w) {
    if (C < 1 || C > MAX_C || T < MIN_T || T > MAX_T) return false;
    const auto up = lad::up256;
    w.n_tiles = lad::ceil_div(T + 2 * PAD, TILE);
    w.fwd = 0;
    w.states = up(C * (T + 2 * PAD) * 8);
    w.lengths = w.states + up(C * w.n_tiles * (int64_t)sizeof(State));
    w.bytes = w.lengths + up(C * 8);
    return true;
}

// A^(SEG 2^j) and A^(TILE 2^j) = A^(SEG 2^(6 + j)) by multiplying with A one frame at a time, as the recurrence itself does:
// repeated squaring loses digits where the entries of A^n (about n r^n, r the pole radius) cancel -- at cutoff 0.001 the result
// is 9e-10 away from scipy with squared powers and 2e-11 with these (tests/_lowpass_model.py).  A power whose entries have all
// decayed below 1e-40 is taken as zero, and so are those after it.
inline void powers(double a1, double a2, Filter &f) {
    static_assert(TILE == SEG << STEPS, "the tile powers continue the segment powers");
    double m[4] = {1.0, 0.0, 0.0, 1.0};
    int64_t n = 0;
    for (int k = 0; k < 2 * STEPS; ++k) {
        for (const int64_t want = (int64_t)SEG << k; n < want; ++n) {
            const double r[4] = {-a1 * m[0] + m[2], -a1 * m[1] + m[3], -a2 * m[0], -a2 * m[1]};
            const bool gone = std::fabs(r[0]) < 1e-40 && std::fabs(r[1]) < 1e-40 && std::fabs(r[2]) < 1e-40 && std::fabs(r[3]) < 1e-40;
            for (int i = 0; i < 4; ++i) m[i] = gone ? 0.0 : r[i];
            if (gone) n = want - 1;
        }
        for (int i = 0; i < 4; ++i) (k < STEPS ? f.seg[k] : f.tile[k - STEPS])[i] = m[i];
    }
}
inline bool overlap(const void *p, int64_t pn, const void *q, int64_t qn) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + (uintptr_t)qn && b < a + (uintptr_t)pn;
}

template <typename Src>
int launch_pass(const Job &job, const Filter &f, int64_t channels, hipStream_t st, bool back) {
    const dim3 grid((unsigned)job.n_tiles, (unsigned)channels);
    hipLaunchKernelGGL(lowpass_local_kernel<Src>, grid, dim3(WAVE), 0, st, job, f);
    if (int rc = lad::check_launch("lowpass_local_kernel")) return rc;
    hipLaunchKernelGGL(lowpass_carry_kernel<Src>, dim3((unsigned)channels), dim3(WAVE), 0, st, job, f);
    if (int rc = lad::check_launch("lowpass_carry_kernel")) return rc;
    if (back)
        hipLaunchKernelGGL((lowpass_apply_kernel<Src, true>), grid, dim3(WAVE), 0, st, job, f);
    else
        hipLaunchKernelGGL((lowpass_apply_kernel<Src, false>), grid, dim3(WAVE), 0, st, job, f);
    return lad::check_launch("lowpass_apply_kernel");
}
}  // namespace

extern "C" int32_t lad_lowpass_tile_frames(void) { return SEG; }

extern "C" int64_t lad_lowpass_workspace_bytes(int64_t channels, int64_t frames) {
    Workspace w;
    if (!layout(channels, frames, w)) {
        lad::fail(LAD_ERR_INVALID, "lad_lowpass_workspace_bytes: channels 1..%d, frames %lld..2^30 (got %lld, %lld)", MAX_C,
                  (long long)MIN_T, (long long)channels, (long long)frames);
        return -1;
    }
    return w.bytes;
}

extern "C" int lad_lowpass(const void *probs, int32_t dtype, int64_t channels, int64_t frames, const int64_t *lengths_host,
                           const double *b_host, const double *a_host, const double *zi_host, double *out, void *workspace,
                           void *stream) {
    using namespace lad;
    Workspace w;
    LAD_REQUIRE(probs && b_host && a_host && zi_host && out && workspace, "lad_lowpass: null buffer");
    LAD_REQUIRE(dtype == LAD_RUNS_F32 || dtype == LAD_RUNS_F64, "lad_lowpass: dtype %d (LAD_RUNS_F32 or LAD_RUNS_F64)", dtype);
    LAD_REQUIRE(layout(channels, frames, w), "lad_lowpass: channels 1..%d, frames %lld..2^30 (got %lld, %lld)", MAX_C,
                (long long)MIN_T, (long long)channels, (long long)frames);
    if (lengths_host)
        for (int64_t c = 0; c < channels; ++c)
            LAD_REQUIRE(lengths_host[c] >= MIN_T && lengths_host[c] <= frames,
                        "lad_lowpass: lengths[%lld] = %lld is outside %lld..frames = %lld (the length of the input vector must be "
                        "greater than padlen = %d)", (long long)c, (long long)lengths_host[c], (long long)MIN_T, (long long)frames, PAD);
    for (int i = 0; i < 3; ++i)
        LAD_REQUIRE(std::isfinite(b_host[i]) && std::isfinite(a_host[i]), "lad_lowpass: non-finite coefficient");
    LAD_REQUIRE(std::isfinite(zi_host[0]) && std::isfinite(zi_host[1]), "lad_lowpass: non-finite zi");
    LAD_REQUIRE(a_host[0] == 1.0, "lad_lowpass: a[0] = %g, the coefficients must be normalised to a[0] = 1", a_host[0]);
    const int64_t in_bytes = channels * frames * (dtype == LAD_RUNS_F32 ? 4 : 8), out_bytes = channels * frames * 8;
    LAD_REQUIRE(!overlap(out, out_bytes, probs, in_bytes), "lad_lowpass: out overlaps probs");
    LAD_REQUIRE(!overlap(out, out_bytes, workspace, w.bytes), "lad_lowpass: out overlaps the workspace");
    LAD_REQUIRE(!overlap(probs, in_bytes, workspace, w.bytes), "lad_lowpass: probs overlaps the workspace");

    Filter f;
    f.b0 = b_host[0], f.b1 = b_host[1], f.b2 = b_host[2], f.a1 = a_host[1], f.a2 = a_host[2];
    f.zi0 = zi_host[0], f.zi1 = zi_host[1];
    powers(f.a1, f.a2, f);
    char *ws = (char *)workspace;
    const hipStream_t st = (hipStream_t)stream;
    Job job;
    job.probs = probs;
    job.lengths = nullptr;
    job.fwd = (double *)(ws + w.fwd);
    job.states = (State *)(ws + w.states);
    job.out = out;
    job.frames = frames;
    job.n_tiles = w.n_tiles;
    if (lengths_host) {
        // (from pageable host memory: the copy has left lengths_host when the call returns)
        LAD_HIP_CHECK(hipMemcpyAsync(ws + w.lengths, lengths_host, (size_t)channels * 8, hipMemcpyHostToDevice, st));
        job.lengths = (const int64_t *)(ws + w.lengths);
    }
    if (int rc = dtype == LAD_RUNS_F32 ? launch_pass<Forward<float>>(job, f, channels, st, false)
                                       : launch_pass<Forward<double>>(job, f, channels, st, false))
        return rc;
    return launch_pass<Backward>(job, f, channels, st, true);
}
