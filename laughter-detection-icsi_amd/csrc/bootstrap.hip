// Bootstrap intervals of the sweep's figures: resample the recording units with replacement, sum the scorers' integers over every
// resample, and pick percentiles among the resulting exact fractions.
//
// Not in the reference, whose analysis/analyse.py writes point figures only.  The convention (the Philox counter of a draw, the sums'
// contract, the figure record, the order of two fractions, the rank of a quantile) is written out in include/lad_hip.h above
// lad_bootstrap_weights: that text is the specification, tests/_bootstrap_model.py a second implementation of it.
//
// Shape: one launch each, no global atomics, no workgroup waits for another, identical bytes on every call.
//   weights_kernel    (replicate): Philox4x32-10 on (draw >> 2, replicate, 0, tag), four draws a call; the counts in an LDS histogram
//                     by integer LDS atomics (additions commute: the order is free), then one coalesced row of stores.
//   sums_kernel       (512 columns, 32 replicates): a small integer GEMM.  A lane owns two columns and keeps 32 x 2 sums in registers;
//                     the rows of x stream through as coalesced 8-byte loads, four rows ahead of their use; the weights of the 32
//                     replicates lie in LDS as [unit][replicate] (64 units a stage, rows padded by 16 bytes) and are read as
//                     16-byte broadcasts, every lane the same address.  x < 2^40 is split into two 20-bit pieces and every piece
//                     has its own 32-bit sum, one v_mad_u32_u24 each: a weight row sums to at most 4096, so a sum of pieces stays
//                     below 4096 * 2^20 = 2^32, and sum = low + (high << 20) is exact.  Per row of x and lane: 2 loads, 8 LDS
//                     reads, 128 multiply-adds.
//   quantiles_kernel  (figure): the B fractions (num, den) into LDS with a permutation of the replicate numbers, padded to a power
//                     of two with invalid entries; a bitonic sort of the permutation by (valid first, exact value, replicate) -- a
//                     total order, so the network's result is the sorted sequence whatever its schedule; then one lane per quantile.
//                     20 bytes an entry: 80 KiB at 4096 replicates.
//   pair_quantiles_kernel (pair of figures): the same sort for the difference or the harmonic mean of two figures.  An entry is the
//                     four integers (n1, d1, n2, d2) and its place in the permutation, 36 bytes: 144 KiB at 4096 replicates; the
//                     value -- a sign and two integers below 2^109 -- is rebuilt inside every comparison, and two values are
//                     compared by their 256-bit cross products, built from 64-bit halves.
// Every read of x, weights and sums is guarded by the extents given, on the device too: values outside the contract give
// unspecified numbers, never an access outside the buffers.
#include "lad_common.h"
#include "lad_philox.h"

namespace {
constexpr int MAX_UNITS = 4096;                     // lad_bootstrap_max_units(): the LDS histogram
constexpr int MAX_REPLICATES = 4096;                // lad_bootstrap_max_replicates(): the sorting network in 80 KiB of LDS
constexpr int64_t MAX_COLUMNS = (int64_t)1 << 32;
constexpr int64_t MAX_FIGURES = (int64_t)1 << 30;
constexpr unsigned TAG = 0x424F4F54u;               // counter word 3 ("BOOT"): apart from the sampler's "SAMP" and the augmentation's small values

constexpr int W_THREADS = 256;

constexpr int S_THREADS = 256;
constexpr int TILE_B = 32;                          // replicates per workgroup
constexpr int COLS = 2;                             // columns per lane
constexpr int TILE_M = S_THREADS * COLS;            // columns per workgroup
constexpr int STAGE_G = 64;                         // units per LDS stage
constexpr int PITCH = TILE_B + 4;                   // an LDS row of weights: 16-byte aligned, 4 banks on from the row before
constexpr int AHEAD = 4;                            // rows of x in flight

constexpr int Q_THREADS = 512;
constexpr int MAX_Q = 16;
constexpr int ENTRY_BYTES = 8 + 8 + 4;

struct Quantiles {
    int32_t n;
    int32_t num[MAX_Q], den[MAX_Q];
};

__global__ __launch_bounds__(W_THREADS) void weights_kernel(int G, unsigned k0, unsigned k1, int32_t *__restrict__ weights) {
    __shared__ int hist[MAX_UNITS];
    const unsigned b = blockIdx.x;
    for (int g = threadIdx.x; g < G; g += W_THREADS) hist[g] = 0;
    __syncthreads();
    const int calls = (G + 3) >> 2;
    for (int c = threadIdx.x; c < calls; c += W_THREADS) {
        const lad::U4 r = lad::philox4x32_10(lad::U4{(unsigned)c, b, 0u, TAG}, k0, k1);
        const unsigned word[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (4 * c + j < G) atomicAdd(&hist[__umulhi(word[j], (unsigned)G)], 1);     // mulhi(word, G) < G
    }
    __syncthreads();
    for (int g = threadIdx.x; g < G; g += W_THREADS) weights[(int64_t)b * G + g] = hist[g];
}

__global__ __launch_bounds__(S_THREADS) void sums_kernel(const unsigned long long *__restrict__ x, const int32_t *__restrict__ weights, int G,
                                                         int64_t M, int B, long long *__restrict__ sums) {
    __shared__ __attribute__((aligned(16))) unsigned w_s[STAGE_G * PITCH];
    const int64_t m0 = (int64_t)blockIdx.x * TILE_M + threadIdx.x;
    const int b0 = blockIdx.y * TILE_B;
    unsigned lo[TILE_B][COLS], hi[TILE_B][COLS];
#pragma unroll
    for (int b = 0; b < TILE_B; ++b)
#pragma unroll
        for (int c = 0; c < COLS; ++c) lo[b][c] = hi[b][c] = 0;

    // rows g .. g + AHEAD - 1 of x, 0 beyond the matrix (their weights in LDS are 0 as well)
    auto load_rows = [&](int g, unsigned long long (&v)[AHEAD][COLS]) {
#pragma unroll
        for (int u = 0; u < AHEAD; ++u)
#pragma unroll
            for (int c = 0; c < COLS; ++c) {
                const int64_t m = m0 + (int64_t)c * S_THREADS;
                v[u][c] = (g + u < G && m < M) ? x[(int64_t)(g + u) * M + m] : 0ull;
            }
    };
    unsigned long long next[AHEAD][COLS];
    load_rows(0, next);
    for (int g0 = 0; g0 < G; g0 += STAGE_G) {
        __syncthreads();                                                           // (the stage before has been read)
        for (int e = threadIdx.x; e < TILE_B * STAGE_G; e += S_THREADS) {
            const int g = e % STAGE_G, b = e / STAGE_G;
            int32_t v = 0;
            if (g0 + g < G && b0 + b < B) v = weights[(int64_t)(b0 + b) * G + g0 + g];
            w_s[g * PITCH + b] = (unsigned)v;
        }
        __syncthreads();
        for (int g = 0; g < STAGE_G && g0 + g < G; g += AHEAD) {
            unsigned long long cur[AHEAD][COLS];
#pragma unroll
            for (int u = 0; u < AHEAD; ++u)
#pragma unroll
                for (int c = 0; c < COLS; ++c) cur[u][c] = next[u][c];
            load_rows(g0 + g + AHEAD, next);
#pragma unroll
            for (int u = 0; u < AHEAD; ++u) {
                unsigned xl[COLS], xh[COLS];
#pragma unroll
                for (int c = 0; c < COLS; ++c) {
                    xl[c] = (unsigned)cur[u][c] & 0xFFFFFu;
                    xh[c] = (unsigned)(cur[u][c] >> 20);                            // (__umul24 reads its low 24 bits: 20 within the contract)
                }
                const uint4 *row = reinterpret_cast<const uint4 *>(&w_s[(g + u) * PITCH]);
#pragma unroll
                for (int q = 0; q < TILE_B / 4; ++q) {
                    const uint4 w4 = row[q];                                        // every lane the same address: a broadcast
                    const unsigned w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int c = 0; c < COLS; ++c) {
                            lo[4 * q + j][c] += __umul24(w[j], xl[c]);
                            hi[4 * q + j][c] += __umul24(w[j], xh[c]);
                        }
                }
            }
        }
    }
#pragma unroll
    for (int b = 0; b < TILE_B; ++b)
#pragma unroll
        for (int c = 0; c < COLS; ++c) {
            const int64_t m = m0 + (int64_t)c * S_THREADS;
            if (b0 + b < B && m < M) sums[(int64_t)(b0 + b) * M + m] = (long long)((unsigned long long)lo[b][c] + ((unsigned long long)hi[b][c] << 20));
        }
}

// (num_i / den_i, i) before (num_j / den_j, j): valid entries (den != 0) first, by the exact value, equal values and the invalid
// ones by the replicate number
__device__ inline bool before(const unsigned long long *num, const unsigned long long *den, int i, int j) {
    const unsigned long long ni = num[i], di = den[i], nj = num[j], dj = den[j];
    if ((di != 0) != (dj != 0)) return di != 0;
    if (di != 0) {
        const unsigned long long l_hi = __umul64hi(ni, dj), l_lo = ni * dj, r_hi = __umul64hi(nj, di), r_lo = nj * di;
        if (l_hi != r_hi) return l_hi < r_hi;
        if (l_lo != r_lo) return l_lo < r_lo;
    }
    return i < j;
}

__global__ __launch_bounds__(Q_THREADS) void quantiles_kernel(const long long *__restrict__ sums, int64_t M, int B, int N,
                                                              const int32_t *__restrict__ figures, Quantiles q, long long *__restrict__ out,
                                                              int32_t *__restrict__ valid) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ int n_valid;
    unsigned long long *num = reinterpret_cast<unsigned long long *>(lds), *den = num + N;
    int *perm = reinterpret_cast<int *>(den + N);
    const int64_t f = blockIdx.x;
    const int32_t *fg = figures + 6 * f;
    const int num_col = fg[0], mult = fg[1], den_a = fg[2], den_b = fg[3], valid_col = fg[4], empty_is_one = fg[5];
    // (the host copy was checked; the device copy is what is read here)
    const bool ok = num_col >= 0 && num_col < M && den_a >= 0 && den_a < M && den_b >= -1 && den_b < M && valid_col >= -1 && valid_col < M;
    if (threadIdx.x == 0) n_valid = 0;
    __syncthreads();
    int mine = 0;
    for (int i = threadIdx.x; i < N; i += Q_THREADS) {
        unsigned long long n = 0, d = 0;
        if (i < B && ok) {
            const long long *row = sums + (int64_t)i * M;
            n = (unsigned long long)row[num_col] * (unsigned long long)mult;
            d = (unsigned long long)row[den_a] + (den_b >= 0 ? (unsigned long long)row[den_b] : 0ull);
            bool good = !(valid_col >= 0 && row[valid_col] == 0);
            if (d == 0) {
                if (empty_is_one) n = d = 1;
                else good = false;
            }
            if (good) ++mine;
            else n = d = 0;
        }
        num[i] = n;
        den[i] = d;
        perm[i] = i;
    }
    if (mine) atomicAdd(&n_valid, mine);
    for (int k = 2; k <= N; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int t = threadIdx.x; t < (N >> 1); t += Q_THREADS) {
                const int i = 2 * t - (t & (j - 1)), l = i + j;                     // the pairs (i, i ^ j) with bit j of i clear
                const int a = perm[i], b = perm[l];
                const bool ascending = (i & k) == 0;
                if (before(num, den, b, a) == ascending) {
                    perm[i] = b;
                    perm[l] = a;
                }
            }
        }
    __syncthreads();
    const int v = n_valid;
    if (threadIdx.x == 0) valid[f] = v;
    if ((int)threadIdx.x < q.n) {
        long long n = -1, d = -1;
        if (v > 0) {
            int64_t rank = ((int64_t)q.num[threadIdx.x] * v + q.den[threadIdx.x] - 1) / q.den[threadIdx.x] - 1;
            rank = rank < 0 ? 0 : (rank > v - 1 ? v - 1 : rank);
            const int p = perm[rank];
            n = (long long)num[p];
            d = (long long)den[p];
        }
        out[(f * q.n + threadIdx.x) * 2] = n;
        out[(f * q.n + threadIdx.x) * 2 + 1] = d;
    }
}

// ---- pairs of figures: the difference and the harmonic mean of two fractions, ordered exactly ------------------------------------
// A value is sign * n / d with n and d below 2^109, held as two 64-bit halves; nothing of it is stored: the four integers of an
// entry lie in LDS and the value is rebuilt inside every comparison.
struct U128 {
    unsigned long long lo, hi;
};
__device__ inline U128 mul64(unsigned long long a, unsigned long long b) { return U128{a * b, __umul64hi(a, b)}; }
__device__ inline U128 add128(U128 a, U128 b) {
    const unsigned long long lo = a.lo + b.lo;
    return U128{lo, a.hi + b.hi + (lo < a.lo ? 1ull : 0ull)};
}
__device__ inline U128 sub128(U128 a, U128 b) {                                    // a >= b
    return U128{a.lo - b.lo, a.hi - b.hi - (a.lo < b.lo ? 1ull : 0ull)};
}
__device__ inline bool less128(U128 a, U128 b) { return a.hi != b.hi ? a.hi < b.hi : a.lo < b.lo; }

struct PairValue {
    U128 n, d;      // |N| and D
    int sign;       // of N: -1, 0, 1
};
// op 0: n1 / d1 - n2 / d2 = (n1 d2 - n2 d1) / (d1 d2); op 1: 2 n1 n2 / (n1 d2 + n2 d1), 0 / 1 where that denominator is 0
__device__ inline PairValue pair_value(int op, unsigned long long n1, unsigned long long d1, unsigned long long n2, unsigned long long d2) {
    const U128 a = mul64(n1, d2), b = mul64(n2, d1);
    PairValue v;
    if (op == 0) {
        const bool neg = less128(a, b);
        v.n = neg ? sub128(b, a) : sub128(a, b);
        v.d = mul64(d1, d2);
        v.sign = neg ? -1 : ((v.n.lo | v.n.hi) != 0 ? 1 : 0);
    } else {
        const U128 p = mul64(n1, n2);
        v.n = U128{p.lo << 1, (p.hi << 1) | (p.lo >> 63)};
        v.d = add128(a, b);
        v.sign = (v.n.lo | v.n.hi) != 0 ? 1 : 0;
        if ((v.d.lo | v.d.hi) == 0) v.d.lo = 1;                                    // (both numerators are 0 then: the value 0 / 1)
    }
    return v;
}
// a * b < c * d, all four below 2^128 and both products below 2^256: four 64-bit words each, compared from the top
__device__ inline int cmp_products(U128 a, U128 b, U128 c, U128 d) {
    unsigned long long l[4], r[4];
    auto mul = [](U128 x, U128 y, unsigned long long (&w)[4]) {
        const U128 p00 = mul64(x.lo, y.lo), p01 = mul64(x.lo, y.hi), p10 = mul64(x.hi, y.lo), p11 = mul64(x.hi, y.hi);
        w[0] = p00.lo;
        unsigned long long t = p00.hi + p01.lo, carry = t < p01.lo ? 1ull : 0ull;
        w[1] = t + p10.lo;
        carry += w[1] < t ? 1ull : 0ull;
        t = p01.hi + p10.hi;
        unsigned long long carry2 = t < p10.hi ? 1ull : 0ull;
        unsigned long long u = t + p11.lo;
        carry2 += u < t ? 1ull : 0ull;
        w[2] = u + carry;
        carry2 += w[2] < u ? 1ull : 0ull;
        w[3] = p11.hi + carry2;
    };
    mul(a, b, l);
    mul(c, d, r);
#pragma unroll
    for (int k = 3; k >= 0; --k)
        if (l[k] != r[k]) return l[k] < r[k] ? -1 : 1;
    return 0;
}

// entry i before entry j: valid entries (d1 != 0) first, by the exact value N / D -- signs, then |N_i| D_j against |N_j| D_i as
// 256-bit products --, equal values and the invalid ones by the replicate number
__device__ inline bool pair_before(int op, const unsigned long long *e, int N, int i, int j) {
    const unsigned long long d1i = e[N + i], d1j = e[N + j];
    if ((d1i != 0) != (d1j != 0)) return d1i != 0;
    if (d1i != 0) {
        const PairValue vi = pair_value(op, e[i], d1i, e[2 * N + i], e[3 * N + i]);
        const PairValue vj = pair_value(op, e[j], d1j, e[2 * N + j], e[3 * N + j]);
        if (vi.sign != vj.sign) return vi.sign < vj.sign;
        if (vi.sign != 0) {
            const int c = cmp_products(vi.n, vj.d, vj.n, vi.d);
            if (c != 0) return (c < 0) == (vi.sign > 0);                           // (of two negative values the larger magnitude comes first)
        }
    }
    return i < j;
}

// (n, d) of a figure for one row of sums, after the substitution; false where the replicate is invalid for the figure
__device__ inline bool figure_of(const long long *row, const int32_t *fg, unsigned long long &n, unsigned long long &d) {
    const int den_b = fg[3], valid_col = fg[4];
    n = (unsigned long long)row[fg[0]] * (unsigned long long)fg[1];
    d = (unsigned long long)row[fg[2]] + (den_b >= 0 ? (unsigned long long)row[den_b] : 0ull);
    bool good = !(valid_col >= 0 && row[valid_col] == 0);
    if (d == 0) {
        if (fg[5]) n = d = 1;
        else good = false;
    }
    return good;
}
__device__ inline bool figure_in_range(const int32_t *fg, int64_t M) {
    return fg[0] >= 0 && fg[0] < M && fg[2] >= 0 && fg[2] < M && fg[3] >= -1 && fg[3] < M && fg[4] >= -1 && fg[4] < M;
}

constexpr int P_THREADS = 512;
constexpr int PAIR_WORDS = 13;
constexpr int PAIR_ENTRY_BYTES = 4 * 8 + 4;         // 144 KiB at 4096 replicates

__global__ __launch_bounds__(P_THREADS) void pair_quantiles_kernel(const long long *__restrict__ sums, int64_t M, int B, int N,
                                                                   const int32_t *__restrict__ pairs, Quantiles q, long long *__restrict__ out,
                                                                   int32_t *__restrict__ valid, int32_t *__restrict__ signs) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ int count[4];                                                       // valid, N < 0, N == 0, N > 0
    unsigned long long *e = reinterpret_cast<unsigned long long *>(lds);           // n1 [N], d1 [N], n2 [N], d2 [N]
    int *perm = reinterpret_cast<int *>(e + 4 * (int64_t)N);
    const int64_t f = blockIdx.x;
    const int32_t *pr = pairs + PAIR_WORDS * f;
    const int op = pr[0];
    // (the host copy was checked; the device copy is what is read here)
    const bool ok = (op == 0 || op == 1) && figure_in_range(pr + 1, M) && figure_in_range(pr + 7, M);
    if (threadIdx.x < 4) count[threadIdx.x] = 0;
    __syncthreads();
    int mine[4] = {0, 0, 0, 0};
    for (int i = threadIdx.x; i < N; i += P_THREADS) {
        unsigned long long n1 = 0, d1 = 0, n2 = 0, d2 = 0;
        if (i < B && ok) {
            const long long *row = sums + (int64_t)i * M;
            const bool good1 = figure_of(row, pr + 1, n1, d1), good2 = figure_of(row, pr + 7, n2, d2);
            if (good1 && good2) {
                ++mine[0];
                ++mine[2 + pair_value(op, n1, d1, n2, d2).sign];
            } else {
                n1 = d1 = n2 = d2 = 0;
            }
        }
        e[i] = n1;
        e[N + i] = d1;
        e[2 * N + i] = n2;
        e[3 * N + i] = d2;
        perm[i] = i;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (mine[k]) atomicAdd(&count[k], mine[k]);
    for (int k = 2; k <= N; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int t = threadIdx.x; t < (N >> 1); t += P_THREADS) {
                const int i = 2 * t - (t & (j - 1)), l = i + j;                     // the pairs (i, i ^ j) with bit j of i clear
                const int a = perm[i], b = perm[l];
                const bool ascending = (i & k) == 0;
                if (pair_before(op, e, N, b, a) == ascending) {
                    perm[i] = b;
                    perm[l] = a;
                }
            }
        }
    __syncthreads();
    const int v = count[0];
    if (threadIdx.x == 0) valid[f] = v;
    if (threadIdx.x < 3) signs[3 * f + threadIdx.x] = count[1 + threadIdx.x];
    if ((int)threadIdx.x < q.n) {
        long long r[4] = {-1, -1, -1, -1};
        if (v > 0) {
            int64_t rank = ((int64_t)q.num[threadIdx.x] * v + q.den[threadIdx.x] - 1) / q.den[threadIdx.x] - 1;
            rank = rank < 0 ? 0 : (rank > v - 1 ? v - 1 : rank);
            const int p = perm[rank];
#pragma unroll
            for (int k = 0; k < 4; ++k) r[k] = (long long)e[k * N + p];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) out[(f * q.n + threadIdx.x) * 4 + k] = r[k];
    }
}

inline bool overlap(const void *p, int64_t pn, const void *q, int64_t qn) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return pn > 0 && qn > 0 && a < b + (uintptr_t)qn && b < a + (uintptr_t)pn;
}
inline bool sizes_ok(int32_t units, int32_t replicates) {
    return units >= 1 && units <= MAX_UNITS && replicates >= 1 && replicates <= MAX_REPLICATES;
}
}  // namespace

extern "C" int64_t lad_bootstrap_max_units(void) { return MAX_UNITS; }
extern "C" int64_t lad_bootstrap_max_replicates(void) { return MAX_REPLICATES; }

extern "C" int lad_bootstrap_weights(int32_t units, int32_t replicates, uint64_t seed, int32_t *weights, void *stream) {
    using namespace lad;
    LAD_REQUIRE(sizes_ok(units, replicates), "lad_bootstrap_weights: units 1..%d, replicates 1..%d (got %d, %d)", MAX_UNITS, MAX_REPLICATES,
                units, replicates);
    LAD_REQUIRE(weights, "lad_bootstrap_weights: null buffer");
    hipLaunchKernelGGL(weights_kernel, dim3((unsigned)replicates), dim3(W_THREADS), 0, (hipStream_t)stream, (int)units,
                       (unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32), weights);
    return check_launch("bootstrap weights_kernel");
}

extern "C" int lad_bootstrap_sums(const int64_t *x, const int32_t *weights, int32_t units, int64_t columns, int32_t replicates, int64_t *sums,
                                  void *stream) {
    using namespace lad;
    LAD_REQUIRE(sizes_ok(units, replicates) && columns >= 0 && columns <= MAX_COLUMNS,
                "lad_bootstrap_sums: units 1..%d, replicates 1..%d, columns 0..2^32 (got %d, %d, %lld)", MAX_UNITS, MAX_REPLICATES, units,
                replicates, (long long)columns);
    LAD_REQUIRE(weights && (columns == 0 || (x && sums)), "lad_bootstrap_sums: null buffer");
    const int64_t out_bytes = (int64_t)replicates * columns * 8;
    LAD_REQUIRE(!overlap(sums, out_bytes, x, (int64_t)units * columns * 8), "lad_bootstrap_sums: sums overlaps x");
    LAD_REQUIRE(!overlap(sums, out_bytes, weights, (int64_t)replicates * units * 4), "lad_bootstrap_sums: sums overlaps the weights");
    if (columns == 0) return LAD_OK;
    const dim3 grid((unsigned)ceil_div(columns, TILE_M), (unsigned)ceil_div(replicates, TILE_B));
    hipLaunchKernelGGL(sums_kernel, grid, dim3(S_THREADS), 0, (hipStream_t)stream, (const unsigned long long *)x, weights, (int)units, columns,
                       (int)replicates, (long long *)sums);
    return check_launch("bootstrap sums_kernel");
}

extern "C" int lad_bootstrap_quantiles(const int64_t *sums, int64_t columns, int32_t replicates, const int32_t *figures,
                                       const int32_t *figures_host, int64_t n_figures, const int32_t *q_num, const int32_t *q_den,
                                       int32_t n_quantiles, int64_t *out, int32_t *valid, void *stream) {
    using namespace lad;
    LAD_REQUIRE(replicates >= 1 && replicates <= MAX_REPLICATES && columns >= 1 && columns <= MAX_COLUMNS && n_figures >= 0 &&
                    n_figures <= MAX_FIGURES && n_quantiles >= 1 && n_quantiles <= MAX_Q,
                "lad_bootstrap_quantiles: replicates 1..%d, columns 1..2^32, figures 0..2^30, quantiles 1..%d (got %d, %lld, %lld, %d)",
                MAX_REPLICATES, MAX_Q, replicates, (long long)columns, (long long)n_figures, n_quantiles);
    LAD_REQUIRE(sums && q_num && q_den && (n_figures == 0 || (figures && figures_host && out && valid)), "lad_bootstrap_quantiles: null buffer");
    Quantiles q;
    q.n = n_quantiles;
    for (int j = 0; j < MAX_Q; ++j) q.num[j] = q.den[j] = 1;
    for (int j = 0; j < n_quantiles; ++j) {
        LAD_REQUIRE(q_num[j] > 0 && q_num[j] < q_den[j], "lad_bootstrap_quantiles: quantile %d is %d / %d, expected 0 < q_num < q_den", j, q_num[j],
                    q_den[j]);
        q.num[j] = q_num[j];
        q.den[j] = q_den[j];
    }
    for (int64_t f = 0; f < n_figures; ++f) {
        const int32_t *fg = figures_host + 6 * f;
        LAD_REQUIRE(fg[0] >= 0 && fg[0] < columns && fg[2] >= 0 && fg[2] < columns && fg[3] >= -1 && fg[3] < columns && fg[4] >= -1 &&
                        fg[4] < columns,
                    "lad_bootstrap_quantiles: figure %lld names the columns (%d, %d, %d, %d) of %lld", (long long)f, fg[0], fg[2], fg[3], fg[4],
                    (long long)columns);
        LAD_REQUIRE((fg[1] == 1 || fg[1] == 2) && (fg[5] == 0 || fg[5] == 1),
                    "lad_bootstrap_quantiles: figure %lld has num_mult %d (1 or 2) and empty_is_one %d (0 or 1)", (long long)f, fg[1], fg[5]);
    }
    const int64_t sums_bytes = (int64_t)replicates * columns * 8, out_bytes = n_figures * n_quantiles * 16;
    LAD_REQUIRE(!overlap(out, out_bytes, sums, sums_bytes) && !overlap(valid, n_figures * 4, sums, sums_bytes),
                "lad_bootstrap_quantiles: an output overlaps the sums");
    LAD_REQUIRE(!overlap(out, out_bytes, figures, n_figures * 24) && !overlap(valid, n_figures * 4, figures, n_figures * 24),
                "lad_bootstrap_quantiles: an output overlaps the figures");
    LAD_REQUIRE(!overlap(out, out_bytes, valid, n_figures * 4), "lad_bootstrap_quantiles: out overlaps valid");
    if (n_figures == 0) return LAD_OK;
    int N = 1;
    while (N < replicates) N <<= 1;
    static DeviceOnce attr_set;   // (80 KiB of dynamic LDS at 4096 replicates: past the 64 KiB a kernel gets without opting in)
    if (!attr_set) {
        LAD_HIP_CHECK(hipFuncSetAttribute((const void *)quantiles_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, MAX_REPLICATES * ENTRY_BYTES));
        attr_set = true;
    }
    hipLaunchKernelGGL(quantiles_kernel, dim3((unsigned)n_figures), dim3(Q_THREADS), (size_t)N * ENTRY_BYTES, (hipStream_t)stream,
                       (const long long *)sums, columns, (int)replicates, N, figures, q, (long long *)out, valid);
    return check_launch("bootstrap quantiles_kernel");
}

extern "C" int lad_bootstrap_pair_quantiles(const int64_t *sums, int64_t columns, int32_t replicates, const int32_t *pairs,
                                            const int32_t *pairs_host, int64_t n_pairs, const int32_t *q_num, const int32_t *q_den,
                                            int32_t n_quantiles, int64_t *out, int32_t *valid, int32_t *signs, void *stream) {
    using namespace lad;
    LAD_REQUIRE(replicates >= 1 && replicates <= MAX_REPLICATES && columns >= 1 && columns <= MAX_COLUMNS && n_pairs >= 0 &&
                    n_pairs <= MAX_FIGURES && n_quantiles >= 1 && n_quantiles <= MAX_Q,
                "lad_bootstrap_pair_quantiles: replicates 1..%d, columns 1..2^32, pairs 0..2^30, quantiles 1..%d (got %d, %lld, %lld, %d)",
                MAX_REPLICATES, MAX_Q, replicates, (long long)columns, (long long)n_pairs, n_quantiles);
    LAD_REQUIRE(sums && q_num && q_den && (n_pairs == 0 || (pairs && pairs_host && out && valid && signs)),
                "lad_bootstrap_pair_quantiles: null buffer");
    Quantiles q;
    q.n = n_quantiles;
    for (int j = 0; j < MAX_Q; ++j) q.num[j] = q.den[j] = 1;
    for (int j = 0; j < n_quantiles; ++j) {
        LAD_REQUIRE(q_num[j] > 0 && q_num[j] < q_den[j], "lad_bootstrap_pair_quantiles: quantile %d is %d / %d, expected 0 < q_num < q_den", j,
                    q_num[j], q_den[j]);
        q.num[j] = q_num[j];
        q.den[j] = q_den[j];
    }
    for (int64_t p = 0; p < n_pairs; ++p) {
        const int32_t *pr = pairs_host + PAIR_WORDS * p;
        LAD_REQUIRE(pr[0] == 0 || pr[0] == 1, "lad_bootstrap_pair_quantiles: pair %lld has op %d (0: difference, 1: harmonic mean)", (long long)p,
                    pr[0]);
        for (int side = 0; side < 2; ++side) {
            const int32_t *fg = pr + 1 + 6 * side;
            LAD_REQUIRE(fg[0] >= 0 && fg[0] < columns && fg[2] >= 0 && fg[2] < columns && fg[3] >= -1 && fg[3] < columns && fg[4] >= -1 &&
                            fg[4] < columns,
                        "lad_bootstrap_pair_quantiles: figure %d of pair %lld names the columns (%d, %d, %d, %d) of %lld", side + 1, (long long)p,
                        fg[0], fg[2], fg[3], fg[4], (long long)columns);
            LAD_REQUIRE((fg[1] == 1 || fg[1] == 2) && (fg[5] == 0 || fg[5] == 1),
                        "lad_bootstrap_pair_quantiles: figure %d of pair %lld has num_mult %d (1 or 2) and empty_is_one %d (0 or 1)", side + 1,
                        (long long)p, fg[1], fg[5]);
        }
    }
    const int64_t sums_bytes = (int64_t)replicates * columns * 8, pairs_bytes = n_pairs * PAIR_WORDS * 4;
    const void *outs[3] = {out, valid, signs};
    const int64_t out_bytes[3] = {n_pairs * n_quantiles * 32, n_pairs * 4, n_pairs * 12};
    for (int a = 0; a < 3; ++a) {
        LAD_REQUIRE(!overlap(outs[a], out_bytes[a], sums, sums_bytes), "lad_bootstrap_pair_quantiles: an output overlaps the sums");
        LAD_REQUIRE(!overlap(outs[a], out_bytes[a], pairs, pairs_bytes), "lad_bootstrap_pair_quantiles: an output overlaps the pairs");
        for (int b = a + 1; b < 3; ++b)
            LAD_REQUIRE(!overlap(outs[a], out_bytes[a], outs[b], out_bytes[b]), "lad_bootstrap_pair_quantiles: two outputs overlap");
    }
    if (n_pairs == 0) return LAD_OK;
    int N = 1;
    while (N < replicates) N <<= 1;
    static DeviceOnce attr_set;   // (144 KiB of dynamic LDS at 4096 replicates, of the 160 KiB a workgroup may take)
    if (!attr_set) {
        LAD_HIP_CHECK(hipFuncSetAttribute((const void *)pair_quantiles_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                          MAX_REPLICATES * PAIR_ENTRY_BYTES));
        attr_set = true;
    }
    hipLaunchKernelGGL(pair_quantiles_kernel, dim3((unsigned)n_pairs), dim3(P_THREADS), (size_t)N * PAIR_ENTRY_BYTES, (hipStream_t)stream,
                       (const long long *)sums, columns, (int)replicates, N, pairs, q, (long long *)out, valid, signs);
    return check_launch("bootstrap pair_quantiles_kernel");
}
