// Two-state Viterbi decoding of a probability track: for K settings (bias, penalty) at once, the table of maximal on-runs
// (first_frame, last_frame) of the best on/off path.  The convention is written out in include/lad_hip.h (lad_viterbi_count); in
// short, with u the frame's bucket floor(v * 65536) of the fixed probability v and S the caller's emission table, the frame score
// is s = S[u] - bias (-2^31 at a NaN frame), a path scores the sum of s over its on frames minus `penalty` per run, and ties are
// decided as the header's recursion decides them.  int64 throughout: the path is a pure function of its inputs.
//
// The recursion (d0, d1) -> (max(d0, d1), max(d0 - P, d1) + s) is a max-plus product with the frame matrix [[0, 0], [s - P, s]],
// which is associative and exact on integers, so the values in front of any frame do not depend on how the product is bracketed:
//   viterbi_product_kernel   one wave owns a tile of 512 frames (lad_sweep_tile.h).  Lane = frame first: the wave loads the tile
//                            once, buckets it and leaves S[u] per frame in LDS (INT32_MIN at NaN).  Then lane = setting: lane k
//                            walks the tile's frames (every lane reads the same LDS word: a broadcast) and runs the recursion
//                            from both unit vectors, which gives the tile's 2x2 product for its (bias, penalty).
//   viterbi_forward_kernel   one workgroup per (channel, setting): exclusive scan of the tile products, applied to (0, -penalty):
//                            (d0, d1) in front of every tile, in place; the total gives the final state and `best`.
//   viterbi_backmap_kernel   the tile walk again from its exact (d0, d1): the psi bits of its frames, 64 per word, and the tile's
//                            backtrace as a map (state of its last frame -> state of the frame before the tile), composed on the way
//   viterbi_reverse_kernel   one workgroup per (channel, setting): exclusive scan of those maps from the last tile backwards,
//                            evaluated at the final state: the state of every tile's last frame
//   viterbi_resolve_kernel   lane = setting: backtrace through the stored psi words from that state: the tile's mask words and
//                            the number of runs that start in it
//   viterbi_ranks_kernel     exclusive scan of the starts over tiles per (channel, setting): the rank of each tile's first run,
//                            the total the run count
//   viterbi_rows_kernel      exclusive scan of the C * K run counts: each table's first row
//   viterbi_fill_kernel      lane = frame: the stored mask words of a tile ARE the ballot words place_runs takes
// Seven launches to count and one to fill, whatever K and C are.  No atomic, no float arithmetic behind the bucket, identical
// bytes on every call.  Every table store is guarded by the caller's capacity.
#include "lad_sweep_tile.h"

namespace {
using namespace lad::sweep;
constexpr int TABLE = 65537;                       // buckets 0..65536: lad_viterbi_table_entries()
constexpr int32_t MAX_EMISSION = 1 << 24;          // |S[u]|, |bias|
constexpr int32_t MAX_PENALTY = 1 << 26;
constexpr int32_t NAN_FRAME = INT32_MIN;           // in the staged scores: no table entry can be this
constexpr long long NAN_SCORE = -(1ll << 31);
constexpr int PSI_WORDS = 2 * WORDS;               // per (channel, setting, tile): psi0 words, then psi1 words

struct Settings {
    int32_t bias[MAX_K], penalty[MAX_K];
};

// S[u] of the tile's frames into this wave's LDS row (lane = frame), INT32_MIN at a NaN frame and beyond the track
template <typename T>
__device__ inline void stage_tile(const T *__restrict__ chan, int64_t tile0, int64_t n, int lane, const int32_t *__restrict__ emission,
                                  int32_t *__restrict__ staged) {
    double v[WORDS];
    load_tile(chan, tile0, n, lane, v);
#pragma unroll
    for (int j = 0; j < WORDS; ++j) {
        int32_t e = NAN_FRAME;
        if (v[j] == v[j]) {
            int u = (int)floor(v[j] * 65536.0);   // exact: v is in (0, 1]
            u = u < 0 ? 0 : (u > TABLE - 1 ? TABLE - 1 : u);
            e = emission[u];
        }
        staged[j * WAVE + lane] = e;
    }
}

__device__ inline long long score_of(int32_t e, int32_t bias) { return e == NAN_FRAME ? NAN_SCORE : (long long)e - (long long)bias; }

// one frame of the header's recursion; p0 / p1: psi0[t] / psi1[t]
__device__ inline void step(long long &d0, long long &d1, long long s, long long P, bool &p0, bool &p1) {
    const long long enter = d0 - P;
    p0 = d1 > d0;
    p1 = !(enter > d1);
    const long long n0 = p0 ? d1 : d0;
    const long long n1 = (p1 ? d1 : enter) + s;
    d0 = n0;
    d1 = n1;
}

// a stretch of frames as the max-plus matrix that takes (d0, d1) in front of it to (d0, d1) behind it
struct Mat {
    long long a00, a01, a10, a11;
    int id;                                        // the empty stretch (no finite matrix is the identity)
    __device__ static inline Mat identity() { return Mat{0, 0, 0, 0, 1}; }
    __device__ static inline Mat compose(const Mat &a, const Mat &b) {   // a first, then b
        if (a.id) return b;
        if (b.id) return a;
        Mat r;
        r.a00 = max(b.a00 + a.a00, b.a01 + a.a10);
        r.a01 = max(b.a00 + a.a01, b.a01 + a.a11);
        r.a10 = max(b.a10 + a.a00, b.a11 + a.a10);
        r.a11 = max(b.a10 + a.a01, b.a11 + a.a11);
        r.id = 0;
        return r;
    }
    __device__ static inline Mat shfl_up(const Mat &x, int d) {
        return Mat{__shfl_up(x.a00, d, WAVE), __shfl_up(x.a01, d, WAVE), __shfl_up(x.a10, d, WAVE), __shfl_up(x.a11, d, WAVE),
                   __shfl_up(x.id, d, WAVE)};
    }
};

// a stretch of frames as its backtrace: bit x = the state in front of it if the state of its last frame is x
struct Back {
    int o;
    __device__ static inline Back identity() { return Back{2}; }
    __device__ static inline Back compose(const Back &a, const Back &b) {   // a first, then b
        return Back{((b.o >> (a.o & 1)) & 1) | (((b.o >> ((a.o >> 1) & 1)) & 1) << 1)};
    }
    __device__ static inline Back shfl_up(const Back &x, int d) { return Back{__shfl_up(x.o, d, WAVE)}; }
};

// exclusive scan of load(i), i in [0, n), under E::compose by one workgroup of THREADS: store(i, load(0) then ... then load(i - 1));
// returns the total in every thread.  wave_total: WAVES elements of LDS.
template <typename E, typename Load, typename Store>
__device__ inline E scan_compose(int64_t n, E *wave_total, Load load, Store store) {
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    E carry = E::identity();
    for (int64_t base = 0; base < n; base += THREADS) {
        const int64_t i = base + threadIdx.x;
        E incl = i < n ? load(i) : E::identity();
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) {
            const E y = E::shfl_up(incl, d);
            if (lane >= d) incl = E::compose(y, incl);
        }
        if (lane == WAVE - 1) wave_total[wave] = incl;
        __syncthreads();
        E before = carry, all = E::identity();
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            const E t = wave_total[w];
            if (w < wave) before = E::compose(before, t);
            all = E::compose(all, t);
        }
        E excl = E::shfl_up(incl, 1);
        if (lane == 0) excl = E::identity();
        if (i < n) store(i, E::compose(before, excl));
        carry = E::compose(carry, all);
        __syncthreads();
    }
    return carry;
}

// what a tile kernel knows of its place: the tile, how many of its frames are inside the track, and whether the wave has one at all
struct Place {
    int64_t tile, tile0;
    int count;
    bool valid;
    __device__ inline Place(int64_t n, int64_t n_tiles) {
        tile = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
        valid = tile < n_tiles;
        tile0 = tile * TILE;
        const int64_t left = n - tile0;
        count = !valid ? 0 : (left < TILE ? (int)left : TILE);
    }
};

// rec[((c * K + k) * n_tiles + tile) * 4 ..] = the tile's product a00, a01, a10, a11
template <typename T>
__global__ __launch_bounds__(THREADS) void viterbi_product_kernel(const T *__restrict__ probs, int64_t n, int K, Settings set,
                                                                   const int32_t *__restrict__ emission, int64_t n_tiles,
                                                                   long long *__restrict__ rec) {
    __shared__ int32_t staged[WAVES][TILE];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    const Place at(n, n_tiles);
    const int c = blockIdx.y;
    if (at.valid) stage_tile(probs + (int64_t)c * n, at.tile0, n, lane, emission, staged[wave]);
    __syncthreads();
    if (!at.valid) return;
    // (lanes >= K walk too, with the zero setting, and only their stores are left out: a wave with eight or fewer lanes left took
    // three times as long in tools/experiments/viterbi_layouts.hip)
    const int32_t bias = set.bias[lane];
    const long long P = set.penalty[lane];
    // the columns of the product: the recursion from (0, -inf) and from (-inf, 0); behind the first frame both are finite
    const long long s0 = score_of(staged[wave][0], bias);
    long long a0 = 0, a1 = s0 - P, b0 = 0, b1 = s0;
    for (int i = 1; i < at.count; ++i) {
        const long long s = score_of(staged[wave][i], bias);
        bool p0, p1;
        step(a0, a1, s, P, p0, p1);
        step(b0, b1, s, P, p0, p1);
    }
    if (lane >= K) return;
    long long *out = rec + (((int64_t)c * K + lane) * n_tiles + at.tile) * 4;
    out[0] = a0;
    out[1] = b0;
    out[2] = a1;
    out[3] = b1;
}

// in place: rec[g][tile][0..1] becomes (d0, d1) in front of the tile; last_state[g], best[g] from the values behind the last frame
__global__ __launch_bounds__(THREADS) void viterbi_forward_kernel(long long *__restrict__ rec, int64_t n_tiles, int K, Settings set,
                                                                   int32_t *__restrict__ last_state, long long *__restrict__ best) {
    __shared__ Mat wave_total[WAVES];
    const int64_t g = blockIdx.x;
    long long *row = rec + g * n_tiles * 4;
    const long long P = set.penalty[g % K];
    const auto apply = [&](const Mat &m, long long &d0, long long &d1) {
        d0 = 0;
        d1 = -P;
        if (!m.id) {
            d0 = max(m.a00, m.a01 - P);
            d1 = max(m.a10, m.a11 - P);
        }
    };
    const Mat all = scan_compose<Mat>(
        n_tiles, wave_total, [&](int64_t i) { return Mat{row[4 * i], row[4 * i + 1], row[4 * i + 2], row[4 * i + 3], 0}; },
        [&](int64_t i, const Mat &m) {
            long long d0, d1;
            apply(m, d0, d1);
            row[4 * i] = d0;
            row[4 * i + 1] = d1;
        });
    if (threadIdx.x == 0) {
        long long d0, d1;
        apply(all, d0, d1);
        last_state[g] = d1 > d0 ? 1 : 0;
        if (best != nullptr) best[g] = max(d0, d1);
    }
}

// psi[(g * n_tiles + tile) * 16 ..]: psi0 of the tile's frames, 64 per word, then psi1; tile_back[g * n_tiles + tile]: its Back map
template <typename T>
__global__ __launch_bounds__(THREADS) void viterbi_backmap_kernel(const T *__restrict__ probs, int64_t n, int K, Settings set,
                                                                   const int32_t *__restrict__ emission, int64_t n_tiles,
                                                                   const long long *__restrict__ rec,
                                                                   unsigned long long *__restrict__ psi, int32_t *__restrict__ tile_back) {
    __shared__ int32_t staged[WAVES][TILE];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    const Place at(n, n_tiles);
    const int c = blockIdx.y;
    if (at.valid) stage_tile(probs + (int64_t)c * n, at.tile0, n, lane, emission, staged[wave]);
    __syncthreads();
    if (!at.valid) return;
    const bool mine = lane < K;                    // (the other lanes walk too and store nothing: see viterbi_product_kernel)
    const int32_t bias = set.bias[lane];
    const long long P = set.penalty[lane];
    const int64_t slot = ((int64_t)c * K + (mine ? lane : 0)) * n_tiles + at.tile;
    long long d0 = mine ? rec[slot * 4] : 0, d1 = mine ? rec[slot * 4 + 1] : 0;
    int g0 = 0, g1 = 1;                            // the state in front of the tile if the frame just walked is off / on
    unsigned long long *out = psi + slot * PSI_WORDS;
#pragma unroll
    for (int j = 0; j < WORDS; ++j) {
        unsigned long long w0 = 0, w1 = 0;
        const int stop = at.count - j * WAVE < WAVE ? at.count - j * WAVE : WAVE;
        for (int l = 0; l < stop; ++l) {
            bool p0, p1;
            step(d0, d1, score_of(staged[wave][j * WAVE + l], bias), P, p0, p1);
            w0 |= (unsigned long long)p0 << l;
            w1 |= (unsigned long long)p1 << l;
            const int n0 = p0 ? g1 : g0, n1 = p1 ? g1 : g0;
            g0 = n0;
            g1 = n1;
        }
        if (mine) {
            out[j] = w0;
            out[WORDS + j] = w1;
        }
    }
    if (mine) tile_back[slot] = g0 | (g1 << 1);
}

// in place: tile_back[g][tile] becomes the state of the tile's last frame
__global__ __launch_bounds__(THREADS) void viterbi_reverse_kernel(int32_t *__restrict__ tile_back, int64_t n_tiles,
                                                                   const int32_t *__restrict__ last_state) {
    __shared__ Back wave_total[WAVES];
    const int64_t g = blockIdx.x;
    int32_t *row = tile_back + g * n_tiles;
    const int last = last_state[g] & 1;
    // reversed order: element r is tile n_tiles - 1 - r; what lies in front of it in the scan are the tiles behind it in the track
    scan_compose<Back>(
        n_tiles, wave_total, [&](int64_t r) { return Back{row[n_tiles - 1 - r] & 3}; },
        [&](int64_t r, const Back &b) { row[n_tiles - 1 - r] = (b.o >> last) & 1; });
}

// mask[(g * n_tiles + tile) * 8 ..]: the tile's on/off words; tile_first[g * n_tiles + tile] = runs that start inside the tile
__global__ __launch_bounds__(THREADS) void viterbi_resolve_kernel(int64_t n, int K, int64_t n_tiles,
                                                                   const unsigned long long *__restrict__ psi,
                                                                   const int32_t *__restrict__ tile_back,
                                                                   unsigned long long *__restrict__ mask, int32_t *__restrict__ tile_first) {
    const int lane = threadIdx.x & (WAVE - 1);
    const Place at(n, n_tiles);
    const int c = blockIdx.y;
    if (!at.valid) return;
    const bool mine = lane < K;                    // (the other lanes walk too and store nothing: see viterbi_product_kernel)
    const int64_t slot = ((int64_t)c * K + (mine ? lane : 0)) * n_tiles + at.tile;
    const unsigned long long *in = psi + slot * PSI_WORDS;
    unsigned long long x = (unsigned long long)(tile_back[slot] & 1);
    unsigned long long m[WORDS];
#pragma unroll
    for (int j = WORDS - 1; j >= 0; --j) {
        const unsigned long long w0 = in[j], w1 = in[WORDS + j];
        unsigned long long w = 0;
        const int stop = at.count - j * WAVE < WAVE ? at.count - j * WAVE : WAVE;
        for (int l = stop - 1; l >= 0; --l) {
            w |= x << l;
            x = ((x ? w1 : w0) >> l) & 1ull;
        }
        m[j] = w;
    }
    const unsigned long long before = at.tile == 0 ? 0ull : x;   // frame 0's predecessor is not part of the path
    if (!mine) return;
    int starts = 0;
#pragma unroll
    for (int j = 0; j < WORDS; ++j) {
        starts += __popcll(starts_of(m, j, before));
        mask[slot * WORDS + j] = m[j];
    }
    tile_first[slot] = starts;
}

// in place: tile_first[g][tile] becomes the rank of the tile's first run; counts[g] = runs of g = c * K + k
__global__ __launch_bounds__(THREADS) void viterbi_ranks_kernel(int32_t *__restrict__ tile_first, int64_t n_tiles, int32_t *__restrict__ counts) {
    int32_t *row = tile_first + (int64_t)blockIdx.x * n_tiles;
    const int32_t all = block_scan<int32_t>(0, n_tiles, [&](int64_t i) { return row[i]; }, [&](int64_t i, int32_t v) { row[i] = v; });
    if (threadIdx.x == 0) counts[blockIdx.x] = all;
}

// first_row[g] = rows of the tables before table g
__global__ __launch_bounds__(THREADS) void viterbi_rows_kernel(const int32_t *__restrict__ counts, int64_t CK, int64_t *__restrict__ first_row) {
    block_scan<long long>(0, CK, [&](int64_t i) { return counts[i]; }, [&](int64_t i, long long v) { first_row[i] = v; });
}

// row (first_row[c * K + k] + rank) of the table = (first_frame, last_frame) of the run of that rank
__global__ __launch_bounds__(THREADS) void viterbi_fill_kernel(int64_t n, int K, int64_t n_tiles, const unsigned long long *__restrict__ mask,
                                                                const int32_t *__restrict__ tile_first,
                                                                const int64_t *__restrict__ first_row, int64_t capacity,
                                                                int32_t *__restrict__ table) {
    const int lane = threadIdx.x & (WAVE - 1);
    const Place at(n, n_tiles);
    if (!at.valid) return;
    const int c = blockIdx.y;
    long long my_row = 0;                            // lane k: the row of the first run that starts in this tile, setting k
    if (lane < K) my_row = first_row[(int64_t)c * K + lane] + tile_first[((int64_t)c * K + lane) * n_tiles + at.tile];
    for (int k = 0; k < K; ++k) {
        const unsigned long long *words = mask + (((int64_t)c * K + k) * n_tiles + at.tile) * WORDS;
        unsigned long long m[WORDS];
#pragma unroll
        for (int j = 0; j < WORDS; ++j) m[j] = words[j];
        const unsigned long long before = at.tile == 0 ? 0ull : words[-1] >> 63;
        const unsigned long long behind = at.tile + 1 >= n_tiles ? 0ull : words[WORDS] & 1ull;
        place_runs(m, before, behind, at.tile0, lane, __shfl(my_row, k, WAVE), capacity, table);
    }
}

struct Workspace {
    int64_t counts, first_row, last_state, tile_first, tile_back, rec, psi, mask, bytes, n_tiles;
};
inline Workspace layout(int64_t C, int64_t T, int64_t K) {   // of sizes that check_sizes has passed
    using lad::up256;
    const int64_t ck = C * K;
    Workspace w;
    w.n_tiles = lad::ceil_div(T, TILE);
    const int64_t slots = ck * w.n_tiles;
    w.counts = 0;
    w.first_row = up256(ck * 4);
    w.last_state = w.first_row + up256(ck * 8);
    w.tile_first = w.last_state + up256(ck * 4);
    w.tile_back = w.tile_first + up256(slots * 4);
    w.rec = w.tile_back + up256(slots * 4);
    w.psi = w.rec + up256(slots * 4 * 8);
    w.mask = w.psi + up256(slots * PSI_WORDS * 8);
    w.bytes = w.mask + up256(slots * WORDS * 8);
    return w;
}
inline int settings_from(const char *who, const int32_t *bias, const int32_t *penalty, int K, Settings &s) {
    for (int k = 0; k < MAX_K; ++k) {
        s.bias[k] = k < K ? bias[k] : 0;
        s.penalty[k] = k < K ? penalty[k] : 0;
        LAD_REQUIRE(s.bias[k] >= -MAX_EMISSION && s.bias[k] <= MAX_EMISSION, "%s: bias[%d] = %d lies outside +-2^24", who, k, s.bias[k]);
        LAD_REQUIRE(s.penalty[k] >= 0 && s.penalty[k] <= MAX_PENALTY, "%s: penalty[%d] = %d lies outside 0..2^26", who, k, s.penalty[k]);
    }
    return LAD_OK;
}
}  // namespace

extern "C" int32_t lad_viterbi_max_settings(void) { return MAX_K; }
extern "C" int32_t lad_viterbi_table_entries(void) { return TABLE; }

extern "C" int64_t lad_viterbi_workspace_bytes(int64_t channels, int64_t frames, int32_t n_settings) {
    if (check_sizes("lad_viterbi_workspace_bytes", "settings", channels, frames, n_settings)) return -1;
    return layout(channels, frames, n_settings).bytes;
}

extern "C" int lad_viterbi_count(const void *probs, int32_t dtype, int64_t channels, int64_t frames, const int32_t *emission,
                                 const int32_t *emission_host, const int32_t *bias, const int32_t *penalty, int32_t n_settings,
                                 void *workspace, int64_t *best, void *stream) {
    using namespace lad;
    LAD_REQUIRE(probs && emission && emission_host && bias && penalty && workspace, "lad_viterbi_count: null buffer");
    if (int rc = check_dtype("lad_viterbi_count", dtype)) return rc;
    if (int rc = check_sizes("lad_viterbi_count", "settings", channels, frames, n_settings)) return rc;
    Settings set;
    if (int rc = settings_from("lad_viterbi_count", bias, penalty, n_settings, set)) return rc;
    for (int u = 0; u < TABLE; ++u)
        LAD_REQUIRE(emission_host[u] >= -MAX_EMISSION && emission_host[u] <= MAX_EMISSION,
                    "lad_viterbi_count: emission_host[%d] = %d lies outside +-2^24", u, emission_host[u]);
    const Workspace w = layout(channels, frames, n_settings);
    char *ws = (char *)workspace;
    int32_t *counts = (int32_t *)(ws + w.counts), *last_state = (int32_t *)(ws + w.last_state);
    int32_t *tile_first = (int32_t *)(ws + w.tile_first), *tile_back = (int32_t *)(ws + w.tile_back);
    int64_t *first_row = (int64_t *)(ws + w.first_row);
    long long *rec = (long long *)(ws + w.rec);
    unsigned long long *psi = (unsigned long long *)(ws + w.psi), *mask = (unsigned long long *)(ws + w.mask);
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)ceil_div(w.n_tiles, WAVES), (unsigned)channels);
    const dim3 per_table((unsigned)(channels * n_settings));
    const int K = n_settings;
    with_track_type(dtype, [&](auto z) {
        using T = decltype(z);
        hipLaunchKernelGGL(viterbi_product_kernel<T>, grid, dim3(THREADS), 0, st, (const T *)probs, frames, K, set, emission, w.n_tiles, rec);
    });
    if (int rc = check_launch("viterbi_product_kernel")) return rc;
    hipLaunchKernelGGL(viterbi_forward_kernel, per_table, dim3(THREADS), 0, st, rec, w.n_tiles, K, set, last_state, (long long *)best);
    if (int rc = check_launch("viterbi_forward_kernel")) return rc;
    with_track_type(dtype, [&](auto z) {
        using T = decltype(z);
        hipLaunchKernelGGL(viterbi_backmap_kernel<T>, grid, dim3(THREADS), 0, st, (const T *)probs, frames, K, set, emission, w.n_tiles,
                           (const long long *)rec, psi, tile_back);
    });
    if (int rc = check_launch("viterbi_backmap_kernel")) return rc;
    hipLaunchKernelGGL(viterbi_reverse_kernel, per_table, dim3(THREADS), 0, st, tile_back, w.n_tiles, (const int32_t *)last_state);
    if (int rc = check_launch("viterbi_reverse_kernel")) return rc;
    hipLaunchKernelGGL(viterbi_resolve_kernel, grid, dim3(THREADS), 0, st, frames, K, w.n_tiles, (const unsigned long long *)psi,
                       (const int32_t *)tile_back, mask, tile_first);
    if (int rc = check_launch("viterbi_resolve_kernel")) return rc;
    hipLaunchKernelGGL(viterbi_ranks_kernel, per_table, dim3(THREADS), 0, st, tile_first, w.n_tiles, counts);
    if (int rc = check_launch("viterbi_ranks_kernel")) return rc;
    hipLaunchKernelGGL(viterbi_rows_kernel, dim3(1), dim3(THREADS), 0, st, (const int32_t *)counts, channels * K, first_row);
    return check_launch("viterbi_rows_kernel");
}

extern "C" int lad_viterbi_fill(const void *workspace, const int32_t *counts_host, int64_t channels, int64_t frames, int32_t n_settings,
                                int32_t *table, int64_t capacity_runs, void *stream) {
    using namespace lad;
    LAD_REQUIRE(workspace && counts_host, "lad_viterbi_fill: null buffer");
    if (int rc = check_sizes("lad_viterbi_fill", "settings", channels, frames, n_settings)) return rc;
    const Workspace w = layout(channels, frames, n_settings);
    LAD_REQUIRE(capacity_runs >= 0, "lad_viterbi_fill: negative capacity");
    const int64_t total = total_runs("lad_viterbi_fill", counts_host, channels * n_settings, frames);
    if (total < 0) return LAD_ERR_INVALID;
    LAD_REQUIRE(total <= capacity_runs, "lad_viterbi_fill: the tables hold %lld runs, the buffer %lld (nothing was written)",
                (long long)total, (long long)capacity_runs);
    if (total == 0) return LAD_OK;
    LAD_REQUIRE(table, "lad_viterbi_fill: null table");
    const char *ws = (const char *)workspace;
    const dim3 grid((unsigned)ceil_div(w.n_tiles, WAVES), (unsigned)channels);
    hipLaunchKernelGGL(viterbi_fill_kernel, grid, dim3(THREADS), 0, (hipStream_t)stream, frames, (int)n_settings, w.n_tiles,
                       (const unsigned long long *)(ws + w.mask), (const int32_t *)(ws + w.tile_first),
                       (const int64_t *)(ws + w.first_row), capacity_runs, table);
    return check_launch("viterbi_fill_kernel");
}
