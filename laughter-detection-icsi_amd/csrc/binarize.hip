// Threshold sweep with hysteresis and gap filling: for K settings (onset, offset, min_gap) at once, the table of events
// (first_frame, last_frame) of a probability track.  The convention is written out in include/lad_hip.h; in short, with
// v the fixed probability in float64 (load_fixed), H = v > onset, L = v > offset (offset <= onset, so H is inside L):
//   hysteresis   active[i] = H[i] or (active[i - 1] and L[i]), active[-1] = 0: every maximal run of L that holds an H frame gives
//                one run, from its first H frame to the end of the L run
//   gap filling  consecutive hysteresis runs are joined iff not (next.first / fps - prev.last / fps > min_gap), float64
// offset == onset and min_gap == 0 is the plain sweep of runs.hip, bit for bit.
//
// A frame's state depends on an unbounded past, so a tile cannot decide alone.  It resolves itself for BOTH carry-ins instead:
//   binarize_tile_kernel  one wave owns a tile of 512 frames as 8 ballot words (lad_sweep_tile.h).  For a setting, a seed S inside
//                         L floods upwards through L's ones as the carry chain of the multi-word add X = L + S + carry-in: inside a
//                         run of ones the sum leaves the bits below the first seed alone, clears the first seed and carries out at
//                         the top, so active = ((X ^ L) | S) & L.  Stored per (channel, setting, tile): the number of run starts
//                         and the state of the tile's last frame, each for carry-in 0 and 1 -- one int32.  A tile inside a held
//                         region without an onset passes its carry-in through.
//   binarize_scan_kernel  one workgroup per (channel, setting): the tiles' maps carry-in -> (carry-out, starts) form a monoid under
//                         composition; its exclusive scan evaluated at active[-1] = 0 is each tile's carry-in and the rank of its
//                         first start, its total the number of hysteresis runs
//   binarize_rows_kernel  exclusive scan of the C * K run counts: each raw table's first row (and the total behind the last)
//   binarize_fill_kernel  the tile pass again with the resolved carry-in: starts and ends placed by rank (place_runs)
//                         into the raw table
//   binarize_heads_kernel / binarize_base_kernel / binarize_merge_kernel
//                         over the raw table: a row is a head unless it joins the row before it in the same (channel, setting);
//                         heads are counted per slice of a table, the slice counts scanned over all tables (which are back to
//                         back, so the scan IS the merged row of each slice's first head), then head i's first frame goes to column
//                         0 of its merged row and the last frame of the row before the next head to column 1.
// Seven launches whatever K and C are (three to count, four to fill).  No atomic anywhere: rows ascend by construction and two
// calls write the same bytes.  Every table store is guarded by the caller's capacity, every raw-table read too.  No scratch.
#pragma clang fp contract(off)
// The tile geometry, the limits, the fixed load, starts / ends and their placement by rank, and the scan are lad_sweep_tile.h's.
#include "lad_sweep_tile.h"

namespace {
using namespace lad::sweep;
constexpr int SLICES = 16;                  // workgroups that share one raw table in the run-level passes

struct Settings {
    double onset[MAX_K], offset[MAX_K];
};
struct Gaps {
    double v[MAX_K];
};

template <typename T>
struct TileRegs {
    double v[WORDS];
    double after;   // the frame behind the tile (every lane holds it: one address, one cache line)
    __device__ inline void load(const T *__restrict__ chan, int64_t tile0, int64_t n, int lane) {
        load_tile(chan, tile0, n, lane, v);
        after = load_fixed(chan, tile0 + TILE, n);
    }
    __device__ inline void masks(double onset, double offset, unsigned long long (&H)[WORDS], unsigned long long (&L)[WORDS]) const {
#pragma unroll
        for (int j = 0; j < WORDS; ++j) {
            L[j] = __ballot(v[j] > offset);
            H[j] = __ballot(v[j] > onset) & L[j];       // (inside L already for offset <= onset; the flood needs it)
        }
    }
};

// hysteresis inside the tile for carry-in cin (was the frame before the tile active?)
__device__ inline void resolve(const unsigned long long (&H)[WORDS], const unsigned long long (&L)[WORDS], unsigned cin,
                               unsigned long long (&A)[WORDS]) {
    unsigned long long c = cin & 1u;
#pragma unroll
    for (int j = 0; j < WORDS; ++j) {
        const unsigned long long x = L[j] + H[j];
        const unsigned long long c1 = x < H[j] ? 1ull : 0ull;
        const unsigned long long y = x + c;
        const unsigned long long c2 = y < x ? 1ull : 0ull;
        // a carry that arrives at a one of L floods on like a seed at bit 0; at a zero it stops there (the `& L` drops it)
        A[j] = ((y ^ L[j]) | H[j]) & L[j];
        c = c1 | c2;
    }
}

// what a tile is to the frames behind it: bits 0..9 starts for carry-in 0, 10..19 starts for carry-in 1 (at most 256 each),
// bit 20 / 21 the state of its last frame for carry-in 0 / 1
constexpr int PACK_N1 = 10, PACK_O = 20;

template <typename T>
__global__ __launch_bounds__(THREADS) void binarize_tile_kernel(const T *__restrict__ probs, int64_t n, int K, Settings set,
                                                                 int64_t n_tiles, uint32_t *__restrict__ tile_info) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t tile = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (tile >= n_tiles) return;                      // (whole waves leave: the ballots below see full waves)
    const int c = blockIdx.y;
    TileRegs<T> r;
    r.load(probs + (int64_t)c * n, tile * TILE, n, lane);
    uint32_t mine = 0;
    for (int k = 0; k < K; ++k) {
        unsigned long long H[WORDS], L[WORDS], A0[WORDS], A1[WORDS];
        r.masks(set.onset[k], set.offset[k], H, L);
        resolve(H, L, 0u, A0);
        resolve(H, L, 1u, A1);
        uint32_t n0 = 0, n1 = 0;
#pragma unroll
        for (int j = 0; j < WORDS; ++j) {
            n0 += (uint32_t)__popcll(starts_of(A0, j, 0ull));
            n1 += (uint32_t)__popcll(starts_of(A1, j, 1ull));
        }
        const uint32_t o = (uint32_t)(A0[WORDS - 1] >> 63) | ((uint32_t)(A1[WORDS - 1] >> 63) << 1);
        if (lane == k) mine = n0 | (n1 << PACK_N1) | (o << PACK_O);
    }
    if (lane < K) tile_info[((int64_t)c * K + lane) * n_tiles + tile] = mine;
}

// a stretch of tiles as a map of its carry-in x: o bit x = the state of its last frame, n[x] = the run starts inside it
struct Carry {
    int32_t n0, n1, o;
};
__device__ inline Carry carry_identity() { return Carry{0, 0, 2}; }
__device__ inline Carry compose(const Carry &a, const Carry &b) {   // a first, then b
    const int a0 = a.o & 1, a1 = (a.o >> 1) & 1;
    Carry r;
    r.n0 = a.n0 + (a0 ? b.n1 : b.n0);
    r.n1 = a.n1 + (a1 ? b.n1 : b.n0);
    r.o = ((b.o >> a0) & 1) | (((b.o >> a1) & 1) << 1);
    return r;
}
__device__ inline Carry shfl_up_carry(const Carry &x, int d) {
    return Carry{__shfl_up(x.n0, d, WAVE), __shfl_up(x.n1, d, WAVE), __shfl_up(x.o, d, WAVE)};
}

// in place: tile_info[g][tile] becomes (rank of the tile's first start << 1) | carry-in; counts[g] = hysteresis runs of g = c * K + k
__global__ __launch_bounds__(THREADS) void binarize_scan_kernel(uint32_t *__restrict__ tile_info, int64_t n_tiles,
                                                                 int32_t *__restrict__ counts) {
    __shared__ int32_t wave_total[WAVES][3];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    uint32_t *row = tile_info + (int64_t)blockIdx.x * n_tiles;
    Carry carry = carry_identity();
    for (int64_t base = 0; base < n_tiles; base += THREADS) {
        const int64_t i = base + threadIdx.x;
        Carry incl = carry_identity();
        if (i < n_tiles) {
            const uint32_t w = row[i];
            incl = Carry{(int32_t)(w & 1023u), (int32_t)((w >> PACK_N1) & 1023u), (int32_t)((w >> PACK_O) & 3u)};
        }
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) {
            const Carry y = shfl_up_carry(incl, d);
            if (lane >= d) incl = compose(y, incl);
        }
        if (lane == WAVE - 1) {
            wave_total[wave][0] = incl.n0;
            wave_total[wave][1] = incl.n1;
            wave_total[wave][2] = incl.o;
        }
        __syncthreads();
        Carry before = carry, all = carry_identity();
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            const Carry t = Carry{wave_total[w][0], wave_total[w][1], wave_total[w][2]};
            if (w < wave) before = compose(before, t);
            all = compose(all, t);
        }
        Carry excl = shfl_up_carry(incl, 1);
        if (lane == 0) excl = carry_identity();
        const Carry p = compose(before, excl);           // every tile before this one, as a map of active[-1]; active[-1] = 0
        if (i < n_tiles) row[i] = ((uint32_t)p.n0 << 1) | (uint32_t)(p.o & 1);
        carry = compose(carry, all);
        __syncthreads();
    }
    if (threadIdx.x == 0) counts[blockIdx.x] = carry.n0;
}

// first_row[g] = rows of the raw tables before table g, first_row[CK] = rows of all of them
__global__ __launch_bounds__(THREADS) void binarize_rows_kernel(const int32_t *__restrict__ counts, int64_t CK,
                                                                 int64_t *__restrict__ first_row) {
    const long long all =
        block_scan<long long>(0, CK, [&](int64_t i) { return counts[i]; }, [&](int64_t i, long long v) { first_row[i] = v; });
    if (threadIdx.x == 0) first_row[CK] = all;
}

// raw table: row (first_row[c * K + k] + rank) = (first_frame, last_frame) of the hysteresis run of that rank
template <typename T>
__global__ __launch_bounds__(THREADS) void binarize_fill_kernel(const T *__restrict__ probs, int64_t n, int K, Settings set,
                                                                 int64_t n_tiles, const uint32_t *__restrict__ tile_info,
                                                                 const int64_t *__restrict__ first_row, int64_t capacity,
                                                                 int32_t *__restrict__ raw) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t tile = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (tile >= n_tiles) return;
    const int c = blockIdx.y;
    const int64_t tile0 = tile * TILE;
    TileRegs<T> r;
    r.load(probs + (int64_t)c * n, tile0, n, lane);
    long long my_row = 0;                            // lane k: the row of the first run that starts in this tile, setting k
    unsigned my_cin = 0;
    if (lane < K) {
        const uint32_t w = tile_info[((int64_t)c * K + lane) * n_tiles + tile];
        my_row = first_row[(int64_t)c * K + lane] + (long long)(w >> 1);
        my_cin = w & 1u;
    }
    for (int k = 0; k < K; ++k) {
        unsigned long long H[WORDS], L[WORDS], A[WORDS];
        r.masks(set.onset[k], set.offset[k], H, L);
        const long long row = __shfl(my_row, k, WAVE);
        const unsigned cin = (unsigned)__shfl((int)my_cin, k, WAVE);
        resolve(H, L, cin, A);
        // the frame behind the tile matters only when the tile's last frame is active: it then goes on iff it is in L
        const unsigned long long behind = __ballot(r.after > set.offset[k]);
        place_runs(A, cin, behind, tile0, lane, row, capacity, raw);
    }
}

// rows [lo, hi) of raw table g that slice s of SLICES looks after, clamped to the caller's capacity
__device__ inline void slice_of(const int64_t *__restrict__ first_row, int64_t g, int s, int64_t capacity, int64_t &table_lo,
                                int64_t &table_hi, int64_t &lo, int64_t &hi) {
    int64_t a = first_row[g], b = first_row[g + 1];
    a = a < 0 ? 0 : (a > capacity ? capacity : a);
    b = b < a ? a : (b > capacity ? capacity : b);
    const int64_t per = (b - a + SLICES - 1) / SLICES;
    table_lo = a;
    table_hi = b;
    lo = a + (int64_t)s * per;
    hi = lo + per;
    lo = lo > b ? b : lo;
    hi = hi > b ? b : hi;
}

// row i of a raw table whose first row is table_lo: does it open a merged run?
__device__ inline bool is_head(const int32_t *__restrict__ raw, int64_t i, int64_t table_lo, double fps, double min_gap) {
    if (i == table_lo) return true;
    const double next_first = (double)raw[2 * i] / fps, prev_last = (double)raw[2 * i - 1] / fps;
    return next_first - prev_last > min_gap;
}

__device__ inline long long block_sum(long long x, long long *wave_sum) {   // the sum over the workgroup, in every thread
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) x += __shfl_xor(x, d, WAVE);
    __syncthreads();
    if (lane == 0) wave_sum[wave] = x;
    __syncthreads();
    long long all = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) all += wave_sum[w];
    return all;
}

// slice_heads[g * SLICES + s] = heads among the rows of slice s of raw table g
__global__ __launch_bounds__(THREADS) void binarize_heads_kernel(const int32_t *__restrict__ raw, const int64_t *__restrict__ first_row,
                                                                  int K, const double *__restrict__ fps, Gaps gaps, int64_t capacity,
                                                                  int32_t *__restrict__ slice_heads) {
    __shared__ long long wave_sum[WAVES];
    const int64_t g = blockIdx.x;
    const int s = blockIdx.y;
    int64_t table_lo, table_hi, lo, hi;
    slice_of(first_row, g, s, capacity, table_lo, table_hi, lo, hi);
    const double f = fps[g / K], gap = gaps.v[g % K];
    long long mine = 0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += THREADS) mine += is_head(raw, i, table_lo, f, gap) ? 1 : 0;
    const long long all = block_sum(mine, wave_sum);
    if (threadIdx.x == 0) slice_heads[g * SLICES + s] = (int32_t)all;
}

// slice_base[j] = heads before slice j over all tables = the merged row of slice j's first head; then the merged counts
__global__ __launch_bounds__(THREADS) void binarize_base_kernel(const int32_t *__restrict__ slice_heads, int64_t CK,
                                                                 int64_t *__restrict__ slice_base, int32_t *__restrict__ counts) {
    const long long all = block_scan<long long>(0, CK * SLICES, [&](int64_t i) { return slice_heads[i]; },
                                                [&](int64_t i, long long v) { slice_base[i] = v; });
    if (threadIdx.x == 0) slice_base[CK * SLICES] = all;
    __syncthreads();   // (one workgroup: its own stores are visible to it behind the barrier)
    for (int64_t g = threadIdx.x; g < CK; g += THREADS) counts[g] = (int32_t)(slice_base[(g + 1) * SLICES] - slice_base[g * SLICES]);
}

// merged table: head i opens merged row (heads before it); the row before the next head (or the table's last row) closes it
__global__ __launch_bounds__(THREADS) void binarize_merge_kernel(const int32_t *__restrict__ raw, const int64_t *__restrict__ first_row,
                                                                  int K, const double *__restrict__ fps, Gaps gaps, int64_t capacity,
                                                                  const int64_t *__restrict__ slice_base, int32_t *__restrict__ table) {
    __shared__ long long wave_sum[WAVES];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    const int64_t g = blockIdx.x;
    const int s = blockIdx.y;
    int64_t table_lo, table_hi, lo, hi;
    slice_of(first_row, g, s, capacity, table_lo, table_hi, lo, hi);
    const double f = fps[g / K], gap = gaps.v[g % K];
    long long rank = slice_base[g * SLICES + s];       // heads before the rows this workgroup has passed
    for (int64_t base = lo; base < hi; base += THREADS) {
        const int64_t i = base + threadIdx.x;
        const bool in = i < hi;
        const bool head = in && is_head(raw, i, table_lo, f, gap);
        const bool tail = in && (i + 1 >= table_hi || is_head(raw, i + 1, table_lo, f, gap));
        const unsigned long long hb = __ballot(head);
        const long long in_wave = __popcll(hb & ((1ull << lane) - 1ull));   // heads of this wave below this lane
        __syncthreads();
        if (lane == 0) wave_sum[wave] = __popcll(hb);
        __syncthreads();
        long long before = rank, all = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            if (w < wave) before += wave_sum[w];
            all += wave_sum[w];
        }
        const long long at = before + in_wave;          // heads before row i
        if (head && at >= 0 && at < capacity) table[2 * at] = raw[2 * i];
        if (tail) {
            const long long row = at + (head ? 1 : 0) - 1;   // (heads at rows <= i) - 1
            if (row >= 0 && row < capacity) table[2 * row + 1] = raw[2 * i + 1];
        }
        rank += all;
    }
}

struct Workspace {
    int64_t counts, first_row, slice_heads, slice_base, tile_info, bytes, n_tiles;
};
inline Workspace layout(int64_t C, int64_t T, int64_t K) {   // of sizes that check_sizes has passed
    using lad::up256;
    const int64_t ck = C * K;
    Workspace w;
    w.n_tiles = lad::ceil_div(T, TILE);
    w.counts = 0;
    w.first_row = up256(ck * 4);
    w.slice_heads = w.first_row + up256((ck + 1) * 8);
    w.slice_base = w.slice_heads + up256(ck * SLICES * 4);
    w.tile_info = w.slice_base + up256((ck * SLICES + 1) * 8);
    w.bytes = w.tile_info + up256(ck * w.n_tiles * 4);
    return w;
}
inline int settings_from(const char *who, const double *onsets, const double *offsets, int K, Settings &s) {
    for (int k = 0; k < MAX_K; ++k) {
        s.onset[k] = k < K ? onsets[k] : 0.0;
        s.offset[k] = k < K ? offsets[k] : 0.0;
        LAD_REQUIRE(std::isfinite(s.onset[k]) && std::isfinite(s.offset[k]), "%s: onset[%d] = %g, offset[%d] = %g: both must be finite",
                    who, k, s.onset[k], k, s.offset[k]);
        LAD_REQUIRE(s.offset[k] <= s.onset[k], "%s: offset[%d] = %.17g lies above onset[%d] = %.17g", who, k, s.offset[k], k, s.onset[k]);
    }
    return LAD_OK;
}
}  // namespace

extern "C" int32_t lad_binarize_max_settings(void) { return MAX_K; }

extern "C" int64_t lad_binarize_workspace_bytes(int64_t channels, int64_t frames, int32_t n_settings) {
    if (check_sizes("lad_binarize_workspace_bytes", "settings", channels, frames, n_settings)) return -1;
    return layout(channels, frames, n_settings).bytes;
}

extern "C" int lad_binarize_count(const void *probs, int32_t dtype, int64_t channels, int64_t frames, const double *onsets,
                                  const double *offsets, int32_t n_settings, void *workspace, void *stream) {
    using namespace lad;
    LAD_REQUIRE(probs && onsets && offsets && workspace, "lad_binarize_count: null buffer");
    if (int rc = check_dtype("lad_binarize_count", dtype)) return rc;
    if (int rc = check_sizes("lad_binarize_count", "settings", channels, frames, n_settings)) return rc;
    const Workspace w = layout(channels, frames, n_settings);
    Settings set;
    if (int rc = settings_from("lad_binarize_count", onsets, offsets, n_settings, set)) return rc;
    char *ws = (char *)workspace;
    int32_t *counts = (int32_t *)(ws + w.counts);
    uint32_t *tile_info = (uint32_t *)(ws + w.tile_info);
    int64_t *first_row = (int64_t *)(ws + w.first_row);
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)ceil_div(w.n_tiles, WAVES), (unsigned)channels);
    const int K = n_settings;
    with_track_type(dtype, [&](auto z) {
        using T = decltype(z);
        hipLaunchKernelGGL(binarize_tile_kernel<T>, grid, dim3(THREADS), 0, st, (const T *)probs, frames, K, set, w.n_tiles, tile_info);
    });
    if (int rc = check_launch("binarize_tile_kernel")) return rc;
    hipLaunchKernelGGL(binarize_scan_kernel, dim3((unsigned)(channels * K)), dim3(THREADS), 0, st, tile_info, w.n_tiles, counts);
    if (int rc = check_launch("binarize_scan_kernel")) return rc;
    hipLaunchKernelGGL(binarize_rows_kernel, dim3(1), dim3(THREADS), 0, st, (const int32_t *)counts, channels * K, first_row);
    return check_launch("binarize_rows_kernel");
}

extern "C" int lad_binarize_fill(const void *probs, int32_t dtype, int64_t channels, int64_t frames, const double *onsets,
                                 const double *offsets, const double *min_gaps, int32_t n_settings, const double *fps,
                                 const double *fps_host, void *workspace, const int32_t *counts_host, int32_t *raw_table,
                                 int32_t *table, int64_t capacity_runs, void *stream) {
    using namespace lad;
    LAD_REQUIRE(probs && onsets && offsets && min_gaps && fps && fps_host && workspace && counts_host, "lad_binarize_fill: null buffer");
    if (int rc = check_dtype("lad_binarize_fill", dtype)) return rc;
    if (int rc = check_sizes("lad_binarize_fill", "settings", channels, frames, n_settings)) return rc;
    const Workspace w = layout(channels, frames, n_settings);
    LAD_REQUIRE(capacity_runs >= 0, "lad_binarize_fill: negative capacity");
    Settings set;
    if (int rc = settings_from("lad_binarize_fill", onsets, offsets, n_settings, set)) return rc;
    Gaps gaps;
    for (int k = 0; k < MAX_K; ++k) {
        gaps.v[k] = k < n_settings ? min_gaps[k] : 0.0;
        LAD_REQUIRE(std::isfinite(gaps.v[k]) && gaps.v[k] >= 0.0, "lad_binarize_fill: min_gap[%d] = %g is not a finite number >= 0", k,
                    gaps.v[k]);
    }
    if (int rc = check_fps("lad_binarize_fill", fps_host, channels)) return rc;
    const int64_t total = total_runs("lad_binarize_fill", counts_host, channels * n_settings, frames);
    if (total < 0) return LAD_ERR_INVALID;
    LAD_REQUIRE(total <= capacity_runs, "lad_binarize_fill: the tables hold %lld runs, the buffers %lld (nothing was written)",
                (long long)total, (long long)capacity_runs);
    if (total == 0) return LAD_OK;                    // (the counts in the workspace are all zero already)
    LAD_REQUIRE(raw_table && table, "lad_binarize_fill: null table");
    LAD_REQUIRE(raw_table != table, "lad_binarize_fill: raw_table and table are the same buffer");
    char *ws = (char *)workspace;
    int32_t *counts = (int32_t *)(ws + w.counts), *slice_heads = (int32_t *)(ws + w.slice_heads);
    const uint32_t *tile_info = (const uint32_t *)(ws + w.tile_info);
    const int64_t *first_row = (const int64_t *)(ws + w.first_row);
    int64_t *slice_base = (int64_t *)(ws + w.slice_base);
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)ceil_div(w.n_tiles, WAVES), (unsigned)channels);
    const int K = n_settings;
    const int64_t CK = channels * K;
    with_track_type(dtype, [&](auto z) {
        using T = decltype(z);
        hipLaunchKernelGGL(binarize_fill_kernel<T>, grid, dim3(THREADS), 0, st, (const T *)probs, frames, K, set, w.n_tiles, tile_info,
                           first_row, capacity_runs, raw_table);
    });
    if (int rc = check_launch("binarize_fill_kernel")) return rc;
    const dim3 run_grid((unsigned)CK, SLICES);
    hipLaunchKernelGGL(binarize_heads_kernel, run_grid, dim3(THREADS), 0, st, (const int32_t *)raw_table, first_row, K, fps, gaps,
                       capacity_runs, slice_heads);
    if (int rc = check_launch("binarize_heads_kernel")) return rc;
    hipLaunchKernelGGL(binarize_base_kernel, dim3(1), dim3(THREADS), 0, st, (const int32_t *)slice_heads, CK, slice_base, counts);
    if (int rc = check_launch("binarize_base_kernel")) return rc;
    hipLaunchKernelGGL(binarize_merge_kernel, run_grid, dim3(THREADS), 0, st, (const int32_t *)raw_table, first_row, K, fps, gaps,
                       capacity_runs, (const int64_t *)slice_base, table);
    return check_launch("binarize_merge_kernel");
}
