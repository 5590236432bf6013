// Redrawing the segment table on the device: which frames of which channel form each training example, drawn afresh for every
// epoch, and the milliseconds of each transcript class under a list of windows.
//
// Replaces the sampling of the reference's create_data_df.py -- get_subsample :84-95 (a window inside a region),
// get_random_segment_from_df :65-81 (a row of a pool, then a window inside it), get_random_non_laughter_segment :32-63 (a
// window of the meeting that lies inside SILENCE / outside LAUGH and INVALID, found there by rejection) -- which the reference
// runs once, with numpy's global generator, when it writes {split}_df.csv; and the label rule of compute_features.py:228-243
// (a Python loop over windows and intervals).  The convention (frames and milliseconds, regions and pools, the three kinds of
// row, the Philox counter) is written out in include/lad_hip.h next to lad_sample_segments: that text is the specification.
//
// Shape: one launch each.
//   sample_kernel    one lane per row, grid-stride past a fixed grid: Philox4x32-10 on (row_id, epoch, tag), the rule of the
//                    row's kind, a binary search in pool_cum for a measure pool.  Three coalesced stores (four with `region`).
//   coverage_kernel  one lane per (window, set): a binary search for the first interval that ends past the hull's lower end, then
//                    the few intervals that start before its upper end.  No running sums are kept: a window meets a handful of
//                    intervals, and F(hi) - F(lo) of sweep_eval.coverage is the sum of those overlaps.
// Neither is near a roof: a 500,000-row table is 2 MB of descriptors in and 8 MB out.  Every region read is guarded by
// n_regions, every pool read by n_pools, every interval read by n_intervals; no LDS, no atomics (identical bytes on every call).
#include "lad_common.h"
#include "lad_philox.h"

namespace {
constexpr int THREADS = 256;
constexpr int MAX_GRID = 256;                       // one workgroup of 4 waves per CU: past 65,536 items the lanes stride
constexpr int64_t MAX_N = (int64_t)1 << 30;        // regions, pools, intervals
constexpr unsigned TAG = 0x53414D50u;               // counter word 3 ("SAMP"): apart from the augmentation's small block numbers

struct Region {
    int32_t chan, lo, hi;
};

__device__ inline Region load_region(const int32_t *__restrict__ regions, int64_t j) {
    return Region{regions[3 * j], regions[3 * j + 1], regions[3 * j + 2]};
}

__global__ __launch_bounds__(THREADS) void sample_kernel(const int32_t *__restrict__ kind, const int32_t *__restrict__ src, int64_t n_rows,
                                                         const int64_t *__restrict__ row_id, const int32_t *__restrict__ regions,
                                                         int64_t n_regions, const int32_t *__restrict__ pool_off,
                                                         const int64_t *__restrict__ pool_cum, int n_pools, int T, unsigned k0, unsigned k1,
                                                         unsigned epoch, int32_t *__restrict__ chan, int64_t *__restrict__ first,
                                                         int32_t *__restrict__ count, int32_t *__restrict__ region) {
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n_rows; i += (int64_t)gridDim.x * THREADS) {
        const unsigned long long id = (unsigned long long)(row_id ? row_id[i] : i);
        const lad::U4 r = lad::philox4x32_10(lad::U4{(unsigned)id, (unsigned)(id >> 32), epoch, TAG}, k0, k1);
        const int kd = kind[i];
        const int64_t s = src[i];
        int64_t j = -1;           // the region the window is drawn from
        int64_t at = -1;          // POOL_MEASURE: the window's offset inside it
        if (kd == LAD_SAMPLE_FIXED) {
            j = s;
        } else if ((kd == LAD_SAMPLE_POOL_ROW || kd == LAD_SAMPLE_POOL_MEASURE) && s >= 0 && s < n_pools) {
            int64_t o0 = pool_off[s], o1 = pool_off[s + 1];
            o0 = o0 < 0 ? 0 : (o0 > n_regions ? n_regions : o0);
            o1 = o1 < o0 ? o0 : (o1 > n_regions ? n_regions : o1);
            if (o1 > o0 && kd == LAD_SAMPLE_POOL_ROW) {
                j = o0 + (int64_t)__umulhi(r.x, (unsigned)(o1 - o0));
            } else if (o1 > o0) {
                const Region last = load_region(regions, o1 - 1);
                const int64_t M = pool_cum[o1 - 1] + ((int64_t)last.hi - last.lo - T + 1);
                if (M >= 1 && M < ((int64_t)1 << 32)) {
                    const int64_t u = (int64_t)__umulhi(r.x, (unsigned)M);
                    int64_t base = o0, n = o1 - o0;      // the last region with pool_cum <= u (pool_cum[o0] = 0 <= u)
                    while (n > 1) {
                        const int64_t half = n >> 1;
                        if (pool_cum[base + half] <= u) base += half;
                        n -= half;
                    }
                    j = base;
                    at = u - pool_cum[base];
                }
            }
        }
        int32_t c = 0, cnt = 0;
        int64_t f = 0;
        if (j >= 0 && j < n_regions) {
            const Region g = load_region(regions, j);
            const int64_t len = (int64_t)g.hi - g.lo;
            if (len > 0) {
                const int64_t n = len < T ? len : T;
                const int64_t room = len - n;            // offsets 0 .. room
                int64_t off = at >= 0 ? at : (int64_t)__umulhi(r.y, (unsigned)(room + 1));
                off = off < 0 ? 0 : (off > room ? room : off);   // (a no-op on a table that keeps the convention)
                c = g.chan;
                f = g.lo + off;
                cnt = (int32_t)n;
            }
        } else {
            j = -1;
        }
        chan[i] = c;
        first[i] = f;
        count[i] = cnt;
        if (region) region[i] = (int32_t)j;
    }
}

__global__ __launch_bounds__(THREADS) void coverage_kernel(const int32_t *__restrict__ set_chan, const int64_t *__restrict__ first,
                                                           const int32_t *__restrict__ count, int64_t n, int fps,
                                                           const int32_t *__restrict__ bounds, const int32_t *__restrict__ offsets,
                                                           int64_t n_intervals, int n_channels, int S, int32_t *__restrict__ out) {
    const int64_t total = n * S;
    for (int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * THREADS) {
        const int64_t i = idx / S;
        const int s = (int)(idx - i * S);
        const int c = set_chan[i];
        int64_t sum = 0;
        if (c >= 0 && c < n_channels) {
            int64_t a = first[i];
            int64_t e = count[i];
            a = a < 0 ? 0 : (a > ((int64_t)1 << 40) ? ((int64_t)1 << 40) : a);
            e = a + (e < 0 ? 0 : e);
            // the hull (A, B], clipped to what an int32 bound can reach
            int64_t A = 1000 * a / fps, B = (1000 * e + fps - 1) / fps;
            A = A > 2147483647ll ? 2147483647ll : A;
            B = B > 2147483647ll ? 2147483647ll : B;
            int64_t o0 = offsets[(int64_t)c * S + s], o1 = offsets[(int64_t)c * S + s + 1];
            o0 = o0 < 0 ? 0 : (o0 > n_intervals ? n_intervals : o0);
            o1 = o1 < o0 ? o0 : (o1 > n_intervals ? n_intervals : o1);
            // the first interval with hi > A (ends ascend with the starts: the intervals are disjoint)
            int64_t lo_i = o0, hi_i = o1;
            while (lo_i < hi_i) {
                const int64_t mid = lo_i + ((hi_i - lo_i) >> 1);
                if (bounds[2 * mid + 1] > A) hi_i = mid;
                else lo_i = mid + 1;
            }
            for (int64_t k = lo_i; k < o1; ++k) {
                const int64_t lo = bounds[2 * k], hi = bounds[2 * k + 1];
                if (lo >= B) break;
                const int64_t x0 = lo > A ? lo : A, x1 = hi < B ? hi : B;
                if (x1 > x0) sum += x1 - x0;
            }
        }
        out[idx] = (int32_t)sum;
    }
}

inline unsigned grid_for(int64_t items) { return (unsigned)std::min<int64_t>(lad::ceil_div(items, THREADS), MAX_GRID); }
}  // namespace

extern "C" int lad_sample_segments(const int32_t *kind, const int32_t *src, int64_t n_rows, const int64_t *row_id, const int32_t *regions,
                                   int64_t n_regions, const int32_t *pool_off, const int64_t *pool_cum, int32_t n_pools,
                                   const int32_t *kind_host, const int32_t *src_host, const int32_t *pool_off_host,
                                   const int64_t *pool_total_host, int32_t T, uint64_t seed, uint32_t epoch, int32_t *chan, int64_t *first,
                                   int32_t *count, int32_t *region, void *stream) {
    using namespace lad;
    LAD_REQUIRE(n_rows >= 0 && n_rows <= ((int64_t)1 << 40) && n_regions >= 0 && n_regions <= MAX_N && n_pools >= 0 && n_pools <= MAX_N,
                "lad_sample_segments: rows 0..2^40, regions 0..2^30, pools 0..2^30 (got %lld, %lld, %d)", (long long)n_rows,
                (long long)n_regions, n_pools);
    LAD_REQUIRE(T >= 1, "lad_sample_segments: T = %d frames per segment, at least 1", T);
    LAD_REQUIRE(pool_off && pool_off_host && (n_pools == 0 || pool_total_host), "lad_sample_segments: null pool table");
    LAD_REQUIRE(n_regions == 0 || (regions && pool_cum), "lad_sample_segments: null region table");
    LAD_REQUIRE(pool_off_host[0] == 0, "lad_sample_segments: pool offsets start at %d, expected 0", pool_off_host[0]);
    for (int64_t p = 0; p < n_pools; ++p) {
        const int64_t o0 = pool_off_host[p], o1 = pool_off_host[p + 1];
        LAD_REQUIRE(o0 <= o1 && o1 <= n_regions, "lad_sample_segments: pool offsets do not ascend within %lld regions at pool %lld (%lld, %lld)",
                    (long long)n_regions, (long long)p, (long long)o0, (long long)o1);
        const int64_t M = pool_total_host[p];
        LAD_REQUIRE(M >= 0 && M < ((int64_t)1 << 32), "lad_sample_segments: pool %lld has measure %lld, the draw holds 0 .. 2^32 - 1",
                    (long long)p, (long long)M);
    }
    if (n_rows == 0) return LAD_OK;
    LAD_REQUIRE(kind && src && chan && first && count, "lad_sample_segments: null buffer");
    LAD_REQUIRE((kind_host == nullptr) == (src_host == nullptr), "lad_sample_segments: kind_host and src_host come together");
    if (kind_host) {
        for (int64_t i = 0; i < n_rows; ++i) {
            const int32_t k = kind_host[i];
            const int64_t s = src_host[i];
            LAD_REQUIRE(k >= LAD_SAMPLE_FIXED && k <= LAD_SAMPLE_POOL_MEASURE, "lad_sample_segments: row %lld has kind %d", (long long)i, k);
            if (k == LAD_SAMPLE_FIXED) {
                LAD_REQUIRE(s >= 0 && s < n_regions, "lad_sample_segments: row %lld names region %lld of %lld", (long long)i, (long long)s,
                            (long long)n_regions);
            } else {
                LAD_REQUIRE(s >= 0 && s < n_pools, "lad_sample_segments: row %lld names pool %lld of %d", (long long)i, (long long)s, n_pools);
                LAD_REQUIRE(pool_off_host[s + 1] > pool_off_host[s], "lad_sample_segments: row %lld draws from the empty pool %lld",
                            (long long)i, (long long)s);
                LAD_REQUIRE(k != LAD_SAMPLE_POOL_MEASURE || pool_total_host[s] >= 1,
                            "lad_sample_segments: row %lld draws from pool %lld, which has measure 0", (long long)i, (long long)s);
            }
        }
    }
    hipLaunchKernelGGL(sample_kernel, dim3(grid_for(n_rows)), dim3(THREADS), 0, (hipStream_t)stream, kind, src, n_rows, row_id, regions,
                       n_regions, pool_off, pool_cum, (int)n_pools, (int)T, (unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32),
                       (unsigned)epoch, chan, first, count, region);
    return check_launch("sample_kernel");
}

extern "C" int lad_window_coverage(const int32_t *set_chan, const int64_t *first, const int32_t *count, int64_t n, int32_t fps,
                                   const int32_t *bounds, const int32_t *offsets, const int32_t *bounds_host, const int32_t *offsets_host,
                                   int64_t n_intervals, int32_t n_channels, int32_t n_sets, int32_t *out, void *stream) {
    using namespace lad;
    LAD_REQUIRE(n >= 0 && n <= MAX_N && n_intervals >= 0 && n_intervals <= MAX_N && n_channels >= 1 && n_channels <= 65535 && n_sets >= 1 &&
                    n_sets <= 64 && fps >= 1 && fps <= 100000,
                "lad_window_coverage: windows 0..2^30, intervals 0..2^30, channels 1..65535, sets 1..64, fps 1..100000 "
                "(got %lld, %lld, %d, %d, %d)",
                (long long)n, (long long)n_intervals, n_channels, n_sets, fps);
    LAD_REQUIRE(offsets && offsets_host, "lad_window_coverage: null offsets");
    LAD_REQUIRE(n_intervals == 0 || (bounds && bounds_host), "lad_window_coverage: null interval bounds");
    const int64_t segments = (int64_t)n_channels * n_sets;
    LAD_REQUIRE(offsets_host[0] == 0 && offsets_host[segments] == n_intervals,
                "lad_window_coverage: index offsets run from %d to %d, expected 0 to %lld", offsets_host[0], offsets_host[segments],
                (long long)n_intervals);
    for (int64_t s = 0; s < segments; ++s) {
        const int64_t o0 = offsets_host[s], o1 = offsets_host[s + 1];
        LAD_REQUIRE(o0 <= o1 && o1 <= n_intervals, "lad_window_coverage: index offsets do not ascend at channel %lld, set %lld (%lld, %lld)",
                    (long long)(s / n_sets), (long long)(s % n_sets), (long long)o0, (long long)o1);
        for (int64_t i = o0; i < o1; ++i) {
            const int32_t lo = bounds_host[2 * i], hi = bounds_host[2 * i + 1];
            LAD_REQUIRE(lo >= 0 && hi > lo, "lad_window_coverage: interval %lld (%d, %d] of channel %lld, set %lld is empty or negative",
                        (long long)i, lo, hi, (long long)(s / n_sets), (long long)(s % n_sets));
            LAD_REQUIRE(i == o0 || lo >= bounds_host[2 * i - 1],
                        "lad_window_coverage: interval %lld (%d, %d] of channel %lld, set %lld is unsorted or overlaps the one before it",
                        (long long)i, lo, hi, (long long)(s / n_sets), (long long)(s % n_sets));
        }
    }
    if (n == 0) return LAD_OK;
    LAD_REQUIRE(set_chan && first && count && out, "lad_window_coverage: null buffer");
    hipLaunchKernelGGL(coverage_kernel, dim3(grid_for(n * n_sets)), dim3(THREADS), 0, (hipStream_t)stream, set_chan, first, count, n, (int)fps,
                       bounds, offsets, n_intervals, (int)n_channels, (int)n_sets, out);
    return check_launch("coverage_kernel");
}
