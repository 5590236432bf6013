// RETIRED (round 6): conv_h2.hip as it stood before the wave-specialised experiment left the product source, with that experiment
// (formerly tools/experiments/conv_h2w.inc, compiled in under -DLAD_H2_WS_BUILD) pasted in and always on.  Never part of the product
// library: `tools/exp_retired.sh conv_h2w conv_h2 [-DLAD_WS_<TAG> ...]` builds tools/libexp_conv_h2w_variants.so = the product objects
// with conv_h2.o replaced by this file (ablations: LAD_WS_NOMFMA, LAD_WS_NODMA, LAD_WS_NOROWS, LAD_WS_NOPUT -- results are garbage
// then, only the launch time means something).  LAD_H2_WS=0 in the environment keeps the 256-row launches on conv_h2_kernel.
// Measured and NOT adopted (profiles/r05_conv_h2w.log): correct (tests/test_h2_gpu.py pass with it, bit-identical results), on a par
// with conv_h2_kernel in the micro-benchmark (0.43 vs 0.42 ms on zeros, 0.52 vs 0.51 on data), slower in the step (0.60 vs 0.55 ms
// mean launch).  Its tile header is the snapshot lad_b3_tile_h2w.h next to it (b3_epilogue with ASMBAR / tid_in).
//
// 64 -> 64 (and 32 -> 32) 3x3 stride-1 convolution on the 16-bit matrix cores with TWO f16 planes per operand ("f16 x 2").
//
// Same layers, same tensors, same epilogue as conv_b3.hip (nn.Conv2d(64, 64, 3, padding=1) of block1, models.py:86-95,110-115,
// forward and data gradient) -- at HALF the matrix instructions: three plane products per fp32-equivalent product instead of
// six.  VERDICT r3 item 1 ("cut the executed MFMA work of block1: the part is power-bound, not schedule-bound") asked for a
// Winograd F(2x2,3x3) prototype; profiles/r04_conv_arith_numerics.log prices both against float64 at K = 576: this form has the
// operand error of that Winograd form (7.5e-8 vs 7.0e-8 of the rms output; the fp32 accumulation error all forms share is
// 2.2e-7) with 2x instead of 2.25x fewer MFMAs -- and none of Winograd's structural costs here (16/9 more weight bytes =
// 393 KB of split planes against 160 KB of LDS, 4x the accumulators per output, 16 transformed values to split per 4 inputs).
//
// Arithmetic.  An operand tile is held as x * 2^k = h1 + h2 + e with h1 = f16(x 2^k), h2 = f16(x 2^k - h1) (both round to
// nearest even; the subtraction is exact in f32) and k chosen PER STAGED TILE so that its largest magnitude lands in
// [2^14, 2^15): |e| <= 2^-22 |x 2^k| (measured 2^-23; 2^-24.6 rms -- an fp32 rounding is 2^-24) for every element within 2^17 of
// the tile's maximum, and <= 2^-25 absolute (2^-40 of the tile's maximum) below that, where h2 leaves the normal range of
// f16.  A product is a1 b2 + a2 b1 + a1 b1 (the dropped a2 b2 is below 2^-22 of it): three v_mfma_f32_16x16x32_f16 with f32
// accumulation, each plane product exact in f32.  The power-of-two scales are exact to apply and to undo:
//   * activations: one scale per (workgroup tile, 32-channel stage), from the maximum the workgroup finds while it stages the
//     rows (a block floating point; nothing outside the kernel knows about it);
//   * weights: one scale per 32-channel stage of the packed image, found by the pack kernel and carried in the image's tail;
//   * the f32 accumulators are re-based when the stage changes (ldexp by the difference, exact) and scaled back in the
//     epilogue; a stage may raise the exponent by at most 8 over its predecessor (what it then loses lies below 2^-40 of
//     the sum so far), so nothing can overflow.
//
// Structure = conv_b3x_kernel: a workgroup owns RB x 128 consecutive output rows and all output channels; the fp32 input rows
// (+ halo) are staged 32 channels at a time (one whole 128-byte line per row), BatchNorm + ReLU of the previous layer applied
// on the way when asked (INBN), split into the two planes: LDS rows of 128 bytes [h1: 32 f16][h2: 32 f16] with the 16-byte
// slots XOR-swizzled by (row & 6) -- ds_read_b128 of the A fragments of v_mfma_f32_16x16x32_f16 (16 rows x 4 k-octets) is then
// conflict-free for every tap shift (brute-forced over all row alignments and both planes).  The packed weights stream tap by
// tap (8 KB = [plane][column tile][k octet][16][8 f16]) through an LDS-DMA ring awaited with counted vmcnt.
#include "lad_common.h"
#include "lad_device.h"
#include "lad_b3_tile_h2w.h"

#include <algorithm>
#include <cstdlib>

namespace {
using namespace lad;
using namespace lad::b3t;

constexpr int KC = 32;         // input channels per stage
constexpr int ROWB = 128;      // bytes per staged row: two planes of 32 f16
constexpr int FPIECES = KC * 4 / 16;   // 16-byte pieces (4 fp32 channels) per row and stage

template <int C>
struct H2 {
    static constexpr int NSTAGE = C / KC;
    static constexpr int NCT = C / 16;                       // 16-column output tiles
    static constexpr int PLANE_B = NCT * 1024;               // one plane of a tap: [column tile][k octet 4][n 16][8 f16]
    static constexpr int TAP_BYTES = 2 * PLANE_B;
    static constexpr int IMG_BYTES = TAPS * NSTAGE * TAP_BYTES;   // [tap][stage][plane][...]
    static constexpr int TAIL_BYTES = 16;                    // int32 scale exponent per stage
};

typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned pack_f16(float lo, float hi) {
    const f32x2 v = {lo, hi};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, h16x2));   // round to nearest even
}
// two (scaled) fp32 values -> their two f16 planes, packed pairs
__device__ __forceinline__ void split2_pair(float a, float b, unsigned &p1, unsigned &p2) {
    const f32x2 v = {a, b};
    const h16x2 h = __builtin_convertvector(v, h16x2);
    p1 = __builtin_bit_cast(unsigned, h);
    p2 = pack_f16(a - (float)h.x, b - (float)h.y);   // (the differences are exact in f32)
}

// scale exponent for a tile / an image stage whose largest magnitude is `amax` (>= 0, finite): amax * 2^k in [2^14, 2^15)
__host__ __device__ __forceinline__ int scale_exp(float amax) {
    const int e = (int)((__builtin_bit_cast(unsigned, amax) >> 23) & 0xffu);
    const int k = 141 - e;
    return k > 100 ? 100 : k;       // (zero / denormal maxima: 2^100 keeps every product finite)
}
__device__ __forceinline__ float pow2f(int k) { return __builtin_bit_cast(float, (unsigned)(127 + k) << 23); }   // -126 <= k <= 127

__device__ __forceinline__ float wave_max64(float v) { return wave_max64_dpp(v); }

// ---- weights: (cout, cin, 3, 3) fp32 -> [tap][stage][plane][column tile][k octet][n 16][8 f16] + the stages' exponents ------
// mode 0: forward, GEMM K = cin, N = cout.  mode 1: data gradient, K = cout, N = cin, taps flipped.  One workgroup per image.
struct PackRec {
    const float *w;
    unsigned char *wt;
    int mode;
    int channels;   // read by the mixed launch only (lad_conv_h2_pack_weights_multi with channels = 0)
};
constexpr int PACK_SPLIT = 16;   // workgroups per image: each finds the stages' maxima itself (36,864 weights: 9 float4 per thread), then writes 1/16 of the planes
template <int C>
__device__ __forceinline__ void pack_h2_image(const PackRec &rec, int part) {
    using K = H2<C>;
    __shared__ float smax[K::NSTAGE][16];
    __shared__ int kexp[K::NSTAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // pass 1: the largest magnitude per K stage (every workgroup of the image computes the same numbers)
    float m[K::NSTAGE];
#pragma unroll
    for (int s = 0; s < K::NSTAGE; ++s) m[s] = 0.f;
    static_assert((C * TAPS) % 4 == 0, "float4 groups stay inside one (co, ci range)");
    for (int idx4 = tid; idx4 < C * C * TAPS / 4; idx4 += 1024) {
        const float4 v = reinterpret_cast<const float4 *>(rec.w)[idx4];
        const float a[4] = {fabsf(v.x), fabsf(v.y), fabsf(v.z), fabsf(v.w)};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int idx = idx4 * 4 + j;
            const int co = idx / (C * TAPS), ci = (idx / TAPS) % C;
            const int k = rec.mode == 0 ? ci : co;
#pragma unroll
            for (int s = 0; s < K::NSTAGE; ++s) m[s] = (k / KC == s) ? fmaxf(m[s], a[j]) : m[s];
        }
    }
#pragma unroll
    for (int s = 0; s < K::NSTAGE; ++s) {
        const float v = wave_max64(m[s]);
        if (lane == 0) smax[s][wave] = v;
    }
    __syncthreads();
    if (tid < K::NSTAGE) {
        float v = 0.f;
        for (int w = 0; w < 16; ++w) v = fmaxf(v, smax[tid][w]);
        kexp[tid] = scale_exp(v);
        if (part == 0) reinterpret_cast<int *>(rec.wt + K::IMG_BYTES)[tid] = kexp[tid];
    }
    __syncthreads();
    // pass 2: this workgroup's share of the planes
    unsigned short *out = reinterpret_cast<unsigned short *>(rec.wt);
    constexpr int SHARE = K::IMG_BYTES / 2 / PACK_SPLIT;
    for (int idx = part * SHARE + tid; idx < (part + 1) * SHARE; idx += 1024) {
        int t = idx;
        const int e = t & 7; t >>= 3;
        const int n = t & 15; t >>= 4;
        const int kq = t & 3; t >>= 2;
        const int ct = t % K::NCT; t /= K::NCT;
        const int plane = t & 1; t >>= 1;
        const int stage = t % K::NSTAGE;
        const int tap = t / K::NSTAGE;
        const int k = stage * KC + kq * 8 + e;
        const int nn = ct * 16 + n;
        const int co = rec.mode == 0 ? nn : k, ci = rec.mode == 0 ? k : nn;
        const int src_tap = rec.mode == 0 ? tap : TAPS - 1 - tap;
        const float v = rec.w[((int64_t)co * C + ci) * TAPS + src_tap] * pow2f(kexp[stage]);
        const _Float16 h1 = (_Float16)v;
        const _Float16 h2 = (_Float16)(v - (float)h1);
        out[idx] = __builtin_bit_cast(unsigned short, plane == 0 ? h1 : h2);
    }
}
template <int C>   // C > 0: every record is a C-channel layer; C = 0: a record names its own channel count (64 or 32)
__global__ __launch_bounds__(1024) void pack_h2_kernel(const PackRec *__restrict__ recs) {
    const PackRec rec = recs[blockIdx.x / PACK_SPLIT];
    const int part = blockIdx.x % PACK_SPLIT;
    if (C == 64 || (C == 0 && rec.channels == 64)) pack_h2_image<64>(rec, part);
    else pack_h2_image<32>(rec, part);
}

#ifdef LAD_STAMP
__device__ unsigned long long lad_dbg_h2[16 * 16384];
#define LAD_H2_STAMP(k) \
    if (threadIdx.x == 0 && blockIdx.x < 16384) lad_dbg_h2[blockIdx.x * 16 + (k)] = __builtin_amdgcn_s_memtime();
#else
#define LAD_H2_STAMP(k)
#endif

// ---- the convolution ----------------------------------------------------------------------------------------------------------
// `in`: fp32 rows [rows][C] (layout: lad_device.h).  INBN: `in` is the previous convolution's raw output and in_coef that
// BatchNorm's float[6][C] (scale, shift, ...): relu(in * scale + shift) on interior rows, 0 on border rows, is formed while a
// stage is staged -- the same fmaf / max as bn_act_kernel.  STAT / addend / abits / partials: b3_epilogue (lad_b3_tile.h).
// RB = 2: 256-row tiles, two workgroups per CU (every launch of two dispatch rounds or more); RB = 1: 128-row tiles, three per CU
// (small launches).  Every other structure that was built and measured -- 384-row tiles, four ring slots, persistent workgroups,
// no weight ring, eight waves per workgroup, and the diagnostic builds without MFMAs / loads / epilogue / split -- lives in
// tools/experiments/retired/conv_h2_variants.hip (tools/exp_h2.sh builds it into a library of its own); all of them run in
// 0.49-0.57 ms per launch at batch 512 (profiles/r04_conv_h2_experiments.log, profiles/r05_conv_h2_8waves.log).
//
// EPI: the epilogue options of the launch as compile-time constants (h2_epi(...): h2_epilogue of lad_b3_tile.h, one instantiation
// per form the training engine launches -- the LAD_H2_FORM list of launch_h2_rb), or H2_EPI_ANY: the shared b3_epilogue with its run-time null tests, for
// every other combination of arguments lad_conv_h2 accepts.  Same bits either way.
constexpr int NSLOT = 3;   // ring slots: the LDS-DMA runs two taps ahead of the MFMAs
constexpr int H2_EPI_ANY = -1;
constexpr int h2_epi(bool bias, int addend, bool partials, bool from_bits) {
    return (bias ? 1 : 0) | (addend << 1) | (partials ? 8 : 0) | (from_bits ? 16 : 0);
}
template <int C, int RB, bool STAT, bool INBN, int EPI>
__global__ __launch_bounds__(THREADS, RB == 1 ? 3 : 2) void conv_h2_kernel(const float *__restrict__ in, const unsigned char *__restrict__ wt,
                                                             const float *__restrict__ bias, const float *addend,
                                                             const unsigned long long *__restrict__ abits, float *out,
                                                             float *__restrict__ partials, Geom g, B3Stat bst,
                                                             const float *__restrict__ in_coef) {
    using K = H2<C>;
    constexpr int NSTAGE = K::NSTAGE, NCT = K::NCT, PLANE_B = K::PLANE_B, TAP_BYTES = K::TAP_BYTES;
    constexpr int TMW = TM * RB, NRT = 2 * RB;                       // output rows per workgroup; 16-row tiles per wavefront
    constexpr int NPRE = ((TMW + 2 * 47) * FPIECES + THREADS - 1) / THREADS;   // registers for one stage at the widest image (W = 46)
    constexpr int CPS = TAPS;                                          // one tap per ring chunk
    constexpr int KP = (CPS - NSLOT) < CPS / 2 ? (CPS - NSLOT) : CPS / 2;
    static_assert(CPS % NSLOT == 0 && NPRE <= 32, "every stage starts in ring slot 0; staging geometry");
    extern __shared__ __attribute__((aligned(128))) unsigned char smem_b[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int halo = g.Wp + 1;
    const int nrows = TMW + 2 * halo;
    const int main_bytes = max(NSLOT * TAP_BYTES + nrows * ROWB, TM * (C + 4) * 4);
    unsigned char *b_s = smem_b;                          // [NSLOT][TAP_BYTES]
    unsigned char *a_s = b_s + NSLOT * TAP_BYTES;         // [nrows][ROWB]
    unsigned char *mask_s = smem_b + main_bytes;          // [TMW]
    float *smax = reinterpret_cast<float *>(mask_s + TMW);   // [4]: the waves' maxima of the stage being staged
    // XCD-aware tile order (conv_b3_kernel): XCD x takes a contiguous range of tiles
    const unsigned per_x = (gridDim.x + 7u) / 8u;
    const unsigned tile_id = (blockIdx.x % 8u) * per_x + blockIdx.x / 8u;
    const int64_t q0 = (int64_t)tile_id * TMW;
    if (q0 >= g.rows) return;

    LAD_H2_STAMP(0)
    // a tap is a whole number of THREADS x 16 bytes: every wave issues the same NW_TAP DMAs per tap, whatever its number, and the
    // counted waits below are immediates
    constexpr int NW_TAP = TAP_BYTES / (THREADS * 16);
    static_assert(TAP_BYTES % (THREADS * 16) == 0 && NW_TAP >= 1, "the DMA count per tap must not depend on the wave");
    auto issue_tap = [&](int tap, int stage, int slot) {
        const unsigned char *src = wt + (int64_t)(tap * NSTAGE + stage) * TAP_BYTES;
        unsigned char *dst = b_s + slot * TAP_BYTES;
#pragma unroll
        for (int r = 0; r < NW_TAP; ++r)
            dma16(src + (r * THREADS + tid) * 16, lds_addr(dst + (r * THREADS + wave * 64) * 16));
    };
    const int *wexp = reinterpret_cast<const int *>(wt + K::IMG_BYTES);

    // ---- staging: piece idx = u * THREADS + tid = 16 bytes (4 channels) of row idx >> 3 of the stage's 128-byte line -------------
    const int64_t start = q0 - halo;
    const int64_t first = start < 0 ? 0 : start;
    const int row_lo = (int)(first - start);
    const int64_t span_rows = min(g.rows - first, (int64_t)(nrows - row_lo));
    auto voff = [&](int u) {
        const int idx = u * THREADS + tid;
        return idx < nrows * FPIECES ? ((idx >> 3) - row_lo) * (C * 4) + (idx & 7) * 16 : -1;
    };
    auto stage_rsrc = [&](int stage) {
        return make_rsrc(reinterpret_cast<const unsigned char *>(in) + first * (C * 4) + stage * (KC * 4), span_rows * (C * 4) - stage * (KC * 4));
    };
    unsigned keep_bits = 0;
    u32x4 pre[NPRE];
    // the loaded pieces -> the values the convolution sees (INBN) and their largest magnitude over this thread
    auto activate = [&](int stage) {
        float m = 0.f;
        f32x4 sc = {0.f, 0.f, 0.f, 0.f}, sh = sc;
        if (INBN) {
            sc = *reinterpret_cast<const f32x4 *>(in_coef + stage * KC + (tid & 7) * 4);
            sh = *reinterpret_cast<const f32x4 *>(in_coef + C + stage * KC + (tid & 7) * 4);
        }
#pragma unroll
        for (int u = 0; u < NPRE; ++u) {
            float4 f = as_f4(pre[u]);
            if (INBN) {
                const bool keep = (keep_bits >> u) & 1u;
                f.x = keep ? fmaxf(fmaf(f.x, sc.x, sh.x), 0.f) : 0.f;
                f.y = keep ? fmaxf(fmaf(f.y, sc.y, sh.y), 0.f) : 0.f;
                f.z = keep ? fmaxf(fmaf(f.z, sc.z, sh.z), 0.f) : 0.f;
                f.w = keep ? fmaxf(fmaf(f.w, sc.w, sh.w), 0.f) : 0.f;
                pre[u] = as_u4(f);
            }
            m = fmaxf(fmaxf(m, fmaxf(fabsf(f.x), fabsf(f.y))), fmaxf(fabsf(f.z), fabsf(f.w)));
        }
        m = wave_max64(m);
        if (lane == 0) smax[wave] = m;
    };
    auto tile_exp = [&]() { return scale_exp(fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]))); };
    // registers -> LDS: 4 channels become 8 bytes in each plane; slot (4 plane + k octet) ^ (row & 6) of the row
    auto put_all = [&](float scl) {
#pragma unroll
        for (int u = 0; u < NPRE; ++u) {
            const int idx = u * THREADS + tid;
            if (idx < nrows * FPIECES) {
                const int row = idx >> 3, piece = idx & 7;
                const float4 f = as_f4(pre[u]);
                unsigned a1, a2, b1, b2;
                split2_pair(f.x * scl, f.y * scl, a1, a2);
                split2_pair(f.z * scl, f.w * scl, b1, b2);
                // (offsets, not pointer bits: an XOR on the pointer would lose the LDS address space and turn the store into a flat one)
                const unsigned off = (unsigned)row * ROWB + ((((piece >> 1) ^ (row & 6)) << 4) | ((piece & 1) << 3));
                *reinterpret_cast<u32x2 *>(a_s + off) = u32x2{a1, b1};
                *reinterpret_cast<u32x2 *>(a_s + (off ^ 64u)) = u32x2{a2, b2};
            }
        }
    };

    // ---- prologue: the first stage's rows are requested first (HBM), then the first NSLOT - 1 taps of weights (L2) ---------------
    {
        const __amdgpu_buffer_rsrc_t in_r = stage_rsrc(0);
#pragma unroll
        for (int u = 0; u < NPRE; ++u) pre[u] = buf_load16(in_r, voff(u));
    }
#pragma unroll
    for (int k = 0; k < NSLOT - 1; ++k) issue_tap(k, 0, k);
    for (int j = tid; j < TMW; j += THREADS) mask_s[j] = interior_row32((uint32_t)q0 + (uint32_t)j, g) ? 1 : 0;
    if (INBN) {
#pragma unroll
        for (int u = 0; u < NPRE; ++u)
            keep_bits |= (interior_row32((uint32_t)(start + ((u * THREADS + tid) >> 3)), g) ? 1u : 0u) << u;
    }
    LAD_H2_STAMP(1)
    activate(0);
    __syncthreads();
    int ktot = tile_exp() + wexp[0];   // exponent of the accumulators: acc = 2^ktot x (sum so far)
    put_all(pow2f(ktot - wexp[0]));
    LAD_H2_STAMP(2)

    // ---- fragments ---------------------------------------------------------------------------------------------------------------
    // A (plane p): lane (m = lane & 15, kq = lane >> 4) reads 16 bytes of row r at slot (4 p + kq) ^ (r & 6); row tile t covers rows
    //    (t >> 1) * 128 + wave * 32 + (t & 1) * 16 + m of the tile (multiples of 16 apart: the swizzle term is the same for all).
    // B (plane p): 16 bytes at p * PLANE_B + column tile * 1024 + kq * 256 + m * 16.
    const int m = lane & 15, kq = lane >> 4;
    const int rl = wave * 32 + m + halo - 1;                           // (- 1: tap column offsets 0, 1, 2)
    const unsigned char *b_lane = b_s + kq * 256 + m * 16;

    f32x4 acc[NRT][NCT];
#pragma unroll
    for (int r = 0; r < NRT; ++r)
#pragma unroll
        for (int c = 0; c < NCT; ++c) acc[r][c] = f32x4{0.f, 0.f, 0.f, 0.f};

    // The stages are straight-line code (NSTAGE is 2 or 1): `last` and the tap's wait are constants in every unrolled tap, where a
    // rolled loop tested them at run time (about 100 scalar branches between the first and the last MFMA of a stage).
#pragma unroll
    for (int stage = 0; stage < NSTAGE; ++stage) {
        const bool last = stage + 1 == NSTAGE;
#pragma unroll
        for (int tap = 0; tap < TAPS; ++tap) {
            const int kc = tap;
            const int slot = kc % NSLOT;
            {
                // tap kc has landed (this wave's part), then everybody's; the slot of tap kc - 1 is free
                constexpr int YOUNGER = NSLOT - 2;
                if (!last) {
                    if (kc > KP && kc <= KP + NSLOT - 1) wait_dma_fixed<YOUNGER, NPRE, NW_TAP>();   // + the requested rows
                    else wait_dma_fixed<YOUNGER, 0, NW_TAP>();
                } else {
                    if (CPS - 1 - kc >= YOUNGER) wait_dma_fixed<YOUNGER, 0, NW_TAP>();
                    else wait_dma_fixed<0, 0, NW_TAP>();
                }
                __syncthreads();
                const int kn = kc + NSLOT - 1;
                if (kn < CPS) issue_tap(kn, stage, kn % NSLOT);
                else if (!last) issue_tap(kn - CPS, stage + 1, kn % NSLOT);
                if (kc == KP && !last) {
                    const __amdgpu_buffer_rsrc_t in_r = stage_rsrc(stage + 1);
#pragma unroll
                    for (int u = 0; u < NPRE; ++u) pre[u] = buf_load16(in_r, voff(u));
                }
            }
            const int rt = rl + (tap / 3 - 1) * g.Wp + (tap % 3);
            const unsigned a1o = (unsigned)rt * ROWB + ((unsigned)(kq ^ (rt & 6)) << 4);
            const unsigned a2o = a1o ^ 64u;
            const int boff = slot * TAP_BYTES;
            f16x8 a1[NRT], a2[NRT];
#pragma unroll
            for (int r = 0; r < NRT; ++r) {
                const int roff = ((r >> 1) * TM + (r & 1) * 16) * ROWB;
                a1[r] = *reinterpret_cast<const f16x8 *>(a_s + a1o + roff);
                a2[r] = *reinterpret_cast<const f16x8 *>(a_s + a2o + roff);
            }
#pragma unroll
            for (int c = 0; c < NCT; ++c) {
                const f16x8 b1 = *reinterpret_cast<const f16x8 *>(b_lane + boff + c * 1024);
                const f16x8 b2 = *reinterpret_cast<const f16x8 *>(b_lane + boff + PLANE_B + c * 1024);
                // smallest terms first: a1 b2, a2 b1, then a1 b1
#pragma unroll
                for (int r = 0; r < NRT; ++r) acc[r][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1[r], b2, acc[r][c], 0, 0, 0);
#pragma unroll
                for (int r = 0; r < NRT; ++r) acc[r][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a2[r], b1, acc[r][c], 0, 0, 0);
#pragma unroll
                for (int r = 0; r < NRT; ++r) acc[r][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1[r], b1, acc[r][c], 0, 0, 0);
            }
        }
#ifdef LAD_STAMP
        if (threadIdx.x == 0 && blockIdx.x < 16384) lad_dbg_h2[blockIdx.x * 16 + 3 + 2 * stage] = __builtin_amdgcn_s_memtime();
#endif
        if (!last) {
            activate(stage + 1);
            __syncthreads();  // every wave has finished reading this stage's rows; the next stage's maxima are in smax
            const int kw = wexp[stage + 1];
            const int kn = min(tile_exp() + kw, ktot + 8);
            const int d = kn - ktot;
            if (d != 0) {
#pragma unroll
                for (int r = 0; r < NRT; ++r)
#pragma unroll
                    for (int c = 0; c < NCT; ++c)
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[r][c][j] = __builtin_ldexpf(acc[r][c][j], d);
            }
            ktot = kn;
            const int ka = kn - kw;                      // <= the exponent the stage's maximum allows: no f16 overflow
            put_all(ka >= -126 ? pow2f(ka) : 0.f);       // (more than 2^126 below its predecessor: the stage contributes nothing)
        }
#ifdef LAD_STAMP
        if (threadIdx.x == 0 && blockIdx.x < 16384) lad_dbg_h2[blockIdx.x * 16 + 4 + 2 * stage] = __builtin_amdgcn_s_memtime();
#endif
    }
    __syncthreads();  // every wave is out of the MFMA loop: ring + input rows become the output tile
    LAD_H2_STAMP(11)
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
        const int64_t qs = q0 + rb * TM;
        if (rb > 0) {
            if (qs >= g.rows) break;
            __syncthreads();
        }
        auto store_acc = [&](float *my) {   // D register j of lane l of tile (r, c): row 4 (l >> 4) + j, column l & 15
#pragma unroll
            for (int rr = 0; rr < 2; ++rr)
#pragma unroll
                for (int c = 0; c < NCT; ++c)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        my[(rr * 16 + (lane >> 4) * 4 + j) * (C + 4) + c * 16 + m] = __builtin_ldexpf(acc[rb * 2 + rr][c][j], -ktot);
        };
        if constexpr (EPI == H2_EPI_ANY)
            b3_epilogue<C, STAT>(store_acc, bias, addend, abits, out, partials, mask_s + rb * TM, reinterpret_cast<float *>(smem_b), qs, g.rows, bst);
        else
            h2_epilogue<C, STAT, (EPI & 1) != 0, (EPI >> 1) & 3, (EPI & 8) != 0, (EPI & 16) != 0>(
                store_acc, bias, addend, abits, out, partials, mask_s + rb * TM, reinterpret_cast<float *>(smem_b), qs, g.rows, bst);
    }
    LAD_H2_STAMP(12)
}

// ---- the same convolution, WAVE-SPECIALISED and persistent (round 5) ---------------------------------------------------------------
// What conv_h2_kernel loses (profiles/r04_conv_h2_experiments.log, r05_power_probe.log): a workgroup spends 42 % of its life outside
// its MFMA stages -- waiting for its first rows, splitting the next stage into LDS, transposing and storing its tile -- and neither a
// second / third co-resident workgroup nor eight waves per workgroup fill those gaps: the launch takes the SUM of its memory skeleton
// (0.27 ms) and of its MFMAs (0.25-0.28 ms).  Here the two jobs run in DIFFERENT WAVES of one 512-thread workgroup per CU that walks
// a contiguous range of tiles:
//   waves 0-3 ("M")  fragments from LDS + MFMAs, tap after tap, tile after tile, and the tile's epilogue.  They issue no load and no
//                    LDS-DMA: nothing they wait for has a memory latency.  A tap's fragments are read in the MIDDLE of the previous
//                    tap's MFMAs (two register sets), so the LDS latency is not exposed although a SIMD holds only one M wave.
//   waves 4-7 ("H")  everything that touches memory, one helper per SIMD:
//                    * the LDS-DMA of the weight ring, SEVEN taps ahead (two 1 KB pieces per wave and tap; one wave issuing all eight
//                      took longer than a tap's MFMAs, two waves issuing four each loaded two SIMDs more than the others);
//                    * the input rows -- requested TWO stages ahead, BatchNorm + ReLU (INBN), maxima, split into the two f16 planes,
//                      written into the OTHER of two row buffers while the M waves read one.
//                    Vector-memory operations retire in order, so the counted vmcnt that waits for a tap's weights also waits for
//                    every row load issued before those weights were requested: with the ring seven taps ahead a row load has
//                    eight taps to land before it is in anybody's way (three slots, as conv_h2_kernel has, gave it four taps --
//                    not enough once a tap is as short as its MFMAs).  The helpers' vector instructions issue in the 8 of 16 cycles
//                    an MFMA leaves the SIMD's issue port free (profiles/r05_issue_overlap2.log, "cross-wave").
// One s_barrier per PAIR of taps orders everything (the ring slots of taps k + 6, k + 7 are free, the weights of taps k, k + 1 have
// landed, a stage's rows are complete before its first tap); the M waves pass the barrier of taps k + 1, k + 2 in the middle of tap k.  Every wave executes the same sequence of
// barriers.  Same arithmetic, same order of operations per output element, same scales as conv_h2_kernel: bit-identical results.
constexpr int WS_THREADS = 512, WS_NSLOT = 8;
template <int C>
struct H2W {
    static constexpr int TMW = 2 * TM;                                                   // 256 output rows per tile
    static constexpr int NPRE = ((TMW + 2 * 47) * FPIECES + THREADS - 1) / THREADS;      // 16-byte pieces per H thread and stage
};

template <int C, bool STAT, bool INBN>
__global__ __launch_bounds__(WS_THREADS, 2) void conv_h2w_kernel(const float *__restrict__ in, const unsigned char *__restrict__ wt,
                                                              const float *__restrict__ bias, const float *addend,
                                                              const unsigned long long *__restrict__ abits, float *out,
                                                              float *__restrict__ partials, Geom g, B3Stat bst,
                                                              const float *__restrict__ in_coef) {
    using K = H2<C>;
    constexpr int NSTAGE = K::NSTAGE, NCT = K::NCT, PLANE_B = K::PLANE_B, TAP_BYTES = K::TAP_BYTES;
    constexpr int TMW = H2W<C>::TMW, NRT = 4, NPRE = H2W<C>::NPRE, NK = NSTAGE * TAPS;   // NK = steps (taps) per tile
    static_assert(NSTAGE == 2, "two stages per tile: a stage's parity names its row buffer");
    static_assert(TAP_BYTES == 8 * 1024 && NK % 2 == 0, "a tap = two 1 KB LDS-DMA pieces per H wave; the fragment sets alternate by tap");
    extern __shared__ __attribute__((aligned(128))) unsigned char smem_b[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int halo = g.Wp + 1;
    const int nrows = TMW + 2 * halo;
    const int abuf = nrows * ROWB;
    unsigned char *b_s = smem_b;                               // [WS_NSLOT][TAP_BYTES]
    unsigned char *a_s = b_s + WS_NSLOT * TAP_BYTES;           // [2][nrows][ROWB]: the row buffer of stage s is a_s + s * abuf
    // The epilogue's transposition area [TM][C + 4] LIES OVER the second row buffer: a tile's epilogue runs between the M waves' step 17
    // and their step 0 of the next tile, i.e. before they enter the barrier of that tile's step 1 -- and the helpers write stage 1's
    // rows of the next tile from that tile's step 2 on (`put` below starts at tap 2), stage 1 of the finished tile is dead.
    float *out_s = reinterpret_cast<float *>(a_s + abuf);
    const int abuf2 = max(abuf, TM * (C + 4) * 4);             // (narrow images: the epilogue area is the larger of the two)
    unsigned char *mask_s = a_s + abuf + abuf2;                // [2][TMW]: by tile parity
    float *smax = reinterpret_cast<float *>(mask_s + 2 * TMW); // [2][4]: the H waves' maxima of the stage being staged (by stage)

    // tile range: XCD x owns a contiguous range of tiles, each of its workgroups a contiguous piece of it
    const int64_t total = (g.rows + TMW - 1) / TMW;
    const int64_t per_x = (total + 7) / 8;
    const int64_t wpx = gridDim.x / 8u;
    const int64_t per_w = (per_x + wpx - 1) / wpx;
    const int64_t xcd = blockIdx.x % 8u;
    const int64_t tb = xcd * per_x + (int64_t)(blockIdx.x / 8u) * per_w;
    const int64_t te = min(min(tb + per_w, (xcd + 1) * per_x), total);
    if (tb >= te) return;
    const int ntile = (int)(te - tb);
    const int *wexp = reinterpret_cast<const int *>(wt + K::IMG_BYTES);
    const int kw0 = wexp[0], kw1 = wexp[1];
#ifndef LAD_WS_NOSTAGGER
    // All workgroups start together and run at the same pace: left alone, every CU requests a stage's rows (45 KB) in the same
    // microsecond and HBM serves 11 MB bursts with idle gaps between them.  The workgroups of an XCD start a ninth of a stage apart.
    for (int i = 0; i < (int)((blockIdx.x / 8u) % 9u); ++i) __builtin_amdgcn_s_sleep(13);   // 13 x 64 cycles ~ one tap
#endif
    auto wg_barrier = [&]() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };
    auto tile_exp = [&](int stage) {
        const float *m = smax + stage * 4;
        return scale_exp(fmaxf(fmaxf(m[0], m[1]), fmaxf(m[2], m[3])));
    };
    auto second_half = [&](int64_t q0) { return q0 + TM < g.rows; };
    // ring slot of step k of tile t: (t * NK + k) % WS_NSLOT

    if (wave < 4) {
        // ================================================================== M waves ===============================================
        const int m = lane & 15, kq = lane >> 4;
        const int rl = wave * 32 + m + halo - 1;
        const unsigned char *b_lane = b_s + kq * 256 + m * 16;
        f16x8 fa1[2][NRT], fa2[2][NRT], fb1[2][NCT], fb2[2][NCT];   // two fragment sets: tap k uses set k & 1
        // fragments of step k of a tile whose first ring slot is `slot0` (runtime) into set `set` (compile time)
        auto load_frags = [&](int k, int slot0, f16x8 (&a1)[NRT], f16x8 (&a2)[NRT], f16x8 (&b1)[NCT], f16x8 (&b2)[NCT]) {
            const int stage = k / TAPS, tap = k % TAPS;
            const unsigned char *a_b = a_s + stage * abuf;
            const int rt = rl + (tap / 3 - 1) * g.Wp + (tap % 3);
            const unsigned a1o = (unsigned)rt * ROWB + ((unsigned)(kq ^ (rt & 6)) << 4);
            const unsigned a2o = a1o ^ 64u;
            const int boff = ((slot0 + k) & (WS_NSLOT - 1)) * TAP_BYTES;
#pragma unroll
            for (int r = 0; r < NRT; ++r) {
                const int roff = ((r >> 1) * TM + (r & 1) * 16) * ROWB;
                a1[r] = *reinterpret_cast<const f16x8 *>(a_b + a1o + roff);
                a2[r] = *reinterpret_cast<const f16x8 *>(a_b + a2o + roff);
            }
#pragma unroll
            for (int c = 0; c < NCT; ++c) {
                b1[c] = *reinterpret_cast<const f16x8 *>(b_lane + boff + c * 1024);
                b2[c] = *reinterpret_cast<const f16x8 *>(b_lane + boff + PLANE_B + c * 1024);
            }
        };
        wg_barrier();   // P1: the maxima of the first stage are in smax
        wg_barrier();   // P2: the first stage's rows are in a_s[0]
        wg_barrier();   // steps 0 and 1 of the first tile: their weights have landed
        load_frags(0, 0, fa1[0], fa2[0], fb1[0], fb2[0]);
        for (int t = 0; t < ntile; ++t) {
            const int64_t q0 = (tb + t) * TMW;
            const bool last_tile = t + 1 == ntile;
            const int slot0 = (t * NK) & (WS_NSLOT - 1), slot0n = ((t + 1) * NK) & (WS_NSLOT - 1);
            f32x4 acc[NRT][NCT];
#pragma unroll
            for (int r = 0; r < NRT; ++r)
#pragma unroll
                for (int c = 0; c < NCT; ++c) acc[r][c] = f32x4{0.f, 0.f, 0.f, 0.f};
            int ktot = 0;
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                constexpr int HALF = NCT / 2;
                const int set = k & 1;
                if (k == 0) {
                    ktot = tile_exp(0) + kw0;
                } else if (k == TAPS) {
                    const int kn = min(tile_exp(1) + kw1, ktot + 8);
                    const int d = kn - ktot;
                    if (d != 0) {
#pragma unroll
                        for (int r = 0; r < NRT; ++r)
#pragma unroll
                            for (int c = 0; c < NCT; ++c)
#pragma unroll
                                for (int j = 0; j < 4; ++j) acc[r][c][j] = __builtin_ldexpf(acc[r][c][j], d);
                    }
                    ktot = kn;
                }
                auto mfmas = [&](int c0) {
#ifdef LAD_WS_NOMFMA
                    return;
#endif
#pragma unroll
                    for (int c = c0; c < c0 + HALF; ++c) {
#pragma unroll
                        for (int r = 0; r < NRT; ++r) acc[r][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa1[set][r], fb2[set][c], acc[r][c], 0, 0, 0);
#pragma unroll
                        for (int r = 0; r < NRT; ++r) acc[r][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa2[set][r], fb1[set][c], acc[r][c], 0, 0, 0);
#pragma unroll
                        for (int r = 0; r < NRT; ++r) acc[r][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa1[set][r], fb1[set][c], acc[r][c], 0, 0, 0);
                    }
                };
                mfmas(0);
                __builtin_amdgcn_sched_barrier(0);
                // in the middle of the tap: the next tap's barrier and fragments (their LDS latency passes under the second half)
                if (k + 1 < NK) {
                    if ((k + 1) % 2 == 0) wg_barrier();   // (one barrier per PAIR of steps: it vouches for the weights of both)
                    load_frags(k + 1, slot0, fa1[set ^ 1], fa2[set ^ 1], fb1[set ^ 1], fb2[set ^ 1]);
                } else if (!last_tile) {
                    wg_barrier();   // steps 0 and 1 of the next tile
                    load_frags(0, slot0n, fa1[set ^ 1], fa2[set ^ 1], fb1[set ^ 1], fb2[set ^ 1]);
                }
                // (no scheduling fence here: the sixteen fragment reads are dealt out between the second half's MFMAs, one per MFMA -- issued
                // in one burst they idle the matrix pipe for ~300 cycles, and the 16th outstanding read has to wait for the first)
                mfmas(HALF);
#ifndef LAD_WS_NOMFMA
                if (k + 1 < NK || !last_tile) {
#pragma unroll
                    for (int i = 0; i < 2 * NRT + 2 * NCT; ++i) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // one MFMA
                        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   // one LDS read
                    }
                }
#endif
                __builtin_amdgcn_sched_barrier(0);
            }
            // epilogue: two 128-row halves through out_s (the H waves join the barriers: `epi_barriers` below)
            const bool two = second_half(q0);
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) {
                if (rb == 1) {
                    wg_barrier();   // E2: every M wave is done with the first half's out_s
                    if (!two) break;
                }
                auto store_acc = [&](float *my) {   // D register j of lane l of tile (r, c): row 4 (l >> 4) + j, column l & 15
#pragma unroll
                    for (int rr = 0; rr < 2; ++rr)
#pragma unroll
                        for (int c = 0; c < NCT; ++c)
#pragma unroll
                            for (int j = 0; j < 4; ++j)
                                my[(rr * 16 + (lane >> 4) * 4 + j) * (C + 4) + c * 16 + m] = __builtin_ldexpf(acc[rb * 2 + rr][c][j], -ktot);
                };
#ifdef LAD_WS_NOEPI
                if (partials != nullptr) wg_barrier();
#pragma unroll
                for (int rr = 0; rr < 2; ++rr)
#pragma unroll
                    for (int c = 0; c < NCT; ++c) asm volatile("" ::"v"(acc[rb * 2 + rr][c]));
                continue;
#endif
                int tid_e = tid;   // (laundered per tile: see b3_epilogue)
                asm volatile("" : "+v"(tid_e));
                b3_epilogue<C, STAT, false, true>(store_acc, bias, addend, abits, out, partials, mask_s + (t & 1) * TMW + rb * TM, out_s,
                                                  q0 + rb * TM, g.rows, bst, B3Scatter{nullptr, 0, 0, 0}, tid_e);
            }
        }
        return;
    }
    // ====================================================================== H waves ===============================================
    // global stage G = 2 t + s (t = tile index in the range, s = stage); its rows live in a_s[s].  During stage G the H waves
    //   tap 0     request the rows of stage G + 2 into pre[G & 1] (free: processed during stage G - 1), then take the rows of
    //             stage G + 1 (pre[(G + 1) & 1], requested a whole stage ago) through BatchNorm + ReLU and find the maxima,
    //   taps 2-8  split them into the planes of a_s[(G + 1) & 1] (last read by the M waves during stage G - 1),
    // and at EVERY tap wait for its weights (their own two DMA pieces), pass the barrier and request the weights seven taps ahead.
    const int htid = tid - 256, hwave = wave - 4;
    const int NG = 2 * ntile;
    const int nsteps = ntile * NK;
    u32x4 pre[2][NPRE];
    unsigned keep_bits[2] = {0u, 0u};
    const unsigned lane16 = lane * 16;
    const unsigned bs_h = lds_addr(b_s) + hwave * 1024;
    const unsigned char *wt_h = wt + hwave * 1024;
    // (a wave-uniform base in scalar registers + one 32-bit lane offset: per-lane 64-bit addresses made the compiler spill, and a scratch
    // reload is a vector-memory operation that the counted waits below do not know about)
    auto issue_w = [&](int k, int slot) {   // weights of tile-local step k -> ring slot `slot`: this wave's two 1 KB pieces
#ifdef LAD_WS_NODMA
        return;
#endif
        const int stage = k / TAPS, tap = k % TAPS;
        const unsigned char *src = wt_h + (tap * NSTAGE + stage) * TAP_BYTES;
        const unsigned dst = bs_h + slot * TAP_BYTES;
        dma16s(src, lane16, dst);
        dma16s(src + 4096, lane16, dst + 4096);
    };
    // wait until at most n of this wave's vector-memory operations are outstanding (n is not a compile-time constant at the ends of the range)
    auto wait_vm = [&](int n) {
#define LAD_VM_CASE(N) case N: asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory"); break;
        switch (n) {
            LAD_VM_CASE(0) LAD_VM_CASE(2) LAD_VM_CASE(4) LAD_VM_CASE(6) LAD_VM_CASE(8) LAD_VM_CASE(10) LAD_VM_CASE(12) LAD_VM_CASE(14)
            LAD_VM_CASE(23)
            default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
        }
#undef LAD_VM_CASE
    };
    static_assert(NPRE == 11 && WS_NSLOT == 8, "the cases of wait_vm: 2 j and 2 j + NPRE for j = 0 .. 7");
    auto request = [&](int G, u32x4 (&dst)[NPRE]) {
#ifdef LAD_WS_NOROWS
#pragma unroll
        for (int u = 0; u < NPRE; ++u) dst[u] = u32x4{0x3f800000u + htid, 0x3f000000u, 0x40000000u + u, 0x3f800000u};
        return;
#endif
        const int64_t q0 = (tb + G / 2) * TMW;
        const int stage = G & 1;
        const int64_t start = q0 - halo;
        const int64_t first = start < 0 ? 0 : start;
        const int row_lo = (int)(first - start);
        const int64_t span_rows = min(g.rows - first, (int64_t)(nrows - row_lo));
        const __amdgpu_buffer_rsrc_t in_r =
            make_rsrc(reinterpret_cast<const unsigned char *>(in) + first * (C * 4) + stage * (KC * 4), span_rows * (C * 4) - stage * (KC * 4));
        // piece u of this thread: row 32 u + (htid >> 3), 16 bytes at (htid & 7) * 16: one per-lane offset + a constant per piece (in the
        // VECTOR offset: the scalar offset of a buffer instruction takes no part in the range check that guards the tensor's two ends)
        const int v0 = ((htid >> 3) - row_lo) * (C * 4) + (htid & 7) * 16;
#pragma unroll
        for (int u = 0; u < NPRE; ++u) {
            const int idx = u * THREADS + htid;
            const bool in_tile = (u + 1) * THREADS <= (TMW + 4) * FPIECES || idx < nrows * FPIECES;   // (only the last pieces can lie past the tile's rows)
            dst[u] = buf_load16(in_r, in_tile ? v0 + u * (32 * C * 4) : -1);
        }
    };
    auto find_keep = [&](int G) {   // (INBN) which of this thread's pieces of stage G lie on interior rows
        const int64_t start = (tb + G / 2) * TMW - halo;
        unsigned kb = 0;
#pragma unroll
        for (int u = 0; u < NPRE; ++u) kb |= (interior_row32((uint32_t)(start + ((u * THREADS + htid) >> 3)), g) ? 1u : 0u) << u;
        return kb;
    };
    auto activate = [&](int stage, u32x4 (&p)[NPRE], unsigned kb) {
        float mx = 0.f;
        f32x4 sc = {0.f, 0.f, 0.f, 0.f}, sh = sc;
        if (INBN) {
            sc = *reinterpret_cast<const f32x4 *>(in_coef + stage * KC + (htid & 7) * 4);
            sh = *reinterpret_cast<const f32x4 *>(in_coef + C + stage * KC + (htid & 7) * 4);
        }
#pragma unroll
        for (int u = 0; u < NPRE; ++u) {
            float4 f = as_f4(p[u]);
            if (INBN) {
                const bool keep = (kb >> u) & 1u;
                f.x = keep ? fmaxf(fmaf(f.x, sc.x, sh.x), 0.f) : 0.f;
                f.y = keep ? fmaxf(fmaf(f.y, sc.y, sh.y), 0.f) : 0.f;
                f.z = keep ? fmaxf(fmaf(f.z, sc.z, sh.z), 0.f) : 0.f;
                f.w = keep ? fmaxf(fmaf(f.w, sc.w, sh.w), 0.f) : 0.f;
                p[u] = as_u4(f);
            }
            mx = fmaxf(fmaxf(mx, fmaxf(fabsf(f.x), fabsf(f.y))), fmaxf(fabsf(f.z), fabsf(f.w)));
        }
        mx = wave_max64(mx);
        if (lane == 0) smax[stage * 4 + hwave] = mx;
    };
    auto put = [&](unsigned char *a_b, const u32x4 (&p)[NPRE], int u, float scl) {
#ifdef LAD_WS_NOPUT
        return;
#endif
        const int idx = u * THREADS + htid;
        if (idx < nrows * FPIECES) {
            // row 32 u + r0, piece = htid & 7: the swizzle term (row & 6) is r0's, so the piece's address is one per-thread offset + 32 u rows
            const int r0 = htid >> 3, piece = htid & 7;
            const float4 f = as_f4(p[u]);
            unsigned a1, a2, b1, b2;
            split2_pair(f.x * scl, f.y * scl, a1, a2);
            split2_pair(f.z * scl, f.w * scl, b1, b2);
            const unsigned off0 = (unsigned)r0 * ROWB + ((((piece >> 1) ^ (r0 & 6)) << 4) | ((piece & 1) << 3));
            *reinterpret_cast<u32x2 *>(a_b + off0 + u * (32 * ROWB)) = u32x2{a1, b1};
            *reinterpret_cast<u32x2 *>(a_b + (off0 ^ 64u) + u * (32 * ROWB)) = u32x2{a2, b2};
        }
    };
    auto write_mask = [&](int t) {   // the row mask of tile t (by tile parity: the epilogue of tile t - 1 may still read the other half)
        mask_s[(t & 1) * TMW + htid] = interior_row32((uint32_t)((tb + t) * TMW) + (uint32_t)htid, g) ? 1 : 0;
    };
    // the barriers the M waves execute in one tile's epilogue (b3_epilogue: one per half when there are partials; one between halves)
    auto epi_barriers = [&](int64_t q0) {
        const bool two = second_half(q0);
        if (partials != nullptr) wg_barrier();
        wg_barrier();
        if (two && partials != nullptr) wg_barrier();
    };
    // prologue: the rows of stages 0 and 1, the first three pairs of taps of weights; stage 0 is processed here, stage 1 during stage 0's taps
    request(0, pre[0]);
    if (NG > 1) request(1, pre[1]);
#pragma unroll
    for (int k = 0; k < WS_NSLOT - 2; ++k) issue_w(k, k);
    if (INBN) keep_bits[0] = find_keep(0);
    write_mask(0);
    // (the queue holds: rows 0, rows 1, twelve weight pieces -- everything but the rows of stage 0 may stay in flight)
    wait_vm((NG > 1 ? NPRE : 0) + 2 * (WS_NSLOT - 2));
    activate(0, pre[0], keep_bits[0]);
    wg_barrier();   // P1
    int te0 = tile_exp(0);   // exponent of the tile's first stage: its accumulators start at 2^(te0 + kw0)
    {
        const float scl = pow2f(te0);
#pragma unroll
        for (int u = 0; u < NPRE; ++u) put(a_s, pre[0], u, scl);
    }
    wg_barrier();   // P2
    for (int t = 0; t < ntile; ++t) {
        const int slot0 = (t * NK) & (WS_NSLOT - 1);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int G = 2 * t + s;
            const bool have_next = G + 1 < NG, have_next2 = G + 2 < NG;
            float scl = 0.f;
#pragma unroll
            for (int tap = 0; tap < TAPS; ++tap) {
                const int k = s * TAPS + tap;
                if (k % 2 == 0) {
                    const int left = nsteps - 2 - (t * NK + k);    // steps after this pair
                    // The four weight pieces of this pair of steps have landed.  Younger operations that may stay in flight: the pieces
                    // of the next two pairs (fewer at the very end) and the rows requested at this stage's tap 0 -- issued behind the
                    // pieces of three pairs ahead, they are younger than this pair's pieces for the next three barriers and must
                    // have landed at the fourth (seven or eight steps after their request).
                    // (One compare per barrier: a switch over the counts cost the helpers ~180 scalar instructions per tap.)
                    const bool rows_young = (s == 0 ? (k >= 2 && k <= 6) : (k >= TAPS + 1 && k <= TAPS + 5)) && have_next2;
                    if (left >= 4) {
                        if (rows_young) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(8 + NPRE) : "memory");
                        else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
                    } else {
                        wait_vm(left >= 2 ? 4 : 0);   // (the last pairs of the range: no row request is outstanding any more)
                    }
                    wg_barrier();
                    if (k == 0 && t > 0) epi_barriers((tb + t - 1) * TMW);   // (the M waves run a tile's epilogue behind the next tile's step 0)
                    // the slots of steps k + 6, k + 7 held steps k - 2, k - 1, whose fragments every M wave had in registers before it
                    // entered this barrier
                    if (left >= WS_NSLOT - 2) {
                        issue_w((k + WS_NSLOT - 2) % NK, (slot0 + k + WS_NSLOT - 2) & (WS_NSLOT - 1));
                        issue_w((k + WS_NSLOT - 1) % NK, (slot0 + k + WS_NSLOT - 1) & (WS_NSLOT - 1));
                    }
                }
                if (tap == 0) {
                    if (have_next2) request(G + 2, pre[s]);
                    if (have_next) {
                        if (INBN) keep_bits[s ^ 1] = find_keep(G + 1);
                        activate(s ^ 1, pre[s ^ 1], keep_bits[s ^ 1]);   // (requested a stage ago; landed by that stage's tap 8 at the latest)
                    }
                    if (s == 1 && t + 1 < ntile) write_mask(t + 1);
                }
                if (tap == 2 && have_next) {   // (the maxima were written before the barrier of tap 1)
                    const int te = tile_exp(s ^ 1);
                    int ka;
                    if (s == 1) {   // next is a tile's first stage
                        te0 = te;
                        ka = te;
                    } else {        // next is the second stage of this tile: min(te + kw1, ktot + 8) - kw1 with ktot = te0 + kw0
                        ka = min(te + kw1, te0 + kw0 + 8) - kw1;
                    }
                    scl = ka >= -126 ? pow2f(ka) : 0.f;
                }
                if (tap >= 2 && have_next) {
                    // pieces [lo, hi) of the NPRE in this tap: spread evenly over taps 2..8 (NOT earlier: the second row buffer is the
                    // previous tile's epilogue area until the M waves have entered the barrier of step 1)
                    // (during a tile's first stage they must be done by tap 7: the barrier in front of steps 8 and 9 vouches for the second
                    // stage's rows)
                    const int span = s == 0 ? TAPS - 3 : TAPS - 2;
                    const int lo = min(NPRE, (tap - 2) * NPRE / span), hi = min(NPRE, (tap - 1) * NPRE / span);
#pragma unroll
                    for (int u = 0; u < NPRE; ++u)
                        if (u >= lo && u < hi) put(a_s + (s ^ 1) * abuf, pre[s ^ 1], u, scl);
                }
            }
        }
    }
    epi_barriers((tb + ntile - 1) * TMW);
}

template <int C>
size_t h2w_lds_bytes(const Geom &g) {
    using K = H2<C>;
    const int nrows = H2W<C>::TMW + 2 * (g.Wp + 1);
    const size_t abuf = (size_t)nrows * ROWB;
    return WS_NSLOT * K::TAP_BYTES + abuf + std::max<size_t>(abuf, (size_t)TM * (C + 4) * 4) + 2 * H2W<C>::TMW + 32;
}


template <int C, int RB>
size_t h2_lds_bytes(const Geom &g) {
    using K = H2<C>;
    const int nrows = TM * RB + 2 * (g.Wp + 1);
    const size_t main_bytes = std::max<size_t>(NSLOT * K::TAP_BYTES + (size_t)nrows * ROWB, (size_t)TM * (C + 4) * 4);
    return main_bytes + TM * RB + 16;   // + the row mask (bytes) + the waves' maxima
}

// launches of fewer than two dispatch rounds of 256-row tiles (two workgroups per CU) take 128-row tiles, three per CU
int h2_two_rounds() {
    static int n = 0;
    if (n == 0) {
        int dev = 0;
        hipDeviceProp_t prop;
        n = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
                ? 4 * prop.multiProcessorCount : 1024;
    }
    return n;
}

bool h2_ws_from_env() {
    const char *e = getenv("LAD_H2_WS");
    return e ? e[0] != '0' : true;
}
bool g_h2_ws = h2_ws_from_env();   // (LAD_H2_WS=0 keeps the 256-row launches on conv_h2_kernel)

struct H2Args {
    const float *in, *in_coef;
    const unsigned char *wt;
    const float *bias, *addend;
    const unsigned long long *abits;
    float *out, *partials;
    B3Stat bst;
    Geom g;
    hipStream_t stream;
};

template <int C, int RB, bool STAT, bool INBN, int EPI>
int launch_h2_form(const H2Args &a) {
    static lad::DeviceOnce attr_set;
    if (!attr_set) {
        LAD_HIP_CHECK(hipFuncSetAttribute((const void *)conv_h2_kernel<C, RB, STAT, INBN, EPI>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
        attr_set = true;
    }
    const int64_t tiles = ceil_div(a.g.rows, TM * RB);
    hipLaunchKernelGGL((conv_h2_kernel<C, RB, STAT, INBN, EPI>), dim3((unsigned)(ceil_div(tiles, 8) * 8)), dim3(THREADS), (h2_lds_bytes<C, RB>(a.g)),
                       a.stream, a.in, a.wt, a.bias, a.addend, a.abits, a.out, a.partials, a.g, a.bst, a.in_coef);
    return check_launch("conv_h2_kernel");
}

// The forms with an epilogue of their own = what the training engine launches (engine.py, _conv_s1):
//   forward: bias + partials (+ addend), with or without the input BatchNorm;
//   data gradient: nothing, a plain addend, a gated addend;
//   data gradient with the BatchNorm sums: mask from x, mask from sign bits with a gated addend.
// Everything else lad_conv_h2 accepts runs the shared epilogue (H2_EPI_ANY): same bits, with its run-time tests -- a form the engine
// starts to launch wants a line here (engine.py has the matching note at _conv_s1).
template <int C, int RB, bool STAT, bool INBN>
int launch_h2_rb(const H2Args &a) {
    const int form = h2_epi(a.bias != nullptr, a.addend == nullptr ? H2_ADD_NONE : a.abits == nullptr ? H2_ADD_PLAIN : H2_ADD_GATED,
                            a.partials != nullptr, STAT && a.bst.bits != nullptr);
#define LAD_H2_FORM(...)                                                                                                           \
    if (form == h2_epi(__VA_ARGS__)) return launch_h2_form<C, RB, STAT, INBN, h2_epi(__VA_ARGS__)>(a);
    if constexpr (STAT) {
        LAD_H2_FORM(false, H2_ADD_NONE, true, false)
        LAD_H2_FORM(false, H2_ADD_GATED, true, true)
    } else {
        LAD_H2_FORM(true, H2_ADD_NONE, true, false)
        LAD_H2_FORM(true, H2_ADD_PLAIN, true, false)
        if constexpr (!INBN) {
            LAD_H2_FORM(false, H2_ADD_NONE, false, false)
            LAD_H2_FORM(false, H2_ADD_PLAIN, false, false)
            LAD_H2_FORM(false, H2_ADD_GATED, false, false)
        }
    }
#undef LAD_H2_FORM
    return launch_h2_form<C, RB, STAT, INBN, H2_EPI_ANY>(a);
}

template <int C, bool STAT, bool INBN>
int launch_h2(const float *in, const float *in_coef, const void *wt, const float *bias, const float *addend, const uint64_t *abits,
              float *out, float *partials, const B3Stat &bst, int64_t batch, int32_t H, int32_t W, void *stream, const char *who) {
    const Geom g = make_geom(batch, H, W);
    LAD_REQUIRE(g.rows < ((int64_t)1 << 31) && g.img < (1 << 20), "%s: more than 2^31 rows, or an image of more than 2^20 positions", who);
    LAD_REQUIRE(W <= 46, "%s: image too wide for the tile (W = %d)", who, W);
    const H2Args a{in, in_coef, (const unsigned char *)wt, bias, addend, (const unsigned long long *)abits, out, partials, bst, g, (hipStream_t)stream};
    if (ceil_div(g.rows, TM * 2) < h2_two_rounds()) return launch_h2_rb<C, 1, STAT, INBN>(a);
    if constexpr (C == 64) {
        if (g_h2_ws) {   // wave-specialised persistent workgroups, one per CU (conv_h2w_kernel)
            static bool attr_ws = false;
            if (!attr_ws) {
                LAD_HIP_CHECK(hipFuncSetAttribute((const void *)conv_h2w_kernel<C, STAT, INBN>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
                attr_ws = true;
            }
            const int groups = h2_two_rounds() / 4 / 8 * 8;   // one workgroup per CU, a multiple of the 8 XCDs
            hipLaunchKernelGGL((conv_h2w_kernel<C, STAT, INBN>), dim3((unsigned)groups), dim3(WS_THREADS), (h2w_lds_bytes<C>(g)),
                               (hipStream_t)stream, in, (const unsigned char *)wt, bias, addend, (const unsigned long long *)abits, out,
                               partials, g, bst, in_coef);
            return check_launch("conv_h2w_kernel");
        }
    }
    return launch_h2_rb<C, 2, STAT, INBN>(a);
}
}  // namespace

extern "C" int64_t lad_conv_h2_packed_weight_bytes(int32_t channels) {
    if (channels == 64) return H2<64>::IMG_BYTES + H2<64>::TAIL_BYTES;
    if (channels == 32) return H2<32>::IMG_BYTES + H2<32>::TAIL_BYTES;
    return -1;
}

// `table`: device array of `n` records {const float *w; void *wt; int32 mode; int32 channels} (24 bytes each) of `channels`-channel
// convolutions -- or, with channels = 0, of the channel count each record names (64 or 32) --; one launch packs them all.
extern "C" int lad_conv_h2_pack_weights_multi(const void *table, int32_t n, int32_t channels, void *stream) {
    using namespace lad;
    LAD_REQUIRE(table && n >= 1, "lad_conv_h2_pack_weights_multi: empty table");
    static_assert(sizeof(PackRec) == 24, "record layout");
    if (channels == 64) hipLaunchKernelGGL(pack_h2_kernel<64>, dim3(n * PACK_SPLIT), dim3(1024), 0, (hipStream_t)stream, (const PackRec *)table);
    else if (channels == 32) hipLaunchKernelGGL(pack_h2_kernel<32>, dim3(n * PACK_SPLIT), dim3(1024), 0, (hipStream_t)stream, (const PackRec *)table);
    else if (channels == 0) hipLaunchKernelGGL(pack_h2_kernel<0>, dim3(n * PACK_SPLIT), dim3(1024), 0, (hipStream_t)stream, (const PackRec *)table);
    else return fail(LAD_ERR_INVALID, "lad_conv_h2_pack_weights_multi: 64 or 32 channels, or 0 = per record (got %d)", channels);
    return check_launch("pack_h2_kernel");
}

// out = conv3x3(act(in)) + bias + addend * [addend_bits], with the options of the bf16 x 3 entry points in one signature:
//   in_coef != NULL: act = relu(BatchNorm(in)) formed while staging (lad_conv_b3c_fwd_f32_bnrelu), else act = identity;
//   addend / addend_bits: lad_conv_b3_fwd_f32_gated (both optional; bits need an addend; out may be addend);
//   bn_x != NULL: `partials` receives the sums of the BatchNorm backward that consumes out (lad_conv_b3_dgrad_bnstat: bn_x,
//   bn_coef, optional bn_bits), else the (sum, sum of squares) of out per 128-row tile (or nothing when partials is NULL).
// wt: an image of lad_conv_h2_pack_weights_multi (mode 0 forward, mode 1 data gradient).
extern "C" int lad_conv_h2(const float *in, const float *in_coef, const void *wt, const float *bias, const float *addend,
                           const uint64_t *addend_bits, float *out, float *partials, const float *bn_x, const uint64_t *bn_bits,
                           const float *bn_coef, int64_t batch, int32_t H, int32_t W, int32_t channels, void *stream) {
    using namespace lad;
    const char *who = "lad_conv_h2";
    LAD_REQUIRE(batch >= 1 && H >= 1 && W >= 1, "%s: bad geometry", who);
    LAD_REQUIRE(in && wt && out, "%s: null buffer", who);
    LAD_REQUIRE(addend_bits == nullptr || addend != nullptr, "%s: sign bits without an addend", who);
    LAD_REQUIRE((const void *)in != (const void *)out, "%s: the convolution cannot run in place", who);
    const bool stat = bn_x != nullptr;
    LAD_REQUIRE(!stat || (partials && bn_coef), "%s: the BatchNorm sums need partials and bn_coef", who);
    LAD_REQUIRE(stat || bn_bits == nullptr, "%s: bn_bits without bn_x", who);
    LAD_REQUIRE(!(stat && in_coef), "%s: an input BatchNorm and the backward sums are not combined", who);
    LAD_REQUIRE(channels == 64 || (addend_bits == nullptr && bn_bits == nullptr), "%s: sign bits are kept for 64-channel activations only", who);
    const B3Stat bst{bn_x, (const unsigned long long *)bn_bits, bn_coef};
    if (channels == 64) {
        if (stat) return launch_h2<64, true, false>(in, nullptr, wt, bias, addend, addend_bits, out, partials, bst, batch, H, W, stream, who);
        if (in_coef) return launch_h2<64, false, true>(in, in_coef, wt, bias, addend, addend_bits, out, partials, bst, batch, H, W, stream, who);
        return launch_h2<64, false, false>(in, nullptr, wt, bias, addend, addend_bits, out, partials, bst, batch, H, W, stream, who);
    }
    if (channels == 32) {
        if (stat) return launch_h2<32, true, false>(in, nullptr, wt, bias, addend, addend_bits, out, partials, bst, batch, H, W, stream, who);
        if (in_coef) return launch_h2<32, false, true>(in, in_coef, wt, bias, addend, addend_bits, out, partials, bst, batch, H, W, stream, who);
        return launch_h2<32, false, false>(in, nullptr, wt, bias, addend, addend_bits, out, partials, bst, batch, H, W, stream, who);
    }
    return fail(LAD_ERR_INVALID, "%s: 64 or 32 channels (got %d)", who, channels);
}

#ifdef LAD_STAMP
extern "C" int lad_debug_read_h2_stamps(unsigned long long *host_dst, int64_t n) {
    return hipMemcpyFromSymbol(host_dst, HIP_SYMBOL(lad_dbg_h2), n * sizeof(unsigned long long)) == hipSuccess ? 0 : -2;
}
#endif
