// Train-time augmentation as a second form of the gather kernel (gather.hip): a batch is still ONE launch from the HBM-resident
// whole-channel feature matrices, and a segment may be mixed with an excerpt of another channel, scaled, warped along time and
// masked on its way out.  Modelled on what Lhotse does to precomputed features -- SpecAugment (time warp, frame masks, feature
// masks, mean fill) and the feature-domain mixer behind MixedCut, log(exp(a) + gain * exp(b)) with the gain taken from an SNR over
// summed energies -- parity with Lhotse unpinned: the convention is the text next to lad_gather_segments_aug in include/lad_hip.h,
// and tests/_augment_model.py is a second implementation of that text.
//
// One workgroup per segment.  The segment (and the noise excerpt, when it mixes) sits in LDS as float4; the time warp writes the
// second buffer, which the mix has left free.  The draws are made once per workgroup (one Philox block per thread, 2 + the number of
// masks of them) and shared through LDS; sums are a 64-wide wave shuffle, then the waves' partials in LDS added in wave order, so a
// segment's result depends on nothing but (seed, epoch, channel, first frame, count): not on where in the batch it stands.  A segment
// none of whose stages fire is copied straight through, 16 bytes per lane on both sides as in gather_kernel: the same bits.
#include <algorithm>

#include "lad_common.h"
#include "lad_device.h"
#include "lad_philox.h"

namespace {
using namespace lad;

constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int MAX_MASKS = 16;                   // of each kind
constexpr int64_t MAX_LDS = 160 * 1024;         // one CU's LDS

struct Scratch {                                // head of the dynamic LDS: sizeof is a multiple of 16, the float4 buffers follow
    U4 draw[2];                                 // blocks 0 and 1 of the convention
    int t0[MAX_MASKS], t1[MAX_MASKS];           // time mask m covers rows [t0, t1)
    int f0[MAX_MASKS], f1[MAX_MASKS];           // feature mask m covers filters [f0, f1)
    float red[WAVES];
};
static_assert(sizeof(Scratch) % 16 == 0, "the float4 buffers behind the scratch must stay 16-byte aligned");

struct AugArgs {
    const float *const *chan_ptr;
    const int64_t *chan_frames;
    const int32_t *chan;
    const int64_t *first;
    const int32_t *count;
    int64_t n_seg;
    int T, F4;
    float pad;
    lad_augment_params p;
    const int32_t *noise;
    int n_noise;
    float4 *out;
};

__device__ __forceinline__ float unit(unsigned u) { return (float)(u >> 8) * (1.0f / 16777216.0f); }

// sum over the workgroup, the same value in every thread: lanes by xor butterfly, then the waves' partials in wave order.
// Contains barriers: every thread of the workgroup calls it.
__device__ __forceinline__ float block_sum(float v, float *red) {
    v = wave_sum64(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = red[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) s += red[w];
    __syncthreads();   // (red is free again)
    return s;
}

// 16-byte piece i of the T x F excerpt that starts at frame `from` of a channel: rows past `rows` or outside the channel are `pad`
__device__ __forceinline__ float4 piece(const float4 *__restrict__ src, int64_t frames, int64_t from, int rows, int F4, float pad, int i) {
    const int t = i / F4, f4 = i - t * F4;
    const int64_t st = from + t;
    if (t < rows && st >= 0 && st < frames) return src[st * F4 + f4];
    return make_float4(pad, pad, pad, pad);
}

__global__ __launch_bounds__(THREADS) void gather_aug_kernel(AugArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    Scratch &s = *reinterpret_cast<Scratch *>(smem);
    const int T = a.T, F4 = a.F4, F = 4 * F4, n4 = T * F4, tid = threadIdx.x;
    float4 *A = reinterpret_cast<float4 *>(smem + sizeof(Scratch)), *B = A + n4;
    const lad_augment_params &p = a.p;
    const int n_masks = max(p.n_time, p.n_freq);
    const bool gain_on = !(p.gain_lo == 0.f && p.gain_hi == 0.f);

    for (int64_t b = blockIdx.x; b < a.n_seg; b += gridDim.x) {
        const int c = a.chan[b], cnt = a.count[b];
        const int64_t from = a.first[b];
        const float4 *src = reinterpret_cast<const float4 *>(a.chan_ptr[c]);
        const int64_t frames = a.chan_frames[c];
        float4 *out = a.out + b * n4;

        // ---- the draws: Philox block k of this segment in thread k ----------------------------------------------------------
        if (tid < 2 + n_masks) {
            const U4 r = philox4x32_10(U4{(unsigned)from, (unsigned)c, p.epoch, (unsigned)tid}, (unsigned)p.seed, (unsigned)(p.seed >> 32));
            if (tid < 2) s.draw[tid] = r;
            else {
                const int m = tid - 2;
                const int wt = m < p.n_time ? (int)__umulhi(r.x, (unsigned)(p.Wt + 1)) : 0;
                const int st = (int)__umulhi(r.y, (unsigned)(T - wt + 1));
                const int wf = m < p.n_freq ? (int)__umulhi(r.z, (unsigned)(p.Wf + 1)) : 0;
                const int sf = (int)__umulhi(r.w, (unsigned)(F - wf + 1));
                s.t0[m] = st; s.t1[m] = st + wt;
                s.f0[m] = sf; s.f1[m] = sf + wf;
            }
        }
        __syncthreads();
        const U4 d0 = s.draw[0], d1 = s.draw[1];
        const bool spec = unit(d0.x) < p.p;
        const bool mix = a.n_noise > 0 && unit(d0.y) < p.mix_p;
        const bool mix_stage = mix || gain_on, warp = spec && p.W > 0, masks = spec && n_masks > 0;

        if (!(mix_stage || warp || masks)) {   // nothing fires: gather_kernel's copy
            for (int i = tid; i < n4; i += THREADS) out[i] = piece(src, frames, from, cnt, F4, a.pad, i);
            __syncthreads();                   // (the draws are read; the next segment may overwrite them)
            continue;
        }

        // ---- 1. gather ----------------------------------------------------------------------------------------------------------
        for (int i = tid; i < n4; i += THREADS) A[i] = piece(src, frames, from, cnt, F4, a.pad, i);

        // ---- 2. mix / gain: log(max(1e-10, G exp(a) + k exp(b))), k from the SNR over the summed energies -------------------------
        if (mix_stage) {
            const float snr_db = p.snr_lo + (p.snr_hi - p.snr_lo) * unit(d0.z);
            const float gain_db = p.gain_lo + (p.gain_hi - p.gain_lo) * unit(d0.w);
            const float G = powf(10.0f, gain_db / 10.0f);
            float k = 0.f;
            float ea = 0.f, eb = 0.f;
            if (mix) {
                const int j = a.noise[__umulhi(d1.x, (unsigned)a.n_noise)];
                const int64_t nframes = a.chan_frames[j];
                const int64_t span = nframes - T + 1;   // (the host refuses noise channels shorter than T frames; guarded all the same)
                const int64_t nfrom = span >= 1 ? (int64_t)__umulhi(d1.y, (unsigned)(span < 0xffffffffll ? span : 0xffffffffll)) : 0;
                const float4 *nsrc = reinterpret_cast<const float4 *>(a.chan_ptr[j]);
                for (int i = tid; i < n4; i += THREADS) {
                    const float4 v = piece(nsrc, nframes, nfrom, T, F4, a.pad, i);
                    B[i] = v;
                    eb += (expf(v.x) + expf(v.y)) + (expf(v.z) + expf(v.w));
                }
                for (int i = tid; i < n4; i += THREADS) {   // (this thread's own pieces: no barrier needed yet)
                    const float4 v = A[i];
                    ea += (expf(v.x) + expf(v.y)) + (expf(v.z) + expf(v.w));
                }
                ea = block_sum(ea, s.red);
                eb = block_sum(eb, s.red);
                k = G * ea / (powf(10.0f, snr_db / 10.0f) * eb);
            }
            for (int i = tid; i < n4; i += THREADS) {
                const float4 v = A[i];
                float4 o = make_float4(G * expf(v.x), G * expf(v.y), G * expf(v.z), G * expf(v.w));
                if (mix) {
                    const float4 n = B[i];
                    o.x += k * expf(n.x); o.y += k * expf(n.y); o.z += k * expf(n.z); o.w += k * expf(n.w);
                }
                A[i] = make_float4(logf(fmaxf(1e-10f, o.x)), logf(fmaxf(1e-10f, o.y)), logf(fmaxf(1e-10f, o.z)), logf(fmaxf(1e-10f, o.w)));
            }
        }
        __syncthreads();   // A is complete, B is free
        float4 *cur = A;

        // ---- 3. time warp: the rows left of c' read [0, c), the rows from c' on read [c, T), linearly between two rows ------------
        if (warp) {
            const int cc = p.W + (int)__umulhi(d1.z, (unsigned)(T - 2 * p.W));
            const int cp = cc + (int)__umulhi(d1.w, (unsigned)(2 * p.W - 1)) - (p.W - 1);
            for (int i = tid; i < n4; i += THREADS) {
                const int t = i / F4, f4 = i - t * F4;
                const int num = t < cp ? t * cc : (t - cp) * (T - cc), den = t < cp ? cp : T - cp, base = t < cp ? 0 : cc;
                const int q = num / den, rem = num - q * den;
                const int i0 = base + q, i1 = min(i0 + 1, T - 1);
                float4 v = A[i0 * F4 + f4];
                if (rem != 0) {
                    const float frac = (float)rem / (float)den;
                    const float4 u = A[i1 * F4 + f4];
                    v = make_float4(fmaf(frac, u.x - v.x, v.x), fmaf(frac, u.y - v.y, v.y), fmaf(frac, u.z - v.z, v.z), fmaf(frac, u.w - v.w, v.w));
                }
                B[i] = v;
            }
            __syncthreads();
            cur = B;
        }

        // ---- 4. masks, filled with the segment's mean after stage 3 ----------------------------------------------------------------
        if (masks) {
            float sum = 0.f;
            for (int i = tid; i < n4; i += THREADS) {
                const float4 v = cur[i];
                sum += (v.x + v.y) + (v.z + v.w);
            }
            const float mean = block_sum(sum, s.red) / (float)(T * F);
            for (int i = tid; i < n4; i += THREADS) {
                const int t = i / F4, f = 4 * (i - t * F4);
                float4 v = cur[i];
                bool row = false, fx = false, fy = false, fz = false, fw = false;
                for (int m = 0; m < n_masks; ++m) {
                    row |= t >= s.t0[m] && t < s.t1[m];
                    const int lo = s.f0[m], hi = s.f1[m];
                    fx |= f >= lo && f < hi;
                    fy |= f + 1 >= lo && f + 1 < hi;
                    fz |= f + 2 >= lo && f + 2 < hi;
                    fw |= f + 3 >= lo && f + 3 < hi;
                }
                if (row || fx) v.x = mean;
                if (row || fy) v.y = mean;
                if (row || fz) v.z = mean;
                if (row || fw) v.w = mean;
                out[i] = v;
            }
        } else {
            for (int i = tid; i < n4; i += THREADS) out[i] = cur[i];
        }
        __syncthreads();   // (LDS is read; the next segment may overwrite it)
    }
}
}  // namespace

extern "C" int lad_gather_segments_aug(const float *const *chan_ptr, const int64_t *chan_frames, const int32_t *chan,
                                       const int64_t *first, const int32_t *count, int64_t n_seg, int32_t n_frames, int32_t F,
                                       float pad, const lad_augment_params *params, const int32_t *noise_list, int32_t n_noise,
                                       int64_t min_noise_frames, float *out, void *stream) {
    using namespace lad;
    LAD_REQUIRE(params, "lad_gather_segments_aug: null parameter struct");
    const lad_augment_params &p = *params;
    const int T = n_frames;
    LAD_REQUIRE(n_seg >= 0 && T >= 1 && F >= 4 && F % 4 == 0, "lad_gather_segments_aug: F must be a multiple of 4 (got %d), n_frames >= 1", F);
    LAD_REQUIRE(p.p >= 0.f && p.p <= 1.f && p.mix_p >= 0.f && p.mix_p <= 1.f,
                "lad_gather_segments_aug: probabilities must lie in [0, 1] (p = %g, mix_p = %g)", (double)p.p, (double)p.mix_p);
    LAD_REQUIRE(p.snr_lo <= p.snr_hi && p.gain_lo <= p.gain_hi, "lad_gather_segments_aug: a range needs lo <= hi (snr %g..%g dB, gain %g..%g dB)",
                (double)p.snr_lo, (double)p.snr_hi, (double)p.gain_lo, (double)p.gain_hi);
    LAD_REQUIRE(p.n_time >= 0 && p.n_time <= MAX_MASKS && p.n_freq >= 0 && p.n_freq <= MAX_MASKS,
                "lad_gather_segments_aug: at most %d masks of each kind (got %d time, %d feature)", MAX_MASKS, p.n_time, p.n_freq);
    LAD_REQUIRE(p.W >= 0 && (int64_t)T > 2 * (int64_t)p.W, "lad_gather_segments_aug: the time warp needs n_frames > 2 W (n_frames = %d, W = %d)", T, p.W);
    LAD_REQUIRE(p.Wt >= 0 && p.Wt <= T && p.Wf >= 0 && p.Wf <= F,
                "lad_gather_segments_aug: mask widths must fit the segment (Wt = %d of %d frames, Wf = %d of %d filters)", p.Wt, T, p.Wf, F);
    LAD_REQUIRE(n_noise >= 0 && (n_noise == 0 || (noise_list && min_noise_frames >= T)),
                "lad_gather_segments_aug: every noise channel needs at least n_frames = %d frames (shortest: %lld)", T, (long long)min_noise_frames);
    const int64_t lds = (int64_t)sizeof(Scratch) + 2 * (int64_t)T * F * (int64_t)sizeof(float);
    LAD_REQUIRE(lds <= MAX_LDS, "lad_gather_segments_aug: a %d x %d segment and its noise excerpt need %lld bytes of LDS, a CU has %lld", T, F,
                (long long)lds, (long long)MAX_LDS);
    LAD_REQUIRE(chan_ptr && chan_frames && chan && first && count && out, "lad_gather_segments_aug: null buffer");
    if (n_seg == 0) return LAD_OK;
    static DeviceOnce attr_set;   // (past the 64 KB a kernel gets without opting in: per device, lad_common.h)
    if (!attr_set) {
        LAD_HIP_CHECK(hipFuncSetAttribute((const void *)gather_aug_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)MAX_LDS));
        attr_set = true;
    }
    AugArgs a;
    a.chan_ptr = chan_ptr; a.chan_frames = chan_frames; a.chan = chan; a.first = first; a.count = count;
    a.n_seg = n_seg; a.T = T; a.F4 = F / 4; a.pad = pad; a.p = p;
    a.noise = noise_list; a.n_noise = n_noise; a.out = (float4 *)out;
    const unsigned grid = (unsigned)std::min<int64_t>(n_seg, 256 * 64);
    hipLaunchKernelGGL(gather_aug_kernel, dim3(grid), dim3(THREADS), (size_t)lds, (hipStream_t)stream, a);
    return check_launch("gather_aug_kernel");
}
