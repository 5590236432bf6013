/*
 * lad_hip.h -- C ABI of liblad_hip.so: the MI355X (gfx950) hot path of laughter-detection-icsi.
 *
 * The reference (LasseWolter/laughter-detection-icsi) is pure Python and has no FFI layer; its seams
 * for this path are Python call signatures.  Each entry point below names the reference interface it
 * replaces (file:line in the reference tree).  The reference-side binding is a ctypes stub
 * (INTEGRATION.md); the host-side mirror of the reference modules lives in laughter-detection-icsi_amd/.
 *
 * Conventions
 *   - every function returns 0 on success, a negative lad_status otherwise; lad_last_error() gives the
 *     thread-local message.  Nothing throws across the ABI.
 *   - all data pointers are caller-owned DEVICE pointers to contiguous buffers unless a parameter is
 *     documented as host memory; the library never frees caller memory.
 *   - `stream` is a hipStream_t passed as void*; launches are asynchronous, no hidden device sync.
 *   - scratch memory is passed in by the caller (size from the matching *_workspace_bytes query).
 *   - plans own small immutable device tables (window, twiddles, filterbank) and may be shared by
 *     threads; launches on distinct streams may run concurrently.
 */
#ifndef LAD_HIP_H
#define LAD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LAD_VERSION 100 /* major*10000 + minor*100 + patch */

enum lad_status {
    LAD_OK = 0,
    LAD_ERR_INVALID = -1, /* bad argument / unsupported shape */
    LAD_ERR_HIP = -2,     /* a HIP runtime call failed */
    LAD_ERR_NOMEM = -3,
    /* not an error: a try-and-fall-back entry point (lad_f16_block_fwd) does not cover this geometry; nothing was launched,
     * lad_last_error() is untouched, the caller takes the general path */
    LAD_NOT_COVERED = 1
};

int lad_version(void);
const char *lad_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * Feature extraction: framed PCM -> window -> rFFT-512 -> power -> mel filterbank -> log [-> DCT].
 * Replaces the object returned by get_feat_extractor (utils/utils.py:6-26; Lhotse
 * Fbank(FbankConfig(num_filters=44, frame_shift=0.01)), config.py:28-31) and its .extract() as
 * reached from load_data.py:47-49 and compute_features.py:84,105-109.
 * ---------------------------------------------------------------------------------------------- */
enum lad_pad_mode {
    LAD_PAD_KALDI_MIRROR = 0,   /* snip_edges=False: T=(N+hop/2)/hop, edge-inclusive mirror padding  */
    LAD_PAD_CENTER_REFLECT = 1, /* librosa center=True, pad_mode="reflect": T=1+N/hop                 */
    LAD_PAD_CENTER_ZERO = 2     /* librosa center=True, pad_mode="constant"                           */
};
enum lad_log_mode {
    LAD_LOG_LN = 0,   /* ln(max(mel, log_floor))        (Kaldi/Lhotse)                */
    LAD_LOG_DB = 1,   /* 10*log10(max(mel, log_floor))  (librosa power_to_db, no top_db) */
    LAD_LOG_NONE = 2  /* raw mel power                                                 */
};

typedef struct lad_fbank_cfg {
    int32_t n_fft;      /* must be 512                                                           */
    int32_t frame_len;  /* samples per frame that enter DC removal / pre-emphasis (<= n_fft)     */
    int32_t hop;        /* frame shift in samples                                                */
    int32_t n_mels;     /* 1..64                                                                 */
    int32_t n_mfcc;     /* 0 = output log-mel; 1..64 = output first n_mfcc DCT coefficients      */
    int32_t pad_mode;   /* lad_pad_mode                                                          */
    int32_t log_mode;   /* lad_log_mode                                                          */
    int32_t remove_dc;  /* subtract the frame mean before pre-emphasis                           */
    float preemph;      /* 0 disables                                                            */
    float log_floor;    /* 1.1920929e-07 for Lhotse, 1e-10 for librosa                           */
} lad_fbank_cfg;

/* window:  HOST float[n_fft]   (analysis window, zero beyond frame_len / centred as the convention needs)
 * melbank: HOST float[(n_fft/2+1) * n_mels], row-major (bin, filter)
 * dct:     HOST float[n_mels * n_mfcc] row-major (filter, coefficient), or NULL when n_mfcc == 0      */
int lad_fbank_plan_create(const lad_fbank_cfg *cfg, const float *window, const float *melbank,
                          const float *dct, void **plan_out);
int lad_fbank_plan_destroy(void *plan);
/* Two kernels implement the same arithmetic: the general one (any hop / frame length / DCT) and a fast one for
 * configurations with hop % 16 == 0, frame_len % 16 == 0, no DCT (the reference's: 400 / 160 / 44 filters), chosen
 * automatically.  which = 1 pins the general kernel (tests compare the two), 0 restores the automatic choice. */
int lad_fbank_plan_set_kernel(void *plan, int32_t which);
int lad_fbank_plan_has_fast_kernel(const void *plan);
/* frames produced for a clip of `samples_per_clip` samples (same formula the kernel uses) */
int64_t lad_fbank_num_frames(const void *plan, int64_t samples_per_clip);
/* pcm: float[n_clips][samples_per_clip] in [-1,1];  out: float[n_clips][T][n_out], n_out = n_mfcc ? n_mfcc : n_mels */
int lad_fbank_forward(void *plan, const float *pcm, int64_t n_clips, int64_t samples_per_clip,
                      float *out, void *stream);
/* one long channel (load_data.py:44-49: whole file as a single cut): out float[T][n_out] */
int lad_fbank_forward_long(void *plan, const float *pcm, int64_t n_samples, float *out, void *stream);

/* Batch assembly from HBM-resident whole-channel feature matrices: segment b = frames [first[b], first[b]+count[b])
 * of matrix chan[b], right-padded to n_frames rows with `pad`.  Replaces PrecomputedFeatures()(cuts) inside
 * LadDataset.__getitem__ (datasets.py:49-68; pad = log(eps) of the training cuts) and InferenceDataset.__getitem__
 * (datasets.py:85-93; pad = 0.0).  chan_ptr: DEVICE array of device pointers to float[chan_frames[c]][F];
 * chan_frames, chan, first, count: device arrays.  out: float[n_seg][n_frames][F]. */
int lad_gather_segments(const float *const *chan_ptr, const int64_t *chan_frames, const int32_t *chan,
                        const int64_t *first, const int32_t *count, int64_t n_seg, int32_t n_frames, int32_t F, float pad,
                        float *out, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Train-time augmentation: lad_gather_segments with SpecAugment and a noise mix on the way (csrc/augment.hip).
 * Modelled on what Lhotse does to precomputed features -- SpecAugment (time warp, frame masks, feature masks, mean fill) and
 * the feature-domain mixer behind MixedCut, log(exp(a) + gain * exp(b)) with the gain taken from an SNR over summed energies.
 * Parity with Lhotse is [UPSTREAM-UNVERIFIED]; the text below IS the specification (tests/_augment_model.py is a second
 * implementation of it, in numpy).
 *
 * Inputs.  Per segment b: chan[b], first[b], count[b] as for lad_gather_segments; T = n_frames, F, pad.
 *
 * Random words.  Philox4x32-10 (csrc/lad_philox.h) with key (seed & 0xffffffff, seed >> 32).  Block k of segment b is
 *   philox(counter = (first[b] & 0xffffffff, chan[b], epoch, k)) -> words r0..r3.
 * A segment's augmentation is a pure function of (seed, epoch, channel, first frame): not of its position in the batch, the
 * batch size, the rank or the world size.  The caller keeps 0 <= first[b] < 2^32.
 *   mulhi(u, n) = (u * n) >> 32         (an integer in [0, n))
 *   unit(u)     = float(u >> 8) * 2^-24 (exact in fp32; the dropout mask's rule)
 * p, mix_p and the four range ends are fp32 (the struct's fields); the gates compare in fp32.
 *
 * Block 0.   spec gate: unit(r0) < p.    mix gate: unit(r1) < mix_p.
 *            snr_db = snr_lo + (snr_hi - snr_lo) * unit(r2).    gain_db = gain_lo + (gain_hi - gain_lo) * unit(r3).
 * Block 1.   noise channel j = noise_list[mulhi(r0, n_noise)];  noise first frame = mulhi(r1, frames[j] - T + 1);
 *            warp centre c = W + mulhi(r2, T - 2 W);  warp shift w = mulhi(r3, 2 W - 1) - (W - 1);  c' = c + w.
 *            (W <= c <= T - W - 1 and |w| <= W - 1, so 1 <= c' <= T - 2.)
 * Block 2+m, for m < max(n_time, n_freq).
 *            time mask m (m < n_time):     width = mulhi(r0, Wt + 1), start = mulhi(r1, T - width + 1);
 *            feature mask m (m < n_freq):  width = mulhi(r2, Wf + 1), start = mulhi(r3, F - width + 1).
 *
 * Stages, in this order.
 *  1. Gather.  As lad_gather_segments, `pad` rows included: x[T][F].
 *  2. Mix / gain.  Runs only if (the mix gate passed and n_noise > 0) or the gain range is not (0, 0); otherwise the values stay
 *     bit-identical copies.  a = the gathered segment, b = frames [noise first frame, + T) of channel j.
 *       Ea = sum of exp(a) over all T * F entries;  Eb = sum of exp(b) over the T * F entries of the excerpt;
 *       G = 10^(gain_db / 10);  k = G * Ea / (10^(snr_db / 10) * Eb), or 0 without mix;
 *       x = log(max(1e-10, G * exp(a) + k * exp(b))).          (accurate expf / logf / powf, fp32 sums)
 *  3. Time warp.  Only if the spec gate passed and W > 0.  Output row t < c' reads position t * c / c' of x; output row t >= c'
 *     reads position c + (t - c') * (T - c) / (T - c').  With q and rem the integer quotient and remainder of that fraction, den
 *     its denominator and base = 0 or c:  i0 = base + q,  i1 = min(i0 + 1, T - 1),  frac = float(rem) / float(den) (fp32), and the
 *     row is x[i0] + frac * (x[i1] - x[i0]) (one subtraction, one fused multiply-add).  Rows with rem = 0 are copies of x[i0].
 *  4. Masks.  Only if the spec gate passed.  The fill value is the mean over all T * F entries after stage 3; every entry of a
 *     row in a time mask or of a filter in a feature mask becomes that value.
 * A segment none of whose stages fire is a copy: its bits are those lad_gather_segments writes.
 *
 * noise_list: DEVICE array of n_noise channel indices (into chan_ptr / chan_frames), or NULL with n_noise = 0 (no mixing);
 * min_noise_frames: the smallest frame count among those channels, as the caller knows it on the host.
 * Refused with LAD_ERR_INVALID before anything is launched: F % 4 != 0; T <= 2 W; Wt > T; Wf > F; more than 16 masks of a kind;
 * a probability outside [0, 1]; lo > hi; min_noise_frames < T; a segment pair (2 * T * F * 4 bytes + scratch) past the 160 KB
 * of LDS of a CU. */
typedef struct lad_augment_params {
    uint64_t seed;
    uint32_t epoch;
    float p, mix_p;            /* SpecAugment gate, mix gate */
    float snr_lo, snr_hi;      /* dB */
    float gain_lo, gain_hi;    /* dB */
    int32_t W;                 /* time warp: the centre moves by less than W frames (0: no warp) */
    int32_t n_time, Wt;        /* time masks: how many, widest */
    int32_t n_freq, Wf;        /* feature masks: how many, widest */
} lad_augment_params;
int lad_gather_segments_aug(const float *const *chan_ptr, const int64_t *chan_frames, const int32_t *chan,
                            const int64_t *first, const int32_t *count, int64_t n_seg, int32_t n_frames, int32_t F, float pad,
                            const lad_augment_params *params, const int32_t *noise_list, int32_t n_noise,
                            int64_t min_noise_frames, float *out, void *stream);

/* Sliding-window inference (segment_laughter.py:90-101): windows at a stride of one frame share 99 % of their input, and the
 * full-resolution layers (stem + the stride-1 blocks) see that overlap unchanged outside `band` rows of a window's top and
 * bottom (band = 3x3 convolutions on the way).  lad_assemble_windows builds the activation of n_windows windows of H rows from
 *   stream_act  the same layers run once over the stream: ONE image of n_windows + H - 1 rows (frame f of the chunk = row f),
 *   strips      the same layers run on n_windows + H - 2 band images of 2 * band rows: strip s = frames [s, s + 2 band) of the
 *               chunk, zero-padded above and below like a window.  Its upper band rows are the top rows of the window that
 *               STARTS at frame s; its lower band rows are the bottom rows of the window that ENDS at frame s + 2 band;
 * rows [0, band) of window w come from strip w, [H - band, H) from strip w + H - 2 band, the rest from the stream.  All three
 * in the shared-border PNHWC layout with row_bytes bytes per position (channels x element size, a multiple of 16).
 * Bit-identical to running the layers on every window in full (engine.predict_windows, tests/test_fullsize_gpu.py). */
int lad_assemble_windows(const void *stream_act, const void *strips, void *out, int64_t n_windows, int32_t H, int32_t W,
                         int32_t band, int32_t row_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * ResNetBigger forward / backward (models.py:82-115 ResidualBlock, :181-239 ResNetBigger; the autograd
 * backward of loss.backward() at train.py:289).  Activations are "PNHWC" with shared borders:
 * float[batch][H+1][W+1][C] followed by a tail of W+2 border rows, channels innermost; padded coordinates
 * (yp, xp) = (y+1, x+1); a "row" is one spatial position, lad_act_rows(batch, H, W) of them.  H, W always name the
 * UNPADDED image size.  INVARIANT: border positions (yp = 0, xp = 0, the tail) hold 0.0f in every tensor an entry
 * point reads; every entry point writes 0.0f there (or leaves them untouched where documented).
 * ---------------------------------------------------------------------------------------------- */

/* rows (spatial positions incl. borders and tail) of a (batch, H, W) activation tensor: allocate rows * channels elements */
int64_t lad_act_rows(int64_t batch, int32_t H, int32_t W);

/* Packed weight image consumed by the MFMA kernels.  w is the reference parameter (cout, cin, kh, kw)
 * with taps = kh*kw in {9, 1}.  mode 0: forward operand; mode 1: data-gradient operand (transposed,
 * spatially flipped).  nn.Conv2d.weight -> models.py:86-106,186-189. */
int64_t lad_conv_packed_weight_floats(int32_t cout, int32_t cin, int32_t taps, int32_t mode);
int lad_conv_pack_weights(const float *w, int32_t cout, int32_t cin, int32_t taps, int32_t mode, float *wt,
                          void *stream);
/* The same packing for many layers in one launch.  descs: DEVICE array of n_desc records
 * { const float *w; float *wt; int32_t cout, cin, taps, mode; } (32 bytes each). */
int lad_conv_pack_weights_multi(const void *descs, int32_t n_desc, void *stream);
/* number of 128-row tiles == rows of the (tile, 2, cout) BatchNorm partial-sum buffer a conv launch writes */
int64_t lad_conv_num_tiles(int64_t batch, int32_t H, int32_t W);
/* stride-1 convolution, 3x3 pad 1 (taps 9) or 1x1 (taps 1): out = conv(in, wt) + bias [+ addend], border rows
 * zeroed.  Used for nn.Conv2d forward (models.py:111-112) with a mode-0 image and for its data gradient with a
 * mode-1 image (then cin/cout are the GEMM K/N channel counts, i.e. swapped).  bias, addend, stat_partials
 * may be NULL.  stat_partials: float[num_tiles][2][cout] per-tile (sum, sum of squares) of the output. */
int lad_conv_fwd(const float *in, const float *wt, const float *bias, const float *addend, float *out,
                 float *stat_partials, int64_t batch, int32_t H, int32_t W, int32_t cin, int32_t cout, int32_t taps,
                 void *stream);
/* stride-2 convolution (3x3 pad 1 or 1x1 pad 0), input HxW -> output ceil(H/2) x ceil(W/2)
 * (models.py:86-89 with stride=2, :102-105 shortcut).  stat_partials sized by the OUTPUT geometry. */
int lad_conv_s2_fwd(const float *in, const float *wt, const float *bias, float *out, float *stat_partials,
                    int64_t batch, int32_t H, int32_t W, int32_t cin, int32_t cout, int32_t taps, void *stream);
/* Eval mode: the BatchNorm that follows a convolution (running statistics) folded into its epilogue.
 * lad_bn_fold: scale = gamma / sqrt(running_var + 1e-5), shift = beta + (conv_bias - running_mean) * scale
 * (nn.BatchNorm2d in eval mode after nn.Conv2d, models.py:110-115,224; conv_bias may be NULL).
 * lad_conv_fwd_eval / lad_conv_s2_fwd_eval: out = [relu](conv(in, wt) * scale + shift [+ addend]), mode-0 image. */
int lad_bn_fold(const float *gamma, const float *beta, const float *running_mean, const float *running_var,
                const float *conv_bias, int32_t channels, float *scale, float *shift, void *stream);
int lad_conv_fwd_eval(const float *in, const float *wt, const float *scale, const float *shift, const float *addend,
                      float *out, int64_t batch, int32_t H, int32_t W, int32_t cin, int32_t cout, int32_t taps,
                      int32_t relu, void *stream);
int lad_conv_s2_fwd_eval(const float *in, const float *wt, const float *scale, const float *shift, float *out,
                         int64_t batch, int32_t H, int32_t W, int32_t cin, int32_t cout, int32_t taps, int32_t relu,
                         void *stream);
/* zero-stuffing: up (HxW) <- src (ceil(H/2) x ceil(W/2)); turns a stride-2 conv's output gradient into the
 * operand of the stride-1 data-/weight-gradient kernels */
int lad_upsample2(const float *src, float *up, int64_t batch, int32_t H, int32_t W, int32_t channels, void *stream);
/* Backward of a stride-2 convolution (3x3 pad 1 or 1x1 pad 0; models.py:86-89 with stride 2, :102-105) at its true
 * cost, without zero-stuffing.  H, W: INPUT size; dout has the ceil(H/2) x ceil(W/2) geometry.
 * lad_conv_s2_dgrad: dx (input geometry, cin channels) from dout (cout channels) and the mode-1 packed image; every
 *   interior position of dx is written (accumulate = 0) or added to (accumulate = 1; required for the 1x1 shortcut,
 *   which only reaches the even/even positions); border positions are left as they are (zero by the layout invariant).
 * lad_conv_s2_wgrad: dw in the reference layout (cout, cin, kh, kw) (+ dbias, may be NULL). */
int lad_conv_s2_dgrad(const float *dout, const float *wt, float *dx, int64_t batch, int32_t H, int32_t W, int32_t cin,
                      int32_t cout, int32_t taps, int32_t accumulate, void *stream);
int64_t lad_conv_s2_wgrad_workspace_floats(int32_t cin, int32_t cout, int32_t taps);
int lad_conv_s2_wgrad(const float *in, const float *dout, float *workspace, float *dw, float *dbias, int64_t batch, int32_t H,
                      int32_t W, int32_t cin, int32_t cout, int32_t taps, void *stream);
/* The weight gradients of a stride-2 block's 3x3 convolution (dout) and of its 1x1 stride-2 shortcut (dout_sc, no bias)
 * in ONE launch: both convolutions read the same input and the shortcut's taps are the 3x3's centre-tap rows, so dw_sc
 * (cout, cin, 1, 1) rides along as a tenth tap.  Bit-identical to lad_conv_s2_wgrad(taps 9) + lad_conv_s2_wgrad(taps 1). */
int64_t lad_conv_s2_wgrad_fused_workspace_floats(int32_t cin, int32_t cout);
int lad_conv_s2_wgrad_fused(const float *in, const float *dout, const float *dout_sc, float *workspace, float *dw,
                            float *dbias, float *dw_sc, int64_t batch, int32_t H, int32_t W, int32_t cin, int32_t cout,
                            void *stream);
/* The same fusion in the other two directions.  lad_conv_s2_fwd_fused: the 3x3 stride-2 convolution (bias) and the 1x1
 * stride-2 shortcut (no bias) of one block in one launch, each with its own output and BatchNorm partials; the 3x3 part is
 * bit-identical to lad_conv_s2_fwd, the shortcut to lad_conv_s2_fwd(taps 1).  lad_conv_s2_dgrad_fused: the block's input
 * gradient dx = dgrad3x3(dout) + dgrad1x1(dout_sc), written once (the 1x1 lands on parity class (0,0) as one more tap);
 * equals lad_conv_s2_dgrad(taps 9, accumulate 0) + lad_conv_s2_dgrad(taps 1, accumulate 1) up to the order of one sum. */
int lad_conv_s2_fwd_fused(const float *in, const float *wt, const float *bias, const float *wt_sc, float *out,
                          float *stat_partials, float *out_sc, float *stat_partials_sc, int64_t batch, int32_t H, int32_t W,
                          int32_t cin, int32_t cout, void *stream);
int lad_conv_s2_dgrad_fused(const float *dout, const float *wt, const float *dout_sc, const float *wt_sc, float *dx,
                            int64_t batch, int32_t H, int32_t W, int32_t cin, int32_t cout, void *stream);
/* The 64 -> 32 stride-2 transition on the bf16 matrix cores with three-way split operands (csrc/conv_b3.hip, conv_s2b3:
 * the space-to-depth view of the input is formed while the rows are staged; fp32-equivalent arithmetic as lad_conv_b3*).
 * lad_conv_s2b3_pack_weights: w (32, 64, 3, 3) and w_sc (32, 64, 1, 1) -> one split image of
 * lad_conv_s2b3_packed_weight_bytes() bytes.  lad_conv_s2b3_fwd: same outputs and BatchNorm partials as
 * lad_conv_s2_fwd_fused(cin 64, cout 32). */
int64_t lad_conv_s2b3_packed_weight_bytes(void);
int lad_conv_s2b3_pack_weights(const float *w, const float *w_sc, void *wt, void *stream);
int lad_conv_s2b3_fwd(const float *in, const void *wt, const float *bias, float *out, float *stat_partials, float *out_sc,
                      float *stat_partials_sc, int64_t batch, int32_t H, int32_t W, void *stream);
/* Its data gradient dx = dgrad3x3(dout) + dgrad1x1(dout_sc) (= lad_conv_s2_dgrad_fused for 64 <- 32), parity class by parity
 * class with the result rows scattered to dx; border rows of dx are not written (zero by the layout invariant).  With
 * stat_partials != NULL also the first pass of the BatchNorm backward that consumes dx (as lad_conv_s2_dgrad_fused_bnstat:
 * input bn_x, sign bits bn_bits, coefficients bn_coef): float[lad_conv_s2b3_dgrad_partials(batch, H, W)][2][64]. */
int64_t lad_conv_s2b3_dgrad_packed_weight_bytes(void);
int lad_conv_s2b3_dgrad_pack_weights(const float *w, const float *w_sc, void *wt, void *stream);
/* lad_conv_s2b3_pack_weights + lad_conv_s2b3_dgrad_pack_weights in one launch (a training step needs both images). */
int lad_conv_s2b3_pack_weights_pair(const float *w, const float *w_sc, void *wt_fwd, void *wt_dgrad, void *stream);
int64_t lad_conv_s2b3_dgrad_partials(int64_t batch, int32_t H, int32_t W);
int lad_conv_s2b3_dgrad(const float *dout, const float *dout_sc, const void *wt, float *dx, float *stat_partials, const float *bn_x,
                        const uint64_t *bn_bits, const float *bn_coef, int64_t batch, int32_t H, int32_t W, void *stream);
/* ... and, for the 64 <- 32 transition, with the first pass of the BatchNorm backward that consumes dx (the bn2 of the
 * 64-channel block below: input bn_x, ReLU decisions from its sign bits bn_bits, coefficients bn_coef) in the epilogue:
 * stat_partials float[lad_conv_s2_dgrad_partials(batch, H, W)][2][64] -> lad_bn_bwd_bits pre_partials / pre_tiles. */
int64_t lad_conv_s2_dgrad_partials(int64_t batch, int32_t H, int32_t W);
int lad_conv_s2_dgrad_fused_bnstat(const float *dout, const float *wt, const float *dout_sc, const float *wt_sc, float *dx,
                                   float *stat_partials, const float *bn_x, const uint64_t *bn_bits, const float *bn_coef,
                                   int64_t batch, int32_t H, int32_t W, int32_t cin, int32_t cout, void *stream);
/* weight (+bias) gradient of a stride-1 conv: dw in the reference layout (cout, cin, kh, kw); dbias may be NULL.
 * GEOMETRY LIMIT: a tile stages 64 rows plus a halo of W+2 rows on either side in a fixed register/LDS budget, so for
 * cin = cout = 64 with 3x3 taps the image may be at most 46 columns wide (the model's widest map is 44, config.py:28-31);
 * wider images are refused with LAD_ERR_INVALID ("image too wide for the tile"), never computed wrongly
 * (tests/test_resnet_gpu.py::test_conv_s1_other_large_geometries). */
int64_t lad_conv_wgrad_workspace_floats(int32_t cin, int32_t cout, int32_t taps);
int lad_conv_wgrad(const float *in, const float *dout, float *workspace, float *dw, float *dbias, int64_t batch,
                   int32_t H, int32_t W, int32_t cin, int32_t cout, int32_t taps, void *stream);

/* 64 -> 64 3x3 stride-1 convolution (the four convolutions of block1, models.py:86-95, forward and data gradient) on the
 * bf16 matrix cores with fp32-equivalent arithmetic: every fp32 operand is the exact sum of three bf16 numbers and a
 * product keeps the six partial products above 2^-24 of it (csrc/conv_b3.hip).  Same f32 output tensor, bias / addend /
 * border / BatchNorm-partial semantics as lad_conv_fwd.  Since round 4 this is the FALLBACK generation of the split-operand
 * layers (engine.f16x2 = False / bench.py --no-h2; the product path is lad_conv_h2 below).
 *   lad_conv_b3_pack_weights: w (64, 64, 3, 3) fp32 -> split, MFMA-ordered image; mode 0 forward, 1 data gradient. */
int64_t lad_conv_b3_packed_weight_bytes(void);
int lad_conv_b3_pack_weights(const float *w, int32_t mode, void *wt, void *stream);
/* the convolution on the ordinary fp32 tensor (float[rows][64]): the three-way split happens while a stage of input
 * rows is staged into LDS, so producers and the other consumers of the tensor are untouched */
int lad_conv_b3_fwd_f32(const float *in, const void *wt, const float *bias, const float *addend, float *out,
                        float *partials, int64_t batch, int32_t H, int32_t W, void *stream);
/* out = conv(in) + bias + addend * [addend_bits]: lad_conv_b3_fwd_f32 whose addend is gated by the sign bits of an
 * activation (lad_bn_act_bits) -- the data gradient of a residual block's first convolution plus the identity shortcut's
 * share dy * [y > 0], taken from dy itself.  out may be the addend's own buffer (each 16 bytes are read, then written, by
 * the same thread). */
int lad_conv_b3_fwd_f32_gated(const float *in, const void *wt, const float *bias, const float *addend,
                              const uint64_t *addend_bits, float *out, float *partials, int64_t batch, int32_t H,
                              int32_t W, void *stream);
/* the data gradient (no bias; addend / addend_bits optional, as above) fused with the first pass of the BatchNorm
 * backward that consumes it: stat_partials float[lad_conv_num_tiles][2][64] = per 128-row tile (sum dz, sum dz*xhat) of
 * that BatchNorm (input bn_x, coefficients bn_coef float[6][64]; its ReLU decisions from the sign bits bn_bits or,
 * bn_bits = NULL, recomputed from bn_x as lad_bn_bwd relu = 2 does) -> lad_bn_bwd / lad_bn_bwd_bits pre_partials. */
int lad_conv_b3_dgrad_bnstat(const float *in, const void *wt, const float *addend, const uint64_t *addend_bits,
                             float *out, float *stat_partials, const float *bn_x, const uint64_t *bn_bits,
                             const float *bn_coef, int64_t batch, int32_t H, int32_t W, void *stream);
/* The split-operand convolution for `channels` = 64 or 32 (32: block2's three stride-1 3x3 convolutions, forward and data
 * gradient): packed image size / packing / forward (fp32 input, optional bias and addend, BatchNorm partials) / data
 * gradient with the consuming BatchNorm's sums (ReLU decisions recomputed from bn_x), as the 64-channel entry points
 * above.  Sign bits exist for 64 channels only. */
int64_t lad_conv_b3c_packed_weight_bytes(int32_t channels);
int lad_conv_b3c_pack_weights(const float *w, int32_t mode, void *wt, int32_t channels, void *stream);
int lad_conv_b3c_fwd_f32(const float *in, const void *wt, const float *bias, const float *addend, float *out,
                         float *partials, int64_t batch, int32_t H, int32_t W, int32_t channels, void *stream);
int lad_conv_b3c_dgrad_bnstat(const float *in, const void *wt, const float *addend, float *out, float *stat_partials,
                              const float *bn_x, const float *bn_coef, int64_t batch, int32_t H, int32_t W,
                              int32_t channels, void *stream);
int lad_conv_b3c_fwd_f32_bnrelu(const float *in, const float *in_coef, const void *wt, const float *bias, float *out,
                                float *partials, int64_t batch, int32_t H, int32_t W, int32_t channels, void *stream);
/* ---- "f16 x 2": the same 64 -> 64 / 32 -> 32 3x3 stride-1 convolutions (models.py:86-96,110-115) on TWO f16 planes per
 * operand, three plane products per fp32-equivalent product (csrc/conv_h2.hip: block floating point per staged tile, the
 * power-of-two scales live inside the kernels and the packed image).  Round 4; replaces lad_conv_b3c_* on the training path.
 * lad_conv_h2_pack_weights_multi: `table` = device array of n records {const float *w; void *wt; int32_t mode; int32_t channels}
 * (mode 0 forward, 1 data gradient; wt holds lad_conv_h2_packed_weight_bytes(channels) bytes; the record's `channels` is read only
 * when the call's `channels` is 0: then the table may mix 64- and 32-channel layers -- one launch per step instead of two).
 * lad_conv_h2: out = conv3x3(act(in)) + bias + addend * [addend_bits];  in_coef != NULL: act = relu(BatchNorm(in)) formed
 * while staging (lad_conv_b3c_fwd_f32_bnrelu);  bn_x != NULL: `partials` receives the sums of the BatchNorm backward that
 * consumes out (lad_conv_b3_dgrad_bnstat), else (sum, sum of squares) of out per 128-row tile, or nothing when NULL.
 * Tile: 256 rows at two workgroups per CU, or 128 rows at three for launches of fewer than two dispatch rounds (chosen by the
 * launcher; the other structures that were measured are built from tools/experiments/retired/ by tools/exp_h2.sh). */
int64_t lad_conv_h2_packed_weight_bytes(int32_t channels);
int lad_conv_h2_pack_weights_multi(const void *table, int32_t n, int32_t channels, void *stream);
/* weight (+ bias) gradient of the 64-channel convolutions on the same arithmetic; arguments as lad_conv_wgrad_b3c. */
int lad_conv_wgrad_h2(const float *in, const float *in_coef, const float *dout, float *workspace, float *dw, float *dbias,
                      int64_t batch, int32_t H, int32_t W, int32_t channels, void *stream);
/* The same weight gradient with the BatchNorm backward of this convolution's output on its gradient side: dy = the gradient
 * arriving at the BatchNorm(+ReLU) that follows the convolution, bn_x = that BatchNorm's input (the convolution's output),
 * bn_coef / bcoef = its forward / backward coefficients (lad_bn_finalize; lad_bn_bwd or lad_bn_bwd_bits called with dx = NULL),
 * bn_bits = sign bits of the block output (lad_bn_act_bits) or NULL (ReLU decisions recomputed from bn_x).  Writes
 * dc = the BatchNorm's input gradient -- what lad_bn_bwd would have written to dx, bit for bit -- for the data-gradient launch,
 * and accumulates dw / dbias from it.  Replaces the reference's autograd nodes NativeBatchNormBackward + ConvolutionBackward
 * (weight) of models.py:86-96 in loss.backward() (train.py:289). */
int lad_conv_wgrad_h2_bnbwd(const float *in, const float *in_coef, const float *dy, const float *bn_x, const uint64_t *bn_bits,
                            const float *bn_coef, const float *bcoef, float *dc, float *workspace, float *dw, float *dbias,
                            int64_t batch, int32_t H, int32_t W, int32_t channels, void *stream);
int lad_conv_h2(const float *in, const float *in_coef, const void *wt, const float *bias, const float *addend,
                const uint64_t *addend_bits, float *out, float *partials, const float *bn_x, const uint64_t *bn_bits,
                const float *bn_coef, int64_t batch, int32_t H, int32_t W, int32_t channels, void *stream);
/* weight (+ bias) gradient of the same convolutions for 64 or 32 channels; in_coef = NULL: `in` is the stored activation,
 * otherwise relu(BatchNorm(in)) is formed while staging (lad_conv_wgrad_b3_bnrelu).  32 channels: W <= 30. */
int64_t lad_conv_wgrad_b3c_workspace_floats(int32_t channels);
int lad_conv_wgrad_b3c(const float *in, const float *in_coef, const float *dout, float *workspace, float *dw, float *dbias,
                       int64_t batch, int32_t H, int32_t W, int32_t channels, void *stream);
/* Forward convolution / weight gradient whose input is relu(BatchNorm(in)), in_coef = that BatchNorm's float[6][64] from
 * lad_bn_finalize: the second convolution of a residual block (models.py:110-112) reading the FIRST one's raw output;
 * scale, shift, ReLU and the zero border are applied while the rows are staged into LDS, with the fmaf / max of lad_bn_act,
 * so the results are bit-identical to lad_bn_act + lad_conv_b3_fwd_f32 / lad_conv_wgrad_b3 and the activation between
 * the two convolutions is never written or read (596 MB each way at batch 512). */
int lad_conv_b3_fwd_f32_bnrelu(const float *in, const float *in_coef, const void *wt, const float *bias, float *out,
                               float *partials, int64_t batch, int32_t H, int32_t W, void *stream);
int lad_conv_wgrad_b3_bnrelu(const float *in, const float *in_coef, const float *dout, float *workspace, float *dw,
                             float *dbias, int64_t batch, int32_t H, int32_t W, void *stream);
/* Deferred sums.  Every weight-gradient entry point (lad_conv_wgrad, lad_conv_wgrad_b3[_bnrelu], lad_conv_s2_wgrad) ends
 * with a small launch that sums its per-workgroup partial slabs (in `workspace`) into dw / dbias.  Between
 * lad_wgrad_defer_begin() and lad_wgrad_defer_flush(stream) those launches are queued instead, and the flush sums all
 * queued layers in ONE launch on `stream` (which must be ordered after the weight-gradient launches): 19 dependent
 * launches per training step become one.  Each deferred call must have been given its OWN workspace (checked) -- the
 * slabs stay there until the flush; dw / dbias are undefined until then.  Process-wide state, not thread-safe: one
 * engine per process, as the data-parallel design has it. */
int lad_wgrad_defer_begin(void);
int lad_wgrad_defer_flush(void *stream);
/* weight (+bias) gradient of the same 64 -> 64 3x3 convolution with the same split arithmetic (csrc/wgrad_mfma.hip:
 * K = rows, so both operands come out of LDS through transposing reads); arguments and workspace
 * (lad_conv_wgrad_workspace_floats(64, 64, 9)) as lad_conv_wgrad; images up to 46 columns wide */
int lad_conv_wgrad_b3(const float *in, const float *dout, float *workspace, float *dw, float *dbias, int64_t batch,
                      int32_t H, int32_t W, void *stream);

/* stem conv3x3 1->64, no bias (models.py:186-189,224).  feat: float[batch][H][W] (the (B,1,100,44) input). */
int lad_stem_fwd(const float *feat, const float *weight, float *out, float *stat_partials, int64_t batch, int32_t H,
                 int32_t W, int32_t cout, void *stream);
/* eval-mode stem with bn1 + ReLU folded in, reading image b as frames [b*frame_stride, b*frame_stride + H) of a
 * (frames, W) feature matrix; frames >= frames_avail read as 0.  frame_stride = 1: the stride-one-frame windows of
 * InferenceDataset (datasets.py:72-93) taken straight from the whole-file features (load_data.py:49-53);
 * frame_stride = H: ordinary (batch, H, W) input. */
int lad_stem_fwd_eval(const float *feat, const float *weight, const float *scale, const float *shift, float *out,
                      int64_t batch, int32_t H, int32_t W, int32_t cout, int64_t frame_stride, int64_t frames_avail,
                      void *stream);
/* Round 6: the stem's batch statistics and its backward from MOMENTS of the input.  The stem convolution has one input channel, so
 * sum x_c and sum x_c^2 over the batch are combinations of F1[t] = sum f_t and F2[t][u] = sum f_t f_u of the nine taps (54 numbers).
 * lad_stem_bn_stats = lad_stem_fwd(out = NULL) + lad_bn_finalize from ONE pass over the features (no 64-channel pass): coef as
 * lad_bn_finalize writes it (the sums are those of the unrounded convolution: the coefficients agree to ~1e-7 relative), running
 * statistics updated; `moments` (lad_stem_moments_doubles() doubles) keeps the totals for the backward pass, `workspace` holds
 * lad_stem_moments_workspace_doubles() doubles.
 * lad_stem_bwd_onepass = lad_stem_bn_bwd_sums + lad_bn_bwd(dx = NULL, relu = 2) + lad_stem_wgrad_bn(x = NULL) with ONE pass over dy
 * instead of two: dw (64, 1, 3, 3), dgamma, dbeta of models.py:186-190,224; workspace: lad_stem_bwd_onepass_workspace_floats(). */
int64_t lad_stem_moments_workspace_doubles(void);
int64_t lad_stem_moments_doubles(void);
int lad_stem_bn_stats(const float *feat, const float *weight, const float *gamma, const float *beta, float *running_mean,
                      float *running_var, float momentum, float *coef, double *moments, double *workspace, int64_t batch, int32_t H,
                      int32_t W, int32_t cout, void *stream);
int64_t lad_stem_bwd_onepass_workspace_floats(void);
int lad_stem_bwd_onepass(const float *feat, const float *weight, const float *dy, const float *coef, const float *gamma,
                         const double *moments, float *workspace, float *dw, float *dgamma, float *dbeta, int64_t batch, int32_t H,
                         int32_t W, int32_t cout, void *stream);
int64_t lad_stem_wgrad_workspace_floats(void);
int lad_stem_wgrad(const float *feat, const float *dout, float *workspace, float *dw, int64_t batch, int32_t H,
                   int32_t W, int32_t cout, void *stream);
/* The same with the stem BatchNorm's backward applied on the fly: dy is the gradient wrt the BatchNorm(+ReLU) output, coef
 * the BatchNorm's float[6][C] forward coefficients and bcoef the float[8][C] backward coefficients left by
 * lad_bn_bwd(..., dx = NULL, ..., relu = 2, mode = 0).  x is the stem convolution's output (the BatchNorm input) if the
 * caller kept it, or NULL: then it is recomputed from feat and weight (the forward's own fmaf chain, bit-identical).
 * The stem needs no data gradient (models.py:224 is the first layer), so the BatchNorm's input gradient is never
 * materialised -- and with x = NULL neither is the convolution output: lad_stem_fwd(out = NULL) gives the batch statistics,
 * lad_stem_fwd_eval(scale = coef, shift = coef + C) the activated output, lad_stem_bn_bwd_sums the backward sums. */
int lad_stem_wgrad_bn(const float *feat, const float *dy, const float *x, const float *weight, const float *coef,
                      const float *bcoef, float *workspace, float *dw, int64_t batch, int32_t H, int32_t W, int32_t cout,
                      void *stream);
/* per workgroup (sum dz, sum dz*xhat) per channel of the stem BatchNorm's backward, x recomputed from feat and weight:
 * partials float[lad_stem_bn_bwd_groups(batch,H,W)][2][C], to be handed to lad_bn_bwd as pre_partials / pre_tiles */
int64_t lad_stem_bn_bwd_groups(int64_t batch, int32_t H, int32_t W);
int lad_stem_bn_bwd_sums(const float *feat, const float *weight, const float *dy, const float *coef, float *partials,
                         int64_t batch, int32_t H, int32_t W, int32_t cout, void *stream);

/* BatchNorm2d (+ residual + ReLU), train and eval (models.py:90,98,106,190; eps 1e-5, momentum 0.1).
 * coef: float[6][C] = scale, shift, mean, invstd, mean_lo, invstd_lo (hi + lo = the double-precision value; the
 * backward pass needs the extra bits, csrc/bn.hip).  count = batch*H*W (positions per channel).
 * stat_partials (float[n_tiles][2][C] from the convolution / stem epilogues) is CONSUMED: large layers reduce it in
 * place in two levels. */
int lad_bn_finalize(float *stat_partials, int64_t n_tiles, int32_t channels, int64_t count, const float *gamma,
                    const float *beta, float *running_mean, float *running_var, float momentum, float *coef,
                    void *stream);
/* Round 6: lad_bn_finalize for the TWO BatchNorm layers behind a stride-2 block's fused conv1 + shortcut launch (bn1 and the
 * shortcut's BatchNorm, models.py:98-106: sums of the same shape) in one launch; the same results as two calls. */
int lad_bn_finalize_pair(float *stat_partials_a, float *stat_partials_b, int64_t n_tiles, int32_t channels, int64_t count,
                         const float *gamma_a, const float *beta_a, float *running_mean_a, float *running_var_a, float *coef_a,
                         const float *gamma_b, const float *beta_b, float *running_mean_b, float *running_var_b, float *coef_b,
                         float momentum, void *stream);
/* y = act(x*scale + shift [+ res | + res*rscale + rshift]) on the interior of a (batch, H, W, channels) PNHWC tensor;
 * border positions of y are written as zero (the layout invariant the MFMA kernels rely on) */
int lad_bn_act(const float *x, const float *coef, const float *res, const float *res_coef, float *y, int64_t batch,
               int32_t H, int32_t W, int32_t channels, int32_t relu, void *stream);
/* backward of the above; relu 0: none, 1: mask = (y > 0), 2 (mode 0 only): mask recomputed as (x*scale+shift > 0), y
 * not read; mode 0: dx; 1: dx and aux = dz (identity shortcut); 2: dx and aux = gradient into the
 * shortcut BatchNorm's input.  bcoef: float[8][C] scratch, workspace: lad_bn_bwd_workspace_floats(C) floats.
 * dx = NULL (mode 0 only): only dgamma, dbeta and bcoef are produced -- for a consumer that applies bcoef itself
 * (lad_stem_wgrad_bn); with pre_partials given as well, x may be NULL (it is not read).
 * pre_partials (float[pre_tiles][2][C], from a producer that reduced while it wrote dy) is CONSUMED: 8192 tiles or more
 * are summed in place in two levels, as lad_bn_finalize does. */
int64_t lad_bn_bwd_workspace_floats(int32_t channels);
int lad_bn_bwd(const float *dy, const float *y, const float *x, const float *coef, const float *gamma,
               const float *xs, const float *scoef, const float *sgamma, float *dx, float *aux, float *dgamma,
               float *dbeta, float *dsgamma, float *dsbeta, float *workspace, float *bcoef, float *pre_partials,
               int64_t pre_tiles, int64_t batch, int32_t H, int32_t W, int32_t channels, int32_t relu, int32_t mode,
               void *stream);
/* Sign-bit flavour for the 64-channel residual blocks (replaces the `out = F.relu(out + shortcut)` mask that autograd
 * keeps for models.py:113-114).  lad_bn_act_bits = lad_bn_act(relu = 1) that also leaves y_bits: one uint64 per row of
 * y (lad_act_rows(batch, H, W) words; bit k*16 + j <-> channel 4*j + k is set iff y > 0).  lad_bn_bwd_bits = lad_bn_bwd
 * (relu = 1, mode 0) that takes the ReLU decisions from y_bits instead of reading y, and writes dx only: the masked
 * gradient dy * [y > 0] the identity shortcut carries is formed by its consumer, lad_conv_b3_fwd_f32_gated, from dy and
 * the same bits.  Per residual block the backward pass moves three activation-sized tensors less. */
int lad_bn_act_bits(const float *x, const float *coef, const float *res, const float *res_coef, float *y,
                    uint64_t *y_bits, int64_t batch, int32_t H, int32_t W, int32_t channels, void *stream);
int lad_bn_bwd_bits(const float *dy, const uint64_t *y_bits, const float *x, const float *coef, const float *gamma,
                    float *dx, float *dgamma, float *dbeta, float *workspace, float *bcoef, float *pre_partials,
                    int64_t pre_tiles, int64_t batch, int32_t H, int32_t W, int32_t channels, void *stream);
/* Data gradient of a stride-1 3x3 convolution (mode-1 image; cin/cout = GEMM K/N channels) fused with the FIRST pass of
 * the BatchNorm backward that consumes it: stat_partials receives, per 128-row tile, (sum dz, sum dz*xhat) of that
 * BatchNorm (input bn_x, output bn_y or NULL = mask recomputed from bn_x, coefficients bn_coef float[6][C]); pass it to
 * lad_bn_bwd as pre_partials with pre_tiles = lad_conv_num_tiles(...) (modes 0 and 1) and the reduce pass is skipped. */
int lad_conv_fwd_bnstat(const float *in, const float *wt, const float *addend, float *out, float *stat_partials,
                        const float *bn_x, const float *bn_y, const float *bn_coef, int64_t batch, int32_t H, int32_t W,
                        int32_t cin, int32_t cout, int32_t taps, void *stream);

/* Head: AvgPool2d(4) -> flatten -> bn2 -> dropout -> linear1 -> bn3 -> dropout -> ReLU -> linear2 -> sigmoid
 * (models.py:229-238) fused with nn.BCELoss and the _calc_metrics counters (train.py:203-224,279-285).
 * params: HOST array of 12 device pointers (bn2.weight, bn2.bias, bn2.running_mean, bn2.running_var,
 * linear1.weight, linear1.bias, bn3.weight, bn3.bias, bn3.running_mean, bn3.running_var, linear2.weight,
 * linear2.bias).  drop1/drop2: masks already scaled by 1/(1-p), or NULL.  stats: float[2F+64] saved for
 * backward; metrics: float[8] = mean BCE, #correct, #pred positive, #true positive, #target positive, B. */
int lad_pool_fwd(const float *x, float *pooled, int64_t batch, int32_t H, int32_t W, int32_t channels, void *stream);
int lad_pool_bwd(const float *dpooled, float *dx, int64_t batch, int32_t H, int32_t W, int32_t channels, void *stream);
int64_t lad_head_workspace_floats(int64_t batch, int32_t F);
int lad_head_fwd_train(const float *const *params, const float *pooled, int64_t batch, int32_t F, const float *drop1,
                       const float *drop2, const int32_t *labels, float momentum, float *h, float *stats,
                       float *probs, float *metrics, void *stream);
/* The same with the dropout masks drawn INSIDE the launch (round 6): drop1 / drop2 are output buffers here (what lad_head_bwd then takes),
 * values 0 or 1 / keep from Philox4x32-10 keyed by `seed` at draw number *rng_counter (device int64, incremented by the kernel: graph
 * replays draw fresh masks); keep >= 1 = no dropout.  nbt: n_nbt device int64 counters incremented by one (the BatchNorm layers'
 * num_batches_tracked, which a train-mode forward advances), or NULL.  Replaces nn.Dropout's mask generation of models.py:232,235
 * (four torch launches per step) and the counter increment (one more). */
int lad_head_fwd_train_rng(const float *const *params, const float *pooled, int64_t batch, int32_t F, float *drop1, float *drop2, float keep,
                           uint64_t seed, int64_t *rng_counter, int64_t *nbt, int32_t n_nbt, const int32_t *labels, float momentum,
                           float *h, float *stats, float *probs, float *metrics, void *stream);
int lad_head_fwd_eval(const float *const *params, const float *pooled, int64_t batch, int32_t F, float *probs,
                      void *stream);
/* nn.BCELoss (mean, log clamped at -100) + the _calc_metrics counters for eval-mode probabilities (train.py:226-259):
 * metrics float[8] = mean BCE, #correct, #pred positive, #true positive, #target positive, n */
int lad_bce_metrics(const float *probs, const int32_t *labels, int64_t n, float *metrics, void *stream);
/* grads: HOST array of 8 device pointers (d bn2.weight, d bn2.bias, d linear1.weight, d linear1.bias, d bn3.weight,
 * d bn3.bias, d linear2.weight, d linear2.bias).  dprobs NULL = loss is the mean BCE against labels. */
int lad_head_bwd(const float *const *params, float *const *grads, const float *pooled, const float *h,
                 const float *stats, const float *probs, const float *dprobs, int64_t batch, int32_t F,
                 const float *drop1, const float *drop2, const int32_t *labels, float *workspace, float *dpooled,
                 void *stream);

/* ------------------------------------------------------------------------------------------------
 * fp16 inference path (eval mode; BASELINE configs[4]): half activations (PNHWC, zero border ring) and half weights,
 * f32 accumulation on the 16-bit matrix cores, BatchNorm folded in (scale/shift from lad_bn_fold).  Same layers as
 * lad_stem_fwd_eval / lad_conv_fwd_eval / lad_conv_s2_fwd_eval / lad_pool_fwd; `void*` activations are _Float16.
 * ---------------------------------------------------------------------------------------------- */
int64_t lad_f16_packed_weight_halfs(int32_t cout, int32_t cin, int32_t taps);
int lad_f16_pack_weights(const float *w, int32_t cout, int32_t cin, int32_t taps, void *wt, void *stream);
int lad_f16_stem_fwd(const float *feat, const float *weight, const float *scale, const float *shift, void *out,
                     int64_t batch, int32_t H, int32_t W, int32_t cout, int64_t frame_stride, int64_t frames_avail,
                     void *stream);
/* (16 channels with an addend, relu and >= 512 images small enough for a CU's LDS: the call runs block_f16_small_kernel's
 * one-convolution form -- several images per workgroup, weights resident -- instead of the tiled kernel; identical results.) */
int lad_f16_conv_fwd(const void *in, const void *wt, const float *scale, const float *shift, const void *addend, void *out,
                     int64_t batch, int32_t H, int32_t W, int32_t cin, int32_t cout, int32_t taps, int32_t relu,
                     void *stream);
int lad_f16_conv_s2_fwd(const void *in, const void *wt, const float *scale, const float *shift, void *out, int64_t batch,
                        int32_t H, int32_t W, int32_t cin, int32_t cout, int32_t taps, int32_t relu, void *stream);
/* One residual block with the identity shortcut, 16 / 32 / 64 channels, in ONE launch with each image resident in a CU's LDS (round 5):
 *   y = relu(bn2(conv2(relu(bn1(conv1(x))))) + x)     -- models.py:110-115 (ResidualBlock.forward) in eval mode, BatchNorms folded.
 * wt1 / wt2: lad_f16_pack_weights images of the two 3x3 convolutions; x, y: shared-border half tensors of `batch` H x W images, y != x.
 * channels 64: covers (H + 1)(W + 1) <= 512 positions with (H + 1)(W + 1) + W <= 562 (LDS) and batch >= 256 (the boundary strips of the
 * sliding-window path: segment_laughter.py:90-101 through engine._forward_eval_stream).  channels 16 / 32: several images per workgroup,
 * both weight images resident in LDS; covers batch >= 512 images small enough that two of their tensors fit 160 KB next to the weights
 * (the windows at resolution levels 3 and 4, the strips of level 2).  Any other geometry returns LAD_NOT_COVERED with nothing launched
 * (no error string) and the caller runs the two convolutions by lad_f16_conv_fwd.  Results are bit-identical to that pair of calls.
 * Trailing rows: like every shared-border tensor, x ends in W + 2 zero rows behind its last image (the rows below the last image's
 * last row: the block reads them as that image's lower border) -- the caller provides them.  The 64-channel form does NOT write
 * y's trailing rows (lad_f16_conv_fwd does): a y that a later launch reads as an image sequence must have had them zeroed once. */
int lad_f16_block_fwd(const void *x, const void *wt1, const float *scale1, const float *shift1, const void *wt2,
                      const float *scale2, const float *shift2, void *y, int64_t batch, int32_t H, int32_t W, int32_t channels,
                      void *stream);
/* Round 6: lad_f16_stem_fwd + lad_f16_block_fwd (64 channels) for the FIRST residual block of the sliding-window strips in ONE launch
 * (models.py:224 + :110-115 in eval mode): strip b = frames [b, b + H) of `feat` ((frames, W) float32, zero-padded above and below, zeros
 * from frames_avail on).  The stem of a strip's rows 1 .. H - 2 is not recomputed: it is read from rows stream_row0 + b + 1 .. of
 * `stream_act` = lad_f16_stem_fwd over the whole frame stream as ONE image of stream_rows rows (frame 0 of `feat` is its frame
 * stream_row0); rows 0 and H - 1 -- the ones that see the strip's own padding -- are computed inside the launch from stem_weight
 * (conv1.weight) and the folded bn1 (stem_scale, stem_shift).  No strip-sized stem tensor is written or read.  Results identical to the
 * two calls; LAD_NOT_COVERED (nothing launched) outside lad_f16_block_fwd's 64-channel coverage or when W > 64 (a lane per column). */
int lad_f16_block_fwd_stem_rows(const void *stream_act, int64_t stream_rows, int64_t stream_row0, const float *feat, int64_t frames_avail,
                                const float *stem_weight, const float *stem_scale, const float *stem_shift, const void *wt1,
                                const float *scale1, const float *shift1, const void *wt2, const float *scale2, const float *shift2, void *y,
                                int64_t batch, int32_t H, int32_t W, void *stream);
/* Round 6: lad_f16_conv_s2_fwd_mapped_sc for the LEVEL-2 STRIPS (phases = 1, cin = 64, cout = 32, relu = 1, out_rows > 0: block2.0's
 * 3x3 stride-2 convolution -> out and its 1x1 shortcut -> out_sc, models.py:98-106, on the strip images of engine._eval_level2_shared)
 * with the input rows resident in LDS as parity classes (filled by LDS-DMA, a third of a strip image at a time, double-buffered) instead
 * of gathered per lane.  Same arguments; identical results on every output a window uses.  LAD_NOT_COVERED (nothing launched) for
 * other geometries than W = 44, out_rows = 12: the caller issues lad_f16_conv_s2_fwd_mapped_sc. */
int lad_f16_conv_s2_strips_fwd(const void *act, const void *wt, const float *scale, const float *shift, void *out, const void *wt_sc,
                               const float *scale_sc, const float *shift_sc, void *out_sc, int64_t n_windows, int32_t H, int32_t W,
                               int32_t band, int32_t strip_rows, int64_t bottom_image0, int64_t stream_row0, int64_t act_rows,
                               int32_t out_rows, void *stream);
/* Round 6: EVERYTHING BEHIND THE SHARED LEVEL 2 of the fp16 sliding-window path in ONE launch -- block3.0 (3x3 stride 2 through the
 * window map + 1x1 shortcut + conv2), block3.1, block4.0, block4.1, AvgPool2d(4) and the classifier, one probability per window:
 * models.py:226-239 in eval mode for the windows of segment_laughter.py:90-101.  `act`, H, W, band, strip_rows, bot_img0, stream_row0,
 * phases (2), phase_img, act_rows: exactly what lad_f16_conv_s2_fwd_mapped takes for the level-2 buffer (32 channels).  conv_params: HOST
 * array of 30 device pointers = {lad_f16_pack_weights image, folded scale, folded shift} of block3.0 conv1, block3.0 shortcut, block3.0
 * conv2, block3.1 conv1, block3.1 conv2 and the same five of block4 (16 channels); head_params, F: as lad_head_fwd_eval.  One
 * 1024-thread workgroup per CU keeps a window in LDS from its level-2 rows to its probability.  Bit-identical to the launches it replaces
 * (lad_f16_conv_s2_fwd_mapped(_sc), lad_f16_conv_fwd, lad_f16_block_fwd, lad_f16_conv_s2_fwd_sc, lad_f16_pool_fwd, lad_head_fwd_eval).
 * Returns LAD_NOT_COVERED (nothing launched) when a window does not fit a CU's LDS or H / W are odd: the caller issues those launches. */
int lad_f16_tail_fwd(const void *act, int64_t n_windows, int32_t H, int32_t W, int32_t band, int32_t strip_rows, int64_t bot_img0,
                     int64_t stream_row0, int32_t phases, int64_t phase_img, int64_t act_rows, const void *const *conv_params,
                     const float *const *head_params, int32_t F, float *probs, void *stream);
/* The stride-2 convolutions behind the level-1 layers in the sliding-window path (engine._forward_eval_stream), reading every
 * window's rows from where they lie -- `act` = the n_windows + H - 2 band strip images of 2 * band rows followed by the stream image
 * of n_windows + H - 1 rows (the operands of lad_assemble_windows, in ONE buffer) -- instead of from an assembled copy: identical
 * results, one 1.2 GB write + read per 2048 windows less.  (cin, cout, taps) = (64, 32, 9) or (64, 32, 1). */
int lad_f16_conv_s2_fwd_windows(const void *act, const void *wt, const float *scale, const float *shift, void *out,
                                int64_t n_windows, int32_t H, int32_t W, int32_t band, int32_t cin, int32_t cout, int32_t taps,
                                int32_t relu, void *stream);
/* The general form (round 3: the SECOND resolution level is shared between the windows too).  `act` (act_rows rows of cin halfs)
 * holds strip images of strip_rows rows -- window b's rows [0, strip_rows) in image b, its rows [H - strip_rows, H) in image
 * bottom_image0 + b (n_windows for strips of their own, H - strip_rows where one strip serves two windows as in
 * lad_assemble_windows) -- of which the first / last `band` rows are used, and, from row stream_row0 on, the stream image(s)
 * every other row comes from:
 * phases 1: row y of window b is stream row b + y; phases 2 (the input level lies behind a stride-2 layer, so windows of even
 * and odd b see different samplings): two stream images phase_rows rows apart, row y of window b = row (b >> 1) + y of image
 * b & 1.  out_rows 0: whole windows out (n_windows images of (H + 1) / 2 rows).  out_rows > 0 (even; H even; phases 1; paired
 * input strips): the NEXT level's strips out, paired the same way -- n_windows + 2 (H / 2 - out_rows) images of out_rows rows,
 * image s = the first out_rows / 2 output rows of window s over the last out_rows / 2 of window s - 2 (H / 2 - out_rows).
 * (cin, cout) = (64, 32) or (32, 16), taps 9 or 1. */
int lad_f16_conv_s2_fwd_mapped(const void *act, const void *wt, const float *scale, const float *shift, void *out,
                               int64_t n_windows, int32_t H, int32_t W, int32_t band, int32_t strip_rows, int64_t bottom_image0,
                               int64_t stream_row0, int32_t phases, int64_t phase_rows, int64_t act_rows, int32_t out_rows,
                               int32_t cin, int32_t cout, int32_t taps, int32_t relu, void *stream);
/* A down-sampling block's conv1 (3x3 stride 2 + BatchNorm + ReLU -> out) and its 1x1 stride-2 shortcut (+ BatchNorm -> out_sc) in ONE
 * launch (round 5): the shortcut reads exactly the rows the 3x3's centre tap gathers (models.py:98-106, eval mode).  Identical bits to
 * lad_f16_conv_s2_fwd(taps 9, relu) + lad_f16_conv_s2_fwd(taps 1, relu 0) / the two lad_f16_conv_s2_fwd_mapped calls on the same input.
 * (cin, cout) = (64, 32), (32, 16), and for the plain form (16, 16); wt_sc: lad_f16_pack_weights(taps = 1); out_sc != out. */
int lad_f16_conv_s2_fwd_sc(const void *in, const void *wt, const float *scale, const float *shift, void *out, const void *wt_sc,
                           const float *scale_sc, const float *shift_sc, void *out_sc, int64_t batch, int32_t H, int32_t W,
                           int32_t cin, int32_t cout, int32_t relu, void *stream);
int lad_f16_conv_s2_fwd_mapped_sc(const void *act, const void *wt, const float *scale, const float *shift, void *out,
                                  const void *wt_sc, const float *scale_sc, const float *shift_sc, void *out_sc, int64_t n_windows,
                                  int32_t H, int32_t W, int32_t band, int32_t strip_rows, int64_t bottom_image0, int64_t stream_row0,
                                  int32_t phases, int64_t phase_rows, int64_t act_rows, int32_t out_rows, int32_t cin, int32_t cout,
                                  int32_t relu, void *stream);
int lad_f16_pool_fwd(const void *x, float *pooled, int64_t batch, int32_t H, int32_t W, int32_t channels, void *stream);

/* clip_grad_norm_ + Adam + zero_grad on a flat buffer (train.py:291-295) */
int32_t lad_grad_sumsq_partials(void);
/* step_counter (DEVICE int64, may be NULL): lad_grad_sumsq increments it, lad_adam_step then takes the step number
 * for the bias corrections from it instead of the host argument `step` -- what a captured hipGraph needs. */
int lad_grad_sumsq(const float *grad, int64_t n, float *partials, int64_t *step_counter, void *stream);
/* acc += scale * grad: gradient accumulation over batches (train.py:287-289, loss / gradient_accumulation_steps). */
int lad_grad_accumulate(float *acc, const float *grad, int64_t n, double scale, void *stream);
int lad_adam_step(float *param, float *grad, float *exp_avg, float *exp_avg_sq, int64_t n,
                  const float *sumsq_partials, double grad_scale, double max_norm, double lr, double beta1,
                  double beta2, double eps, int64_t step, const int64_t *step_counter, int32_t zero_grad,
                  float *norm_out, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Threshold sweep of a probability track on the device: run tables for K thresholds in one pass.
 * Replaces the per-frame loop of get_laughter_instances (laugh_segmenter.py:74-111, with fix_over_underflow :57-71) up to
 * the integer run table: p > 1 -> 1, p <= 0 -> 1e-7, else p (NaN included); frame i is on for threshold k iff
 * (double)p[i] > thresholds[k], compared in float64 whatever the track's type; a table row is one maximal run
 * (first_frame, last_frame), rows in ascending frame order.  first / fps, last / fps and the min_length filter stay with the
 * caller.  Two steps, four launches whatever K and channels are, no atomics (identical bytes on every call):
 *   lad_runs_count  -> workspace: int32 counts[channels * K] at its start (runs of channel c, threshold k at c * K + k);
 *                      the caller copies them to the host to size the table
 *   lad_runs_fill   -> table: int32[total][2], the (c, k) tables back to back in c * K + k order
 * probs: float32 or float64 [channels][frames], contiguous.  thresholds: HOST double[n_thresholds].
 * ---------------------------------------------------------------------------------------------- */
enum lad_runs_dtype { LAD_RUNS_F32 = 0, LAD_RUNS_F64 = 1 };
/* frames one wave handles (laugh_segmenter.py:74-111 has no such notion: the tests place their edge cases from it) */
int32_t lad_runs_tile_frames(void);
/* largest n_thresholds of one call (64; the evaluation sweep of laugh_segmenter.py:74-111 uses 29) */
int32_t lad_runs_max_thresholds(void);
/* bytes of workspace for lad_runs_count / lad_runs_fill (laugh_segmenter.py:74-111); needs no GPU.  -1 and lad_last_error() for
 * channels outside 1..65535, frames outside 1..2^30 or n_thresholds outside 1..lad_runs_max_thresholds(). */
int64_t lad_runs_workspace_bytes(int64_t channels, int64_t frames, int32_t n_thresholds);
/* counting pass of laugh_segmenter.py:74-111 (three launches on `stream`); dtype: lad_runs_dtype */
int lad_runs_count(const void *probs, int32_t dtype, int64_t channels, int64_t frames, const double *thresholds,
                   int32_t n_thresholds, void *workspace, void *stream);
/* the run tables of laugh_segmenter.py:74-111 (one launch): same probs / thresholds / workspace as the lad_runs_count before it.
 * counts_host: HOST int32[channels * n_thresholds], the counts the caller read back.  capacity_runs: rows `table` holds; if the
 * counts sum to more, LAD_ERR_INVALID with lad_last_error() set and nothing is launched.  The kernel never writes a row at or
 * beyond capacity_runs, whatever the workspace holds. */
int lad_runs_fill(const void *probs, int32_t dtype, int64_t channels, int64_t frames, const double *thresholds,
                  int32_t n_thresholds, const void *workspace, const int32_t *counts_host, int32_t *table,
                  int64_t capacity_runs, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Scores of the sweep against transcript intervals, from the run tables above while they are still on the device.
 * Replaces analysis/analyse.py: eval_preds :152-225 and laugh_match :120-149 up to the per-channel integers (and the TextGrid
 * files that textgrid_to_df :49-61 reads back), on the index of analysis/preprocess.py:27-46, 49-120, 133-167, time base
 * analysis/utils.py:8-37 (milliseconds, Python's round).  A run (first, last) of channel c is start = first / fps[c],
 * end = last / fps[c] in float64, kept for min_length l iff end - start > l (laugh_segmenter.py:74-111), and the interval
 * (a, b] = (rint(start * 1000), rint(end * 1000)].  scores[c][k][l] = { n_pred, n_valid, pred_ms, corr_ms, fp_speech_ms,
 * fp_noise_ms, fp_silence_ms } (enum lad_score_field) summed over the kept runs: n_valid counts runs with (a, b] \ INVALID
 * non-empty, or every run if the channel has no invalid interval (analyse.py:185-187); pred_ms = |(a, b] \ INVALID|; the other
 * four are |(a, b] n class|.
 * Index (CSR): int32 bounds[n_intervals][2] = (lo, hi], int32 offsets[channels * 5 + 1], segment c * 5 + class with the
 * classes of enum lad_score_class; within a segment intervals are non-empty, sorted and disjoint, 0 <= lo < hi; LAUGH, SPEECH,
 * NOISE and SILENCE come with INVALID already subtracted (laugh_match :129-131 subtracts it from the prediction instead).
 * Integer sums accumulated with vector global atomics on int64: identical bytes on every call.
 * ---------------------------------------------------------------------------------------------- */
enum lad_score_class { LAD_SCORE_INVALID = 0, LAD_SCORE_LAUGH = 1, LAD_SCORE_SPEECH = 2, LAD_SCORE_NOISE = 3, LAD_SCORE_SILENCE = 4 };
enum lad_score_field { LAD_SCORE_N_PRED = 0, LAD_SCORE_N_VALID = 1, LAD_SCORE_PRED_MS = 2, LAD_SCORE_CORR_MS = 3,
                       LAD_SCORE_FP_SPEECH_MS = 4, LAD_SCORE_FP_NOISE_MS = 5, LAD_SCORE_FP_SILENCE_MS = 6, LAD_SCORE_FIELDS = 7 };
/* largest n_min_lengths of one call (8; the evaluation sweep of cluster_scripts/gen_eval_exp.py:30-36 uses 3) */
int32_t lad_score_max_min_lengths(void);
/* bytes of workspace for lad_score_runs (analyse.py:152-225); needs no GPU.  -1 and lad_last_error() for channels outside
 * 1..65535, n_intervals outside 0..2^30, n_thresholds outside 1..lad_runs_max_thresholds() or n_min_lengths outside
 * 1..lad_score_max_min_lengths(). */
int64_t lad_score_workspace_bytes(int64_t channels, int64_t n_intervals, int32_t n_thresholds, int32_t n_min_lengths);
/* eval_preds / laugh_match of analyse.py:120-225 for every (channel, threshold, min_length) at once: a memset and two launches on
 * `stream`.  runs_workspace, table, counts_host, channels, frames, n_thresholds: as given to / left by lad_runs_count and
 * lad_runs_fill (only the counts at the start of runs_workspace are read).  bounds, offsets, fps: DEVICE; bounds_host,
 * offsets_host, fps_host: HOST copies of the same values, checked before anything is launched; min_lengths: HOST
 * double[n_min_lengths].  scores: DEVICE int64[channels][n_thresholds][n_min_lengths][7].
 * LAD_ERR_INVALID with lad_last_error() set, nothing launched and nothing written, for sizes out of range, an index whose offsets
 * do not ascend from 0 to n_intervals or whose intervals are empty, unsorted or overlapping, an fps that is not positive and
 * finite, or millisecond overflow: to_frames(frames / fps[c]) (utils.py:8-15) must stay below 2^31 for every channel. */
int lad_score_runs(const void *runs_workspace, const int32_t *table, const int32_t *counts_host, int64_t channels,
                   int64_t frames, int32_t n_thresholds, const int32_t *bounds, const int32_t *offsets,
                   const int32_t *bounds_host, const int32_t *offsets_host, int64_t n_intervals, const double *fps,
                   const double *fps_host, const double *min_lengths, int32_t n_min_lengths, void *workspace,
                   int64_t *scores, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Event-level scores of the sweep (csrc/events.hip): which transcribed laughs were found, which predicted laughs were real, into
 * how many pieces a laugh was split and how far its boundaries lie off.  lad_score_runs measures predicted milliseconds and
 * analyse.py:255-257 counts events on both sides (num_of_pred_laughs, valid_pred_laughs, num_of_transc_laughs) without ever
 * matching them; nothing in the reference does this.  The text below IS the specification (tests/_events_model.py is a second
 * implementation of it, per-millisecond sets and per-pair loops).
 *
 * Inputs.  Those of lad_score_runs: the run tables of lad_runs_* or lad_binarize_* with their counts at the start of that
 * workspace, the CSR index, fps and min_lengths; and two integers, min_overlap_ms >= 0 and min_overlap_pct in 0..100.
 * Predictions.  A run (first, last) of channel c is the millisecond interval (a, b] exactly as for lad_score_runs:
 * a = rint(first / fps[c] * 1000), b = rint(last / fps[c] * 1000) in float64 with IEEE division and contraction off; the run is
 * kept for min_length l iff last / fps[c] - first / fps[c] > l.  Within one table a and b do not decrease and a_next >= b_prev,
 * so the intervals are disjoint.  a == b is possible; such a run overlaps nothing.
 * Reference events.  The events of channel c are the intervals (lo, hi] of its LAUGH segment of the index: transcribed laughter
 * with INVALID subtracted, adjacent and overlapping rows merged.  An event is such a maximal interval, not a transcript row.
 * Pairs.  The overlap of an event and a prediction is ov(e, p) = max(0, min(b, hi) - max(a, lo)); e and p are linked iff ov >= 1.
 * Per event, over the kept predictions of one (c, k, l): cov_e = the sum of ov; frag_e = the number of links; first_e and last_e
 * = the first and last linked prediction in table order; touched iff frag_e >= 1; hit iff cov_e >= max(1, min_overlap_ms) and
 * 100 * cov_e >= min_overlap_pct * (hi - lo).
 * Per kept prediction: lov_p = |(a, b] n LAUGH| (F(b) - F(a) with lad_score_runs' coverage function), pred_p = |(a, b] \ INVALID|;
 * hit iff lov_p >= max(1, min_overlap_ms) and 100 * lov_p >= min_overlap_pct * pred_p.  All products are int64.
 * Output.  events[c][k][l] = seven int64 values (enum lad_event_field):
 *   N_REF          events of the channel (the same for every k, l)
 *   REF_TOUCHED    events with at least one link
 *   REF_HIT        events that are hit
 *   PRED_HIT       kept predictions that are hit
 *   LINKS          sum of frag_e over all events
 *   ONSET_ABS_MS   sum over hit events of abs(a(first_e) - lo)
 *   OFFSET_ABS_MS  sum over hit events of abs(b(last_e) - hi)
 * so that REF_HIT <= REF_TOUCHED <= N_REF, LINKS >= REF_TOUCHED, PRED_HIT <= lad_score_runs' n_valid, REF_HIT == REF_TOUCHED for
 * (min_overlap_ms, min_overlap_pct) = (1, 0), and a channel without a participant (five empty sets) has seven zeros.
 * Integer sums accumulated with vector global atomics on int64: identical bytes on every call.
 * ---------------------------------------------------------------------------------------------- */
enum lad_event_field { LAD_EVENT_N_REF = 0, LAD_EVENT_REF_TOUCHED = 1, LAD_EVENT_REF_HIT = 2, LAD_EVENT_PRED_HIT = 3,
                       LAD_EVENT_LINKS = 4, LAD_EVENT_ONSET_ABS_MS = 5, LAD_EVENT_OFFSET_ABS_MS = 6, LAD_EVENT_FIELDS = 7 };
/* bytes of workspace for lad_score_events with run tables of total_runs rows in all (the sum of the counts); needs no GPU.  -1 and
 * lad_last_error() for what lad_score_workspace_bytes refuses or total_runs outside 0..2^38. */
int64_t lad_score_events_workspace_bytes(int64_t channels, int64_t n_intervals, int32_t n_thresholds, int32_t n_min_lengths,
                                         int64_t total_runs);
/* the seven values for every (channel, threshold, min_length) at once: a memset and at most three launches on `stream`, whatever
 * n_thresholds and channels are.  Arguments, limits and checks as lad_score_runs (tables of lad_runs_fill, or the merged table and
 * merged counts of lad_binarize_fill); workspace: its own, of lad_score_events_workspace_bytes for the sum of counts_host;
 * events: DEVICE int64[channels][n_thresholds][n_min_lengths][7].  LAD_ERR_INVALID with lad_last_error() set, nothing launched and
 * nothing written, for what lad_score_runs refuses, min_overlap_ms < 0 or min_overlap_pct outside 0..100. */
int lad_score_events(const void *runs_workspace, const int32_t *table, const int32_t *counts_host, int64_t channels,
                     int64_t frames, int32_t n_thresholds, const int32_t *bounds, const int32_t *offsets,
                     const int32_t *bounds_host, const int32_t *offsets_host, int64_t n_intervals, const double *fps,
                     const double *fps_host, const double *min_lengths, int32_t n_min_lengths,
                     int32_t min_overlap_ms, int32_t min_overlap_pct, void *workspace, int64_t *events, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Threshold sweep with hysteresis and gap filling (csrc/binarize.hip): the event tables of K settings in one pass.
 * The reference has one threshold and a minimum length (laugh_segmenter.py:74-111); these are the two further controls of
 * event-detection post-processing, onset / offset / min_duration_off of pyannote.audio's Binarize restated on this project's
 * frame and time conventions (parity with pyannote itself is not pinned).  The text below IS the specification
 * (tests/_binarize_model.py is a second implementation of it, a per-frame loop).
 *
 * Frames.  v[i] is the fixed probability in float64 exactly as lad_runs_count: p > 1 -> 1, p <= 0 -> 1e-7, anything else
 * unchanged, NaN included; a float32 sample is widened exactly.
 * Settings.  Setting k is (onsets[k], offsets[k], min_gaps[k]), doubles, all finite, offsets[k] <= onsets[k], min_gaps[k] >= 0.
 * Masks.  H[i] = v[i] > onset, L[i] = v[i] > offset, compared in float64 whatever the track's type.  NaN is in neither, and H
 * lies inside L.
 * Hysteresis.  active[-1] = 0, active[i] = H[i] or (active[i - 1] and L[i]).  Equivalently every maximal run of L that holds at
 * least one H frame yields exactly one run, from its first H frame to the end of the L run.  Consecutive hysteresis runs have
 * at least one off frame between them: next.first - prev.last >= 2.
 * Gap filling, per channel c.  Two consecutive hysteresis runs are joined iff NOT (next.first / fps[c] - prev.last / fps[c] >
 * min_gap): float64, IEEE division, no reciprocal, contraction off -- the rule lad_score_runs uses for end - start > min_length.
 * Joining is pairwise on the original neighbours, so chains collapse; a merged run is (first of its first, last of its last).
 * min_gap = 0 never joins.
 * Minimum length.  After gap filling, where it is for the plain sweep: with the caller, or in lad_score_runs.
 * Reduction.  With offsets[k] == onsets[k] and min_gaps[k] == 0 the result is the run table of lad_runs_count / lad_runs_fill
 * for thresholds[k] = onsets[k], bit for bit.
 *
 * Two steps, seven launches whatever K and channels are, no atomics (identical bytes on every call):
 *   lad_binarize_count -> workspace: int32 counts[channels * K] at its start, the HYSTERESIS runs of channel c, setting k at
 *                         c * K + k: an upper bound of the merged counts.  The caller copies them to the host to size the buffers.
 *   lad_binarize_fill  -> raw_table: the hysteresis runs, table: the runs after gap filling, each int32[.][2], the (c, k)
 *                         tables back to back in c * K + k order, rows ascending; the counts at the start of the workspace are
 *                         REPLACED by the merged counts.  After that the workspace and `table` can be handed to lad_score_runs
 *                         (n_thresholds = K, counts_host = the merged counts read back) as if lad_runs_count / lad_runs_fill had
 *                         produced them.
 * probs: DEVICE float32 or float64 [channels][frames], contiguous (dtype: lad_runs_dtype).  onsets, offsets, min_gaps: HOST
 * double[n_settings].  The tile is lad_runs_tile_frames() frames.
 * ---------------------------------------------------------------------------------------------- */
/* largest n_settings of one call (64) */
int32_t lad_binarize_max_settings(void);
/* bytes of workspace for lad_binarize_count / lad_binarize_fill; needs no GPU.  -1 and lad_last_error() for channels outside
 * 1..65535, frames outside 1..2^30 or n_settings outside 1..lad_binarize_max_settings(). */
int64_t lad_binarize_workspace_bytes(int64_t channels, int64_t frames, int32_t n_settings);
/* counting step (three launches on `stream`).  LAD_ERR_INVALID with lad_last_error() set and nothing launched for sizes out of
 * range, an unknown dtype, a null pointer, a non-finite onset or offset, or offsets[k] > onsets[k]. */
int lad_binarize_count(const void *probs, int32_t dtype, int64_t channels, int64_t frames, const double *onsets,
                       const double *offsets, int32_t n_settings, void *workspace, void *stream);
/* fill step (four launches on `stream`): same probs / onsets / offsets / workspace as the lad_binarize_count before it.
 * fps: DEVICE double[channels]; fps_host: HOST copy of the same values, checked before anything is launched.  counts_host: HOST
 * int32[channels * n_settings], the hysteresis counts the caller read back.  raw_table, table: DEVICE int32[capacity_runs][2]
 * each, two different buffers.  LAD_ERR_INVALID with lad_last_error() set, nothing launched and nothing written, for what
 * lad_binarize_count refuses, a min_gap that is negative or not finite, an fps that is not positive and finite, counts that are
 * not run counts of such a track, or counts that sum to more than capacity_runs.  The kernels never write or read a row at or
 * beyond capacity_runs, whatever the workspace holds.  Counts that sum to 0 return LAD_OK without a launch. */
int lad_binarize_fill(const void *probs, int32_t dtype, int64_t channels, int64_t frames, const double *onsets,
                      const double *offsets, const double *min_gaps, int32_t n_settings, const double *fps,
                      const double *fps_host, void *workspace, const int32_t *counts_host, int32_t *raw_table,
                      int32_t *table, int64_t capacity_runs, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Two-state Viterbi decoding of the probability track (csrc/viterbi.hip): the run tables of the best on/off path for K settings
 * in one pass.  The sweeps above decide each frame from that frame alone and repair the result with rules in seconds, which
 * cannot see confidence; here each frame contributes its log-odds, each additional event costs a penalty, and the decoder returns
 * the set of events with the best total score.  The reference has nothing like it.  The text below IS the specification
 * (tests/_viterbi_model.py is a second implementation of it, in Python integers, with a brute-force maximiser beside it).
 *
 * Everything is integer arithmetic in int64.  The decoded path is then a pure function of its inputs, independent of the order
 * of the scans, with identical bytes on every call.
 *
 * Frames.  v[i] is the fixed probability exactly as in lad_runs_count: p > 1 becomes 1, p <= 0 becomes 1e-7, NaN is kept, and a
 * float32 sample is widened exactly.  The bucket of a frame is u[i] = (int)floor(v[i] * 65536.0), which lies in 0..65536.  The
 * product is exact in float64.
 * Emission table.  The caller supplies S, an int32 array of lad_viterbi_table_entries() = 65537 values with |S[u]| <= 2^24.  It
 * does not have to be monotone.  The library never computes a logarithm: device `log` is not bit-equal to numpy's, while a
 * look-up is.
 * Settings.  Setting k is (bias[k], penalty[k]), both int32, with |bias| <= 2^24 and 0 <= penalty <= 2^26.  The frame score is
 * s_k[i] = S[u[i]] - bias[k].  At a NaN frame the score is -2^31 instead.  No optimal path is on at such a frame, so NaN padding
 * of a shorter channel stays off.
 * Objective.  The states are off (0) and on (1), with off before frame 0.  A path's score is the sum of s[i] over its on frames,
 * minus `penalty` for every frame that is on while its predecessor is off.  Leaving a run costs nothing.  With T <= 2^30, every
 * partial sum stays inside +-2^62.
 * Recursion.  Ties are decided exactly like this.  Start with d0 = 0, d1 = -penalty.  For t = 0..T-1, with (d0, d1) the values
 * before frame t:
 *   psi0[t] = (d1 > d0)              the state at t-1 if the state at t is off; a tie means off
 *   psi1[t] = !(d0 - penalty > d1)   the state at t-1 if the state at t is on; a tie means on
 *   d0' = max(d0, d1)
 *   d1' = max(d0 - penalty, d1) + s[t]
 * The state at T-1 is (d1 > d0), and best = max(d0, d1).  Backtrace with psi.  Frame 0's predecessor is not part of the path.
 * Consequences.  The path's score equals `best`, and no other path scores more.  With penalty 0, a frame with s > 0 is on and a
 * frame with s < 0 is off; a frame with s == 0 takes the state of the frame behind it, and is off at the end.
 * Output.  The maximal on-runs of the path are rows (first_frame, last_frame), ascending, in int32 run tables laid out as
 * lad_runs_fill lays them out: the (c, k) tables back to back in c * K + k order, with the int32 counts at the start of the
 * workspace.  The workspace and table can therefore be handed to lad_score_runs and lad_score_events unchanged, with
 * n_thresholds = K.
 *
 * Two steps, seven launches and one whatever K and channels are, no atomics, no float arithmetic behind the bucket:
 *   lad_viterbi_count -> workspace: the on/off masks of every (channel, setting), 64 frames per word, and int32
 *                        counts[channels * K] at its start; `best` if asked for.  The caller copies the counts to the host.
 *   lad_viterbi_fill  -> table: int32[total][2] from the stored masks; the track is not read again.
 * The tile is lad_runs_tile_frames() frames.
 * ---------------------------------------------------------------------------------------------- */
/* largest n_settings of one call (64) */
int32_t lad_viterbi_max_settings(void);
/* entries of the emission table (65537: buckets 0..65536) */
int32_t lad_viterbi_table_entries(void);
/* bytes of workspace for lad_viterbi_count / lad_viterbi_fill; needs no GPU.  -1 and lad_last_error() for channels outside
 * 1..65535, frames outside 1..2^30 or n_settings outside 1..lad_viterbi_max_settings(). */
int64_t lad_viterbi_workspace_bytes(int64_t channels, int64_t frames, int32_t n_settings);
/* decoding step (seven launches on `stream`).  probs: DEVICE float32 or float64 [channels][frames], contiguous (dtype:
 * lad_runs_dtype).  emission: DEVICE int32[65537]; emission_host: HOST copy of the same values, range-checked before anything is
 * launched.  bias, penalty: HOST int32[n_settings].  best: DEVICE int64[channels * n_settings] (c * K + k), or NULL.
 * LAD_ERR_INVALID with lad_last_error() set and nothing launched for sizes out of range, an unknown dtype, a null pointer other
 * than `best`, or a table entry, bias or penalty outside its bound. */
int lad_viterbi_count(const void *probs, int32_t dtype, int64_t channels, int64_t frames, const int32_t *emission,
                      const int32_t *emission_host, const int32_t *bias, const int32_t *penalty, int32_t n_settings,
                      void *workspace, int64_t *best, void *stream);
/* the run tables (one launch on `stream`) from the masks the lad_viterbi_count before it left in `workspace`, with the same
 * channels, frames and n_settings.  counts_host: HOST int32[channels * n_settings], the counts the caller read back.  table:
 * DEVICE int32[capacity_runs][2].  LAD_ERR_INVALID with lad_last_error() set, nothing launched and nothing written, for sizes out
 * of range, a null pointer, counts that are not run counts of such a track, or counts that sum to more than capacity_runs.  The
 * kernel never writes a row at or beyond capacity_runs, whatever the workspace holds.  Counts that sum to 0 return LAD_OK without
 * a launch. */
int lad_viterbi_fill(const void *workspace, const int32_t *counts_host, int64_t channels, int64_t frames, int32_t n_settings,
                     int32_t *table, int64_t capacity_runs, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Dense threshold sweep (csrc/surface.hip): the scores of lad_score_runs for up to 4096 ascending levels in one pass over the
 * track, without any run table.  The reference evaluates 29 thresholds (cluster_scripts/gen_eval_exp.py:30-36); a precision /
 * recall surface, or an average precision, needs hundreds or thousands, and lad_runs_* + lad_score_runs cost a round per 64.
 * The run tables of different thresholds are nested (the component tree of the 1-D signal): every row appears unchanged in the
 * tables of a contiguous range of levels, and a track of T frames has at most T distinct rows.  The text below IS the
 * specification; sweep_eval.score_surface_host is a second implementation of it, and by construction the result equals
 * lad_runs_count + lad_runs_fill + lad_score_runs called level by level.
 *
 * Frame value.  q[i] is the fixed probability in float64 exactly as lad_runs_count: p > 1 -> 1, p <= 0 -> 1e-7, NaN kept, NaN
 * beyond the track.
 * Levels.  HOST double[n_levels], finite and strictly ascending, 1 <= n_levels <= lad_surface_max_levels().  bin[i] = the number
 * of levels strictly below q[i], 0 for NaN: frame i is on at level j iff q[i] > levels[j] iff j < bin[i] (lad_runs_count's
 * comparison).
 * Nodes.  One for every maximal frame interval [first, last] with top = min(bin[first..last]) > 0 whose two outside neighbours,
 * where they exist, have a bin below top; base = the larger of the two neighbours' bins, 0 for a neighbour beyond the track.  The
 * interval is a row of the run table of exactly the levels base <= j < top.
 * A node's integers.  Those of lad_score_runs for the run (first, last) of channel c: start = first / fps[c], end = last / fps[c],
 * kept for min_length l iff end - start > l, (a, b] = (rint(start * 1000), rint(end * 1000)], w = { 1, valid, pred_ms, corr_ms,
 * fp_speech_ms, fp_noise_ms, fp_silence_ms } with valid = pred_ms > 0 or the channel has no INVALID interval.
 * Output.  scores[c][j][l][f] = the sum of w[f] over the nodes of channel c that are kept for l and have base <= j < top: DEVICE
 * int64[channels][n_levels][n_min_lengths][7], every value written by every call.  A channel with five empty sets still counts
 * n_pred and n_valid.
 * Integer sums only, accumulated with vector atomics on int64 and one prefix sum over the levels: identical bytes on every call.
 * One host-to-device copy (the levels), one memset and SIX launches on `stream`, whatever channels, n_levels and n_min_lengths
 * are.  A frame's two nearest-smaller searches read at most 2 * ceil(log2(frames)) minima each, whatever the track looks like.
 * ---------------------------------------------------------------------------------------------- */
/* largest n_levels of one call (4096) */
int32_t lad_surface_max_levels(void);
/* frames one workgroup handles (2048; the tests place their edge cases from it) */
int32_t lad_surface_tile_frames(void);
/* bytes of workspace for lad_score_surface; needs no GPU.  -1 and lad_last_error() for channels outside 1..65535, frames outside
 * 1..2^30, n_intervals outside 0..2^30, n_levels outside 1..lad_surface_max_levels() or n_min_lengths outside
 * 1..lad_score_max_min_lengths(). */
int64_t lad_surface_workspace_bytes(int64_t channels, int64_t frames, int64_t n_intervals, int32_t n_levels, int32_t n_min_lengths);
/* probs: DEVICE float32 or float64 [channels][frames], contiguous (dtype: lad_runs_dtype).  levels: HOST.  The index, fps and
 * min_lengths as for lad_score_runs: bounds, offsets, fps DEVICE; bounds_host, offsets_host, fps_host HOST copies, checked before
 * anything is launched; min_lengths HOST double[n_min_lengths].  workspace: DEVICE, lad_surface_workspace_bytes of the same sizes.
 * LAD_ERR_INVALID with lad_last_error() set, nothing launched and nothing written, for everything lad_score_runs refuses (sizes, a
 * null buffer, the index, fps, millisecond overflow, a NaN min_length), an unknown dtype, and levels that are not finite or do not
 * ascend strictly. */
int lad_score_surface(const void *probs, int32_t dtype, int64_t channels, int64_t frames, const double *levels, int32_t n_levels,
                      const int32_t *bounds, const int32_t *offsets, const int32_t *bounds_host, const int32_t *offsets_host,
                      int64_t n_intervals, const double *fps, const double *fps_host, const double *min_lengths,
                      int32_t n_min_lengths, void *workspace, int64_t *scores, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Event-level scores on the dense sweep (csrc/surface_events.hip): the seven values of lad_score_events for every level of
 * lad_score_surface, together with that call's own seven, from one set of bins and one tree.  The block above lad_score_events
 * stays the specification of the seven event fields (ties and a == b runs included), the block above lad_score_surface that of
 * frame values, levels and nodes; this block only says what the predictions are.  sweep_eval.score_surface_host(..., events=) is a
 * second implementation.
 *
 * Predictions.  For channel c, level j and min_length l: the nodes of lad_score_surface's component tree with base <= j < top that
 * are kept for l, in frame order -- exactly the kept rows of the run table of level j, each the millisecond interval (a, b] of its
 * (first, last).
 * Output.  scores[c][j][l][7] (enum lad_score_field) as lad_score_surface writes it, and events[c][j][l][7] (enum lad_event_field):
 * both DEVICE int64[channels][n_levels][n_min_lengths][7], every value written by every call.  events equals what lad_runs_count +
 * lad_runs_fill + lad_score_events give level by level, bit for bit.
 * How.  PRED_HIT and LINKS are sums over nodes (a node's links: the LAUGH intervals with lo < b minus those with hi <= a, none for
 * a == b) and go through the difference array over the levels with the seven time fields.  REF_TOUCHED, REF_HIT and the two error
 * sums are sums over (event, level): since rint(f / fps * 1000) does not decrease with the frame f, a run [s, e] is linked to the
 * event (lo, hi] iff s <= F1, e >= F0 and a < b, with F0 the first frame whose millisecond is > lo and F1 the last whose
 * millisecond is < hi; those frames are walked once per 64 adjacent levels.  Work: frames * levels / 64 wave steps for events that
 * tile the track, whatever their number; an event longer than the track, or one as long as it, is exact and is walked by one wave
 * per 64 levels.
 * Integer sums only, accumulated with vector atomics on int64 and one prefix sum over the levels: identical bytes on every call.
 * One host-to-device copy (the levels), two memsets and SEVEN launches on `stream`, whatever channels, n_levels, n_min_lengths and
 * the number of events are; no loop over levels or events on the host.
 * ---------------------------------------------------------------------------------------------- */
/* bytes of workspace for lad_score_surface_events; needs no GPU.  -1 and lad_last_error() for what lad_surface_workspace_bytes
 * refuses. */
int64_t lad_surface_events_workspace_bytes(int64_t channels, int64_t frames, int64_t n_intervals, int32_t n_levels,
                                           int32_t n_min_lengths);
/* Arguments as lad_score_surface, then min_overlap_ms >= 0 and min_overlap_pct in 0..100 as lad_score_events; workspace: DEVICE,
 * lad_surface_events_workspace_bytes of the same sizes.  LAD_ERR_INVALID with lad_last_error() set, nothing launched and nothing
 * written, for everything lad_score_surface refuses and for min_overlap_ms < 0 or min_overlap_pct outside 0..100. */
int lad_score_surface_events(const void *probs, int32_t dtype, int64_t channels, int64_t frames, const double *levels,
                             int32_t n_levels, const int32_t *bounds, const int32_t *offsets, const int32_t *bounds_host,
                             const int32_t *offsets_host, int64_t n_intervals, const double *fps, const double *fps_host,
                             const double *min_lengths, int32_t n_min_lengths, int32_t min_overlap_ms, int32_t min_overlap_pct,
                             void *workspace, int64_t *scores, int64_t *events, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Sampling-rate conversion of one channel by up / down = sr_out / sr_in (reduced), polyphase FIR on the device.
 * Replaces the host resampling of the reference's readers: librosa.load(audio_path, sr=44100) in front of the wav cuts
 * (segment_laughter.py:134) and librosa.load(sr=8000) of the code it descends from (laugh_segmenter.py:157-185).
 * Convention: scipy.signal.resample_poly with its defaults.  For a prototype filter h of 2 * half + 1 taps
 *   y[n] = sum_j x[j] * h[half + n * down - j * up],  j in [0, n_in) with the h index in [0, 2 * half]
 * (zero phase, x zero-extended at both ends), n in [0, lad_resample_out_len(n_in, up, down)).
 * Table layout: float32 table[up][K], K = 2 * (half / up) + 1 + (half % up != 0), L = (K - 1) / 2 = half / up;
 *   table[p][t] = h[half + p - (t - L) * up]  where that index lies in [0, 2 * half], 0 elsewhere
 * so every h[i] sits in exactly one cell (p = (i - half) mod up, t = L - (i - half - p) / up) and the zero padding is at
 * the two ends of a row: t = 0 where half + p + L * up > 2 * half, t = K - 1 where half + p - (K - 1 - L) * up < 0.
 * Output n with n * down = c * up + p is sum_{t = 0}^{K - 1} table[p][t] * x[c - L + t], summed in that order with one fused
 * multiply-add per tap: the order depends on nothing but p, and a call for outputs [out_first, out_first + n_out) writes the
 * same bits as those outputs of a call for the whole signal.
 * ---------------------------------------------------------------------------------------------- */
enum lad_resample_dtype { LAD_RESAMPLE_F32 = 0, LAD_RESAMPLE_I16 = 1 };
/* ceil(n_in * up / down): the length librosa.load(sr=...) returns (segment_laughter.py:134); needs no GPU.  -1 and
 * lad_last_error() for n_in < 0, up or down < 1, or n_in * up beyond 64 bits. */
int64_t lad_resample_out_len(int64_t n_in, int32_t up, int32_t down);
/* outputs one workgroup computes from one staged input span (segment_laughter.py:134 has no such notion: the tests place
 * their chunk cuts from it) */
int32_t lad_resample_tile_outputs(void);
/* limits of lad_resample (laugh_segmenter.py:157-185 resamples on the host without any): largest up, down and K ... */
int32_t lad_resample_max_up(void);
int32_t lad_resample_max_down(void);
int32_t lad_resample_max_taps(void);
/* ... and the LDS one workgroup may use for the table and a tile's input span (laugh_segmenter.py:157-185) */
int64_t lad_resample_max_lds_bytes(void);
/* LDS bytes a ratio needs (the table -- none for up == 1 with K >= 3 * down -- plus one tile's input span, about
 * (tile - 1) * down / up + K + 8 samples); needs no GPU.  A ratio is
 * supported iff it is within the three limits above and this is <= lad_resample_max_lds_bytes(); -1 and lad_last_error()
 * outside the three limits (segment_laughter.py:134). */
int64_t lad_resample_lds_bytes(int32_t up, int32_t down, int32_t K);
/* y[0 .. n_out) = outputs out_first .. out_first + n_out of the conversion of x[0 .. n_in) (segment_laughter.py:134,
 * laugh_segmenter.py:157-185); one launch on `stream`.  x: DEVICE float32 or int16 PCM (x_dtype: lad_resample_dtype; int16 is
 * scaled by 1 / 32768 in the kernel); table: DEVICE, layout above; y: DEVICE float32[n_out].  LAD_ERR_INVALID with
 * lad_last_error() set and nothing launched for an unknown x_dtype, up, down or K < 1, a ratio beyond the limits,
 * out_first + n_out > lad_resample_out_len(n_in, up, down), or a null pointer; n_out == 0 returns LAD_OK without a launch. */
int lad_resample(const void *x, int32_t x_dtype, int64_t n_in, const float *table, int32_t up, int32_t down, int32_t K,
                 int64_t out_first, int64_t n_out, float *y, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Zero-phase low-pass of probability tracks on the device: one biquad run forwards and backwards, float64.
 * Replaces lowpass (laugh_segmenter.py:49-55, called from :170 and :195) for tracks in GPU memory.
 * Convention: scipy.signal.filtfilt(b, a, x) with its defaults for len(b) == len(a) == 3, a[0] == 1: odd extension by
 * padlen = 9 frames at both ends (ext[e] = 2 x[0] - x[9 - e], ext[T + 9 + j] = 2 x[T-1] - x[T-2-j]); direct form II transposed
 *   y = b0 x + z0;  z0 = b1 x + z1 - a1 y;  z1 = b2 x - a2 y
 * forwards from zi * ext[0], then over the reversed forward result from zi * (its first element); the middle T frames.
 * The serial recurrence is parallelised as a scan of the affine maps z -> A^m z + c, A = [[-a1, 1], [-a2, 0]]: a lane runs
 * lad_lowpass_tile_frames() frames, a wave composes its 64 lanes, one launch carries the state from wave tile to wave tile.
 * Six launches whatever channels and frames are, no workgroup waits for another, no atomics (identical bytes on every call).
 * ---------------------------------------------------------------------------------------------- */
/* frames of the extended track one lane runs serially; a wave tile is 64 of them (laugh_segmenter.py:49-55 has no such notion:
 * the tests place their edge cases from it) */
int32_t lad_lowpass_tile_frames(void);
/* bytes of workspace for lad_lowpass (laugh_segmenter.py:49-55); needs no GPU.  -1 and lad_last_error() for channels outside
 * 1..65535 or frames outside 10..2^30 (scipy refuses a track of padlen = 9 frames or fewer). */
int64_t lad_lowpass_workspace_bytes(int64_t channels, int64_t frames);
/* out[c][0 .. lengths[c]) = filtfilt of probs[c][0 .. lengths[c]) (laugh_segmenter.py:49-55), out[c][lengths[c] .. frames) = NaN.
 * probs: DEVICE float32 or float64 [channels][frames], contiguous (dtype: lad_runs_dtype; a float32 sample is widened exactly);
 * frames is the row stride of probs and out.  lengths_host: HOST int64[channels], each 10..frames, or NULL for `frames`
 * everywhere (it has been copied when the call returns).  b_host, a_host: HOST double[3]; zi_host: HOST double[2], the
 * lfilter_zi(b, a) of the caller.  out: DEVICE float64 [channels][frames].  workspace: DEVICE, lad_lowpass_workspace_bytes.
 * LAD_ERR_INVALID with lad_last_error() set, nothing launched and nothing written, for sizes or a length out of range, a null
 * pointer, an unknown dtype, a[0] != 1, a non-finite coefficient, or out overlapping probs or the workspace.  The input is
 * never written; every store is guarded by the channel's length and the row stride. */
int lad_lowpass(const void *probs, int32_t dtype, int64_t channels, int64_t frames, const int64_t *lengths_host,
                const double *b_host, const double *a_host, const double *zi_host, double *out, void *workspace,
                void *stream);

/* ------------------------------------------------------------------------------------------------
 * Rank filtering of probability tracks on the device (csrc/rankfilt.hip): median, minimum, maximum or any other order statistic
 * of a sliding window.  Not in the reference, whose only smoother is lowpass (laugh_segmenter.py:49-55); it stands at the same
 * place, in front of the thresholds.
 * Convention: for channel c with length n = lengths[c] (or `frames` when lengths_host is NULL) and h = (window - 1) / 2
 *   out[c][i] = sort_ascending( probs[c][clamp(i - h + j, 0, n - 1)]  for j in 0 .. window-1 )[rank]    for 0 <= i < n
 *   out[c][i] = NaN                                                                                      for n <= i < frames
 * i.e. edge replication at the channel's own length (scipy.ndimage's mode='nearest'): the pad of a ragged tensor never enters
 * a window.  rank = h is the median, rank = 0 the minimum, rank = window - 1 the maximum.  n <= h is legal, every index then
 * clamps.  The result is a selected input value in the dtype of probs, never an arithmetic result.  -0.0 and 0.0 compare
 * equal, and which of the two comes back is unspecified.  The input must hold no NaN inside a channel's length; if it does,
 * only the outputs whose window contains the NaN are unspecified, no other frame and no other channel is affected.
 * One workgroup per (channel, lad_rank_filter_tile_frames() output frames), one lane per frame: a bitwise binary search on
 * order-preserving keys in LDS, 32 or 64 passes of `window` reads per frame whatever the data holds.  One launch whatever the
 * sizes, no workgroup waits for another, no atomics (identical bytes on every call).
 * ---------------------------------------------------------------------------------------------- */
/* output frames per workgroup tile (the tests place their edge cases from it) */
int32_t lad_rank_filter_tile_frames(void);
/* the largest window: 1023 frames */
int32_t lad_rank_filter_max_window(void);
/* bytes of workspace for lad_rank_filter; needs no GPU.  -1 and lad_last_error() for channels outside 1..65535, frames outside
 * 1..2^30, or a window that is even or outside 1..lad_rank_filter_max_window(). */
int64_t lad_rank_filter_workspace_bytes(int64_t channels, int64_t frames, int32_t window);
/* probs: DEVICE float32 or float64 [channels][frames], contiguous (dtype: lad_runs_dtype); frames is the row stride of probs and
 * out.  lengths_host: HOST int64[channels], each 1..frames, or NULL for `frames` everywhere (it has been copied when the call
 * returns).  window: odd, 1..lad_rank_filter_max_window(); rank: 0..window - 1.  out: DEVICE [channels][frames] of the dtype of
 * probs.  workspace: DEVICE, lad_rank_filter_workspace_bytes.  LAD_ERR_INVALID with lad_last_error() set, nothing launched and
 * nothing written, for a size, window, rank or length out of range, an even window, a null pointer, an unknown dtype, or out
 * overlapping probs or the workspace (or probs overlapping the workspace).  The input is never written; every store is guarded
 * by the row stride. */
int lad_rank_filter(const void *probs, int32_t dtype, int64_t channels, int64_t frames, const int64_t *lengths_host,
                    int32_t window, int32_t rank, void *out, void *workspace, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Confidence of an instance (csrc/spanstats.hip): the sum and the earliest peak of the probability track over every row of the
 * span tables, whichever decoder cut them (lad_runs_fill, lad_binarize_fill, lad_viterbi_fill, or the caller).  Not in the
 * reference, which returns bare (start, end).
 * Convention: for the track p of channel c and a row (first, last) of one of its tables, 0 <= first <= last < frames:
 *   frame value   v(i) is lad_runs_count's: the element as float64, > 1 -> 1.0, <= 0 -> 0.0000001.  w(i) = v(i), or 0.0 where the
 *                 element is NaN (hysteresis gap filling, Viterbi paths and caller-made tables can put NaN frames inside a span).
 *   sum           Q(i) = rint(w(i) * 2^32) in float64, round-half-even, as an int64: the product is exact, so Q is a pure function
 *                 of the element.  sum = Q(first) + ... + Q(last), int64: at most 2^62 with frames <= 2^30, it cannot overflow.
 *   peak          the earliest frame of first..last at which w is largest, compared on w itself, not on Q.  peak_value = w(peak),
 *                 one of the track's own fixed values bit for bit; 0.0 only if every frame of the span is NaN.
 *   invalid rows  first < 0, last >= frames or first > last: nothing is read, the row yields (sum 0, peak -1, peak_value 0.0).
 *   derived       on the host, from the integers (laugh_segmenter.confidences): n = last - first + 1,
 *                 mean = float64(sum) / float64(n * 2^32), one IEEE division; peak_time = peak / fps, as `start` is computed.
 *                 No floating-point sum runs on the device.
 * lad_span_stats_prepare runs once per track, independent of any setting, and writes into the workspace the inclusive int64
 * prefix sums of Q per channel and a binary tree of maxima of w (float64, level h: the maximum of 2^h frames; level 0 is the
 * track): five launches whatever the sizes and the data (chunk sums and tree levels 1..11 per lad_span_stats_tile_frames()
 * frames, the scan of the chunk sums, the chunks again, two more launches of 11 tree levels each); no atomics, no workgroup
 * waits for another.  lad_span_stats is one copy of channels + 1 int64 and one launch, one lane per row: the sum is two reads
 * of the prefix sums, the peak at most 3 ceil(log2 frames) + 2 reads of the tree (up the two edges of the span, two reads a
 * level, then down into the leftmost child that holds the maximum, one read a level): 92 for the largest track, 59 for 360,000
 * frames, whatever the length of the span and whatever the track holds.  Two calls write identical bytes.
 * ---------------------------------------------------------------------------------------------- */
/* frames per workgroup of the prepare passes, and the frames under a node of tree level 11 (the tests place their edges from it) */
int32_t lad_span_stats_tile_frames(void);
/* bytes of workspace for lad_span_stats_prepare / lad_span_stats; needs no GPU.  -1 and lad_last_error() for channels outside
 * 1..65535 or frames outside 1..2^30. */
int64_t lad_span_stats_workspace_bytes(int64_t channels, int64_t frames);
/* probs: DEVICE float32 or float64 [channels][frames], contiguous (dtype: lad_runs_dtype).  workspace: DEVICE,
 * lad_span_stats_workspace_bytes.  LAD_ERR_INVALID with lad_last_error() set, nothing launched and nothing written, for a null
 * pointer, an unknown dtype, sizes out of range or probs overlapping the workspace.  The track is only read. */
int lad_span_stats_prepare(const void *probs, int32_t dtype, int64_t channels, int64_t frames, void *workspace, void *stream);
/* probs, dtype, channels, frames, workspace: as given to lad_span_stats_prepare, which has run on this stream or has finished.
 * table: DEVICE int32 [total][2], the tables of the channels * n_settings (channel, setting) pairs back to back in
 * c * n_settings + k order; counts_host: HOST int32[channels * n_settings], their row counts (as lad_score_runs takes them).
 * sums: DEVICE int64[total]; peaks: DEVICE int32[total]; peak_values: DEVICE double[total]: one entry per row, nothing beyond
 * row total - 1 is written.  The last channels + 1 int64 of the workspace take the first row of every channel for the launch:
 * calls that share a workspace are ordered by their stream; everything else is only read.  A total of zero rows is LAD_OK with
 * nothing launched.  LAD_ERR_INVALID with lad_last_error() set, nothing launched and nothing written, for a null pointer (table
 * may be NULL for zero rows), an unknown dtype, sizes out of range (n_settings < 1 included), a negative count, or an output
 * overlapping probs, the table, the workspace or another output. */
int lad_span_stats(const void *probs, int32_t dtype, int64_t channels, int64_t frames, const void *workspace, const int32_t *table,
                   const int32_t *counts_host, int32_t n_settings, int64_t *sums, int32_t *peaks, double *peak_values,
                   void *stream);

/* ------------------------------------------------------------------------------------------------
 * Redrawing the segment table (csrc/sample.hip): which frames of which channel form each training example, drawn afresh for
 * every epoch from regions and pools of regions.  Replaces, on the device, the sampling of the reference's create_data_df.py
 * (get_subsample :84-95, get_random_segment_from_df :65-81, the rejection loops of get_random_non_laughter_segment :32-63) and
 * the label rule of compute_features.py:228-243.  The text below IS the specification (tests/_sample_model.py is a second
 * implementation of it, in Python integers).  Integers only.
 *
 * Frames and milliseconds.  fps frames per second (100 or 128), T frames per segment.  Frame f spans the milliseconds
 * (1000 f / fps, 1000 (f + 1) / fps] in exact rational arithmetic.  A window of frames [a, a + n) lies inside a transcript
 * interval (lo, hi] (ms) iff 1000 a >= lo fps and 1000 (a + n) <= hi fps, compared as int64 products; the frames of (lo, hi] on
 * a channel with frames_c feature rows are therefore [ceil(lo fps / 1000), min(floor(hi fps / 1000), frames_c)).  The
 * millisecond hull of a window is (floor(1000 a / fps), ceil(1000 (a + n) / fps)]; a window inside an interval by the frame
 * rule has its hull inside it too, and at 100 fps both rules are exact.
 *
 * Regions and pools.  A region is (chan, lo, hi) in frames, hi > lo: regions int32 [n_regions][3].  Pool p is the slice
 * pool_off[p] .. pool_off[p + 1] of the region array (pool_off int32 [n_pools + 1], ascending from 0, at most n_regions).
 * pool_cum[j] (int64 [n_regions]) is the sum of (hi - lo - T + 1) over the regions of j's pool that precede j; it is read for
 * measure pools only, whose regions all have hi - lo >= T.
 *
 * Rows.  Row i has kind[i] and src[i]:
 *   LAD_SAMPLE_FIXED         src = a region:  n = min(T, hi - lo), first = lo + mulhi(r1, hi - lo - n + 1)
 *   LAD_SAMPLE_POOL_ROW      src = a pool:    region j = pool_off[p] + mulhi(r0, regions in p), then as FIXED
 *                                             (create_data_df.py:75-79: a row of the pool, then a window inside it)
 *   LAD_SAMPLE_POOL_MEASURE  src = a pool of total measure M = sum of (hi - lo - T + 1) < 2^32:  u = mulhi(r0, M); j = the last
 *                                             region of the pool with pool_cum[j] <= u; first = lo_j + (u - pool_cum[j]); n = T
 *                                             (every window of T frames inside the pool's regions is equally likely: the
 *                                             exact form of the reference's rejection loops, no rejection needed)
 * Random words.  (r0, r1, r2, r3) = philox4x32_10(counter = (row_id & 0xffffffff, row_id >> 32, epoch, 0x53414D50),
 * key = (seed & 0xffffffff, seed >> 32)); mulhi(u, n) = (u * n) >> 32.  The tag in word 3 keeps these draws apart from the
 * augmentation's, which uses small k there.  row_id is the row's place in the table before any permutation or sharding
 * (row_id NULL: i itself), so a row's window is a pure function of (seed, epoch, row_id): not of batch size, rank or world size.
 *
 * Outputs.  chan int32, first int64, count int32 (n_rows each): what lad_gather_segments takes; region (int32, or NULL): the
 * region index j the row was drawn from.  By construction lo_j <= first and first + count <= hi_j.
 *
 * Host copies.  pool_off_host and pool_total_host (int64 [n_pools]: M of a measure pool, anything in [0, 2^32) for another) are
 * checked before anything is launched, and so are kind_host / src_host when they are not NULL: a kind outside 0..2, a src
 * outside its array, a POOL_ROW row of an empty pool, a POOL_MEASURE row of a pool with M = 0, M >= 2^32, offsets that do not
 * ascend from 0 or pass n_regions, T < 1, sizes above 2^30 or a null buffer return LAD_ERR_INVALID with lad_last_error() set.
 * The kernel still guards every region read by n_regions and every pool read by n_pools; a row it cannot draw gets count 0.
 * n_rows == 0 returns LAD_OK without a launch.
 * ---------------------------------------------------------------------------------------------- */
enum lad_sample_kind { LAD_SAMPLE_FIXED = 0, LAD_SAMPLE_POOL_ROW = 1, LAD_SAMPLE_POOL_MEASURE = 2 };
int lad_sample_segments(const int32_t *kind, const int32_t *src, int64_t n_rows, const int64_t *row_id, const int32_t *regions,
                        int64_t n_regions, const int32_t *pool_off, const int64_t *pool_cum, int32_t n_pools,
                        const int32_t *kind_host, const int32_t *src_host, const int32_t *pool_off_host,
                        const int64_t *pool_total_host, int32_t T, uint64_t seed, uint32_t epoch, int32_t *chan, int64_t *first,
                        int32_t *count, int32_t *region, void *stream);
/* out[i][s] = milliseconds of set s of channel set_chan[i] inside the hull of window i = frames [first[i], first[i] + count[i])
 * at fps frames per second: F(hull_hi) - F(hull_lo) with F the coverage function of lad_score_runs' index (a negative first or
 * count is read as 0).  bounds int32 [n_intervals][2], offsets int32 [n_channels * n_sets + 1]: the CSR layout of
 * lad_score_runs with n_sets sets per channel instead of 5; within a set intervals are non-empty, sorted and disjoint,
 * 0 <= lo < hi.  The host copies are checked before the launch as lad_score_runs checks its index (LAD_ERR_INVALID, nothing
 * launched); a set_chan outside [0, n_channels) gives a row of zeros.  out: DEVICE int32 [n][n_sets]. */
int lad_window_coverage(const int32_t *set_chan, const int64_t *first, const int32_t *count, int64_t n, int32_t fps,
                        const int32_t *bounds, const int32_t *offsets, const int32_t *bounds_host, const int32_t *offsets_host,
                        int64_t n_intervals, int32_t n_channels, int32_t n_sets, int32_t *out, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Bootstrap intervals of the sweep's figures (csrc/bootstrap.hip): a percentile bootstrap over recording units (channels or
 * meetings).  Not in the reference, which writes point figures only.  The text below IS the specification
 * (tests/_bootstrap_model.py is a second implementation of it, in Python integers and fractions).  Integers only: the device
 * never rounds, and the host divides once per reported number.
 *
 * Units and replicates.  G units (1..lad_bootstrap_max_units()), B replicates (1..lad_bootstrap_max_replicates()).  Replicate b
 * is G draws with replacement; weights[b][g] is how often unit g was drawn, so every row sums to G.
 *
 * Random words.  Draw i of replicate b is word i & 3 of philox4x32_10(counter = (i >> 2, b, 0, 0x424F4F54), key = (seed &
 * 0xffffffff, seed >> 32)); the unit is mulhi(word, G) = (word * G) >> 32, the rule of lad_sample_segments.  The tag in word 3
 * ("BOOT") keeps these draws apart from the sampler's 0x53414D50 and from the augmentation's small values.  The weights are a
 * pure function of (seed, b, G): two evaluations with one seed see the same resamples.
 *
 * Sums.  x is int64 [G][M], one row of M integers per unit; sums[b][m] = sum over g of weights[b][g] * x[g][m], in 64-bit
 * integers.  Contract: 0 <= x < 2^40, weights >= 0 and every weight row sums to at most 4096; every sum is then below 2^52.
 * Values outside the contract give unspecified sums and never an access outside the buffers.  Integer addition has no order, so
 * the bytes do not depend on how the product is tiled.
 *
 * Figures.  A figure is six int32: (num_col, num_mult, den_col_a, den_col_b, valid_col, empty_is_one); num_mult is 1 or 2,
 * den_col_b and valid_col may be -1, empty_is_one is 0 or 1.  For replicate b: num = num_mult * sums[b][num_col]; den =
 * sums[b][den_col_a], plus sums[b][den_col_b] unless den_col_b is -1.  The replicate is invalid when valid_col >= 0 and
 * sums[b][valid_col] == 0, and when den == 0 and empty_is_one == 0; with den == 0 and empty_is_one == 1 it counts as the fraction
 * 1 / 1 (the reference's rule: precision is 1 where nothing is predicted).  Both num and den are below 2^54.
 *
 * Order and quantiles.  v = the number of valid replicates of the figure.  The valid ones are ordered by the exact value
 * num / den: num1 * den2 against num2 * den1 as 128-bit products; equal values by the replicate number, ascending.  Quantile
 * q_num / q_den (0 < q_num < q_den, int32) is the pair (num, den) at rank max(ceil(q_num * v / q_den) - 1, 0) of that order, in
 * integers; (-1, -1) when v == 0.
 *
 * Shared by the three calls: LAD_ERR_INVALID with lad_last_error() set, nothing launched and nothing written, for a null
 * pointer, a size out of range, an output overlapping an input or another output, a bad figure or a bad quantile.  Identical
 * bytes on every call; no global atomics; nothing beyond the stated extents is written.
 * ---------------------------------------------------------------------------------------------- */
/* both 4096; neither needs a GPU */
int64_t lad_bootstrap_max_units(void);
int64_t lad_bootstrap_max_replicates(void);
/* weights: DEVICE int32 [replicates][units].  One launch, one workgroup per replicate: the counts in an LDS histogram. */
int lad_bootstrap_weights(int32_t units, int32_t replicates, uint64_t seed, int32_t *weights, void *stream);
/* x: DEVICE int64 [units][columns]; weights: DEVICE int32 [replicates][units]; sums: DEVICE int64 [replicates][columns].
 * columns 0..2^32; columns == 0 is LAD_OK without a launch (x and sums may be NULL then).  One launch. */
int lad_bootstrap_sums(const int64_t *x, const int32_t *weights, int32_t units, int64_t columns, int32_t replicates, int64_t *sums,
                       void *stream);
/* sums: DEVICE int64 [replicates][columns], columns >= 1; figures: DEVICE int32 [n_figures][6] and figures_host, the same
 * values on the HOST, checked before anything is launched (columns in range, num_mult 1 or 2, the flag 0 or 1); q_num, q_den:
 * HOST int32 [n_quantiles], 1 <= n_quantiles <= 16; out: DEVICE int64 [n_figures][n_quantiles][2]; valid: DEVICE int32
 * [n_figures].  n_figures == 0 is LAD_OK without a launch.  One launch, one workgroup per figure. */
int lad_bootstrap_quantiles(const int64_t *sums, int64_t columns, int32_t replicates, const int32_t *figures,
                            const int32_t *figures_host, int64_t n_figures, const int32_t *q_num, const int32_t *q_den,
                            int32_t n_quantiles, int64_t *out, int32_t *valid, void *stream);

/* Pairs of figures: the difference of two systems, and the harmonic mean of two figures of one (event F1), under the same
 * resamples.  A pair is 13 int32: (op, figure1[6], figure2[6]); both figures are six-integer figures as above, over columns of
 * the one sums matrix.  For replicate b each figure gives (n, d) and a validity by the rule above, the substitution of 1 / 1
 * included; the pair is valid for b iff both figures are.  n1, d1, n2, d2 are below 2^54.
 *
 * The value of a valid replicate is N / D:
 *   op 0, difference:     N = n1 * d2 - n2 * d1 (signed), D = d1 * d2;
 *   op 1, harmonic mean:  N = 2 * n1 * n2, D = n1 * d2 + n2 * d1, and the value 0 / 1 where D is 0 (both numerators are 0 then:
 *                         event_f1's rule "0 where precision + recall is 0").
 * |N| and D are below 2^109.  No other op is accepted.
 *
 * Order.  The valid replicates are ordered by the exact value N / D: by the sign of N first, then |N_i| * D_j against |N_j| * D_i as
 * 256-bit products (built from 64-bit halves; of two negative values the larger magnitude comes first); equal values by the
 * replicate number, ascending.  v = the number of valid replicates; quantile q_num / q_den is the replicate at rank
 * max(ceil(q_num * v / q_den) - 1, 0) of that order.
 *
 * sums, q_num, q_den, n_quantiles: as for lad_bootstrap_quantiles.  pairs: DEVICE int32 [n_pairs][13] and pairs_host, the same
 * values on the HOST, checked before anything is launched (op 0 or 1, columns in range, num_mult 1 or 2, the flag 0 or 1).
 * out: DEVICE int64 [n_pairs][n_quantiles][4], the (n1, d1, n2, d2) of that replicate after the substitution, all -1 when v == 0:
 * the host forms N / D from them and divides once.  valid: DEVICE int32 [n_pairs].  signs: DEVICE int32 [n_pairs][3], how many
 * valid replicates have N < 0, N == 0 and N > 0.
 * The family's refusals hold (a bad op is a bad figure; each of the three outputs against the sums, the pairs and one another).
 * n_pairs == 0 is LAD_OK without a launch.  One launch, one workgroup per pair; the whole order in LDS, 36 bytes a replicate
 * (padded to a power of two): 144 KiB at 4096.  No global atomics; identical bytes on every call. */
int lad_bootstrap_pair_quantiles(const int64_t *sums, int64_t columns, int32_t replicates, const int32_t *pairs,
                                 const int32_t *pairs_host, int64_t n_pairs, const int32_t *q_num, const int32_t *q_den,
                                 int32_t n_quantiles, int64_t *out, int32_t *valid, int32_t *signs, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Calibration of the probability track against the transcript (csrc/calibration.hip): the label histogram of a track, and a
 * 65537-entry map applied to a track.  Not in the reference, which treats the network's output as a probability and never checks
 * it.  The text below IS the specification (tests/_calibration_model.py is a second implementation of it, with per-millisecond
 * sets and a Python loop over the frames).  The device only adds integers; every figure (Brier, NLL, ECE, ROC AUC, the
 * reliability table) and every fit (Platt, temperature, isotonic) follows on the host from the 5 x 65538 integers of a row
 * (calibration.py).
 *
 * Frames.  v[i] is the fixed probability exactly as in lad_runs_count: p > 1 becomes 1, p <= 0 becomes 1e-7, NaN is kept, and a
 * float32 sample is widened exactly.  The bucket of a frame is u[i] = (int)floor(v[i] * 65536.0), in 0..65536, as in
 * lad_viterbi_count.  A NaN frame goes to slot 65537, so a histogram row has lad_label_histogram_slots() = 65538 slots.
 * Time.  For channel c with n_c frames (lengths_host[c], or `frames` when lengths_host is NULL), m_j = rint((double)j / fps[c] *
 * 1000) for j = 0..n_c: IEEE division, no reciprocal, contraction off, the expression of lad_score_runs for a run's ends.  Frame i
 * (0 <= i < n_c) owns the millisecond interval (m_i, m_{i+1}].  A run first..last of the scorers is (m_first, m_last], the
 * frames first..last-1: the convention the scorers already use.  Frames at or beyond n_c are not read.
 * Weights.  w_k(i) = F_k(m_{i+1}) - F_k(m_i) for the five segments k of the index (enum lad_score_class; LAUGH, SPEECH, NOISE and
 * SILENCE come with INVALID already subtracted), F the coverage function of lad_score_runs: the milliseconds of class k in
 * (0, x].  Milliseconds in none of the five sets (beyond the channel's length) belong to nobody.
 * Output.  hist[g][k][slot], int64, n_groups x 5 x 65538 entries: the sum of w_k(i) over the frames i of every channel c with
 * group[c] == g whose slot is `slot`.  group_host: HOST int32[channels] with values in -1..n_groups-1; -1 leaves the channel out;
 * NULL puts channel c into group c, and n_groups must equal channels then.  The entry point zeroes hist itself.
 * Consequences.  For every channel and class the sum over all 65538 slots equals F_k(m_{n_c}).  A channel without a participant
 * (five empty sets) adds nothing.  All sums stay below 2^47: a channel holds fewer than 2^31 ms (lad_score_runs' millisecond-
 * overflow check, here on m_{n_c}) and there are at most 65535 channels.
 * Arithmetic.  Integer sums only, accumulated with vector global atomics on int64: identical bytes on every call.
 *
 * Launches: one memset of hist, one copy each of the lengths and the groups where they are given, and two launches whatever the
 * sizes: the running lengths of the index (one workgroup per (channel, class)), then one workgroup per (channel,
 * lad_label_histogram_tile_frames() frames).  A workgroup sorts its frames by slot in LDS, sums the weights of equal slots there,
 * and issues at most one atomic per distinct (class, slot) it met, none for a sum of zero: a constant track costs at most five
 * atomics a workgroup.  An index without any interval returns after the memset.
 * ---------------------------------------------------------------------------------------------- */
/* slots of a histogram row (65538: buckets 0..65536, then the NaN frames) */
int32_t lad_label_histogram_slots(void);
/* frames per workgroup (the tests place their edges from it) */
int32_t lad_label_histogram_tile_frames(void);
/* bytes of workspace for lad_label_histogram; needs no GPU.  -1 and lad_last_error() for channels outside 1..65535, frames
 * outside 1..2^30 or n_intervals outside 0..2^30. */
int64_t lad_label_histogram_workspace_bytes(int64_t channels, int64_t frames, int64_t n_intervals);
/* probs: DEVICE float32 or float64 [channels][frames], contiguous (dtype: lad_runs_dtype), only read.  lengths_host: HOST
 * int64[channels], each 1..frames, or NULL.  bounds, offsets, fps: DEVICE, the index and the frame rates as lad_score_runs takes
 * them; bounds_host, offsets_host, fps_host: HOST copies of the same values, checked before anything is launched.  workspace:
 * DEVICE, lad_label_histogram_workspace_bytes.  hist: DEVICE int64[n_groups][5][65538].  The host arrays have been copied when
 * the call returns.
 * LAD_ERR_INVALID with lad_last_error() set, nothing launched and nothing written, for everything lad_score_runs refuses of the
 * index and fps (offsets that do not ascend from 0 to n_intervals, intervals that are empty, unsorted or overlapping, an fps that
 * is not positive and finite, millisecond overflow of m_{n_c}), sizes out of range, an unknown dtype, a null pointer, a length
 * outside 1..frames, a group outside -1..n_groups-1, n_groups outside 1..channels (or not channels when group_host is NULL), or
 * hist, probs and the workspace overlapping one another. */
int lad_label_histogram(const void *probs, int32_t dtype, int64_t channels, int64_t frames, const int64_t *lengths_host,
                        const int32_t *bounds, const int32_t *offsets, const int32_t *bounds_host, const int32_t *offsets_host,
                        int64_t n_intervals, const double *fps, const double *fps_host, const int32_t *group_host,
                        int32_t n_groups, void *workspace, int64_t *hist, void *stream);
/* out[c][i] = table[u[i]] with u the bucket above; a NaN frame gives NaN.  table: DEVICE double[65537], read as it is (the caller
 * keeps it in [0, 1]); out: DEVICE double[channels][frames].  One launch, one lane per frame, the table read through the cache;
 * every decoder, smoother and scorer takes the result as a float64 track.  LAD_ERR_INVALID with lad_last_error() set, nothing
 * launched and nothing written, for sizes out of range, an unknown dtype, a null pointer, or out overlapping probs or the table. */
int lad_track_remap(const void *probs, int32_t dtype, int64_t channels, int64_t frames, const double *table, double *out,
                    void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LAD_HIP_H */
