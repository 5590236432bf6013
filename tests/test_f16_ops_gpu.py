"""The fp16 BASE kernels (csrc/conv_f16.hip: lad_f16_pack_weights, lad_f16_conv_fwd, lad_f16_conv_s2_fwd, lad_f16_stem_fwd,
lad_f16_pool_fwd) against a float64 evaluation of the same formulas on the same operands, operator by operator.  Every fused fp16
kernel is tested bit for bit against these entry points (tests/test_resnet_gpu.py); this file is what anchors them.

Arithmetic and bound (tests/_f16_model.py, derived there; tests/test_f16_model_cpu.py shows what the bound lets through and what not):
  convolution   halfs in, n = taps * cin exact products summed in fp32 on the matrix cores, t = fmaf(acc, scale, shift) [+ addend],
                ReLU, ONE rounding to half.  stem: fp32 in, nine fmaf, fmaf(acc, scale, shift), ReLU, one rounding to half.
                pool: fp32 sum of 16 halfs times 1/16, written as fp32.
      u = 2^-23, S = the exact sum, A = sum |x_i w_i|
      e32   = n u A |scale| + 2 u (|S scale| + |shift| + |addend|)
      bound = 2^-11 (|t_ref| + e32) + e32 + 2^-24            (pool: e32 alone)
  asserted: |float(got) - ref| <= bound at EVERY interior element of every case, ref = max(t_ref, 0) with ReLU; border positions and the
  W + 2 rows behind the last image exactly zero (outputs are pre-filled with 3.0).  No tolerance relative to max |ref|.
  lad_f16_pack_weights: the documented image, bit for bit.

Kernel variants reached, from the launchers' conditions (launch_h1 / launch_h2 / lad_f16_conv_fwd in conv_f16.hip; rows = B (H + 1)(W + 1)
+ W + 2):
  lad_f16_conv_fwd     128-row tiles (conv_f16_s1_kernel<.., 4>): every case at 16 / 32 channels but the small-block ones, and at 64
                       channels below 131,072 rows; (60, 13, 6) is 5,888 rows = 46 whole tiles with the tail in a 47th, (61, 13, 6) ends
                       inside a tile.
                       256-row tiles (<.., 8>: 64 channels, rows >= 512 * 256, the tile fits 80 KB of LDS): (29, 100, 44) = 131,851
                       rows and (700, 13, 14) = 147,016 rows.
                       persistent (conv_f16_s1p_kernel: 64 channels, rows >= 4096 * 256, 256 + 2 (W + 2) <= 384): (2119, 10, 44) =
                       1,048,951 rows.
                       small-block (block_f16_small_kernel<16, SINGLE>: 16 channels, addend, relu, batch >= 512): (517, 7, 5) and
                       (600, 25, 11) in their (addend, relu) form; (511, 7, 5) and the other three forms stay on the tiled kernel.
  lad_f16_conv_s2_fwd  one tile per workgroup everywhere but (1400, 25, 11) at 16 -> 16: 137,208 output rows = 1,072 tiles of 128 on
                       256 * 4 = 1,024 workgroups (PER_CU = 4 for both 16 -> 16 forms), so 48 workgroups walk a second tile.
  The large batches are K distinct images repeated periodically (K odd, no divisor of 128, (H + 1)(W + 1) no multiple of 128: every
  copy sits at another phase of the tile grid); the reference is computed for the K images and compared, on the device, with every copy.

Largest err / bound observed on the MI355X, per entry point (each case prints its own):
  lad_f16_conv_fwd      64 channels 0.78 on 128-row tiles, 0.70 on 256-row tiles, 0.72 persistent; 32 channels 0.89; 16 channels 0.94
                        tiled, 0.92 on the small-block route
  lad_f16_conv_s2_fwd   3x3: 0.61 (64 -> 32), 0.75 (32 -> 16), 0.87 (16 -> 16; 0.86 in the tile loop);
                        1x1: 0.94 (64 -> 32), 0.96 (32 -> 16), 0.99 (16 -> 16; 0.98 in the tile loop)
  lad_f16_stem_fwd      0.99
  lad_f16_pool_fwd      0.02
  The fewer products, the closer to 1: with n = 9 (stem) or 16 (the 16 -> 16 1x1) e32 is a few 1e-6 of the sum, the bound is all but the
  half rounding alone, 2^-11 |t|, and that is attained (to within 2^-11 relative) by any t just above a power of two that lies next to
  the midpoint of two halfs -- among 1e4 to 1e6 outputs the largest err / bound is then 0.98 to 0.99 for a correct kernel.  With
  n = 576 the fp32 term is two thirds of the bound and a kernel uses a fraction of it (0.6 to 0.8).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _f16_model as fm
from test_resnet_gpu import _lib, act_rows, borders_are_zero, from_pnhwc, to_pnhwc

pytestmark = pytest.mark.gpu

FILL = 3.0


def rng_of(*key):
    return np.random.default_rng([7, *key])


def signed_scale(rng, C):
    """Both signs, |scale| in [0.5, 1.5]."""
    return ((rng.random(C) + 0.5) * np.where(np.arange(C) % 3 == 1, -1.0, 1.0)).astype(np.float32)


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)


def pack(h, lib, w, st):
    """w (cout, cin, k, k) fp32 numpy -> the packed image on the device."""
    cout, cin, k = w.shape[0], w.shape[1], w.shape[2]
    wt = torch.full((int(lib.lad_f16_packed_weight_halfs(cout, cin, k * k)),), FILL, device="cuda", dtype=torch.float16)
    wg = dev(w)
    h.check(lib.lad_f16_pack_weights(h.ptr(wg), cout, cin, k * k, h.ptr(wt), st), "lad_f16_pack_weights")
    return wt


def pnhwc_half(x, B=None):
    """x (K, C, H, W) half values (numpy) -> the flat half PNHWC buffer of B images on the device, image b = x[b % K], zero borders
    and a zero tail.  The K-image body is tiled on the device."""
    K, C, H, W = x.shape
    small = to_pnhwc(torch.from_numpy(x).float()).half()
    if B is None or B == K:
        return small
    img = (H + 1) * (W + 1) * C
    buf = torch.zeros(act_rows(B, H, W) * C, device="cuda", dtype=torch.float16)
    torch.index_select(small[:K * img].view(K, img), 0, torch.arange(B, device="cuda") % K, out=buf[:B * img].view(B, img))
    return buf


def worst_ratio(out, ref, bound, B, what):
    """out: the flat device buffer of B images of ref's (C, H, W); ref, bound: (K, C, H, W) float64 numpy, image b is held against
    ref[b % K].  Borders and tail exactly zero, EVERY interior element within its bound (a NaN counts as outside).  Returns max err / bound."""
    K, C, H, W = ref.shape
    assert borders_are_zero(out, B, C, H, W), what
    body = out[:B * (H + 1) * (W + 1) * C].view(B, H + 1, W + 1, C)[:, 1:, 1:, :]
    r, bd = dev(ref.transpose(0, 2, 3, 1), torch.float64), dev(bound.transpose(0, 2, 3, 1), torch.float64)
    worst, outside, seen = 0.0, 0, 0
    for k in (range(K) if K != B else [None]):
        got, rk, bk = (body.double(), r, bd) if k is None else (body[k::K].double(), r[k], bd[k])
        err = (got - rk).abs()
        outside += int((~(err <= bk)).sum())
        seen += err.numel()
        worst = max(worst, float(torch.nan_to_num(err / bk, nan=float("inf")).max()))
    assert seen == B * C * H * W
    print(f"{what}: max err / bound = {worst:.3f}")
    assert outside == 0, (what, outside, worst)
    return worst


# ---- lad_f16_pack_weights ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cout,cin,taps", [(64, 64, 9), (32, 32, 9), (16, 16, 9), (32, 64, 9), (16, 32, 9), (16, 16, 9), (32, 64, 1), (16, 32, 1),
                                           (16, 16, 1)],
                         ids=["s1-64", "s1-32", "s1-16", "s2-64-32-3x3", "s2-32-16-3x3", "s2-16-16-3x3", "s2-64-32-1x1", "s2-32-16-1x1",
                              "s2-16-16-1x1"])
def test_packed_weight_image_is_the_documented_layout_bit_for_bit(cout, cin, taps):
    """wt[tap][cin / 16][2][COUTP][8], element (tap, s, h, co, j) = half(w[co][16 s + 8 h + j][tap]), zeros for co >= cout: the nine
    forms in use (the 16 -> 16 3x3 of the stride-2 layer takes the image of the stride-1 one), with ties to even in both directions, a
    half subnormal, -0.0 and the largest half planted among random weights."""
    h = _lib()
    lib = h.lib()
    rng = rng_of(cout, cin, taps)
    w = (rng.standard_normal((cout, cin, taps)) * 0.1).astype(np.float32)
    planted = np.float32([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 3e-6, -0.0, 65504.0, 2.0 ** -25, 2.0 ** -24 + 2.0 ** -26])
    for i, v in enumerate(planted):
        w[(5 * i + 3) % cout, (7 * i + 9) % cin, (2 * i + 1) % taps] = v
        w[cout - 1 - i % cout, cin - 1 - (3 * i) % cin, (taps - 1 - i) % taps] = v
    k = 3 if taps == 9 else 1
    want = fm.pack_image(w)
    assert float(np.float16(np.float32(1 + 2.0 ** -11))) == 1.0 and float(np.float16(np.float32(1 + 3 * 2.0 ** -11))) == 1 + 2.0 ** -9
    assert int(lib.lad_f16_packed_weight_halfs(cout, cin, taps)) == want.size
    got = pack(h, lib, w.reshape(cout, cin, k, k), h.stream_handle())
    torch.cuda.synchronize()
    got_bits = got.view(torch.int16).cpu().numpy().view(np.uint16)
    diff = np.flatnonzero(got_bits != want.view(np.uint16).ravel())
    assert diff.size == 0, (diff.size, diff[:8])


# ---- lad_f16_conv_fwd ----------------------------------------------------------------------------------------------------------------
WSTD = {64: 0.06, 32: 0.08, 16: 0.1}
S1_SMALL = [(3, 13, 6), (2, 25, 11), (1, 1, 1), (5, 2, 1), (2, 1, 7), (2, 5, 63), (2, 5, 64), (8, 10, 44), (60, 13, 6), (61, 13, 6)]
S1_LARGE = [(64, 29, 100, 44, 3), (64, 700, 13, 14, 5), (64, 2119, 10, 44, 7), (16, 517, 7, 5, 5), (16, 600, 25, 11, 7), (16, 511, 7, 5, 5)]


def conv_s1_case(C, B, H, W, K):
    h = _lib()
    lib = h.lib()
    st = h.stream_handle()
    rng = rng_of(C, B, H, W)
    x = fm.half(rng.standard_normal((K, C, H, W)))
    add = fm.half(rng.standard_normal((K, C, H, W)))
    w = fm.half(rng.standard_normal((C, C, 3, 3)) * WSTD[C])
    scale, shift = signed_scale(rng, C), (rng.standard_normal(C) * 0.2).astype(np.float32)
    S, A = fm.conv_sum(x, w), fm.conv_sum(np.abs(x), np.abs(w))
    wt = pack(h, lib, w.astype(np.float32), st)
    xin, ain, sc, sh = pnhwc_half(x, B), pnhwc_half(add, B), dev(scale), dev(shift)
    worst = 0.0
    for addend, relu in ((None, 0), (None, 1), (add, 1), (add, 0)):
        ref, bound = fm.epilogue_bound(S, A, 9 * C, scale, shift, addend, relu)
        out = torch.full((act_rows(B, H, W) * C,), FILL, device="cuda", dtype=torch.float16)
        h.check(lib.lad_f16_conv_fwd(h.ptr(xin), h.ptr(wt), h.ptr(sc), h.ptr(sh), h.ptr(ain) if addend is not None else None, h.ptr(out),
                                     B, H, W, C, C, 9, relu, st), "lad_f16_conv_fwd")
        torch.cuda.synchronize()
        worst = max(worst, worst_ratio(out, ref, bound, B, f"conv_fwd C={C} ({B},{H},{W}) addend={addend is not None} relu={relu}"))
    return worst


@pytest.mark.parametrize("B,H,W", S1_SMALL)
@pytest.mark.parametrize("C", [64, 32, 16])
def test_stride1_convolution_against_float64(C, B, H, W):
    """lad_f16_conv_fwd on the 128-row tiled kernel, the four (addend, relu) forms: images of one position, one column, one row, 64 and
    65 positions per row, a batch that ends on a tile boundary and one that does not."""
    assert act_rows(B, H, W) < 512 * 256
    conv_s1_case(C, B, H, W, B)


@pytest.mark.parametrize("C,B,H,W,K", S1_LARGE)
def test_stride1_convolution_of_large_batches_against_float64(C, B, H, W, K):
    """The kernels lad_f16_conv_fwd only takes from a row count on (256-row tiles, the persistent kernel) or an image count on (the
    small-block route at 16 channels, with its neighbour one image below): K distinct images repeated over the batch."""
    rows = act_rows(B, H, W)
    assert K % 2 == 1 and 128 % K != 0 and ((H + 1) * (W + 1)) % 128 != 0
    if C == 64:
        assert rows >= 512 * 256 and (rows >= 4096 * 256) == (B == 2119) and 256 + 2 * (W + 2) <= 384
    else:
        assert (B >= 512) == (B != 511)
    conv_s1_case(C, B, H, W, K)


# ---- lad_f16_conv_s2_fwd -------------------------------------------------------------------------------------------------------------
S2_FORMS = [(64, 32, 9), (32, 16, 9), (16, 16, 9), (64, 32, 1), (32, 16, 1), (16, 16, 1)]
S2_SHAPES = [(3, 7, 5), (2, 8, 6), (2, 7, 6), (2, 8, 5), (1, 1, 1), (2, 2, 1), (3, 25, 11)]


def conv_s2_case(cin, cout, taps, B, H, W, K):
    h = _lib()
    lib = h.lib()
    st = h.stream_handle()
    rng = rng_of(cin, cout, taps, B, H, W)
    k = 3 if taps == 9 else 1
    x = fm.half(rng.standard_normal((K, cin, H, W)))
    x[:, :, H - 1, :] = 7.0        # a tap one past the edge must read the zero border, not these
    x[:, :, :, W - 1] = 7.0
    w = fm.half(rng.standard_normal((cout, cin, k, k)) * WSTD[cin] * (3.0 if taps == 1 else 1.0))
    scale, shift = signed_scale(rng, cout), (rng.standard_normal(cout) * 0.2).astype(np.float32)
    S, A = fm.conv_sum(x, w, 2), fm.conv_sum(np.abs(x), np.abs(w), 2)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    assert S.shape == (K, cout, Ho, Wo)
    wt = pack(h, lib, w.astype(np.float32), st)
    xin, sc, sh = pnhwc_half(x, B), dev(scale), dev(shift)
    for relu in (0, 1):
        ref, bound = fm.epilogue_bound(S, A, taps * cin, scale, shift, None, relu)
        out = torch.full((act_rows(B, Ho, Wo) * cout,), FILL, device="cuda", dtype=torch.float16)
        h.check(lib.lad_f16_conv_s2_fwd(h.ptr(xin), h.ptr(wt), h.ptr(sc), h.ptr(sh), h.ptr(out), B, H, W, cin, cout, taps, relu, st),
                "lad_f16_conv_s2_fwd")
        torch.cuda.synchronize()
        worst_ratio(out, ref, bound, B, f"conv_s2_fwd {cin}->{cout} taps={taps} ({B},{H},{W}) relu={relu}")


@pytest.mark.parametrize("cin,cout,taps,B,H,W", [f + s for f in S2_FORMS for s in S2_SHAPES] + [(64, 32, 9, 1, 100, 44), (64, 32, 1, 1, 100, 44)])
def test_stride2_convolution_against_float64(cin, cout, taps, B, H, W):
    """lad_f16_conv_s2_fwd, 3x3 pad 1 and 1x1 pad 0, with and without ReLU: both parities of H and of W, images of one position and of
    one column, the model's 100 x 44 at 64 -> 32; the input's last row and column hold 7.0."""
    conv_s2_case(cin, cout, taps, B, H, W, B)


@pytest.mark.parametrize("taps", [9, 1])
def test_stride2_convolution_with_more_tiles_than_workgroups_against_float64(taps):
    """16 -> 16 on 1,400 images of 25 x 11: 137,208 output rows = 1,072 tiles on 1,024 workgroups, the tile loop runs twice."""
    B, H, W = 1400, 25, 11
    assert -(-act_rows(B, (H + 1) // 2, (W + 1) // 2) // 128) > 1024
    conv_s2_case(16, 16, taps, B, H, W, 7)


# ---- lad_f16_stem_fwd ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,frame_stride,frames_avail", [(3, 13, 6, 13, 39), (2, 100, 44, 100, 200), (40, 10, 44, 1, 45), (5, 7, 5, 1, 0),
                                                             (130, 3, 3, 1, 131), (2, 5, 64, 5, 10), (3, 4, 1, 4, 12)])
def test_stem_against_float64(B, H, W, frame_stride, frames_avail):
    """lad_f16_stem_fwd: back-to-back images and windows one frame apart, a file that ends inside the later windows (123.0 behind its end
    must not be read), no frames at all (relu(shift) everywhere), one column, 64 columns, more than one tile."""
    h = _lib()
    lib = h.lib()
    st = h.stream_handle()
    C = 64
    rng = rng_of(B, H, W, frame_stride)
    frames = max((B - 1) * frame_stride + H, frames_avail) + 2
    feat = (3.0 * rng.standard_normal((frames, W)) - 6.0).astype(np.float32)
    feat[frames_avail:] = 123.0
    w = (rng.standard_normal((C, 1, 3, 3)) * 0.3).astype(np.float32)
    scale, shift = signed_scale(rng, C), (rng.standard_normal(C) * 0.3).astype(np.float32)
    ref, bound = fm.stem_case(feat, w, scale, shift, B, H, W, frame_stride, frames_avail)
    if frames_avail == 0:
        assert np.array_equal(ref, np.broadcast_to(np.maximum(shift.astype(np.float64), 0).reshape(1, C, 1, 1), ref.shape))
    else:
        assert np.abs(ref).max() > 1.0
    out = torch.full((act_rows(B, H, W) * C,), FILL, device="cuda", dtype=torch.float16)
    fg, wg, sc, sh = dev(feat), dev(w), dev(scale), dev(shift)
    h.check(lib.lad_f16_stem_fwd(h.ptr(fg), h.ptr(wg), h.ptr(sc), h.ptr(sh), h.ptr(out), B, H, W, C, frame_stride, frames_avail, st),
            "lad_f16_stem_fwd")
    torch.cuda.synchronize()
    worst_ratio(out, ref, bound, B, f"stem_fwd ({B},{H},{W}) stride={frame_stride} avail={frames_avail}")


# ---- lad_f16_pool_fwd ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,C", [(3, 13, 6, 16), (2, 4, 4, 16), (2, 7, 9, 16), (5, 12, 22, 32), (300, 13, 6, 16)])
def test_pool_against_float64(B, H, W, C):
    """lad_f16_pool_fwd: the fp32 term of the bound alone (the output is fp32); rows and columns behind the last whole 4 x 4 window hold
    1000.0; the output order is avg_pool2d(...).flatten(1)."""
    h = _lib()
    lib = h.lib()
    rng = rng_of(B, H, W, C)
    x = fm.half(rng.standard_normal((B, C, H, W)))
    x[:, :, 4 * (H // 4):, :] = 1000.0
    x[:, :, :, 4 * (W // 4):] = 1000.0
    ref, bound = fm.pool_case(x)
    want = F.avg_pool2d(torch.from_numpy(x), 4).flatten(1).numpy()
    assert ref.shape == want.shape and np.abs(ref - want).max() <= 1e-14 and np.abs(ref).max() < 10.0
    pooled = torch.full((B * ref.shape[1],), FILL, device="cuda")
    xin = pnhwc_half(x)
    h.check(lib.lad_f16_pool_fwd(h.ptr(xin), h.ptr(pooled), B, H, W, C, h.stream_handle()), "lad_f16_pool_fwd")
    torch.cuda.synchronize()
    err = np.abs(pooled.cpu().numpy().astype(np.float64).reshape(ref.shape) - ref)
    worst = float((err / bound).max())
    print(f"pool_fwd ({B},{H},{W},{C}): max err / bound = {worst:.3f}")
    assert not (~(err <= bound)).any(), (int((~(err <= bound)).sum()), worst)
