"""The arithmetic of the fp16 base kernels (csrc/conv_f16.hip: epilogue_f16, stem_f16_kernel, pool_f16_kernel, pack_f16_kernel) restated
in float64, with a DERIVED bound on what a correct kernel may differ from it: the model of tests/test_f16_model_cpu.py and
tests/test_f16_ops_gpu.py.  numpy and torch in float64; imports nothing from the library.

What the kernels compute
  convolution   x, w IEEE halfs; the n = taps * cin products (each exact in fp32: 11 + 11 significant bits) summed in fp32 on the matrix
                cores in an unspecified order -> acc;  t = fmaf(acc, scale, shift) [+ float(addend)];  max(t, 0) if relu;  ONE conversion
                to half.  3x3: pad 1; 1x1: pad 0; stride 2 gives ceil(H / 2) x ceil(W / 2).
  stem          fp32 features and weights, a nine-term fmaf chain -> acc;  max(fmaf(acc, scale, shift), 0);  one conversion to half.
                Image b = frames [b * frame_stride, b * frame_stride + H), zero from frames_avail on, zero-padded above and below.
  pool          the fp32 sum of the 16 halfs of a 4 x 4 window, times 1/16 (exact), written as fp32.

The reference evaluates these formulas in float64 ON THE SAME OPERANDS (the half-rounded x, w, addend; scale, shift, features and stem
weights as the fp32 numbers they are stored as) and returns t_ref, the value before the final rounding.

The bound, per output element.  u = 2^-23 (one fp32 operation is within u |result| whether it rounds to nearest, 2^-24, or truncates,
2^-23: the accumulation inside the MFMA may do either).  n = number of products, S = their exact sum, A = sum |x_i w_i| (the same
convolution on |x|, |w|).
  accumulation   any order of n fp32 additions of exact products: |acc - S| <= ((1 + u)^(n-1) - 1) A <= n u A  (n u < 1e-4 here, the
                 second-order part of (1 + u)^(n-1) is inside the slack between n - 1 and n).  The stem's fmaf chain: 9 roundings, same form.
  epilogue       fmaf: one rounding of acc * scale + shift, <= u (|S scale| + |shift|) up to second order; the addition of the addend: one
                 more, <= u (|S scale| + |shift| + |addend|).  Together <= 2 u (|S scale| + |shift| + |addend|).
      e32   = n u A |scale|  +  2 u (|S scale| + |shift| + |addend|)
  half rounding  round to nearest of the fp32 value t (|t - t_ref| <= e32): <= 2^-11 |t| <= 2^-11 (|t_ref| + e32) for normal halfs; below 2^-14
                 at most half a subnormal step, which the constant 2^-24 (one whole step) covers.
      bound = 2^-11 (|t_ref| + e32)  +  e32  +  2^-24
ReLU is monotone and 1-Lipschitz and commutes with the rounding, so the same bound holds against max(t_ref, 0).  Nothing in the bound
is measured.  Pool writes fp32: its bound is e32 alone (n = 16, scale = 1/16, no shift, no addend).
"""
import numpy as np
import torch

U32 = 2.0 ** -23
HALF_RND = 2.0 ** -11
HALF_SUB = 2.0 ** -24


def half(a):
    """Round to IEEE half (nearest even) and return the values as float64."""
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float64)


def out_size(n, stride):
    return (n + stride - 1) // stride


def _t64(a, like=None):
    """a (numpy, torch, a list) as a float64 torch tensor, on the device of `like` (its own if it is a tensor, else the CPU)."""
    t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))
    return t.to(dtype=torch.float64, device=like.device if like is not None else t.device)


def _back(t, like):
    """A result in the kind of the operand it came from: numpy for numpy, a tensor (where it lives) for a tensor."""
    return t if isinstance(like, torch.Tensor) else t.numpy()


def conv_sum(x, w, stride=1):
    """sum over (ci, ky, kx) of x[b, ci, stride y + ky - pad, stride x + kx - pad] w[co, ci, ky, kx] in float64, zeros outside the image.
    x (B, Cin, H, W), w (Cout, Cin, k, k) with k = 3 (pad 1) or k = 1 (pad 0) -> (B, Cout, ceil(H / stride), ceil(W / stride)).
    A loop over the taps; each tap is one float64 matrix product over the channels.  numpy in, numpy out; torch tensors are taken where
    they lie (the large batches of the GPU tests: the same loop in float64 on the device) and a tensor comes back."""
    xt = _t64(x)
    wt = _t64(w, xt)
    B, cin, H, W = xt.shape
    cout, cin_w, k, k2 = wt.shape
    assert cin == cin_w and k == k2 and k in (1, 3) and stride in (1, 2)
    pad = k // 2
    Ho, Wo = out_size(H, stride), out_size(W, stride)
    # channels last (a tap's operand is (positions, Cin)); k // 2 zero rows / columns in front, enough behind for every tap
    xp = torch.zeros((B, max(stride * (Ho - 1) + k, H + pad), max(stride * (Wo - 1) + k, W + pad), cin), dtype=torch.float64, device=xt.device)
    xp[:, pad:pad + H, pad:pad + W] = xt.permute(0, 2, 3, 1)
    out = torch.zeros((B * Ho * Wo, cout), dtype=torch.float64, device=xt.device)
    for ky in range(k):
        for kx in range(k):
            xs = xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]
            out += xs.reshape(-1, cin) @ wt[:, :, ky, kx].T
    return _back(out.reshape(B, Ho, Wo, cout).permute(0, 3, 1, 2).contiguous(), x)


def epilogue_bound(S, A, n, scale, shift, addend=None, relu=False, to_half=True):
    """(ref, bound) from the exact sum S, the absolute sum A and the number of products n (see the module docstring).
    scale / shift: per channel (axis 1); addend: like S, or None.  numpy or torch like conv_sum, following S."""
    St = _t64(S)
    At, sc, sh = _t64(A, St), _t64(scale, St).reshape(1, -1, 1, 1), _t64(shift, St).reshape(1, -1, 1, 1)
    ad = torch.zeros_like(St) if addend is None else _t64(addend, St)
    t_ref = St * sc + sh + ad
    e32 = n * U32 * At * sc.abs() + 2 * U32 * ((St * sc).abs() + sh.abs() + ad.abs())
    bound = HALF_RND * (t_ref.abs() + e32) + e32 + HALF_SUB if to_half else e32 + torch.zeros_like(St)
    return _back(t_ref.clamp(min=0.0) if relu else t_ref, S), _back(bound, S)


def is_half(a):
    t = _t64(a)
    return bool(torch.equal(t.to(torch.float16).double(), t))


def conv_case(x, w, scale, shift, addend=None, relu=False, stride=1):
    """The convolution kernels: x, w, addend hold half values (any float dtype), scale / shift fp32 values -> (ref, bound), float64,
    shape (B, Cout, Ho, Wo); numpy or torch like conv_sum, following x."""
    assert is_half(x) and is_half(w) and (addend is None or is_half(addend)), "operands must be half values"
    S, A = conv_sum(x, w, stride), conv_sum(abs(x), abs(w), stride)
    n = w.shape[1] * w.shape[2] * w.shape[3]
    return epilogue_bound(S, A, n, scale, shift, addend, relu)


def stem_images(feat, B, H, W, frame_stride, frames_avail):
    """The B images the stem reads: image b = frames [b * frame_stride, b * frame_stride + H) of feat ((frames, W)), zero from
    frames_avail on (rows of feat behind it are NOT read) -> (B, 1, H, W) float64."""
    feat = np.asarray(feat, np.float64)
    img = np.zeros((B, 1, H, W))
    for b in range(B):
        for y in range(H):
            f = b * frame_stride + y
            if f < frames_avail:
                img[b, 0, y] = feat[f]
    return img


def stem_case(feat, w, scale, shift, B, H, W, frame_stride, frames_avail):
    """lad_f16_stem_fwd: fp32 feat (frames, W), fp32 w (Cout, 1, 3, 3) -> (ref, bound) of relu(bn(conv)), (B, Cout, H, W)."""
    x = stem_images(np.asarray(feat, np.float32), B, H, W, frame_stride, frames_avail)
    w = np.asarray(np.asarray(w, np.float32), np.float64)
    S, A = conv_sum(x, w), conv_sum(np.abs(x), np.abs(w))
    return epilogue_bound(S, A, 9, scale, shift, None, True)


def pool_case(x):
    """lad_f16_pool_fwd: x (B, C, H, W) half values -> (ref, bound), (B, C * PH * PW) in the order f = c PH PW + ph PW + pw.  Rows and
    columns from 4 (H // 4), 4 (W // 4) on are not read."""
    x = np.asarray(x, np.float64)
    assert np.array_equal(half(x), x)
    B, C, H, W = x.shape
    PH, PW = H // 4, W // 4
    S, A = np.zeros((B, C, PH, PW)), np.zeros((B, C, PH, PW))
    for dy in range(4):
        for dx in range(4):
            v = x[:, :, dy:4 * PH:4, dx:4 * PW:4]
            S += v
            A += np.abs(v)
    ref, bound = epilogue_bound(S, A, 16, np.full(C, 0.0625), np.zeros(C), None, False, to_half=False)
    return ref.reshape(B, -1), bound.reshape(B, -1)


def pack_image(w):
    """lad_f16_pack_weights: w fp32 (cout, cin, taps) (or (cout, cin, k, k)) -> float16 [taps][cin / 16][2][COUTP][8] with
    element (tap, s, h, co, j) = half(w[co][16 s + 8 h + j][tap]), COUTP = 32 ceil(cout / 32), +0 for co >= cout."""
    w = np.asarray(w, np.float32)
    cout, cin = w.shape[:2]
    w = w.reshape(cout, cin, -1)
    taps = w.shape[2]
    assert cin % 16 == 0 and taps in (1, 9)
    coutp = 32 * ((cout + 31) // 32)
    img = np.zeros((taps, cin // 16, 2, coutp, 8), np.float16)
    for tap in range(taps):
        for s in range(cin // 16):
            for h in range(2):
                for j in range(8):
                    img[tap, s, h, :cout, j] = w[:, 16 * s + 8 * h + j, tap].astype(np.float16)
    return img


# ---- an fp32 emulation of the kernel arithmetic and its mutants (tests/test_f16_model_cpu.py: the bound holds, the mutants are seen) ----
def _trunc24(v):
    """float64 -> the nearest-towards-zero number of 24 significant bits."""
    m, e = np.frexp(v)
    return np.ldexp(np.trunc(m * 2.0 ** 24) * 2.0 ** -24, e)


def im2col(x, k, stride):
    """(B, Cin, H, W) -> (k * k * Cin, B * Ho * Wo): row (ky * k + kx) * Cin + ci, the kernels' tap-major order."""
    B, cin, H, W = x.shape
    pad = k // 2
    Ho, Wo = out_size(H, stride), out_size(W, stride)
    xp = np.zeros((B, cin, max(stride * (Ho - 1) + k, H + pad), max(stride * (Wo - 1) + k, W + pad)))
    xp[:, :, pad:pad + H, pad:pad + W] = x
    rows = []
    for ky in range(k):
        for kx in range(k):
            xs = xp[:, :, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]
            rows.append(xs.transpose(1, 0, 2, 3).reshape(cin, -1))
    return np.concatenate(rows, 0)


def emulate_conv(x, w, scale, shift, addend=None, relu=False, stride=1, truncate=False, drop_product=None, drop_tap_at_edge=None,
                 addend_after_relu=False):
    """The convolution kernels' arithmetic in fp32, sequentially: acc = fl(acc + x_i w_i) over the n products in tap-major order
    (fl = round to nearest, or truncation to 24 bits), fmaf, + addend, ReLU, one conversion to half.  Returns (out, affected): out
    (B, Cout, Ho, Wo) half values as float64, affected the outputs a mutant changed the exact sum of.
    Mutants: drop_product = k: product k of every output is left out; drop_tap_at_edge = tap: that tap is left out at the outputs of the
    image's last row and last column; addend_after_relu: max(fmaf, 0) + addend."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    B, cin, H, W = x.shape
    cout, _, k, _ = w.shape
    Ho, Wo = out_size(H, stride), out_size(W, stride)
    cols = im2col(x, k, stride)                                       # (n, M)
    wm = w.transpose(0, 2, 3, 1).reshape(cout, -1)                    # (Cout, n), same order
    n, M = cols.shape
    edge = np.zeros((B, Ho, Wo), bool)
    edge[:, Ho - 1, :] = True
    edge[:, :, Wo - 1] = True
    edge = edge.reshape(1, M)
    acc = np.zeros((cout, M), np.float32)
    affected = np.zeros((cout, M), bool)
    for i in range(n):
        p = wm[:, i, None] * cols[None, i, :]                         # exact: 22 significant bits
        if drop_product is not None and i == drop_product:
            affected |= p != 0
            continue
        if drop_tap_at_edge is not None and i // cin == drop_tap_at_edge:
            affected |= (p != 0) & edge
            p = np.where(edge, 0.0, p)
        if truncate:
            acc = _trunc24(acc.astype(np.float64) + p).astype(np.float32)
        else:
            acc = acc + p.astype(np.float32)
    sc = np.asarray(scale, np.float32).astype(np.float64).reshape(-1, 1)
    sh = np.asarray(shift, np.float32).astype(np.float64).reshape(-1, 1)
    t = (acc.astype(np.float64) * sc + sh).astype(np.float32)         # fmaf: one rounding (the product is exact in float64)
    ad = None if addend is None else np.asarray(addend, np.float32).reshape(B, cout, -1).transpose(1, 0, 2).reshape(cout, M)
    if addend_after_relu:
        affected |= (t < 0) | (t + ad < 0)
        t = np.maximum(t, np.float32(0)) + ad
    else:
        if ad is not None:
            t = t + ad
        if relu:
            t = np.maximum(t, np.float32(0))
    out = t.astype(np.float16).astype(np.float64)
    shape = lambda a: np.ascontiguousarray(a.reshape(cout, B, Ho, Wo).transpose(1, 0, 2, 3))
    return shape(out), shape(affected)
