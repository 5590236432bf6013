"""Launch sequencer for the ResNetBigger hot path on the MI355X (no autograd, no torch compute kernels).

`ResNetEngine` walks the layers of a `models.ResNetBigger` and issues the C-ABI calls of liblad_hip.so
(include/lad_hip.h) for
    forward            models.py:222-239 (ResNetBigger.forward), models.py:110-115 (ResidualBlock.forward)
    backward           what loss.backward() computes at train.py:289
    clip + Adam        train.py:291-295
on torch-owned device buffers.  PyTorch is used for memory, streams and (optionally) the dropout RNG only.

Memory plan.  Parameters live in ONE flat fp32 buffer in `model.parameters()` order
(each tensor 16-byte aligned), gradients in a second flat buffer of the same shape -> one all-reduce, one
norm, one Adam launch.  Activations are "PNHWC" with shared zero borders (csrc/lad_device.h): [batch][H+1][W+1][C] plus
a short tail; a plan for batch size B owns every activation / gradient buffer and is reused step after
step (no allocation inside the step).  Everything derived from the weights -- packed MFMA images, fp16 images, eval-mode
BatchNorm folds -- belongs to the model (_ConvParams / _BnParams, one record per layer); the layer table of an input geometry
(_blocks_for) holds sizes and points at those records.
"""
import contextlib
import ctypes
import functools
import math
import struct
from typing import FrozenSet, NamedTuple, Optional, Tuple

import torch

import _hip

_VP = ctypes.c_void_p


# windows per launch group of predict_windows.  Half precision: the layers that still run per window (levels 3 and 4) are small
# launches, and 8192 windows amortise them better than 2048 did (2.03 -> 2.28 M windows/s on the 60 min channel); f32 keeps
# every window's level-1 activation (1.2 MB), so its groups stay at 2048
PREDICT_CHUNK = {"fp16": 8192, "fp32": 2048}
# the stage widths every kernel and fusion of the library is instantiated for (config.MODEL_MAP['resnet_base']); other widths run on the
# exact-f32 kernels (ResNetEngine.base_widths)
BASE_WIDTHS = (64, 32, 16, 16)
# fp16: windows whose level-1 / level-2 frame streams are computed in one go (engine.stream_super): five tensors of 5.8 KB per frame at
# level 1 -- 10 GB for a 60-minute channel's 360,000 windows, 30 GB at this cap
STREAM_SUPER_MAX = 1 << 20


_NOT_TIMED = contextlib.nullcontext()


class _Declined(Exception):
    """Leaves the body of ResNetEngine._marked without an event pair (_try_launch)."""


class _LazyLevels(dict):
    """Rotating activation buffers of an eval plan, keyed by resolution level, created on first use."""

    def __init__(self, make):
        super().__init__()
        self._make = make

    def __missing__(self, key):
        value = self[key] = self._make(key)
        return value


def _align4(n):
    return (n + 3) & ~3


def _b3_shape(cin, cout, taps, stride):
    """A layer shape the split-operand (bf16 x 3, f16 x 2) stride-1 kernels have instances for."""
    return cin == cout and cin in (64, 32) and taps == 9 and stride == 1


def _s2b3_shape(cin, cout, taps, stride):
    """The 64 -> 32 stride-2 transition, which has a split-operand kernel of its own (with its 1x1 shortcut)."""
    return cin == 64 and cout == 32 and taps == 9 and stride == 2


class _ConvParams:
    """One convolution of the MODEL: its views into the flat parameter / gradient buffers and every packed image of its weights.
    Which images exist follows from the layer's shape alone, so the layer's _ConvSpec of every geometry points here (cs.par);
    ResNetEngine._pack_weights / _eval_prepare keep the images current."""

    def __init__(self, name, cin, cout, taps, stride, base_widths, views, lib, dev):
        self.name, self.cin, self.cout, self.taps = name, cin, cout, taps
        self.w, self.gw = views[name + ".weight"]
        self.b, self.gb = views.get(name + ".bias", (None, None))   # (a 1x1 shortcut has none)
        self.shortcut = None   # conv1 of a block with a projection shortcut: that convolution's record (the s2b3 images hold both)

        def image(n, dtype):
            return torch.zeros(int(n), device=dev, dtype=dtype)

        # exact-f32 MFMA images, forward / data gradient, and the fp16 image of the half-precision inference kernels
        self.wt_f = image(lib.lad_conv_packed_weight_floats(cout, cin, taps, 0), torch.float32)
        self.wt_d = image(lib.lad_conv_packed_weight_floats(cout, cin, taps, 1), torch.float32)
        self.wt_h = image(lib.lad_f16_packed_weight_halfs(cout, cin, taps), torch.float16)
        if _b3_shape(cin, cout, taps, stride) and base_widths:
            # split (bf16 x 3) images, forward and data gradient, and the f16 x 2 images (csrc/conv_h2.hip)
            self.wt3_f, self.wt3_d = (image(lib.lad_conv_b3c_packed_weight_bytes(cin), torch.uint8) for _ in range(2))
            self.wt2_f, self.wt2_d = (image(lib.lad_conv_h2_packed_weight_bytes(cin), torch.uint8) for _ in range(2))
        if _s2b3_shape(cin, cout, taps, stride) and base_widths:
            # ... with its shortcut: one split image per direction (3x3 + 1x1 together)
            self.wt3_s2f = image(lib.lad_conv_s2b3_packed_weight_bytes(), torch.uint8)
            self.wt3_s2d = image(lib.lad_conv_s2b3_dgrad_packed_weight_bytes(), torch.uint8)


class _BnParams:
    """One BatchNorm of the MODEL: affine parameters and their gradients (views into the flat buffers), the running statistics,
    and the eval-mode fold (scale, shift) that ResNetEngine._eval_prepare keeps current (conv_bias: the bias of the convolution in
    front, which the fold's shift absorbs; the head's two BatchNorm1d are applied by the head kernels and leave theirs unused)."""

    def __init__(self, name, c, views, bufs, dev, conv_bias=None):
        self.name, self.c, self.conv_bias = name, c, conv_bias
        self.g, self.gg = views[name + ".weight"]
        self.b, self.gb = views[name + ".bias"]
        self.rm, self.rv = bufs[name + ".running_mean"], bufs[name + ".running_var"]
        if not (self.rm.is_cuda and self.rm.is_contiguous() and self.rm.dtype == torch.float32):
            raise _hip.LadHipError(f"{name}: running statistics must be contiguous float32 GPU tensors")
        self.fold = (torch.zeros(c, device=dev), torch.zeros(c, device=dev))


class _ConvSpec:
    """One convolution on one input geometry: sizes and which kernels have an instance for them.  par: the layer's _ConvParams
    (None in the tensor-free tables of block_geometry)."""

    def __init__(self, name, cin, cout, taps, stride, h_in, w_in, base_widths=True):
        self.name, self.cin, self.cout, self.taps, self.stride = name, cin, cout, taps, stride
        self.h_in, self.w_in = h_in, w_in
        self.h_out = (h_in + stride - 1) // stride
        self.w_out = (w_in + stride - 1) // stride
        # what the split-operand kernels have instances for, at the stage widths they were validated on (shape only: whether a step
        # uses them is train_schedule's decision).  b3: forward and data gradient (64 or 32 channels); b3_full: 64 channels, where
        # the sign bits exist as well
        self.b3 = _b3_shape(cin, cout, taps, stride) and w_in <= 46 and base_widths
        self.b3_full = self.b3 and cin == 64
        self.b3_wgrad = self.b3 and (cin == 64 or w_in <= 30)   # the 32-channel weight-gradient window holds 64 rows + 2 (W + 2)
        # the 64 -> 32 stride-2 transition with its shortcut: one split image per direction (3x3 + 1x1 together)
        self.s2b3 = _s2b3_shape(cin, cout, taps, stride) and (w_in + 1) // 2 <= 45 and base_widths
        self.par = None

    def rows(self, B):
        """Rows of the layer's input tensor for batch B (shared zero borders + tail)."""
        return B * (self.h_in + 1) * (self.w_in + 1) + self.w_in + 2


class _BlockSpec:
    """conv1 / conv2 / sc_conv: _ConvSpec of this geometry; bn1 / bn2 / sc_bn: the model's _BnParams."""

    def __init__(self, name):
        self.name = name
        self.conv1 = self.bn1 = self.conv2 = self.bn2 = self.sc_conv = self.sc_bn = None


def block_geometry(stem_cout, filter_sizes, H, W, base_widths):
    """The residual blocks of ResNetBigger for an (H, W) input, convolutions only and without tensors (models.py:73-76)."""
    blocks = []
    cin, h, w = stem_cout, H, W
    for bi, cout in enumerate(filter_sizes, start=1):
        for j in range(2):
            name = f"block{bi}.{j}"
            stride = 2 if (j == 0 and bi > 1) else 1
            b = _BlockSpec(name)
            b.conv1 = _ConvSpec(name + ".conv1", cin, cout, 9, stride, h, w, base_widths)
            h, w = b.conv1.h_out, b.conv1.w_out
            b.conv2 = _ConvSpec(name + ".conv2", cout, cout, 9, 1, h, w, base_widths)
            if stride != 1 or cin != cout:
                b.sc_conv = _ConvSpec(name + ".shortcut.0", cin, cout, 1, stride, b.conv1.h_in, b.conv1.w_in, base_widths)
            blocks.append(b)
            cin = cout
    return blocks


class _ConvChoice(NamedTuple):
    """Kernels of one convolution in one training step."""
    arith: str         # forward and data gradient: "f32" (exact-f32 MFMA) | "b3" (bf16 x 3) | "h2" (f16 x 2)
    wgrad: str         # weight gradient: "f32" | "b3c" | "h2"
    wgrad_bn: bool     # the weight-gradient launch may apply the BatchNorm backward of the layer's own output (csrc/wgrad_mfma.hip, DOBN)
    label_fwd: str     # kernel_events labels of the two launches (bench.py keys on them)
    label_dgrad: str


class _BlockChoice(NamedTuple):
    entry: str             # "s2b3" | "s2_fused" (conv1 and the 1x1 shortcut in one launch, forward and data gradient) | "plain"
    a1_virtual: bool       # relu(bn1(c1)) is formed while conv2 and its weight gradient stage c1: never written
    bits: bool             # the residual ReLU's decisions travel as sign bits (lad_bn_act_bits)
    # whose arithmetic carries the first pass of the BatchNorm backward that consumes a data gradient: None, "f32" (fuse_bn_bwd:
    # lad_conv_fwd_bnstat, whatever the layer's own arithmetic) or "split" (fuse_bn_bwd_b3: the layer's split-operand launch)
    dgrad2_bn: Optional[str]   # conv2's data gradient + this block's bn1
    dgrad1_bn: Optional[str]   # conv1's data gradient + bn2 of the block below
    sc_wgrad_fused: bool   # stride-2 block: the shortcut's weight gradient as a tenth tap of conv1's
    conv1: _ConvChoice
    conv2: _ConvChoice
    sc: Optional[_ConvChoice]


class _TrainSchedule(NamedTuple):
    """Every kernel choice of one train-mode forward and its backward (train_schedule)."""
    blocks: Tuple[_BlockChoice, ...]
    stem_onepass: bool
    images: FrozenSet[Tuple[str, str]]   # packed split-operand weight images the step reads: ("h2" | "b3c" | "s2b3", convolution)
    opts: Tuple[Tuple[str, object], ...]  # the flag values it was built from


_ROW_LIMIT = (1 << 31) - (1 << 20)


def train_schedule(blocks, B, opts, stem_onepass):
    """The kernels of a training step at batch B: a pure function of the layer geometry (block_geometry) and the flag values
    (opts: {name of KERNEL_OPTIONS: value}).  forward(train=True) stores the result in its plan and backward() reads nothing else,
    so the two passes cannot disagree (a virtual a1 that was never written must not be read from HBM)."""
    o = dict(opts)

    def arith(cs):
        # 64 channels (round 3): conv_b3x / wgrad_b3x address a tensor relative to the workgroup's own rows (64-bit bases),
        # only row NUMBERS are 32-bit.  32 channels: the weight gradient still runs on the round-2 kernel, whose byte offsets
        # are 32-bit (2 GiB per tensor = batch > 14,000 at 32 x 50 x 22); past that the layer runs on the exact-f32 kernels
        fits = cs.rows(B) < _ROW_LIMIT if cs.cin == 64 else cs.rows(B) * cs.cin * 4 < _ROW_LIMIT
        if not (o["bf16x3"] and cs.b3 and (cs.cin == 64 or o["bf16x3_32"]) and fits):
            return "f32"
        return "h2" if o["f16x2"] and (cs.cin == 64 or o["f16x2_32"]) else "b3"

    def conv(cs, dgrad_f32=False, label_fwd=None):
        a = arith(cs)
        # same split arithmetic as the forward / data-gradient launches of the layer; at 32 channels bf16 x 3 only
        wg = "f32" if a == "f32" or not cs.b3_wgrad else "h2" if a == "h2" and cs.cin == 64 else "b3c"
        f32_label = f"conv_s{cs.stride}<{cs.cin},{cs.cout},{cs.taps}>"
        return _ConvChoice(a, wg, bool(o["fuse_bn_bwd_wgrad"]) and wg == "h2",
                           label_fwd or (f32_label if a == "f32" else f"conv_{a}<{cs.cin},{cs.cout},{cs.taps}>"),
                           f"conv_s1<{cs.cout},{cs.cin},{cs.taps}>" if a == "f32" or dgrad_f32 else f"conv_{a}<{cs.cout},{cs.cin},{cs.taps}>")

    out = []
    for bi, b in enumerate(blocks):
        c1, c2, sc = b.conv1, b.conv2, b.sc_conv
        a1, a2 = arith(c1), arith(c2)
        below_bits = bi > 0 and out[bi - 1].bits
        entry = "plain"
        if c1.stride != 1 and o["fuse_s2_shortcut"]:
            entry = "s2b3" if o["bf16x3"] and o["s2_b3"] and c1.s2b3 and c1.rows(B) < _ROW_LIMIT else "s2_fused"
        # identity-shortcut blocks on the split-operand kernels: the residual ReLU's decisions travel as sign bits
        # (8 bytes per row instead of re-reading y and writing / re-reading the masked gradient: csrc/bn.hip, conv_b3.hip)
        bits = bool(o["relu_bits"]) and sc is None and c1.b3_full and a1 != "f32" and not o["fuse_bn_bwd"]
        dgrad2_bn = "f32" if o["fuse_bn_bwd"] else "split" if o["fuse_bn_bwd_b3"] and a2 != "f32" else None
        if c1.stride != 1:   # the sums of the block below's bn2 in the epilogue, when that block keeps sign bits
            fused = entry == "s2b3" or (entry == "s2_fused" and c1.cin == 64 and c1.cout == 32)
            dgrad1_bn = "split" if fused and o["fuse_bn_bwd_b3"] and below_bits else None
        elif bits:
            dgrad1_bn = "split" if o["fuse_bn_bwd_b3"] and below_bits else None
        else:   # (the f32 epilogue needs y and c2 of the block below: identity shortcuts only; the stem keeps no convolution output)
            dgrad1_bn = "f32" if o["fuse_bn_bwd"] and bi > 0 and blocks[bi - 1].sc_conv is None else None
        s2_label = f"conv_{'s2b3' if entry == 's2b3' else 's2'}<{c1.cin},{c1.cout},9>" if c1.stride != 1 else None
        out.append(_BlockChoice(entry, bool(o["virtual_a1"]) and a2 != "f32" and c2.b3_wgrad, bits, dgrad2_bn, dgrad1_bn,
                                c1.stride != 1 and bool(o["fuse_s2_shortcut_wgrad"]),
                                conv(c1, dgrad1_bn == "f32", s2_label), conv(c2, dgrad2_bn == "f32"), conv(sc) if sc is not None else None))
    images = {(ch.arith if ch.arith == "h2" else "b3c", cs.name) for b, blk in zip(blocks, out)
              for cs, ch in ((b.conv1, blk.conv1), (b.conv2, blk.conv2)) if ch.arith != "f32"}
    images |= {("s2b3", b.conv1.name) for b, blk in zip(blocks, out) if blk.entry == "s2b3"}
    return _TrainSchedule(tuple(out), bool(stem_onepass), frozenset(images), tuple(o.items()))


def conv_s1_entry(arith, cin, in_coef=False, gated=False, bn=None):
    """Entry point of a stride-1 3x3 / 1x1 convolution launch (forward, or data gradient = convolution with the flipped image).
    in_coef: BatchNorm + ReLU applied to the input while staging; gated: the addend passes a sign-bit gate; bn: the epilogue
    leaves the sums of a BatchNorm backward whose ReLU mask is recomputed from its input ("x"), read from sign bits ("bits")
    or from its output ("y").  A combination the library has no kernel for is an error, not a fall-back."""
    if arith == "h2" and bn != "y":
        return "lad_conv_h2"
    if arith == "b3" and in_coef and not gated and bn is None:
        return "lad_conv_b3c_fwd_f32_bnrelu"
    if arith == "b3" and gated and not in_coef and cin == 64 and bn in (None, "bits"):
        return "lad_conv_b3_dgrad_bnstat" if bn else "lad_conv_b3_fwd_f32_gated"
    if arith == "b3" and not in_coef and not gated and bn in (None, "x"):
        return "lad_conv_b3c_dgrad_bnstat" if bn else "lad_conv_b3c_fwd_f32"
    if arith == "f32" and not in_coef and not gated and bn != "bits":
        return "lad_conv_fwd_bnstat" if bn else "lad_conv_fwd"
    raise _hip.LadHipError(f"no stride-1 convolution kernel for arithmetic {arith!r} at {cin} channels with in_coef={in_coef}, "
                           f"gated={gated}, bn={bn!r}")


def conv_wgrad_entry(kind, in_coef=False, bn=False):
    """Entry point of a stride-1 weight-gradient launch.  in_coef: BatchNorm + ReLU applied to the input while staging (a virtual
    a1); bn: the launch applies the BatchNorm backward of the layer's own output and writes the gradient its data gradient reads."""
    if kind == "h2":
        return "lad_conv_wgrad_h2_bnbwd" if bn else "lad_conv_wgrad_h2"
    if kind == "b3c" and not bn:
        return "lad_conv_wgrad_b3c"
    if kind == "f32" and not bn and not in_coef:
        return "lad_conv_wgrad"
    raise _hip.LadHipError(f"no weight-gradient kernel for {kind!r} with in_coef={in_coef}, bn={bn}")


# ---------------------------------------------------------------------------------------- sliding-window inference: the layout
def _s2_shortcut_rides(b, opts):
    """fp16 eval: the 1x1 shortcut of down-sampling block b inside conv1's launch?  Measured per group of 8,192 windows
    (profiles/r05_infer_s2_shortcut.log): 64 -> 32: 344 us against 314 + 72; 16 -> 16: 41 against 30 + 14; 32 -> 16: 219 against
    157 + 44 -- there the second accumulator costs the launch more than the second gather saves."""
    return bool(opts["f16_s2_shortcut_fused"]) and b.conv1.cin != 32


def _block_fits_lds(b, B, opts, hw=None):
    """Worth trying lad_f16_block_fwd (include/lad_hip.h) on B images of block b (hw: their height and width when they are not the
    spec's own, as for the strips of a window geometry)?  Identity block; 64 channels on >= 256 images of at most 512 positions
    (the boundary strips of level 1), or 16 / 32 channels on >= 512 small images (the strips of level 2, the windows at levels
    3 and 4).  The entry point itself answers LAD_NOT_COVERED for what does not fit a CU's LDS."""
    c = b.conv1
    if b.sc_conv is not None or c.stride != 1 or c.taps != 9 or c.cin != c.cout:
        return False
    h, w = hw if hw is not None else (c.h_in, c.w_in)
    img = (h + 1) * (w + 1)
    if c.cin == 64:
        return bool(opts["strip_block_fused"]) and B >= 256 and img <= 512 and img + w <= 562
    return bool(opts["small_block_fused"]) and c.cin in (16, 32) and B >= 512 and img <= 2048


def _tail_blocks_ok(tail):
    """The layers lad_f16_tail_fwd runs: two (down-sampling block with a 1x1 shortcut, identity block) pairs, 32 -> 16 -> 16 channels."""
    if len(tail) != 4:
        return False
    for k, b in enumerate(tail):
        down = k % 2 == 0
        cin = 32 if k == 0 else 16
        if (b.conv1.cin, b.conv1.cout, b.conv1.taps, b.conv1.stride) != (cin, 16, 9, 2 if down else 1):
            return False
        if (b.conv2.cin, b.conv2.cout, b.conv2.taps, b.conv2.stride) != (16, 16, 9, 1):
            return False
        if down != (b.sc_conv is not None) or (down and (b.sc_conv.cin, b.sc_conv.cout, b.sc_conv.taps, b.sc_conv.stride) != (cin, 16, 1, 2)):
            return False
    return True


class _StreamLayout(NamedTuple):
    """Where everything of one group of B sliding windows lies and which launches are tried on it (stream_layout).  Rows are rows of
    a PNHWC tensor (one position, all channels).  cat = [strips: n_strip_max images of img_t_rows][stream image][spare rows] at
    level 1, cat2 = [strips: n_strip2_max images of img_t2][phase-0 stream image][phase-1 stream image][tail] at level 2."""
    B: int
    H: int
    W: int
    half: bool
    mode: str                  # "per_window" | "assembled" | "direct" | "shared2"
    run: Optional[Tuple[int, int]]   # (windows of the run, its largest group) when the streams are the run's, not the group's
    # level 1 (None from Ht on in "per_window"; stream_row0 and cat_rows None in "assembled": no common buffer there)
    n1: int                    # leading stride-1 identity blocks at full resolution
    band: int                  # rows of a window that differ from the stream at the end of level 1 (either end)
    Ht: Optional[int]          # rows of a strip: the top band rows of one window over the bottom band rows of another
    Hs: Optional[int]          # rows of the GROUP's stream image (stream_rows: of the image the windows read)
    n_strip: Optional[int]     # strips of this group: one per frame offset
    n_strip_max: Optional[int]   # ... of the run's largest group: what cat has room for
    img_t_rows: Optional[int]  # rows of one strip image
    stream_row0: Optional[int]   # first row of the stream image in cat (of the run's first window: a group adds d * (W + 1))
    cat_rows: Optional[int]
    # level 2 (None outside "shared2")
    k3: Optional[int]          # the block that leaves level 2 (the next down-sampling one)
    H2: Optional[int]
    W2: Optional[int]
    band2: Optional[int]
    Ht2: Optional[int]
    shift2: Optional[int]      # level-2 strip s = top of window s over bottom of window s - shift2
    h2s: Optional[int]         # rows of one phase's stream image
    n_strip2: Optional[int]
    n_strip2_max: Optional[int]
    img_t2: Optional[int]
    img_s2: Optional[int]
    stream2_base: Optional[int]   # first row of the phase-0 stream image in cat2
    rows2: Optional[int]
    # launches that are TRIED (lad_f16_block_fwd*, lad_f16_conv_s2_strips_fwd and lad_f16_tail_fwd may still answer LAD_NOT_COVERED,
    # and the launch code falls back where it always did); all False in fp32
    window_fused: Tuple[bool, ...]    # per block of the model: lad_f16_block_fwd on the B windows
    rides: Tuple[bool, ...]           # per block: a down-sampling block's 1x1 shortcut in conv1's launch (any image count)
    stream_fused: Tuple[bool, ...]    # blocks[:n1] on the stream image
    strip_fused: Tuple[bool, ...]     # blocks[:n1] on the n_strip strips
    stem_kept: bool                   # the stream's stem output is kept for the strips' first block
    strip_stem_rows: bool             # ... which runs as lad_f16_block_fwd_stem_rows (no stem launch for the strips)
    stream2_fused: Tuple[bool, ...]   # blocks[n1 + 1:k3] on the two phase streams
    strip2_fused: Tuple[bool, ...]    # blocks[n1 + 1:k3] on the n_strip2 level-2 strips
    strips2_resident: bool            # the level-2 strips' entry on lad_f16_conv_s2_strips_fwd
    tail_fused: bool                  # everything behind level 2 on lad_f16_tail_fwd

    @property
    def stream_rows(self):
        """Rows of the level-1 stream image the windows read: the run's, or the group's own."""
        return self.Hs if self.run is None else self.run[0] + self.H - 1


def stream_layout(blocks, B, H, W, half, opts, run=None):
    """The layout of one group of B windows of H frames at a stride of one frame: a pure function of the layer geometry
    (block_geometry), the group and the switch values (opts: {name of INFER_OPTIONS: value}); run: (windows, largest group) of the
    run of groups whose streams are computed once, or None.  _forward_eval_stream stores the result in the window plan and its
    launches read nothing else."""
    o = dict(opts)
    n = len(blocks)
    window_fused = tuple(bool(half) and _block_fits_lds(b, B, o) for b in blocks)
    rides = tuple(bool(half) and b.sc_conv is not None and b.conv1.stride == 2 and b.sc_conv.stride == 2 and b.conv1.taps == 9
                  and b.sc_conv.taps == 1 and _s2_shortcut_rides(b, o) for b in blocks)
    n1 = 0
    while n1 < n and blocks[n1].conv1.stride == 1 and blocks[n1].sc_conv is None and blocks[n1].conv1.h_out == H:
        n1 += 1
    band = 1 + 2 * n1                       # 3x3 convolutions at full resolution: the stem + two per block
    if n1 == 0 or H < 4 * band or B < 2:    # nothing to share
        return _StreamLayout(B, H, W, bool(half), "per_window", None, n1, band, *(None,) * 20, window_fused, rides, (), (), False, False,
                             (), (), False, False)
    Hs, Ht = B + H - 1, 2 * band
    n_strip = B + H - Ht                    # one strip per frame offset: the top rows of one window, the bottom rows of another
    nb = blocks[n1] if n1 < n else None
    # `direct`: the strips and the stream go into ONE buffer and the stride-2 block that follows reads every window's rows
    # from where they lie (lad_f16_conv_s2_fwd_windows) -- no assembled copy (1.2 GB written and read per 2048 windows)
    direct = bool(half and nb is not None and nb.sc_conv is not None and nb.conv1.stride == 2
                  and (nb.conv1.cin, nb.conv1.cout) == (64, 32) and o["stream_direct"])
    img_t_rows = (Ht + 1) * (W + 1)
    # level 2 shared as well: the stride-2 block and the stride-1 blocks behind it, up to the next stride-2 block
    k3 = n1 + 1
    while direct and k3 < n and blocks[k3].conv1.stride == 1 and blocks[k3].sc_conv is None:
        k3 += 1
    n2 = k3 - n1 - 1
    margin2 = 1 + 2 * n2                    # stride-1 3x3 convolutions at level 2
    band2 = band // 2 + 1 + margin2         # rows of a window that differ from the stream at the end of level 2 (either end)
    Ht2 = 2 * band2                         # level-2 strips, paired like level 1's: top of window s over bottom of window s - shift2
    shift2 = 2 * (H // 2 - Ht2)
    share2 = bool(direct and o["stream_level2"] and H % 2 == 0 and k3 < n and blocks[k3].sc_conv is not None
                  and blocks[k3].conv1.stride == 2 and (blocks[k3].conv1.cin, blocks[k3].conv1.cout) == (32, 16)
                  and H // 2 >= 2 * Ht2)
    if not (share2 and o["stream_super"]):
        run = None                          # (a run's streams are a feature of the fully shared path)
    mode = "shared2" if share2 else "direct" if direct else "assembled"
    stream_rows = Hs if run is None else run[0] + H - 1
    n_strip_max = n_strip if run is None else run[1] + H - Ht
    stream_row0 = cat_rows = None
    if direct:
        # ONE buffer: [strips of the group (a run: room for its largest)][the stream]; + two zero rows where the odd-phase level-2
        # stream reads the level-1 stream from its second row on
        stream_row0 = n_strip_max * img_t_rows
        cat_rows = stream_row0 + (stream_rows + 1) * (W + 1) + W + 2 + (2 * (W + 1) if share2 else 0)
    strip_fused = tuple(bool(half) and _block_fits_lds(b, n_strip, o, (Ht, W)) for b in blocks[:n1])
    stream_fused = tuple(bool(half) and _block_fits_lds(b, 1, o, (stream_rows, W)) for b in blocks[:n1])
    stem_kept = bool(half and o["strip_stem_shared"])
    # rows 1 .. Ht - 2 of strip s ARE rows s + 1 .. of the stream's stem output: the first block's launch takes them from there
    strip_stem_rows = stem_kept and Ht >= 3 and strip_fused[0] and blocks[0].conv1.cin == 64
    level1 = (n1, band, Ht, Hs, n_strip, n_strip_max, img_t_rows, stream_row0, cat_rows)
    if not share2:
        return _StreamLayout(B, H, W, bool(half), mode, None, *level1, *(None,) * 13, window_fused, rides, stream_fused, strip_fused,
                             stem_kept, strip_stem_rows, (), (), False, False)
    H2, W2 = nb.conv1.h_out, nb.conv1.w_out
    h2s = (stream_rows + 1) // 2            # rows of a level-2 stream image
    n_strip2 = B + shift2
    n_strip2_max = n_strip2 if run is None else run[1] + shift2
    img_t2, img_s2 = (Ht2 + 1) * (W2 + 1), (h2s + 1) * (W2 + 1)
    stream2_base = n_strip2_max * img_t2
    rows2 = stream2_base + 2 * img_s2 + W2 + 2
    return _StreamLayout(B, H, W, True, mode, run, *level1, k3, H2, W2, band2, Ht2, shift2, h2s, n_strip2, n_strip2_max, img_t2, img_s2,
                         stream2_base, rows2, window_fused, rides, stream_fused, strip_fused, stem_kept, strip_stem_rows,
                         tuple(_block_fits_lds(b, 2, o, (h2s, W2)) for b in blocks[n1 + 1:k3]),
                         tuple(_block_fits_lds(b, n_strip2, o, (Ht2, W2)) for b in blocks[n1 + 1:k3]),
                         rides[n1] and bool(o["strip2_resident"]) and (nb.conv1.cin, nb.conv1.cout) == (64, 32),
                         bool(o["tail_fused"]) and _tail_blocks_ok(blocks[k3:]))


class _StreamRun:
    """A run of groups of predict_windows (fp16) whose level-1 / level-2 streams are computed ONCE.  cat, cat2 and stem (the run's
    buffers, _sup_buffer) are filled when the run's first group computes the streams."""
    __slots__ = ("i0", "S", "B_max", "base", "frames_avail", "cat", "cat2", "stem")

    def __init__(self, i0, S, B_max, base, frames_avail):
        self.i0, self.S, self.B_max = i0, S, B_max      # first window, windows, largest group
        self.base, self.frames_avail = base, frames_avail   # address of the run's first frame, frames from there on
        self.cat = self.cat2 = self.stem = None


class ResNetEngine:
    # flags that select kernels / fusions per layer: a train-mode forward freezes them into its schedule (train_schedule), which its
    # backward follows whatever happens to the attributes in between
    KERNEL_OPTIONS =("bf16x3", "bf16x3_32", "f16x2", "f16x2_32", "relu_bits", "virtual_a1", "fuse_bn_bwd", "fuse_bn_bwd_b3", "fuse_bn_bwd_wgrad", "fuse_s2_shortcut",
                      "fuse_s2_shortcut_wgrad", "s2_b3")
    # switches of the sliding-window inference path: stream_layout freezes them into the layout of a group of windows
    INFER_OPTIONS = ("stream_direct", "stream_level2", "stream_super", "strip_block_fused", "small_block_fused", "tail_fused", "strip2_resident",
                     "strip_stem_shared", "f16_s2_shortcut_fused")

    def __init__(self, model):
        self.model = model
        self.device = None
        self._flat_p = self._flat_g = None
        self._plans = {}
        self._step_count = 0
        self._grad_dirty = False  # flat grad buffer holds a gradient that must be accumulated into
        self._train_forwards = 0
        self._weights_version = 0
        # data-gradient epilogues can carry the first pass of the BatchNorm backward that follows (lad_conv_fwd_bnstat).
        # Measured at bs 512: -1.0 ms of reduce passes, +0.3 ms in the four fused conv launches, +0.3 ms in the finalize
        # kernels (18 k tile partials instead of 1 k): net -0.24 ms/step (0.9 %), while the dominant kernel's own launch
        # time grows 2.7 %.  Off by default for that reason; the path is covered by tests/test_resnet_gpu.py.
        self.fuse_bn_bwd = False
        self.overlap_wgrad = False  # weight gradients on a side stream (see _on_side); bench.py --overlap-wgrad
        # ... those of the 16- / 32-channel layers only: True, False, or "auto" = from 256 segments per step on (round 6, after the launch
        # merges: -0.65 % of the step at batch 512 in three A/B pairs on one box, 11.09 -> 11.01 ms; +3.5 % at batch 32, where every
        # kernel is launch-bound and the two event waits cost more than the overlap returns)
        self.overlap_wgrad_small = "auto"
        # the stem's batch statistics and its BatchNorm + weight-gradient backward from 54 moments of the input (one input channel): no
        # 64-channel statistics pass in forward, one pass over dy instead of two in backward (csrc/stem.hip; round 6)
        self.stem_onepass = True
        # The 64 -> 64 3x3 stride-1 convolutions (block1: 8 launches per step, forward + data gradient) run on the bf16 matrix
        # cores with three-way split operands (csrc/conv_b3.hip): fp32-equivalent results (2.9e-7 vs 4.4e-7 of the largest
        # output for the f32 MFMA, both against float64; tests/test_resnet_gpu.py) at 0.95 instead of 1.31 ms per launch.
        # False: every convolution on the exact-f32 MFMA.
        self.bf16x3 = True
        # ... and their data-gradient launches carry the first pass of the BatchNorm backward that consumes them (bn1 of the
        # block: mask recomputed from its input; bn2 of the block below: mask from its sign bits): three of the four
        # two-tensor reduce passes per step disappear for one tensor read in the epilogue.
        self.fuse_bn_bwd_b3 = True
        self.fuse_bn_bwd_wgrad = True   # the BatchNorm backward's element-wise pass inside the 64-channel weight-gradient launches
        # Round 4: the same layers on TWO f16 planes per operand instead of three bf16 planes (csrc/conv_h2.hip, wgrad_h2 in
        # csrc/wgrad_mfma.hip): three plane products per fp32-equivalent product instead of six, block floating point per staged
        # tile.  Error against float64 within 1.5x of the exact-f32 kernel's (tests/test_h2_gpu.py; the fp32 accumulation
        # dominates both), 0.78 -> 0.5 ms per convolution launch.  False: the bf16 x 3 kernels of rounds 2-3 (bf16x3 must be on).
        self.f16x2 = True
        self.f16x2_32 = True    # ... and block2's 32 -> 32 convolutions, forward and data gradient (their weight gradient stays bf16 x 3)
        self.bf16x3_32 = True   # block2's 32 -> 32 convolutions (forward, data gradient) on the same kernel: 0.116 -> 0.081 ms each
        # ... and the activation between the two convolutions of such a block stays virtual: BatchNorm + ReLU are applied
        # while conv2 and its weight gradient stage conv1's raw output (lad_conv_b3_fwd_f32_bnrelu, lad_conv_wgrad_b3_bnrelu).
        self.virtual_a1 = True
        # the 64 -> 32 stride-2 transition (forward + data gradient, with its shortcut) on the split-operand path: the space-to-depth
        # view of the input is formed while staging (csrc/conv_b3.hip, conv_s2b3 / dgrad_s2b3; round 3)
        self.s2_b3 = True
        # sliding-window inference, fp16: the stride-2 block behind level 1 reads the stream / strips directly (no assembled copy)
        self.stream_direct = True
        # ... and the SECOND resolution level is shared between the windows as well (two phase streams + strips)
        self.stream_level2 = True
        # ... and a 64-channel identity block on the boundary strips runs as ONE launch with the strip resident in LDS (round 5)
        self.strip_block_fused = True
        self.small_block_fused = True        # ... and the 16- / 32-channel identity blocks of small images likewise (several per workgroup)
        # fp16 sliding windows: the frame STREAMS of levels 1 and 2 are computed once for up to STREAM_SUPER_MAX windows, not once
        # per group of PREDICT_CHUNK windows (a group's stream launches are 1,500-tile launches: 11 % of its time); round 5
        self.stream_super = True
        # fp16 sliding windows: everything behind the shared level 2 (block3, block4, pooling, classifier) in one launch per group of
        # windows, a window resident in a CU's LDS throughout (lad_f16_tail_fwd; round 6) -- instead of nine launches of small kernels
        self.tail_fused = True
        # ... and block2.0's stride-2 entry on the level-2 strips reads its input from LDS (parity classes by LDS-DMA) instead of gathering it
        self.strip2_resident = True
        # ... and the strips have no stem launch: their inner rows ARE the stream's, the two edge rows are computed in the first block's launch
        self.strip_stem_shared = True
        self._sup_cache = {}
        self._sup_plans = {}                 # {"l1" / "l2": keys of the run-long eval plans, released with the run's buffer}
        self._layouts = {}                   # {(B, H, W, half, switch values, run): _StreamLayout}
        # fp16 eval: a down-sampling block's 1x1 shortcut rides in its 3x3 convolution's launch (lad_f16_conv_s2_fwd*_sc; round 5)
        self.f16_s2_shortcut_fused = True
        self.fuse_s2_shortcut = True         # ... and its forward / data gradient inside conv1's launches (lad_conv_s2_*_fused)
        self.fuse_s2_shortcut_wgrad = True   # a stride-2 block's 1x1 shortcut weight gradient as a tenth tap of conv1's
        self.defer_wgrad_sums = True   # the 19 per-layer sums of weight-gradient slabs in one launch (csrc/slab_reduce.hip)
        self._defer_on = False
        self._schedules = {}   # {(B, H, W, flag values): _TrainSchedule}
        self.relu_bits = True  # False: the residual ReLU mask is re-read from y and the shortcut gradient goes through HBM
        self._side = None
        self._side_readers = {}
        self._side_pending = False
        self.debug_capture = None  # tools/: dict that receives clones of the backward intermediates per block
        self.kernel_events = None  # bench.py: {kernel label: [(start_event, end_event), ...]} when profiling is on
        # Stage widths other than resnet_base's (resnet_with_augmentation: [128, 64, 32, 32] on 128 x 44 windows) run on the exact-f32
        # MFMA kernels only: every split-operand path, sign-bit path and fusion above was validated on the resnet_base layer graph
        # alone and is switched off (the layer flags b3 / s2b3 in _build_specs follow), and so is fp16 inference (no half-precision
        # kernels at 128 channels: predict_windows raises).
        self.base_widths = list(model.filter_sizes) == list(BASE_WIDTHS)
        if not self.base_widths:
            for k in self.KERNEL_OPTIONS:
                setattr(self, k, False)

    # ------------------------------------------------------------------------------------ flat storage
    def lib(self):
        return _hip.lib()

    # The engine has no library handle of its own: every launch goes through _hip.launch, which calls _hip.lib().  `_lib` stays as
    # the name under which tests and tools put a counting or wrapping proxy in the library's place, and take it out again.
    _lib = property(lambda self: _hip._lib, lambda self, value: setattr(_hip, "_lib", value))

    def _named_params(self):
        return list(self.model.named_parameters())

    def ensure_flat(self):
        """Move parameters into one flat buffer (and gradients into another) if they are not there already.
        Called at the top of every entry point: `model.to(device)` / `set_device` re-allocate parameter storage."""
        params = self._named_params()
        dev = params[0][1].device
        if dev.type != "cuda":
            raise _hip.LadHipError("ResNetBigger runs on the MI355X only: call model.set_device('cuda') first "
                                   "(the HIP path has no CPU fallback)")
        ok = self._flat_p is not None and self._flat_p.device == dev
        if ok:
            base = self._flat_p.data_ptr()
            for (name, p), off in zip(params, self._offsets):
                if p.data_ptr() != base + 4 * off or p.dtype != torch.float32:
                    ok = False
                    break
        if ok:
            return
        offs, total = [], 0
        for _, p in params:
            offs.append(total)
            total += _align4(p.numel())
        flat_p = torch.zeros(total, device=dev, dtype=torch.float32)
        flat_g = torch.zeros(total, device=dev, dtype=torch.float32)
        with torch.no_grad():
            for (name, p), off in zip(params, offs):
                view = flat_p[off:off + p.numel()].view(p.shape)
                view.copy_(p.data.to(torch.float32))
                old_grad = p.grad
                p.data = view
                gview = flat_g[off:off + p.numel()].view(p.shape)
                if old_grad is not None:
                    gview.copy_(old_grad)
                    p.grad = gview
        self._flat_p, self._flat_g, self._offsets, self._n_flat = flat_p, flat_g, offs, total
        self._acc_g = None   # gradient-accumulation buffer of the fused loop (accumulated_grad)
        self._exp_avg = torch.zeros_like(flat_p)
        self._exp_avg_sq = torch.zeros_like(flat_p)
        self._norm_partials = torch.zeros(int(self.lib().lad_grad_sumsq_partials()), device=dev)
        self._norm_out = torch.zeros(1, device=dev)
        self._step_dev = torch.zeros(1, device=dev, dtype=torch.int64)
        self._rng_counter = torch.zeros(1, device=dev, dtype=torch.int64)   # dropout-mask draws so far (lad_head_fwd_train_rng)
        self._rng_seed = None
        self.device = dev
        self._plans = {}
        self._views = {name: (flat_p[off:off + p.numel()].view(p.shape), flat_g[off:off + p.numel()].view(p.shape))
                       for (name, p), off in zip(params, offs)}
        # the 22 `num_batches_tracked` counters become views of one int64 buffer: one increment launch per step
        bns = [m for m in self.model.modules() if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d))]
        self._nbt = torch.zeros(len(bns), device=dev, dtype=torch.int64)
        with torch.no_grad():
            for i, m in enumerate(bns):
                self._nbt[i] = m.num_batches_tracked.to(dev)
                m._buffers["num_batches_tracked"] = self._nbt[i]
        self._build_specs()
        self._weights_version += 1
        self._param_list = [p for _, p in params]

    def bump_num_batches_tracked(self):
        self.ensure_flat()
        self._nbt.add_(1)

    def grad_views(self):
        return {k: v[1] for k, v in self._views.items()}

    def attach_grads(self):
        """Make every parameter's .grad the matching view of the flat gradient buffer."""
        for name, p in self._named_params():
            g = self._views[name][1]
            if p.grad is None or p.grad.data_ptr() != g.data_ptr():
                p.grad = g

    # ------------------------------------------------------------------------------------ layer table
    def _build_specs(self):
        """The model's own records: one _ConvParams per convolution of the residual blocks and one _BnParams per BatchNorm, with
        every buffer derived from the weights (packed images, eval folds).  Built with the flat buffers and living as long as they
        do; the layer tables of the geometries (_blocks_for) only point here."""
        m = self.model
        bufs = dict(m.named_buffers())
        lib, dev = self.lib(), self.device

        def bn(name, c, conv_bias=None):
            return _BnParams(name, c, self._views, bufs, dev, conv_bias)

        self.stem_w, self.stem_gw = self._views["conv1.weight"]
        self.stem_cout = self.stem_w.shape[0]
        self.stem_bn = bn("bn1", self.stem_cout)
        self._convs, self._bns = {}, {}   # {layer name: record}, in the order of the model's layers
        for b in block_geometry(self.stem_cout, m.filter_sizes, 1, 1, self.base_widths):   # (names and channel counts only)
            for cs, bn_name in ((b.conv1, ".bn1"), (b.conv2, ".bn2"), (b.sc_conv, ".shortcut.1")):
                if cs is not None:
                    par = self._convs[cs.name] = _ConvParams(cs.name, cs.cin, cs.cout, cs.taps, cs.stride, self.base_widths, self._views, lib, dev)
                    self._bns[b.name + bn_name] = bn(b.name + bn_name, cs.cout, par.b)
            if b.sc_conv is not None:
                self._convs[b.conv1.name].shortcut = self._convs[b.sc_conv.name]
        self._geom_specs = {}
        # freshness of everything derived from the weights (_pack_weights, _eval_prepare)
        self._packed = None       # (weights stamp, data-gradient images too, split images) of the last pack of the MFMA images
        self._folded = None       # state tag of the BatchNorm folds
        self._f16_packed = None   # ... of the half-precision images
        self._pack_tables = {}    # device tables of the multi-layer pack launches: {data-gradient images too | ("h2", layer names)}
        self._tail_ptrs = None
        self.head_bn2 = bn("bn2", m.linear_layer_size)
        self.head_bn3 = bn("bn3", 32)
        names = ["bn2.weight", "bn2.bias", None, None, "linear1.weight", "linear1.bias", "bn3.weight", "bn3.bias",
                 None, None, "linear2.weight", "linear2.bias"]
        ptrs = []
        for i, n in enumerate(names):
            if n is not None:
                ptrs.append(self._views[n][0].data_ptr())
            else:
                t = {2: self.head_bn2.rm, 3: self.head_bn2.rv, 8: self.head_bn3.rm, 9: self.head_bn3.rv}[i]
                ptrs.append(t.data_ptr())
        self._head_params = (_VP * 12)(*ptrs)
        gnames = ["bn2.weight", "bn2.bias", "linear1.weight", "linear1.bias", "bn3.weight", "bn3.bias",
                  "linear2.weight", "linear2.bias"]
        self._head_grads = (_VP * 8)(*[self._views[n][1].data_ptr() for n in gnames])

    def _blocks_for(self, H, W, partial=False):
        """Layer specs for an (H, W) input: sizes and kernel eligibility are the geometry's, the parameters, packed weights and
        folds are the model's records (_build_specs), shared by every geometry.
        partial: only the leading full-resolution layers will run on this geometry (the stream / strip images of the
        sliding-window path): the pooling and classifier-size checks of a whole forward do not apply."""
        key = (H, W, partial)
        if key in self._geom_specs:
            return self._geom_specs[key]
        blocks = block_geometry(self.stem_cout, self.model.filter_sizes, H, W, self.base_widths)
        for b in blocks:
            b.bn1, b.bn2 = self._bns[b.name + ".bn1"], self._bns[b.name + ".bn2"]
            b.conv1.par, b.conv2.par = self._convs[b.conv1.name], self._convs[b.conv2.name]
            if b.sc_conv is not None:
                b.sc_conv.par, b.sc_bn = self._convs[b.sc_conv.name], self._bns[b.name + ".shortcut.1"]
        h, w = blocks[-1].conv2.h_out, blocks[-1].conv2.w_out
        if partial:
            self._geom_specs[key] = (blocks, h, w, 0)
            return self._geom_specs[key]
        if h < 4 or w < 4:
            raise ValueError(f"input ({H},{W}) is too small: AvgPool2d(4) sees a {h}x{w} map")
        feat = blocks[-1].conv2.cout * (h // 4) * (w // 4)
        if feat != self.model.linear_layer_size:
            # same failure the reference hits (BatchNorm1d size check) for e.g. resnet_with_augmentation on (100,44)
            raise RuntimeError(f"running_mean should contain {feat} elements not {self.model.linear_layer_size}")
        self._geom_specs[key] = (blocks, h, w, feat)
        return self._geom_specs[key]

    # ------------------------------------------------------------------------------------ plans
    def _plan(self, B, H, W, train):
        key = (B, H, W, train)
        p = self._plans.get(key)
        if p is not None:
            return p
        dev = self.device
        blocks, h4, w4, feat = self._blocks_for(H, W)
        lib = self.lib()

        def act(h, w, c):
            return torch.zeros(int(lib.lad_act_rows(B, h, w)) * c, device=dev, dtype=torch.float32)

        p = {"blocks": blocks, "h4": h4, "w4": w4, "feat": feat}
        c0 = self.stem_cout
        p["stem_a"] = act(H, W, c0)
        p["stem_coef"] = torch.zeros(6 * c0, device=dev)
        if train:   # the stem's statistics and backward from moments of the input (stem_onepass)
            p["stem_mom"] = torch.zeros(int(lib.lad_stem_moments_doubles()), device=dev, dtype=torch.float64)
            p["stem_mom_ws"] = torch.zeros(int(lib.lad_stem_moments_workspace_doubles()), device=dev, dtype=torch.float64)
            p["stem_bwd_ws"] = torch.zeros(int(lib.lad_stem_bwd_onepass_workspace_floats()), device=dev)
        max_tiles = int(lib.lad_conv_num_tiles(B, H, W))
        for b in blocks:   # the stride-2 data gradient on the split-operand path writes its BatchNorm sums per parity class
            if b.conv1.s2b3:
                max_tiles = max(max_tiles, int(lib.lad_conv_s2b3_dgrad_partials(B, b.conv1.h_in, b.conv1.w_in)))
        cmax = max([64] + [b.conv1.cout for b in blocks])   # (128 at the resnet_with_augmentation widths)
        p["partials"] = torch.zeros(max_tiles * 2 * cmax, device=dev)
        p["partials_sc"] = torch.zeros(max(int(lib.lad_conv_num_tiles(B, b.conv1.h_out, b.conv1.w_out)) * 2 * b.conv1.cout
                                           for b in blocks if b.sc_conv is not None) if any(b.sc_conv is not None for b in blocks) else 0,
                                       device=dev)
        acts = []
        for b in blocks:
            ho, wo, co = b.conv1.h_out, b.conv1.w_out, b.conv1.cout
            d = {"c1": act(ho, wo, co), "a1": act(ho, wo, co), "c2": act(ho, wo, co), "y": act(ho, wo, co),
                 "coef1": torch.zeros(6 * co, device=dev), "coef2": torch.zeros(6 * co, device=dev)}
            if b.sc_conv is not None:
                d["cs"] = act(ho, wo, co)
                d["coefs"] = torch.zeros(6 * co, device=dev)
            elif train and b.conv1.b3_full:
                # sign bits of y, one uint64 per row: what the backward pass needs of the residual ReLU (lad_bn_act_bits)
                d["ybits"] = torch.zeros(int(lib.lad_act_rows(B, ho, wo)), device=dev, dtype=torch.int64)
            acts.append(d)
        p["acts"] = acts
        p["pooled"] = torch.zeros(B * feat, device=dev)
        p["probs"] = torch.zeros(B, device=dev)
        if train:
            p["h"] = torch.zeros(B * 32, device=dev)
            p["hstats"] = torch.zeros(2 * feat + 64, device=dev)
            p["metrics"] = torch.zeros(8, device=dev)
            p["head_ws"] = torch.zeros(int(lib.lad_head_workspace_floats(B, feat)), device=dev)
            p["dpooled"] = torch.zeros(B * feat, device=dev)
            # gradient scratch: per resolution level, 5 buffers sized for the widest tensor at that level
            levels = {}
            # buffers a (possibly side-stream) weight-gradient launch reads are never recycled inside one backward
            for b, d in zip(blocks, acts):
                ho, wo, co = b.conv1.h_out, b.conv1.w_out, b.conv1.cout
                d["dc1"], d["dc2"] = act(ho, wo, co), act(ho, wo, co)
                if b.conv1.stride != 1:
                    d["aux"] = act(ho, wo, co)  # gradient into the shortcut BatchNorm's input: read by its weight gradient
            sizes = {(H, W): c0}
            for b in blocks:
                sizes[(b.conv1.h_out, b.conv1.w_out)] = max(sizes.get((b.conv1.h_out, b.conv1.w_out), 0), b.conv1.cout)
                sizes[(b.conv1.h_in, b.conv1.w_in)] = max(sizes.get((b.conv1.h_in, b.conv1.w_in), 0), b.conv1.cin,
                                                            b.conv1.cout)
            for (h, w), c in sizes.items():
                levels[(h, w)] = [act(h, w, c) for _ in range(4)]
            p["g"] = levels
            ws = max(max(int(lib.lad_conv_wgrad_workspace_floats(cs.cin, cs.cout, cs.taps)),
                         int(lib.lad_conv_s2_wgrad_fused_workspace_floats(cs.cin, cs.cout)) if cs.stride != 1 else 0)
                     for b in blocks for cs in (b.conv1, b.conv2, b.sc_conv) if cs is not None)
            ws = max(ws, int(lib.lad_stem_wgrad_workspace_floats()), int(lib.lad_conv_wgrad_b3c_workspace_floats(32)))
            p["wgrad_ws"] = torch.zeros(ws, device=dev)
            # one workspace per convolution as well: with the slab sums deferred to one launch at the end of backward
            # (lad_wgrad_defer_*), every layer's partial slabs must survive until then (0.4 GB in all)
            p["wgrad_ws_of"] = {}
            for b in blocks:
                for cs in (b.conv1, b.conv2, b.sc_conv):
                    if cs is not None:
                        n = int(lib.lad_conv_wgrad_workspace_floats(cs.cin, cs.cout, cs.taps))
                        if cs.b3_wgrad:
                            n = max(n, int(lib.lad_conv_wgrad_b3c_workspace_floats(cs.cin)))
                        if cs.stride != 1:   # (conv1 of a stride-2 block also holds the shortcut's slabs in the fused launch)
                            n = int(lib.lad_conv_s2_wgrad_fused_workspace_floats(cs.cin, cs.cout)) if cs.taps == 9 else \
                                int(lib.lad_conv_s2_wgrad_workspace_floats(cs.cin, cs.cout, cs.taps))
                        p["wgrad_ws_of"][cs.name] = torch.zeros(n, device=dev)
            p["bn_ws"] = torch.zeros(int(lib.lad_bn_bwd_workspace_floats(cmax)), device=dev)
            p["bcoef"] = torch.zeros(8 * cmax, device=dev)
        self._plans[key] = p
        return p

    # ------------------------------------------------------------------------------------ helpers
    def _launch(self, name, *args, tag="", stream=None, may_decline=False):
        """One checked launch on the engine's device: the current stream, or `stream` (the side stream's handle)."""
        return _hip.launch(name, *args, stream=stream, device=self.device, tag=tag, may_decline=may_decline)

    def _marked(self, label):
        """Context manager: HIP events on the launch stream (torch's current stream) around the body when bench.py asked for per-kernel
        timing of `label`; the pair is kept only when the body finished."""
        if self.kernel_events is None or label not in self.kernel_events:
            return _NOT_TIMED
        return self._event_pair(label)

    @contextlib.contextmanager
    def _event_pair(self, label):
        stream = torch.cuda.current_stream(self.device)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record(stream)
        yield
        end.record(stream)
        self.kernel_events[label].append((start, end))

    def _try_launch(self, label, name, *args, tag=""):
        """A try-and-fall-back entry point: False when it answers LAD_NOT_COVERED (nothing was launched, no event pair is kept: the
        caller falls back), True when the kernel was launched."""
        try:
            with self._marked(label):
                if not self._launch(name, *args, tag=tag, may_decline=True):
                    raise _Declined
        except _Declined:
            return False
        return True

    def notify_weights_changed(self):
        """Parameters or running statistics were written behind the engine's back (a graph replay, a write through
        `param.data`, a broadcast): every cached derivative (packed MFMA images, BatchNorm folds, fp16 packs) is stale."""
        self._weights_version += 1

    def _weights_stamp(self):
        # a Parameter's _version moves when torch writes it in place (optimizer.step, load_state_dict, init; after
        # `p.data = view` the Parameter keeps its OWN counter, the flat buffer's does not move);
        # _weights_version moves when our own Adam kernel writes the flat buffer
        return (self._weights_version, sum(p._version for p in self._param_list))

    def _state_tag(self):
        bufs = sum(b._version for b in self.model.buffers())
        return self._weights_stamp() + (bufs, self._train_forwards)

    def _pack_weights(self, need_dgrad, sched=None):
        """Refresh the packed MFMA weight images the pass about to run reads, if the parameters changed since they were packed: the
        exact-f32 images (forward only for eval-mode callers) and the split-operand images of a training step's schedule."""
        ver = self._weights_stamp()
        want = sched.images if sched is not None else frozenset()
        have = self._packed
        fresh = have is not None and have[0] == ver
        if fresh and have[1] >= need_dgrad and want <= have[2]:
            return
        if not (fresh and have[1] >= need_dgrad):
            table = self._pack_tables.get(need_dgrad)
            if table is None:  # device table of {w, wt, cout, cin, taps, mode} records: pointers never move
                recs = [struct.pack("<QQiiii", par.w.data_ptr(), (par.wt_f if mode == 0 else par.wt_d).data_ptr(), par.cout, par.cin, par.taps, mode)
                        for par in self._convs.values() for mode in ((0, 1) if need_dgrad else (0,))]
                table = self._pack_tables[need_dgrad] = (torch.frombuffer(bytearray(b"".join(recs)), dtype=torch.uint8).to(self.device), len(recs))
            self._launch("lad_conv_pack_weights_multi", table[0], table[1])
        h2 = []
        for kind, name in sorted(want - have[2] if fresh else want):   # (a training step: both directions of every image)
            par = self._convs[name]
            if kind == "s2b3":   # both images in one launch
                self._launch("lad_conv_s2b3_pack_weights_pair", par.w, par.shortcut.w, par.wt3_s2f, par.wt3_s2d)
            elif kind == "b3c":
                for mode, wt in ((0, par.wt3_f), (1, par.wt3_d)):
                    self._launch("lad_conv_b3c_pack_weights", par.w, mode, wt, par.cin)
            else:
                h2.append(par)
        if h2:
            # the f16 x 2 images: ONE launch packs every layer and direction of both channel counts (a record names its own; 16 workgroups
            # per image).  The table is cached under the layers it lists: which ones run on f16 x 2 depends on the flags
            hkey = ("h2",) + tuple(par.name for par in h2)
            htab = self._pack_tables.get(hkey)
            if htab is None:
                recs = [struct.pack("<QQii", par.w.data_ptr(), wt.data_ptr(), mode, par.cin) for par in h2
                        for mode, wt in ((0, par.wt2_f), (1, par.wt2_d))]
                htab = self._pack_tables[hkey] = (torch.frombuffer(bytearray(b"".join(recs)), dtype=torch.uint8).to(self.device), len(recs))
            self._launch("lad_conv_h2_pack_weights_multi", htab[0], htab[1], 0)
        self._packed = (ver, need_dgrad or have[1], want | have[2]) if fresh else (ver, need_dgrad, want)

    def _eval_prepare(self, half):
        """What an eval-mode pass reads of the model, refreshed if parameters or running statistics changed since: the exact-f32
        forward images (fp32), the per-channel (scale, shift) of every BatchNorm that follows a convolution, folded from the
        running statistics (eval mode of models.py:110-115,224), and the half-precision images, refreshed with the folds (fp16)."""
        if not half:
            self._pack_weights(need_dgrad=False)
        tag = self._state_tag()
        if self._folded != tag:
            for bn in (self.stem_bn, *self._bns.values()):
                self._launch("lad_bn_fold", bn.g, bn.b, bn.rm, bn.rv, bn.conv_bias, bn.c, *bn.fold, tag=bn.name)
            self._folded = tag
        if half and self._f16_packed != tag:
            for par in self._convs.values():
                self._launch("lad_f16_pack_weights", par.w, par.cout, par.cin, par.taps, par.wt_h, tag=par.name)
            self._f16_packed = tag

    def _schedule(self, B, H, W):
        """The schedule of a training step under the flags as they are now (built once per batch size, geometry and flag values)."""
        key = (B, H, W, self.stem_onepass) + tuple(getattr(self, k) for k in self.KERNEL_OPTIONS)
        sched = self._schedules.get(key)
        if sched is None:
            sched = self._schedules[key] = train_schedule(self._blocks_for(H, W)[0], B, {k: getattr(self, k) for k in self.KERNEL_OPTIONS},
                                                          self.stem_onepass)
        return sched

    def _conv_s1(self, cs, arith, direction, x, out, B, label=None, *, in_coef=None, bias=None, addend=None, abits=None, partials=None, bn=None):
        """One stride-1 convolution launch on `arith`.  direction "fwd", or "dgrad": the data gradient = stride-1 convolution of dout
        with the flipped / transposed image (GEMM K = cout, N = cin).  in_coef: BatchNorm + ReLU of the input, applied while staging;
        addend (+ abits: gated by sign bits) is added to the result; bn = (x, mask, coef) of the BatchNorm whose backward consumes
        `out`: its first pass rides in the epilogue and leaves per-tile sums in `partials` (mask None: ReLU decisions recomputed from
        x; int64: sign bits; float: the BatchNorm's output y).
        lad_conv_h2 has an epilogue compiled for each combination of options launched from here (csrc/conv_h2.hip, the LAD_H2_FORM list of
        launch_h2_rb); any other combination runs the shared epilogue with run-time tests -- same results, slower: a new form wants a line there."""
        bx, bmask, bcoef = bn if bn is not None else (None, None, None)
        fn = conv_s1_entry(arith, cs.cin, in_coef is not None, abits is not None,
                           None if bn is None else "x" if bmask is None else "bits" if bmask.dtype == torch.int64 else "y")
        fwd, h, w = direction == "fwd", cs.h_in, cs.w_in
        wt = getattr(cs.par, {"h2": "wt2_", "b3": "wt3_", "f32": "wt_"}[arith] + ("f" if fwd else "d"))
        cio = (cs.cin, cs.cout) if fwd else (cs.cout, cs.cin)
        if fn == "lad_conv_h2":
            args = (x, in_coef, wt, bias, addend, abits, out, partials, bx, bmask, bcoef, B, h, w, cs.cin)
        elif fn == "lad_conv_b3c_fwd_f32":
            args = (x, wt, bias, addend, out, partials, B, h, w, cs.cin)
        elif fn == "lad_conv_b3c_fwd_f32_bnrelu":
            args = (x, in_coef, wt, bias, out, partials, B, h, w, cs.cin)
        elif fn == "lad_conv_b3c_dgrad_bnstat":   # ReLU decisions recomputed from the BatchNorm's input (csrc/conv_b3.hip, STAT epilogue)
            args = (x, wt, addend, out, partials, bx, bcoef, B, h, w, cs.cin)
        elif fn == "lad_conv_b3_fwd_f32_gated":
            args = (x, wt, bias, addend, abits, out, partials, B, h, w)
        elif fn == "lad_conv_b3_dgrad_bnstat":    # + the sums of a BatchNorm that kept its own sign bits
            args = (x, wt, addend, abits, out, partials, bx, bmask, bcoef, B, h, w)
        elif fn == "lad_conv_fwd":
            args = (x, wt, bias, addend, out, partials, B, h, w, *cio, cs.taps)
        else:
            args = (x, wt, addend, out, partials, bx, bmask, bcoef, B, h, w, *cio, cs.taps)
        with self._marked(label):
            self._launch(fn, *args, tag=f"({direction}) {cs.name}")

    def _conv_fwd(self, cs, ch, x, out, partials, B, in_coef=None):
        """Forward convolution with bias; `partials` receives the per-tile sums of the BatchNorm that follows."""
        if cs.stride == 1:
            self._conv_s1(cs, ch.arith, "fwd", x, out, B, ch.label_fwd, in_coef=in_coef, bias=cs.par.b, partials=partials)
            return
        with self._marked(ch.label_fwd):
            self._launch("lad_conv_s2_fwd", x, cs.par.wt_f, cs.par.b, out, partials, B, cs.h_in, cs.w_in, cs.cin, cs.cout, cs.taps, tag=cs.name)

    def _bn_coef(self, bn, coef, partials, B, h, w):
        n_tiles = int(self.lib().lad_conv_num_tiles(B, h, w))
        self._launch("lad_bn_finalize", partials, n_tiles, bn.c, B * h * w, bn.g, bn.b, bn.rm, bn.rv, 0.1, coef, tag=bn.name)

    def _bn_coef_pair(self, bn_a, coef_a, part_a, bn_b, coef_b, part_b, B, h, w):
        """_bn_coef for a stride-2 block's bn1 and its shortcut BatchNorm (sums of one shape, left by one launch) in one launch."""
        n_tiles = int(self.lib().lad_conv_num_tiles(B, h, w))
        self._launch("lad_bn_finalize_pair", part_a, part_b, n_tiles, bn_a.c, B * h * w, bn_a.g, bn_a.b, bn_a.rm, bn_a.rv, coef_a,
                     bn_b.g, bn_b.b, bn_b.rm, bn_b.rv, coef_b, 0.1, tag=bn_a.name)

    def _bn_act(self, x, coef, res, rcoef, y, B, h, w, c, relu=1):
        self._launch("lad_bn_act", x, coef, res, rcoef, y, B, h, w, c, relu)

    # ------------------------------------------------------------------------------------ forward
    def forward(self, x, train, labels=None, drop_masks=None):
        """x: GPU float32 (B,1,H,W) or (B,H,W) -> probs (B,) (a plan-owned buffer, valid until the next call).

        train=True uses batch statistics, updates the running statistics and keeps what backward() needs.
        With labels (int32, (B,)) the head also produces the mean BCE loss and the metric counters.
        drop_masks: None (no dropout), a pair of mask tensors, or "rng": the head draws the masks of `model.dropout.p` itself (seeded
        by torch's CUDA generator seed) AND advances num_batches_tracked -- callers then skip bump_num_batches_tracked()."""
        self.ensure_flat()
        _hip.require_cuda(x, "x", torch.float32)
        if x.dim() == 4:
            if x.shape[1] != 1:
                raise ValueError("ResNetBigger expects a single input channel: (B,1,T,F)")
            B, _, H, W = x.shape
        elif x.dim() == 3:
            B, H, W = x.shape
        else:
            raise ValueError("x must be (B,1,T,F) or (B,T,F)")
        if B == 0:
            return torch.zeros(0, device=x.device)
        if not train:
            return self._forward_eval(x.view(-1), B, H, W, frame_stride=H, frames_avail=B * H)
        if B < 2:
            # torch: "Expected more than 1 value per channel when training" (BatchNorm1d on (1, F))
            raise ValueError("Expected more than 1 value per channel when training, got input size "
                             f"torch.Size([{B}, {self.model.linear_layer_size}])")
        p = self._plan(B, H, W, True)
        blocks = p["blocks"]
        # the kernel choices of this pass and of its backward, which reads them from the plan (virtual activations that were never
        # written, sign bits that exist or not, packed weight images), whatever happens to the flags in between
        sched = p["schedule"] = self._schedule(B, H, W)
        self._pack_weights(need_dgrad=True, sched=sched)
        part = p["partials"]
        # stem (models.py:224)
        # The stem convolution (K = 9) is cheaper to recompute than to store: a statistics-only pass, then conv + BatchNorm +
        # ReLU in one kernel (the folded-BN stem kernel with the batch coefficients); the 596 MB convolution output is
        # never written, and backward() recomputes it the same way (lad_stem_bn_bwd_sums, lad_stem_wgrad_bn).
        if sched.stem_onepass:
            # ... and its batch statistics need no convolution pass at all: one input channel, so sum x and sum x^2 are combinations of 54
            # moments of the nine taps (csrc/stem.hip, lad_stem_bn_stats: one pass over the 9 MB of features)
            bn = self.stem_bn
            self._launch("lad_stem_bn_stats", x, self.stem_w, bn.g, bn.b, bn.rm, bn.rv, 0.1, p["stem_coef"], p["stem_mom"], p["stem_mom_ws"],
                         B, H, W, self.stem_cout)
        else:
            self._launch("lad_stem_fwd", x, self.stem_w, None, part, B, H, W, self.stem_cout)
            self._bn_coef(self.stem_bn, p["stem_coef"], part, B, H, W)
        c0 = self.stem_cout
        scale, shift = p["stem_coef"][:c0], p["stem_coef"][c0:2 * c0]
        self._launch("lad_stem_fwd_eval", x, self.stem_w, scale, shift, p["stem_a"], B, H, W, c0, H, B * H, tag="(train)")
        cur = p["stem_a"]
        for b, ch, a in zip(blocks, sched.blocks, p["acts"]):
            ho, wo, co = b.conv1.h_out, b.conv1.w_out, b.conv1.cout
            if ch.entry == "plain":
                self._conv_fwd(b.conv1, ch.conv1, cur, a["c1"], part, B)
                self._bn_coef(b.bn1, a["coef1"], part, B, ho, wo)
            else:
                c1, par = b.conv1, b.conv1.par
                with self._marked(ch.conv1.label_fwd):
                    if ch.entry == "s2b3":   # conv1 and the 1x1 shortcut on the split-operand path (csrc/conv_b3.hip, conv_s2b3_kernel)
                        self._launch("lad_conv_s2b3_fwd", cur, par.wt3_s2f, par.b, a["c1"], part, a["cs"], p["partials_sc"], B, c1.h_in, c1.w_in,
                                     tag=c1.name)
                    else:   # ... in one launch of the exact-f32 kernel (csrc/conv_mfma.hip, conv_s2_kernel<SC>)
                        self._launch("lad_conv_s2_fwd_fused", cur, par.wt_f, par.b, b.sc_conv.par.wt_f, a["c1"], part, a["cs"], p["partials_sc"],
                                     B, c1.h_in, c1.w_in, c1.cin, c1.cout, tag=c1.name)
                # bn1 and the shortcut's BatchNorm: one launch
                self._bn_coef_pair(b.bn1, a["coef1"], part, b.sc_bn, a["coefs"], p["partials_sc"], B, ho, wo)
            if ch.a1_virtual:
                # relu(bn1(c1)) is formed while conv2 (and, in backward, its weight gradient) stage c1: never written
                self._conv_fwd(b.conv2, ch.conv2, a["c1"], a["c2"], part, B, in_coef=a["coef1"])
            else:
                self._bn_act(a["c1"], a["coef1"], None, None, a["a1"], B, ho, wo, co)
                self._conv_fwd(b.conv2, ch.conv2, a["a1"], a["c2"], part, B)
            self._bn_coef(b.bn2, a["coef2"], part, B, ho, wo)
            if b.sc_conv is not None:
                if ch.entry == "plain":
                    self._conv_fwd(b.sc_conv, ch.sc, cur, a["cs"], part, B)
                    self._bn_coef(b.sc_bn, a["coefs"], part, B, ho, wo)
                self._bn_act(a["c2"], a["coef2"], a["cs"], a["coefs"], a["y"], B, ho, wo, co)
            elif ch.bits:
                self._launch("lad_bn_act_bits", a["c2"], a["coef2"], cur, None, a["y"], a["ybits"], B, ho, wo, co)
            else:
                self._bn_act(a["c2"], a["coef2"], cur, None, a["y"], B, ho, wo, co)
            a["x"] = cur
            cur = a["y"]
        last = blocks[-1].conv2
        self._launch("lad_pool_fwd", cur, p["pooled"], B, p["h4"], p["w4"], last.cout)
        m1 = m2 = None
        rng = isinstance(drop_masks, str) and drop_masks == "rng"
        if drop_masks is not None and not rng:
            m1, m2 = drop_masks
            _hip.require_cuda(m1, "drop mask 1", torch.float32)
            _hip.require_cuda(m2, "drop mask 2", torch.float32)
            if tuple(m1.shape) != (B, p["feat"]) or tuple(m2.shape) != (B, 32):
                raise ValueError("dropout masks must be (B,linear_layer_size) and (B,32)")
        if labels is not None:
            _hip.require_cuda(labels, "labels", torch.int32)
            if labels.numel() != B:
                raise ValueError("labels must have one entry per sample")
        if rng:
            # the head's launch draws the two dropout masks itself and advances the BatchNorm layers' num_batches_tracked: none of
            # torch's four mask launches + one increment per step (csrc/head.hip, Philox4x32-10; round 6)
            keep = 1.0 - float(self.model.dropout.p)
            if keep < 1.0:
                if "m1" not in p:
                    p["m1"] = torch.zeros((B, p["feat"]), device=self.device)
                    p["m2"] = torch.zeros((B, 32), device=self.device)
                m1, m2 = p["m1"], p["m2"]
            seed = int(torch.cuda.default_generators[self.device.index or 0].initial_seed()) & ((1 << 64) - 1)
            if seed != self._rng_seed:       # (torch.manual_seed since the last draw: the sequence starts again)
                self._rng_seed = seed
                self._rng_counter.zero_()
            self._launch("lad_head_fwd_train_rng", self._head_params, p["pooled"], B, p["feat"], m1, m2, keep, seed, self._rng_counter, self._nbt,
                         int(self._nbt.numel()), labels, 0.1, p["h"], p["hstats"], p["probs"], p["metrics"])
        else:
            self._launch("lad_head_fwd_train", self._head_params, p["pooled"], B, p["feat"], m1, m2, labels, 0.1, p["h"], p["hstats"],
                         p["probs"], p["metrics"])
        p["saved"] = (x, labels, m1, m2, B, H, W)
        self._last_train_plan = p
        self._train_forwards += 1  # running statistics moved: the eval-mode folds are stale
        return p["probs"]

    # ------------------------------------------------------------------------------------ eval (inference) path
    def _plan_eval(self, B, H, W, dtype=torch.float32, partial=False, owner=None):
        """owner: the run buffer ("l1" / "l2", _sup_buffer) this plan lives and dies with."""
        key = (B, H, W, "eval", dtype) + (("partial",) if partial else ())
        if owner is not None and key not in self._sup_plans.setdefault(owner, []):
            self._sup_plans[owner].append(key)
        p = self._plans.get(key)
        if p is not None:
            return p
        dev = self.device
        blocks, h4, w4, feat = self._blocks_for(H, W, partial)
        p = {"blocks": blocks, "h4": h4, "w4": w4, "feat": feat}
        levels = {(H, W): self.stem_cout}
        for b in blocks:
            k = (b.conv1.h_out, b.conv1.w_out)
            levels[k] = max(levels.get(k, 0), b.conv1.cout)
        # four rotating buffers per resolution level: block input, conv1 output, shortcut branch, block output
        rows_of = lambda k: int(self.lib().lad_act_rows(B, k[0], k[1]))  # noqa: E731
        # (allocated when a level is first used: the sliding-window path never touches the per-window buffers of the levels it
        # shares -- 19 GB for 8192 windows at level 1)
        p["lv"] = _LazyLevels(lambda k: [torch.zeros(rows_of(k) * levels[k], device=dev, dtype=dtype) for _ in range(4)])
        p["pooled"] = torch.zeros(B * feat, device=dev)
        p["probs"] = torch.zeros(B, device=dev)
        self._plans[key] = p
        return p

    # eval-mode convolution by precision: (entry point at stride 1, at stride 2, weight image of _ConvParams, label prefix)
    _CONV_EVAL = {False: ("lad_conv_fwd_eval", "lad_conv_s2_fwd_eval", "wt_f", "conv_s"),
                  True: ("lad_f16_conv_fwd", "lad_f16_conv_s2_fwd", "wt_h", "conv_f16_s")}

    def _conv_eval(self, half, cs, bn, x, addend, out, B, relu):
        s1, s2, image, prefix = self._CONV_EVAL[half]
        wt = getattr(cs.par, image)
        with self._marked(f"{prefix}{cs.stride}<{cs.cin},{cs.cout},{cs.taps}>"):
            if cs.stride == 1:
                self._launch(s1, x, wt, *bn.fold, addend, out, B, cs.h_in, cs.w_in, cs.cin, cs.cout, cs.taps, relu, tag=cs.name)
            else:
                if addend is not None and not half:
                    raise _hip.LadHipError("stride-2 eval convolution takes no residual")
                self._launch(s2, x, wt, *bn.fold, out, B, cs.h_in, cs.w_in, cs.cin, cs.cout, cs.taps, relu, tag=cs.name)

    # ---- the eval forward in pieces (shared by the plain and the streaming sliding-window paths) ------------------------------
    def _eval_stem(self, half, fptr, out, out_byte_offset, B, H, W, frame_stride, frames_avail):
        optr = ctypes.c_void_p(out.data_ptr() + out_byte_offset)
        self._launch("lad_f16_stem_fwd" if half else "lad_stem_fwd_eval", fptr, self.stem_w, *self.stem_bn.fold, optr, B, H, W,
                     self.stem_cout, frame_stride, max(0, frames_avail))

    def _eval_blocks(self, half, p, blocks, cur, B, fused, rides, final_out=None):
        """Residual blocks `blocks` of plan p on the activation `cur` (one of the plan's rotating buffers of its level).
        fused / rides: per block, whether lad_f16_block_fwd is tried and whether a down-sampling block's shortcut rides in conv1's
        launch (the layout's flags for these blocks on B images).  final_out: where the LAST block's output goes instead of a
        rotating buffer (a slice of a caller's tensor)."""
        conv = functools.partial(self._conv_eval, half)
        lv = p["lv"]
        for bi, b in enumerate(blocks):
            L = lv[(b.conv1.h_out, b.conv1.w_out)]
            free = [t for t in L if t is not cur]
            a1, y = free[0], free[1]
            if final_out is not None and bi == len(blocks) - 1:
                y = final_out
            if fused[bi]:
                # both convolutions + the residual with the image(s) resident in LDS (csrc/conv_f16.hip: block_f16_strip_kernel at 64
                # channels, block_f16_small_kernel at 16 / 32)
                if self._try_launch(f"block_f16<{b.conv1.cin}>", "lad_f16_block_fwd", cur, *self._f16_args(b.conv1, b.bn1),
                                    *self._f16_args(b.conv2, b.bn2), y, B, b.conv1.h_in, b.conv1.w_in, b.conv1.cin, tag=b.conv1.name):
                    cur = y
                    continue    # (else this geometry is not covered, nothing was launched -> the two convolutions)
            if rides[bi]:
                cs = free[2]
                self._s2_plain_f16(b, cur, (a1, cs), B, b.conv1.h_in, b.conv1.w_in, True)
                conv(b.conv2, b.bn2, a1, cs, y, B, 1)
                cur = y
                continue
            conv(b.conv1, b.bn1, cur, None, a1, B, 1)
            if b.sc_conv is not None:
                cs = free[2]
                conv(b.sc_conv, b.sc_bn, cur, None, cs, B, 0)
                conv(b.conv2, b.bn2, a1, cs, y, B, 1)
            else:
                conv(b.conv2, b.bn2, a1, cur, y, B, 1)
            cur = y
        return cur

    @staticmethod
    def _f16_args(cs, bn):
        """{fp16 weight image, folded scale, folded shift} of one convolution, as the half-precision entry points take them."""
        return cs.par.wt_h, bn.fold[0], bn.fold[1]

    def _s2_entry_f16(self, b, launch_one, launch_sc, rides):
        """conv1 (-> slot 0) and the 1x1 shortcut (-> slot 1) of the down-sampling block b in half precision: ONE launch
        (launch_sc()) when the shortcut rides, else launch_one(convolution, its BatchNorm, slot, relu) for each; with the event
        marks bench.py keys on."""
        if rides:
            with self._marked(f"conv_f16_s2sc<{b.conv1.cin},{b.conv1.cout}>"):
                launch_sc()
            return
        for cs, bn, slot, relu in ((b.conv1, b.bn1, 0, 1), (b.sc_conv, b.sc_bn, 1, 0)):
            with self._marked(f"conv_f16_s2<{cs.cin},{cs.cout},{cs.taps}>"):
                launch_one(cs, bn, slot, relu)

    def _s2_plain_f16(self, b, src, dst, B, h, w, rides):
        """... on B whole images of h x w at src; dst: the two outputs (tensors, or device pointers into one)."""
        def one(cs, bn, slot, relu):
            self._launch("lad_f16_conv_s2_fwd", src, *self._f16_args(cs, bn), dst[slot], B, h, w, cs.cin, cs.cout, cs.taps, relu, tag=cs.name)

        def both():
            self._launch("lad_f16_conv_s2_fwd_sc", src, *self._f16_args(b.conv1, b.bn1), dst[0], *self._f16_args(b.sc_conv, b.sc_bn), dst[1],
                         B, h, w, b.conv1.cin, b.conv1.cout, 1, tag=b.conv1.name)
        self._s2_entry_f16(b, one, both, rides)

    def _s2_mapped_f16(self, b, src, dst, wmap, rides, strips_resident=False):
        """... reading every image through the window map of include/lad_hip.h, wmap = (images, H, W, band, strip rows, strip shift,
        first stream row, phases, rows of a phase image, rows of src, output rows per image or 0 for all), from the tensor src
        ([strips][stream(s)]).  strips_resident: the one-launch form is tried on lad_f16_conv_s2_strips_fwd first (the strips' input
        rows resident in LDS as parity classes instead of gathered per lane: csrc/s2strip_f16.hip, round 6)."""
        def one(cs, bn, slot, relu):
            self._launch("lad_f16_conv_s2_fwd_mapped", src, *self._f16_args(cs, bn), dst[slot], *wmap, cs.cin, cs.cout, cs.taps, relu, tag=cs.name)

        def both():
            args = (src, *self._f16_args(b.conv1, b.bn1), dst[0], *self._f16_args(b.sc_conv, b.sc_bn), dst[1])
            # (no event pair of its own: _s2_entry_f16 times whichever of the two launches runs)
            if strips_resident and self._launch("lad_f16_conv_s2_strips_fwd", *args, *wmap[:7], *wmap[9:], tag=b.conv1.name, may_decline=True):
                return
            self._launch("lad_f16_conv_s2_fwd_mapped_sc", *args, *wmap, b.conv1.cin, b.conv1.cout, 1, tag=b.conv1.name)
        self._s2_entry_f16(b, one, both, rides)

    def _eval_tail(self, half, p, cur, B, probs_out=None):
        """Pooling and classifier.  probs_out (predict_windows): the slice of ITS output these windows belong to -- the head writes
        there (no copy per chunk)."""
        last = p["blocks"][-1].conv2
        p["block_out"] = cur
        self._launch("lad_f16_pool_fwd" if half else "lad_pool_fwd", cur, p["pooled"], B, p["h4"], p["w4"], last.cout)
        probs = probs_out if probs_out is not None else p["probs"]
        self._launch("lad_head_fwd_eval", self._head_params, p["pooled"], B, p["feat"], probs)
        return probs

    def _require_half(self):
        if not self.base_widths:
            raise ValueError(f"precision 'fp16' runs the stage widths {list(BASE_WIDTHS)} (resnet_base) only; this model has "
                             f"{list(self.model.filter_sizes)}: use precision 'fp32'")

    def _layout(self, blocks, B, H, W, half, run=None):
        """The layout of a group of windows under the switches as they are now (built once per group size, geometry, switch values
        and run)."""
        key = (B, H, W, half, run) + tuple(getattr(self, k) for k in self.INFER_OPTIONS)
        lay = self._layouts.get(key)
        if lay is None:
            lay = self._layouts[key] = stream_layout(blocks, B, H, W, half, {k: getattr(self, k) for k in self.INFER_OPTIONS}, run)
        return lay

    def _forward_eval_any(self, half, feat_flat, B, H, W, frame_stride, frames_avail, feat_offset_floats=0, probs_out=None):
        """Eval-mode forward of B images taken from a (frames, W) feature matrix (see lad_stem_fwd_eval): every BatchNorm is
        folded into the epilogue of the convolution in front of it, so the whole model is stem + 19 convolution launches +
        pool + head.  half: activations / weights in fp16 on the 16-bit matrix cores (csrc/conv_f16.hip), f32 in and out."""
        if half:
            self._require_half()
        p = self._plan_eval(B, H, W, torch.float16 if half else torch.float32)
        blocks = p["blocks"]
        lay = self._layout(blocks, B, H, W, half)
        self._eval_prepare(half)
        cur = p["lv"][(H, W)][0]
        fptr = ctypes.c_void_p(feat_flat.data_ptr() + 4 * feat_offset_floats)
        self._eval_stem(half, fptr, cur, 0, B, H, W, frame_stride, frames_avail)
        cur = self._eval_blocks(half, p, blocks, cur, B, lay.window_fused, lay.rides)
        return self._eval_tail(half, p, cur, B, probs_out)

    def _forward_eval(self, feat_flat, B, H, W, frame_stride, frames_avail, feat_offset_floats=0):
        return self._forward_eval_any(False, feat_flat, B, H, W, frame_stride, frames_avail, feat_offset_floats)

    def _forward_eval_stream(self, half, feat_flat, B, H, W, frames_avail, feat_offset_floats=0, run=None, d=0, probs_out=None):
        """The same probabilities for B windows AT A STRIDE OF ONE FRAME, with the full-resolution layers (stem + the stride-1
        blocks of level 1: 75 % of the model's arithmetic) run once over the shared stream and on one boundary strip per
        frame offset instead of on every window (csrc/gather.hip, lad_assemble_windows, for the argument): a ninth of that work.
        In half precision the second level is shared the same way (_stream_level2).  Where everything lies and what is launched is
        the group's _StreamLayout (stream_layout), kept in the window plan as p["layout"].
        run (predict_windows, fp16) with d = this group's first window within it: the streams are computed ONCE for a run of
        groups.  A row of a stream depends on the frames within `band` rows of it only, so every row a window uses is the row the
        group's own stream image would hold, bit for bit."""
        dtype = torch.float16 if half else torch.float32
        pw = self._plan_eval(B, H, W, dtype)
        lay = pw["layout"] = self._layout(pw["blocks"], B, H, W, half, None if run is None else (run.S, run.B_max))
        if lay.mode == "per_window":
            return self._forward_eval_any(half, feat_flat, B, H, W, 1, frames_avail, feat_offset_floats, probs_out)
        if lay.run is None:
            run, d = None, 0
        plans = {"pw": pw, "ps": self._plan_eval(1, lay.Hs, W, dtype, partial=True),
                 "pt": self._plan_eval(lay.n_strip, lay.Ht, W, dtype, partial=True)}
        self._eval_prepare(half)
        bufs = {}
        src = (feat_flat.data_ptr() + 4 * feat_offset_floats, frames_avail)   # the group's first frame, frames from there on
        self._stream_level1(lay, plans, bufs, run, src)
        self._strips_level1(lay, plans, bufs, run, src, d)
        if lay.mode == "shared2":
            self._stream_level2(lay, plans, bufs, run, d)
        return self._stream_tail(lay, plans, bufs, d, probs_out)

    def _stream_level1(self, lay, plans, bufs, run, src):
        """The level-1 stream: frames [0, B + H - 1) of the group -- or [0, S + H - 1) of the run, once -- as one tall image through
        the stem and blocks[:n1].  Leaves bufs["cat"] (None in "assembled"), ["stem"] (the kept stem output, or None) and
        ["stream"] (the stream's level-1 output where it is a tensor of its own: "assembled")."""
        half, W, C, n1 = lay.half, lay.W, self.stem_cout, lay.n1
        dtype = torch.float16 if half else torch.float32
        rows, ride = lay.stream_rows, lay.rides[:n1]
        if run is not None:
            # ONE buffer for the run: [strips of the current group (room for the largest)][the run's stream]
            bufs["cat"] = run.cat
            if run.cat is None:
                key = (run.S, run.B_max, lay.H, W)
                bufs["cat"] = run.cat = self._sup_buffer("l1", lay.cat_rows * C, dtype, key)
                psS = self._plan_eval(1, rows, W, dtype, partial=True, owner="l1")
                if lay.stem_kept:
                    # the run's stem output is KEPT (2 GB for a 60-minute channel): the strips' first block reads its inner rows from it
                    cS = run.stem = self._sup_buffer("l0", int(self.lib().lad_act_rows(1, rows, W)) * C, dtype, key)
                else:
                    cS = psS["lv"][(rows, W)][0]
                self._eval_stem(half, ctypes.c_void_p(run.base), cS, 0, 1, rows, W, 1, run.frames_avail)
                self._eval_blocks(half, psS, psS["blocks"][:n1], cS, 1, lay.stream_fused, ride, final_out=run.cat[lay.stream_row0 * C:])
            bufs["stem"], bufs["stream"] = run.stem, None
            return
        pw, ps = plans["pw"], plans["ps"]
        cat = out_s = None
        if lay.cat_rows is not None:
            cat = pw.get("l1cat")
            if cat is None or cat.numel() != lay.cat_rows * C:
                cat = pw["l1cat"] = torch.zeros(lay.cat_rows * C, device=self.device, dtype=dtype)
            out_s = cat[lay.stream_row0 * C:]
        stem = None
        if lay.stem_kept:
            if ps.get("stem_keep") is None:
                ps["stem_keep"] = torch.zeros(int(self.lib().lad_act_rows(1, rows, W)) * C, device=self.device, dtype=dtype)
            cs = stem = ps["stem_keep"]
        else:
            cs = ps["lv"][(rows, W)][0]
        self._eval_stem(half, ctypes.c_void_p(src[0]), cs, 0, 1, rows, W, 1, src[1])
        bufs["cat"], bufs["stem"] = cat, stem
        bufs["stream"] = self._eval_blocks(half, ps, ps["blocks"][:n1], cs, 1, lay.stream_fused, ride, final_out=out_s)

    def _strips_level1(self, lay, plans, bufs, run, src, d):
        """The level-1 strips: frames [s, s + 2 band) for every offset s (gather.hip: upper half = top of window s, lower half =
        bottom of window s - (H - 2 band)) through the stem and blocks[:n1], into the head of cat.  Leaves bufs["strips"]."""
        half, W, C, n1, n_strip, Ht = lay.half, lay.W, self.stem_cout, lay.n1, lay.n_strip, lay.Ht
        cat, pt = bufs["cat"], plans["pt"]
        out_t = None
        if cat is not None:
            # (the strips' tail rows are the stream's border row: zeros either way -- except behind a run's shorter last group, where
            # an earlier group's strips lie: the W + 2 rows its last strip reads below itself must be zero)
            out_t = cat[:(n_strip * lay.img_t_rows + W + 2) * C]
            if n_strip < lay.n_strip_max:
                cat[n_strip * lay.img_t_rows * C:(n_strip * lay.img_t_rows + W + 2) * C].zero_()
        ct = None
        b0 = pt["blocks"][0]
        fused, ride = lay.strip_fused, lay.rides[:n1]
        if lay.strip_stem_rows:
            # Rows 1 .. Ht - 2 of strip s ARE rows s + 1 .. of the stream's stem output (their input frames lie inside the strip either way):
            # the first block's launch takes them from there and computes the strip's first and last row itself
            # (lad_f16_block_fwd_stem_rows; round 6) -- no stem launch for the strips, no strip-sized stem tensor written or read
            y0 = out_t if n1 == 1 else pt["lv"][(Ht, W)][1]
            if self._try_launch(f"block_f16<{b0.conv1.cin}>", "lad_f16_block_fwd_stem_rows", bufs["stem"], lay.stream_rows, d,
                                ctypes.c_void_p(src[0]), max(0, src[1]), self.stem_w, *self.stem_bn.fold, *self._f16_args(b0.conv1, b0.bn1),
                                *self._f16_args(b0.conv2, b0.bn2), y0, n_strip, Ht, W, tag=b0.conv1.name):
                ct = y0 if n1 == 1 else self._eval_blocks(half, pt, pt["blocks"][1:n1], y0, n_strip, fused[1:], ride[1:], final_out=out_t)
        if ct is None:
            ct = pt["lv"][(Ht, W)][0]
            self._eval_stem(half, ctypes.c_void_p(src[0]), ct, 0, n_strip, Ht, W, 1, src[1])
            ct = self._eval_blocks(half, pt, pt["blocks"][:n1], ct, n_strip, fused, ride, final_out=out_t)
        bufs["strips"] = ct

    def _sup_buffer(self, name, numel, dtype, run_key):
        """Zero-initialised buffer of a run's streams (+ the strips of its current group), kept between runs of the same run_key
        (run length, largest group, window geometry: [strips][stream][spare zero rows] -- two runs of equal size but another split
        would find old stream data where zero rows are expected): every region of it is rewritten or explicitly zeroed where a reader
        expects zeros (the W + 2 rows behind a shorter last group's strips); the border rows, tails and spare rows that nobody writes
        stay as allocated.  A run of another key REPLACES the buffer and the run-long eval plans that fed it (four activation
        buffers per level: 8 + 2 GB for a 60-minute channel), so a long-lived process holds one run's memory whatever it predicts."""
        key = ("sup", name, numel, dtype, run_key)
        buf = self._sup_cache.get(key)
        if buf is None:
            for k in [k for k in self._sup_cache if k[1] == name]:
                del self._sup_cache[k]
            for pk in self._sup_plans.pop(name, []):
                self._release_plan(pk)
            buf = self._sup_cache[key] = torch.zeros(numel, device=self.device, dtype=dtype)
        return buf

    def _release_plan(self, key):
        """Forget an eval plan, and its geometry's layer table when no other plan uses it (nothing of the weights goes with it: images
        and folds are the model's)."""
        p = self._plans.pop(key, None)
        if p is None or any(q.get("blocks") is p["blocks"] for q in self._plans.values()):
            return
        for gk in [gk for gk, gv in self._geom_specs.items() if gv[0] is p["blocks"]]:
            del self._geom_specs[gk]

    def _stream_level2(self, lay, plans, bufs, run, d):
        """fp16 sliding windows, second resolution level.  Row r of window i at level 2 looks at level-1 rows 2r - 1 .. 2r + 1 of the
        window = stream rows i + 2r - 1 ..: windows i = 2j + phase share ONE level-2 stream per phase (row j + r of it), which
        is the stride-2 block run on the level-1 stream from row `phase` on; the rows that see a window's own top / bottom
        (band2 of them, either end) come from strips of Ht2 = 2 band2 rows, paired like level 1's (strip s = the first band2
        rows of window s over the last band2 of window s - shift2: the same 12 positions of the same phase stream, padded
        above for the one and below for the other), whose stride-2 layer reads the level-1 strips and stream through the
        window map.  Leaves bufs["cat2"] = [strips][phase-0 stream][phase-1 stream]; the two streams are computed once per run."""
        dtype, esize = torch.float16, 2
        H, W, n1, k3, Ht2, W2, h2s = lay.H, lay.W, lay.n1, lay.k3, lay.Ht2, lay.W2, lay.h2s
        pw, cat = plans["pw"], bufs["cat"]
        nb = pw["blocks"][n1]
        C1, C2 = nb.conv1.cin, nb.conv1.cout
        ps2 = self._plan_eval(2, 2 * h2s, W, dtype, partial=True)
        pt2 = self._plan_eval(lay.n_strip2, 2 * Ht2, W, dtype, partial=True)
        streams_ready = False
        if run is None:
            cat2 = pw.get("l2cat")
            if cat2 is None or cat2.numel() != lay.rows2 * C2:
                cat2 = pw["l2cat"] = torch.zeros(lay.rows2 * C2, device=self.device, dtype=dtype)
        elif run.cat2 is not None:
            cat2, streams_ready = run.cat2, True
        else:
            cat2 = run.cat2 = self._sup_buffer("l2", lay.rows2 * C2, dtype, (run.S, run.B_max, H, W))
            ps2 = self._plan_eval(2, 2 * h2s, W, dtype, partial=True, owner="l2")   # (a replaced buffer took the old run's plans with it)
        bufs["cat2"] = cat2
        out_t2 = cat2[:(lay.n_strip2 * lay.img_t2 + W2 + 2) * C2]
        if lay.n_strip2 < lay.n_strip2_max:
            cat2[lay.n_strip2 * lay.img_t2 * C2:(lay.n_strip2 * lay.img_t2 + W2 + 2) * C2].zero_()

        def rest_of_level(p, b, L, n_img, fused, final_out):
            y = final_out if k3 == n1 + 1 else L[2]
            self._conv_eval(True, b.conv2, b.bn2, L[0], L[1], y, n_img, 1)
            if k3 > n1 + 1:
                self._eval_blocks(True, p, p["blocks"][n1 + 1:k3], y, n_img, fused, lay.rides[n1 + 1:k3], final_out=final_out)

        if not streams_ready:   # the two phase streams: the stride-2 block on the level-1 stream from row `phase` on
            Ls, bs = ps2["lv"][(h2s, W2)], ps2["blocks"][n1]
            for phase in (0, 1):
                src = ctypes.c_void_p(cat.data_ptr() + (lay.stream_row0 + phase * (W + 1)) * C1 * esize)
                off = phase * lay.img_s2 * C2 * esize
                self._s2_plain_f16(bs, src, (ctypes.c_void_p(Ls[0].data_ptr() + off), ctypes.c_void_p(Ls[1].data_ptr() + off)),
                                   1, lay.stream_rows, W, lay.rides[n1])
            rest_of_level(ps2, bs, Ls, 2, lay.stream2_fused, cat2[lay.stream2_base * C2:])
        # the strips: the first and the last Ht2 rows of every window, read from the level-1 strips and stream where they lie
        Lt, bt = pt2["lv"][(Ht2, W2)], pt2["blocks"][n1]
        wmap = (lay.B, H, W, lay.band, lay.Ht, H - lay.Ht, lay.stream_row0 + d * (W + 1), 1, 0, lay.cat_rows, Ht2)
        self._s2_mapped_f16(bt, cat, Lt, wmap, lay.rides[n1], lay.strips2_resident)
        rest_of_level(pt2, bt, Lt, lay.n_strip2, lay.strip2_fused, out_t2)

    def _stream_tail(self, lay, plans, bufs, d, probs_out):
        """Everything behind the shared levels, per window: the down-sampling block that leaves them reads every window's rows from
        the strips and the stream(s) where they lie ("shared2": from cat2, two phases; "direct": from cat), or from an assembled
        copy of every window's level-1 output ("assembled")."""
        half, B, H, W, n1 = lay.half, lay.B, lay.H, lay.W, lay.n1
        pw = plans["pw"]
        blocks = pw["blocks"]
        fused, ride = lay.window_fused, lay.rides
        if lay.mode == "assembled":
            cur = pw["lv"][(H, W)][0]
            self._launch("lad_assemble_windows", bufs["stream"], bufs["strips"], cur, B, H, W, lay.band, self.stem_cout * (2 if half else 4))
            cur = self._eval_blocks(half, pw, blocks[n1:], cur, B, fused[n1:], ride[n1:])
            return self._eval_tail(half, pw, cur, B, probs_out)
        if lay.mode == "direct":
            k, src = n1, bufs["cat"]
            wmap = (B, H, W, lay.band, lay.Ht, H - lay.Ht, lay.stream_row0, 1, 0, lay.cat_rows, 0)
        else:
            # (d even: the phases keep their parity, the group's window 0 lies d / 2 rows down either phase stream)
            k, src = lay.k3, bufs["cat2"]
            wmap = (B, lay.H2, lay.W2, lay.band2, lay.Ht2, lay.shift2, lay.stream2_base + (d // 2) * (lay.W2 + 1), 2, lay.img_s2, lay.rows2, 0)
            if lay.tail_fused:   # in ONE launch where the tail kernel covers the geometry (csrc/tail_f16.hip, round 6)
                probs = probs_out if probs_out is not None else pw["probs"]
                if self._try_launch("tail_f16", "lad_f16_tail_fwd", src, *wmap[:-1], self._tail_params(blocks[k:]), self._head_params,
                                    pw["feat"], probs):
                    return probs
        b = blocks[k]
        L = pw["lv"][(b.conv1.h_out, b.conv1.w_out)]
        if lay.mode == "direct" and not ride[k]:   # (two launches: the entry point that needs no map)
            def one(cs, bn, slot, relu):
                self._launch("lad_f16_conv_s2_fwd_windows", src, *self._f16_args(cs, bn), L[slot], B, H, W, lay.band, cs.cin, cs.cout, cs.taps,
                             relu, tag=cs.name)
            self._s2_entry_f16(b, one, None, False)
        else:
            self._s2_mapped_f16(b, src, L, wmap, ride[k])
        self._conv_eval(True, b.conv2, b.bn2, L[0], L[1], L[2], B, 1)
        cur = self._eval_blocks(half, pw, blocks[k + 1:], L[2], B, fused[k + 1:], ride[k + 1:])
        return self._eval_tail(half, pw, cur, B, probs_out)

    def _stream_super_cap(self, F):
        """Windows per run of shared streams that the device's free memory allows (half of it): per frame a run keeps five
        64-channel tensors at level 1 (four rotating plan buffers + the stream) and five 32-channel ones per phase at level 2."""
        free, _ = torch.cuda.mem_get_info(self.device)
        free += torch.cuda.memory_reserved(self.device) - torch.cuda.memory_allocated(self.device)   # (torch's cache is reusable)
        held = sum(b.numel() * b.element_size() for b in self._sup_cache.values())                  # (a run of this size replaces it)
        per_frame = 2 * (6 * (F + 1) * self.stem_cout + 5 * ((F + 1) // 2 + 1) * 32)   # (+ the stem's output at level 1, kept for the strips)
        return max(0, int(0.5 * (free + held)) // per_frame)

    def _tail_params(self, tail):
        """HOST array of the 30 device pointers lad_f16_tail_fwd takes: {fp16 weight image, folded scale, folded shift} per convolution
        of the blocks behind level 2 (the model's buffers, refreshed in place: built once)."""
        if self._tail_ptrs is None:
            ptrs = []
            for b in tail:
                for cs, bn in ((b.conv1, b.bn1),) + (((b.sc_conv, b.sc_bn),) if b.sc_conv is not None else ()) + ((b.conv2, b.bn2),):
                    ptrs += [cs.par.wt_h.data_ptr(), bn.fold[0].data_ptr(), bn.fold[1].data_ptr()]
            self._tail_ptrs = (_VP * len(ptrs))(*ptrs)
        return self._tail_ptrs

    def predict_windows(self, feats, n_frames=100, chunk=None, start=0, stop=None, out=None, precision="fp32", stream=True):
        """Probabilities of the stride-one-frame windows of a whole-file feature matrix (the loop of
        segment_laughter.py:90-101 over InferenceDataset, datasets.py:72-93): window i = feats[i:i+n_frames],
        zero-padded on the right at the end of the file.  feats: GPU float32 (T, F).  Windows [start, stop) only
        (rank sharding); returns a GPU float32 vector of stop-start probabilities.  precision "fp16" runs the
        convolutions on the 16-bit matrix cores with half activations (tolerance: tests/test_resnet_gpu.py).
        stream (default): the full-resolution layers are shared between the overlapping windows (_forward_eval_stream);
        False: every window goes through the whole model on its own, as the reference's loop does."""
        if precision not in ("fp32", "fp16"):
            raise ValueError("precision must be 'fp32' or 'fp16'")
        half = precision == "fp16"
        if half:
            self._require_half()
        chunk = PREDICT_CHUNK[precision] if chunk is None else chunk
        self.ensure_flat()
        _hip.require_cuda(feats, "feats", torch.float32)
        if feats.dim() != 2:
            raise ValueError("feats must be (T, F)")
        T, F = feats.shape
        stop = T if stop is None else min(stop, T)
        n = max(0, stop - start)
        if out is None:
            out = torch.empty(n, device=feats.device, dtype=torch.float32)
        elif out.dim() != 1 or out.numel() < n:
            raise ValueError(f"out must be a vector of at least {n} elements (one per window of [start, stop))")
        flat = feats.view(-1)
        i = start
        direct = out.dtype == torch.float32 and out.is_contiguous() and out.device == feats.device
        # fp16: the streams of levels 1 and 2 once per RUN of groups (even group sizes: a group then starts at an even window of its run)
        use_runs = half and stream and self.stream_super and chunk % 2 == 0 and stop - start > chunk
        run = None
        while i < stop:
            B = min(chunk, stop - i)
            dst = out[i - start:i - start + B]
            if use_runs and (run is None or i >= run.i0 + run.S):
                S = min(stop - i, max(chunk, min(STREAM_SUPER_MAX, self._stream_super_cap(F)) // chunk * chunk))
                run = _StreamRun(i, S, min(chunk, S), flat.data_ptr() + 4 * i * F, T - i)
            if stream:
                probs = self._forward_eval_stream(half, flat, B, n_frames, F, frames_avail=T - i, feat_offset_floats=i * F, run=run,
                                                  d=0 if run is None else i - run.i0, probs_out=dst if direct else None)
            else:
                probs = self._forward_eval_any(half, flat, B, n_frames, F, 1, frames_avail=T - i, feat_offset_floats=i * F,
                                               probs_out=dst if direct else None)
            if not direct:
                dst.copy_(probs[:B])
            i += B
        return out

    # ------------------------------------------------------------------------------------ backward
    def _bn_bwd(self, p, bn, dy, y, x, coef, dx, B, h, w, relu, mode=0, aux=None, sbn=None, xs=None, scoef=None, pre=False):
        """pre=True: the launch that produced dy already left this BatchNorm's per-tile sums in p["partials"]."""
        sg, sgg, sgb = (sbn.g, sbn.gg, sbn.gb) if sbn is not None else (None, None, None)
        self._launch("lad_bn_bwd", dy, y, x, coef, bn.g, xs, scoef, sg, dx, aux, bn.gg, bn.gb, sgg, sgb, p["bn_ws"], p["bcoef"],
                     p["partials"] if pre else None, int(self.lib().lad_conv_num_tiles(B, h, w)) if pre else 0, B, h, w, bn.c, relu, mode,
                     tag=bn.name)

    # Weight gradients are off the critical path of backward (nothing needs them before the optimiser), so they CAN run
    # on a side stream next to the data-gradient chain (overlap_wgrad = True): two MFMA kernels sharing the CUs fill each
    # other's bubbles.  Off by default: every kernel then runs alone, and a per-kernel duration (the roofline figure of
    # bench.py, rocprofv3's averages) means what it says; with the overlap the step is faster but each co-scheduled
    # launch takes longer.  Ordering when on:
    #   side waits for main up to the launch point (its operands exist);
    #   main waits for the recorded side event before it OVERWRITES a gradient buffer a pending wgrad reads (_w);
    #   main joins side at the end of backward (the flat gradient is complete before all-reduce / clip / Adam).
    def _side_stream(self):
        if self._side is None or self._side.device != self.device:
            self._side = torch.cuda.Stream(self.device)
        return self._side

    def _on_side(self, launch, read_buffer, small=False):
        """Run launch(stream handle) on the side stream (None: on the current stream, as _launch takes it); remember that it reads
        `read_buffer`.  small: a 16- / 32-channel layer's launch (overlap_wgrad_small: only these go to the side stream)."""
        if not (self.overlap_wgrad or (small and self._overlap_small_on())):
            launch(None)
            return
        side = self._side_stream()
        side.wait_stream(torch.cuda.current_stream(self.device))
        launch(ctypes.c_void_p(side.cuda_stream))
        ev = torch.cuda.Event()
        ev.record(side)
        self._side_readers[read_buffer.data_ptr()] = ev
        self._side_pending = True

    def _overlap_small_on(self):
        if self.overlap_wgrad_small != "auto":
            return bool(self.overlap_wgrad_small)
        p = getattr(self, "_last_train_plan", None)   # "auto": by the batch size of the step that runs (or ran last)
        return p is not None and p["saved"][4] >= 256

    def _w(self, buf):
        """`buf` is about to be overwritten on the main stream: wait for a side-stream reader, if any."""
        ev = self._side_readers.pop(buf.data_ptr(), None)
        if ev is not None:
            torch.cuda.current_stream(self.device).wait_event(ev)
        return buf

    def _join_side(self):
        if self._side_pending:
            torch.cuda.current_stream(self.device).wait_stream(self._side)
            self._side_pending = False
            self._side_readers.clear()

    def _wg_ws(self, p, cs):
        return p["wgrad_ws_of"][cs.name] if self._defer_on else p["wgrad_ws"]

    def _conv_wgrad(self, p, cs, kind, x, dout, B, *, in_coef=None, bn=None):
        """Weight (and bias) gradient of a stride-1 convolution on `kind`, from its input x and the gradient dout of its output.
        in_coef: x is the raw output of the convolution before (a virtual a1): BatchNorm + ReLU are applied while staging.
        bn = (dy, bn_x, bits, coef): the launch first applies the element-wise half of the BatchNorm backward of the layer's own
        output (p["bcoef"], left by lad_bn_bwd*) to dy and WRITES dout for the data-gradient launch: main stream only."""
        fn = conv_wgrad_entry(kind, in_coef is not None, bn is not None)
        h, w, ws, gw, gb = cs.h_in, cs.w_in, self._wg_ws(p, cs), cs.par.gw, cs.par.gb
        if bn is not None:
            dy, bx, bits, coef = bn
            self._launch(fn, x, in_coef, dy, bx, bits, coef, p["bcoef"], dout, ws, gw, gb, B, h, w, cs.cin, tag=cs.name)
        elif kind == "f32":
            self._on_side(lambda st: self._launch(fn, x, dout, ws, gw, gb, B, h, w, cs.cin, cs.cout, cs.taps, tag=cs.name, stream=st),
                          dout, small=cs.cin <= 32)
        else:   # same split arithmetic as the forward / data-gradient launches of this layer (csrc/wgrad_mfma.hip)
            self._on_side(lambda st: self._launch(fn, x, in_coef, dout, ws, gw, gb, B, h, w, cs.cin, tag=cs.name, stream=st),
                          dout, small=cs.cin <= 32)

    def backward(self, dprobs=None):
        """Gradient of the last train-mode forward into the flat gradient buffer (overwrites it).

        dprobs None: the loss is the mean BCE against the labels given to forward() (train.py:279-289);
        otherwise dprobs (B,) is dLoss/dprobs from autograd."""
        try:
            self._backward(dprobs)
        except BaseException:
            if self._defer_on:   # leave the library's deferral switched off and its queue empty
                self._defer_on = False
                self.lib().lad_wgrad_defer_begin()
                self.lib().lad_wgrad_defer_flush(None)
            raise

    def _backward(self, dprobs):
        p = getattr(self, "_last_train_plan", None)
        if p is None or "saved" not in p:
            raise _hip.LadHipError("backward() without a preceding train-mode forward()")
        x, labels, m1, m2, B, H, W = p["saved"]
        if dprobs is None and labels is None:
            raise _hip.LadHipError("backward() needs dprobs or labels passed to forward()")
        lib = self.lib()
        blocks, acts, sched = p["blocks"], p["acts"], p["schedule"]
        last = blocks[-1].conv2
        # weight-gradient slab sums: one launch at the end instead of one per layer (not with the side stream: the flush
        # would have to follow launches on two streams)
        self._defer_on = self.defer_wgrad_sums and not self.overlap_wgrad
        if self._defer_on:
            _hip.check(self.lib().lad_wgrad_defer_begin(), "lad_wgrad_defer_begin")
        self._launch("lad_head_bwd", self._head_params, self._head_grads, p["pooled"], p["h"], p["hstats"], p["probs"], dprobs, B, p["feat"],
                     m1, m2, labels, p["head_ws"], p["dpooled"])
        g_out = p["g"][(last.h_out, last.w_out)]
        dy = g_out[0]
        self._launch("lad_pool_bwd", p["dpooled"], dy, B, p["h4"], p["w4"], last.cout)
        pre2 = False  # did the producer of `dy` already reduce for this block's bn2?
        pre2_tiles = 0  # ... into how many partials, if not one per 128-row tile (the stride-2 data gradient)
        for bi in range(len(blocks) - 1, -1, -1):
            b, a, ch = blocks[bi], acts[bi], sched.blocks[bi]
            c1s, c2s = b.conv1, b.conv2
            ho, wo, co = c1s.h_out, c1s.w_out, c1s.cout
            hi, wi = c1s.h_in, c1s.w_in
            G = p["g"][(ho, wo)]
            free = [t for t in G if t is not dy]
            aux, da1 = (self._w(a["aux"]) if "aux" in a else free[0]), free[1]
            dc2, dc1 = self._w(a["dc2"]), self._w(a["dc1"])
            bits = a["ybits"] if ch.bits else None
            lower = acts[bi - 1]   # (the block below: read only where the schedule says that its bn2's sums ride in a launch of this one)
            # the element-wise half of a 64-channel BatchNorm backward rides in the weight-gradient launch that consumes it
            # (lad_conv_wgrad_h2_bnbwd writes dc for the data-gradient launch): lad_bn_bwd* then only leaves the coefficients.
            # On the main stream only: the launch also writes the gradient its data-gradient launch reads
            fuse2 = ch.bits and ch.conv2.wgrad_bn and not self.overlap_wgrad
            fuse1 = ch.conv1.wgrad_bn and not self.overlap_wgrad
            if ch.bits:
                # dc2 only; the shortcut's share dy * [y > 0] is formed from dy and the bits in conv1's data gradient below
                self._launch("lad_bn_bwd_bits", dy, bits, a["c2"], a["coef2"], b.bn2.g, None if fuse2 else dc2, b.bn2.gg, b.bn2.gb, p["bn_ws"],
                             p["bcoef"], p["partials"] if pre2 else None,
                             (pre2_tiles or int(lib.lad_conv_num_tiles(B, ho, wo))) if pre2 else 0, B, ho, wo, co, tag=b.bn2.name)
            elif b.sc_conv is None:
                self._bn_bwd(p, b.bn2, dy, a["y"], a["c2"], a["coef2"], dc2, B, ho, wo, 1, mode=1, aux=aux, pre=pre2)
            else:
                self._bn_bwd(p, b.bn2, dy, a["y"], a["c2"], a["coef2"], dc2, B, ho, wo, 1, mode=2, aux=aux,
                             sbn=b.sc_bn, xs=a["cs"], scoef=a["coefs"])
            xin, xcoef = (a["c1"], a["coef1"]) if ch.a1_virtual else (a["a1"], None)
            self._conv_wgrad(p, c2s, ch.conv2.wgrad, xin, dc2, B, in_coef=xcoef, bn=(dy, a["c2"], bits, a["coef2"]) if fuse2 else None)
            # conv2's data gradient, with the first pass of bn1's backward in its epilogue (ReLU decisions recomputed from c1)
            stat = (a["c1"], None, a["coef1"]) if ch.dgrad2_bn else None
            self._conv_s1(c2s, "f32" if ch.dgrad2_bn == "f32" else ch.conv2.arith, "dgrad", dc2, da1, B, ch.conv2.label_dgrad,
                          bn=stat, partials=p["partials"] if stat else None)
            self._bn_bwd(p, b.bn1, da1, None, a["c1"], a["coef1"], None if fuse1 else dc1, B, ho, wo, 2, mode=0, pre=stat is not None)
            if c1s.stride == 1:   # (with the BatchNorm backward on board, the launch writes dc1)
                self._conv_wgrad(p, c1s, ch.conv1.wgrad, a["x"], dc1, B, bn=(da1, a["c1"], None, a["coef1"]) if fuse1 else None)
            if self.debug_capture is not None:
                self.debug_capture[b.name] = {"dy": dy.clone(), "dc2": dc2.clone(), "aux": aux.clone() if bits is None else None, "da1": da1.clone(),
                                              "dc1": dc1.clone()}
            if c1s.stride == 1:
                dx = dy  # dy is dead after the first bn_bwd; never aliases dc1 / aux
                if b.sc_conv is not None:
                    # a stride-1 projection shortcut (resnet_with_augmentation's block1.0, 64 -> 128): aux is the gradient into its
                    # BatchNorm's input; the 1x1 convolution's data gradient (into da1, dead since bn1's backward) becomes the
                    # addend of conv1's data gradient below, its weight gradient reads aux
                    self._conv_wgrad(p, b.sc_conv, ch.sc.wgrad, a["x"], aux, B)
                    self._conv_s1(b.sc_conv, ch.sc.arith, "dgrad", aux, da1, B)
                    aux = da1
                # conv1's data gradient; who consumes dx: the bn2 of the block below (mask from its sign bits on the split-operand
                # kernels, from its y on exact f32), or the stem's BatchNorm, whose sums come from lad_stem_bn_bwd_sums.  A block
                # that keeps sign bits adds the shortcut's share dy * [y > 0] here
                stat = (lower["c2"], lower["ybits" if ch.dgrad1_bn == "split" else "y"], lower["coef2"]) if ch.dgrad1_bn else None
                self._conv_s1(c1s, "f32" if ch.dgrad1_bn == "f32" else ch.conv1.arith, "dgrad", dc1, dx, B, ch.conv1.label_dgrad,
                              addend=dy if ch.bits else aux, abits=bits, bn=stat, partials=p["partials"] if stat else None)
                pre2, pre2_tiles = stat is not None, 0
            else:
                # stride-2 block: gradients of conv1 and of the 1x1 shortcut at their true cost (csrc/conv_s2_bwd.hip)
                dx = p["g"][(hi, wi)][0]
                sc = b.sc_conv

                def s2_wgrad(cs, dout, xin=a["x"]):   # one convolution's weight gradient in a launch of its own
                    self._on_side(lambda sst: self._launch("lad_conv_s2_wgrad", xin, dout, self._wg_ws(p, cs), cs.par.gw, cs.par.gb, B, hi, wi,
                                                           cs.cin, cs.cout, cs.taps, tag=cs.name, stream=sst), dout, small=cs.cin <= 32)

                if ch.sc_wgrad_fused:   # conv1's and the shortcut's weight gradients in one launch (same input rows; csrc/conv_s2_bwd.hip)
                    self._on_side(lambda sst, c1s=c1s, sc=sc, dc1=dc1, aux=aux, xin=a["x"]: self._launch(
                        "lad_conv_s2_wgrad_fused", xin, dc1, aux, self._wg_ws(p, c1s), c1s.par.gw, c1s.par.gb, sc.par.gw, B, hi, wi, c1s.cin, c1s.cout,
                        tag=c1s.name, stream=sst), dc1, small=c1s.cin <= 32)
                    if dc1.data_ptr() in self._side_readers:   # (it ran on the side stream) the launch reads aux as well
                        self._side_readers[aux.data_ptr()] = self._side_readers[dc1.data_ptr()]
                else:
                    s2_wgrad(c1s, dc1)
                # with the sums of the block below's bn2 in the epilogue when that block keeps sign bits (dx is final when it is written)
                stat = (lower["c2"], lower["ybits"], lower["coef2"]) if ch.dgrad1_bn else (None, None, None)
                n_part = 0
                if ch.entry == "s2b3":
                    # both data gradients on the split-operand path, parity class by parity class (dgrad_s2b3_kernel)
                    n_part = int(lib.lad_conv_s2b3_dgrad_partials(B, hi, wi))
                    assert not ch.dgrad1_bn or n_part * 2 * 64 <= p["partials"].numel()
                    self._launch("lad_conv_s2b3_dgrad", dc1, aux, c1s.par.wt3_s2d, dx, p["partials"] if ch.dgrad1_bn else None, *stat, B, hi, wi,
                                 tag=c1s.name)
                elif ch.entry == "s2_fused" and ch.dgrad1_bn:
                    n_part = int(lib.lad_conv_s2_dgrad_partials(B, hi, wi))
                    assert n_part * 2 * 64 <= p["partials"].numel()
                    self._launch("lad_conv_s2_dgrad_fused_bnstat", dc1, c1s.par.wt_d, aux, sc.par.wt_d, dx, p["partials"], *stat, B, hi, wi,
                                 c1s.cin, c1s.cout, tag=c1s.name)
                elif ch.entry == "s2_fused":   # both data gradients in one launch, dx written once
                    self._launch("lad_conv_s2_dgrad_fused", dc1, c1s.par.wt_d, aux, sc.par.wt_d, dx, B, hi, wi, c1s.cin, c1s.cout, tag=c1s.name)
                else:
                    self._launch("lad_conv_s2_dgrad", dc1, c1s.par.wt_d, dx, B, hi, wi, c1s.cin, c1s.cout, 9, 0, tag=c1s.name)
                pre2, pre2_tiles = ch.dgrad1_bn is not None, n_part
                if not ch.sc_wgrad_fused:
                    s2_wgrad(sc, aux)
                if ch.entry == "plain":
                    self._launch("lad_conv_s2_dgrad", aux, sc.par.wt_d, dx, B, hi, wi, sc.cin, sc.cout, 1, 1, tag=sc.name)
            dy = dx
        # stem: bn1 + conv1 weight gradient.  The input needs no gradient and the convolution is recomputed from the features:
        # sums (x recomputed) -> lad_bn_bwd finalises them into dgamma / dbeta / bcoef (dx = None: nothing to apply) ->
        # the weight-gradient kernel applies the BatchNorm backward on the fly.  Neither x nor dz ever exist in HBM.
        if sched.stem_onepass:
            # ONE pass over dy (the BatchNorm's sums and the centred tap products together), the rest from the forward's moments
            bn = self.stem_bn
            self._launch("lad_stem_bwd_onepass", x, self.stem_w, dy, p["stem_coef"], bn.g, p["stem_mom"], p["stem_bwd_ws"], self.stem_gw, bn.gg,
                         bn.gb, B, H, W, self.stem_cout)
        else:
            groups = int(lib.lad_stem_bn_bwd_groups(B, H, W))
            self._launch("lad_stem_bn_bwd_sums", x, self.stem_w, dy, p["stem_coef"], p["partials"], B, H, W, self.stem_cout)
            bn = self.stem_bn
            self._launch("lad_bn_bwd", dy, None, None, p["stem_coef"], bn.g, None, None, None, None, None, bn.gg, bn.gb, None, None,
                         p["bn_ws"], p["bcoef"], p["partials"], groups, B, H, W, bn.c, 2, 0, tag=bn.name)
            self._on_side(lambda sst: self._launch("lad_stem_wgrad_bn", x, dy, None, self.stem_w, p["stem_coef"], p["bcoef"], p["wgrad_ws"],
                                                   self.stem_gw, B, H, W, self.stem_cout, stream=sst), dy)
        if self._defer_on:
            self._defer_on = False
            self._join_side()   # (the one launch that sums every layer's slabs follows the weight-gradient launches of both streams)
            self._launch("lad_wgrad_defer_flush")
        self._join_side()
        self._grad_dirty = True

    def export_relu_masks(self):
        """ReLU decisions of the last train-mode forward, as CPU 0/1 tensors in the reference's (B,C,H,W) layout:
        {"stem", "block<k>.<j>.a1", "block<k>.<j>.y", "head"}.  For parity tests only (tests/test_resnet_gpu.py: with these
        decisions imposed on a CPU autograd run the two backward passes compute the same function)."""
        p = getattr(self, "_last_train_plan", None)
        if p is None or "saved" not in p:
            raise _hip.LadHipError("export_relu_masks() without a preceding train-mode forward()")
        x, labels, m1, m2, B, H, W = p["saved"]

        def unpack(buf, h, w, c):
            body = buf[:B * (h + 1) * (w + 1) * c].view(B, h + 1, w + 1, c)[:, 1:, 1:, :]
            return (body > 0).permute(0, 3, 1, 2).cpu()

        out = {"stem": unpack(p["stem_a"], H, W, self.stem_cout)}
        for b, ch, a in zip(p["blocks"], p["schedule"].blocks, p["acts"]):
            ho, wo, co = b.conv1.h_out, b.conv1.w_out, b.conv1.cout
            if ch.a1_virtual:
                # never stored: the sign of the kernels' fmaf(c1, scale, shift), taken from the same expression in double (the
                # product is exact there and the sum keeps its sign; a separate fp32 multiply + add does NOT always agree)
                c = a["c1"][:B * (ho + 1) * (wo + 1) * co].view(B, ho + 1, wo + 1, co)[:, 1:, 1:, :].double()
                sc, sh = a["coef1"][:co].double(), a["coef1"][co:2 * co].double()
                out[b.name + ".a1"] = (c * sc + sh > 0).permute(0, 3, 1, 2).cpu()
            else:
                out[b.name + ".a1"] = unpack(a["a1"], ho, wo, co)
            out[b.name + ".y"] = unpack(a["y"], ho, wo, co)
        # head: relu(dropout(bn3(h))) with batch statistics; h = linear1 output kept for the backward
        h = p["h"].view(B, 32).double()
        mean, var = h.mean(0), h.var(0, unbiased=False)
        u = (h - mean) / torch.sqrt(var + 1e-5) * self.head_bn3.g.double() + self.head_bn3.b.double()
        if m2 is not None:
            u = u * m2.double()
        out["head"] = (u > 0).cpu()
        return out

    # ------------------------------------------------------------------------------------ optimiser
    def reset_optimizer(self):
        """A fresh Adam, as run_epoch creates at train.py:336."""
        self.ensure_flat()
        self._exp_avg.zero_()
        self._exp_avg_sq.zero_()
        self._step_dev.zero_()
        self._step_count = 0

    def reset_dropout_rng(self):
        """Restart the sequence of dropout-mask draws of the fused step (masks are a function of torch's CUDA seed and the draw number; a
        change of the seed restarts it by itself, a torch.manual_seed with the SAME value cannot be told from no call)."""
        self.ensure_flat()
        self._rng_counter.zero_()

    def flat_grad(self):
        self.ensure_flat()
        return self._flat_g

    def flat_param(self):
        self.ensure_flat()
        return self._flat_p

    def accumulated_grad(self):
        """The accumulation buffer of the fused loop's gradient accumulation (zeros until accumulate_grad() is called)."""
        self.ensure_flat()
        if getattr(self, "_acc_g", None) is None:
            self._acc_g = torch.zeros_like(self._flat_g)
        return self._acc_g

    def accumulate_grad(self, scale):
        """accumulated_grad() += scale * flat_grad(): `(loss / gradient_accumulation_steps).backward()` of train.py:287-289
        (the engine's backward overwrites the flat gradient, so the running sum lives in a buffer of its own)."""
        acc = self.accumulated_grad()
        self._launch("lad_grad_accumulate", acc, self._flat_g, self._n_flat, float(scale))
        return acc

    def clip_and_step(self, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_norm=1.0, grad_scale=1.0, zero_grad=True, grad=None):
        """clip_grad_norm_(max_norm) + Adam.step() + zero_grad() (train.py:291-295) in two launches.
        grad_scale multiplies the gradient first (1/world_size after a sum all-reduce).  grad: the gradient buffer to step
        with (default: the flat gradient; the accumulation buffer under gradient accumulation)."""
        self.ensure_flat()
        g = self._flat_g if grad is None else grad
        if g.numel() != self._n_flat or g.dtype != torch.float32 or not g.is_cuda:
            raise _hip.LadHipError("clip_and_step: grad must be a float32 GPU buffer of the flat parameter size")
        self._step_count += 1  # host mirror; the kernels use the device-side counter (hipGraph replays)
        self._launch("lad_grad_sumsq", g, self._n_flat, self._norm_partials, self._step_dev)
        self._launch("lad_adam_step", self._flat_p, g, self._exp_avg, self._exp_avg_sq, self._n_flat, self._norm_partials, float(grad_scale),
                     float(max_norm if max_norm is not None else 0.0), float(lr), float(betas[0]), float(betas[1]), float(eps),
                     self._step_count, self._step_dev, 1 if zero_grad else 0, self._norm_out)
        self.notify_weights_changed()
        if zero_grad:
            self._grad_dirty = False
        return self._norm_out

    def optimizer_state(self):
        """Tensors that make up the optimiser + parameter state (for snapshot / restore around graph warm-up)."""
        self.ensure_flat()
        return [self._flat_p, self._flat_g, self._exp_avg, self._exp_avg_sq, self._step_dev]

    def eval_metrics(self, probs, labels, out=None):
        """Counter vector (same layout as metrics()) of eval-mode probabilities against int32 labels, on the device."""
        _hip.require_cuda(probs, "probs", torch.float32)
        _hip.require_cuda(labels, "labels", torch.int32)
        if out is None:
            out = torch.zeros(8, device=probs.device)
        self._launch("lad_bce_metrics", probs, labels, probs.numel(), out)
        return out

    def metrics(self):
        """float32[8] device tensor of the last train forward: mean BCE, #correct, #pred+, #true+, #target+, B."""
        return self._last_train_plan["metrics"]


def dropout_masks(B, feat, rate, device, generator=None):
    """Inverted-dropout masks for the two nn.Dropout calls of models.py:232,235 (torch RNG, tiny tensors)."""
    if rate <= 0.0:
        return None
    keep = 1.0 - rate
    m1 = torch.empty((B, feat), device=device).bernoulli_(keep, generator=generator).div_(keep)
    m2 = torch.empty((B, 32), device=device).bernoulli_(keep, generator=generator).div_(keep)
    return m1, m2


def metrics_from_counters(m):
    """(loss, accuracy, precision, recall) from the head's counter vector, as _calc_metrics (train.py:203-224)."""
    loss, corr, pp, tp, tt, n = [float(v) for v in m[:6]]
    acc = corr / n if n else float("nan")
    prec = 1.0 if pp == 0 else tp / pp
    rec = tp / tt if tt != 0 else float("nan")
    return loss, acc, prec, rec
