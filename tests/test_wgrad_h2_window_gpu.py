"""wgrad_h2_kernel's input window at a fixed pitch with guard slots (csrc/wgrad_mfma.hip): the same bits as the circular,
swizzled window it replaces.

A workgroup takes more than one tile only above 512 tiles of 32 rows, so only tensors of some size ever wrap the window.  For
each shape and each of the four forms (plain; BatchNorm + ReLU on the input side; the BatchNorm backward on the gradient side
with the ReLU decisions from the BatchNorm's input, and from sign bits together with the input-side BatchNorm) the weight
gradient, the bias gradient and the BatchNorm input gradient `dc` are compared by SHA-256 with digests recorded from the build
before the change (tests/golden/wgrad_h2_parent.json); inputs come from seeded CPU generators, coefficient tables included, so
no other kernel takes part.  The weight gradient is also held against float64 autograd at the bars of
test_wgrad_h2_matches_the_f32_weight_gradient (2e-4 of max), so the test still says something should the digests go stale."""
import hashlib
import json
import os

import pytest
import torch
import torch.nn.functional as F

from test_resnet_gpu import _lib, act_rows, from_pnhwc, to_pnhwc

pytestmark = pytest.mark.gpu

C = 64
SHAPES = [(20, 100, 44),   # the bench width: about 5.5 tiles per workgroup, the window wraps
          (20, 100, 46),   # the widest halo: 126 of 128 slots live
          (840, 13, 6),    # 32 rows span several image rows, and the window still wraps
          (3, 13, 6), (1, 1, 1)]
FORMS = ["plain", "in_coef", "bnbwd_x", "bnbwd_bits"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_h2_parent.json")


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def make_inputs(B, H, W, form, ramp=False):
    """Everything a launch reads, from one seeded CPU generator (the same draws for every form of a shape)."""
    g = torch.Generator().manual_seed(9000 + B * 131 + H * 7 + W)
    x = torch.randn(B, C, H, W, generator=g) * 1.5 + 0.5
    dy = torch.randn(B, C, H, W, generator=g) * torch.exp(torch.randn(1, C, 1, 1, generator=g))
    cx = torch.randn(B, C, H, W, generator=g) * 2 + 1                       # the BatchNorm's input on the gradient side
    in_coef = torch.stack([torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3])   # scale, shift
    coef = torch.zeros(6, C)                                                # scale, shift, mean, istd, mean_lo, istd_lo
    coef[0], coef[1] = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.4
    coef[2], coef[3] = torch.randn(C, generator=g) * 0.1 + 1, torch.rand(C, generator=g) * 0.2 + 0.4
    coef[4], coef[5] = coef[2] * 2.0 ** -26, coef[3] * 2.0 ** -26
    bcoef = torch.zeros(8, C)                                               # rows 0, 1, 2, 4, 6: k1, k2, k3, k2_lo, k3_lo
    bcoef[0], bcoef[1], bcoef[2] = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.01, torch.randn(C, generator=g) * 0.01
    bcoef[4], bcoef[6] = bcoef[1] * 2.0 ** -26, bcoef[2] * 2.0 ** -26
    bits = torch.randint(-2 ** 63, 2 ** 63 - 1, (act_rows(B, H, W),), generator=g, dtype=torch.int64)
    if ramp:   # test_wgrad_h2_running_scales_follow_the_data: magnitudes grow by 2^40 down every image, zeros first
        r = torch.linspace(-20, 20, H).view(1, 1, H, 1)
        x = (x - 0.5) * torch.exp2(r)
        x[0:2] = 0.0
        dy = dy * 1e-12 * torch.exp2(-r.flip(2) * 0.5)
        dy[5] *= 1e6
    return dict(x=x, dy=dy, cx=cx, in_coef=in_coef, coef=coef, bcoef=bcoef, bits=bits)


def launch(B, H, W, form, t):
    """One launch of the form; returns the outputs (GPU tensors) by name."""
    h = _lib()
    lib = h.lib()
    st = h.stream_handle()
    xin, dyg = to_pnhwc(t["x"]), to_pnhwc(t["dy"])
    in_coef = t["in_coef"].reshape(-1).cuda() if form in ("in_coef", "bnbwd_bits") else None
    ws = torch.zeros(int(lib.lad_conv_wgrad_workspace_floats(C, C, 9)), device="cuda")
    dw, db = torch.zeros(C, C, 3, 3, device="cuda"), torch.zeros(C, device="cuda")
    out = {"dw": dw, "dbias": db}
    if form in ("plain", "in_coef"):
        h.check(lib.lad_conv_wgrad_h2(h.ptr(xin), h.ptr(in_coef), h.ptr(dyg), h.ptr(ws), h.ptr(dw), h.ptr(db), B, H, W, C, st), "lad_conv_wgrad_h2")
    else:
        cx, coef, bcoef = to_pnhwc(t["cx"]), t["coef"].reshape(-1).cuda(), t["bcoef"].reshape(-1).cuda()
        bits = t["bits"].cuda() if form == "bnbwd_bits" else None
        dc = torch.full((act_rows(B, H, W) * C,), -3.0, device="cuda")
        h.check(lib.lad_conv_wgrad_h2_bnbwd(h.ptr(xin), h.ptr(in_coef), h.ptr(dyg), h.ptr(cx), h.ptr(bits), h.ptr(coef), h.ptr(bcoef), h.ptr(dc),
                                            h.ptr(ws), h.ptr(dw), h.ptr(db), B, H, W, C, st), "lad_conv_wgrad_h2_bnbwd")
        out["dc"] = dc
    torch.cuda.synchronize()
    return out


def digests(B, H, W, form, ramp=False):
    return {k: sha(v) for k, v in launch(B, H, W, form, make_inputs(B, H, W, form, ramp)).items()}


def case_key(B, H, W, form, ramp=False):
    return f"{B}x{H}x{W}/{form}" + ("/ramp" if ramp else "")


def float64_dw(x, dout):
    wr = torch.zeros(C, C, 3, 3, requires_grad=True, dtype=torch.float64)
    (F.conv2d(x.double(), wr, None, padding=1) * dout.double()).sum().backward()
    return wr.grad


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_wgrad_h2_window_gives_the_bits_of_the_circular_window(B, H, W, form, golden):
    t = make_inputs(B, H, W, form)
    out = launch(B, H, W, form, t)
    # float64: the operands as the kernel sees them (the input-side BatchNorm + ReLU; dc as the kernel wrote it)
    x = t["x"]
    if form in ("in_coef", "bnbwd_bits"):
        x = torch.relu(x.double() * t["in_coef"][0].double().view(1, C, 1, 1) + t["in_coef"][1].double().view(1, C, 1, 1))
    dout = from_pnhwc(out["dc"], B, C, H, W) if "dc" in out else t["dy"]
    ref = float64_dw(x, dout)
    scale = ref.abs().max().item()
    err = (out["dw"].cpu().double() - ref).abs().max().item()
    got = {k: sha(v) for k, v in out.items()}
    print(case_key(B, H, W, form), "dw error / max =", err / max(scale, 1e-300), got)
    assert err <= 2e-4 * scale, err / scale
    assert got == golden[case_key(B, H, W, form)]


def test_wgrad_h2_window_guard_rows_follow_an_exponent_drop(golden):
    """Built like test_wgrad_h2_running_scales_follow_the_data: every few tiles the input exponent drops and the window's
    2 x halo older rows are staged again -- guard copies included -- over many wraps of the window."""
    B, H, W = 24, 100, 44
    t = make_inputs(B, H, W, "plain", ramp=True)
    out = launch(B, H, W, "plain", t)
    ref = float64_dw(t["x"], t["dy"])
    scale = ref.abs().max().item()
    err = (out["dw"].cpu().double() - ref).abs().max().item()
    got = {k: sha(v) for k, v in out.items()}
    print(case_key(B, H, W, "plain", True), "dw error / max =", err / scale, got)
    assert bool(torch.isfinite(out["dw"]).all())
    assert err <= 2e-6 * scale, err / scale
    assert got == golden[case_key(B, H, W, "plain", True)]
