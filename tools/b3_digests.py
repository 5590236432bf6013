"""SHA-256 digests of what the bf16 x 3 entry points write for seeded inputs: the recorder behind tests/test_b3_parent_bits_gpu.py,
which imports the cases, the inputs and the launches from here.

    LAD_HIP_LIB=<library of the commit to record> python tools/b3_digests.py [out.json]     (default: tests/golden/b3_parent.json)

Convolutions (conv_b3x_kernel, conv_s2b3_kernel, dgrad_s2b3_kernel): lad_conv_b3c_fwd_f32 and lad_conv_b3c_fwd_f32_bnrelu at 64 and
32 channels, lad_conv_b3_fwd_f32_gated in place, lad_conv_b3_dgrad_bnstat with and without bn_bits, lad_conv_b3c_dgrad_bnstat,
lad_conv_s2b3_fwd and lad_conv_s2b3_dgrad (with and without the BatchNorm sums).  Weight gradients (wgrad_b3x_kernel at 64 channels,
wgrad_b3_kernel at 32): lad_conv_wgrad_b3c with and without in_coef.  Every input comes from a seeded CPU generator, coefficient
tables and sign bits included, so the only kernels that take part are the entry point's own and the weight packers.  A combination an
entry point refuses (the stride-2 transition of a one-pixel image; the 32-channel weight gradient at W = 46, whose 64-row tile and
halo exceed the window) is recorded as "refused", so that the argument checks are held in place too."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conv_h2_digests import SHAPES as H2_SHAPES, act_rows, to_pnhwc, sha  # noqa: E402  (also puts the package on sys.path)

GOLDEN = os.path.join(ROOT, "tests", "golden", "b3_parent.json")

# (C, B, H, W) of tools/conv_h2_digests.py below its 256-row threshold (these kernels have one tile size): one pixel; tiles crossing
# image boundaries (3 x 13 x 6 is also the smallest launch with two 256-row tiles); three tiles; the widest image; 32 channels
CONV_SHAPES = H2_SHAPES[:5]
CONV_FORMS = ["fwd", "fwd_addend", "bnrelu", "gated_inplace", "dgrad_stat_x", "dgrad_stat_bits_gated", "dgrad_stat_c", "s2_fwd", "s2_dgrad",
              "s2_dgrad_stat"]
ONLY_64 = ("gated_inplace", "dgrad_stat_x", "dgrad_stat_bits_gated", "s2_fwd", "s2_dgrad", "s2_dgrad_stat")   # entry points without a channel count
# (B, H, W) of tests/test_wgrad_h2_window_gpu.py: in the first three a workgroup takes several tiles, the window wraps and the last
# workgroups get no tile (they write a zero slab); the widest halo; one tile; one pixel
WGRAD_SHAPES = [(20, 100, 44), (20, 100, 46), (840, 13, 6), (3, 13, 6), (1, 1, 1)]


def conv_key(shape, form):
    C, B, H, W = shape
    return f"conv/C{C}/{B}x{H}x{W}/{form}"


def wgrad_key(C, shape, in_bn):
    B, H, W = shape
    return f"wgrad/C{C}/{B}x{H}x{W}" + ("/in_coef" if in_bn else "")


def conv_cases():
    return [(s, f) for s in CONV_SHAPES for f in CONV_FORMS if s[0] == 64 or f not in ONLY_64]


def wgrad_cases():
    return [(C, s, bn) for C in (64, 32) for s in WGRAD_SHAPES for bn in (False, True)]


def _coef(C, g):
    coef = torch.zeros(6, C)                                               # scale, shift, mean, istd, mean_lo, istd_lo
    coef[0], coef[1] = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.4
    coef[2], coef[3] = torch.randn(C, generator=g) * 0.1 + 1, torch.rand(C, generator=g) * 0.2 + 0.4
    coef[4], coef[5] = coef[2] * 2.0 ** -26, coef[3] * 2.0 ** -26
    return coef


_conv_inputs = {}


def make_conv_inputs(shape):
    """Everything a convolution launch of any form reads, from one seeded CPU generator; on the GPU, cached per shape."""
    if shape in _conv_inputs:
        return _conv_inputs[shape]
    import _hip as h
    lib = h.lib()
    st = h.stream_handle()
    C, B, H, W = shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    g = torch.Generator().manual_seed(11000 + C * 1009 + B * 131 + H * 7 + W)
    x = torch.randn(B, C, H, W, generator=g) * 1.5 + 0.5
    add = torch.randn(B, C, H, W, generator=g)
    bnx = torch.randn(B, C, H, W, generator=g) * 2 + 1                     # input of the BatchNorm whose backward consumes `out`
    w = torch.randn(C, C, 3, 3, generator=g) * 0.1
    bias = torch.randn(C, generator=g)
    in_coef = torch.zeros(6, C)
    in_coef[0], in_coef[1] = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    rows = act_rows(B, H, W)
    abits = torch.randint(-2 ** 63, 2 ** 63 - 1, (rows,), generator=g, dtype=torch.int64)
    bbits = torch.randint(-2 ** 63, 2 ** 63 - 1, (rows,), generator=g, dtype=torch.int64)
    t = dict(x=to_pnhwc(x), add=to_pnhwc(add), bnx=to_pnhwc(bnx), bias=bias.cuda(), in_coef=in_coef.reshape(-1).cuda(),
             coef=_coef(C, g).reshape(-1).cuda(), abits=abits.cuda(), bbits=bbits.cuda(), wt={})
    wg = w.cuda()
    for mode in (0, 1):
        wt = torch.zeros(int(lib.lad_conv_b3c_packed_weight_bytes(C)), device="cuda", dtype=torch.uint8)
        h.check(lib.lad_conv_b3c_pack_weights(h.ptr(wg), mode, h.ptr(wt), C, st), "lad_conv_b3c_pack_weights")
        t["wt"][mode] = wt
    if C == 64:   # the stride-2 transition 64 -> 32
        w3, w1 = (torch.randn(32, 64, 3, 3, generator=g) * 0.1).cuda(), (torch.randn(32, 64, 1, 1, generator=g) * 0.3).cuda()
        t["s2_bias"] = torch.randn(32, generator=g).cuda()
        t["s2_d3"], t["s2_d1"] = (to_pnhwc(torch.randn(B, 32, Ho, Wo, generator=g)) for _ in range(2))
        t["s2_wt"] = torch.zeros(int(lib.lad_conv_s2b3_packed_weight_bytes()), device="cuda", dtype=torch.uint8)
        t["s2_wtd"] = torch.zeros(int(lib.lad_conv_s2b3_dgrad_packed_weight_bytes()), device="cuda", dtype=torch.uint8)
        h.check(lib.lad_conv_s2b3_pack_weights(h.ptr(w3), h.ptr(w1), h.ptr(t["s2_wt"]), st), "lad_conv_s2b3_pack_weights")
        h.check(lib.lad_conv_s2b3_dgrad_pack_weights(h.ptr(w3), h.ptr(w1), h.ptr(t["s2_wtd"]), st), "lad_conv_s2b3_dgrad_pack_weights")
    torch.cuda.synchronize()
    _conv_inputs[shape] = t
    return t


def launch_conv(shape, form, t):
    """One launch of the form.  Returns its outputs (GPU tensors) by name, or None when the entry point refuses it."""
    import _hip as h
    lib = h.lib()
    st = h.stream_handle()
    P = h.ptr
    C, B, H, W = shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    rows = act_rows(B, H, W)
    out = torch.full((rows * C,), 9.0, device="cuda")
    part = torch.full((int(lib.lad_conv_num_tiles(B, H, W)) * 2 * C,), -7.0, device="cuda")
    fwd, dgrad = t["wt"][0], t["wt"][1]
    res = {"out": out, "partials": part}
    if form == "fwd":
        rc = lib.lad_conv_b3c_fwd_f32(P(t["x"]), P(fwd), P(t["bias"]), None, P(out), P(part), B, H, W, C, st)
    elif form == "fwd_addend":
        rc = lib.lad_conv_b3c_fwd_f32(P(t["x"]), P(fwd), P(t["bias"]), P(t["add"]), P(out), P(part), B, H, W, C, st)
    elif form == "bnrelu":
        rc = lib.lad_conv_b3c_fwd_f32_bnrelu(P(t["x"]), P(t["in_coef"]), P(fwd), P(t["bias"]), P(out), P(part), B, H, W, C, st)
    elif form == "gated_inplace":
        out = t["add"].clone()
        res = {"out": out}
        rc = lib.lad_conv_b3_fwd_f32_gated(P(t["x"]), P(dgrad), None, P(out), P(t["abits"]), P(out), None, B, H, W, st)
    elif form == "dgrad_stat_x":
        rc = lib.lad_conv_b3_dgrad_bnstat(P(t["x"]), P(dgrad), None, None, P(out), P(part), P(t["bnx"]), None, P(t["coef"]), B, H, W, st)
    elif form == "dgrad_stat_bits_gated":
        rc = lib.lad_conv_b3_dgrad_bnstat(P(t["x"]), P(dgrad), P(t["add"]), P(t["abits"]), P(out), P(part), P(t["bnx"]), P(t["bbits"]),
                                          P(t["coef"]), B, H, W, st)
    elif form == "dgrad_stat_c":
        rc = lib.lad_conv_b3c_dgrad_bnstat(P(t["x"]), P(dgrad), P(t["add"]), P(out), P(part), P(t["bnx"]), P(t["coef"]), B, H, W, C, st)
    elif form == "s2_fwd":
        o3, o1 = (torch.full((act_rows(B, Ho, Wo) * 32,), 4.0, device="cuda") for _ in range(2))
        p3, p1 = (torch.full((int(lib.lad_conv_num_tiles(B, Ho, Wo)) * 2 * 32,), 9.0, device="cuda") for _ in range(2))
        res = {"out": o3, "partials": p3, "out_sc": o1, "partials_sc": p1}
        rc = lib.lad_conv_s2b3_fwd(P(t["x"]), P(t["s2_wt"]), P(t["s2_bias"]), P(o3), P(p3), P(o1), P(p1), B, H, W, st)
    elif form in ("s2_dgrad", "s2_dgrad_stat"):
        dx = torch.zeros(rows * C, device="cuda")   # (border rows are not written: zero by the layout invariant)
        dx.view(-1, C)[:B * (H + 1) * (W + 1)].view(B, H + 1, W + 1, C)[:, 1:, 1:] = 3.0
        res = {"dx": dx}
        if form == "s2_dgrad":
            rc = lib.lad_conv_s2b3_dgrad(P(t["s2_d3"]), P(t["s2_d1"]), P(t["s2_wtd"]), P(dx), None, None, None, None, B, H, W, st)
        else:
            n_part = int(lib.lad_conv_s2b3_dgrad_partials(B, H, W))
            res["partials"] = part = torch.full((max(n_part, 0) * 2 * C,), 7.0, device="cuda")
            rc = lib.lad_conv_s2b3_dgrad(P(t["s2_d3"]), P(t["s2_d1"]), P(t["s2_wtd"]), P(dx), P(part), P(t["bnx"]), P(t["bbits"]), P(t["coef"]),
                                         B, H, W, st)
    else:
        raise ValueError(form)
    torch.cuda.synchronize()
    return None if rc != 0 else res


_wgrad_inputs = {}


def make_wgrad_inputs(C, shape):
    if (C, shape) in _wgrad_inputs:
        return _wgrad_inputs[(C, shape)]
    B, H, W = shape
    g = torch.Generator().manual_seed(13000 + C * 1009 + B * 131 + H * 7 + W)
    x = torch.randn(B, C, H, W, generator=g) * 1.5 + 0.5
    dy = torch.randn(B, C, H, W, generator=g) * torch.exp(torch.randn(1, C, 1, 1, generator=g))
    in_coef = torch.zeros(6, C)
    in_coef[0], in_coef[1] = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    _wgrad_inputs.clear()   # (one shape's tensors on the device at a time)
    _wgrad_inputs[(C, shape)] = t = dict(x=to_pnhwc(x), dy=to_pnhwc(dy), in_coef=in_coef.reshape(-1).cuda())
    return t


def launch_wgrad(C, shape, in_bn, t):
    import _hip as h
    lib = h.lib()
    B, H, W = shape
    ws = torch.zeros(int(lib.lad_conv_wgrad_b3c_workspace_floats(C)), device="cuda")
    dw, db = torch.full((C, C, 3, 3), 5.0, device="cuda"), torch.full((C,), 5.0, device="cuda")
    rc = lib.lad_conv_wgrad_b3c(h.ptr(t["x"]), h.ptr(t["in_coef"]) if in_bn else None, h.ptr(t["dy"]), h.ptr(ws), h.ptr(dw), h.ptr(db), B, H, W, C,
                                h.stream_handle())
    torch.cuda.synchronize()
    return None if rc != 0 else {"dw": dw, "dbias": db}


def _digest(res):
    return "refused" if res is None else {k: sha(v) for k, v in res.items()}


def conv_digests(shape, form):
    return _digest(launch_conv(shape, form, make_conv_inputs(shape)))


def wgrad_digests(C, shape, in_bn):
    return _digest(launch_wgrad(C, shape, in_bn, make_wgrad_inputs(C, shape)))


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    import _hip as h
    rec = {conv_key(s, f): conv_digests(s, f) for s, f in conv_cases()}
    rec.update({wgrad_key(C, s, bn): wgrad_digests(C, s, bn) for C, s, bn in wgrad_cases()})
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    n_ref = sum(1 for v in rec.values() if v == "refused")
    print(f"{len(rec)} cases ({n_ref} refused by the entry point) from {h.LIB_PATH} -> {path}")


if __name__ == "__main__":
    main()
