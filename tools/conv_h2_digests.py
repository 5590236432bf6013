"""SHA-256 digests of what lad_conv_h2 writes (`out` and `partials`) for seeded inputs: the recorder behind
tests/test_conv_h2_epilogue_gpu.py, which imports the cases, the inputs and the launches from here.

    LAD_HIP_LIB=<library of the commit to record> python tools/conv_h2_digests.py [out.json]     (default: tests/golden/conv_h2_parent.json)

Every input comes from a seeded CPU generator, coefficient tables and sign bits included, so the only kernels that take part are
lad_conv_h2 and the weight packer.  A combination the entry point refuses (the backward sums together with an input BatchNorm;
sign bits at 32 channels) is recorded as "refused", so that the argument checks are held in place too."""
import hashlib
import json
import os
import struct
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "laughter-detection-icsi_amd", "utils"), os.path.join(ROOT, "laughter-detection-icsi_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_h2_parent.json")

# (C, B, H, W): the 128-row kernel (one pixel; tiles crossing image boundaries; the widest image; 32 channels), then the smallest
# launches that take the 256-row kernel (1024 tiles of 256 rows)
SHAPES = [(64, 1, 1, 1), (64, 3, 13, 6), (64, 2, 25, 11), (64, 5, 7, 46), (32, 3, 13, 6), (64, 64, 100, 44), (32, 230, 50, 22)]
FORMS = ["bias_partials", "addend", "gated_inplace", "stat_x", "stat_bits_gated"]
# exponent cases: (name, shape, forms)
#   tiny : inputs x 1e-25 against weights x 1e-20, bias of the outputs' size: subnormal outputs, accumulator exponents beyond 126
#   range: image 1 has its second 32 channels x 1e12 (re-basing up to the +8 cap), image 2 x 1e-12 (far down), image 3 an all-zero
#          first stage
EXPONENT = [("tiny", (64, 3, 13, 6), FORMS), ("range", (64, 4, 25, 11), FORMS), ("range", (64, 64, 100, 44), ["bias_partials", "stat_bits_gated"])]


def act_rows(B, H, W):
    return B * (H + 1) * (W + 1) + (W + 1) + 1


def to_pnhwc(x):
    B, C, H, W = x.shape
    buf = torch.zeros(act_rows(B, H, W) * C)
    buf[:B * (H + 1) * (W + 1) * C].view(B, H + 1, W + 1, C)[:, 1:, 1:, :] = x.permute(0, 2, 3, 1)
    return buf.cuda()


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def case_key(shape, form, in_bn, expo=None):
    C, B, H, W = shape
    return f"C{C}/{B}x{H}x{W}/{form}" + ("/in_coef" if in_bn else "") + (f"/{expo}" if expo else "")


def cases():
    """Every (shape, form, in_bn, exponent case) of the test, in the order they are recorded."""
    out = [(s, f, bn, None) for s in SHAPES for f in FORMS for bn in (False, True)]
    out += [(s, f, bn, e) for e, s, fs in EXPONENT for f in fs for bn in (False, True)]
    return out


_inputs = {}


def make_inputs(shape, expo=None):
    """Everything a launch of any form reads, from one seeded CPU generator; on the GPU, cached per (shape, exponent case)."""
    if (shape, expo) in _inputs:
        return _inputs[(shape, expo)]
    C, B, H, W = shape
    g = torch.Generator().manual_seed(7000 + C * 1009 + B * 131 + H * 7 + W)
    x = torch.randn(B, C, H, W, generator=g) * 1.5 + 0.5
    add = torch.randn(B, C, H, W, generator=g)
    bnx = torch.randn(B, C, H, W, generator=g) * 2 + 1                     # input of the BatchNorm whose backward consumes `out`
    w = torch.randn(C, C, 3, 3, generator=g) * 0.1
    bias = torch.randn(C, generator=g)
    in_coef = torch.zeros(6, C)
    in_coef[0], in_coef[1] = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3   # scale, shift
    coef = torch.zeros(6, C)                                               # scale, shift, mean, istd, mean_lo, istd_lo
    coef[0], coef[1] = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.4
    coef[2], coef[3] = torch.randn(C, generator=g) * 0.1 + 1, torch.rand(C, generator=g) * 0.2 + 0.4
    coef[4], coef[5] = coef[2] * 2.0 ** -26, coef[3] * 2.0 ** -26
    rows = act_rows(B, H, W)
    abits = torch.randint(-2 ** 63, 2 ** 63 - 1, (rows,), generator=g, dtype=torch.int64)
    bbits = torch.randint(-2 ** 63, 2 ** 63 - 1, (rows,), generator=g, dtype=torch.int64)
    if expo == "tiny":
        x, w = x * 1e-25, w * 1e-20
        bias, add = bias * 2e-44, add * 2e-44
        in_coef[1] *= 1e-25
    elif expo == "range":
        x[1 % B, 32:] *= 1e12
        x[2 % B, 32:] *= 1e-12
        x[3 % B, :32] = 0.0
        in_coef[1, :32] = -torch.rand(32, generator=g)                    # (with the input BatchNorm some tiles keep a zero first stage)
    import _hip as h
    lib = h.lib()
    t = dict(x=to_pnhwc(x), add=to_pnhwc(add), bnx=to_pnhwc(bnx), bias=bias.cuda(), in_coef=in_coef.reshape(-1).cuda(),
             coef=coef.reshape(-1).cuda(), abits=abits.cuda(), bbits=bbits.cuda(), wt={})
    wg = w.cuda()
    for mode in (0, 1):
        wt = torch.zeros(int(lib.lad_conv_h2_packed_weight_bytes(C)), device="cuda", dtype=torch.uint8)
        table = torch.frombuffer(bytearray(struct.pack("<QQii", wg.data_ptr(), wt.data_ptr(), mode, 0)), dtype=torch.uint8).cuda()
        h.check(lib.lad_conv_h2_pack_weights_multi(h.ptr(table), 1, C, h.stream_handle()), "lad_conv_h2_pack_weights_multi")
        torch.cuda.synchronize()
        t["wt"][mode] = wt
    if len(_inputs) >= 2:   # (the large shapes: keep the device memory of two cases at most)
        _inputs.pop(next(iter(_inputs)))
    _inputs[(shape, expo)] = t
    return t


def launch(shape, form, in_bn, t):
    """One launch of the form.  Returns {"out": tensor, "partials": tensor} (GPU), or None when the entry point refuses it."""
    import _hip as h
    lib = h.lib()
    st = h.stream_handle()
    C, B, H, W = shape
    rows = act_rows(B, H, W)
    n_tiles = int(lib.lad_conv_num_tiles(B, H, W))
    P = h.ptr
    in_coef = P(t["in_coef"]) if in_bn else None
    out = torch.full((rows * C,), 9.0, device="cuda")
    part = torch.full((n_tiles * 2 * C,), -7.0, device="cuda")
    fwd, dgrad = t["wt"][0], t["wt"][1]
    if form == "bias_partials":
        a = (P(t["x"]), in_coef, P(fwd), P(t["bias"]), None, None, P(out), P(part), None, None, None)
    elif form == "addend":
        a = (P(t["x"]), in_coef, P(fwd), P(t["bias"]), P(t["add"]), None, P(out), P(part), None, None, None)
    elif form == "gated_inplace":
        out = t["add"].clone()
        a = (P(t["x"]), in_coef, P(dgrad), None, P(out), P(t["abits"]), P(out), None, None, None, None)
    elif form == "stat_x":
        a = (P(t["x"]), in_coef, P(dgrad), None, None, None, P(out), P(part), P(t["bnx"]), None, P(t["coef"]))
    elif form == "stat_bits_gated":
        a = (P(t["x"]), in_coef, P(dgrad), None, P(t["add"]), P(t["abits"]), P(out), P(part), P(t["bnx"]), P(t["bbits"]), P(t["coef"]))
    else:
        raise ValueError(form)
    rc = lib.lad_conv_h2(*a, B, H, W, C, st)
    torch.cuda.synchronize()
    if rc != 0:
        return None
    return {"out": out, "partials": part}


def digests(shape, form, in_bn, expo=None):
    res = launch(shape, form, in_bn, make_inputs(shape, expo))
    return "refused" if res is None else {k: sha(v) for k, v in res.items()}


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    import _hip as h
    rec = {}
    for shape, form, in_bn, expo in cases():
        rec[case_key(shape, form, in_bn, expo)] = digests(shape, form, in_bn, expo)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    n_ref = sum(1 for v in rec.values() if v == "refused")
    print(f"{len(rec)} cases ({n_ref} refused by the entry point) from {h.LIB_PATH} -> {path}")


if __name__ == "__main__":
    main()
