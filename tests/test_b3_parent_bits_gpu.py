"""The bf16 x 3 kernels after their dead template axes and duplicated code were removed (csrc/conv_b3.hip, csrc/wgrad_mfma.hip,
csrc/lad_b3_tile.h): the same bits as the build before the change.

The kernels' instruction streams are held by profiles/split_family_isa.log; this file holds what that log cannot see -- the host
launch code (grid, LDS size, the attribute call, the slab reduction behind the weight gradients).  For every case of
tools/b3_digests.py (which holds the cases, the seeded inputs and the launches) the outputs are compared by SHA-256 with digests
recorded from the parent commit's library (tests/golden/b3_parent.json).  Convolutions: lad_conv_b3c_fwd_f32 (with and without
an addend) and lad_conv_b3c_fwd_f32_bnrelu at 64 and 32 channels, lad_conv_b3_fwd_f32_gated in place, lad_conv_b3_dgrad_bnstat
with and without bn_bits, lad_conv_b3c_dgrad_bnstat, lad_conv_s2b3_fwd and lad_conv_s2b3_dgrad with and without the BatchNorm
sums -- at one pixel, with tiles crossing image boundaries (the smallest launch with two 256-row tiles), at the widest image and
at 32 channels.  Weight gradients: lad_conv_wgrad_b3c at 64 and 32 channels with and without in_coef, at the shapes of
tests/test_wgrad_h2_window_gpu.py (several tiles per workgroup, and workgroups without a tile that must write a zero slab).  A
combination an entry point refuses was recorded as "refused" and must still be refused."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import b3_digests as rec  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(rec.GOLDEN) as f:
        return json.load(f)


def test_every_case_has_a_recorded_digest(golden):
    keys = [rec.conv_key(*c) for c in rec.conv_cases()] + [rec.wgrad_key(*c) for c in rec.wgrad_cases()]
    assert len(set(keys)) == len(keys) and set(keys) == set(golden)
    # the refusals are the argument checks of the entry points, nothing else
    for shape, form in rec.conv_cases():
        refused = form.startswith("s2_") and (shape[2] < 2 or shape[3] < 2)
        assert (golden[rec.conv_key(shape, form)] == "refused") == refused, (shape, form)
    for C, shape, in_bn in rec.wgrad_cases():
        refused = C == 32 and 64 + 2 * (shape[2] + 2) > 128     # a 64-row tile and its halo do not fit the 128-row window
        assert (golden[rec.wgrad_key(C, shape, in_bn)] == "refused") == refused, (C, shape)


@pytest.mark.parametrize("shape,form", rec.conv_cases(), ids=[rec.conv_key(*c) for c in rec.conv_cases()])
def test_conv_b3_gives_the_bits_of_the_parent_build(shape, form, golden):
    got = rec.conv_digests(shape, form)
    print(rec.conv_key(shape, form), got)
    assert got == golden[rec.conv_key(shape, form)]


@pytest.mark.parametrize("C,shape,in_bn", rec.wgrad_cases(), ids=[rec.wgrad_key(*c) for c in rec.wgrad_cases()])
def test_wgrad_b3_gives_the_bits_of_the_parent_build(C, shape, in_bn, golden):
    got = rec.wgrad_digests(C, shape, in_bn)
    print(rec.wgrad_key(C, shape, in_bn), got)
    assert got == golden[rec.wgrad_key(C, shape, in_bn)]


def test_the_outputs_are_not_trivial():
    """What the digests cover: finite, non-zero outputs and sums that replaced what the buffers were filled with."""
    import torch
    shape = (64, 3, 13, 6)
    t = rec.make_conv_inputs(shape)
    for form in ("fwd", "bnrelu", "gated_inplace", "dgrad_stat_bits_gated", "s2_fwd", "s2_dgrad_stat"):
        for name, v in rec.launch_conv(shape, form, t).items():
            assert bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0, (form, name)
            if name.startswith("partials"):
                assert not bool((v == -7.0).any() | (v == 9.0).any() | (v == 7.0).any()), (form, name)   # every sum was written
    for C in (64, 32):
        for in_bn in (False, True):
            res = rec.launch_wgrad(C, (3, 13, 6), in_bn, rec.make_wgrad_inputs(C, (3, 13, 6)))
            for name, v in res.items():
                assert bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0 and not bool((v == 5.0).any()), (C, in_bn, name)
