"""conv_h2_kernel with straight-line stages and the epilogue options as template parameters (csrc/conv_h2.hip, h2_epilogue in
csrc/lad_b3_tile.h): the same bits as the build before the change.

For every shape, every form of launch (bias + partials; + a plain addend; a gated addend in place; the BatchNorm sums with the
mask from x; the sums from sign bits with a gated addend), each with and without the input BatchNorm, `out` and `partials` are
compared by SHA-256 with digests recorded from the parent commit's library (tests/golden/conv_h2_parent.json, written by
tools/conv_h2_digests.py, which also holds the cases, the seeded inputs and the launches).  A combination lad_conv_h2 refuses
(the sums together with an input BatchNorm, sign bits at 32 channels) was recorded as "refused" and must still be refused.

Shapes: the 128-row kernel at one pixel, with tiles crossing image boundaries, at the widest image and at 32 channels; and the
smallest launches that take the 256-row kernel.  Exponent cases: inputs x 1e-25 against weights x 1e-20 with a bias of the
outputs' size (subnormal outputs, accumulator exponents beyond 126); an image whose second 32 channels are x 1e12, one where they
are x 1e-12 (re-basing up to the +8 cap and far down) and one with an all-zero first stage."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import conv_h2_digests as rec  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(rec.GOLDEN) as f:
        return json.load(f)


def test_every_case_has_a_recorded_digest(golden):
    keys = [rec.case_key(*c) for c in rec.cases()]
    assert len(set(keys)) == len(keys) and set(keys) == set(golden)
    # the refusals are the argument checks of lad_conv_h2, nothing else
    for (shape, form, in_bn, expo), k in zip(rec.cases(), keys):
        refused = (form.startswith("stat") and in_bn) or (shape[0] == 32 and form in ("gated_inplace", "stat_bits_gated"))
        assert (golden[k] == "refused") == refused, k


@pytest.mark.parametrize("shape,form,in_bn,expo", rec.cases(), ids=[rec.case_key(*c) for c in rec.cases()])
def test_conv_h2_gives_the_bits_of_the_parent_build(shape, form, in_bn, expo, golden):
    got = rec.digests(shape, form, in_bn, expo)
    print(rec.case_key(shape, form, in_bn, expo), got)
    assert got == golden[rec.case_key(shape, form, in_bn, expo)]


def test_the_outputs_are_not_trivial():
    """What the digests cover: finite, non-zero outputs and sums (the tiny case: subnormal outputs that are not all flushed)."""
    import torch
    for shape, expo in (((64, 3, 13, 6), None), ((64, 3, 13, 6), "tiny"), ((64, 4, 25, 11), "range")):
        res = rec.launch(shape, "bias_partials", False, rec.make_inputs(shape, expo))
        out, part = res["out"], res["partials"]
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(part).all())
        assert float(out.abs().max()) > 0
        if expo == "tiny":
            assert 0 < float(out.abs().max()) < 1.2e-38        # below the smallest normal float
        else:
            assert float(part.abs().max()) > 0
