"""The model of the fp16 base kernels (tests/_f16_model.py) tested on its own, without a GPU: the float64 reference is the
convolution torch computes in float64; an fp32 emulation of the kernel arithmetic stays inside the derived bound; emulations with a
defect of the kind the bound is there to catch (a product left out, a tap left out at the image's last row and column, the addend
applied behind the ReLU) leave it at more than half of the outputs they touch -- the condition on the power of the GPU tests that
use the same bound (tests/test_f16_ops_gpu.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _f16_model as fm

# (channels, std of the weights): the product's widths with weights of the size its layers have; n = 576 / 288 / 144 products
WIDTHS = [(64, 0.06), (32, 0.08), (16, 0.1)]
MUT_SHAPE = (6, 6, 5)


def draw(C, wstd, B, H, W, seed, cout=None, k=3):
    rng = np.random.default_rng([seed, C, B, H, W, k])
    cout = cout or C
    x = fm.half(rng.standard_normal((B, C, H, W)))
    w = fm.half(rng.standard_normal((cout, C, k, k)) * wstd)
    scale = ((rng.random(cout) + 0.5) * rng.choice([-1.0, 1.0], cout)).astype(np.float32)
    shift = (rng.standard_normal(cout) * 0.2).astype(np.float32)
    return rng, x, w, scale, shift


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("k", [3, 1])
@pytest.mark.parametrize("B,H,W", [(2, 7, 5), (1, 8, 6), (2, 7, 6), (1, 8, 5), (3, 1, 1), (1, 2, 1), (1, 13, 6)])
def test_the_float64_reference_is_torch_conv2d_in_float64(stride, k, B, H, W):
    rng = np.random.default_rng([stride, k, B, H, W])
    x, w = rng.standard_normal((B, 5, H, W)), rng.standard_normal((7, 5, k, k))
    got = fm.conv_sum(x, w, stride)
    ref = F.conv2d(torch.from_numpy(x), torch.from_numpy(w), stride=stride, padding=k // 2).numpy()
    assert got.shape == ref.shape == (B, 7, (H + stride - 1) // stride, (W + stride - 1) // stride)
    assert np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max()


def test_reference_and_bound_of_one_element_by_hand():
    """One output, two products: every term of the bound written out."""
    x = np.zeros((1, 16, 1, 1))
    w = np.zeros((1, 16, 1, 1))
    x[0, 0, 0, 0], x[0, 1, 0, 0], w[0, 0, 0, 0], w[0, 1, 0, 0] = 1.5, -2.0, 0.5, 0.25
    ref, bound = fm.conv_case(x, w, np.float32([-2.0]), np.float32([0.125]), addend=np.full((1, 1, 1, 1), 3.0), relu=True)
    S, A, u = 0.25, 1.25, 2.0 ** -23
    t = S * -2.0 + 0.125 + 3.0
    e32 = 16 * u * A * 2.0 + 2 * u * (0.5 + 0.125 + 3.0)
    assert ref.shape == (1, 1, 1, 1) and ref[0, 0, 0, 0] == t == 2.625
    assert bound[0, 0, 0, 0] == 2.0 ** -11 * (t + e32) + e32 + 2.0 ** -24
    ref0, _ = fm.conv_case(x, w, np.float32([-2.0]), np.float32([0.125]), addend=np.full((1, 1, 1, 1), -3.0), relu=True)
    assert ref0[0, 0, 0, 0] == 0.0


def test_tensors_in_give_the_same_reference_and_bound_as_numpy_in():
    """The GPU tests hand the model device tensors for their largest batches: the same loop, the same numbers, a tensor back."""
    rng, x, w, scale, shift = draw(16, 0.1, 2, 5, 4, 9)
    add = fm.half(rng.standard_normal(x.shape))
    ref, bound = fm.conv_case(x, w, scale, shift, add, True)
    tref, tbound = fm.conv_case(torch.from_numpy(x).half(), torch.from_numpy(w).float(), torch.from_numpy(scale), torch.from_numpy(shift),
                                torch.from_numpy(add), True)
    assert isinstance(ref, np.ndarray) and isinstance(tref, torch.Tensor) and tref.dtype == torch.float64
    assert np.array_equal(tref.numpy(), ref) and np.array_equal(tbound.numpy(), bound)
    with pytest.raises(AssertionError):
        fm.conv_case(x + 2.0 ** -13, w, scale, shift)          # not half values


def test_stem_images_and_pool_order():
    feat = np.arange(7 * 3, dtype=np.float32).reshape(7, 3) + 1
    img = fm.stem_images(feat, 3, 4, 3, 2, 5)
    assert np.array_equal(img[1, 0], np.stack([feat[2], feat[3], feat[4], np.zeros(3)]))      # frame 5 is behind the end of the file
    assert np.array_equal(img[2, 0, 0], feat[4]) and not img[2, 0, 1:].any()
    rng = np.random.default_rng(5)
    x = fm.half(rng.standard_normal((2, 3, 9, 14)))
    x[:, :, 8:], x[:, :, :, 12:] = 1000.0, 1000.0
    ref, bound = fm.pool_case(x)
    want = F.avg_pool2d(torch.from_numpy(x), 4).flatten(1).numpy()
    assert ref.shape == want.shape == (2, 3 * 2 * 3) and np.abs(ref - want).max() <= 1e-14
    assert bound.max() < 1e-5


def test_pack_image_layout_and_rounding():
    w = np.zeros((3, 16, 9), np.float32)
    w[2, 13, 4] = 1 + 2.0 ** -11          # a tie: to even, down
    w[1, 5, 0] = 1 + 3 * 2.0 ** -11       # a tie: to even, up
    w[0, 0, 8] = -0.0
    img = fm.pack_image(w)
    assert img.shape == (9, 1, 2, 32, 8) and img.dtype == np.float16
    assert float(img[4, 0, 1, 2, 5]) == 1.0 and float(img[0, 0, 0, 1, 5]) == 1 + 2.0 ** -9
    assert img.view(np.uint16)[8, 0, 0, 0, 0] == 0x8000
    assert np.count_nonzero(img.view(np.uint16)) == 3


def ratio(out, ref, bound):
    return np.abs(out - ref) / bound


@pytest.mark.parametrize("truncate", [False, True])
@pytest.mark.parametrize("C,wstd", WIDTHS)
def test_fp32_emulation_of_the_kernel_arithmetic_stays_inside_the_bound(C, wstd, truncate):
    """Sequential fp32 accumulation, rounding to nearest or truncating to 24 bits, every (addend, relu) form, stride 1 and the
    stride-2 forms: every element within the bound."""
    B, H, W = 2, 7, 6
    rng, x, w, scale, shift = draw(C, wstd, B, H, W, 1)
    add = fm.half(rng.standard_normal((B, C, H, W)))
    worst = 0.0
    for addend, relu in ((None, 0), (None, 1), (add, 1), (add, 0)):
        ref, bound = fm.conv_case(x, w, scale, shift, addend, relu)
        out, _ = fm.emulate_conv(x, w, scale, shift, addend, relu, truncate=truncate)
        r = ratio(out, ref, bound)
        assert r.max() <= 1.0, (addend is not None, relu, r.max())
        worst = max(worst, r.max())
    cout = {64: 32, 32: 16, 16: 16}[C]
    for k in (3, 1):
        _, x2, w2, sc2, sh2 = draw(C, wstd, B, H, W, 2, cout=cout, k=k)
        for relu in (0, 1):
            ref, bound = fm.conv_case(x2, w2, sc2, sh2, None, relu, stride=2)
            out, _ = fm.emulate_conv(x2, w2, sc2, sh2, None, relu, stride=2, truncate=truncate)
            assert ratio(out, ref, bound).max() <= 1.0, (k, relu)
    print(f"C = {C}, truncate = {truncate}: max err / bound = {worst:.3f}")


def flagged_share(out, ref, bound, affected):
    seen = affected & (ref != 0)
    assert seen.sum() >= 200, seen.sum()
    return float((np.abs(out - ref)[seen] > bound[seen]).mean())


@pytest.mark.parametrize("C,wstd", WIDTHS)
def test_a_dropped_product_is_flagged(C, wstd):
    B, H, W = MUT_SHAPE
    rng, x, w, scale, shift = draw(C, wstd, B, H, W, 3)
    add = fm.half(rng.standard_normal((B, C, H, W)))
    for addend, relu in ((None, 0), (add, 1)):
        ref, bound = fm.conv_case(x, w, scale, shift, addend, relu)
        out, affected = fm.emulate_conv(x, w, scale, shift, addend, relu, drop_product=4 * C + C // 3)   # a product of the centre tap
        share = flagged_share(out, ref, bound, affected)
        print(f"C = {C}, addend = {addend is not None}, relu = {relu}: one product dropped, flagged at {share:.3f}")
        assert share >= 0.5


@pytest.mark.parametrize("C,wstd", WIDTHS)
def test_a_tap_dropped_at_the_last_row_and_column_is_flagged(C, wstd):
    B, H, W = MUT_SHAPE
    rng, x, w, scale, shift = draw(C, wstd, B, H, W, 4)
    add = fm.half(rng.standard_normal((B, C, H, W)))
    ref, bound = fm.conv_case(x, w, scale, shift, add, 1)
    out, affected = fm.emulate_conv(x, w, scale, shift, add, 1, drop_tap_at_edge=0)      # tap (-1, -1): inside the image there
    assert not affected[:, :, :H - 1, :W - 1].any() and affected[:, :, H - 1, 1:].any() and affected[:, :, 1:, W - 1].any()
    good = ~affected
    assert (np.abs(out - ref)[good] <= bound[good]).all()
    share = flagged_share(out, ref, bound, affected)
    print(f"C = {C}: a tap dropped at the last row and column, flagged at {share:.3f}")
    assert share >= 0.5


@pytest.mark.parametrize("C,wstd", WIDTHS)
def test_the_addend_applied_behind_the_relu_is_flagged(C, wstd):
    B, H, W = MUT_SHAPE
    rng, x, w, scale, shift = draw(C, wstd, B, H, W, 5)
    add = fm.half(rng.standard_normal((B, C, H, W)))
    ref, bound = fm.conv_case(x, w, scale, shift, add, 1)
    out, affected = fm.emulate_conv(x, w, scale, shift, add, 1, addend_after_relu=True)
    good = ~affected
    assert (np.abs(out - ref)[good] <= bound[good]).all()
    share = flagged_share(out, ref, bound, affected)
    print(f"C = {C}: addend behind the ReLU, flagged at {share:.3f}")
    assert share >= 0.5
