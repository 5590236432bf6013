"""Host side of the train-time augmentation (no GPU): the numpy model of the convention (tests/_augment_model.py) against
Philox's known answers and the ranges the convention promises, the configuration's refusals, the presets and train.py's flags."""
import ctypes
import math

import numpy as np
import pytest

import _augment_model as am

SEEDS = (1234, 2024, 0x1234567890)
GEOMETRIES = ((100, 44, 5, 20, 8), (128, 44, 8, 25, 10))   # T, F, W, Wt, Wf
N_SEG = 4096


@pytest.mark.parametrize("counter, key, want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    """Random123's kat_vectors for philox4x32-10."""
    assert " ".join(f"{w:08x}" for w in am.philox4x32_10(counter, key)) == want


def test_unit_and_mulhi():
    assert am.unit(0) == 0.0 and am.unit(0xffffffff) == np.float32(1.0 - 2.0 ** -24) and am.unit(0x100) == np.float32(2.0 ** -24)
    assert am.mulhi(0xffffffff, 7) == 6 and am.mulhi(0, 7) == 0 and am.mulhi(0x80000000, 7) == 3


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("T, F, W, Wt, Wf", GEOMETRIES)
def test_draw_ranges_and_coverage(seed, T, F, W, Wt, Wf):
    import augment
    cfg = augment.AugmentConfig(seed=seed, p=0.9, mix_p=0.5, snr_lo=5.0, snr_hi=20.0, gain_lo=-6.0, gain_hi=6.0, W=W, n_time=2, Wt=Wt,
                                n_freq=2, Wf=Wf)
    n_spec = n_mix = 0
    t_widths, f_widths, centres, shifts = set(), set(), set(), set()
    for i in range(N_SEG):
        d = am.draws(cfg, 0, i % 3, 100 * i, T, F, n_noise=3)
        n_spec += d["spec"]
        n_mix += d["mix_gate"]
        assert 5.0 <= d["snr_db"] <= 20.0 and -6.0 <= d["gain_db"] <= 6.0 and 0 <= d["noise_slot"] < 3
        assert W <= d["c"] <= T - W - 1 and -(W - 1) <= d["w"] <= W - 1 and 1 <= d["c2"] <= T - 2
        centres.add(d["c"])
        shifts.add(d["w"])
        assert len(d["time"]) == 2 and len(d["freq"]) == 2
        for start, width in d["time"]:
            assert 0 <= width <= Wt and 0 <= start and start + width <= T
            t_widths.add(width)
        for start, width in d["freq"]:
            assert 0 <= width <= Wf and 0 <= start and start + width <= F
            f_widths.add(width)
    assert t_widths == set(range(Wt + 1)) and f_widths == set(range(Wf + 1))
    assert centres == set(range(W, T - W)) and shifts == set(range(-(W - 1), W))
    for n, q in ((n_spec, 0.9), (n_mix, 0.5)):
        assert abs(n / N_SEG - q) <= 4.0 * math.sqrt(q * (1.0 - q) / N_SEG), (n / N_SEG, q)


def test_draws_depend_on_seed_epoch_channel_and_first_frame_only():
    import augment
    cfg = augment.from_preset("spec+mix", seed=7)
    base = am.draws(cfg, 3, 1, 4200, 100, 44, n_noise=5)
    assert base == am.draws(cfg, 3, 1, 4200, 100, 44, n_noise=5)
    assert base != am.draws(cfg, 4, 1, 4200, 100, 44, n_noise=5)
    assert base != am.draws(cfg, 3, 2, 4200, 100, 44, n_noise=5)
    assert base != am.draws(cfg, 3, 1, 4201, 100, 44, n_noise=5)
    assert base != am.draws(augment.from_preset("spec+mix", seed=8), 3, 1, 4200, 100, 44, n_noise=5)


def test_warp_rows_cover_both_halves():
    for T, c, c2 in ((100, 50, 46), (100, 5, 1), (100, 94, 98), (11, 5, 9), (11, 5, 1), (11, 5, 5)):
        rows = am.warp_rows(T, c, c2)
        assert rows[0][:1] == (0,) and rows[0][2] == 0 and rows[c2][0] == c and rows[c2][2] == 0
        assert all(0 <= i0 <= i1 <= T - 1 and 0 <= rem < den for i0, i1, rem, den in rows)
        assert all(i0 < c for i0, _, _, _ in rows[:c2]) and all(i0 >= c for i0, _, _, _ in rows[c2:])
        if c == c2:
            assert all(rem == 0 and i0 == t for t, (i0, _, rem, _) in enumerate(rows))


def test_config_refusals():
    import augment
    A = augment.AugmentConfig
    for bad in (dict(p=-0.1), dict(p=1.5), dict(mix_p=2.0), dict(mix_p=float("nan")), dict(snr_lo=3.0, snr_hi=2.0),
                dict(gain_lo=1.0, gain_hi=-1.0), dict(n_time=17), dict(n_freq=17), dict(W=-1), dict(Wt=-2), dict(seed=-1),
                dict(seed=2 ** 64), dict(W=2.5)):
        with pytest.raises(ValueError):
            A(**bad)
    spec = A(p=0.9, W=5, n_time=2, Wt=20, n_freq=2, Wf=8)
    spec.validate_for(100, 44)
    spec.validate_for(41, 8)
    for T, F in ((100, 42), (10, 44), (19, 44), (100, 4), (1000, 44)):   # F % 4, T <= 2 W, Wt > T, Wf > F, LDS
        with pytest.raises(ValueError):
            spec.validate_for(T, F)
    A(W=5).validate_for(11, 4)
    A().validate_for(464, 44)                                            # 163 632 of 163 840 bytes: the last T that fits at 44 filters
    with pytest.raises(ValueError):
        A().validate_for(465, 44)
    mix = A(mix_p=0.5, snr_lo=5.0, snr_hi=20.0)
    mix.validate_for(100, 44, [100, 5000])
    for frames in (None, [], [99, 5000]):
        with pytest.raises(ValueError):
            mix.validate_for(100, 44, frames)
    with pytest.raises(ValueError):
        spec.params(-1)
    with pytest.raises(ValueError):
        spec.params(2 ** 32)
    p = spec.params(7)
    assert (p.epoch, p.W, p.n_time, p.Wt, p.n_freq, p.Wf) == (7, 5, 2, 20, 2, 8) and p.p == np.float32(0.9)


def test_presets_are_data():
    import augment
    import config
    assert set(config.AUGMENT) == {"spec", "mix", "spec+mix"}
    assert config.AUGMENT["spec"] == dict(p=0.9, W=5, n_time=2, Wt=20, n_freq=2, Wf=8)
    assert config.AUGMENT["mix"] == dict(mix_p=0.5, snr_lo=5.0, snr_hi=20.0, gain_lo=-6.0, gain_hi=6.0)
    assert config.AUGMENT["spec+mix"] == {**config.AUGMENT["spec"], **config.AUGMENT["mix"]}
    assert augment.from_preset("none") is None and augment.from_preset(None) is None
    c = augment.from_preset("spec+mix", seed=5)
    assert c.seed == 5 and c.p == 0.9 and c.mix_p == 0.5 and c.mixes and not augment.from_preset("spec").mixes
    with pytest.raises(ValueError):
        augment.from_preset("specaugment")


def test_train_flags():
    import train
    base = ["--config", "resnet_base", "--checkpoint_dir", "ck", "--data_root", "d"]
    parser = train.make_parser()
    args = parser.parse_args(base)
    assert args.augment == "none" and args.augment_seed is None and args.noise is None
    assert train.augment_from_args(args) == (None, None)
    args = parser.parse_args(base + ["--augment", "spec+mix", "--noise", "self", "--seed", "11"])
    cfg, noise = train.augment_from_args(args)
    assert cfg.seed == 11 and cfg.mixes and cfg.p == 0.9 and noise == "self"
    cfg, noise = train.augment_from_args(parser.parse_args(base + ["--augment", "spec", "--augment_seed", "99", "--seed", "11"]))
    assert cfg.seed == 99 and not cfg.mixes and noise is None
    for bad in (["--augment", "mix"], ["--noise", "self"], ["--augment", "spec", "--augment_seed", "-3"]):
        with pytest.raises(ValueError):
            train.augment_from_args(parser.parse_args(base + bad))
    with pytest.raises(SystemExit):
        parser.parse_args(base + ["--augment", "everything"])


def test_c_abi_refuses_before_any_launch():
    """The host side of lad_gather_segments_aug: every refusal returns LAD_ERR_INVALID with a message, on a machine without a GPU
    (nothing is launched, no buffer is touched)."""
    import _hip
    lib = _hip.lib()
    buf = (ctypes.c_int64 * 8)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)

    def call(T=100, F=44, n_noise=0, min_noise=0, **kw):
        f = dict(seed=1, epoch=0, p=0.9, mix_p=0.5, snr_lo=5.0, snr_hi=20.0, gain_lo=-6.0, gain_hi=6.0, W=5, n_time=2, Wt=20, n_freq=2, Wf=8)
        f.update(kw)
        params = _hip.AugmentParams(**f)
        return lib.lad_gather_segments_aug(ptr, ptr, ptr, ptr, ptr, 0, T, F, 0.0, ctypes.byref(params), ptr if n_noise else None,
                                           n_noise, min_noise, ptr, None)

    assert call() == 0 and call(n_noise=3, min_noise=100) == 0 and call(T=11, F=4, Wt=11, Wf=4) == 0 and call(T=464) == 0   # (no segments: nothing to launch)
    for kw in (dict(F=42), dict(T=10), dict(Wt=101), dict(Wf=45), dict(n_time=17), dict(n_freq=17), dict(p=1.5), dict(p=-0.5),
               dict(mix_p=float("nan")), dict(snr_lo=21.0), dict(gain_hi=-7.0), dict(n_noise=3, min_noise=99), dict(T=465),
               dict(W=-1)):
        assert call(**kw) == _hip.LAD_ERR_INVALID, kw
        assert b"lad_gather_segments_aug" in lib.lad_last_error()
