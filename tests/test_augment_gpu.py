"""GPU tests of the train-time augmentation (csrc/augment.hip) against the numpy model of the convention (tests/_augment_model.py),
stage by stage, then all stages together and train.py end to end.

Shapes: (T, F) = (100, 44), (128, 44) and (11, 4) with W = 5 (the smallest legal warp, one float4 per row); batches of 1, 3, 64 and
257; counts 0, 1, T - 1 and T; a segment that runs past its channel's end; a noise channel of exactly T frames.  The model's
results are computed once per (geometry, configuration) for the 257 segments and shared: a batch of B is their first B."""
import csv
import functools
import os

import numpy as np
import pytest
import torch

import _augment_model as am

pytestmark = pytest.mark.gpu

GEOMETRIES = ((100, 44), (128, 44), (11, 4))
BATCHES = (1, 3, 64, 257)
PAD = -23.025850929940457
SEED = 0x1234567890
U24 = 2.0 ** -24


def _mask_widths(T, F):
    return min(20, T), min(8, F)


@functools.lru_cache(maxsize=None)
def _data(T, F):
    """Channels of 3 T + 50, 10 T, exactly T and T - 1 frames (the last too short to be noise) and the 257 segments."""
    rng = np.random.default_rng(1000 * T + F)
    lengths = (3 * T + 50, 10 * T, T, T - 1)
    mats = [(3.0 * rng.standard_normal((n, F)) - 6.0).astype(np.float32) for n in lengths]
    n = max(BATCHES)
    chan = (np.arange(n) % 4).astype(np.int32)
    count = np.array([(T, T - 1, 1, 0)[(i // 4) % 4] for i in range(n)], np.int32)
    first = np.array([rng.integers(0, max(1, lengths[c] - T + 1)) for c in chan], np.int64)
    first[0], count[0] = 0, T                       # whole, from the channel's start
    first[1], count[1] = lengths[1] - T // 2, T     # runs past its channel's end
    first[2], count[2] = 0, T                       # the channel of exactly T frames, whole
    first[3], count[3] = 0, T                       # asks for one frame more than the channel has
    return mats, chan, first, count


@functools.lru_cache(maxsize=None)
def _store(T, F):
    import datasets
    store = datasets.FeatureStore()
    for i, m in enumerate(_data(T, F)[0]):
        store.add_features(f"c{i}", m)
    return store


NOISE = (0, 1, 2)   # every channel with at least T frames


def _run(T, F, cfg, B, epoch=0, noise=None, sel=None):
    """The kernel on the first B segments (or on segments `sel`) -> float32 (B, T, F)."""
    import datasets
    _, chan, first, count = _data(T, F)
    sel = np.arange(B) if sel is None else np.asarray(sel)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a[sel])).cuda()
    out = datasets.gather_segments_augmented(_store(T, F), dev(chan), dev(first), dev(count), T, PAD, cfg, epoch, noise)
    return out.cpu().numpy()


def _plain(T, F, B):
    import datasets
    _, chan, first, count = _data(T, F)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a[:B])).cuda()
    return datasets.gather_segments(_store(T, F), dev(chan), dev(first), dev(count), T, PAD).cpu().numpy()


def _cfg(kind, T, F, **kw):
    import augment
    Wt, Wf = _mask_widths(T, F)
    fields = {"masks": dict(p=0.9, n_time=2, Wt=Wt, n_freq=2, Wf=Wf),
              "warp": dict(p=0.9, W=5),
              "mix": dict(mix_p=0.5, snr_lo=5.0, snr_hi=20.0, gain_lo=-6.0, gain_hi=6.0),
              "mix_nogain": dict(mix_p=0.5, snr_lo=5.0, snr_hi=20.0),
              "gain": dict(gain_lo=-6.0, gain_hi=6.0),
              "all": dict(p=0.9, W=5, n_time=2, Wt=Wt, n_freq=2, Wf=Wf, mix_p=0.5, snr_lo=5.0, snr_hi=20.0, gain_lo=-6.0, gain_hi=6.0)}[kind]
    return augment.AugmentConfig(seed=SEED, **{**fields, **kw})


@functools.lru_cache(maxsize=None)
def _model(T, F, kind, epoch=0):
    """The numpy model on all 257 segments of the geometry (computed once, read only)."""
    mats, chan, first, count = _data(T, F)
    cfg = _cfg(kind, T, F)
    noise = NOISE if cfg.mixes else None
    return [am.augment_segment(cfg, epoch, mats, int(chan[b]), int(first[b]), int(count[b]), T, PAD, noise) for b in range(len(chan))]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _mix_bound(T, F, ref):
    """2 T F 2^-24 for two any-order fp32 sums of positive terms + 8 ulps (2^-23 relative) for expf, logf, the powers and the
    division; in ln units, |ref| >= 1 scales the second term."""
    return 2.0 * T * F * U24 + 8.0 * 2.0 ** -23 * np.maximum(1.0, np.abs(ref))


def test_the_plain_gather_is_the_reference_of_these_tests():
    for T, F in GEOMETRIES:
        mats, chan, first, count = _data(T, F)
        got = _plain(T, F, 257)
        for b in range(257):
            assert np.array_equal(_bits(got[b]), _bits(am.gather(mats, chan[b], first[b], count[b], T, PAD))), (T, F, b)


@pytest.mark.parametrize("T, F", GEOMETRIES)
@pytest.mark.parametrize("B", BATCHES)
def test_off_is_off(T, F, B):
    import augment
    plain = _bits(_plain(T, F, B))
    Wt, Wf = _mask_widths(T, F)
    off = augment.AugmentConfig(seed=SEED, p=0.0, mix_p=0.0, W=5, n_time=2, Wt=Wt, n_freq=2, Wf=Wf, snr_lo=5.0, snr_hi=20.0)
    assert np.array_equal(_bits(_run(T, F, off, B)), plain)
    assert np.array_equal(_bits(_run(T, F, off, B, noise=NOISE, epoch=3)), plain)
    assert np.array_equal(_bits(_run(T, F, augment.AugmentConfig(seed=SEED, p=1.0), B)), plain)   # the gate passes, no stage is configured


def test_dataset_without_augmentation_is_the_plain_gather():
    import datasets
    import segments
    T, F = 100, 44
    mats, chan, first, count = _data(T, F)
    store = _store(T, F)
    table = segments.SegmentTable(chan.copy(), first.copy(), count.copy(), (np.arange(257) % 2).astype(np.int32), list(store.keys), T)
    ds = datasets.LadDataset(store, table)
    assert ds.augment is None and ds.noise is None
    idx = [5, 0, 256, 17, 1]
    batch = ds[idx]
    assert np.array_equal(_bits(batch["inputs"].cpu().numpy()), _bits(_plain(T, F, 257)[idx]))
    assert batch["input_lens"].tolist() == count[idx].tolist() and batch["is_laugh"].tolist() == [1, 0, 0, 1, 1]
    # ... and with augmentation the same dataset serves the kernel's batch for its epoch
    cfg = _cfg("all", T, F)
    aug = datasets.LadDataset(store, table, augment=cfg, noise="self")
    assert aug.noise.frames == [350, 1000, 100]
    aug.set_epoch(2)
    assert np.array_equal(_bits(aug[idx]["inputs"].cpu().numpy()), _bits(_run(T, F, cfg, None, epoch=2, noise=NOISE, sel=idx)))
    with pytest.raises(ValueError):
        datasets.LadDataset(store, table, augment=cfg)                    # mixes, no noise
    with pytest.raises(ValueError):
        datasets.LadDataset(store, table, augment=cfg, noise=["c3"])      # 99 frames
    with pytest.raises(ValueError):
        datasets.gather_segments_augmented(store, torch.zeros(1, dtype=torch.int32).cuda(), torch.full((1,), 2 ** 32).cuda(),
                                           torch.zeros(1, dtype=torch.int32).cuda(), T, PAD, _cfg("masks", T, F), 0, None)


@pytest.mark.parametrize("T, F", GEOMETRIES)
@pytest.mark.parametrize("B", BATCHES)
def test_masks_only(T, F, B):
    got, plain, ref = _run(T, F, _cfg("masks", T, F), B), _plain(T, F, B), _model(T, F, "masks")
    n_filled = 0
    for b in range(B):
        r = ref[b]
        filled = r["filled"]
        assert np.array_equal(_bits(got[b])[~filled], _bits(plain[b])[~filled]), b          # unfilled: the plain gather's bits
        if filled.any():
            v = got[b][filled]
            assert np.all(_bits(v) == _bits(v[:1])), b                                      # one fill value ...
            bound = T * F * U24 * float(np.abs(plain[b]).max())
            assert abs(float(v[0]) - r["mean"]) <= bound, (b, float(v[0]), r["mean"], bound)  # ... the mean, to the any-order fp32 bound
            n_filled += 1
    assert B < 64 or n_filled > B // 2


@pytest.mark.parametrize("T, F", GEOMETRIES)
@pytest.mark.parametrize("B", BATCHES)
def test_warp_only(T, F, B):
    got, plain, ref = _run(T, F, _cfg("warp", T, F), B), _plain(T, F, B), _model(T, F, "warp")
    n_warped = 0
    worst = 0.0
    for b in range(B):
        rows = ref[b]["warp"]
        if rows is None:
            assert np.array_equal(_bits(got[b]), _bits(plain[b])), b
            continue
        n_warped += 1
        for t, (i0, i1, rem, den) in enumerate(rows):
            if rem == 0:
                assert np.array_equal(_bits(got[b][t]), _bits(plain[b][i0])), (b, t)
            else:
                ulp = np.spacing(np.maximum(np.abs(plain[b][i0]), np.abs(plain[b][i1])).astype(np.float32)).astype(np.float64)
                err = np.abs(got[b][t].astype(np.float64) - ref[b]["x"][t])
                worst = max(worst, float((err / ulp).max()))
                assert np.all(err <= 2.0 * ulp), (b, t, float((err / ulp).max()))
    print(f"warp {T}x{F} B={B}: {n_warped} warped segments, largest error {worst:.3f} ulp of max(|x[i0]|, |x[i1]|) (bound 2)")
    assert B < 64 or n_warped > B // 2


@pytest.mark.parametrize("kind", ("mix", "mix_nogain", "gain"))
@pytest.mark.parametrize("T, F", GEOMETRIES)
@pytest.mark.parametrize("B", BATCHES)
def test_mix_and_gain(T, F, B, kind):
    cfg = _cfg(kind, T, F)
    got, plain, ref = _run(T, F, cfg, B, noise=NOISE if cfg.mixes else None), _plain(T, F, B), _model(T, F, kind)
    worst, n_mixed = 0.0, 0
    for b in range(B):
        if not ref[b]["mixed"]:
            assert np.array_equal(_bits(got[b]), _bits(plain[b])), b      # the stage is skipped: copies
            continue
        n_mixed += 1
        err = np.abs(got[b].astype(np.float64) - ref[b]["x"])
        bound = _mix_bound(T, F, ref[b]["x"])
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), (b, float((err / bound).max()))
    print(f"{kind} {T}x{F} B={B}: {n_mixed} segments through the stage, largest err / bound = {worst:.3f} "
          f"(bound {2.0 * T * F * U24 + 8.0 * 2.0 ** -23:.2e} ln units at |ref| <= 1)")
    if kind == "mix_nogain":
        assert B < 64 or 0 < n_mixed < B
        used = {ref[b]["draws"]["noise_chan"] for b in range(B) if ref[b]["mixed"]}
        assert B < 64 or used == set(NOISE)                               # the channel of exactly T frames included
    else:
        assert n_mixed == B


@pytest.mark.parametrize("T, F", GEOMETRIES)
def test_all_stages(T, F):
    cfg = _cfg("all", T, F)
    a = _run(T, F, cfg, 64, epoch=1, noise=NOISE)
    assert np.array_equal(_bits(a), _bits(_run(T, F, cfg, 64, epoch=1, noise=NOISE)))       # same (seed, epoch): same bits
    other = _run(T, F, cfg, 64, epoch=2, noise=NOISE)
    assert not np.array_equal(_bits(a), _bits(other))                                       # another epoch: another batch
    assert np.array_equal(_bits(_run(T, F, cfg, 257, epoch=1, noise=NOISE)[:64]), _bits(a))  # whatever the batch size
    # a segment's result does not depend on where it stands: alone, first of 64, last of 64
    b = 37
    alone = _run(T, F, cfg, None, epoch=1, noise=NOISE, sel=[b])
    front = _run(T, F, cfg, None, epoch=1, noise=NOISE, sel=[b] + [i for i in range(64) if i != b])
    back = _run(T, F, cfg, None, epoch=1, noise=NOISE, sel=[i for i in range(64) if i != b] + [b])
    assert np.array_equal(_bits(alone[0]), _bits(a[b])) and np.array_equal(_bits(front[0]), _bits(a[b]))
    assert np.array_equal(_bits(back[63]), _bits(a[b]))
    # the stages compose in the convention's order.  Bound: the mix bound on every value that enters the warp (a convex
    # combination: it does not amplify) + 2 ulp for the warp + the any-order fp32 bound T F 2^-24 max|x| for the fill value
    ref = _model(T, F, "all", epoch=1)
    for s in range(64):
        x = ref[s]["x"]
        big = float(np.abs(ref[s]["before_masks"]).max())
        bound = float(_mix_bound(T, F, big)) + 2.0 * float(np.spacing(np.float32(big))) + T * F * U24 * big
        err = np.abs(a[s].astype(np.float64) - x)
        assert np.all(err <= bound), (s, float(err.max()), bound)


def test_more_segments_than_workgroups():
    """Past 16384 segments a workgroup takes more than one: every copy of a segment still gets the same bits."""
    T, F = 11, 4
    cfg = _cfg("all", T, F)
    n = 16384 + 5
    sel = np.arange(n) % 64
    got = _run(T, F, cfg, None, noise=NOISE, sel=sel)
    assert np.array_equal(_bits(got), _bits(_run(T, F, cfg, 64, noise=NOISE))[sel])


def _write_wav(path, x):
    from scipy.io import wavfile
    wavfile.write(path, 16000, (np.clip(x, -1, 1) * 32767).astype(np.int16))


def test_train_script_with_augmentation(tmp_path, capsys, monkeypatch):
    """train.py --augment spec+mix --noise self on synthetic clips: finite losses, the training batches are augmented, the dev loader's
    are bit-equal to those of a loader built without augmentation."""
    import load_data
    import synth
    import train
    root = tmp_path / "data"
    (root / "data_dfs").mkdir(parents=True)
    (root / "m1").mkdir()
    clips = synth.make_clips(3, n_samples=16000 * 12, seed=77).cpu().numpy()
    for i in range(3):
        _write_wav(root / "m1" / f"chan{i}.wav", clips[i])
    rng = np.random.default_rng(0)
    for split, n, chans in (("train", 64, (0, 1)), ("dev", 16, (2,))):
        with open(root / "data_dfs" / f"{split}_df.csv", "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["start", "duration", "sub_start", "sub_duration", "audio_path", "meeting_id", "chan_id", "label"])
            for i in range(n):
                s = round(float(rng.uniform(0, 10.5)), 2)
                c = chans[i % len(chans)]
                w.writerow([s, 1.0, s, 1.0, f"m1/chan{c}.wav", "m1", f"chan{c}", int(rng.random() < 0.5)])
    made = []
    orig = load_data.create_training_dataloader

    def spy(*a, **kw):
        made.append(orig(*a, **kw))
        return made[-1]
    monkeypatch.setattr(load_data, "create_training_dataloader", spy)
    ck = tmp_path / "ck"
    train.main(["--config", "resnet_base", "--checkpoint_dir", str(ck), "--data_root", str(root), "--batch_size", "16",
                "--log_frequency", "1", "--max_steps", "3", "--augment", "spec+mix", "--noise", "self", "--seed", "5"])
    monkeypatch.undo()
    assert "Augmentation: spec+mix (seed 5, 2 noise channels)" in capsys.readouterr().out
    rows = list(csv.reader(open(ck / "metrics.csv")))
    losses = [float(r[5]) for r in rows[1:]] + [float(r[9]) for r in rows[1:]]
    assert len(rows) == 4 and all(np.isfinite(losses))
    dev, trn = made
    assert dev.dataset.augment is None and trn.dataset.augment is not None and trn.dataset.augment.seed == 5
    assert sorted(trn.dataset.store.keys[i] for i in trn.dataset.noise.index.tolist()) == ["m1/chan0.wav", "m1/chan1.wav"]
    data_dir = str(root / "data_dfs")
    plain_dev = orig(data_dir, "dev", shuffle=True, seed=5, batch_size=16, audio_root=str(root))
    n = 0
    for x, y in zip(dev, plain_dev):
        assert torch.equal(x["inputs"], y["inputs"]) and torch.equal(x["is_laugh"], y["is_laugh"])
        n += 1
    assert n == 1
    plain_trn = orig(data_dir, "train", batch_size=16, audio_root=str(root), store=plain_dev.dataset.store)
    assert any(not torch.equal(x["inputs"], y["inputs"]) for x, y in zip(trn, plain_trn))
