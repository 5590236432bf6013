"""GPU tests of the zero-phase low-pass (csrc/lowpass.hip; lowpass.lowpass_device; laugh_segmenter.lowpass_device;
segment_laughter.py --lowpass; evaluate_sweep.py --lowpass).

The reference is scipy on the host (the reference's own calls, tests/_lowpass_model.reference).  The error bar is derived from
the filter, not from the kernel (tests/_lowpass_model.tol): 64 ulps of max(1, max|x|) amplified by 1 / (1 - r)^2, r the pole
radius -- 4.4e-11 at cutoff 0.01, 4.3e-9 at 0.001; float32 arithmetic would sit six orders above it.  The largest
err / tol is printed by each test (run with -s).  The decisions behind the filter
(run tables, scores, TextGrids, CSV files) are compared for equality."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _lowpass_model as lm
import _score_model as sm
from oracle import recipe

pytestmark = pytest.mark.gpu

THRESHOLDS = [float(t) for t in lm.SWEEP_THRESHOLDS]
MIN_LENGTHS = lm.SWEEP_MIN_LENGTHS
M = "Bmr001"
GUARD = 4096 + 64


def _seg():
    import _hip
    return int(_hip.lib().lad_lowpass_tile_frames())


def _dev(x, cutoff=0.01, lengths=None):
    import lowpass
    got = lowpass.lowpass_device(torch.from_numpy(np.ascontiguousarray(x)).cuda(), cutoff=cutoff, lengths=lengths)
    assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == x.shape
    return got.cpu().numpy()


def _ratio(got, x, cutoff):
    """max |got - scipy| over the bar, for one channel."""
    import lowpass
    _, a = lowpass.butter2(cutoff)
    return float(np.max(np.abs(got - lm.reference(np.asarray(x, np.float64), cutoff)))) / lm.tol(x, a)


@pytest.fixture(scope="module")
def filtered_tracks():
    """The three plateau tracks of the decision tests and their host-filtered form, computed once."""
    tracks = [lm.make_track(seed, 4000) for seed in (1, 2, 3)]
    return tracks, [lm.reference(t, 0.01) for t in tracks]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_lengths_around_lane_segments_and_wave_tiles(dtype):
    L = _seg()
    lengths = lm.gpu_lengths(L)
    assert len(lengths) >= 12 and min(lengths) == 10
    worst = 0.0
    for T in lengths:
        x = lm.make_track(T, max(T, 64))[:T].astype(dtype)
        r = _ratio(_dev(x), x, 0.01)
        worst = max(worst, r)
        assert r <= 1.0, (T, r)
    print(f"{np.dtype(dtype).name}, cutoff 0.01, {len(lengths)} lengths up to {max(lengths)}: largest err / tol = {worst:.3g}")


@pytest.mark.parametrize("cutoff", [0.001, 0.05, 0.2])
def test_other_cutoffs(cutoff):
    T = 64 * _seg() + 3
    x = lm.make_track(T, T)
    r = _ratio(_dev(x, cutoff), x, cutoff)
    print(f"cutoff {cutoff}, {T} frames: err / tol = {r:.3g}")
    assert r <= 1.0


def test_channels_of_different_lengths():
    L = _seg()
    T = 64 * L + 40
    lengths = [T, 10, 2 * L + 5]
    rng = np.random.default_rng(5)
    x = np.full((3, T), np.nan)
    for c, n in enumerate(lengths):
        x[c, :n] = rng.uniform(-0.3, 1.3, n)
    for dtype in (np.float64, np.float32):
        xd = x.astype(dtype)
        got = _dev(xd, lengths=lengths)
        for c, n in enumerate(lengths):
            r = _ratio(got[c, :n], xd[c, :n], 0.01)
            print(f"{np.dtype(dtype).name} channel {c}, {n} of {T} frames: err / tol = {r:.3g}")
            assert r <= 1.0, (c, r)
            assert np.isnan(got[c, n:]).all(), c
    # without lengths every channel is as long as the row
    full = rng.uniform(-0.3, 1.3, (3, T))
    got = _dev(full)
    for c in range(3):
        assert _ratio(got[c], full[c], 0.01) <= 1.0, c
    # a (T,) tensor is one channel
    assert np.array_equal(_dev(full[1]), got[1])


def test_guards_input_untouched_and_identical_bytes():
    import lowpass
    L = _seg()
    T = 64 * L + 40
    lengths = [T, 10, 2 * L + 5]
    rng = np.random.default_rng(6)
    x = np.full((3, T), np.nan)
    for c, n in enumerate(lengths):
        x[c, :n] = rng.uniform(-0.3, 1.3, n)
    p = torch.from_numpy(x).cuda()
    before = p.clone()
    b, a = lowpass.butter2(0.01)
    big = torch.full((GUARD + 3 * T + GUARD,), -7.0, dtype=torch.float64, device="cuda")
    out = big[GUARD:GUARD + 3 * T].view(3, T)
    got = lowpass.filtfilt_device(p, b, a, lengths=lengths, out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    assert bool((big[:GUARD] == -7.0).all()) and bool((big[GUARD + 3 * T:] == -7.0).all())
    assert torch.equal(p.view(torch.int64), before.view(torch.int64))               # (bit patterns: NaN != NaN)
    first = out.clone()
    for c, n in enumerate(lengths):
        assert _ratio(first[c, :n].cpu().numpy(), x[c, :n], 0.01) <= 1.0
    out.fill_(-7.0)
    lowpass.filtfilt_device(p, b, a, lengths=lengths, out=out)
    assert torch.equal(out.view(torch.int64), first.view(torch.int64))
    again = lowpass.lowpass_device(p, lengths=lengths)
    assert torch.equal(again.view(torch.int64), first.view(torch.int64))


def test_a_nan_poisons_its_own_channel_only():
    L = _seg()
    T = 5 * L + 7
    rng = np.random.default_rng(7)
    x = rng.uniform(-0.3, 1.3, (3, T))
    x[1, 2 * L + 3] = np.nan
    assert np.isnan(lm.reference(x[1], 0.01)).all()                                  # scipy: the whole channel
    got = _dev(x)
    assert np.isnan(got[1]).all()
    for c in (0, 2):
        assert _ratio(got[c], x[c], 0.01) <= 1.0, c


def _raw(p, out, lengths, b, a, zi, dtype=1):
    """lad_lowpass through the C ABI with a workspace between two guard bands; returns its code."""
    import _hip
    lib = _hip.lib()
    C, T = p.shape
    f64p = ctypes.POINTER(ctypes.c_double)
    n = lib.lad_lowpass_workspace_bytes(C, T)
    assert n > 0
    ws_big = torch.full((GUARD + n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    ws = ws_big[GUARD:GUARD + n]
    arrs = [np.ascontiguousarray(v, np.float64) for v in (b, a, zi)]
    lens = None if lengths is None else np.ascontiguousarray(lengths, np.int64)
    lptr = None if lens is None else lens.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    rc = lib.lad_lowpass(_hip.ptr(p), dtype, C, T, lptr, *[v.ctypes.data_as(f64p) for v in arrs], _hip.ptr(out), _hip.ptr(ws),
                         _hip.stream_handle())
    torch.cuda.synchronize()
    assert bool((ws_big[:GUARD] == 0xA5).all()) and bool((ws_big[GUARD + n:] == 0xA5).all())
    return rc


def test_refusals_write_nothing_and_leave_the_path_usable():
    import _hip
    import lowpass
    lib = _hip.lib()
    b, a = lowpass.butter2(0.01)
    zi = lowpass.zi2(b, a)
    T = 300
    x = np.random.default_rng(8).uniform(0, 1, (2, T))
    p = torch.from_numpy(x).cuda()

    def fresh():
        return torch.full((2, T), -7.0, dtype=torch.float64, device="cuda")
    cases = [("a length of 9", dict(lengths=[T, 9]), b"lengths[1] = 9"),
             ("a length beyond the row", dict(lengths=[T + 1, T]), b"lengths[0]"),
             ("a[0] = 2", dict(a=[2.0, a[1], a[2]]), b"a[0]"),
             ("a NaN coefficient", dict(b=[b[0], float("nan"), b[2]]), b"non-finite")]
    for name, change, message in cases:
        kw = dict(lengths=None, b=b, a=a, zi=zi)
        kw.update(change)
        out = fresh()
        rc = _raw(p, out, **kw)
        assert rc == _hip.LAD_ERR_INVALID and message in lib.lad_last_error(), (name, lib.lad_last_error())
        assert bool((out == -7.0).all()), name
    # out aliasing probs: refused, and the input keeps its values
    rc = _raw(p, p, None, b, a, zi)
    assert rc == _hip.LAD_ERR_INVALID and b"overlaps probs" in lib.lad_last_error()
    assert np.array_equal(p.cpu().numpy(), x)
    # a 9-frame row cannot even be sized
    assert lib.lad_lowpass_workspace_bytes(1, 9) == -1
    # the same buffers, a good call
    out = fresh()
    assert _raw(p, out, [T, 10], b, a, zi) == 0
    got = out.cpu().numpy()
    assert _ratio(got[0], x[0], 0.01) <= 1.0 and _ratio(got[1, :10], x[1, :10], 0.01) <= 1.0 and np.isnan(got[1, 10:]).all()
    # the Python surface
    for bad in (p.to(torch.float16), (p * 10).to(torch.int32), torch.rand(2, 600, device="cuda")[:, ::2], p.view(2, 3, 100)):
        with pytest.raises(_hip.LadHipError):
            lowpass.lowpass_device(bad)
    with pytest.raises(ValueError, match="padlen"):
        lowpass.lowpass_device(p[:, :9].contiguous())
    with pytest.raises(ValueError, match="padlen"):
        lowpass.lowpass_device(p, lengths=[T, 9])
    with pytest.raises(_hip.LadHipError, match="lengths"):
        lowpass.lowpass_device(p, lengths=[T, T + 1])


def _margin(filtered):
    return float(np.min(np.abs(np.asarray(filtered)[:, None] - np.asarray(THRESHOLDS)[None, :])))


@pytest.mark.parametrize("k", [0, 1, 2])
def test_decisions_behind_the_filter(filtered_tracks, k):
    """The instances cut from the device-filtered track are the host's: the same dictionary, keys, order and floats."""
    import laugh_segmenter as ls
    x, ref = filtered_tracks[0][k], filtered_tracks[1][k]
    margin = _margin(ref)
    print(f"seed {k + 1}: nearest frame to a threshold {margin:.2e}, {int((ref <= 0).sum())} frames <= 0")
    assert margin > 1e-7                                       # no decision hangs on the last digits of either filter
    assert (ref <= 0).sum() > 100                              # fix_over_underflow has work to do
    want = ls.get_laughter_instances(ls.lowpass(x), THRESHOLDS, MIN_LENGTHS, 100.)
    got = ls.get_laughter_instances_device(ls.lowpass_device(torch.from_numpy(x).cuda()), THRESHOLDS, MIN_LENGTHS, 100.)
    assert list(got.items()) == list(want.items())
    assert sum(len(v) for v in want.values()) > 50


def test_scores_behind_the_filter(filtered_tracks):
    import laugh_segmenter as ls
    import sweep_eval as se
    lengths = [4000, 3100, 2500]
    tracks = [t[:n] for t, n in zip(filtered_tracks[0], lengths)]
    host_filtered = [ls.lowpass(t) for t in tracks]
    for f in host_filtered:
        assert _margin(f) > 1e-7
    parts = ["fe001", "me002", "mn003"]
    rows = sm.make_rows(71, M, parts, 40.0, n_per_type=40, max_len_s=1.5)
    chans = [{"meeting_id": M, "part_id": p, "chan": f"chan{i}", "length": 40.0} for i, p in enumerate(parts)]
    index = se.TranscriptIndex(rows, chans)
    channels = [(M, f"chan{i}") for i in range(3)]
    padded = np.full((3, max(lengths)), np.nan)
    for c, t in enumerate(tracks):
        padded[c, :len(t)] = t
    want = se.score_sweep_host(host_filtered, channels, THRESHOLDS, MIN_LENGTHS, 100.0, index)
    got = se.score_sweep_device(torch.from_numpy(padded).cuda(), channels, THRESHOLDS, MIN_LENGTHS, 100.0, index, lowpass=0.01,
                                lengths=lengths)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert (want.sum(axis=(1, 2)) > 0).all()                   # every channel and every field scored something
    # without the filter the scores are others: the switch does something
    raw = se.score_sweep_device(torch.from_numpy(padded).cuda(), channels, THRESHOLDS, MIN_LENGTHS, 100.0, index)
    assert not np.array_equal(raw, want)
    with pytest.raises(ValueError):
        se.score_sweep_device(torch.from_numpy(padded).cuda(), channels, THRESHOLDS, MIN_LENGTHS, 100.0, index, lengths=lengths)


def _write_wav(path, x):
    from scipy.io import wavfile
    wavfile.write(path, 16000, (np.clip(x, -1, 1) * 32767).astype(np.int16))


def _checkpoint(tmp_path, seed=101):
    import contextlib
    import io

    import config
    import torch_utils
    cfg = config.MODEL_MAP["resnet_base"]
    with contextlib.redirect_stdout(io.StringIO()):
        m = cfg["model"](dropout_rate=0.0, linear_layer_size=cfg["linear_layer_size"], filter_sizes=cfg["filter_sizes"])
    full = m.state_dict()
    for k, v in recipe.make_state(seed).items():
        full[k] = torch.from_numpy(v.copy())
    m.load_state_dict(full)
    ck = tmp_path / "ckpt"
    with contextlib.redirect_stdout(io.StringIO()):
        torch_utils.save_checkpoint(torch_utils.make_state_dict(m, None, 0, 0, 1.0), True, str(ck))
    return str(ck)


def _tree(root):
    out = {}
    for dirpath, dirs, files in os.walk(root):
        dirs.sort()
        for f in sorted(files):
            path = os.path.join(dirpath, f)
            out[os.path.relpath(path, root)] = open(path, "rb").read()
    return out


def _threshold_in_a_gap(values, quantile):
    """The midpoint of the gap of at least 1e-6 between consecutive sorted values that is nearest to the quantile."""
    v = np.sort(np.asarray(values, np.float64))
    at = int(quantile * (len(v) - 1))
    order = sorted(range(len(v) - 1), key=lambda i: abs(i - at))
    i = next(i for i in order if v[i + 1] - v[i] >= 1e-6)
    return float((v[i] + v[i + 1]) / 2), float(v[i + 1] - v[i])


def test_segment_laughter_with_lowpass(tmp_path, capsys):
    import audio_utils
    import laugh_segmenter as ls
    import segment_laughter
    import textgrid
    ck = _checkpoint(tmp_path)
    wav = tmp_path / "chan.wav"
    _write_wav(wav, recipe.make_clips(24, 1, n_samples=16000 * 6)[0])
    base = ["--model_path", ck, "--config", "resnet_base", "--min_lengths", "0,0.1", "--input_audio_file", str(wav), "--precision", "fp16"]
    # a first run for the raw track the thresholds are picked from
    raw_npy = tmp_path / "raw.npy"
    segment_laughter.main(base + ["--output_dir", str(tmp_path / "first"), "--save_probs", str(raw_npy)])
    raw = np.load(raw_npy)
    assert raw.ndim == 1 and raw.size > 100
    filtered = lm.reference(raw, 0.01)
    picked = [_threshold_in_a_gap(filtered, q) for q in (1 / 3, 2 / 3)]
    thresholds = [t for t, _ in picked]
    for t, gap in picked:
        assert gap >= 1e-6 and 0.0 < t < 1.0 and float(np.min(np.abs(filtered - t))) >= 5e-7
    assert thresholds[0] < thresholds[1]
    trees = {}
    for seg in ("device", "host"):
        npy = tmp_path / f"{seg}.npy"
        segment_laughter.main(base + ["--thresholds", ",".join(repr(t) for t in thresholds), "--output_dir", str(tmp_path / seg),
                                      "--lowpass", "0.01", "--segmenter", seg, "--save_probs", str(npy)])
        assert "4-setting sweep" in capsys.readouterr().out
        assert np.array_equal(np.load(npy), raw)                                     # --save_probs keeps writing the raw track
        trees[seg] = _tree(tmp_path / seg)
    assert len(trees["host"]) == 4 and trees["host"] == trees["device"]
    # both are the instances of the host-filtered track
    length = audio_utils.get_audio_length(str(wav))
    want = ls.get_laughter_instances(filtered, thresholds, [0.0, 0.1], fps=len(raw) / float(length))
    assert sum(len(v) for v in want.values()) > 0
    for (thr, min_l), instances in want.items():
        path = tmp_path / "want.TextGrid"
        textgrid.write_laughter_textgrid(str(path), instances, xmax=length)
        assert trees["host"][os.path.join(f"t_{thr}", f"l_{min_l}", "chan.TextGrid")] == open(path, "rb").read(), (thr, min_l)


def test_evaluate_sweep_with_lowpass(tmp_path, capsys):
    import evaluate_sweep
    args = sm.write_corpus(tmp_path)
    out = {}
    for scorer in ("host", "device"):
        evaluate_sweep.main(args + ["--lowpass", "0.01", "--scorer", scorer, "--out_dir", str(tmp_path / scorer)])
        assert f"({scorer} scorer)" in capsys.readouterr().out
        out[scorer] = {f: open(tmp_path / scorer / f, "rb").read() for f in sorted(os.listdir(tmp_path / scorer))}
    assert list(out["host"]) == ["eval_df_per_meeting.csv", "sum_stats.csv"]
    assert out["host"] == out["device"]
    evaluate_sweep.main(args + ["--scorer", "device", "--out_dir", str(tmp_path / "plain")])
    assert open(tmp_path / "plain" / "eval_df_per_meeting.csv", "rb").read() != out["host"]["eval_df_per_meeting.csv"]
