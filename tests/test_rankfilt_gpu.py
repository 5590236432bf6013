"""GPU tests of the median / rank filter (csrc/rankfilt.hip; rankfilt.rank_filter_device / median_filter_device;
laugh_segmenter.median_filter_device; sweep_eval.score_sweep_device / score_surface_device with median=; segment_laughter.py
--median; evaluate_sweep.py --median).

The model is tests/_rankfilt_model.py, the header's convention as a loop over frames.  The filter selects one of its inputs, so
every comparison is np.array_equal (value equality; -0.0 == 0.0): no tolerance appears anywhere.  The decisions behind the
filter (instances, scores, TextGrids, CSV files) are compared for equality as well."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _rankfilt_model as rm
import _score_model as sm
from oracle import recipe

pytestmark = pytest.mark.gpu

M = "Bmr001"
GUARD = 4096 + 64
THRESHOLDS = [0.2, 0.35, 0.5, 0.65, 0.8]
MIN_LENGTHS = [0.0, 0.1, 0.2]


def _tile():
    import _hip
    return int(_hip.lib().lad_rank_filter_tile_frames())


def _dev(x, window, rank, lengths=None):
    import rankfilt
    got = rankfilt.rank_filter_device(torch.from_numpy(np.ascontiguousarray(x)).cuda(), window, rank, lengths=lengths)
    assert got.is_cuda and tuple(got.shape) == x.shape and got.dtype == torch.from_numpy(x).dtype
    return got.cpu().numpy()


def _lengths(window):
    tile, h = _tile(), (window - 1) // 2
    return sorted({T for T in (1, 2, h, h + 1, tile - 1, tile, tile + 1, 2 * tile + 3) if T >= 1})


@pytest.mark.parametrize("window", [1, 3, 51, 1023])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_equal_to_the_model(dtype, window):
    """Every T of the list (T <= h and T around a tile edge with window = 1023 among them) on a random and an fp16-rounded track,
    every kind of track at the two largest T; minimum, median, maximum and window // 3."""
    lengths = _lengths(window)
    n = 0
    for T in lengths:
        kinds = ["random", "fp16"] + (["tied", "constant", "ramp"] if T >= lengths[-2] else [])
        for kind in kinds:
            x = rm.track(kind, T, dtype, seed=window)
            for rank in rm.ranks(window):
                got = _dev(x, window, rank)
                assert np.array_equal(got, rm.rank_filter(x, window, rank)), (T, kind, rank)
                n += 1
    print(f"{np.dtype(dtype).name}, window {window}: {n} calls at T in {lengths}")


def test_median_form_and_out_argument():
    import laugh_segmenter as ls
    import rankfilt
    x = rm.track("fp16", _tile() + 9, np.float32)
    p = torch.from_numpy(x).cuda()
    want = rm.median_filter(x, 51)
    assert np.array_equal(rankfilt.median_filter_device(p, 51).cpu().numpy(), want)
    assert np.array_equal(ls.median_filter_device(p, 51).cpu().numpy(), want)
    assert np.array_equal(ls.rank_filter_device(p, 51, 0).cpu().numpy(), rm.rank_filter(x, 51, 0))
    assert np.array_equal(ls.median_filter(x, 51), want)
    out = torch.empty_like(p)
    assert ls.median_filter_device(p, 51, out=out).data_ptr() == out.data_ptr() and np.array_equal(out.cpu().numpy(), want)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_channels_of_different_lengths(dtype):
    tile = _tile()
    T = 2 * tile + 3
    lengths = [tile + 7, 1, T]
    rng = np.random.default_rng(5)
    x = np.full((3, T), np.nan, dtype)
    for c, n in enumerate(lengths):
        x[c, :n] = rm.track("tied", n, dtype, seed=c)
    poisoned = x.copy()
    for c, n in enumerate(lengths):
        poisoned[c, n:] = rng.choice([1e30, -1e30, 0.5, np.inf], T - n)            # the pad may hold anything
    for window, rank in ((51, 25), (1023, 511), (1023, 0), (3, 2)):
        got = _dev(x, window, rank, lengths=lengths)
        got_poisoned = _dev(poisoned, window, rank, lengths=lengths)
        for c, n in enumerate(lengths):
            alone = _dev(np.ascontiguousarray(x[c, :n]), window, rank)
            assert np.array_equal(alone, rm.rank_filter(x[c, :n], window, rank)), (window, c)
            for g in (got, got_poisoned):
                assert np.array_equal(g[c, :n], alone), (window, c)
                assert np.isnan(g[c, n:]).all() and g[c, n:].size == T - n, (window, c)
    # without lengths every channel is as long as the row
    full = np.stack([rm.track("random", T, dtype, seed=c) for c in range(3)])
    got = _dev(full, 51, 25)
    for c in range(3):
        assert np.array_equal(got[c], rm.rank_filter(full[c], 51, 25)), c


def test_guards_input_untouched_and_identical_bytes():
    import rankfilt
    tile = _tile()
    T = 2 * tile + 3
    lengths = [tile + 7, 1, T]
    for dtype, bits in ((torch.float32, torch.int32), (torch.float64, torch.int64)):
        x = np.full((3, T), np.nan)
        for c, n in enumerate(lengths):
            x[c, :n] = rm.track("fp16", n, np.float64, seed=c)
        p = torch.from_numpy(x).to(dtype).cuda()
        before = p.clone()
        big = torch.full((GUARD + 3 * T + GUARD,), -7.0, dtype=dtype, device="cuda")
        out = big[GUARD:GUARD + 3 * T].view(3, T)
        got = rankfilt.median_filter_device(p, 1023, lengths=lengths, out=out)
        assert got.data_ptr() == out.data_ptr()
        torch.cuda.synchronize()
        assert bool((big[:GUARD] == -7.0).all()) and bool((big[GUARD + 3 * T:] == -7.0).all())
        assert torch.equal(p.view(bits), before.view(bits))                          # (bit patterns: NaN != NaN)
        first = out.clone()
        xs = p.cpu().numpy()
        for c, n in enumerate(lengths):
            assert np.array_equal(first[c, :n].cpu().numpy(), rm.median_filter(xs[c, :n], 1023)), c
        out.fill_(-7.0)
        rankfilt.median_filter_device(p, 1023, lengths=lengths, out=out)
        assert torch.equal(out.view(bits), first.view(bits))
        again = rankfilt.median_filter_device(p, 1023, lengths=lengths)
        assert torch.equal(again.view(bits), first.view(bits))


@pytest.mark.parametrize("window", [51, 1023])
def test_a_nan_touches_only_the_windows_that_hold_it(window):
    tile, h = _tile(), (window - 1) // 2
    T = 3 * tile + 7
    i = tile + 3
    for dtype in (np.float32, np.float64):
        x = np.stack([rm.track("random", T, dtype, seed=c) for c in range(3)])
        x[1, i] = np.nan
        for rank in (0, h, window - 1):
            got = _dev(x, window, rank)
            for c in (0, 2):
                assert np.array_equal(got[c], rm.rank_filter(x[c], window, rank)), c
            clean = np.ones(T, bool)
            clean[max(0, i - h):i + h + 1] = False
            want = rm.rank_filter(x[1], window, rank)                                # (its windows without the NaN are as ever)
            assert clean.sum() > 0 and not np.isnan(want[clean]).any()
            assert np.array_equal(got[1][clean], want[clean]), rank


def _raw(p, out, window, rank, lengths=None, dtype=None, C=None, T=None, ws="own"):
    """lad_rank_filter through the C ABI with a workspace between two guard bands; returns its code."""
    import _hip
    lib = _hip.lib()
    C = p.shape[0] if C is None else C
    T = p.shape[1] if T is None else T
    n = lib.lad_rank_filter_workspace_bytes(p.shape[0], p.shape[1], 3)
    assert n >= 0
    ws_big = torch.full((GUARD + n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    if isinstance(ws, str):
        ws = ws_big[GUARD:GUARD + n]
    lens = None if lengths is None else np.ascontiguousarray(lengths, np.int64)
    lptr = None if lens is None else lens.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    dtype = (0 if p.dtype == torch.float32 else 1) if dtype is None else dtype
    rc = lib.lad_rank_filter(_hip.ptr(p), dtype, C, T, lptr, window, rank, _hip.ptr(out), _hip.ptr(ws), _hip.stream_handle())
    torch.cuda.synchronize()
    assert bool((ws_big[:GUARD] == 0xA5).all()) and bool((ws_big[GUARD + n:] == 0xA5).all())
    return rc


def test_refusals_write_nothing_and_leave_the_path_usable():
    import _hip
    import rankfilt
    lib = _hip.lib()
    T = 300
    x = np.stack([rm.track("random", T, np.float64, seed=c) for c in range(2)])
    p = torch.from_numpy(x).cuda()

    def fresh():
        return torch.full((2, T), -7.0, dtype=torch.float64, device="cuda")
    cases = [("no channel", dict(C=0), b"channels"),
             ("too many channels", dict(C=65536), b"channels"),
             ("no frame", dict(T=0), b"frames"),
             ("too many frames", dict(T=(1 << 30) + 1), b"frames"),
             ("window 0", dict(window=0), b"window"),
             ("an even window", dict(window=50), b"window"),
             ("window 1025", dict(window=1025), b"window"),
             ("a negative window", dict(window=-3), b"window"),
             ("rank -1", dict(rank=-1), b"rank"),
             ("rank = window", dict(rank=51), b"rank"),
             ("a length of 0", dict(lengths=[T, 0]), b"lengths[1] = 0"),
             ("a length beyond the row", dict(lengths=[T + 1, T]), b"lengths[0]"),
             ("dtype 2", dict(dtype=2), b"dtype"),
             ("dtype -1", dict(dtype=-1), b"dtype"),
             ("no workspace", dict(ws=None), b"null")]
    for name, change, message in cases:
        kw = dict(window=51, rank=25)
        kw.update(change)
        out = fresh()
        rc = _raw(p, out, **kw)
        assert rc == _hip.LAD_ERR_INVALID and message in lib.lad_last_error(), (name, lib.lad_last_error())
        assert bool((out == -7.0).all()), name
    out = fresh()
    for name, args in (("no probs", (None, out)), ("no out", (p, None))):
        n = lib.lad_rank_filter_workspace_bytes(2, T, 51)
        ws = torch.empty(n, dtype=torch.uint8, device="cuda")
        rc = lib.lad_rank_filter(_hip.ptr(args[0]), 1, 2, T, None, 51, 25, _hip.ptr(args[1]), _hip.ptr(ws), _hip.stream_handle())
        assert rc == _hip.LAD_ERR_INVALID and b"null" in lib.lad_last_error(), name
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    # out aliasing probs, wholly or by one element: refused, and the input keeps its values
    both = torch.cat([p.reshape(-1), p.reshape(-1)])
    for name, o in (("the same", both[:2 * T]), ("its last element", both[2 * T - 1:4 * T - 1])):
        rc = _raw(both[:2 * T].view(2, T), o, 51, 25)
        assert rc == _hip.LAD_ERR_INVALID and b"overlaps probs" in lib.lad_last_error(), name
    assert np.array_equal(both.cpu().numpy(), np.concatenate([x.reshape(-1)] * 2))
    # out inside the workspace
    ws = torch.full((2 * T * 8 + 512,), 0xA5, dtype=torch.uint8, device="cuda")
    rc = _raw(p, ws[8:8 + 2 * T * 8].view(torch.float64).view(2, T), 51, 25, ws=ws)
    assert rc == _hip.LAD_ERR_INVALID and b"overlaps the workspace" in lib.lad_last_error()
    assert bool((ws == 0xA5).all())
    # the same buffers, a good call
    out = fresh()
    assert _raw(p, out, 51, 25, lengths=[T, 10]) == 0
    got = out.cpu().numpy()
    assert np.array_equal(got[0], rm.median_filter(x[0], 51)) and np.array_equal(got[1, :10], rm.median_filter(x[1, :10], 51))
    assert np.isnan(got[1, 10:]).all()
    # the Python surface
    for bad in (p.to(torch.float16), (p * 10).to(torch.int32), torch.rand(2, 600, device="cuda")[:, ::2], p.view(2, 3, 100)):
        with pytest.raises(_hip.LadHipError):
            rankfilt.median_filter_device(bad, 51)
    for window in (0, 2, 50, 1025, -1):
        with pytest.raises(ValueError):
            rankfilt.median_filter_device(p, window)
    for rank in (-1, 51):
        with pytest.raises(ValueError):
            rankfilt.rank_filter_device(p, 51, rank)
    for lengths in ([T, 0], [T, T + 1], [T]):
        with pytest.raises(ValueError):
            rankfilt.median_filter_device(p, 51, lengths=lengths)
    with pytest.raises(_hip.LadHipError):
        rankfilt.median_filter_device(p, 51, out=torch.empty(2, T, device="cuda"))           # float32 for a float64 track
    assert np.array_equal(rankfilt.median_filter_device(p, 51).cpu().numpy()[1], rm.median_filter(x[1], 51))


@pytest.fixture(scope="module")
def tracks():
    """Three float32 plateau tracks of different lengths and their model-filtered form (window 51), computed once."""
    lengths = [4000, 3100, 2500]
    raw = [recipe.make_prob_track(seed, n).astype(np.float32) for seed, n in zip((1, 2, 3), lengths)]
    return raw, [rm.median_filter(t, 51) for t in raw]


def _padded(raw, dtype=np.float32):
    padded = np.full((len(raw), max(len(t) for t in raw)), np.nan, dtype)
    for c, t in enumerate(raw):
        padded[c, :len(t)] = t
    return torch.from_numpy(padded).cuda()


@pytest.mark.parametrize("k", [0, 1])
def test_decisions_behind_the_filter(tracks, k):
    """The instances cut from the device-filtered track are those cut from the host-filtered one: the same dictionary."""
    import laugh_segmenter as ls
    x, ref = tracks[0][k], tracks[1][k]
    host = ls.median_filter(x, 51)
    assert np.array_equal(host, ref)
    want = ls.get_laughter_instances(host, THRESHOLDS, MIN_LENGTHS, 100.)
    got = ls.get_laughter_instances_device(ls.median_filter_device(torch.from_numpy(x).cuda(), 51), THRESHOLDS, MIN_LENGTHS, 100.)
    assert list(got.items()) == list(want.items())
    assert sum(len(v) for v in want.values()) > 20
    assert list(ls.get_laughter_instances(x, THRESHOLDS, MIN_LENGTHS, 100.).items()) != list(want.items())      # the filter does something


def _index():
    import sweep_eval as se
    parts = ["fe001", "me002"]
    rows = sm.make_rows(71, M, parts, 40.0, n_per_type=40, max_len_s=1.5)
    chans = [{"meeting_id": M, "part_id": p, "chan": f"chan{i}", "length": 40.0} for i, p in enumerate(parts)]
    return se.TranscriptIndex(rows, chans), [(M, f"chan{i}") for i in range(2)]


@pytest.mark.parametrize("family", ["plain", "plain+events", "hysteresis+events", "viterbi"])
def test_sweep_scores_behind_the_filter(tracks, family):
    import laugh_segmenter as ls
    import sweep_eval as se
    raw = tracks[0][:2]
    lengths = [len(t) for t in raw]
    host_filtered = [ls.median_filter(t, 51) for t in raw]
    index, channels = _index()
    kw = {}
    if family.startswith("hysteresis"):
        kw.update(offset_drops=[0.0, 0.1], min_gaps=[0.0, 0.2])
    if family == "viterbi":
        kw.update(penalties=[0.0, 2.0])
    if family.endswith("events"):
        kw.update(events=(20, 50))
    thresholds = [0.35, 0.5, 0.65]
    want = se.score_sweep_host(host_filtered, channels, thresholds, MIN_LENGTHS, 100.0, index, **kw)
    got = se.score_sweep_device(_padded(raw), channels, thresholds, MIN_LENGTHS, 100.0, index, median=51, lengths=lengths, **kw)
    if "events" in kw:
        assert len(got) == 2 and np.array_equal(got[1], want[1]) and want[1][..., 1:].any()
        got, want = got[0], want[0]
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert (want.reshape(2, -1, 7).sum(axis=1) > 0).all()                            # every channel and every field scored something
    if family == "plain":
        # without the filter the scores are others: the switch does something
        plain = se.score_sweep_device(_padded(raw), channels, thresholds, MIN_LENGTHS, 100.0, index)
        assert not np.array_equal(plain, want)
        # float64 tracks, and no lengths on rows of one length
        same = [t[:2500].astype(np.float64) for t in raw]
        got = se.score_sweep_device(_padded(same, np.float64), channels, thresholds, MIN_LENGTHS, 100.0, index, median=51)
        assert np.array_equal(got, se.score_sweep_host([ls.median_filter(t, 51) for t in same], channels, thresholds, MIN_LENGTHS, 100.0, index))
        for score in (se.score_sweep_device, se.score_surface_device):
            with pytest.raises(ValueError, match="lowpass and median"):
                score(_padded(raw), channels, thresholds, MIN_LENGTHS, 100.0, index, lowpass=0.01, median=51, lengths=lengths)
        with pytest.raises(ValueError):
            se.score_sweep_device(_padded(raw), channels, thresholds, MIN_LENGTHS, 100.0, index, median=50, lengths=lengths)


@pytest.mark.parametrize("events", [None, (20, 50)])
def test_surface_scores_behind_the_filter(tracks, events):
    import laugh_segmenter as ls
    import sweep_eval as se
    raw = tracks[0][:2]
    lengths = [len(t) for t in raw]
    host_filtered = [ls.median_filter(t, 51) for t in raw]
    index, channels = _index()
    levels = [i / 20 for i in range(21)]
    kw = {} if events is None else dict(events=events)
    want = se.score_sweep_host(host_filtered, channels, levels, MIN_LENGTHS, 100.0, index, **kw)
    got = se.score_surface_device(_padded(raw), channels, levels, MIN_LENGTHS, 100.0, index, median=51, lengths=lengths, **kw)
    if events is not None:
        assert len(got) == 2 and np.array_equal(got[1], want[1]) and want[1][..., 1:].any()
        got, want = got[0], want[0]
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert (want.reshape(2, -1, 7).sum(axis=1) > 0).all()


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


def test_segment_laughter_with_median(tmp_path, capsys):
    import audio_utils
    import laugh_segmenter as ls
    import segment_laughter
    import textgrid
    ck = _checkpoint(tmp_path)
    wav = tmp_path / "chan.wav"
    _write_wav(wav, recipe.make_clips(24, 1, n_samples=16000 * 6)[0])
    base = ["--model_path", ck, "--config", "resnet_base", "--min_lengths", "0,0.1", "--input_audio_file", str(wav), "--precision", "fp16"]
    # a first run for the raw track the thresholds are picked from: values of the filtered track itself, where > is strict
    raw_npy = tmp_path / "raw.npy"
    segment_laughter.main(base + ["--output_dir", str(tmp_path / "first"), "--save_probs", str(raw_npy)])
    raw = np.load(raw_npy)
    assert raw.ndim == 1 and raw.size > 100 and raw.dtype == np.float32
    filtered = rm.median_filter(raw, 51)
    thresholds = [float(np.sort(filtered)[int(q * (len(filtered) - 1))]) for q in (1 / 3, 2 / 3)]
    assert 0.0 < thresholds[0] < thresholds[1] < 1.0
    flags = ["--thresholds", ",".join(repr(t) for t in thresholds)]
    trees = {}
    for seg in ("device", "host"):
        for name, more in ((seg, ["--median", "51"]), (seg + " plain", [])):
            npy = tmp_path / f"{name}.npy"
            segment_laughter.main(base + flags + more + ["--output_dir", str(tmp_path / name), "--segmenter", seg, "--save_probs", str(npy)])
            assert "4-setting sweep" in capsys.readouterr().out
            assert np.array_equal(np.load(npy), raw)                                 # --save_probs keeps writing the raw track
            trees[name] = _tree(tmp_path / name)
    assert len(trees["host"]) == 4 and trees["host"] == trees["device"]
    assert len(trees["host plain"]) == 4 and trees["host plain"] == trees["device plain"] and trees["host plain"] != trees["host"]
    # they are the instances of the filtered track, and without the flag those of the raw one
    length = audio_utils.get_audio_length(str(wav))
    for name, track in (("host", filtered), ("host plain", raw)):
        want = ls.get_laughter_instances(track, thresholds, [0.0, 0.1], fps=len(raw) / float(length))
        assert sum(len(v) for v in want.values()) > 0
        for (thr, min_l), instances in want.items():
            path = tmp_path / "want.TextGrid"
            textgrid.write_laughter_textgrid(str(path), instances, xmax=length)
            assert trees[name][os.path.join(f"t_{thr}", f"l_{min_l}", "chan.TextGrid")] == open(path, "rb").read(), (name, thr, min_l)


def _files(d):
    return {f: open(d / f, "rb").read() for f in sorted(os.listdir(d))}


@pytest.mark.parametrize("more", [[], ["--offset_drops", "0,0.1", "--min_gaps", "0.2"], ["--penalties", "1.0"], ["--events"],
                                  ["--threshold_grid", "20"], ["--event_grid", "20"]], ids=lambda m: (m or ["plain"])[0].lstrip("-"))
def test_evaluate_sweep_with_median(tmp_path, capsys, more):
    import evaluate_sweep
    args = sm.write_corpus(tmp_path)
    if "grid" in "".join(more):
        at = args.index("--thresholds")
        args = args[:at] + args[at + 2:]
    out = {}
    for scorer in ("host", "device"):
        evaluate_sweep.main(args + more + ["--median", "51", "--scorer", scorer, "--out_dir", str(tmp_path / scorer)])
        assert f"({scorer} scorer)" in capsys.readouterr().out
        out[scorer] = _files(tmp_path / scorer)
    assert out["host"] == out["device"] and len(out["host"]) >= 2
    # the files are those of tracks filtered beforehand, with the same columns as without the flag
    evaluate_sweep.main(args + more + ["--scorer", "device", "--out_dir", str(tmp_path / "plain")])
    plain = _files(tmp_path / "plain")
    assert list(plain) == list(out["host"]) and plain["eval_df_per_meeting.csv"] != out["host"]["eval_df_per_meeting.csv"]
    assert [v.split(b"\n")[0] for v in plain.values()] == [v.split(b"\n")[0] for v in out["host"].values()]
    if not more:
        evaluate_sweep.main(args + ["--scorer", "host", "--out_dir", str(tmp_path / "plain host")])
        assert _files(tmp_path / "plain host") == plain and list(plain) == ["eval_df_per_meeting.csv", "sum_stats.csv"]
        for m in os.listdir(tmp_path / "probs"):
            for f in os.listdir(tmp_path / "probs" / m):
                np.save(tmp_path / "probs" / m / f, rm.median_filter(np.load(tmp_path / "probs" / m / f), 51))
        evaluate_sweep.main(args + ["--scorer", "device", "--out_dir", str(tmp_path / "before")])
        assert _files(tmp_path / "before") == out["host"]
