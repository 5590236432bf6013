"""GPU tests of the sweep scorer (csrc/score.hip; sweep_eval.score_sweep_device; evaluate_sweep.py --scorer device).

Integer bookkeeping plus IEEE float64 division, multiplication and rint: every comparison is an equality -- against the host scorer
(sweep_eval.score_instances on laugh_segmenter.get_laughter_instances) and against the per-millisecond model of
tests/_score_model.py, which shares nothing with either."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _score_model as sm
from oracle import recipe

pytestmark = pytest.mark.gpu

EVAL_THRESHOLDS = [float(t) for t in np.concatenate((np.linspace(0, 0.9, 19).round(2), np.linspace(0.91, 1, 10).round(2)))]
EVAL_MIN_LENGTHS = [0.0, 0.1, 0.2]
F32_ROUNDS_UP = [0.05, 0.1, 0.15, 0.2, 0.3, 0.4, 0.55, 0.6, 0.8, 0.85, 0.91, 0.92, 0.93, 0.97, 0.98, 0.99]
AWKWARD_FPS = 360000 / 3600.0049375
M = "Bmr001"


def _corpus(seed, parts, duration, n_per_type, max_len_s, unmapped=()):
    import sweep_eval as se
    rows = sm.make_rows(seed, M, parts, duration, n_per_type=n_per_type, max_len_s=max_len_s)
    chans = [{"meeting_id": M, "part_id": p, "chan": f"chan{i}", "length": duration * 0.97} for i, p in enumerate(parts)]
    chans += [{"meeting_id": M, "part_id": None, "chan": c, "length": duration} for c in unmapped]
    return rows, chans, se.TranscriptIndex(rows, chans)


def _dev(tracks, channels, thresholds, min_lengths, fps, index, dtype=np.float32):
    """score_sweep_device of tracks of different lengths: NaN padding to the longest."""
    import sweep_eval as se
    T = max(len(t) for t in tracks)
    padded = np.full((len(tracks), T), np.nan, dtype)
    for c, t in enumerate(tracks):
        padded[c, :len(t)] = t
    got = se.score_sweep_device(torch.from_numpy(padded).cuda(), channels, thresholds, min_lengths, fps, index)
    assert got.dtype == np.int64 and got.shape == (len(tracks), len(thresholds), len(min_lengths), 7)
    return got


def _model_scores(model, track, chan, thresholds, min_lengths, fps):
    import laugh_segmenter as ls
    inst = ls.get_laughter_instances(track, thresholds, min_lengths, fps)
    return np.array([[model.score(inst[(t, l)], M, chan) for l in min_lengths] for t in thresholds], np.int64)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_full_size_track_and_the_87_settings(dtype):
    import sweep_eval as se
    rows, chans, index = _corpus(61, ["fe001"], 3600.0, 6000, 0.4)
    sets = index.scoring_sets(M, "chan0")
    assert all(len(s) > 1000 for s in sets), [len(s) for s in sets]
    ch = [(M, "chan0")]
    p = recipe.make_prob_track(5, 360000).astype(dtype)
    host = se.score_sweep_host([p], ch, EVAL_THRESHOLDS, EVAL_MIN_LENGTHS, 100.0, index)
    dev = _dev([p], ch, EVAL_THRESHOLDS, EVAL_MIN_LENGTHS, 100.0, index, dtype)
    assert np.array_equal(dev, host)
    assert (host[:, :, :, 0].reshape(-1) > 0).sum() > 40 and (host.sum(axis=(0, 1, 2)) > 0).all()        # every field at work
    # a (T,) tensor is one channel
    one = se.score_sweep_device(torch.from_numpy(p).cuda(), ch, [0.5], [0.2], 100.0, index)
    assert np.array_equal(one, host[:, [EVAL_THRESHOLDS.index(0.5)]][:, :, [2]])
    print(f"360,000 frames, 87 settings, {sum(len(s) for s in sets)} intervals: {int(host[0, :, :, 0].sum())} kept runs scored")


def test_against_the_set_model_directly():
    T = 36000
    for fps in (100.0, AWKWARD_FPS):
        duration = T / fps
        rows, chans, index = _corpus(62, ["fe001"], duration * 1.05, 300, duration / 200)
        model = sm.Model(rows, chans, sm.to_frames(duration * 1.2) + 10)
        p = recipe.make_prob_track(6, T)
        want = _model_scores(model, p, "chan0", EVAL_THRESHOLDS, EVAL_MIN_LENGTHS, fps)
        got = _dev([p], [(M, "chan0")], EVAL_THRESHOLDS, EVAL_MIN_LENGTHS, fps, index, np.float64)
        assert np.array_equal(got[0], want), fps
        assert (want.sum(axis=(0, 1)) > 0).all()


def test_ten_channels_in_one_call_and_identical_bytes():
    import sweep_eval as se
    parts = [f"me{i:03d}" for i in range(9)]
    rows, chans, index = _corpus(63, parts, 370.0, 200, 2.0, unmapped=("chanX",))
    rows = [r for r in rows if r["part_id"] != "me004"]                                # a participant without any row
    index = se.TranscriptIndex(rows, chans)
    channels = [(M, f"chan{i}") for i in range(9)] + [(M, "chanX")]
    lengths = [36000 + 17, 36000, 35999, 30000, 511, 512, 513, 20000, 1, 36000]
    tracks = [recipe.make_prob_track(40 + c, n) if n >= 100 else np.full(n, 0.9) for c, n in enumerate(lengths)]
    tracks[3] = np.full(lengths[3], np.nan)                                            # a channel without any run
    tracks[7][::2] = 0.0                                                               # a channel of single frames
    fps = [100.0, AWKWARD_FPS, 99.5, 100.0, 50.0, 2000.0, 100.0, 100.0, 100.0, 97.25]
    many = _dev(tracks, channels, EVAL_THRESHOLDS, EVAL_MIN_LENGTHS, fps, index)
    host = se.score_sweep_host([t.astype(np.float32) for t in tracks], channels, EVAL_THRESHOLDS, EVAL_MIN_LENGTHS, fps, index)
    assert np.array_equal(many, host)
    for c in range(10):
        one = _dev([tracks[c]], [channels[c]], EVAL_THRESHOLDS, EVAL_MIN_LENGTHS, fps[c], index)
        assert np.array_equal(one[0], many[c]), c
    assert not many[3].any() and not many[8].any() and many[0, :, :, 0].sum() > 1000
    assert many[9, :, :, 0].sum() > 1000 and not many[9, :, :, 3:].any()                # no participant: runs counted, no class hit
    assert np.array_equal(many[9, :, :, 0], many[9, :, :, 1])
    again = _dev(tracks, channels, EVAL_THRESHOLDS, EVAL_MIN_LENGTHS, fps, index)
    assert again.tobytes() == many.tobytes()


def test_tile_edges_single_frames_and_the_largest_k_and_l():
    import _hip
    import sweep_eval as se
    lib = _hip.lib()
    tile, kmax, lmax = int(lib.lad_runs_tile_frames()), int(lib.lad_runs_max_thresholds()), int(lib.lad_score_max_min_lengths())
    assert tile == 512 and lmax >= 8
    T = 3 * tile + 70
    edges = list(range(64, T, 64))
    below = np.full(T, 0.25)
    below[[0, T - 1] + [e - 1 for e in edges]] = 0.75                                   # single frames before every word / tile edge
    above = np.full(T, 0.25)
    above[[0, T - 1] + edges] = 0.75
    both = np.maximum(below, above)                                                    # two-frame runs across every edge
    holes = np.full(T, 0.75)
    holes[[0, T - 1] + edges] = 0.25
    long = np.full(T, 0.25)
    long[tile // 2:2 * tile + tile // 2 + 5] = 0.75                                    # one run through two whole tiles
    tracks = [below, above, both, holes, long]
    parts = [f"fe{i:03d}" for i in range(5)]
    rows, chans, index = _corpus(64, parts, T / 100.0 * 1.1, 40, 0.4)
    model = sm.Model(rows, chans, sm.to_frames(T / 100.0 * 1.3) + 10)
    channels = [(M, f"chan{i}") for i in range(5)]
    thresholds, min_lengths = [0.0, 0.5, 1.0], [-1.0, 0.0, 0.005, 0.1]
    got = _dev(tracks, channels, thresholds, min_lengths, 100.0, index, np.float64)
    assert np.array_equal(got, se.score_sweep_host(tracks, channels, thresholds, min_lengths, 100.0, index))
    for c, t in enumerate(tracks):
        assert np.array_equal(got[c], _model_scores(model, t, f"chan{c}", thresholds, min_lengths, 100.0)), c
    # single-frame runs: counted for a negative min_length only (0 > 0 is false)
    assert got[0, 1, :, 0].tolist() == [len(edges) + 2, 0, 0, 0] and got[1, 1, :, 0].tolist() == [len(edges) + 2, 0, 0, 0]
    assert got[2, 1, :, 0].tolist() == [len(edges) + 2, len(edges), len(edges), 0]      # two frames: 0.01 s (frames 0 and T - 1 alone)
    assert got[4, 1, :, 0].tolist() == [1, 1, 1, 1]
    assert got[:, 0, :, 0].tolist() == [[1, 1, 1, 1]] * 5 and not got[:, 2].any()       # threshold 0: one run; threshold 1: none
    # K and L at their maxima
    thresholds = [float(t) for t in np.linspace(0.0, 1.0, kmax)]
    min_lengths = [float(l) for l in np.linspace(-0.01, 0.3, lmax)]
    p = [recipe.make_prob_track(9, 36000), both]
    rows, chans, index = _corpus(65, ["fe001", "fe002"], 380.0, 300, 1.0)
    channels = [(M, "chan0"), (M, "chan1")]
    got = _dev(p, channels, thresholds, min_lengths, 100.0, index)
    assert np.array_equal(got, se.score_sweep_host([t.astype(np.float32) for t in p], channels, thresholds, min_lengths, 100.0, index))
    assert got[0, 1:-1, 0, 0].min() > 0


def test_awkward_fps_float32_thresholds_and_half_milliseconds():
    import sweep_eval as se
    T = 36000
    rows, chans, index = _corpus(66, ["fe001", "fe002"], 380.0, 300, 1.0)
    model = sm.Model(rows, chans, 420000)
    channels = [(M, "chan0"), (M, "chan1")]
    # probabilities equal to float32(t) and its neighbours, where float32 rounds t up: on iff the float64 value exceeds t
    p = recipe.make_prob_track(8, T).astype(np.float32)
    rng = np.random.default_rng(8)
    for t in F32_ROUNDS_UP:
        c = np.float32(t)
        at = rng.integers(0, T, 300)
        p[at] = np.array([np.nextafter(c, np.float32(-1)), c, np.nextafter(c, np.float32(2))], np.float32)[rng.integers(0, 3, 300)]
    q = recipe.make_prob_track(10, T).astype(np.float32)
    for fps in (AWKWARD_FPS, 2000.0):
        got = _dev([p, q], channels, EVAL_THRESHOLDS, EVAL_MIN_LENGTHS, fps, index)
        assert np.array_equal(got, se.score_sweep_host([p, q], channels, EVAL_THRESHOLDS, EVAL_MIN_LENGTHS, fps, index)), fps
    # fps = 2000: (f / 2000) * 1000 is exactly f / 2, every odd frame a half millisecond; frames 0..7 -> 0, 0, 1, 2, 2, 2, 3, 4 ms
    assert [round((f / 2000.0) * 1000.0) for f in range(8)] == [0, 0, 1, 2, 2, 2, 3, 4]
    rows = [{"meeting_id": M, "part_id": "fe001", "chan": "chan0", "start": 0.0, "end": 1.0, "length": 1.0, "type": "laugh",
             "laugh_type": "laugh"}]
    chans = [{"meeting_id": M, "part_id": "fe001", "chan": "chan0", "length": 1.0}]
    index, model = se.TranscriptIndex(rows, chans), sm.Model(rows, chans, 1200)
    for first, last, ms in ((1, 3, 2), (0, 1, 0), (1, 2, 1), (3, 5, 0), (5, 7, 2), (2, 7, 3), (1, 7, 4)):
        t = np.zeros(64)
        t[first:last + 1] = 0.9
        got = _dev([t], [(M, "chan0")], [0.5], [0.0], 2000.0, index, np.float64)[0, 0, 0]
        assert got.tolist() == [1, 1, ms, ms, 0, 0, 0], (first, last, got)
        assert tuple(got) == model.score([(first / 2000.0, last / 2000.0)], M, "chan0")
    # a long track at 2000 frames/s against the model (Python's round)
    t = recipe.make_prob_track(12, 4000)
    rows, chans, index = _corpus(67, ["fe001"], 2.2, 60, 0.05)
    model = sm.Model(rows, chans, 3000)
    got = _dev([t], [(M, "chan0")], EVAL_THRESHOLDS, [-1.0, 0.0, 0.001], 2000.0, index, np.float64)
    assert np.array_equal(got[0], _model_scores(model, t, "chan0", EVAL_THRESHOLDS, [-1.0, 0.0, 0.001], 2000.0))


def _raw_call(p, thresholds, min_lengths, fps, bounds, offsets, scores, L=None, n_intervals=None):
    """lad_runs_count + lad_runs_fill + lad_score_runs through the C ABI; returns the code of lad_score_runs."""
    import _hip
    lib = _hip.lib()
    C, T = p.shape
    K = len(thresholds)
    L = len(min_lengths) if L is None else L
    n = len(bounds) if n_intervals is None else n_intervals
    thr = (ctypes.c_double * K)(*thresholds)
    mls = (ctypes.c_double * max(len(min_lengths), L))(*min_lengths)
    fps_host = np.asarray(fps, np.float64)
    i32p, f64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    st = _hip.stream_handle()
    ws = torch.empty(lib.lad_runs_workspace_bytes(C, T, K), dtype=torch.uint8, device="cuda")
    sws = torch.empty(max(lib.lad_score_workspace_bytes(C, len(bounds), K, min(L, 8)), 256), dtype=torch.uint8, device="cuda")
    _hip.check(lib.lad_runs_count(_hip.ptr(p), 0, C, T, thr, K, _hip.ptr(ws), st), "lad_runs_count")
    counts = np.ascontiguousarray(ws[:4 * C * K].view(torch.int32).cpu().numpy())
    total = int(counts.sum())
    table = torch.empty((max(total, 1), 2), dtype=torch.int32, device="cuda")
    cptr = counts.ctypes.data_as(i32p)
    _hip.check(lib.lad_runs_fill(_hip.ptr(p), 0, C, T, thr, K, _hip.ptr(ws), cptr, _hip.ptr(table), total, st), "lad_runs_fill")
    b_host = np.ascontiguousarray(bounds, np.int32).reshape(-1, 2)
    o_host = np.ascontiguousarray(offsets, np.int32)
    b_dev = torch.from_numpy(b_host if len(b_host) else np.zeros((1, 2), np.int32)).cuda()
    o_dev, f_dev = torch.from_numpy(o_host).cuda(), torch.from_numpy(fps_host).cuda()
    rc = lib.lad_score_runs(_hip.ptr(ws), _hip.ptr(table), cptr, C, T, K, _hip.ptr(b_dev), _hip.ptr(o_dev), b_host.ctypes.data_as(i32p),
                            o_host.ctypes.data_as(i32p), n, _hip.ptr(f_dev), fps_host.ctypes.data_as(f64p), mls, L, _hip.ptr(sws),
                            _hip.ptr(scores), st)
    torch.cuda.synchronize()
    return rc


def test_errors_write_nothing_and_leave_the_path_usable():
    import _hip
    import sweep_eval as se
    lib = _hip.lib()
    lmax = int(lib.lad_score_max_min_lengths())
    p = torch.full((1, 1000), 0.9, device="cuda")
    good_b, good_o = [[100, 200], [300, 400], [0, 50]], [0, 0, 2, 3, 3, 3]
    guard = 16

    def fresh(L=1):
        return torch.full((L * 7 + guard,), -7, dtype=torch.int64, device="cuda")
    cases = [("unsorted", dict(bounds=[[300, 400], [100, 200], [0, 50]]), b"unsorted or overlaps"),
             ("overlapping", dict(bounds=[[100, 350], [300, 400], [0, 50]]), b"unsorted or overlaps"),
             ("empty interval", dict(bounds=[[100, 100], [300, 400], [0, 50]]), b"empty or negative"),
             ("descending offsets", dict(offsets=[0, 2, 1, 3, 3, 3]), b"do not ascend"),
             ("offsets short of n", dict(offsets=[0, 0, 2, 2, 2, 2]), b"index offsets run"),
             ("L above the maximum", dict(min_lengths=[0.0] * (lmax + 1)), b"min_lengths 1.."),
             ("millisecond overflow", dict(fps=[1e-4]), b"millisecond overflow"),
             ("fps 0", dict(fps=[0.0]), b"positive finite")]
    for name, change, message in cases:
        kw = dict(thresholds=[0.5], min_lengths=[0.2], fps=[100.0], bounds=good_b, offsets=good_o)
        kw.update(change)
        scores = fresh()
        rc = _raw_call(p, scores=scores, **kw)
        assert rc == _hip.LAD_ERR_INVALID and message in lib.lad_last_error(), (name, lib.lad_last_error())
        assert bool((scores == -7).all()), name                                         # nothing was written
    # the same buffers, a good call: seven values, the guard behind them untouched
    scores = fresh()
    assert _raw_call(p, [0.5], [0.2], [100.0], good_b, good_o, scores) == 0
    out = scores.cpu().numpy()
    assert out[:7].tolist() == [1, 1, 9990, 200, 50, 0, 0] and (out[7:] == -7).all()
    # the Python surface
    rows, chans, index = _corpus(68, ["fe001"], 12.0, 20, 0.5)
    ch = [(M, "chan0")]
    for bad in (p.cpu(), p.to(torch.float16), (p * 10).to(torch.int32), torch.rand(2, 2000, device="cuda")[:, ::2]):
        with pytest.raises((_hip.LadHipError, ValueError)):
            se.score_sweep_device(bad, ch, [0.5], [0.2], 100.0, index)
    with pytest.raises(_hip.LadHipError, match="min_lengths"):
        se.score_sweep_device(p, ch, [0.5], [0.1] * (lmax + 1), 100.0, index)
    with pytest.raises(_hip.LadHipError, match="thresholds"):
        se.score_sweep_device(p, ch, [0.5] * (int(lib.lad_runs_max_thresholds()) + 1), [0.2], 100.0, index)
    with pytest.raises(_hip.LadHipError, match="millisecond overflow"):
        se.score_sweep_device(p, ch, [0.5], [0.2], 1e-4, index)
    with pytest.raises(ValueError):
        se.score_sweep_device(p, ch + ch, [0.5], [0.2], 100.0, index)
    got = se.score_sweep_device(p, ch, [0.5], [0.2], 100.0, index)
    assert np.array_equal(got, se.score_sweep_host([np.full(1000, 0.9)], ch, [0.5], [0.2], 100.0, index)) and got[0, 0, 0, 2] > 0
    assert se.score_sweep_device(torch.zeros((1, 0), device="cuda"), ch, [0.5], [0.2], 100.0, index).shape == (1, 1, 1, 7)
    # the DeviceIndex itself may be passed (built once, kept by the index)
    dix = index.to_device(ch)
    assert dix is index.to_device(ch) and dix.n_intervals == dix.offsets_host[-1] > 0
    assert np.array_equal(se.score_sweep_device(p, ch, [0.5], [0.2], 100.0, dix), got)


def test_evaluate_sweep_device_against_host(tmp_path, capsys):
    import evaluate_sweep
    args = sm.write_corpus(tmp_path)
    out = {}
    for scorer in ("host", "device"):
        evaluate_sweep.main(args + ["--scorer", scorer, "--out_dir", str(tmp_path / scorer)])
        assert f"({scorer} scorer)" in capsys.readouterr().out
        out[scorer] = {f: open(tmp_path / scorer / f, "rb").read() for f in sorted(os.listdir(tmp_path / scorer))}
    assert list(out["host"]) == ["eval_df_per_meeting.csv", "sum_stats.csv"]
    assert out["host"] == out["device"]
    assert out["host"]["eval_df_per_meeting.csv"].count(b"\n") == 1 + 2 * 3 * 2
