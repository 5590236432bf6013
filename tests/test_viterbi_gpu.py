"""GPU tests of the two-state Viterbi decoder on the device (csrc/viterbi.hip; laugh_segmenter.viterbi_frame_spans_device /
viterbi_instances_device; sweep_eval.score_sweep_device with penalties; evaluate_sweep.py --penalties --scorer device).

Integer arithmetic: every comparison is an equality with the per-frame model of tests/_viterbi_model.py.  The tracks are built
with the table S[u] = u - 32768, so that a frame's score is a chosen integer and ties are placed on purpose; their values are
float32-representable, so one model serves both dtypes."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _score_model as sm
import _viterbi_model as vm
from oracle import recipe

pytestmark = pytest.mark.gpu

CENTRED = (np.arange(65537, dtype=np.int64) - 32768).astype(np.int32)
TILE = 512
LENGTHS = [1, 2, TILE - 1, TILE, TILE + 1, 4 * TILE, 4 * TILE + 1, 9 * TILE + 5]
M = "Bmr001"
I32P = ctypes.POINTER(ctypes.c_int32)


def _settings70():
    """70 settings (two rounds underneath): every small bias and penalty, ties included, and the ends of both ranges."""
    rng = np.random.default_rng(7)
    fixed = [(0, 0), (0, 1), (1, 0), (-1, 0), (0, 5), (2, 30), (-2, 200), (0, 1 << 26), (1 << 24, 0), (-(1 << 24), 3)]
    return fixed + [(int(b), int(p)) for b, p in zip(rng.integers(-3, 4, 60), rng.integers(0, 80, 60))]


def track_of(scores):
    return np.array([np.nan if s is None else (s + 32768) / 65536.0 for s in scores], dtype=np.float64)


def _tuples(a):
    return [tuple(int(v) for v in r) for r in a]


def _dev(p, settings, table=CENTRED):
    """viterbi_frame_spans_device of a numpy track (T,) or (C, T) as lists of tuples."""
    import laugh_segmenter as ls
    got = ls.viterbi_frame_spans_device(torch.from_numpy(np.ascontiguousarray(p)).cuda(), settings, table)
    if np.ndim(p) == 1:
        got = [got]
    for per_channel in got:
        assert len(per_channel) == len(settings)
        for g in per_channel:
            assert g.dtype == np.int64 and g.ndim == 2 and g.shape[1] == 2
    got = [[_tuples(g) for g in per_channel] for per_channel in got]
    return got[0] if np.ndim(p) == 1 else got


def _model(scores, settings):
    """[(runs, best)] per setting for a list of integer frame scores (None: NaN) under CENTRED."""
    out = []
    for bias, penalty in settings:
        s = [vm.NAN_SCORE if v is None else v - bias for v in scores]
        path, best = vm.decode(s, penalty)
        out.append((vm.runs(path), best))
    return out


def _count_fill(p, settings, table=CENTRED, capacity=None, guard=1):
    """lad_viterbi_count + lad_viterbi_fill through ctypes on a (C, T) numpy track -> (rc of the fill, counts, rows (numpy, with
    `guard` rows of -7 behind the capacity), best)."""
    import _hip
    lib = _hip.lib()
    dev = torch.from_numpy(np.ascontiguousarray(p)).cuda()
    C, T = dev.shape
    K = len(settings)
    bias = (ctypes.c_int32 * K)(*[s[0] for s in settings])
    penalty = (ctypes.c_int32 * K)(*[s[1] for s in settings])
    table = np.ascontiguousarray(table, dtype=np.int32)
    table_dev = torch.from_numpy(table).cuda()
    ws = torch.empty(lib.lad_viterbi_workspace_bytes(C, T, K), dtype=torch.uint8, device="cuda")
    best = torch.empty(C * K, dtype=torch.int64, device="cuda")
    stream = _hip.stream_handle(dev.device)
    _hip.check(lib.lad_viterbi_count(_hip.ptr(dev), 0 if dev.dtype == torch.float32 else 1, C, T, _hip.ptr(table_dev),
                                     table.ctypes.data_as(I32P), bias, penalty, K, _hip.ptr(ws), _hip.ptr(best), stream), "lad_viterbi_count")
    counts = np.ascontiguousarray(ws[:4 * C * K].view(torch.int32).cpu().numpy())
    total = int(counts.sum())
    capacity = total if capacity is None else capacity
    rows = torch.full((capacity + guard, 2), -7, dtype=torch.int32, device="cuda")
    rc = lib.lad_viterbi_fill(_hip.ptr(ws), counts.ctypes.data_as(I32P), C, T, K, _hip.ptr(rows), capacity, stream)
    return rc, counts, rows.cpu().numpy(), best.cpu().numpy()


@pytest.fixture(scope="module")
def random_case():
    """{T: (scores of three channels -- the second with NaN frames, the third shorter --, {channel: model per setting})}: random
    integer scores in -6..6 with stretches of zeros, computed once for all 70 settings."""
    import _hip
    assert int(_hip.lib().lad_runs_tile_frames()) == TILE and int(_hip.lib().lad_viterbi_max_settings()) == 64
    settings = _settings70()
    out = {}
    for T in LENGTHS:
        rng = np.random.default_rng(T)
        chans = []
        for c, n in enumerate((T, T, max(1, T - T // 3))):
            s = [int(v) for v in rng.integers(-6, 7, n)]
            for at in rng.integers(0, n, n // 100):
                s[at:at + 5] = [0] * len(s[at:at + 5])
            if c == 1:
                for at in rng.integers(0, n, n // 40):
                    s[at] = None
            chans.append(s)
        out[T] = (chans, {c: _model(s, settings) for c, s in enumerate(chans)})
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("T", LENGTHS)
def test_random_tracks_against_the_model(random_case, T, dtype):
    settings = _settings70()
    chans, model = random_case[T]
    padded = np.full((3, T), np.nan, dtype)
    for c, s in enumerate(chans):
        padded[c, :len(s)] = track_of(s)
    n_runs = 0
    for K in (1, 64, 70):
        one = _dev(padded[0], settings[:K])
        three = _dev(padded, settings[:K])
        for k in range(K):
            assert one[k] == model[0][k][0], (T, K, k)
            for c in range(3):
                assert three[c][k] == model[c][k][0], (T, K, c, k)
                n_runs += len(three[c][k])
    assert n_runs > 0 or T <= 2
    # `best`, and the tables laid out as lad_runs_fill lays them out, from the entry points themselves
    rc, counts, rows, best = _count_fill(padded, settings[:64])
    assert rc == 0
    want_rows = [r for c in range(3) for k in range(64) for r in model[c][k][0]]
    assert counts.tolist() == [len(model[c][k][0]) for c in range(3) for k in range(64)]
    assert _tuples(rows[:-1]) == want_rows and rows[-1].tolist() == [-7, -7]
    assert best.tolist() == [model[c][k][1] for c in range(3) for k in range(64)]


def _expect(scores, settings, dtype):
    """The device's runs for integer scores, checked against the model; returned for explicit expectations."""
    got = _dev(track_of(scores).astype(dtype), settings)
    assert got == [m[0] for m in _model(scores, settings)]
    return got


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_constructed_tracks(dtype):
    T = 4 * TILE + 1
    few = [(0, 0), (0, 1), (0, 100), (2, 7), (-4, 0), (3, 1 << 26)]
    assert _expect([3] * T, few, dtype) == [[(0, T - 1)]] * 3 + [[(0, T - 1)], [(0, T - 1)], []]     # all on; (3, .): every score 0
    assert _expect([-3] * T, few, dtype) == [[], [], [], [], [(0, T - 1)], []]                        # all off; bias -4 turns it on
    # NaN inside a run: it ends there and pays again behind it, at and beside the tile edges
    s = [5] * T
    for at in (0, 7, TILE - 1, TILE, 2 * TILE + 1, 3 * TILE - 1, T - 1):
        s[at] = None
    cut = [(1, 6), (8, TILE - 2), (TILE + 1, 2 * TILE), (2 * TILE + 2, 3 * TILE - 2), (3 * TILE, T - 2)]
    got = _expect(s, [(0, 0), (0, 29), (0, 31)], dtype)
    assert got[0] == cut and got[1] == cut and got[2] == cut[1:]                                     # (1, 6) is worth 30
    # zero-score frames at the tile edges: they take the state of the frame behind them (penalty 0), off at the end
    s = [(-1, 1)[(i // 37) % 2] for i in range(T)]
    for e in (TILE, 2 * TILE, 3 * TILE, 4 * TILE):
        for at in range(e - 2, min(e + 2, T)):
            s[at] = 0
    s[T - 1] = 0
    got = _expect(s, [(0, 0), (0, 1), (0, 36), (0, 37), (0, 38), (1, 0), (-1, 0)], dtype)
    path = [0] * T
    for a, b in got[0]:
        path[a:b + 1] = [1] * (b - a + 1)
    for t in range(T):
        assert path[t] == (1 if s[t] > 0 else 0 if s[t] < 0 else (path[t + 1] if t + 1 < T else 0)), t
    # a whole track of zeros, and zeros in front of one positive frame in the last tile
    assert _expect([0] * T, [(0, 0), (0, 5)], dtype) == [[], []]
    assert _expect([0] * (T - 1) + [1], [(0, 0), (0, 1), (0, 2)], dtype) == [[(0, T - 1)], [], []]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_one_unit_of_evidence_tiles_away(dtype):
    """A plateau of n = 3 * tile + 7 frames of +1 between long stretches of -1 is worth exactly n: at a penalty of n - 1 it is an
    event, at n + 1 it is not, and at n the tie is the model's to decide -- the forward carry and the backtrace carry both cross
    several tiles.  The mirror: a pause of n frames of -1 between two strong runs is bridged iff it costs no more than a second event."""
    n = 3 * TILE + 7
    for lead in (2 * TILE + 3, TILE):
        s = [-1] * lead + [1] * n + [-1] * (2 * TILE + 3)
        got = _expect(s, [(0, n - 1), (0, n), (0, n + 1)], dtype)
        assert got[0] == [(lead, lead + n - 1)] and got[2] == []
        assert got[1] in ([], [(lead, lead + n - 1)])
        s = [-1] * lead + [3000] * 10 + [-1] * n + [3000] * 10 + [-1] * 40
        got = _expect(s, [(0, n - 1), (0, n), (0, n + 1)], dtype)
        assert got[0] == [(lead, lead + 9), (lead + 10 + n, lead + 19 + n)]
        assert got[1] == got[2] == [(lead, lead + 19 + n)]                                           # a tie goes on
    # one frame more or less of evidence far away flips it
    s = [-1] * TILE + [1] * n + [-1] * TILE
    assert _dev(track_of(s + [-1]).astype(dtype), [(0, n - 1)]) == [[(TILE, TILE + n - 1)]]
    s[TILE + 5] = 0
    assert _expect(s, [(0, n - 1)], dtype) == [[]]


def test_identical_bytes_and_capacity():
    import _hip
    lib = _hip.lib()
    s = [int(v) for v in np.random.default_rng(11).integers(-6, 7, 9 * TILE + 5)]
    p = np.stack([track_of(s), track_of(s[::-1])]).astype(np.float32)
    settings = _settings70()[:64]
    rc, counts, rows, best = _count_fill(p, settings)
    rc2, counts2, rows2, best2 = _count_fill(p, settings)
    assert rc == rc2 == 0 and counts.tobytes() == counts2.tobytes() and rows.tobytes() == rows2.tobytes() and best.tobytes() == best2.tobytes()
    total = int(counts.sum())
    assert total > 1000 and (rows[:-1] >= 0).all()
    # one row short: refused, nothing written -- the rows and the guard row behind them keep their fill value
    rc, _, short, _ = _count_fill(p, settings, capacity=total - 1)
    assert rc == _hip.LAD_ERR_INVALID and b"lad_viterbi_fill" in lib.lad_last_error() and (short == -7).all()
    # counts that are no run counts, sizes out of range, null pointers
    ws = torch.zeros(lib.lad_viterbi_workspace_bytes(2, 9 * TILE + 5, 64), dtype=torch.uint8, device="cuda")
    out = torch.full((8, 2), -7, dtype=torch.int32, device="cuda")
    bad = np.full(128, 9 * TILE, np.int32)
    stream = _hip.stream_handle(out.device)
    assert lib.lad_viterbi_fill(_hip.ptr(ws), bad.ctypes.data_as(I32P), 2, 9 * TILE + 5, 64, _hip.ptr(out), 8, stream) == _hip.LAD_ERR_INVALID
    zero = np.zeros(128, np.int32)
    assert lib.lad_viterbi_fill(_hip.ptr(ws), zero.ctypes.data_as(I32P), 2, 9 * TILE + 5, 64, None, 0, stream) == 0     # nothing to write
    assert lib.lad_viterbi_fill(_hip.ptr(ws), zero.ctypes.data_as(I32P), 2, 9 * TILE + 5, 65, _hip.ptr(out), 8, stream) == _hip.LAD_ERR_INVALID
    assert lib.lad_viterbi_fill(None, zero.ctypes.data_as(I32P), 2, 9 * TILE + 5, 64, _hip.ptr(out), 8, stream) == _hip.LAD_ERR_INVALID
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7).all()


def test_count_refuses_bad_arguments():
    import _hip
    lib = _hip.lib()
    dev = torch.full((1, 100), 0.75, dtype=torch.float32, device="cuda")
    table_dev = torch.from_numpy(CENTRED).cuda()
    ws = torch.zeros(lib.lad_viterbi_workspace_bytes(1, 100, 2), dtype=torch.uint8, device="cuda")
    stream = _hip.stream_handle(dev.device)

    def call(probs=dev, dtype=0, C=1, T=100, emission=table_dev, host=CENTRED, bias=(0, 0), penalty=(0, 0), K=2, workspace=ws):
        host = None if host is None else np.ascontiguousarray(host, dtype=np.int32).ctypes.data_as(I32P)
        return lib.lad_viterbi_count(_hip.ptr(probs), dtype, C, T, _hip.ptr(emission), host, (ctypes.c_int32 * 2)(*bias),
                                     (ctypes.c_int32 * 2)(*penalty), K, _hip.ptr(workspace), None, stream)
    wide = CENTRED.copy()
    wide[40000] = (1 << 24) + 1
    for kw in (dict(dtype=2), dict(C=0), dict(T=0), dict(K=0), dict(K=65), dict(probs=None), dict(emission=None), dict(host=None),
               dict(workspace=None), dict(host=wide), dict(bias=(0, (1 << 24) + 1)), dict(bias=(-(1 << 24) - 1, 0)),
               dict(penalty=(-1, 0)), dict(penalty=(0, (1 << 26) + 1))):
        assert call(**kw) == _hip.LAD_ERR_INVALID, kw
        assert b"lad_viterbi_count" in lib.lad_last_error(), kw
    torch.cuda.synchronize()
    assert int(ws.sum()) == 0                                                                         # nothing was launched
    assert call() == 0                                                                                # a null `best` is fine
    torch.cuda.synchronize()
    assert ws[:8].view(torch.int32).tolist() == [1, 1]                                                # p = 0.75 scores 16384: one run


def test_default_table_and_instances():
    """The public forms with the default emission table on realistic tracks: two channels of different lengths, 87 settings."""
    import laugh_segmenter as ls
    table = ls.viterbi_emission_table()
    thresholds = [float(t) for t in np.concatenate((np.linspace(0.05, 0.9, 18).round(2), np.linspace(0.91, 1, 10).round(2), [0.5001]))]
    settings = ls.viterbi_settings(thresholds, [0.0, 2.0, 4.0], table)
    assert len(settings) == 87
    tracks = [recipe.make_prob_track(5, 3000).astype(np.float32), recipe.make_prob_track(6, 2200).astype(np.float32)]
    tracks[1][::97] = np.nan
    padded = np.full((2, 3000), np.nan, np.float32)
    for c, t in enumerate(tracks):
        padded[c, :len(t)] = t
    got = ls.viterbi_frame_spans_device(torch.from_numpy(padded).cuda(), settings)
    for c, t in enumerate(tracks):
        want = ls._viterbi_spans_host(t, settings, table)
        for k in range(87):
            assert np.array_equal(got[c][k], want[k]), (c, k)
        for k in (0, 40, 86):
            assert _tuples(got[c][k]) == vm.spans(t.tolist(), table, *settings[k])[0]
    dev = torch.from_numpy(tracks[0]).cuda()
    inst = ls.viterbi_instances_device(dev, [0.3, 0.6], [0.0, 0.2], 36000 / 360.37, [0.0, 3.0])
    assert inst == ls.viterbi_instances(tracks[0], [0.3, 0.6], [0.0, 0.2], 36000 / 360.37, [0.0, 3.0])
    assert list(inst) == [(t, q, l) for t in (0.3, 0.6) for q in (0.0, 3.0) for l in (0.0, 0.2)]
    import _hip
    with pytest.raises(_hip.LadHipError):
        ls.viterbi_frame_spans_device(tracks[0], settings)                                           # no CPU fallback
    with pytest.raises(_hip.LadHipError):
        ls.viterbi_instances_device(torch.from_numpy(padded).cuda())
    empty = ls.viterbi_frame_spans_device(torch.zeros(0, device="cuda"), settings[:2])
    assert len(empty) == 2 and all(g.shape == (0, 2) for g in empty)


def test_score_sweep_device_against_host():
    import sweep_eval as se
    T = 4000
    thresholds, min_lengths, penalties = [0.2, 0.5, 0.9], [0.0, 0.2], [0.0, 2.0, 4.0]
    fps = [100.0, 36000 / 360.37]
    duration = T / min(fps)
    rows = sm.make_rows(81, M, ["fe001", "me002"], duration * 1.05, n_per_type=60, max_len_s=1.0)
    chans = [{"meeting_id": M, "part_id": p, "chan": f"chan{i}", "length": duration} for i, p in enumerate(["fe001", "me002"])]
    index = se.TranscriptIndex(rows, chans)
    channels = [(M, "chan0"), (M, "chan1")]
    tracks = [recipe.make_prob_track(82, T).astype(np.float32), recipe.make_prob_track(83, T - 100).astype(np.float32)]
    tracks[1][::61] = np.nan
    padded = np.full((2, T), np.nan, np.float32)
    for c, t in enumerate(tracks):
        padded[c, :len(t)] = t
    dev = torch.from_numpy(padded).cuda()
    want, want_ev = se.score_sweep_host(tracks, channels, thresholds, min_lengths, fps, index, penalties=penalties, events=(100, 25))
    got, got_ev = se.score_sweep_device(dev, channels, thresholds, min_lengths, fps, index, penalties=penalties, events=(100, 25))
    assert got.shape == got_ev.shape == (2, 3, 3, 2, 7) and got.dtype == got_ev.dtype == np.int64
    assert np.array_equal(got, want) and np.array_equal(got_ev, want_ev)
    assert np.array_equal(se.score_sweep_device(dev, channels, thresholds, min_lengths, fps, index, penalties=penalties), want)
    assert (got.sum(axis=(0, 1, 2, 3)) > 0).all() and got_ev[..., 2].sum() > 0
    with pytest.raises(ValueError):
        se.score_sweep_device(dev, channels, thresholds, min_lengths, fps, index, penalties=penalties, offset_drops=[0.0])
    # the low-pass composes in front
    import laugh_segmenter as ls
    smooth = se.score_sweep_device(dev, channels, thresholds, min_lengths, fps, index, penalties=penalties, lowpass=0.05,
                                   lengths=[len(t) for t in tracks])
    low = ls.lowpass_device(dev, cutoff=0.05, lengths=[len(t) for t in tracks]).cpu().numpy()
    assert np.array_equal(smooth, se.score_sweep_host([low[c, :len(t)] for c, t in enumerate(tracks)], channels, thresholds, min_lengths,
                                                      fps, index, penalties=penalties))


def test_evaluate_sweep_penalties_device_against_host(tmp_path, capsys):
    import evaluate_sweep
    args = sm.write_corpus(tmp_path)
    out = {}
    for scorer in ("host", "device"):
        where = tmp_path / scorer
        evaluate_sweep.main(args + ["--penalties", "0,2,4", "--events", "--scorer", scorer, "--out_dir", str(where)])
        assert f"18 settings ({scorer} scorer)" in capsys.readouterr().out
        out[scorer] = {f: open(where / f, "rb").read() for f in sorted(os.listdir(where))}
    assert list(out["host"]) == ["eval_df_per_meeting.csv", "event_df_per_meeting.csv", "event_sum_stats.csv", "sum_stats.csv"]
    assert out["host"] == out["device"]
    assert out["host"]["eval_df_per_meeting.csv"].count(b"\n") == 1 + 2 * 3 * 3 * 2
