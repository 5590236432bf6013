"""GPU tests of the event scorer (csrc/events.hip; sweep_eval.score_sweep_device(events=); evaluate_sweep.py --events --scorer device).

Everything is integers: every comparison is an equality -- against the host scorer (sweep_eval.event_scores_instances) and, on the
small cases, against the per-pair model of tests/_events_model.py, which shares nothing with either."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _events_model as em
import _score_model as sm
from oracle import recipe

pytestmark = pytest.mark.gpu

EVAL_THRESHOLDS = [float(t) for t in np.concatenate((np.linspace(0, 0.9, 19).round(2), np.linspace(0.91, 1, 10).round(2)))]
EVAL_MIN_LENGTHS = [0.0, 0.1, 0.2]
MODEL_THRESHOLDS = [0.3, 0.5, 0.6, 0.7]
AWKWARD_FPS = 360000 / 3600.0049375
CRITERIA = [(1, 0), (200, 50)]
M = "Bmr001"


def _corpus(seed, parts, duration, n_per_type, max_len_s, unmapped=()):
    import sweep_eval as se
    rows = sm.make_rows(seed, M, parts, duration, n_per_type=n_per_type, max_len_s=max_len_s)
    chans = [{"meeting_id": M, "part_id": p, "chan": f"chan{i}", "length": duration * 0.97} for i, p in enumerate(parts)]
    chans += [{"meeting_id": M, "part_id": None, "chan": c, "length": duration} for c in unmapped]
    return rows, chans, se.TranscriptIndex(rows, chans)


def _dev(tracks, channels, thresholds, min_lengths, fps, index, crit, dtype=np.float32, **kw):
    """score_sweep_device(events=crit) of tracks of different lengths (NaN padding to the longest) -> (scores, events); the time
    scores beside the events are those of a call without events=."""
    import sweep_eval as se
    T = max(len(t) for t in tracks)
    padded = np.full((len(tracks), T), np.nan, dtype)
    for c, t in enumerate(tracks):
        padded[c, :len(t)] = t
    p = torch.from_numpy(padded).cuda()
    scores, events = se.score_sweep_device(p, channels, thresholds, min_lengths, fps, index, events=crit, **kw)
    assert events.dtype == np.int64 and events.shape == scores.shape and events.shape[-1] == 7
    assert np.array_equal(scores, se.score_sweep_device(p, channels, thresholds, min_lengths, fps, index, **kw))
    return scores, events


def _invariants(scores, events, crit):
    n_ref, touched, hit, pred_hit, links = (events[..., f] for f in range(5))
    assert (hit <= touched).all() and (touched <= n_ref).all() and (links >= touched).all() and (pred_hit <= scores[..., 1]).all()
    assert (events >= 0).all() and (events[..., 5:][hit == 0] == 0).all()
    if crit == (1, 0):
        assert np.array_equal(hit, touched)


@pytest.fixture(scope="module")
def small():
    """The corpus of tests/test_events_cpu.py with the model's events."""
    rows, chans, index = _corpus(62, ["fe001"], 1.05 * 360, 300, 1.8)
    assert chans[0]["length"] == 0.97 * 378
    model = em.EventModel(rows, chans, sm.to_frames(1.05 * 360 * 1.2) + 10)
    return index, model, model.events(M, "chan0"), recipe.make_prob_track(6, 36000)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_small_corpus_all_settings(small, dtype):
    import laugh_segmenter as ls
    import sweep_eval as se
    index, model, model_events, p = small
    p = p.astype(dtype)
    ch = [(M, "chan0")]
    for fps in (100.0, AWKWARD_FPS):
        inst = ls.get_laughter_instances(p, MODEL_THRESHOLDS, EVAL_MIN_LENGTHS, fps)
        pairs = {key: model.pairs(spans, M, "chan0", model_events) for key, spans in inst.items()}
        for crit in CRITERIA:
            scores, events = _dev([p], ch, EVAL_THRESHOLDS, EVAL_MIN_LENGTHS, fps, index, crit, dtype)
            host_scores, host_events = se.score_sweep_host([p], ch, EVAL_THRESHOLDS, EVAL_MIN_LENGTHS, fps, index, events=crit)
            assert np.array_equal(scores, host_scores) and np.array_equal(events, host_events), (fps, crit)
            _invariants(scores, events, crit)
            assert (events[..., 0] == 97).all() and (events[0, :, :, 2] > 0).sum() > 30
            for t in MODEL_THRESHOLDS:
                for l, min_l in enumerate(EVAL_MIN_LENGTHS):
                    assert tuple(events[0, EVAL_THRESHOLDS.index(t), l]) == model.score_pairs(pairs[(t, min_l)], *crit), (fps, crit, t, min_l)
    if dtype == np.float64:
        _, events = _dev([p], ch, [0.3, 0.5], [0.0, 0.2], 100.0, index, (200, 50), dtype)
        assert events[0, 0, 0].tolist() == [97, 89, 64, 60, 139, 43041, 45957] and events[0, 1, 1].tolist() == [97, 47, 10, 30, 61, 1384, 1161]


def _edge_tracks(tile):
    T = 3 * tile + 70
    edges = list(range(64, T, 64))
    below = np.full(T, 0.25)
    below[[0, T - 1] + [e - 1 for e in edges]] = 0.75                                   # single frames before every word / tile edge
    both = below.copy()
    both[edges] = 0.75                                                                 # two-frame runs across every edge
    holes = np.full(T, 0.75)
    holes[[0, T - 1] + edges] = 0.25
    long = np.full(T, 0.25)
    long[tile // 2:2 * tile + tile // 2 + 5] = 0.75                                    # one run through two whole tiles
    nan = holes.copy()
    nan[100:700] = np.nan                                                              # off for every threshold
    return T, [below, long, both, holes, nan]


def test_table_boundaries_and_empty_tables():
    import _hip
    import laugh_segmenter as ls
    import sweep_eval as se
    tile = int(_hip.lib().lad_runs_tile_frames())
    assert tile == 512
    T, tracks = _edge_tracks(tile)
    fps = 100.0
    # an index made from the run tables of threshold 0.5: events that end exactly on run ends, the first and the last event of a
    # channel over the first and the last run of its table
    rows = []
    for c, t in enumerate(tracks):
        spans = ls.get_laughter_frame_spans(t, 0.5)
        ends = [int(last) / fps for _, last in spans]
        laughs = [(0.0, 0.25)] + [(e - 0.25, e) for e in ends[::3] if e > 0.5] + [(ends[-1] - 0.25, ends[-1] + 0.1)]
        rows += [{"meeting_id": M, "part_id": f"fe{c:03d}", "chan": f"chan{c}", "start": s, "end": e, "length": e - s, "type": "laugh",
                  "laugh_type": "laugh"} for s, e in laughs]
        rows.append({"meeting_id": M, "part_id": f"fe{c:03d}", "chan": f"chan{c}", "start": 3.0, "end": 3.3, "length": 0.3,
                     "type": "invalid", "laugh_type": None})
    chans = [{"meeting_id": M, "part_id": f"fe{c:03d}", "chan": f"chan{c}", "length": T / fps * 1.1} for c in range(5)]
    index = se.TranscriptIndex(rows, chans)
    model = em.EventModel(rows, chans, sm.to_frames(T / fps * 1.3) + 10)
    channels = [(M, f"chan{c}") for c in range(5)]
    thresholds, min_lengths = [0.0, 0.5, 1.0], [-1.0, 0.0, 0.005, 0.1]
    for crit in CRITERIA + [(0, 100)]:
        scores, events = _dev(tracks, channels, thresholds, min_lengths, fps, index, crit, np.float64)
        host_scores, host_events = se.score_sweep_host(tracks, channels, thresholds, min_lengths, fps, index, events=crit)
        assert np.array_equal(events, host_events) and np.array_equal(scores, host_scores), crit
        _invariants(scores, events, crit)
        for c, t in enumerate(tracks):
            inst = ls.get_laughter_instances(t, thresholds, min_lengths, fps)
            want = [[model.score(inst[(thr, l)], M, f"chan{c}", *crit) for l in min_lengths] for thr in thresholds]
            assert events[c].tolist() == [[list(w) for w in ws] for ws in want], (crit, c)
    # the tables of threshold 1.0 are empty and sit between full ones: only the events are counted there
    n_ref = [len(index.scoring_sets(*mc)[1]) for mc in channels]
    assert min(n_ref) >= 2 and max(n_ref) >= 8 and events[:, 2, :, 0].tolist() == [[n] * 4 for n in n_ref] and not events[:, 2, :, 1:].any()
    # threshold 0: one run over the whole track touches every event, first and last
    assert events[:, 0, :, 1].tolist() == [[n] * 4 for n in n_ref] and events[:, 0, :, 4].tolist() == [[n] * 4 for n in n_ref]
    # single-frame runs (a == b) are kept for min_length -1 only and overlap nothing
    assert scores[0, 1, :, 0].tolist() == [T // 64 + 2, 0, 0, 0] and not events[0, 1, :, 1:].any()
    # the holes track at 0.5: runs of 63 frames, every event that ends on a run end is touched, the first and the last one too
    assert events[3, 1, 0, 1] == n_ref[3] and events[3, 1, 3, 4] >= n_ref[3]


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
    crit = (200, 50)
    scores, many = _dev(tracks, channels, EVAL_THRESHOLDS, EVAL_MIN_LENGTHS, fps, index, crit)
    host = se.score_sweep_host([t.astype(np.float32) for t in tracks], channels, EVAL_THRESHOLDS, EVAL_MIN_LENGTHS, fps, index,
                               events=crit)[1]
    assert np.array_equal(many, host)
    _invariants(scores, many, crit)
    for c in range(10):
        one = _dev([tracks[c]], [channels[c]], EVAL_THRESHOLDS, EVAL_MIN_LENGTHS, fps[c], index, crit)[1]
        assert np.array_equal(one[0], many[c]), c
    assert not many[9].any() and not many[4].any()                                      # no participant; a participant without a row
    assert (many[3, :, :, 0] > 50).all() and not many[3, :, :, 1:].any()                # no run: the events are still counted
    assert many[0, :, :, 2].sum() > 500 and many[0, :, :, 3].sum() > 500 and many[1, :, :, 5].sum() > 0
    again = _dev(tracks, channels, EVAL_THRESHOLDS, EVAL_MIN_LENGTHS, fps, index, crit)[1]
    assert again.tobytes() == many.tobytes()


def test_the_largest_k_and_l():
    import _hip
    import sweep_eval as se
    lib = _hip.lib()
    kmax, lmax = int(lib.lad_runs_max_thresholds()), int(lib.lad_score_max_min_lengths())
    assert kmax == 64 and lmax == 8
    thresholds = [float(t) for t in np.linspace(0.0, 1.0, kmax)]
    min_lengths = [float(l) for l in np.linspace(-0.01, 0.3, lmax)]
    _, tracks = _edge_tracks(512)
    p = [recipe.make_prob_track(9, 36000), tracks[2]]
    rows, chans, index = _corpus(65, ["fe001", "fe002"], 380.0, 300, 1.0)
    channels = [(M, "chan0"), (M, "chan1")]
    for crit in CRITERIA:
        scores, events = _dev(p, channels, thresholds, min_lengths, 100.0, index, crit)
        host = se.score_sweep_host([t.astype(np.float32) for t in p], channels, thresholds, min_lengths, 100.0, index, events=crit)[1]
        assert events.shape == (2, 64, 8, 7) and np.array_equal(events, host)
        _invariants(scores, events, crit)
    assert events[0, 1:-1, 0, 1].min() > 0 and (events[0, :30, -1, 2] > 0).all() and events[0, 40:, -1, 1:].max() == 0


def _away_from(values, wanted, drops):
    """The thresholds nearest to `wanted` (stepping upwards) that, like threshold - drop for every drop, lie at least 1e-6 from
    every value."""
    v = np.sort(np.asarray(values, np.float64))
    out = []
    for t in wanted:
        while True:
            at = np.searchsorted(v, [t - d for d in drops])
            near = np.concatenate([np.abs(v[np.minimum(at, len(v) - 1)] - [t - d for d in drops]),
                                   np.abs(v[np.maximum(at - 1, 0)] - [t - d for d in drops])])
            if near.min() >= 1e-6:
                break
            t += 1e-5
        out.append(float(t))
    return out


def test_binarize_rounds_and_the_lowpass_in_front(small):
    import laugh_segmenter as ls
    import sweep_eval as se
    index, _, _, p = small
    ch = [(M, "chan0")]
    drops, gaps = [0.0, 0.1, 0.2], [0.0, 0.3, 1.0]
    # 29 x 3 x 3 = 261 settings: more than one round of lad_binarize_max_settings()
    for crit in CRITERIA:
        scores, events = _dev([p], ch, EVAL_THRESHOLDS, EVAL_MIN_LENGTHS, 100.0, index, crit, np.float64, offset_drops=drops, min_gaps=gaps)
        host = se.score_sweep_host([p], ch, EVAL_THRESHOLDS, EVAL_MIN_LENGTHS, 100.0, index, offset_drops=drops, min_gaps=gaps,
                                   events=crit)[1]
        assert events.shape == (1, 29, 3, 3, 3, 7) and np.array_equal(events, host)
        _invariants(scores, events, crit)
    assert events[0, EVAL_THRESHOLDS.index(0.6), 1, 1, 2].tolist()[:2] == [97, 86]
    plain = _dev([p], ch, EVAL_THRESHOLDS, EVAL_MIN_LENGTHS, 100.0, index, crit, np.float64)[1]
    assert np.array_equal(events[:, :, 0, 0], plain) and (events[:, :, 2, 2, :, 4] != plain[..., 4]).any()
    # 3 x 3 x 3 settings behind the low-pass, three channels of different lengths: the host form is fed laugh_segmenter.lowpass
    lengths = [4000, 3100, 2500]
    tracks = [recipe.make_prob_track(80 + c, n) for c, n in enumerate(lengths)]
    host_filtered = [ls.lowpass(t) for t in tracks]
    thresholds = _away_from(ls.fix_probs(np.concatenate(host_filtered)), [0.3, 0.5, 0.6], drops)
    decisions = np.array([t - d for t in thresholds for d in drops])
    margin = float(np.min(np.abs(ls.fix_probs(np.concatenate(host_filtered))[:, None] - decisions[None, :])))
    print(f"thresholds {thresholds}: nearest smoothed value to a decision level {margin:.2e}")
    assert margin >= 1e-6                                       # no decision hangs on the last digits of either filter
    parts = ["fe001", "me002", "mn003"]
    rows = sm.make_rows(71, M, parts, 40.0, n_per_type=40, max_len_s=1.5)
    chans = [{"meeting_id": M, "part_id": q, "chan": f"chan{i}", "length": 40.0} for i, q in enumerate(parts)]
    index = se.TranscriptIndex(rows, chans)
    channels = [(M, f"chan{i}") for i in range(3)]
    for crit in CRITERIA:
        scores, events = _dev(tracks, channels, thresholds, EVAL_MIN_LENGTHS, 100.0, index, crit, np.float64, lowpass=0.01, lengths=lengths,
                              offset_drops=drops, min_gaps=gaps)
        host_scores, host = se.score_sweep_host(host_filtered, channels, thresholds, EVAL_MIN_LENGTHS, 100.0, index, offset_drops=drops,
                                                min_gaps=gaps, events=crit)
        assert events.shape == (3, 3, 3, 3, 3, 7) and np.array_equal(events, host) and np.array_equal(scores, host_scores)
    assert (events[..., 1].sum(axis=(1, 2, 3, 4)) > 0).all()
    raw = _dev(tracks, channels, thresholds, EVAL_MIN_LENGTHS, 100.0, index, crit, np.float64, offset_drops=drops, min_gaps=gaps)[1]
    assert not np.array_equal(raw, events)                      # the switch does something


def _raw_call(p, thresholds, min_lengths, fps, bounds, offsets, events, crit=(1, 0), counts=None, null=None):
    """lad_runs_count + lad_runs_fill + lad_score_events through the C ABI; returns the code of lad_score_events."""
    import _hip
    lib = _hip.lib()
    C, T = p.shape
    K, L = len(thresholds), len(min_lengths)
    thr = (ctypes.c_double * K)(*thresholds)
    mls = (ctypes.c_double * L)(*min_lengths)
    fps_host = np.asarray(fps, np.float64)
    i32p, f64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    st = _hip.stream_handle()
    ws = torch.empty(lib.lad_runs_workspace_bytes(C, T, K), dtype=torch.uint8, device="cuda")
    _hip.check(lib.lad_runs_count(_hip.ptr(p), 0, C, T, thr, K, _hip.ptr(ws), st), "lad_runs_count")
    true_counts = np.ascontiguousarray(ws[:4 * C * K].view(torch.int32).cpu().numpy())
    total = int(true_counts.sum())
    table = torch.empty((max(total, 1), 2), dtype=torch.int32, device="cuda")
    _hip.check(lib.lad_runs_fill(_hip.ptr(p), 0, C, T, thr, K, _hip.ptr(ws), true_counts.ctypes.data_as(i32p), _hip.ptr(table), total, st),
               "lad_runs_fill")
    ews = torch.empty(lib.lad_score_events_workspace_bytes(C, len(bounds), K, L, total), dtype=torch.uint8, device="cuda")
    counts = true_counts if counts is None else np.ascontiguousarray(counts, np.int32)
    b_host = np.ascontiguousarray(bounds, np.int32).reshape(-1, 2)
    o_host = np.ascontiguousarray(offsets, np.int32)
    b_dev, o_dev, f_dev = torch.from_numpy(b_host).cuda(), torch.from_numpy(o_host).cuda(), torch.from_numpy(fps_host).cuda()
    args = [_hip.ptr(ws), _hip.ptr(table), counts.ctypes.data_as(i32p), C, T, K, _hip.ptr(b_dev), _hip.ptr(o_dev),
            b_host.ctypes.data_as(i32p), o_host.ctypes.data_as(i32p), len(b_host), _hip.ptr(f_dev), fps_host.ctypes.data_as(f64p), mls, L,
            *crit, _hip.ptr(ews), _hip.ptr(events), st]
    if null is not None:
        args[null] = None
    rc = lib.lad_score_events(*args)
    torch.cuda.synchronize()
    return rc


def test_errors_write_nothing_and_leave_the_path_usable():
    import _hip
    import sweep_eval as se
    lib = _hip.lib()
    p = torch.full((1, 1000), 0.9, device="cuda")
    good_b, good_o = [[100, 200], [300, 400], [0, 50]], [0, 0, 2, 3, 3, 3]
    guard = 16

    def fresh():
        return torch.full((7 + guard,), -7, dtype=torch.int64, device="cuda")
    cases = [("pct above 100", dict(crit=(1, 101)), b"min_overlap_pct 0..100"),
             ("negative pct", dict(crit=(1, -1)), b"min_overlap_pct 0..100"),
             ("negative ms", dict(crit=(-1, 0)), b"min_overlap_ms >= 0"),
             ("unsorted", dict(bounds=[[300, 400], [100, 200], [0, 50]]), b"unsorted or overlaps"),
             ("empty interval", dict(bounds=[[100, 100], [300, 400], [0, 50]]), b"empty or negative"),
             ("descending offsets", dict(offsets=[0, 2, 1, 3, 3, 3]), b"do not ascend"),
             ("offsets short of n", dict(offsets=[0, 0, 2, 2, 2, 2]), b"index offsets run"),
             ("counts that are no run counts", dict(counts=[501]), b"is not a run count"),
             ("negative counts", dict(counts=[-1]), b"is not a run count"),
             ("fps 0", dict(fps=[0.0]), b"positive finite"),
             ("millisecond overflow", dict(fps=[1e-4]), b"millisecond overflow"),
             ("null workspace", dict(null=17), b"null buffer"),
             ("null events", dict(null=18), b"null buffer"),
             ("null offsets", dict(null=7), b"null buffer"),
             ("null bounds", dict(null=6), b"null interval bounds")]
    for name, change, message in cases:
        kw = dict(thresholds=[0.5], min_lengths=[0.2], fps=[100.0], bounds=good_b, offsets=good_o)
        kw.update(change)
        events = fresh()
        rc = _raw_call(p, events=events, **kw)
        assert rc == _hip.LAD_ERR_INVALID and message in lib.lad_last_error(), (name, lib.lad_last_error())
        assert b"lad_score_events:" in lib.lad_last_error(), name
        assert bool((events == -7).all()), name                                         # nothing was written
    # a table of total_runs rows cannot be sized with fewer than none
    assert lib.lad_score_events_workspace_bytes(1, 3, 1, 1, -1) == -1 and b"runs 0..2^38" in lib.lad_last_error()
    # the same buffers, a good call: seven values, the guard behind them untouched.  One run (0, 9990]; events (100, 200], (300, 400]
    events = fresh()
    assert _raw_call(p, [0.5], [0.2], [100.0], good_b, good_o, events) == 0
    out = events.cpu().numpy()
    assert out[:7].tolist() == [2, 2, 2, 1, 2, 100 + 300, 9790 + 9590] and (out[7:] == -7).all()
    events = fresh()
    assert _raw_call(p, [0.5], [0.2], [100.0], good_b, good_o, events, crit=(1, 3)) == 0               # 200 of 9990 ms: 2 per cent
    assert events.cpu().numpy()[:7].tolist() == [2, 2, 2, 0, 2, 400, 19380]
    # the Python surface
    rows, chans, index = _corpus(68, ["fe001"], 12.0, 20, 0.5)
    ch = [(M, "chan0")]
    for bad in (p.cpu(), p.cpu().numpy()):
        with pytest.raises(_hip.LadHipError):
            se.score_sweep_device(bad, ch, [0.5], [0.2], 100.0, index, events=(1, 0))
    for bad in ((1, 101), (-1, 0)):
        with pytest.raises(_hip.LadHipError, match="min_overlap"):
            se.score_sweep_device(p, ch, [0.5], [0.2], 100.0, index, events=bad)
    with pytest.raises(TypeError):
        se.score_sweep_device(p, ch, [0.5], [0.2], 100.0, index, events=(1.5, 0))
    scores, events = se.score_sweep_device(p, ch, [0.5], [0.2], 100.0, index, events=(1, 0))
    host = se.score_sweep_host([np.full(1000, 0.9)], ch, [0.5], [0.2], 100.0, index, events=(1, 0))
    assert np.array_equal(scores, host[0]) and np.array_equal(events, host[1]) and events[0, 0, 0, 1] > 0
    # a track without a frame: nothing to launch on, the events are counted
    scores, events = se.score_sweep_device(torch.zeros((1, 0), device="cuda"), ch, [0.5], [0.2], 100.0, index, events=(1, 0))
    assert not scores.any() and events[0, 0, 0].tolist() == [len(index.scoring_sets(*ch[0])[1]), 0, 0, 0, 0, 0, 0]


def test_evaluate_sweep_events_device_against_host(tmp_path, capsys):
    import evaluate_sweep
    args = sm.write_corpus(tmp_path)
    four = ["eval_df_per_meeting.csv", "event_df_per_meeting.csv", "event_sum_stats.csv", "sum_stats.csv"]
    for name, extra in (("plain", []), ("binarize", ["--offset_drops", "0,0.1", "--min_gaps", "0,0.25"])):
        out = {}
        for scorer in ("host", "device"):
            where = tmp_path / f"{name}_{scorer}"
            evaluate_sweep.main(args + extra + ["--events", "--event_min_overlap_ms", "100", "--event_min_overlap_pct", "25", "--scorer",
                                                scorer, "--out_dir", str(where)])
            assert f"({scorer} scorer)" in capsys.readouterr().out
            out[scorer] = {f: open(where / f, "rb").read() for f in sorted(os.listdir(where))}
        assert list(out["host"]) == four and out["host"] == out["device"]
        assert out["host"]["event_df_per_meeting.csv"].count(b"\n") == 1 + 2 * 3 * 2 * (4 if extra else 1)
        # without --events the directory listing is the old one, and the two old files are the same bytes
        where = tmp_path / f"{name}_old"
        evaluate_sweep.main(args + extra + ["--scorer", "device", "--out_dir", str(where)])
        assert sorted(os.listdir(where)) == ["eval_df_per_meeting.csv", "sum_stats.csv"]
        for f in os.listdir(where):
            assert open(where / f, "rb").read() == out["device"][f]
