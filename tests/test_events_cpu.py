"""Event-level scores of the sweep (sweep_eval.event_scores_instances / event_rows / event_sum_stats, evaluate_sweep.py --events,
the size query of csrc/events.hip), the part that needs no GPU.

The yardstick is tests/_events_model.py: per-millisecond sets and a loop over every (event, prediction) pair.  Everything is
integers, so every comparison is an equality."""
import csv
import math
import os

import numpy as np
import pytest

import _events_model as em
import _score_model as sm
from oracle import recipe

EVAL_THRESHOLDS = [float(t) for t in np.concatenate((np.linspace(0, 0.9, 19).round(2), np.linspace(0.91, 1, 10).round(2)))]
EVAL_MIN_LENGTHS = [0.0, 0.1, 0.2]
AWKWARD_FPS = 360000 / 3600.0049375
M = "Bmr001"
CRITERIA = [(1, 0), (200, 50)]
MODEL_THRESHOLDS = [0.3, 0.5, 0.6, 0.7]
DROPS_GAPS = [(0.0, 0.0), (0.1, 0.3), (0.2, 0.3)]
CH = [(M, "chan0")]


@pytest.fixture(scope="module", autouse=True)
def built_lib():
    """The library is built in-tree if it is not there yet (as tests/test_cabi.py does)."""
    import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import importlib.util
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        spec = importlib.util.spec_from_file_location("lad_build", os.path.join(root, "laughter-detection-icsi_amd", "build.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.build(verbose=False)
    return _hip


@pytest.fixture(scope="module")
def corpus():
    """The seeded corpus, its index, the model and the model's event list (a loop over the universe: made once)."""
    import sweep_eval as se
    rows = sm.make_rows(62, M, ["fe001"], 1.05 * 360, n_per_type=300, max_len_s=1.8)
    chans = [{"meeting_id": M, "part_id": "fe001", "chan": "chan0", "length": 0.97 * 378}]
    index = se.TranscriptIndex(rows, chans)
    model = em.EventModel(rows, chans, sm.to_frames(1.05 * 360 * 1.2) + 10)
    events = model.events(M, "chan0")
    assert len(events) == 97 and [list(e) for e in events] == index.scoring_sets(M, "chan0")[1].tolist()
    return index, model, events, recipe.make_prob_track(6, 36000)


@pytest.mark.parametrize("fps", [100.0, AWKWARD_FPS])
def test_host_scorer_against_the_model(corpus, fps):
    import laugh_segmenter as ls
    import sweep_eval as se
    index, model, events, p = corpus
    plain = ls.get_laughter_instances(p, MODEL_THRESHOLDS, EVAL_MIN_LENGTHS, fps)
    drops, gaps = sorted({d for d, _ in DROPS_GAPS}), sorted({g for _, g in DROPS_GAPS})
    binarized = ls.binarize_instances(p, MODEL_THRESHOLDS, EVAL_MIN_LENGTHS, fps, drops, gaps)
    binarized = {k: v for k, v in binarized.items() if (k[1], k[2]) in DROPS_GAPS}
    assert len(plain) == 12 and len(binarized) == 36
    pairs = {key: model.pairs(spans, M, "chan0", events) for key, spans in binarized.items()}
    for crit in CRITERIA:
        got = se.event_scores_instances(binarized, index, M, "chan0", *crit)
        assert list(got) == list(binarized)
        for key in binarized:
            want = model.score_pairs(pairs[key], *crit)
            assert got[key] == want, (fps, crit, key, got[key], want)
            assert all(type(v) is int for v in got[key])
        plain_got = se.event_scores_instances(plain, index, M, "chan0", *crit)
        assert all(plain_got[(t, l)] == got[(t, 0.0, 0.0, l)] for t, l in plain)
    if fps == 100.0:        # the anchors of the convention, from a per-pair loop
        def one(inst, key, crit):
            return list(se.event_scores_instances({key: inst[key]}, index, M, "chan0", *crit)[key])
        assert one(plain, (0.3, 0.0), (1, 0)) == [97, 89, 89, 119, 139, 63893, 66693]
        assert one(plain, (0.3, 0.0), (200, 50)) == [97, 89, 64, 60, 139, 43041, 45957]
        assert one(plain, (0.5, 0.2), (200, 50)) == [97, 47, 10, 30, 61, 1384, 1161]
        assert one(binarized, (0.6, 0.1, 0.3, 0.2), (1, 0)) == [97, 86, 86, 66, 96, 141711, 150307]


@pytest.mark.parametrize("fps", [100.0, AWKWARD_FPS])
def test_invariants_on_every_cell(corpus, fps):
    import sweep_eval as se
    index, _, _, p = corpus
    by = {}
    for crit in [(1, 0), (200, 0), (1, 50), (200, 50), (0, 0), (100000, 100)]:
        scores, ev = se.score_sweep_host([p], CH, EVAL_THRESHOLDS, EVAL_MIN_LENGTHS, fps, index, events=crit)
        assert np.array_equal(scores, se.score_sweep_host([p], CH, EVAL_THRESHOLDS, EVAL_MIN_LENGTHS, fps, index))
        assert ev.dtype == np.int64 and ev.shape == scores.shape == (1, 29, 3, 7)
        n_ref, touched, hit, pred_hit, links = (ev[..., f] for f in range(5))
        assert (n_ref == 97).all() and (hit <= touched).all() and (touched <= n_ref).all() and (links >= touched).all()
        assert (pred_hit <= scores[..., 1]).all() and (ev >= 0).all()
        assert (ev[..., 5:][hit == 0] == 0).all()
        by[crit] = ev
    assert np.array_equal(by[(1, 0)][..., 2], by[(1, 0)][..., 1]) and np.array_equal(by[(0, 0)], by[(1, 0)])
    assert (by[(1, 0)][..., 1] > 0).sum() > 40 and by[(200, 50)][..., 2].max() > 30
    # what does not depend on the criterion; raising either criterion never raises a hit count
    for crit in by:
        assert np.array_equal(by[crit][..., [0, 1, 4]], by[(1, 0)][..., [0, 1, 4]])
    for low, high in (((1, 0), (200, 0)), ((1, 0), (1, 50)), ((200, 0), (200, 50)), ((1, 50), (200, 50)), ((200, 50), (100000, 100))):
        assert (by[high][..., 2] <= by[low][..., 2]).all() and (by[high][..., 3] <= by[low][..., 3]).all()
        assert (by[high][..., 2] < by[low][..., 2]).any()
    # drop 0 with gap 0 equals the plain sweep, beside settings that differ from it
    thr = MODEL_THRESHOLDS
    scores, ev = se.score_sweep_host([p], CH, thr, EVAL_MIN_LENGTHS, fps, index, offset_drops=[0.0, 0.1], min_gaps=[0.0, 0.3],
                                     events=(200, 50))
    assert ev.shape == scores.shape == (1, 4, 2, 2, 3, 7)
    at = [EVAL_THRESHOLDS.index(t) for t in thr]
    assert np.array_equal(ev[:, :, 0, 0], by[(200, 50)][:, at])
    assert (ev[:, :, 1, 1, :, 4] != ev[:, :, 0, 0, :, 4]).any()
    assert (ev[..., 2] <= ev[..., 1]).all() and (ev[..., 4] >= ev[..., 1]).all() and (ev[..., 3] <= scores[..., 1]).all()


def _index(rows, length=10.0, part="fe001"):
    import sweep_eval as se
    full = [{"meeting_id": M, "part_id": "fe001", "chan": "chan0", "start": s, "end": e, "length": e - s, "type": k,
             "laugh_type": "laugh" if k == "laugh" else None} for k, s, e in rows]
    chans = [{"meeting_id": M, "part_id": part, "chan": "chan0", "length": length}]
    return se.TranscriptIndex(full, chans), em.EventModel(full, chans, 30000)


def _both(index, model, spans, crit=(1, 0)):
    import sweep_eval as se
    got = se.event_scores_instances({"k": spans}, index, M, "chan0", *crit)["k"]
    assert got == model.score(spans, M, "chan0", *crit), (spans, crit)
    return list(got)


def test_hand_made_cases():
    import sweep_eval as se
    index, model = _index([("laugh", 2.0, 3.0)])
    assert index.scoring_sets(M, "chan0")[1].tolist() == [[2000, 3000]]
    # b == lo: no link; b == lo + 1: a link of 1 ms
    assert _both(index, model, [(1.5, 2.0)]) == [1, 0, 0, 0, 0, 0, 0]
    assert _both(index, model, [(1.5, 2.001)]) == [1, 1, 1, 1, 1, 500, 999]
    assert _both(index, model, [(1.5, 2.001)], (2, 0)) == [1, 1, 0, 0, 1, 0, 0]
    # a == hi - 1: a link of 1 ms; a == hi: none
    assert _both(index, model, [(2.999, 3.5)]) == [1, 1, 1, 1, 1, 999, 500]
    assert _both(index, model, [(3.0, 3.5)]) == [1, 0, 0, 0, 0, 0, 0]
    # a prediction with a == b overlaps nothing, between two that do: it is neither the first nor the last link
    assert _both(index, model, [(2.5, 2.5)]) == [1, 0, 0, 0, 0, 0, 0]
    assert _both(index, model, [(2.1, 2.2), (2.5, 2.5), (2.7, 2.8)]) == [1, 1, 1, 2, 2, 100, 200]
    assert _both(index, model, [(2.5, 2.5), (2.7, 2.8), (2.9, 2.9)]) == [1, 1, 1, 1, 1, 700, 200]
    # the percentages: 500 of 1000 ms is 50 per cent of the event, the prediction lies half in LAUGH
    assert _both(index, model, [(2.5, 3.5)], (500, 50)) == [1, 1, 1, 1, 1, 500, 500]
    assert _both(index, model, [(2.5, 3.5)], (501, 50)) == [1, 1, 0, 0, 1, 0, 0]
    assert _both(index, model, [(2.5, 3.5)], (500, 51)) == [1, 1, 0, 0, 1, 0, 0]
    assert _both(index, model, [(2.0, 2.2), (2.4, 2.7), (3.0, 3.1)], (500, 50)) == [1, 1, 1, 0, 2, 0, 300]     # the event is hit, no piece is
    assert _both(index, model, [(2.0, 2.2), (2.4, 2.7), (3.0, 3.1)], (200, 50)) == [1, 1, 1, 2, 2, 0, 300]
    # a track without runs
    assert _both(index, model, []) == [1, 0, 0, 0, 0, 0, 0]
    # a 1 ms event (what INVALID leaves of a laugh)
    index, model = _index([("laugh", 2.0, 2.3), ("invalid", 2.001, 2.3)])
    assert index.scoring_sets(M, "chan0")[1].tolist() == [[2000, 2001]]
    assert _both(index, model, [(1.0, 2.0), (2.0, 2.001), (2.001, 3.0)], (1, 100)) == [1, 1, 1, 1, 1, 0, 0]
    assert _both(index, model, [(1.0, 2.0), (2.001, 3.0)]) == [1, 0, 0, 0, 0, 0, 0]
    assert _both(index, model, [(1.0, 4.0)], (1, 100)) == [1, 1, 1, 0, 1, 1000, 1999]
    # one prediction over five events; the events are merged intervals, not rows: two adjacent rows are one event
    index, model = _index([("laugh", 1.0 * i, 1.0 * i + 0.3) for i in range(1, 6)] + [("laugh", 5.3, 5.6)])
    assert len(index.scoring_sets(M, "chan0")[1]) == 5
    assert _both(index, model, [(0.5, 5.5)]) == [5, 5, 5, 1, 5, 500 + 1500 + 2500 + 3500 + 4500, 4200 + 3200 + 2200 + 1200 + 100]
    assert _both(index, model, [(0.5, 5.5)], (1, 34)) == [5, 5, 5, 1, 5, 12500, 10900]          # 1700 of 5000 ms in LAUGH
    assert _both(index, model, [(0.5, 5.5)], (1, 35)) == [5, 5, 5, 0, 5, 12500, 10900]
    # one event under 70 fragments
    index, model = _index([("laugh", 1.0, 9.0)])
    spans = [(1.0 + 0.1 * i, 1.0 + 0.1 * i + 0.05) for i in range(70)]
    assert _both(index, model, spans, (50, 40)) == [1, 1, 1, 70, 70, 0, 1050]                   # 3500 of 8000 ms
    assert _both(index, model, spans, (50, 50)) == [1, 1, 0, 70, 70, 0, 0]
    assert _both(index, model, spans, (51, 40)) == [1, 1, 1, 0, 70, 0, 1050]
    # an event wholly inside INVALID-trimmed laughter
    index, model = _index([("laugh", 2.0, 4.0), ("invalid", 2.0, 2.5), ("invalid", 3.0, 4.0)])
    assert index.scoring_sets(M, "chan0")[1].tolist() == [[2500, 3000]]
    assert _both(index, model, [(2.2, 3.5)], (500, 100)) == [1, 1, 1, 1, 1, 300, 500]           # 1300 ms, 500 outside INVALID
    assert _both(index, model, [(2.0, 2.5), (3.0, 4.0)]) == [1, 0, 0, 0, 0, 0, 0]
    # a channel without laughs, and one without a participant
    index, model = _index([("speech", 1.0, 2.0), ("invalid", 3.0, 4.0)])
    assert _both(index, model, [(0.5, 5.5)]) == [0] * 7
    index, model = _index([("laugh", 2.0, 3.0)], part=None)
    assert _both(index, model, [(0.5, 5.5)]) == [0] * 7
    # refused criteria
    for bad in ((-1, 0), (1, -1), (1, 101)):
        with pytest.raises(ValueError):
            se.event_scores_instances({"k": []}, index, M, "chan0", *bad)
    with pytest.raises(TypeError):
        se.event_scores_instances({"k": []}, index, M, "chan0", 1.5, 0)


def test_event_rows_and_sum_stats():
    import sweep_eval as se
    assert se.EVENT_FIELDS == ("n_ref", "ref_touched", "ref_hit", "pred_hit", "links", "onset_abs_ms", "offset_abs_ms")
    assert se.EVENT_COLUMNS == ["meeting", "threshold", "min_len", "event_precision", "event_recall", "event_f1", "num_ref_events",
                                "ref_events_touched", "ref_events_hit", "valid_pred_laughs", "pred_laughs_hit", "links",
                                "fragments_per_touched_event", "mean_onset_err", "mean_offset_err"]
    assert se.EVENT_COLUMNS_BINARIZE == se.EVENT_COLUMNS[:3] + ["offset_drop", "min_gap"] + se.EVENT_COLUMNS[3:]
    assert se.EVENT_SUM_COLUMNS == se.EVENT_COLUMNS[1:] and se.EVENT_SUM_COLUMNS_BINARIZE == se.EVENT_COLUMNS_BINARIZE[1:]
    rows = [{"meeting_id": m, "part_id": p, "chan": c, "start": 1.0, "end": 2.0, "length": 1.0, "type": "laugh", "laugh_type": "laugh"}
            for m, p, c in (("Bmr001", "fe001", "chan0"), ("Bmr001", "me002", "chan3"), ("Bed002", "mn003", "chan1"))]
    chans = [{"meeting_id": "Bmr001", "part_id": "fe001", "chan": "chan0", "length": 10.0},
             {"meeting_id": "Bmr001", "part_id": "me002", "chan": "chan3", "length": 10.0},
             {"meeting_id": "Bmr001", "part_id": "", "chan": "chan5", "length": 10.0},
             {"meeting_id": "Bed002", "part_id": "mn003", "chan": "chan1", "length": 10.0}]
    index = se.TranscriptIndex(rows, chans)
    channels = [("Bmr001", "chan0"), ("Bmr001", "chan5"), ("Bed002", "chan1"), ("Bmr001", "chan3")]
    thresholds, min_lengths = [0.2, 0.8], [0.0]
    scores, events = np.zeros((4, 2, 1, 7), np.int64), np.zeros((4, 2, 1, 7), np.int64)
    scores[:, 0, 0, 1] = [4, 99, 0, 6]                    # n_valid; the channel without a participant is left out
    events[:, 0, 0] = [[3, 2, 1, 2, 5, 700, 100], [9, 9, 9, 9, 9, 9, 9], [0, 0, 0, 0, 0, 0, 0], [5, 3, 2, 3, 4, 301, 201]]
    events[:, 1, 0] = [[3, 0, 0, 0, 0, 0, 0], [0] * 7, [2, 1, 0, 0, 1, 0, 0], [5, 0, 0, 0, 0, 0, 0]]
    scores[:, 1, 0, 1] = [0, 0, 3, 0]
    got = se.event_rows(scores, events, channels, thresholds, min_lengths, index)
    assert [r[:3] for r in got] == [["Bed002", 0.2, 0.0], ["Bed002", 0.8, 0.0], ["Bmr001", 0.2, 0.0], ["Bmr001", 0.8, 0.0]]
    assert all(len(r) == len(se.EVENT_COLUMNS) for r in got)
    nan = math.isnan
    # no event, no valid prediction: precision 1, recall NaN, F1 NaN, fragments NaN, errors NaN
    r = got[0]
    assert r[3] == 1 and nan(r[4]) and nan(r[5]) and r[6:12] == [0] * 6 and all(nan(v) for v in r[12:])
    # valid predictions, none hit, no event hit: 0, 0, F1 0; one touched event with one link; no hit event: errors NaN
    r = got[1]
    assert r[3:6] == [0.0, 0.0, 0.0] and r[6:12] == [2, 1, 0, 3, 0, 1] and r[12] == 1.0 and nan(r[13]) and nan(r[14])
    # the participants' integers are summed first, then one division per figure
    r = got[2]
    p, rec = 5 / 10, 3 / 8
    assert r[3:6] == [p, rec, 2 * p * rec / (p + rec)] and r[6:12] == [8, 5, 3, 10, 5, 9]
    assert r[12:] == [9 / 5, 1001 / 3000.0, 301 / 3000.0]
    # no valid prediction but events: precision 1, recall 0
    r = got[3]
    assert r[3] == 1 and r[4] == 0.0 and r[5] == 0.0 and nan(r[12]) and nan(r[13])
    # over all meetings, from the summed integers, ordered by (min_len, threshold)
    stats = se.event_sum_stats(got)
    assert [s[:2] for s in stats] == [[0.2, 0.0], [0.8, 0.0]] and all(len(s) == len(se.EVENT_SUM_COLUMNS) for s in stats)
    assert stats[0][2:] == got[2][3:]                                                     # (Bed002 adds nothing at 0.2)
    assert stats[1][2:5] == [0 / 3, 0 / 10, 0.0] and stats[1][5:11] == [10, 1, 0, 3, 0, 1] and stats[1][11] == 1.0
    # the millisecond sums come back from the rows' means: two meetings with hits
    events[2, 0, 0] = [2, 2, 2, 1, 3, 1234567, 7]
    scores[2, 0, 0, 1] = 1
    got = se.event_rows(scores, events, channels, thresholds, min_lengths, index)
    s = se.event_sum_stats(got)[0]
    assert s[5:11] == [10, 7, 5, 11, 6, 12] and s[12:] == [(1001 + 1234567) / 5000.0, (301 + 7) / 5000.0]
    # the binarize axes: offset_drop and min_gap behind min_len, grouped by all four
    sc, ev = np.zeros((4, 2, 1, 2, 1, 7), np.int64), np.zeros((4, 2, 1, 2, 1, 7), np.int64)
    sc[:, :, 0, 1], ev[:, :, 0, 1] = scores, events
    got = se.event_rows(sc, ev, channels, thresholds, min_lengths, index, offset_drops=[0.1], min_gaps=[0.0, 0.3])
    assert len(got) == 8 and all(len(r) == len(se.EVENT_COLUMNS_BINARIZE) for r in got)
    assert got[1][:5] == ["Bed002", 0.2, 0.0, 0.1, 0.3] and got[1][8:14] == [2, 2, 2, 1, 1, 3]
    stats = se.event_sum_stats(got, binarize=True)
    assert len(stats) == 4 and stats[1][:4] == [0.2, 0.0, 0.1, 0.3] and stats[1][4:] == s[2:]
    with pytest.raises(ValueError):
        se.event_rows(scores, events[:, :1], channels, thresholds, min_lengths, index)


def test_evaluate_sweep_flags_and_host_run(tmp_path):
    import evaluate_sweep
    import sweep_eval as se
    parser = evaluate_sweep.build_parser()
    base = ["--probs_dir", "p", "--transcripts", "t.csv", "--channels", "c.csv", "--out_dir", "o"]
    args = parser.parse_args(base)
    assert (args.events, args.event_min_overlap_ms, args.event_min_overlap_pct) == (False, 1, 0)
    args = parser.parse_args(base + ["--events", "--event_min_overlap_ms", "0", "--event_min_overlap_pct", "100"])
    assert (args.events, args.event_min_overlap_ms, args.event_min_overlap_pct) == (True, 0, 100)
    for bad in (["--event_min_overlap_pct", "101"], ["--event_min_overlap_pct", "-1"], ["--event_min_overlap_ms", "-1"],
                ["--event_min_overlap_ms", "1.5"]):
        with pytest.raises(SystemExit):
            parser.parse_args(base + bad)
    args = sm.write_corpus(tmp_path)
    evaluate_sweep.main(args + ["--out_dir", str(tmp_path / "plain")])
    evaluate_sweep.main(args + ["--events", "--event_min_overlap_ms", "100", "--event_min_overlap_pct", "20", "--out_dir",
                                str(tmp_path / "events")])
    assert sorted(os.listdir(tmp_path / "plain")) == ["eval_df_per_meeting.csv", "sum_stats.csv"]
    assert sorted(os.listdir(tmp_path / "events")) == ["eval_df_per_meeting.csv", "event_df_per_meeting.csv", "event_sum_stats.csv",
                                                       "sum_stats.csv"]
    for f in os.listdir(tmp_path / "plain"):
        assert open(tmp_path / "plain" / f, "rb").read() == open(tmp_path / "events" / f, "rb").read()
    rows = list(csv.reader(open(tmp_path / "events" / "event_df_per_meeting.csv")))
    assert rows[0] == se.EVENT_COLUMNS and len(rows) == 1 + 2 * 3 * 2
    assert [r[0] for r in rows[1:]] == ["Bed002"] * 6 + ["Bmr001"] * 6
    assert all(int(r[6]) > 0 for r in rows[1:]) and any(int(r[8]) > 0 and 0 < float(r[3]) < 1 and float(r[12]) > 1 for r in rows[1:])
    valid = [r[9] for r in csv.reader(open(tmp_path / "events" / "eval_df_per_meeting.csv"))][1:]
    assert [r[9] for r in rows[1:]] == valid                                              # valid_pred_laughs: the time scorer's
    stats = list(csv.reader(open(tmp_path / "events" / "event_sum_stats.csv")))
    assert stats[0] == se.EVENT_SUM_COLUMNS and len(stats) == 1 + 6
    for s in stats[1:]:
        sel = [r for r in rows[1:] if r[1:3] == s[:2]]
        assert [int(s[i]) for i in range(5, 11)] == [sum(int(r[i + 1]) for r in sel) for i in range(5, 11)]
    # with the binarize flags: two more columns
    evaluate_sweep.main(args + ["--events", "--offset_drops", "0,0.1", "--min_gaps", "0.2", "--out_dir", str(tmp_path / "binarize")])
    rows = list(csv.reader(open(tmp_path / "binarize" / "event_df_per_meeting.csv")))
    assert rows[0] == se.EVENT_COLUMNS_BINARIZE and len(rows) == 1 + 2 * 3 * 2 * 2
    assert list(csv.reader(open(tmp_path / "binarize" / "event_sum_stats.csv")))[0] == se.EVENT_SUM_COLUMNS_BINARIZE


def test_event_size_query_needs_no_gpu():
    import _hip
    lib = _hip.lib()
    lmax, kmax = lib.lad_score_max_min_lengths(), lib.lad_runs_max_thresholds()
    query = lib.lad_score_events_workspace_bytes
    assert query(1, 0, 1, 1, 0) > 0
    small, big = query(1, 1000, 29, 3, 5000), query(10, 100000, 29, 3, 500000)
    assert 0 < small < big and big >= 4 * 100000 + 8 * 10 * 29 + 12 * 500000
    assert query(1, 1000, 29, 3, 5001) >= small + 12 - 3 * 256 and query(1, 1000, 29, 3, 5000 + 64) > small
    assert query(65535, 1 << 20, kmax, lmax, 1 << 38) > 12 * (1 << 38)
    for bad in ((0, 10, 1, 1, 5), (65536, 10, 1, 1, 5), (1, -1, 1, 1, 5), (1, (1 << 30) + 1, 1, 1, 5), (1, 10, 0, 1, 5),
                (1, 10, kmax + 1, 1, 5), (1, 10, 1, 0, 5), (1, 10, 1, lmax + 1, 5), (1, 10, 1, 1, -1), (1, 10, 1, 1, (1 << 38) + 1)):
        assert query(*bad) == -1
        assert b"lad_score_events_workspace_bytes" in lib.lad_last_error()
    assert _hip.SIGNATURES["lad_score_events"][1][15:17] == [_hip.c_i32, _hip.c_i32]
