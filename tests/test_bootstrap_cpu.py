"""CPU tests of the bootstrap intervals (bootstrap.py, sweep_eval.bootstrap_sum_stats_host, evaluate_sweep.py --bootstrap): the host
form against tests/_bootstrap_model.py, a second implementation of the convention in include/lad_hip.h in Python integers and
fractions.  Everything is integers and single IEEE divisions, so every comparison but one is equality; the exception is the point
figures against calc_sum_stats, whose sums run in float seconds."""
import csv
import os

import numpy as np
import pytest

import _bootstrap_model as model
import _score_model as sm
from oracle import recipe

GS, BS = [1, 2, 7, 20], [1, 2, 64]
THRESHOLDS, MIN_LENGTHS = [0.25, 0.5, 0.75], [0.0, 0.2]


def _same(a, b):
    """Equal rows, NaN matching NaN."""
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        assert len(ra) == len(rb), (ra, rb)
        for va, vb in zip(ra, rb):
            assert va == vb or (va != va and vb != vb), (ra, rb)
            assert type(va) is type(vb) or {type(va), type(vb)} <= {int, float}, (ra, rb)


def _index(transc_ms, n_meetings=3):
    """One channel per entry of transc_ms, spread over n_meetings meetings, each with one laugh row of that many milliseconds (at
    least 200: a shorter one is filed under INVALID), and one channel without a participant."""
    import sweep_eval as se
    rows, chans, channels = [], [], []
    for g, ms in enumerate(transc_ms):
        m, part, chan = f"M{g % n_meetings}", f"p{g:02d}", f"chan{g}"
        chans.append({"meeting_id": m, "part_id": part, "chan": chan, "length": 100.0})
        channels.append((m, chan))
        assert ms == 0 or ms >= 200
        if ms:
            rows.append({"meeting_id": m, "part_id": part, "chan": chan, "start": 1.0, "end": 1.0 + ms / 1000, "length": ms / 1000,
                         "type": "laugh", "laugh_type": "laugh"})
    chans.append({"meeting_id": "M0", "part_id": None, "chan": "chanX", "length": 100.0})
    channels.insert(1 if len(channels) > 1 else 0, ("M0", "chanX"))                # (not the last one: unit numbers skip it)
    return se.TranscriptIndex(rows, chans), channels


def _scores(seed, C, shape=(len(THRESHOLDS), len(MIN_LENGTHS)), zero_pred=False):
    """Seeded score and event arrays (C, *shape, 7) with corr_ms <= pred_ms, pred_hit <= n_valid, ref_hit <= n_ref."""
    rng = np.random.default_rng(seed)
    scores = rng.integers(0, 50, (C, *shape, 7))
    scores[..., 2] = 0 if zero_pred else rng.integers(0, 400_000, (C, *shape))
    scores[..., 3] = (scores[..., 2] * rng.random((C, *shape))).astype(np.int64)
    scores[..., 1] = rng.integers(0, 30, (C, *shape)) * (rng.random((C, *shape)) < 0.8)
    events = rng.integers(0, 50, (C, *shape, 7))
    events[..., 0] = rng.integers(0, 12, (C, 1, 1))                                # n_ref: a property of the channel
    events[..., 2] = (events[..., 0] * rng.random((C, *shape))).astype(np.int64)
    events[..., 3] = (scores[..., 1] * rng.random((C, *shape))).astype(np.int64)
    return scores.astype(np.int64), events.astype(np.int64)


def _model_rows(scores, events, channels, index, unit_of, transc, B, seed, level):
    """The rows of the model in calc_sum_stats' order, from the per-channel arrays."""
    G = len(transc)
    w = model.weights(G, B, seed)
    time_rows, event_rows, valids = [], [], []
    for l, min_l in enumerate(MIN_LENGTHS):
        for k, thr in enumerate(THRESHOLDS):
            t_cells, e_cells = [[0, 0] for _ in range(G)], [[0, 0, 0, 0] for _ in range(G)]
            for c, g in enumerate(unit_of):
                if g < 0:
                    continue
                s, e = scores[c, k, l].tolist(), events[c, k, l].tolist()
                t_cells[g] = [t_cells[g][0] + s[2], t_cells[g][1] + s[3]]
                e_cells[g] = [a + b for a, b in zip(e_cells[g], (s[1], e[3], e[2], e[0]))]
            row, valid = model.time_row([tuple(c) for c in t_cells], transc, w, level)
            time_rows.append([thr, min_l] + row)
            valids.append(valid)
            event_rows.append([thr, min_l] + model.event_row(e_cells, w, level))
    return time_rows, event_rows, valids


def test_weights_are_the_models_and_sum_to_the_unit_count():
    import bootstrap
    for seed, b in ((0, 0), (0x123456789ABCDEF0, 77)):
        want = model.draw_words(seed, b, 0)
        got = bootstrap.philox4x32_10([0], [b], [0], [model.TAG], seed & 0xFFFFFFFF, seed >> 32)
        assert [int(v[0]) for v in got] == list(want)
        # ... and the first draws of that replicate are those words under mulhi
        row = bootstrap.weights_host(1000, b + 1, seed)[b]
        counted = np.zeros(1000, np.int64)
        for i in range(4):
            counted[(want[i] * 1000) >> 32] += 1
        assert (row >= counted).all()
    for G in (1, 2, 3, 7, 63, 64, 65, 450):
        for B, seed in ((1, 0), (5, 3), (64, 2 ** 63 + 5)):
            w = bootstrap.weights_host(G, B, seed)
            assert w.dtype == np.int32 and w.shape == (B, G) and (w.sum(axis=1) == G).all() and (w >= 0).all()
            if G <= 65:
                assert w.tolist() == model.weights(G, B, seed)
    assert bootstrap.weights_host(7, 4, 1).tolist() != bootstrap.weights_host(7, 4, 2).tolist()
    assert bootstrap.weights_host(7, 9, 1)[:4].tolist() == bootstrap.weights_host(7, 4, 1).tolist()    # a pure function of (seed, b, G)
    for G, B in ((0, 1), (4097, 1), (1, 0), (1, 4097)):
        with pytest.raises(ValueError):
            bootstrap.weights_host(G, B, 0)


@pytest.mark.parametrize("G", GS)
def test_host_form_is_the_model(G):
    import sweep_eval as se
    transc = [0 if g % 5 == 3 else 200 + 137 * g for g in range(G)]
    index, channels = _index(transc)
    scores, events = _scores(100 + G, len(channels))
    for unit in ("channel", "meeting"):
        unit_of, unit_ms = se.bootstrap_units(channels, index, unit)
        assert unit_of[channels.index(("M0", "chanX"))] == -1 and sorted(set(unit_of) - {-1}) == list(range(len(unit_ms)))
        if unit == "channel":
            assert unit_ms == transc and [g for g in unit_of if g >= 0] == list(range(G))
        else:
            assert unit_ms == [sum(t for g, t in enumerate(transc) if g % 3 == m) for m in range(min(G, 3))]
        for B in BS:
            got, got_ev = se.bootstrap_sum_stats_host(scores, channels, THRESHOLDS, MIN_LENGTHS, index, n_boot=B, seed=9, level=90, unit=unit,
                                                      events=events)
            want, want_ev, _ = _model_rows(scores, events, channels, index, unit_of, unit_ms, B, 9, 90)
            _same(got, want)
            _same(got_ev, want_ev)
            _same(se.bootstrap_sum_stats_host(scores, channels, THRESHOLDS, MIN_LENGTHS, index, n_boot=B, seed=9, level=90, unit=unit), got)
            if len(unit_ms) == 1:                                                  # one unit: every interval collapses onto the point figure
                for r in got:
                    assert r[2] == r[3] == r[4] and r[-1] == B
                    assert r[5] == r[6] == r[7] and r[8] == r[9] == r[10]


def test_zero_predicted_time_is_precision_one():
    import sweep_eval as se
    index, channels = _index([300, 450, 250, 900])
    scores, _ = _scores(5, len(channels), zero_pred=True)
    for r in se.bootstrap_sum_stats_host(scores, channels, THRESHOLDS, MIN_LENGTHS, index, n_boot=64, seed=1):
        assert r[2:5] == [1.0, 1.0, 1.0] and r[5:8] == [0.0, 0.0, 0.0] and r[8:11] == [0.0, 0.0, 0.0] and r[11] == 64


def test_replicates_without_transcribed_laughter_are_invalid_for_recall_and_f1():
    import sweep_eval as se
    B, transc = 64, [0, 0, 700, 0]
    index, channels = _index(transc)
    scores, events = _scores(6, len(channels))
    unit_of, unit_ms = se.bootstrap_units(channels, index)
    want, _, valids = _model_rows(scores, events, channels, index, unit_of, unit_ms, B, 4, 95)
    n_invalid = sum(1 for row in model.weights(4, B, 4) if row[2] == 0)
    assert 1 <= n_invalid <= B - 1                                                 # (the model itself: some replicate misses unit 2)
    for valid in valids:
        assert valid == [B, B - n_invalid, B - n_invalid]                          # F1 is invalid exactly where recall is
    got = se.bootstrap_sum_stats_host(scores, channels, THRESHOLDS, MIN_LENGTHS, index, n_boot=B, seed=4)
    _same(got, want)
    assert all(r[-1] == B - n_invalid for r in got)
    # nothing transcribed at all: recall and F1 are NaN throughout, with no valid replicate
    index0, channels0 = _index([0, 0, 0])
    for r in se.bootstrap_sum_stats_host(_scores(7, len(channels0))[0], channels0, THRESHOLDS, MIN_LENGTHS, index0, n_boot=8):
        assert all(v != v for v in r[5:11]) and r[-1] == 0 and all(v == v for v in r[2:5])


def test_ties_go_to_the_lowest_replicate():
    import bootstrap
    import sweep_eval as se
    # every replicate has the value 1/2, as the pair (b + 1, 2 b + 2): rank r is replicate r
    B = 40
    sums = np.array([[b + 1, 2 * b + 2] for b in range(B)], np.int64)
    out, valid = bootstrap.select_host(sums, [(0, 1, 1, -1, -1, 0)], [(1, 40), (1, 2), (39, 40)])
    assert valid.tolist() == [B] and out[0].tolist() == [[1, 2], [20, 40], [39, 78]]
    assert model.quantiles(sums.tolist(), [(0, 1, 1, -1, -1, 0)], [(1, 40), (1, 2), (39, 40)])[0][0] == [(1, 2), (20, 40), (39, 78)]
    # all units equal: every replicate has the same sums, and the pair is that of replicate 0 -- the unit sums themselves
    index, channels = _index([400] * 5)
    scores, _ = _scores(8, 1)
    scores = np.repeat(scores, len(channels), axis=0)
    for r in se.bootstrap_sum_stats_host(scores, channels, THRESHOLDS, MIN_LENGTHS, index, n_boot=16, seed=2):
        assert r[2] == r[3] == r[4] and r[5] == r[6] == r[7] and r[8] == r[9] == r[10] and r[-1] == 16


def test_point_figures_against_calc_sum_stats():
    import sweep_eval as se
    rows = sm.make_rows(11, "Bmr001", ["fe001", "me002"], 30.0, n_per_type=15) + sm.make_rows(12, "Bed002", ["mn003"], 30.0, n_per_type=15)
    chans = [{"meeting_id": "Bmr001", "part_id": "fe001", "chan": "chan0", "length": 30.0},
             {"meeting_id": "Bmr001", "part_id": "me002", "chan": "chan3", "length": 29.317},
             {"meeting_id": "Bmr001", "part_id": "", "chan": "chan5", "length": 30.0},
             {"meeting_id": "Bed002", "part_id": "mn003", "chan": "chan1", "length": 25.0049375}]
    part_chan = {(c["meeting_id"], c["part_id"]): c["chan"] for c in chans}
    rows = [dict(r, chan=part_chan[(r["meeting_id"], r["part_id"])]) for r in rows]
    index = se.TranscriptIndex(rows, chans)
    channels = [("Bmr001", "chan0"), ("Bmr001", "chan3"), ("Bmr001", "chan5"), ("Bed002", "chan1")]
    tracks = [recipe.make_prob_track(30 + i, 3000 - 100 * i) for i in range(4)]
    for m in index.meetings:                                                       # laugh_ms is the integer behind tot_len
        assert index.laugh_ms(m) == sum(index.laugh_ms(m, p) for p in {r["part_id"] for r in rows if r["meeting_id"] == m})
        assert abs(index.laugh_ms(m) / 1000 - index.tot_len(m, "laugh")) <= 1e-9 and index.laugh_ms(m) > 0
    assert index.laugh_ms("Bmr001", "nobody") == 0
    thresholds = [0.1, 0.3, 0.5, 0.7, 0.9]
    scores = se.score_sweep_host(tracks, channels, thresholds, MIN_LENGTHS, 100.0, index)
    want = se.calc_sum_stats(se.eval_rows(scores, channels, thresholds, MIN_LENGTHS, index))
    got = se.bootstrap_sum_stats_host(scores, channels, thresholds, MIN_LENGTHS, index, n_boot=4)
    bound = (len(channels) + 4) * 2.0 ** -52                                      # the rounding of the float-second sums on the reference's route
    assert len(got) == len(want) and any(r[2] < 1 for r in got)
    for g, w in zip(got, want):
        assert g[:2] == w[:2]
        assert abs(g[2] - w[2]) <= bound * abs(w[2]) and abs(g[5] - w[3]) <= bound * abs(w[3])
        # F1 = 2 corr / (pred + transc) is 2PR / (P + R) by algebra: P and R carry the bound above (F1 moves by at most as much,
        # relatively), and the float form adds four roundings; F1 <= 1, so relative and absolute bounds coincide here
        f1 = 0.0 if w[2] + w[3] == 0 else 2 * w[2] * w[3] / (w[2] + w[3])
        assert abs(g[8] - f1) <= bound + 4 * 2.0 ** -52


def test_quantile_ranks_and_levels():
    import bootstrap
    assert bootstrap.quantile_pairs(95) == [(1, 40), (39, 40)] == model.level_quantiles(95)
    assert [bootstrap.rank_of(*q, 2000) for q in bootstrap.quantile_pairs(95)] == [49, 1949]
    assert [model.rank(*q, 2000) for q in bootstrap.quantile_pairs(95)] == [49, 1949]
    assert bootstrap.quantile_pairs("99.9") == [(1, 2000), (1999, 2000)]
    assert bootstrap.rank_of(1, 2000, 2000) == 0 and bootstrap.rank_of(1999, 2000, 2000) == 1998
    assert bootstrap.rank_of(1, 40, 1) == 0 == bootstrap.rank_of(39, 40, 1) and bootstrap.rank_of(39, 40, 2) == 1
    for v in range(1, 70):
        for q in ((1, 40), (39, 40), (1, 3), (1, 2)):
            assert bootstrap.rank_of(*q, v) == model.rank(*q, v) < v
    for bad in (0, 100, 101, -5, "x"):
        with pytest.raises((ValueError, ZeroDivisionError)):
            bootstrap.quantile_pairs(bad)


def test_select_host_is_the_model_on_seeded_sums():
    import bootstrap
    rng = np.random.default_rng(3)
    figures = [(0, 1, 1, -1, -1, 1), (0, 1, 1, -1, -1, 0), (0, 2, 1, 2, 2, 0), (3, 1, 2, -1, 1, 1)]
    for B in (1, 2, 63, 200):
        sums = rng.integers(0, 2 ** 52, (B, 4))
        sums[rng.random((B, 4)) < 0.3] = 0                                         # zero denominators and zero validity columns
        sums[:, 3] = sums[:, 3] % 7                                                # ... and many ties
        for qs in ([(1, 2)], [(1, 40), (39, 40)], [(1, 1000), (1, 4), (1, 2), (3, 4), (999, 1000)]):
            out, valid = bootstrap.select_host(sums, figures, qs)
            want, want_valid = model.quantiles(sums.tolist(), figures, qs)
            assert valid.tolist() == want_valid and out.tolist() == [[list(p) for p in f] for f in want]
    with pytest.raises(ValueError):
        bootstrap.check_matrix(np.array([[1, 2 ** 40]]))
    with pytest.raises(ValueError):
        bootstrap.check_matrix(np.array([[-1, 5]]))
    assert bootstrap.check_matrix([[0, 2 ** 40 - 1]]).dtype == np.int64


def test_entry_points_refuse_without_a_gpu():
    import ctypes

    import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import importlib.util
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        spec = importlib.util.spec_from_file_location("lad_build", os.path.join(root, "laughter-detection-icsi_amd", "build.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.build(verbose=False)
    lib = _hip.lib()
    assert lib.lad_bootstrap_max_units() == 4096 == lib.lad_bootstrap_max_replicates()
    null, one = ctypes.c_void_p(0), (ctypes.c_int32 * 1)(1)
    assert lib.lad_bootstrap_weights(0, 1, 0, null, null) == _hip.LAD_ERR_INVALID and b"lad_bootstrap_weights" in lib.lad_last_error()
    assert lib.lad_bootstrap_weights(4, 4, 0, null, null) == _hip.LAD_ERR_INVALID
    assert lib.lad_bootstrap_sums(null, null, 4, 4, 4, null, null) == _hip.LAD_ERR_INVALID and b"lad_bootstrap_sums" in lib.lad_last_error()
    assert lib.lad_bootstrap_quantiles(null, 4, 4, null, None, 1, one, one, 1, null, null, null) == _hip.LAD_ERR_INVALID
    assert b"lad_bootstrap_quantiles" in lib.lad_last_error()


def _files(path):
    return {f: open(path / f, "rb").read() for f in sorted(os.listdir(path))}


def test_evaluate_sweep_bootstrap_under_the_host_scorer(tmp_path):
    import evaluate_sweep
    import sweep_eval as se
    args = sm.write_corpus(tmp_path)
    at = args.index("--thresholds")
    no_list = args[:at] + args[at + 2:]
    boot = ["--bootstrap", "16", "--bootstrap_seed", "3"]
    variants = {"plain": (args, ["sum_stats_ci.csv"], se.SUM_CI_COLUMNS),
                "events": (args + ["--events"], ["event_sum_stats_ci.csv", "sum_stats_ci.csv"], se.SUM_CI_COLUMNS),
                "penalties": (args + ["--penalties", "0.0,2.0"], ["sum_stats_ci.csv"], se.columns(se.SUM_CI_COLUMNS, se.ls.VITERBI)),
                "event_grid": (no_list + ["--event_grid", "8"], ["event_sum_stats_ci.csv", "sum_stats_ci.csv"], se.SUM_CI_COLUMNS)}
    for name, (base, new, header) in variants.items():
        evaluate_sweep.main(base + ["--out_dir", str(tmp_path / name)])
        evaluate_sweep.main(base + boot + ["--out_dir", str(tmp_path / (name + "_ci"))])
        evaluate_sweep.main(base + boot + ["--out_dir", str(tmp_path / (name + "_ci2"))])
        before, after = _files(tmp_path / name), _files(tmp_path / (name + "_ci"))
        assert sorted(after) == sorted(list(before) + new), name
        assert {k: after[k] for k in before} == before, name                      # the files of a call without the flag, byte for byte
        assert after == _files(tmp_path / (name + "_ci2")), name                  # same seed, same bytes
        table = list(csv.reader(open(tmp_path / (name + "_ci") / "sum_stats_ci.csv")))
        stats = list(csv.reader(open(tmp_path / name / "sum_stats.csv")))
        assert table[0] == header and len(table) == len(stats)
        n_keys = len(header) - 10
        for r, s in zip(table[1:], stats[1:]):
            assert r[:n_keys] == s[:n_keys]
            p, lo, hi = (float(v) for v in r[n_keys:n_keys + 3])
            assert lo <= hi and 0 <= lo and hi <= 1 and abs(p - float(s[n_keys])) < 1e-12 and int(r[-1]) == 16
        if "event_sum_stats_ci.csv" in new:
            ev = list(csv.reader(open(tmp_path / (name + "_ci") / "event_sum_stats_ci.csv")))
            ev_stats = list(csv.reader(open(tmp_path / name / "event_sum_stats.csv")))
            assert ev[0] == se.EVENT_SUM_CI_COLUMNS and len(ev) == len(ev_stats)
            for r, s in zip(ev[1:], ev_stats[1:]):
                assert r[:2] == s[:2] and float(r[2]) == float(s[2]) and float(r[5]) == float(s[3])
    # another seed or unit, other intervals; the point figures stay
    evaluate_sweep.main(args + ["--bootstrap", "16", "--bootstrap_seed", "4", "--out_dir", str(tmp_path / "seed4")])
    evaluate_sweep.main(args + boot + ["--bootstrap_unit", "meeting", "--bootstrap_level", "80", "--out_dir", str(tmp_path / "meeting")])
    ci = _files(tmp_path / "plain_ci")["sum_stats_ci.csv"]
    assert _files(tmp_path / "seed4")["sum_stats_ci.csv"] != ci != _files(tmp_path / "meeting")["sum_stats_ci.csv"]
    for bad in (["--bootstrap", "0"], ["--bootstrap", "4097"], ["--bootstrap", "8", "--bootstrap_level", "100"],
                ["--bootstrap", "8", "--bootstrap_unit", "frame"], ["--bootstrap", "8", "--bootstrap_seed", "-1"]):
        with pytest.raises(SystemExit):
            evaluate_sweep.build_parser().parse_args(args + bad + ["--out_dir", "o"])
