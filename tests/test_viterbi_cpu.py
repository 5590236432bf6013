"""CPU tests of the two-state Viterbi decoder: the specification's own consequences (tests/_viterbi_model.py against brute force),
the host forms of laugh_segmenter.py against that model, the new axis of sweep_eval.py and the command lines, and the size queries
of csrc/viterbi.hip, which need no GPU.  Integer arithmetic: every comparison is an equality."""
import hashlib
import os

import numpy as np
import pytest

import _score_model as sm
import _viterbi_model as vm
from oracle import recipe

M = "Bmr001"
CENTRED = (np.arange(65537, dtype=np.int64) - 32768).astype(np.int32)       # S[u] = u - 32768: a frame's score is chosen directly


def track_of(scores, dtype=np.float64):
    """The track whose frames score exactly `scores` under CENTRED with bias 0 (None: a NaN frame); u / 65536 is exact in float32."""
    return np.array([np.nan if s is None else (s + 32768) / 65536.0 for s in scores], dtype=dtype)


def as_tuples(a):
    return [tuple(int(v) for v in r) for r in a]


def with_nans(p, seed):
    p = p.copy()
    rng = np.random.default_rng(seed)
    p[rng.integers(0, len(p), len(p) // 50)] = np.nan
    return p


def test_model_against_brute_force():
    rng = np.random.default_rng(1)
    seen_tie = 0
    for _ in range(400):
        T = int(rng.integers(1, 13))
        s = [int(v) for v in rng.integers(-4, 5, T)]
        penalty = int(rng.integers(0, 6))
        path, best = vm.decode(s, penalty)
        want = vm.brute_force(s, penalty)
        assert best == want and vm.path_score(path, s, penalty) == want, (s, penalty)
        seen_tie += best == 0
    assert seen_tie > 10


def test_penalty_zero_rule():
    import laugh_segmenter as ls
    rng = np.random.default_rng(2)
    for _ in range(50):
        s = [int(v) for v in rng.integers(-2, 3, int(rng.integers(1, 60)))]
        path, _ = vm.decode(s, 0)
        for t, v in enumerate(s):
            if v > 0:
                assert path[t] == 1
            elif v < 0:
                assert path[t] == 0
            else:
                assert path[t] == (path[t + 1] if t + 1 < len(s) else 0)
        assert as_tuples(ls._viterbi_spans_host(track_of(s), [(0, 0)], CENTRED)[0]) == vm.runs(path)


def test_host_form_against_the_model():
    import laugh_segmenter as ls
    rng = np.random.default_rng(3)
    settings = [(0, 0), (0, 3), (2, 7), (-1, 40), (5, 1 << 26), (-(1 << 24), 0), (1 << 24, 0)]
    n_runs = 0
    for case in range(12):
        T = int(rng.integers(1, 400))
        s = [None if rng.random() < 0.03 else int(v) for v in rng.integers(-6, 7, T)]
        p = track_of(s, np.float32 if case % 2 else np.float64)
        got = ls._viterbi_spans_host(p, settings, CENTRED)
        for (bias, penalty), g in zip(settings, got):
            want, _ = vm.spans(p.tolist(), CENTRED, bias, penalty)
            assert g.dtype == np.int64 and as_tuples(g) == want, (case, bias, penalty)
            assert all(x is not None for a, b in want for x in s[a:b + 1])              # a NaN frame is never on
            n_runs += len(want)
    assert n_runs > 300
    # the default table on a realistic track, through the public forms
    table = ls.viterbi_emission_table()
    p = with_nans(recipe.make_prob_track(5, 3000), 5)
    for thr, pen in ((0.5, 0.0), (0.3, 2.0), (0.9, 4.0), (1.0, 1.0)):
        (bias, penalty), = ls.viterbi_settings([thr], [pen], table)
        want, _ = vm.spans(p.tolist(), table, bias, penalty)
        assert as_tuples(ls.viterbi_frame_spans(p, thr, pen)) == want
        assert as_tuples(ls.viterbi_frame_spans(p, thr, pen, table=table)) == want
    assert len(ls.viterbi_frame_spans(p, 0.5, 4.0)) < len(ls.viterbi_frame_spans(p, 0.5, 0.0))       # the penalty does something
    assert ls.viterbi_frame_spans(np.zeros(0), 0.5, 1.0).shape == (0, 2)
    assert as_tuples(ls.viterbi_frame_spans(np.full(7, np.nan), 0.5, 0.0)) == []
    assert as_tuples(ls.viterbi_frame_spans(np.array([2.0, 1.0, np.nan, -1.0, 0.0, 1.5]), 0.5, 0.0)) == [(0, 1), (5, 5)]


def test_confidence_decides():
    """What the rules in seconds cannot do: a short confident event pays for itself, a long weak one does not, and a gap is bridged
    exactly when the evidence inside it is weaker than the price of a second event."""
    import laugh_segmenter as ls
    s = [-5] * 20 + [40] * 3 + [-5] * 20 + [1] * 30 + [-5] * 20
    assert as_tuples(ls._viterbi_spans_host(track_of(s), [(0, 100)], CENTRED)[0]) == [(20, 22)]
    # a pause that costs 19 or 20 is bridged at a penalty of 20 (a tie goes on), one that costs 21 is not
    for gap, want in ((19, [(10, 58)]), (20, [(10, 59)]), (21, [(10, 19), (41, 60)])):
        s = [-5] * 10 + [30] * 10 + [-1] * gap + [30] * 20 + [-5] * 10
        assert as_tuples(ls._viterbi_spans_host(track_of(s), [(0, 20)], CENTRED)[0]) == want == vm.runs(vm.decode(s, 20)[0]), gap


def test_emission_table_and_settings():
    import laugh_segmenter as ls
    table = ls.viterbi_emission_table()
    assert table.dtype == np.int32 and table.shape == (65537,)
    assert (np.diff(table) >= 0).all() and table[32768] == 0 and np.abs(table + table[::-1]).max() <= 1
    for u in (0, 1, 1000, 32768, 50000, 65536):
        x = (u + 0.5) / 65537
        assert table[u] == round(1024 * np.log(x / (1 - x)))
    assert 11.7 * 1024 < table[-1] < 11.9 * 1024 and -11.9 * 1024 < table[0] < -11.7 * 1024
    assert ls.viterbi_emission_table(unit=16).max() == round(16 * np.log((65536.5 / 65537) / (0.5 / 65537)))
    got = ls.viterbi_settings([0.25, 0.5, 1.0], [0.0, 2.0, 0.3], table)
    assert got == [(int(table[u]), pen) for u in (16384, 32768, 65536) for pen in (0, 2048, 307)]       # thresholds-major
    assert all(isinstance(v, int) for s in got for v in s)
    assert ls.viterbi_settings([0.5], [1.0], CENTRED, unit=10) == [(0, 10)]
    for thr in (0.0, -0.1, 1.01, float("nan")):
        with pytest.raises(ValueError):
            ls.viterbi_settings([thr], [1.0], table)
    for pen in (-0.5, float("inf"), float("nan"), 1e9):
        with pytest.raises(ValueError):
            ls.viterbi_settings([0.5], [pen], table)
    with pytest.raises(ValueError):
        ls.viterbi_frame_spans(np.zeros(4), 0.5, 1.0, table=np.zeros(5, np.int32))
    with pytest.raises(ValueError):
        ls.viterbi_frame_spans(np.zeros(4), 0.5, 1.0, table=np.full(65537, 1 << 25, np.int64))


def test_instances_keys_and_values():
    import laugh_segmenter as ls
    table = ls.viterbi_emission_table()
    p = with_nans(recipe.make_prob_track(6, 2500), 6).astype(np.float32)
    thresholds, min_lengths, penalties = [0.6, 0.3], [0.2, 0.0], [2.0, 0.0, 5.5]
    fps = 36000 / 360.37
    got = ls.viterbi_instances(p, thresholds, min_lengths, fps, penalties)
    assert list(got) == [(t, q, l) for t in thresholds for q in penalties for l in min_lengths]
    keys = [(t, q) for t in thresholds for q in penalties]
    want = vm.instances(p.tolist(), table, ls.viterbi_settings(thresholds, penalties, table), keys, min_lengths, fps)
    assert got == want
    assert all(type(v) is float for inst in got.values() for pair in inst for v in pair)
    assert sum(len(v) for v in got.values()) > 50
    assert list(ls.viterbi_instances(p)) == [(0.5, 0.0, 0.2)]
    with pytest.raises(ValueError):
        ls.viterbi_instances(p, fps=0.0)


def test_score_sweep_host_with_penalties():
    import laugh_segmenter as ls
    import sweep_eval as se
    T = 4000
    thresholds, min_lengths, penalties = [0.2, 0.5, 0.9], [0.0, 0.2], [0.0, 2.0]
    fps = [100.0, 36000 / 360.37]
    duration = T / min(fps)
    rows = sm.make_rows(81, M, ["fe001", "me002"], duration * 1.05, n_per_type=60, max_len_s=1.0)
    chans = [{"meeting_id": M, "part_id": p, "chan": f"chan{i}", "length": duration} for i, p in enumerate(["fe001", "me002"])]
    index = se.TranscriptIndex(rows, chans)
    model = sm.Model(rows, chans, sm.to_frames(duration * 1.2) + 10)
    channels = [(M, "chan0"), (M, "chan1")]
    tracks = [recipe.make_prob_track(82, T), with_nans(recipe.make_prob_track(83, T - 100), 83)]
    got, ev = se.score_sweep_host(tracks, channels, thresholds, min_lengths, fps, index, penalties=penalties, events=(1, 0))
    assert got.dtype == ev.dtype == np.int64 and got.shape == ev.shape == (2, 3, 2, 2, 7)
    assert np.array_equal(got, se.score_sweep_host(tracks, channels, thresholds, min_lengths, fps, index, penalties=penalties))
    table = ls.viterbi_emission_table()
    keys = [(t, q) for t in thresholds for q in penalties]
    for c, t in enumerate(tracks):
        inst = vm.instances(t.tolist(), table, ls.viterbi_settings(thresholds, penalties, table), keys, min_lengths, fps[c])
        assert inst == ls.viterbi_instances(t, thresholds, min_lengths, fps[c], penalties)
        events = se.event_scores_instances(inst, index, M, f"chan{c}", 1, 0)
        for k, thr in enumerate(thresholds):
            for q, pen in enumerate(penalties):
                for l, min_l in enumerate(min_lengths):
                    assert tuple(got[c, k, q, l]) == model.score(inst[(thr, pen, min_l)], M, f"chan{c}"), (c, thr, pen, min_l)
                    assert tuple(ev[c, k, q, l]) == events[(thr, pen, min_l)]
    assert (got.sum(axis=(0, 1, 2, 3)) > 0).all() and not np.array_equal(got[:, :, 0], got[:, :, 1])
    for clash in (dict(offset_drops=[0.0]), dict(min_gaps=[0.1]), dict(offset_drops=[0.0], min_gaps=[0.0])):
        with pytest.raises(ValueError):
            se.score_sweep_host(tracks, channels, thresholds, min_lengths, fps, index, penalties=penalties, **clash)
    # the axis absent: today's array and today's rows
    plain = se.score_sweep_host(tracks, channels, thresholds, min_lengths, fps, index)
    assert plain.shape == (2, 3, 2, 7)
    rows15 = se.eval_rows(got, channels, thresholds, min_lengths, index, penalties=penalties)
    assert len(rows15) == 3 * 2 * 2 and all(len(r) == len(se.EVAL_COLUMNS_VITERBI) == 15 for r in rows15)
    assert se.EVAL_COLUMNS_VITERBI[:5] == ["meeting", "threshold", "min_len", "penalty", "precision"]
    assert [tuple(r[1:4]) for r in rows15] == [(t, l, q) for t in thresholds for q in penalties for l in min_lengths]
    as_plain = se.eval_rows(got[:, :, 1], channels, thresholds, min_lengths, index)
    assert [r[:3] + r[4:] for r in rows15 if r[3] == 2.0] == as_plain
    s15 = se.calc_sum_stats(rows15, penalties=penalties)
    assert len(s15) == 12 and all(len(r) == len(se.SUM_COLUMNS_VITERBI) == 5 for r in s15)
    assert se.SUM_COLUMNS_VITERBI == ["threshold", "min_len", "penalty", "precision", "recall"]
    assert [r[:2] + r[3:] for r in s15 if r[2] == 2.0] == se.calc_sum_stats(as_plain)
    erows = se.event_rows(got, ev, channels, thresholds, min_lengths, index, penalties=penalties)
    assert all(len(r) == len(se.EVENT_COLUMNS_VITERBI) == 16 for r in erows) and se.EVENT_COLUMNS_VITERBI[3] == "penalty"
    as_plain_ev = se.event_rows(got[:, :, 1], ev[:, :, 1], channels, thresholds, min_lengths, index)
    assert repr([r[:3] + r[4:] for r in erows if r[3] == 2.0]) == repr(as_plain_ev)                  # (repr: NaN equals NaN)
    esum = se.event_sum_stats(erows, penalties=penalties)
    assert len(esum) == 12 and all(len(r) == len(se.EVENT_SUM_COLUMNS_VITERBI) == 15 for r in esum)
    assert repr([r[:2] + r[3:] for r in esum if r[2] == 2.0]) == repr(se.event_sum_stats(as_plain_ev))
    with pytest.raises(ValueError):
        se.calc_sum_stats(rows15, binarize=True, penalties=penalties)
    # the existing column lists are what they were
    assert len(se.EVAL_COLUMNS) == 14 and len(se.EVAL_COLUMNS_BINARIZE) == 16 and "penalty" not in se.EVAL_COLUMNS_BINARIZE


# sha256 of the two files a default run over sm.write_corpus wrote before the option existed
DEFAULT_RUN = {"eval_df_per_meeting.csv": "109b9cc893944f841da7847ff7f06b79b95a765fc1a5eb358d09fd370726dc02",
               "sum_stats.csv": "c7f23c09c319165a84832c1d6aeacecbdf267bc529274320f865e2d084aea4c2"}


def test_evaluate_sweep_penalties(tmp_path, capsys):
    import evaluate_sweep
    args = sm.write_corpus(tmp_path)
    evaluate_sweep.main(args + ["--out_dir", str(tmp_path / "plain")])
    evaluate_sweep.main(args + ["--out_dir", str(tmp_path / "new"), "--penalties", "0,2,4", "--events"])
    assert "18 settings (host scorer)" in capsys.readouterr().out
    assert sorted(os.listdir(tmp_path / "plain")) == sorted(DEFAULT_RUN)
    for name, digest in DEFAULT_RUN.items():
        assert hashlib.sha256(open(tmp_path / "plain" / name, "rb").read()).hexdigest() == digest, name
    read = lambda d, f: open(tmp_path / d / f).read().splitlines()
    new = read("new", "eval_df_per_meeting.csv")
    assert new[0].split(",")[:5] == ["meeting", "threshold", "min_len", "penalty", "precision"] and len(new) == 1 + 2 * 3 * 3 * 2
    assert [l.split(",")[1:4] for l in new[1:19]] == [[str(t), str(l), str(q)] for t in (0.2, 0.5, 0.8) for q in (0.0, 2.0, 4.0)
                                                       for l in (0.0, 0.2)]
    summary = read("new", "sum_stats.csv")
    assert summary[0] == "threshold,min_len,penalty,precision,recall" and len(summary) == 1 + 18
    assert len({l.rsplit(",", 2)[0] for l in summary[1:]}) == 18                       # grouped by all three
    assert read("new", "event_df_per_meeting.csv")[0].split(",")[:5] == ["meeting", "threshold", "min_len", "penalty", "event_precision"]
    assert read("new", "event_sum_stats.csv")[0].split(",")[:4] == ["threshold", "min_len", "penalty", "event_precision"]
    # fewer, longer predictions as the penalty grows
    n_pred = {q: sum(int(l.split(",")[9]) for l in new[1:] if l.split(",")[3] == q and l.split(",")[2] == "0.0") for q in ("0.0", "2.0", "4.0")}
    assert n_pred["0.0"] > n_pred["2.0"] > n_pred["4.0"] > 0
    parser = evaluate_sweep.build_parser()
    base = ["--probs_dir", "p", "--transcripts", "t", "--channels", "c", "--out_dir", "o"]
    assert parser.parse_args(base).penalties is None
    for bad in (["--penalties", "-1"], ["--penalties", "inf"], ["--penalties", "x"]):
        with pytest.raises(SystemExit):
            parser.parse_args(base + bad)
    with pytest.raises(SystemExit):
        evaluate_sweep.main(args + ["--out_dir", str(tmp_path / "clash"), "--penalties", "1", "--min_gaps", "0.1"])


def test_segment_laughter_penalties(tmp_path, monkeypatch):
    """Host-only: the model pass is replaced by a fixed track; what is checked is which directories get which instances."""
    import laugh_segmenter as ls
    import segment_laughter
    track = recipe.make_prob_track(91, 3000).astype(np.float32)
    monkeypatch.setattr(segment_laughter, "predict_file", lambda model, path, **kw: (track, 30.0))
    thresholds, min_lengths = [0.3, 0.6], [0.0, 0.2]

    def tree(root):
        return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)
    _, plain = segment_laughter.load_and_pred(None, "meeting.wav", thresholds, min_lengths, str(tmp_path / "plain"), verbose=False)
    assert plain == ls.get_laughter_instances(track, thresholds, min_lengths, 100.0)
    assert tree(tmp_path / "plain") == sorted(f"t_{t}/l_{l}/meeting.TextGrid" for t in thresholds for l in min_lengths)   # as today
    _, new = segment_laughter.load_and_pred(None, "meeting.wav", thresholds, min_lengths, str(tmp_path / "new"), verbose=False,
                                            penalties=[0.0, 3.0])
    assert new == ls.viterbi_instances(track, thresholds, min_lengths, 100.0, [0.0, 3.0])
    assert tree(tmp_path / "new") == sorted(f"t_{t}/l_{l}/p_{q}/meeting.TextGrid" for t in thresholds for l in min_lengths
                                            for q in (0.0, 3.0))
    assert len(new[(0.3, 3.0, 0.0)]) < len(new[(0.3, 0.0, 0.0)])
    with pytest.raises(ValueError):
        segment_laughter.load_and_pred(None, "meeting.wav", thresholds, min_lengths, str(tmp_path / "clash"), verbose=False,
                                       penalties=[1.0], min_gaps=[0.1])
    parser = segment_laughter.build_parser()
    assert parser.parse_args(["--input_audio_file", "a.wav"]).penalties is None
    assert parser.parse_args(["--input_audio_file", "a.wav", "--penalties", "0,2.5"]).penalties == [0.0, 2.5]
    with pytest.raises(SystemExit):
        parser.parse_args(["--input_audio_file", "a.wav", "--penalties", "-1"])


def test_size_queries_need_no_gpu():
    import _hip
    lib = _hip.lib()
    assert lib.lad_viterbi_table_entries() == 65537 and lib.lad_viterbi_max_settings() == 64
    tile = lib.lad_runs_tile_frames()
    small, large = lib.lad_viterbi_workspace_bytes(1, 1, 1), lib.lad_viterbi_workspace_bytes(3, 9 * tile + 5, 64)
    assert 0 < small < large
    assert large >= 3 * 64 * 10 * (tile // 8)                                          # at least the masks: one bit per frame
    assert lib.lad_viterbi_workspace_bytes(65535, 1 << 30, 64) > 0
    for bad in ((0, 100, 1), (65536, 100, 1), (1, 0, 1), (1, (1 << 30) + 1, 1), (1, 100, 0), (1, 100, 65)):
        assert lib.lad_viterbi_workspace_bytes(*bad) == -1
        assert b"lad_viterbi_workspace_bytes" in lib.lad_last_error()
