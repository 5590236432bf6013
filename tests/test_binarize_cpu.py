"""CPU tests of hysteresis and gap filling on the host (laugh_segmenter.binarize_frame_spans / binarize_instances, the two extra axes
of sweep_eval.score_sweep_host, the --offset_drops / --min_gaps flags).  Integer bookkeeping and IEEE float64 division: every
comparison is an equality -- against the per-frame model of tests/_binarize_model.py, which shares nothing with the package."""
import json
import os

import numpy as np
import pytest

import _binarize_model as bm
import _score_model as sm
from oracle import recipe

ONSETS = [0.0, 0.2, 0.5, 0.9, 1.0]
DROPS = [0.0, 0.05, 0.3, 1.5]
GAPS = [0.0, 0.03, 0.2, 1.0, 1e9]
FPS = [100.0, 36000 / 360.37]
NAN = float("nan")


def with_nans(p, seed):
    q = p.copy()
    rng = np.random.default_rng(seed)
    q[rng.integers(0, len(q), len(q) // 40)] = np.nan
    at = int(rng.integers(100, len(q) - 100))
    q[at:at + 30] = np.nan
    return q


def as_tuples(a):
    return [tuple(int(v) for v in r) for r in a]


@pytest.fixture(scope="module")
def tracks():
    return [recipe.make_prob_track(71, 36000), with_nans(recipe.make_prob_track(72, 36000), 72)]


@pytest.fixture(scope="module")
def model_runs(tracks):
    """{(track, onset, drop): hysteresis runs of the per-frame loop}, computed once."""
    return {(i, on, dr): bm.hysteresis_runs(t.tolist(), on, on - dr) for i, t in enumerate(tracks) for on in ONSETS for dr in DROPS}


def test_frame_spans_against_the_model(tracks, model_runs):
    import laugh_segmenter as ls
    seen_join = seen_late_start = 0
    for i, t in enumerate(tracks):
        for on in ONSETS:
            for dr in DROPS:
                held = model_runs[(i, on, dr)]
                plain = as_tuples(ls.get_laughter_frame_spans(t, on - dr))
                seen_late_start += sum(1 for r in held if r not in plain)
                for fps in FPS:
                    for gap in GAPS:
                        want = bm.fill_gaps(held, gap, fps)
                        got = ls.binarize_frame_spans(t, on, on - dr, gap, fps)
                        assert got.dtype == np.int64 and got.shape == (len(want), 2)
                        assert as_tuples(got) == want, (i, on, dr, gap, fps)
                        seen_join += len(held) - len(want)
    assert seen_join > 1000 and seen_late_start > 1000                  # both controls at work


def test_instances_against_the_model(tracks):
    import laugh_segmenter as ls
    min_lengths = [0.0, 0.1, 0.2]
    for t in (tracks[1][:6000], tracks[0][:6000].astype(np.float32)):
        for fps in FPS:
            got = ls.binarize_instances(t, ONSETS, min_lengths, fps, DROPS, GAPS)
            want = bm.instances(t.tolist(), ONSETS, min_lengths, fps, DROPS, GAPS)
            assert list(got.keys()) == list(want.keys())                 # thresholds-major, then drop, then gap, then min_length
            assert got == want
            assert all(type(v) is float for spans in got.values() for s in spans for v in s)


CONSTRUCTED = [
    # (name, probs, onset, offset, min_gap, fps, expected)
    ("one frame on", [0.9], 0.5, 0.3, 0.0, 100.0, [(0, 0)]),
    ("one frame held only", [0.4], 0.5, 0.3, 0.0, 100.0, []),
    ("two frames", [0.9, 0.4], 0.5, 0.3, 0.0, 100.0, [(0, 1)]),
    ("two frames, onset second", [0.4, 0.9], 0.5, 0.3, 0.0, 100.0, [(1, 1)]),
    ("three frames", [0.4, 0.9, 0.4], 0.5, 0.3, 0.0, 100.0, [(1, 2)]),
    ("three frames, release in the middle", [0.9, 0.1, 0.9], 0.5, 0.3, 0.0, 100.0, [(0, 0), (2, 2)]),
    ("all held, no onset", [0.4] * 50, 0.5, 0.3, 0.0, 100.0, []),
    ("onset at frame 0", [0.9] + [0.4] * 9 + [0.1] * 5, 0.5, 0.3, 0.0, 100.0, [(0, 9)]),
    ("two onsets in one held region", [0.1, 0.4, 0.9, 0.4, 0.9, 0.4, 0.1], 0.5, 0.3, 0.0, 100.0, [(2, 5)]),
    ("starts at the H frame", [0.1, 0.4, 0.4, 0.9, 0.4, 0.1], 0.5, 0.3, 0.0, 100.0, [(3, 4)]),
    ("NaN ends a hold", [0.9, 0.4, NAN, 0.4, 0.4, 0.9], 0.5, 0.3, 0.0, 100.0, [(0, 1), (5, 5)]),
    ("value equal to the offset releases", [0.9, 0.25, 0.4], 0.5, 0.25, 0.0, 100.0, [(0, 0)]),      # (0.25: the same in float32)
    ("value equal to the onset does not start", [0.5, 0.4], 0.5, 0.3, 0.0, 100.0, []),
    ("p > 1 is 1: no onset at 1", [1.5, 0.4], 1.0, 0.3, 0.0, 100.0, []),
    ("p > 1 is 1: held", [1.5, 2.0, 0.4], 0.9, 0.3, 0.0, 100.0, [(0, 2)]),
    ("p <= 0 is 1e-7: above offset 0", [0.9, 0.0, -1.0, 0.9], 0.5, 0.0, 0.0, 100.0, [(0, 3)]),
    ("p <= 0 is 1e-7: an onset at 0", [0.0, -3.0], 0.0, 0.0, 0.0, 100.0, [(0, 1)]),
    ("negative offset holds everything but NaN", [0.0, 0.9, 0.0, NAN, 0.0], 0.5, -1.0, 0.0, 100.0, [(1, 2)]),
]


@pytest.mark.parametrize("case", CONSTRUCTED, ids=[c[0] for c in CONSTRUCTED])
def test_constructed_tracks(case):
    import laugh_segmenter as ls
    _, probs, onset, offset, gap, fps, want = case
    assert bm.spans(probs, onset, offset, gap, fps) == want
    for dtype in (np.float64, np.float32):
        assert as_tuples(ls.binarize_frame_spans(np.asarray(probs, dtype), onset, offset, gap, fps)) == want


def test_empty_input():
    import laugh_segmenter as ls
    got = ls.binarize_frame_spans([], 0.5, 0.3, 0.1, 100.0)
    assert got.shape == (0, 2) and got.dtype == np.int64
    assert ls.binarize_instances([], [0.5], [0.2], 100.0, [0.1], [0.3]) == {(0.5, 0.1, 0.3, 0.2): []}


@pytest.mark.parametrize("fps", FPS)
def test_gaps_exactly_at_the_join_boundary(fps):
    """Two single-frame-wide events, the second `d` frames behind the first: joined iff not (b / fps - a / fps > min_gap), with
    min_gap the float64 value of that very difference, its neighbours below and above, and 0."""
    import laugh_segmenter as ls
    for a in (0, 7, 1234):
        for d in (2, 3, 5, 100):
            b = a + d
            p = np.full(b + 3, 0.1)
            p[[a, b]] = 0.9
            exact = b / fps - a / fps
            for gap, joined in ((exact, True), (np.nextafter(exact, 0.0), False), (np.nextafter(exact, 10.0), True), (0.0, False)):
                want = [(a, b)] if joined else [(a, a), (b, b)]
                assert bm.spans(p.tolist(), 0.5, 0.5, float(gap), fps) == want
                assert as_tuples(ls.binarize_frame_spans(p, 0.5, 0.5, float(gap), fps)) == want, (a, d, gap)
    # chains collapse: pairwise on the original neighbours
    p = np.full(40, 0.1)
    p[[1, 4, 7, 20, 23]] = 0.9
    assert as_tuples(ls.binarize_frame_spans(p, 0.5, 0.5, 3 / fps, fps)) == bm.spans(p.tolist(), 0.5, 0.5, 3 / fps, fps)
    assert as_tuples(ls.binarize_frame_spans(p, 0.5, 0.5, 1e9, fps)) == [(1, 23)]


def test_reduces_to_the_reference_goldens(golden_dir):
    import laugh_segmenter as ls
    cases = json.load(open(os.path.join(golden_dir, "segmenter.json")))
    assert len(cases) >= 3
    for c in cases:
        p = recipe.make_prob_track(c["seed"], c["n"]) if "seed" in c else np.array(c["probs"])
        plain = ls.get_laughter_instances(p, c["thresholds"], c["min_lengths"], c["fps"])
        got = ls.binarize_instances(p, c["thresholds"], c["min_lengths"], c["fps"])          # drop = 0, gap = 0
        assert list(got.keys()) == [(thr, 0.0, 0.0, min_l) for thr, min_l in plain]
        for (thr, min_l), spans in plain.items():
            assert got[(thr, 0.0, 0.0, min_l)] == spans
        for thr in c["thresholds"]:
            assert np.array_equal(ls.binarize_frame_spans(p, thr, thr, 0.0, c["fps"]), ls.get_laughter_frame_spans(p, thr))


def test_argument_errors():
    import laugh_segmenter as ls
    p = [0.1, 0.9, 0.4]
    for bad in (dict(offset_drops=[-0.1]), dict(min_gaps=[-1.0]), dict(offset_drops=[float("inf")]), dict(min_gaps=[NAN]),
                dict(offset_drops=[NAN])):
        with pytest.raises(ValueError):
            ls.binarize_instances(p, [0.5], [0.2], 100.0, **bad)
    with pytest.raises(ValueError):
        ls.binarize_instances(p, [float("inf")], [0.2], 100.0)
    for args in ((0.5, 0.6), (0.5, 0.3, -0.01), (0.5, 0.3, float("inf")), (NAN, 0.3), (0.5, -float("inf"))):
        with pytest.raises(ValueError):
            ls.binarize_frame_spans(p, *args)
    for fps in (0.0, -100.0, float("inf"), NAN):
        with pytest.raises(ValueError):
            ls.binarize_frame_spans(p, 0.5, 0.3, 0.0, fps)


def test_score_sweep_host_with_the_new_axes():
    import sweep_eval as se
    M = "Bmr001"
    T = 6000
    thresholds, min_lengths, drops, gaps = [0.2, 0.5, 0.9], [0.0, 0.2], [0.0, 0.3], [0.0, 0.2, 1.0]
    fps = [100.0, FPS[1]]
    duration = T / min(fps)
    rows = sm.make_rows(81, M, ["fe001", "me002"], duration * 1.05, n_per_type=60, max_len_s=1.0)
    chans = [{"meeting_id": M, "part_id": p, "chan": f"chan{i}", "length": duration} for i, p in enumerate(["fe001", "me002"])]
    index = se.TranscriptIndex(rows, chans)
    model = sm.Model(rows, chans, sm.to_frames(duration * 1.2) + 10)
    channels = [(M, "chan0"), (M, "chan1")]
    tracks = [recipe.make_prob_track(82, T), with_nans(recipe.make_prob_track(83, T - 100), 83)]
    got = se.score_sweep_host(tracks, channels, thresholds, min_lengths, fps, index, offset_drops=drops, min_gaps=gaps)
    assert got.dtype == np.int64 and got.shape == (2, 3, 2, 3, 2, 7)
    for c, t in enumerate(tracks):
        inst = bm.instances(t.tolist(), thresholds, min_lengths, fps[c], drops, gaps)
        for k, thr in enumerate(thresholds):
            for d, drop in enumerate(drops):
                for g, gap in enumerate(gaps):
                    for l, min_l in enumerate(min_lengths):
                        assert tuple(got[c, k, d, g, l]) == model.score(inst[(thr, drop, gap, min_l)], M, f"chan{c}"), (c, thr, drop, gap)
    assert (got.sum(axis=(0, 1, 2, 3, 4)) > 0).all()
    # the axes absent: today's array; drop 0 and gap 0 are that array
    plain = se.score_sweep_host(tracks, channels, thresholds, min_lengths, fps, index)
    assert plain.shape == (2, 3, 2, 7) and np.array_equal(got[:, :, 0, 0], plain)
    one = se.score_sweep_host(tracks, channels, thresholds, min_lengths, fps, index, min_gaps=gaps)   # one axis given: the other [0]
    assert one.shape == (2, 3, 1, 3, 2, 7) and np.array_equal(one[:, :, 0], got[:, :, 0])
    # eval_rows / calc_sum_stats carry the two keys
    rows16 = se.eval_rows(got, channels, thresholds, min_lengths, index, offset_drops=drops, min_gaps=gaps)
    rows14 = se.eval_rows(plain, channels, thresholds, min_lengths, index)
    assert len(rows16) == 3 * 2 * 3 * 2 and all(len(r) == len(se.EVAL_COLUMNS_BINARIZE) == 16 for r in rows16)
    assert [r[:3] + r[5:] for r in rows16 if r[3] == 0.0 and r[4] == 0.0] == rows14
    assert [tuple(r[1:5]) for r in rows16] == [(t, l, d, g) for t in thresholds for d in drops for g in gaps for l in min_lengths]
    s16, s14 = se.calc_sum_stats(rows16, binarize=True), se.calc_sum_stats(rows14)
    assert len(s16) == 36 and all(len(r) == len(se.SUM_COLUMNS_BINARIZE) == 6 for r in s16)
    assert [r[:2] + r[4:] for r in s16 if r[2] == 0.0 and r[3] == 0.0] == s14


def test_evaluate_sweep_flags(tmp_path, capsys):
    import evaluate_sweep
    args = sm.write_corpus(tmp_path)
    evaluate_sweep.main(args + ["--out_dir", str(tmp_path / "plain")])
    evaluate_sweep.main(args + ["--out_dir", str(tmp_path / "zero"), "--offset_drops", "0", "--min_gaps", "0"])
    evaluate_sweep.main(args + ["--out_dir", str(tmp_path / "new"), "--offset_drops", "0,0.15", "--min_gaps", "0,0.2,1"])
    assert "36 settings (host scorer)" in capsys.readouterr().out
    read = lambda d, f: open(tmp_path / d / f).read().splitlines()
    plain = read("plain", "eval_df_per_meeting.csv")
    assert plain[0].split(",")[:4] == ["meeting", "threshold", "min_len", "precision"] and len(plain) == 1 + 2 * 3 * 2   # as today
    assert read("plain", "sum_stats.csv")[0] == "threshold,min_len,precision,recall"

    def without_axes(lines, at):
        return [",".join(c for i, c in enumerate(l.split(",")) if i not in at) for l in lines]
    zero = read("zero", "eval_df_per_meeting.csv")
    assert zero[0].split(",")[:6] == ["meeting", "threshold", "min_len", "offset_drop", "min_gap", "precision"]
    assert without_axes(zero, (3, 4)) == plain                                        # drop 0, gap 0: the plain sweep's numbers
    assert without_axes(read("zero", "sum_stats.csv"), (2, 3)) == read("plain", "sum_stats.csv")
    new = read("new", "eval_df_per_meeting.csv")
    assert len(new) == 1 + 2 * 3 * 2 * 3 * 2
    assert without_axes([l for l in new[1:] if l.split(",")[3:5] == ["0.0", "0.0"]], (3, 4)) == plain[1:]
    summary = read("new", "sum_stats.csv")
    assert summary[0] == "threshold,min_len,offset_drop,min_gap,precision,recall" and len(summary) == 1 + 36
    assert len({l.rsplit(",", 2)[0] for l in summary[1:]}) == 36                       # grouped by all four
    parser = evaluate_sweep.build_parser()
    base = ["--probs_dir", "p", "--transcripts", "t", "--channels", "c", "--out_dir", "o"]
    assert parser.parse_args(base).offset_drops is None and parser.parse_args(base).min_gaps is None
    for bad in (["--offset_drops", "-0.1"], ["--min_gaps", "nan"], ["--min_gaps", "a"]):
        with pytest.raises(SystemExit):
            parser.parse_args(base + bad)


def test_segment_laughter_flags(tmp_path, monkeypatch):
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
                                            offset_drops=[0.0, 0.2], min_gaps=[0.0, 0.5])
    assert new == ls.binarize_instances(track, thresholds, min_lengths, 100.0, [0.0, 0.2], [0.0, 0.5])
    assert tree(tmp_path / "new") == sorted(f"t_{t}/l_{l}/d_{d}_g_{g}/meeting.TextGrid" for t in thresholds for l in min_lengths
                                            for d in (0.0, 0.2) for g in (0.0, 0.5))
    for t in thresholds:
        for l in min_lengths:
            a = open(tmp_path / "plain" / f"t_{t}" / f"l_{l}" / "meeting.TextGrid", "rb").read()
            assert open(tmp_path / "new" / f"t_{t}" / f"l_{l}" / "d_0.0_g_0.0" / "meeting.TextGrid", "rb").read() == a
    assert len(new[(0.3, 0.2, 0.5, 0.0)]) < len(new[(0.3, 0.0, 0.0, 0.0)])             # the controls did something
    parser = segment_laughter.build_parser()
    args = parser.parse_args(["--input_audio_file", "a.wav"])
    assert args.offset_drops is None and args.min_gaps is None
    args = parser.parse_args(["--input_audio_file", "a.wav", "--offset_drops", "0,0.1", "--min_gaps", "0.25"])
    assert args.offset_drops == [0.0, 0.1] and args.min_gaps == [0.25]
    with pytest.raises(SystemExit):
        parser.parse_args(["--input_audio_file", "a.wav", "--offset_drops", "-1"])
