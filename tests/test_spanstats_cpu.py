"""Host tests of the span statistics (laugh_segmenter.span_stats / confidences, the stats=True forms, segment_laughter.py's flags).

Every comparison is equality: the statistics are integers and selected track values (include/lad_hip.h above lad_span_stats), and
the derived figures one IEEE division each.  The yardstick is tests/_spanstats_model.py, a loop over the frames of every span."""
import inspect
import os

import numpy as np
import pytest

import _spanstats_cases as cases
import _spanstats_model as model

FRAMES = [1, 2, 257, 2049, 4097]


def _real_tables(x):
    import laugh_segmenter as ls
    t = {f"threshold_{thr}": ls.get_laughter_frame_spans(x, thr) for thr in cases.THRESHOLDS}
    for s in cases.HYSTERESIS:
        t[f"hysteresis_{s}"] = ls.binarize_frame_spans(x, *s, fps=cases.FPS)
    for pen in cases.VITERBI[1]:
        t[f"viterbi_{pen}"] = ls.viterbi_frame_spans(x, cases.VITERBI[0][0], pen)
    return t


@pytest.mark.parametrize("kind", cases.TRACKS)
def test_host_form_equals_the_model(kind):
    import laugh_segmenter as ls
    for T in FRAMES:
        for dtype in (np.float32, np.float64):
            x = cases.track(kind, T, dtype)
            tables = cases.hand_tables(T)
            if T <= 2049 and dtype == np.float32 or T == 257:
                tables.update(_real_tables(x))
            for name, spans in tables.items():
                got = ls.span_stats(x, spans)
                assert [g.dtype for g in got] == [np.int64, np.int64, np.float64] and all(g.shape == (len(spans),) for g in got)
                cases.assert_same(got, cases.model_arrays(x, spans), (kind, T, np.dtype(dtype).name, name))
    # what the tracks are for
    T = 2049
    assert ls.span_stats(cases.track("rising", T, np.float32), [[5, 900]])[1][0] == 900
    assert ls.span_stats(cases.track("falling", T, np.float32), [[5, 900]])[1][0] == 5
    assert ls.span_stats(cases.track("plateaus", T, np.float64), [[40, 70]])[1][0] == 40                      # inside one plateau: its first frame
    wild = cases.track("wild", T, np.float64)
    assert np.isnan(wild).any() and (wild > 1).any() and (wild == 0).any() and (wild < 0).any()
    nan_run = np.array([[100, 103]])
    assert np.isnan(wild[100:104]).all()
    assert [a[0] for a in ls.span_stats(wild, nan_run)] == [0, 100, 0.0]              # every frame NaN: the first frame, 0.0
    assert any(np.isnan(wild[a:b + 1]).any() for a, b in _real_tables(wild)["hysteresis_(0.5, 0.3, 0.05)"])   # a gap bridged NaN frames


def test_invalid_rows_and_refusals():
    import laugh_segmenter as ls
    x = cases.track("noise", 300, np.float32)
    s, p, v = ls.span_stats(x, cases.hand_tables(300)["invalid"])
    assert s[1:4].tolist() == [0, 0, 0] and p[1:4].tolist() == [-1, -1, -1] and v[1:4].tolist() == [0.0, 0.0, 0.0]
    assert p[0] >= 2 and p[4] == 299 and s[0] > 0 and v[4] == float(x[299])
    with pytest.raises(ValueError):
        ls.span_stats(np.zeros((2, 3)), [[0, 1]])


def test_confidences_by_hand():
    import laugh_segmenter as ls
    n = 1000
    ones = np.ones(n, np.float32)
    s, p, v = ls.span_stats(ones, [[0, n - 1]])
    assert s[0] == n << 32 and p[0] == 0 and v[0] == 1.0
    c = ls.confidences(s, p, v, [[0, n - 1]], 100.0)
    assert c.dtype == np.float64 and c.shape == (1, 3) and c.tolist() == [[1.0, 0.0, 1.0]]
    zeros = np.zeros(n, np.float64)
    s, p, v = ls.span_stats(zeros, [[3, 12], [7, 7]])
    q = int(np.rint(np.float64(0.0000001) * 2.0 ** 32))
    assert q == 429 and s.tolist() == [10 * q, q] and p.tolist() == [3, 7] and v.tolist() == [0.0000001, 0.0000001]
    c = ls.confidences(s, p, v, [[3, 12], [7, 7]], 50.0)
    assert c[:, 0].tolist() == [q / 2.0 ** 32, q / 2.0 ** 32] and c[:, 1].tolist() == [3 / 50.0, 7 / 50.0]
    # a quarter and three quarters, three frames: (1 + 3 + 3) / 4 / 3
    x = np.array([0.9, 0.25, 0.75, 0.75, 0.1])
    s, p, v = ls.span_stats(x, [[1, 3]])
    assert s[0] == 7 << 30 and p[0] == 2 and v[0] == 0.75
    assert ls.confidences(s, p, v, [[1, 3]], 100.0).tolist() == [[float(7 << 30) / float(3 << 32), 2 / 100.0, 0.75]]
    # against the model's own division on a real table
    x = cases.track("noise", 2049, np.float32)
    spans = ls.get_laughter_frame_spans(x, 0.5)
    rows = model.span_stats(x.tolist(), spans.tolist())
    want = [list(model.confidence(r, a, b, 100.0)) for r, (a, b) in zip(rows, spans.tolist())]
    assert ls.confidences(*ls.span_stats(x, spans), spans, 100.0).tolist() == want
    # an invalid row: no division by zero
    assert ls.confidences([0], [-1], [0.0], [[5, 4]], 100.0).tolist() == [[0.0, -1 / 100.0, 0.0]]


@pytest.mark.parametrize("family", ["threshold", "hysteresis", "viterbi"])
def test_stats_of_the_host_instances(family):
    import laugh_segmenter as ls
    x = cases.track("wild" if family == "hysteresis" else "noise", 3000, np.float32)
    thresholds, min_lengths, fps = [0.3, 0.6], [0.0, 0.02, 0.2], 100.0
    if family == "threshold":
        fn, kw, spans_of = ls.get_laughter_instances, {}, lambda k: ls.get_laughter_frame_spans(x, k[0])
    elif family == "hysteresis":
        fn, kw = ls.binarize_instances, {"offset_drops": [0.0, 0.2], "min_gaps": [0.0, 0.05]}
        spans_of = lambda k: ls.binarize_frame_spans(x, k[0], k[0] - k[1], k[2], fps)                     # noqa: E731
    else:
        fn, kw, spans_of = ls.viterbi_instances, {"penalties": [0.0, 2.0]}, lambda k: ls.viterbi_frame_spans(x, k[0], k[1])
    assert inspect.signature(fn).parameters["stats"].default is False
    plain = fn(x, thresholds, min_lengths, fps, **kw)
    both = fn(x, thresholds, min_lengths, fps, stats=True, **kw)
    assert isinstance(both, tuple) and len(both) == 2
    inst, stats = both
    assert inst == plain and list(inst) == list(plain) and list(stats) == list(plain)
    assert fn(x, thresholds, min_lengths, fps, stats=False, **kw) == plain
    seen = 0
    for key, rows in inst.items():
        got = stats[key]
        assert got.dtype == np.float64 and got.shape == (len(rows), 3)
        spans = [(a, b) for a, b in spans_of(key).tolist() if b / fps - a / fps > key[-1]]
        assert [(a / fps, b / fps) for a, b in spans] == rows
        want = [list(model.confidence(r, a, b, fps)) for r, (a, b) in zip(model.span_stats(x.tolist(), spans), spans)]
        assert got.tolist() == want, key
        seen += len(rows)
    assert seen > 50
    assert len(inst[(*list(inst)[0][:-1], 0.2)]) < len(inst[list(inst)[0]])                   # the min_length filter dropped some


def test_workspace_bytes_without_a_gpu():
    import _hip
    lib = _hip.lib()
    chunk = int(lib.lad_span_stats_tile_frames())
    assert chunk == cases.CHUNK
    small, large = lib.lad_span_stats_workspace_bytes(1, 1), lib.lad_span_stats_workspace_bytes(3, 360000)
    assert small > 0 and large >= 3 * 360000 * 8 * 2 and large % 256 == 0
    assert lib.lad_span_stats_workspace_bytes(65535, 1) > 0 and lib.lad_span_stats_workspace_bytes(1, 2 ** 30) >= 2 ** 34
    for bad in ((0, 10), (65536, 10), (1, 0), (1, 2 ** 30 + 1), (-1, 10), (1, -5)):
        assert lib.lad_span_stats_workspace_bytes(*bad) == -1
        assert b"lad_span_stats_workspace_bytes" in lib.lad_last_error()


def test_segment_laughter_flags(tmp_path, monkeypatch):
    """Host-only: the model pass is replaced by a fixed track; what is checked is the parser, the files and their bytes."""
    import laugh_segmenter as ls
    import segment_laughter
    parser = segment_laughter.build_parser()
    args = parser.parse_args(["--input_audio_file", "a.wav"])
    assert args.confidence == "False" and args.min_confidence is None
    args = parser.parse_args(["--input_audio_file", "a.wav", "--confidence", "True", "--min_confidence", "0.6"])
    assert args.confidence == "True" and args.min_confidence == 0.6
    with pytest.raises(SystemExit):
        parser.parse_args(["--input_audio_file", "a.wav", "--min_confidence", "high"])
    defaults = {k: p.default for k, p in inspect.signature(segment_laughter.load_and_pred).parameters.items() if p.default is not p.empty}
    assert defaults == {"save_to_textgrid": True, "rank": 0, "world": 1, "precision": "fp32", "save_to_audio_files": False, "verbose": True,
                        "save_probs": None, "segmenter": "host", "resample": False, "save_audio_rate": None, "lowpass": None,
                        "offset_drops": None, "min_gaps": None, "penalties": None, "median": None, "confidence": False,
                        "min_confidence": None}

    x = cases.track("noise", 3000, np.float32)
    smooth = ls.median_filter(x, 21)
    monkeypatch.setattr(segment_laughter, "predict_file", lambda model, path, **kw: (x, 30.0))
    thresholds, min_lengths = [0.3, 0.6], [0.0, 0.2]

    def tree(root):
        return {os.path.relpath(os.path.join(d, f), root): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(root) for f in fs}

    def run(name, **kw):
        _, d = segment_laughter.load_and_pred(None, "meeting.wav", thresholds, min_lengths, str(tmp_path / name), verbose=False, **kw)
        return d, tree(tmp_path / name)
    plain, plain_tree = run("plain", median=21)
    assert run("again", median=21, confidence=False, min_confidence=None) == (plain, plain_tree)
    assert sorted(plain_tree) == sorted(f"t_{t}/l_{l}/meeting.TextGrid" for t in thresholds for l in min_lengths)
    conf, conf_tree = run("conf", median=21, confidence=True)
    assert conf == plain and {k: v for k, v in conf_tree.items() if k.endswith(".TextGrid")} == plain_tree
    assert sorted(conf_tree) == sorted(f"t_{t}/l_{l}/meeting.{e}" for t in thresholds for l in min_lengths for e in ("TextGrid", "confidence.csv"))
    inst, stats = ls.get_laughter_instances(smooth, thresholds, min_lengths, 100.0, stats=True)      # the smoothed track's figures
    for key, rows in inst.items():
        lines = conf_tree[f"t_{key[0]}/l_{key[1]}/meeting.confidence.csv"].decode().split("\n")
        assert lines[0] == "start,end,mean_prob,peak_time,peak_prob" and lines[-1] == "" and len(lines) == len(rows) + 2
        assert lines[1:-1] == [",".join(repr(float(v)) for v in (*r, *c)) for r, c in zip(rows, stats[key].tolist())]
    assert len(plain[(0.3, 0.0)]) > 5
    cut = 0.55
    kept, kept_tree = run("kept", median=21, min_confidence=cut, confidence=True)
    dropped = 0
    for key, rows in inst.items():
        want = [r for r, c in zip(rows, stats[key].tolist()) if not c[0] < cut]
        dropped += len(rows) - len(want)
        assert kept[key] == want
        lines = kept_tree[f"t_{key[0]}/l_{key[1]}/meeting.confidence.csv"].decode().split("\n")
        assert [tuple(float(v) for v in l.split(",")[:2]) for l in lines[1:-1]] == want
    assert dropped > 0 and sum(map(len, kept.values())) > 0
    only, only_tree = run("only", median=21, min_confidence=cut)                  # the filter alone writes no csv
    assert only == kept and only_tree == {k: v for k, v in kept_tree.items() if k.endswith(".TextGrid")}
    hyst, hyst_tree = run("hyst", offset_drops=[0.1], min_gaps=[0.05], confidence=True)
    assert sorted(hyst_tree) == sorted(f"t_{t}/l_{l}/d_0.1_g_0.05/meeting.{e}" for t in thresholds for l in min_lengths
                                       for e in ("TextGrid", "confidence.csv"))
    vit, vit_tree = run("vit", penalties=[1.0], confidence=True)
    assert sorted(vit_tree) == sorted(f"t_{t}/l_{l}/p_1.0/meeting.{e}" for t in thresholds for l in min_lengths
                                      for e in ("TextGrid", "confidence.csv"))
