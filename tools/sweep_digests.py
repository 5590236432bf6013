"""SHA-256 digests of what the sweep's Python layer returns and writes for seeded inputs: the recorder behind
tests/test_sweep_parent_cpu.py and tests/test_sweep_parent_gpu.py, which import the cases and the inputs from here.

    python tools/sweep_digests.py cpu|gpu [out.json]     (default: tests/golden/sweep_parent.json; the other part is kept)

What is held in place is the public surface of laugh_segmenter.py, sweep_eval.py, evaluate_sweep.py and segment_laughter.py for the
three span families (frame-by-frame thresholds, hysteresis and gap filling, the two-state Viterbi decoder): dictionaries with their
key order and float reprs, span arrays, score arrays, row lists, the files and directories the two scripts write, the lines they
print, and the refusals with their messages.  Only public names are used, so the same file records a commit and checks a later one.

A case is serialised before it is hashed: a dictionary as repr of its (key, value) list in iteration order; an array as dtype, shape
and bytes; a list of arrays as the arrays in order; a directory as its sorted relative paths and the bytes of every file; a refusal
as the exception's type and message."""
import atexit
import contextlib
import hashlib
import io
import json
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "laughter-detection-icsi_amd", "utils"), os.path.join(ROOT, "laughter-detection-icsi_amd"), ROOT,
           os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

GOLDEN = os.path.join(ROOT, "tests", "golden", "sweep_parent.json")

TRACKS = [(5, 2500), (6, 1300), (7, 600)]       # 2500 frames cross a 512-frame tile edge and the 2048-frame workgroup edge
THRESHOLDS = [0.01, 0.1, 0.25, 0.4, 0.5, 0.6, 0.75, 0.9, 1.0]
MIN_LENGTHS = [0.0, 0.1, 0.2]
OFFSET_DROPS, MIN_GAPS = [0.0, 0.1, 0.3], [0.0, 0.05, 0.2]        # 81 settings: two rounds of at most lad_binarize_max_settings()
PENALTIES = [0.0, 0.5, 1, 2, 3, 4, 6, 8]                          # 72 settings: two rounds of at most lad_viterbi_max_settings()
FPS = 100.0
FPS_PER_CHANNEL = [100.0, 99.7, 100.3]
EVENTS = (200, 50)
LOWPASS = 0.05
FAMILIES = {"plain": {}, "hysteresis": dict(offset_drops=OFFSET_DROPS, min_gaps=MIN_GAPS), "viterbi": dict(penalties=PENALTIES)}
SCRIPT_FLAGS = {"plain": [], "hysteresis": ["--offset_drops", "0,0.1", "--min_gaps", "0,0.2"], "viterbi": ["--penalties", "0,2"]}
SEGMENT_AXES = {"plain": {}, "hysteresis": dict(offset_drops=[0.0, 0.1], min_gaps=[0.0, 0.2]), "viterbi": dict(penalties=[0.0, 2.0])}


# ---- serialisation ---------------------------------------------------------------------------------------------------------------
def _feed(h, obj):
    if isinstance(obj, dict):
        h.update(b"dict:" + repr(list(obj.items())).encode())
    elif isinstance(obj, np.ndarray):
        h.update(f"array:{obj.dtype.str}:{obj.shape}:".encode() + np.ascontiguousarray(obj).tobytes())
    elif isinstance(obj, (list, tuple)) and obj and all(isinstance(v, (np.ndarray, list, tuple)) for v in obj):
        h.update(f"list:{len(obj)}:".encode())
        for v in obj:
            _feed(h, v)
    else:
        h.update(b"repr:" + repr(obj).encode())


def sha(obj):
    h = hashlib.sha256()
    _feed(h, obj)
    return h.hexdigest()


def tree(root):
    """The sorted relative paths under root and the bytes of every file."""
    paths = sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)
    return [(p.replace(os.sep, "/"), open(os.path.join(root, p), "rb").read()) for p in paths]


def refusal(fn):
    try:
        fn()
    except (Exception, SystemExit) as e:
        return f"{type(e).__name__}: {e}"
    return "accepted"


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def tracks64():
    from oracle import recipe
    return [recipe.make_prob_track(seed, n) for seed, n in TRACKS]


def padded(tracks, dtype):
    out = np.full((len(tracks), max(len(t) for t in tracks)), np.nan, dtype)
    for c, t in enumerate(tracks):
        out[c, :len(t)] = t
    return out


def binarize_settings():
    return [(thr, thr - drop, gap) for thr in THRESHOLDS for drop in OFFSET_DROPS for gap in MIN_GAPS]


_corpus = {}


def corpus():
    """tests/_score_model.write_corpus(T=3000) in a directory of its own: (the command line of evaluate_sweep, index, channels,
    tracks)."""
    if not _corpus:
        import pathlib

        import _score_model as sm
        import evaluate_sweep
        import sweep_eval
        tmp = pathlib.Path(tempfile.mkdtemp(prefix="sweep_digests_"))
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        args = sm.write_corpus(tmp, T=3000)
        rows = evaluate_sweep.read_csv(str(tmp / "transcripts.csv"), sweep_eval.ROW_COLUMNS, ("start", "end", "length"))
        chans = evaluate_sweep.read_csv(str(tmp / "channels.csv"), sweep_eval.CHANNEL_COLUMNS, ("length",))
        index = sweep_eval.TranscriptIndex(rows, chans)
        channels, tracks = evaluate_sweep.load_tracks(str(tmp / "probs"), index)
        _corpus.update(tmp=tmp, args=args[:args.index("--thresholds")], index=index, channels=channels, tracks=tracks)
    return _corpus


# ---- cases -----------------------------------------------------------------------------------------------------------------------
def instances(family, probs, device=False):
    import laugh_segmenter as ls
    fn = {"plain": ls.get_laughter_instances, "hysteresis": ls.binarize_instances, "viterbi": ls.viterbi_instances}[family]
    if device:
        fn = getattr(ls, fn.__name__ + "_device")
    return fn(probs, THRESHOLDS, MIN_LENGTHS, FPS, **FAMILIES[family])


def _stats(se, family, scores, events=None):
    """eval_rows / calc_sum_stats (event_rows / event_sum_stats with events) of one sweep."""
    c = corpus()
    axes = FAMILIES[family]
    kind = dict(penalties=PENALTIES) if family == "viterbi" else dict(binarize=family == "hysteresis")
    if events is None:
        rows = se.eval_rows(scores, c["channels"], THRESHOLDS, MIN_LENGTHS, c["index"], **axes)
        return rows, se.calc_sum_stats(rows, **kind)
    rows = se.event_rows(scores, events, c["channels"], THRESHOLDS, MIN_LENGTHS, c["index"], **axes)
    return rows, se.event_sum_stats(rows, **kind)


def _sweep_cases(cases, prefix, sweep):
    """The score arrays of one scorer for the three families, without and with events=, and the rows made of them.  sweep(axes,
    events) -> what score_sweep_* returns.  Each sweep runs once however many of its cases are asked for."""
    import sweep_eval as se
    memo = {}

    def run(family, events):
        if (family, events) not in memo:
            memo[(family, events)] = sweep(FAMILIES[family], EVENTS if events else None)
        return memo[(family, events)]
    for family in FAMILIES:
        cases[f"{prefix}/{family}/scores"] = lambda f=family: run(f, False)
        cases[f"{prefix}/{family}/scores_with_events"] = lambda f=family: list(run(f, True))
        cases[f"{prefix}/{family}/eval_rows"] = lambda f=family: repr(_stats(se, f, run(f, False))[0])
        cases[f"{prefix}/{family}/calc_sum_stats"] = lambda f=family: repr(_stats(se, f, run(f, False))[1])
        cases[f"{prefix}/{family}/event_rows"] = lambda f=family: repr(_stats(se, f, *run(f, True))[0])
        cases[f"{prefix}/{family}/event_sum_stats"] = lambda f=family: repr(_stats(se, f, *run(f, True))[1])


def _evaluate_sweep(scorer, family, events, lowpass):
    import evaluate_sweep
    c = corpus()
    out = tempfile.mkdtemp(prefix="out_", dir=c["tmp"])
    argv = c["args"] + ["--thresholds", "0.2,0.5,0.8", "--min_lengths", "0.0,0.2", "--scorer", scorer, "--out_dir", out]
    argv += SCRIPT_FLAGS[family] + (["--events", "--event_min_overlap_ms", "200", "--event_min_overlap_pct", "50"] if events else [])
    argv += ["--lowpass", str(LOWPASS)] if lowpass else []
    with contextlib.redirect_stdout(io.StringIO()) as said:
        evaluate_sweep.main(argv)
    return tree(out), said.getvalue().replace(out, "<out>")


def _script_cases(cases, scorer):
    for family in FAMILIES:
        for events in (False, True):
            for lowpass in (False, True):
                name = f"evaluate_sweep/{scorer}/{family}" + ("/events" if events else "") + ("/lowpass" if lowpass else "")
                cases[name] = lambda f=family, e=events, l=lowpass: repr(_evaluate_sweep(scorer, f, e, l))


def _load_and_pred(segmenter, family):
    """segment_laughter.load_and_pred behind a stub predict that returns a fixed track: the directories, the TextGrid bytes, the
    "Found ..." lines and the dictionary."""
    import segment_laughter
    from oracle import recipe
    track = recipe.make_prob_track(91, 3000).astype(np.float32)
    if segmenter == "device":
        import torch
        stub, name = (lambda model, path, **kw: (torch.from_numpy(track).cuda(), 30.0)), "predict_file_device"
    else:
        stub, name = (lambda model, path, **kw: (track, 30.0)), "predict_file"
    out = tempfile.mkdtemp(prefix="seg_", dir=corpus()["tmp"])
    kept = getattr(segment_laughter, name)
    setattr(segment_laughter, name, stub)
    try:
        with contextlib.redirect_stdout(io.StringIO()) as said:
            _, got = segment_laughter.load_and_pred(None, "meeting.wav", [0.3, 0.6], [0.0, 0.2], out, segmenter=segmenter,
                                                    **SEGMENT_AXES[family])
    finally:
        setattr(segment_laughter, name, kept)
    found = [line for line in said.getvalue().splitlines() if line.startswith("Found ")]
    return repr((tree(out), found, list(got.items())))


def cpu_cases():
    """{name: function without arguments that returns what is digested}, for the host forms."""
    import laugh_segmenter as ls
    import sweep_eval as se
    cases = {}
    for (seed, n), t in zip(TRACKS, tracks64()):
        for family in FAMILIES:          # (the float32 cast seldom moves a frame across a threshold: one case for both)
            cases[f"host/{family}_instances/{n}"] = lambda f=family, p=t: repr(
                [list(instances(f, p.astype(dtype)).items()) for dtype in (np.float64, np.float32)])
        cases[f"host/get_laughter_frame_spans/{n}"] = lambda p=t: ls.get_laughter_frame_spans(p, 0.4)
        cases[f"host/binarize_frame_spans/{n}"] = lambda p=t: ls.binarize_frame_spans(p, 0.6, 0.35, 0.05, 99.7)
        cases[f"host/viterbi_frame_spans/{n}"] = lambda p=t: ls.viterbi_frame_spans(p, 0.4, 2.0)
    c = corpus
    _sweep_cases(cases, "score_sweep_host", lambda axes, events: se.score_sweep_host(
        c()["tracks"], c()["channels"], THRESHOLDS, MIN_LENGTHS, FPS_PER_CHANNEL, c()["index"], events=events, **axes))
    _script_cases(cases, "host")
    for family in FAMILIES:
        cases[f"load_and_pred/host/{family}"] = lambda f=family: _load_and_pred("host", f)
    p = tracks64()[2]
    refusals = {
        "penalties_with_drops/score_sweep_host": lambda: se.score_sweep_host(
            c()["tracks"], c()["channels"], THRESHOLDS, MIN_LENGTHS, FPS, c()["index"], offset_drops=[0.1], penalties=[1.0]),
        "penalties_with_gaps/eval_rows": lambda: se.eval_rows(np.zeros((3, 1, 1, 1, 7), np.int64), c()["channels"], [0.5], [0.2],
                                                              c()["index"], min_gaps=[0.1], penalties=[1.0]),
        "penalties_with_binarize/calc_sum_stats": lambda: se.calc_sum_stats([], binarize=True, penalties=[1.0]),
        "penalties_with_gaps/load_and_pred": lambda: _load_and_pred_clash(),
        "penalties_with_gaps/evaluate_sweep": lambda: _evaluate_sweep_clash(),
        "offset_above_onset": lambda: ls.binarize_frame_spans(p, 0.3, 0.5),
        "negative_drop": lambda: ls.binarize_instances(p, THRESHOLDS, MIN_LENGTHS, FPS, [0.1, -0.1], [0.0]),
        "drop_checked_before_gap": lambda: ls.binarize_instances(p, THRESHOLDS, MIN_LENGTHS, FPS, [float("nan")], [-1.0]),
        "negative_gap": lambda: ls.binarize_instances(p, THRESHOLDS, MIN_LENGTHS, FPS, [0.1], [0.0, -1.0]),
        "hysteresis_fps": lambda: ls.binarize_instances(p, THRESHOLDS, MIN_LENGTHS, 0.0, [0.1], [0.0]),
        "setting_checked_before_fps": lambda: ls.binarize_instances(p, THRESHOLDS, MIN_LENGTHS, 0.0, [0.1], [-1.0]),
        "threshold_zero_to_decoder": lambda: ls.viterbi_instances(p, [0.5, 0.0], MIN_LENGTHS, FPS, [1.0]),
        "negative_penalty": lambda: ls.viterbi_instances(p, [0.5], MIN_LENGTHS, FPS, [1.0, -0.5]),
        "penalty_too_large": lambda: ls.viterbi_instances(p, [0.5], MIN_LENGTHS, FPS, [1e9]),
        "emission_table_shape": lambda: ls.viterbi_instances(p, [0.5], MIN_LENGTHS, FPS, [1.0], table=np.zeros(7, np.int32)),
        "table_checked_before_threshold": lambda: ls.viterbi_instances(p, [0.0], MIN_LENGTHS, FPS, [1.0], table=np.zeros(7, np.int32)),
        "decoder_fps": lambda: ls.viterbi_instances(p, [0.5], MIN_LENGTHS, -1.0, [1.0]),
        "fps_per_channel_count": lambda: se.score_sweep_host(c()["tracks"], c()["channels"], THRESHOLDS, MIN_LENGTHS, [100.0, 99.0],
                                                             c()["index"]),
    }
    cases["refusals/host"] = lambda: {name: refusal(fn) for name, fn in refusals.items()}
    return cases


def _load_and_pred_clash():
    import segment_laughter
    kept = segment_laughter.predict_file
    segment_laughter.predict_file = lambda model, path, **kw: (tracks64()[2].astype(np.float32), 6.0)
    try:
        segment_laughter.load_and_pred(None, "meeting.wav", [0.5], [0.2], os.path.join(corpus()["tmp"], "clash"), verbose=False,
                                       penalties=[1.0], min_gaps=[0.1])
    finally:
        segment_laughter.predict_file = kept


def _evaluate_sweep_clash():
    import evaluate_sweep
    c = corpus()
    evaluate_sweep.main(c["args"] + ["--out_dir", os.path.join(c["tmp"], "clash"), "--penalties", "1", "--min_gaps", "0.1"])


def gpu_cases():
    """The same list through the device forms (needs the MI355X)."""
    import torch

    import laugh_segmenter as ls
    import sweep_eval as se
    cases = {}
    tracks = tracks64()
    for (seed, n), t in zip(TRACKS, tracks):
        for family in FAMILIES:
            cases[f"device/{family}_instances/{n}"] = lambda f=family, p=t: repr(
                [list(instances(f, torch.from_numpy(p.astype(dtype)).cuda(), device=True).items()) for dtype in (np.float64, np.float32)])
    table = ls.viterbi_emission_table()
    both = lambda: [torch.from_numpy(padded(tracks, dtype)).cuda() for dtype in (np.float64, np.float32)]
    cases["device/get_laughter_frame_spans/3x2500"] = lambda: [ls.get_laughter_frame_spans_device(p, THRESHOLDS) for p in both()]
    cases["device/binarize_frame_spans/3x2500"] = \
        lambda: [ls.binarize_frame_spans_device(p, binarize_settings(), FPS_PER_CHANNEL) for p in both()]
    cases["device/viterbi_frame_spans/3x2500"] = \
        lambda: [ls.viterbi_frame_spans_device(p, ls.viterbi_settings(THRESHOLDS, PENALTIES, table)) for p in both()]
    one = lambda: torch.from_numpy(tracks[0]).cuda()
    cases["device/get_laughter_frame_spans/2500"] = lambda: ls.get_laughter_frame_spans_device(one(), THRESHOLDS)
    cases["device/binarize_frame_spans/2500"] = lambda: ls.binarize_frame_spans_device(one(), binarize_settings(), 99.7)
    cases["device/viterbi_frame_spans/2500"] = lambda: ls.viterbi_frame_spans_device(one(), ls.viterbi_settings(THRESHOLDS, PENALTIES, table))
    c = corpus

    def device_sweep(lowpass):
        def sweep(axes, events):
            probs = torch.from_numpy(padded(c()["tracks"], np.float32)).cuda()
            lengths = [len(t) for t in c()["tracks"]] if lowpass else None
            return se.score_sweep_device(probs, c()["channels"], THRESHOLDS, MIN_LENGTHS, FPS_PER_CHANNEL, c()["index"],
                                         lowpass=LOWPASS if lowpass else None, lengths=lengths, events=events, **axes)
        return sweep
    _sweep_cases(cases, "score_sweep_device", device_sweep(False))
    _sweep_cases(cases, "score_sweep_device/lowpass", device_sweep(True))
    _script_cases(cases, "device")
    for family in FAMILIES:
        cases[f"load_and_pred/device/{family}"] = lambda f=family: _load_and_pred("device", f)
    two = lambda: torch.from_numpy(padded(tracks, np.float32)).cuda()
    refusals = {
        "matrix_to_get_laughter_instances_device": lambda: ls.get_laughter_instances_device(two(), THRESHOLDS, MIN_LENGTHS, FPS),
        "matrix_to_binarize_instances_device": lambda: ls.binarize_instances_device(two(), THRESHOLDS, MIN_LENGTHS, FPS, [0.1], [0.0]),
        "matrix_to_viterbi_instances_device": lambda: ls.viterbi_instances_device(two(), THRESHOLDS, MIN_LENGTHS, FPS, [1.0]),
        "host_array_to_get_laughter_frame_spans_device": lambda: ls.get_laughter_frame_spans_device(tracks[2], THRESHOLDS),
        "cube_to_viterbi_frame_spans_device": lambda: ls.viterbi_frame_spans_device(two()[None], [(0, 0)]),
        "cube_to_score_sweep_device": lambda: se.score_sweep_device(two()[None], c()["channels"], THRESHOLDS, MIN_LENGTHS, FPS, c()["index"]),
        "penalties_with_drops/score_sweep_device": lambda: se.score_sweep_device(
            two(), c()["channels"], THRESHOLDS, MIN_LENGTHS, FPS, c()["index"], offset_drops=[0.1], penalties=[1.0]),
        "offset_above_onset": lambda: ls.binarize_frame_spans_device(one(), [(0.3, 0.5, 0.0)]),
        "threshold_zero_to_decoder": lambda: ls.viterbi_instances_device(one(), [0.0], MIN_LENGTHS, FPS, [1.0]),
        "negative_penalty": lambda: ls.viterbi_instances_device(one(), [0.5], MIN_LENGTHS, FPS, [-1.0]),
        "setting_out_of_range": lambda: ls.viterbi_frame_spans_device(one(), [(0, -1)]),
        "lengths_without_lowpass": lambda: se.score_sweep_device(two(), c()["channels"], THRESHOLDS, MIN_LENGTHS, FPS, c()["index"],
                                                                 lengths=[3, 3, 3]),
    }
    cases["refusals/device"] = lambda: {name: refusal(fn) for name, fn in refusals.items()}
    return cases


def digests(cases):
    return {name: sha(fn()) for name, fn in cases.items()}


def cell_counts(device=False):
    """{family: (non-empty cells, cells)} of the three dictionaries over the three float64 tracks."""
    out = {}
    for family in FAMILIES:
        cells = []
        for t in tracks64():
            if device:
                import torch
                t = torch.from_numpy(t).cuda()
            cells += [len(v) for v in instances(family, t, device).values()]
        out[family] = (sum(1 for n in cells if n), len(cells))
    return out


def main():
    part = sys.argv[1]
    path = sys.argv[2] if len(sys.argv) > 2 else GOLDEN
    rec = {}
    if os.path.exists(path):
        with open(path) as f:
            rec = json.load(f)
    rec[part] = digests(cpu_cases() if part == "cpu" else gpu_cases())
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(rec[part])} {part} cases, cells {cell_counts(part == 'gpu')} -> {path}")


if __name__ == "__main__":
    main()
