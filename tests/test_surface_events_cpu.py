"""Event-level scores on the dense sweep (sweep_eval.score_surface_host(..., events=), event_pr_summary, csrc/surface_events.hip's
size query and refusals, evaluate_sweep.py --event_grid), the part that needs no GPU.

The yardstick is what the repository already has: sweep_eval.score_sweep_host(..., events=), threshold by threshold.  Every
comparison of scores is an equality of whole arrays."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import _score_model as sm
from oracle import recipe
from test_surface_cpu import AWKWARD_FPS, HAND, M

CRITERIA = [(1, 0), (20, 50), (0, 100)]
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


def _row(kind, start, end):
    return {"meeting_id": M, "part_id": "fe001", "chan": "chan0", "start": start, "end": end, "length": end - start, "type": kind,
            "laugh_type": "laugh" if kind == "laugh" else None}


def _hand_index(spans, length):
    import sweep_eval as se
    chans = [{"meeting_id": M, "part_id": "fe001", "chan": "chan0", "length": length},
             {"meeting_id": M, "part_id": None, "chan": "chanX", "length": length}]
    return se.TranscriptIndex([_row(*s) for s in spans], chans)


def _seeded_index(seed, duration, n_per_type, max_len_s, invalid=True):
    rows = sm.make_rows(seed, M, ["fe001"], duration * 1.05, n_per_type=n_per_type, max_len_s=max_len_s)
    if not invalid:
        rows = [r for r in rows if r["type"] != "invalid" and not (r["type"] == "laugh" and (r["length"] < 0.2 or r["laugh_type"] == "breath-laugh"))]
    import sweep_eval as se
    chans = [{"meeting_id": M, "part_id": "fe001", "chan": "chan0", "length": duration * 0.97},
             {"meeting_id": M, "part_id": None, "chan": "chanX", "length": duration}]
    return se.TranscriptIndex(rows, chans)


def _both(tracks, channels, levels, min_lengths, fps, index, criteria):
    """(scores, events) of the surface form, held to the per-level sweep and to the surface form without events=."""
    import sweep_eval as se
    want_scores, want = se.score_sweep_host(tracks, channels, levels, min_lengths, fps, index, events=criteria)
    scores, got = se.score_surface_host(tracks, channels, levels, min_lengths, fps, index, events=criteria)
    assert got.dtype == np.int64 and got.shape == (len(tracks), len(levels), len(min_lengths), 7) == scores.shape
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert np.array_equal(scores, want_scores)
    assert np.array_equal(scores, se.score_surface_host(tracks, channels, levels, min_lengths, fps, index))
    return scores, got


def _recall_does_not_grow(events):
    hit = events[..., 2]
    assert (np.diff(hit, axis=1) <= 0).all()                           # n_ref is the same at every level
    assert (np.diff(events[..., 1], axis=1) <= 0).all()                # and neither does the number of touched events


@pytest.mark.parametrize("fps", [100.0, AWKWARD_FPS, 2000.0])
@pytest.mark.parametrize("invalid", [True, False])
def test_surface_events_equal_the_sweep_on_seeded_tracks(fps, invalid):
    T = 4000 if fps < 1000 else 24000                                   # 40 s, 12 s: laughs of 0.2 s and more fit in
    duration = T / fps
    index = _seeded_index(71, duration, 40, duration / 30, invalid)
    sets = index.scoring_sets(M, "chan0")
    assert (len(sets[0]) > 0) == invalid and len(sets[1]) >= 5
    min_lengths = [0.0, 0.1 * 100 / fps, 0.2 * 100 / fps]
    for seed in (3, 4):
        p = recipe.make_prob_track(seed, T).astype(np.float32)
        p[100:260] = np.nan                                                         # NaN blocks
        p[3000:3003] = np.nan
        p[300:310] = 1.5                                                            # above 1, at and below 0
        p[400:420] = -0.1
        p[430] = 0.0
        p[:5] = 0.99                                                                # a run that touches each end
        p[-7:] = 0.99
        levels = sorted(set(np.linspace(0.0, 1.0, 32).tolist() + [float(p[1000]), 0.5]))      # a frame's own value is a level
        assert float(p[1000]) in levels and len(levels) in (33, 34)
        for criteria in CRITERIA:
            _, ev = _both([p], CH, levels, min_lengths, fps, index, criteria)
            assert (ev[0, :, :, 0] == len(sets[1])).all() and ev[0, 0, 0, 1] > 0 and ev[0, :, :, 3:].any()
            assert (ev[..., 2] <= ev[..., 1]).all() and (ev[..., 4] >= ev[..., 1]).all()
            if criteria == (1, 0):
                assert np.array_equal(ev[..., 1], ev[..., 2])
            _recall_does_not_grow(ev)


@pytest.mark.parametrize("name", list(HAND))
def test_surface_events_equal_the_sweep_on_hand_written_tracks(name):
    track = np.asarray(HAND[name], np.float64)
    index = _hand_index([("laugh", 0.02, 0.3), ("speech", 0.05, 0.11), ("invalid", 0.07, 0.08), ("noise", 0.15, 0.4)], 0.35)
    assert index.scoring_sets(M, "chan0")[1].tolist() == [[20, 70], [80, 300]]
    for levels in ([0.0, 0.1, 0.25, 0.5, 0.6, 0.75, 0.9, 1.0], [0.0], [1.0], [i / 40 for i in range(41)]):
        for fps in (100.0, AWKWARD_FPS, 2000.0):
            for criteria in CRITERIA:
                _, ev = _both([track], CH, levels, [-1.0, 0.0, 0.015, 0.05], fps, index, criteria)
                _recall_does_not_grow(ev)


def test_a_channel_without_a_participant_has_seven_zeros():
    index = _seeded_index(72, 40.0, 40, 1.0)
    p = recipe.make_prob_track(9, 4000)
    levels = [i / 16 for i in range(17)]
    scores, ev = _both([p, p], [(M, "chan0"), (M, "chanX")], levels, [0.0, 0.1, 0.2], 100.0, index, (1, 0))
    assert not ev[1].any() and scores[1, :, :, 0].sum() > 100
    assert ev[0, :, :, 1].any() and ev[0, 0, 0, 0] == len(index.scoring_sets(M, "chan0")[1])


def test_events_at_the_ends_of_the_track_longer_than_it_and_between_two_frames():
    """100 frames at 100 fps: ms(f) = 10 f.  The laugh rows leave the events (0, 35], (203, 207] (between frames 20 and 21: linked
    only to a run that holds both), (500, 750], (950, 2000] (its window ends at the last frame, the event behind the track)."""
    spans = [("laugh", 0.0, 0.035 + 0.2), ("invalid", 0.035, 0.203), ("laugh", 0.203, 0.207 + 0.25), ("invalid", 0.207, 0.5),
             ("laugh", 0.5, 0.75), ("laugh", 0.95, 2.0)]
    index = _hand_index(spans, 2.0)
    assert index.scoring_sets(M, "chan0")[1].tolist() == [[0, 35], [203, 207], [500, 750], [950, 2000]]
    levels = [0.1, 0.3, 0.5, 0.7]
    rng = np.random.default_rng(5)
    tracks = {"all on": np.full(100, 0.9), "frame 20 only": np.where(np.arange(100) == 20, 0.9, 0.0),
              "frames 20 and 21": np.where((np.arange(100) >= 20) & (np.arange(100) <= 21), 0.9, 0.2),
              "frame 0 and the last one off": np.concatenate([[0.0], np.full(98, 0.6), [0.0]]),
              "steps": np.repeat([0.2, 0.8, 0.4, 0.6, 0.0, 0.9, 0.35, 0.75, 0.2, 0.6], 10), "noise": rng.random(100)}
    for name, track in tracks.items():
        for criteria in CRITERIA:
            _, ev = _both([track], CH, levels, [0.0, 0.05], 100.0, index, criteria)
            if name == "all on" and criteria == (1, 0):
                assert ev[0, :, 0].tolist() == [[4, 4, 4, 1, 4, 203 + 500 + 950, 955 + 783 + 240 + 1010]] * 4      # one run, (0, 990]
            if name == "frame 20 only":
                assert not ev[0, :, :, 1:].any()                                     # (200, 200]: a run that overlaps nothing
            if name == "frames 20 and 21" and criteria == (0, 100):
                assert ev[0, 2, 0].tolist() == [4, 1, 1, 1, 1, 3, 3]                 # (200, 210] covers (203, 207] whole
    # one event as long as the track, and one longer than it on both sides of a short track
    whole = _hand_index([("laugh", 0.0, 1.0)], 1.0)
    for track in tracks.values():
        _both([track], CH, levels, [0.0, 0.05], 100.0, whole, (20, 50))
        _both([track[:30]], CH, levels, [0.0, 0.05], 100.0, whole, (20, 50))
        _both([track], CH, levels, [0.0, 0.05], AWKWARD_FPS, _hand_index([("laugh", 0.01, 3.0)], 3.0), (0, 100))
    # nothing transcribed: N_REF = 0 and no field is set
    _, ev = _both([tracks["steps"]], CH, levels, [0.0], 100.0, _hand_index([("speech", 0.1, 0.5)], 1.0), (1, 0))
    assert not ev.any()


def test_refused_criteria_and_empty_axes():
    import sweep_eval as se
    index = _seeded_index(72, 40.0, 40, 1.0)
    p = recipe.make_prob_track(9, 4000)
    for bad in ((-1, 0), (1, 101), (1, -1)):
        with pytest.raises(ValueError, match="min_overlap"):
            se.score_surface_host([p], CH, [0.5], [0.2], 100.0, index, events=bad)
    with pytest.raises(TypeError):
        se.score_surface_host([p], CH, [0.5], [0.2], 100.0, index, events=(1.5, 0))
    scores, ev = se.score_surface_host([p], CH, [], [0.2], 100.0, index, events=(1, 0))
    assert scores.shape == ev.shape == (1, 0, 1, 7)
    scores, ev = se.score_surface_host([np.zeros(0)], CH, [0.5], [0.2], 100.0, index, events=(1, 0))
    n_ref = len(index.scoring_sets(M, "chan0")[1])
    assert ev.tolist() == [[[[n_ref, 0, 0, 0, 0, 0, 0]]]] and not scores.any()


def test_event_pr_summary_on_a_hand_computed_table():
    import sweep_eval as se
    nan = float("nan")
    tail = [4, 2, 2, 4, 2, 2, 1.0, 0.01, 0.02]                         # (the nine figures behind F1 are not read)
    rows = [[0.0, 0.0, 0.5, 0.5, 0.5] + tail, [0.25, 0.0, 0.5, 0.5, 0.5] + tail, [0.5, 0.0, 1.0, 0.25, 0.4] + tail,
            [0.75, 0.0, 1.0, 0.0, 0.0] + tail,
            [0.0, 0.2, 0.5, nan, nan] + tail, [0.25, 0.2, 1.0, nan, nan] + tail]
    assert len(rows[0]) == len(se.EVENT_SUM_COLUMNS) and se.EVENT_SUM_COLUMNS[:4] == ["threshold", "min_len", "event_precision", "event_recall"]
    got = se.event_pr_summary(rows)
    # AP = (.5 - .5) * .5 + (.5 - .25) * .5 + (.25 - 0) * 1 + (0 - 0) * 1; F1 = .5, .5, .4, 0: the best one first at threshold 0
    assert got[0] == [0.0, 0.375, 0.5, 0.0]
    assert got[1][0] == 0.2 and all(math.isnan(v) for v in got[1][1:]) and len(got) == 2
    assert se.EVENT_PR_COLUMNS == ["min_len", "event_average_precision", "best_event_f1", "best_event_f1_threshold"]
    assert se.event_pr_summary(rows[::-1])[0] == got[0]
    assert got == se.pr_summary([r[:4] for r in rows])[:1] + got[1:]
    # a later, larger F1 wins: P = .25, R = 1 -> .4; P = .75, R = .75 -> .75
    assert se.event_pr_summary([[0.1, 0.0, 0.25, 1.0, 0.4] + tail, [0.6, 0.0, 0.75, 0.75, 0.75] + tail])[0][2:] == [0.75, 0.6]


def test_surface_events_size_query_and_refusals_need_no_gpu():
    import _hip
    lib = _hip.lib()
    kmax, lmax = lib.lad_surface_max_levels(), lib.lad_score_max_min_lengths()
    assert lib.lad_surface_events_workspace_bytes(1, 1, 0, 1, 1) > 0
    small, big = lib.lad_surface_events_workspace_bytes(1, 36000, 1000, 131, 3), lib.lad_surface_events_workspace_bytes(10, 360000, 100000, kmax, 3)
    assert 0 < small < big and big >= 10 * (2 * 360000 * 2 + (kmax + 1) * 3 * 9 * 8) + 4 * 100000
    assert big > lib.lad_surface_workspace_bytes(10, 360000, 100000, kmax, 3)
    assert lib.lad_surface_events_workspace_bytes(65535, 1 << 20, 1 << 20, kmax, lmax) > 0
    assert lib.lad_surface_events_workspace_bytes(1, 1 << 30, 0, 1, 1) > 0
    for bad in ((0, 10, 10, 1, 1), (65536, 10, 10, 1, 1), (1, 0, 10, 1, 1), (1, (1 << 30) + 1, 10, 1, 1), (1, 10, -1, 1, 1),
                (1, 10, (1 << 30) + 1, 1, 1), (1, 10, 10, 0, 1), (1, 10, 10, kmax + 1, 1), (1, 10, 10, 1, 0), (1, 10, 10, 1, lmax + 1)):
        assert lib.lad_surface_events_workspace_bytes(*bad) == -1
        assert b"lad_surface_events_workspace_bytes" in lib.lad_last_error()
    # everything is checked on the host before anything touches a device buffer: the pointers below are never followed
    fake = ctypes.c_void_p(256)
    i32p, f64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    offsets, bounds, fps, mls = np.zeros(6, np.int32), np.zeros((1, 2), np.int32), np.full(1, 100.0), (ctypes.c_double * 1)(0.2)

    def call(levels, dtype=0, K=None, L=1, min_ms=1, min_pct=0, events=fake):
        lv = (ctypes.c_double * len(levels))(*levels)
        return lib.lad_score_surface_events(fake, dtype, 1, 1000, lv, len(levels) if K is None else K, fake, fake, bounds.ctypes.data_as(i32p),
                                            offsets.ctypes.data_as(i32p), 0, fake, fps.ctypes.data_as(f64p), mls, L, min_ms, min_pct, fake,
                                            fake, events, None)
    for levels, message in (([0.5, 0.4], b"ascend strictly"), ([0.5, 0.5], b"ascend strictly"), ([0.1, float("nan")], b"not finite"),
                            ([float("-inf"), 0.5], b"not finite")):
        assert call(levels) == _hip.LAD_ERR_INVALID and message in lib.lad_last_error(), lib.lad_last_error()
        assert b"lad_score_surface_events" in lib.lad_last_error()
    assert call([0.5], dtype=7) == _hip.LAD_ERR_INVALID and b"dtype" in lib.lad_last_error()
    assert call([0.5], K=0) == _hip.LAD_ERR_INVALID and b"levels 1..4096" in lib.lad_last_error()
    assert call([0.5], L=lmax + 1) == _hip.LAD_ERR_INVALID and b"min_lengths 1.." in lib.lad_last_error()
    for min_ms, min_pct in ((-1, 0), (1, -1), (1, 101)):
        assert call([0.5], min_ms=min_ms, min_pct=min_pct) == _hip.LAD_ERR_INVALID and b"min_overlap_pct 0..100" in lib.lad_last_error()
    assert call([0.5], events=None) == _hip.LAD_ERR_INVALID and b"null buffer" in lib.lad_last_error()
    fps[0] = 0.0
    assert call([0.5]) == _hip.LAD_ERR_INVALID and b"positive finite" in lib.lad_last_error()
    fps[0] = 1e-4
    assert call([0.5]) == _hip.LAD_ERR_INVALID and b"millisecond overflow" in lib.lad_last_error()
    fps[0], offsets[5] = 100.0, 3
    assert call([0.5]) == _hip.LAD_ERR_INVALID and b"index offsets run" in lib.lad_last_error()


def test_surface_events_device_has_no_cpu_fallback():
    import _hip
    import sweep_eval as se
    index = _seeded_index(73, 10.0, 10, 0.5)
    p = torch.rand(1000)
    for bad in (p, p.view(1, 1000), p.numpy(), p.double()):
        with pytest.raises(_hip.LadHipError):
            se.score_surface_device(bad, CH, [0.25, 0.5], [0.2], 100.0, index, events=(1, 0))


def _files(path):
    return {f: open(path / f, "rb").read() for f in sorted(os.listdir(path))}


def test_evaluate_sweep_event_grid_under_the_host_scorer(tmp_path):
    import csv

    import evaluate_sweep
    import sweep_eval as se
    args = sm.write_corpus(tmp_path)
    at = args.index("--thresholds")
    listed, base = args[at + 1], args[:at] + args[at + 2:]
    criteria = ["--event_min_overlap_ms", "20", "--event_min_overlap_pct", "50"]
    evaluate_sweep.main(base + criteria + ["--event_grid", "16", "--out_dir", str(tmp_path / "events")])
    evaluate_sweep.main(base + ["--threshold_grid", "16", "--out_dir", str(tmp_path / "grid")])
    evaluate_sweep.main(base + criteria + ["--thresholds", ",".join(repr(i / 16) for i in range(17)), "--events", "--out_dir",
                                           str(tmp_path / "list")])
    events, grid, plain = _files(tmp_path / "events"), _files(tmp_path / "grid"), _files(tmp_path / "list")
    assert list(grid) == ["eval_df_per_meeting.csv", "pr_summary.csv", "sum_stats.csv"]       # without the flag: the old listings
    assert list(plain) == ["eval_df_per_meeting.csv", "event_df_per_meeting.csv", "event_sum_stats.csv", "sum_stats.csv"]
    assert list(events) == ["eval_df_per_meeting.csv", "event_df_per_meeting.csv", "event_pr_summary.csv", "event_sum_stats.csv",
                            "pr_summary.csv", "sum_stats.csv"]
    for name in grid:
        assert events[name] == grid[name], name
    for name in ("event_df_per_meeting.csv", "event_sum_stats.csv"):
        assert events[name] == plain[name], name
    assert events["event_df_per_meeting.csv"].count(b"\n") == 1 + 2 * 17 * 2
    summary = list(csv.reader(open(tmp_path / "events" / "event_pr_summary.csv")))
    stats = [[float(v) for v in r] for r in list(csv.reader(open(tmp_path / "events" / "event_sum_stats.csv")))[1:]]
    assert summary[0] == se.EVENT_PR_COLUMNS and [[float(v) for v in r] for r in summary[1:]] == se.event_pr_summary(stats)
    assert [float(r[0]) for r in summary[1:]] == [0.0, 0.2] and all(0 < float(r[1]) <= 1 and 0 < float(r[2]) <= 1 for r in summary[1:])
    recall = {}
    for r in stats:
        recall.setdefault(r[1], []).append((r[0], r[3]))
    for rows in recall.values():
        values = [v for _, v in sorted(rows)]
        assert all(x >= y for x, y in zip(values, values[1:])) and values[0] > values[-1]       # event recall does not grow
    # other criteria, other files; --lowpass goes in front of the tree as it goes in front of the list
    evaluate_sweep.main(base + ["--event_grid", "16", "--out_dir", str(tmp_path / "loose")])
    assert _files(tmp_path / "loose")["event_sum_stats.csv"] != events["event_sum_stats.csv"]
    assert _files(tmp_path / "loose")["sum_stats.csv"] == events["sum_stats.csv"]
    evaluate_sweep.main(base + criteria + ["--event_grid", "16", "--lowpass", "0.1", "--out_dir", str(tmp_path / "events_lp")])
    evaluate_sweep.main(base + criteria + ["--thresholds", ",".join(repr(i / 16) for i in range(17)), "--events", "--lowpass", "0.1",
                                           "--out_dir", str(tmp_path / "list_lp")])
    smooth = _files(tmp_path / "events_lp")
    assert smooth["event_sum_stats.csv"] == _files(tmp_path / "list_lp")["event_sum_stats.csv"] != events["event_sum_stats.csv"]
    # what the flag cannot be combined with
    for extra in (["--thresholds", listed], ["--threshold_grid", "16"], ["--events"], ["--offset_drops", "0.1"], ["--min_gaps", "0.1"],
                  ["--penalties", "1.0"]):
        with pytest.raises(SystemExit, match="--event_grid cannot be combined with") as e:
            evaluate_sweep.main(base + ["--event_grid", "16", "--out_dir", str(tmp_path / "never")] + extra)
        assert extra[0] in str(e.value)
    assert not os.path.exists(tmp_path / "never")
    with pytest.raises(SystemExit, match="--threshold_grid cannot be combined with --events"):      # today's sentence stays
        evaluate_sweep.main(base + ["--threshold_grid", "16", "--events", "--out_dir", str(tmp_path / "never")])
    for bad in ("0", "4096", "-3", "x"):
        with pytest.raises(SystemExit):
            evaluate_sweep.build_parser().parse_args(base + ["--event_grid", bad, "--out_dir", "o"])
    assert evaluate_sweep.build_parser().parse_args(base + ["--event_grid", "4095", "--out_dir", "o"]).event_grid == 4095


def test_surface_events_object_has_no_scratch(tmp_path):
    """The gfx950 code object of csrc/surface_events.hip: no private (scratch) segment in any of its seven kernels."""
    import re
    import subprocess

    import _hip
    _hip.lib()
    llvm = "/opt/rocm/lib/llvm/bin"
    obj = os.path.join(os.path.dirname(os.path.abspath(_hip.__file__)), "csrc", "build", "surface_events.o")
    tools = [os.path.join(llvm, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    if not (os.path.exists(obj) and all(os.path.exists(t) for t in tools)):
        pytest.skip("no object file of surface_events.hip / no llvm tools in this tree")
    fb, co = tmp_path / "surface_events.fatbin", tmp_path / "surface_events.co"
    subprocess.run([tools[0], f"--dump-section=.hip_fatbin={fb}", obj], check=True, capture_output=True)
    subprocess.run([tools[1], "--type=o", "--unbundle", f"--input={fb}", f"--output={co}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"], check=True, capture_output=True)
    notes = subprocess.run([tools[2], "--notes", str(co)], capture_output=True, text=True, check=True).stdout
    scratch = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", notes)
    assert len(scratch) == 7 and set(scratch) == {"0"}, scratch      # bins (float32, float64), tree, cum, nodes, match, prefix
