"""Dense threshold sweep through the component tree (sweep_eval.score_surface_host, pr_summary, csrc/surface.hip's size queries and
refusals, evaluate_sweep.py --threshold_grid), the part that needs no GPU.

The yardstick is what the repository already has: sweep_eval.score_sweep_host, threshold by threshold.  Every comparison of scores
is an equality of whole arrays."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import _score_model as sm
from oracle import recipe

AWKWARD_FPS = 360000 / 3600.0049375
MIN_LENGTHS = [0.0, 0.1, 0.2]
M = "Bmr001"


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


def _index(seed, duration, n_per_type, max_len_s, invalid=True):
    import sweep_eval as se
    rows = sm.make_rows(seed, M, ["fe001"], duration * 1.05, n_per_type=n_per_type, max_len_s=max_len_s)
    if not invalid:
        rows = [r for r in rows if r["type"] != "invalid" and not (r["type"] == "laugh" and (r["length"] < 0.2 or r["laugh_type"] == "breath-laugh"))]
    chans = [{"meeting_id": M, "part_id": "fe001", "chan": "chan0", "length": duration * 0.97},
             {"meeting_id": M, "part_id": None, "chan": "chanX", "length": duration}]
    return se.TranscriptIndex(rows, chans)


def _both(tracks, channels, levels, min_lengths, fps, index):
    import sweep_eval as se
    want = se.score_sweep_host(tracks, channels, levels, min_lengths, fps, index)
    got = se.score_surface_host(tracks, channels, levels, min_lengths, fps, index)
    assert got.dtype == np.int64 and got.shape == (len(tracks), len(levels), len(min_lengths), 7)
    assert np.array_equal(got, want)
    return got


@pytest.mark.parametrize("fps", [100.0, AWKWARD_FPS, 2000.0])
@pytest.mark.parametrize("invalid", [True, False])
def test_surface_host_equals_the_sweep_on_seeded_tracks(fps, invalid):
    T = 12000
    duration = T / fps
    index = _index(71, duration, 150, duration / 100, invalid)
    assert (len(index.scoring_sets(M, "chan0")[0]) > 0) == invalid
    for seed in (3, 4):
        p = recipe.make_prob_track(seed, T).astype(np.float32)
        p[100:260] = np.nan                                                         # NaN blocks
        p[5000:5003] = np.nan
        p[300:310] = 1.5                                                            # above 1, at and below 0
        p[400:420] = -0.1
        p[430] = 0.0
        p[:5] = 0.99                                                                # a run that touches each end
        p[-7:] = 0.99
        levels = sorted(set(np.linspace(0.0, 1.0, 129).tolist() + [float(p[1000]), 0.5]))
        assert len(levels) == 130 and levels[0] == 0.0 and levels[-1] == 1.0 and float(p[1000]) in levels
        levels = levels[:64] + [(levels[63] + levels[64]) / 2] + levels[64:]
        assert len(levels) == 131
        got = _both([p], [(M, "chan0")], levels, MIN_LENGTHS, fps, index)
        assert (got.sum(axis=(0, 1, 2))[:3] > 0).all() and got[0, 0, 0, 0] > 0 and not got[0, -1].any()


HAND = {
    "constant": [0.6] * 12,
    "ramp up": [i / 20 for i in range(1, 21)],
    "ramp down": [i / 20 for i in range(20, 0, -1)],
    "plateau tie": [.2, .6, .6, .2, .6, .1, .1, .9],
    "all NaN": [float("nan")] * 9,
    "single frame": [0.7],
    "two frames": [0.7, 0.3],
    "equal to a level": [0.1, 0.5, 0.5, 0.25, 0.75, 0.75, 0.75, 0.5, 0.1, 1.0, 1.0, 0.0, 0.3],
    "nested": [.1, .3, .5, .7, .9, .7, .5, .8, .8, .5, .3, .35, .3, .1, .0, .6, float("nan"), .6, .6, .2] * 2,
}


@pytest.mark.parametrize("name", list(HAND))
def test_surface_host_equals_the_sweep_on_hand_written_tracks(name):
    import sweep_eval as se
    track = np.asarray(HAND[name], np.float64)
    assert 1 <= len(track) <= 40
    rows = [{"meeting_id": M, "part_id": "fe001", "chan": "chan0", "start": s, "end": e, "length": e - s, "type": k,
             "laugh_type": "laugh" if k == "laugh" else None}
            for k, s, e in (("laugh", 0.02, 0.3), ("speech", 0.05, 0.11), ("invalid", 0.07, 0.08), ("noise", 0.15, 0.4))]
    chans = [{"meeting_id": M, "part_id": "fe001", "chan": "chan0", "length": 0.35}]
    index = se.TranscriptIndex(rows, chans)
    for levels in ([0.0, 0.1, 0.25, 0.5, 0.6, 0.75, 0.9, 1.0], [0.0], [1.0], [i / 40 for i in range(41)]):
        for fps in (100.0, 2000.0):
            _both([track], [(M, "chan0")], levels, [-1.0, 0.0, 0.015, 0.05], fps, index)
    # strict >: a frame equal to a level is off at that level and on at the one below
    if name == "equal to a level":
        got = _both([track], [(M, "chan0")], [0.25, 0.5, 0.75], [-1.0], 100.0, index)
        assert got[0, :, 0, 0].tolist() == [4, 2, 1]            # runs of {p > .25}: 4; {p > .5}: 2; {p > .75}: the two frames at 1.0


def test_channel_without_a_participant_and_levels_that_are_refused():
    import sweep_eval as se
    index = _index(72, 40.0, 40, 0.5)
    p = recipe.make_prob_track(9, 4000)
    levels = [i / 16 for i in range(17)]
    got = _both([p, p], [(M, "chan0"), (M, "chanX")], levels, MIN_LENGTHS, 100.0, index)
    assert got[1, :, :, 0].sum() > 100 and np.array_equal(got[1, :, :, 0], got[1, :, :, 1]) and not got[1, :, :, 3:].any()
    assert got[1, :, :, 2].sum() > 0                                # (pred_ms: nothing is INVALID there; no class is hit, as in score_sweep_host)
    assert np.array_equal(got[0, :, :, 0], got[1, :, :, 0]) and got[0, :, :, 3:].any()
    for bad in ([0.5, 0.4], [0.5, 0.5], [0.1, float("nan")], [float("inf")]):
        with pytest.raises(ValueError, match="ascend strictly"):
            se.score_surface_host([p], [(M, "chan0")], bad, MIN_LENGTHS, 100.0, index)
    assert se.score_surface_host([p], [(M, "chan0")], [], MIN_LENGTHS, 100.0, index).shape == (1, 0, 3, 7)
    assert se.score_surface_host([np.zeros(0)], [(M, "chan0")], [0.5], [0.2], 100.0, index).tolist() == [[[[0] * 7]]]


def test_pr_summary_on_a_hand_computed_table():
    import sweep_eval as se
    nan = float("nan")
    rows = [[0.0, 0.0, 0.5, 0.5], [0.25, 0.0, 0.5, 0.5], [0.5, 0.0, 1.0, 0.25], [0.75, 0.0, 1.0, 0.0],       # threshold, min_len, P, R
            [0.0, 0.2, 0.5, nan], [0.25, 0.2, 1.0, nan], [0.5, 0.2, 1.0, nan], [0.75, 0.2, 1.0, nan]]
    got = se.pr_summary(rows)
    # AP = (.5 - .5) * .5 + (.5 - .25) * .5 + (.25 - 0) * 1 + (0 - 0) * 1; F1 = .5, .5, .4, 0: the best one first at threshold 0
    assert got[0] == [0.0, 0.375, 0.5, 0.0]
    assert got[1][0] == 0.2 and all(math.isnan(v) for v in got[1][1:]) and len(got) == 2
    assert se.PR_COLUMNS == ["min_len", "average_precision", "best_f1", "best_f1_threshold"]
    # the order of the rows does not matter, an inf recall is "nothing transcribed" too, and F1 is 0 where P = R = 0
    assert se.pr_summary(rows[::-1]) [0] == got[0]
    assert all(math.isnan(v) for v in se.pr_summary([[0.0, 0.1, 1.0, float("inf")]])[0][1:])
    assert se.pr_summary([[0.0, 0.1, 0.0, 0.0], [0.5, 0.1, 0.0, 0.0]]) == [[0.1, 0.0, 0.0, 0.0]]
    # a later, larger F1 wins: P = .25, R = 1 -> .4; P = .75, R = .75 -> .75 (2 * .5625 / 1.5, exact in binary)
    assert se.pr_summary([[0.1, 0.0, 0.25, 1.0], [0.6, 0.0, 0.75, 0.75]])[0][2:] == [0.75, 0.6]


def test_surface_size_queries_and_refusals_need_no_gpu():
    import _hip
    lib = _hip.lib()
    kmax, lmax, tile = lib.lad_surface_max_levels(), lib.lad_score_max_min_lengths(), lib.lad_surface_tile_frames()
    assert kmax == 4096 and tile > 0 and tile % 64 == 0
    assert lib.lad_surface_workspace_bytes(1, 1, 0, 1, 1) > 0
    small, big = lib.lad_surface_workspace_bytes(1, 36000, 1000, 131, 3), lib.lad_surface_workspace_bytes(10, 360000, 100000, kmax, 3)
    assert 0 < small < big and big >= 10 * (2 * 360000 * 2 + (kmax + 1) * 3 * 7 * 8) + 4 * 100000
    assert lib.lad_surface_workspace_bytes(65535, 1 << 20, 1 << 20, kmax, lmax) > 0
    assert lib.lad_surface_workspace_bytes(1, 1 << 30, 0, 1, 1) > 0
    for bad in ((0, 10, 10, 1, 1), (65536, 10, 10, 1, 1), (1, 0, 10, 1, 1), (1, (1 << 30) + 1, 10, 1, 1), (1, 10, -1, 1, 1),
                (1, 10, (1 << 30) + 1, 1, 1), (1, 10, 10, 0, 1), (1, 10, 10, kmax + 1, 1), (1, 10, 10, 1, 0), (1, 10, 10, 1, lmax + 1)):
        assert lib.lad_surface_workspace_bytes(*bad) == -1
        assert b"lad_surface_workspace_bytes" in lib.lad_last_error()
    # the levels are checked on the host before anything touches a device buffer: the pointers below are never followed
    fake = ctypes.c_void_p(256)
    i32p, f64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    offsets, bounds, fps, mls = np.zeros(6, np.int32), np.zeros((1, 2), np.int32), np.full(1, 100.0), (ctypes.c_double * 1)(0.2)

    def call(levels, dtype=0, K=None, L=1):
        lv = (ctypes.c_double * len(levels))(*levels)
        return lib.lad_score_surface(fake, dtype, 1, 1000, lv, len(levels) if K is None else K, fake, fake, bounds.ctypes.data_as(i32p),
                                     offsets.ctypes.data_as(i32p), 0, fake, fps.ctypes.data_as(f64p), mls, L, fake, fake, None)
    for levels, message in (([0.5, 0.4], b"ascend strictly"), ([0.5, 0.5], b"ascend strictly"), ([0.1, float("nan")], b"not finite"),
                            ([float("-inf"), 0.5], b"not finite")):
        assert call(levels) == _hip.LAD_ERR_INVALID and message in lib.lad_last_error(), lib.lad_last_error()
    assert call([0.5], dtype=7) == _hip.LAD_ERR_INVALID and b"dtype" in lib.lad_last_error()
    assert call([0.5], K=0) == _hip.LAD_ERR_INVALID and b"levels 1..4096" in lib.lad_last_error()
    assert call([0.5], L=lmax + 1) == _hip.LAD_ERR_INVALID and b"min_lengths 1.." in lib.lad_last_error()
    fps[0] = 0.0
    assert call([0.5]) == _hip.LAD_ERR_INVALID and b"positive finite" in lib.lad_last_error()
    fps[0] = 1e-4
    assert call([0.5]) == _hip.LAD_ERR_INVALID and b"millisecond overflow" in lib.lad_last_error()
    fps[0], offsets[5] = 100.0, 3
    assert call([0.5]) == _hip.LAD_ERR_INVALID and b"index offsets run" in lib.lad_last_error()


def test_surface_device_has_no_cpu_fallback():
    import _hip
    import sweep_eval as se
    index = _index(73, 10.0, 10, 0.5)
    ch = [(M, "chan0")]
    p = torch.rand(1000)
    for bad in (p, p.view(1, 1000), p.numpy(), p.double()):
        with pytest.raises(_hip.LadHipError):
            se.score_surface_device(bad, ch, [0.25, 0.5], [0.2], 100.0, index)


def _files(path):
    return {f: open(path / f, "rb").read() for f in sorted(os.listdir(path))}


def test_evaluate_sweep_threshold_grid_under_the_host_scorer(tmp_path):
    import csv

    import evaluate_sweep
    import sweep_eval as se
    args = sm.write_corpus(tmp_path)
    at = args.index("--thresholds")
    listed, base = args[at + 1], args[:at] + args[at + 2:]
    evaluate_sweep.main(base + ["--threshold_grid", "16", "--out_dir", str(tmp_path / "grid")])
    evaluate_sweep.main(base + ["--thresholds", ",".join(repr(i / 16) for i in range(17)), "--out_dir", str(tmp_path / "list")])
    grid, plain = _files(tmp_path / "grid"), _files(tmp_path / "list")
    assert list(plain) == ["eval_df_per_meeting.csv", "sum_stats.csv"]                      # without the flag: the old listing
    assert list(grid) == ["eval_df_per_meeting.csv", "pr_summary.csv", "sum_stats.csv"]
    assert grid["eval_df_per_meeting.csv"] == plain["eval_df_per_meeting.csv"] and grid["sum_stats.csv"] == plain["sum_stats.csv"]
    assert grid["eval_df_per_meeting.csv"].count(b"\n") == 1 + 2 * 17 * 2
    summary = list(csv.reader(open(tmp_path / "grid" / "pr_summary.csv")))
    stats = [[float(v) for v in r] for r in list(csv.reader(open(tmp_path / "grid" / "sum_stats.csv")))[1:]]
    assert summary[0] == se.PR_COLUMNS and [[float(v) for v in r] for r in summary[1:]] == se.pr_summary(stats)
    assert [float(r[0]) for r in summary[1:]] == [0.0, 0.2] and all(0 < float(r[1]) < 1 and 0 < float(r[2]) < 1 for r in summary[1:])
    # --lowpass goes in front of the tree as it goes in front of the list
    evaluate_sweep.main(base + ["--threshold_grid", "16", "--lowpass", "0.1", "--out_dir", str(tmp_path / "grid_lp")])
    evaluate_sweep.main(base + ["--thresholds", ",".join(repr(i / 16) for i in range(17)), "--lowpass", "0.1", "--out_dir",
                                str(tmp_path / "list_lp")])
    smooth = _files(tmp_path / "grid_lp")
    assert smooth["sum_stats.csv"] == _files(tmp_path / "list_lp")["sum_stats.csv"] != grid["sum_stats.csv"]
    # what the flag cannot be combined with
    for extra, sentence in ((["--thresholds", listed], "explicit --thresholds"), (["--offset_drops", "0.1"], "--offset_drops"),
                            (["--min_gaps", "0.1"], "--min_gaps"), (["--penalties", "1.0"], "--penalties"), (["--events"], "--events")):
        with pytest.raises(SystemExit, match="--threshold_grid cannot be combined with") as e:
            evaluate_sweep.main(base + ["--threshold_grid", "16", "--out_dir", str(tmp_path / "never")] + extra)
        assert sentence in str(e.value)
    assert not os.path.exists(tmp_path / "never")
    for bad in ("0", "4096", "-3", "x"):
        with pytest.raises(SystemExit):
            evaluate_sweep.build_parser().parse_args(base + ["--threshold_grid", bad, "--out_dir", "o"])
    assert evaluate_sweep.build_parser().parse_args(base + ["--threshold_grid", "4095", "--out_dir", "o"]).threshold_grid == 4095
    # the default threshold is what it was
    evaluate_sweep.main(base + ["--out_dir", str(tmp_path / "default")])
    evaluate_sweep.main(base + ["--thresholds", "0.5", "--out_dir", str(tmp_path / "half")])
    assert _files(tmp_path / "default") == _files(tmp_path / "half")


def test_surface_object_has_no_scratch(tmp_path):
    """The gfx950 code object of csrc/surface.hip: no private (scratch) segment in any of its six kernels."""
    import re
    import subprocess

    import _hip
    _hip.lib()
    llvm = "/opt/rocm/lib/llvm/bin"
    obj = os.path.join(os.path.dirname(os.path.abspath(_hip.__file__)), "csrc", "build", "surface.o")
    tools = [os.path.join(llvm, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    if not (os.path.exists(obj) and all(os.path.exists(t) for t in tools)):
        pytest.skip("no object file of surface.hip / no llvm tools in this tree")
    fb, co = tmp_path / "surface.fatbin", tmp_path / "surface.co"
    subprocess.run([tools[0], f"--dump-section=.hip_fatbin={fb}", obj], check=True, capture_output=True)
    subprocess.run([tools[1], "--type=o", "--unbundle", f"--input={fb}", f"--output={co}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"], check=True, capture_output=True)
    notes = subprocess.run([tools[2], "--notes", str(co)], capture_output=True, text=True, check=True).stdout
    scratch = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", notes)
    assert len(scratch) == 6 and set(scratch) == {"0"}, scratch      # bins (float32, float64), tree, cum, nodes, prefix
