"""Scoring the threshold sweep against transcript intervals (sweep_eval.py, csrc/score.hip), the part that needs no GPU: the
transcript index, the host scorer, the evaluation rows, the size queries, the script's flags and the code object.

The yardstick is the per-millisecond model of tests/_score_model.py (boolean arrays of milliseconds, the reference's loops
transcribed); every comparison is an equality."""
import csv
import math
import os

import numpy as np
import pytest
import torch

import _score_model as sm
from oracle import recipe

EVAL_THRESHOLDS = [float(t) for t in np.concatenate((np.linspace(0, 0.9, 19).round(2), np.linspace(0.91, 1, 10).round(2)))]
EVAL_MIN_LENGTHS = [0.0, 0.1, 0.2]
AWKWARD_FPS = 360000 / 3600.0049375


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


def _chans(meeting, parts, length, extra_unmapped=True):
    out = [{"meeting_id": meeting, "part_id": p, "chan": f"chan{i}", "length": length} for i, p in enumerate(parts)]
    if extra_unmapped:
        out.append({"meeting_id": meeting, "part_id": None, "chan": "chanX", "length": length})
    return out


def _mask(model, iv):
    m = np.zeros(model.N, bool)
    for lo, hi in iv:
        assert 0 <= lo < hi
        m[lo + 1:hi + 1] = True
    return m


def test_time_base_rounds_half_to_even():
    import sweep_eval as se
    assert [int(v) for v in se.to_frames([0.0005, 0.0015, 0.0025, 1.0, 2.3456])] == [0, 2, 2, 1000, 2346]
    assert [round(t * 1000.0) for t in (0.0005, 0.0015, 0.0025)] == [0, 2, 2]
    # fps = 2000: every odd frame lands on a half millisecond
    f = np.arange(8)
    assert [(int(i) / 2000.0) * 1000.0 for i in f] == [i / 2 for i in f]
    assert [round((int(i) / 2000.0) * 1000.0) for i in f] == [0, 0, 1, 2, 2, 2, 3, 4]
    assert [int(v) for v in se.to_frames(f / 2000.0)] == [0, 0, 1, 2, 2, 2, 3, 4]
    # the awkward fps: numpy.rint agrees with Python's round on the whole frame-to-millisecond map, and the map is monotone
    frames = np.arange(36001)
    ms = se.to_frames(frames / AWKWARD_FPS)
    assert ms.tolist() == [round((int(i) / AWKWARD_FPS) * 1000.0) for i in frames]
    assert (np.diff(ms) >= 0).all()


def test_transcript_index_against_the_set_model():
    import sweep_eval as se
    rows = sm.make_rows(1, "Bmr001", ["fe001", "me002", "me010"], 60.0) + sm.make_rows(2, "Bed002", ["mn003"], 60.0)
    # hand-placed rows: overlapping, adjacent, empty, half-way ends, a breath-laugh, a short laugh
    hand = [("laugh", 1.0, 2.0, "laugh"), ("laugh", 1.5, 2.5, "laugh"), ("laugh", 2.5, 3.0, "laugh"), ("laugh", 5.0, 5.0, "laugh"),
            ("laugh", 6.0, 6.1, "laugh"), ("laugh", 7.0, 8.0, "breath-laugh"), ("laugh", 0.0005, 0.0015, "laugh"),
            ("speech", 2.8, 4.0, None), ("noise", 3.9, 4.5, None), ("invalid", 1.9, 2.1, None), ("invalid", 9.0, 9.0, None)]
    for kind, s, e, lt in hand:
        rows.append({"meeting_id": "Bro003", "part_id": "fe004", "chan": "chan0", "start": s, "end": e,
                     "length": 0.5 if (s, e) == (0.0005, 0.0015) else e - s, "type": kind, "laugh_type": lt})
    chans = _chans("Bmr001", ["fe001", "me002", "me010"], 63.2185) + _chans("Bed002", ["mn003"], 50.0005) + _chans("Bro003", ["fe004", "me005"], 12.0)
    model = sm.Model(rows, chans, 70000)
    index = se.TranscriptIndex(rows, chans)
    assert index.meetings == ["Bed002", "Bmr001", "Bro003"]
    n_checked = 0
    for c in chans:
        m, chan, p = c["meeting_id"], c["chan"], c["part_id"]
        assert index.participant(m, chan) == p
        if p is None:
            assert index.intervals(m, chan) is None
            assert all(len(s) == 0 for s in index.scoring_sets(m, chan))
            continue
        got = index.intervals(m, chan)
        want = {"invalid": model.get(model.invalid, m, p), "laugh": model.get(model.laugh, m, p), "speech": model.get(model.speech, m, p),
                "noise": model.get(model.noise, m, p), "silence": model.silence[m][p]}
        assert list(got) == list(se.CLASSES)
        for k in se.CLASSES:
            iv = got[k]
            assert iv.dtype == np.int64 and iv.ndim == 2 and iv.shape[1] == 2
            assert (iv[:, 1] > iv[:, 0]).all() and (iv[1:, 0] > iv[:-1, 1]).all(), (m, chan, k)     # normalised: sorted, apart
            assert np.array_equal(_mask(model, iv), want[k]), (m, chan, k)
            n_checked += len(iv)
        # SILENCE is the complement within (0, to_frames(length)]
        full = model.oc(0, sm.to_frames(c["length"]))
        assert np.array_equal(_mask(model, got["silence"]), full & ~(want["invalid"] | want["laugh"] | want["speech"] | want["noise"]))
        # the scoring sets: INVALID taken out of the other four
        sets = index.scoring_sets(m, chan)
        for j, k in enumerate(se.CLASSES):
            assert np.array_equal(_mask(model, sets[j]), want[k] if j == 0 else want[k] & ~want["invalid"]), (m, chan, k)
    assert n_checked > 200                                   # (merged intervals of 4 x 160 seeded rows)
    for m in index.meetings:
        for kind, idx in (("invalid", model.invalid), ("laugh", model.laugh), ("speech", model.speech), ("noise", model.noise)):
            assert index.tot_len(m, kind) == model.tot(idx, m, "tot_len"), (m, kind)               # float sums in the same order
            assert index.tot_events(m, kind) == model.tot(idx, m, "tot_events"), (m, kind)
        assert index.num_laugh_rows(m) == model.laugh_rows.get(m, 0)
    # the hand-placed meeting, spelled out
    got = index.intervals("Bro003", "chan0")
    assert got["laugh"].tolist() == [[0, 2], [1000, 3000]]                 # 0.0005 -> 0, 0.0015 -> 2; overlapping + adjacent rows merged
    assert got["invalid"].tolist() == [[1900, 2100], [6000, 6100], [7000, 8000]]
    assert index.tot_events("Bro003", "laugh") == 4 and index.tot_events("Bro003", "invalid") == 5     # (the empty laugh row is short: invalid)
    assert index.tot_len("Bro003", "laugh") == 0.002 + 1.0 + 1.0 + 0.5          # a sum of row lengths, not of the union (2.002)
    assert index.num_laugh_rows("Bro003") == 7
    assert index.intervals("Bro003", "chan1")["silence"].tolist() == [[0, 12000]]      # a participant without any row
    assert index.scoring_sets("Bro003", "chan0")[1].tolist() == [[0, 2], [1000, 1900], [2100, 3000]]


def _instances(track, fps, thresholds=EVAL_THRESHOLDS, min_lengths=EVAL_MIN_LENGTHS):
    import laugh_segmenter as ls
    return ls.get_laughter_instances(track, thresholds, min_lengths, fps)


@pytest.mark.parametrize("fps", [100.0, AWKWARD_FPS, 2000.0])
def test_score_instances_against_the_set_model(fps):
    import sweep_eval as se
    T = 36000
    duration = T / fps
    for seed in (3, 4, 5):
        rows = sm.make_rows(seed, "Bmr001", ["fe001"], duration * 1.05, n_per_type=60, max_len_s=duration / 40)
        chans = _chans("Bmr001", ["fe001"], duration * 0.97)                # the transcript runs past the end of the channel
        N = sm.to_frames(duration * 1.05 + duration / 40) + 10
        model, index = sm.Model(rows, chans, N), se.TranscriptIndex(rows, chans)
        inst = _instances(recipe.make_prob_track(seed, T), fps)
        got = se.score_instances(inst, index, "Bmr001", "chan0")
        assert list(got) == list(inst) and len(got) == 87
        busy = 0
        for key, spans in inst.items():
            want = model.score(spans, "Bmr001", "chan0")
            assert got[key] == want, (seed, fps, key, got[key], want)
            assert all(type(v) is int for v in got[key])
            busy += all(v > 0 for v in want)
        assert busy >= 20                                                   # (the comparison saw every field at work)


def _one_channel_index(rows, length=10.0):
    import sweep_eval as se
    full = [{"meeting_id": "Bmr001", "part_id": "fe001", "chan": "chan0", "start": s, "end": e, "length": e - s, "type": k,
             "laugh_type": "laugh" if k == "laugh" else None} for k, s, e in rows]
    chans = _chans("Bmr001", ["fe001"], length)
    return se.TranscriptIndex(full, chans), sm.Model(full, chans, 30000)


def test_hand_written_cases():
    import sweep_eval as se
    inst = {(0.5, 0.2): [(1.0, 2.0), (3.0, 3.0), (4.0, 4.5)], (0.5, 0.0): []}

    def both(index, model, d=inst, chan="chan0"):
        got = se.score_instances(d, index, "Bmr001", chan)
        for k, spans in d.items():
            assert got[k] == model.score(spans, "Bmr001", chan), k
        return got
    # no intervals at all: everything predicted is silence, and a zero-length prediction counts as valid
    index, model = _one_channel_index([])
    assert both(index, model) == {(0.5, 0.2): (3, 3, 1500, 0, 0, 0, 1500), (0.5, 0.0): (0, 0, 0, 0, 0, 0, 0)}
    # INVALID covers the whole track
    index, model = _one_channel_index([("invalid", 0.0, 10.0), ("laugh", 1.0, 2.0)])
    assert both(index, model)[(0.5, 0.2)] == (3, 0, 0, 0, 0, 0, 0)
    # a prediction half inside INVALID; the zero-length one is contained in a non-empty INVALID
    index, model = _one_channel_index([("invalid", 1.5, 3.5), ("speech", 0.0, 1.2)])
    assert both(index, model)[(0.5, 0.2)] == (3, 2, 1000, 0, 200, 0, 800)
    # a laugh interval overlapping an invalid one
    index, model = _one_channel_index([("laugh", 0.5, 1.8), ("invalid", 1.6, 1.7), ("noise", 4.2, 4.3)])
    assert both(index, model)[(0.5, 0.2)] == (3, 2, 1400, 700, 0, 100, 600)
    # intervals past the end of the track (SILENCE ends with the channel; what is predicted beyond it is in no class)
    index, model = _one_channel_index([("laugh", 4.4, 20.0)], length=4.2)
    assert both(index, model)[(0.5, 0.2)] == (3, 3, 1500, 100, 0, 0, 1200)
    # a channel without a participant: nothing to compare with
    assert se.score_instances(inst, index, "Bmr001", "chanX")[(0.5, 0.2)] == (3, 3, 1500, 0, 0, 0, 0)


def test_eval_rows_and_sum_stats():
    import sweep_eval as se
    T, fps = 6000, 100.0
    rows = sm.make_rows(7, "Bmr001", ["me010", "fe001", "me002"], 60.0) + sm.make_rows(8, "Bed002", ["mn003"], 60.0)
    rows = [r for r in rows if not (r["meeting_id"] == "Bed002" and r["type"] == "laugh")]              # a meeting without laughs
    chans = _chans("Bmr001", ["me010", "fe001", "me002"], 60.0) + _chans("Bed002", ["mn003"], 60.0) + _chans("Bns003", ["fe009"], 60.0)
    index, model = se.TranscriptIndex(rows, chans), sm.Model(rows, chans, 70000)
    channels = [(c["meeting_id"], c["chan"]) for c in chans]
    tracks = [recipe.make_prob_track(20 + i, T) for i in range(len(channels))]
    tracks[-2] = np.zeros(T)                                                                             # Bns003: no predictions at all
    thresholds, min_lengths = [0.3, 0.5, 0.99], [0.2, 0.0]
    scores = se.score_sweep_host(tracks, channels, thresholds, min_lengths, fps, index)
    assert scores.shape == (len(channels), 3, 2, 7) and scores.dtype == np.int64
    got = se.eval_rows(scores, channels, thresholds, min_lengths, index)
    assert se.EVAL_COLUMNS == ["meeting", "threshold", "min_len", "precision", "recall", "corr_pred_time", "tot_pred_time",
                               "tot_transc_laugh_time", "num_of_pred_laughs", "valid_pred_laughs", "num_of_transc_laughs",
                               "tot_fp_speech_time", "tot_fp_noise_time", "tot_fp_silence_time"]
    want = []
    for m in ("Bed002", "Bmr001", "Bns003"):
        for thr in thresholds:
            for min_l in min_lengths:
                per_part = {}
                for (mm, chan), track in zip(channels, tracks):
                    p = model.chan_to_part.get(mm, {}).get(chan)
                    if mm == m and p is not None:
                        per_part[p] = model.score(_instances(track, fps, [thr], [min_l])[(thr, min_l)], m, chan)
                want.append(model.eval_preds(per_part, m, thr, min_l))
    assert len(got) == len(want) == 18
    for g, w in zip(got, want):
        assert len(g) == 14 and g[:4] == w[:4] and g[5:] == w[5:], (g, w)
        assert g[4] == w[4] or (math.isnan(g[4]) and math.isnan(w[4])), (g, w)
    bed, bmr, bns = got[0], got[6], got[12]
    assert math.isnan(bed[4]) and bed[7] == 0 and bed[10] == 0                                          # no laughs: recall NaN
    assert bmr[8] > 10 and 0 < bmr[3] < 1 and bmr[6] > bmr[5] > 0
    assert bns[3] == 1 and bns[8] == 0 and bns[6] == 0                                                   # no predictions: precision 1
    # the participant order matters to the float sums: the three of Bmr001 added in channel order give other bits somewhere
    stats = se.calc_sum_stats(got)
    assert se.SUM_COLUMNS == ["threshold", "min_len", "precision", "recall"]
    assert [(s[1], s[0]) for s in stats] == sorted((min_l, thr) for thr in thresholds for min_l in min_lengths)
    for thr, min_l, prec, recall in stats:
        sel = [r for r in want if r[1] == thr and r[2] == min_l]
        corr, pred, transc = 0, 0, 0
        for r in sel:
            corr, pred, transc = corr + r[5], pred + r[6], transc + r[7]
        assert prec == (1 if pred == 0 else corr / pred) and recall == corr / transc
    assert se.calc_sum_stats([["m", 0.5, 0.2, 1, float("nan"), 0, 0, 0, 0, 0, 0, 0, 0, 0]])[0][2] == 1.0


def test_score_size_queries_need_no_gpu():
    import _hip
    lib = _hip.lib()
    lmax, kmax = lib.lad_score_max_min_lengths(), lib.lad_runs_max_thresholds()
    assert lmax >= 8
    assert lib.lad_score_workspace_bytes(1, 0, 1, 1) > 0
    small, big = lib.lad_score_workspace_bytes(1, 1000, 29, 3), lib.lad_score_workspace_bytes(10, 100000, 29, 3)
    assert 0 < small < big and big >= 4 * 100000 + 8 * 10 * 29
    assert lib.lad_score_workspace_bytes(65535, 1 << 20, kmax, lmax) > 0
    for bad in ((0, 10, 1, 1), (65536, 10, 1, 1), (1, -1, 1, 1), (1, (1 << 30) + 1, 1, 1), (1, 10, 0, 1), (1, 10, kmax + 1, 1),
                (1, 10, 1, 0), (1, 10, 1, lmax + 1)):
        assert lib.lad_score_workspace_bytes(*bad) == -1
        assert b"lad_score_workspace_bytes" in lib.lad_last_error()


def test_device_scorer_has_no_cpu_fallback():
    import _hip
    import sweep_eval as se
    index, _ = _one_channel_index([("laugh", 1.0, 2.0)])
    ch = [("Bmr001", "chan0")]
    p = torch.rand(1000)
    for bad in (p, p.view(1, 1000), p.numpy(), p.double()):
        with pytest.raises(_hip.LadHipError):
            se.score_sweep_device(bad, ch, [0.5], [0.2], 100.0, index)
    # the host route is untouched by that
    assert se.score_sweep_host([np.full(300, 0.9)], ch, [0.5], [0.2], 100.0, index)[0, 0, 0].tolist() == [1, 1, 2990, 1000, 0, 0, 1990]


def test_evaluate_sweep_script_flags_and_host_run(tmp_path):
    import evaluate_sweep
    parser = evaluate_sweep.build_parser()
    base = ["--probs_dir", "p", "--transcripts", "t.csv", "--channels", "c.csv", "--out_dir", "o"]
    assert parser.parse_args(base).scorer == "host"
    assert parser.parse_args(base + ["--scorer", "device"]).scorer == "device"
    for bad in ("gpu", "Device", ""):
        with pytest.raises(SystemExit):
            parser.parse_args(base + ["--scorer", bad])
    args = sm.write_corpus(tmp_path)
    evaluate_sweep.main(args + ["--out_dir", str(tmp_path / "out")])
    rows = list(csv.reader(open(tmp_path / "out" / "eval_df_per_meeting.csv")))
    import sweep_eval as se
    assert rows[0] == se.EVAL_COLUMNS and len(rows) == 1 + 2 * 3 * 2
    assert [r[0] for r in rows[1:]] == ["Bed002"] * 6 + ["Bmr001"] * 6
    assert any(int(r[8]) > 0 and 0 < float(r[3]) < 1 for r in rows[1:])
    stats = list(csv.reader(open(tmp_path / "out" / "sum_stats.csv")))
    assert stats[0] == se.SUM_COLUMNS and len(stats) == 1 + 6


def test_score_object_has_no_scratch_and_no_scalar_memory_writes(tmp_path):
    """The gfx950 code object of csrc/score.hip: no private (scratch) segment in either kernel; memory is written by vector global
    stores and vector global atomics only -- no scalar-unit instruction that stores, does an atomic or writes its cache back."""
    import re
    import subprocess

    import _hip
    _hip.lib()
    llvm = "/opt/rocm/lib/llvm/bin"
    obj = os.path.join(os.path.dirname(os.path.abspath(_hip.__file__)), "csrc", "build", "score.o")
    tools = [os.path.join(llvm, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump", "llvm-readelf")]
    if not (os.path.exists(obj) and all(os.path.exists(t) for t in tools)):
        pytest.skip("no object file of score.hip / no llvm tools in this tree")
    fb, co = tmp_path / "score.fatbin", tmp_path / "score.co"
    subprocess.run([tools[0], f"--dump-section=.hip_fatbin={fb}", obj], check=True, capture_output=True)
    subprocess.run([tools[1], "--type=o", "--unbundle", f"--input={fb}", f"--output={co}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"], check=True, capture_output=True)
    notes = subprocess.run([tools[3], "--notes", str(co)], capture_output=True, text=True, check=True).stdout
    scratch = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", notes)
    assert len(scratch) == 2 and set(scratch) == {"0"}, scratch                      # the scan and the row kernel
    dis = subprocess.run([tools[2], "-d", "--mcpu=gfx950", str(co)], capture_output=True, text=True, check=True).stdout
    mnemonics = set(re.findall(r"^\s+([a-z][a-z0-9_]+)", dis, flags=re.M))
    writes = {m for m in mnemonics if "store" in m or "atomic" in m}
    assert writes and all(m.startswith("global_store_") or m.startswith("global_atomic_add") for m in writes), writes
    assert any(m.startswith("global_atomic_add_x2") for m in writes)                # the int64 accumulator
    assert not any(m.startswith("s_") and ("store" in m or "atomic" in m or "dcache" in m) for m in mnemonics)
    assert not any(m.startswith("scratch_") for m in mnemonics)
    assert "v_div_fixup_f64" in mnemonics and "v_rndne_f64" in {m.split("_e")[0] for m in mnemonics}   # IEEE division, rint
