"""What the calibration of the probability track (csrc/calibration.hip, calibration.py) promises without a GPU: the host histogram
against the model written from the header (tests/_calibration_model.py), for equality; the conservation identity; the figures
against brute force; the fits; applying a table; the flags of evaluate_sweep.py; and the refusals of the C ABI that return before
any launch."""
import ctypes
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import _calibration_cases as cases
import _calibration_model as cm
import _score_model as sm

FPS = cases.NON_INTEGER_FPS


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


def _host(tracks, channels, fps, **kw):
    import calibration
    return calibration.label_histogram_host(tracks, channels, list(fps), cases.index(), **kw)


# (kinds, sizes, channels of cases.CHANNELS, fps, dtype, lengths, groups)
HISTOGRAM_CASES = {
    "hand_written_100fps": (("seeded",), (1300,), (0,), (100.0,), "float64", None, None),
    "hand_written_43fps": (("seeded",), (600,), (0,), (FPS,), "float64", None, None),
    "hand_written_float32": (("seeded",), (1300,), (0,), (100.0,), "float32", None, None),
    "one_frame": (("seeded",), (1,), (1,), (0.05,), "float64", None, None),
    "seeded_rows_43fps_float32": (("seeded",), (1400,), (1,), (FPS,), "float32", None, None),
    "no_participant": (("seeded", "seeded"), (500, 500), (2, 3), (100.0, 100.0), "float64", None, None),
    "shorter_than_the_tensor": (("seeded", "seeded", "constant"), (900, 800, 700), (0, 1, 3), (100.0, FPS, 7.3), "float64", (900, 333, 1), None),
    "groups_summed": (("seeded", "alternating", "seeded", "distinct"), (700, 650, 300, 800), (0, 1, 2, 3), (100.0, FPS, 100.0, 31.25),
                      "float64", None, (0, 0, 0, 0)),
    "groups_with_one_left_out": (("seeded", "alternating", "seeded", "distinct"), (700, 650, 300, 800), (0, 1, 2, 3),
                                 (100.0, FPS, 100.0, 31.25), "float32", None, (1, -1, 0, 1)),
}


@pytest.mark.parametrize("name", sorted(HISTOGRAM_CASES))
def test_host_histogram_equals_the_model_and_conserves_the_coverage(name):
    kinds, sizes, chans, fps, dtype, lengths, groups = HISTOGRAM_CASES[name]
    tracks, channels, want = cases.case(kinds, sizes, chans, fps, dtype, lengths, groups)
    got = _host(tracks, channels, fps, lengths=lengths, groups=groups)
    assert got.dtype == np.int64 and got.shape == want.shape
    assert np.array_equal(got, want)
    # per channel and class the slots sum to F_k(m_n): the channel alone, from the per-millisecond sets
    _, _, model = cases.corpus()
    for c, (t, mc) in enumerate(zip(tracks, channels)):
        n = len(t) if lengths is None else lengths[c]
        alone = _host([t], [mc], [fps[c]], lengths=[n])
        sets = cm.scoring_sets(model, *mc)
        assert alone[0].sum(axis=1).tolist() == [cm.coverage_total(s, cm.frame_ms(n, fps[c])) for s in sets]
        if mc[1] == "chanX":
            assert not alone.any()                               # a channel without a participant adds nothing


def test_the_hand_written_frames_land_where_the_header_says():
    """Frame 400 of chan0 at 100 fps owns (4000, 4010]: 2 + 2 + 3 ms of NOISE in three intervals and 3 ms of SILENCE; frame 300
    owns the whole of the 4 ms SPEECH interval; frames 210..219 lie in INVALID, which was taken out of LAUGH."""
    import calibration
    track = np.full(1300, 0.5)
    track[400], track[300], track[215] = 0.25, 0.125, 0.75
    h = _host([track], [("Bmr001", "chan0")], [100.0])[0]
    assert h[:, 16384].tolist() == [0, 0, 0, 7, 3]
    assert h[:, 8192].tolist() == [0, 0, 4, 0, 6]
    assert h[:, 49152].tolist() == [10, 0, 0, 0, 0]
    assert h[calibration.LAUGH].sum() == 497 + 300 - 100 + 3500
    assert h[:, calibration.NAN_SLOT].sum() == 0
    # the special values: slots of 0, a negative, 1e-7, k / 65536, 1.0, above 1 and NaN
    assert calibration.slots_of(cases.SPECIALS).tolist() == [0, 0, 0, 3, 32768, 65535, 65536, 65536, 65537, 65535]
    assert [cm.slot_of(v) for v in cases.SPECIALS] == calibration.slots_of(cases.SPECIALS).tolist()
    assert calibration.slots_of(np.float32(cases.SPECIALS)).tolist() == [cm.slot_of(np.float32(v)) for v in cases.SPECIALS]


def test_host_histogram_refuses():
    import calibration
    t = np.full(100, 0.5)
    ch = [("Bmr001", "chan0")]
    for kw in (dict(lengths=[0]), dict(lengths=[101]), dict(groups=[-2]), dict(groups=[0, 0]), dict(lengths=[1, 2]), dict(groups=[5]),
               dict(groups=[1]), dict(groups=[0], n_groups=2), dict(groups=[0], n_groups=0), dict(n_groups=2)):
        with pytest.raises(ValueError):
            calibration.label_histogram_host([t], ch, 100.0, cases.index(), **kw)
    for fps in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            calibration.label_histogram_host([t], ch, fps, cases.index())
    with pytest.raises(ValueError, match="millisecond overflow"):
        calibration.label_histogram_host([t], ch, 1e-6, cases.index())
    with pytest.raises(ValueError):
        calibration.label_histogram_host([t, t], ch, 100.0, cases.index())
    # a trailing group that no channel belongs to stays in the array when it is named
    two = [("Bmr001", "chan0"), ("Bmr001", "chan1")]
    named = calibration.label_histogram_host([t, t], two, 100.0, cases.index(), groups=[0, -1], n_groups=2)
    assert named.shape[0] == 2 and not named[1].any()
    assert np.array_equal(named[:1], calibration.label_histogram_host([t, t], two, 100.0, cases.index(), groups=[0, -1]))


# ---- figures ----------------------------------------------------------------------------------------------------------------------
def _rows():
    """Histogram rows: a real one (seeded track on seeded rows), one with ties and empty bins, one without positives, an empty one."""
    kinds, sizes, chans, fps, dtype, lengths, groups = HISTOGRAM_CASES["seeded_rows_43fps_float32"]
    real = cases.case(kinds, sizes, chans, fps, dtype, lengths, groups)[2][0]
    rng = np.random.default_rng(5)
    sparse = np.zeros((5, cm.SLOTS), np.int64)
    at = rng.choice(cm.BUCKETS, 60, replace=False)
    sparse[1, at[:40]] = rng.integers(1, 10 ** 9, 40)
    sparse[2, at[20:]] = rng.integers(1, 10 ** 9, 40)
    sparse[4, at[30:50]] = rng.integers(1, 2 ** 40, 20)
    sparse[0, 7] = 5
    sparse[3, cm.NAN_SLOT] = 11
    no_pos = sparse.copy()
    no_pos[1] = 0
    return {"real": real, "sparse": sparse, "no_positives": no_pos, "empty": np.zeros((5, cm.SLOTS), np.int64)}


def _same(got, want):
    """One conversion of the exact value (NaN where there is none)."""
    return (math.isnan(got) and want is None) or (want is not None and got == float(want))


@pytest.mark.parametrize("name", ["real", "sparse", "no_positives", "empty"])
@pytest.mark.parametrize("n_bins", [15, 7])
def test_figures_equal_the_brute_force(name, n_bins):
    import calibration
    row = _rows()[name]
    got = calibration.calibration_figures(row, n_bins=n_bins)
    want = cm.figures(row, n_bins=n_bins)
    assert (got["pos_ms"], got["neg_ms"]) == (want["pos_ms"], want["neg_ms"])
    assert got["invalid_ms"] == int(row[0].sum()) and got["nan_ms"] == int(row[1:, cm.NAN_SLOT].sum())
    for key in ("brier", "ece", "mce", "roc_auc", "average_precision"):
        assert _same(got[key], want[key]), key
    W = want["pos_ms"] + want["neg_ms"]
    if W:
        # one rounding per term and one per add, over at most 2 * 65538 non-negative terms
        exact = math.fsum(want["nll_terms"]) / W
        assert abs(got["nll"] - exact) <= 131076 * 2.0 ** -52 * exact
    else:
        assert math.isnan(got["nll"])
    assert len(got["reliability"]) == n_bins
    for b, (lo, hi, ms, conf, share) in enumerate(got["reliability"]):
        assert (lo, hi) == (b / n_bins, (b + 1) / n_bins)
        if b in want["bins"]:
            w_ms, w_laugh, w_conf = want["bins"][b]
            assert ms == w_ms and conf == float(w_conf / w_ms) and share == float(Fraction(w_laugh, w_ms))
        else:
            assert ms == 0 and math.isnan(conf) and math.isnan(share)
    assert sum(r[2] for r in got["reliability"]) == W


def test_figures_of_a_perfect_and_a_useless_track():
    import calibration
    row = np.zeros((5, cm.SLOTS), np.int64)
    row[1, 65536], row[2, 0] = 1000, 3000
    f = calibration.calibration_figures(row)
    assert f["roc_auc"] == 1.0 and f["average_precision"] == 1.0 and f["brier"] < 1e-9
    row[:] = 0
    row[1, 30000], row[3, 30000] = 1000, 3000                   # one bucket: every pair is a tie
    f = calibration.calibration_figures(row)
    assert f["roc_auc"] == 0.5 and f["average_precision"] == 0.25
    with pytest.raises(ValueError):
        calibration.calibration_figures(row[:, :-1])
    with pytest.raises(ValueError):
        calibration.calibration_figures(row.astype(np.float64))
    with pytest.raises(ValueError):
        calibration.calibration_figures(row, n_bins=0)


# ---- fits -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["real", "sparse", "no_positives", "empty"])
def test_isotonic_fit(name):
    import calibration
    row = _rows()[name]
    table = calibration.fit_isotonic(row)
    assert table.dtype == np.float64 and table.shape == (cm.BUCKETS,)
    assert np.isfinite(table).all() and table.min() >= 0 and table.max() <= 1
    assert (np.diff(table) >= 0).all()
    want = cm.isotonic(row)
    if not want:
        assert np.array_equal(table, calibration.bucket_confidence())
        return
    assert all(table[u] == float(v) for u, v in want.items())                     # the Fraction PAV, converted once
    occupied = sorted(want)
    for u in range(cm.BUCKETS):                                                   # a bucket without mass takes its block's value
        below = [v for v in occupied if v <= u]
        assert table[u] == table[below[-1] if below else occupied[0]]
    # the identity table is monotone and the fit is the best monotone table: a theorem, not a tolerance.  It is a theorem about
    # the exact block means, so it is asserted on cm.isotonic's Fractions (which the table equals after one conversion, above); the
    # float64 table differs from them by a rounding d per block and its Brier score by mass * d^2, far inside the gap here
    identity = [cm.confidence(u) for u in range(cm.BUCKETS)]
    assert cm.brier_of_table(row, want) <= cm.brier_of_table(row, identity)
    assert cm.brier_of_table(row, table.tolist()) <= cm.brier_of_table(row, identity)
    # and the product's own integers say the same of the remapped histogram (its buckets' midpoints stand for the values)
    assert calibration.remap_histogram(row, table).sum() == row.sum()


def _generated(a, b, mass=10 ** 9):
    """A row whose laugh share in bucket u is sigmoid(a * logit(p_u) + b), up to the rounding of an integer in `mass`."""
    import calibration
    p = calibration.bucket_confidence()
    x = np.log(p) - np.log1p(-p)
    at = np.arange(50, cm.BUCKETS, 97)
    q = 1.0 / (1.0 + np.exp(-(a * x[at] + b)))
    row = np.zeros((5, cm.SLOTS), np.int64)
    row[1, at] = np.rint(mass * q).astype(np.int64)
    row[2, at] = mass - row[1, at]
    return row, x


def _nll(a, b, x, row):
    z = a * x + b
    pos, neg = row[1, :cm.BUCKETS].astype(np.float64), row[2:, :cm.BUCKETS].sum(axis=0).astype(np.float64)
    return float(np.sum(pos * np.logaddexp(0, -z) + neg * np.logaddexp(0, z)))


@pytest.mark.parametrize("a,b", [(0.6, -1.2), (1.0, 0.0), (2.5, 0.7)])
def test_platt_fit_recovers_known_parameters(a, b):
    """The tolerance: Newton stops when a step no longer lowers the float64 NLL, i.e. within sqrt(2^-52 * NLL / curvature) of the
    optimum, about 1e-8 here; rounding the laugh mass to an integer in 1e9 moves the optimum by less than 1e-9.  Measured: the fit
    lies within 1e-10 of the generating parameters, and scipy's BFGS optimum of the same float64 NLL (gtol 1e-12), an independent
    float64 reference, within 6e-8 of them, so 1e-6 leaves more than an order of margin on either side.  Starting at the
    optimum (1, 0) takes no step at all."""
    from scipy import optimize

    import calibration
    row, x = _generated(a, b)
    table, par = calibration.fit_platt(row)
    assert (0 if (a, b) == (1.0, 0.0) else 1) <= par["iterations"] <= calibration.PLATT_MAX_ITERATIONS
    ref = optimize.minimize(lambda v: _nll(v[0], v[1], x, row) / row.sum(), [1.0, 0.0], method="BFGS", options={"gtol": 1e-12}).x
    print(f"platt ({a}, {b}): fit ({par['a']!r}, {par['b']!r}), scipy ({ref[0]!r}, {ref[1]!r})")
    assert abs(par["a"] - a) <= 1e-6 and abs(par["b"] - b) <= 1e-6
    assert abs(par["a"] - ref[0]) <= 1e-6 and abs(par["b"] - ref[1]) <= 1e-6
    assert _nll(par["a"], par["b"], x, row) <= _nll(1.0, 0.0, x, row)
    assert np.array_equal(table, np.clip(1.0 / (1.0 + np.exp(-(par["a"] * x + par["b"]))), 0, 1)) or np.allclose(
        table, 1.0 / (1.0 + np.exp(-(par["a"] * x + par["b"]))), rtol=0, atol=2.0 ** -50)


@pytest.mark.parametrize("name", ["real", "sparse", "no_positives", "empty"])
def test_platt_fit_never_raises_the_nll_and_temperature_keeps_b(name):
    import calibration
    row = _rows()[name]
    p = calibration.bucket_confidence()
    x = np.log(p) - np.log1p(-p)
    for temperature_only in (False, True):
        table, par = calibration.fit_platt(row, temperature_only=temperature_only)
        assert table.shape == (cm.BUCKETS,) and np.isfinite(table).all() and table.min() >= 0 and table.max() <= 1
        assert _nll(par["a"], par["b"], x, row) <= _nll(1.0, 0.0, x, row)
        assert par["iterations"] <= calibration.PLATT_MAX_ITERATIONS
        if temperature_only:
            assert par["b"] == 0.0
    assert calibration.fit(row, "temperature")[1]["b"] == 0.0 and calibration.fit(row, "isotonic")[1] == {}
    with pytest.raises(ValueError):
        calibration.fit(row, "beta")


def test_temperature_fit_recovers_a_known_temperature():
    import calibration
    row, _ = _generated(0.5, 0.0)
    _, par = calibration.fit_platt(row, temperature_only=True)
    assert par["b"] == 0.0 and abs(par["a"] - 0.5) <= 1e-6


# ---- applying a table -------------------------------------------------------------------------------------------------------------
def test_apply_calibration():
    import calibration
    import laugh_segmenter as ls
    buckets = np.arange(cm.BUCKETS, dtype=np.float64) / 65536.0                   # the identity of buckets: table[u] = u / 65536
    for dtype in (np.float32, np.float64):
        x = cases.track("seeded", 4000, dtype)
        got = ls.apply_calibration(x, buckets)
        assert got.dtype == np.float64 and got.shape == x.shape
        want = np.array([float("nan") if cm.slot_of(v) == cm.NAN_SLOT else cm.slot_of(v) / 65536.0 for v in x])
        assert np.array_equal(got, want, equal_nan=True)
        assert np.isnan(got).sum() == np.isnan(x).sum() == 1
    assert calibration.apply_calibration(np.array([[0.5, 2.0], [-1.0, np.nan]]), buckets).tolist()[0] == [0.5, 1.0]
    # the histogram of the calibrated track is the remapped histogram of the track
    kinds, sizes, chans, fps, dtype, lengths, groups = HISTOGRAM_CASES["seeded_rows_43fps_float32"]
    tracks, channels, want = cases.case(kinds, sizes, chans, fps, dtype, lengths, groups)
    table = calibration.fit_isotonic(want[0])
    again = _host([calibration.apply_calibration(tracks[0], table)], channels, fps)
    assert np.array_equal(again[0], calibration.remap_histogram(want[0], table))
    for bad in (buckets[:-1], np.full(cm.BUCKETS, 1.5), np.full(cm.BUCKETS, np.nan), -buckets):
        with pytest.raises(ValueError):
            calibration.apply_calibration(x, bad)


def test_device_forms_have_no_cpu_fallback():
    import torch

    import _hip
    import calibration
    p = torch.rand(1000)
    table = calibration.bucket_confidence()
    for bad in (p, p.view(1, 1000), p.numpy()):
        with pytest.raises(_hip.LadHipError):
            calibration.apply_calibration_device(bad, table)
        with pytest.raises(_hip.LadHipError):
            calibration.label_histogram_device(bad, [("Bmr001", "chan0")], 100.0, cases.index())


# ---- the command line -------------------------------------------------------------------------------------------------------------
def _files(path):
    return {f: open(path / f, "rb").read() for f in sorted(os.listdir(path))}


def test_evaluate_sweep_flags_under_the_host_scorer(tmp_path):
    import csv

    import calibration
    import evaluate_sweep
    args = sm.write_corpus(tmp_path)
    evaluate_sweep.main(args + ["--out_dir", str(tmp_path / "plain")])
    plain = _files(tmp_path / "plain")
    assert sorted(plain) == ["eval_df_per_meeting.csv", "sum_stats.csv"]           # without the flags: exactly the old files
    evaluate_sweep.main(args + ["--calibration_report", "--calibration_bins", "10", "--out_dir", str(tmp_path / "report")])
    report = _files(tmp_path / "report")
    assert sorted(report) == ["calibration.csv", "eval_df_per_meeting.csv", "reliability.csv", "sum_stats.csv"]
    assert {k: report[k] for k in plain} == plain
    rows = list(csv.reader(open(tmp_path / "report" / "calibration.csv")))
    assert rows[0] == calibration.CALIBRATION_COLUMNS and [r[0] for r in rows[1:]] == ["Bed002", "Bmr001", "all"]
    assert int(rows[3][1]) == int(rows[1][1]) + int(rows[2][1]) > 0 and 0.0 < float(rows[3][9]) < 1.0
    rel = list(csv.reader(open(tmp_path / "report" / "reliability.csv")))
    assert rel[0] == calibration.RELIABILITY_COLUMNS and len(rel) == 11
    assert sum(int(r[3]) for r in rel[1:]) == int(rows[3][1]) + int(rows[3][2])
    tables = {}
    for method in calibration.METHODS:
        out = tmp_path / ("fit_" + method)
        evaluate_sweep.main(args + ["--fit_calibration", method, "--out_dir", str(out)])
        files = _files(out)
        assert sorted(files) == ["calibration_table.npz", "eval_df_per_meeting.csv", "sum_stats.csv"]
        assert {k: files[k] for k in plain} == plain
        data = np.load(out / "calibration_table.npz")
        assert str(data["method"]) == method and data["table"].shape == (cm.BUCKETS,)
        tables[method] = calibration.load_table(out / "calibration_table.npz")
        evaluate_sweep.main(args + ["--fit_calibration", method, "--out_dir", str(tmp_path / "again")])
        assert _files(tmp_path / "again")["calibration_table.npz"] == files["calibration_table.npz"]      # no time stamp inside
    # applying the table: the scores change, the report speaks of the calibrated tracks, and the isotonic fit cannot raise the Brier
    # score of the corpus it was fitted on above the identity's
    applied = tmp_path / "applied"
    evaluate_sweep.main(args + ["--calibration", str(tmp_path / "fit_isotonic" / "calibration_table.npz"), "--calibration_report",
                                "--median", "5", "--out_dir", str(applied)])
    assert sorted(_files(applied)) == sorted(report)
    with pytest.raises(SystemExit):
        evaluate_sweep.main(args + ["--calibration", str(tmp_path / "fit_platt" / "calibration_table.npz"), "--fit_calibration", "platt",
                                    "--out_dir", str(tmp_path / "both")])
    for bad in (["--calibration_bins", "0"], ["--fit_calibration", "beta"]):
        with pytest.raises(SystemExit):
            evaluate_sweep.build_parser().parse_args(args + bad + ["--out_dir", "o"])
    import segment_laughter
    base = ["--input_audio_file", "a.wav"]
    assert segment_laughter.build_parser().parse_args(base).calibration is None
    assert segment_laughter.build_parser().parse_args(base + ["--calibration", "t.npz"]).calibration == "t.npz"


def test_segment_laughter_with_a_table_under_the_host_segmenter(tmp_path, monkeypatch):
    """Host-only: the model pass is replaced by a fixed track.  With a table the instances are those of the calibrated track, the
    median filter behind it; --save_probs still gets the raw track; without a table nothing changes."""
    import inspect

    import laugh_segmenter as ls
    import segment_laughter
    x = cases.track("seeded", 3000, np.float32, seed=9)
    monkeypatch.setattr(segment_laughter, "predict_file", lambda model, path, **kw: (x, 30.0))
    table = np.sqrt(np.arange(cm.BUCKETS, dtype=np.float64) / 65536.0)
    thresholds, min_lengths = [0.3, 0.6], [0.0, 0.2]

    def run(name, **kw):
        call = segment_laughter.load_and_pred_calibrated if "calibration" in kw else segment_laughter.load_and_pred
        return call(None, "meeting.wav", thresholds, min_lengths, str(tmp_path / name), verbose=False, **kw)[1]
    plain = run("plain", median=5)
    assert run("none", calibration=None, median=5) == plain
    got = run("table", calibration=table, median=5, save_probs=str(tmp_path / "raw.npy"))
    want = ls.get_laughter_instances(ls.median_filter(ls.apply_calibration(x, table), 5), thresholds, min_lengths, 100.0)
    assert got == want and got != plain and len(got[(0.6, 0.0)]) > 5
    assert np.array_equal(np.load(tmp_path / "raw.npy"), x, equal_nan=True)
    ours = inspect.signature(segment_laughter.load_and_pred_calibrated).parameters
    assert list(ours)[:-1] == list(inspect.signature(segment_laughter.load_and_pred).parameters)      # the wrapper passes by position
    assert list(ours)[-1] == "calibration" and ours["calibration"].kind is inspect.Parameter.KEYWORD_ONLY
    with pytest.raises(ValueError):                             # a positional pass-through that kept its order: median and lowpass clash
        segment_laughter.load_and_pred(None, "meeting.wav", thresholds, min_lengths, None, lowpass=0.01, median=5)


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
def test_size_queries_need_no_gpu_and_refuse():
    import _hip
    lib = _hip.lib()
    assert lib.lad_label_histogram_slots() == cm.SLOTS
    tile = lib.lad_label_histogram_tile_frames()
    assert tile >= 64 and tile & (tile - 1) == 0
    small, big = lib.lad_label_histogram_workspace_bytes(1, 1000, 0), lib.lad_label_histogram_workspace_bytes(20, 360000, 100000)
    assert 0 < small < big and big >= 4 * 100000 + 12 * 20
    assert lib.lad_label_histogram_workspace_bytes(65535, 1 << 30, 1 << 30) > 0
    for bad in ((0, 10, 1), (65536, 10, 1), (1, 0, 1), (1, (1 << 30) + 1, 1), (1, 10, -1), (1, 10, (1 << 30) + 1)):
        assert lib.lad_label_histogram_workspace_bytes(*bad) == -1
        assert b"lad_label_histogram_workspace_bytes" in lib.lad_last_error()


def test_c_abi_refuses_before_any_launch():
    """Every call below returns LAD_ERR_INVALID from the host checks: the device pointers are never followed."""
    import _hip
    lib = _hip.lib()
    null, dev = ctypes.c_void_p(0), ctypes.c_void_p(1 << 20)
    i32, i64, f64 = (lambda *v: (ctypes.c_int32 * len(v))(*v)), (lambda *v: (ctypes.c_int64 * len(v))(*v)), (lambda *v: (ctypes.c_double * len(v))(*v))
    offsets, bounds = i32(0, 0, 1, 2, 2, 2, 2, 3, 3, 3, 3), i32(10, 20, 30, 40, 5, 9)     # two channels, three intervals
    ok = dict(probs=dev, dtype=0, channels=2, frames=100, lengths=i64(100, 50), bounds=dev, offsets=dev, bounds_host=bounds,
              offsets_host=offsets, n=3, fps=dev, fps_host=f64(100.0, 50.0), group=i32(0, -1), n_groups=1,
              ws=ctypes.c_void_p(1 << 30), hist=ctypes.c_void_p(1 << 40), stream=null)

    def call(**change):
        a = dict(ok, **change)
        return lib.lad_label_histogram(*a.values())
    bad = [dict(channels=0), dict(channels=65536), dict(frames=0), dict(frames=(1 << 30) + 1), dict(n=-1), dict(dtype=2),
           dict(probs=null), dict(hist=null), dict(ws=null), dict(offsets=null), dict(fps=null), dict(bounds=null),
           dict(lengths=i64(100, 0)), dict(lengths=i64(101, 50)), dict(group=i32(0, 1)), dict(group=i32(-2, 0)), dict(n_groups=0),
           dict(n_groups=3), dict(group=None, n_groups=1), dict(fps_host=f64(100.0, 0.0)), dict(fps_host=f64(float("nan"), 1.0)),
           dict(fps_host=f64(100.0, 1e-8)), dict(offsets_host=i32(0, 0, 1, 2, 2, 2, 2, 3, 3, 3, 2)),
           dict(offsets_host=i32(1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3)), dict(bounds_host=i32(10, 10, 30, 40, 5, 9)),
           dict(bounds_host=i32(10, 20, 15, 40, 5, 9), offsets_host=i32(0, 0, 2, 2, 2, 2, 2, 3, 3, 3, 3)),
           dict(hist=dev), dict(ws=dev)]
    for change in bad:
        assert call(**change) == _hip.LAD_ERR_INVALID, change
        assert b"lad_label_histogram" in lib.lad_last_error(), change
    assert b"millisecond overflow" not in lib.lad_last_error()
    assert call(fps_host=f64(100.0, 1e-8)) == _hip.LAD_ERR_INVALID and b"millisecond overflow" in lib.lad_last_error()
    # the overflow check is on m_n of the channel's own length: 50 frames at this rate fit, 100 would not
    assert call(fps_host=f64(100.0, 2.4e-5), lengths=i64(100, 100)) == _hip.LAD_ERR_INVALID
    assert b"millisecond overflow" in lib.lad_last_error()
    assert call(fps_host=f64(100.0, 2.4e-5), group=i32(0, 1)) == _hip.LAD_ERR_INVALID and b"group" in lib.lad_last_error()

    def remap(probs=dev, dtype=1, channels=1, frames=10, table=ctypes.c_void_p(1 << 30), out=ctypes.c_void_p(1 << 40)):
        return lib.lad_track_remap(probs, dtype, channels, frames, table, out, null)
    for change in (dict(channels=0), dict(frames=0), dict(frames=(1 << 30) + 1), dict(dtype=-1), dict(probs=null), dict(table=null),
                   dict(out=null), dict(out=dev), dict(out=ctypes.c_void_p((1 << 30) + 8))):
        assert remap(**change) == _hip.LAD_ERR_INVALID, change
        assert b"lad_track_remap" in lib.lad_last_error(), change
