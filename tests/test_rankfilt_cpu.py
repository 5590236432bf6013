"""What the median / rank filter (csrc/rankfilt.hip, rankfilt.py, laugh_segmenter.rank_filter / median_filter) promises without a
GPU: the host forms against the model (tests/_rankfilt_model.py) and against scipy.ndimage, value for value; the size queries and
the refusals; the flags; and that there is no CPU fallback behind the device forms.

scipy.ndimage's 1-D rank filter with mode='nearest' is the convention whenever T >= (window - 1) / 2; below that its 1-D path
returns zeros, so scipy is asserted only from there on and the model alone below it.  All comparisons are np.array_equal."""
import os

import numpy as np
import pytest
import torch

import _rankfilt_model as rm

LENGTHS = [1, 2, 3, 25, 64, 300, 1100]
WINDOWS = [1, 3, 5, 51, 101, 1023]


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


def _check(x, window, rank):
    from scipy import ndimage

    import laugh_segmenter as ls
    got = ls.rank_filter(x, window, rank)
    assert got.dtype == x.dtype and got.shape == x.shape
    assert np.array_equal(got, rm.rank_filter(x, window, rank)), (x.size, window, rank)
    if x.size >= (window - 1) // 2:
        assert np.array_equal(got, ndimage.rank_filter(x, rank, size=window, mode="nearest")), (x.size, window, rank)
    assert np.isin(got, x).all()                          # a selected input value, never an arithmetic result


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_host_forms_against_the_model_and_scipy(dtype, window):
    from scipy import ndimage

    import laugh_segmenter as ls
    for T in LENGTHS:
        x = rm.track("tied", T, dtype, seed=window)
        assert T < 300 or 0.2 <np.mean(x == dtype(0.375)) < 0.4
        for rank in rm.ranks(window):
            _check(x, window, rank)
        med = ls.median_filter(x, window)
        assert np.array_equal(med, rm.median_filter(x, window))
        if T >= (window - 1) // 2:
            assert np.array_equal(med, ndimage.median_filter(x, size=window, mode="nearest"))


@pytest.mark.parametrize("kind", ["constant", "ramp", "random", "fp16"])
def test_host_forms_on_constant_ramp_and_other_tracks(kind):
    for dtype in (np.float32, np.float64):
        for T, window in ((1, 1023), (3, 5), (25, 51), (300, 101), (1100, 1023), (64, 3)):
            x = rm.track(kind, T, dtype)
            for rank in rm.ranks(window):
                _check(x, window, rank)
    import laugh_segmenter as ls
    c = rm.track("constant", 300, np.float32)
    assert np.array_equal(ls.median_filter(c, 101), c)
    r = rm.track("ramp", 300, np.float64)
    assert np.array_equal(ls.median_filter(r, 101)[50:-50], r[50:-50])          # a line is its own median away from the ends


def test_host_forms_keep_values_and_take_other_inputs():
    import laugh_segmenter as ls
    x = [0.1, 0.9, 0.1, 0.1, 0.9, 0.9, 0.9, 0.1, 0.9]
    got = ls.median_filter(x, 3)                          # a list: float64
    assert got.dtype == np.float64 and got.tolist() == [0.1, 0.1, 0.1, 0.1, 0.9, 0.9, 0.9, 0.9, 0.9]
    half = np.asarray(x, np.float16)
    assert ls.median_filter(half, 3).dtype == np.float64 and np.array_equal(ls.median_filter(half, 3), rm.median_filter(half.astype(np.float64), 3))
    assert np.array_equal(ls.rank_filter(x, 3, 0), rm.rank_filter(np.asarray(x), 3, 0))
    assert np.array_equal(ls.rank_filter(x, 1, 0), np.asarray(x))


BAD_WINDOWS = [0, 2, 4, 50, 1024, 1025, -1, -3]


def test_size_queries_need_no_gpu_and_refuse():
    import _hip
    lib = _hip.lib()
    assert lib.lad_rank_filter_max_window() == 1023
    assert lib.lad_rank_filter_tile_frames() >= 64
    for ok in ((1, 1, 1), (1, 360000, 51), (10, 360000, 1023), (1, 1 << 30, 3), (65535, 100, 101), (1, 2, 1023)):
        assert lib.lad_rank_filter_workspace_bytes(*ok) >= 0, ok
    bad = [(1, 100, w) for w in BAD_WINDOWS] + [(0, 100, 3), (65536, 100, 3), (-1, 100, 3), (1, 0, 3), (1, -5, 3), (1, (1 << 30) + 1, 3)]
    for case in bad:
        assert lib.lad_rank_filter_workspace_bytes(*case) == -1, case
        assert b"lad_rank_filter_workspace_bytes" in lib.lad_last_error()


def test_host_forms_refuse_what_the_library_refuses():
    import laugh_segmenter as ls
    x = rm.track("random", 40, np.float64)
    for w in BAD_WINDOWS + [3.5, "3", True]:
        with pytest.raises(ValueError):
            ls.median_filter(x, w)
        with pytest.raises(ValueError):
            ls.rank_filter(x, w, 0)
    for rank in (-1, 5, 6, 2.5):
        with pytest.raises(ValueError):
            ls.rank_filter(x, 5, rank)
    for shape in ((0,), (2, 20), ()):
        with pytest.raises(ValueError):
            ls.median_filter(np.zeros(shape), 3)


def test_device_forms_have_no_cpu_fallback():
    import _hip
    import laugh_segmenter as ls
    import rankfilt
    p = torch.rand(1000)
    for bad in (p, p.numpy(), (p * 10).to(torch.int32), p.view(2, 5, 100), p.view(10, 100)):
        with pytest.raises(_hip.LadHipError):
            ls.median_filter_device(bad, 5)
        with pytest.raises(_hip.LadHipError):
            ls.rank_filter_device(bad, 5, 0)
        with pytest.raises(_hip.LadHipError):
            rankfilt.median_filter_device(bad, 5)
        with pytest.raises(_hip.LadHipError):
            rankfilt.rank_filter_device(bad, 5, 4)
    assert ls.median_filter_device is not rankfilt.median_filter_device and ls.median_filter_device.__module__ == "laugh_segmenter"


def _parsers():
    import evaluate_sweep
    import segment_laughter
    return ((segment_laughter, ["--input_audio_file", "a.wav"]),
            (evaluate_sweep, ["--probs_dir", "p", "--transcripts", "t.csv", "--channels", "c.csv", "--out_dir", "o"]))


def test_median_flag():
    for module, base in _parsers():
        parser = module.build_parser()
        assert parser.parse_args(base).median is None
        for good in (1, 3, 51, 1023):
            got = parser.parse_args(base + ["--median", str(good)]).median
            assert isinstance(got, int) and got == good
        for bad in ("0", "2", "50", "1024", "1025", "-1", "-3", "5.0", "x", ""):
            with pytest.raises(SystemExit):
                parser.parse_args(base + ["--median", bad])


def test_median_with_lowpass_is_refused_by_both_programs(tmp_path):
    import _score_model as sm
    import evaluate_sweep
    import segment_laughter
    for module, base in _parsers():
        with pytest.raises(SystemExit, match="--median cannot be combined with --lowpass"):
            module.main(base + ["--median", "51", "--lowpass", "0.01"])
    args = sm.write_corpus(tmp_path)
    with pytest.raises(SystemExit, match="--lowpass"):
        evaluate_sweep.main(args + ["--median", "5", "--lowpass", "0.01", "--out_dir", str(tmp_path / "out")])
    assert not os.path.exists(tmp_path / "out")
    with pytest.raises(ValueError, match="lowpass and median"):
        segment_laughter.load_and_pred(None, "a.wav", [0.5], [0.2], None, lowpass=0.01, median=5)

def test_evaluate_sweep_with_median_under_the_host_scorer(tmp_path, capsys):
    """--median filters before the host scorer: the files are those of tracks filtered beforehand, and others than without."""
    import _score_model as sm
    import evaluate_sweep
    args = sm.write_corpus(tmp_path)

    def files(d):
        return {f: open(d / f, "rb").read() for f in sorted(os.listdir(d))}
    evaluate_sweep.main(args + ["--median", "51", "--out_dir", str(tmp_path / "flag")])
    evaluate_sweep.main(args + ["--out_dir", str(tmp_path / "plain")])
    for m in os.listdir(tmp_path / "probs"):
        for f in os.listdir(tmp_path / "probs" / m):
            np.save(tmp_path / "probs" / m / f, rm.median_filter(np.load(tmp_path / "probs" / m / f), 51))
    evaluate_sweep.main(args + ["--out_dir", str(tmp_path / "before")])
    assert list(files(tmp_path / "flag")) == ["eval_df_per_meeting.csv", "sum_stats.csv"]
    assert files(tmp_path / "flag") == files(tmp_path / "before")
    assert files(tmp_path / "flag") != files(tmp_path / "plain")
