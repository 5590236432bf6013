"""Sampling-rate conversion, the part that needs no GPU: the filter designer and the polyphase table of resample.py against scipy,
the float64 model of tests/_resample_model.py against scipy.signal.resample_poly, the host-only entries of the C ABI, and the
existing refusal of audio that is not at 16 kHz."""
import os
import wave

import numpy as np
import pytest
from scipy import signal

import _resample_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import importlib.util
        spec = importlib.util.spec_from_file_location("lad_build", os.path.join(ROOT, "laughter-detection-icsi_amd", "build.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.build(verbose=False)
    return _hip.lib()


def write_wav(path, sr, pcm16):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(sr)
        f.writeframes(np.asarray(pcm16, dtype=np.int16).tobytes())


@pytest.mark.parametrize("sr_in,sr_out", rm.PAIRS)
def test_design_matches_scipy_firwin(sr_in, sr_out):
    import resample
    up, down = resample.ratio(sr_in, sr_out)
    assert (up, down) == rm.ratio(sr_in, sr_out)
    h, half = resample.design_lowpass(up, down)
    ref, ref_half = rm.scipy_filter(up, down)
    assert half == ref_half == 10 * max(up, down) and h.dtype == np.float64 and h.shape == ref.shape
    err = np.abs(h - ref).max()
    print(f"{sr_in}->{sr_out}: design vs firwin {err:.2e}")
    assert err <= 1e-14
    assert abs(h.sum() - up) <= 1e-12 * up


def test_design_keywords_give_a_steeper_filter():
    import resample
    h, half = resample.design_lowpass(1, 3, zeros=20, beta=8.0)
    ref = signal.firwin(2 * 60 + 1, 1.0 / 3, window=("kaiser", 8.0))
    assert half == 60 and np.abs(h - ref).max() <= 1e-14


@pytest.mark.parametrize("sr_in,sr_out", rm.PAIRS)
def test_model_matches_scipy_resample_poly(sr_in, sr_out):
    up, down = rm.ratio(sr_in, sr_out)
    h, half = rm.scipy_filter(up, down)
    x = rm.noise(sr_in, dtype=np.float64)
    want = signal.resample_poly(x, up, down)
    y, mag = rm.model(x, up, down, h, half)
    assert y.shape == want.shape == (rm.out_len(x.shape[0], up, down),)
    err = np.abs(y - want).max()
    print(f"{sr_in}->{sr_out}: model vs resample_poly {err:.2e}")
    assert err <= 1e-13
    assert np.all(mag >= np.abs(y) - 1e-12)
    # the same taps passed as a window reproduce it too
    assert np.abs(signal.resample_poly(x, up, down, window=h / up) - want).max() <= 1e-13
    # a subset of outputs is the slice of all of them
    some = np.array([0, 1, y.shape[0] // 2, y.shape[0] - 1])
    assert np.array_equal(rm.model(x, up, down, h, half, outputs=some)[0], y[some])


@pytest.mark.parametrize("sr_in,sr_out", rm.PAIRS)
def test_table_holds_every_tap_once_where_the_header_says(sr_in, sr_out):
    import resample
    up, down = rm.ratio(sr_in, sr_out)
    h, half = resample.design_lowpass(up, down)
    table, K = resample.polyphase_table(h, half, up, down)
    assert table.dtype == np.float32 and table.shape == (up, K) and table.flags["C_CONTIGUOUS"]
    L = (K - 1) // 2
    assert K == rm.taps_per_output(half, up) and L == half // up
    # include/lad_hip.h: h[i] sits at p = (i - half) mod up, t = L - (i - half - p) / up; everything else is 0
    want = np.zeros((up, K), dtype=np.float32)
    seen = np.zeros((up, K), dtype=np.int64)
    for i in range(2 * half + 1):
        m = i - half
        p = m % up
        t = L - (m - p) // up
        assert 0 <= t < K
        want[p, t] = np.float32(h[i])
        seen[p, t] += 1
    assert seen.max() == 1 and seen.sum() == 2 * half + 1
    assert np.array_equal(table, want)
    # with taps that are all distinct and non-zero the table is a placement of exactly those values
    ramp = np.arange(1, 2 * half + 2, dtype=np.float64)
    t2, _ = resample.polyphase_table(ramp, half, up, down)
    assert np.array_equal(np.sort(t2[t2 != 0]), ramp.astype(np.float32)) and np.array_equal(t2 != 0, seen == 1)
    # the zero padding is at the two ends of a row
    for p in range(up):
        nz = np.nonzero(seen[p])[0]
        assert np.array_equal(nz, np.arange(nz[0], nz[-1] + 1)) and nz[0] <= 1 and nz[-1] >= K - 2


def test_table_rows_restate_the_formula():
    """sum_t table[p][t] * x[c - L + t] with n * down = c * up + p is the model's y[n] (float64 table here: exact restatement)."""
    import resample
    up, down = 160, 441
    h, half = resample.design_lowpass(up, down)
    _, K = resample.polyphase_table(h, half, up, down)
    L = (K - 1) // 2
    idx = half + np.arange(up)[:, None] - (np.arange(K)[None, :] - L) * up
    t64 = np.where((idx >= 0) & (idx <= 2 * half), h[np.clip(idx, 0, 2 * half)], 0.0)
    x = rm.noise(44100, dtype=np.float64)[:3000]
    y, _ = rm.model(x, up, down, h, half)
    xp = np.concatenate([np.zeros(K), x, np.zeros(2 * K)])
    for n in (0, 1, 2, 17, 500, y.shape[0] - 2, y.shape[0] - 1):
        c, p = divmod(n * down, up)
        got = float(np.dot(t64[p], xp[K + c - L: K + c - L + K]))
        assert abs(got - y[n]) <= 1e-13, n


def test_ratio():
    import resample
    assert resample.ratio(44100, 16000) == (160, 441)
    assert resample.ratio(16000, 16000) == (1, 1)
    assert resample.ratio(48000, 16000) == (1, 3)
    assert resample.ratio(16000, 44100) == (441, 160)
    assert resample.ratio(11025, 16000) == (640, 441)
    with pytest.raises(ValueError):
        resample.ratio(0, 16000)


def test_out_len_needs_no_gpu(lib):
    import resample
    for up, down in ((160, 441), (441, 160), (1, 3), (2, 1), (640, 441)):
        for n in (0, 1, 440, 441, 442, 2 ** 40):
            assert lib.lad_resample_out_len(n, up, down) == -(-n * up // down), (n, up, down)
            assert resample.out_len(n, up, down) == -(-n * up // down)
    assert lib.lad_resample_out_len(-1, 1, 3) == -1 and b"lad_resample_out_len" in lib.lad_last_error()
    assert lib.lad_resample_out_len(5, 0, 3) == -1
    assert lib.lad_resample_out_len(2 ** 62, 4, 1) == -1


def test_limits_cover_every_listed_pair_and_need_no_gpu(lib):
    import resample
    lim = resample.limits()
    assert lim["tile_outputs"] > 0 and lim["max_lds_bytes"] <= 160 * 1024
    for sr_in, sr_out in rm.PAIRS:
        up, down = rm.ratio(sr_in, sr_out)
        K = rm.taps_per_output(10 * max(up, down), up)
        assert up <= lim["max_up"] and down <= lim["max_down"] and K <= lim["max_taps"]
        need = lib.lad_resample_lds_bytes(up, down, K)
        assert 0 < need <= lim["max_lds_bytes"], (sr_in, sr_out, need)
    assert lib.lad_resample_lds_bytes(lim["max_up"] + 1, 1, 21) == -1
    # a null launch is refused on the host, and an empty range returns before anything is touched
    assert lib.lad_resample(None, 0, 100, None, 1, 3, 61, 0, 0, None, None) == 0
    assert lib.lad_resample(None, 0, 100, None, 1, 3, 61, 0, 34, None, None) == -1 and b"null" in lib.lad_last_error()
    assert lib.lad_resample(None, 0, 100, None, 1, 3, 61, 30, 5, None, None) == -1      # 34 outputs in all
    assert lib.lad_resample(None, 0, 100, None, 0, 3, 61, 0, 0, None, None) == -1
    assert lib.lad_resample(None, 7, 100, None, 1, 3, 61, 0, 0, None, None) == -1
    assert lib.lad_resample(None, 0, 100, None, 1000, 999, 1000, 0, 0, None, None) == -1 and b"limits" in lib.lad_last_error()


def test_a_ratio_beyond_the_limits_is_a_value_error(lib):
    import resample
    with pytest.raises(ValueError, match="limits"):
        resample.Resampler(16000, 16001, device="cpu")
    with pytest.raises(ValueError, match="limits"):
        resample.Resampler(44100, 48000, device="cpu", zeros=60)     # 147/160: 160 x 111 taps do not fit the LDS budget


def test_load_audio_still_refuses_another_rate(tmp_path):
    import load_data
    wav = tmp_path / "a48.wav"
    write_wav(wav, 48000, np.zeros(4800, dtype=np.int16))
    with pytest.raises(ValueError, match="expected 16000 Hz audio, got 48000"):
        load_data.load_audio(str(wav))
    # the device loader without resample=True says the same, before anything is uploaded
    with pytest.raises(ValueError, match="expected 16000 Hz audio, got 48000"):
        load_data.load_audio_device(str(wav), device="cpu")
    # and the file's own rate still loads
    assert load_data.load_audio(str(wav), sampling_rate=48000).shape == (4800,)
