"""csrc/resample.hip against the float64 model of tests/_resample_model.py (scipy.signal.resample_poly's convention).

Error bar, derived and not chosen: a float32 sum of K fused multiply-adds of float32-rounded taps and float32 samples satisfies
|y_gpu[n] - y_f64[n]| <= (K + 3) * 2^-24 * sum_j |x[j] * h[...]| (tap rounding 2^-24, K roundings of the running sum, first
order); the model computes the bound per output and it is asserted for every output.  A wrong phase, tap or index is off by 1e-2
or more on this input."""
import contextlib
import io
import wave

import numpy as np
import pytest
import torch

import _resample_model as rm

pytestmark = pytest.mark.gpu

_REF = {}


def reference(sr_in, sr_out):
    """(x float32, y float64, bound float64, K) for the seeded noise of the pair: computed once, never modified."""
    key = (sr_in, sr_out)
    if key not in _REF:
        up, down = rm.ratio(sr_in, sr_out)
        h, half = rm.scipy_filter(up, down)
        x = rm.noise(sr_in)
        y, mag = rm.model(x, up, down, h, half)
        K = rm.taps_per_output(half, up)
        for a in (x, y, mag):
            a.setflags(write=False)
        _REF[key] = (x, y, rm.bound(mag, K), K)
    return _REF[key]


def check(got, y, bound, what):
    got = got.double().cpu().numpy()
    assert got.shape == y.shape, (what, got.shape, y.shape)
    if got.size == 0:
        return 0.0
    err = np.abs(got - y)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{what}: max |err| {err.max():.3e}, worst err / bound {worst:.3f}")
    assert np.all(err <= bound), (what, float(err.max()), worst)
    return float(err.max())


def write_wav(path, sr, pcm16):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(sr)
        f.writeframes(np.asarray(pcm16, dtype=np.int16).tobytes())


@pytest.mark.parametrize("sr_in,sr_out", rm.PAIRS)
def test_every_pair_against_the_float64_model(sr_in, sr_out):
    import resample
    from scipy import signal
    x, y, bound, K = reference(sr_in, sr_out)
    r = resample.Resampler(sr_in, sr_out, "cuda")
    assert r.K == K and (r.up, r.down) == rm.ratio(sr_in, sr_out)
    got = r(torch.tensor(x, device="cuda"))
    assert got.dtype == torch.float32 and got.is_cuda
    assert got.shape[0] == signal.resample_poly(x.astype(np.float64), r.up, r.down).shape[0]
    check(got, y, bound, f"{sr_in}->{sr_out} (K = {K})")
    assert torch.equal(resample.resample(torch.tensor(x, device="cuda"), sr_in, sr_out), got)


@pytest.mark.parametrize("sr_in,sr_out", [(44100, 16000), (16000, 44100)])
def test_short_and_empty_inputs(sr_in, sr_out):
    import resample
    up, down = rm.ratio(sr_in, sr_out)
    h, half = rm.scipy_filter(up, down)
    K = rm.taps_per_output(half, up)
    r = resample.Resampler(sr_in, sr_out, "cuda")
    full = rm.noise(sr_in, seed=3)
    for n_in in (0, 1, 5, K - 1, K, K + 1):
        x = full[:n_in].copy()
        y, mag = rm.model(x, up, down, h, half)
        got = r(torch.tensor(x, device="cuda"))
        assert got.shape[0] == rm.out_len(n_in, up, down)
        check(got, y, rm.bound(mag, K), f"{sr_in}->{sr_out} n_in = {n_in}")


@pytest.mark.parametrize("sr_in,sr_out", [(44100, 16000), (48000, 16000), (16000, 44100), (8000, 16000)])
def test_int16_equals_the_scaled_float_input(sr_in, sr_out):
    import resample
    pcm = (np.clip(rm.noise(sr_in, seed=5) * 0.3, -1, 1) * 32767).astype(np.int16)
    pcm[:3] = (-32768, 32767, 0)
    x16 = torch.from_numpy(pcm).cuda()
    r = resample.Resampler(sr_in, sr_out, "cuda")
    a = r(x16)
    b = r(x16.float() / 32768)
    assert torch.equal(a, b) and float(a.abs().max()) > 0.1
    # a view that does not start on a 16-byte boundary takes the element-wise staging path: same bits
    assert torch.equal(r(x16[1:]), r(x16[1:].clone()))
    xf = x16.float() / 32768
    assert torch.equal(r(xf[3:]), r(xf[3:].clone()))


@pytest.mark.parametrize("sr_in,sr_out", [(44100, 16000), (48000, 16000), (16000, 44100)])
def test_chunks_equal_the_slice_of_the_whole_call(sr_in, sr_out):
    import resample
    x, y, bound, K = reference(sr_in, sr_out)
    tile = resample.limits()["tile_outputs"]
    r = resample.Resampler(sr_in, sr_out, "cuda")
    xd = torch.tensor(x, device="cuda")
    whole = r(xd)
    total = whole.shape[0]
    assert total > 2 * tile + 300
    for a in (0, 1, tile - 1, tile, tile + 1):
        for b in (a + tile + 300, total, a + 1, a):
            got = r(xd, start=a, stop=b)
            assert got.shape[0] == b - a and torch.equal(got, whole[a:b]), (a, b)
    assert torch.equal(r(xd, stop=tile + 7), whole[:tile + 7]) and torch.equal(r(xd, start=total - 5), whole[total - 5:])
    with pytest.raises(ValueError):
        r(xd, start=0, stop=total + 1)


def test_indices_beyond_32_bits():
    """14,000,000 int16 samples at 44.1 kHz: n * down passes 2^31 at output 4,869,578."""
    import resample
    sr_in, sr_out, n_in = 44100, 16000, 14_000_000
    up, down = rm.ratio(sr_in, sr_out)
    h, half = rm.scipy_filter(up, down)
    K = rm.taps_per_output(half, up)
    pcm = np.random.default_rng(77).integers(-20000, 20000, n_in, dtype=np.int16)
    xd = torch.from_numpy(pcm).cuda()
    r = resample.Resampler(sr_in, sr_out, "cuda")
    whole = r(xd)
    total = rm.out_len(n_in, up, down)
    assert whole.shape[0] == total == 5_079_366
    x64 = pcm.astype(np.float64) / 32768
    for a, b in ((4_900_000, 4_904_096), (total - 4096, total)):
        assert a * down > 2 ** 31
        outs = np.arange(a, b, dtype=np.int64)
        y, mag = rm.model(x64, up, down, h, half, outputs=outs)
        check(whole[a:b], y, rm.bound(mag, K), f"outputs {a}..{b} of {total}")
        assert torch.equal(r(xd, start=a, stop=b), whole[a:b])


def test_identity_makes_no_kernel_call(monkeypatch):
    import _hip
    import resample
    r = resample.Resampler(16000, 16000, "cuda")
    assert r.identity and r.table is None

    def boom(*a, **k):
        raise AssertionError("the identity ratio must not reach the library")
    monkeypatch.setattr(_hip, "lib", boom)
    x = torch.from_numpy(rm.noise(16000)).cuda()
    out = r(x)
    assert out.data_ptr() == x.data_ptr() and torch.equal(out, x)
    x16 = torch.tensor([-32768, 0, 16384, 32767], dtype=torch.int16, device="cuda")
    assert torch.equal(r(x16), x16.float() / 32768)
    assert torch.equal(r(x, start=3, stop=10), x[3:10])


def test_a_ratio_beyond_the_limits_raises():
    import resample
    lim = resample.limits()
    with pytest.raises(ValueError, match=f"up <= {lim['max_up']}"):
        resample.Resampler(16000, 16001, "cuda")
    with pytest.raises(ValueError, match="limits"):
        resample.resample(torch.zeros(100, device="cuda"), 16001, 16000)
    with pytest.raises(ValueError, match="bytes of LDS"):
        resample.Resampler(44100, 48000, "cuda", zeros=60)


def test_inference_dataloader_resamples_when_asked(tmp_path):
    import config
    import load_data
    import resample
    from utils import get_feat_extractor
    sr, secs = 48000, 2
    pcm = (np.clip(np.random.default_rng(9).standard_normal(sr * secs) * 0.1, -1, 1) * 32767).astype(np.int16)
    wav = tmp_path / "a48.wav"
    write_wav(wav, sr, pcm)
    loader = load_data.create_inference_dataloader(str(wav), resample=True)
    feats = loader.dataset.feats
    ex = get_feat_extractor(num_samples=config.FEAT["num_samples"], num_filters=config.FEAT["num_filters"])
    want = ex.extract_long(resample.Resampler(48000, 16000, "cuda")(torch.from_numpy(pcm).cuda()))
    assert torch.equal(feats, want)
    assert abs(feats.shape[0] - 200) <= 1 and feats.shape[1] == 44
    with pytest.raises(ValueError, match="expected 16000 Hz audio, got 48000"):
        load_data.create_inference_dataloader(str(wav))
    # the device loader alone: int16 reaches the kernel as int16
    y = load_data.load_audio_device(str(wav), resample=True)
    assert torch.equal(y, resample.resample(torch.from_numpy(pcm).cuda(), 48000, 16000))
    # a 16 kHz file through the device loader is load_audio's samples
    wav16 = tmp_path / "a16.wav"
    write_wav(wav16, 16000, pcm[:16000])
    assert torch.equal(load_data.load_audio_device(str(wav16)).cpu(), torch.from_numpy(load_data.load_audio(str(wav16))))
    # .npy carries no rate: source_rate says it
    np.save(tmp_path / "a48.npy", pcm.astype(np.float32) / 32768)
    z = load_data.load_audio_device(str(tmp_path / "a48.npy"), resample=True, source_rate=48000)
    assert torch.equal(z, y)


def test_segment_laughter_script_with_resample_and_44100_cuts(tmp_path):
    from oracle import recipe
    import audio_utils
    import models
    import segment_laughter
    import torch_utils
    with contextlib.redirect_stdout(io.StringIO()):
        m = models.ResNetBigger(dropout_rate=0.0, linear_layer_size=48, filter_sizes=[64, 32, 16, 16])
    sd = recipe.make_state(171)
    full = m.state_dict()
    for k, v in sd.items():
        full[k] = torch.from_numpy(v.copy())
    m.load_state_dict(full)
    m.set_device("cuda")
    state = torch_utils.make_state_dict(m, None, 0, 0, float("inf"))
    torch_utils.save_checkpoint(state, is_best=True, checkpoint=str(tmp_path / "ckpt"))
    sr, secs = 44100, 3
    clip = recipe.make_clips(9, 1, n_samples=sr * secs, sr=sr).reshape(-1)
    wav = tmp_path / "track.wav"
    write_wav(wav, sr, (clip * 32767).clip(-32768, 32767).astype(np.int16))
    out = tmp_path / "out"
    with contextlib.redirect_stdout(io.StringIO()):
        segment_laughter.main(["--config", "resnet_base", "--model_path", str(tmp_path / "ckpt"), "--input_audio_file", str(wav),
                               "--output_dir", str(out), "--resample", "True", "--save_to_audio_files", "True",
                               "--save_audio_rate", "44100", "--thresholds", "0.0", "--min_lengths", "0.0"])
    d = out / "t_0.0" / "l_0.0"
    tg = (d / "track.TextGrid").read_text()
    assert (d / "laugh_0.wav").exists()
    with wave.open(str(d / "laugh_0.wav"), "rb") as f:
        assert f.getframerate() == 44100 and f.getnframes() > 0
    xmax = [float(l.split("=")[1]) for l in tg.splitlines() if l.strip().startswith("xmax")]
    assert xmax and abs(xmax[0] - audio_utils.get_audio_length(str(wav))) < 1e-9 and abs(xmax[0] - secs) < 1e-9
    # without --resample the script refuses the file as before
    with pytest.raises(ValueError, match="expected 16000 Hz audio, got 44100"):
        with contextlib.redirect_stdout(io.StringIO()):
            segment_laughter.main(["--config", "resnet_base", "--model_path", str(tmp_path / "ckpt"), "--input_audio_file", str(wav),
                                   "--output_dir", str(tmp_path / "out2"), "--thresholds", "0.0", "--min_lengths", "0.0"])
