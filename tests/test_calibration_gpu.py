"""The calibration kernels on the GPU (csrc/calibration.hip): the device histogram == the host histogram == the model written from
the header (tests/_calibration_model.py), with the frame counts placed around lad_label_histogram_tile_frames(); the tracks that
take the aggregation path to its ends (one slot, every frame another slot, two values); identical bytes on every call, into a
histogram full of garbage; the table applied on the device == on the host, bit for bit; both routes of evaluate_sweep.py write the
same files; and the refusals, which leave the output untouched."""
import os

import numpy as np
import pytest
import torch

import _calibration_cases as cases
import _calibration_model as cm
import _score_model as sm

pytestmark = pytest.mark.gpu
FPS = cases.NON_INTEGER_FPS


def _tile():
    import _hip
    return _hip.lib().lad_label_histogram_tile_frames()


def _padded(tracks, dtype):
    out = np.full((len(tracks), max(len(t) for t in tracks)), np.nan, dtype)
    for c, t in enumerate(tracks):
        out[c, :len(t)] = t
    return torch.from_numpy(out).cuda()


def _check(kinds, sizes, chans, fps, dtype="float64", lengths=None, groups=None):
    """device == host == model for one case; the tensor is as long as the longest track, `lengths` (or the tracks' own) say the rest."""
    import calibration
    tracks, channels, want = cases.case(tuple(kinds), tuple(sizes), tuple(chans), tuple(fps), dtype, lengths, groups)
    true = [len(t) for t in tracks] if lengths is None else list(lengths)
    host = calibration.label_histogram_host(tracks, channels, list(fps), cases.index(), lengths=true, groups=groups)
    assert np.array_equal(host, want)
    probs = _padded(tracks, np.dtype(dtype))
    if len(tracks) == 1 and lengths is None:
        probs, true = probs[0], None                            # a (T,) tensor, no lengths
    got = calibration.label_histogram_device(probs, channels, list(fps), cases.index(), lengths=true, groups=groups)
    assert got.dtype == np.int64 and got.shape == want.shape
    assert np.array_equal(got, want)
    return got


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("which", ["one", "tile-1", "tile", "tile+1", "3tile+5"])
def test_one_channel_around_the_tile(which, dtype):
    tile = _tile()
    n = {"one": 1, "tile-1": tile - 1, "tile": tile, "tile+1": tile + 1, "3tile+5": 3 * tile + 5}[which]
    got = _check(["seeded"], [n], [1], [100.0 if n > 1 else 0.05], dtype)
    assert got.sum() > 0


@pytest.mark.parametrize("kind", ["constant", "distinct", "alternating"])
def test_the_ends_of_the_aggregation_path(kind):
    """One slot (a workgroup adds five sums), every frame another slot (nothing to aggregate), two alternating values."""
    got = _check([kind], [3 * _tile() + 5], [1], [100.0], "float32")
    occupied = int((got[0].sum(axis=0) > 0).sum())
    assert occupied == {"constant": 1, "alternating": 2}.get(kind, occupied) and (kind != "distinct" or occupied > 2900)


@pytest.mark.parametrize("fps", [100.0, FPS])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_the_hand_written_index_and_the_special_values(fps, dtype):
    _check(["seeded"], [1300 if fps == 100.0 else 600], [0], [fps], dtype)


@pytest.mark.parametrize("groups", [None, (0, 0, 0), (1, -1, 0)])
def test_three_channels_with_their_own_lengths_and_rates(groups):
    tile = _tile()
    _check(["seeded", "seeded", "alternating"], [3 * tile + 5, 2 * tile, tile + 700], [0, 1, 3], [100.0, FPS, 7.3], "float64",
           lengths=(3 * tile + 5, tile + 1, 1500), groups=groups)


def test_channels_without_a_participant_and_padding_without_lengths():
    import calibration
    _check(["seeded", "seeded"], [500, 1200], [2, 3], [100.0, 100.0], "float32")
    alone = _check(["seeded"], [700], [2], [100.0])              # an index without any interval: the memset is all there is
    assert not alone.any()
    # without lengths the NaN padding of a ragged tensor is counted, in the NaN slot
    tracks = [cases.track("seeded", 900, np.float32, seed=3), cases.track("seeded", 400, np.float32, seed=4)]
    probs = _padded(tracks, np.float32)
    channels = [cases.CHANNELS[1], cases.CHANNELS[3]]
    got = calibration.label_histogram_device(probs, channels, 100.0, cases.index())
    assert np.array_equal(got, calibration.label_histogram_host(list(probs.cpu().numpy()), channels, 100.0, cases.index()))
    assert got[1, :, cm.NAN_SLOT].sum() > 0
    # a trailing group that no channel belongs to stays when it is named, on both forms; a group count beyond the channels is refused
    named = calibration.label_histogram_device(probs, channels, 100.0, cases.index(), groups=[0, -1], n_groups=2)
    assert named.shape[0] == 2 and not named[1].any() and np.array_equal(named[0], got[0])
    assert np.array_equal(named, calibration.label_histogram_host(list(probs.cpu().numpy()), channels, 100.0, cases.index(),
                                                                  groups=[0, -1], n_groups=2))
    import _hip
    with pytest.raises(_hip.LadHipError):
        calibration.label_histogram_device(probs, channels, 100.0, cases.index(), groups=[0, 5])
    with pytest.raises(ValueError):
        calibration.label_histogram_host(list(probs.cpu().numpy()), channels, 100.0, cases.index(), groups=[0, 5])


def _raw(probs, lengths, fps, groups, n_groups, hist, channels):
    """lad_label_histogram itself, into the caller's histogram."""
    import _hip
    dix = cases.index().to_device(channels, probs.device)
    C, T = probs.shape
    ws = _hip.workspace("lad_label_histogram_workspace_bytes", C, T, dix.n_intervals, device=probs.device)
    fps = np.asarray(fps, np.float64)
    _hip.launch("lad_label_histogram", probs, 0 if probs.dtype == torch.float32 else 1, C, T, lengths, dix.bounds, dix.offsets,
                dix.bounds_host, dix.offsets_host, dix.n_intervals, torch.from_numpy(fps).to(probs.device), fps, groups, n_groups, ws, hist)
    torch.cuda.synchronize()
    return hist


def test_identical_bytes_into_a_histogram_full_of_garbage():
    tile = _tile()
    tracks, channels, want = cases.case(("seeded", "constant"), (3 * tile + 5, 2 * tile + 1), (1, 3), (100.0, FPS), "float32", None, (0, 0))
    probs = _padded(tracks, np.float32)
    lengths, groups = np.asarray([len(t) for t in tracks], np.int64), np.zeros(2, np.int32)
    first = _raw(probs, lengths, [100.0, FPS], groups, 1, torch.full((1, 5, cm.SLOTS), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device="cuda"),
                 channels)
    second = _raw(probs, lengths, [100.0, FPS], groups, 1, torch.full((1, 5, cm.SLOTS), 7, dtype=torch.int64, device="cuda"), channels)
    assert np.array_equal(first.cpu().numpy(), want)
    assert first.cpu().numpy().tobytes() == second.cpu().numpy().tobytes()


def test_refusals_reach_python_and_write_nothing():
    import _hip
    import calibration
    channels = [cases.CHANNELS[0], cases.CHANNELS[1]]
    probs = torch.rand(2, 300, device="cuda")
    ok = dict(lengths=np.asarray([300, 200], np.int64), fps=[100.0, 50.0], groups=np.asarray([0, 1], np.int32), n_groups=2)
    bad = [dict(lengths=np.asarray([301, 200], np.int64)), dict(lengths=np.asarray([300, 0], np.int64)), dict(fps=[100.0, 0.0]),
           dict(fps=[100.0, float("nan")]), dict(fps=[1e-7, 50.0]), dict(groups=np.asarray([0, 2], np.int32)),
           dict(groups=np.asarray([-2, 0], np.int32)), dict(n_groups=3), dict(n_groups=0), dict(groups=None, n_groups=1)]
    for change in bad:
        hist = torch.full((3, 5, cm.SLOTS), 12345, dtype=torch.int64, device="cuda")
        with pytest.raises(_hip.LadHipError, match="lad_label_histogram"):
            _raw(probs, hist=hist, channels=channels, **dict(ok, **change))
        torch.cuda.synchronize()
        assert bool((hist == 12345).all()), change
    with pytest.raises(_hip.LadHipError):
        calibration.label_histogram_device(probs, channels, 100.0, cases.index(), lengths=[300, 301])
    with pytest.raises(_hip.LadHipError):
        calibration.label_histogram_device(probs, channels, [100.0, -1.0], cases.index())
    with pytest.raises(_hip.LadHipError):
        calibration.label_histogram_device(probs.half(), channels, 100.0, cases.index())
    with pytest.raises(ValueError):
        calibration.label_histogram_device(probs, channels[:1], 100.0, cases.index())
    table = torch.from_numpy(calibration.bucket_confidence()).cuda()
    out = torch.full((2, 300), -7.0, dtype=torch.float64, device="cuda")
    with pytest.raises(_hip.LadHipError, match="lad_track_remap"):
        _hip.launch("lad_track_remap", probs, 0, 2, 300, table, table)             # out overlaps the table
    with pytest.raises(_hip.LadHipError, match="lad_track_remap"):
        _hip.launch("lad_track_remap", probs, 5, 2, 300, table, out)
    with pytest.raises((ValueError, _hip.LadHipError)):
        calibration.apply_calibration_device(probs, calibration.bucket_confidence(), out=torch.empty(2, 300, device="cuda"))      # float32 out
    with pytest.raises(ValueError):
        calibration.apply_calibration_device(probs, np.full(cm.BUCKETS, 2.0))
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_apply_calibration_device_equals_the_host_form(dtype):
    import calibration
    import laugh_segmenter as ls
    tile = _tile()
    rng = np.random.default_rng(8)
    table = np.sort(rng.random(cm.BUCKETS))
    table[0], table[-1] = 0.0, 1.0
    x = np.stack([cases.track("seeded", 2 * tile + 3, dtype, seed=5), cases.track("distinct", 2 * tile + 3, dtype),
                  cases.track("seeded", 2 * tile + 3, dtype, seed=6)])
    x[2, -300:] = np.nan
    want = calibration.apply_calibration(x, table)
    got = ls.apply_calibration_device(torch.from_numpy(x).cuda(), table)
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == x.shape
    assert got.cpu().numpy().tobytes() == want.tobytes()
    one = calibration.apply_calibration_device(torch.from_numpy(x[0]).cuda(), table)
    assert tuple(one.shape) == x[0].shape and one.cpu().numpy().tobytes() == want[0].tobytes()
    out = torch.full(x.shape, -7.0, dtype=torch.float64, device="cuda")
    back = calibration.apply_calibration_device(torch.from_numpy(x).cuda(), torch.from_numpy(table).cuda(), out=out)
    assert back.data_ptr() == out.data_ptr() and out.cpu().numpy().tobytes() == want.tobytes()
    out1 = torch.full((x.shape[1],), -7.0, dtype=torch.float64, device="cuda")
    calibration.apply_calibration_device(torch.from_numpy(x[2]).cuda(), table, out=out1)
    assert out1.cpu().numpy().tobytes() == want[2].tobytes()
    # the calibrated track goes into the histogram as it is: device == host of the host-calibrated track
    channels = [cases.CHANNELS[0], cases.CHANNELS[1], cases.CHANNELS[3]]
    h = calibration.label_histogram_device(got, channels, 100.0, cases.index())
    assert np.array_equal(h, calibration.label_histogram_host(list(want), channels, 100.0, cases.index()))


def _files(path):
    return {f: open(path / f, "rb").read() for f in sorted(os.listdir(path))}


def test_evaluate_sweep_writes_the_same_bytes_on_both_routes(tmp_path):
    import evaluate_sweep
    args = sm.write_corpus(tmp_path)
    variants = {"report": ["--calibration_report"], "report_median": ["--calibration_report", "--median", "5", "--calibration_bins", "10"],
                "platt": ["--fit_calibration", "platt"], "temperature": ["--fit_calibration", "temperature"],
                "isotonic": ["--fit_calibration", "isotonic", "--calibration_report"]}
    for name, flags in variants.items():
        for scorer in ("host", "device"):
            evaluate_sweep.main(args + flags + ["--scorer", scorer, "--out_dir", str(tmp_path / f"{name}_{scorer}")])
        host, device = _files(tmp_path / f"{name}_host"), _files(tmp_path / f"{name}_device")
        assert sorted(host) == sorted(device) and len(host) >= 3, name
        assert host == device, name
    for method in ("platt", "isotonic"):
        flags = ["--calibration", str(tmp_path / f"{method}_host" / "calibration_table.npz"), "--calibration_report", "--penalties", "0.0,2.0"]
        for scorer in ("host", "device"):
            evaluate_sweep.main(args + flags + ["--scorer", scorer, "--out_dir", str(tmp_path / f"applied_{method}_{scorer}")])
        host, device = _files(tmp_path / f"applied_{method}_host"), _files(tmp_path / f"applied_{method}_device")
        assert host == device and sorted(host) == ["calibration.csv", "eval_df_per_meeting.csv", "reliability.csv", "sum_stats.csv"], method
        assert host["eval_df_per_meeting.csv"] != _files(tmp_path / "report_host")["eval_df_per_meeting.csv"]
