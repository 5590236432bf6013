"""GPU tests of the dense threshold sweep (csrc/surface.hip; sweep_eval.score_surface_device; evaluate_sweep.py --threshold_grid).

Integer bookkeeping plus IEEE float64 division, multiplication and rint: every comparison is an equality of whole arrays -- against
sweep_eval.score_surface_host (which tests/test_surface_cpu.py holds to score_sweep_host) and, on 64 levels, against
score_sweep_device, the kernels that were there before."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import _score_model as sm
from oracle import recipe

pytestmark = pytest.mark.gpu

AWKWARD_FPS = 360000 / 3600.0049375
MIN_LENGTHS = [0.0, 0.1, 0.2]
M = "Bmr001"
NAMES = ["seeded", "constant", "ramp up", "ramp down", "sawtooth", "plateau", "two plateaus", "dip", "NaN tile"]
CHANNELS = [(M, f"chan{i}") for i in range(len(NAMES))]


def _tile():
    import _hip
    return int(_hip.lib().lad_surface_tile_frames())


def _tracks(T, t):
    """The nine tracks of NAMES, T frames each, their features placed from the tile t (and clipped to a short track)."""
    ramp = (np.arange(T) + 1.0) / (T + 1.0)
    saw = 0.05 + 0.9 * (np.arange(T) % 37) / 36.0
    plateau = np.full(T, 0.2)
    plateau[max(t - 3, 0):t + 3] = 0.7                         # from 3 frames before a tile border to 3 behind it
    two = plateau.copy()
    two[t + 10:t + 40] = 0.7                                   # an equal plateau in the next tile: a node of its own
    two[2 * t - 1:2 * t + 1] = 0.7                             # and a pair across the next border, a dip of 0.45 between them
    two[t + 40:2 * t - 1] = 0.45
    dip = np.full(T, 0.8)
    dip[(3 * T) // 4] = 0.3
    nan_tile = recipe.make_prob_track(21, T) if T >= 100 else np.full(T, 0.6)
    nan_tile[t - 5:2 * t + 7] = np.nan                         # a whole tile and a little on both sides
    nan_tile[:min(3, T)] = np.nan
    seeded = recipe.make_prob_track(20, T) if T >= 100 else np.linspace(0.9, 0.1, T)
    return [seeded, np.full(T, 0.6), ramp, ramp[::-1].copy(), saw, plateau, two, dip, nan_tile]


@functools.lru_cache(maxsize=None)
def _index(duration):
    import sweep_eval as se
    parts = [f"fe{i:03d}" for i in range(len(NAMES))]
    rows = sm.make_rows(81, M, parts, duration * 1.05, n_per_type=60, max_len_s=duration / 50)
    chans = [{"meeting_id": M, "part_id": p, "chan": f"chan{i}", "length": duration * 0.97} for i, p in enumerate(parts)]
    chans.append({"meeting_id": M, "part_id": None, "chan": "chanX", "length": duration})
    return se.TranscriptIndex(rows, chans)


def _levels(K, also=()):
    lv = sorted(set(np.linspace(0.0, 1.0, K - len(also)).tolist()) | set(also))
    assert len(lv) == K
    return lv


def _dev(tracks, channels, levels, min_lengths, fps, index, dtype=np.float32, **kw):
    import sweep_eval as se
    T = max(len(t) for t in tracks)
    padded = np.full((len(tracks), T), np.nan, dtype)
    for c, t in enumerate(tracks):
        padded[c, :len(t)] = t
    got = se.score_surface_device(torch.from_numpy(padded).cuda(), channels, levels, min_lengths, fps, index, **kw)
    assert got.dtype == np.int64 and got.shape == (len(tracks), len(levels), len(min_lengths), 7)
    return got


@pytest.mark.parametrize("size", ["1", "2", "t-1", "t", "t+1", "4t+3", "9t+5"])
def test_device_equals_host_on_every_track_shape(size):
    import sweep_eval as se
    t = _tile()
    T = {"1": 1, "2": 2, "t-1": t - 1, "t": t, "t+1": t + 1, "4t+3": 4 * t + 3, "9t+5": 9 * t + 5}[size]
    dtype = np.float64 if size in ("t+1", "9t+5") else np.float32
    tracks = [x.astype(dtype) for x in _tracks(T, t)]
    index = _index(9 * t / 100.0)
    levels = _levels(131, also=(float(tracks[0][T // 2]), 0.6))        # a value of the seeded track and the constant one: strict >
    host = se.score_surface_host(tracks, CHANNELS, levels, MIN_LENGTHS, 100.0, index)
    got = _dev(tracks, CHANNELS, levels, MIN_LENGTHS, 100.0, index, dtype)
    for c, name in enumerate(NAMES):
        assert np.array_equal(got[c], host[c]), (name, T)
    q = float(np.asarray(0.6, dtype))                                                   # (float32(0.6) > 0.6: on at the level 0.6)
    assert got[1, :, 0, 0].tolist() == [int(q > lv and T > 1) for lv in levels]         # the constant track: one run, longer than 0 s
    if T > t + 40:
        assert host[:, :, :, 0].sum(axis=(1, 2)).min() > 0 and host[0, :, :, 2:].any()


def _lds_edge(fields, L):
    """{"lds_fits": the largest K at which the nodes kernel still keeps the difference array of one channel in LDS, "lds_over": the
    smallest at which it adds to global memory}: the array has K + 1 rows of L min_lengths x `fields` int64, and the entry point
    takes LDS iff those bytes are at most MAX_PRIVATE_BYTES (csrc/lad_surface_tree.h; read from there, so the cases move with it)."""
    import _hip
    header = os.path.join(os.path.dirname(os.path.abspath(_hip.__file__)), "csrc", "lad_surface_tree.h")
    kib = int(re.search(r"constexpr int MAX_PRIVATE_BYTES = (\d+) \* 1024;", open(header).read()).group(1))
    rows = kib * 1024 // (L * fields * 8)
    return {"lds_fits": rows - 1, "lds_over": rows}


@pytest.mark.parametrize("K", [1, 2, 131, "max", "lds_fits", "lds_over"])
@pytest.mark.parametrize("L", [1, 3, 8])
def test_level_and_min_length_counts(K, L):
    import _hip
    import sweep_eval as se
    t = _tile()
    K = {"max": int(_hip.lib().lad_surface_max_levels()), **_lds_edge(7, L)}.get(K, K)     # (L = 1: 876 and 877 levels)
    T = 4 * t + 3
    tracks = [x.astype(np.float32) for x in _tracks(T, t)][:3] + [_tracks(T, t)[6].astype(np.float32)]
    channels = CHANNELS[:3] + [CHANNELS[6]]
    index = _index(9 * t / 100.0)
    levels = [0.5] if K == 1 else _levels(K)
    min_lengths = [float(v) for v in np.linspace(-0.01, 0.3, L)]
    host = se.score_surface_host(tracks, channels, levels, min_lengths, 100.0, index)
    assert np.array_equal(_dev(tracks, channels, levels, min_lengths, 100.0, index), host)
    assert host[0, 0, 0, 0] > 0


def test_three_time_bases_padding_an_unmapped_channel_and_identical_bytes():
    import sweep_eval as se
    t = _tile()
    index = _index(9 * t / 100.0)
    lengths = [4 * t + 3, 3 * t, t + 17, 4 * t - 1]
    tracks = [recipe.make_prob_track(30 + c, n).astype(np.float32) for c, n in enumerate(lengths)]
    channels = CHANNELS[:3] + [(M, "chanX")]
    fps = [100.0, AWKWARD_FPS, 2000.0, 100.0]
    levels = _levels(131)
    host = se.score_surface_host(tracks, channels, levels, MIN_LENGTHS, fps, index)
    got = _dev(tracks, channels, levels, MIN_LENGTHS, fps, index)
    assert np.array_equal(got, host)
    assert got[3, :, :, 0].sum() > 100 and np.array_equal(got[3, :, :, 0], got[3, :, :, 1]) and not got[3, :, :, 3:].any()
    assert _dev(tracks, channels, levels, MIN_LENGTHS, fps, index).tobytes() == got.tobytes()
    for c in range(4):                                                                  # one channel at a time: the same rows
        assert np.array_equal(_dev([tracks[c]], [channels[c]], levels, MIN_LENGTHS, fps[c], index)[0], got[c]), c
    # an all-NaN track, alone and next to another one; a (T,) tensor is one channel; no frame at all: zeros without a launch
    nan = np.full(2 * t + 1, np.nan, np.float32)
    assert not _dev([nan], channels[:1], levels, MIN_LENGTHS, 100.0, index).any()
    both = _dev([tracks[0], nan], channels[:2], levels, MIN_LENGTHS, 100.0, index)
    assert not both[1].any() and np.array_equal(both[0], got[0])
    one = se.score_surface_device(torch.from_numpy(tracks[0]).cuda(), channels[:1], levels, MIN_LENGTHS, 100.0, index)
    assert np.array_equal(one[0], got[0])
    empty = se.score_surface_device(torch.zeros((1, 0), device="cuda"), channels[:1], levels, MIN_LENGTHS, 100.0, index)
    assert empty.shape == (1, 131, 3, 7) and not empty.any()
    assert se.score_surface_device(torch.from_numpy(tracks[0]).cuda(), channels[:1], [], MIN_LENGTHS, 100.0, index).shape == (1, 0, 3, 7)


def test_against_the_run_table_kernels_on_64_levels():
    import sweep_eval as se
    t = _tile()
    T = 9 * t + 5
    index = _index(9 * t / 100.0)
    tracks = [x.astype(np.float32) for x in _tracks(T, t)]
    levels = _levels(64, also=(0.6,))
    padded = torch.from_numpy(np.stack(tracks)).cuda()
    want = se.score_sweep_device(padded, CHANNELS, levels, MIN_LENGTHS, 100.0, index)
    got = se.score_surface_device(padded, CHANNELS, levels, MIN_LENGTHS, 100.0, index)
    assert np.array_equal(got, want) and want[:, :, :, 0].sum() > 1000


def test_lowpass_in_front_of_the_tree():
    import laugh_segmenter as ls
    import sweep_eval as se
    t = _tile()
    index = _index(9 * t / 100.0)
    lengths = [2 * t + 9, t + 100]
    tracks = [recipe.make_prob_track(40 + c, n).astype(np.float32) for c, n in enumerate(lengths)]
    padded = np.full((2, max(lengths)), np.nan, np.float32)
    for c, x in enumerate(tracks):
        padded[c, :len(x)] = x
    dev = torch.from_numpy(padded).cuda()
    smooth = ls.lowpass_device(dev, cutoff=0.05, lengths=lengths).cpu().numpy()
    levels = _levels(131)
    got = se.score_surface_device(dev, CHANNELS[:2], levels, MIN_LENGTHS, 100.0, index, lowpass=0.05, lengths=lengths)
    want = se.score_surface_host([smooth[c, :n] for c, n in enumerate(lengths)], CHANNELS[:2], levels, MIN_LENGTHS, 100.0, index)
    assert np.array_equal(got, want) and want[:, :, :, 0].sum() > 100
    assert not np.array_equal(got, se.score_surface_device(dev, CHANNELS[:2], levels, MIN_LENGTHS, 100.0, index))
    with pytest.raises(ValueError, match="cutoff"):
        se.score_surface_device(dev, CHANNELS[:2], levels, MIN_LENGTHS, 100.0, index, lengths=lengths)


def test_evaluate_sweep_threshold_grid_device_against_host(tmp_path, capsys):
    import evaluate_sweep
    args = sm.write_corpus(tmp_path)
    at = args.index("--thresholds")
    base = args[:at] + args[at + 2:] + ["--threshold_grid", "64"]
    out = {}
    for scorer in ("host", "device"):
        evaluate_sweep.main(base + ["--scorer", scorer, "--out_dir", str(tmp_path / scorer)])
        assert f"({scorer} scorer)" in capsys.readouterr().out
        out[scorer] = {f: open(tmp_path / scorer / f, "rb").read() for f in sorted(os.listdir(tmp_path / scorer))}
    assert list(out["host"]) == ["eval_df_per_meeting.csv", "pr_summary.csv", "sum_stats.csv"]
    assert out["host"] == out["device"]
    assert out["host"]["eval_df_per_meeting.csv"].count(b"\n") == 1 + 2 * 65 * 2


def test_refusals_leave_the_path_usable():
    import _hip
    import sweep_eval as se
    lib = _hip.lib()
    kmax, lmax = int(lib.lad_surface_max_levels()), int(lib.lad_score_max_min_lengths())
    index = _index(9 * _tile() / 100.0)
    ch = CHANNELS[:1]
    p = torch.from_numpy(recipe.make_prob_track(50, 3000).astype(np.float32)).cuda().view(1, -1)
    for bad in (p.cpu(), p.to(torch.float16), (p * 10).to(torch.int32), torch.rand(2, 6000, device="cuda")[:1, ::2]):
        with pytest.raises((_hip.LadHipError, ValueError)):
            se.score_surface_device(bad, ch, [0.25, 0.5], [0.2], 100.0, index)
    with pytest.raises(_hip.LadHipError, match="levels 1.."):
        se.score_surface_device(p, ch, _levels(kmax + 1), [0.2], 100.0, index)
    with pytest.raises(_hip.LadHipError, match="min_lengths 1.."):
        se.score_surface_device(p, ch, [0.5], [0.1] * (lmax + 1), 100.0, index)
    with pytest.raises(_hip.LadHipError, match="millisecond overflow"):
        se.score_surface_device(p, ch, [0.5], [0.2], 1e-4, index)
    with pytest.raises(ValueError, match="ascend strictly"):
        se.score_surface_device(p, ch, [0.5, 0.5], [0.2], 100.0, index)
    with pytest.raises(ValueError):
        se.score_surface_device(p, ch + ch, [0.5], [0.2], 100.0, index)
    # the DeviceIndex itself may be passed, and the path works after the refusals
    got = se.score_surface_device(p, ch, [0.25, 0.5], [0.2], 100.0, index.to_device(ch))
    assert np.array_equal(got, se.score_surface_host([p[0].cpu().numpy()], ch, [0.25, 0.5], [0.2], 100.0, index)) and got[0, 0, 0, 2] > 0
