"""GPU tests of the event-level scores on the dense sweep (csrc/surface_events.hip; sweep_eval.score_surface_device(..., events=);
evaluate_sweep.py --event_grid).

Integer bookkeeping plus IEEE float64 division, multiplication and rint: every comparison is an equality of whole arrays -- against
sweep_eval.score_surface_host(..., events=) (which tests/test_surface_events_cpu.py holds to score_sweep_host) and, on 64 levels,
against score_sweep_device(..., events=): lad_runs_count + lad_runs_fill + lad_score_runs + lad_score_events."""
import os

import numpy as np
import pytest
import torch

import _score_model as sm
from oracle import recipe
from test_surface_gpu import AWKWARD_FPS, CHANNELS, M, MIN_LENGTHS, NAMES, _index, _lds_edge, _levels, _tile, _tracks

pytestmark = pytest.mark.gpu

CRITERIA = [(1, 0), (20, 50), (0, 100)]


def _dev(tracks, channels, levels, min_lengths, fps, index, criteria, dtype=np.float32, **kw):
    import sweep_eval as se
    T = max(len(t) for t in tracks)
    padded = np.full((len(tracks), T), np.nan, dtype)
    for c, t in enumerate(tracks):
        padded[c, :len(t)] = t
    scores, events = se.score_surface_device(torch.from_numpy(padded).cuda(), channels, levels, min_lengths, fps, index, events=criteria, **kw)
    for got in (scores, events):
        assert got.dtype == np.int64 and got.shape == (len(tracks), len(levels), len(min_lengths), 7)
    return scores, events


def _same(got, want, names=None):
    for which, g, w in zip(("scores", "events"), got, want):
        for c in range(len(g)):
            assert np.array_equal(g[c], w[c]), (which, names[c] if names else c, np.argwhere(g[c] != w[c])[:5].tolist())


def _hand_index(spans, length, n_channels=1):
    """The same laugh (and other) rows for the first n_channels of CHANNELS."""
    import sweep_eval as se
    rows = [{"meeting_id": M, "part_id": f"fe{i:03d}", "chan": f"chan{i}", "start": s, "end": e, "length": e - s, "type": kind,
             "laugh_type": "laugh" if kind == "laugh" else None} for i in range(n_channels) for kind, s, e in spans]
    chans = [{"meeting_id": M, "part_id": f"fe{i:03d}", "chan": f"chan{i}", "length": length} for i in range(n_channels)]
    return se.TranscriptIndex(rows, chans)


@pytest.mark.parametrize("size", ["1", "t-1", "t", "t+1", "4t+3", "9t+5"])
def test_device_equals_host_on_every_track_shape(size):
    import sweep_eval as se
    t = _tile()
    T = {"1": 1, "t-1": t - 1, "t": t, "t+1": t + 1, "4t+3": 4 * t + 3, "9t+5": 9 * t + 5}[size]
    dtype = np.float64 if size in ("t+1", "9t+5") else np.float32
    tracks = [x.astype(dtype) for x in _tracks(T, t)]
    index = _index(9 * t / 100.0)
    levels = _levels(131, also=(float(tracks[0][T // 2]), 0.6))        # a value of the seeded track and the constant one: strict >
    criteria = CRITERIA[len(size) % 3]
    host = se.score_surface_host(tracks, CHANNELS, levels, MIN_LENGTHS, 100.0, index, events=criteria)
    _same(_dev(tracks, CHANNELS, levels, MIN_LENGTHS, 100.0, index, criteria, dtype), host, NAMES)
    assert (host[1][:, :, :, 0] > 0).all()
    if T > t + 40:
        assert host[1][:, :, :, 1].sum(axis=(1, 2)).min() > 0 and host[1][0, :, :, 2:].any()


@pytest.mark.parametrize("K", [1, 2, 131, "lds_fits", "lds_over"])
@pytest.mark.parametrize("L", [1, 3, 8])
def test_level_and_min_length_counts(K, L):
    import sweep_eval as se
    t = _tile()
    K = _lds_edge(9, L).get(K, K)                  # nine fields in this difference array (L = 1: 681 and 682 levels)
    T = 4 * t + 3
    tracks = [x.astype(np.float32) for x in _tracks(T, t)][:3] + [_tracks(T, t)[6].astype(np.float32)]
    channels = CHANNELS[:3] + [CHANNELS[6]]
    index = _index(9 * t / 100.0)
    levels = [0.5] if K == 1 else _levels(K)
    min_lengths = [float(v) for v in np.linspace(-0.01, 0.3, L)]
    host = se.score_surface_host(tracks, channels, levels, min_lengths, 100.0, index, events=(20, 50))
    _same(_dev(tracks, channels, levels, min_lengths, 100.0, index, (20, 50)), host)
    assert host[1][0, 0, 0, 1] > 0


def test_the_largest_level_count():
    import _hip
    import sweep_eval as se
    t = _tile()
    K = int(_hip.lib().lad_surface_max_levels())
    T = 2 * t + 3
    tracks = [x.astype(np.float32) for x in _tracks(T, t)][:3] + [_tracks(T, t)[6].astype(np.float32)]
    channels = CHANNELS[:3] + [CHANNELS[6]]
    index = _index(9 * t / 100.0)
    levels = _levels(K)
    host = se.score_surface_host(tracks, channels, levels, [0.1], 100.0, index, events=(1, 0))
    _same(_dev(tracks, channels, levels, [0.1], 100.0, index, (1, 0)), host)
    assert host[1][0, :, 0, 1].max() > 0 and len(set(host[1][0, :, 0, 4].tolist())) > 10


def test_three_time_bases_padding_an_unmapped_channel_and_identical_bytes():
    import sweep_eval as se
    t = _tile()
    index = _index(9 * t / 100.0)
    lengths = [4 * t + 3, 3 * t, 8 * t + 17, 4 * t - 1]
    tracks = [recipe.make_prob_track(30 + c, n).astype(np.float32) for c, n in enumerate(lengths)]
    channels = CHANNELS[:3] + [(M, "chanX")]
    fps = [100.0, AWKWARD_FPS, 2000.0, 100.0]
    levels = _levels(131)
    host = se.score_surface_host(tracks, channels, levels, MIN_LENGTHS, fps, index, events=(20, 50))
    got = _dev(tracks, channels, levels, MIN_LENGTHS, fps, index, (20, 50))
    _same(got, host)
    assert not got[1][3].any() and got[0][3, :, :, 0].sum() > 100                  # no participant: seven zeros
    assert all(got[1][c, :, :, 2].any() for c in range(2)) and got[1][2, :, :, 3].any()
    again = _dev(tracks, channels, levels, MIN_LENGTHS, fps, index, (20, 50))
    assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes()
    for c in range(4):                                                              # one channel at a time: the same rows
        alone = _dev([tracks[c]], [channels[c]], levels, MIN_LENGTHS, fps[c], index, (20, 50))
        assert np.array_equal(alone[0][0], got[0][c]) and np.array_equal(alone[1][0], got[1][c]), c
    # an all-NaN track next to another one; no frame at all: no launch, the events still counted
    nan = np.full(2 * t + 1, np.nan, np.float32)
    both = _dev([tracks[0], nan], channels[:2], levels, MIN_LENGTHS, 100.0, index, (20, 50))
    assert not both[0][1].any() and not both[1][1, :, :, 1:].any() and (both[1][1, :, :, 0] == host[1][1, 0, 0, 0]).all()
    assert np.array_equal(both[1][0], got[1][0])
    scores, events = se.score_surface_device(torch.zeros((1, 0), device="cuda"), channels[:1], levels, MIN_LENGTHS, 100.0, index, events=(1, 0))
    assert scores.shape == events.shape == (1, 131, 3, 7) and not scores.any() and not events[..., 1:].any()
    assert (events[..., 0] == host[1][0, 0, 0, 0]).all()


def test_against_the_run_table_kernels_on_64_levels():
    import sweep_eval as se
    t = _tile()
    T = 9 * t + 5
    index = _index(9 * t / 100.0)
    tracks = [x.astype(np.float32) for x in _tracks(T, t)]
    levels = _levels(64, also=(0.6,))
    padded = torch.from_numpy(np.stack(tracks)).cuda()
    want = se.score_sweep_device(padded, CHANNELS, levels, MIN_LENGTHS, 100.0, index, events=(20, 50))
    got = se.score_surface_device(padded, CHANNELS, levels, MIN_LENGTHS, 100.0, index, events=(20, 50))
    _same(got, want, NAMES)
    assert want[1][:, :, :, 2].sum() > 100 and want[1][:, :, :, 5].sum() > 0


def test_events_across_tile_borders_over_the_whole_track_and_none():
    import sweep_eval as se
    t = _tile()
    T = 4 * t + 3
    tracks = [x.astype(np.float32) for x in _tracks(T, t)]
    levels = _levels(131, also=(0.6,))
    ms = lambda frame: frame / 100.0                                                   # noqa: E731  (seconds of a frame at 100 fps)
    spans = {"across a border": [("laugh", ms(t - 3), ms(t + 3) + 0.2), ("invalid", ms(t + 3), ms(t + 3) + 0.3),
                                 ("laugh", ms(2 * t - 40), ms(2 * t + 1))],
             "three tiles": [("laugh", ms(t - 100), ms(3 * t + 100))],
             "the whole track": [("laugh", 0.0, ms(T))],
             "longer than the track": [("laugh", 0.0, ms(T) * 3)],
             "no laugh": [("speech", 1.0, 5.0), ("invalid", 2.0, 3.0)]}
    for i, (name, rows) in enumerate(spans.items()):
        index = _hand_index(rows, ms(T) * 3, len(NAMES))
        n_events = len(index.scoring_sets(*CHANNELS[0])[1])
        assert n_events == {"across a border": 2, "no laugh": 0}.get(name, 1), name
        for criteria in CRITERIA[i % 3:i % 3 + 1]:
            host = se.score_surface_host(tracks, CHANNELS, levels, MIN_LENGTHS, 100.0, index, events=criteria)
            _same(_dev(tracks, CHANNELS, levels, MIN_LENGTHS, 100.0, index, criteria), host, [f"{name}: {n}" for n in NAMES])
            assert (host[1][..., 0] == n_events).all() and host[1][..., 1:].any() == (n_events > 0)


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
    got = se.score_surface_device(dev, CHANNELS[:2], levels, MIN_LENGTHS, 100.0, index, lowpass=0.05, lengths=lengths, events=(20, 50))
    want = se.score_surface_host([smooth[c, :n] for c, n in enumerate(lengths)], CHANNELS[:2], levels, MIN_LENGTHS, 100.0, index,
                                 events=(20, 50))
    _same(got, want)
    assert want[1][:, :, :, 2].sum() > 10
    assert not np.array_equal(got[1], se.score_surface_device(dev, CHANNELS[:2], levels, MIN_LENGTHS, 100.0, index, events=(20, 50))[1])
    with pytest.raises(ValueError, match="cutoff"):
        se.score_surface_device(dev, CHANNELS[:2], levels, MIN_LENGTHS, 100.0, index, lengths=lengths, events=(20, 50))


def test_evaluate_sweep_event_grid_device_against_host(tmp_path, capsys):
    import evaluate_sweep
    args = sm.write_corpus(tmp_path)
    at = args.index("--thresholds")
    base = args[:at] + args[at + 2:] + ["--event_grid", "64", "--event_min_overlap_ms", "20", "--event_min_overlap_pct", "50"]
    out = {}
    for scorer in ("host", "device"):
        evaluate_sweep.main(base + ["--scorer", scorer, "--out_dir", str(tmp_path / scorer)])
        assert f"({scorer} scorer)" in capsys.readouterr().out
        out[scorer] = {f: open(tmp_path / scorer / f, "rb").read() for f in sorted(os.listdir(tmp_path / scorer))}
    assert list(out["host"]) == ["eval_df_per_meeting.csv", "event_df_per_meeting.csv", "event_pr_summary.csv", "event_sum_stats.csv",
                                 "pr_summary.csv", "sum_stats.csv"]
    assert out["host"] == out["device"]
    assert out["host"]["event_df_per_meeting.csv"].count(b"\n") == 1 + 2 * 65 * 2


def test_refusals_leave_the_path_usable():
    import _hip
    import sweep_eval as se
    lib = _hip.lib()
    kmax, lmax = int(lib.lad_surface_max_levels()), int(lib.lad_score_max_min_lengths())
    index = _index(9 * _tile() / 100.0)
    ch = CHANNELS[:1]
    p = torch.from_numpy(recipe.make_prob_track(50, 3000).astype(np.float32)).cuda().view(1, -1)
    ev = dict(events=(1, 0))
    for bad in (p.cpu(), p.to(torch.float16), (p * 10).to(torch.int32), torch.rand(2, 6000, device="cuda")[:1, ::2]):
        with pytest.raises((_hip.LadHipError, ValueError)):
            se.score_surface_device(bad, ch, [0.25, 0.5], [0.2], 100.0, index, **ev)
    with pytest.raises(_hip.LadHipError, match="levels 1.."):
        se.score_surface_device(p, ch, _levels(kmax + 1), [0.2], 100.0, index, **ev)
    with pytest.raises(_hip.LadHipError, match="min_lengths 1.."):
        se.score_surface_device(p, ch, [0.5], [0.1] * (lmax + 1), 100.0, index, **ev)
    with pytest.raises(_hip.LadHipError, match="millisecond overflow"):
        se.score_surface_device(p, ch, [0.5], [0.2], 1e-4, index, **ev)
    for bad in ((-1, 0), (1, 101)):
        with pytest.raises(_hip.LadHipError, match="min_overlap_pct 0..100"):
            se.score_surface_device(p, ch, [0.5], [0.2], 100.0, index, events=bad)
    with pytest.raises(ValueError, match="ascend strictly"):
        se.score_surface_device(p, ch, [0.5, 0.5], [0.2], 100.0, index, **ev)
    with pytest.raises(ValueError):
        se.score_surface_device(p, ch + ch, [0.5], [0.2], 100.0, index, **ev)
    # the DeviceIndex itself may be passed, and the path works after the refusals
    got = se.score_surface_device(p, ch, [0.25, 0.5], [0.2], 100.0, index.to_device(ch), **ev)
    want = se.score_surface_host([p[0].cpu().numpy()], ch, [0.25, 0.5], [0.2], 100.0, index, **ev)
    _same(got, want)
    assert got[1][0, 0, 0, 2] > 0 and got[0][0, 0, 0, 2] > 0
