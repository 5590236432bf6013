"""GPU tests of hysteresis and gap filling on the device (csrc/binarize.hip; laugh_segmenter.binarize_frame_spans_device /
binarize_instances_device; sweep_eval.score_sweep_device with offset_drops / min_gaps).

Integer bookkeeping and IEEE float64 division: every comparison is an equality -- against the plain device sweep (csrc/runs.hip)
where the settings reduce to it, against the per-frame model of tests/_binarize_model.py, and against the host forms."""
import ctypes

import numpy as np
import pytest
import torch

import _binarize_model as bm
import _lowpass_model as lm
import _score_model as sm
from oracle import recipe

pytestmark = pytest.mark.gpu

EVAL_THRESHOLDS = [float(t) for t in np.concatenate((np.linspace(0, 0.9, 19).round(2), np.linspace(0.91, 1, 10).round(2)))]
ONSETS = [0.0, 0.2, 0.5, 0.9, 1.0]
DROPS = [0.0, 0.05, 0.3, 1.5]
GAPS = [0.0, 0.03, 0.2, 1.0, 1e9]
AWKWARD_FPS = 36000 / 360.37
M = "Bmr001"


def _tile():
    import _hip
    return int(_hip.lib().lad_runs_tile_frames())


def _tuples(a):
    return [tuple(int(v) for v in r) for r in a]


def _dev(p, settings, fps=100.0):
    """binarize_frame_spans_device of a numpy track (T,) or (C, T) as lists of tuples."""
    import laugh_segmenter as ls
    got = ls.binarize_frame_spans_device(torch.from_numpy(np.ascontiguousarray(p)).cuda(), settings, fps)
    if np.ndim(p) == 1:
        got = [got]
    for per_channel in got:
        assert len(per_channel) == len(settings)
        for g in per_channel:
            assert g.dtype == np.int64 and g.ndim == 2 and g.shape[1] == 2
    got = [[_tuples(g) for g in per_channel] for per_channel in got]
    return got[0] if np.ndim(p) == 1 else got


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_reduces_to_the_plain_sweep(dtype):
    import laugh_segmenter as ls
    tile = _tile()
    settings = [(t, t, 0.0) for t in EVAL_THRESHOLDS]
    n_runs = 0
    for seed, n in enumerate([1, 2, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile, 1000, 36000]):
        p = (recipe.make_prob_track(seed, n) if n >= 100 else np.random.default_rng(seed).random(n)).astype(dtype)
        if n >= 1000:                       # values at float32(t) and its neighbours, where float32 rounds t up
            rng = np.random.default_rng(seed)
            for t in EVAL_THRESHOLDS:
                c = np.float32(t)
                p[rng.integers(0, n, 20)] = np.array([np.nextafter(c, np.float32(-1)), c, np.nextafter(c, np.float32(2))])[rng.integers(0, 3, 20)]
        dev = torch.from_numpy(p).cuda()
        plain = ls.get_laughter_frame_spans_device(dev, EVAL_THRESHOLDS)
        got = ls.binarize_frame_spans_device(dev, settings, 100.0)
        assert len(got) == len(plain) == 29
        for k in range(29):
            assert np.array_equal(got[k], plain[k]), (n, EVAL_THRESHOLDS[k])
            n_runs += len(plain[k])
    assert n_runs > 10000


def test_carry_across_tiles():
    tile = _tile()
    T = 4 * tile + 3
    setting = [(0.5, 0.3, 0.0)]
    for dtype in (np.float32, np.float64):
        held = np.full(T, 0.4, dtype)
        assert _dev(held, setting) == [[]]                                             # all held, no onset: no run
        for s in (0, 63, 64, tile - 1, tile, tile + 1, 2 * tile - 1):
            p = held.copy()
            p[s] = 0.9
            assert _dev(p, setting) == [[(s, T - 1)]], s
            for e in (s + 1, 2 * tile, 2 * tile + 1, 3 * tile - 1):
                q = p.copy()
                q[e] = 0.1
                assert _dev(q, setting) == [[(s, e - 1)]] == [bm.spans(q.tolist(), 0.5, 0.3)], (s, e)
        p = held.copy()
        p[5] = 0.9
        p[2 * tile + 17] = np.nan                                                      # a NaN in the third tile ends the run there
        assert _dev(p, setting) == [[(5, 2 * tile + 16)]]
        p[2 * tile + 17] = 0.1
        p[3 * tile + 1] = 0.9                                                          # a second onset behind the release
        assert _dev(p, setting) == [[(5, 2 * tile + 16), (3 * tile + 1, T - 1)]]
        p[tile + 3] = 0.95                                                             # a second onset inside the hold: still one run
        assert _dev(p, setting) == [[(5, 2 * tile + 16), (3 * tile + 1, T - 1)]]


@pytest.fixture(scope="module")
def random_case():
    """Three channels of float32-representable values (so that one model serves both dtypes), the third NaN-padded short, at two
    lengths; {n: (tracks (3, n) float64, lengths, {(c, onset, drop): hysteresis runs of the per-frame loop})}."""
    out = {}
    for n in (36000, 3 * 512 + 7):
        lengths = [n, n, n - n // 7]
        tracks = np.full((3, n), np.nan)
        for c in range(3):
            t = recipe.make_prob_track(50 + c, lengths[c]).astype(np.float32).astype(np.float64)
            if c == 1:
                rng = np.random.default_rng(c)
                t[rng.integers(0, len(t), len(t) // 40)] = np.nan
            tracks[c, :lengths[c]] = t
        runs = {(c, on, dr): bm.hysteresis_runs(tracks[c].tolist(), on, on - dr) for c in range(3) for on in ONSETS for dr in DROPS}
        out[n] = (tracks, lengths, runs)
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [36000, 3 * 512 + 7])
def test_random_tracks_against_the_model(random_case, n, dtype):
    assert _tile() == 512
    tracks, lengths, runs = random_case[n]
    fps = [100.0, AWKWARD_FPS, 97.25]
    triples = [(on, dr, gap) for on in ONSETS for dr in DROPS for gap in GAPS]
    settings = [(on, on - dr, gap) for on, dr, gap in triples]                         # 100 settings: two calls underneath
    got = _dev(tracks.astype(dtype), settings, fps)
    joined = 0
    for c in range(3):
        for k, (on, dr, gap) in enumerate(triples):
            want = bm.fill_gaps(runs[(c, on, dr)], gap, fps[c])
            assert got[c][k] == want, (c, on, dr, gap)
            joined += len(runs[(c, on, dr)]) - len(want)
    assert joined > 100


def test_gap_filling_across_tiles():
    tile = _tile()
    T = 3 * tile
    p = np.full((2, T), 0.1)
    p[0, ::3] = 0.9                                                                    # single-frame events every 3 frames
    p[1, 1::3] = 0.9
    gaps = [0.0, 0.02, 0.03, 0.04, 1e9]
    got = _dev(p, [(0.5, 0.5, g) for g in gaps], 100.0)
    for c in range(2):
        for k, g in enumerate(gaps):
            assert got[c][k] == bm.spans(p[c].tolist(), 0.5, 0.5, g, 100.0), (c, g)
        assert len(got[c][0]) == T // 3 and got[c][-1] == [(c, T - 3 + c)]              # min_gap 1e9: one run per channel
    assert len(got[0][1]) == T // 3 and len(got[0][3]) == 1                            # 0.03 s apart: 0.02 keeps, 0.04 joins


def test_sixty_four_settings_and_more():
    import _hip
    import laugh_segmenter as ls
    kmax = int(_hip.lib().lad_binarize_max_settings())
    assert kmax == 64
    p = recipe.make_prob_track(7, 5000)
    p[1000:1010] = np.nan
    onsets = np.linspace(0.05, 1.0, 16)
    settings = [(float(on), float(on - dr), float(g)) for on in onsets for dr in (0.0, 0.2) for g in (0.0, 0.15)]
    assert len(settings) == kmax and len(set(settings)) == kmax
    dev = torch.from_numpy(p).cuda()
    got = ls.binarize_frame_spans_device(dev, settings, AWKWARD_FPS)
    for s, g in zip(settings, got):
        assert np.array_equal(g, ls.binarize_frame_spans(p, *s, fps=AWKWARD_FPS)), s
    more = settings + [(0.5, 0.1, float(g)) for g in np.linspace(0.0, 2.0, 70)]         # 134 settings: three calls underneath
    got = ls.binarize_frame_spans_device(dev, more, AWKWARD_FPS)
    assert len(got) == len(more)
    for s, g in zip(more, got):
        assert np.array_equal(g, ls.binarize_frame_spans(p, *s, fps=AWKWARD_FPS)), s
    assert len(got[-1]) < len(got[kmax])


def _raw_call(p, settings, fps, capacity=None, sentinel=-7):
    """lad_binarize_count + lad_binarize_fill through the C ABI -> (code of the fill, raw counts, merged counts, raw table, table)."""
    import _hip
    lib = _hip.lib()
    C, T = p.shape
    K = len(settings)
    cols = [(ctypes.c_double * K)(*[s[j] for s in settings]) for j in range(3)]
    fps_host = np.asarray(fps, np.float64)
    fps_dev = torch.from_numpy(fps_host).cuda()
    st = _hip.stream_handle()
    ws = torch.empty(lib.lad_binarize_workspace_bytes(C, T, K), dtype=torch.uint8, device="cuda")
    dtype = 0 if p.dtype == torch.float32 else 1
    _hip.check(lib.lad_binarize_count(_hip.ptr(p), dtype, C, T, cols[0], cols[1], K, _hip.ptr(ws), st), "lad_binarize_count")
    raw_counts = np.ascontiguousarray(ws[:4 * C * K].view(torch.int32).cpu().numpy())
    total = int(raw_counts.sum())
    capacity = total if capacity is None else capacity
    raw = torch.full((max(capacity, 1) + 4, 2), sentinel, dtype=torch.int32, device="cuda")
    table = torch.full((max(capacity, 1) + 4, 2), sentinel, dtype=torch.int32, device="cuda")
    rc = lib.lad_binarize_fill(_hip.ptr(p), dtype, C, T, cols[0], cols[1], cols[2], K, _hip.ptr(fps_dev),
                               fps_host.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), _hip.ptr(ws),
                               raw_counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), _hip.ptr(raw), _hip.ptr(table), capacity, st)
    torch.cuda.synchronize()
    counts = ws[:4 * C * K].view(torch.int32).cpu().numpy().copy()
    return rc, raw_counts, counts, raw.cpu().numpy(), table.cpu().numpy()


def test_determinism_capacity_and_refusals():
    import _hip
    lib = _hip.lib()
    tracks = np.stack([recipe.make_prob_track(21, 20000), recipe.make_prob_track(22, 20000)])
    p = torch.from_numpy(tracks).cuda()
    settings = [(0.5, 0.5, 0.0), (0.5, 0.3, 0.05), (0.8, 0.2, 0.3), (0.3, 0.3, 1e9)]
    fps = [100.0, AWKWARD_FPS]
    rc, raw_counts, counts, raw, table = _raw_call(p, settings, fps)
    assert rc == 0
    total, merged = int(raw_counts.sum()), int(counts.sum())
    assert 0 < merged < total and (counts <= raw_counts).all() and counts[3] == 1 and counts[0] == raw_counts[0]
    assert (table[merged:] == -7).all() and (raw[total:] == -7).all()                   # nothing behind the tables
    assert (table[:merged] >= 0).all() and (raw[:total] >= 0).all()
    edges, raw_edges = np.concatenate([[0], np.cumsum(counts)]), np.concatenate([[0], np.cumsum(raw_counts)])
    for c in range(2):
        for k, (on, off, gap) in enumerate(settings):
            i = c * len(settings) + k
            assert _tuples(raw[raw_edges[i]:raw_edges[i + 1]]) == bm.hysteresis_runs(tracks[c].tolist(), on, off), (c, k)
            assert _tuples(table[edges[i]:edges[i + 1]]) == bm.spans(tracks[c].tolist(), on, off, gap, fps[c]), (c, k)
    again = _raw_call(p, settings, fps)
    assert again[0] == 0 and again[2].tobytes() == counts.tobytes() and again[4].tobytes() == table.tobytes()
    assert again[3].tobytes() == raw.tobytes()
    # one row short: refused, the sentinel-filled tables and the counts in the workspace unchanged
    rc, raw_counts2, counts2, raw2, table2 = _raw_call(p, settings, fps, capacity=total - 1)
    assert rc == _hip.LAD_ERR_INVALID and b"the tables hold" in lib.lad_last_error()
    assert (table2 == -7).all() and (raw2 == -7).all() and np.array_equal(counts2, raw_counts2)
    # refused before any launch
    for change, message in ((dict(settings=[(0.3, 0.5, 0.0)]), b"lies above"), (dict(settings=[(0.5, 0.3, -0.1)]), b"min_gap"),
                            (dict(settings=[(0.5, 0.3, float("inf"))]), b"min_gap"), (dict(fps=[100.0, 0.0]), b"positive finite"),
                            (dict(fps=[-1.0, 100.0]), b"positive finite"), (dict(fps=[float("nan"), 100.0]), b"positive finite")):
        kw = dict(settings=[(0.5, 0.3, 0.1)], fps=fps)
        kw.update(change)
        if message == b"lies above":
            K = 1
            cols = [(ctypes.c_double * K)(kw["settings"][0][j]) for j in range(2)]
            ws = torch.full((lib.lad_binarize_workspace_bytes(2, 20000, K),), 0x55, dtype=torch.uint8, device="cuda")
            rc = lib.lad_binarize_count(_hip.ptr(p), 1, 2, 20000, cols[0], cols[1], K, _hip.ptr(ws), _hip.stream_handle())
            torch.cuda.synchronize()
            assert rc == _hip.LAD_ERR_INVALID and message in lib.lad_last_error() and bool((ws == 0x55).all())
            continue
        rc, rc_counts, counts3, raw3, table3 = _raw_call(p, **kw)
        assert rc == _hip.LAD_ERR_INVALID and message in lib.lad_last_error(), (change, lib.lad_last_error())
        assert (table3 == -7).all() and (raw3 == -7).all() and np.array_equal(counts3, rc_counts)
    assert lib.lad_binarize_workspace_bytes(1, 1000, 65) == -1 and b"settings 1..64" in lib.lad_last_error()
    assert lib.lad_binarize_workspace_bytes(0, 1000, 1) == -1 and lib.lad_binarize_workspace_bytes(1, 2 ** 30 + 1, 1) == -1
    assert lib.lad_binarize_workspace_bytes(65535, 2 ** 30, 64) > 0
    # the path is usable afterwards
    assert _raw_call(p, settings, fps)[4].tobytes() == table.tobytes()


def _corpus(seed, parts, duration, n_per_type, max_len_s):
    import sweep_eval as se
    rows = sm.make_rows(seed, M, parts, duration, n_per_type=n_per_type, max_len_s=max_len_s)
    chans = [{"meeting_id": M, "part_id": p, "chan": f"chan{i}", "length": duration * 0.97} for i, p in enumerate(parts)]
    return se.TranscriptIndex(rows, chans)


@pytest.mark.parametrize("lowpass", [None, 0.01])
def test_scores_against_the_host_scorer(lowpass):
    import laugh_segmenter as ls
    import sweep_eval as se
    T, C = 36000, 3
    index = _corpus(31, ["fe001", "me002", "mn003"], 380.0, 100, 1.0)                  # 3 x 4 x 100 transcript rows
    channels = [(M, f"chan{i}") for i in range(C)]
    lengths = [T, T - 1000, T]
    fps = [100.0, AWKWARD_FPS, 97.25]
    thresholds, min_lengths, drops, gaps = EVAL_THRESHOLDS[3::5], [0.0, 0.1, 0.2], [0.0, 0.1, 0.3], [0.0, 0.2, 1.0]
    padded = np.full((C, T), np.nan, np.float32)
    for c in range(C):       # the plateau tracks of the low-pass tests: a filtered one crosses every level
        padded[c, :lengths[c]] = lm.make_track(60 + c, lengths[c]) if lowpass is not None else recipe.make_prob_track(60 + c, lengths[c])
    tracks = [padded[c, :lengths[c]] for c in range(C)]
    if lowpass is not None:
        tracks = [ls.lowpass(t, cutoff=lowpass) for t in tracks]                       # scipy on the host
        levels = np.asarray(sorted({0.0} | {t - d for t in thresholds for d in drops}))
        for t in tracks:     # no decision hangs on the last digits of either filter (they agree to lm.tol: some 1e-11)
            assert float(np.min(np.abs(t[:, None] - levels[None, :]))) > 1e-7
    dev = se.score_sweep_device(torch.from_numpy(padded).cuda(), channels, thresholds, min_lengths, fps, index, lowpass=lowpass,
                                lengths=lengths if lowpass is not None else None, offset_drops=drops, min_gaps=gaps)
    assert dev.dtype == np.int64 and dev.shape == (C, len(thresholds), 3, 3, 3, 7)
    host = se.score_sweep_host(tracks, channels, thresholds, min_lengths, fps, index, offset_drops=drops, min_gaps=gaps)
    assert np.array_equal(dev, host)
    assert (host.sum(axis=(0, 1, 2, 3, 4)) > 0).all() and (host[..., 0].reshape(-1) > 0).sum() > 100
    # drop 0 and gap 0 are the plain device sweep
    plain = se.score_sweep_device(torch.from_numpy(padded).cuda(), channels, thresholds, min_lengths, fps, index, lowpass=lowpass,
                                  lengths=lengths if lowpass is not None else None)
    assert np.array_equal(dev[:, :, 0, 0], plain)
    assert (dev[:, :, 0, 2, 0, 0] <= plain[:, :, 0, 0]).all() and (dev[:, :, 0, 2, 0, 0] < plain[:, :, 0, 0]).any()   # gaps join


def test_scored_sweep_of_two_rounds():
    """80 settings: a round of lad_binarize_max_settings() = 64 and one of 16, three tiles and a ragged end, two channels."""
    import sweep_eval as se
    T, C = 3 * 512 + 7, 2
    fps = [100.0, 97.25]
    index = _corpus(31, ["fe001", "me002"], T / 97.25, 12, 1.0)                         # channel length 0.97 * T / 97.25
    channels = [(M, f"chan{i}") for i in range(C)]
    thresholds, drops, gaps, min_lengths = [0.2, 0.35, 0.5, 0.65, 0.8], [0.0, 0.05, 0.1, 0.2], [0.0, 0.05, 0.2, 1.0], [0.0, 0.1]
    tracks = np.stack([recipe.make_prob_track(60 + c, T) for c in range(C)]).astype(np.float32)
    host = se.score_sweep_host(list(tracks), channels, thresholds, min_lengths, fps, index, offset_drops=drops, min_gaps=gaps)
    # nothing here passes on empty tables, and the two rounds score different settings
    assert host.shape == (2, 5, 4, 4, 2, 7) and (host[..., 0, 0] > 0).all() and (host.sum(axis=(0, 1, 2, 3, 4)) > 0).all()
    flat = host.reshape(C, 80, 2, 7)
    assert not np.array_equal(flat[:, :16], flat[:, 64:])
    d = torch.from_numpy(tracks).cuda()
    dev = se.score_sweep_device(d, channels, thresholds, min_lengths, fps, index, offset_drops=drops, min_gaps=gaps)
    assert dev.dtype == np.int64 and dev.shape == (2, 5, 4, 4, 2, 7)
    assert np.array_equal(dev, host)
    assert np.array_equal(dev[:, :, 0, 0], se.score_sweep_device(d, channels, thresholds, min_lengths, fps, index))
    again = se.score_sweep_device(d, channels, thresholds, min_lengths, fps, index, offset_drops=drops, min_gaps=gaps)
    assert again.tobytes() == dev.tobytes()


def test_instances_device_against_host():
    import laugh_segmenter as ls
    thresholds, min_lengths, drops, gaps = [0.2, 0.5, 0.9], [0.0, 0.1, 0.2], [0.0, 0.1, 0.4], [0.0, 0.05, 0.5]
    for dtype in (np.float32, np.float64):
        p = recipe.make_prob_track(33, 36000).astype(dtype)
        for fps in (100.0, AWKWARD_FPS):
            want = ls.binarize_instances(p, thresholds, min_lengths, fps, drops, gaps)
            got = ls.binarize_instances_device(torch.from_numpy(p).cuda(), thresholds, min_lengths, fps, drops, gaps)
            assert list(got.keys()) == list(want.keys()) and got == want
            assert all(type(v) is float for spans in got.values() for s in spans for v in s)
    # an empty track and the refusals of the Python surface
    assert ls.binarize_instances_device(torch.zeros(0, device="cuda"), [0.5], [0.2], 100.0, [0.1], [0.2]) == {(0.5, 0.1, 0.2, 0.2): []}
    import _hip
    for bad in (torch.zeros(10), torch.zeros(10, device="cuda", dtype=torch.float16)):
        with pytest.raises(_hip.LadHipError):
            ls.binarize_frame_spans_device(bad, [(0.5, 0.3, 0.0)], 100.0)
    with pytest.raises(ValueError):
        ls.binarize_frame_spans_device(torch.zeros(10, device="cuda"), [(0.3, 0.5, 0.0)], 100.0)
    with pytest.raises(ValueError):
        ls.binarize_frame_spans_device(torch.zeros(10, device="cuda"), [(0.5, 0.3, 0.0)], 0.0)
