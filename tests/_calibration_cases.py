"""The cases tests/test_calibration_cpu.py and tests/test_calibration_gpu.py share: one hand-written and two seeded transcripts, the
tracks (special values, a constant one, one with every frame in another slot, two alternating values), and the model's histogram of
each case, computed once per process."""
import functools

import numpy as np

import _calibration_model as cm
import _score_model as sm

N_MS = 40000                             # the model's universe: every transcript row ends below it
NON_INTEGER_FPS = 44100.0 / 1024.0       # 43.06640625: frames of 23.22 ms
CHANNELS = [("Bmr001", "chan0"), ("Bmr001", "chan1"), ("Bmr001", "chanX"), ("Bed002", "chan2")]
SPECIALS = [0.0, -0.5, 1e-7, 3.0 / 65536.0, 0.5, 65535.0 / 65536.0, 1.0, 1.5, float("nan"), 0.9999999]

# chan0, at 100 frames per second (frames of 10 ms): boundaries inside a frame, INVALID overlapping LAUGH, an interval shorter than a
# frame, a frame (4000, 4010] straddling three intervals, an interval that ends beyond the channel's length
_HAND = [("speech", 0.0, 0.95), ("laugh", 1.003, 1.5), ("laugh", 2.0, 2.3), ("invalid", 2.1, 2.2), ("speech", 3.0, 3.004),
         ("noise", 4.001, 4.003), ("noise", 4.004, 4.006), ("noise", 4.007, 4.012), ("laugh", 5.5, 9.0), ("speech", 11.5, 13.0)]


@functools.lru_cache(maxsize=None)
def corpus():
    """(rows, channel table, the per-millisecond model)."""
    rows = [{"meeting_id": "Bmr001", "part_id": "fe001", "chan": None, "start": s, "end": e, "length": e - s, "type": k,
             "laugh_type": "laugh" if k == "laugh" else None} for k, s, e in _HAND]
    rows += sm.make_rows(21, "Bmr001", ["me002"], 30.0, n_per_type=12) + sm.make_rows(22, "Bed002", ["mn003"], 30.0, n_per_type=12)
    chans = [{"meeting_id": "Bmr001", "part_id": "fe001", "chan": "chan0", "length": 12.0},
             {"meeting_id": "Bmr001", "part_id": "me002", "chan": "chan1", "length": 30.0},
             {"meeting_id": "Bmr001", "part_id": None, "chan": "chanX", "length": 30.0},
             {"meeting_id": "Bed002", "part_id": "mn003", "chan": "chan2", "length": 25.0049375}]
    return rows, chans, sm.Model(rows, chans, N_MS)


@functools.lru_cache(maxsize=None)
def index():
    import sweep_eval as se
    rows, chans, _ = corpus()
    return se.TranscriptIndex(rows, chans)


def track(kind, n, dtype=np.float64, seed=0):
    """seeded: random values, a third of them from eight levels, the SPECIALS at seeded places; constant: one slot; distinct: every
    frame in a slot of its own; alternating: two values."""
    if kind == "constant":
        return np.full(n, 0.7, dtype)
    if kind == "distinct":
        return ((np.arange(n) * 20 + 1) / 65536.0 + 1e-9).astype(dtype)
    if kind == "alternating":
        return np.where(np.arange(n) % 2 == 0, 0.25, 0.75).astype(dtype)
    rng = np.random.default_rng(1000 + seed)
    x = rng.random(n)
    levels = rng.random(8)
    pick = rng.random(n) < 1 / 3
    x[pick] = levels[rng.integers(0, 8, int(pick.sum()))]
    at = rng.permutation(n)[:len(SPECIALS)]
    x[at] = np.asarray(SPECIALS)[:len(at)]
    return x.astype(dtype)


@functools.lru_cache(maxsize=None)
def case(kinds, sizes, chans, fps, dtype="float64", lengths=None, groups=None):
    """(tracks, [(meeting, chan)], the model's dense histogram) -- all arguments tuples, so that a case is computed once."""
    _, _, model = corpus()
    tracks = [track(k, n, np.dtype(dtype), seed=j) for j, (k, n) in enumerate(zip(kinds, sizes))]
    channels = [CHANNELS[c] for c in chans]
    sets = [cm.scoring_sets(model, *mc) for mc in channels]
    n_groups = len(tracks) if groups is None else max(max(groups) + 1, 1)
    want = cm.dense(cm.label_histogram(tracks, sets, list(fps), None if lengths is None else list(lengths),
                                       None if groups is None else list(groups)), n_groups)
    want.setflags(write=False)
    return tracks, channels, want
