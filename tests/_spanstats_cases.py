"""The tracks and the hand-made span tables that tests/test_spanstats_cpu.py and tests/test_spanstats_gpu.py share, and the
comparison of a form's three arrays with the model (tests/_spanstats_model.py): integers as integers, peak values as bytes."""
import functools

import numpy as np

import _spanstats_model as model

TRACKS = ["noise", "ones", "rising", "falling", "plateaus", "wild", "fp16"]
CHUNK = 2048        # lad_span_stats_tile_frames(): frames per workgroup of the prepare passes, and under a node of tree level 11
BLOCK = 256         # frames per step of the workgroup scan
THRESHOLDS = [0.1, 0.5, 0.9]
HYSTERESIS = [(0.5, 0.3, 0.05), (0.9, 0.1, 0.5)]      # (onset, offset, min_gap s): at 100 fps the gaps bridge 5 and 50 frames, NaN ones too
VITERBI = ([0.5], [0.0, 2.0])                         # thresholds, penalties (nats)
FPS = 100.0


@functools.lru_cache(maxsize=None)
def _track(kind, T, dtype):
    rng = np.random.default_rng(1000 + TRACKS.index(kind))
    if kind == "noise":
        x = rng.random(T)
    elif kind == "ones":                    # one span over the whole track at every threshold below 1
        x = np.ones(T)
    elif kind == "rising":                  # the peak of every span is its last frame
        x = np.linspace(0.01, 0.99, T)
    elif kind == "falling":                 # ... its first frame
        x = np.linspace(0.99, 0.01, T)
    elif kind == "plateaus":                # runs of 37 equal values: a tie goes to the earliest frame
        x = np.repeat(rng.integers(1, 9, T // 37 + 1) / 8.0, 37)[:T]
    elif kind == "wild":                    # values > 1, <= 0 (0.0 and negative ones) and NaN, single and in runs
        x = rng.random(T) * 2.0 - 0.5
        i = np.arange(T)
        x[i % 11 == 5] = 0.0
        x[i % 13 == 2] = 1.5
        x[i % 7 == 3] = np.nan
        x[(i % 500 >= 100) & (i % 500 < 104)] = np.nan
    elif kind == "fp16":                    # fp16-representable values, 33 distinct ones: many ties
        x = (rng.integers(0, 33, T) / 32.0).astype(np.float16).astype(np.float32)
    x = np.ascontiguousarray(x.astype(dtype))
    x.setflags(write=False)
    return x


def track(kind, T, dtype):
    """The read-only track `kind` of T frames as float32 or float64."""
    return _track(kind, int(T), np.dtype(dtype).name)


def edges_of(T):
    """The frames at which a pass of the device form changes workgroup, scan step or tree node of a stored launch."""
    e = {64, 128}
    e.update(range(BLOCK, T + 1, BLOCK) if T <= 3 * CHUNK else [BLOCK, CHUNK - BLOCK])
    e.update(range(CHUNK, T + 1, CHUNK) if T <= 3 * CHUNK else [CHUNK, 2 * CHUNK, CHUNK * CHUNK - CHUNK, CHUNK * CHUNK])
    return sorted(x for x in e if x <= T)


def hand_tables(T, every_frame=True, long_spans=True):
    """{name: int64 (n, 2)}: every frame its own span, one span over the whole track, spans that start or end on, one before and
    one after each edge, zero rows, and the three kinds of invalid row between valid neighbours."""
    t = {}
    if every_frame:
        t["every_frame"] = np.stack([np.arange(T), np.arange(T)], axis=1)
    if long_spans:
        t["whole"] = np.array([[0, T - 1]])
    rows = []
    for e in edges_of(T):
        near = [f for f in (e - 1, e, e + 1) if 0 <= f < T]
        for a in near:
            rows += [(a, b) for b in near + [min(T - 1, e + 70)] if a <= b]
            rows += [(max(0, e - 70), a)]
            if long_spans:
                rows += [(0, a), (a, T - 1)]
    t["edges"] = np.array(rows, np.int64).reshape(-1, 2)
    t["empty"] = np.zeros((0, 2), np.int64)
    lo, hi = (2, 5) if T >= 6 else (0, 0)
    t["invalid"] = np.array([[lo, hi], [-1, hi], [lo, T], [hi + 1, lo] if T >= 6 else [1, 0], [T - 1, T - 1]])
    return {k: v.astype(np.int64).reshape(-1, 2) for k, v in t.items()}


def model_arrays(x, spans):
    """The model's (sums, peaks, peak_values) of the spans of one track."""
    return model.as_arrays(model.span_stats(x.tolist(), np.asarray(spans).reshape(-1, 2).tolist()))


def assert_same(got, want, what):
    """Sums and peaks as integers, peak values as bytes."""
    for g, w, name in zip(got, want, ("sums", "peaks", "peak_values")):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if name == "peak_values":
            assert g.dtype == np.float64 and np.array_equal(g.view(np.int64), w.view(np.int64)), (what, name)
        else:
            assert g.dtype.kind == "i" and np.array_equal(g.astype(np.int64), w), (what, name)
