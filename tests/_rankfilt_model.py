"""The convention of lad_rank_filter (include/lad_hip.h) restated in plain Python: the model of tests/test_rankfilt_cpu.py and
tests/test_rankfilt_gpu.py.  Written from the header's two lines, independently of laugh_segmenter.rank_filter: no padding, no
window view, no partition -- a loop over the frames with clamped indices and a sort of each window's values.

    out[i] = sort_ascending( x[clamp(i - h + j, 0, n - 1)]  for j in 0 .. window-1 )[rank]      h = (window - 1) / 2
"""
import numpy as np


def rank_filter(x, window, rank):
    """x: 1-D float32 / float64 numpy of n >= 1 frames without NaN -> the same dtype, every element one of x's."""
    x = np.asarray(x)
    assert x.ndim == 1 and x.size >= 1 and x.dtype in (np.float32, np.float64)
    assert window % 2 == 1 and 1 <= window <= 1023 and 0 <= rank < window
    n, h = x.size, (window - 1) // 2
    out = np.empty_like(x)
    offsets = np.arange(window) - h
    for i in range(n):
        idx = np.minimum(np.maximum(i + offsets, 0), n - 1)
        out[i] = np.sort(x[idx], kind="stable")[rank]
    return out


def median_filter(x, window):
    return rank_filter(x, window, (window - 1) // 2)


def ranks(window):
    """The ranks the tests take: minimum, median, maximum and window // 3, without repeats, in that order."""
    out = []
    for r in (0, (window - 1) // 2, window - 1, window // 3):
        if r not in out:
            out.append(r)
    return out


def track(kind, n, dtype, seed=0):
    """A test track of n frames.  'random': uniform in [-0.2, 1.2), all values different; 'tied': 30 % of the frames at one value,
    0.375, the rest random; 'fp16': random values rounded to fp16 and clipped to [0, 1] (few distinct values, as the model's own
    track); 'constant': 0.625 everywhere; 'ramp': a strictly rising line through zero (negative values: both halves of the key
    map)."""
    rng = np.random.default_rng([seed, n, {"random": 1, "tied": 2, "fp16": 3, "constant": 4, "ramp": 5}[kind]])
    if kind == "constant":
        x = np.full(n, 0.625)
    elif kind == "ramp":
        x = (np.arange(n) - n // 3) / 64.0
    else:
        x = rng.uniform(-0.2, 1.2, n)
        if kind == "tied":
            x[rng.random(n) < 0.3] = 0.375
        elif kind == "fp16":
            x = np.clip(x, 0.0, 1.0).astype(np.float16).astype(np.float64)
    return x.astype(dtype)
