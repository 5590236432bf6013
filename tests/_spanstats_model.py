"""Independent model of the span statistics (the convention above lad_span_stats in include/lad_hip.h): a Python loop over the
frames of every span in Python ints and floats, numpy.rint on single values, the earliest maximum kept explicitly.  It shares no
code with laugh_segmenter.span_stats and is the yardstick of both the host and the device form."""
import numpy as np

TWO32 = float(2 ** 32)


def frame_value(x):
    """w of one element: the decoders' fixed value (float64; > 1 -> 1.0, <= 0 -> 0.0000001), 0.0 for NaN."""
    v = float(x)
    if v != v:
        return 0.0
    if v > 1:
        return 1.0
    if v <= 0:
        return 0.0000001
    return v


_FIXED = {}


def fixed(w):
    """Q of one frame value: rint(w * 2^32), round-half-even, as a Python int (remembered per value: tracks of few distinct values
    make a span of millions of frames affordable)."""
    q = _FIXED.get(w)
    if q is None:
        if len(_FIXED) > 1 << 20:
            _FIXED.clear()
        q = _FIXED[w] = int(np.rint(np.float64(w) * TWO32))
    return q


def span_stats(track, spans):
    """[(sum, peak, peak_value)] per row (first, last) of `spans`: Python int, int, float."""
    T = len(track)
    out = []
    for first, last in spans:
        first, last = int(first), int(last)
        if first < 0 or last >= T or first > last:
            out.append((0, -1, 0.0))
            continue
        total, peak, best = 0, -1, -1.0
        for i in range(first, last + 1):
            w = frame_value(track[i])
            total += fixed(w)
            if w > best:            # (strictly: the earliest of equal maxima stays)
                peak, best = i, w
        out.append((total, peak, best))
    return out


def as_arrays(rows):
    """The model's rows as (sums int64, peaks int64, peak_values float64)."""
    return (np.array([r[0] for r in rows], np.int64).reshape(-1), np.array([r[1] for r in rows], np.int64).reshape(-1),
            np.array([r[2] for r in rows], np.float64).reshape(-1))


def confidence(row, first, last, fps):
    """(mean, peak_time, peak_value) of one valid row: Python floats."""
    total, peak, value = row
    return (float(total) / float((last - first + 1) * 2 ** 32), peak / fps, value)
