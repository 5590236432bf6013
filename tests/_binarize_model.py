"""Second implementation of the hysteresis / gap-filling convention of include/lad_hip.h (lad_binarize_count), written from its
text: a per-frame state machine and a pairwise join loop in plain Python.  Imports nothing from the package."""
import math


def fixed(p):
    """p > 1 -> 1, p <= 0 -> 1e-7, anything else unchanged (NaN included), as a Python float (float64)."""
    p = float(p)
    if p > 1:
        return 1.0
    if p <= 0:
        return 0.0000001
    return p


def hysteresis_runs(probs, onset, offset):
    """[(first_frame, last_frame)] of active[i] = H[i] or (active[i - 1] and L[i]), active[-1] = 0."""
    runs = []
    active = False
    first = None
    for i, p in enumerate(probs):
        v = fixed(p)
        high, low = v > onset, v > offset          # NaN > x is False: in neither mask
        now = high or (active and low)
        if now and not active:
            first = i
        if active and not now:
            runs.append((first, i - 1))
        active = now
    if active:
        runs.append((first, len(probs) - 1))
    return runs


def fill_gaps(runs, min_gap, fps):
    """Two consecutive runs are joined iff not (next.first / fps - prev.last / fps > min_gap): pairwise on the original neighbours."""
    out = []
    for j, (first, last) in enumerate(runs):
        if j > 0 and not (first / fps - runs[j - 1][1] / fps > min_gap):
            out[-1] = (out[-1][0], last)
        else:
            out.append((first, last))
    return out


def spans(probs, onset, offset, min_gap=0.0, fps=100.0):
    assert math.isfinite(onset) and math.isfinite(offset) and math.isfinite(min_gap) and offset <= onset and min_gap >= 0
    return fill_gaps(hysteresis_runs(probs, onset, offset), float(min_gap), float(fps))


def instances(probs, thresholds, min_lengths, fps, offset_drops, min_gaps):
    """{(thr, drop, gap, min_l): [(start_s, end_s)]}: thresholds-major, then drop, then gap, then min_length."""
    fps = float(fps)
    out = {}
    for thr in thresholds:
        for drop in offset_drops:
            held = hysteresis_runs(probs, thr, thr - drop)
            for gap in min_gaps:
                merged = [(a / fps, b / fps) for a, b in fill_gaps(held, float(gap), fps)]
                for min_l in min_lengths:
                    out[(thr, drop, gap, min_l)] = [s for s in merged if s[1] - s[0] > min_l]
    return out
