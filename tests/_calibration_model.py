"""The yardstick of tests/test_calibration_cpu.py and tests/test_calibration_gpu.py: a second implementation of the label histogram,
written from the text above lad_label_histogram in include/lad_hip.h, and brute-force forms of the figures and of the isotonic fit.

A set of milliseconds is a boolean array as in tests/_score_model.py (element m is millisecond m, (lo, hi] the slice lo + 1 .. hi);
the five sets of a channel come from that model's indices, with INVALID taken out of the other four here.  The histogram is a plain
dict {(group, class, slot): milliseconds} filled by a Python loop over the frames.  Nothing here is shared with the product
(calibration.py, sweep_eval.py, csrc/calibration.hip)."""
import math
from fractions import Fraction

import numpy as np

SLOTS = 65538
BUCKETS = 65537
NAN_SLOT = 65537


def scoring_sets(model, meeting, chan):
    """[INVALID, LAUGH, SPEECH, NOISE, SILENCE] of a channel as boolean arrays over the model's milliseconds, the last four without
    INVALID; five empty sets for a channel without a participant."""
    part = model.chan_to_part.get(meeting, {}).get(chan)
    if part is None:
        return [np.zeros(model.N, bool)] * 5
    inv = model.get(model.invalid, meeting, part)
    silence = model.silence.get(meeting, {}).get(part, np.zeros(model.N, bool))
    return [inv] + [s & ~inv for s in (model.get(model.laugh, meeting, part), model.get(model.speech, meeting, part),
                                       model.get(model.noise, meeting, part), silence)]


def slot_of(p):
    """The slot of one sample (a numpy scalar or a float): widened to float64, > 1 -> 1, <= 0 -> 1e-7, NaN -> 65537."""
    v = float(np.float64(p))
    if math.isnan(v):
        return NAN_SLOT
    if v > 1:
        v = 1.0
    elif v <= 0:
        v = 0.0000001
    return int(math.floor(v * 65536.0))


def frame_ms(j, fps):
    return int(round(float(np.float64(j) / np.float64(fps) * np.float64(1000.0))))      # Python's round: half to even, as rint


def label_histogram(tracks, sets_per_channel, fps, lengths=None, groups=None):
    """{(g, k, slot): ms}, zero entries left out.  sets_per_channel: per channel five boolean arrays; fps: one per channel."""
    hist = {}
    for c, (track, sets) in enumerate(zip(tracks, sets_per_channel)):
        g = c if groups is None else groups[c]
        if g < 0:
            continue
        n = len(track) if lengths is None else lengths[c]
        for i in range(n):
            lo, hi = frame_ms(i, fps[c]), frame_ms(i + 1, fps[c])
            slot = slot_of(track[i])
            for k, s in enumerate(sets):
                w = int(s[lo + 1:hi + 1].sum())                                    # (beyond the universe nobody owns a millisecond)
                if w:
                    hist[(g, k, slot)] = hist.get((g, k, slot), 0) + w
    return hist


def dense(hist, n_groups):
    out = np.zeros((n_groups, 5, SLOTS), np.int64)
    for (g, k, slot), w in hist.items():
        out[g, k, slot] = w
    return out


def coverage_total(s, m_end):
    """F_k(m_n): the milliseconds of a set in (0, m_n]."""
    return int(s[1:m_end + 1].sum())


# ---- figures from the definitions -------------------------------------------------------------------------------------------------
def confidence(u):
    return Fraction(2 * u + 1, 2 * BUCKETS)


def _pos_neg(row):
    row = np.asarray(row)
    pos = {u: int(row[1, u]) for u in range(BUCKETS) if row[1, u]}
    neg = {u: int(row[2, u] + row[3, u] + row[4, u]) for u in range(BUCKETS) if row[2, u] or row[3, u] or row[4, u]}
    return pos, neg


def figures(row, n_bins=15):
    """Exact Fractions (None where there is no denominator) for brier, ece, mce, roc_auc, average_precision; nll_terms: the
    non-negative float terms of the NLL's numerator, for math.fsum."""
    pos, neg = _pos_neg(row)
    P, N = sum(pos.values()), sum(neg.values())
    W = P + N
    out = {"pos_ms": P, "neg_ms": N}
    out["brier"] = None if not W else (sum(w * (1 - confidence(u)) ** 2 for u, w in pos.items())
                                       + sum(w * confidence(u) ** 2 for u, w in neg.items())) / W
    out["nll_terms"] = [-(w * math.log(float(confidence(u)))) for u, w in pos.items()] + \
                       [-(w * math.log1p(-float(confidence(u)))) for u, w in neg.items()]
    # AUC: over all pairs (positive ms, negative ms): 1 if the positive's bucket is higher, 1/2 if equal
    if P and N:
        wins = Fraction(0)
        for u, a in pos.items():
            for v, b in neg.items():
                if u > v:
                    wins += a * b
                elif u == v:
                    wins += Fraction(a * b, 2)
        out["roc_auc"] = wins / (P * N)
    else:
        out["roc_auc"] = None
    # ECE / MCE from the definition
    bins = {}
    for u in set(pos) | set(neg):
        b = u * n_bins // BUCKETS
        ms, laugh, conf = bins.get(b, (0, 0, Fraction(0)))
        w = pos.get(u, 0) + neg.get(u, 0)
        bins[b] = (ms + w, laugh + pos.get(u, 0), conf + w * confidence(u))
    gaps = {b: abs(Fraction(laugh, ms) - conf / ms) for b, (ms, laugh, conf) in bins.items()}
    out["ece"] = None if not W else sum(Fraction(bins[b][0], W) * gaps[b] for b in bins)
    out["mce"] = None if not W else max(gaps.values())
    out["bins"] = bins
    # average precision: thresholds at every bucket, descending
    if P:
        ap = Fraction(0)
        for u in sorted(pos, reverse=True):
            tp = sum(w for v, w in pos.items() if v >= u)
            fp = sum(w for v, w in neg.items() if v >= u)
            ap += Fraction(pos[u], P) * Fraction(tp, tp + fp)
        out["average_precision"] = ap
    else:
        out["average_precision"] = None
    return out


def isotonic(row):
    """Textbook pool-adjacent-violators on Fractions: the non-decreasing sequence closest to the laugh share of the buckets that hold
    mass, in the mass-weighted squared error.  Returns {bucket: Fraction} for the buckets with mass."""
    pos, neg = _pos_neg(row)
    points = [(u, Fraction(pos.get(u, 0), pos.get(u, 0) + neg.get(u, 0)), pos.get(u, 0) + neg.get(u, 0))
              for u in sorted(set(pos) | set(neg))]
    blocks = [[[u], value, mass] for u, value, mass in points]
    changed = True
    while changed:                                             # merge any adjacent pair that violates the order, until none does
        changed = False
        for j in range(len(blocks) - 1):
            if blocks[j][1] > blocks[j + 1][1]:
                a, b = blocks[j], blocks[j + 1]
                mass = a[2] + b[2]
                blocks[j:j + 2] = [[a[0] + b[0], (a[1] * a[2] + b[1] * b[2]) / mass, mass]]
                changed = True
                break
    return {u: value for members, value, _ in blocks for u in members}


def brier_of_table(row, table):
    """The Brier score of the row under a table (a sequence of 65537 numbers), in Fractions."""
    pos, neg = _pos_neg(row)
    W = sum(pos.values()) + sum(neg.values())
    return (sum(w * (1 - Fraction(table[u])) ** 2 for u, w in pos.items()) + sum(w * Fraction(table[u]) ** 2 for u, w in neg.items())) / W
