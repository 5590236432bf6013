"""Second implementation of the bootstrap convention, written from the text above lad_bootstrap_weights in include/lad_hip.h and not
from bootstrap.py or the kernels: Python integers and fractions.Fraction, loops over replicates and draws.  The Philox is the one of
tests/_augment_model.py, which tests/test_augment_cpu.py pins to the known answers."""
import math
from fractions import Fraction

from _augment_model import mulhi, philox4x32_10

TAG = 0x424F4F54


def draw_words(seed, b, call):
    """The four words of call `call` (draws 4 * call .. 4 * call + 3) of replicate b."""
    return philox4x32_10((call, b, 0, TAG), (seed & 0xFFFFFFFF, seed >> 32))


def weights(G, B, seed):
    """[B][G] counts: draw i of replicate b is word i & 3 of call i >> 2, its unit mulhi(word, G)."""
    rows = []
    for b in range(B):
        row = [0] * G
        words = [w for call in range((G + 3) // 4) for w in draw_words(seed, b, call)]
        for i in range(G):
            row[mulhi(words[i], G)] += 1                                           # (words[i]: word i & 3 of call i >> 2)
        rows.append(row)
    return rows


def sums(x, w):
    """x [G][M], w [B][G] -> [B][M], Python integers."""
    M = len(x[0]) if x else 0
    return [[sum(wb[g] * x[g][m] for g in range(len(x))) for m in range(M)] for wb in w]


def replicate_pair(row, figure):
    """(num, den) of one replicate's sums, or None where the replicate is invalid for the figure."""
    num_col, mult, den_a, den_b, valid_col, one = figure
    num = mult * row[num_col]
    den = row[den_a] + (row[den_b] if den_b != -1 else 0)
    if valid_col >= 0 and row[valid_col] == 0:
        return None
    if den == 0:
        return (1, 1) if one else None
    return (num, den)


def rank(q_num, q_den, v):
    return max(math.ceil(Fraction(q_num * v, q_den)) - 1, 0)


def quantiles(s, figures, qs):
    """s [B][M]; figures: six-integer records; qs [(q_num, q_den)] -> (out [F][Q] of (num, den), valid [F])."""
    out, valid = [], []
    for figure in figures:
        pairs = [(replicate_pair(row, figure), b) for b, row in enumerate(s)]
        kept = sorted(((Fraction(*p), b, p) for p, b in pairs if p is not None), key=lambda t: (t[0], t[1]))
        valid.append(len(kept))
        out.append([kept[rank(qn, qd, len(kept))][2] if kept else (-1, -1) for qn, qd in qs])
    return out, valid


def level_quantiles(level):
    lo = (100 - Fraction(str(level))) / 200
    return [(lo.numerator, lo.denominator), ((1 - lo).numerator, (1 - lo).denominator)]


def _value(pair):
    return float("nan") if pair == (-1, -1) else pair[0] / pair[1]


def time_row(cells, transc, w, level):
    """One row behind its keys for one setting: cells [G] of (pred_ms, corr_ms), transc [G] ms, w [B][G] -> precision, lo, hi, recall,
    lo, hi, f1, lo, hi, n_boot_valid."""
    x = [[p, c, t] for (p, c), t in zip(cells, transc)]
    figures = [(1, 1, 0, -1, -1, 1), (1, 1, 2, -1, -1, 0), (1, 2, 0, 2, 2, 0)]
    out, valid = quantiles(sums(x, w), figures, level_quantiles(level))
    pred, corr, tr = (sum(r[i] for r in x) for i in range(3))
    nan = float("nan")
    point = [1.0 if pred == 0 else corr / pred, nan if tr == 0 else corr / tr, nan if tr == 0 else 2 * corr / (pred + tr)]
    row = []
    for p, (lo, hi) in zip(point, out):
        row += [p, _value(lo), _value(hi)]
    return row + [min(valid)], valid


def event_row(cells, w, level):
    """cells [G] of (n_valid, pred_hit, ref_hit, n_ref) -> event_precision, lo, hi, event_recall, lo, hi, n_boot_valid."""
    x = [list(c) for c in cells]
    figures = [(1, 1, 0, -1, -1, 1), (2, 1, 3, -1, -1, 0)]
    out, valid = quantiles(sums(x, w), figures, level_quantiles(level))
    n_valid, pred_hit, ref_hit, n_ref = (sum(r[i] for r in x) for i in range(4))
    nan = float("nan")
    point = [1.0 if n_valid == 0 else pred_hit / n_valid, nan if n_ref == 0 else ref_hit / n_ref]
    row = []
    for p, (lo, hi) in zip(point, out):
        row += [p, _value(lo), _value(hi)]
    return row + [min(valid)]
