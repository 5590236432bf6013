"""Second implementation of the pair convention, written from the text above lad_bootstrap_pair_quantiles in include/lad_hip.h and
not from bootstrap.py or the kernel: fractions.Fraction and sorted.  Also the hand-built rows that the CPU and the GPU tests share:
exact ties, and near ties at the bound of the contract that only a full 256-bit comparison orders."""
from fractions import Fraction
from math import gcd

from _bootstrap_model import rank, replicate_pair

DIFFERENCE, HARMONIC = 0, 1


def value(op, n1, d1, n2, d2):
    """The exact value of a valid replicate."""
    p, r = Fraction(n1, d1), Fraction(n2, d2)
    if op == DIFFERENCE:
        return p - r
    assert op == HARMONIC
    return Fraction(0) if p + r == 0 else 2 * p * r / (p + r)


def pair_quantiles(s, pairs, qs, key=None):
    """s [B][M]; pairs: 13 integers each; qs [(q_num, q_den)] -> (out [P][Q] of (n1, d1, n2, d2), valid [P], signs [P] of
    [below, at, above 0]).  key: another sort key of (op, n1, d1, n2, d2) in place of the exact value (a deliberately wrong one)."""
    out, valid, signs = [], [], []
    for pair in pairs:
        op, one, two = pair[0], tuple(pair[1:7]), tuple(pair[7:13])
        kept = []
        for b, row in enumerate(s):
            p, r = replicate_pair(row, one), replicate_pair(row, two)
            if p is not None and r is not None:
                kept.append(((key or value)(op, *p, *r), b, p + r))
        kept.sort(key=lambda t: (t[0], t[1]))
        valid.append(len(kept))
        exact = [value(op, *e) for _, _, e in kept]
        signs.append([sum(v < 0 for v in exact), sum(v == 0 for v in exact), sum(v > 0 for v in exact)])
        out.append([kept[rank(qn, qd, len(kept))][2] if kept else (-1, -1, -1, -1) for qn, qd in qs])
    return out, valid, signs


def number(op, entry):
    """What is reported for an entry: one conversion of the exact value."""
    return float("nan") if tuple(entry) == (-1, -1, -1, -1) else float(value(op, *entry))


# ---- two deliberately short comparisons -----------------------------------------------------------------------------------------
def _magnitudes(op, n1, d1, n2, d2):
    if op == DIFFERENCE:
        return n1 * d2 - n2 * d1, d1 * d2
    den = n1 * d2 + n2 * d1
    return (2 * n1 * n2, den) if den else (0, 1)


def float_key(op, n1, d1, n2, d2):
    """The value through float64."""
    if op == DIFFERENCE:
        return n1 / d1 - n2 / d2
    num, den = _magnitudes(op, n1, d1, n2, d2)
    return float(num) / float(den)


class High128:
    """A value whose order keeps only the high 128 bits of the two 256-bit cross products."""

    def __init__(self, op, n1, d1, n2, d2):
        self.num, self.den = _magnitudes(op, n1, d1, n2, d2)

    def _cmp(self, other):
        sign, other_sign = (self.num > 0) - (self.num < 0), (other.num > 0) - (other.num < 0)
        if sign != other_sign:
            return -1 if sign < other_sign else 1
        left, right = (abs(self.num) * other.den) >> 128, (abs(other.num) * self.den) >> 128
        return 0 if left == right else (-1 if (left < right) == (sign > 0) else 1)

    def __lt__(self, other):
        return self._cmp(other) < 0

    def __eq__(self, other):
        return self._cmp(other) == 0


# ---- hand-built rows --------------------------------------------------------------------------------------------------------------
# Both over a sums matrix of four columns (n1, d1, n2, d2), read by the figures (0, 1, 1, -1, -1, 0) and (2, 1, 3, -1, -1, 0).
PLAIN_PAIRS = [(op, 0, 1, 1, -1, -1, 0, 2, 1, 3, -1, -1, 0) for op in (DIFFERENCE, HARMONIC)]
SWAPPED_PAIRS = [(op, 2, 1, 3, -1, -1, 0, 0, 1, 1, -1, -1, 0) for op in (DIFFERENCE, HARMONIC)]        # B - A: the order reversed


def tie_rows():
    """Eight replicates of two values, each value once as (n1, d1, n2, d2) and three times as a multiple of that: equal values,
    so the order within a value is the replicate number.  The multiples come first."""
    a, b = (3, 7, 2, 5), (1, 4, 1, 6)                                                # 3/7 - 2/5 = 1/35 < 1/4 - 1/6 = 1/12
    return [[2 * v for v in b], [2 * v for v in a], list(a), list(b), [6 * v for v in a], [4 * v for v in b], [3 * v for v in b],
            [5 * v for v in a]]


def near_tie_rows():
    """Two replicates X and Y whose integers all lie in [2^53, 2^54) and whose differences X > Y are exactly 1 / (d1 d2 d1' d2')
    apart, X first: N_X D_Y - N_Y D_X = 1.  The four denominators are pairwise coprime odd numbers just below 2^54; N_X is the
    inverse of D_Y modulo D_X, less a whole multiple t of D_X (a shift by t moves both values by the integer t), and
    n1 d2 - n2 d1 = N is solved for n1 modulo d1.  The first set of denominators below 2^54 whose numerators are all in range."""
    top = 1 << 54

    def split(N, a, b):
        """(n1, n2) with n1 * b - n2 * a == N, both in [2^53, 2^54), or None."""
        n1 = N * pow(b, -1, a) % a
        n2, rest = divmod(n1 * b - N, a)
        assert rest == 0
        return (n1, n2) if top // 2 <= n1 < top and top // 2 <= n2 < top else None
    for start in range(1, 20001, 2):
        dens, k = [], start
        while len(dens) < 4:
            if all(gcd(top - k, d) == 1 for d in dens):
                dens.append(top - k)
            k += 2
        d1, d2, e1, e2 = dens
        DX, DY = d1 * d2, e1 * e2
        NX = pow(DY, -1, DX)
        NY = (NX * DY - 1) // DX
        assert NX * DY - NY * DX == 1
        for t in (-1, 0, 1, 2):                                                    # X - t and Y - t: the same distance
            x, y = split(NX - t * DX, d1, d2), split(NY - t * DY, e1, e2)
            if x and y:
                return [[x[0], d1, x[1], d2], [y[0], e1, y[1], e2]]
    raise AssertionError("no near tie in range")
