"""Second implementation of the two-state Viterbi decoder, written from the text above lad_viterbi_count in include/lad_hip.h: a
per-frame loop in Python integers, and a brute-force maximiser over all 2^T paths for tiny tracks.  Nothing here is shared with
laugh_segmenter.py or csrc/viterbi.hip."""
import math

NAN_SCORE = -2 ** 31
BUCKETS = 65536


def fixed(p):
    """fix_over_underflow on a Python float, NaN kept."""
    if p > 1:
        return 1.0
    if p <= 0:
        return 0.0000001
    return p


def scores(probs, table, bias):
    """s[i] = S[floor(v[i] * 65536)] - bias, -2^31 at a NaN frame: Python ints."""
    out = []
    for p in probs:
        v = fixed(float(p))
        out.append(NAN_SCORE if v != v else int(table[int(math.floor(v * 65536.0))]) - int(bias))
    return out


def decode(s, penalty):
    """The recursion of the header on integer frame scores -> (path as a list of 0 / 1, best)."""
    T = len(s)
    d0, d1 = 0, -penalty
    psi0, psi1 = [], []
    for t in range(T):
        psi0.append(1 if d1 > d0 else 0)
        psi1.append(0 if d0 - penalty > d1 else 1)
        d0, d1 = max(d0, d1), max(d0 - penalty, d1) + s[t]
    state = 1 if d1 > d0 else 0
    best = max(d0, d1)
    path = [0] * T
    for t in range(T - 1, -1, -1):
        path[t] = state
        state = psi1[t] if state else psi0[t]
    return path, best


def path_score(path, s, penalty):
    """Sum of s over the on frames minus `penalty` per frame that is on while its predecessor is off (off before frame 0)."""
    total, prev = 0, 0
    for x, v in zip(path, s):
        if x:
            total += v - (0 if prev else penalty)
        prev = x
    return total


def brute_force(s, penalty):
    """The best score over all 2^T paths (T <= 14)."""
    T = len(s)
    assert T <= 14
    return max(path_score([(bits >> t) & 1 for t in range(T)], s, penalty) for bits in range(1 << T))


def runs(path):
    """Maximal runs of 1 -> [(first_frame, last_frame)]."""
    out, start = [], None
    for i, x in enumerate(path):
        if x and start is None:
            start = i
        if not x and start is not None:
            out.append((start, i - 1))
            start = None
    if start is not None:
        out.append((start, len(path) - 1))
    return out


def spans(probs, table, bias, penalty):
    """[(first_frame, last_frame)] of the decoded path of one track and one setting, and its best score."""
    path, best = decode(scores(probs, table, bias), penalty)
    return runs(path), best


def instances(probs, table, settings, keys, min_lengths, fps):
    """{(*key, min_length): [(start_s, end_s)]}: first / fps, last / fps, kept iff end - start > min_length (Python floats)."""
    out = {}
    for key, (bias, penalty) in zip(keys, settings):
        rs, _ = spans(probs, table, bias, penalty)
        inst = [(a / fps, b / fps) for a, b in rs]
        for min_l in min_lengths:
            out[(*key, min_l)] = [i for i in inst if i[1] - i[0] > min_l]
    return out
