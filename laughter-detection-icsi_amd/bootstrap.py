"""Percentile bootstrap over recording units: resample weights, weighted integer sums, exact quantiles of ratios of sums.

Not in the reference, whose analysis/analyse.py writes point figures only.  The convention stands in include/lad_hip.h above
lad_bootstrap_weights (the Philox counter of a draw, the contract of the sums, the six integers of a figure, the order of two
fractions, the rank of a quantile); tests/_bootstrap_model.py is a second implementation of it.

    weights_host / weights_device      int32 (B, G): how often each of G units occurs in replicate b, a pure function of (seed, b, G)
    sums_host / sums_device            int64 (B, M) = weights @ x for x int64 (G, M), 0 <= x < 2^40
    select_host / quantiles_device     per figure the (num, den) pairs at the ranks of the quantiles, and the number of valid replicates
    intervals_host / intervals_device  the three steps for a matrix of cells (a few columns per cell and one shared last column),
                                       the device form in chunks of cells so that no sums buffer exceeds SUMS_BYTES_CAP
    pair_select_host / pair_quantiles_device    per pair of figures (their difference, or their harmonic mean) the (n1, d1, n2, d2) at
                                       the ranks of the quantiles, the valid replicates and how many lie below, at and above 0
    pair_intervals_host / pair_intervals_device the same three steps for the cells of two systems under one set of resamples

The host forms are numpy and Python integers and never produce a float; the device forms are csrc/bootstrap.hip and have no CPU
fallback.  Both return the same integers.  sweep_eval.bootstrap_sum_stats_host / _device build the rows from them.
"""
import ctypes
from fractions import Fraction

import numpy as np

TAG = 0x424F4F54               # counter word 3 of a draw ("BOOT")
MAX_UNITS = 4096               # include/lad_hip.h: lad_bootstrap_max_units()
MAX_REPLICATES = 4096          # ... lad_bootstrap_max_replicates()
MAX_VALUE = 1 << 40            # the contract of lad_bootstrap_sums: 0 <= x < 2^40
SUMS_BYTES_CAP = 1 << 30       # intervals_device: no sums buffer is larger than this
SHARED = -1                    # in a cell's figure template: the matrix's last column (shared by all cells)
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint64 arrays that hold 32-bit words (csrc/lad_philox.h) -> four such arrays."""
    c0, c1, c2, c3 = (np.asarray(v, np.uint64) & _M32 for v in (c0, c1, c2, c3))
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2           # 32 x 32 -> 64: no overflow
        c0, c1, c2, c3 = ((p1 >> s32) ^ c1 ^ k0) & _M32, p1 & _M32, ((p0 >> s32) ^ c3 ^ k1) & _M32, p0 & _M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def _check_sizes(G, B):
    if not 1 <= G <= MAX_UNITS or not 1 <= B <= MAX_REPLICATES:
        raise ValueError(f"units 1..{MAX_UNITS} and replicates 1..{MAX_REPLICATES}, got {G} and {B}")


def weights_host(G, B, seed):
    """int32 (B, G): draw i of replicate b is word i & 3 of philox4x32_10((i >> 2, b, 0, TAG), (seed lo, seed hi)), its unit
    (word * G) >> 32.  Every row sums to G."""
    _check_sizes(G, B)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    calls = (G + 3) // 4
    c0 = np.broadcast_to(np.arange(calls, dtype=np.uint64)[None, :], (B, calls))
    c1 = np.broadcast_to(np.arange(B, dtype=np.uint64)[:, None], (B, calls))
    words = np.stack(philox4x32_10(c0, c1, np.zeros((B, calls), np.uint64), np.full((B, calls), TAG, np.uint64),
                                   seed & 0xFFFFFFFF, seed >> 32), axis=2).reshape(B, 4 * calls)[:, :G]
    units = ((words * np.uint64(G)) >> np.uint64(32)).astype(np.int64)
    out = np.zeros((B, G), np.int32)
    np.add.at(out, (np.repeat(np.arange(B), G), units.ravel()), 1)
    return out


def check_matrix(x):
    """x as a contiguous int64 (G, M) array inside the contract of lad_bootstrap_sums (ValueError otherwise)."""
    x = np.ascontiguousarray(x, dtype=np.int64)
    if x.ndim != 2 or not 1 <= x.shape[0] <= MAX_UNITS:
        raise ValueError(f"x must be (units, columns) with 1..{MAX_UNITS} units, got {x.shape}")
    if x.size and (int(x.min()) < 0 or int(x.max()) >= MAX_VALUE):
        raise ValueError(f"values of x must lie in 0 .. 2^40 - 1, got {int(x.min())} .. {int(x.max())}")
    return x


def sums_host(x, weights):
    """int64 (B, M) = weights @ x (below 2^52 within the contract: int64 holds every partial sum)."""
    return np.asarray(weights, np.int64) @ np.asarray(x, np.int64)


def quantile_pairs(level):
    """The two quantiles of a central interval of `level` per cent as exact (num, den) pairs: (100 - level) / 200 and 1 - that,
    via Fraction(str(level)) (level 95 -> 1/40 and 39/40; "99.9" -> 1/2000 and 1999/2000)."""
    lo = (100 - Fraction(str(level))) / 200
    if not 0 < lo < Fraction(1, 2):
        raise ValueError(f"level must lie strictly between 0 and 100, got {level}")
    hi = 1 - lo
    if hi.denominator >= 2 ** 31:
        raise ValueError(f"level {level} needs a denominator beyond int32")
    return [(lo.numerator, lo.denominator), (hi.numerator, hi.denominator)]


def rank_of(q_num, q_den, v):
    """max(ceil(q_num * v / q_den) - 1, 0), in integers."""
    return max(-((-q_num * v) // q_den) - 1, 0)


_KEY_SHIFT = 110


def _key(num, den):
    """An integer that orders fractions with 0 < den < 2^54 exactly as their values: floor(num * 2^110 / den).  Two different
    values differ by at least 1 / (den1 * den2) > 2^-108, so their scaled forms differ by more than 4 and the floors keep the
    order; equal values have equal floors."""
    return (num << _KEY_SHIFT) // den


def select_host(sums, figures, quantiles):
    """sums int64 (B, M); figures [(num_col, num_mult, den_col_a, den_col_b, valid_col, empty_is_one)]; quantiles [(num, den)]
    -> (out int64 (F, Q, 2), valid int32 (F,)).  Python integers throughout."""
    sums = np.asarray(sums, np.int64)
    out = np.full((len(figures), len(quantiles), 2), -1, np.int64)
    valid = np.zeros(len(figures), np.int32)
    for f, (num_col, mult, den_a, den_b, valid_col, one) in enumerate(figures):
        num = (sums[:, num_col] * mult).tolist()
        den = (sums[:, den_a] + (sums[:, den_b] if den_b >= 0 else 0)).tolist()
        good = (sums[:, valid_col] != 0).tolist() if valid_col >= 0 else [True] * len(num)
        kept = []
        for b, (n, d, g) in enumerate(zip(num, den, good)):
            if d == 0:
                if not one:
                    continue
                n = d = 1
            if g:
                if d >= 1 << 54:
                    raise ValueError(f"figure {f}: a denominator of {d} is beyond the contract (below 2^54)")
                kept.append((_key(n, d), b, n, d))
        kept.sort()                                                                # by the exact value, then the replicate
        valid[f] = len(kept)
        if kept:
            for j, (qn, qd) in enumerate(quantiles):
                out[f, j] = kept[rank_of(qn, qd, len(kept))][2:]
    return out, valid


def weights_device(G, B, seed, device="cuda"):
    """weights_host on the GPU (lad_bootstrap_weights): int32 (B, G) tensor."""
    import torch

    import _hip
    _check_sizes(G, B)
    device = torch.device(device)
    if device.type != "cuda":
        raise _hip.LadHipError("the bootstrap's device form has no CPU fallback")
    with torch.cuda.device(device):
        w = torch.empty((B, G), dtype=torch.int32, device=device)
        _hip.launch("lad_bootstrap_weights", G, B, int(seed) & 0xFFFFFFFFFFFFFFFF, w)
    return w


def sums_device(x, weights):
    """x int64 (G, M) and weights int32 (B, G), both GPU tensors -> int64 (B, M) tensor (lad_bootstrap_sums).  The caller has
    checked the contract (check_matrix) where x was still on the host."""
    import torch

    import _hip
    _hip.require_cuda(x, "x", torch.int64)
    _hip.require_cuda(weights, "weights", torch.int32)
    (G, M), B = x.shape, weights.shape[0]
    if weights.shape != (B, G):
        raise ValueError(f"weights {tuple(weights.shape)} for {G} units")
    with torch.cuda.device(x.device):
        sums = torch.empty((B, M), dtype=torch.int64, device=x.device)
        _hip.launch("lad_bootstrap_sums", x, weights, G, M, B, sums)
    return sums


def quantiles_device(sums, figures, quantiles):
    """select_host for sums in GPU memory (lad_bootstrap_quantiles): only out and valid cross to the host."""
    import torch

    import _hip
    _hip.require_cuda(sums, "sums", torch.int64)
    B, M = sums.shape
    figures_host = np.ascontiguousarray(np.asarray(figures, np.int32).reshape(-1, 6))
    F, Q = len(figures_host), len(quantiles)
    with torch.cuda.device(sums.device):
        fig = torch.from_numpy(figures_host if F else np.zeros((1, 6), np.int32)).to(sums.device)
        out = torch.empty((max(F, 1), Q, 2), dtype=torch.int64, device=sums.device)
        valid = torch.empty((max(F, 1),), dtype=torch.int32, device=sums.device)
        q_num, q_den = ((ctypes.c_int32 * Q)(*[q[i] for q in quantiles]) for i in (0, 1))
        _hip.launch("lad_bootstrap_quantiles", sums, M, B, fig, figures_host, F, q_num, q_den, Q, out, valid)
        return out[:F].cpu().numpy(), valid[:F].cpu().numpy()


def cell_figures(template, cell, per_cell, shared_col):
    """The figures of one cell from its template: a template column c >= 0 is column cell * per_cell + c, SHARED is shared_col;
    -1 in den_col_b / valid_col ("none") is written as None in the template."""
    def col(c):
        return -1 if c is None else shared_col if c == SHARED else cell * per_cell + c
    return [(col(n), mult, col(a), col(b), col(v), one) for n, mult, a, b, v, one in template]


def _split(x, per_cell):
    n_cells, rest = divmod(x.shape[1] - 1, per_cell)
    if rest:
        raise ValueError(f"{x.shape[1]} columns are not cells of {per_cell} and one shared column")
    return n_cells


def intervals_host(x, per_cell, template, n_boot, seed, quantiles):
    """x int64 (G, n_cells * per_cell + 1): per cell `per_cell` columns, then one column shared by all cells.  template: the
    figures of a cell (cell_figures).  -> (out int64 (n_cells, len(template), Q, 2), valid int32 (n_cells, len(template)))."""
    x = check_matrix(x)
    n_cells = _split(x, per_cell)
    sums = sums_host(x, weights_host(x.shape[0], n_boot, seed))
    figures = [f for cell in range(n_cells) for f in cell_figures(template, cell, per_cell, x.shape[1] - 1)]
    out, valid = select_host(sums, figures, quantiles)
    return out.reshape(n_cells, len(template), len(quantiles), 2), valid.reshape(n_cells, len(template))


def intervals_device(x, per_cell, template, n_boot, seed, quantiles, device="cuda", cap=None):
    """intervals_host on the GPU: the matrix is uploaded once, the weights are drawn once, and the cells go through
    lad_bootstrap_sums + lad_bootstrap_quantiles in chunks whose sums buffer (n_boot rows of the chunk's columns and the shared
    one, int64) stays within `cap` bytes (default SUMS_BYTES_CAP; at least one cell a chunk).  Equal to intervals_host whatever the
    chunk size."""
    import torch
    x = check_matrix(x)
    n_cells = _split(x, per_cell)
    cap = SUMS_BYTES_CAP if cap is None else cap
    step = max(1, (cap // (8 * n_boot) - 1) // per_cell)
    weights = weights_device(x.shape[0], n_boot, seed, device)
    xd = torch.from_numpy(x).to(weights.device)
    outs, valids = [], []
    for c0 in range(0, n_cells, step):
        n = min(step, n_cells - c0)
        chunk = torch.cat([xd[:, c0 * per_cell:(c0 + n) * per_cell], xd[:, -1:]], dim=1).contiguous()
        figures = [f for cell in range(n) for f in cell_figures(template, cell, per_cell, n * per_cell)]
        out, valid = quantiles_device(sums_device(chunk, weights), figures, quantiles)
        outs.append(out)
        valids.append(valid)
    Q = len(quantiles)
    out = np.concatenate(outs) if outs else np.zeros((0, Q, 2), np.int64)
    valid = np.concatenate(valids) if valids else np.zeros(0, np.int32)
    return out.reshape(n_cells, len(template), Q, 2), valid.reshape(n_cells, len(template))


# ---- pairs of figures: the difference of two systems and the harmonic mean of two figures (lad_bootstrap_pair_quantiles) --------------
DIFFERENCE, HARMONIC = 0, 1    # the op of a pair
_PAIR_KEY_SHIFT = 220


def pair_fraction(op, n1, d1, n2, d2):
    """The value of a pair as Python integers (N, D), D > 0: op 0 n1 / d1 - n2 / d2 = (n1 d2 - n2 d1) / (d1 d2); op 1 the harmonic
    mean 2 n1 n2 / (n1 d2 + n2 d1), 0 / 1 where that denominator is 0."""
    n1, d1, n2, d2 = int(n1), int(d1), int(n2), int(d2)
    if op == DIFFERENCE:
        return n1 * d2 - n2 * d1, d1 * d2
    if op != HARMONIC:
        raise ValueError(f"op is {DIFFERENCE} (difference) or {HARMONIC} (harmonic mean), got {op}")
    den = n1 * d2 + n2 * d1
    return (2 * n1 * n2, den) if den else (0, 1)


def pair_value(op, entry):
    """The reported number of one entry (n1, d1, n2, d2) of pair_select_host / pair_quantiles_device: one correctly rounded
    conversion of the exact fraction (Python's int / int); NaN for the all -1 entry of an empty order."""
    if int(entry[1]) < 0:
        return float("nan")
    num, den = pair_fraction(op, *entry)
    return num / den


def _replicate_fractions(sums, figure, f):
    """Per replicate the (n, d) of a six-integer figure after the substitution, None where the replicate is invalid."""
    num_col, mult, den_a, den_b, valid_col, one = figure
    num = (sums[:, num_col] * mult).tolist()
    den = (sums[:, den_a] + (sums[:, den_b] if den_b >= 0 else 0)).tolist()
    good = (sums[:, valid_col] != 0).tolist() if valid_col >= 0 else [True] * len(num)
    out = []
    for n, d, g in zip(num, den, good):
        if d == 0:
            n, d, g = (1, 1, g) if one else (0, 0, False)
        if g and d >= 1 << 54:
            raise ValueError(f"pair {f}: a denominator of {d} is beyond the contract (below 2^54)")
        out.append((n, d) if g else None)
    return out


def pair_select_host(sums, pairs, quantiles):
    """sums int64 (B, M); pairs [(op, figure1, figure2)] or 13 integers each, the figures as select_host takes them; quantiles
    [(num, den)] -> (out int64 (P, Q, 4) of (n1, d1, n2, d2), valid int32 (P,), signs int32 (P, 3)).  Python integers throughout:
    the order is that of floor(N * 2^220 / D), which is the order of the values (two different ones, with D below 2^109, differ by
    more than 2^-218) and equal for equal values; then the replicate number."""
    sums = np.asarray(sums, np.int64)
    pairs = np.asarray([_flat_pair(p) for p in pairs], np.int64).reshape(-1, 13).tolist()
    out = np.full((len(pairs), len(quantiles), 4), -1, np.int64)
    valid = np.zeros(len(pairs), np.int32)
    signs = np.zeros((len(pairs), 3), np.int32)
    for f, pair in enumerate(pairs):
        op = pair[0]
        kept = []
        for b, (one, two) in enumerate(zip(_replicate_fractions(sums, pair[1:7], f), _replicate_fractions(sums, pair[7:13], f))):
            if one is not None and two is not None:
                num, den = pair_fraction(op, *one, *two)
                kept.append(((num << _PAIR_KEY_SHIFT) // den, b, one + two))
                signs[f, 1 + (num > 0) - (num < 0)] += 1
        kept.sort()
        valid[f] = len(kept)
        if kept:
            for j, (qn, qd) in enumerate(quantiles):
                out[f, j] = kept[rank_of(qn, qd, len(kept))][2]
    return out, valid, signs


def _flat_pair(pair):
    """(op, figure1, figure2) or the 13 integers themselves -> the 13 integers."""
    pair = list(pair)
    return [pair[0], *pair[1], *pair[2]] if len(pair) == 3 else pair


def pair_quantiles_device(sums, pairs, quantiles):
    """pair_select_host for sums in GPU memory (lad_bootstrap_pair_quantiles): only out, valid and signs cross to the host."""
    import torch

    import _hip
    _hip.require_cuda(sums, "sums", torch.int64)
    B, M = sums.shape
    pairs_host = np.ascontiguousarray(np.asarray([_flat_pair(p) for p in pairs], np.int32).reshape(-1, 13))
    P, Q = len(pairs_host), len(quantiles)
    with torch.cuda.device(sums.device):
        pd = torch.from_numpy(pairs_host if P else np.zeros((1, 13), np.int32)).to(sums.device)
        out = torch.empty((max(P, 1), Q, 4), dtype=torch.int64, device=sums.device)
        valid = torch.empty((max(P, 1),), dtype=torch.int32, device=sums.device)
        signs = torch.empty((max(P, 1), 3), dtype=torch.int32, device=sums.device)
        q_num, q_den = ((ctypes.c_int32 * Q)(*[q[i] for q in quantiles]) for i in (0, 1))
        _hip.launch("lad_bootstrap_pair_quantiles", sums, M, B, pd, pairs_host, P, q_num, q_den, Q, out, valid, signs)
        return out[:P].cpu().numpy(), valid[:P].cpu().numpy(), signs[:P].cpu().numpy()


def pair_cell_figures(template, cell, per_cell, n_cells, shared_col):
    """The pairs of one cell from its template [(op, figure1, figure2)]: a figure is (system, num_col, num_mult, den_col_a,
    den_col_b, valid_col, empty_is_one), system 0 (A) or 1 (B), its columns as cell_figures reads them within that system's cell:
    column c >= 0 is (system * n_cells + cell) * per_cell + c."""
    def figure(fg):
        system, (n, mult, a, b, v, one) = fg[0], fg[1:]

        def col(c):
            return -1 if c is None else shared_col if c == SHARED else (system * n_cells + cell) * per_cell + c
        return (col(n), mult, col(a), col(b), col(v), one)
    return [(op, figure(one), figure(two)) for op, one, two in template]


def _pair_split(x, per_cell, systems, template):
    n_cells, rest = divmod(x.shape[1] - 1, per_cell * systems)
    if systems not in (1, 2) or rest:
        raise ValueError(f"{x.shape[1]} columns are not the cells of {systems} system(s), {per_cell} columns each, and one shared column")
    if any(fg[0] not in range(systems) for _, one, two in template for fg in (one, two)):
        raise ValueError(f"a figure of the template reads a system outside 0..{systems - 1}")
    return n_cells


def pair_intervals_host(x, per_cell, template, n_boot, seed, quantiles, systems=2):
    """x int64 (G, systems * n_cells * per_cell + 1): the cells of system A, then the same cells of system B, then one column shared
    by all (systems=1: one system's cells and the shared column, for pairs of its own figures).  template: the pairs of a cell
    (pair_cell_figures).  The weights are those of intervals_host for this seed: the two systems, and a separate evaluation of
    either, see the same resamples.  -> (out int64 (n_cells, len(template), Q, 4), valid int32 (n_cells, len(template)), signs
    int32 (n_cells, len(template), 3))."""
    x = check_matrix(x)
    n_cells = _pair_split(x, per_cell, systems, template)
    sums = sums_host(x, weights_host(x.shape[0], n_boot, seed))
    pairs = [p for cell in range(n_cells) for p in pair_cell_figures(template, cell, per_cell, n_cells, x.shape[1] - 1)]
    out, valid, signs = pair_select_host(sums, pairs, quantiles)
    T = len(template)
    return out.reshape(n_cells, T, len(quantiles), 4), valid.reshape(n_cells, T), signs.reshape(n_cells, T, 3)


def pair_intervals_device(x, per_cell, template, n_boot, seed, quantiles, systems=2, device="cuda", cap=None):
    """pair_intervals_host on the GPU: the matrix is uploaded once, the weights are drawn once and shared by both systems (that is
    the pairing), and the cells go through lad_bootstrap_sums + lad_bootstrap_pair_quantiles in chunks.  A chunk holds the same
    cells of every system and the shared column, and its sums buffer stays within `cap` bytes (default SUMS_BYTES_CAP; at least
    one cell a chunk).  Equal to pair_intervals_host whatever the chunk size."""
    import torch
    x = check_matrix(x)
    n_cells = _pair_split(x, per_cell, systems, template)
    cap = SUMS_BYTES_CAP if cap is None else cap
    step = max(1, (cap // (8 * n_boot) - 1) // (per_cell * systems))
    weights = weights_device(x.shape[0], n_boot, seed, device)
    xd = torch.from_numpy(x).to(weights.device)
    outs, valids, signs = [], [], []
    for c0 in range(0, n_cells, step):
        n = min(step, n_cells - c0)
        parts = [xd[:, (s * n_cells + c0) * per_cell:(s * n_cells + c0 + n) * per_cell] for s in range(systems)]
        chunk = torch.cat(parts + [xd[:, -1:]], dim=1).contiguous()
        pairs = [p for cell in range(n) for p in pair_cell_figures(template, cell, per_cell, n, systems * n * per_cell)]
        out, valid, sign = pair_quantiles_device(sums_device(chunk, weights), pairs, quantiles)
        outs.append(out)
        valids.append(valid)
        signs.append(sign)
    Q, T = len(quantiles), len(template)
    out = np.concatenate(outs) if outs else np.zeros((0, Q, 4), np.int64)
    valid = np.concatenate(valids) if valids else np.zeros(0, np.int32)
    sign = np.concatenate(signs) if signs else np.zeros((0, 3), np.int32)
    return out.reshape(n_cells, T, Q, 4), valid.reshape(n_cells, T), sign.reshape(n_cells, T, 3)
