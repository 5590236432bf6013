"""CPU tests of the paired bootstrap (bootstrap.pair_select_host / pair_intervals_host, sweep_eval.bootstrap_diff_sum_stats_host,
bootstrap_sum_stats_host(event_f1=True), evaluate_sweep.py --compare_probs_dir / --bootstrap_event_f1): the host forms against
tests/_bootstrap_pair_model.py, a second implementation of the convention in include/lad_hip.h in fractions.Fraction.  Integers
and single conversions of exact fractions throughout, so every comparison is equality."""
import os
import shutil
from fractions import Fraction

import numpy as np
import pytest

import _bootstrap_model as model
import _bootstrap_pair_model as pm
import _score_model as sm
from oracle import recipe

QS = [(1, 40), (1, 2), (39, 40)]
# Over eight columns: 0 / 1 a small fraction with many ties, 2 / 3 a large one, 4 a validity column with zeros, 5 a denominator with
# zeros, 6 all zero, 7 positive in every row.  Both ops, both substitutions, a validity column on either side, two-column
# denominators and num_mult 2, a pair without a valid replicate (its validity column is all zero), a figure against itself.
RANDOM_PAIRS = [(0, 0, 1, 1, -1, -1, 0, 2, 1, 3, -1, -1, 0), (1, 0, 1, 1, -1, -1, 0, 2, 1, 3, -1, -1, 0),
                (0, 0, 1, 5, -1, -1, 1, 2, 1, 3, -1, -1, 0), (1, 0, 1, 5, -1, -1, 1, 2, 1, 3, -1, 4, 0),
                (0, 2, 1, 3, -1, 4, 0, 0, 1, 5, -1, -1, 0), (1, 2, 2, 3, 5, 5, 0, 0, 1, 1, -1, -1, 1),
                (0, 0, 2, 1, 5, -1, 1, 2, 2, 3, 1, 4, 1), (1, 6, 1, 5, -1, -1, 0, 6, 1, 7, -1, -1, 0),
                (0, 0, 1, 1, -1, 6, 1, 2, 1, 3, -1, -1, 1), (1, 0, 1, 1, -1, -1, 0, 2, 1, 3, -1, 6, 0),
                (0, 2, 1, 3, -1, -1, 0, 2, 1, 3, -1, -1, 0), (1, 0, 1, 1, -1, -1, 0, 0, 1, 1, -1, -1, 0),
                (0, 6, 1, 7, -1, -1, 0, 0, 1, 1, -1, -1, 0), (1, 6, 1, 7, -1, -1, 0, 6, 1, 5, -1, -1, 1),
                (0, 0, 1, 5, -1, -1, 1, 0, 1, 5, -1, -1, 0), (1, 2, 2, 3, 3, -1, 0, 0, 2, 1, 1, 4, 0)]


def random_sums(B):
    """int64 (B, 8): what RANDOM_PAIRS reads.  Sums below 2^52, so num_mult 2 and two denominator columns stay below 2^54."""
    rng = np.random.default_rng(1000 + B)
    s = rng.integers(0, 2 ** 52, (B, 8))
    s[:, 0], s[:, 1] = s[:, 0] % 5, s[:, 1] % 4 + 1                                # many equal values
    s[:, 3] = np.maximum(s[:, 3], 1)
    s[:, 4] *= rng.random(B) < 0.8
    s[:, 5] *= rng.random(B) < 0.7
    s[:, 6] = 0
    s[:, 7] = s[:, 7] % 9 + 1
    return s


def _same(a, b):
    """Equal rows, NaN matching NaN."""
    assert len(a) == len(b) and len(a) > 0
    for ra, rb in zip(a, b):
        assert len(ra) == len(rb) and all(x == y or (x != x and y != y) for x, y in zip(ra, rb)), (ra, rb)


def check_select(select, sums, pairs, qs=QS):
    """select (pair_select_host, or a device form of it) against the model."""
    out, valid, signs = select(np.asarray(sums, np.int64), pairs, qs)
    want, want_valid, want_signs = pm.pair_quantiles(np.asarray(sums).tolist(), pairs, qs)
    assert valid.tolist() == want_valid and signs.tolist() == want_signs
    assert [[tuple(e) for e in p] for p in out.tolist()] == want
    assert (signs.sum(axis=1) == valid).all()
    return out, valid, signs


@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, 1000])
def test_pair_select_host_is_the_model_on_random_sums(B):
    import bootstrap
    out, valid, _ = check_select(bootstrap.pair_select_host, random_sums(B), RANDOM_PAIRS)
    assert valid[8] == 0 and valid[9] == 0 and (out[8] == -1).all()                # the all-zero validity column: v == 0
    assert valid[0] == B and (valid <= B).all()
    # the two ways of writing a pair are one
    nested = [(p[0], p[1:7], p[7:13]) for p in RANDOM_PAIRS]
    for got, want in zip(bootstrap.pair_select_host(random_sums(B), nested, QS), bootstrap.pair_select_host(random_sums(B), RANDOM_PAIRS, QS)):
        assert np.array_equal(got, want)


def test_a_system_against_itself_and_the_two_systems_swapped():
    import bootstrap
    s = random_sums(257)
    out, valid, signs = bootstrap.pair_select_host(s, [RANDOM_PAIRS[10], RANDOM_PAIRS[14]], QS)
    assert valid[0] == 257 and signs[0].tolist() == [0, 257, 0]
    assert 0 < valid[1] < 257 and signs[1].tolist() == [0, valid[1], 0]           # (invalid where either side is)
    assert all(bootstrap.pair_value(0, e) == 0.0 for e in out.reshape(-1, 4))
    swapped = [(p[0], *p[7:13], *p[1:7]) for p in RANDOM_PAIRS]
    _, valid, signs = bootstrap.pair_select_host(s, RANDOM_PAIRS, QS)
    _, valid_s, signs_s = bootstrap.pair_select_host(s, swapped, QS)
    assert np.array_equal(valid, valid_s)
    for p, (a, b) in zip(RANDOM_PAIRS, zip(signs.tolist(), signs_s.tolist())):
        assert b == (a[::-1] if p[0] == 0 else a)                                  # (a harmonic mean does not change)
    assert any(a[0] and a[2] and a[0] != a[2] for a in signs.tolist())


def zero_figure_sums(B):
    """Six columns: 0 / 1 and 2 / (1 + 3) with a validity column 3 that has zeros, 4 all zero, 5 positive in every row."""
    s = random_sums(B)[:, :6]
    s[:, 3] = s[:, 4]
    s[:, 4] = 0
    s[:, 5] = np.arange(B) % 7 + 1
    return s


ZERO_FIGURES = [(0, 1, 1, -1, -1, 0), (2, 2, 1, 3, 3, 0), (2, 1, 3, -1, -1, 1)]
ZERO_FIGURE = (4, 1, 5, -1, -1, 0)                                                 # constantly 0 / d


def test_difference_against_a_zero_figure_is_the_figure_alone():
    import bootstrap
    for B in (1, 64, 333):
        s = zero_figure_sums(B)
        out, valid, signs = bootstrap.pair_select_host(s, [(0, f, ZERO_FIGURE) for f in ZERO_FIGURES], QS)
        alone, alone_valid = bootstrap.select_host(s, ZERO_FIGURES, QS)
        assert np.array_equal(out[:, :, :2], alone) and np.array_equal(valid, alone_valid)
        assert (signs[:, 0] == 0).all()
        assert B == 1 or 0 < valid[1] < B


def check_ties(select):
    rows = pm.tie_rows()
    qs = [(r, 8) for r in range(1, 8)] + [(15, 16)]                                # the ranks 0 .. 7
    out, valid, _ = check_select(select, rows, pm.PLAIN_PAIRS + pm.SWAPPED_PAIRS, qs)
    assert valid.tolist() == [8] * 4
    low, high = [1, 2, 4, 7], [0, 3, 5, 6]                                         # the replicates of 1/35, and of 1/12: in their own order
    assert out[0].tolist() == [rows[b] for b in low + high]
    assert out[2].tolist() == [rows[b][2:] + rows[b][:2] for b in high + low]      # B - A: the values reversed, not the replicates
    h = [pm.value(1, *rows[b]) for b in range(8)]
    assert len(set(h)) == 2 and out[1].tolist() == [rows[b] for b in sorted(range(8), key=lambda b: (h[b], b))]


def check_near_ties(select):
    """Two differences one unit of 1 / (d1 d2 d1' d2') apart, all eight integers in [2^53, 2^54)."""
    x, y = pm.near_tie_rows()
    assert all(2 ** 53 <= v < 2 ** 54 for v in x + y)
    assert pm.value(0, *x) - pm.value(0, *y) == Fraction(1, x[1] * x[3] * y[1] * y[3])
    rows = [x, y, x, y, y]                                                         # ascending: y (1, 3, 4), then x (0, 2)
    qs = [(r, 5) for r in range(1, 5)] + [(9, 10)]
    out, valid, signs = check_select(select, rows, pm.PLAIN_PAIRS[:1] + pm.SWAPPED_PAIRS[:1], qs)
    assert out[0].tolist() == [y, y, y, x, x] and signs[0].tolist() == [0, 0, 5]
    assert out[1].tolist() == [v[2:] + v[:2] for v in (x, x, y, y, y)] and signs[1].tolist() == [5, 0, 0]
    return rows, qs


def test_ties_go_by_the_replicate_number():
    import bootstrap
    check_ties(bootstrap.pair_select_host)


def test_near_ties_at_the_bound_need_all_256_bits():
    import bootstrap
    rows, qs = check_near_ties(bootstrap.pair_select_host)
    want = pm.pair_quantiles(rows, pm.PLAIN_PAIRS[:1], qs)[0]
    # a comparison that keeps the high 128 bits of the products, or goes through float64, calls the two values equal and leaves
    # the replicates in their own order: it fails this very check
    for short in (pm.High128, pm.float_key):
        got = pm.pair_quantiles(rows, pm.PLAIN_PAIRS[:1], qs, key=short)[0]
        assert got != want and got[0] == [tuple(r) for r in rows]
    # and random rows at the bound, both ops: every n and d in [2^54 - 2^20, 2^54)
    rng = np.random.default_rng(54)
    top = 2 ** 54 - rng.integers(1, 2 ** 20, (200, 4))
    top[::7] = top[3]                                                              # some exact ties among them
    check_select(bootstrap.pair_select_host, top, pm.PLAIN_PAIRS + pm.SWAPPED_PAIRS)
    with pytest.raises(ValueError):
        bootstrap.pair_select_host(np.array([[1, 2 ** 54, 1, 2]]), pm.PLAIN_PAIRS, QS)
    with pytest.raises(ValueError):
        bootstrap.pair_select_host(np.array([[1, 2, 1, 2]]), [(2,) + pm.PLAIN_PAIRS[0][1:]], QS)


def test_pair_value_is_one_conversion_of_the_exact_fraction():
    import bootstrap
    rng = np.random.default_rng(7)
    for e in rng.integers(1, 2 ** 54, (200, 4)).tolist() + [[0, 5, 0, 7], [1, 1, 1, 1], [0, 3, 2, 3]]:
        for op in (0, 1):
            assert bootstrap.pair_value(op, e) == pm.number(op, e)
    assert bootstrap.pair_value(1, [0, 5, 0, 7]) == 0.0
    assert all(v != v for v in (bootstrap.pair_value(0, [-1] * 4), bootstrap.pair_value(1, np.full(4, -1))))


def test_entry_point_refuses_without_a_gpu():
    import ctypes

    import _hip
    import bootstrap
    if not os.path.exists(_hip.LIB_PATH):
        import importlib.util
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        spec = importlib.util.spec_from_file_location("lad_build", os.path.join(root, "laughter-detection-icsi_amd", "build.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.build(verbose=False)
    lib = _hip.lib()
    null, one, two = ctypes.c_void_p(0), (ctypes.c_int32 * 1)(1), (ctypes.c_int32 * 1)(2)
    assert lib.lad_bootstrap_pair_quantiles(null, 4, 4, null, None, 1, one, two, 1, null, null, null, null) == _hip.LAD_ERR_INVALID
    assert b"lad_bootstrap_pair_quantiles" in lib.lad_last_error()
    assert lib.lad_bootstrap_pair_quantiles(null, 4, 4097, null, None, 0, one, two, 1, null, null, null, null) == _hip.LAD_ERR_INVALID
    with pytest.raises(_hip.LadHipError):
        bootstrap.pair_intervals_device(np.ones((3, 5), np.int64), 2, [], 4, 0, [(1, 2)], device="cpu")


# ---- the rows of two systems --------------------------------------------------------------------------------------------------------
THRESHOLDS, MIN_LENGTHS, B, SEED = [0.3, 0.5, 0.7], [0.0, 0.2], 48, 9


def corpus():
    """Six channels with a participant in three meetings and one without, tracks of 3,000 frames for two systems: B's track is
    A's with a fifth of another track mixed in, so the two are close and their errors correlated."""
    import sweep_eval as se
    parts = {"Bmr001": ["fe001", "me002", "me003"], "Bed002": ["mn003", "fn004"], "Bro003": ["me010"]}
    rows, chans, channels = [], [], []
    for i, (m, ps) in enumerate(sorted(parts.items())):
        rows += sm.make_rows(20 + i, m, ps, 30.0, n_per_type=12)
        for j, p in enumerate(ps):
            chans.append({"meeting_id": m, "part_id": p, "chan": f"chan{j}", "length": 30.0 - j})
            channels.append((m, f"chan{j}"))
    chans.append({"meeting_id": "Bro003", "part_id": "", "chan": "chan9", "length": 30.0})
    channels.insert(2, ("Bro003", "chan9"))
    part_chan = {(c["meeting_id"], c["part_id"]): c["chan"] for c in chans}
    rows = [dict(r, chan=part_chan[(r["meeting_id"], r["part_id"])]) for r in rows]
    tracks_a = [recipe.make_prob_track(40 + c, 3000) for c in range(len(channels))]
    tracks_b = [0.8 * t + 0.2 * recipe.make_prob_track(90 + c, 3000) for c, t in enumerate(tracks_a)]
    return se.TranscriptIndex(rows, chans), channels, tracks_a, tracks_b


_SWEEPS = {}


def sweeps():
    """The corpus scored once for both systems: {name: (thresholds, decoder keywords, (scores, events) of A, of B)}."""
    import sweep_eval as se
    if not _SWEEPS:
        index, channels, tracks_a, tracks_b = corpus()
        for name, thr, kw in (("plain", THRESHOLDS, {}), ("hysteresis", THRESHOLDS, {"offset_drops": [0.0, 0.1], "min_gaps": [0.05]}),
                              ("viterbi", THRESHOLDS[:2], {"penalties": [0.0, 2.0]})):
            both = [se.score_sweep_host(t, channels, thr, MIN_LENGTHS, 100.0, index, events=(1, 0), **kw) for t in (tracks_a, tracks_b)]
            _SWEEPS[name] = (thr, kw, both[0], both[1])
        _SWEEPS["corpus"] = (index, channels)
    return _SWEEPS


def direct_rows(scores_a, scores_b, fields, per_system, channels, index, unit, level=95):
    """The rows of one table straight from weights_host and Fractions.  scores_*: (C, n_cells, 7) arrays in calc_sum_stats' row order;
    fields(scores) -> (C, n_cells, k) integers; per_system(cell sums (k,), transcribed) -> the figures as Fraction or None."""
    import bootstrap
    import sweep_eval as se
    unit_of, transc = se.bootstrap_units(channels, index, unit)
    G = len(transc)
    w = bootstrap.weights_host(G, B, SEED).tolist()
    assert w == model.weights(G, B, SEED)
    qs = model.level_quantiles(level)
    nan = float("nan")
    rows = []
    per_unit = []
    for s in (scores_a, scores_b):
        f = fields(s)
        per_unit.append([[[sum(int(f[c, j, i]) for c, g in enumerate(unit_of) if g == u) for i in range(f.shape[2])] for u in range(G)]
                         for j in range(f.shape[1])])
    for j in range(len(per_unit[0])):
        plain = [per_system([sum(col) for col in zip(*cells[j])], sum(transc)) for cells in per_unit]
        row, valids = [], []
        for f, (a, b) in enumerate(zip(*plain)):
            reps = []
            for wb in w:
                both = [per_system([sum(wg * u[i] for wg, u in zip(wb, cells[j])) for i in range(len(cells[j][0]))],
                                   sum(wg * t for wg, t in zip(wb, transc)))[f] for cells in per_unit]
                if None not in both:
                    reps.append(both[0] - both[1])
            order = sorted(range(len(reps)), key=lambda r: (reps[r], r))
            lo, hi = (float(reps[order[model.rank(qn, qd, len(reps))]]) if reps else nan for qn, qd in qs)
            row += [nan if a is None else float(a), nan if b is None else float(b), nan if a is None or b is None else float(a - b), lo, hi,
                    sum(r > 0 for r in reps) / len(reps) if reps else nan]
            valids.append(len(reps))
        rows.append(row + [min(valids)])
    return rows


def time_figures(cell, transc):
    pred, corr = cell
    return (Fraction(corr, pred) if pred else Fraction(1), Fraction(corr, transc) if transc else None,
            Fraction(2 * corr, pred + transc) if transc else None)


def event_figures(cell, _):
    n_valid, pred_hit, ref_hit, n_ref = cell
    return (Fraction(pred_hit, n_valid) if n_valid else Fraction(1), Fraction(ref_hit, n_ref) if n_ref else None)


@pytest.mark.parametrize("name,unit", [("plain", "channel"), ("plain", "meeting"), ("hysteresis", "channel"), ("viterbi", "channel")])
def test_diff_rows_are_a_direct_recomputation(name, unit):
    import sweep_eval as se
    index, channels = sweeps()["corpus"]
    thr, kw, (sa, ea), (sb, eb) = sweeps()[name]
    rows, event_rows = se.bootstrap_diff_sum_stats_host(sa, sb, channels, thr, MIN_LENGTHS, index, n_boot=B, seed=SEED, unit=unit, events_a=ea,
                                                        events_b=eb, **kw)
    _same(se.bootstrap_diff_sum_stats_host(sa, sb, channels, thr, MIN_LENGTHS, index, n_boot=B, seed=SEED, unit=unit, **kw), rows)
    decoder = se.ls.decoder_for(**{k: kw.get(k) for k in ("offset_drops", "min_gaps", "penalties")})[0]
    n_keys = len(se.columns(se.SUM_DIFF_COLUMNS, decoder)) - 19
    assert n_keys == 2 + len(decoder.axes) and len(se.SUM_DIFF_COLUMNS) == 21 and len(se.EVENT_SUM_DIFF_COLUMNS) == 15
    assert se.SUM_DIFF_COLUMNS[2:8] == ["precision_a", "precision_b", "precision_diff", "precision_diff_lo", "precision_diff_hi", "precision_gt"]
    # calc_sum_stats' order: its keys are the rows' keys
    stats = se.calc_sum_stats(se.eval_rows(sa, channels, thr, MIN_LENGTHS, index, **kw), **kw)
    assert [r[:n_keys] for r in rows] == [r[:n_keys] for r in stats] == [r[:n_keys] for r in event_rows]
    # the array's cells in that order
    axes = se.ls.decoder_for(**{k: kw.get(k) for k in ("offset_drops", "min_gaps", "penalties")})[1]
    cells = se._cells(thr, MIN_LENGTHS, axes)
    order = sorted(range(len(cells)), key=lambda j: (cells[j][2], cells[j][1], *cells[j][3]))
    C = len(channels)
    flat = [np.asarray(a).reshape(C, len(cells), 7)[:, order] for a in (sa, sb, ea, eb)]
    want = direct_rows(flat[0], flat[1], lambda s: s[:, :, 2:4], time_figures, channels, index, unit)
    _same([r[n_keys:] for r in rows], want)
    joined = [np.concatenate([s, e], axis=2) for s, e in ((flat[0], flat[2]), (flat[1], flat[3]))]
    want = direct_rows(joined[0], joined[1], lambda j: j[:, :, [1, 10, 9, 7]], event_figures, channels, index, unit)
    _same([r[n_keys:] for r in event_rows], want)
    # the point figures are those of the single-system rows; the paired interval is narrower than the two single ones together
    single = se.bootstrap_sum_stats_host(sa, channels, thr, MIN_LENGTHS, index, n_boot=B, seed=SEED, unit=unit, **kw)
    _same([[r[n_keys], r[n_keys + 6], r[n_keys + 12]] for r in rows], [[r[n_keys], r[n_keys + 3], r[n_keys + 6]] for r in single])
    assert all(r[n_keys + 3] <= r[n_keys + 4] for r in rows)


def test_a_system_against_itself_has_no_difference():
    import sweep_eval as se
    index, channels = sweeps()["corpus"]
    thr, kw, (sa, ea), (sb, eb) = sweeps()["plain"]
    rows, event_rows = se.bootstrap_diff_sum_stats_host(sa, sa, channels, thr, MIN_LENGTHS, index, n_boot=B, seed=SEED, events_a=ea, events_b=ea)
    for table, n in ((rows, 3), (event_rows, 2)):
        for r in table:
            for f in range(n):
                a, b, diff, lo, hi, gt = r[2 + 6 * f:8 + 6 * f]
                assert a == b and diff == lo == hi == 0.0 and gt == 0.0
            assert r[-1] == B
    ab = se.bootstrap_diff_sum_stats_host(sa, sb, channels, thr, MIN_LENGTHS, index, n_boot=B, seed=SEED)
    ba = se.bootstrap_diff_sum_stats_host(sb, sa, channels, thr, MIN_LENGTHS, index, n_boot=B, seed=SEED)
    for r, s in zip(ab, ba):
        assert r[-1] == s[-1] and (r[2], r[3], r[4]) == (s[3], s[2], -s[4]) and (r[5], r[6]) == (-s[6], -s[5])
    assert any(r[4] != 0 for r in ab)
    with pytest.raises(ValueError):
        se.bootstrap_diff_sum_stats_host(sa, sb[:-1], channels, thr, MIN_LENGTHS, index, n_boot=B)
    with pytest.raises(ValueError):
        se.bootstrap_diff_sum_stats_host(sa, sb, channels, thr, MIN_LENGTHS, index, n_boot=B, events_a=ea)


def test_event_f1_rows():
    import bootstrap
    import sweep_eval as se
    index, channels = sweeps()["corpus"]
    for name in ("plain", "viterbi"):
        thr, kw, (sa, ea), _ = sweeps()[name]
        args = (sa, channels, thr, MIN_LENGTHS, index)
        before = se.bootstrap_sum_stats_host(*args, n_boot=B, seed=SEED, events=ea, **kw)
        for got, want in zip(se.bootstrap_sum_stats_host(*args, n_boot=B, seed=SEED, events=ea, event_f1=False, **kw), before):
            _same(got, want)
        rows, event_rows = se.bootstrap_sum_stats_host(*args, n_boot=B, seed=SEED, events=ea, event_f1=True, **kw)
        _same(rows, before[0])
        _same([r[:-4] + r[-1:] for r in event_rows], before[1])                    # the default's rows with three columns put in
        stats = se.event_sum_stats(se.event_rows(sa, ea, *args[1:], **kw), **kw)
        n_keys = len(stats[0]) - 12
        assert [r[:n_keys] for r in stats] == [r[:n_keys] for r in event_rows]
        _same([[r[-4]] for r in event_rows], [[s[n_keys + 2]] for s in stats])     # event_sum_stats' event_f1
        assert all(r[-3] <= r[-2] for r in event_rows) and any(r[-3] < r[-4] < r[-2] for r in event_rows)
        # the two ends: the harmonic means of the replicates' precision and recall, from weights_host and Fractions
        unit_of, transc = se.bootstrap_units(channels, index)
        w = bootstrap.weights_host(len(transc), B, SEED).tolist()
        cells = se._cells(thr, MIN_LENGTHS, se.ls.decoder_for(None, None, kw.get("penalties"))[1])
        order = sorted(range(len(cells)), key=lambda j: (cells[j][2], cells[j][1], *cells[j][3]))
        s, e = (np.asarray(a).reshape(len(channels), len(cells), 7) for a in (sa, ea))
        for row, j in zip(event_rows, order):
            units = [[int(x) for x in (s[c, j, 1], e[c, j, 3], e[c, j, 2], e[c, j, 0])] for c, g in enumerate(unit_of) if g >= 0]
            reps = []
            for wb in w:
                p, r = event_figures([sum(wg * u[i] for wg, u in zip(wb, units)) for i in range(4)], None)
                if r is not None:
                    reps.append(Fraction(0) if p + r == 0 else 2 * p * r / (p + r))
            order_r = sorted(range(len(reps)), key=lambda i: (reps[i], i))
            want = [float(reps[order_r[model.rank(qn, qd, len(reps))]]) for qn, qd in model.level_quantiles(95)]
            assert row[-3:-1] == want and row[-1] == len(reps)
    assert se.EVENT_SUM_CI_F1_COLUMNS[-4:] == ["event_f1", "event_f1_lo", "event_f1_hi", "n_boot_valid"]
    with pytest.raises(ValueError):
        se.bootstrap_sum_stats_host(*args, n_boot=B, event_f1=True)


# ---- evaluate_sweep.py ----------------------------------------------------------------------------------------------------------------
def write_second_system(tmp_path):
    """probs_b next to write_corpus' probs: the same channels, every track pulled a fifth of the way towards another one."""
    for m in sorted(os.listdir(tmp_path / "probs")):
        os.makedirs(tmp_path / "probs_b" / m)
        for i, f in enumerate(sorted(os.listdir(tmp_path / "probs" / m))):
            t = np.load(tmp_path / "probs" / m / f)
            np.save(tmp_path / "probs_b" / m / f, (0.8 * t + 0.2 * recipe.make_prob_track(70 + i, len(t))).astype(np.float32))
    return ["--compare_probs_dir", str(tmp_path / "probs_b")]


def files(path):
    return {f: open(path / f, "rb").read() for f in sorted(os.listdir(path))}


def test_evaluate_sweep_compares_two_systems_under_the_host_scorer(tmp_path):
    import csv

    import evaluate_sweep
    import sweep_eval as se
    args = sm.write_corpus(tmp_path)
    compare = write_second_system(tmp_path)
    boot = ["--bootstrap", "16", "--bootstrap_seed", "3"]
    for name, extra, new in (("plain", [], ["sum_stats_diff.csv"]),
                             ("events", ["--events"], ["event_sum_stats_diff.csv", "sum_stats_diff.csv"]),
                             ("lowpass", ["--lowpass", "0.2", "--penalties", "0.0,2.0"], ["sum_stats_diff.csv"])):
        evaluate_sweep.main(args + extra + boot + ["--out_dir", str(tmp_path / name)])
        evaluate_sweep.main(args + extra + boot + compare + ["--out_dir", str(tmp_path / (name + "_diff"))])
        before, after = files(tmp_path / name), files(tmp_path / (name + "_diff"))
        assert sorted(after) == sorted(list(before) + new), name
        assert {k: after[k] for k in before} == before, name                      # every other file, byte for byte
        table = list(csv.reader(open(tmp_path / (name + "_diff") / "sum_stats_diff.csv")))
        ci = list(csv.reader(open(tmp_path / name / "sum_stats_ci.csv")))
        decoder = se.ls.VITERBI if name == "lowpass" else None
        assert table[0] == (se.columns(se.SUM_DIFF_COLUMNS, decoder) if decoder else se.SUM_DIFF_COLUMNS) and len(table) == len(ci)
        n_keys = len(table[0]) - 19
        for r, c in zip(table[1:], ci[1:]):
            assert r[:n_keys] == c[:n_keys] and r[n_keys] == c[n_keys] and r[n_keys + 6] == c[n_keys + 3]     # A's point figures
            assert float(r[n_keys + 3]) <= float(r[n_keys + 4]) and 0 <= float(r[n_keys + 5]) <= 1
    assert list(csv.reader(open(tmp_path / "events_diff" / "event_sum_stats_diff.csv")))[0] == se.EVENT_SUM_DIFF_COLUMNS
    # event F1: three more columns in the one file, every other file as it was
    evaluate_sweep.main(args + ["--events"] + boot + ["--bootstrap_event_f1", "--out_dir", str(tmp_path / "f1")])
    before, after = files(tmp_path / "events"), files(tmp_path / "f1")
    assert sorted(before) == sorted(after)
    assert {k for k in before if before[k] != after[k]} == {"event_sum_stats_ci.csv"}
    f1, plain = (list(csv.reader(open(tmp_path / d / "event_sum_stats_ci.csv"))) for d in ("f1", "events"))
    stats = list(csv.reader(open(tmp_path / "events" / "event_sum_stats.csv")))
    assert f1[0] == se.EVENT_SUM_CI_F1_COLUMNS and [r[:-4] + r[-1:] for r in f1] == plain
    assert [r[-4] for r in f1[1:]] == [s[4] for s in stats[1:]]
    # refusals
    with pytest.raises(SystemExit):
        evaluate_sweep.main(args + compare + ["--out_dir", str(tmp_path / "no_bootstrap")])
    with pytest.raises(SystemExit):
        evaluate_sweep.main(args + boot + ["--bootstrap_event_f1", "--out_dir", str(tmp_path / "no_events")])
    with pytest.raises(SystemExit):
        evaluate_sweep.main(args + ["--events", "--bootstrap_event_f1", "--out_dir", str(tmp_path / "no_bootstrap")])
    shutil.copytree(tmp_path / "probs_b", tmp_path / "probs_c")
    os.remove(tmp_path / "probs_c" / "Bed002" / "chan1.npy")
    with pytest.raises(SystemExit):
        evaluate_sweep.main(args + boot + ["--compare_probs_dir", str(tmp_path / "probs_c"), "--out_dir", str(tmp_path / "mismatch")])
    assert not os.path.exists(tmp_path / "mismatch") and not os.path.exists(tmp_path / "no_bootstrap")
