"""GPU tests of the paired bootstrap (csrc/bootstrap.hip: lad_bootstrap_pair_quantiles; bootstrap.pair_quantiles_device /
pair_intervals_device; sweep_eval.bootstrap_diff_sum_stats_device and bootstrap_sum_stats_device(event_f1=True); evaluate_sweep.py
--scorer device --compare_probs_dir).

Everything is integers, so every comparison is equality.  The yardsticks are bootstrap.pair_select_host (which
tests/test_bootstrap_pair_cpu.py holds against tests/_bootstrap_pair_model.py) and, for the hand-built rows, that model itself.
Every call goes through the C ABI twice, with guard words behind every output: identical bytes, the guards and the inputs untouched."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _bootstrap_pair_model as pm
import _score_model as sm
import test_bootstrap_pair_cpu as cpu

pytestmark = pytest.mark.gpu

_I32P = ctypes.POINTER(ctypes.c_int32)
GUARD = 7
O_FILL, V_FILL, S_FILL = -79, -80, -81


def _lib():
    import _hip
    return _hip, _hip.lib()


def _pair_quantiles(sums, pairs, qs):
    """sums int64 (B, M) numpy -> (out (P, Q, 4), valid (P,), signs (P, 3)) through lad_bootstrap_pair_quantiles."""
    _hip, lib = _lib()
    sums = np.ascontiguousarray(sums, np.int64)
    B, M = sums.shape
    ph = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 13))
    P, Q = len(ph), len(qs)
    sd, pd = torch.from_numpy(sums).cuda(), torch.from_numpy(ph).cuda()
    s_before, p_before = sd.clone(), pd.clone()
    q_num, q_den = ((ctypes.c_int32 * Q)(*[q[i] for q in qs]) for i in (0, 1))
    outs = []
    for _ in range(2):
        out = torch.full((P * Q * 4 + GUARD,), O_FILL, dtype=torch.int64, device="cuda")
        valid = torch.full((P + GUARD,), V_FILL, dtype=torch.int32, device="cuda")
        signs = torch.full((P * 3 + GUARD,), S_FILL, dtype=torch.int32, device="cuda")
        _hip.check(lib.lad_bootstrap_pair_quantiles(_hip.ptr(sd), M, B, _hip.ptr(pd), ph.ctypes.data_as(_I32P), P, q_num, q_den, Q, _hip.ptr(out),
                                                    _hip.ptr(valid), _hip.ptr(signs), _hip.stream_handle(sd.device)),
                   "lad_bootstrap_pair_quantiles")
        outs.append([t.cpu().numpy() for t in (out, valid, signs)])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*outs))                  # identical bytes on two calls
    out, valid, signs = outs[0]
    assert (out[P * Q * 4:] == O_FILL).all() and (valid[P:] == V_FILL).all() and (signs[P * 3:] == S_FILL).all()
    assert torch.equal(sd, s_before) and torch.equal(pd, p_before)
    return out[:P * Q * 4].reshape(P, Q, 4), valid[:P], signs[:P * 3].reshape(P, 3)


@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, 1000, 4096])
def test_pair_quantiles_are_the_host_forms_on_random_sums(B):
    # 512 lanes a pair, the replicates padded to a power of two with invalid entries: 63 -> 64, 65 -> 128, 1000 -> 1024 (one
    # compare-exchange a lane and stage), 4096 (four a lane, the whole 144 KiB of LDS)
    import bootstrap
    sums = cpu.random_sums(B)
    assert len(cpu.RANDOM_PAIRS) == 16 and len(cpu.QS) == 3
    want = bootstrap.pair_select_host(sums, cpu.RANDOM_PAIRS, cpu.QS)
    for got, w in zip(_pair_quantiles(sums, cpu.RANDOM_PAIRS, cpu.QS), want):
        assert got.dtype == w.dtype and np.array_equal(got, w)
    assert want[1][8] == 0 and want[1][0] == B
    if B == 1000:                                                                  # the wrapper, and one quantile / sixteen
        for qs in ([(1, 2)], [(k, 17) for k in range(1, 17)]):
            got = bootstrap.pair_quantiles_device(torch.from_numpy(sums).cuda(), cpu.RANDOM_PAIRS, qs)
            for g, w in zip(got, bootstrap.pair_select_host(sums, cpu.RANDOM_PAIRS, qs)):
                assert np.array_equal(g, w)


def test_ties_near_ties_and_rows_at_the_bound():
    cpu.check_ties(_pair_quantiles)
    cpu.check_near_ties(_pair_quantiles)
    rng = np.random.default_rng(54)
    top = 2 ** 54 - rng.integers(1, 2 ** 20, (200, 4))
    top[::7] = top[3]
    cpu.check_select(_pair_quantiles, top, pm.PLAIN_PAIRS + pm.SWAPPED_PAIRS)


def test_difference_against_a_zero_figure_is_lad_bootstrap_quantiles():
    import bootstrap
    for B in (64, 333):
        s = cpu.zero_figure_sums(B)
        out, valid, signs = _pair_quantiles(s, [(0, *f, *cpu.ZERO_FIGURE) for f in cpu.ZERO_FIGURES], cpu.QS)
        alone, alone_valid = bootstrap.quantiles_device(torch.from_numpy(s).cuda(), cpu.ZERO_FIGURES, cpu.QS)
        assert np.array_equal(out[:, :, :2], alone) and np.array_equal(valid, alone_valid) and (signs[:, 0] == 0).all()
        assert (out[:, :, 2] == 0).all() and (out[:, :, 3] > 0).all()


def test_refusals_leave_the_outputs_untouched():
    _hip, lib = _lib()
    B, M, P, Q = 6, 7, 2, 2
    st = _hip.stream_handle(torch.device("cuda", torch.cuda.current_device()))
    sums = torch.arange(1, B * M + 1, dtype=torch.int64, device="cuda").reshape(B, M)
    out = torch.full((P * Q * 4 + GUARD,), O_FILL, dtype=torch.int64, device="cuda")
    valid = torch.full((P + GUARD,), V_FILL, dtype=torch.int32, device="cuda")
    signs = torch.full((P * 3 + GUARD,), S_FILL, dtype=torch.int32, device="cuda")
    ph = np.array([[0, 0, 1, 1, -1, -1, 1, 2, 2, 3, 4, 5, 0], [1, 6, 1, 5, -1, 4, 0, 0, 1, 1, -1, -1, 1]], np.int32)
    pd = torch.from_numpy(ph).cuda()
    null = ctypes.c_void_p(0)

    def ptr(t):
        return t if isinstance(t, ctypes.c_void_p) or t is None else _hip.ptr(t)

    def inside(t, offset=0):
        return ctypes.c_void_p(t.data_ptr() + offset)

    def call(s=sums, columns=M, replicates=B, p=pd, p_host=ph, n=P, qn=(1, 39), qd=(40, 40), o=out, v=valid, sg=signs):
        host = None if p_host is None else np.ascontiguousarray(p_host, np.int32).ctypes.data_as(_I32P)
        nq = len(qn)
        return lib.lad_bootstrap_pair_quantiles(ptr(s), columns, replicates, ptr(p), host, n, (ctypes.c_int32 * nq)(*qn),
                                                (ctypes.c_int32 * nq)(*qd), nq, ptr(o), ptr(v), ptr(sg), st)

    def bad_pair(word, value):
        p = ph.copy()
        p[1, word] = value
        return dict(p_host=p)
    cases = [dict(s=null), dict(p=null), dict(p_host=None), dict(o=null), dict(v=null), dict(sg=null),                    # a null pointer
             dict(columns=0), dict(columns=2 ** 32 + 1), dict(replicates=0), dict(replicates=4097), dict(n=-1), dict(n=2 ** 30 + 1),
             dict(qn=(), qd=()), dict(qn=(1,) * 17, qd=(2,) * 17),                                                         # a size
             dict(qn=(0, 1), qd=(40, 40)), dict(qn=(1, 40), qd=(40, 40)), dict(qn=(1, 41), qd=(40, 40)), dict(qn=(-1, 1), qd=(40, 40)),
             dict(qn=(1, 1), qd=(0, 40)),                                                                                  # a quantile
             bad_pair(0, 2), bad_pair(0, -1)]                                                                              # the op
    for side in (1, 7):                                                                                                    # a figure
        cases += [bad_pair(side, -1), bad_pair(side, M), bad_pair(side + 1, 0), bad_pair(side + 1, 3), bad_pair(side + 2, -1),
                  bad_pair(side + 2, M), bad_pair(side + 3, -2), bad_pair(side + 3, M), bad_pair(side + 4, -2), bad_pair(side + 4, M),
                  bad_pair(side + 5, 2), bad_pair(side + 5, -1)]
    cases += [dict(o=inside(sums, 16)), dict(v=inside(sums, 0)), dict(sg=inside(sums, 8)), dict(o=inside(pd, 0)), dict(v=inside(pd, 8)),
              dict(sg=inside(pd, 100)), dict(v=inside(out, 8)), dict(sg=inside(out, 40)), dict(sg=inside(valid, 4)),
              dict(v=inside(signs, 12))]                                                                                   # an overlap
    for kw in cases:
        assert call(**kw) == _hip.LAD_ERR_INVALID and b"lad_bootstrap_pair_quantiles" in lib.lad_last_error(), kw
    torch.cuda.synchronize()
    assert (out == O_FILL).all() and (valid == V_FILL).all() and (signs == S_FILL).all()
    # nothing to do: LAD_OK, nothing launched, nothing written
    assert call(n=0, p=null, p_host=None, o=null, v=null, sg=null) == 0
    torch.cuda.synchronize()
    assert (out == O_FILL).all() and (valid == V_FILL).all() and (signs == S_FILL).all()
    # and the call that all of the above varied is a good one
    assert call() == 0
    torch.cuda.synchronize()
    want, want_valid, want_signs = pm.pair_quantiles(sums.cpu().tolist(), ph.tolist(), [(1, 40), (39, 40)])
    assert out[:P * Q * 4].reshape(P, Q, 4).cpu().tolist() == [[list(e) for e in p] for p in want]
    assert valid[:P].cpu().tolist() == want_valid and signs[:P * 3].reshape(P, 3).cpu().tolist() == want_signs
    assert (out[P * Q * 4:] == O_FILL).all() and (valid[P:] == V_FILL).all() and (signs[P * 3:] == S_FILL).all()


def test_pair_intervals_device_is_the_host_form_whatever_the_chunk(monkeypatch):
    import bootstrap
    import sweep_eval as se
    rng = np.random.default_rng(3)
    G, n_cells, n_boot = 9, 7, 65
    x = rng.integers(0, 2 ** 40, (G, 2 * n_cells * 2 + 1))
    x[:, 2:4] = 0                                                                  # a cell of A without predicted time
    x[1:, -1] = 0                                                                  # transcribed time in one unit: replicates without any
    calls = []
    real = bootstrap.sums_device
    monkeypatch.setattr(bootstrap, "sums_device", lambda x, w: (calls.append(tuple(x.shape)), real(x, w))[1])
    want = bootstrap.pair_intervals_host(x, 2, se._TIME_DIFFS, n_boot, 5, cpu.QS)
    for cap, n_calls in ((None, 1), (1, n_cells), (8 * n_boot * 9, 4)):            # the default; one cell a chunk; two (9 columns)
        del calls[:]
        got = bootstrap.pair_intervals_device(x, 2, se._TIME_DIFFS, n_boot, 5, cpu.QS, cap=cap)
        for g, w in zip(got, want):
            assert g.shape == w.shape and np.array_equal(g, w)
        assert len(calls) == n_calls and all(cap is None or c[1] == 5 or 8 * n_boot * c[1] <= cap for c in calls)
    assert 0 < want[1].min() < n_boot == want[1].max() and len({tuple(v) for v in want[2].reshape(-1, 3).tolist()}) > 2
    # one system: pairs of its own figures
    xe = rng.integers(0, 50, (G, n_cells * 4 + 1))
    want = bootstrap.pair_intervals_host(xe, 4, se._EVENT_F1_PAIR, n_boot, 5, cpu.QS, systems=1)
    for cap in (None, 1):
        for g, w in zip(bootstrap.pair_intervals_device(xe, 4, se._EVENT_F1_PAIR, n_boot, 5, cpu.QS, systems=1, cap=cap), want):
            assert np.array_equal(g, w)
    _hip, _ = _lib()
    with pytest.raises(_hip.LadHipError):
        bootstrap.pair_intervals_device(x, 2, se._TIME_DIFFS, 4, 0, [(1, 2)], device="cpu")
    with pytest.raises(ValueError):
        bootstrap.pair_intervals_device(x[:, 1:], 2, se._TIME_DIFFS, 4, 0, [(1, 2)])


@pytest.mark.parametrize("name", ["plain", "hysteresis", "viterbi"])
def test_diff_rows_of_the_device_form_are_the_host_forms(name):
    import sweep_eval as se
    index, channels = cpu.sweeps()["corpus"]
    thr, kw, (sa, ea), (sb, eb) = cpu.sweeps()[name]
    args, boot = (channels, thr, cpu.MIN_LENGTHS, index), dict(n_boot=cpu.B, seed=cpu.SEED)
    for more in ({}, {"events_a": ea, "events_b": eb}, {"events_a": ea, "events_b": eb, "unit": "meeting", "level": "99.9"}):
        want = se.bootstrap_diff_sum_stats_host(sa, sb, *args, **boot, **kw, **more)
        got = se.bootstrap_diff_sum_stats_device(sa, sb, *args, **boot, **kw, **more)
        for g, w in zip(*((got, want) if more else ([got], [want]))):
            cpu._same(g, w)
    want = se.bootstrap_sum_stats_host(sa, *args, **boot, events=ea, event_f1=True, **kw)
    got = se.bootstrap_sum_stats_device(sa, *args, **boot, events=ea, event_f1=True, **kw)
    for g, w in zip(got, want):
        cpu._same(g, w)
    assert len(got[1][0]) == len(se.columns(se.EVENT_SUM_CI_F1_COLUMNS, se.ls.decoder_for(**{k: kw.get(k) for k in
                                                                                          ("offset_drops", "min_gaps", "penalties")})[0]))


def test_evaluate_sweep_device_scorer_writes_the_host_scorers_bytes(tmp_path):
    import evaluate_sweep
    args = sm.write_corpus(tmp_path) + cpu.write_second_system(tmp_path) + ["--bootstrap", "200", "--bootstrap_seed", "11"]
    for name, extra in (("plain", []), ("events", ["--events", "--bootstrap_event_f1"])):
        written = {}
        for scorer in ("host", "device"):
            out = tmp_path / f"{name}_{scorer}"
            evaluate_sweep.main(args + extra + ["--scorer", scorer, "--out_dir", str(out)])
            written[scorer] = cpu.files(out)
        assert written["host"] == written["device"] and "sum_stats_diff.csv" in written["host"], name
        assert ("event_sum_stats_diff.csv" in written["host"]) == (name == "events")
    assert os.path.exists(tmp_path / "events_device" / "event_sum_stats_ci.csv")
