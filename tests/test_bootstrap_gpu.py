"""GPU tests of the bootstrap intervals (csrc/bootstrap.hip: lad_bootstrap_weights / lad_bootstrap_sums / lad_bootstrap_quantiles;
bootstrap.py's device forms; sweep_eval.bootstrap_sum_stats_device; evaluate_sweep.py --scorer device --bootstrap).

Everything is integers, so every comparison is equality.  The yardsticks are tests/_bootstrap_model.py (Python integers and
fractions) and, for the integer product, numpy's int64 matmul.  Every call goes through the C ABI twice, with guard words behind
every output: identical bytes, the guards and the inputs untouched."""
import ctypes

import numpy as np
import pytest
import torch

import _bootstrap_model as model
import _score_model as sm
from oracle import recipe

pytestmark = pytest.mark.gpu

_I32P = ctypes.POINTER(ctypes.c_int32)
GUARD = 7
W_FILL, S_FILL, O_FILL, V_FILL = -77, -78, -79, -80


def _lib():
    import _hip
    return _hip, _hip.lib()


def _weights(G, B, seed):
    _hip, lib = _lib()
    outs = []
    for _ in range(2):
        w = torch.full((B * G + GUARD,), W_FILL, dtype=torch.int32, device="cuda")
        _hip.check(lib.lad_bootstrap_weights(G, B, seed, _hip.ptr(w), _hip.stream_handle(w.device)), "lad_bootstrap_weights")
        outs.append(w.cpu().numpy())
    assert outs[0].tobytes() == outs[1].tobytes() and (outs[0][B * G:] == W_FILL).all()
    return outs[0][:B * G].reshape(B, G)


def _sums(x, w):
    """x int64 (G, M), w int32 (B, G) numpy -> int64 (B, M) through lad_bootstrap_sums."""
    _hip, lib = _lib()
    (G, M), B = x.shape, w.shape[0]
    xd, wd = torch.from_numpy(np.ascontiguousarray(x)).cuda(), torch.from_numpy(np.ascontiguousarray(w)).cuda()
    x_before, w_before = xd.clone(), wd.clone()
    outs = []
    for _ in range(2):
        s = torch.full((B * M + GUARD,), S_FILL, dtype=torch.int64, device="cuda")
        _hip.check(lib.lad_bootstrap_sums(_hip.ptr(xd), _hip.ptr(wd), G, M, B, _hip.ptr(s), _hip.stream_handle(s.device)), "lad_bootstrap_sums")
        outs.append(s.cpu().numpy())
    assert outs[0].tobytes() == outs[1].tobytes() and (outs[0][B * M:] == S_FILL).all()
    assert torch.equal(xd, x_before) and torch.equal(wd, w_before)
    return outs[0][:B * M].reshape(B, M)


def _quantiles(sums, figures, qs):
    """sums int64 (B, M) numpy -> (out [F][Q] of (num, den), valid [F]) through lad_bootstrap_quantiles."""
    _hip, lib = _lib()
    B, M = sums.shape
    fh = np.ascontiguousarray(np.asarray(figures, np.int32).reshape(-1, 6))
    F, Q = len(fh), len(qs)
    sd, fd = torch.from_numpy(np.ascontiguousarray(sums)).cuda(), torch.from_numpy(fh).cuda()
    s_before, f_before = sd.clone(), fd.clone()
    q_num, q_den = ((ctypes.c_int32 * Q)(*[q[i] for q in qs]) for i in (0, 1))
    outs = []
    for _ in range(2):
        out = torch.full((F * Q * 2 + GUARD,), O_FILL, dtype=torch.int64, device="cuda")
        valid = torch.full((F + GUARD,), V_FILL, dtype=torch.int32, device="cuda")
        _hip.check(lib.lad_bootstrap_quantiles(_hip.ptr(sd), M, B, _hip.ptr(fd), fh.ctypes.data_as(_I32P), F, q_num, q_den, Q, _hip.ptr(out),
                                               _hip.ptr(valid), _hip.stream_handle(sd.device)), "lad_bootstrap_quantiles")
        outs.append((out.cpu().numpy(), valid.cpu().numpy()))
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes()
    out, valid = outs[0]
    assert (out[F * Q * 2:] == O_FILL).all() and (valid[F:] == V_FILL).all()
    assert torch.equal(sd, s_before) and torch.equal(fd, f_before)
    return [[tuple(p) for p in f] for f in out[:F * Q * 2].reshape(F, Q, 2).tolist()], valid[:F].tolist()


# ---- weights ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 2, 3, 63, 64, 65, 4096])
def test_weights_are_the_models(G):
    # one workgroup of 256 lanes per replicate, four draws a Philox call: 63 / 64 / 65 units are 16 / 16 / 17 calls, 4096 units
    # four calls a lane and the whole histogram
    for B, seed in ((1, 0), (65, 0xFEDCBA9876543210)):
        got = _weights(G, B, seed)
        assert (got.sum(axis=1) == G).all()
        assert got.tolist() == model.weights(G, B, seed)


def test_weights_of_4096_replicates():
    import bootstrap
    got = _weights(3, 4096, 12345)
    assert got.tolist() == model.weights(3, 4096, 12345)
    assert np.array_equal(got, bootstrap.weights_host(3, 4096, 12345))
    assert np.array_equal(bootstrap.weights_device(450, 2000, 7).cpu().numpy(), bootstrap.weights_host(450, 2000, 7))


# ---- sums ------------------------------------------------------------------------------------------------------------------------
# The tile of sums_kernel: 32 replicates x 512 columns a workgroup (256 lanes, two columns a lane: tid and tid + 256), the weights
# staged 64 units at a time, the rows of x loaded four ahead.  So the edges are B = 32 k, M = 256 (a lane's second column begins)
# and 512 k, G = 4 k and 64 k; the issue's minimum set (G 1 / 63 / 64 / 65, B 1 / 63 / 64 / 65 / 257, M 1 / 255 / 256 / 257 / 1000)
# is in the list as well.
SUM_SHAPES = [(1, 1, 1), (63, 63, 255), (64, 64, 256), (65, 65, 257), (1, 257, 1000), (65, 1, 1000), (64, 257, 1),
              (3, 31, 511), (4, 32, 512), (5, 33, 513), (127, 2, 1025), (128, 33, 3), (129, 65, 600), (63, 64, 1000), (450, 40, 700)]


def _random_weights(rng, B, G, total=4096):
    """Rows of non-negative weights that sum to `total` (the contract's maximum)."""
    cuts = np.sort(rng.integers(0, total + 1, (B, G - 1)), axis=1)
    return np.diff(np.concatenate([np.zeros((B, 1), np.int64), cuts, np.full((B, 1), total)], axis=1), axis=1).astype(np.int32)


@pytest.mark.parametrize("G,B,M", SUM_SHAPES)
def test_sums_are_numpys(G, B, M):
    rng = np.random.default_rng(G * 1000003 + B * 1009 + M)
    x = rng.integers(0, 2 ** 40, (G, M))
    x[rng.random((G, M)) < 0.1] = 2 ** 40 - 1
    w = _random_weights(rng, B, G)
    assert (w.sum(axis=1) == 4096).all() and (w >= 0).all()
    assert np.array_equal(_sums(x, w), w.astype(np.int64) @ x)
    assert np.array_equal(_sums(x, np.ones((B, G), np.int32)), np.broadcast_to(x.sum(axis=0), (B, M)))      # all ones: column sums
    hot = np.zeros((B, G), np.int32)
    hot[np.arange(B), np.arange(B) % G] = 1
    assert np.array_equal(_sums(x, hot), x[np.arange(B) % G])                                                # one-hot rows: rows of x


def test_sums_at_the_bound_of_the_contract():
    G, B, M = 4096, 8, 65
    x = np.full((G, M), 2 ** 40 - 1, np.int64)
    w = np.zeros((B, G), np.int32)
    w[0, 1234] = 4096
    w[1] = 1
    w[2, 0] = w[2, 4095] = 2048
    w[3:, ::2] = 2
    assert (w.sum(axis=1) == 4096).all()
    got = _sums(x, w)
    assert (got == 4096 * (2 ** 40 - 1)).all()                                     # (a 32-bit truncation or a lost high half shows here)
    import bootstrap
    x = np.random.default_rng(1).integers(0, 2 ** 40, (450, 1500))
    wd = bootstrap.weights_device(450, 70, 3)
    assert np.array_equal(bootstrap.sums_device(torch.from_numpy(x).cuda(), wd).cpu().numpy(), bootstrap.sums_host(x, wd.cpu().numpy()))


# ---- quantiles -------------------------------------------------------------------------------------------------------------------
FIGURES = [(0, 1, 1, -1, -1, 1), (0, 1, 1, -1, -1, 0), (0, 2, 1, 2, 2, 0), (3, 1, 2, -1, 1, 1), (4, 1, 5, -1, -1, 0), (5, 2, 4, 5, -1, 1)]
QS = {1: [(1, 2)], 2: [(1, 40), (39, 40)], 5: [(1, 1000), (1, 4), (1, 2), (3, 4), (999, 1000)]}


def _check_quantiles(sums, figures, qs):
    got, valid = _quantiles(sums, figures, qs)
    want, want_valid = model.quantiles(sums.tolist(), figures, qs)
    assert valid == want_valid
    assert got == want
    return got, valid


@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, 1000, 4096])
def test_quantiles_are_the_models_on_random_sums(B):
    # 512 lanes a figure, the replicates padded to a power of two with invalid entries: 63 -> 64, 65 -> 128, 1000 -> 1024 (one
    # compare-exchange a lane and stage), 4096 (four a lane, 80 KiB of LDS)
    rng = np.random.default_rng(B)
    sums = rng.integers(0, 2 ** 52, (B, 6))
    sums[rng.random((B, 6)) < 0.2] = 0                                             # zero denominators, zero validity columns
    sums[:, 3] %= 5                                                                # many equal values
    sums[:, 4] = (sums[:, 4] % 3) * (2 ** 40 + 1)
    sums[:, 5] = (sums[:, 5] % 4 + 1) * (2 ** 41 + 3)
    for Q, qs in QS.items():
        _check_quantiles(sums, FIGURES if Q == 2 else FIGURES[:3], qs)


def test_quantiles_of_ties_invalid_replicates_and_substitutions():
    B = 100
    # all tied: replicate b has the pair (b + 1) / (2 b + 2); rank r is replicate r
    tied = np.array([[b + 1, 2 * b + 2] for b in range(B)], np.int64)
    got, valid = _check_quantiles(tied, [(0, 1, 1, -1, -1, 0)], QS[5])
    assert valid == [B] and got[0] == [(1, 2), (25, 50), (50, 100), (75, 150), (100, 200)]
    # all invalid: a zero denominator without the substitution, and a zero validity column
    zero = np.zeros((B, 3), np.int64)
    zero[:, 0] = 5
    got, valid = _check_quantiles(zero, [(0, 1, 1, -1, -1, 0), (0, 1, 0, -1, 2, 1)], QS[2])
    assert valid == [0, 0] and got == [[(-1, -1)] * 2] * 2
    # a mix: every third replicate invalid (validity column 0), every other of the rest 1 / 1 by substitution (den 0, flag 1)
    mix = np.zeros((B, 3), np.int64)
    mix[:, 0] = np.arange(B) % 7
    mix[:, 1] = np.where(np.arange(B) % 2 == 0, 0, 10)
    mix[:, 2] = np.arange(B) % 3
    got, valid = _check_quantiles(mix, [(0, 1, 1, -1, 2, 1), (0, 1, 1, -1, 2, 0)], QS[5])
    assert valid[0] == B - 34 and valid[1] < valid[0] and got[0][-1] == (1, 1)
    # fractions that differ only beyond double precision: the order is exact
    # ((2^51 + 1) / 2^52 against (2^51 + 2) / (2^52 + 1) are one unit in the last place apart; (2^52 - 3) / (2^52 - 1) against
    # (2^52 - 2) / 2^52 are the same double, 1 - 2^-51)
    for a, b, same_double in (((2 ** 51 + 1, 2 ** 52), (2 ** 51 + 2, 2 ** 52 + 1), False),
                              ((2 ** 52 - 3, 2 ** 52 - 1), (2 ** 52 - 2, 2 ** 52), True)):
        assert (a[0] / a[1] == b[0] / b[1]) == same_double and a[0] * b[1] < b[0] * a[1]
        close = np.array([b, a, b, a, a, b, b, a], np.int64)
        got, valid = _check_quantiles(close, [(0, 1, 1, -1, -1, 0)], [(1, 8), (1, 2), (5, 8), (7, 8)])
        assert got[0] == [a, a, b, b] and valid == [8]
    # num_mult 2 and two denominator columns at the top of the contract: both factors just below 2^54
    top = np.array([[2 ** 52 - 1 - i, 2 ** 52 - 1, 2 ** 52 - 1 - 3 * i] for i in range(9)], np.int64)
    _check_quantiles(top, [(0, 2, 1, 2, -1, 0)], QS[5])


# ---- the wrappers ----------------------------------------------------------------------------------------------------------------
def _corpus():
    """Seven channels in three meetings (one of them without a participant), tracks of 3,000 frames."""
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
    tracks = [recipe.make_prob_track(40 + c, 3000) for c in range(len(channels))]
    return se.TranscriptIndex(rows, chans), channels, tracks


def _same(a, b):
    assert len(a) == len(b) and len(a) > 0
    for ra, rb in zip(a, b):
        assert len(ra) == len(rb) and all(x == y or (x != x and y != y) for x, y in zip(ra, rb)), (ra, rb)


def test_device_form_is_the_host_form(monkeypatch):
    import bootstrap
    import sweep_eval as se
    index, channels, tracks = _corpus()
    assert len(channels) == 7
    thresholds, min_lengths, B = [0.1, 0.3, 0.5, 0.7, 0.9], [0.0, 0.2], 64
    levels = [i / 64 for i in range(65)]
    plain, plain_ev = se.score_sweep_host(tracks, channels, thresholds, min_lengths, 100.0, index, events=(1, 0))
    vit = se.score_sweep_host(tracks, channels, thresholds[1:4], min_lengths, 100.0, index, penalties=[0.0, 2.0])
    dense, dense_ev = se.score_surface_host(tracks, channels, levels, min_lengths, 100.0, index, events=(20, 50))
    cases = [(plain, thresholds, {}), (plain, thresholds, {"events": plain_ev}), (vit, thresholds[1:4], {"penalties": [0.0, 2.0]}),
             (dense, levels, {}), (dense, levels, {"events": dense_ev, "unit": "meeting", "level": "99.9"})]
    calls = []
    real = bootstrap.sums_device
    monkeypatch.setattr(bootstrap, "sums_device", lambda x, w: (calls.append(tuple(x.shape)), real(x, w))[1])
    for cap in (None, 4096):                                                       # 4096 bytes: (8 - 1) // 2 = 3 cells of the time matrix a chunk
        if cap is not None:
            monkeypatch.setattr(bootstrap, "SUMS_BYTES_CAP", cap)
        for scores, thr, kw in cases:
            del calls[:]
            want = se.bootstrap_sum_stats_host(scores, channels, thr, min_lengths, index, n_boot=B, seed=5, **kw)
            got = se.bootstrap_sum_stats_device(scores, channels, thr, min_lengths, index, n_boot=B, seed=5, **kw)
            if "events" in kw:
                _same(got[1], want[1])
                got, want = got[0], want[0]
            _same(got, want)
            assert len(calls) == (1 + ("events" in kw)) if cap is None else len(calls) >= 3
            assert all(n * m * 8 <= (cap or 2 ** 30) or m <= 5 for n, m in [(B, c[1]) for c in calls])
    assert any(r[3] < r[4] for r in got)                                           # (intervals with a width)
    with pytest.raises(ValueError):
        se.bootstrap_sum_stats_device(plain * 2 ** 30, channels, thresholds, min_lengths, index, n_boot=B)     # x beyond 2^40: refused on the host
    _hip, _ = _lib()
    with pytest.raises(_hip.LadHipError):
        bootstrap.intervals_device(np.ones((3, 3), np.int64), 2, [(1, 1, 0, None, None, 1)], 4, 0, [(1, 2)], device="cpu")


def test_evaluate_sweep_device_scorer_writes_the_host_scorers_bytes(tmp_path):
    import os

    import evaluate_sweep
    args = sm.write_corpus(tmp_path)
    boot = ["--bootstrap", "64", "--bootstrap_seed", "11"]
    for name, extra in (("plain", []), ("events", ["--events"]), ("hysteresis", ["--offset_drops", "0.0,0.1", "--min_gaps", "0.05"])):
        files = {}
        for scorer in ("host", "device"):
            out = tmp_path / f"{name}_{scorer}"
            evaluate_sweep.main(args + extra + boot + ["--scorer", scorer, "--out_dir", str(out)])
            files[scorer] = {f: open(out / f, "rb").read() for f in sorted(os.listdir(out))}
        assert files["host"] == files["device"] and "sum_stats_ci.csv" in files["host"], name
        assert ("event_sum_stats_ci.csv" in files["host"]) == (name == "events")


def test_refusals_leave_the_outputs_untouched():
    _hip, lib = _lib()
    G, B, M, F, Q = 5, 6, 7, 2, 2
    st = _hip.stream_handle(torch.device("cuda", torch.cuda.current_device()))
    x = torch.arange(G * M, dtype=torch.int64, device="cuda").reshape(G, M)
    w = torch.full((B * G + GUARD,), W_FILL, dtype=torch.int32, device="cuda")
    sums = torch.full((B * M + GUARD,), S_FILL, dtype=torch.int64, device="cuda")
    out = torch.full((F * Q * 2 + GUARD,), O_FILL, dtype=torch.int64, device="cuda")
    valid = torch.full((F + GUARD,), V_FILL, dtype=torch.int32, device="cuda")
    good_w = torch.ones((B, G), dtype=torch.int32, device="cuda")
    good_sums = torch.arange(1, B * M + 1, dtype=torch.int64, device="cuda").reshape(B, M)
    fh = np.array([[0, 1, 1, -1, -1, 1], [2, 2, 3, 4, 5, 0]], np.int32)
    fd = torch.from_numpy(fh).cuda()

    def ptr(t):
        return t if isinstance(t, ctypes.c_void_p) or t is None else _hip.ptr(t)

    def inside(t, offset=0):
        return ctypes.c_void_p(t.data_ptr() + offset)

    def weights(units=G, replicates=B, buf=w):
        return lib.lad_bootstrap_weights(units, replicates, 1, ptr(buf), st)

    def sums_(x_=x, w_=good_w, units=G, columns=M, replicates=B, s=sums):
        return lib.lad_bootstrap_sums(ptr(x_), ptr(w_), units, columns, replicates, ptr(s), st)

    def quantiles(s=good_sums, columns=M, replicates=B, f=fd, f_host=fh, n=F, qn=(1, 39), qd=(40, 40), o=out, v=valid):
        host = None if f_host is None else np.ascontiguousarray(f_host, np.int32).ctypes.data_as(_I32P)
        nq = len(qn)
        return lib.lad_bootstrap_quantiles(ptr(s), columns, replicates, ptr(f), host, n, (ctypes.c_int32 * nq)(*qn), (ctypes.c_int32 * nq)(*qd),
                                           nq, ptr(o), ptr(v), st)
    null = ctypes.c_void_p(0)
    for kw in (dict(units=0), dict(units=4097), dict(replicates=0), dict(replicates=4097), dict(buf=null)):
        assert weights(**kw) == _hip.LAD_ERR_INVALID and b"lad_bootstrap_weights" in lib.lad_last_error(), kw
    for kw in (dict(x_=null), dict(w_=null), dict(s=null), dict(units=0), dict(units=4097), dict(replicates=0), dict(replicates=4097),
               dict(columns=-1), dict(columns=2 ** 32 + 1), dict(s=inside(x, 8)), dict(s=inside(good_w, 0))):
        assert sums_(**kw) == _hip.LAD_ERR_INVALID and b"lad_bootstrap_sums" in lib.lad_last_error(), kw

    def bad_figure(col, value):
        f = fh.copy()
        f[1, col] = value
        return dict(f_host=f)
    for kw in (dict(s=null), dict(f=null), dict(f_host=None), dict(o=null), dict(v=null), dict(columns=0), dict(replicates=0),
               dict(replicates=4097), dict(n=-1), dict(qn=(), qd=()), dict(qn=(1,) * 17, qd=(2,) * 17), dict(qn=(0, 1), qd=(40, 40)),
               dict(qn=(1, 40), qd=(40, 40)), dict(qn=(1, 41), qd=(40, 40)), dict(qn=(-1, 1), qd=(40, 40)), dict(qn=(1, 1), qd=(0, 40)),
               bad_figure(0, -1), bad_figure(0, M), bad_figure(1, 0), bad_figure(1, 3), bad_figure(2, -1), bad_figure(2, M),
               bad_figure(3, -2), bad_figure(3, M), bad_figure(4, -2), bad_figure(4, M), bad_figure(5, 2), bad_figure(5, -1),
               dict(o=inside(good_sums, 16)), dict(v=inside(good_sums, 0)), dict(o=inside(fd, 0)), dict(v=inside(fd, 8)),
               dict(v=inside(out, 8))):
        assert quantiles(**kw) == _hip.LAD_ERR_INVALID and b"lad_bootstrap_quantiles" in lib.lad_last_error(), kw
    torch.cuda.synchronize()
    assert (w == W_FILL).all() and (sums == S_FILL).all() and (out == O_FILL).all() and (valid == V_FILL).all()
    # nothing to do: LAD_OK, nothing launched, nothing written
    assert sums_(columns=0, x_=null, s=null) == 0 and quantiles(n=0, f=null, f_host=None, o=null, v=null) == 0
    torch.cuda.synchronize()
    assert (sums == S_FILL).all() and (out == O_FILL).all() and (valid == V_FILL).all()
    # and the calls that all of the above varied are good ones
    assert weights() == 0 and sums_() == 0 and quantiles() == 0
    torch.cuda.synchronize()
    assert w[:B * G].reshape(B, G).cpu().tolist() == model.weights(G, B, 1) and (w[B * G:] == W_FILL).all()
    assert torch.equal(sums[:B * M].reshape(B, M), x.sum(dim=0).expand(B, M)) and (sums[B * M:] == S_FILL).all()
    want, want_valid = model.quantiles(good_sums.cpu().tolist(), [tuple(f) for f in fh.tolist()], [(1, 40), (39, 40)])
    assert out[:F * Q * 2].reshape(F, Q, 2).cpu().tolist() == [[list(p) for p in f] for f in want] and valid[:F].cpu().tolist() == want_valid
    assert (out[F * Q * 2:] == O_FILL).all() and (valid[F:] == V_FILL).all()
