"""GPU tests of the span statistics (csrc/spanstats.hip: lad_span_stats_prepare / lad_span_stats; laugh_segmenter.span_stats_device
and the stats=True device forms; segment_laughter.py --confidence / --min_confidence).

Everything is integers, selected track values and single IEEE divisions, so every comparison is equality: sums and peaks as
integers, peak values as bytes.  The yardstick is tests/_spanstats_model.py, a Python loop over the frames of every span."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import recipe

import _spanstats_cases as cases
import _spanstats_model as model

pytestmark = pytest.mark.gpu

_I32P = ctypes.POINTER(ctypes.c_int32)
FRAMES = [1, 2, 255, 256, 257, 2047, 2048, 2049, 4097]
# One launch of the first and third prepare pass covers 2048 frames per workgroup and writes tree levels 1..11; one workgroup of the
# second tree launch covers 2048 nodes of level 11 = 2048 * 2048 frames and writes levels 12..22.  Three frames beyond that the
# second tree launch has two workgroups, the third one (levels 23..) has two real nodes to reduce, the scan of the chunk sums has
# 2049 entries (more than one of its steps), and a span can cross frame 2^22, the first edge that only level 22 and up see.
BIG_FRAMES = 2048 * 2048 + 3
GUARD = 5


def _lib():
    import _hip
    return _hip, _hip.lib()


def _device_form(x2, table, counts, K):
    """prepare + lad_span_stats through the C ABI on the (C, T) numpy track x2 and the device table (total, 2) int32 with its host
    counts: the three arrays on the host.  Checked on the way: two calls write identical bytes, the guard words behind the last
    row, the track and the table are untouched."""
    _hip, lib = _lib()
    p = torch.from_numpy(np.array(x2)).cuda()
    C, T = p.shape
    dtype = 0 if p.dtype == torch.float32 else 1
    counts = np.ascontiguousarray(counts, np.int32)
    total = int(counts.sum())
    assert table.shape == (total, 2) and table.dtype == torch.int32 and len(counts) == C * K
    table = table.contiguous() if total else torch.zeros((1, 2), dtype=torch.int32, device="cuda")
    bits = torch.int32 if dtype == 0 else torch.int64
    p_before, table_before = p.view(bits).clone(), table.clone()
    st = _hip.stream_handle(p.device)
    outs = []
    for _ in range(2):
        ws = torch.empty(lib.lad_span_stats_workspace_bytes(C, T), dtype=torch.uint8, device="cuda")
        sums = torch.full((total + GUARD,), -77, dtype=torch.int64, device="cuda")
        peaks = torch.full((total + GUARD,), -78, dtype=torch.int32, device="cuda")
        values = torch.full((total + GUARD,), -79.5, dtype=torch.float64, device="cuda")
        _hip.check(lib.lad_span_stats_prepare(_hip.ptr(p), dtype, C, T, _hip.ptr(ws), st), "lad_span_stats_prepare")
        _hip.check(lib.lad_span_stats(_hip.ptr(p), dtype, C, T, _hip.ptr(ws), _hip.ptr(table), counts.ctypes.data_as(_I32P), K,
                                      _hip.ptr(sums), _hip.ptr(peaks), _hip.ptr(values), st), "lad_span_stats")
        outs.append((sums.cpu().numpy(), peaks.cpu().numpy(), values.cpu().numpy()))
    for a, b in zip(*outs):
        assert a.tobytes() == b.tobytes()
    sums, peaks, values = outs[0]
    assert (sums[total:] == -77).all() and (peaks[total:] == -78).all() and (values[total:] == -79.5).all()
    assert torch.equal(p.view(bits), p_before) and torch.equal(table, table_before)
    return sums[:total], peaks[:total], values[:total]


def _check_tables(x2, per_channel, what):
    """per_channel[c][k]: the int64 (n, 2) spans of setting k of channel c.  The device form on all of them at once against the
    model on each."""
    K = len(per_channel[0])
    flat = [np.asarray(s, np.int64).reshape(-1, 2) for chan in per_channel for s in chan]
    counts = np.array([len(s) for s in flat], np.int32)
    table = torch.from_numpy(np.concatenate(flat).astype(np.int32)).cuda()
    got = _device_form(x2, table, counts, K)
    want = [cases.model_arrays(x2[c], s) for c, chan in enumerate(per_channel) for s in chan]
    cases.assert_same(got, [np.concatenate([w[i] for w in want]) for i in range(3)], what)


def _decoder_tables(x2):
    """The real tables of the three decoders on the (C, T) track, as they lie on the device: [(name, table, counts, K)]."""
    import laugh_segmenter as ls
    p = torch.from_numpy(np.array(x2)).cuda()
    probs, dtype, _ = ls.device_track(p)
    out = []
    vt = ls._viterbi_table(None)
    for name, decoder, chunk, ctx in (
            ("threshold", ls.THRESHOLD, list(cases.THRESHOLDS), {}),
            ("hysteresis", ls.HYSTERESIS, list(cases.HYSTERESIS), {"fps_host": ls.fps_per_channel(cases.FPS, len(x2))}),
            ("viterbi", ls.VITERBI, ls.viterbi_settings(*cases.VITERBI, vt), {"table": vt})):
        _, table, counts, _ = ls._device_tables(decoder, probs, dtype, chunk, ctx)
        out.append((name, table, counts, len(chunk)))
    return out


def _check_decoder_tables(x2, what):
    seen = 0
    for name, table, counts, K in _decoder_tables(x2):
        got = _device_form(x2, table, counts, K)
        rows, edges = table.cpu().numpy().astype(np.int64), np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])
        want = [cases.model_arrays(x2[i // K], rows[edges[i]:edges[i + 1]]) for i in range(len(counts))]
        cases.assert_same(got, [np.concatenate([w[i] for w in want]) for i in range(3)], (*what, name))
        seen += len(rows)
    return seen


@pytest.mark.parametrize("T", FRAMES)
def test_one_channel_against_the_model(T):
    seen = 0
    for kind in cases.TRACKS:
        for dtype in (np.float32, np.float64):
            x2 = cases.track(kind, T, dtype)[None]
            hand = cases.hand_tables(T)
            names = sorted(hand)
            _check_tables(x2, [[hand[n] for n in names]], (kind, T, np.dtype(dtype).name, "hand"))        # one table per "setting"
            _check_tables(x2, [[hand["empty"]]], (kind, T, "zero rows"))
            if dtype == np.float32 or kind == "wild":
                seen += _check_decoder_tables(x2, (kind, T, np.dtype(dtype).name))
    assert seen > 0 or T < 255


def test_invalid_rows_yield_nothing_and_leave_their_neighbours():
    T = 2049
    x2 = cases.track("noise", T, np.float32)[None]
    spans = cases.hand_tables(T)["invalid"]
    table = torch.from_numpy(spans.astype(np.int32)).cuda()
    s, p, v = _device_form(x2, table, np.array([len(spans)], np.int32), 1)
    assert s[1:4].tolist() == [0, 0, 0] and p[1:4].tolist() == [-1, -1, -1] and v[1:4].tolist() == [0.0, 0.0, 0.0]
    want = cases.model_arrays(x2[0], spans)
    cases.assert_same((s, p, v), want, "invalid")
    assert want[1][0] >= 2 and want[1][4] == T - 1


@pytest.mark.parametrize("T", [257, 4097])
def test_three_channels_one_of_them_empty(T):
    """The middle channel is NaN throughout: every decoder leaves its tables empty, and the hand-made tables give it no row."""
    for kinds, dtype in ((("noise", "wild"), np.float32), (("plateaus", "fp16"), np.float64)):
        x2 = np.stack([cases.track(kinds[0], T, dtype), np.full(T, np.nan, dtype), cases.track(kinds[1], T, dtype)])
        hand = cases.hand_tables(T, every_frame=T < 1000)
        names = sorted(hand)
        none = [hand["empty"]] * len(names)
        _check_tables(x2, [[hand[n] for n in names], none, [hand[n] for n in reversed(names)]], (kinds, T, "hand"))
        for name, table, counts, K in _decoder_tables(x2):
            assert counts.reshape(3, K)[1].sum() == 0 and counts.reshape(3, K)[[0, 2]].sum() > 0, name
        assert _check_decoder_tables(x2, (kinds, T)) > 0


def test_beyond_one_workgroup_of_the_second_tree_launch():
    T = BIG_FRAMES
    # one span as long as a constant track: by hand
    ones = np.ones((1, T), np.float32)
    table = torch.tensor([[0, T - 1], [1, T - 2], [T - 1, T - 1]], dtype=torch.int32, device="cuda")
    s, p, v = _device_form(ones, table, np.array([3], np.int32), 1)
    assert s.tolist() == [T << 32, (T - 2) << 32, 1 << 32] and p.tolist() == [0, 1, T - 1] and v.tolist() == [1.0, 1.0, 1.0]
    # short spans around every edge up to frame 2^22, and one long span, against the model
    x2 = cases.track("fp16", T, np.float32)[None]
    hand = cases.hand_tables(T, every_frame=False, long_spans=False)
    assert 2048 * 2048 in cases.edges_of(T) and len(hand["edges"]) > 50
    _check_tables(x2, [[hand["edges"], np.array([[1, T - 2]]), hand["invalid"]]], ("fp16", T))
    # ramps: the peak of the whole track is its last and its first frame (float64: every value of the ramp is distinct)
    for kind, peak in (("rising", T - 1), ("falling", 0)):
        x = cases.track(kind, T, np.float64)
        whole = torch.tensor([[0, T - 1], [2048 * 2048 - 1, 2048 * 2048]], dtype=torch.int32, device="cuda")
        s, p, v = _device_form(x[None], whole, np.array([2], np.int32), 1)
        assert p[0] == peak and v[0] == float(x[peak]) and p[1] == (2048 * 2048 if kind == "rising" else 2048 * 2048 - 1)
        assert s[1] == model.fixed(float(x[2048 * 2048 - 1])) + model.fixed(float(x[2048 * 2048]))


def test_refusals_leave_the_outputs_untouched():
    _hip, lib = _lib()
    T, C, K = 300, 2, 2
    p = torch.from_numpy(np.stack([cases.track("noise", T, np.float32), cases.track("wild", T, np.float32)])).cuda()
    ws_bytes = lib.lad_span_stats_workspace_bytes(C, T)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    st = _hip.stream_handle(p.device)
    _hip.check(lib.lad_span_stats_prepare(_hip.ptr(p), 0, C, T, _hip.ptr(ws), st), "lad_span_stats_prepare")
    table = torch.tensor([[0, 5], [7, 9], [10, 299], [3, 3]], dtype=torch.int32, device="cuda")
    counts = np.array([1, 1, 0, 2], np.int32)
    sums = torch.full((8,), -77, dtype=torch.int64, device="cuda")
    peaks = torch.full((8,), -78, dtype=torch.int32, device="cuda")
    values = torch.full((8,), -79.5, dtype=torch.float64, device="cuda")
    ws_before = ws.clone()

    def call(probs=p, dtype=0, channels=C, frames=T, workspace=ws, tab=table, cnt=counts, k=K, s=sums, pk=peaks, v=values):
        ptr = lambda t: t if isinstance(t, ctypes.c_void_p) else _hip.ptr(t)        # noqa: E731
        return lib.lad_span_stats(ptr(probs), dtype, channels, frames, ptr(workspace), ptr(tab),
                                  cnt.ctypes.data_as(_I32P) if cnt is not None else None, k, ptr(s), ptr(pk), ptr(v), st)

    def inside(t, offset):
        return ctypes.c_void_p(t.data_ptr() + offset)
    refused = [dict(probs=None), dict(workspace=None), dict(tab=None), dict(cnt=None), dict(s=None), dict(pk=None), dict(v=None),
               dict(dtype=2), dict(dtype=-1), dict(channels=0), dict(channels=65536), dict(frames=0), dict(frames=2 ** 30 + 1), dict(k=0),
               dict(cnt=np.array([1, -1, 0, 2], np.int32)),
               dict(s=inside(p, 0)), dict(pk=inside(p, 8)), dict(v=inside(p, 16)),                     # outputs inside the track
               dict(s=inside(table, 0)), dict(v=inside(table, 8)),                                     # ... the table
               dict(s=inside(ws, 0)), dict(pk=inside(ws, ws_bytes - 4)), dict(v=inside(ws, 256))]      # ... the workspace
    for kw in refused:
        lib.lad_span_stats_workspace_bytes(1, 1)
        assert call(**kw) == _hip.LAD_ERR_INVALID, kw
        assert b"lad_span_stats" in lib.lad_last_error(), kw
    for kw in (dict(probs=None), dict(workspace=None), dict(dtype=5), dict(channels=0), dict(frames=2 ** 30 + 1)):
        args = dict(probs=p, dtype=0, channels=C, frames=T, workspace=ws)
        args.update(kw)
        rc = lib.lad_span_stats_prepare(_hip.ptr(args["probs"]), args["dtype"], args["channels"], args["frames"], _hip.ptr(args["workspace"]), st)
        assert rc == _hip.LAD_ERR_INVALID and b"lad_span_stats_prepare" in lib.lad_last_error(), kw
    assert lib.lad_span_stats_prepare(_hip.ptr(p), 0, C, T, inside(p, 64), st) == _hip.LAD_ERR_INVALID      # probs inside the workspace
    torch.cuda.synchronize()
    assert (sums == -77).all() and (peaks == -78).all() and (values == -79.5).all() and torch.equal(ws, ws_before)
    # zero rows: LAD_OK, nothing launched, nothing written (a null table is fine then)
    assert call(tab=None, cnt=np.zeros(4, np.int32)) == 0
    torch.cuda.synchronize()
    assert (sums == -77).all() and (peaks == -78).all() and (values == -79.5).all() and torch.equal(ws, ws_before)
    # and the call that all of the above varied is a good one
    assert call() == 0
    torch.cuda.synchronize()
    x = p.cpu().numpy()
    want = [cases.model_arrays(x[c], s) for c, s in ((0, [[0, 5]]), (0, [[7, 9]]), (1, [[10, 299], [3, 3]]))]
    got = (sums.cpu().numpy()[:4], peaks.cpu().numpy()[:4], values.cpu().numpy()[:4])
    cases.assert_same(got, [np.concatenate([w[i] for w in want]) for i in range(3)], "the good call")
    assert (sums[4:] == -77).all() and (peaks[4:] == -78).all() and (values[4:] == -79.5).all()


def test_span_stats_device_is_the_host_form():
    import _hip
    import laugh_segmenter as ls
    T = 4097
    x2 = np.stack([cases.track("noise", T, np.float32), cases.track("wild", T, np.float32)])
    p = torch.from_numpy(x2).cuda()
    for probs, rows in ((p, [0, 0, 1, 1]), (p[1], [1, 1])):
        track2, dtype, _ = ls.device_track(probs)
        _, table, counts, _ = ls._device_tables(ls.THRESHOLD, track2, dtype, [0.3, 0.7], {})
        got = ls.span_stats_device(probs, table, counts)
        assert [g.dtype for g in got] == [np.int64, np.int64, np.float64]
        spans, edges = table.cpu().numpy().astype(np.int64), np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])
        want = [ls.span_stats(x2[c], spans[edges[i]:edges[i + 1]]) for i, c in enumerate(rows)]
        cases.assert_same(got, [np.concatenate([w[i] for w in want]) for i in range(3)], "span_stats_device")
    with pytest.raises(_hip.LadHipError):
        ls.span_stats_device(p.cpu(), table, counts)                                   # no CPU fallback
    with pytest.raises(_hip.LadHipError):
        ls.span_stats_device(p.half(), table, counts)


def _same_stats(dev, host):
    (d_inst, d_stats), (h_inst, h_stats) = dev, host
    assert d_inst == h_inst and list(d_inst) == list(h_inst) and list(d_stats) == list(h_stats) == list(h_inst)
    n = 0
    for key, rows in h_inst.items():
        assert d_stats[key].dtype == np.float64 and d_stats[key].shape == (len(rows), 3)
        assert d_stats[key].tobytes() == h_stats[key].tobytes(), key
        n += len(rows)
    return n


def test_instances_device_with_stats_equal_the_host_forms():
    import _hip
    import laugh_segmenter as ls
    x = cases.track("wild", 6000, np.float32)
    p = torch.from_numpy(np.array(x)).cuda()
    thresholds, min_lengths = [0.2, 0.5, 0.8], [0.0, 0.05, 0.2]
    assert _same_stats(ls.get_laughter_instances_device(p, thresholds, min_lengths, 100.0, stats=True),
                       ls.get_laughter_instances(p.cpu(), thresholds, min_lengths, 100.0, stats=True)) > 100
    assert ls.get_laughter_instances_device(p, thresholds, min_lengths, 100.0) == ls.get_laughter_instances(x, thresholds, min_lengths, 100.0)
    # 5 * 4 * 4 = 80 settings: two rounds of the hysteresis family, one prepare
    five, drops, gaps = [0.1, 0.3, 0.5, 0.7, 0.9], [0.0, 0.1, 0.2, 0.3], [0.0, 0.02, 0.05, 0.5]
    assert len(five) * len(drops) * len(gaps) > _hip.lib().lad_binarize_max_settings()
    dev = ls.binarize_instances_device(p, five, min_lengths, 100.0, drops, gaps, stats=True)
    assert len(dev[0]) == 80 * 3
    assert _same_stats(dev, ls.binarize_instances(p.cpu(), five, min_lengths, 100.0, drops, gaps, stats=True)) > 1000
    short = torch.from_numpy(np.array(cases.track("noise", 3000, np.float64))).cuda()
    assert _same_stats(ls.viterbi_instances_device(short, [0.4, 0.6], min_lengths, 100.0, [0.0, 2.0], stats=True),
                       ls.viterbi_instances(short.cpu(), [0.4, 0.6], min_lengths, 100.0, [0.0, 2.0], stats=True)) > 20
    none = ls.get_laughter_instances_device(p, [1.0], [0.0], 100.0, stats=True)          # a round whose tables have no row at all
    assert none[0] == {(1.0, 0.0): []} and none[1][(1.0, 0.0)].shape == (0, 3)
    empty = ls.get_laughter_instances_device(torch.zeros(0, dtype=torch.float32, device="cuda"), [0.5], [0.2], 100.0, stats=True)
    assert empty[0] == {(0.5, 0.2): []} and empty[1][(0.5, 0.2)].shape == (0, 3)


def _write_wav(path, x):
    from scipy.io import wavfile
    wavfile.write(path, 16000, (np.clip(x, -1, 1) * 32767).astype(np.int16))


def _checkpoint(tmp_path, seed=101):
    import contextlib
    import io

    import config
    import torch_utils
    cfg = config.MODEL_MAP["resnet_base"]
    with contextlib.redirect_stdout(io.StringIO()):
        m = cfg["model"](dropout_rate=0.0, linear_layer_size=cfg["linear_layer_size"], filter_sizes=cfg["filter_sizes"])
    full = m.state_dict()
    for k, v in recipe.make_state(seed).items():
        full[k] = torch.from_numpy(v.copy())
    m.load_state_dict(full)
    ck = tmp_path / "ckpt"
    with contextlib.redirect_stdout(io.StringIO()):
        torch_utils.save_checkpoint(torch_utils.make_state_dict(m, None, 0, 0, 1.0), True, str(ck))
    return str(ck)


def _tree(root):
    return {os.path.relpath(os.path.join(d, f), root): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(root) for f in fs}


def test_segment_laughter_confidence(tmp_path):
    import audio_utils
    import laugh_segmenter as ls
    import segment_laughter
    wav = tmp_path / "chan.wav"
    _write_wav(wav, recipe.make_clips(22, 1, n_samples=16000 * 10)[0])
    model_ = segment_laughter.build_model("resnet_base", _checkpoint(tmp_path), torch.device("cuda", 0))
    min_lengths = [0.0, 0.1]

    def run(name, thresholds, **kw):
        _, d = segment_laughter.load_and_pred(model_, str(wav), thresholds, min_lengths, str(tmp_path / name), verbose=False,
                                              precision="fp16", **kw)
        return d, _tree(tmp_path / name)
    run("probe", [0.5], save_probs=str(tmp_path / "track.npy"))
    track = np.load(tmp_path / "track.npy")
    fps = len(track) / float(audio_utils.get_audio_length(str(wav)))
    thresholds = sorted({float(np.quantile(track, q)) for q in (0.3, 0.6)})             # levels the track does cross
    # without the flags: the files and bytes of a call that does not know them
    plain, plain_tree = run("plain", thresholds)
    again, again_tree = run("again", thresholds, confidence=False, min_confidence=None)
    assert (plain, plain_tree) == (again, again_tree) and all(k.endswith(".TextGrid") for k in plain_tree)
    assert len(plain_tree) == len(thresholds) * len(min_lengths) and sum(map(len, plain.values())) > 0
    # --confidence: identical bytes under both segmenters, for every decoder family
    for name, kw in (("thr", {}), ("hyst", {"offset_drops": [0.0, 0.05], "min_gaps": [0.05]}), ("vit", {"penalties": [1.0]})):
        host, host_tree = run(name + "_host", thresholds, confidence=True, segmenter="host", **kw)
        dev, dev_tree = run(name + "_device", thresholds, confidence=True, segmenter="device", **kw)
        assert host == dev and host_tree == dev_tree
        assert sum(k.endswith(".confidence.csv") for k in host_tree) == sum(k.endswith(".TextGrid") for k in host_tree) == len(host)
        if name == "thr":
            assert host == plain and {k: v for k, v in host_tree.items() if k.endswith(".TextGrid")} == plain_tree
            conf_tree = host_tree
    # the csv holds the model's figures, and --min_confidence removes exactly the instances whose model mean is below it
    expect, means = {}, []
    for thr in thresholds:
        spans = ls.get_laughter_frame_spans(track, thr).tolist()
        rows = model.span_stats(track.tolist(), spans)
        for min_l in min_lengths:
            expect[(thr, min_l)] = [((a / fps, b / fps), model.confidence(r, a, b, fps)) for r, (a, b) in zip(rows, spans)
                                    if b / fps - a / fps > min_l]
            means += [c[0] for _, c in expect[(thr, min_l)]]
            lines = conf_tree[f"t_{thr}/l_{min_l}/chan.confidence.csv"].decode().split("\n")
            assert lines[0] == "start,end,mean_prob,peak_time,peak_prob" and lines[-1] == ""
            assert lines[1:-1] == [",".join(repr(float(v)) for v in (*se, *c)) for se, c in expect[(thr, min_l)]]
    cut = sorted(means)[len(means) // 2]
    for seg in ("host", "device"):
        kept, kept_tree = run("kept_" + seg, thresholds, confidence=True, min_confidence=cut, segmenter=seg)
        for key, rows in expect.items():
            want = [(se, c) for se, c in rows if not c[0] < cut]
            assert kept[key] == [se for se, _ in want]
            lines = kept_tree[f"t_{key[0]}/l_{key[1]}/chan.confidence.csv"].decode().split("\n")
            assert lines[1:-1] == [",".join(repr(float(v)) for v in (*se, *c)) for se, c in want]
            ref = tmp_path / "ref.TextGrid"
            import textgrid
            textgrid.write_laughter_textgrid(str(ref), kept[key], xmax=audio_utils.get_audio_length(str(wav)))
            assert kept_tree[f"t_{key[0]}/l_{key[1]}/chan.TextGrid"] == ref.read_bytes()
        assert sum(map(len, kept.values())) < sum(map(len, plain.values())) or len(set(means)) < 2
