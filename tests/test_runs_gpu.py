"""GPU tests of the device-side threshold sweep (csrc/runs.hip; laugh_segmenter.get_laughter_instances_device and
get_laughter_frame_spans_device; segment_laughter.py --segmenter device).

Everything here is integer bookkeeping plus IEEE float64 divisions, so every comparison is equality: against the stored results
of the reference's own get_laughter_instances (tests/golden/segmenter.json), against the per-frame loop
oracle.segmenter_oracle.run_indices, and against the host sweep laugh_segmenter.get_laughter_instances."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from oracle import recipe, segmenter_oracle as so

pytestmark = pytest.mark.gpu

# the 29 thresholds and 3 min_lengths of the evaluation sweep (cluster_scripts/gen_eval_exp.py:30-36)
EVAL_THRESHOLDS = [float(t) for t in np.concatenate((np.linspace(0, 0.9, 19).round(2), np.linspace(0.91, 1, 10).round(2)))]
EVAL_MIN_LENGTHS = [0.0, 0.1, 0.2]
# float32(t) > t at these (so a float32 comparison accepts p == float32(t) where the reference rejects it)
F32_ROUNDS_UP = [0.05, 0.1, 0.15, 0.2, 0.3, 0.4, 0.55, 0.6, 0.8, 0.85, 0.91, 0.92, 0.93, 0.97, 0.98, 0.99]


def _tile():
    import _hip
    return int(_hip.lib().lad_runs_tile_frames())


def _dev_spans(p, thresholds):
    import laugh_segmenter as ls
    got = ls.get_laughter_frame_spans_device(torch.from_numpy(np.ascontiguousarray(p)).cuda(), thresholds)
    for g in got:
        assert g.dtype == np.int64 and g.ndim == 2 and g.shape[1] == 2
    return [[tuple(int(v) for v in r) for r in g] for g in got]


def _check_vs_loop(p, thresholds):
    got = _dev_spans(p, thresholds)
    assert len(got) == len(thresholds)
    for thr, g in zip(thresholds, got):
        assert g == so.run_indices(p, thr), (len(p), p.dtype, thr)


def test_eval_thresholds_are_the_reference_sweep():
    assert len(EVAL_THRESHOLDS) == 29 and EVAL_THRESHOLDS[0] == 0.0 and EVAL_THRESHOLDS[-1] == 1.0
    assert [t for t in EVAL_THRESHOLDS if float(np.float32(t)) > t] == F32_ROUNDS_UP


def test_reference_goldens(golden_dir):
    import laugh_segmenter as ls
    cases = json.load(open(os.path.join(golden_dir, "segmenter.json")))
    assert len(cases) >= 3
    for c in cases:
        p = recipe.make_prob_track(c["seed"], c["n"]) if "seed" in c else np.array(c["probs"], dtype=np.float64)
        ref = {tuple(k): [tuple(s) for s in v] for k, v in c["result"]}
        if len(p) == 0:
            d = ls.get_laughter_instances_device(torch.zeros(0, dtype=torch.float64, device="cuda"), c["thresholds"],
                                                 c["min_lengths"], c["fps"])
        else:
            d = ls.get_laughter_instances_device(torch.from_numpy(p).cuda(), c["thresholds"], c["min_lengths"], c["fps"])
        assert list(d.keys()) == list(ref.keys())
        for k in ref:
            assert d[k] == ref[k], (c.get("seed", c.get("name")), k)
            assert all(type(v) is float for s in d[k] for v in s)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_run_indices_vs_per_frame_loop(dtype):
    tile = _tile()
    assert tile >= 64 and tile % 64 == 0
    thresholds = [0.0, 1.0] + EVAL_THRESHOLDS
    for seed, n in enumerate([1, 2, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile, 1000, 36000]):
        p = recipe.make_prob_track(seed, n) if n >= 100 else np.random.default_rng(seed).random(n)
        _check_vs_loop(p.astype(dtype), thresholds)


def test_values_at_float32_of_each_threshold():
    """p == float32(t) and its two float32 neighbours, as a float32 track: on iff the float64 value exceeds t."""
    accepted = []
    for t in EVAL_THRESHOLDS:
        c = np.float32(t)
        p = np.array([np.nextafter(c, np.float32(-1)), np.nan, c, np.nan, np.nextafter(c, np.float32(2))], dtype=np.float32)
        want = [(i, i) for i in (0, 2, 4) if so.fix_prob(float(p[i])) > t]
        got = _dev_spans(p, [t])[0]
        assert got == so.run_indices(p, t) == want, t
        if (2, 2) in got:
            accepted.append(t)
        # the same three values as float64: the comparison is the same one
        assert _dev_spans(p.astype(np.float64), [t])[0] == want, t
        # and among all 29 thresholds at once
        k = EVAL_THRESHOLDS.index(t)
        assert _dev_spans(p, EVAL_THRESHOLDS)[k] == want, t
    # p == float32(t) is accepted exactly where float32 rounds t up (and at t = 0, where the frame is lifted to 1e-7)
    assert accepted == [0.0] + F32_ROUNDS_UP


def test_fixups_and_nan():
    p = np.array([-1.0, 0.0, 1e-7, 1.0, 2.0, np.nan, 0.5, np.nan, -0.0, np.inf, -np.inf, 3e-8], dtype=np.float64)
    thresholds = [0.0, 1e-7, 5e-8, 0.5, 1.0, 0.99]
    for dt in (np.float64, np.float32):
        _check_vs_loop(p.astype(dt), thresholds)
    # threshold 0 accepts the frames that fix_over_underflow lifted to 1e-7, and never a NaN
    assert _dev_spans(p, [0.0])[0] == [(0, 4), (6, 6), (8, 11)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_constructed_tracks(dtype):
    import laugh_segmenter as ls
    tile = _tile()
    thresholds = [0.0, 0.5, 1.0]
    for T in (1, 2, 63, 64, 65, tile, tile + 1, 3 * tile + 7):
        on, off = np.full(T, 0.75, dtype), np.full(T, 0.25, dtype)
        assert _dev_spans(on, thresholds) == [[(0, T - 1)], [(0, T - 1)], []]
        assert _dev_spans(off, thresholds) == [[(0, T - 1)], [], []]
        alt = np.where(np.arange(T) % 2 == 0, 0.75, 0.25).astype(dtype)          # the capacity bound: ceil(T / 2) runs
        assert _dev_spans(alt, [0.5])[0] == [(i, i) for i in range(0, T, 2)]
        alt1 = np.where(np.arange(T) % 2 == 1, 0.75, 0.25).astype(dtype)
        assert _dev_spans(alt1, [0.5])[0] == [(i, i) for i in range(1, T, 2)]
    T = 3 * tile + 70
    edges = list(range(64, T, 64))
    below = np.full(T, 0.25, dtype)
    below[[0, T - 1] + [e - 1 for e in edges]] = 0.75                             # last frame of every wave word / tile
    above = np.full(T, 0.25, dtype)
    above[[0, T - 1] + edges] = 0.75                                              # first frame of every wave word / tile
    both = np.maximum(below, above)                                               # two-frame runs across every edge
    holes = np.full(T, 0.75, dtype)
    holes[[0, T - 1] + edges] = 0.25                                              # runs that end and start at every edge
    long = np.full(T, 0.25, dtype)
    long[tile // 2:2 * tile + tile // 2 + 5] = 0.75                               # one run through two whole tiles
    for p in (below, above, both, holes, long):
        _check_vs_loop(p, thresholds)
        assert _dev_spans(p, [0.5])[0] == [tuple(int(v) for v in r) for r in ls.get_laughter_frame_spans(p, 0.5)]
    assert _dev_spans(long, [0.5])[0] == [(tile // 2, 2 * tile + tile // 2 + 4)]
    assert len(_dev_spans(both, [0.5])[0]) == len(edges) + 2


def test_full_size_track_and_the_87_settings():
    import laugh_segmenter as ls
    p = recipe.make_prob_track(5, 360000).astype(np.float32)
    host = ls.get_laughter_instances(p, thresholds=EVAL_THRESHOLDS, min_lengths=EVAL_MIN_LENGTHS, fps=100.0)
    dev = ls.get_laughter_instances_device(torch.from_numpy(p).cuda(), thresholds=EVAL_THRESHOLDS, min_lengths=EVAL_MIN_LENGTHS,
                                           fps=100.0)
    assert len(dev) == 87 and list(dev.keys()) == list(host.keys())
    for k in host:
        assert dev[k] == host[k], k
    print(f"360,000 frames, 87 settings: {sum(len(v) for v in dev.values())} instances")
    three = [0.1, 0.5, 0.93]
    for thr, g in zip(three, _dev_spans(p, three)):
        assert g == so.run_indices(p, thr), thr
    # an fps that is not a round number (segment_laughter.py:103-104: frames / file length), and duplicate thresholds
    fps = 360000 / 3600.0049375
    thr = [0.5, 0.2, 0.5]
    host = ls.get_laughter_instances(p, thresholds=thr, min_lengths=[0.2, 0.0], fps=fps)
    dev = ls.get_laughter_instances_device(torch.from_numpy(p).cuda(), thresholds=thr, min_lengths=[0.2, 0.0], fps=fps)
    assert list(dev.keys()) == list(host.keys()) and all(dev[k] == host[k] for k in host)


def test_ten_channels_in_one_call_and_identical_bytes():
    import laugh_segmenter as ls
    T = 36000 + 17
    tracks = np.stack([recipe.make_prob_track(40 + c, T) for c in range(10)]).astype(np.float32)
    tracks[3] = 0.0                                                                # a channel without a run above 1e-7
    tracks[7, ::2] = 0.0                                                           # a channel of single frames
    d = torch.from_numpy(tracks).cuda()
    many = ls.get_laughter_frame_spans_device(d, EVAL_THRESHOLDS)
    assert len(many) == 10 and all(len(m) == 29 for m in many)
    for c in range(10):
        one = ls.get_laughter_frame_spans_device(d[c], EVAL_THRESHOLDS)
        for k in range(29):
            assert np.array_equal(many[c][k], one[k]), (c, k)
    for c in (0, 3, 7):
        assert [tuple(int(v) for v in r) for r in many[c][10]] == so.run_indices(tracks[c], EVAL_THRESHOLDS[10])
    counts_a, table_a = ls._device_run_tables(d, EVAL_THRESHOLDS)
    counts_b, table_b = ls._device_run_tables(d, EVAL_THRESHOLDS)
    assert counts_a.tobytes() == counts_b.tobytes() and table_a.tobytes() == table_b.tobytes() and len(table_a) > 1000


def test_errors():
    import _hip
    import laugh_segmenter as ls
    p = torch.rand(1000, device="cuda")
    kmax = int(_hip.lib().lad_runs_max_thresholds())
    assert kmax >= 64
    assert len(ls.get_laughter_frame_spans_device(p, [0.5] * kmax)) == kmax
    with pytest.raises(_hip.LadHipError, match="thresholds"):
        ls.get_laughter_frame_spans_device(p, [0.5] * (kmax + 1))
    with pytest.raises((_hip.LadHipError, ValueError)):
        ls.get_laughter_instances_device(p.cpu())
    with pytest.raises((_hip.LadHipError, ValueError)):
        ls.get_laughter_instances_device(torch.rand(2000, device="cuda")[::2])
    with pytest.raises((_hip.LadHipError, ValueError)):
        ls.get_laughter_instances_device((p * 10).to(torch.int32))
    with pytest.raises((_hip.LadHipError, ValueError)):
        ls.get_laughter_instances_device(p.to(torch.float16))
    with pytest.raises((_hip.LadHipError, ValueError)):
        ls.get_laughter_instances_device(p.view(10, 100))          # one track per call (channels: get_laughter_frame_spans_device)
    # the calls above left the path usable
    assert ls.get_laughter_instances_device(torch.full((300,), 0.9, device="cuda"), [0.5], [0.2], 100.0) == {(0.5, 0.2): [(0.0, 2.99)]}
    assert ls.get_laughter_instances_device(torch.full((1,), 0.9, device="cuda"), [0.5], [0.0], 100.0) == {(0.5, 0.0): []}
    assert ls.get_laughter_instances_device(torch.zeros(0, device="cuda"), [0.5], [0.2], 100.0) == {(0.5, 0.2): []}


def test_capacity_too_small_is_an_error_and_writes_nothing():
    import _hip
    lib = _hip.lib()
    T, K = 5000, 3
    p = torch.from_numpy(np.where(np.arange(T) % 2 == 0, 0.75, 0.25).astype(np.float32)).cuda()      # 2500 runs at 0.5
    thr = (ctypes.c_double * K)(0.2, 0.5, 0.8)
    ws = torch.empty(lib.lad_runs_workspace_bytes(1, T, K), dtype=torch.uint8, device="cuda")
    st = _hip.stream_handle()
    _hip.check(lib.lad_runs_count(_hip.ptr(p), 0, 1, T, thr, K, _hip.ptr(ws), st), "lad_runs_count")
    counts = np.ascontiguousarray(ws[:4 * K].view(torch.int32).cpu().numpy())
    assert counts.tolist() == [1, 2500, 0]
    total, guard = 2501, 64
    cptr = counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    buf = torch.full((total + guard, 2), -7, dtype=torch.int32, device="cuda")
    rc = lib.lad_runs_fill(_hip.ptr(p), 0, 1, T, thr, K, _hip.ptr(ws), cptr, _hip.ptr(buf), total - 1, st)
    assert rc == _hip.LAD_ERR_INVALID and b"2501 runs" in lib.lad_last_error()
    torch.cuda.synchronize()
    assert bool((buf == -7).all())                                                  # nothing was launched
    _hip.check(lib.lad_runs_fill(_hip.ptr(p), 0, 1, T, thr, K, _hip.ptr(ws), cptr, _hip.ptr(buf), total, st), "lad_runs_fill")
    out = buf.cpu().numpy()
    assert (out[total:] == -7).all()                                                # the guard rows behind the table
    assert out[0].tolist() == [0, T - 1] and out[1:total].tolist() == [[i, i] for i in range(0, T, 2)]
    # counts that understate what the workspace holds: the kernel still stops at the capacity
    buf.fill_(-7)
    short = np.array([1, 100, 0], np.int32)
    _hip.check(lib.lad_runs_fill(_hip.ptr(p), 0, 1, T, thr, K, _hip.ptr(ws), short.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                 _hip.ptr(buf), 101, st), "lad_runs_fill")
    out = buf.cpu().numpy()
    assert (out[101:] == -7).all() and out[1:101].tolist() == [[i, i] for i in range(0, 200, 2)]


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
    out = {}
    for dirpath, dirs, files in os.walk(root):
        dirs.sort()
        for f in sorted(files):
            path = os.path.join(dirpath, f)
            out[os.path.relpath(path, root)] = open(path, "rb").read()
    return out


def test_segment_laughter_device_against_host(tmp_path, capsys):
    import segment_laughter
    ck = _checkpoint(tmp_path)
    wav = tmp_path / "chan.wav"
    _write_wav(wav, recipe.make_clips(22, 1, n_samples=16000 * 30)[0])
    trees, lines = {}, {}
    for seg in ("host", "device"):
        segment_laughter.main(["--model_path", ck, "--config", "resnet_base", "--thresholds", ",".join(map(str, EVAL_THRESHOLDS)),
                               "--min_lengths", "0,0.1,0.2", "--input_audio_file", str(wav), "--output_dir", str(tmp_path / seg),
                               "--precision", "fp16", "--save_to_audio_files", "True", "--segmenter", seg,
                               "--save_probs", str(tmp_path / f"{seg}.npy")])
        lines[seg] = capsys.readouterr().out
        assert "87-setting sweep" in lines[seg] and "real-time factor of the whole script" in lines[seg]
        trees[seg] = _tree(tmp_path / seg)
    assert list(trees["host"]) == list(trees["device"])
    assert sum(k.endswith(".TextGrid") for k in trees["host"]) == 87 and any(k.endswith(".wav") for k in trees["host"])
    for k, v in trees["host"].items():
        assert trees["device"][k] == v, k
    assert np.array_equal(np.load(tmp_path / "host.npy"), np.load(tmp_path / "device.npy"))
    found = [l for l in lines["host"].splitlines() if l.startswith("Found ")]
    assert len(found) == 87 and found == [l for l in lines["device"].splitlines() if l.startswith("Found ")]
    # the default is the host sweep
    model = segment_laughter.build_model("resnet_base", ck, torch.device("cuda", 0))
    _, a = segment_laughter.load_and_pred(model, str(wav), [0.5], [0.2], None, save_to_textgrid=False, verbose=False)
    _, b = segment_laughter.load_and_pred(model, str(wav), [0.5], [0.2], None, save_to_textgrid=False, verbose=False,
                                          segmenter="device")
    assert a == b
    with pytest.raises(ValueError):
        segment_laughter.load_and_pred(model, str(wav), [0.5], [0.2], None, segmenter="gpu")


def test_sixteen_million_frames_and_the_largest_threshold_count():
    """2^24 + 3 frames (46 hours at 100 frames/s) and as many thresholds as one call takes: every run count against the host's
    count of starts, four of the tables in full against the host's vectorised pass."""
    import _hip
    import laugh_segmenter as ls
    T = (1 << 24) + 3
    K = int(_hip.lib().lad_runs_max_thresholds())
    p = recipe.make_prob_track(7, T).astype(np.float32)
    thresholds = [float(t) for t in np.linspace(0.0, 1.0, K)]
    got = ls.get_laughter_frame_spans_device(torch.from_numpy(p).cuda(), thresholds)
    fixed = ls.fix_probs(p)
    total = 0
    for k, thr in enumerate(thresholds):
        m = fixed > thr
        assert len(got[k]) == int(m[0]) + int(np.count_nonzero(m[1:] & ~m[:-1])), thr
        total += len(got[k])
        if k in (0, 1, K // 2, K - 2):
            assert np.array_equal(got[k], ls.run_spans(m)), thr
    assert len(got[0]) == 1 and len(got[K - 1]) == 0 and total > 1_000_000
    print(f"{T} frames, {K} thresholds: {total} runs")


def test_four_ranks_with_the_device_segmenter(tmp_path):
    """`--gpus 4 --segmenter device` (the four ranks on device 0 over gloo, as tests/test_data_gpu.py rehearses the sharded script): the
    gathered track stays on the GPU, rank 0 cuts it there; TextGrids and the saved track equal the single-rank host run's."""
    import subprocess
    import sys
    ck = _checkpoint(tmp_path)
    wav = tmp_path / "chan.wav"
    _write_wav(wav, recipe.make_clips(23, 1, n_samples=16000 * 30)[0])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = os.path.join(root, "laughter-detection-icsi_amd", "segment_laughter.py")
    env = dict(os.environ, LAD_REHEARSE_ON_ONE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    got = {}
    for gpus, seg in ((1, "host"), (4, "device")):
        out_dir, npy = tmp_path / f"out_{seg}", tmp_path / f"p_{seg}.npy"
        r = subprocess.run([sys.executable, script, "--model_path", ck, "--config", "resnet_base", "--thresholds", "0.3,0.5",
                            "--min_lengths", "0.0,0.2", "--input_audio_file", str(wav), "--output_dir", str(out_dir),
                            "--precision", "fp16", "--gpus", str(gpus), "--save_probs", str(npy), "--segmenter", seg],
                           capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        assert "4-setting sweep" in r.stdout
        got[seg] = (np.load(npy), _tree(out_dir))
    assert got["host"][0].shape == (3000,) and np.array_equal(got["host"][0], got["device"][0])
    assert len(got["host"][1]) == 4 and got["host"][1] == got["device"][1]
