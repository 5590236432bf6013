"""The threshold sweep of one 60-minute channel, host against device, in one process:
    python tools/bench_sweep.py [--minutes 60] [--samples 10] [--warmup 2] [--out profiles/<name>.json]      (GPU box)

Track: the fp16 probabilities of bench.py's inference record (synth.make_clips(3600, seed=9876) through its model), 360,000
frames; settings: the 29 thresholds x 3 min_lengths of the evaluation sweep (cluster_scripts/gen_eval_exp.py:30-36).  A second
track with many more runs (oracle.recipe.make_prob_track(5, T) as float32) shows how the legs scale with the run count.
  (a) host leg    device-to-host copy of the track + laugh_segmenter.get_laughter_instances
  (b) device leg  laugh_segmenter.get_laughter_instances_device end to end (launches + counts + table copy + dictionary)
  (c) launches    lad_runs_count (three launches) and lad_runs_fill (one) by device events, buffers allocated beforehand
  (d) channels    ten tracks as one (10, T) call against ten (T,) calls (run tables only)
Legs (a) and (b) alternate within a round; every figure is min / median / max over the samples.  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "laughter-detection-icsi_amd", "utils"), os.path.join(ROOT, "laughter-detection-icsi_amd"), ROOT]

THRESHOLDS = [float(t) for t in np.concatenate((np.linspace(0, 0.9, 19).round(2), np.linspace(0.91, 1, 10).round(2)))]
MIN_LENGTHS = [0.0, 0.1, 0.2]


def spread(xs, digits=6):
    return {"min": round(min(xs), digits), "median": round(statistics.median(xs), digits), "max": round(max(xs), digits), "n": len(xs)}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def launches_ms(probs2d, samples, warmup):
    """(c): device events around the three launches of lad_runs_count and the one of lad_runs_fill."""
    import _hip
    lib = _hip.lib()
    C, T = probs2d.shape
    K = len(THRESHOLDS)
    thr = (ctypes.c_double * K)(*THRESHOLDS)
    ws = torch.empty(lib.lad_runs_workspace_bytes(C, T, K), dtype=torch.uint8, device=probs2d.device)
    st = _hip.stream_handle(probs2d.device)
    _hip.check(lib.lad_runs_count(_hip.ptr(probs2d), 0, C, T, thr, K, _hip.ptr(ws), st), "lad_runs_count")
    counts = np.ascontiguousarray(ws[:4 * C * K].view(torch.int32).cpu().numpy())
    cptr = counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    total = int(counts.sum(dtype=np.int64))
    table = torch.empty((total, 2), dtype=torch.int32, device=probs2d.device)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    count_ms, fill_ms = [], []
    for i in range(warmup + samples):
        ev[0].record()
        _hip.check(lib.lad_runs_count(_hip.ptr(probs2d), 0, C, T, thr, K, _hip.ptr(ws), st), "lad_runs_count")
        ev[1].record()
        _hip.check(lib.lad_runs_fill(_hip.ptr(probs2d), 0, C, T, thr, K, _hip.ptr(ws), cptr, _hip.ptr(table), total, st), "lad_runs_fill")
        ev[2].record()
        torch.cuda.synchronize()
        if i >= warmup:
            count_ms.append(ev[0].elapsed_time(ev[1]))
            fill_ms.append(ev[1].elapsed_time(ev[2]))
    return {"count_ms": spread(count_ms, 4), "fill_ms": spread(fill_ms, 4), "both_ms": spread([a + b for a, b in zip(count_ms, fill_ms)], 4),
            "runs_in_tables": total, "table_bytes": total * 8, "workspace_bytes": ws.numel()}


def legs(probs, samples, warmup):
    """(a) and (b) on one (T,) float32 GPU track, alternating; the two dictionaries must be equal."""
    import laugh_segmenter as ls

    def host():
        return ls.get_laughter_instances(probs.cpu().numpy(), THRESHOLDS, MIN_LENGTHS, 100.0)

    def device():
        return ls.get_laughter_instances_device(probs, THRESHOLDS, MIN_LENGTHS, 100.0)
    host_s, dev_s, copy_s = [], [], []
    for i in range(warmup + samples):
        th, dh = wall(host)
        td, dd = wall(device)
        tc, _ = wall(lambda: probs.cpu().numpy())
        if i == 0:
            assert list(dh.keys()) == list(dd.keys()) and all(dh[k] == dd[k] for k in dh), "device sweep differs from the host sweep"
            n_inst = sum(len(v) for v in dh.values())
        if i >= warmup:
            host_s.append(th)
            dev_s.append(td)
            copy_s.append(tc)
    return {"frames": int(probs.numel()), "settings": len(THRESHOLDS) * len(MIN_LENGTHS), "instances_in_dictionary": n_inst,
            "host_leg_s": spread(host_s), "device_leg_s": spread(dev_s), "track_copy_alone_s": spread(copy_s),
            "identical_dictionaries": True,
            "host_over_device_median": round(statistics.median(host_s) / statistics.median(dev_s), 2),
            "launches": launches_ms(probs.view(1, -1), max(samples, 20), warmup)}


def channels(probs, samples, warmup, C=10):
    """(d): C tracks (the measured one, rotated) as one (C, T) call against C (T,) calls; run tables only."""
    import laugh_segmenter as ls
    many = torch.stack([probs.roll(c * 1009) for c in range(C)]).contiguous()
    one_s, ten_s = [], []
    for i in range(warmup + samples):
        t1, a = wall(lambda: ls.get_laughter_frame_spans_device(many, THRESHOLDS))
        t10, b = wall(lambda: [ls.get_laughter_frame_spans_device(many[c], THRESHOLDS) for c in range(C)])
        if i == 0:
            assert all(np.array_equal(a[c][k], b[c][k]) for c in range(C) for k in range(len(THRESHOLDS)))
        if i >= warmup:
            one_s.append(t1)
            ten_s.append(t10)
    return {"channels": C, "one_call_s": spread(one_s), "calls_per_channel_s": spread(ten_s),
            "launches_one_call": launches_ms(many, max(samples, 20), warmup)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_sweep.py needs an MI355X (a CPU run says nothing about these legs)")
    import bench
    import config
    import synth
    from oracle import recipe
    from utils import get_feat_extractor
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ex = get_feat_extractor(config.FEAT["num_samples"], config.FEAT["num_filters"])
    model = bench._make_model(0.0, dev, degenerate_ok=False)
    model.eval()
    seconds = int(a.minutes * 60)
    pcm = synth.make_clips(seconds, seed=9876, device=dev).view(-1)
    feats = ex.extract_long(pcm)
    model.engine.predict_windows(feats, precision="fp16")                        # (warm-up: buffers)
    model_s, probs = wall(lambda: model.engine.predict_windows(ex.extract_long(pcm), precision="fp16").clone())
    del pcm, feats
    rec = {"metric": "87-setting threshold sweep of one channel: host leg against device leg", "unit": "s",
           "gpu": torch.cuda.get_device_name(dev), "cpu_model": bench._cpu_model(), "host_cores": os.cpu_count(),
           "torch": torch.__version__, "minutes": a.minutes, "thresholds": len(THRESHOLDS), "min_lengths": len(MIN_LENGTHS),
           "model_pass_fp16_s": round(model_s, 4), "samples": a.samples, "warmup": a.warmup,
           "model_track": legs(probs, a.samples, a.warmup),
           "recipe_track": legs(torch.from_numpy(recipe.make_prob_track(5, probs.numel()).astype(np.float32)).to(dev), a.samples, a.warmup),
           "ten_channels_model_track": channels(probs, a.samples, a.warmup)}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
