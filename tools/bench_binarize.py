"""What hysteresis and gap filling cost on top of the plain threshold sweep of one 60-minute channel, in one process:
    python tools/bench_binarize.py [--minutes 60] [--samples 5] [--warmup 1] [--out profiles/<name>.json]      (GPU box)

Tracks: the fp16 probabilities of bench.py's inference record (synth.make_clips(3600, seed=9876) through its model), 360,000
frames, and oracle.recipe.make_prob_track(5, T) as float32, which has many more runs.  Settings: the 29 thresholds x 3 min_lengths
of the evaluation sweep (cluster_scripts/gen_eval_exp.py:30-36), and for the binarized sweep 3 offset drops x 3 minimum gaps on
top of them (261 run tables in five rounds of at most lad_binarize_max_settings()).
  (a) plain device leg      laugh_segmenter.get_laughter_instances_device: 29 run tables, 87 dictionary entries
  (b) binarized device leg  laugh_segmenter.binarize_instances_device: 261 event tables, 783 dictionary entries
  (c) binarized host leg    device-to-host copy of the track + laugh_segmenter.binarize_instances of the same settings
  (d) launches              one round of 64 settings, lad_binarize_count (three launches) and lad_binarize_fill (four) by device
                            events, buffers allocated beforehand, next to lad_runs_count + lad_runs_fill of the 29 thresholds
The legs alternate within a round after the warm-ups; every figure is min / median / max over the samples.  No target is set: the
record says what (b) cost relative to (a) on the same track in the same process.  Prints one JSON line."""
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
OFFSET_DROPS = [0.0, 0.1, 0.2]
MIN_GAPS = [0.0, 0.1, 0.3]


def spread(xs, digits=6):
    return {"min": round(min(xs), digits), "median": round(statistics.median(xs), digits), "max": round(max(xs), digits), "n": len(xs)}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def launches_ms(probs2d, samples, warmup):
    """(d): device events around the two steps of each sweep, one round each."""
    import _hip
    import laugh_segmenter as ls
    lib = _hip.lib()
    C, T = probs2d.shape
    dev = probs2d.device
    st = _hip.stream_handle(dev)
    i32p, f64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    # the plain sweep of the 29 thresholds
    K = len(THRESHOLDS)
    thr = (ctypes.c_double * K)(*THRESHOLDS)
    ws = torch.empty(lib.lad_runs_workspace_bytes(C, T, K), dtype=torch.uint8, device=dev)
    _hip.check(lib.lad_runs_count(_hip.ptr(probs2d), 0, C, T, thr, K, _hip.ptr(ws), st), "lad_runs_count")
    counts = np.ascontiguousarray(ws[:4 * C * K].view(torch.int32).cpu().numpy())
    total = int(counts.sum(dtype=np.int64))
    table = torch.empty((max(total, 1), 2), dtype=torch.int32, device=dev)
    # one round of the binarized sweep: the first lad_binarize_max_settings() of the 261 settings
    _, settings = ls.HYSTERESIS.keys(THRESHOLDS, (OFFSET_DROPS, MIN_GAPS), {})
    settings = settings[:int(lib.lad_binarize_max_settings())]
    B = len(settings)
    cols = [(ctypes.c_double * B)(*[s[j] for s in settings]) for j in range(3)]
    fps_host = np.full(C, 100.0)
    fps_dev = torch.from_numpy(fps_host).to(dev)
    bws = torch.empty(lib.lad_binarize_workspace_bytes(C, T, B), dtype=torch.uint8, device=dev)
    _hip.check(lib.lad_binarize_count(_hip.ptr(probs2d), 0, C, T, cols[0], cols[1], B, _hip.ptr(bws), st), "lad_binarize_count")
    bcounts = np.ascontiguousarray(bws[:4 * C * B].view(torch.int32).cpu().numpy())
    btotal = int(bcounts.sum(dtype=np.int64))
    both = torch.empty((2, max(btotal, 1), 2), dtype=torch.int32, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    plain_ms, count_ms, fill_ms = [], [], []
    for i in range(warmup + samples):
        ev[0].record()
        _hip.check(lib.lad_runs_count(_hip.ptr(probs2d), 0, C, T, thr, K, _hip.ptr(ws), st), "lad_runs_count")
        _hip.check(lib.lad_runs_fill(_hip.ptr(probs2d), 0, C, T, thr, K, _hip.ptr(ws), counts.ctypes.data_as(i32p), _hip.ptr(table),
                                     total, st), "lad_runs_fill")
        ev[1].record()
        ev[2].record()
        _hip.check(lib.lad_binarize_count(_hip.ptr(probs2d), 0, C, T, cols[0], cols[1], B, _hip.ptr(bws), st), "lad_binarize_count")
        ev[3].record()
        _hip.check(lib.lad_binarize_fill(_hip.ptr(probs2d), 0, C, T, cols[0], cols[1], cols[2], B, _hip.ptr(fps_dev),
                                         fps_host.ctypes.data_as(f64p), _hip.ptr(bws), bcounts.ctypes.data_as(i32p), _hip.ptr(both[0]),
                                         _hip.ptr(both[1]), btotal, st), "lad_binarize_fill")
        ev[4].record()
        torch.cuda.synchronize()
        if i >= warmup:
            plain_ms.append(ev[0].elapsed_time(ev[1]))
            count_ms.append(ev[2].elapsed_time(ev[3]))
            fill_ms.append(ev[3].elapsed_time(ev[4]))
    merged = int(bws[:4 * C * B].view(torch.int32).sum().item())
    return {"plain_29_thresholds_count_and_fill_ms": spread(plain_ms, 4), "plain_runs_in_tables": total,
            "binarize_settings_in_round": B, "binarize_count_ms": spread(count_ms, 4), "binarize_fill_ms": spread(fill_ms, 4),
            "binarize_both_ms": spread([a + b for a, b in zip(count_ms, fill_ms)], 4), "hysteresis_runs_in_tables": btotal,
            "merged_runs_in_tables": merged, "binarize_workspace_bytes": bws.numel()}


def legs(probs, samples, warmup):
    """(a), (b) and (c) on one (T,) float32 GPU track, alternating; (b) and (c) must give the same dictionary."""
    import laugh_segmenter as ls

    def plain():
        return ls.get_laughter_instances_device(probs, THRESHOLDS, MIN_LENGTHS, 100.0)

    def device():
        return ls.binarize_instances_device(probs, THRESHOLDS, MIN_LENGTHS, 100.0, OFFSET_DROPS, MIN_GAPS)

    def host():
        return ls.binarize_instances(probs.cpu().numpy(), THRESHOLDS, MIN_LENGTHS, 100.0, OFFSET_DROPS, MIN_GAPS)
    plain_s, dev_s, host_s = [], [], []
    for i in range(warmup + samples):
        tp, dp = wall(plain)
        td, dd = wall(device)
        th, dh = wall(host)
        if i == 0:
            assert list(dh.keys()) == list(dd.keys()) and all(dh[k] == dd[k] for k in dh), "device binarization differs from the host's"
            assert all(dd[(t, 0.0, 0.0, l)] == dp[(t, l)] for t in THRESHOLDS for l in MIN_LENGTHS), "drop 0, gap 0 is not the plain sweep"
            n_plain, n_bin = sum(len(v) for v in dp.values()), sum(len(v) for v in dd.values())
        if i >= warmup:
            plain_s.append(tp)
            dev_s.append(td)
            host_s.append(th)
    n_tables = len(THRESHOLDS) * len(OFFSET_DROPS) * len(MIN_GAPS)
    return {"frames": int(probs.numel()), "plain_tables": len(THRESHOLDS), "binarized_tables": n_tables,
            "plain_instances_in_dictionary": n_plain, "binarized_instances_in_dictionary": n_bin,
            "plain_device_leg_s": spread(plain_s), "binarized_device_leg_s": spread(dev_s), "binarized_host_leg_s": spread(host_s),
            "identical_dictionaries": True,
            "binarized_over_plain_device_median": round(statistics.median(dev_s) / statistics.median(plain_s), 2),
            "binarized_device_per_table_over_plain_per_table_median":
                round(statistics.median(dev_s) / n_tables / (statistics.median(plain_s) / len(THRESHOLDS)), 2),
            "binarized_host_over_device_median": round(statistics.median(host_s) / statistics.median(dev_s), 2),
            "launches": launches_ms(probs.view(1, -1), max(samples, 20), warmup)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_binarize.py needs an MI355X (a CPU run says nothing about these legs)")
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
    model.engine.predict_windows(ex.extract_long(pcm), precision="fp16")         # (warm-up: buffers)
    probs = model.engine.predict_windows(ex.extract_long(pcm), precision="fp16").clone()
    del pcm
    rec = {"metric": "threshold sweep of one channel with hysteresis and gap filling against the plain device sweep", "unit": "s",
           "gpu": torch.cuda.get_device_name(dev), "cpu_model": bench._cpu_model(), "host_cores": os.cpu_count(),
           "torch": torch.__version__, "minutes": a.minutes, "thresholds": len(THRESHOLDS), "min_lengths": len(MIN_LENGTHS),
           "offset_drops": OFFSET_DROPS, "min_gaps": MIN_GAPS, "samples": a.samples, "warmup": a.warmup,
           "model_track": legs(probs, a.samples, a.warmup),
           "recipe_track": legs(torch.from_numpy(recipe.make_prob_track(5, probs.numel()).astype(np.float32)).to(dev), a.samples, a.warmup)}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
