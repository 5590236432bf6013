"""The confidence of every instance of a 60-minute channel's evaluation sweep, host against device, in one process:
    python tools/bench_spanstats.py [--minutes 60] [--samples 5] [--warmup 1] [--out profiles/<name>.json]      (GPU box)

Settings: the 29 thresholds x 3 min_lengths of the evaluation sweep.  Tracks of 360,000 frames as float32: the fp16 probabilities
of bench.py's inference record (synth.make_clips(3600, seed=9876) through its model), oracle.recipe.make_prob_track(5, T), and a
constant track at 1.0 -- one span as long as the track at every threshold below 1, the case the bound on reads per row exists for.
  (A) host leg     the device sweep of get_laughter_instances_device + a copy of the track to the host + laugh_segmenter.span_stats
                   on every threshold's list of spans (the public host form: it fixes and sums the track once per list)
  (B) device leg   get_laughter_instances_device(..., stats=True): prepare once, lad_span_stats on the round's table
  (C) as it stands get_laughter_instances_device without statistics: (B) - (C) is what they add
  kernels          lad_span_stats_prepare (five launches) and lad_span_stats (one copy, one launch) alone, by device events, on the
                   tables of the 29 thresholds
The legs alternate within a round after the warm-ups; every figure is min / median / max over the samples.  The first round checks
that (A) and (B) return the same figures.  No target is set.  Prints one JSON line."""
import argparse
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
FPS = 100.0


def spread(xs, digits=6):
    return {"min": round(min(xs), digits), "median": round(statistics.median(xs), digits), "max": round(max(xs), digits), "n": len(xs)}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def kernels_ms(probs, samples, warmup):
    """Device events around lad_span_stats_prepare and around lad_span_stats on the tables of THRESHOLDS, buffers allocated beforehand."""
    import _hip
    import laugh_segmenter as ls
    import spanstats
    lib = _hip.lib()
    track, dtype, _ = ls.device_track(probs)
    C, T = track.shape
    _, table, counts, _ = ls._device_tables(ls.THRESHOLD, track, dtype, THRESHOLDS, {})
    total = int(counts.sum())
    ws = torch.empty(lib.lad_span_stats_workspace_bytes(C, T), dtype=torch.uint8, device=track.device)
    sums = torch.empty(max(total, 1), dtype=torch.int64, device=track.device)
    peaks = torch.empty(max(total, 1), dtype=torch.int32, device=track.device)
    values = torch.empty(max(total, 1), dtype=torch.float64, device=track.device)
    st = _hip.stream_handle(track.device)
    cptr = counts.ctypes.data_as(spanstats._I32P)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    prep, rows = [], []
    for i in range(warmup + samples):
        ev[0].record()
        _hip.check(lib.lad_span_stats_prepare(_hip.ptr(track), dtype, C, T, _hip.ptr(ws), st), "lad_span_stats_prepare")
        ev[1].record()
        _hip.check(lib.lad_span_stats(_hip.ptr(track), dtype, C, T, _hip.ptr(ws), _hip.ptr(table), cptr, len(THRESHOLDS), _hip.ptr(sums),
                                      _hip.ptr(peaks), _hip.ptr(values), st), "lad_span_stats")
        ev[2].record()
        torch.cuda.synchronize()
        if i >= warmup:
            prep.append(ev[0].elapsed_time(ev[1]))
            rows.append(ev[1].elapsed_time(ev[2]))
    longest = int((table[:total, 1] - table[:total, 0]).max().item()) + 1 if total else 0
    return {"rows": total, "longest_span_frames": longest, "prepare_ms": spread(prep, 4), "span_stats_ms": spread(rows, 4)}


def legs(probs, samples, warmup):
    """(A), (B) and (C) on one (T,) float32 GPU track, the legs alternating."""
    import laugh_segmenter as ls

    def host():
        lists = ls.get_laughter_frame_spans_device(probs, THRESHOLDS)            # (the sweep of get_laughter_instances_device)
        x = probs.cpu().numpy()
        return ls._instances_from_spans([(thr,) for thr in THRESHOLDS], lists, MIN_LENGTHS, FPS, [ls.span_stats(x, s) for s in lists])

    def device():
        return ls.get_laughter_instances_device(probs, THRESHOLDS, MIN_LENGTHS, FPS, stats=True)

    def plain():
        return ls.get_laughter_instances_device(probs, THRESHOLDS, MIN_LENGTHS, FPS)
    a_s, b_s, c_s = [], [], []
    for i in range(warmup + samples):
        ta, fa = wall(host)
        tb, fb = wall(device)
        tc, fc = wall(plain)
        if i == 0:
            assert fa[0] == fb[0] == fc, "the three legs cut different instances"
            assert all(fa[1][k].tobytes() == fb[1][k].tobytes() for k in fc), "the device statistics differ from the host's"
        if i >= warmup:
            a_s.append(ta)
            b_s.append(tb)
            c_s.append(tc)
    return {"frames": int(probs.numel()), "instances": int(sum(len(v) for v in fc.values())),
            "A_host_leg_s": spread(a_s), "B_device_leg_s": spread(b_s), "C_without_stats_s": spread(c_s), "identical_figures": True,
            "B_minus_C_median_s": round(statistics.median(b_s) - statistics.median(c_s), 6),
            "A_over_B_median": round(statistics.median(a_s) / statistics.median(b_s), 2),
            "kernels": kernels_ms(probs, max(samples, 20), warmup)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_spanstats.py needs an MI355X (a CPU run says nothing about these legs)")
    import _hip
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
    T = probs.numel()
    made = torch.from_numpy(recipe.make_prob_track(5, T).astype(np.float32)).to(dev)
    ones = torch.ones(T, dtype=torch.float32, device=dev)
    lib = _hip.lib()
    rec = {"metric": "confidence of every instance of the evaluation sweep: span_stats on the host after a copy of the track against "
                     "get_laughter_instances_device(stats=True)",
           "unit": "s", "gpu": torch.cuda.get_device_name(dev), "cpu_model": bench._cpu_model(), "host_cores": os.cpu_count(),
           "torch": torch.__version__, "minutes": a.minutes, "thresholds": len(THRESHOLDS), "min_lengths": len(MIN_LENGTHS),
           "samples": a.samples, "warmup": a.warmup, "tile_frames": int(lib.lad_span_stats_tile_frames()),
           "prepare_launches": 5, "span_stats_launches": 1,
           "prefix_reads_per_row": 2, "tree_reads_per_row_bound": 3 * int(np.ceil(np.log2(max(T, 2)))) + 2,
           "model_track": legs(probs, a.samples, a.warmup), "recipe_track": legs(made, a.samples, a.warmup),
           "constant_track": legs(ones, a.samples, a.warmup)}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
