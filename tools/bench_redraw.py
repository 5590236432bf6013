"""What redrawing the training table costs before an epoch: one lad_sample_segments launch over the whole table, timed in one process:
    python tools/bench_redraw.py [--rows 500000] [--samples 20] [--warmup 3] [--bench-json <file>] [--out profiles/<name>.json]   (GPU box)

Index: 20 synthetic meetings of 4 channels, one hour each, laughs / speech / noise / invalid rows with gaps between them
(sampling.SegmentPools.from_transcripts at the configured frame rate); table: config.SAMPLING['reference'] over all meetings,
repeated to --rows rows (every row has its own row_id, so every row draws its own window).  Per sample, device events around
the one launch of sampling.DrawTable.draw into preallocated outputs, a new epoch each time; median of --samples after --warmup.
--bench-json: the JSON line of `python bench.py` taken on the same box just before; the epoch the draw precedes takes
rows / (its segments per second), and the draw is to stay under 1 % of that.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "laughter-detection-icsi_amd", "utils"), os.path.join(ROOT, "laughter-detection-icsi_amd"), ROOT]


def spread(xs, digits=5):
    return {"min": round(min(xs), digits), "median": round(statistics.median(xs), digits), "max": round(max(xs), digits), "n": len(xs)}


def synthetic_index(meetings=20, parts=4, seconds=3600.0, seed=0):
    """(rows, channels) as sweep_eval.TranscriptIndex takes them."""
    rng = np.random.default_rng(seed)
    rows, chans = [], []
    cycle = (("laugh", 0.3, 2.5), ("speech", 1.0, 6.0), ("noise", 0.2, 1.5), ("speech", 1.0, 4.0), ("invalid", 0.2, 1.0))
    for m in range(meetings):
        mid = f"Bsy{m:03d}"
        for p in range(parts):
            part, chan = f"p{m:03d}{p}", f"chan{p}"
            chans.append({"meeting_id": mid, "part_id": part, "chan": chan, "length": seconds})
            t = float(rng.uniform(0.0, 3.0))
            while True:
                for kind, lo, hi in cycle:
                    length = round(float(rng.uniform(lo, hi)), 3)
                    if t + length > seconds - 2.0:
                        break
                    rows.append({"meeting_id": mid, "part_id": part, "chan": chan, "start": round(t, 3), "end": round(t + length, 3),
                                 "length": length, "type": kind, "laugh_type": "laugh" if kind == "laugh" else ""})
                    t = round(t + length + float(rng.uniform(0.0, 3.0)), 3)
                else:
                    continue
                break
    return rows, chans


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=500000)
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=23)
    ap.add_argument("--bench-json", type=str, default=None, help="file holding the JSON line of bench.py from the same box")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_redraw.py needs an MI355X (a CPU run says nothing about this launch)")
    import bench
    import config
    import sampling
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    fps = config.FEAT["num_samples"]
    T = int(round(config.SAMPLING["reference"]["subsample_duration"] * fps))
    rows, chans = synthetic_index()
    pools = sampling.SegmentPools.from_transcripts(rows, chans, fps, T)
    plan = pools.plan("reference", pools.meetings)
    idx = np.arange(a.rows) % len(plan)
    table = sampling.DrawTable(plan.kind[idx], plan.src[idx], pools.regions, pools.pool_off, pools.pool_cum, pools.pool_total, T, device=dev)
    out = (torch.empty(a.rows, dtype=torch.int32, device=dev), torch.empty(a.rows, dtype=torch.int64, device=dev),
           torch.empty(a.rows, dtype=torch.int32, device=dev))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for i in range(a.warmup + a.samples):
        ev[0].record()
        table.draw(a.seed, i, out=out)
        ev[1].record()
        torch.cuda.synchronize()
        if i >= a.warmup:
            ms.append(ev[0].elapsed_time(ev[1]))
    chan, first, count = (t.cpu().numpy() for t in out)
    assert np.all(first >= 0) and np.all(first + count <= pools.frames[chan]) and np.all(count > 0)     # (it drew windows)
    kinds = np.bincount(plan.kind[idx], minlength=3)
    rec = {"metric": "one redraw of the training table: lad_sample_segments over all rows", "unit": "ms",
           "gpu": torch.cuda.get_device_name(dev), "cpu_model": bench._cpu_model(), "torch": torch.__version__,
           "rows": a.rows, "rows_fixed": int(kinds[0]), "rows_pool_row": int(kinds[1]), "rows_pool_measure": int(kinds[2]),
           "plan_rows_before_repeating": len(plan), "regions": len(pools.regions), "pools": len(pools.pool_names), "meetings": len(pools.meetings),
           "fps": fps, "frames_per_segment": T, "samples": a.samples, "warmup": a.warmup, "timing": "device events around one launch",
           "draw_ms": spread(ms), "bytes_in": int(a.rows * 8), "bytes_out": int(a.rows * 16)}
    if a.bench_json:
        with open(a.bench_json) as f:
            line = [l for l in f.read().splitlines() if l.strip().startswith("{")][-1]
        step = json.loads(line)
        epoch_ms = a.rows / float(step["value"]) * 1e3
        rec["bench_segments_per_s"] = step["value"]
        rec["epoch_ms"] = round(epoch_ms, 1)
        rec["draw_over_epoch"] = round(statistics.median(ms) / epoch_ms, 7)
        rec["bar"] = "draw_ms.median < 0.01 * rows / bench_segments_per_s"
        rec["bar_met"] = bool(statistics.median(ms) < 0.01 * epoch_ms)
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
