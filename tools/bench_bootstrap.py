"""Bootstrap intervals of the sweep's summary, host form against device form, in one process:
    python tools/bench_bootstrap.py [--replicates 2000] [--samples 5] [--warmup 1] [--out profiles/bootstrap.json]      (GPU box)

Inputs are SYNTHETIC: seeded score arrays of realistic size (a unit predicts up to 60 minutes in milliseconds, a fraction of it
correct; 5 to 15 minutes of transcribed laughter per unit), every channel its own unit, behind a stand-in for the transcript index
that answers the two questions the bootstrap asks of it.  No track is scored here: the bootstrap starts from the scorers' integers.
Shapes: G = 20 and 450 units; 87 cells (29 thresholds x 3 min_lengths), 783 cells (the 29 x 3 x 3 x 3 hysteresis sweep) and 12,291
cells (the dense surface: 4,097 levels x 3 min_lengths).
  (A) host leg     sweep_eval.bootstrap_sum_stats_host: numpy Philox, an int64 matmul without BLAS, Python integers for the order
  (B) device leg   sweep_eval.bootstrap_sum_stats_device, by the host clock around a call that ends with the rows on the host
  kernels          lad_bootstrap_weights, lad_bootstrap_sums and lad_bootstrap_quantiles alone, by device events, on the time
                   matrix of the shape (2 columns a cell and the shared one, 3 figures a cell)
The legs alternate within a round after the warm-ups; every figure is min / median / max over the samples.  Where the first host
call takes longer than --host_budget_s the host leg is timed ONCE, by that call, without a warm-up, and the record says so.  Every host sample is compared with the device rows of the same round.  There is no parent figure: the commit before
this one cannot compute any of this, so the host form on the same box is the only baseline.  No target is set.  Prints one JSON line."""
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
SHAPES = [("sweep_87_cells", dict(thresholds=THRESHOLDS)),
          ("hysteresis_783_cells", dict(thresholds=THRESHOLDS, offset_drops=[0.0, 0.1, 0.2], min_gaps=[0.0, 0.1, 0.2])),
          ("dense_12291_cells", dict(thresholds=[i / 4096 for i in range(4097)]))]


class UnitIndex:
    """What sweep_eval.bootstrap_units asks of a TranscriptIndex, for synthetic units: every channel has a participant and so many
    milliseconds of transcribed laughter."""

    def __init__(self, transc_ms):
        self.ms = {f"p{g}": int(v) for g, v in enumerate(transc_ms)}

    def participant(self, meeting_id, chan):
        return "p" + chan[4:]

    def laugh_ms(self, meeting_id, part_id=None):
        return self.ms[part_id] if part_id is not None else sum(v for p, v in self.ms.items() if p == "p" + meeting_id[1:])


def spread(xs, digits=6):
    return {"min": round(min(xs), digits), "median": round(statistics.median(xs), digits), "max": round(max(xs), digits), "n": len(xs)}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def make_scores(seed, G, shape):
    rng = np.random.default_rng(seed)
    scores = np.zeros((G, *shape, 7), np.int64)
    scores[..., 2] = rng.integers(0, 3_600_000, (G, *shape))
    scores[..., 3] = (scores[..., 2] * rng.random((G, *shape)) * 0.3).astype(np.int64)
    return scores, rng.integers(300_000, 900_000, G)


def same(a, b):
    return len(a) == len(b) and all(len(x) == len(y) and all(p == q or (p != p and q != q) for p, q in zip(x, y)) for x, y in zip(a, b))


def kernels_ms(G, n_cells, B, samples, warmup):
    import _hip
    import bootstrap
    lib = _hip.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    M = 2 * n_cells + 1
    x = torch.from_numpy(np.random.default_rng(1).integers(0, 3_600_000, (G, M))).to(dev)
    w = torch.empty((B, G), dtype=torch.int32, device=dev)
    sums = torch.empty((B, M), dtype=torch.int64, device=dev)
    template = [(1, 1, 0, None, None, 1), (1, 1, bootstrap.SHARED, None, None, 0), (1, 2, 0, bootstrap.SHARED, bootstrap.SHARED, 0)]
    fh = np.asarray([f for c in range(n_cells) for f in bootstrap.cell_figures(template, c, 2, M - 1)], np.int32)
    fd = torch.from_numpy(fh).to(dev)
    out = torch.empty((len(fh), 2, 2), dtype=torch.int64, device=dev)
    valid = torch.empty(len(fh), dtype=torch.int32, device=dev)
    i32 = bootstrap.ctypes.c_int32
    qn, qd = (i32 * 2)(1, 39), (i32 * 2)(40, 40)
    st = _hip.stream_handle(dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    t_w, t_s, t_q = [], [], []
    for i in range(warmup + samples):
        ev[0].record()
        _hip.check(lib.lad_bootstrap_weights(G, B, 0, _hip.ptr(w), st), "lad_bootstrap_weights")
        ev[1].record()
        _hip.check(lib.lad_bootstrap_sums(_hip.ptr(x), _hip.ptr(w), G, M, B, _hip.ptr(sums), st), "lad_bootstrap_sums")
        ev[2].record()
        _hip.check(lib.lad_bootstrap_quantiles(_hip.ptr(sums), M, B, _hip.ptr(fd), fh.ctypes.data_as(bootstrap.ctypes.POINTER(i32)), len(fh), qn,
                                               qd, 2, _hip.ptr(out), _hip.ptr(valid), st), "lad_bootstrap_quantiles")
        ev[3].record()
        torch.cuda.synchronize()
        if i >= warmup:
            t_w.append(ev[0].elapsed_time(ev[1]))
            t_s.append(ev[1].elapsed_time(ev[2]))
            t_q.append(ev[2].elapsed_time(ev[3]))
    macs = float(B) * G * M
    return {"columns": M, "figures": len(fh), "weights_ms": spread(t_w, 4), "sums_ms": spread(t_s, 4), "quantiles_ms": spread(t_q, 4),
            "sums_multiply_adds": macs, "sums_tera_multiply_adds_per_s_at_median": round(macs / (statistics.median(t_s) * 1e-3) / 1e12, 3)}


def legs(G, name, axes, B, samples, warmup, host_budget_s):
    import laugh_segmenter as ls
    import sweep_eval as se
    lists = {k: v for k, v in axes.items() if k != "thresholds"}
    thresholds = axes["thresholds"]
    shape = se._score_shape(G, thresholds, MIN_LENGTHS, ls.decoder_for(lists.get("offset_drops"), lists.get("min_gaps"), None)[1])[1:-1]
    n_cells = int(np.prod(shape))
    scores, transc = make_scores(G * 100003 + n_cells, G, shape)
    channels = [(f"m{g}", f"chan{g}") for g in range(G)]
    index = UnitIndex(transc)

    def host():
        return se.bootstrap_sum_stats_host(scores, channels, thresholds, MIN_LENGTHS, index, n_boot=B, seed=0, **lists)

    def device():
        return se.bootstrap_sum_stats_device(scores, channels, thresholds, MIN_LENGTHS, index, n_boot=B, seed=0, **lists)
    once = False
    a_s, b_s = [], []
    for i in range(warmup + samples):
        tb, rows = wall(device)
        if not once:
            ta, want = wall(host)
            assert same(rows, want), f"{name}, G = {G}: the device rows differ from the host's"
            if i == 0 and ta > host_budget_s:
                once, a_s = True, [ta]                                             # (the first call is the one sample)
            elif i >= warmup:
                a_s.append(ta)
        if i >= warmup:
            b_s.append(tb)
    widths = [r[4] - r[3] for r in rows if r[4] == r[4]]
    return {"units": G, "cells": n_cells, "replicates": B, "A_host_leg_s": spread(a_s), "host_timed_once_without_warmup": once,
            "B_device_leg_s": spread(b_s), "identical_rows": True, "A_over_B_median": round(statistics.median(a_s) / statistics.median(b_s), 2),
            "median_precision_interval_width": round(statistics.median(widths), 6) if widths else None,
            "kernels": kernels_ms(G, n_cells, B, max(samples, 20), warmup)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicates", type=int, default=2000)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host_budget_s", type=float, default=20.0, help="a host sample estimated to take longer is taken once")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_bootstrap.py needs an MI355X (a CPU run says nothing about these legs)")
    import bench
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rec = {"metric": "bootstrap intervals of precision, recall and F1 for every cell of a sweep: sweep_eval.bootstrap_sum_stats_host against "
                     "sweep_eval.bootstrap_sum_stats_device, both ending with the rows on the host",
           "unit": "s", "inputs": "synthetic seeded unit scores of realistic size; no track is scored", "gpu": torch.cuda.get_device_name(dev),
           "cpu_model": bench._cpu_model(), "host_cores": os.cpu_count(), "torch": torch.__version__, "numpy": np.__version__,
           "samples": a.samples, "warmup": a.warmup, "host_budget_s": a.host_budget_s, "baseline": "the host form on the same box (no parent figure exists)",
           "shapes": {}}
    for name, axes in SHAPES:
        for G in (20, 450):
            rec["shapes"][f"{name}_G{G}"] = legs(G, name, axes, a.replicates, a.samples, a.warmup, a.host_budget_s)
            print(f"{name} G={G}: {json.dumps(rec['shapes'][f'{name}_G{G}'])}", file=sys.stderr, flush=True)
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
