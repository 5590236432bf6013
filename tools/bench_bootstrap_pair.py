"""Paired bootstrap of two systems (the interval of A - B for every cell of a sweep), host form against device form, in one process:
    python tools/bench_bootstrap_pair.py [--replicates 2000] [--samples 5] [--warmup 1] [--out profiles/bootstrap_pair.json]    (GPU box)

In the manner of tools/bench_bootstrap.py, whose synthetic inputs, stand-in transcript index and helpers it uses: system A is that
tool's seeded score array, system B the same predictions with between 90 and 110 per cent of A's correct time (never more than
predicted), so the two are close, as two checkpoints are.  No track is scored here.
Shapes: G = 20 and 450 units; 87 cells (29 thresholds x 3 min_lengths) and 783 cells (the 29 x 3 x 3 x 3 hysteresis sweep).
  (A) host leg     sweep_eval.bootstrap_diff_sum_stats_host: numpy Philox, an int64 matmul without BLAS, Python integers for the order
  (B) device leg   sweep_eval.bootstrap_diff_sum_stats_device, by the host clock around a call that ends with the rows on the host
  kernel           lad_bootstrap_pair_quantiles alone, by device events, on the sums of the shape's paired time matrix (4 columns a
                   cell and the shared one, 3 differences a cell), next to lad_bootstrap_quantiles on the same sums for system A's
                   3 figures a cell: what the 256-bit order costs over the 128-bit one
The legs alternate within a round after the warm-ups; every figure is min / median / max over the samples.  Where the first host
call takes longer than --host_budget_s the host leg is timed ONCE, by that call, without a warm-up, and the record says so.  Every
host sample is compared with the device rows of the same round.  There is no parent figure: the commit before this one cannot compute
any of this, so the host form on the same box is the only baseline.  No target is set.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_bootstrap as bb  # noqa: E402  (puts the package on sys.path)

SHAPES = bb.SHAPES[:2]


def make_pair(seed, G, shape):
    scores_a, transc = bb.make_scores(seed, G, shape)
    rng = np.random.default_rng(seed + 1)
    scores_b = scores_a.copy()
    scores_b[..., 3] = np.minimum((scores_a[..., 3] * rng.uniform(0.9, 1.1, (G, *shape))).astype(np.int64), scores_a[..., 2])
    return scores_a, scores_b, transc


def kernel_ms(G, n_cells, B, samples, warmup):
    import _hip
    import bootstrap
    import sweep_eval as se
    lib = _hip.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    M = 4 * n_cells + 1
    x = torch.from_numpy(np.random.default_rng(1).integers(0, 3_600_000, (G, M))).to(dev)
    sums = bootstrap.sums_device(x, bootstrap.weights_device(G, B, 0, dev))
    ph = np.asarray([bootstrap._flat_pair(p) for c in range(n_cells) for p in bootstrap.pair_cell_figures(se._TIME_DIFFS, c, 2, n_cells, M - 1)],
                    np.int32)
    fh = np.asarray([f for c in range(n_cells) for f in bootstrap.cell_figures(se._TIME_FIGURES, c, 2, M - 1)], np.int32)
    pd, fd = torch.from_numpy(ph).to(dev), torch.from_numpy(fh).to(dev)
    out = torch.empty((len(ph), 2, 4), dtype=torch.int64, device=dev)
    valid = torch.empty(len(ph), dtype=torch.int32, device=dev)
    signs = torch.empty((len(ph), 3), dtype=torch.int32, device=dev)
    i32 = bootstrap.ctypes.c_int32
    i32p = bootstrap.ctypes.POINTER(i32)
    qn, qd = (i32 * 2)(1, 39), (i32 * 2)(40, 40)
    st = _hip.stream_handle(dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    t_p, t_q = [], []
    for i in range(warmup + samples):
        ev[0].record()
        _hip.check(lib.lad_bootstrap_pair_quantiles(_hip.ptr(sums), M, B, _hip.ptr(pd), ph.ctypes.data_as(i32p), len(ph), qn, qd, 2, _hip.ptr(out),
                                                    _hip.ptr(valid), _hip.ptr(signs), st), "lad_bootstrap_pair_quantiles")
        ev[1].record()
        _hip.check(lib.lad_bootstrap_quantiles(_hip.ptr(sums), M, B, _hip.ptr(fd), fh.ctypes.data_as(i32p), len(fh), qn, qd, 2, _hip.ptr(out),
                                               _hip.ptr(valid), st), "lad_bootstrap_quantiles")
        ev[2].record()
        torch.cuda.synchronize()
        if i >= warmup:
            t_p.append(ev[0].elapsed_time(ev[1]))
            t_q.append(ev[1].elapsed_time(ev[2]))
    return {"columns": M, "pairs": len(ph), "pair_quantiles_ms": bb.spread(t_p, 4), "figures": len(fh), "quantiles_ms_same_sums": bb.spread(t_q, 4),
            "pair_over_single_median": round(statistics.median(t_p) / statistics.median(t_q), 2)}


def legs(G, name, axes, B, samples, warmup, host_budget_s):
    import laugh_segmenter as ls
    import sweep_eval as se
    lists = {k: v for k, v in axes.items() if k != "thresholds"}
    thresholds = axes["thresholds"]
    shape = se._score_shape(G, thresholds, bb.MIN_LENGTHS, ls.decoder_for(lists.get("offset_drops"), lists.get("min_gaps"), None)[1])[1:-1]
    n_cells = int(np.prod(shape))
    scores_a, scores_b, transc = make_pair(G * 100003 + n_cells, G, shape)
    channels = [(f"m{g}", f"chan{g}") for g in range(G)]
    index = bb.UnitIndex(transc)

    def host():
        return se.bootstrap_diff_sum_stats_host(scores_a, scores_b, channels, thresholds, bb.MIN_LENGTHS, index, n_boot=B, seed=0, **lists)

    def device():
        return se.bootstrap_diff_sum_stats_device(scores_a, scores_b, channels, thresholds, bb.MIN_LENGTHS, index, n_boot=B, seed=0, **lists)
    once = False
    a_s, b_s = [], []
    for i in range(warmup + samples):
        tb, rows = bb.wall(device)
        if not once:
            ta, want = bb.wall(host)
            assert bb.same(rows, want), f"{name}, G = {G}: the device rows differ from the host's"
            if i == 0 and ta > host_budget_s:
                once, a_s = True, [ta]                                             # (the first call is the one sample)
            elif i >= warmup:
                a_s.append(ta)
        if i >= warmup:
            b_s.append(tb)
    single = se.bootstrap_sum_stats_device(scores_a, channels, thresholds, bb.MIN_LENGTHS, index, n_boot=B, seed=0, **lists)
    n_keys = len(rows[0]) - 19
    paired = [r[n_keys + 4] - r[n_keys + 3] for r in rows if r[n_keys + 4] == r[n_keys + 4]]
    alone = [r[n_keys + 2] - r[n_keys + 1] for r in single if r[n_keys + 2] == r[n_keys + 2]]
    return {"units": G, "cells": n_cells, "replicates": B, "A_host_leg_s": bb.spread(a_s), "host_timed_once_without_warmup": once,
            "B_device_leg_s": bb.spread(b_s), "identical_rows": True, "A_over_B_median": round(statistics.median(a_s) / statistics.median(b_s), 2),
            "median_precision_diff_interval_width": round(statistics.median(paired), 6) if paired else None,
            "median_precision_interval_width_of_A_alone": round(statistics.median(alone), 6) if alone else None,
            "kernel": kernel_ms(G, n_cells, B, max(samples, 20), warmup)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicates", type=int, default=2000)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host_budget_s", type=float, default=20.0, help="a host sample estimated to take longer is taken once")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_bootstrap_pair.py needs an MI355X (a CPU run says nothing about these legs)")
    import bench
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rec = {"metric": "paired bootstrap intervals of the difference A - B of precision, recall and F1 for every cell of a sweep: "
                     "sweep_eval.bootstrap_diff_sum_stats_host against sweep_eval.bootstrap_diff_sum_stats_device, both ending with the rows "
                     "on the host",
           "unit": "s", "inputs": "synthetic seeded unit scores of realistic size for two close systems; no track is scored",
           "gpu": torch.cuda.get_device_name(dev), "cpu_model": bench._cpu_model(), "host_cores": os.cpu_count(), "torch": torch.__version__,
           "numpy": np.__version__, "samples": a.samples, "warmup": a.warmup, "host_budget_s": a.host_budget_s,
           "baseline": "the host form on the same box (no parent figure exists)", "shapes": {}}
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
