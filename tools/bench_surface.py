"""The dense threshold sweep of one 60-minute channel, run-table rounds against the component tree, in one process:
    python tools/bench_surface.py [--minutes 60] [--samples 5] [--warmup 1] [--intervals 3000] [--out profiles/surface_60min.json]   (GPU box)

Tracks: the fp16 probabilities of bench.py's inference record (synth.make_clips(3600, seed=9876) through its model), 360,000 frames,
and oracle.recipe.make_prob_track(5, T) as float32 (many more runs); index: seeded rows, `--intervals` per type, as
tools/bench_score.py; K levels in {29, 64, 256, 1024, 4096} (the 29 of the evaluation sweep, else K evenly spaced in 0..1), L = 3.
  (A) run-table rounds  sweep_eval.score_sweep_device in ceil(K / 64) calls of at most lad_runs_max_thresholds() thresholds: what
                        there was before csrc/surface.hip
  (B) component tree    sweep_eval.score_surface_device end to end (workspace, the copy of the levels, six launches, the scores to
                        the host), and lad_score_surface alone by device events, buffers allocated beforehand
  (B) on a monotone ramp and on a constant track of the same length: the cases in which a plain walk to the nearest smaller value
      degenerates; their times belong next to the random track's
(A) and (B) alternate within a round and must give the same integers; every figure is min / median / max over the samples.
Every step on the GPU runs under a time limit of its own: a step that overruns it ends the process (exit status 124), and so does
the first error.  Prints one JSON line."""
import argparse
import contextlib
import ctypes
import json
import os
import statistics
import sys
import threading

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "laughter-detection-icsi_amd", "utils"), os.path.join(ROOT, "laughter-detection-icsi_amd"), ROOT,
                os.path.join(ROOT, "tools")]

from bench_score import CHANNEL, MIN_LENGTHS, THRESHOLDS, make_index, spread, wall  # noqa: E402

KS = (29, 64, 256, 1024, 4096)


@contextlib.contextmanager
def limit(seconds, what):
    """A GPU step under its own time limit: the process ends (124) if the step is still running when it runs out."""
    def overrun():
        sys.stderr.write(f"tools/bench_surface.py: {what} did not finish within {seconds} s\n")
        sys.stderr.flush()
        os._exit(124)
    timer = threading.Timer(seconds, overrun)
    timer.daemon = True
    timer.start()
    try:
        yield
    finally:
        timer.cancel()


def levels_for(K):
    return list(THRESHOLDS) if K == len(THRESHOLDS) else [float(v) for v in np.linspace(0.0, 1.0, K)]


def rounds(probs, levels, index):
    """(A): the run-table route, 64 thresholds per call."""
    import _hip
    import sweep_eval as se
    step = int(_hip.lib().lad_runs_max_thresholds())
    return np.concatenate([se.score_sweep_device(probs, [CHANNEL], levels[k:k + step], MIN_LENGTHS, 100.0, index)
                           for k in range(0, len(levels), step)], axis=1)


def launches_ms(probs2d, levels, index, samples, warmup):
    """lad_score_surface alone (a copy of the levels, a memset and six launches) by device events."""
    import _hip
    lib = _hip.lib()
    C, T = probs2d.shape
    K, L = len(levels), len(MIN_LENGTHS)
    dix = index.to_device([CHANNEL], probs2d.device)
    lv = (ctypes.c_double * K)(*levels)
    mls = (ctypes.c_double * L)(*MIN_LENGTHS)
    fps_host = np.full(C, 100.0)
    fps_dev = torch.from_numpy(fps_host).to(probs2d.device)
    i32p, f64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    ws = torch.empty(lib.lad_surface_workspace_bytes(C, T, dix.n_intervals, K, L), dtype=torch.uint8, device=probs2d.device)
    scores = torch.empty((C, K, L, 7), dtype=torch.int64, device=probs2d.device)
    st = _hip.stream_handle(probs2d.device)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for i in range(warmup + samples):
        ev[0].record()
        _hip.check(lib.lad_score_surface(_hip.ptr(probs2d), 0, C, T, lv, K, _hip.ptr(dix.bounds), _hip.ptr(dix.offsets),
                                         dix.bounds_host.ctypes.data_as(i32p), dix.offsets_host.ctypes.data_as(i32p), dix.n_intervals,
                                         _hip.ptr(fps_dev), fps_host.ctypes.data_as(f64p), mls, L, _hip.ptr(ws), _hip.ptr(scores), st),
                   "lad_score_surface")
        ev[1].record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(ev[0].elapsed_time(ev[1]))
    return spread(ms, 4)


def tree_only(probs, index, samples, warmup, step_s):
    """(B) alone, per K: end to end and by events."""
    import sweep_eval as se
    out = {}
    for K in KS:
        levels = levels_for(K)
        with limit(step_s, f"the component tree, K = {K}"):
            b_s = [wall(lambda: se.score_surface_device(probs, [CHANNEL], levels, MIN_LENGTHS, 100.0, index))[0]
                   for _ in range(warmup + samples)][warmup:]
            out[str(K)] = {"tree_s": spread(b_s), "lad_score_surface_ms": launches_ms(probs.view(1, -1), levels, index, max(samples, 10), warmup)}
    return out


def legs(probs, index, samples, warmup, step_s):
    """(A) and (B) on one (T,) float32 GPU track, alternating, per K; the two must give the same integers."""
    import sweep_eval as se
    index.to_device([CHANNEL], probs.device)
    out = {"frames": int(probs.numel())}
    for K in KS:
        levels = levels_for(K)
        a_s, b_s = [], []
        with limit(step_s, f"run-table rounds against the component tree, K = {K}"):
            for i in range(warmup + samples):
                ta, da = wall(lambda: rounds(probs, levels, index))
                tb, db = wall(lambda: se.score_surface_device(probs, [CHANNEL], levels, MIN_LENGTHS, 100.0, index))
                if i == 0:
                    assert np.array_equal(da, db), f"K = {K}: the component tree's scores differ from the run-table rounds'"
                    kept = int(db[0, :, :, 0].sum())
                if i >= warmup:
                    a_s.append(ta)
                    b_s.append(tb)
            out[str(K)] = {"rounds": -(-K // 64), "kept_runs_over_all_levels": kept, "run_table_rounds_s": spread(a_s), "tree_s": spread(b_s),
                           "identical_scores": True, "A_over_B_median": round(statistics.median(a_s) / statistics.median(b_s), 2),
                           "lad_score_surface_ms": launches_ms(probs.view(1, -1), levels, index, max(samples, 10), warmup)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--intervals", type=int, default=3000, help="transcript rows per type")
    ap.add_argument("--step_limit", type=float, default=120.0, help="seconds each GPU step may take before the tool gives up")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_surface.py needs an MI355X (a CPU run says nothing about these legs)")
    import bench
    import config
    import synth
    from oracle import recipe
    from utils import get_feat_extractor
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    with limit(a.step_limit, "the model's track"):
        ex = get_feat_extractor(config.FEAT["num_samples"], config.FEAT["num_filters"])
        model = bench._make_model(0.0, dev, degenerate_ok=False)
        model.eval()
        pcm = synth.make_clips(int(a.minutes * 60), seed=9876, device=dev).view(-1)
        probs = model.engine.predict_windows(ex.extract_long(pcm), precision="fp16").float().clone().view(-1)
        torch.cuda.synchronize()
        del pcm
    T = probs.numel()
    index = make_index(2024, T / 100.0, a.intervals)
    on_gpu = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)    # noqa: E731
    rec = {"metric": "dense threshold sweep of one channel: run-table rounds of 64 thresholds against one component tree",
           "unit": "s", "gpu": torch.cuda.get_device_name(dev), "cpu_model": bench._cpu_model(), "host_cores": os.cpu_count(),
           "torch": torch.__version__, "minutes": a.minutes, "levels": list(KS), "min_lengths": len(MIN_LENGTHS),
           "rows_per_type": a.intervals, "samples": a.samples, "warmup": a.warmup,
           "model_track": legs(probs, index, a.samples, a.warmup, a.step_limit),
           "recipe_track": legs(on_gpu(recipe.make_prob_track(5, T)), index, a.samples, a.warmup, a.step_limit),
           "ramp_track": tree_only(on_gpu((np.arange(T) + 1.0) / (T + 1.0)), index, a.samples, a.warmup, a.step_limit),
           "constant_track": tree_only(on_gpu(np.full(T, 0.6)), index, a.samples, a.warmup, a.step_limit)}
    wins = [K for K in KS if all(rec[t][str(K)]["A_over_B_median"] > 1 for t in ("model_track", "recipe_track"))]
    rec["tree_wins_on_both_tracks_at_levels"] = wins
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
