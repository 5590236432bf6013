"""Scoring the 87-setting sweep of one 60-minute channel against a transcript index, in one process:
    python tools/bench_score.py [--minutes 60] [--samples 10] [--warmup 2] [--intervals 3000] [--out profiles/<name>.json]   (GPU box)

Tracks: the fp16 probabilities of bench.py's inference record (synth.make_clips(3600, seed=9876) through its model), 360,000 frames,
and oracle.recipe.make_prob_track(5, T) as float32 (many more runs); settings: the 29 thresholds x 3 min_lengths of the evaluation
sweep (cluster_scripts/gen_eval_exp.py:30-36); index: seeded rows, `--intervals` per type (laugh, speech, noise, invalid).
  (A) dictionary route  laugh_segmenter.get_laughter_instances_device (run tables to the host, the dictionary of float tuples) +
                        sweep_eval.score_instances on it: what could be done before csrc/score.hip
  (B) device route      sweep_eval.score_sweep_device end to end (launches + the C x K counts + the scores to the host); the index is
                        on the device already (TranscriptIndex.to_device keeps it: built once per corpus)
  (C) launches          lad_runs_count, lad_runs_fill and lad_score_runs by device events, buffers allocated beforehand
(A) and (B) alternate within a round; every figure is min / median / max over the samples.  Prints one JSON line."""
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
CHANNEL = ("Bmr001", "chan0")


def spread(xs, digits=6):
    return {"min": round(min(xs), digits), "median": round(statistics.median(xs), digits), "max": round(max(xs), digits), "n": len(xs)}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def make_index(seed, duration_s, n_per_type):
    """Seeded transcript of one channel: n_per_type rows of each type, up to 1.5 s long, every sixth laugh a breath-laugh."""
    import sweep_eval as se
    rng = np.random.default_rng(seed)
    rows = []
    for kind in ("laugh", "speech", "noise", "invalid"):
        starts = np.round(np.sort(rng.random(n_per_type)) * duration_s, 3)
        lengths = np.round(rng.random(n_per_type) * 1.5, 3)
        for i, (s, n) in enumerate(zip(starts.tolist(), lengths.tolist())):
            rows.append((CHANNEL[0], "fe001", CHANNEL[1], s, s + n, n, kind,
                         ("breath-laugh" if i % 6 == 0 else "laugh") if kind == "laugh" else None))
    return se.TranscriptIndex(rows, [(CHANNEL[0], "fe001", CHANNEL[1], duration_s)])


def launches_ms(probs2d, index, samples, warmup):
    """(C): device events around lad_runs_count (three launches), lad_runs_fill (one) and lad_score_runs (a memset + two)."""
    import _hip
    lib = _hip.lib()
    C, T = probs2d.shape
    K, L = len(THRESHOLDS), len(MIN_LENGTHS)
    dix = index.to_device([CHANNEL], probs2d.device)
    thr = (ctypes.c_double * K)(*THRESHOLDS)
    mls = (ctypes.c_double * L)(*MIN_LENGTHS)
    fps_host = np.full(C, 100.0)
    fps_dev = torch.from_numpy(fps_host).to(probs2d.device)
    i32p, f64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    ws = torch.empty(lib.lad_runs_workspace_bytes(C, T, K), dtype=torch.uint8, device=probs2d.device)
    sws = torch.empty(lib.lad_score_workspace_bytes(C, dix.n_intervals, K, L), dtype=torch.uint8, device=probs2d.device)
    scores = torch.empty((C, K, L, 7), dtype=torch.int64, device=probs2d.device)
    st = _hip.stream_handle(probs2d.device)
    _hip.check(lib.lad_runs_count(_hip.ptr(probs2d), 0, C, T, thr, K, _hip.ptr(ws), st), "lad_runs_count")
    counts = np.ascontiguousarray(ws[:4 * C * K].view(torch.int32).cpu().numpy())
    cptr = counts.ctypes.data_as(i32p)
    total = int(counts.sum(dtype=np.int64))
    table = torch.empty((max(total, 1), 2), dtype=torch.int32, device=probs2d.device)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    count_ms, fill_ms, score_ms = [], [], []
    for i in range(warmup + samples):
        ev[0].record()
        _hip.check(lib.lad_runs_count(_hip.ptr(probs2d), 0, C, T, thr, K, _hip.ptr(ws), st), "lad_runs_count")
        ev[1].record()
        _hip.check(lib.lad_runs_fill(_hip.ptr(probs2d), 0, C, T, thr, K, _hip.ptr(ws), cptr, _hip.ptr(table), total, st), "lad_runs_fill")
        ev[2].record()
        _hip.check(lib.lad_score_runs(_hip.ptr(ws), _hip.ptr(table), cptr, C, T, K, _hip.ptr(dix.bounds), _hip.ptr(dix.offsets),
                                      dix.bounds_host.ctypes.data_as(i32p), dix.offsets_host.ctypes.data_as(i32p), dix.n_intervals,
                                      _hip.ptr(fps_dev), fps_host.ctypes.data_as(f64p), mls, L, _hip.ptr(sws), _hip.ptr(scores), st),
                   "lad_score_runs")
        ev[3].record()
        torch.cuda.synchronize()
        if i >= warmup:
            count_ms.append(ev[0].elapsed_time(ev[1]))
            fill_ms.append(ev[1].elapsed_time(ev[2]))
            score_ms.append(ev[2].elapsed_time(ev[3]))
    return {"count_ms": spread(count_ms, 4), "fill_ms": spread(fill_ms, 4), "score_ms": spread(score_ms, 4),
            "all_ms": spread([a + b + c for a, b, c in zip(count_ms, fill_ms, score_ms)], 4), "runs_in_tables": total,
            "index_intervals": dix.n_intervals, "score_bytes_to_host": C * K * L * 7 * 8}


def legs(probs, index, samples, warmup):
    """(A) and (B) on one (T,) float32 GPU track, alternating; the two must give the same integers."""
    import laugh_segmenter as ls
    import sweep_eval as se
    index.to_device([CHANNEL], probs.device)

    def dictionary():
        inst = ls.get_laughter_instances_device(probs, THRESHOLDS, MIN_LENGTHS, 100.0)
        return se.score_instances(inst, index, *CHANNEL)

    def device():
        return se.score_sweep_device(probs, [CHANNEL], THRESHOLDS, MIN_LENGTHS, 100.0, index)

    def sweep_only():
        return ls.get_laughter_instances_device(probs, THRESHOLDS, MIN_LENGTHS, 100.0)
    a_s, b_s, sweep_s = [], [], []
    for i in range(warmup + samples):
        ta, da = wall(dictionary)
        tb, db = wall(device)
        ts, _ = wall(sweep_only)
        if i == 0:
            want = np.array([[da[(t, l)] for l in MIN_LENGTHS] for t in THRESHOLDS], np.int64)
            assert np.array_equal(db[0], want), "the device scores differ from the host scorer's"
            kept = int(want[:, :, 0].sum())
        if i >= warmup:
            a_s.append(ta)
            b_s.append(tb)
            sweep_s.append(ts)
    return {"frames": int(probs.numel()), "settings": len(THRESHOLDS) * len(MIN_LENGTHS), "kept_runs_scored": kept,
            "dictionary_route_s": spread(a_s), "device_route_s": spread(b_s), "of_A_the_device_sweep_and_its_dictionary_s": spread(sweep_s),
            "identical_scores": True, "A_over_B_median": round(statistics.median(a_s) / statistics.median(b_s), 2),
            "launches": launches_ms(probs.view(1, -1), index, max(samples, 20), warmup)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--intervals", type=int, default=3000, help="transcript rows per type")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_score.py needs an MI355X (a CPU run says nothing about these legs)")
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
    index = make_index(2024, probs.numel() / 100.0, a.intervals)
    rec = {"metric": "87-setting sweep of one channel scored against a transcript index: dictionary route against device route",
           "unit": "s", "gpu": torch.cuda.get_device_name(dev), "cpu_model": bench._cpu_model(), "host_cores": os.cpu_count(),
           "torch": torch.__version__, "minutes": a.minutes, "thresholds": len(THRESHOLDS), "min_lengths": len(MIN_LENGTHS),
           "rows_per_type": a.intervals, "intervals_per_class": [len(s) for s in index.scoring_sets(*CHANNEL)],
           "model_pass_fp16_s": round(model_s, 4), "samples": a.samples, "warmup": a.warmup,
           "model_track": legs(probs, index, a.samples, a.warmup),
           "recipe_track": legs(torch.from_numpy(recipe.make_prob_track(5, probs.numel()).astype(np.float32)).to(dev), index, a.samples,
                                a.warmup)}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
