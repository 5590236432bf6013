"""Time and event scores of the dense threshold sweep of one 60-minute channel, run-table rounds against the component tree, in one
process:
    python tools/bench_surface_events.py [--minutes 60] [--samples 5] [--warmup 1] [--intervals 3000]
                                         [--out profiles/surface_events_60min.json]   (GPU box)

Tracks: the fp16 probabilities of bench.py's inference record (synth.make_clips(3600, seed=9876) through its model), 360,000 frames,
and oracle.recipe.make_prob_track(5, T) as float32 (many more runs); index: seeded rows, `--intervals` per type, as
tools/bench_score.py; K levels in {29, 64, 256, 1024, 4096} as tools/bench_surface.py, L = 3, criteria (20 ms, 50 %).
  (A) run-table rounds  sweep_eval.score_sweep_device(..., events=) in ceil(K / 64) calls of at most lad_runs_max_thresholds()
                        thresholds: lad_runs_count + lad_runs_fill + lad_score_runs + lad_score_events per round
  (B) component tree    sweep_eval.score_surface_device(..., events=) end to end (workspace, the copy of the levels, seven launches,
                        both arrays to the host), and lad_score_surface_events alone by device events, buffers allocated beforehand
  (B) on the recipe track against an index whose only laugh is as long as the track: one event, walked by one wave per 64 levels
(A) and (B) alternate within a round and must give the same integers in both arrays; every figure is min / median / max over the
samples.  Every step on the GPU runs under a time limit of its own: a step that overruns it ends the process (exit status 124), and
so does the first error.  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "laughter-detection-icsi_amd", "utils"), os.path.join(ROOT, "laughter-detection-icsi_amd"), ROOT,
                os.path.join(ROOT, "tools")]

from bench_score import CHANNEL, MIN_LENGTHS, make_index, spread, wall  # noqa: E402
from bench_surface import KS, levels_for, limit  # noqa: E402

CRITERIA = (20, 50)


def rounds(probs, levels, index):
    """(A): the run-table route, 64 thresholds per call -> (scores, events)."""
    import _hip
    import sweep_eval as se
    step = int(_hip.lib().lad_runs_max_thresholds())
    parts = [se.score_sweep_device(probs, [CHANNEL], levels[k:k + step], MIN_LENGTHS, 100.0, index, events=CRITERIA)
             for k in range(0, len(levels), step)]
    return np.concatenate([p[0] for p in parts], axis=1), np.concatenate([p[1] for p in parts], axis=1)


def launches_ms(probs2d, levels, index, samples, warmup):
    """lad_score_surface_events alone (a copy of the levels, two memsets and seven launches) by device events."""
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
    ws = torch.empty(lib.lad_surface_events_workspace_bytes(C, T, dix.n_intervals, K, L), dtype=torch.uint8, device=probs2d.device)
    scores = torch.empty((C, K, L, 7), dtype=torch.int64, device=probs2d.device)
    events = torch.empty((C, K, L, 7), dtype=torch.int64, device=probs2d.device)
    st = _hip.stream_handle(probs2d.device)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for i in range(warmup + samples):
        ev[0].record()
        _hip.check(lib.lad_score_surface_events(_hip.ptr(probs2d), 0, C, T, lv, K, _hip.ptr(dix.bounds), _hip.ptr(dix.offsets),
                                                dix.bounds_host.ctypes.data_as(i32p), dix.offsets_host.ctypes.data_as(i32p),
                                                dix.n_intervals, _hip.ptr(fps_dev), fps_host.ctypes.data_as(f64p), mls, L, *CRITERIA,
                                                _hip.ptr(ws), _hip.ptr(scores), _hip.ptr(events), st), "lad_score_surface_events")
        ev[1].record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(ev[0].elapsed_time(ev[1]))
    return spread(ms, 4)


def legs(probs, index, samples, warmup, step_s):
    """(A) and (B) on one (T,) float32 GPU track, alternating, per K; the two must give the same integers."""
    import sweep_eval as se
    dix = index.to_device([CHANNEL], probs.device)
    out = {"frames": int(probs.numel()), "events": int(np.diff(dix.offsets_host)[1])}
    for K in KS:
        levels = levels_for(K)
        a_s, b_s = [], []
        with limit(step_s, f"run-table rounds against the component tree, K = {K}"):
            for i in range(warmup + samples):
                ta, da = wall(lambda: rounds(probs, levels, index))
                tb, db = wall(lambda: se.score_surface_device(probs, [CHANNEL], levels, MIN_LENGTHS, 100.0, index, events=CRITERIA))
                if i == 0:
                    assert np.array_equal(da[0], db[0]), f"K = {K}: the component tree's time scores differ from the run-table rounds'"
                    assert np.array_equal(da[1], db[1]), f"K = {K}: the component tree's event scores differ from the run-table rounds'"
                    links = int(db[1][0, :, :, 4].sum())
                if i >= warmup:
                    a_s.append(ta)
                    b_s.append(tb)
            out[str(K)] = {"rounds": -(-K // 64), "links_over_all_levels": links, "run_table_rounds_s": spread(a_s), "tree_s": spread(b_s),
                           "identical_scores": True, "A_over_B_median": round(statistics.median(a_s) / statistics.median(b_s), 2),
                           "lad_score_surface_events_ms": launches_ms(probs.view(1, -1), levels, index, max(samples, 10), warmup)}
    return out


def whole_track_index(duration_s):
    """One laugh from 0 to the end of the track: the longest window an event can have."""
    import sweep_eval as se
    rows = [(CHANNEL[0], "fe001", CHANNEL[1], 0.0, duration_s, duration_s, "laugh", "laugh")]
    return se.TranscriptIndex(rows, [(CHANNEL[0], "fe001", CHANNEL[1], duration_s)])


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
        raise SystemExit("tools/bench_surface_events.py needs an MI355X (a CPU run says nothing about these legs)")
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
    recipe_track = torch.from_numpy(np.ascontiguousarray(recipe.make_prob_track(5, T), np.float32)).to(dev)
    rec = {"metric": "time and event scores of the dense threshold sweep of one channel: run-table rounds of 64 thresholds against one "
                     "component tree",
           "unit": "s", "gpu": torch.cuda.get_device_name(dev), "cpu_model": bench._cpu_model(), "host_cores": os.cpu_count(),
           "torch": torch.__version__, "minutes": a.minutes, "levels": list(KS), "min_lengths": len(MIN_LENGTHS), "criteria": list(CRITERIA),
           "rows_per_type": a.intervals, "samples": a.samples, "warmup": a.warmup,
           "model_track": legs(probs, index, a.samples, a.warmup, a.step_limit),
           "recipe_track": legs(recipe_track, index, a.samples, a.warmup, a.step_limit),
           "recipe_track_one_event_as_long_as_the_track": legs(recipe_track, whole_track_index(T / 100.0), a.samples, a.warmup, a.step_limit)}
    rec["tree_wins_at_levels"] = {t: [K for K in KS if rec[t][str(K)]["A_over_B_median"] > 1]
                                  for t in ("model_track", "recipe_track", "recipe_track_one_event_as_long_as_the_track")}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
