"""Event-level scores of the sweep of one 60-minute channel, in one process:
    python tools/bench_events.py [--minutes 60] [--samples 10] [--warmup 2] [--intervals 3000] [--out profiles/<name>.json]   (GPU box)

Tracks: the fp16 probabilities of bench.py's inference record (synth.make_clips(3600, seed=9876) through its model), 360,000 frames,
and oracle.recipe.make_prob_track(5, T) as float32 (many more runs); settings: the 29 thresholds x 3 min_lengths of the evaluation
sweep (cluster_scripts/gen_eval_exp.py:30-36), and with them 3 offset drops x 3 minimum gaps (261 settings, five rounds of
csrc/binarize.hip); index: tools/bench_score.py's seeded rows, `--intervals` per type; criteria (200 ms, 50 per cent).
  (A) dictionary route  laugh_segmenter.get_laughter_instances_device (binarize_instances_device for the 261) + sweep_eval.
                        event_scores_instances on the dictionary: what could be done before csrc/events.hip
  (B) device route      sweep_eval.score_sweep_device(events=...) end to end: both score arrays
  (P) plain device      sweep_eval.score_sweep_device without events=: (B) - (P) is what the events add, per sample
(A), (B) and (P) alternate within a round; every figure is min / median / max over the samples.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "laughter-detection-icsi_amd", "utils"), os.path.join(ROOT, "laughter-detection-icsi_amd"), ROOT,
                os.path.join(ROOT, "tools")]

from bench_score import CHANNEL, MIN_LENGTHS, THRESHOLDS, make_index, spread, wall  # noqa: E402

OFFSET_DROPS = [0.0, 0.1, 0.2]
MIN_GAPS = [0.0, 0.1, 0.3]
CRITERIA = (200, 50)


def legs(probs, index, samples, warmup, binarize):
    """(A), (B) and (P) on one (T,) float32 GPU track, alternating; (A) and (B) must give the same integers."""
    import laugh_segmenter as ls
    import sweep_eval as se
    index.to_device([CHANNEL], probs.device)
    axes = dict(offset_drops=OFFSET_DROPS, min_gaps=MIN_GAPS) if binarize else {}

    def dictionary():
        if binarize:
            inst = ls.binarize_instances_device(probs, THRESHOLDS, MIN_LENGTHS, 100.0, OFFSET_DROPS, MIN_GAPS)
        else:
            inst = ls.get_laughter_instances_device(probs, THRESHOLDS, MIN_LENGTHS, 100.0)
        return se.event_scores_instances(inst, index, *CHANNEL, *CRITERIA)

    def device():
        return se.score_sweep_device(probs, [CHANNEL], THRESHOLDS, MIN_LENGTHS, 100.0, index, events=CRITERIA, **axes)

    def plain():
        return se.score_sweep_device(probs, [CHANNEL], THRESHOLDS, MIN_LENGTHS, 100.0, index, **axes)
    a_s, b_s, p_s = [], [], []
    for i in range(warmup + samples):
        ta, da = wall(dictionary)
        tb, (_, db) = wall(device)
        tp, _ = wall(plain)
        if i == 0:
            cell = db[0].reshape(-1, 7)             # (the dictionary's key order: thresholds-major, min_length last)
            assert np.array_equal(cell, np.array(list(da.values()), np.int64)), "the device event scores differ from the host scorer's"
        if i >= warmup:
            a_s.append(ta)
            b_s.append(tb)
            p_s.append(tp)
    return {"frames": int(probs.numel()), "cells": int(cell.shape[0]), "ref_events": int(cell[0, 0]),
            "links_over_all_settings": int(cell[:, 4].sum()), "ref_hit_over_all_settings": int(cell[:, 2].sum()),
            "dictionary_route_s": spread(a_s), "device_route_s": spread(b_s), "plain_device_scorer_s": spread(p_s),
            "events_added_s": spread([b - p for b, p in zip(b_s, p_s)]), "identical_events": True,
            "A_over_B_median": round(statistics.median(a_s) / statistics.median(b_s), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--intervals", type=int, default=3000, help="transcript rows per type")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_events.py needs an MI355X (a CPU run says nothing about these legs)")
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
    pcm = synth.make_clips(int(a.minutes * 60), seed=9876, device=dev).view(-1)
    probs = model.engine.predict_windows(ex.extract_long(pcm), precision="fp16").clone()
    del pcm
    index = make_index(2024, probs.numel() / 100.0, a.intervals)
    tracks = {"model_track": probs,
              "recipe_track": torch.from_numpy(recipe.make_prob_track(5, probs.numel()).astype(np.float32)).to(dev)}
    rec = {"metric": "event-level scores of the sweep of one channel: dictionary route against device route, and what events= adds",
           "unit": "s", "gpu": torch.cuda.get_device_name(dev), "cpu_model": bench._cpu_model(), "host_cores": os.cpu_count(),
           "torch": torch.__version__, "minutes": a.minutes, "thresholds": len(THRESHOLDS), "min_lengths": len(MIN_LENGTHS),
           "offset_drops": OFFSET_DROPS, "min_gaps": MIN_GAPS, "criteria_ms_pct": list(CRITERIA), "rows_per_type": a.intervals,
           "laugh_intervals": len(index.scoring_sets(*CHANNEL)[1]), "samples": a.samples, "warmup": a.warmup}
    for name, p in tracks.items():
        # cells: settings x min_lengths, 29 x 3 = 87 and 261 x 3 = 783
        rec[name] = {"sweep_87": legs(p, index, a.samples, a.warmup, False), "binarize_261": legs(p, index, a.samples, a.warmup, True)}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
