"""What augmentation adds to the assembly of a training batch, launch against launch in one process:
    python tools/bench_augment.py [--batch 512] [--samples 20] [--warmup 3] [--bench-json <file>] [--out profiles/<name>.json]   (GPU box)

Store: 8 synthetic channels of 60 s (synth.make_clips through the feature extractor, 6000 x 44 each); batch: 512 one-second
segments at random offsets, the shape of a training step.  Per sample, device events around
  (a) lad_gather_segments      the plain gather -- unchanged by the augmentation, so its time is the parent's
  (b) lad_gather_segments_aug  preset 'spec+mix', noise = the same 8 channels
alternating; medians of --samples launches after --warmup of each.  The difference is what a training step pays.
--bench-json: the JSON line of `python bench.py` taken on the same box just before; its ms_per_step is the yardstick (the added
time is to stay under 2 % of it).  Prints one JSON line."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--preset", type=str, default="spec+mix")
    ap.add_argument("--bench-json", type=str, default=None, help="file holding the JSON line of bench.py from the same box")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_augment.py needs an MI355X (a CPU run says nothing about these launches)")
    import augment
    import bench
    import config
    import datasets
    import synth
    from utils import get_feat_extractor
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    T, F = config.FEAT["num_samples"], config.FEAT["num_filters"]
    store = datasets.FeatureStore(get_feat_extractor(T, F))
    pcm = synth.make_clips(8, n_samples=16000 * 60, seed=2468, device=dev)
    for c in range(pcm.shape[0]):
        store.add_audio(f"c{c}", pcm[c])
    rng = np.random.default_rng(0)
    B = a.batch
    chan = torch.from_numpy(rng.integers(0, 8, B).astype(np.int32)).to(dev)
    first = torch.from_numpy(rng.integers(0, store.mats[0].shape[0] - T, B).astype(np.int64)).to(dev)
    count = torch.full((B,), T, dtype=torch.int32, device=dev)
    cfg = augment.from_preset(a.preset, seed=1234)
    noise = datasets.NoiseChannels(store, range(8))
    out = torch.empty((B, T, F), device=dev, dtype=torch.float32)

    def plain():
        datasets.gather_segments(store, chan, first, count, T, datasets.LOG_EPSILON, out=out)

    def aug(epoch):
        datasets.gather_segments_augmented(store, chan, first, count, T, datasets.LOG_EPSILON, cfg, epoch, noise, out=out, check_first=False)

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])
    plain_ms, aug_ms = [], []
    for i in range(a.warmup + a.samples):
        tp = timed(plain)
        ta = timed(lambda: aug(i))
        if i >= a.warmup:
            plain_ms.append(tp)
            aug_ms.append(ta)
    aug(0)
    frac_changed = float((out != datasets.gather_segments(store, chan, first, count, T, datasets.LOG_EPSILON)).any(dim=(1, 2)).float().mean())
    added = statistics.median(aug_ms) - statistics.median(plain_ms)
    rec = {"metric": f"assembly of one training batch: lad_gather_segments against lad_gather_segments_aug ('{a.preset}')", "unit": "ms",
           "gpu": torch.cuda.get_device_name(dev), "cpu_model": bench._cpu_model(), "torch": torch.__version__,
           "batch": B, "frames": T, "filters": F, "samples": a.samples, "warmup": a.warmup, "timing": "device events around one launch",
           "gather_ms": spread(plain_ms), "gather_aug_ms": spread(aug_ms), "added_ms_median": round(added, 5),
           "segments_changed_fraction": round(frac_changed, 4), "bytes_out": B * T * F * 4}
    if a.bench_json:
        with open(a.bench_json) as f:
            line = [l for l in f.read().splitlines() if l.strip().startswith("{")][-1]
        step = json.loads(line)
        rec["bench_ms_per_step"] = step["ms_per_step"]
        rec["bench_segments_per_s"] = step.get("value")
        rec["added_over_step"] = round(added / step["ms_per_step"], 5)
        rec["bar"] = "added_ms_median < 0.02 * bench_ms_per_step"
        rec["bar_met"] = bool(added < 0.02 * step["ms_per_step"])
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
