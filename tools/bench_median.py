"""The median filter of a 60-minute channel, host against device, in one process:
    python tools/bench_median.py [--minutes 60] [--samples 5] [--warmup 1] [--out profiles/<name>.json]      (GPU box)

Tracks: the fp16 probabilities of bench.py's inference record (synth.make_clips(3600, seed=9876) through its model), 360,000
frames as float32, and oracle.recipe.make_prob_track(5, T) as float32.  Windows of 11, 51, 101 and 1023 frames.
  (a) host leg     device-to-host copy of the track + scipy.ndimage.median_filter(mode='nearest') + copy back to the device
  (b) device leg   laugh_segmenter.median_filter_device, end to end (allocations and the size query included)
  (c) kernel       the one launch of lad_rank_filter by device events, buffers allocated beforehand
  (d) bound        (c) at window 101 on a constant track and on a ramp of the same length, next to the two tracks above: the work
                   per frame depends on the window alone
The legs alternate within a round after the warm-ups; every figure is min / median / max over the samples.  The first round
checks that both legs return the same values.  No target is set.  Prints one JSON line."""
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

WINDOWS = [11, 51, 101, 1023]
BOUND_WINDOW = 101


def spread(xs, digits=6):
    return {"min": round(min(xs), digits), "median": round(statistics.median(xs), digits), "max": round(max(xs), digits), "n": len(xs)}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def kernel_ms(probs, window, samples, warmup):
    """(c): device events around one lad_rank_filter (one launch) at the median's rank."""
    import _hip
    lib = _hip.lib()
    p2 = probs.view(1, -1)
    C, T = p2.shape
    ws = torch.empty(lib.lad_rank_filter_workspace_bytes(C, T, window), dtype=torch.uint8, device=p2.device)
    out = torch.empty_like(p2)
    st = _hip.stream_handle(p2.device)
    dtype = 0 if p2.dtype == torch.float32 else 1
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for i in range(warmup + samples):
        ev[0].record()
        _hip.check(lib.lad_rank_filter(_hip.ptr(p2), dtype, C, T, None, window, (window - 1) // 2, _hip.ptr(out), _hip.ptr(ws), st),
                   "lad_rank_filter")
        ev[1].record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(ev[0].elapsed_time(ev[1]))
    return spread(ms, 4)


def legs(probs, samples, warmup):
    """(a), (b) and (c) on one (T,) float32 GPU track, the legs alternating, per window."""
    from scipy import ndimage

    import laugh_segmenter as ls
    out = {"frames": int(probs.numel()), "distinct_values": int(torch.unique(probs).numel())}
    for window in WINDOWS:
        def host():
            return torch.from_numpy(ndimage.median_filter(probs.cpu().numpy(), size=window, mode="nearest")).to(probs.device)

        def device():
            return ls.median_filter_device(probs, window)
        host_s, dev_s = [], []
        for i in range(warmup + samples):
            th, fh = wall(host)
            td, fd = wall(device)
            if i == 0:
                assert torch.equal(fh, fd), f"the device median differs from scipy's at window {window}"
            if i >= warmup:
                host_s.append(th)
                dev_s.append(td)
        out[f"window_{window}"] = {"host_leg_s": spread(host_s), "device_leg_s": spread(dev_s), "identical_values": True,
                                   "host_over_device_median": round(statistics.median(host_s) / statistics.median(dev_s), 2),
                                   "kernel_ms": kernel_ms(probs, window, max(samples, 20), warmup)}
    return out


def bound(tracks, samples, warmup):
    """(d): the kernel alone at one window on tracks that differ only in what they hold."""
    return {"window": BOUND_WINDOW, **{name: kernel_ms(t, BOUND_WINDOW, max(samples, 20), warmup) for name, t in tracks.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_median.py needs an MI355X (a CPU run says nothing about these legs)")
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
    tracks = {"model_track": probs, "recipe_track": made, "constant_track": torch.full((T,), 0.625, dtype=torch.float32, device=dev),
              "ramp_track": torch.linspace(0.0, 1.0, T, dtype=torch.float32, device=dev)}
    lib = _hip.lib()
    rec = {"metric": "median filter of one channel: copy + scipy.ndimage.median_filter + copy back against median_filter_device",
           "unit": "s", "gpu": torch.cuda.get_device_name(dev), "cpu_model": bench._cpu_model(), "host_cores": os.cpu_count(),
           "torch": torch.__version__, "minutes": a.minutes, "windows": WINDOWS, "samples": a.samples, "warmup": a.warmup,
           "tile_frames": int(lib.lad_rank_filter_tile_frames()),
           "model_track": legs(probs, a.samples, a.warmup), "recipe_track": legs(made, a.samples, a.warmup),
           "kernel_alone_by_track_ms": bound(tracks, a.samples, a.warmup)}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
