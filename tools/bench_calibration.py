"""The label histogram and the calibration map of 60-minute channels, host against device, in one process:
    python tools/bench_calibration.py [--minutes 60] [--samples 5] [--warmup 1] [--out profiles/<name>.json]      (GPU box)

Tracks: the fp16 probabilities of bench.py's inference record (synth.make_clips(3600, seed=9876) through its model), 360,000
frames as float32; oracle.recipe.make_prob_track(5, T) as float32; a constant track.  One channel each, and twenty channels as one
(20, T) call summed into one group.  The transcript is seeded: per channel 400 rows of each type over the hour.
  (a) host leg     device-to-host copy of the track + calibration.label_histogram_host
  (b) device leg   calibration.label_histogram_device, end to end (allocations, the size query, the index upload of the first
                   call apart, and the histogram copied to the host at the end)
  (c) launches     lad_label_histogram (a memset, two copies where given, two launches) by device events, buffers allocated beforehand
  (d) remap        device-to-host copy + calibration.apply_calibration + copy back, against apply_calibration_device, and its one
                   launch by device events
The legs alternate within a round after the warm-ups; every figure is min / median / max over the samples.  The first round
checks that both legs return the same integers / bytes.  The constant track against the seeded one is the evidence that the
aggregation works: every frame of it adds to the same five counters.  No target is set.  Prints one JSON line."""
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

MANY = 20


def spread(xs, digits=6):
    return {"min": round(min(xs), digits), "median": round(statistics.median(xs), digits), "max": round(max(xs), digits), "n": len(xs)}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def transcript(n_channels, seconds, per_type=400, seed=77):
    """Seeded rows and the channel table of one meeting: per participant `per_type` rows of each type, up to 3 s long."""
    rng = np.random.default_rng(seed)
    rows, chans = [], []
    for c in range(n_channels):
        part = f"p{c:03d}"
        chans.append({"meeting_id": "Bmr001", "part_id": part, "chan": f"chan{c}", "length": float(seconds)})
        for kind in ("laugh", "speech", "noise", "invalid"):
            starts = np.round(np.sort(rng.random(per_type)) * (seconds - 3.0), 3)
            lengths = np.round(rng.random(per_type) * 3.0, 3)
            for s, n in zip(starts.tolist(), lengths.tolist()):
                rows.append({"meeting_id": "Bmr001", "part_id": part, "chan": f"chan{c}", "start": s, "end": s + n, "length": n,
                             "type": kind, "laugh_type": "laugh" if kind == "laugh" else None})
    return rows, chans


def launches_ms(p2, dix, fps_host, groups, n_groups, samples, warmup):
    """(c): device events around one lad_label_histogram."""
    import _hip
    C, T = p2.shape
    ws = _hip.workspace("lad_label_histogram_workspace_bytes", C, T, dix.n_intervals, device=p2.device)
    hist = torch.empty((n_groups, 5, 65538), dtype=torch.int64, device=p2.device)
    fps_dev = torch.from_numpy(fps_host).to(p2.device)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for i in range(warmup + samples):
        ev[0].record()
        _hip.launch("lad_label_histogram", p2, 0 if p2.dtype == torch.float32 else 1, C, T, None, dix.bounds, dix.offsets, dix.bounds_host,
                    dix.offsets_host, dix.n_intervals, fps_dev, fps_host, groups, n_groups, ws, hist)
        ev[1].record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(ev[0].elapsed_time(ev[1]))
    return spread(ms, 4)


def histogram_legs(p2, channels, fps, index, groups, samples, warmup):
    """(a), (b) and (c) on one (C, T) float32 GPU tensor."""
    import calibration
    C, T = p2.shape
    dix = index.to_device(channels, p2.device)                 # (kept by the index: uploaded once, as a caller's second call finds it)
    fps_host = np.full(C, float(fps))

    def host():
        return calibration.label_histogram_host(list(p2.cpu().numpy()), channels, fps, index, groups=groups)

    def device():
        return calibration.label_histogram_device(p2, channels, fps, index, groups=groups)
    host_s, dev_s = [], []
    for i in range(warmup + samples):
        th, fh = wall(host)
        td, fd = wall(device)
        if i == 0:
            assert np.array_equal(fh, fd), "the device histogram differs from the host's"
            occupied = int((fd.sum(axis=(0, 1)) > 0).sum())
        if i >= warmup:
            host_s.append(th)
            dev_s.append(td)
    g = None if groups is None else np.asarray(groups, np.int32)
    return {"channels": C, "frames": T, "intervals": dix.n_intervals, "occupied_slots": occupied, "host_leg_s": spread(host_s),
            "device_leg_s": spread(dev_s), "identical_integers": True,
            "host_over_device_median": round(statistics.median(host_s) / statistics.median(dev_s), 2),
            "launches_ms": launches_ms(p2, dix, fps_host, g, C if g is None else 1, max(samples, 20), warmup)}


def remap_legs(p2, table, samples, warmup):
    """(d) on one (C, T) float32 GPU tensor."""
    import _hip
    import calibration
    table_dev = torch.from_numpy(table).to(p2.device)

    def host():
        return torch.from_numpy(calibration.apply_calibration(p2.cpu().numpy(), table)).to(p2.device)

    def device():
        return calibration.apply_calibration_device(p2, table_dev)
    host_s, dev_s = [], []
    for i in range(warmup + samples):
        th, fh = wall(host)
        td, fd = wall(device)
        if i == 0:
            assert fh.cpu().numpy().tobytes() == fd.cpu().numpy().tobytes(), "the device map differs from the host's"
        if i >= warmup:
            host_s.append(th)
            dev_s.append(td)
    out = torch.empty(p2.shape, dtype=torch.float64, device=p2.device)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for i in range(warmup + max(samples, 20)):
        ev[0].record()
        _hip.launch("lad_track_remap", p2, 0, p2.shape[0], p2.shape[1], table_dev, out)
        ev[1].record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(ev[0].elapsed_time(ev[1]))
    return {"channels": int(p2.shape[0]), "frames": int(p2.shape[1]), "host_leg_s": spread(host_s), "device_leg_s": spread(dev_s),
            "identical_bytes": True, "host_over_device_median": round(statistics.median(host_s) / statistics.median(dev_s), 2),
            "launch_ms": spread(ms, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_calibration.py needs an MI355X (a CPU run says nothing about these legs)")
    import _hip
    import bench
    import calibration
    import config
    import sweep_eval
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
    probs = model.engine.predict_windows(ex.extract_long(pcm), precision="fp16").clone().float()
    del pcm
    T = probs.numel()
    fps = T / float(seconds)
    made = torch.from_numpy(recipe.make_prob_track(5, T).astype(np.float32)).to(dev)
    constant = torch.full((T,), 0.625, dtype=torch.float32, device=dev)
    rows, chans = transcript(MANY, seconds)
    index = sweep_eval.TranscriptIndex(rows, chans)
    channels = [("Bmr001", f"chan{c}") for c in range(MANY)]
    one = {name: histogram_legs(t.view(1, T), channels[:1], fps, index, None, a.samples, a.warmup)
           for name, t in (("model_track", probs), ("recipe_track", made), ("constant_track", constant))}
    many = {name: histogram_legs(t.view(1, T).repeat(MANY, 1).contiguous(), channels, fps, index, [0] * MANY, a.samples, a.warmup)
            for name, t in (("model_track", probs), ("recipe_track", made), ("constant_track", constant))}
    row = calibration.label_histogram_device(made.view(1, T), channels[:1], fps, index)[0]
    table = calibration.fit_isotonic(row)
    rec = {"metric": "label histogram of probability tracks against a transcript, and a calibration table applied to them: host legs "
                     "(copy + numpy) against the device legs",
           "unit": "s", "gpu": torch.cuda.get_device_name(dev), "cpu_model": bench._cpu_model(), "host_cores": os.cpu_count(),
           "torch": torch.__version__, "minutes": a.minutes, "samples": a.samples, "warmup": a.warmup, "fps": fps,
           "tile_frames": int(_hip.lib().lad_label_histogram_tile_frames()), "one_channel": one, "twenty_channels_one_group": many,
           "constant_over_recipe_launches_median": {
               "one_channel": round(one["constant_track"]["launches_ms"]["median"] / one["recipe_track"]["launches_ms"]["median"], 3),
               "twenty_channels": round(many["constant_track"]["launches_ms"]["median"] / many["recipe_track"]["launches_ms"]["median"], 3)},
           "remap_one_channel": remap_legs(made.view(1, T), table, a.samples, a.warmup),
           "remap_twenty_channels": remap_legs(made.view(1, T).repeat(MANY, 1).contiguous(), table, a.samples, a.warmup),
           "not_measured": ["float64 tracks", "ragged tensors (lengths)", "one group per channel for twenty channels (a 52 MB histogram "
                            "to zero and copy)", "the fits (host only)", "hardware counters of the histogram kernel",
                            "an alternative without the sort (one atomic per frame), so the gain of the aggregation itself is "
                            "bounded only by the constant-against-seeded comparison"]}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
