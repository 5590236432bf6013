"""The smoothed threshold sweep of a 60-minute channel (low-pass + sweep), host against device, in one process:
    python tools/bench_lowpass.py [--minutes 60] [--samples 10] [--warmup 2] [--out profiles/<name>.json]      (GPU box)

Track: the fp16 probabilities of bench.py's inference record (synth.make_clips(3600, seed=9876) through its model), 360,000
frames; cutoff 0.01 (the reference's, laugh_segmenter.py:49); settings: the 29 thresholds x 3 min_lengths of the evaluation sweep.
  (a) host leg    device-to-host copy of the track + laugh_segmenter.lowpass (scipy) + laugh_segmenter.get_laughter_instances
  (b) device leg  laugh_segmenter.lowpass_device + laugh_segmenter.get_laughter_instances_device, end to end
  (c) launches    the six launches of lad_lowpass by device events, buffers allocated beforehand
  (d) channels    a (10, T) tensor (the track, rotated): ten host filters against one device call, and its launches
Legs (a) and (b) alternate within a round; every figure is min / median / max over the samples.  Prints one JSON line.
The float64 vector rate of the chip is not measured here; the figures are times of this kernel as it is, nothing more."""
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
CUTOFF = 0.01


def spread(xs, digits=6):
    return {"min": round(min(xs), digits), "median": round(statistics.median(xs), digits), "max": round(max(xs), digits), "n": len(xs)}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def launches_ms(probs2d, samples, warmup):
    """(c): device events around one lad_lowpass (six launches)."""
    import _hip
    import lowpass
    lib = _hip.lib()
    C, T = probs2d.shape
    f64p = ctypes.POINTER(ctypes.c_double)
    b, a = lowpass.butter2(CUTOFF)
    zi = lowpass.zi2(b, a)
    ws = torch.empty(lib.lad_lowpass_workspace_bytes(C, T), dtype=torch.uint8, device=probs2d.device)
    out = torch.empty((C, T), dtype=torch.float64, device=probs2d.device)
    st = _hip.stream_handle(probs2d.device)
    dtype = 0 if probs2d.dtype == torch.float32 else 1
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for i in range(warmup + samples):
        ev[0].record()
        _hip.check(lib.lad_lowpass(_hip.ptr(probs2d), dtype, C, T, None, b.ctypes.data_as(f64p), a.ctypes.data_as(f64p),
                                   zi.ctypes.data_as(f64p), _hip.ptr(out), _hip.ptr(ws), st), "lad_lowpass")
        ev[1].record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(ev[0].elapsed_time(ev[1]))
    return {"lowpass_ms": spread(ms, 4), "workspace_bytes": ws.numel()}


def legs(probs, samples, warmup):
    """(a) and (b) on one (T,) float32 GPU track, alternating."""
    import laugh_segmenter as ls

    def host():
        return ls.get_laughter_instances(ls.lowpass(probs.cpu().numpy(), cutoff=CUTOFF), THRESHOLDS, MIN_LENGTHS, 100.0)

    def device():
        return ls.get_laughter_instances_device(ls.lowpass_device(probs, cutoff=CUTOFF), THRESHOLDS, MIN_LENGTHS, 100.0)
    host_s, dev_s, filt_host_s, filt_dev_s = [], [], [], []
    for i in range(warmup + samples):
        th, dh = wall(host)
        td, dd = wall(device)
        x = probs.cpu().numpy()
        tfh, fh = wall(lambda: ls.lowpass(x, cutoff=CUTOFF))
        tfd, fd = wall(lambda: ls.lowpass_device(probs, cutoff=CUTOFF))
        if i == 0:
            err = float(np.max(np.abs(fd.cpu().numpy() - fh)))
            same = list(dh.keys()) == list(dd.keys()) and all(dh[k] == dd[k] for k in dh)
            n_inst = sum(len(v) for v in dh.values())
        if i >= warmup:
            host_s.append(th)
            dev_s.append(td)
            filt_host_s.append(tfh)
            filt_dev_s.append(tfd)
    return {"frames": int(probs.numel()), "settings": len(THRESHOLDS) * len(MIN_LENGTHS), "instances_in_dictionary": n_inst,
            "host_leg_s": spread(host_s), "device_leg_s": spread(dev_s), "host_filter_alone_s": spread(filt_host_s),
            "device_filter_alone_s": spread(filt_dev_s), "max_abs_diff_of_the_filtered_tracks": err,
            "identical_dictionaries": bool(same),
            "host_over_device_median": round(statistics.median(host_s) / statistics.median(dev_s), 2),
            "launches": launches_ms(probs.view(1, -1), max(samples, 20), warmup)}


def channels(probs, samples, warmup, C=10):
    """(d): C tracks as one (C, T) tensor: copy + C host filters against one device call."""
    import laugh_segmenter as ls
    many = torch.stack([probs.roll(c * 1009) for c in range(C)]).contiguous()
    host_s, dev_s = [], []
    for i in range(warmup + samples):
        th, a = wall(lambda: [ls.lowpass(row, cutoff=CUTOFF) for row in many.cpu().numpy()])
        td, b = wall(lambda: ls.lowpass_device(many, cutoff=CUTOFF))
        if i == 0:
            err = float(np.max(np.abs(b.cpu().numpy() - np.stack(a))))
        if i >= warmup:
            host_s.append(th)
            dev_s.append(td)
    return {"channels": C, "frames": int(many.shape[1]), "host_copy_and_filters_s": spread(host_s), "device_one_call_s": spread(dev_s),
            "max_abs_diff_of_the_filtered_tracks": err,
            "host_over_device_median": round(statistics.median(host_s) / statistics.median(dev_s), 2),
            "launches_one_call": launches_ms(many, max(samples, 20), warmup)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_lowpass.py needs an MI355X (a CPU run says nothing about these legs)")
    import bench
    import config
    import synth
    from utils import get_feat_extractor
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ex = get_feat_extractor(config.FEAT["num_samples"], config.FEAT["num_filters"])
    model = bench._make_model(0.0, dev, degenerate_ok=False)
    model.eval()
    seconds = int(a.minutes * 60)
    pcm = synth.make_clips(seconds, seed=9876, device=dev).view(-1)
    probs = model.engine.predict_windows(ex.extract_long(pcm), precision="fp16").clone()
    del pcm
    rec = {"metric": "low-pass (cutoff 0.01) + 87-setting threshold sweep of one channel: host leg against device leg", "unit": "s",
           "gpu": torch.cuda.get_device_name(dev), "cpu_model": bench._cpu_model(), "host_cores": os.cpu_count(),
           "torch": torch.__version__, "minutes": a.minutes, "cutoff": CUTOFF, "thresholds": len(THRESHOLDS),
           "min_lengths": len(MIN_LENGTHS), "samples": a.samples, "warmup": a.warmup,
           "model_track": legs(probs, a.samples, a.warmup),
           "ten_channels_model_track": channels(probs, a.samples, a.warmup)}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
