"""Rate conversion of one 60-minute channel to 16 kHz, host route against device route, in one process:
    python tools/bench_resample.py [--minutes 60] [--samples 10] [--warmup 2] [--out profiles/<name>.json]      (GPU box)

Channels: seeded noise as int16 PCM at 48 kHz (1/3: one phase, 61 taps) and at 44.1 kHz (160/441: 160 phases, 56 taps), as
scipy.io.wavfile.read hands a 16-bit file over.
  (A) host route   int16 -> float32 / 32768, scipy.signal.resample_poly in float32, upload of the 16 kHz float32 track: what a user
                   does today.  scipy runs the filter on one core; (A16) is the same over 16 equal pieces in 16 threads (the pieces'
                   edges are not stitched: a timing, not a result)
  (B) device route upload of the int16 file + resample.Resampler
  (C) kernel       lad_resample alone by device events, its algorithmic bytes (2 per input sample + 4 per output) over that time and
                   that rate over the 8 TB/s HBM peak
  (D) for scale    the fbank launch and the fp16 model pass of the same channel at 16 kHz
Legs (A) and (B) alternate within a round; every figure is min / median / max over the samples.  Prints one JSON line."""
import argparse
import concurrent.futures as cf
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "laughter-detection-icsi_amd", "utils"), os.path.join(ROOT, "laughter-detection-icsi_amd"), ROOT]

HBM_PEAK = 8.0e12
THREADS = 16


def spread(xs, digits=6):
    return {"min": round(min(xs), digits), "median": round(statistics.median(xs), digits), "max": round(max(xs), digits), "n": len(xs)}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def channel(sr, minutes, samples, warmup, dev, ex, model):
    from scipy import signal
    import resample
    n_in = int(sr * 60 * minutes)
    g = torch.Generator(device=dev).manual_seed(sr)
    pcm16 = (torch.randn(n_in, device=dev, generator=g) * 3000).clamp_(-32768, 32767).to(torch.int16).cpu().numpy()
    r = resample.Resampler(sr, 16000, dev)
    up, down = r.up, r.down
    pool = cf.ThreadPoolExecutor(THREADS)

    def host():
        x = pcm16.astype(np.float32) / 32768.0
        return torch.from_numpy(signal.resample_poly(x, up, down)).to(dev)

    def host16():
        x = pcm16.astype(np.float32) / 32768.0
        step = -(-n_in // (THREADS * down)) * down
        parts = list(pool.map(lambda i: signal.resample_poly(x[i * step:(i + 1) * step], up, down), range(-(-n_in // step))))
        return torch.from_numpy(np.concatenate(parts)).to(dev)

    def device():
        return r(torch.from_numpy(pcm16).to(dev))

    a_s, a16_s, b_s, up_s = [], [], [], []
    for i in range(warmup + samples):
        ta, ya = wall(host)
        tb, yb = wall(device)
        ta16, _ = wall(host16)
        tu, _ = wall(lambda: torch.from_numpy(pcm16).to(dev))
        if i == 0:
            assert ya.shape == yb.shape and ya.dtype == yb.dtype == torch.float32
            diff = float((ya - yb).abs().max())
            assert diff < 1e-4, diff
        print(f"{sr} Hz round {i}: host {ta:.3f} s, host x{THREADS} {ta16:.3f} s, device {tb:.4f} s", file=sys.stderr, flush=True)
        if i >= warmup:
            a_s.append(ta)
            a16_s.append(ta16)
            b_s.append(tb)
            up_s.append(tu)
        del ya, yb

    xd = torch.from_numpy(pcm16).to(dev)
    y = r(xd)
    n_out = y.numel()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    k_ms = []
    for i in range(warmup + max(samples, 20)):
        ev[0].record()
        r(xd)
        ev[1].record()
        torch.cuda.synchronize()
        if i >= warmup:
            k_ms.append(ev[0].elapsed_time(ev[1]))
    bytes_alg = 2 * n_in + 4 * n_out
    rate = bytes_alg / (statistics.median(k_ms) * 1e-3)
    fbank_s, model_s = [], []
    for i in range(warmup + samples):
        tf, feats = wall(lambda: ex.extract_long(y))
        tm, _ = wall(lambda: model.engine.predict_windows(feats, precision="fp16"))
        if i >= warmup:
            fbank_s.append(tf)
            model_s.append(tm)
    pool.shutdown()
    return {"sr_in": sr, "up": up, "down": down, "taps_per_output": r.K, "n_in": n_in, "n_out": n_out,
            "host_route_s": spread(a_s), "host_route_16_threads_s": spread(a16_s), "device_route_s": spread(b_s),
            "int16_upload_alone_s": spread(up_s), "max_abs_diff_device_vs_scipy_f32": diff,
            "host_over_device_median": round(statistics.median(a_s) / statistics.median(b_s), 2),
            "host16_over_device_median": round(statistics.median(a16_s) / statistics.median(b_s), 2),
            "kernel_ms": spread(k_ms, 4), "kernel_algorithmic_bytes": bytes_alg, "kernel_bytes_per_s_median": round(rate, 0),
            "kernel_fraction_of_8TBs_hbm_peak": round(rate / HBM_PEAK, 4),
            "fbank_launch_s": spread(fbank_s), "model_pass_fp16_s": spread(model_s)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", type=str, default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_resample.py needs an MI355X (a CPU run says nothing about these legs)")
    import bench
    import config
    from utils import get_feat_extractor
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ex = get_feat_extractor(config.FEAT["num_samples"], config.FEAT["num_filters"])
    model = bench._make_model(0.0, dev, degenerate_ok=False)
    model.eval()
    rec = {"metric": "rate conversion of one channel to 16 kHz: host route (scipy + upload) against device route (upload + HIP kernel)",
           "unit": "s", "gpu": torch.cuda.get_device_name(dev), "cpu_model": bench._cpu_model(), "host_cores": os.cpu_count(),
           "host_threads_used": THREADS, "torch": torch.__version__, "minutes": a.minutes, "samples": a.samples, "warmup": a.warmup,
           "channels": [channel(sr, a.minutes, a.samples, a.warmup, dev, ex, model) for sr in (48000, 44100)]}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
