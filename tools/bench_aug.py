#!/usr/bin/env python3
"""Throughput of ResNetBigger at the resnet_with_augmentation widths ([128, 64, 32, 32], 128 x 44 windows) on one MI355X.

    python tools/bench_aug.py [--batches 512,32] [--steps 10] [--warmup 3] [--windows 20000]

Prints one JSON line: per batch size the fused train step (train_step: forward, backward, clip, Adam; graphed below 256 segments as
bench.py does), and fp32 predict_windows over a synthetic track.  FLOP counts are the model's matrix work (convolutions + head:
19.5 GFLOP per training segment, 6.50 per forward window) against the 157.3 TFLOP/s f32 matrix peak.
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402,F401  (sys.path of the package)
from oracle import recipe  # noqa: E402

AUG = dict(linear_layer_size=128, filter_sizes=[128, 64, 32, 32])
T_FRAMES = 128
PEAK_F32 = 157.3e12


def fwd_flops(filter_sizes=(128, 64, 32, 32), H=T_FRAMES, W=44, feat=128):
    """Multiply-adds x 2 of one window's forward pass (every convolution + the two linear layers)."""
    macs = H * W * 9 * 1 * 64
    cin, h, w = 64, H, W
    for bi, cout in enumerate(filter_sizes):
        for j in range(2):
            stride = 2 if (bi > 0 and j == 0) else 1
            ho, wo = (h + stride - 1) // stride, (w + stride - 1) // stride
            c_in = cin if j == 0 else cout
            macs += ho * wo * 9 * c_in * cout + ho * wo * 9 * cout * cout
            if j == 0 and (stride != 1 or c_in != cout):
                macs += ho * wo * c_in * cout
            h, w = ho, wo
        cin = cout
    macs += feat * 32 + 32
    return 2 * macs


def time_it(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="512,32")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--windows", type=int, default=20000)
    ap.add_argument("--only", default="train,predict")
    args = ap.parse_args()
    import models
    with contextlib.redirect_stdout(io.StringIO()):
        m = models.ResNetBigger(dropout_rate=0.5, **AUG)
    sd = recipe.make_state(1, filter_sizes=tuple(AUG["filter_sizes"]), linear_layer_size=AUG["linear_layer_size"])
    full = m.state_dict()
    for k, v in sd.items():
        full[k] = torch.from_numpy(v.copy())
    m.load_state_dict(full)
    m.set_device("cuda")
    f1 = fwd_flops()
    out = {"model": "resnet_with_augmentation", "window": [T_FRAMES, 44], "fwd_gflop_per_window": round(f1 / 1e9, 3)}
    if "train" in args.only:
        m.train()
        for B in [int(b) for b in args.batches.split(",")]:
            x = torch.from_numpy(recipe.make_features(2, B, n_frames=T_FRAMES)).cuda()
            t = torch.from_numpy(recipe.make_labels(3, B)).cuda()
            if B < 256:
                step = m.make_graphed_train_step(B, n_frames=T_FRAMES)
                dt = time_it(lambda: step(x, t), args.steps, args.warmup)
            else:
                dt = time_it(lambda: m.train_step(x, t), args.steps, args.warmup)
            out[f"train_bs{B}"] = {"ms_per_step": round(dt * 1e3, 3), "segments_per_s": round(B / dt, 1),
                                   "f32_peak_share": round(3 * f1 * B / dt / PEAK_F32, 3)}
    if "predict" in args.only:
        m.eval()
        g = torch.Generator().manual_seed(5)
        feats = (torch.randn(args.windows, 44, generator=g) * 2.0 - 8.0).cuda()
        dt = time_it(lambda: m.engine.predict_windows(feats, n_frames=T_FRAMES), max(1, args.steps // 5), 1)
        out["predict_fp32"] = {"windows": args.windows, "s": round(dt, 4), "windows_per_s": round(args.windows / dt, 1),
                               "f32_peak_share": round(f1 * args.windows / dt / PEAK_F32, 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
