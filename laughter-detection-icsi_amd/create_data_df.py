#!/usr/bin/env python3
"""Write {split}_df.csv from the transcript tables: counterpart of the reference's create_data_df.py (:98-206), one device draw.

    python create_data_df.py --transcripts T.csv --channels C.csv --splits SPLITS.json --out_dir DIR [--preset reference]
                             [--seed 23] [--epoch 0]

--transcripts / --channels are the CSVs evaluate_sweep.py reads (the columns of sweep_eval.ROW_COLUMNS / CHANNEL_COLUMNS);
SPLITS.json maps split name -> list of meeting ids (the reference hard-codes Lhotse's ICSI partition, :15-29; bring your own).
Per laugh row of a split's meetings the preset's negatives and windows of the row are drawn on the GPU (sampling.Sampler:
csrc/sample.hip) at the configured frame rate, FEAT['num_samples'], and written in the reference's schema (:171-172), times
rounded to 2 decimals (:182).  At 100 frames per second those decimals are the drawn frame numbers exactly:
segments.table_from_csv of the output gives the draw back.  The default seed is the reference's random_seed (config.py:57 there).
"""
import argparse
import csv
import json
import os
import sys

_PKG = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.join(_PKG, "utils"), _PKG):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import config as config_mod  # noqa: E402
import sampling  # noqa: E402
import sweep_eval  # noqa: E402
from evaluate_sweep import read_csv  # noqa: E402


def check_rows(rows, split, meetings):
    """The asserts of create_data_df.py:185-203."""
    for r in rows:
        d = dict(zip(sampling.COLUMNS, r))
        if min(d["start"], d["duration"], d["sub_start"], d["sub_duration"]) < 0:
            raise AssertionError(f"{split}: row with a negative time: {r}")
        if d["label"] not in (0, 1):
            raise AssertionError(f"{split}: label {d['label']} is not 0 or 1")
        if d["audio_path"].split("/")[0] not in meetings:
            raise AssertionError(f"{split}: {d['audio_path']} belongs to a meeting outside the split")


def create_data_df(transcripts, channels, splits, out_dir, preset="reference", seed=23, epoch=0, device="cuda"):
    """-> ({split: number of rows}, laugh rows left out because they hold no whole frame); writes out_dir/{split}_df.csv."""
    fps = config_mod.FEAT['num_samples']
    p = config_mod.SAMPLING[preset] if isinstance(preset, str) else preset
    T = int(round(float(p.get('subsample_duration', 1.0)) * fps))
    pools = sampling.SegmentPools.from_transcripts(transcripts, channels, fps=fps, T=T)
    os.makedirs(out_dir, exist_ok=True)
    written = {}
    for split, meetings in splits.items():
        unknown = [m for m in meetings if m not in pools.meetings]
        if unknown:
            raise ValueError(f"split {split} names meetings the transcript tables do not hold: {unknown}")
        rows = sampling.Sampler(pools, pools.plan(p, meetings), seed, device=device).rows(epoch)
        check_rows(rows, split, set(meetings))
        with open(os.path.join(out_dir, f"{split}_df.csv"), "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(sampling.COLUMNS)
            w.writerows(rows)
        written[split] = len(rows)
    return written, pools.dropped


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--transcripts", required=True)
    ap.add_argument("--channels", required=True)
    ap.add_argument("--splits", required=True, help="JSON: {split: [meeting ids]}")
    ap.add_argument("--out_dir", required=True)
    ap.add_argument("--preset", default="reference", choices=list(config_mod.SAMPLING))
    ap.add_argument("--seed", type=int, default=23)
    ap.add_argument("--epoch", type=int, default=0)
    args = ap.parse_args(argv)
    rows = read_csv(args.transcripts, sweep_eval.ROW_COLUMNS, ("start", "end", "length"))
    chans = read_csv(args.channels, sweep_eval.CHANNEL_COLUMNS, ("length",))
    with open(args.splits) as f:
        splits = json.load(f)
    written, dropped = create_data_df(rows, chans, splits, args.out_dir, args.preset, args.seed, args.epoch)
    if dropped:
        print(f"{dropped} laugh rows hold no whole frame and are left out")
    for split, n in written.items():
        print(f"{split}: {n} rows -> {os.path.join(args.out_dir, split + '_df.csv')}")


if __name__ == "__main__":
    main()
