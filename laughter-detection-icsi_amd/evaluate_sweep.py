#!/usr/bin/env python3
"""Precision and recall of the threshold sweep against the transcript, from saved probability tracks.

Counterpart of the reference's evaluation (analysis/analyse.py: create_evaluation_df :227-266, eval_preds :152-225,
calc_sum_stats :269-298, on the indices of analysis/preprocess.py).  The reference gets there through one TextGrid file per
(channel, threshold, min_length) that segment_laughter.py writes and analyse.py reads back; here the tracks
`segment_laughter.py --save_probs` wrote are swept and scored directly:

    python evaluate_sweep.py --probs_dir <dir with <meeting>/<chan>.npy> --transcripts rows.csv --channels channels.csv \\
        --thresholds 0,0.05,...,1 --min_lengths 0,0.1,0.2 --out_dir <out>

--transcripts: CSV with the columns of the reference's parse.py DataFrames (meeting_id, part_id, chan, start, end, length, type,
laugh_type; type in laugh / speech / noise / invalid).  --channels: CSV meeting_id, part_id, chan, length (seconds; an empty part_id
for a channel that belongs to no participant -- it is not evaluated, analyse.py:27-28).  The frame rate of a channel is its frame
count over its length (segment_laughter.py:103-104) unless --fps is given.

Writes `eval_df_per_meeting.csv` (the 14 columns of analyse.py:255-257) and `sum_stats.csv` (config.py:38-39 of the reference).
`--scorer device` (default `host`) uploads all tracks as one NaN-padded (C, T) tensor and scores the whole sweep on the GPU
(csrc/runs.hip + csrc/score.hip through sweep_eval.score_sweep_device); both scorers write the same bytes.
`--lowpass CUTOFF` (default: off) smooths every track first, as the reference's lowpass (laugh_segmenter.py:49-55) does before
its thresholds: on the host with scipy, under the device scorer on the GPU (csrc/lowpass.hip) with each track's true length.
`--median FRAMES` (default: off; not in the reference) passes every track through a median filter of FRAMES frames first (odd,
1..1023; the ends replicated): laugh_segmenter.median_filter under the host scorer, csrc/rankfilt.hip under the device scorer with
each track's true length -- the same values bit for bit, so both scorers still write the same bytes.  Not together with --lowpass.
`--offset_drops` / `--min_gaps` (default: absent) add hysteresis and gap filling to the sweep (laugh_segmenter.binarize_instances
under the host scorer, csrc/binarize.hip under the device scorer): the CSVs get the columns offset_drop and min_gap behind min_len
and the summary is grouped by all four.  Without the two flags the files are what they were.
`--events` (default: off; not in the reference, which counts events and never matches them) also writes
`event_df_per_meeting.csv` and `event_sum_stats.csv`: event-level precision, recall and F1, fragments per touched event and mean
onset / offset errors (sweep_eval.event_rows; the convention stands above lad_score_events in include/lad_hip.h), with
`--event_min_overlap_ms` and `--event_min_overlap_pct` deciding when an event or a prediction counts as hit; under the device
scorer from csrc/events.hip.  Without the flag the directory holds the two files above and nothing else.
`--penalties` (default: absent; not in the reference) decodes every track with the two-state Viterbi decoder instead of cutting it
frame by frame (laugh_segmenter.viterbi_instances under the host scorer, csrc/viterbi.hip under the device scorer): a frame counts
its log-odds relative to the threshold, every event costs the penalty in nats, and the best set of events is scored.  The CSVs get
the column penalty behind min_len.  It cannot be combined with --offset_drops / --min_gaps.
`--threshold_grid N` (default: absent) evaluates the dense grid of thresholds i / N, i = 0..N, instead of a list: every threshold
from one component tree per track (sweep_eval.score_surface_host under the host scorer, csrc/surface.hip through
sweep_eval.score_surface_device under the device scorer, `--lowpass` as above).  The two CSVs keep their columns, and
`pr_summary.csv` (min_len, average_precision, best_f1, best_f1_threshold: sweep_eval.pr_summary) is written next to them.  It
cannot be combined with an explicit --thresholds, nor with --offset_drops, --min_gaps, --penalties or --events, whose tables are not
nested in the threshold.  Without the flag the files are what they were.
`--event_grid N` (default: absent) is the dense grid with the event-level scores: the thresholds i / N as above, the three files of
`--threshold_grid N`, the two event files of `--thresholds <the same list> --events` (criteria from `--event_min_overlap_ms` /
`--event_min_overlap_pct`) and `event_pr_summary.csv` (min_len, event_average_precision, best_event_f1, best_event_f1_threshold:
sweep_eval.event_pr_summary), both score arrays from the same component tree (sweep_eval.score_surface_host(..., events=) under
the host scorer, csrc/surface_events.hip through sweep_eval.score_surface_device(..., events=) under the device scorer).  It
cannot be combined with --thresholds, --threshold_grid, --events, --offset_drops, --min_gaps or --penalties.
`--bootstrap B` (default: absent; not in the reference) also writes `sum_stats_ci.csv`: per setting precision, recall and F1 with a
percentile-bootstrap interval each and the number of valid replicates (sweep_eval.bootstrap_sum_stats_host under the host scorer,
csrc/bootstrap.hip through sweep_eval.bootstrap_sum_stats_device under the device scorer: the same bytes), from B resamples of the
recording units (`--bootstrap_unit channel`, the default, or `meeting`), the resamples a pure function of `--bootstrap_seed`
(default 0), the interval the central `--bootstrap_level` per cent (default 95).  With `--events` or `--event_grid` it also writes
`event_sum_stats_ci.csv` (event precision and recall; with `--bootstrap_event_f1` also event_f1, event_f1_lo and event_f1_hi in
front of n_boot_valid: event F1 is not a ratio of sums, its replicates are exact harmonic means ordered by
lad_bootstrap_pair_quantiles).  It works with every decoder family and both grids.  Without the flag the directory holds what it
held before.
`--compare_probs_dir DIR` (needs `--bootstrap`; default: absent) is a second system B for the same channels: its tracks go through
the same smoother, decoder and scorer as those of `--probs_dir` (system A), and `sum_stats_diff.csv` has per setting both systems'
precision, recall and F1, the exact difference A - B, its interval under the same resamples and the share of resamples in which A
is strictly greater (sweep_eval.bootstrap_diff_sum_stats_host / _device: the same bytes under either scorer); with `--events` /
`--event_grid` also `event_sum_stats_diff.csv`, for event precision and recall.  Every other file is that of `--probs_dir` alone.
`--calibration_report` (default: off; not in the reference) also writes `calibration.csv` -- per meeting and for `all` the
threshold-free, frame-level figures of the tracks as they are evaluated (behind `--calibration`, `--lowpass` / `--median`): laugh
and non-laugh milliseconds, Brier score, NLL, ECE / MCE over `--calibration_bins` bins (default 15), ROC AUC and average precision
(calibration.calibration_figures) -- and `reliability.csv`, the reliability table of all meetings together.  Both come from one
label histogram grouped by meeting (calibration.label_histogram_host under the host scorer, csrc/calibration.hip through
calibration.label_histogram_device under the device scorer: the same integers, so the same bytes -- except behind `--lowpass`, where
the device filter equals scipy's only within the rounding of float64 and a smoothed value next to a bucket's edge may fall on
either side; behind `--median` and without a smoother the two routes see the same values bit for bit).
`--fit_calibration {platt,temperature,isotonic}` (default: absent) fits a calibration map on the tracks as loaded, before any
smoothing, and writes `calibration_table.npz` (the 65537-entry table, the method, its parameters, the figures before and after).
`--calibration FILE` (default: absent) applies such a table to every track first, before `--lowpass` / `--median` and every
decoder (calibration.apply_calibration, or lad_track_remap under the device scorer): fit on the dev split, apply on the test split.
With `--compare_probs_dir` the one table is applied to both systems, as the smoother and the decoder are; two systems that need a
table each are calibrated beforehand.  Not together with `--fit_calibration`.  Without the three flags the directory holds what it held before.
"""
import argparse
import csv
import os
import sys

_PKG = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.join(_PKG, "utils"), _PKG):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

import calibration  # noqa: E402
import laugh_segmenter  # noqa: E402
import sweep_eval  # noqa: E402

SURFACE_MAX_LEVELS = 4096      # include/lad_hip.h: lad_surface_max_levels() (the host scorer takes the same grids)
MAX_REPLICATES = 4096          # ... lad_bootstrap_max_replicates()


def read_csv(path, columns, numeric):
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    for r in rows:
        missing = [c for c in columns if c not in r]
        if missing:
            raise ValueError(f"{path} lacks the columns {missing}")
        for c in numeric:
            r[c] = float(r[c])
    return rows


def load_tracks(probs_dir, index):
    """[(meeting_id, chan)], [track] for every <meeting>/<chan>.npy whose channel the channel table lists, in sorted order."""
    known = set(index.channels())
    channels, tracks = [], []
    for meeting in sorted(os.listdir(probs_dir)):
        mdir = os.path.join(probs_dir, meeting)
        if not os.path.isdir(mdir):
            continue
        for name in sorted(os.listdir(mdir)):
            if name.endswith(".npy") and (meeting, name[:-4]) in known:
                channels.append((meeting, name[:-4]))
                tracks.append(np.load(os.path.join(mdir, name)).reshape(-1))
    if not channels:
        raise ValueError(f"no <meeting>/<chan>.npy under {probs_dir} matches the channel table")
    return channels, tracks


def cutoff_arg(text):
    """--lowpass: a cutoff of Nyquist strictly between 0 and 1 (scipy.signal.butter's range)."""
    value = float(text)
    if not 0.0 < value < 1.0:
        raise argparse.ArgumentTypeError(f"the cutoff must lie strictly between 0 and 1 (of Nyquist), got {text}")
    return value


def window_arg(text):
    """--median: an odd number of frames from 1 to 1023 (include/lad_hip.h: lad_rank_filter_max_window())."""
    try:
        value = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"an odd integer from 1 to 1023, got {text}")
    if not 1 <= value <= 1023 or value % 2 == 0:
        raise argparse.ArgumentTypeError(f"an odd integer from 1 to 1023, got {text}")
    return value


def float_list(text):
    """--offset_drops / --min_gaps: a comma-separated list of non-negative numbers."""
    values = [float(t) for t in text.split(',')]
    if not all(np.isfinite(v) and v >= 0 for v in values):
        raise argparse.ArgumentTypeError(f"finite values >= 0, got {text}")
    return values


def non_negative_int(text):
    value = int(text)
    if value < 0:
        raise argparse.ArgumentTypeError(f"an integer >= 0, got {text}")
    return value


def percent(text):
    value = int(text)
    if not 0 <= value <= 100:
        raise argparse.ArgumentTypeError(f"an integer in 0..100, got {text}")
    return value


def grid_size(text):
    """--threshold_grid: N steps from 0 to 1, N + 1 levels, at most as many as one call of lad_score_surface takes."""
    value = int(text)
    if not 1 <= value <= SURFACE_MAX_LEVELS - 1:
        raise argparse.ArgumentTypeError(f"an integer in 1..{SURFACE_MAX_LEVELS - 1}, got {text}")
    return value


def replicates_arg(text):
    """--bootstrap: as many replicates as one call of lad_bootstrap_quantiles takes (the host form takes the same range)."""
    value = int(text)
    if not 1 <= value <= MAX_REPLICATES:
        raise argparse.ArgumentTypeError(f"an integer in 1..{MAX_REPLICATES}, got {text}")
    return value


def level_arg(text):
    """--bootstrap_level: a decimal strictly between 0 and 100, kept as text (bootstrap.quantile_pairs reads it exactly)."""
    try:
        import bootstrap
        bootstrap.quantile_pairs(text)
    except (ValueError, ZeroDivisionError):
        raise argparse.ArgumentTypeError(f"a decimal strictly between 0 and 100, got {text}")
    return text


def bins_arg(text):
    """--calibration_bins: the equal-width bins of ECE, MCE and the reliability table."""
    value = int(text)
    if not 1 <= value <= 65537:
        raise argparse.ArgumentTypeError(f"an integer in 1..65537, got {text}")
    return value


def upload(tracks, table=None):
    """All tracks as one NaN-padded (C, T) GPU tensor: float32 if every track is float16 / float32, else float64.  table: a
    calibration table, applied on the device first (the result is float64; the padding stays NaN)."""
    import torch
    dtype = np.float32 if all(t.dtype in (np.float16, np.float32) for t in tracks) else np.float64
    padded = np.full((len(tracks), max(len(t) for t in tracks)), np.nan, dtype)
    for c, t in enumerate(tracks):
        padded[c, :len(t)] = t
    probs = torch.from_numpy(padded).cuda()
    return probs if table is None else laugh_segmenter.apply_calibration_device(probs, table)


def score_device(tracks, channels, thresholds, min_lengths, fps, index, lowpass=None, surface=False, median=None, table=None,
                 **axes_and_events):
    lengths = [len(t) for t in tracks] if lowpass is not None or median is not None else None
    score = sweep_eval.score_surface_device if surface else sweep_eval.score_sweep_device
    return score(upload(tracks, table), channels, thresholds, min_lengths, fps, index, lowpass=lowpass, lengths=lengths,
                 **({} if median is None else {"median": median}), **axes_and_events)


def write_csv(path, columns, rows):
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(columns)
        for r in rows:
            w.writerow([repr(v) if isinstance(v, float) else v for v in r])


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument('--probs_dir', required=True, type=str, help='<meeting>/<chan>.npy, as segment_laughter.py --save_probs writes')
    parser.add_argument('--transcripts', required=True, type=str, help='CSV: meeting_id,part_id,chan,start,end,length,type,laugh_type')
    parser.add_argument('--channels', required=True, type=str, help='CSV: meeting_id,part_id,chan,length')
    parser.add_argument('--thresholds', type=str, default=None,
                        help='Single value or comma-separated list of thresholds to evaluate; default: 0.5')
    parser.add_argument('--threshold_grid', type=grid_size, default=None, metavar='N',
                        help=f'(not in the reference) evaluate the thresholds i / N, i = 0..N, N in 1..{SURFACE_MAX_LEVELS - 1}, all from one '
                             'component tree per track, and also write pr_summary.csv (average precision and the best F1 per min_len); '
                             'not with --thresholds, --offset_drops, --min_gaps, --penalties or --events; default: absent')
    parser.add_argument('--event_grid', type=grid_size, default=None, metavar='N',
                        help='(not in the reference) --threshold_grid N with the event-level scores of every threshold from the same '
                             'component tree: also writes event_df_per_meeting.csv, event_sum_stats.csv and event_pr_summary.csv (event '
                             'average precision and the best event F1 per min_len); not with --thresholds, --threshold_grid, --events, '
                             '--offset_drops, --min_gaps or --penalties; default: absent')
    parser.add_argument('--min_lengths', type=str, default='0.2', help='Single value or comma-separated list of min_lengths to evaluate')
    parser.add_argument('--fps', type=float, default=None, help='frames per second of every track (default: frames / channel length)')
    parser.add_argument('--scorer', type=str, default='host', choices=['host', 'device'],
                        help='host: laugh_segmenter.get_laughter_instances + sweep_eval.score_instances per channel; '
                             'device: the sweep and its scores on the GPU (csrc/runs.hip, csrc/score.hip)')
    parser.add_argument('--lowpass', type=cutoff_arg, default=None, metavar='CUTOFF',
                        help='smooth every track before the sweep: second-order Butterworth at CUTOFF of Nyquist, forwards and '
                             'backwards (laugh_segmenter.lowpass under the host scorer, csrc/lowpass.hip under the device scorer; the '
                             "reference's own cutoff is 0.01); default: off")
    parser.add_argument('--median', type=window_arg, default=None, metavar='FRAMES',
                        help='(not in the reference) pass every track through a median filter of FRAMES frames before the sweep (odd, '
                             '1..1023, the ends replicated: laugh_segmenter.median_filter under the host scorer, csrc/rankfilt.hip under '
                             'the device scorer); not with --lowpass; default: off')
    parser.add_argument('--offset_drops', type=float_list, default=None,
                        help='(not in the reference) comma-separated list: hysteresis, an event that starts above a threshold lasts '
                             'until the track falls to or below threshold - drop; default: absent (no hysteresis axis)')
    parser.add_argument('--min_gaps', type=float_list, default=None,
                        help='(not in the reference) comma-separated list of seconds: events separated by a pause of at most this '
                             'become one, before the min_length filter; default: absent (no gap-filling axis)')
    parser.add_argument('--penalties', type=float_list, default=None,
                        help='(not in the reference) comma-separated list of nats: two-state Viterbi decoding of every track, a frame '
                             'counting its log-odds relative to the threshold and every event costing this much; default: absent '
                             '(the frame-by-frame sweep)')
    parser.add_argument('--events', action='store_true',
                        help='(not in the reference) also write event_df_per_meeting.csv and event_sum_stats.csv: event-level '
                             'precision / recall / F1, fragmentation and onset / offset errors against the merged laugh intervals')
    parser.add_argument('--event_min_overlap_ms', type=non_negative_int, default=1,
                        help='an event (a prediction) is hit if at least this many of its milliseconds are predicted (transcribed '
                             'laughter), and at least 1; default: 1')
    parser.add_argument('--event_min_overlap_pct', type=percent, default=0,
                        help='... and at least this many per cent of it (of its part outside INVALID), 0..100; default: 0')
    parser.add_argument('--bootstrap', type=replicates_arg, default=None, metavar='B',
                        help='(not in the reference) also write sum_stats_ci.csv (and event_sum_stats_ci.csv with --events / '
                             f'--event_grid): percentile-bootstrap intervals from B resamples of the recording units, B in 1..{MAX_REPLICATES}; '
                             'default: absent')
    parser.add_argument('--bootstrap_seed', type=non_negative_int, default=0,
                        help='the resamples are a pure function of this seed and the replicate number; default: 0')
    parser.add_argument('--bootstrap_level', type=level_arg, default='95', metavar='PERCENT',
                        help='the central interval reported, read as an exact decimal (95 -> the quantiles 1/40 and 39/40); default: 95')
    parser.add_argument('--bootstrap_unit', type=str, default='channel', choices=['channel', 'meeting'],
                        help='what is resampled: the evaluated channels, or the meetings (three meetings have ten distinct '
                             'resamples); default: channel')
    parser.add_argument('--bootstrap_event_f1', action='store_true',
                        help='with --bootstrap and --events / --event_grid: event_sum_stats_ci.csv also has event_f1 with its interval')
    parser.add_argument('--compare_probs_dir', type=str, default=None, metavar='DIR',
                        help='(needs --bootstrap) a second system for the same channels, <meeting>/<chan>.npy as --probs_dir: also write '
                             'sum_stats_diff.csv (and event_sum_stats_diff.csv with --events / --event_grid), the difference --probs_dir '
                             'minus DIR of every figure with its interval under the same resamples; default: absent')
    parser.add_argument('--calibration_report', action='store_true',
                        help='(not in the reference) also write calibration.csv (per meeting and for all: Brier score, NLL, ECE, MCE, '
                             'ROC AUC, average precision of the tracks as they are evaluated) and reliability.csv; the same bytes under '
                             'either --scorer except behind --lowpass (the two filters agree within float64 rounding); default: off')
    parser.add_argument('--calibration_bins', type=bins_arg, default=15, metavar='N',
                        help='the equal-width bins of ECE, MCE and the reliability table, 1..65537; default: 15')
    parser.add_argument('--fit_calibration', type=str, default=None, choices=list(calibration.METHODS),
                        help='(not in the reference) fit a calibration map on the tracks as loaded (Platt scaling, temperature scaling '
                             'or isotonic regression on the label histogram) and write calibration_table.npz; not with --calibration; '
                             'default: absent')
    parser.add_argument('--calibration', type=str, default=None, metavar='FILE',
                        help='(not in the reference) a calibration_table.npz: its table is applied to every track first, before '
                             '--lowpass / --median and every decoder (with --compare_probs_dir: to the tracks of both systems); '
                             'default: absent')
    parser.add_argument('--out_dir', required=True, type=str)
    return parser


def calibration_histogram(tracks, channels, fps, index, groups, scorer, table=None, lowpass=None, median=None):
    """The label histogram (G, 5, 65538) of the tracks behind the table and the smoother, on the host or on the device as `scorer`
    says: the tracks as they are evaluated, or with neither the tracks as loaded."""
    if scorer == "device":
        probs, lengths = upload(tracks, table), [len(t) for t in tracks]
        if lowpass is not None:
            probs = laugh_segmenter.lowpass_device(probs, cutoff=lowpass, lengths=lengths)
        elif median is not None:
            probs = laugh_segmenter.median_filter_device(probs, median, lengths=lengths)
        return calibration.label_histogram_device(probs, channels, fps, index, lengths=lengths, groups=groups)
    if table is not None:
        tracks = [laugh_segmenter.apply_calibration(t, table) for t in tracks]
    if lowpass is not None:
        tracks = [laugh_segmenter.lowpass(t, cutoff=lowpass) for t in tracks]
    elif median is not None:
        tracks = [laugh_segmenter.median_filter(t, median) for t in tracks]
    return calibration.label_histogram_host(tracks, channels, fps, index, groups=groups)


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.compare_probs_dir is not None and args.bootstrap is None:
        raise SystemExit("--compare_probs_dir needs --bootstrap: the comparison is an interval of the difference")
    if args.bootstrap_event_f1 and (args.bootstrap is None or not (args.events or args.event_grid is not None)):
        raise SystemExit("--bootstrap_event_f1 needs --bootstrap and --events or --event_grid")
    if args.median is not None and args.lowpass is not None:
        raise SystemExit("--median cannot be combined with --lowpass: they are two smoothers for the same place")
    if args.fit_calibration is not None and args.calibration is not None:
        raise SystemExit("--fit_calibration cannot be combined with --calibration: the fit is made on the tracks as loaded")
    table = None if args.calibration is None else calibration.load_table(args.calibration)
    grid = args.threshold_grid
    if args.event_grid is not None:
        for flag in ("thresholds", "threshold_grid", "events", "offset_drops", "min_gaps", "penalties"):
            if getattr(args, flag):
                raise SystemExit(f"--event_grid cannot be combined with --{flag}")
        grid = args.event_grid
        thresholds = [i / grid for i in range(grid + 1)]
    elif args.threshold_grid is not None:
        if args.thresholds is not None:
            raise SystemExit("--threshold_grid cannot be combined with an explicit --thresholds")
        for flag in ("offset_drops", "min_gaps", "penalties", "events"):
            if getattr(args, flag):
                raise SystemExit(f"--threshold_grid cannot be combined with --{flag}: its tables are not nested in the threshold")
        thresholds = [i / args.threshold_grid for i in range(args.threshold_grid + 1)]
    else:
        thresholds = [float(t) for t in (args.thresholds or '0.5').split(',')]
    min_lengths = [float(t) for t in args.min_lengths.split(',')]
    rows = read_csv(args.transcripts, sweep_eval.ROW_COLUMNS, ("start", "end", "length"))
    chans = read_csv(args.channels, sweep_eval.CHANNEL_COLUMNS, ("length",))
    index = sweep_eval.TranscriptIndex(rows, chans)
    channels, tracks = load_tracks(args.probs_dir, index)
    systems = [tracks]
    if args.compare_probs_dir is not None:
        channels_b, tracks_b = load_tracks(args.compare_probs_dir, index)
        if channels_b != channels:
            raise SystemExit(f"--compare_probs_dir holds {len(channels_b)} channels, --probs_dir {len(channels)}: they must be the same "
                             f"(differing: {sorted(set(channels) ^ set(channels_b))[:4]})")
        systems.append(tracks_b)
    length = {(c["meeting_id"], c["chan"]): c["length"] for c in chans}
    if args.lowpass is not None:
        for (meeting, chan), t in [ct for system in systems for ct in zip(channels, system)]:
            if len(t) <= 9:
                raise ValueError(f"--lowpass: the track of {meeting}/{chan} has {len(t)} frames, the filter needs more than 9")
    extra = dict(offset_drops=args.offset_drops, min_gaps=args.min_gaps, penalties=args.penalties)
    try:
        decoder, _ = laugh_segmenter.decoder_for(**extra)
    except ValueError:
        raise SystemExit("--penalties cannot be combined with --offset_drops / --min_gaps")
    with_events = args.events or args.event_grid is not None
    criteria = dict(events=(args.event_min_overlap_ms, args.event_min_overlap_pct)) if with_events else {}

    calibrated = {} if table is None else {"table": table}

    def frame_rates(tracks):
        return [args.fps if args.fps is not None else len(t) / length[mc] for mc, t in zip(channels, tracks)]

    def score(tracks):
        fps = frame_rates(tracks)
        if args.scorer == "device":
            if grid is not None:
                return score_device(tracks, channels, thresholds, min_lengths, fps, index, lowpass=args.lowpass, surface=True,
                                    median=args.median, **calibrated, **criteria)
            return score_device(tracks, channels, thresholds, min_lengths, fps, index, lowpass=args.lowpass, median=args.median, **calibrated,
                                **extra, **criteria)
        if table is not None:
            tracks = [laugh_segmenter.apply_calibration(t, table) for t in tracks]
        if args.lowpass is not None:
            tracks = [laugh_segmenter.lowpass(t, cutoff=args.lowpass) for t in tracks]
        elif args.median is not None:
            tracks = [laugh_segmenter.median_filter(t, args.median) for t in tracks]
        if grid is not None:
            return sweep_eval.score_surface_host(tracks, channels, thresholds, min_lengths, fps, index, **criteria)
        return sweep_eval.score_sweep_host(tracks, channels, thresholds, min_lengths, fps, index, **extra, **criteria)
    scores = score(tracks)
    if with_events:
        scores, events = scores
    per_meeting = sweep_eval.eval_rows(scores, channels, thresholds, min_lengths, index, **extra)
    os.makedirs(args.out_dir, exist_ok=True)

    def write(name, base_columns, rows):
        write_csv(os.path.join(args.out_dir, name), sweep_eval.columns(base_columns, decoder), rows)
    write("eval_df_per_meeting.csv", sweep_eval.EVAL_COLUMNS, per_meeting)
    sum_stats = sweep_eval.calc_sum_stats(per_meeting, **extra)
    write("sum_stats.csv", sweep_eval.SUM_COLUMNS, sum_stats)
    if grid is not None:
        write_csv(os.path.join(args.out_dir, "pr_summary.csv"), sweep_eval.PR_COLUMNS, sweep_eval.pr_summary(sum_stats))
    if with_events:
        per_meeting_events = sweep_eval.event_rows(scores, events, channels, thresholds, min_lengths, index, **extra)
        write("event_df_per_meeting.csv", sweep_eval.EVENT_COLUMNS, per_meeting_events)
        event_stats = sweep_eval.event_sum_stats(per_meeting_events, **extra)
        write("event_sum_stats.csv", sweep_eval.EVENT_SUM_COLUMNS, event_stats)
        if args.event_grid is not None:
            write_csv(os.path.join(args.out_dir, "event_pr_summary.csv"), sweep_eval.EVENT_PR_COLUMNS,
                      sweep_eval.event_pr_summary(event_stats))
    if args.bootstrap is not None:
        resample = sweep_eval.bootstrap_sum_stats_device if args.scorer == "device" else sweep_eval.bootstrap_sum_stats_host
        ci = resample(scores, channels, thresholds, min_lengths, index, n_boot=args.bootstrap, seed=args.bootstrap_seed,
                      level=args.bootstrap_level, unit=args.bootstrap_unit, events=events if with_events else None, **extra,
                      **({"event_f1": True} if args.bootstrap_event_f1 else {}))
        if with_events:
            ci, event_ci = ci
            write("event_sum_stats_ci.csv", sweep_eval.EVENT_SUM_CI_F1_COLUMNS if args.bootstrap_event_f1 else sweep_eval.EVENT_SUM_CI_COLUMNS,
                  event_ci)
        write("sum_stats_ci.csv", sweep_eval.SUM_CI_COLUMNS, ci)
    if args.compare_probs_dir is not None:
        scores_b = score(systems[1])
        scores_b, events_b = scores_b if with_events else (scores_b, None)
        compare = sweep_eval.bootstrap_diff_sum_stats_device if args.scorer == "device" else sweep_eval.bootstrap_diff_sum_stats_host
        diff = compare(scores, scores_b, channels, thresholds, min_lengths, index, n_boot=args.bootstrap, seed=args.bootstrap_seed,
                       level=args.bootstrap_level, unit=args.bootstrap_unit, events_a=events if with_events else None, events_b=events_b,
                       **extra)
        if with_events:
            diff, event_diff = diff
            write("event_sum_stats_diff.csv", sweep_eval.EVENT_SUM_DIFF_COLUMNS, event_diff)
        write("sum_stats_diff.csv", sweep_eval.SUM_DIFF_COLUMNS, diff)
    if args.calibration_report:
        meetings = sorted({m for m, _ in channels})
        hist = calibration_histogram(tracks, channels, frame_rates(tracks), index, [meetings.index(m) for m, _ in channels], args.scorer,
                                     table=table, lowpass=args.lowpass, median=args.median)
        figures = [calibration.calibration_figures(h, n_bins=args.calibration_bins) for h in (*hist, hist.sum(axis=0))]
        write_csv(os.path.join(args.out_dir, "calibration.csv"), calibration.CALIBRATION_COLUMNS,
                  [calibration.figure_row(name, f) for name, f in zip(meetings + ["all"], figures)])
        write_csv(os.path.join(args.out_dir, "reliability.csv"), calibration.RELIABILITY_COLUMNS, calibration.reliability_rows(figures[-1]))
    if args.fit_calibration is not None:
        row = calibration_histogram(tracks, channels, frame_rates(tracks), index, [0] * len(channels), args.scorer)[0]
        fitted, parameters = calibration.fit(row, args.fit_calibration)
        calibration.save_table(os.path.join(args.out_dir, "calibration_table.npz"), fitted, args.fit_calibration, parameters,
                               calibration.calibration_figures(row, n_bins=args.calibration_bins),
                               calibration.calibration_figures(calibration.remap_histogram(row, fitted), n_bins=args.calibration_bins))
    print(f"{len(channels)} channels, {int(np.prod(scores.shape[1:-1]))} settings ({args.scorer} scorer): "
          f"{len(per_meeting)} rows -> {args.out_dir}")


if __name__ == '__main__':
    main()
