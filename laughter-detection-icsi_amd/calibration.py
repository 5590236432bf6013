"""Calibration of the probability track against the transcript (csrc/calibration.hip).

Not in the reference, which treats the network's output as a probability and never checks it.  Everything built on the track since
the threshold sweep does the same: the Viterbi decoder scores a frame by its log-odds, --confidence reports a span's mean
probability, the bootstrap compares systems at fixed thresholds.  This module says whether a frame at 0.9 is laughter nine times in
ten, and repairs the track if it is not.

The primitive is the label histogram of a track (the convention is written out above lad_label_histogram in include/lad_hip.h): per
bucket of the track's value -- the 65537 buckets of the Viterbi decoder and one more slot for NaN frames -- the milliseconds of each
transcript class (INVALID, LAUGH, SPEECH, NOISE, SILENCE) that the frames in the bucket own.  Frame i of a channel owns the
milliseconds (m_i, m_{i+1}], m_j = rint(j / fps * 1000).  Integer sums only, so the host form, the device form and the model of the
tests agree for equality.  Every figure and every fit follows on the host from the 5 x 65538 integers of one histogram row.

    label_histogram_host     int64 (G, 5, 65538) in numpy (the parity form)
    label_histogram_device   the same array for tracks in GPU memory (lad_label_histogram).  No CPU fallback.
    calibration_figures      Brier, NLL, ECE / MCE, ROC AUC, average precision and the reliability table of one row
    fit_platt, fit_isotonic  a float64 (65537,) table per bucket; fit_platt(temperature_only=True) is temperature scaling
    apply_calibration        table[bucket] on the host, NaN kept
    apply_calibration_device the same on the device (lad_track_remap): a float64 track for every decoder, smoother and scorer
    remap_histogram          the histogram of the calibrated track from the histogram of the track, in integers
    save_table, load_table   calibration_table.npz (the same bytes for the same content)
"""
import io
import json
import math
import zipfile
from fractions import Fraction

import numpy as np

import laugh_segmenter as ls
import sweep_eval

BUCKETS = ls.VITERBI_BUCKETS + 1     # 65537 table entries, buckets 0..65536 (lad_viterbi_table_entries())
SLOTS = BUCKETS + 1                  # lad_label_histogram_slots(): the NaN frames behind the buckets
NAN_SLOT = BUCKETS
N_CLASSES = len(sweep_eval.CLASSES)
LAUGH = sweep_eval.CLASSES.index("laugh")
_DEN = 2 * BUCKETS                   # p_u = (2 u + 1) / _DEN: the middle of bucket u, as viterbi_emission_table takes it
PLATT_MAX_ITERATIONS = 100
CALIBRATION_COLUMNS = ["meeting", "pos_ms", "neg_ms", "invalid_ms", "nan_ms", "brier", "nll", "ece", "mce", "roc_auc", "average_precision"]
RELIABILITY_COLUMNS = ["bin", "lo", "hi", "ms", "mean_confidence", "laugh_share"]
METHODS = ("platt", "temperature", "isotonic")


def slots_of(track):
    """The slot of every frame, int64: floor(v * 65536) of the fixed probability v (laugh_segmenter.fix_probs), 65537 for NaN."""
    v = ls.fix_probs(np.asarray(track).reshape(-1))
    nan = np.isnan(v)
    u = np.floor(np.where(nan, 0.0, v) * float(ls.VITERBI_BUCKETS)).astype(np.int64)
    u[nan] = NAN_SLOT
    return u


def bucket_confidence():
    """p_u for u = 0..65536, float64: (2 u + 1) / (2 * 65537)."""
    return (2.0 * np.arange(BUCKETS, dtype=np.float64) + 1.0) / float(_DEN)


def _groups(groups, C, n_groups, check):
    """(None or int32 (C,), G).  groups=None: one group per channel, G = C.  Otherwise G = n_groups, or the largest group + 1 (at
    least 1) where it is not given: name it to keep trailing groups that no channel belongs to.  check: ValueError for what
    lad_label_histogram refuses -- a group outside -1..G-1, G outside 1..C, or G != C without groups (the device form leaves that
    to the library)."""
    if groups is None:
        if check and n_groups is not None and int(n_groups) != C:
            raise ValueError(f"without groups every channel is its own: n_groups {n_groups} must equal the {C} channels")
        return None, C if n_groups is None else int(n_groups)
    groups = np.ascontiguousarray(np.asarray(groups, dtype=np.int32).reshape(-1))
    if groups.shape != (C,):
        raise ValueError(f"{groups.size} groups for {C} channels")
    G = int(n_groups) if n_groups is not None else (max(int(groups.max()) + 1, 1) if C else 1)
    if check and C and not (1 <= G <= C and groups.min() >= -1 and groups.max() < G):
        raise ValueError(f"groups lie in -1..n_groups - 1 and n_groups in 1..channels, got {int(groups.min())}..{int(groups.max())} "
                         f"with n_groups {G} for {C} channels")
    return groups, G


def frame_ms(n, fps):
    """m_0..m_n of a channel of n frames, int64 (run_ms' expression: one IEEE division, one product, rint)."""
    return np.rint(np.arange(n + 1, dtype=np.float64) / np.float64(fps) * sweep_eval.FACTOR).astype(np.int64)


def label_histogram_host(tracks, channels, fps, index, lengths=None, groups=None, n_groups=None):
    """tracks: C arrays (float32 / float64, lengths may differ), smoothed or not; channels: C (meeting_id, chan); fps: a float or C
    floats; index: a TranscriptIndex; lengths: C frame counts (default: the whole of every track); groups: C ints in -1..G-1 (-1: the
    channel is left out; default: channel c is group c); n_groups: G, 1..C (default: the largest group + 1) -> int64 (G, 5, 65538):
    hist[g][k][slot] = the milliseconds of class k owned by the frames of group g's channels whose value lies in `slot`.  It
    refuses what lad_label_histogram refuses (ValueError).  The parity form of label_histogram_device."""
    channels = list(channels)
    C = len(channels)
    if len(tracks) != C:
        raise ValueError(f"{len(tracks)} tracks for {C} channels")
    f = ls.fps_per_channel(fps, C)
    groups, G = _groups(groups, C, n_groups, check=True)
    lengths = [len(t) for t in tracks] if lengths is None else [int(n) for n in lengths]
    if len(lengths) != C:
        raise ValueError(f"{len(lengths)} lengths for {C} channels")
    hist = np.zeros((G, N_CLASSES, SLOTS), np.int64)
    for c, (track, mc) in enumerate(zip(tracks, channels)):
        n = lengths[c]
        if not 1 <= n <= len(track):
            raise ValueError(f"lengths[{c}] = {n} is outside 1..{len(track)}")
        m = frame_ms(n, f[c])
        if m[-1] >= 2 ** 31:
            raise ValueError(f"millisecond overflow: {n} frames at fps {f[c]} end at {m[-1]} ms, int32 holds 2^31 - 1")
        g = c if groups is None else int(groups[c])
        if g < 0:
            continue
        slot = slots_of(np.asarray(track).reshape(-1)[:n])
        for k, iv in enumerate(index.scoring_sets(*mc)):
            if len(iv):
                np.add.at(hist[g, k], slot, np.diff(sweep_eval.coverage(iv, m)))
    return hist


def label_histogram_device(probs, channels, fps, index, lengths=None, groups=None, n_groups=None):
    """probs: (C, T) or (T,) float32 / float64 GPU tensor, smoothed or not -> the array of label_histogram_host for the same tracks,
    int64 numpy (G, 5, 65538): lad_label_histogram (include/lad_hip.h; csrc/calibration.hip), only the histogram crosses to the host.
    lengths: the true frame counts of a ragged tensor (frames behind them are not read; without them the NaN padding is counted in the
    NaN slot); groups, n_groups: as for the host form; index: a TranscriptIndex or the DeviceIndex of these channels.  What the
    library refuses (a length outside 1..T, a group or n_groups out of range, an fps that is not positive and finite, millisecond
    overflow) is a LadHipError.  No CPU fallback."""
    import torch

    import _hip
    p2, dtype, _ = _hip.device_track(probs, "label histogram")
    channels = list(channels)
    C, T = p2.shape
    if C != len(channels):
        raise ValueError(f"{C} tracks for {len(channels)} channels")
    fps_host = ls.fps_per_channel(fps, C, each=float)
    lengths = _hip.channel_lengths(lengths, C)
    groups, G = _groups(groups, C, n_groups, check=False)
    if C == 0 or T == 0:
        return np.zeros((G, N_CLASSES, SLOTS), np.int64)
    dix = index if isinstance(index, sweep_eval.DeviceIndex) else index.to_device(channels, p2.device)
    if dix.channels != channels or dix.device != p2.device:
        raise ValueError("the DeviceIndex was built for other channels or another device")
    with torch.cuda.device(p2.device):
        ws = _hip.workspace("lad_label_histogram_workspace_bytes", C, T, dix.n_intervals, device=p2.device)
        hist = torch.empty((G, N_CLASSES, SLOTS), dtype=torch.int64, device=p2.device)
        _hip.launch("lad_label_histogram", p2, dtype, C, T, lengths, dix.bounds, dix.offsets, dix.bounds_host, dix.offsets_host,
                    dix.n_intervals, torch.from_numpy(fps_host).to(p2.device), fps_host, groups, G, ws, hist)
        return hist.cpu().numpy()


# ---- figures of one histogram row ------------------------------------------------------------------------------------------------
def _row(hist_row):
    h = np.asarray(hist_row)
    if h.shape != (N_CLASSES, SLOTS) or h.dtype.kind not in "iu":
        raise ValueError(f"a histogram row is an integer array ({N_CLASSES}, {SLOTS}), got {h.dtype} {h.shape}")
    if (h < 0).any():
        raise ValueError("a histogram row holds no negative entry")
    return h.astype(np.int64)


def _pos_neg(hist_row):
    """(pos, neg): Python-int lists over the 65537 buckets: LAUGH, and SPEECH + NOISE + SILENCE."""
    h = _row(hist_row)
    return h[LAUGH, :BUCKETS].tolist(), (h[LAUGH + 1:, :BUCKETS].sum(axis=0)).tolist()


def _ratio(num, den):
    """num / den converted once (NaN for an empty denominator)."""
    return float(Fraction(num, den)) if den else float("nan")


def _exact_sum(terms):
    """(numerator, denominator) of the exact sum of Fractions, not reduced: the terms are added in pairs, then the pairs, so that
    the long products meet operands of their own size (a running sum over 65537 denominators would redo a megabit product per
    term)."""
    pairs = [(t.numerator, t.denominator) for t in terms] or [(0, 1)]
    while len(pairs) > 1:
        merged = [(a * d + c * b, b * d) for (a, b), (c, d) in zip(pairs[0::2], pairs[1::2])]
        if len(pairs) % 2:
            merged.append(pairs[-1])
        pairs = merged
    return pairs[0]


def calibration_figures(hist_row, n_bins=15):
    """The threshold-free figures of one histogram row (int (5, 65538)), a dict.  Positives are the LAUGH milliseconds, negatives
    SPEECH + NOISE + SILENCE; `invalid_ms` (the INVALID row, every slot) and `nan_ms` (what NaN frames own of the other four) are
    reported and used for nothing else.  The confidence of bucket u is p_u = (2 u + 1) / (2 * 65537).
        pos_ms, neg_ms      integers
        brier               sum pos_u (1 - p_u)^2 + neg_u p_u^2 over pos_ms + neg_ms
        nll                 nats per ms: -(sum pos_u log p_u + neg_u log(1 - p_u)) / (pos_ms + neg_ms); a float64 sum over the buckets
                            in ascending order, the positive term of a bucket before its negative one (math.log, math.log1p)
        ece, mce            over n_bins equal-width bins, bin = u * n_bins // 65537: the mass-weighted mean and the maximum of
                            |laugh share - mean confidence| over the bins that hold mass
        roc_auc             the Mann-Whitney statistic of the buckets, ties at one half
        average_precision   sum over descending buckets of (the recall gained at the bucket) * (the precision down to it)
        reliability         rows (lo, hi, ms, mean_confidence, laugh_share) per bin, NaN where the bin is empty
    Every figure but nll is computed in Python integers and fractions and converted once; a figure without a denominator (no
    positive, no negative or no mass) is NaN."""
    n_bins = int(n_bins)
    if n_bins < 1:
        raise ValueError(f"n_bins >= 1, got {n_bins}")
    h = _row(hist_row)
    pos, neg = _pos_neg(h)
    P, N = sum(pos), sum(neg)
    W = P + N
    occupied = [u for u in range(BUCKETS) if pos[u] or neg[u]]
    brier_num = sum(pos[u] * (_DEN - (2 * u + 1)) ** 2 + neg[u] * (2 * u + 1) ** 2 for u in occupied)
    total = 0.0
    for u in occupied:
        p = (2 * u + 1) / _DEN
        if pos[u]:
            total += -(pos[u] * math.log(p))
        if neg[u]:
            total += -(neg[u] * math.log1p(-p))
    bin_ms, bin_pos, bin_conf = [0] * n_bins, [0] * n_bins, [0] * n_bins          # bin_conf: sum of mass * (2 u + 1)
    for u in occupied:
        b = u * n_bins // BUCKETS
        bin_ms[b] += pos[u] + neg[u]
        bin_pos[b] += pos[u]
        bin_conf[b] += (pos[u] + neg[u]) * (2 * u + 1)
    gaps = [abs(bin_pos[b] * _DEN - bin_conf[b]) for b in range(n_bins)]           # |share - confidence| * ms * _DEN
    ece = _ratio(sum(gaps), W * _DEN)
    mce = float(max(Fraction(gaps[b], bin_ms[b] * _DEN) for b in range(n_bins) if bin_ms[b])) if W else float("nan")
    below = auc_num = 0
    for u in occupied:                                                              # ascending: `below` = negatives in lower buckets
        auc_num += pos[u] * (2 * below + neg[u])
        below += neg[u]
    tp = fp = 0
    terms = []                                                  # the recall gained at a bucket times the precision down to it, times P
    for u in reversed(occupied):
        tp += pos[u]
        fp += neg[u]
        if pos[u]:
            terms.append(Fraction(pos[u] * tp, tp + fp))
    ap_num, ap_den = _exact_sum(terms)
    reliability = [(b / n_bins, (b + 1) / n_bins, bin_ms[b], _ratio(bin_conf[b], bin_ms[b] * _DEN), _ratio(bin_pos[b], bin_ms[b]))
                   for b in range(n_bins)]
    return {"pos_ms": P, "neg_ms": N, "invalid_ms": int(h[0].sum()), "nan_ms": int(h[1:, NAN_SLOT].sum()),
            "brier": _ratio(brier_num, W * _DEN * _DEN), "nll": total / W if W else float("nan"), "ece": ece, "mce": mce,
            "roc_auc": _ratio(auc_num, 2 * P * N), "average_precision": ap_num / (ap_den * P) if P else float("nan"),
            "reliability": reliability}


# ---- fits: a float64 (65537,) table, every value finite and in [0, 1] -------------------------------------------------------------
def check_table(table):
    """A calibration table as contiguous float64 (65537,); ValueError unless every value is finite and lies in [0, 1]."""
    table = np.ascontiguousarray(table, dtype=np.float64)
    if table.shape != (BUCKETS,) or not np.isfinite(table).all() or table.min() < 0.0 or table.max() > 1.0:
        raise ValueError(f"a calibration table is float64 ({BUCKETS},) with finite values in [0, 1]")
    return table


def _platt_nll(a, b, x, pos, neg):
    z = a * x + b
    return float(np.sum(pos * np.logaddexp(0.0, -z) + neg * np.logaddexp(0.0, z)))


def _sigmoid(z):
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def fit_platt(hist_row, temperature_only=False):
    """Platt scaling: q_u = sigmoid(a * logit(p_u) + b), (a, b) minimising the mass-weighted NLL of the row over the 65537 points.
    Newton's method from (1, 0), the step halved until the NLL does not grow, at most PLATT_MAX_ITERATIONS steps; it stops when a
    step no longer lowers the NLL.  temperature_only: b stays 0 (temperature scaling, T = 1 / a).  A row without positives or
    without negatives has no finite optimum: the iteration cap ends it.  Returns (table, {"a", "b", "iterations"})."""
    pos, neg = (np.asarray(v, dtype=np.float64) for v in _pos_neg(hist_row))
    p = bucket_confidence()
    x = np.log(p) - np.log1p(-p)
    a, b = 1.0, 0.0
    iterations = 0
    if pos.sum() + neg.sum() > 0:
        scale = 1.0 / (pos.sum() + neg.sum())
        pos, neg = pos * scale, neg * scale
        w = pos + neg
        loss = _platt_nll(a, b, x, pos, neg)
        for iterations in range(1, PLATT_MAX_ITERATIONS + 1):
            s = _sigmoid(a * x + b)
            r = w * s - pos                                     # d loss / d z
            hess = w * s * (1.0 - s)
            ga, gb = float(np.sum(r * x)), float(np.sum(r))
            haa, hab, hbb = float(np.sum(hess * x * x)), float(np.sum(hess * x)), float(np.sum(hess))
            if temperature_only:
                da, db = (-ga / haa if haa > 0 else -ga), 0.0
            else:
                ridge = 1e-12 * (haa + hbb)
                det = (haa + ridge) * (hbb + ridge) - hab * hab
                if det > 0:
                    da, db = -((hbb + ridge) * ga - hab * gb) / det, -((haa + ridge) * gb - hab * ga) / det
                else:
                    da, db = -ga, -gb
            step, better = 1.0, None
            for _ in range(60):
                trial = _platt_nll(a + step * da, b + step * db, x, pos, neg)
                if math.isfinite(trial) and trial < loss:
                    better = trial
                    break
                step *= 0.5
            if better is None:
                iterations -= 1
                break
            a, b, loss = a + step * da, b + step * db, better
    table = np.clip(_sigmoid(a * x + b), 0.0, 1.0)
    return check_table(table), {"a": float(a), "b": float(b), "iterations": int(iterations)}


def fit_isotonic(hist_row):
    """Isotonic regression of the laugh share on the bucket: pool-adjacent-violators over the buckets that hold mass, on integer
    (pos, pos + neg) pairs; two means are compared by cross-multiplication, so the pooling is exact, and a block's value is one
    division.  A bucket without mass takes the value of the block of the nearest bucket with mass below it, the leading ones that
    of the first block.  A row without any mass gives the identity, p_u.  Returns the table."""
    pos, neg = _pos_neg(hist_row)
    blocks = []                                                 # [pos, mass, first bucket]
    for u in range(BUCKETS):
        if not (pos[u] or neg[u]):
            continue
        blocks.append([pos[u], pos[u] + neg[u], u])
        while len(blocks) > 1 and blocks[-2][0] * blocks[-1][1] >= blocks[-1][0] * blocks[-2][1]:      # mean before >= mean behind
            last = blocks.pop()
            blocks[-1][0] += last[0]
            blocks[-1][1] += last[1]
    if not blocks:
        return bucket_confidence()
    table = np.empty(BUCKETS, np.float64)
    starts = [0] + [blk[2] for blk in blocks[1:]] + [BUCKETS]
    for j, blk in enumerate(blocks):
        table[starts[j]:starts[j + 1]] = blk[0] / blk[1]
    return check_table(table)


def fit(hist_row, method):
    """(table, parameters) of one of METHODS: "platt", "temperature" (Platt with b = 0) or "isotonic" (no parameters)."""
    if method == "isotonic":
        return fit_isotonic(hist_row), {}
    if method not in METHODS:
        raise ValueError(f"method is one of {METHODS}, got {method!r}")
    return fit_platt(hist_row, temperature_only=method == "temperature")


# ---- applying a table -------------------------------------------------------------------------------------------------------------
def apply_calibration(track, table):
    """table[bucket of the frame] for every frame of a host track, float64 of the track's shape; a NaN frame stays NaN."""
    table = check_table(table)
    track = np.asarray(track)
    u = slots_of(track)
    out = np.where(u == NAN_SLOT, np.nan, table[np.minimum(u, BUCKETS - 1)])
    return out.reshape(track.shape)


def apply_calibration_device(probs, table, out=None):
    """apply_calibration for a (T,) or (C, T) float32 / float64 track in GPU memory (lad_track_remap): a float64 tensor of the
    track's shape that stays on the device, bit for bit the host form.  table: the host table, or a float64 GPU tensor that holds it
    already.  out: a contiguous float64 GPU tensor of that shape to write into.  No CPU fallback."""
    import torch

    import _hip
    p2, dtype, single = _hip.device_track(probs, "calibration")
    if isinstance(table, torch.Tensor):
        _hip.require_cuda(table, "table", torch.float64)
        if table.shape != (BUCKETS,):
            raise ValueError(f"a calibration table has {BUCKETS} entries")
    else:
        table = torch.from_numpy(check_table(table)).to(p2.device)
    out2 = _hip.out_track(out, p2, single, torch.float64)
    C, T = p2.shape
    if C and T:
        with torch.cuda.device(p2.device):
            _hip.launch("lad_track_remap", p2, dtype, C, T, table, out2)
    return out2[0] if single else out2


def remap_histogram(hist_row, table):
    """The histogram row of the calibrated track from the row of the track itself: the mass of bucket u moves to the bucket of
    table[u], the NaN slot stays.  Exact: a calibrated frame's value depends on its bucket alone."""
    h = _row(hist_row)
    to = slots_of(check_table(table))
    out = np.zeros_like(h)
    for k in range(N_CLASSES):
        np.add.at(out[k], to, h[k, :BUCKETS])
    out[:, NAN_SLOT] = h[:, NAN_SLOT]
    return out


# ---- files ------------------------------------------------------------------------------------------------------------------------
def _plain(figures):
    return {k: ([list(r) for r in v] if k == "reliability" else v) for k, v in figures.items()}


def save_table(path, table, method, parameters, before, after):
    """calibration_table.npz: `table` float64 (65537,), `method`, and as JSON text `parameters`, `figures_before` and `figures_after`
    (calibration_figures of the fitted row and of remap_histogram's).  An uncompressed archive with a fixed time stamp: the same
    content gives the same bytes."""
    arrays = {"table": check_table(table), "method": np.array(str(method)), "parameters": np.array(json.dumps(parameters, sort_keys=True)),
              "figures_before": np.array(json.dumps(_plain(before), sort_keys=True)),
              "figures_after": np.array(json.dumps(_plain(after), sort_keys=True))}
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())


def load_table(path):
    """The table of a file save_table wrote (or any .npz with a `table`), checked; a bare .npy holds the table alone."""
    data = np.load(path, allow_pickle=False)
    return check_table(data["table"] if hasattr(data, "files") else data)


def figure_row(name, figures):
    """One row of calibration.csv (CALIBRATION_COLUMNS)."""
    return [name] + [figures[k] for k in CALIBRATION_COLUMNS[1:]]


def reliability_rows(figures):
    """The rows of reliability.csv (RELIABILITY_COLUMNS)."""
    return [[b, *r] for b, r in enumerate(figures["reliability"])]
