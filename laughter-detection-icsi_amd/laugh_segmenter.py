"""Drop-in for the live part of the reference's laugh_segmenter.py: probability track -> laughter instances.

Reference: laugh_segmenter.py:57-71 (fix_over_underflow), :19-24 (collapse / frame_span_to_time_span), :35-42
(cut_laughter_segments), :74-111 (get_laughter_instances), :141-149 (format_outputs).  Same function names, arguments and result
({(threshold, min_length): [(start_s, end_s), ...]}); the per-frame Python loop (87 passes over 360,000 frames in the evaluation
sweeps, cluster_scripts/gen_eval_exp.py:30-36) is replaced by one vectorised run-length pass per threshold.  Integer run boundaries
are bit-exact with the reference (tests/test_host_logic.py against vectors produced by the reference itself).  The Gillick-era MFCC
code below laugh_segmenter.py:115 is dead in the reference and is not reproduced.

Three decoders turn the track into integer (first_frame, last_frame) spans, each described once by a `Decoder` record:
    THRESHOLD    the reference's rule: frame i is laughter iff p[i] > threshold (csrc/runs.hip)
    HYSTERESIS   an event starts above an onset threshold and lasts until the track falls to or below a lower offset threshold;
                 events separated by a short pause become one, before the minimum-length filter (csrc/binarize.hip; the convention
                 is written out above lad_binarize_count in include/lad_hip.h).  Not in the reference.
    VITERBI      two-state Viterbi decoding: a frame contributes its log-odds relative to the threshold (an int32 look-up:
                 `viterbi_emission_table`), every event costs a penalty, and the best-scoring set of events is returned
                 (csrc/viterbi.hip; lad_viterbi_count in include/lad_hip.h).  Not in the reference.
A record names its extra axes, validates its settings, holds its host form and the ctypes calls of its device form, and says how
segment_laughter.py names its directories.  Everything else is written once over a record: `_instances` (the dictionaries),
`_device_frame_spans` (rounds of at most the library's settings per call) and `_device_tables` (count, one read-back of the counts,
fill; sweep_eval's scorers read the tables where they lie).  `decoder_for` picks the record from the optional axes.  The public
functions -- get_laughter_* (THRESHOLD), binarize_* (HYSTERESIS), viterbi_* (VITERBI), each as `*_frame_spans` and `*_instances`,
on the host and as `*_device` for a track in GPU memory -- are wrappers.  A device form returns what its host form returns, bit for
bit; only the compact tables cross to the host; there is no CPU fallback.  torch and _hip are imported by the device forms only.

Every `*_instances` form takes stats=True and then also says how sure each instance is: mean probability, time of the peak and probability
at the peak (`span_stats`, `confidences`; csrc/spanstats.hip for a track in GPU memory; the convention is written out above
lad_span_stats in include/lad_hip.h).  It reads spans only, so it is written once, in `_instances` / `_device_frame_spans`.
"""
import math
import ctypes
from typing import Callable, NamedTuple

import numpy as np


def frame_span_to_time_span(frame_span, fps=100.):
    return (frame_span[0] / fps, frame_span[1] / fps)


def collapse_to_start_and_end_frame(instance_list):
    return (instance_list[0], instance_list[-1])


def seconds_to_samples(s, sr):
    return s * sr


def cut_laughter_segments(instance_list, y, sr):
    new_audio = []
    for start, end in instance_list:
        clip = y[int(seconds_to_samples(start, sr)):int(seconds_to_samples(end, sr))]
        new_audio = np.concatenate([new_audio, clip])
    return new_audio


def lowpass(sig, filter_order=2, cutoff=0.01):
    """Second-order Butterworth low-pass at `cutoff` of Nyquist, forwards and backwards (laugh_segmenter.py:49-55).  The reference
    overwrites `filter_order` with 2 inside the function, so any `filter_order` gives the second-order filter; so does this."""
    from scipy import signal
    filter_order = 2
    b, a = signal.butter(filter_order, cutoff, output='ba')
    return signal.filtfilt(b, a, sig)


def lowpass_device(probs, cutoff=0.01, lengths=None):
    """`lowpass` for a (T,) or (C, T) track in GPU memory (csrc/lowpass.hip through lowpass.py): a float64 tensor of the same shape
    that stays on the device, e.g. for get_laughter_instances_device.  No CPU fallback."""
    import lowpass as lowpass_mod
    return lowpass_mod.lowpass_device(probs, cutoff=cutoff, lengths=lengths)


def rank_filter(sig, window, rank):
    """Element `rank` of the sorted window of `window` frames (odd, 1..1023) around every frame of a 1-D track, its ends replicated
    (scipy.ndimage.rank_filter with mode='nearest'; the convention is written out above lad_rank_filter in include/lad_hip.h).
    Not in the reference.  float32 / float64 in, the same dtype out (anything else is taken as float64): the result is one of the
    track's own values.  Host parity form of csrc/rankfilt.hip: every window is sorted, O(T window log window)."""
    import rankfilt
    window, rank = rankfilt.check_window(window, rank)
    sig = np.asarray(sig)
    if sig.dtype not in (np.float32, np.float64):
        sig = sig.astype(np.float64)
    if sig.ndim != 1 or sig.size < 1:
        raise ValueError(f"the track is 1-D with at least one frame, got shape {sig.shape}")
    if sig.size > 2 ** 30:
        raise ValueError(f"the track has {sig.size} frames, more than 2^30")
    h = (window - 1) // 2
    windows = np.lib.stride_tricks.sliding_window_view(np.pad(sig, h, mode="edge"), window)
    out = np.empty_like(sig)
    step = max(1, (1 << 22) // window)      # (the sorted copies of 4 M elements at a time, not of T * window)
    for i0 in range(0, sig.size, step):
        out[i0:i0 + step] = np.partition(windows[i0:i0 + step], rank, axis=1)[:, rank]
    return out


def median_filter(sig, window):
    """The median of `window` frames (odd, 1..1023) around every frame, the track's ends replicated: rank_filter at rank
    (window - 1) / 2, scipy.ndimage.median_filter(sig, window, mode='nearest').  It removes every flicker shorter than window / 2
    frames, keeps every edge where it was and returns only values the track already holds."""
    import rankfilt
    return rank_filter(sig, *rankfilt.check_window(window))


def rank_filter_device(probs, window, rank, lengths=None, out=None):
    """`rank_filter` for a (T,) or (C, T) track in GPU memory (csrc/rankfilt.hip through rankfilt.py): a tensor of the same shape and
    dtype that stays on the device, bit for bit what the host form returns.  No CPU fallback."""
    import rankfilt
    return rankfilt.rank_filter_device(probs, window, rank, lengths=lengths, out=out)


def median_filter_device(probs, window, lengths=None, out=None):
    """`median_filter` for a (T,) or (C, T) track in GPU memory, e.g. for get_laughter_instances_device.  No CPU fallback."""
    import rankfilt
    return rankfilt.median_filter_device(probs, window, lengths=lengths, out=out)


def apply_calibration(track, table):
    """A fitted calibration table (float64 (65537,), one value per bucket of the Viterbi decoder: calibration.fit_platt /
    fit_isotonic) applied to a host track: table[floor(v * 65536)] of the fixed probability v, NaN kept, float64.  Not in the
    reference.  It stands in front of the smoothers and every decoder."""
    import calibration
    return calibration.apply_calibration(track, table)


def apply_calibration_device(probs, table, out=None):
    """`apply_calibration` for a (T,) or (C, T) track in GPU memory (csrc/calibration.hip through calibration.py): a float64 tensor
    of the same shape that stays on the device, bit for bit what the host form returns.  No CPU fallback."""
    import calibration
    return calibration.apply_calibration_device(probs, table, out=out)


def fix_over_underflow(prob):
    """p > 1 -> 1; p <= 0 -> 1e-7 (so that threshold 0 still accepts the frame); else p."""
    if prob > 1:
        return 1
    if prob <= 0:
        return 0.0000001
    return prob


def fix_probs(probs):
    """Vector form of fix_over_underflow in float64 (the reference maps Python floats)."""
    p = np.asarray(probs, dtype=np.float64).copy()
    p[p > 1] = 1.0
    p[p <= 0] = 0.0000001
    return p


def run_spans(mask):
    """Maximal runs of True in a boolean vector -> int64 array (n_runs, 2) of (first_frame, last_frame)."""
    m = np.asarray(mask, dtype=bool)
    if m.size == 0:
        return np.zeros((0, 2), np.int64)
    d = np.diff(m.astype(np.int8))
    starts = np.flatnonzero(d == 1) + 1
    ends = np.flatnonzero(d == -1)
    if m[0]:
        starts = np.concatenate([[0], starts])
    if m[-1]:
        ends = np.concatenate([ends, [m.size - 1]])
    return np.stack([starts, ends], axis=1).astype(np.int64)


def format_outputs(instances, wav_paths=None):
    """[{'start', 'end'}] (+ 'filename' when the instances were cut into wav files): laugh_segmenter.py:141-149, what
    segment_laughter.py:148 prints after writing `laugh_<i>.wav`."""
    outs = []
    for i, inst in enumerate(instances):
        d = {'start': inst[0], 'end': inst[1]}
        if wav_paths is not None:
            d = {'filename': wav_paths[i], **d}   # IndexError on a short list, as the reference
        outs.append(d)
    return outs


# ---- confidence of an instance (include/lad_hip.h: lad_span_stats has the convention) --------------------------------------------
def span_stats(probs, spans):
    """(sums int64 (n,), peaks int64 (n,), peak_values float64 (n,)) of the int64 (n, 2) spans (first_frame, last_frame) of a 1-D
    track: w = the decoders' frame value (fix_probs), 0.0 for a NaN frame; sum = the int64 sum of rint(w * 2^32) over the span;
    peak = the earliest frame of the span at which w is largest, peak_value = w there.  A span with first < 0, last >= frames or
    first > last reads nothing: (0, -1, 0.0).  Not in the reference.  Host parity form of csrc/spanstats.hip: a cumulative sum, and
    one argmax per span of more than one frame."""
    w = fix_probs(probs)
    if w.ndim != 1:
        raise ValueError(f"the track is 1-D, got shape {w.shape}")
    w[np.isnan(w)] = 0.0
    spans = np.asarray(spans, dtype=np.int64).reshape(-1, 2)
    first, last = spans[:, 0], spans[:, 1]
    ok = (first >= 0) & (last < len(w)) & (first <= last)
    cum = np.concatenate([[0], np.cumsum(np.rint(w * 4294967296.0).astype(np.int64))])
    sums, peaks, values = np.zeros(len(spans), np.int64), np.full(len(spans), -1, np.int64), np.zeros(len(spans), np.float64)
    sums[ok] = cum[last[ok] + 1] - cum[first[ok]]
    peaks[ok] = first[ok]                                   # (a span of one frame)
    for i in np.flatnonzero(ok & (last > first)):
        peaks[i] = first[i] + np.argmax(w[first[i]:last[i] + 1])        # (the first of equal maxima)
    values[ok] = w[peaks[ok]]
    return sums, peaks, values


def span_stats_device(probs, table, counts):
    """`span_stats` for a (T,) or (C, T) float32 / float64 track in GPU memory and span tables that lie there too (csrc/spanstats.hip
    through spanstats.py): table int32 (total, 2), the tables back to back in c * K + k order, counts their row counts, as
    _device_tables returns them.  The same three arrays, one entry per row, bit for bit.  No CPU fallback."""
    import spanstats
    return spanstats.span_stats_device(probs, table, counts)


def confidences(sums, peaks, peak_values, spans, fps):
    """float64 (n, 3): (mean, peak_time, peak_value) per span from the integers of span_stats: n = last - first + 1, mean =
    float64(sum) / float64(n * 2^32), one IEEE division; peak_time = peak / fps, as a span's start is computed.  A row that
    span_stats refused (peak -1) has mean 0.0."""
    spans = np.asarray(spans, dtype=np.int64).reshape(-1, 2)
    n = np.where(np.asarray(peaks) >= 0, spans[:, 1] - spans[:, 0] + 1, 1)
    out = np.empty((len(spans), 3), np.float64)
    out[:, 0] = np.asarray(sums, dtype=np.int64).astype(np.float64) / (n << 32).astype(np.float64)
    out[:, 1] = np.asarray(peaks, dtype=np.int64) / fps
    out[:, 2] = peak_values
    return out


# ---- what the decoders share -----------------------------------------------------------------------------------------------------
class Decoder(NamedTuple):
    """One way from a probability track to spans.  `ctx` is the dictionary of what a call prepares once: "fps_host" (float64 numpy
    (C,)), "table" (the emission table) and, through on_device, their copies in GPU memory."""
    axes: tuple                 # names of the extra axes in key order: a key is (threshold, *axes, min_length)
    what: str                   # the word in device_track's message
    lib: str                    # the family's prefix in include/lad_hip.h
    keys: Callable              # (thresholds, axis_values, ctx) -> ([(threshold, *axis values)], [setting]), thresholds-major; validates
    host_spans: Callable        # (probs, settings, fps, ctx) -> [int64 (n, 2) per setting]
    round_size: Callable        # (lib, n_settings) -> settings per device call
    count: Callable             # (track, chunk, ws, ctx): lad_*_count of the settings `chunk`
    fill: Callable              # (track, chunk, ws, counts, total, ctx) -> (the table the scorers read, its counts)
    dir_suffix: Callable        # key -> the directories segment_laughter.py adds below t_<thr>/l_<min_len>
    found_line: Callable        # (n, key) -> what segment_laughter.py prints per setting


def _check_fps(fps):
    fps = float(fps)
    if not (math.isfinite(fps) and fps > 0):
        raise ValueError(f"fps must be positive and finite, got {fps}")
    return fps


def fps_per_channel(fps, C, each=_check_fps):
    """One fps or C of them -> float64 numpy (C,).  each=float leaves a value that is not positive and finite to whoever divides by
    it (the library refuses it: LadHipError)."""
    f = [fps] * C if np.ndim(fps) == 0 else list(fps)
    if len(f) != C:
        raise ValueError(f"fps: one value or one per channel ({C}), got {len(f)}")
    return np.asarray([each(x) for x in f], dtype=np.float64)


def device_track(probs, what="sweep"):
    """_hip.device_track: what every device form asks of its probability tensor."""
    import _hip
    return _hip.device_track(probs, what)


def on_device(ctx, name, device):
    """ctx[name], a numpy array, in GPU memory: uploaded at its first use in a call, not once per round."""
    import torch
    if name + "_dev" not in ctx:
        ctx[name + "_dev"] = torch.from_numpy(ctx[name]).to(device)
    return ctx[name + "_dev"]


def _doubles(values):
    return (ctypes.c_double * len(values))(*[float(v) for v in values])


def _read_counts(ws, n):
    """The n int32 row counts at the start of a family's workspace (synchronises)."""
    import torch
    return np.ascontiguousarray(ws[:4 * n].view(torch.int32).cpu().numpy())


def _table(total, device, n=None):
    import torch
    return torch.empty((max(total, 1), 2) if n is None else (n, max(total, 1), 2), dtype=torch.int32, device=device)


def _instances_from_spans(keys, spans_list, min_lengths, fps, stats_list=None):
    """{(*key, min_length): [(start_s, end_s), ...]}, keys-major: first / fps, last / fps and end - start > min_length in float64
    (the arithmetic of the reference's Python floats) on the integer spans of each key.  stats_list (the span_stats triple of
    each key's spans): -> (that dictionary, {same key: float64 (n, 3) `confidences` of exactly its instances, in their order})."""
    instance_dict, stats_dict = {}, {}
    for i, (key, spans) in enumerate(zip(keys, spans_list)):
        starts, ends = spans[:, 0] / fps, spans[:, 1] / fps
        length = ends - starts
        conf = confidences(*stats_list[i], spans, fps) if stats_list is not None else None
        for min_l in min_lengths:
            keep = length > min_l
            instance_dict[(*key, min_l)] = list(zip(starts[keep].tolist(), ends[keep].tolist()))
            if conf is not None:
                stats_dict[(*key, min_l)] = conf[keep]
    return instance_dict if stats_list is None else (instance_dict, stats_dict)


# ---- THRESHOLD: the reference's frame-by-frame rule (include/lad_hip.h: lad_runs_count) ------------------------------------------
def _runs_spans_host(probs, settings, fps, ctx):
    p = fix_probs(probs)
    return [run_spans(p > thr) for thr in settings]


def _runs_count(track, chunk, ws, ctx):
    import _hip
    _hip.launch("lad_runs_count", *track, _doubles(chunk), len(chunk), ws)


def _runs_fill(track, chunk, ws, counts, total, ctx):
    import _hip
    table = _table(total, ws.device)
    _hip.launch("lad_runs_fill", *track, _doubles(chunk), len(chunk), ws, counts, table, total)
    return table[:total], counts


THRESHOLD = Decoder(
    axes=(), what="sweep", lib="lad_runs",
    keys=lambda thresholds, axis_values, ctx: ([(thr,) for thr in thresholds], thresholds),
    host_spans=_runs_spans_host,
    round_size=lambda lib, n: n,        # one round whatever n is: the library refuses more than lad_runs_max_thresholds()
    count=_runs_count, fill=_runs_fill,
    dir_suffix=lambda key: (),
    found_line=lambda n, key: f"Found {n} laughs for threshold {key[0]} and min_length {key[1]}.")


# ---- HYSTERESIS: hysteresis and gap filling (include/lad_hip.h: lad_binarize_count has the convention) ---------------------------
def _check_setting(onset, offset, min_gap):
    onset, offset, min_gap = float(onset), float(offset), float(min_gap)
    if not (math.isfinite(onset) and math.isfinite(offset) and math.isfinite(min_gap)):
        raise ValueError(f"onset, offset and min_gap must be finite, got ({onset}, {offset}, {min_gap})")
    if offset > onset:
        raise ValueError(f"offset {offset} lies above onset {onset}")
    if min_gap < 0:
        raise ValueError(f"min_gap must be >= 0, got {min_gap}")
    return onset, offset, min_gap


def _hysteresis_spans(p, onset, offset):
    """p: fixed probabilities.  Every maximal run of p > offset that holds a frame with p > onset -> (its first such frame, the
    end of the run): int64 (n, 2)."""
    held = run_spans(p > offset)
    if len(held) == 0:
        return held
    onsets = np.flatnonzero(p > onset)
    at = np.searchsorted(onsets, held[:, 0], side="left")             # the first onset frame at or behind the run's start
    first = onsets[np.minimum(at, len(onsets) - 1)] if len(onsets) else np.zeros(len(held), np.int64)
    has = (at < len(onsets)) & (first <= held[:, 1])
    return np.stack([first[has], held[has, 1]], axis=1).astype(np.int64)


def _fill_gaps(spans, min_gap, fps):
    """Consecutive runs are joined iff not (next.first / fps - prev.last / fps > min_gap), pairwise on the original neighbours."""
    if len(spans) < 2:
        return spans
    head = np.concatenate([[True], spans[1:, 0] / fps - spans[:-1, 1] / fps > min_gap])
    tail = np.concatenate([head[1:], [True]])
    return np.stack([spans[head, 0], spans[tail, 1]], axis=1)


def _binarize_keys(thresholds, axis_values, ctx):
    offset_drops, min_gaps = axis_values
    for drop in offset_drops:
        if not (math.isfinite(float(drop)) and float(drop) >= 0):
            raise ValueError(f"an offset drop must be finite and >= 0, got {drop}")
    triples = [(thr, drop, gap) for thr in thresholds for drop in offset_drops for gap in min_gaps]
    settings = [_check_setting(thr, thr - drop, gap) for thr, drop, gap in triples]        # offset = thr - drop, once, Python float
    return triples, settings


def _binarize_spans_host(probs, settings, fps, ctx):
    p = fix_probs(probs)
    held = {}
    spans_list = []
    for onset, offset, gap in settings:
        if (onset, offset) not in held:
            held[(onset, offset)] = _hysteresis_spans(p, onset, offset)
        spans_list.append(_fill_gaps(held[(onset, offset)], gap, fps))
    return spans_list


def _binarize_count(track, chunk, ws, ctx):
    import _hip
    onset, offset, _ = zip(*chunk)
    _hip.launch("lad_binarize_count", *track, _doubles(onset), _doubles(offset), len(chunk), ws)


def _binarize_fill(track, chunk, ws, counts, total, ctx):
    import _hip
    tables = _table(total, ws.device, 2)    # the hysteresis runs go to tables[0], the merged ones to tables[1] and their counts over the raw ones
    _hip.launch("lad_binarize_fill", *track, *[_doubles(col) for col in zip(*chunk)], len(chunk), on_device(ctx, "fps_host", ws.device),
                ctx["fps_host"], ws, counts, tables[0], tables[1], total)
    counts = _read_counts(ws, len(counts))
    return tables[1][:int(counts.sum(dtype=np.int64))], counts


HYSTERESIS = Decoder(
    axes=("offset_drop", "min_gap"), what="sweep", lib="lad_binarize",
    keys=_binarize_keys, host_spans=_binarize_spans_host,
    round_size=lambda lib, n: int(lib.lad_binarize_max_settings()),
    count=_binarize_count, fill=_binarize_fill,
    dir_suffix=lambda key: (f"d_{key[1]}_g_{key[2]}",),
    found_line=lambda n, key: f"Found {n} laughs for threshold {key[0]}, offset drop {key[1]}, min_gap {key[2]} and min_length {key[3]}.")


# ---- VITERBI: two-state Viterbi decoding (include/lad_hip.h: lad_viterbi_count has the convention) -------------------------------
VITERBI_BUCKETS = 65536        # a frame's bucket is floor(v * 65536): 0..65536, lad_viterbi_table_entries() = 65537 table values
VITERBI_NAN_SCORE = -2 ** 31
_VITERBI_MAX_EMISSION, _VITERBI_MAX_PENALTY = 2 ** 24, 2 ** 26


def viterbi_emission_table(unit=1024):
    """The default emission table: int32 (65537,), S[u] = rint(unit * logit((u + 0.5) / 65537)) -- `unit` steps per nat, the log-odds
    of the middle of bucket u, so both end points are finite (about +-11.8 nats)."""
    p = (np.arange(VITERBI_BUCKETS + 1, dtype=np.float64) + 0.5) / (VITERBI_BUCKETS + 1)
    return np.rint(unit * (np.log(p) - np.log1p(-p))).astype(np.int32)


def _viterbi_table(table):
    table = viterbi_emission_table() if table is None else np.ascontiguousarray(table, dtype=np.int32)
    if table.shape != (VITERBI_BUCKETS + 1,) or np.abs(table.astype(np.int64)).max() > _VITERBI_MAX_EMISSION:
        raise ValueError(f"the emission table is int32 ({VITERBI_BUCKETS + 1},) with |S[u]| <= 2^24")
    return table


def viterbi_settings(thresholds, penalties, table, unit=1024):
    """[(bias, penalty)] as the decoder takes them, thresholds-major: bias = table[floor(threshold * 65536)] (a frame at the
    threshold scores 0), penalty = rint(penalty in nats * unit).  ValueError for a threshold outside (0, 1] or a penalty that is
    negative or not finite."""
    out = []
    for thr in thresholds:
        if not 0.0 < float(thr) <= 1.0:
            raise ValueError(f"a threshold of the decoder lies in (0, 1], got {thr}")
        for pen in penalties:
            if not (math.isfinite(float(pen)) and float(pen) >= 0):
                raise ValueError(f"a penalty must be finite and >= 0, got {pen}")
            penalty = int(np.rint(float(pen) * unit))
            if penalty > _VITERBI_MAX_PENALTY:
                raise ValueError(f"penalty {pen} is {penalty} table units, beyond 2^26")
            out.append((int(table[int(math.floor(float(thr) * VITERBI_BUCKETS))]), penalty))
    return out


def _check_viterbi_settings(settings):
    settings = [(int(b), int(p)) for b, p in settings]
    for bias, penalty in settings:
        if abs(bias) > _VITERBI_MAX_EMISSION or not 0 <= penalty <= _VITERBI_MAX_PENALTY:
            raise ValueError(f"a setting is (bias, penalty) with |bias| <= 2^24 and 0 <= penalty <= 2^26, got ({bias}, {penalty})")
    return settings


def _viterbi_keys(thresholds, axis_values, ctx):
    """Also settles ctx["table"]: the table given, checked, or the default one."""
    table = ctx["table"] = _viterbi_table(ctx.get("table"))
    penalties, = axis_values
    return [(thr, pen) for thr in thresholds for pen in penalties], viterbi_settings(thresholds, penalties, table)


def _viterbi_spans_host(probs, settings, table):
    """[int64 (n, 2) array per setting (bias, penalty)]: the header's recursion as a loop over frames, vectorised over the settings."""
    p = fix_probs(probs)
    T, K = len(p), len(settings)
    if T == 0 or K == 0:
        return [np.zeros((0, 2), np.int64) for _ in settings]
    nan = np.isnan(p)
    u = np.floor(np.where(nan, 0.0, p) * float(VITERBI_BUCKETS)).astype(np.int64)
    emitted = table.astype(np.int64)[u]
    bias = np.asarray([s[0] for s in settings], np.int64)
    pen = np.asarray([s[1] for s in settings], np.int64)
    d0, d1 = np.zeros(K, np.int64), -pen
    psi0, psi1 = np.zeros((T, K), bool), np.zeros((T, K), bool)
    nan_score = np.full(K, VITERBI_NAN_SCORE, np.int64)
    for t in range(T):
        s = nan_score if nan[t] else emitted[t] - bias
        enter = d0 - pen
        psi0[t] = d1 > d0
        psi1[t] = ~(enter > d1)
        d0, d1 = np.maximum(d0, d1), np.maximum(enter, d1) + s
    state = d1 > d0
    on = np.zeros((T, K), bool)
    for t in range(T - 1, -1, -1):
        on[t] = state
        state = np.where(state, psi1[t], psi0[t])
    return [run_spans(on[:, k]) for k in range(K)]


def _viterbi_count(track, chunk, ws, ctx):
    import _hip
    bias, penalty = ((ctypes.c_int32 * len(chunk))(*col) for col in zip(*chunk))
    _hip.launch("lad_viterbi_count", *track, on_device(ctx, "table", ws.device), ctx["table"], bias, penalty, len(chunk), ws, ctx.get("best"))


def _viterbi_fill(track, chunk, ws, counts, total, ctx):
    import _hip
    runs = _table(total, ws.device)
    _hip.launch("lad_viterbi_fill", ws, counts, *track[2:], len(chunk), runs, total)
    return runs[:total], counts


VITERBI = Decoder(
    axes=("penalty",), what="decoder", lib="lad_viterbi",
    keys=_viterbi_keys, host_spans=lambda probs, settings, fps, ctx: _viterbi_spans_host(probs, settings, ctx["table"]),
    round_size=lambda lib, n: int(lib.lad_viterbi_max_settings()),
    count=_viterbi_count, fill=_viterbi_fill,
    dir_suffix=lambda key: (f"p_{key[1]}",),
    found_line=lambda n, key: f"Found {n} laughs for threshold {key[0]}, penalty {key[1]} and min_length {key[2]}.")


# ---- written once over a record --------------------------------------------------------------------------------------------------
def decoder_for(offset_drops=None, min_gaps=None, penalties=None):
    """(decoder, the values of its axes as lists) from the optional axes of the public functions and the command lines: penalties ->
    VITERBI; offset_drops or min_gaps -> HYSTERESIS (one given: the other is [0.0], which changes nothing); none -> THRESHOLD.  The
    Viterbi decoder has neither an offset nor a gap rule: both kinds together are refused."""
    if penalties is not None:
        if offset_drops is not None or min_gaps is not None:
            raise ValueError("penalties (the Viterbi decoder) cannot be combined with offset_drops or min_gaps")
        return VITERBI, (list(penalties),)
    if offset_drops is None and min_gaps is None:
        return THRESHOLD, ()
    return HYSTERESIS, (list(offset_drops) if offset_drops is not None else [0.0], list(min_gaps) if min_gaps is not None else [0.0])


def _device_tables(decoder, probs, dtype, chunk, ctx, want_best=False):
    """Count + fill of one round (include/lad_hip.h) on a (C, T) tensor that device_track has passed, T >= 1, for the settings
    `chunk`, at most decoder.round_size of them.  Everything stays on the device: returns (workspace, table, counts, best) with
    `workspace` the family's workspace, a uint8 tensor (the tables' counts at its start, where the scorers read them), `table` the
    (total, 2) int32 tables back to back in c * K + k order, counts their row counts, int32 numpy (C * K,), and best the int64
    (C * K,) path scores of the Viterbi decoder on the device (None unless asked for).  The counts cross to the host once, after
    the count (HYSTERESIS: and after its fill)."""
    import torch

    import _hip
    C, T = probs.shape
    K = len(chunk)
    ws = _hip.workspace(decoder.lib + "_workspace_bytes", C, T, K, device=probs.device)
    with torch.cuda.device(probs.device):
        ctx["best"] = best = torch.empty(C * K, dtype=torch.int64, device=probs.device) if want_best else None
        track = (probs, dtype, C, T)
        decoder.count(track, chunk, ws, ctx)
        counts = _read_counts(ws, C * K)
        table, counts = decoder.fill(track, chunk, ws, counts, int(counts.sum(dtype=np.int64)), ctx)
        return ws, table, counts, best


def _device_run_tables(probs, thresholds):
    """(counts (C, K) int64, table (total, 2) int32 numpy) of one THRESHOLD round on a (C, T) tensor: kept for tests/test_runs_gpu.py."""
    probs, dtype, _ = device_track(probs)
    _, table, counts, _ = _device_tables(THRESHOLD, probs, dtype, list(thresholds), {})
    return counts.astype(np.int64).reshape(len(probs), -1), table.cpu().numpy()


def _device_frame_spans(decoder, probs, settings, ctx):
    """[int64 (n, 2) array per setting] for a (T,) tensor, one such list per channel for a (C, T) one: the tables of
    _device_tables on the host, in rounds of at most decoder.round_size settings.  ctx["fps"], if there: one value or one per
    channel.  ctx["want_stats"]: ctx["stats"] becomes the span_stats triple of every one of those arrays, in the same nesting:
    lad_span_stats_prepare once per call, lad_span_stats on every round's table while it lies on the device (csrc/spanstats.hip)."""
    import _hip
    probs, dtype, single = device_track(probs, decoder.what)
    C, T = probs.shape
    want_stats = bool(ctx.get("want_stats"))
    if "fps" in ctx:
        ctx["fps_host"] = fps_per_channel(ctx["fps"], C)
    if T == 0 or C == 0 or not settings:
        out = [[np.zeros((0, 2), np.int64) for _ in settings] for _ in range(C)]
        stats = [[(np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float64)) for _ in settings] for _ in range(C)]
    else:
        out, stats = [[] for _ in range(C)], [[] for _ in range(C)]
        if want_stats:
            import spanstats
            stats_ws = spanstats.prepare_device(probs, dtype)
        step = decoder.round_size(_hip.lib(), len(settings))
        for k0 in range(0, len(settings), step):
            _, table, counts, _ = _device_tables(decoder, probs, dtype, settings[k0:k0 + step], ctx)
            if want_stats:
                triple = spanstats.to_host(*spanstats.stats_device(probs, dtype, stats_ws, table, counts))
            rows, edges = table.cpu().numpy(), np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])
            for i in range(len(counts)):                # the tables lie back to back in c * K + k order
                out[i // (len(counts) // C)].append(rows[edges[i]:edges[i + 1]].astype(np.int64))
                if want_stats:
                    stats[i // (len(counts) // C)].append(tuple(a[edges[i]:edges[i + 1]] for a in triple))
    if want_stats:
        ctx["stats"] = stats[0] if single else stats
    return out[0] if single else out


def _instances(decoder, probs, thresholds, min_lengths, fps, axis_values, device, table=None, stats=False):
    """{(threshold, *axis values, min_length): [(start_s, end_s), ...]}, thresholds-major, then the axes in their order, then
    min_length: the decoder's spans as (first / fps, last / fps), kept iff end - start > min_length.  device: probs is a (T,) track
    in GPU memory and the spans come from there; the seconds and the filter are evaluated on the host either way.  stats: ->
    (that dictionary, {same key: float64 (n, 3) array (mean, peak_time, peak_value) of exactly its instances, in their order}), the
    integers from span_stats on the host or from csrc/spanstats.hip on the device (`confidences` either way); without it nothing
    of that runs."""
    if device and getattr(probs, "ndim", None) != 1:
        import _hip
        raise _hip.LadHipError(f"probs must be a (T,) GPU tensor (the device {decoder.what} has no CPU fallback)")
    ctx = {"table": table, "want_stats": bool(stats)}
    keys, settings = decoder.keys(list(thresholds), [list(values) for values in axis_values], ctx)
    min_lengths = list(min_lengths)
    if decoder is not THRESHOLD:            # (the reference's own sweep takes fps as it comes)
        fps = ctx["fps"] = np.float64(_check_fps(fps))
    spans = _device_frame_spans(decoder, probs, settings, ctx) if device else decoder.host_spans(probs, settings, fps, ctx)
    if not stats:
        return _instances_from_spans(keys, spans, min_lengths, fps)
    return _instances_from_spans(keys, spans, min_lengths, fps, ctx["stats"] if device else [span_stats(probs, s) for s in spans])


# ---- the public forms ------------------------------------------------------------------------------------------------------------
def get_laughter_instances(probs, thresholds=[0.5], min_lengths=[0.2], fps=100., stats=False):
    """{(threshold, min_length): [(start_s, end_s), ...]} exactly as laugh_segmenter.py:74-111: frame i is laughter iff
    p[i] > threshold; maximal runs -> (first/fps, last/fps); kept iff end - start > min_length.  Keys thresholds-major, as the
    reference iterates.  stats=True (not in the reference; here and in the five forms below): -> (that dictionary, {same key:
    float64 (n, 3) array of (mean probability, time of the peak, probability at the peak) of exactly its instances, in their
    order}) -- see span_stats and confidences."""
    return _instances(THRESHOLD, probs, thresholds, min_lengths, fps, (), device=False, stats=stats)


def get_laughter_instances_device(probs, thresholds=[0.5], min_lengths=[0.2], fps=100., stats=False):
    """get_laughter_instances for a (T,) track in GPU memory: the same dictionary (keys, thresholds-major order, Python floats)."""
    return _instances(THRESHOLD, probs, thresholds, min_lengths, fps, (), device=True, stats=stats)


def get_laughter_frame_spans(probs, threshold):
    """Integer (first_frame, last_frame) runs for one threshold: the bit-exact core of get_laughter_instances."""
    return THRESHOLD.host_spans(probs, [threshold], None, {})[0]


def get_laughter_frame_spans_device(probs, thresholds):
    """Device form of get_laughter_frame_spans for a list of thresholds.  probs: (T,) GPU tensor (float32 / float64, contiguous) ->
    [int64 (n, 2) array of (first_frame, last_frame) per threshold], each equal to get_laughter_frame_spans(probs.cpu(), thr);
    (C, T) -> one such list per channel, from the same four launches."""
    return _device_frame_spans(THRESHOLD, probs, list(thresholds), {})


def binarize_frame_spans(probs, onset, offset, min_gap=0.0, fps=100.):
    """Integer (first_frame, last_frame) events of one setting: hysteresis between `onset` and `offset` (offset <= onset), then
    gap filling by `min_gap` seconds at `fps` frames per second.  int64 (n, 2).  offset == onset and min_gap == 0 is
    get_laughter_frame_spans(probs, onset)."""
    return HYSTERESIS.host_spans(probs, [_check_setting(onset, offset, min_gap)], np.float64(_check_fps(fps)), {})[0]


def binarize_frame_spans_device(probs, settings, fps=100.):
    """Device form of binarize_frame_spans for a list of settings (onset, offset, min_gap).  probs: (T,) GPU tensor (float32 /
    float64, contiguous) -> [int64 (n, 2) array per setting], each equal to binarize_frame_spans(probs.cpu(), *setting, fps);
    (C, T) -> one such list per channel, fps a float or one per channel.  More settings than lad_binarize_max_settings() are
    split into several calls.  No CPU fallback."""
    return _device_frame_spans(HYSTERESIS, probs, [_check_setting(*s) for s in settings], {"fps": fps})


def binarize_instances(probs, thresholds=[0.5], min_lengths=[0.2], fps=100., offset_drops=[0.0], min_gaps=[0.0], stats=False):
    """{(threshold, offset_drop, min_gap, min_length): [(start_s, end_s), ...]}, keys thresholds-major, then drop, then gap, then
    min_length.  The onset is the threshold and the offset is threshold - offset_drop (drop >= 0); events are (first / fps,
    last / fps) and kept iff end - start > min_length, after gap filling.  drop = 0 and gap = 0 give the lists of
    get_laughter_instances."""
    return _instances(HYSTERESIS, probs, thresholds, min_lengths, fps, (offset_drops, min_gaps), device=False, stats=stats)


def binarize_instances_device(probs, thresholds=[0.5], min_lengths=[0.2], fps=100., offset_drops=[0.0], min_gaps=[0.0], stats=False):
    """binarize_instances for a (T,) track in GPU memory: the same dictionary (keys, order, Python floats)."""
    return _instances(HYSTERESIS, probs, thresholds, min_lengths, fps, (offset_drops, min_gaps), device=True, stats=stats)


def viterbi_frame_spans(probs, threshold, penalty, table=None, unit=1024):
    """Integer (first_frame, last_frame) runs of the best on/off path for one setting: log-odds relative to `threshold`, `penalty`
    nats per event (viterbi_settings).  int64 (n, 2).  This is the parity form of csrc/viterbi.hip -- a Python loop over the frames
    -- not a fast one: a 60 min track takes seconds."""
    table = _viterbi_table(table)
    return _viterbi_spans_host(probs, viterbi_settings([threshold], [penalty], table, unit), table)[0]


def viterbi_frame_spans_device(probs, settings, table=None):
    """Device form of the decoder for a list of settings (bias, penalty) as viterbi_settings returns them.  probs: (T,) GPU tensor
    (float32 / float64, contiguous) -> [int64 (n, 2) array per setting]; (C, T) -> one such list per channel.  More settings than
    lad_viterbi_max_settings() go in several rounds.  No CPU fallback."""
    device_track(probs, VITERBI.what)       # (refused before the table and the settings are looked at)
    ctx = {"table": _viterbi_table(table)}
    return _device_frame_spans(VITERBI, probs, _check_viterbi_settings(settings), ctx)


def viterbi_instances(probs, thresholds=[0.5], min_lengths=[0.2], fps=100., penalties=[0.0], table=None, stats=False):
    """{(threshold, penalty, min_length): [(start_s, end_s), ...]}, keys thresholds-major, then penalty, then min_length: the runs of
    the decoded path as (first / fps, last / fps), kept iff end - start > min_length.  Host form (see viterbi_frame_spans)."""
    return _instances(VITERBI, probs, thresholds, min_lengths, fps, (penalties,), device=False, table=table, stats=stats)


def viterbi_instances_device(probs, thresholds=[0.5], min_lengths=[0.2], fps=100., penalties=[0.0], table=None, stats=False):
    """viterbi_instances for a (T,) track in GPU memory: the same dictionary (keys, order, Python floats)."""
    return _instances(VITERBI, probs, thresholds, min_lengths, fps, (penalties,), device=True, table=table, stats=stats)
