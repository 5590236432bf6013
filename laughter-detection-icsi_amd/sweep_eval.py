"""Scores of the threshold sweep against the transcript: what the reference's analysis/ computes from 87 TextGrid files per channel.

Reference: analysis/utils.py:8-37 (to_frames, to_sec, p_len: a time base of integer milliseconds, Python's round), analysis/
preprocess.py:13-24 (seg_invalid), :27-46 (append_to_index), :49-120 (the laugh / invalid / speech / noise indices), :133-167 (the
silence index), analysis/analyse.py:120-149 (laugh_match), :152-225 (eval_preds), :255-257 (the 14 columns), :269-298
(calc_sum_stats).  The reference keeps every set as a `portion` interval union and measures it by iterating its milliseconds;
here a set is a sorted (n, 2) array of (lo, hi] end points and an overlap is a difference of two coverage values.

    TranscriptIndex        the five interval sets per channel (INVALID, LAUGH, SPEECH, NOISE, SILENCE) and the per-meeting totals
    score_instances        host scorer of one channel's get_laughter_instances dictionary -> {(thr, min_l): 7 ints}
    score_sweep_host       the host sweep + score_instances for several tracks -> int64 (C, K, L, 7)
    score_sweep_device     the same array for tracks in GPU memory (csrc/runs.hip + csrc/score.hip): besides the C x K run counts
                           only the scores cross to the host.  No CPU fallback.
                           Both take offset_drops= / min_gaps= (laugh_segmenter.HYSTERESIS) and then return (C, K, D, G, L, 7),
                           or penalties= (laugh_segmenter.VITERBI) and then return (C, K, P, L, 7): the family comes from
                           laugh_segmenter.decoder_for, once per call, and its Decoder record supplies the axes (columns, array
                           shape, key tuples), the settings and the device tables.
    score_surface_host     the array of score_sweep_host for ascending levels without a loop over them: each node of the track's
                           component tree scored once, a difference array over the levels, one cumulative sum
    score_surface_device   the same array for tracks in GPU memory and up to 4096 levels in one call (csrc/surface.hip).  No CPU
                           fallback.
                           Both take events=(min_overlap_ms, min_overlap_pct) and then return (scores, events): the event fields
                           of every level from the same nodes (csrc/surface_events.hip: lad_score_surface_events)
    pr_summary             average precision and the best F1 per min_len from calc_sum_stats' rows of one dense grid
    event_pr_summary       the same three figures from event_sum_stats' rows (event precision / recall) of one dense grid
    eval_rows              per (meeting, threshold, min_len) the 14 columns of create_evaluation_df
    calc_sum_stats         threshold, min_len, precision, recall over all meetings
    event_scores_instances host event scorer of one channel's dictionary -> {key: 7 ints} (include/lad_hip.h: lad_score_events has
                           the convention; not in the reference, which counts events on both sides and never matches them)
                           score_sweep_host / score_sweep_device take events=(min_overlap_ms, min_overlap_pct) and then return
                           (scores, events), the second from event_scores_instances / csrc/events.hip
    event_rows             per (meeting, threshold, min_len) event precision, recall, F1, fragmentation and boundary errors
    event_sum_stats        the same figures over all meetings
    bootstrap_units        the resampling unit (channel or meeting) of every evaluated channel, and each unit's transcribed ms
    bootstrap_sum_stats_host    percentile-bootstrap intervals of precision, recall and F1 (and of event precision / recall with
                           events=) over those units: exact quantiles of ratios of integer sums (bootstrap.py)
    bootstrap_sum_stats_device  the same rows from csrc/bootstrap.hip.  No CPU fallback.
    bootstrap_diff_sum_stats_host / _device   two systems scored on the same channels: their point figures, the exact difference A - B
                           with its interval under the same resamples, and the share of resamples in which A is strictly better
    label_histogram_host / _device, calibration_figures   the frame-level, threshold-free view of the track (calibration.py; csrc/
                           calibration.hip): per bucket of the track's value the milliseconds of every class, and from them Brier
                           score, NLL, ECE, ROC AUC and the reliability table

Everything is integer arithmetic plus a few IEEE float64 operations, so host and device agree exactly.
"""
import ctypes
import operator

import numpy as np

import bootstrap
import laugh_segmenter as ls

CLASSES = ("invalid", "laugh", "speech", "noise", "silence")          # include/lad_hip.h: enum lad_score_class
FIELDS = ("n_pred", "n_valid", "pred_ms", "corr_ms", "fp_speech_ms", "fp_noise_ms", "fp_silence_ms")   # enum lad_score_field
EVAL_COLUMNS = ["meeting", "threshold", "min_len", "precision", "recall", "corr_pred_time", "tot_pred_time", "tot_transc_laugh_time",
                "num_of_pred_laughs", "valid_pred_laughs", "num_of_transc_laughs", "tot_fp_speech_time", "tot_fp_noise_time",
                "tot_fp_silence_time"]                                # analyse.py:255-257
SUM_COLUMNS = ["threshold", "min_len", "precision", "recall"]         # analyse.py:290
PR_COLUMNS = ["min_len", "average_precision", "best_f1", "best_f1_threshold"]     # pr_summary (not in the reference)
EVENT_PR_COLUMNS = ["min_len", "event_average_precision", "best_event_f1", "best_event_f1_threshold"]        # event_pr_summary
EVENT_FIELDS = ("n_ref", "ref_touched", "ref_hit", "pred_hit", "links", "onset_abs_ms", "offset_abs_ms")      # enum lad_event_field
EVENT_COLUMNS = ["meeting", "threshold", "min_len", "event_precision", "event_recall", "event_f1", "num_ref_events",
                 "ref_events_touched", "ref_events_hit", "valid_pred_laughs", "pred_laughs_hit", "links",
                 "fragments_per_touched_event", "mean_onset_err", "mean_offset_err"]
EVENT_SUM_COLUMNS = EVENT_COLUMNS[1:]


def columns(base, decoder):
    """One of EVAL_COLUMNS, SUM_COLUMNS, EVENT_COLUMNS, EVENT_SUM_COLUMNS for a laugh_segmenter.Decoder: its extra axes (not in the
    reference) follow min_len."""
    at = base.index("min_len") + 1
    return base[:at] + list(decoder.axes) + base[at:]


EVAL_COLUMNS_BINARIZE, EVAL_COLUMNS_VITERBI = columns(EVAL_COLUMNS, ls.HYSTERESIS), columns(EVAL_COLUMNS, ls.VITERBI)
SUM_COLUMNS_BINARIZE, SUM_COLUMNS_VITERBI = columns(SUM_COLUMNS, ls.HYSTERESIS), columns(SUM_COLUMNS, ls.VITERBI)
EVENT_COLUMNS_BINARIZE, EVENT_COLUMNS_VITERBI = columns(EVENT_COLUMNS, ls.HYSTERESIS), columns(EVENT_COLUMNS, ls.VITERBI)
EVENT_SUM_COLUMNS_BINARIZE, EVENT_SUM_COLUMNS_VITERBI = columns(EVENT_SUM_COLUMNS, ls.HYSTERESIS), columns(EVENT_SUM_COLUMNS, ls.VITERBI)
ROW_COLUMNS = ("meeting_id", "part_id", "chan", "start", "end", "length", "type", "laugh_type")
CHANNEL_COLUMNS = ("meeting_id", "part_id", "chan", "length")
FACTOR = 1000.0                # utils.py:14: 1000 / frame_duration, frame_duration = 1 ms (config.py:46-52)
MIN_LAUGH_LENGTH = 0.2         # preprocess.py:22: cfg["model"]["min_length"]
_EMPTY = np.zeros((0, 2), np.int64)


def to_frames(t):
    """utils.py:8-15: round(t * factor), Python's round on a float (half to even); numpy.rint is the same function."""
    return np.rint(np.asarray(t, dtype=np.float64) * FACTOR).astype(np.int64)


def to_sec(n):
    """utils.py:18-25"""
    return n / FACTOR


# ---- interval sets: int64 (n, 2) arrays of (lo, hi], sorted, disjoint, non-empty, not touching -----------------------------------
def normalise(iv):
    """Union of arbitrary (lo, hi] rows: empty ones (hi <= lo) dropped, the part below 0 cut off (no prediction reaches it),
    overlapping and adjacent ones merged."""
    iv = np.asarray(iv, dtype=np.int64).reshape(-1, 2)
    iv = np.stack([np.maximum(iv[:, 0], 0), iv[:, 1]], axis=1)
    iv = iv[iv[:, 1] > iv[:, 0]]
    if len(iv) == 0:
        return _EMPTY
    iv = iv[np.argsort(iv[:, 0], kind="stable")]
    reach = np.maximum.accumulate(iv[:, 1])
    first = np.concatenate([[True], iv[1:, 0] > reach[:-1]])           # a row that starts beyond everything before it
    starts = np.flatnonzero(first)
    ends = np.concatenate([starts[1:], [len(iv)]]) - 1
    return np.stack([iv[starts, 0], reach[ends]], axis=1)


def _member(iv, x):
    """x in the set, element-wise."""
    if len(iv) == 0:
        return np.zeros(len(x), bool)
    i = np.searchsorted(iv[:, 0], x, side="left") - 1                  # the last interval with lo < x
    return (i >= 0) & (x <= iv[np.maximum(i, 0), 1])


def subtract(a, b):
    """a minus b for two normalised sets."""
    if len(a) == 0 or len(b) == 0:
        return a
    pts = np.unique(np.concatenate([a.ravel(), b.ravel()]))
    right = pts[1:]                                                     # (pts[i], pts[i + 1]] lies wholly inside or outside each set
    keep = _member(a, right) & ~_member(b, right)
    return normalise(np.stack([pts[:-1][keep], right[keep]], axis=1))


def _cum(iv):
    return np.concatenate([[0], np.cumsum(iv[:, 1] - iv[:, 0])])[:-1] if len(iv) else np.zeros(0, np.int64)


def coverage(iv, x):
    """F(x) = milliseconds of the set in (0, x], element-wise (csrc/score.hip evaluates the same expression)."""
    x = np.asarray(x, dtype=np.int64)
    if len(iv) == 0:
        return np.zeros(x.shape, np.int64)
    i = np.searchsorted(iv[:, 0], x, side="left") - 1
    j = np.maximum(i, 0)
    return np.where(i >= 0, _cum(iv)[j] + np.minimum(x, iv[j, 1]) - iv[j, 0], 0)


def _records(table, columns):
    """Rows as dictionaries: a pandas DataFrame, an iterable of mappings, or an iterable of tuples in column order."""
    if hasattr(table, "to_dict") and hasattr(table, "columns"):
        table = table.to_dict("records")
    out = []
    for r in table:
        out.append(dict(r) if hasattr(r, "keys") else dict(zip(columns, r)))
        missing = [c for c in columns if c not in out[-1]]
        if missing:
            raise ValueError(f"row {len(out) - 1} lacks {missing}")
    return out


class DeviceIndex:
    """The CSR form csrc/score.hip reads, for a list of channels: bounds int32 (n, 2), offsets int32 (C * 5 + 1) on the device, and
    the host copies lad_score_runs checks before it launches anything."""

    def __init__(self, channels, bounds_host, offsets_host, device):
        import torch
        self.channels = list(channels)
        self.bounds_host = np.ascontiguousarray(bounds_host, dtype=np.int32).reshape(-1, 2)
        self.offsets_host = np.ascontiguousarray(offsets_host, dtype=np.int32)
        self.bounds = torch.from_numpy(self.bounds_host if len(self.bounds_host) else np.zeros((1, 2), np.int32)).to(device)
        self.offsets = torch.from_numpy(self.offsets_host).to(device)
        self.device = self.bounds.device                                           # ("cuda" -> the device it resolved to)

    @property
    def n_intervals(self):
        return len(self.bounds_host)


class TranscriptIndex:
    """preprocess.py's five indices from the transcript rows (columns of parse.py's DataFrames: meeting_id, part_id, chan, start,
    end, length, type, laugh_type; type in laugh / speech / noise / invalid) and the channel table (meeting_id, part_id, chan,
    length; part_id None or '' for a channel that is mapped to no participant: analyse.py:27-28 does not evaluate it).
    Built once per corpus, pure numpy."""

    def __init__(self, rows, channels):
        rows = _records(rows, ROW_COLUMNS)
        chans = _records(channels, CHANNEL_COLUMNS)
        self._part = {}                     # (meeting, chan) -> part_id or None
        self._length = {}                   # (meeting, part) -> channel length in seconds
        for c in chans:
            part = c["part_id"] if c["part_id"] not in (None, "") else None
            key = (c["meeting_id"], c["chan"])
            if key in self._part:
                raise ValueError(f"channel {key} is listed twice")
            self._part[key] = part
            if part is not None:
                if (c["meeting_id"], part) in self._length:
                    raise ValueError(f"participant {part} of {c['meeting_id']} has two channels")
                self._length[(c["meeting_id"], part)] = float(c["length"])
        for r in rows:
            if r["type"] not in CLASSES[:4]:
                raise ValueError(f"row type {r['type']!r}: one of {CLASSES[:4]}")
        self.meetings = sorted({c["meeting_id"] for c in chans} | {r["meeting_id"] for r in rows})
        self._raw = {}                      # (meeting, part) -> {class: [(lo, hi), ...]}
        self._tot = {m: {k: [0, 0] for k in CLASSES[:4]} for m in self.meetings}      # class -> [tot_len, tot_events]
        self._laugh_rows = {m: 0 for m in self.meetings}
        # preprocess.py:193-196: the invalid rows first, then the laugh rows (which add to the invalid index), speech, noise;
        # each by meeting, participants ascending, rows by start (:66-86, :108-118)
        for kind in ("invalid", "laugh", "speech", "noise"):
            sel = [r for r in rows if r["type"] == kind]
            sel.sort(key=lambda r: float(r["start"]))                              # (stable)
            sel.sort(key=lambda r: (r["meeting_id"], r["part_id"]))
            for r in sel:
                m = r["meeting_id"]
                target = kind
                if kind == "laugh":
                    self._laugh_rows[m] += 1
                    if float(r["length"]) < MIN_LAUGH_LENGTH or r["laugh_type"] == "breath-laugh":      # seg_invalid :13-24
                        target = "invalid"
                lo, hi = int(to_frames(float(r["start"]))), int(to_frames(float(r["end"])))
                if hi >= 2 ** 31:
                    raise ValueError(f"row ends at {hi} ms: millisecond values are int32")
                self._raw.setdefault((m, r["part_id"]), {k: [] for k in CLASSES[:4]})[target].append((lo, hi))
                self._tot[m][target][0] += to_sec(max(hi - lo, 0))                 # append_to_index :42-45 (p_len of one interval)
                self._tot[m][target][1] += 1
        self._sets = {}
        self._device = {}

    # ---- per meeting -------------------------------------------------------------------------------------------------------------
    def tot_len(self, meeting_id, kind="laugh"):
        """Sum of the rows' lengths in seconds (not the length of their union): index[meeting]['tot_len']."""
        return self._tot[meeting_id][kind][0]

    def tot_events(self, meeting_id, kind="laugh"):
        return self._tot[meeting_id][kind][1]

    def laugh_ms(self, meeting_id, part_id=None):
        """The integer milliseconds behind tot_len(meeting_id, "laugh"): the sum of max(hi - lo, 0) over the rows filed under
        "laugh" (not the length of their union), of the whole meeting or of one participant."""
        return sum(max(hi - lo, 0) for (m, part), raw in self._raw.items() if m == meeting_id and part_id in (None, part)
                   for lo, hi in raw["laugh"])

    def num_laugh_rows(self, meeting_id):
        """Rows of type laugh in the input table (parse.laugh_only_df of the meeting: analyse.py:163-164)."""
        return self._laugh_rows[meeting_id]

    # ---- per channel -------------------------------------------------------------------------------------------------------------
    def channels(self, meeting_id=None):
        return [k for k in self._part if meeting_id is None or k[0] == meeting_id]

    def participant(self, meeting_id, chan):
        return self._part[(meeting_id, chan)]

    def intervals(self, meeting_id, chan):
        """{class: int64 (n, 2) array of (lo, hi]} as preprocess.py holds them (each class the union of its own rows, SILENCE the
        rest of (0, to_frames(length)]); None for a channel without a participant."""
        part = self._part[(meeting_id, chan)]
        if part is None:
            return None
        key = (meeting_id, part)
        if key not in self._sets:
            raw = self._raw.get(key, {})
            sets = {k: normalise(raw.get(k, [])) for k in CLASSES[:4]}
            full = normalise([(0, int(to_frames(self._length[key])))])
            if len(full) and full[0, 1] >= 2 ** 31:
                raise ValueError(f"channel {chan} of {meeting_id} ends at {full[0, 1]} ms: millisecond values are int32")
            silence = full
            for k in ("laugh", "invalid", "speech", "noise"):                      # preprocess.py:157-163
                silence = subtract(silence, sets[k])
            sets["silence"] = silence
            self._sets[key] = sets
        return self._sets[key]

    def scoring_sets(self, meeting_id, chan):
        """The five sets in class order as the scorers use them: INVALID, and the other four minus INVALID (laugh_match :129-131
        subtracts INVALID from the prediction; subtracting it from the classes once gives the same overlaps).  Five empty sets for
        a channel without a participant."""
        sets = self.intervals(meeting_id, chan)
        if sets is None:
            return [_EMPTY] * len(CLASSES)
        return [sets["invalid"]] + [subtract(sets[k], sets["invalid"]) for k in CLASSES[1:]]

    def to_device(self, channels, device="cuda"):
        """DeviceIndex of a list of (meeting_id, chan) (kept: a second call with the same list returns the same tensors)."""
        import torch
        key = (tuple(channels), str(torch.device(device)))
        if key not in self._device:
            parts = [s for mc in channels for s in self.scoring_sets(*mc)]
            offsets = np.concatenate([[0], np.cumsum([len(p) for p in parts])])
            if offsets[-1] >= 2 ** 30:
                raise ValueError("the index holds more than 2^30 intervals")
            bounds = np.concatenate(parts) if parts else _EMPTY
            self._device[key] = DeviceIndex(channels, bounds, offsets, device)
        return self._device[key]


def _score_spans(a, b, sets):
    """The seven integers for predictions (a, b] (int64 arrays) against the five scoring sets."""
    cover = [coverage(s, b) - coverage(s, a) for s in sets]
    pred = (b - a) - cover[0]
    valid = pred > 0 if len(sets[0]) else np.ones(len(a), bool)                    # analyse.py:185-187
    return (len(a), int(np.count_nonzero(valid)), int(pred.sum()), int(cover[1].sum()), int(cover[2].sum()), int(cover[3].sum()),
            int(cover[4].sum()))


def score_instances(instances, index, meeting_id, chan):
    """Host scorer of one channel: instances as get_laughter_instances returns them -> {(thr, min_l): (n_pred, n_valid, pred_ms,
    corr_ms, fp_speech_ms, fp_noise_ms, fp_silence_ms)}, each prediction (start_s, end_s) being the millisecond interval
    (to_frames(start), to_frames(end)] (analyse.py:179-181)."""
    sets = index.scoring_sets(meeting_id, chan)
    out = {}
    for key, spans in instances.items():
        s = np.asarray(spans, dtype=np.float64).reshape(-1, 2)
        out[key] = _score_spans(to_frames(s[:, 0]), to_frames(s[:, 1]), sets)
    return out


def _event_criteria(events):
    """(min_overlap_ms, min_overlap_pct) as two ints (TypeError for anything that is not an integer)."""
    min_ms, min_pct = (operator.index(v) for v in events)
    return min_ms, min_pct


def _event_spans(a, b, sets, min_ms, min_pct):
    """The seven integers of lad_score_events for predictions (a, b] (int64 arrays in table order) against the scoring sets."""
    invalid, laugh = sets[0], sets[1]
    need = max(1, min_ms)
    lov = coverage(laugh, b) - coverage(laugh, a)
    pred = (b - a) - (coverage(invalid, b) - coverage(invalid, a))
    pred_hit = int(np.count_nonzero((lov >= need) & (100 * lov >= min_pct * pred)))
    real = b > a                                                                   # a == b overlaps nothing
    a, b = a[real], b[real]
    if len(laugh) == 0 or len(a) == 0:
        return (len(laugh), 0, 0, pred_hit, 0, 0, 0)
    # the predictions left are disjoint with a and b ascending, so those linked to (lo, hi] are the rows from the first with b > lo
    # up to the last with a < hi, and cov is the coverage of the prediction set itself
    lo, hi = laugh[:, 0], laugh[:, 1]
    i0, i1 = np.searchsorted(b, lo, side="right"), np.searchsorted(a, hi, side="left")
    frag = i1 - i0
    spans = np.stack([a, b], axis=1)
    cov = coverage(spans, hi) - coverage(spans, lo)
    hit = (cov >= need) & (100 * cov >= min_pct * (hi - lo))
    onset = np.abs(a[np.minimum(i0, len(a) - 1)] - lo)
    offset = np.abs(b[np.maximum(i1 - 1, 0)] - hi)
    return (len(laugh), int(np.count_nonzero(frag)), int(np.count_nonzero(hit)), pred_hit, int(frag.sum()), int(onset[hit].sum()),
            int(offset[hit].sum()))


def event_scores_instances(instances, index, meeting_id, chan, min_overlap_ms=1, min_overlap_pct=0):
    """Host event scorer of one channel: instances as get_laughter_instances / binarize_instances return them -> {key: (n_ref,
    ref_touched, ref_hit, pred_hit, links, onset_abs_ms, offset_abs_ms)} by the convention above lad_score_events in
    include/lad_hip.h: the events are the channel's LAUGH intervals (transcribed laughter minus INVALID, merged), a prediction is
    (to_frames(start), to_frames(end)], a pair is linked iff it shares a millisecond.  An event is hit iff the predictions cover
    max(1, min_overlap_ms) ms and min_overlap_pct per cent of it, a prediction iff LAUGH covers as much of its part outside INVALID."""
    min_ms, min_pct = _event_criteria((min_overlap_ms, min_overlap_pct))
    if min_ms < 0 or not 0 <= min_pct <= 100:
        raise ValueError(f"min_overlap_ms >= 0 and min_overlap_pct in 0..100, got ({min_ms}, {min_pct})")
    sets = index.scoring_sets(meeting_id, chan)
    out = {}
    for key, spans in instances.items():
        s = np.asarray(spans, dtype=np.float64).reshape(-1, 2)
        out[key] = _event_spans(to_frames(s[:, 0]), to_frames(s[:, 1]), sets, min_ms, min_pct)
    return out


def _cells(thresholds, min_lengths, axes):
    """[(index into a score array behind the channel, threshold, min_length, the values of the decoder's axes)], thresholds-major,
    then the axes in their order, then min_length.  axes: their value lists, as laugh_segmenter.decoder_for returns them."""
    extras = [((), ())]
    for axis in axes:
        extras = [(at + (i,), extra + (v,)) for at, extra in extras for i, v in enumerate(axis)]
    return [((k, *at, l), thr, min_l, extra) for k, thr in enumerate(thresholds) for at, extra in extras
            for l, min_l in enumerate(min_lengths)]


def _score_shape(C, thresholds, min_lengths, axes):
    return (C, len(thresholds), *[len(a) for a in axes], len(min_lengths), len(FIELDS))


def score_sweep_host(tracks, channels, thresholds, min_lengths, fps, index, offset_drops=None, min_gaps=None, events=None,
                     penalties=None):
    """laugh_segmenter.get_laughter_instances + score_instances per track -> int64 (C, K, L, 7).  tracks: C arrays (lengths may
    differ); channels: C (meeting_id, chan); fps: a float or C floats.
    offset_drops / min_gaps (either given) or penalties: the dictionaries of laugh_segmenter.HYSTERESIS or VITERBI instead, and
    the lengths of their axes behind K: (C, K, D, G, L, 7) or (C, K, P, L, 7); ValueError for both kinds together.
    events=(min_overlap_ms, min_overlap_pct): returns (scores, events), the second an array of the same shape with the seven
    EVENT_FIELDS of event_scores_instances."""
    thresholds, min_lengths = list(thresholds), list(min_lengths)
    f = ls.fps_per_channel(fps, len(channels), each=float).tolist()
    decoder, axes = ls.decoder_for(offset_drops, min_gaps, penalties)
    cells = _cells(thresholds, min_lengths, axes)
    out = np.zeros(_score_shape(len(channels), thresholds, min_lengths, axes), np.int64)
    ev = None if events is None else np.zeros(out.shape, np.int64)
    for c, (track, mc) in enumerate(zip(tracks, channels)):
        instances = ls._instances(decoder, track, thresholds, min_lengths, f[c], axes, device=False)
        got = score_instances(instances, index, *mc)
        got_ev = None if events is None else event_scores_instances(instances, index, *mc, *events)
        for at, thr, min_l, extra in cells:
            out[(c, *at)] = got[(thr, *extra, min_l)]
            if ev is not None:
                ev[(c, *at)] = got_ev[(thr, *extra, min_l)]
    return out if events is None else (out, ev)


def _device_head(probs, what, channels, behind, fps, index, lowpass, median, lengths, events):
    """What the two device scorers do alike before they reach the library, in the order of their checks: the track
    (laugh_segmenter.device_track), the one-smoother rule, the channel count, fps, the result of a call with nothing to launch on
    (the result has the shape (C, *behind)), the smoother, the rule for `lengths`, the DeviceIndex.  Returns (None, that result)
    or ((probs, dtype, DeviceIndex, fps as a float64 host array, the event criteria or None), None)."""
    probs, dtype, _ = ls.device_track(probs, what)
    if lowpass is not None and median is not None:
        raise ValueError("lowpass and median are two smoothers for the same place: give one of them")
    C, T = probs.shape
    if C != len(channels):
        raise ValueError(f"{C} tracks for {len(channels)} channels")
    fps_host = ls.fps_per_channel(fps, C, each=float)
    out_shape = (C, *behind)
    criteria = None if events is None else _event_criteria(events)
    if T == 0 or 0 in out_shape:
        if criteria is None:
            return None, np.zeros(out_shape, np.int64)
        ev = np.zeros(out_shape, np.int64)          # (nothing to launch on: no prediction, the events of each channel counted)
        if 0 not in out_shape:
            offsets = (index if isinstance(index, DeviceIndex) else index.to_device(channels, probs.device)).offsets_host
            ev[..., 0] = np.diff(offsets)[1::len(CLASSES)].reshape((C,) + (1,) * (len(out_shape) - 2))
        return None, (np.zeros(out_shape, np.int64), ev)
    if lowpass is not None:
        probs, dtype, _ = ls.device_track(ls.lowpass_device(probs, cutoff=lowpass, lengths=lengths), what)
    elif median is not None:
        probs, dtype, _ = ls.device_track(ls.median_filter_device(probs, median, lengths=lengths), what)
    elif lengths is not None:
        raise ValueError("lengths are the true frame counts for the low-pass: give a cutoff as well")
    dix = index if isinstance(index, DeviceIndex) else index.to_device(channels, probs.device)
    if dix.channels != channels or dix.device != probs.device:
        raise ValueError("the DeviceIndex was built for other channels or another device")
    return (probs, dtype, dix, fps_host, criteria), None


def _index_and_lengths(dix, ctx, min_lengths):
    """The ten arguments every scoring entry point ends its inputs with: the index on the device and on the host, fps
    (ctx["fps_host"]) on the device and on the host, the min_lengths and their number."""
    return (dix.bounds, dix.offsets, dix.bounds_host, dix.offsets_host, dix.n_intervals, ls.on_device(ctx, "fps_host", dix.device),
            ctx["fps_host"], (ctypes.c_double * len(min_lengths))(*[float(m) for m in min_lengths]), len(min_lengths))


def score_sweep_device(probs, channels, thresholds, min_lengths, fps, index, lowpass=None, lengths=None, offset_drops=None,
                       min_gaps=None, events=None, penalties=None, median=None):
    """probs: (C, T) or (T,) float32 / float64 GPU tensor, a shorter channel padded with NaN (off for every threshold) -> int64 numpy
    (C, K, L, 7), equal to score_sweep_host of the same tracks.  channels: C (meeting_id, chan); fps: a float or C floats; index: a
    TranscriptIndex (or the DeviceIndex of these channels).  The decoder's count + fill (laugh_segmenter._device_tables) + lad_score_runs
    (include/lad_hip.h) per round of at most decoder.round_size settings: the run tables never leave the device.
    lowpass: a cutoff (of Nyquist): every track is smoothed on the device first (laugh_segmenter.lowpass_device: lad_lowpass before
    the count), channel c over its first lengths[c] frames (lengths=None: all T; the padding stays NaN).
    median: a window in frames (odd, 1..1023): every track goes through the median filter on the device first instead
    (laugh_segmenter.median_filter_device: lad_rank_filter), with `lengths` as for lowpass; ValueError for both smoothers together.
    offset_drops / min_gaps (either given) or penalties: HYSTERESIS or VITERBI instead of THRESHOLD -> (C, K, D, G, L, 7) or
    (C, K, P, L, 7), equal to score_sweep_host with the same lists; ValueError for both kinds together.
    events=(min_overlap_ms, min_overlap_pct): returns (scores, events), the second an int64 array of the same shape with the seven
    EVENT_FIELDS, equal to score_sweep_host's: lad_score_events on the same workspace and table as lad_score_runs, in the same
    round; the two score arrays are all that crosses to the host.  Without it no further launch is made."""
    import torch

    import _hip
    channels, thresholds, min_lengths = list(channels), list(thresholds), list(min_lengths)
    decoder, axes = ls.decoder_for(offset_drops, min_gaps, penalties)
    out_shape = _score_shape(len(channels), thresholds, min_lengths, axes)
    head, empty = _device_head(probs, "scorer", channels, out_shape[1:], fps, index, lowpass, median, lengths, events)
    if head is None:
        return empty
    probs, dtype, dix, fps_host, criteria = head
    C, T = probs.shape
    L = len(min_lengths)
    lib = _hip.lib()
    ctx = {"fps_host": fps_host}
    index_and_lengths = _index_and_lengths(dix, ctx, min_lengths)
    settings = decoder.keys(thresholds, axes, ctx)[1]
    step = decoder.round_size(lib, len(settings))
    parts, ev_parts = [], []
    for k0 in range(0, len(settings), step):
        chunk = settings[k0:k0 + step]
        n = len(chunk)
        sws = _hip.workspace("lad_score_workspace_bytes", C, dix.n_intervals, n, L, device=probs.device)
        ws, table, counts, _ = ls._device_tables(decoder, probs, dtype, chunk, ctx)
        with torch.cuda.device(probs.device):
            # what the two scorers are given alike: the tables, the index, fps and min_lengths
            scored = (ws, table, counts, C, T, n, *index_and_lengths)
            scores = torch.empty((C, n, L, len(FIELDS)), dtype=torch.int64, device=probs.device)
            _hip.launch("lad_score_runs", *scored, sws, scores)
            if criteria is not None:
                ews = _hip.workspace("lad_score_events_workspace_bytes", C, dix.n_intervals, n, L, len(table), device=probs.device)
                ev = torch.empty((C, n, L, len(EVENT_FIELDS)), dtype=torch.int64, device=probs.device)
                _hip.launch("lad_score_events", *scored, *criteria, ews, ev)
                ev_parts.append(ev.cpu().numpy())
        parts.append(scores.cpu().numpy())
    scores = np.concatenate(parts, axis=1).reshape(out_shape)
    return scores if criteria is None else (scores, np.concatenate(ev_parts, axis=1).reshape(out_shape))


def _surface_levels(levels):
    """The levels of the dense sweep as float64: finite and strictly ascending (what lad_score_surface asks of them)."""
    lv = np.asarray([float(t) for t in levels], dtype=np.float64)
    if not np.isfinite(lv).all() or (np.diff(lv) <= 0).any():
        raise ValueError("the levels of the dense sweep must be finite and ascend strictly")
    return lv


def _surface_nodes(track, levels):
    """The component tree of one track (include/lad_hip.h: lad_score_surface has the convention): int64 arrays first, last, base,
    top, one entry per node -- the frame interval [first, last] is a row of the run table of the levels base <= j < top.  One loop
    over the frames with a stack of the frames that still wait for a smaller bin to their right."""
    q = ls.fix_probs(track)
    bins = np.searchsorted(levels, q, side="left")                                  # levels strictly below q
    bins[np.isnan(q)] = 0
    b = bins.tolist()
    T = len(b)
    right = [T] * T                                                                # the nearest frame to the right with a smaller bin
    left = [0] * T                                                                 # the nearest frame to the left with a bin <= this one
    stack = []
    for i, x in enumerate(b):
        while stack and b[stack[-1]] > x:
            right[stack.pop()] = i
        left[i] = stack[-1] if stack else -1
        stack.append(i)
    left, right = np.asarray(left, np.int64), np.asarray(right, np.int64)
    padded = np.concatenate([bins, [0]])                                           # (index -1 and T: a neighbour beyond the track)
    lb, rb = padded[left], padded[right]
    rep = np.flatnonzero((bins > 0) & (lb < bins))                                 # the leftmost minimum of its interval
    return left[rep] + 1, right[rep] - 1, np.maximum(lb[rep], rb[rep]), bins[rep]


def _surface_event_fields(nodes, a, b, kept, sets, n_frames, fps, K, min_ms, min_pct):
    """The seven EVENT_FIELDS of one track for every (level, min_length), int64 (K, L, 7), from its component tree: nodes = (first,
    last, base, top) of _surface_nodes, (a, b] their millisecond intervals, kept bool (nodes, L).  PRED_HIT and LINKS are sums over
    nodes and go through a difference array over the levels.  The rest is per event (lo, hi]: to_frames(f / fps) does not decrease
    with the frame f, so with F0 the first frame whose millisecond is > lo and F1 the last whose millisecond is < hi, a node is linked
    to the event iff first <= F1, last >= F0 and a < b; the linked nodes of one level are disjoint and in order, so the first one has
    the smallest a and the last one the largest b."""
    first, last, base, top = nodes
    invalid, laugh = sets[0], sets[1]
    L = kept.shape[1]
    need = max(1, min_ms)
    out = np.zeros((K, L, len(EVENT_FIELDS)), np.int64)
    out[:, :, 0] = len(laugh)
    if len(laugh) == 0 or len(first) == 0:
        return out                                                                 # no event: no link, no prediction overlaps LAUGH
    lov = coverage(laugh, b) - coverage(laugh, a)
    pred = (b - a) - (coverage(invalid, b) - coverage(invalid, a))
    pred_hit = ((lov >= need) & (100 * lov >= min_pct * pred)).astype(np.int64)
    lo, hi = laugh[:, 0], laugh[:, 1]
    links = np.where(b > a, np.searchsorted(lo, b, side="left") - np.searchsorted(hi, a, side="right"), 0)
    w = np.stack([pred_hit, links], axis=1)
    diff = np.zeros((K + 1, L, 2), np.int64)
    for l in range(L):
        np.add.at(diff[:, l], base[kept[:, l]], w[kept[:, l]])
        np.subtract.at(diff[:, l], top[kept[:, l]], w[kept[:, l]])
    out[:, :, 3:5] = np.cumsum(diff, axis=0)[:K]
    ms = to_frames(np.arange(n_frames) / fps)
    real = b > a
    far = np.iinfo(np.int64).max
    for e_lo, e_hi in laugh.tolist():
        f0, f1 = int(np.searchsorted(ms, e_lo, side="right")), int(np.searchsorted(ms, e_hi, side="left")) - 1
        if f0 >= n_frames or f1 < 0:
            continue
        linked = np.flatnonzero(real & (first <= f1) & (last >= f0))
        if len(linked) == 0:
            continue
        cov, frag = np.zeros((K + 1, L), np.int64), np.zeros((K + 1, L), np.int64)
        first_a, last_b = np.full((K, L), far, np.int64), np.full((K, L), -1, np.int64)
        ov = np.minimum(b[linked], e_hi) - np.maximum(a[linked], e_lo)
        for n, o in zip(linked.tolist(), ov.tolist()):
            k = kept[n]
            rows = slice(int(base[n]), int(top[n]))
            cov[rows] += np.where(k, o, 0)
            frag[rows] += k
            first_a[rows] = np.minimum(first_a[rows], np.where(k, a[n], far))
            last_b[rows] = np.maximum(last_b[rows], np.where(k, b[n], -1))
        cov, frag = cov[:K], frag[:K]
        touched = frag > 0
        hit = touched & (cov >= need) & (100 * cov >= min_pct * (e_hi - e_lo))
        out[:, :, 1] += touched
        out[:, :, 2] += hit
        out[:, :, 5] += np.where(hit, np.abs(first_a - e_lo), 0)
        out[:, :, 6] += np.where(hit, np.abs(last_b - e_hi), 0)
    return out


def score_surface_host(tracks, channels, levels, min_lengths, fps, index, events=None):
    """The array of score_sweep_host(tracks, channels, levels, min_lengths, fps, index), int64 (C, K, L, 7), for ascending levels
    without a loop over them: every node of a track's component tree (_surface_nodes) is scored once, its seven integers go to a
    difference array over the levels, +w at row base and -w at row top, and one cumulative sum gives all K rows.  The parity form
    of score_surface_device.
    events=(min_overlap_ms, min_overlap_pct): returns (scores, events), the second the array of score_sweep_host(..., events=) with
    the seven EVENT_FIELDS, from the same nodes (_surface_event_fields; include/lad_hip.h: lad_score_surface_events) and without a
    call of the per-level scorers.  Event recall (ref_hit / n_ref) does not grow with the level: a kept run of a higher level lies
    inside a kept run of every lower one, so what covers an event at level j + 1 covers it at level j."""
    lv, min_lengths = _surface_levels(levels), list(min_lengths)
    f = ls.fps_per_channel(fps, len(channels), each=float).tolist()
    K, L = len(lv), len(min_lengths)
    criteria = None if events is None else _event_criteria(events)
    if criteria is not None and (criteria[0] < 0 or not 0 <= criteria[1] <= 100):
        raise ValueError(f"min_overlap_ms >= 0 and min_overlap_pct in 0..100, got {criteria}")
    out = np.zeros((len(channels), K, L, len(FIELDS)), np.int64)
    ev = None if criteria is None else np.zeros((len(channels), K, L, len(EVENT_FIELDS)), np.int64)
    for c, (track, mc) in enumerate(zip(tracks, channels)):
        first, last, base, top = _surface_nodes(track, lv)
        sets = index.scoring_sets(*mc)
        starts, ends = first / f[c], last / f[c]
        a, b = to_frames(starts), to_frames(ends)
        cover = [coverage(s, b) - coverage(s, a) for s in sets]
        pred = (b - a) - cover[0]
        valid = pred > 0 if len(sets[0]) else np.ones(len(a), bool)                # analyse.py:185-187
        w = np.stack([np.ones(len(a), np.int64), valid.astype(np.int64), pred, *cover[1:]], axis=1)
        length = ends - starts
        diff = np.zeros((K + 1, L, len(FIELDS)), np.int64)
        for l, min_l in enumerate(min_lengths):
            keep = length > min_l
            np.add.at(diff[:, l], base[keep], w[keep])
            np.subtract.at(diff[:, l], top[keep], w[keep])
        out[c] = np.cumsum(diff, axis=0)[:K]
        if ev is not None and K and L:
            kept = length[:, None] > np.asarray(min_lengths, np.float64)[None, :]
            ev[c] = _surface_event_fields((first, last, base, top), a, b, kept, sets, len(track), f[c], K, *criteria)
    return out if ev is None else (out, ev)


def score_surface_device(probs, channels, levels, min_lengths, fps, index, lowpass=None, lengths=None, events=None, median=None):
    """probs: (C, T) or (T,) float32 / float64 GPU tensor, a shorter channel padded with NaN -> int64 numpy (C, K, L, 7), equal to
    score_surface_host (and so to score_sweep_host) of the same tracks, for up to lad_surface_max_levels() ascending levels in one
    call of lad_score_surface (include/lad_hip.h; csrc/surface.hip): no run table is built and only the scores cross to the host.
    channels, fps, index, lowpass, median and lengths as for score_sweep_device.  No CPU fallback.
    events=(min_overlap_ms, min_overlap_pct): returns (scores, events), the second an int64 array of the same shape with the seven
    EVENT_FIELDS, equal to score_surface_host's: both from one call of lad_score_surface_events (csrc/surface_events.hip), one set
    of bins and one tree."""
    import torch

    import _hip
    channels, min_lengths = list(channels), list(min_lengths)
    lv = _surface_levels(levels)
    K, L = len(lv), len(min_lengths)
    out_shape = (len(channels), K, L, len(FIELDS))
    head, empty = _device_head(probs, "surface scorer", channels, out_shape[1:], fps, index, lowpass, median, lengths, events)
    if head is None:
        return empty
    probs, dtype, dix, fps_host, criteria = head
    C, T = probs.shape
    size_query = "lad_surface_workspace_bytes" if criteria is None else "lad_surface_events_workspace_bytes"
    with torch.cuda.device(probs.device):
        ws = _hip.workspace(size_query, C, T, dix.n_intervals, K, L, device=probs.device)
        scores = torch.empty(out_shape, dtype=torch.int64, device=probs.device)
        ctx = {"fps_host": fps_host}
        track_and_index = (probs, dtype, C, T, lv, K, *_index_and_lengths(dix, ctx, min_lengths))
        if criteria is None:
            _hip.launch("lad_score_surface", *track_and_index, ws, scores)
            return scores.cpu().numpy()
        ev = torch.empty(out_shape, dtype=torch.int64, device=probs.device)
        _hip.launch("lad_score_surface_events", *track_and_index, *criteria, ws, scores, ev)
        return scores.cpu().numpy(), ev.cpu().numpy()


def pr_summary(sum_rows):
    """Per min_len of one dense grid, from the rows of calc_sum_stats (threshold, min_len, precision, recall; thresholds ascending
    within a min_len): rows [min_len, average_precision, best_f1, best_f1_threshold].  With P_j, R_j the precision and recall at
    threshold j of K, average_precision = sum_j (R_j - R_{j+1}) * P_j with R_K = 0 (recall does not grow with the threshold, so no
    term is negative); F1_j = 2 P_j R_j / (P_j + R_j), 0 where both are 0, the best one the largest, at the lowest threshold that
    reaches it.  A min_len whose recall is NaN or inf (nothing transcribed) has NaN for all three."""
    groups = {}
    for thr, min_len, prec, recall in sum_rows:
        groups.setdefault(min_len, []).append((thr, float(prec), float(recall)))
    out = []
    nan = float("nan")
    for min_len in sorted(groups):
        rows = sorted(groups[min_len])
        P, R = [r[1] for r in rows], [r[2] for r in rows]
        if not all(np.isfinite(R)):
            out.append([min_len, nan, nan, nan])
            continue
        ap = 0.0
        for j in range(len(rows)):
            ap += (R[j] - (R[j + 1] if j + 1 < len(rows) else 0.0)) * P[j]
        best, best_thr = -1.0, nan
        for (thr, _, _), p, r in zip(rows, P, R):
            f1 = 0.0 if p + r == 0 else 2 * p * r / (p + r)
            if f1 > best:
                best, best_thr = f1, thr
        out.append([min_len, ap, best, best_thr])
    return out


def event_pr_summary(event_sum_rows):
    """pr_summary's rule on the event-level figures of one dense grid: from the rows of event_sum_stats (EVENT_SUM_COLUMNS:
    threshold, min_len, event_precision, event_recall, ...) rows of EVENT_PR_COLUMNS per min_len: the event average precision
    sum_j (R_j - R_{j+1}) * P_j, the best event F1 and the lowest threshold that reaches it.  Event recall does not grow with the
    threshold (a kept run of a higher level lies inside a kept run of every lower one), so no term is negative.  A min_len without
    an event (NaN recall) has NaN for all three."""
    return pr_summary([r[:4] for r in event_sum_rows])


def eval_rows(scores, channels, thresholds, min_lengths, index, offset_drops=None, min_gaps=None, penalties=None):
    """eval_preds (analyse.py:152-225) for every meeting and setting: a list of 14-value rows in EVAL_COLUMNS order, meetings
    ascending, thresholds-major.  scores: (C, K, L, 7) of score_sweep_host / score_sweep_device for `channels`.  Channels without a
    participant are left out (analyse.py:27-28); the float sums run over participants in ascending part_id order (:173-197).
    offset_drops / min_gaps (either given): scores is (C, K, D, G, L, 7) and a row has the 16 values of EVAL_COLUMNS_BINARIZE
    (offset_drop and min_gap behind min_len), thresholds-major, then drop, then gap, then min_len.
    penalties: scores is (C, K, P, L, 7) and a row has the 15 values of EVAL_COLUMNS_VITERBI (penalty behind min_len)."""
    scores = np.asarray(scores)
    axes = ls.decoder_for(offset_drops, min_gaps, penalties)[1]
    settings = [(at, (thr, min_l, *extra)) for at, thr, min_l, extra in _cells(thresholds, min_lengths, axes)]
    per_meeting = {}
    for c, (m, chan) in enumerate(channels):
        part = index.participant(m, chan)
        if part is not None:
            per_meeting.setdefault(m, []).append((part, c))
    rows = []
    for m in sorted(per_meeting):
        parts = sorted(per_meeting[m])
        tot_transc = index.tot_len(m, "laugh")
        n_transc = index.num_laugh_rows(m)
        for at, key in settings:
            corr_t = incorr_t = speech_t = noise_t = silence_t = 0
            n_pred = n_valid = 0
            for _, c in parts:
                s = [int(v) for v in scores[(c,) + at]]
                n_pred += s[0]
                n_valid += s[1]
                if s[0] == 0:
                    continue                                                       # (no row of this participant: groupby skips it)
                pred_length = to_sec(s[2])                                         # laugh_match :133-145
                correct = to_sec(s[3])
                corr_t += correct
                incorr_t += pred_length - correct
                speech_t += to_sec(s[4])
                noise_t += to_sec(s[5])
                silence_t += to_sec(s[6])
            pred_t = corr_t + incorr_t
            prec = 1 if pred_t == 0 else corr_t / pred_t
            recall = float("nan") if tot_transc == 0 else corr_t / tot_transc
            rows.append([m, *key, prec, recall, corr_t, pred_t, tot_transc, n_pred, n_valid, n_transc, speech_t, noise_t, silence_t])
    return rows


def calc_sum_stats(rows, binarize=False, penalties=None, offset_drops=None, min_gaps=None):
    """analyse.py:269-298: per (min_len, threshold) the sums of corr_pred_time, tot_pred_time and tot_transc_laugh_time over the
    meetings (in row order), precision = corr / pred (1 where pred is 0), recall = corr / transcribed (float division: NaN or inf
    where that is 0).  Rows of SUM_COLUMNS, ordered by (min_len, threshold) as the groupby.
    binarize: the rows are eval_rows' 16-value ones; grouped by (min_len, threshold, offset_drop, min_gap), rows of
    SUM_COLUMNS_BINARIZE.
    penalties (not None): the rows are eval_rows' 15-value ones; grouped by (min_len, threshold, penalty), rows of SUM_COLUMNS_VITERBI.
    offset_drops / min_gaps (either given) say what binarize=True says, so that eval_rows' keywords can be passed on as they are."""
    n_keys = 2 + len(_rows_decoder(binarize, penalties, offset_drops, min_gaps).axes)
    sums = {}
    for r in rows:
        acc = sums.setdefault((r[2], r[1]) + tuple(r[3:1 + n_keys]), [0, 0, 0])
        acc[0] += r[1 + n_keys + 2]
        acc[1] += r[1 + n_keys + 3]
        acc[2] += r[1 + n_keys + 4]
    out = []
    for key in sorted(sums):
        corr, pred, transc = (np.float64(v) for v in sums[key])
        with np.errstate(divide="ignore", invalid="ignore"):
            prec = 1.0 if pred == 0 else float(corr / pred)
            recall = float(corr / transc)
        out.append([key[1], key[0], *key[2:], prec, recall])
    return out


def _rows_decoder(binarize, penalties, offset_drops=None, min_gaps=None):
    """The decoder whose rows calc_sum_stats / event_sum_stats were given: a row has the meeting, threshold and min_len, then the
    decoder's axes."""
    try:
        return ls.decoder_for([] if binarize else offset_drops, min_gaps, penalties)[0]
    except ValueError:
        raise ValueError("rows are of the hysteresis sweep or of the Viterbi decoder, not both") from None


def _event_figures(n_ref, touched, hit, n_valid, pred_hit, links, onset_ms, offset_ms):
    """The twelve values behind the keys of an event row, from integers: one float64 division per figure."""
    prec = 1 if n_valid == 0 else pred_hit / n_valid                               # (the reference's rule for time precision)
    recall = float("nan") if n_ref == 0 else hit / n_ref
    if recall != recall:
        f1 = float("nan")
    else:
        f1 = 0.0 if prec + recall == 0 else 2 * prec * recall / (prec + recall)
    nan = float("nan")
    return [prec, recall, f1, n_ref, touched, hit, n_valid, pred_hit, links, links / touched if touched else nan,
            onset_ms / (FACTOR * hit) if hit else nan, offset_ms / (FACTOR * hit) if hit else nan]


def event_rows(scores, events, channels, thresholds, min_lengths, index, offset_drops=None, min_gaps=None, penalties=None):
    """Per meeting and setting, in eval_rows' order, the values of EVENT_COLUMNS (EVENT_COLUMNS_BINARIZE with offset_drops / min_gaps,
    EVENT_COLUMNS_VITERBI with penalties)
    from the two arrays of score_sweep_host / score_sweep_device with events=.  The integers are summed over the meeting's
    participants first (channels without one are left out).  event_precision = pred_laughs_hit / valid_pred_laughs (scores'
    n_valid), 1 where there is no valid prediction; event_recall = ref_events_hit / num_ref_events, NaN without an event; event_f1
    NaN with a NaN recall and 0 where precision + recall is 0; fragments_per_touched_event = links / ref_events_touched, NaN
    without one; mean_onset_err and mean_offset_err in seconds over the hit events, NaN without one."""
    scores, events = np.asarray(scores), np.asarray(events)
    if scores.shape != events.shape:
        raise ValueError(f"scores {scores.shape} and events {events.shape} are not of one sweep")
    axes = ls.decoder_for(offset_drops, min_gaps, penalties)[1]
    settings = [(at, (thr, min_l, *extra)) for at, thr, min_l, extra in _cells(thresholds, min_lengths, axes)]
    per_meeting = {}
    for c, (m, chan) in enumerate(channels):
        if index.participant(m, chan) is not None:
            per_meeting.setdefault(m, []).append(c)
    rows = []
    for m in sorted(per_meeting):
        for at, key in settings:
            e = [sum(int(events[(c,) + at][f]) for c in per_meeting[m]) for f in range(len(EVENT_FIELDS))]
            n_valid = sum(int(scores[(c,) + at][1]) for c in per_meeting[m])
            rows.append([m, *key, *_event_figures(e[0], e[1], e[2], n_valid, e[3], e[4], e[5], e[6])])
    return rows


def event_sum_stats(rows, binarize=False, penalties=None, offset_drops=None, min_gaps=None):
    """The figures of event_rows over all meetings, from the summed integers, grouped and ordered as calc_sum_stats: rows of
    EVENT_SUM_COLUMNS (EVENT_SUM_COLUMNS_BINARIZE; EVENT_SUM_COLUMNS_VITERBI with penalties).  A row holds its two error sums as
    means in seconds; mean * 1000 * hit is within a few units in the last place of the integer it came from, so rint gives that
    integer back (sums below 2^50 ms)."""
    n_keys = 2 + len(_rows_decoder(binarize, penalties, offset_drops, min_gaps).axes)
    sums = {}
    for r in rows:
        v = r[1 + n_keys + 3:]                                                     # behind precision, recall and F1
        hit = v[2]
        ms = [int(np.rint(mean * FACTOR * hit)) if hit else 0 for mean in v[7:9]]
        acc = sums.setdefault((r[2], r[1]) + tuple(r[3:1 + n_keys]), [0] * 8)
        for i, x in enumerate(list(v[:6]) + ms):
            acc[i] += int(x)
    return [[key[1], key[0], *key[2:], *_event_figures(*sums[key])] for key in sorted(sums)]


# ---- bootstrap intervals of the summary figures (bootstrap.py; csrc/bootstrap.hip) ---------------------------------------------
SUM_CI_COLUMNS = ["threshold", "min_len", "precision", "precision_lo", "precision_hi", "recall", "recall_lo", "recall_hi", "f1", "f1_lo",
                  "f1_hi", "n_boot_valid"]
EVENT_SUM_CI_COLUMNS = ["threshold", "min_len", "event_precision", "event_precision_lo", "event_precision_hi", "event_recall",
                        "event_recall_lo", "event_recall_hi", "n_boot_valid"]
# A cell of the time matrix holds (pred_ms, corr_ms), a cell of the event matrix (n_valid, pred_hit, ref_hit, n_ref); the shared
# last column of both is the unit's transcribed milliseconds.  The figures of a cell, as bootstrap.cell_figures reads them:
_S = bootstrap.SHARED
_TIME_FIGURES = [(1, 1, 0, None, None, 1),          # precision = corr / pred, 1 where nothing is predicted
                 (1, 1, _S, None, None, 0),         # recall = corr / transcribed, invalid where nothing is transcribed
                 (1, 2, 0, _S, _S, 0)]              # F1 = 2 corr / (pred + transcribed), invalid where recall is
_EVENT_FIGURES = [(1, 1, 0, None, None, 1),         # event precision = pred_hit / n_valid, 1 without a valid prediction
                  (2, 1, 3, None, None, 0)]         # event recall = ref_hit / n_ref, invalid without an event


def bootstrap_units(channels, index, unit="channel"):
    """The resampling unit of every evaluated channel: (unit_of, transc_ms).  unit_of[c] is the unit number of channels[c], -1 for
    a channel without a participant (left out, as in eval_rows); transc_ms[g] the transcribed laughter of unit g in integer
    milliseconds (TranscriptIndex.laugh_ms).  unit="channel": every evaluated channel is a unit, in the order given, with its
    participant's milliseconds; unit="meeting": the meetings with an evaluated channel, ascending, with the meeting's."""
    if unit not in ("channel", "meeting"):
        raise ValueError(f"unit is 'channel' or 'meeting', got {unit!r}")
    evaluated = [(c, m, index.participant(m, chan)) for c, (m, chan) in enumerate(channels)]
    evaluated = [(c, m, part) for c, m, part in evaluated if part is not None]
    unit_of = [-1] * len(channels)
    if unit == "channel":
        for g, (c, _, _) in enumerate(evaluated):
            unit_of[c] = g
        return unit_of, [index.laugh_ms(m, part) for _, m, part in evaluated]
    meetings = sorted({m for _, m, _ in evaluated})
    for c, m, _ in evaluated:
        unit_of[c] = meetings.index(m)
    return unit_of, [index.laugh_ms(m) for m in meetings]


def _unit_matrix(fields, unit_of, transc_ms):
    """int64 (G, n_cells * F + 1): fields (C, n_cells, F) summed over the channels of every unit, then the shared column."""
    G = len(transc_ms)
    per_unit = np.zeros((G,) + fields.shape[1:], np.int64)
    evaluated = [c for c, g in enumerate(unit_of) if g >= 0]
    np.add.at(per_unit, [unit_of[c] for c in evaluated], fields[evaluated])
    return np.concatenate([per_unit.reshape(G, -1), np.asarray(transc_ms, np.int64).reshape(G, 1)], axis=1)


def _ratio(num, den):
    """One IEEE division of two integers (Python's int / int is correctly rounded); NaN for the pair (-1, -1) of an empty order."""
    return float("nan") if num < 0 else int(num) / int(den)


def _number(fraction):
    """One IEEE division for a fraction (num, den) of Python integers; NaN for None (a figure that does not exist)."""
    return float("nan") if fraction is None else fraction[0] / fraction[1]


def _time_fractions(cell, transc):
    """Precision, recall and F1 of a cell (pred_ms, corr_ms) as (num, den), None where the figure is NaN."""
    pred, corr = cell
    return ((corr, pred) if pred else (1, 1), (corr, transc) if transc else None, (2 * corr, pred + transc) if transc else None)


def _event_fractions(cell, _):
    """Event precision and recall of a cell (n_valid, pred_hit, ref_hit, n_ref) as (num, den), None where the figure is NaN."""
    n_valid, pred_hit, ref_hit, n_ref = cell
    return ((pred_hit, n_valid) if n_valid else (1, 1), (ref_hit, n_ref) if n_ref else None)


def _sweep_cells(scores, channels, thresholds, min_lengths, events, offset_drops, min_gaps, penalties):
    """What both bootstraps ask of a score array: (scores, its cells -- _cells runs in the array's own order --, their order in
    calc_sum_stats' rows)."""
    scores = np.asarray(scores)
    axes = ls.decoder_for(offset_drops, min_gaps, penalties)[1]
    cells = _cells(list(thresholds), list(min_lengths), axes)
    if scores.shape != _score_shape(len(channels), list(thresholds), list(min_lengths), axes):
        raise ValueError(f"scores {scores.shape} are not of this sweep")
    if events is not None and np.asarray(events).shape != scores.shape:
        raise ValueError(f"scores {scores.shape} and events {np.asarray(events).shape} are not of one sweep")
    return scores, cells, sorted(range(len(cells)), key=lambda j: (cells[j][2], cells[j][1], *cells[j][3]))


def _event_fields(flat, events):
    """(C, n_cells, 4): a cell of the event matrix, (n_valid, pred_hit, ref_hit, n_ref)."""
    ev = np.asarray(events).reshape(flat.shape[0], flat.shape[1], len(EVENT_FIELDS))
    return np.stack([flat[:, :, 1], ev[:, :, 3], ev[:, :, 2], ev[:, :, 0]], axis=2)


def _bootstrap_sum_stats(intervals, pair_intervals, scores, channels, thresholds, min_lengths, index, n_boot, seed, level, unit, events,
                         offset_drops, min_gaps, penalties, event_f1):
    if event_f1 and events is None:
        raise ValueError("event_f1=True needs events=")
    scores, cells, order = _sweep_cells(scores, channels, thresholds, min_lengths, events, offset_drops, min_gaps, penalties)
    unit_of, transc_ms = bootstrap_units(channels, index, unit)
    if not transc_ms:
        raise ValueError("no channel with a participant: nothing to resample")
    quantiles = bootstrap.quantile_pairs(level)
    flat = scores.reshape(len(channels), len(cells), len(FIELDS))

    def rows_of(x, per_cell, template, fractions):
        out, valid = intervals(x, per_cell, template, n_boot, seed, quantiles)
        total = [int(v) for v in x.sum(axis=0)]
        rows = []
        for j in order:
            _, thr, min_l, extra = cells[j]
            row = [thr, min_l, *extra]
            for f, figure in enumerate(fractions(total[j * per_cell:(j + 1) * per_cell], total[-1])):
                row += [_number(figure), _ratio(*out[j, f, 0]), _ratio(*out[j, f, 1])]
            rows.append(row + [int(valid[j].min())])
        return rows

    time_rows = rows_of(_unit_matrix(flat[:, :, 2:4], unit_of, transc_ms), 2, _TIME_FIGURES, _time_fractions)
    if events is None:
        return time_rows
    x = _unit_matrix(_event_fields(flat, events), unit_of, transc_ms)
    event_rows_ = rows_of(x, 4, _EVENT_FIGURES, _event_fractions)
    if event_f1:
        # the harmonic mean of the cell's own precision and recall (valid where both are: where recall is, so n_boot_valid stands)
        out, _, _ = pair_intervals(x, 4, _EVENT_F1_PAIR, n_boot, seed, quantiles, systems=1)
        total = [int(v) for v in x.sum(axis=0)]
        for row, j in zip(event_rows_, order):
            n_valid, pred_hit, ref_hit, n_ref = total[4 * j:4 * j + 4]
            point = _event_figures(n_ref, 0, ref_hit, n_valid, pred_hit, 0, 0, 0)[2]           # (event_sum_stats' own arithmetic)
            row[-1:-1] = [float(point), *(bootstrap.pair_value(bootstrap.HARMONIC, out[j, 0, k]) for k in (0, 1))]
    return time_rows, event_rows_


def bootstrap_sum_stats_host(scores, channels, thresholds, min_lengths, index, n_boot=2000, seed=0, level=95, unit="channel", events=None,
                             offset_drops=None, min_gaps=None, penalties=None, event_f1=False):
    """Percentile-bootstrap intervals of calc_sum_stats' figures over recording units (include/lad_hip.h: lad_bootstrap_weights has
    the convention).  scores: the array of any of the four scorers for `channels`; the decoder's lists as eval_rows takes them.
    The units (bootstrap_units: channels, or meetings) are resampled with replacement n_boot times, the weights a pure function of
    (seed, replicate), so two evaluations with one seed see the same resamples; every figure is recomputed on each resample as a
    ratio of integer sums, the replicates are ordered exactly, and the quantiles (100 - level) / 200 and 1 - that (exact rationals:
    Fraction(str(level))) are one replicate's pair each, divided once.
    Returns rows of SUM_CI_COLUMNS (the decoder's axes behind min_len: columns(SUM_CI_COLUMNS, decoder)), in calc_sum_stats' order:
    threshold, min_len, precision, precision_lo, precision_hi, recall, ..., f1, f1_lo, f1_hi, n_boot_valid.  The point figures come
    from the plain unit sums: precision = corr_ms / pred_ms (1 at zero predicted time), recall = corr_ms / transcribed ms,
    f1 = 2 corr_ms / (pred_ms + transcribed ms) (both NaN at zero transcribed time); a replicate with zero transcribed time is
    invalid for recall and f1, n_boot_valid is the smallest number of valid replicates among the row's three figures, and an
    interval without a valid replicate is NaN.
    events: the second array of a scorer called with events= -> (rows, event rows), the second of EVENT_SUM_CI_COLUMNS:
    event_precision = pred_hit / n_valid (1 without a valid prediction), event_recall = ref_hit / n_ref (valid iff n_ref > 0).
    event_f1=True (with events=): the event rows carry event_f1, event_f1_lo, event_f1_hi in front of n_boot_valid
    (EVENT_SUM_CI_F1_COLUMNS).  Event F1 is not a ratio of sums: a replicate's value is the exact harmonic mean of its event
    precision and recall (bootstrap.HARMONIC: 0 where both are 0), the replicates are ordered by 256-bit cross products, and the
    two ends are one conversion of an exact fraction each; the point figure is event_sum_stats' event_f1, by its own arithmetic.
    The difference of two systems is bootstrap_diff_sum_stats_host; event F1 of two systems is not differenced (a difference of
    two harmonic means is four figures and 512-bit products), and average precision has no interval.
    This is the parity form: numpy and Python integers, no float before the final division."""
    return _bootstrap_sum_stats(bootstrap.intervals_host, bootstrap.pair_intervals_host, scores, channels, thresholds, min_lengths, index,
                                n_boot, seed, level, unit, events, offset_drops, min_gaps, penalties, event_f1)


def bootstrap_sum_stats_device(scores, channels, thresholds, min_lengths, index, n_boot=2000, seed=0, level=95, unit="channel", events=None,
                               offset_drops=None, min_gaps=None, penalties=None, event_f1=False, device="cuda"):
    """bootstrap_sum_stats_host on the GPU (csrc/bootstrap.hip through bootstrap.intervals_device): the per-unit matrix is checked
    on the host (0 <= x < 2^40) and uploaded once, the cells go through lad_bootstrap_sums and lad_bootstrap_quantiles in chunks
    whose sums buffer stays within bootstrap.SUMS_BYTES_CAP, and only the selected pairs and the valid counts come back.  Equal
    rows (NaN matching NaN) whatever the chunk size; event_f1=True through lad_bootstrap_pair_quantiles.  No CPU fallback."""

    def intervals(x, per_cell, template, n_boot, seed, quantiles):
        return bootstrap.intervals_device(x, per_cell, template, n_boot, seed, quantiles, device=device)

    def pair_intervals(x, per_cell, template, n_boot, seed, quantiles, systems=2):
        return bootstrap.pair_intervals_device(x, per_cell, template, n_boot, seed, quantiles, systems=systems, device=device)
    return _bootstrap_sum_stats(intervals, pair_intervals, scores, channels, thresholds, min_lengths, index, n_boot, seed, level, unit, events,
                                offset_drops, min_gaps, penalties, event_f1)


# ---- the difference of two systems under the same resamples (bootstrap.pair_intervals_*; lad_bootstrap_pair_quantiles) ----------------
def _diff_columns(figures):
    return ["threshold", "min_len", *(f + s for f in figures for s in ("_a", "_b", "_diff", "_diff_lo", "_diff_hi", "_gt")), "n_boot_valid"]


SUM_DIFF_COLUMNS = _diff_columns(("precision", "recall", "f1"))
EVENT_SUM_DIFF_COLUMNS = _diff_columns(("event_precision", "event_recall"))
EVENT_SUM_CI_F1_COLUMNS = EVENT_SUM_CI_COLUMNS[:-1] + ["event_f1", "event_f1_lo", "event_f1_hi", "n_boot_valid"]
_A, _B = 0, 1                  # the system a figure of a pair template reads (bootstrap.pair_cell_figures)
_TIME_DIFFS = [(bootstrap.DIFFERENCE, (_A, *f), (_B, *f)) for f in _TIME_FIGURES]
_EVENT_DIFFS = [(bootstrap.DIFFERENCE, (_A, *f), (_B, *f)) for f in _EVENT_FIGURES]
_EVENT_F1_PAIR = [(bootstrap.HARMONIC, (_A, *_EVENT_FIGURES[0]), (_A, *_EVENT_FIGURES[1]))]


def _bootstrap_diff_sum_stats(pair_intervals, scores_a, scores_b, channels, thresholds, min_lengths, index, n_boot, seed, level, unit,
                              events_a, events_b, offset_drops, min_gaps, penalties):
    if (events_a is None) != (events_b is None):
        raise ValueError("events_a and events_b go together")
    scores_a, cells, order = _sweep_cells(scores_a, channels, thresholds, min_lengths, events_a, offset_drops, min_gaps, penalties)
    scores_b = np.asarray(scores_b)
    if scores_b.shape != scores_a.shape:
        raise ValueError(f"scores_a {scores_a.shape} and scores_b {scores_b.shape} are not of one sweep and the same channels")
    if events_b is not None and np.asarray(events_b).shape != scores_b.shape:
        raise ValueError(f"scores {scores_b.shape} and events_b {np.asarray(events_b).shape} are not of one sweep")
    unit_of, transc_ms = bootstrap_units(channels, index, unit)
    if not transc_ms:
        raise ValueError("no channel with a participant: nothing to resample")
    quantiles = bootstrap.quantile_pairs(level)
    flat_a, flat_b = (s.reshape(len(channels), len(cells), len(FIELDS)) for s in (scores_a, scores_b))
    nan = float("nan")

    def rows_of(fields_a, fields_b, per_cell, template, fractions):
        xa, xb = (_unit_matrix(f, unit_of, transc_ms) for f in (fields_a, fields_b))
        x = np.concatenate([xa[:, :-1], xb], axis=1)                               # A's cells, B's cells, the shared column
        out, valid, signs = pair_intervals(x, per_cell, template, n_boot, seed, quantiles)
        total_a, total_b = ([int(v) for v in m.sum(axis=0)] for m in (xa, xb))
        rows = []
        for j in order:
            _, thr, min_l, extra = cells[j]
            row = [thr, min_l, *extra]
            both = (fractions(t[j * per_cell:(j + 1) * per_cell], t[-1]) for t in (total_a, total_b))
            for f, (a, b) in enumerate(zip(*both)):
                diff = nan if a is None or b is None else bootstrap.pair_value(bootstrap.DIFFERENCE, (*a, *b))
                v = int(valid[j, f])
                row += [_number(a), _number(b), diff, *(bootstrap.pair_value(bootstrap.DIFFERENCE, out[j, f, k]) for k in (0, 1)),
                        int(signs[j, f, 2]) / v if v else nan]
            rows.append(row + [int(valid[j].min())])
        return rows

    time_rows = rows_of(flat_a[:, :, 2:4], flat_b[:, :, 2:4], 2, _TIME_DIFFS, _time_fractions)
    if events_a is None:
        return time_rows
    return time_rows, rows_of(_event_fields(flat_a, events_a), _event_fields(flat_b, events_b), 4, _EVENT_DIFFS, _event_fractions)


def bootstrap_diff_sum_stats_host(scores_a, scores_b, channels, thresholds, min_lengths, index, n_boot=2000, seed=0, level=95, unit="channel",
                                  events_a=None, events_b=None, offset_drops=None, min_gaps=None, penalties=None):
    """Two systems A and B, scored by one sweep on the same channels (score arrays of one shape: ValueError otherwise): is A better
    than B?  Both are resampled with the same weights -- those of bootstrap_sum_stats_host for this seed --, every figure of both is
    recomputed on each resample, and the replicates are ordered by the exact difference A - B (include/lad_hip.h:
    lad_bootstrap_pair_quantiles).  The errors of two systems on the same channels are correlated, so this interval is as a rule
    much narrower than either system's own.
    Returns rows of SUM_DIFF_COLUMNS (the decoder's axes behind min_len: columns(SUM_DIFF_COLUMNS, decoder)), in calc_sum_stats'
    order: threshold, min_len, then for each of precision, recall and f1 six columns -- <f>_a and <f>_b, the point figures of
    bootstrap_sum_stats_host; <f>_diff, the exact A - B of the plain unit sums converted once (NaN where either is NaN);
    <f>_diff_lo and <f>_diff_hi, the quantiles (100 - level) / 200 and 1 - that of the replicates' differences, each
    float(Fraction(n1, d1) - Fraction(n2, d2)) of one replicate; <f>_gt, the share of valid replicates in which A is strictly
    greater (NaN without one) -- and n_boot_valid, the smallest number of valid replicates among the row's figures (a replicate is
    valid for a difference where it is for both systems' figures).
    events_a, events_b (both): -> (rows, event rows), the second of EVENT_SUM_DIFF_COLUMNS, for event_precision and event_recall.
    Event F1 of two systems is not differenced: a difference of two harmonic means is four figures, and ordering it exactly takes
    512-bit products.  Nor is average precision.
    This is the parity form: numpy and Python integers, no float before the final conversion."""
    return _bootstrap_diff_sum_stats(bootstrap.pair_intervals_host, scores_a, scores_b, channels, thresholds, min_lengths, index, n_boot, seed,
                                     level, unit, events_a, events_b, offset_drops, min_gaps, penalties)


def bootstrap_diff_sum_stats_device(scores_a, scores_b, channels, thresholds, min_lengths, index, n_boot=2000, seed=0, level=95,
                                    unit="channel", events_a=None, events_b=None, offset_drops=None, min_gaps=None, penalties=None,
                                    device="cuda"):
    """bootstrap_diff_sum_stats_host on the GPU (csrc/bootstrap.hip through bootstrap.pair_intervals_device): one matrix of both
    systems' cells, one draw of the weights, lad_bootstrap_sums and lad_bootstrap_pair_quantiles in chunks within
    bootstrap.SUMS_BYTES_CAP.  Equal rows (NaN matching NaN) whatever the chunk size.  No CPU fallback."""

    def pair_intervals(x, per_cell, template, n_boot, seed, quantiles):
        return bootstrap.pair_intervals_device(x, per_cell, template, n_boot, seed, quantiles, device=device)
    return _bootstrap_diff_sum_stats(pair_intervals, scores_a, scores_b, channels, thresholds, min_lengths, index, n_boot, seed, level, unit,
                                     events_a, events_b, offset_drops, min_gaps, penalties)


def label_histogram_host(tracks, channels, fps, index, lengths=None, groups=None):
    """calibration.label_histogram_host: per bucket of the track's value the milliseconds of every transcript class that the frames
    in the bucket own, int64 (G, 5, 65538) (include/lad_hip.h: lad_label_histogram has the convention).  The one frame-level,
    threshold-free view of the track: calibration.calibration_figures reads Brier, NLL, ECE, ROC AUC and the reliability table
    from a row of it."""
    import calibration
    return calibration.label_histogram_host(tracks, channels, fps, index, lengths=lengths, groups=groups)


def label_histogram_device(probs, channels, fps, index, lengths=None, groups=None):
    """calibration.label_histogram_device: the same array for tracks in GPU memory (csrc/calibration.hip).  No CPU fallback."""
    import calibration
    return calibration.label_histogram_device(probs, channels, fps, index, lengths=lengths, groups=groups)


def calibration_figures(hist_row, n_bins=15):
    """calibration.calibration_figures of one histogram row."""
    import calibration
    return calibration.calibration_figures(hist_row, n_bins=n_bins)
