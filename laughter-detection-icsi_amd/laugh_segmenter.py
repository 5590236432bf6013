"""Drop-in for the live part of the reference's laugh_segmenter.py: probability track -> laughter instances.

Reference: laugh_segmenter.py:57-71 (fix_over_underflow), :19-24 (collapse / frame_span_to_time_span), :35-42
(cut_laughter_segments), :74-111 (get_laughter_instances), :141-149 (format_outputs).  Same function names, arguments and result
({(threshold, min_length): [(start_s, end_s), ...]}); the per-frame Python loop (87 passes over 360,000 frames in
the evaluation sweeps, cluster_scripts/gen_eval_exp.py:30-36) is replaced by one vectorised run-length pass per
threshold.  Integer run boundaries are bit-exact with the reference (tests/test_host_logic.py against vectors produced
by the reference itself); this is host-side integer bookkeeping on a (T,) vector, not part of the GPU arithmetic.
The Gillick-era MFCC code below laugh_segmenter.py:115 is dead in the reference and is not reproduced.

`get_laughter_instances_device` / `get_laughter_frame_spans_device` are the opt-in device form of the same sweep for a track that
is already in GPU memory (csrc/runs.hip: the run tables of all thresholds, and of several channels, in four launches): only the
compact tables cross to the host, and the dictionary is the host function's bit for bit.  They have no CPU fallback.

`binarize_frame_spans` / `binarize_instances` add the two further controls of event-detection post-processing, which the reference
does not have: hysteresis (an event starts above an onset threshold and lasts until the track falls to or below a lower offset
threshold) and gap filling (events separated by a short pause become one, before the minimum-length filter).  The convention is
written out in include/lad_hip.h (lad_binarize_count).  `binarize_frame_spans_device` / `binarize_instances_device` are their
device forms (csrc/binarize.hip), with the same results and no CPU fallback.

`viterbi_frame_spans` / `viterbi_instances` replace the frame-by-frame decision by two-state Viterbi decoding, which the reference
does not have either: a frame contributes its log-odds relative to the threshold (an int32 look-up: `viterbi_emission_table`), every
event costs a penalty, and the best-scoring set of events is returned.  The convention is written out in include/lad_hip.h
(lad_viterbi_count).  `viterbi_frame_spans_device` / `viterbi_instances_device` are the device forms (csrc/viterbi.hip), with the same
results and no CPU fallback.
"""
import math
import ctypes

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


def get_laughter_instances(probs, thresholds=[0.5], min_lengths=[0.2], fps=100.):
    """{(threshold, min_length): [(start_s, end_s), ...]} exactly as laugh_segmenter.py:74-111:
    frame i is laughter iff p[i] > threshold; maximal runs -> (first/fps, last/fps); kept iff end - start > min_length."""
    p = fix_probs(probs)
    instance_dict = {}
    for thr in thresholds:
        spans = run_spans(p > thr)
        inst_all = [(int(a) / fps, int(b) / fps) for a, b in spans]
        for min_l in min_lengths:
            instance_dict[(thr, min_l)] = [inst for inst in inst_all if inst[1] - inst[0] > min_l]
    # the reference iterates thresholds-major, min_lengths-minor: restore that key order
    return {(thr, min_l): instance_dict[(thr, min_l)] for thr in thresholds for min_l in min_lengths}


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


def get_laughter_frame_spans(probs, threshold):
    """Integer (first_frame, last_frame) runs for one threshold: the bit-exact core of get_laughter_instances."""
    return run_spans(fix_probs(probs) > threshold)


def _device_track(probs, what="sweep"):
    """What every device form asks of its probability tensor: (T,) or (C, T), in GPU memory, contiguous, float32 or float64.
    Returns (the (C, T) tensor, its lad_runs_dtype, whether it was a (T,) one)."""
    import torch

    import _hip
    single = getattr(probs, "ndim", None) == 1
    if single and hasattr(probs, "unsqueeze"):
        probs = probs.unsqueeze(0)
    if getattr(probs, "ndim", None) != 2:
        raise _hip.LadHipError(f"probs must be a (T,) or (C, T) GPU tensor (the device {what} has no CPU fallback)")
    _hip.require_cuda(probs, "probs")
    if probs.dtype not in (torch.float32, torch.float64):
        raise _hip.LadHipError(f"probs must be float32 or float64, got {probs.dtype}")
    return probs, 0 if probs.dtype == torch.float32 else 1, single


def _device_tables(probs, dtype, settings, fps_host=None, binarize=False, extra_bytes=0):
    """Count + fill of one family (include/lad_hip.h) on a (C, T) tensor that _device_track has passed, T >= 1: lad_runs_* for K
    thresholds, or with binarize lad_binarize_* for K (onset, offset, min_gap), at most lad_binarize_max_settings() of them, with
    fps_host a float64 numpy (C,).  Everything stays on the device: returns (workspace, table, counts, fps_dev) with `workspace` a
    uint8 tensor whose first lad_*_workspace_bytes bytes are the family's workspace (the tables' counts at its start, where
    lad_score_runs reads them) followed by extra_bytes for the caller, `table` the (total, 2) int32 tables back to back in
    c * K + k order, counts their row counts, int32 numpy (C * K,), and fps_dev fps_host on the device (None without one)."""
    import torch

    import _hip
    lib = _hip.lib()
    name = "lad_binarize" if binarize else "lad_runs"
    C, T = probs.shape
    K = len(settings)
    cols = [(ctypes.c_double * K)(*[float(v) for v in col]) for col in (zip(*settings) if binarize else [settings])]
    ws_bytes = getattr(lib, name + "_workspace_bytes")(C, T, K)
    _hip.check(0 if ws_bytes >= 0 else _hip.LAD_ERR_INVALID, name + "_workspace_bytes")
    with torch.cuda.device(probs.device):
        stream = _hip.stream_handle(probs.device)
        ws = torch.empty(ws_bytes + extra_bytes, dtype=torch.uint8, device=probs.device)
        fps_dev = None if fps_host is None else torch.from_numpy(fps_host).to(probs.device)
        track = (_hip.ptr(probs), dtype, C, T)

        def counts_now():
            return np.ascontiguousarray(ws[:4 * C * K].view(torch.int32).cpu().numpy())     # (synchronises)
        _hip.check(getattr(lib, name + "_count")(*track, *cols[:2], K, _hip.ptr(ws), stream), name + "_count")
        counts = counts_now()
        total = int(counts.sum(dtype=np.int64))
        cptr = counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        tables = torch.empty((2 if binarize else 1, max(total, 1), 2), dtype=torch.int32, device=probs.device)
        if binarize:            # the hysteresis runs go to tables[0], the merged ones to tables[1] and their counts over the raw ones
            _hip.check(lib.lad_binarize_fill(*track, *cols, K, _hip.ptr(fps_dev), fps_host.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                             _hip.ptr(ws), cptr, _hip.ptr(tables[0]), _hip.ptr(tables[1]), total, stream),
                       "lad_binarize_fill")
            counts = counts_now()
        else:
            _hip.check(lib.lad_runs_fill(*track, *cols, K, _hip.ptr(ws), cptr, _hip.ptr(tables[0]), total, stream), "lad_runs_fill")
        return ws, tables[-1][:int(counts.sum(dtype=np.int64))], counts, fps_dev


def _device_run_tables(probs, thresholds):
    """probs: (C, T) float32 / float64 GPU tensor, T >= 1.  Returns (counts (C, K) int64, table (total, 2) int32 numpy): the
    (c, k) tables back to back in c * K + k order."""
    probs, dtype, _ = _device_track(probs)
    _, table, counts, _ = _device_tables(probs, dtype, list(thresholds))
    return counts.astype(np.int64).reshape(len(probs), -1), table.cpu().numpy()


def _split_tables(counts, table):
    """[[ (n, 2) int64 array per threshold ] per channel] from the back-to-back tables."""
    edges = np.concatenate([[0], np.cumsum(counts.reshape(-1))])
    C, K = counts.shape
    return [[table[edges[c * K + k]:edges[c * K + k + 1]].astype(np.int64) for k in range(K)] for c in range(C)]


def _device_frame_spans(probs, settings, fps=None, binarize=False):
    """[int64 (n, 2) array per setting] for a (T,) tensor, one such list per channel for a (C, T) one: the tables of
    _device_tables on the host.  The plain sweep is one call whatever the number of thresholds (the library refuses more than
    lad_runs_max_thresholds()); settings go in rounds of at most lad_binarize_max_settings()."""
    import _hip
    probs, dtype, single = _device_track(probs)
    C, T = probs.shape
    fps_host = _fps_per_channel(fps, C) if binarize else None
    if T == 0 or C == 0 or not settings:
        out = [[np.zeros((0, 2), np.int64) for _ in settings] for _ in range(C)]
    else:
        out = [[] for _ in range(C)]
        step = int(_hip.lib().lad_binarize_max_settings()) if binarize else len(settings)
        for k0 in range(0, len(settings), step):
            _, table, counts, _ = _device_tables(probs, dtype, settings[k0:k0 + step], fps_host, binarize)
            part = _split_tables(counts.astype(np.int64).reshape(C, -1), table.cpu().numpy())
            for c in range(C):
                out[c] += part[c]
    return out[0] if single else out


def get_laughter_frame_spans_device(probs, thresholds):
    """Device form of get_laughter_frame_spans for a list of thresholds.  probs: (T,) GPU tensor (float32 / float64, contiguous) ->
    [int64 (n, 2) array of (first_frame, last_frame) per threshold], each equal to get_laughter_frame_spans(probs.cpu(), thr);
    (C, T) -> one such list per channel, from the same four launches."""
    return _device_frame_spans(probs, list(thresholds))


def _instances_from_spans(keys, spans_list, min_lengths, fps):
    """{(*key, min_length): [(start_s, end_s), ...]}, keys-major: first / fps, last / fps and end - start > min_length in float64
    (the arithmetic of the reference's Python floats) on the integer spans of each key."""
    instance_dict = {}
    for key, spans in zip(keys, spans_list):
        starts, ends = spans[:, 0] / fps, spans[:, 1] / fps
        length = ends - starts
        for min_l in min_lengths:
            keep = length > min_l
            instance_dict[(*key, min_l)] = list(zip(starts[keep].tolist(), ends[keep].tolist()))
    return instance_dict


def get_laughter_instances_device(probs, thresholds=[0.5], min_lengths=[0.2], fps=100.):
    """get_laughter_instances for a (T,) track in GPU memory: the same dictionary (keys, thresholds-major order, Python floats).
    The run tables come from the device; the seconds and the min_length filter are evaluated on them on the host."""
    import _hip
    if getattr(probs, "ndim", None) != 1:
        raise _hip.LadHipError("probs must be a (T,) GPU tensor (the device sweep has no CPU fallback)")
    thresholds = list(thresholds)
    return _instances_from_spans([(thr,) for thr in thresholds], get_laughter_frame_spans_device(probs, thresholds), min_lengths, fps)


# ---- hysteresis and gap filling (include/lad_hip.h: lad_binarize_count has the convention) ----------------------------------------
def _check_setting(onset, offset, min_gap):
    onset, offset, min_gap = float(onset), float(offset), float(min_gap)
    if not (math.isfinite(onset) and math.isfinite(offset) and math.isfinite(min_gap)):
        raise ValueError(f"onset, offset and min_gap must be finite, got ({onset}, {offset}, {min_gap})")
    if offset > onset:
        raise ValueError(f"offset {offset} lies above onset {onset}")
    if min_gap < 0:
        raise ValueError(f"min_gap must be >= 0, got {min_gap}")
    return onset, offset, min_gap


def _check_fps(fps):
    fps = float(fps)
    if not (math.isfinite(fps) and fps > 0):
        raise ValueError(f"fps must be positive and finite, got {fps}")
    return fps


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


def binarize_frame_spans(probs, onset, offset, min_gap=0.0, fps=100.):
    """Integer (first_frame, last_frame) events of one setting: hysteresis between `onset` and `offset` (offset <= onset), then
    gap filling by `min_gap` seconds at `fps` frames per second.  int64 (n, 2).  offset == onset and min_gap == 0 is
    get_laughter_frame_spans(probs, onset)."""
    onset, offset, min_gap = _check_setting(onset, offset, min_gap)
    return _fill_gaps(_hysteresis_spans(fix_probs(probs), onset, offset), min_gap, np.float64(_check_fps(fps)))


def _binarize_keys(thresholds, offset_drops, min_gaps):
    for drop in offset_drops:
        if not (math.isfinite(float(drop)) and float(drop) >= 0):
            raise ValueError(f"an offset drop must be finite and >= 0, got {drop}")
    triples = [(thr, drop, gap) for thr in thresholds for drop in offset_drops for gap in min_gaps]
    settings = [_check_setting(thr, thr - drop, gap) for thr, drop, gap in triples]        # offset = thr - drop, once, Python float
    return triples, settings


def binarize_instances(probs, thresholds=[0.5], min_lengths=[0.2], fps=100., offset_drops=[0.0], min_gaps=[0.0]):
    """{(threshold, offset_drop, min_gap, min_length): [(start_s, end_s), ...]}, keys thresholds-major, then drop, then gap, then
    min_length.  The onset is the threshold and the offset is threshold - offset_drop (drop >= 0); events are (first / fps,
    last / fps) and kept iff end - start > min_length, after gap filling.  drop = 0 and gap = 0 give the lists of
    get_laughter_instances."""
    thresholds, min_lengths, offset_drops, min_gaps = list(thresholds), list(min_lengths), list(offset_drops), list(min_gaps)
    triples, settings = _binarize_keys(thresholds, offset_drops, min_gaps)
    fps = np.float64(_check_fps(fps))
    p = fix_probs(probs)
    held = {}
    spans_list = []
    for onset, offset, gap in settings:
        if (onset, offset) not in held:
            held[(onset, offset)] = _hysteresis_spans(p, onset, offset)
        spans_list.append(_fill_gaps(held[(onset, offset)], gap, fps))
    return _instances_from_spans(triples, spans_list, min_lengths, fps)


def _fps_per_channel(fps, C, each=_check_fps):
    """One fps or C of them -> float64 numpy (C,).  each=float leaves a value that is not positive and finite to whoever divides by
    it (the library refuses it: LadHipError)."""
    f = [fps] * C if np.ndim(fps) == 0 else list(fps)
    if len(f) != C:
        raise ValueError(f"fps: one value or one per channel ({C}), got {len(f)}")
    return np.asarray([each(x) for x in f], dtype=np.float64)


def binarize_frame_spans_device(probs, settings, fps=100.):
    """Device form of binarize_frame_spans for a list of settings (onset, offset, min_gap).  probs: (T,) GPU tensor (float32 /
    float64, contiguous) -> [int64 (n, 2) array per setting], each equal to binarize_frame_spans(probs.cpu(), *setting, fps);
    (C, T) -> one such list per channel, fps a float or one per channel.  More settings than lad_binarize_max_settings() are
    split into several calls.  No CPU fallback."""
    return _device_frame_spans(probs, [_check_setting(*s) for s in settings], fps, binarize=True)


def binarize_instances_device(probs, thresholds=[0.5], min_lengths=[0.2], fps=100., offset_drops=[0.0], min_gaps=[0.0]):
    """binarize_instances for a (T,) track in GPU memory: the same dictionary (keys, order, Python floats)."""
    import _hip
    if getattr(probs, "ndim", None) != 1:
        raise _hip.LadHipError("probs must be a (T,) GPU tensor (the device sweep has no CPU fallback)")
    thresholds, min_lengths, offset_drops, min_gaps = list(thresholds), list(min_lengths), list(offset_drops), list(min_gaps)
    triples, settings = _binarize_keys(thresholds, offset_drops, min_gaps)
    fps = np.float64(_check_fps(fps))
    return _instances_from_spans(triples, binarize_frame_spans_device(probs, settings, fps), min_lengths, fps)


# ---- two-state Viterbi decoding (include/lad_hip.h: lad_viterbi_count has the convention) -----------------------------------------
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


def viterbi_frame_spans(probs, threshold, penalty, table=None, unit=1024):
    """Integer (first_frame, last_frame) runs of the best on/off path for one setting: log-odds relative to `threshold`, `penalty`
    nats per event (viterbi_settings).  int64 (n, 2).  This is the parity form of csrc/viterbi.hip -- a Python loop over the frames
    -- not a fast one: a 60 min track takes seconds."""
    table = _viterbi_table(table)
    return _viterbi_spans_host(probs, viterbi_settings([threshold], [penalty], table, unit), table)[0]


def _viterbi_keys(thresholds, penalties, table, unit=1024):
    return [(thr, pen) for thr in thresholds for pen in penalties], viterbi_settings(thresholds, penalties, table, unit)


def viterbi_instances(probs, thresholds=[0.5], min_lengths=[0.2], fps=100., penalties=[0.0], table=None):
    """{(threshold, penalty, min_length): [(start_s, end_s), ...]}, keys thresholds-major, then penalty, then min_length: the runs of
    the decoded path as (first / fps, last / fps), kept iff end - start > min_length.  Host form (see viterbi_frame_spans)."""
    thresholds, min_lengths, penalties = list(thresholds), list(min_lengths), list(penalties)
    table = _viterbi_table(table)
    keys, settings = _viterbi_keys(thresholds, penalties, table)
    return _instances_from_spans(keys, _viterbi_spans_host(probs, settings, table), min_lengths, np.float64(_check_fps(fps)))


def _device_viterbi_tables(probs, dtype, settings, table_host, table_dev=None, extra_bytes=0, want_best=False):
    """lad_viterbi_count + lad_viterbi_fill (include/lad_hip.h) on a (C, T) tensor that _device_track has passed, T >= 1, for at most
    lad_viterbi_max_settings() settings (bias, penalty): the sibling of _device_tables, with the same (workspace, table, counts)
    in front -- the counts at the start of the workspace, where the scorers read them, extra_bytes behind it for the caller -- and
    `best`, the int64 (C * K,) scores on the device (None unless asked for)."""
    import torch

    import _hip
    lib = _hip.lib()
    C, T = probs.shape
    K = len(settings)
    i32p = ctypes.POINTER(ctypes.c_int32)
    bias = (ctypes.c_int32 * K)(*[s[0] for s in settings])
    penalty = (ctypes.c_int32 * K)(*[s[1] for s in settings])
    ws_bytes = lib.lad_viterbi_workspace_bytes(C, T, K)
    _hip.check(0 if ws_bytes >= 0 else _hip.LAD_ERR_INVALID, "lad_viterbi_workspace_bytes")
    with torch.cuda.device(probs.device):
        stream = _hip.stream_handle(probs.device)
        if table_dev is None:
            table_dev = torch.from_numpy(table_host).to(probs.device)
        ws = torch.empty(ws_bytes + extra_bytes, dtype=torch.uint8, device=probs.device)
        best = torch.empty(C * K, dtype=torch.int64, device=probs.device) if want_best else None
        _hip.check(lib.lad_viterbi_count(_hip.ptr(probs), dtype, C, T, _hip.ptr(table_dev), table_host.ctypes.data_as(i32p), bias, penalty,
                                         K, _hip.ptr(ws), _hip.ptr(best), stream), "lad_viterbi_count")
        counts = np.ascontiguousarray(ws[:4 * C * K].view(torch.int32).cpu().numpy())     # (synchronises)
        total = int(counts.sum(dtype=np.int64))
        runs = torch.empty((max(total, 1), 2), dtype=torch.int32, device=probs.device)
        _hip.check(lib.lad_viterbi_fill(_hip.ptr(ws), counts.ctypes.data_as(i32p), C, T, K, _hip.ptr(runs), total, stream),
                   "lad_viterbi_fill")
        return ws, runs[:total], counts, best


def viterbi_frame_spans_device(probs, settings, table=None):
    """Device form of the decoder for a list of settings (bias, penalty) as viterbi_settings returns them.  probs: (T,) GPU tensor
    (float32 / float64, contiguous) -> [int64 (n, 2) array per setting]; (C, T) -> one such list per channel.  More settings than
    lad_viterbi_max_settings() go in several rounds.  No CPU fallback."""
    import torch

    import _hip
    probs, dtype, single = _device_track(probs, "decoder")
    table = _viterbi_table(table)
    settings = _check_viterbi_settings(settings)
    C, T = probs.shape
    if T == 0 or C == 0 or not settings:
        out = [[np.zeros((0, 2), np.int64) for _ in settings] for _ in range(C)]
    else:
        out = [[] for _ in range(C)]
        step = int(_hip.lib().lad_viterbi_max_settings())
        table_dev = torch.from_numpy(table).to(probs.device)
        for k0 in range(0, len(settings), step):
            _, runs, counts, _ = _device_viterbi_tables(probs, dtype, settings[k0:k0 + step], table, table_dev)
            part = _split_tables(counts.astype(np.int64).reshape(C, -1), runs.cpu().numpy())
            for c in range(C):
                out[c] += part[c]
    return out[0] if single else out


def viterbi_instances_device(probs, thresholds=[0.5], min_lengths=[0.2], fps=100., penalties=[0.0], table=None):
    """viterbi_instances for a (T,) track in GPU memory: the same dictionary (keys, order, Python floats)."""
    import _hip
    if getattr(probs, "ndim", None) != 1:
        raise _hip.LadHipError("probs must be a (T,) GPU tensor (the device decoder has no CPU fallback)")
    thresholds, min_lengths, penalties = list(thresholds), list(min_lengths), list(penalties)
    table = _viterbi_table(table)
    keys, settings = _viterbi_keys(thresholds, penalties, table)
    return _instances_from_spans(keys, viterbi_frame_spans_device(probs, settings, table), min_lengths, np.float64(_check_fps(fps)))
