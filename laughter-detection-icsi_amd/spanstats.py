"""Confidence of an instance on the MI355X (csrc/spanstats.hip): the sum and the earliest peak of the track over every span.

Not in the reference, which returns bare (start, end).  The convention is written out above lad_span_stats in include/lad_hip.h:
the frame value of every decoder, 0.0 for a NaN frame; the sum of rint(w * 2^32) as an int64; the earliest frame at which w is
largest, and w there.  Integers and float64 compares only, so the device form equals the host form (laugh_segmenter.span_stats)
bit for bit; the mean and the peak's time are derived on the host (laugh_segmenter.confidences).  There is no CPU fallback.
"""

import numpy as np


def prepare_device(probs, dtype):
    """lad_span_stats_prepare on a (C, T) tensor that laugh_segmenter.device_track has passed, T >= 1: the workspace (a uint8 GPU
    tensor: prefix sums and the tree of maxima), written once per track, independent of any setting."""
    import torch

    import _hip
    C, T = probs.shape
    ws = _hip.workspace("lad_span_stats_workspace_bytes", C, T, device=probs.device)
    with torch.cuda.device(probs.device):
        _hip.launch("lad_span_stats_prepare", probs, dtype, C, T, ws)
    return ws


def stats_device(probs, dtype, ws, table, counts):
    """lad_span_stats on the tables of one round: table (total, 2) int32 on the device, counts int32 numpy (C * K,), the tables back
    to back in c * K + k order.  Returns (sums int64, peaks int32, peak_values float64), GPU tensors of `total` entries."""
    import torch

    import _hip
    C, T = probs.shape
    counts = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
    if counts.size == 0 or counts.size % C:
        raise ValueError(f"{counts.size} counts for {C} channels: one per (channel, setting)")
    _hip.require_cuda(table, "table", torch.int32)
    total = int(counts.sum(dtype=np.int64))
    if table.ndim != 2 or table.shape[1] != 2 or table.shape[0] < total or table.device != probs.device:
        raise ValueError(f"table must be ({total}, 2) int32 on the device of probs, got {tuple(table.shape)}")
    with torch.cuda.device(probs.device):
        # (one entry at least: the library takes no null pointer, and a tensor without elements may have one)
        sums = torch.empty(max(total, 1), dtype=torch.int64, device=probs.device)
        peaks = torch.empty(max(total, 1), dtype=torch.int32, device=probs.device)
        values = torch.empty(max(total, 1), dtype=torch.float64, device=probs.device)
        _hip.launch("lad_span_stats", probs, dtype, C, T, ws, table, counts, counts.size // C, sums, peaks, values)
    return sums[:total], peaks[:total], values[:total]


def to_host(sums, peaks, values):
    """The three arrays of stats_device on the host, as laugh_segmenter.span_stats returns them: int64, int64, float64."""
    return sums.cpu().numpy(), peaks.cpu().numpy().astype(np.int64), values.cpu().numpy()


def span_stats_device(probs, table, counts):
    """laugh_segmenter.span_stats for a (T,) or (C, T) float32 / float64 GPU tensor and span tables that lie on the device: table
    (total, 2) int32, the tables of every (channel, setting) back to back in c * K + k order, counts their row counts (C * K
    ints on the host) -- what laugh_segmenter._device_tables returns.  -> (sums int64 (total,), peaks int64 (total,), peak_values
    float64 (total,)), numpy, one entry per row; only these cross to the host."""
    import laugh_segmenter
    probs, dtype, _ = laugh_segmenter.device_track(probs, "span statistics")
    C, T = probs.shape
    counts = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
    if C == 0 or T == 0:
        if counts.sum(dtype=np.int64) != 0:
            raise ValueError("an empty track has no spans")
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float64)
    return to_host(*stats_device(probs, dtype, prepare_device(probs, dtype), table, counts))
