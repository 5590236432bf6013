"""Median and rank filtering of probability tracks on the MI355X (csrc/rankfilt.hip).

Not in the reference, whose only smoother is `lowpass` (laugh_segmenter.py:49-55); this one stands at the same place, in front of
the thresholds.  The convention is written out above lad_rank_filter in include/lad_hip.h: a window of `window` frames (odd) around
every frame with the track's ends replicated (scipy.ndimage's mode='nearest'), sorted, its element `rank` taken.  The median is
rank = (window - 1) / 2, the minimum rank 0, the maximum rank window - 1.  The result is one of the track's own values, so the
device form equals the host form (laugh_segmenter.rank_filter) bit for bit.  There is no CPU fallback.
"""

MAX_WINDOW = 1023      # lad_rank_filter_max_window()


def check_window(window, rank=None):
    """(window, rank) as ints; ValueError for what lad_rank_filter refuses: a window that is even or outside 1..1023, a rank outside
    0..window - 1 (rank=None: the median's)."""
    if isinstance(window, bool) or int(window) != window:
        raise ValueError(f"window must be an odd integer from 1 to {MAX_WINDOW}, got {window!r}")
    window = int(window)
    if not 1 <= window <= MAX_WINDOW or window % 2 == 0:
        raise ValueError(f"window must be an odd integer from 1 to {MAX_WINDOW}, got {window}")
    if rank is None:
        return window, (window - 1) // 2
    if isinstance(rank, bool) or int(rank) != rank or not 0 <= int(rank) < window:
        raise ValueError(f"rank must be an integer from 0 to window - 1 = {window - 1}, got {rank!r}")
    return window, int(rank)


def rank_filter_device(probs, window, rank, lengths=None, out=None):
    """Element `rank` of the sorted window of `window` frames around every frame, the ends replicated, on the device.  probs: (T,) or
    (C, T) float32 / float64 GPU tensor, contiguous -> a tensor of the same shape and dtype.  lengths: C ints, channel c is filtered
    over its first lengths[c] frames (its end is replicated there) and the rest of its row comes back as NaN.  out: a contiguous GPU
    tensor of the same shape and dtype to write into."""
    import torch

    import _hip
    p2, dtype, single = _hip.device_track(probs, "rank filter")
    window, rank = check_window(window, rank)
    C, T = p2.shape
    lengths = _hip.channel_lengths(lengths, C)
    if lengths is not None and C and T and (lengths.min() < 1 or lengths.max() > T):
        raise ValueError(f"every length lies in 1..{T}, got {int(lengths.min())}..{int(lengths.max())}")
    out2 = _hip.out_track(out, p2, single, p2.dtype)
    if C == 0 or T == 0:
        return out2[0] if single else out2
    with torch.cuda.device(p2.device):
        ws = _hip.workspace("lad_rank_filter_workspace_bytes", C, T, window, device=p2.device)
        _hip.launch("lad_rank_filter", p2, dtype, C, T, lengths, window, rank, out2, ws)
    return out2[0] if single else out2


def median_filter_device(probs, window, lengths=None, out=None):
    """Device form of laugh_segmenter.median_filter for a track that is already in GPU memory: rank_filter_device at the median's
    rank, (window - 1) / 2."""
    return rank_filter_device(probs, window, check_window(window)[1], lengths=lengths, out=out)
