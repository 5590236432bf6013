"""Zero-phase low-pass of probability tracks on the MI355X (csrc/lowpass.hip).

Reference seam: laugh_segmenter.py:49-55 (`lowpass(sig, filter_order=2, cutoff=0.01)`: scipy.signal.butter + filtfilt on the
host, called from :170 and :195 before the thresholds).  The convention here is scipy.signal.filtfilt with its defaults for the
second-order Butterworth filter: odd extension by 9 frames, forwards and backwards in direct form II transposed from
lfilter_zi's steady state, all in float64 (float32 arithmetic is 3e-5 to 9e-5 away from scipy at cutoff 0.01: DESIGN.md
section 5).

The filter is designed here in float64 from the closed form of the bilinear transform (no scipy); the kernel runs the
recurrence as a scan of affine maps.  There is no CPU fallback.
"""
import math

import numpy as np

PADLEN = 9     # scipy.signal.filtfilt's default: 3 * max(len(a), len(b))


def butter2(cutoff):
    """(b, a) of the second-order Butterworth low-pass with its -3 dB point at `cutoff` of Nyquist: scipy.signal.butter(2, cutoff,
    output='ba') from the closed form of the bilinear transform, K = tan(pi cutoff / 2)."""
    cutoff = float(cutoff)
    if not 0.0 < cutoff < 1.0:
        raise ValueError(f"Digital filter critical frequencies must be 0 < Wn < 1, got {cutoff}")
    K = math.tan(math.pi * cutoff / 2)
    n = 1.0 / (1.0 + math.sqrt(2.0) * K + K * K)
    b0 = K * K * n
    b = np.array([b0, 2.0 * b0, b0], dtype=np.float64)
    a = np.array([1.0, 2.0 * (K * K - 1.0) * n, (1.0 - math.sqrt(2.0) * K + K * K) * n], dtype=np.float64)
    return b, a


def zi2(b, a):
    """scipy.signal.lfilter_zi(b, a) for one biquad with a[0] == 1: the state of direct form II transposed in the steady state of
    a unit step, (I - A) zi = (b1 - a1 b0, b2 - a2 b0) with A = [[-a1, 1], [-a2, 0]].  The 2x2 system is solved as LAPACK's gesv does
    (partial pivoting, the multiplier formed with the pivot's reciprocal): near cutoff 0 it is ill-conditioned, and Cramer's rule
    is 2.5e-12 away from scipy at cutoff 0.001 where this is not one bit away."""
    b = np.asarray(b, dtype=np.float64)
    a = np.asarray(a, dtype=np.float64)
    if b.shape != (3,) or a.shape != (3,) or a[0] != 1.0:
        raise ValueError("zi2 takes one biquad: len(b) == len(a) == 3, a[0] == 1")
    rows = [(1.0 + float(a[1]), -1.0, float(b[1] - a[1] * b[0])), (float(a[2]), 1.0, float(b[2] - a[2] * b[0]))]
    if abs(rows[1][0]) > abs(rows[0][0]):
        rows.reverse()
    (p00, p01, c0), (p10, p11, c1) = rows
    mult = p10 * (1.0 / p00)
    z1 = (c1 - mult * c0) / (p11 - mult * p01)
    return np.array([(c0 - p01 * z1) / p00, z1], dtype=np.float64)


def filtfilt_device(probs, b, a, lengths=None, out=None):
    """scipy.signal.filtfilt(b, a, probs) with its defaults for one biquad, on the device.  probs: (T,) or (C, T) float32 / float64
    GPU tensor, contiguous -> float64 tensor of the same shape.  lengths: C ints, channel c is filtered over its first lengths[c]
    frames (its odd extension is taken at that end) and the rest of its row comes back as NaN.  out: a contiguous float64 GPU
    tensor of the same shape to write into."""
    import torch

    import _hip
    p2, dtype, single = _hip.device_track(probs, "low-pass")
    C, T = p2.shape
    lengths = _hip.channel_lengths(lengths, C)
    shortest = T if lengths is None or C == 0 else int(lengths.min())
    if shortest <= PADLEN:
        raise ValueError(f"The length of the input vector x must be greater than padlen, which is {PADLEN}.")
    out2 = _hip.out_track(out, p2, single, torch.float64)
    if C == 0:
        return out2[0] if single else out2
    bb = np.ascontiguousarray(b, dtype=np.float64)
    aa = np.ascontiguousarray(a, dtype=np.float64)
    zi = zi2(bb, aa)
    with torch.cuda.device(p2.device):
        ws = _hip.workspace("lad_lowpass_workspace_bytes", C, T, device=p2.device)
        _hip.launch("lad_lowpass", p2, dtype, C, T, lengths, bb, aa, zi, out2, ws)
    return out2[0] if single else out2


def lowpass_device(probs, cutoff=0.01, lengths=None):
    """Device form of laugh_segmenter.lowpass for a track that is already in GPU memory: the second-order Butterworth low-pass at
    `cutoff` of Nyquist, forwards and backwards.  probs: (T,) or (C, T) float32 / float64 GPU tensor -> float64 tensor of the same
    shape, within the rounding of float64 of scipy's result (tests/test_lowpass_gpu.py).  lengths: per-channel frame counts of a
    NaN-padded (C, T) tensor."""
    b, a = butter2(cutoff)
    return filtfilt_device(probs, b, a, lengths=lengths)
