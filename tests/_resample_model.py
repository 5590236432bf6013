"""The yardstick of tests/test_resample_cpu.py and tests/test_resample_gpu.py: the float64 restatement of the resampling
convention, written from the formula and sharing nothing with the product (resample.py, csrc/resample.hip):

    y[n] = sum_j x[j] * h[half + n * down - j * up],  j in [0, n_in) with the h index in [0, 2 * half],  n < ceil(n_in * up / down)

with h = scipy.signal.firwin(2 * half + 1, 1 / max(up, down), window=('kaiser', 5.0)) * up, half = 10 * max(up, down): what
scipy.signal.resample_poly(x, up, down) computes with its defaults.  Also the error bar of a float32 sum of K products of
float32-rounded taps and samples, per output:  |y_gpu[n] - y[n]| <= (K + 3) * 2^-24 * sum_j |x[j] * h[...]|."""
import math

import numpy as np
from scipy import signal

RATES = (8000, 11025, 22050, 32000, 44100, 48000, 96000)
PAIRS = tuple((r, 16000) for r in RATES) + tuple((16000, r) for r in RATES)


def ratio(sr_in, sr_out):
    g = math.gcd(sr_in, sr_out)
    return sr_out // g, sr_in // g


def scipy_filter(up, down):
    """(h float64, half) of scipy.signal.resample_poly's defaults."""
    half = 10 * max(up, down)
    return signal.firwin(2 * half + 1, 1.0 / max(up, down), window=("kaiser", 5.0)) * up, half


def out_len(n_in, up, down):
    return -(-n_in * up // down)


def noise(sr, seed=0, dtype=np.float32):
    """Seeded unit-scale noise of 0.3 s + 7 samples at `sr`."""
    return np.random.default_rng(1000 + seed + sr).standard_normal(int(0.3 * sr) + 7).astype(dtype)


def model(x, up, down, h, half, outputs=None):
    """(y float64, mag float64) for the outputs asked for (default: all): y[n] by the formula above, mag[n] = sum_j |x[j] * h[...]|.
    x: 1-D array, used in float64."""
    x = np.asarray(x, dtype=np.float64)
    n_in = x.shape[0]
    n = np.arange(out_len(n_in, up, down), dtype=np.int64) if outputs is None else np.asarray(outputs, dtype=np.int64)
    q = n * down
    j_lo = -((half - q) // up)                      # ceil((q - half) / up): the first j with h index <= 2 * half
    taps = (2 * half) // up + 1                     # no output has more j's in range than this
    y = np.zeros(n.shape[0], dtype=np.float64)
    mag = np.zeros(n.shape[0], dtype=np.float64)
    for k in range(taps):
        j = j_lo + k
        i = half + q - j * up
        ok = (i >= 0) & (i <= 2 * half) & (j >= 0) & (j < n_in)
        term = np.where(ok, x[np.clip(j, 0, max(n_in - 1, 0))] if n_in else 0.0, 0.0) * np.where(ok, h[np.clip(i, 0, 2 * half)], 0.0)
        y += term
        mag += np.abs(term)
    return y, mag


def bound(mag, K):
    """The error bar of the float32 kernel per output."""
    return (K + 3) * 2.0 ** -24 * mag


def taps_per_output(half, up):
    """K of the documented table layout (include/lad_hip.h)."""
    return 2 * (half // up) + 1 + (1 if half % up else 0)
