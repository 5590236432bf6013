"""Sampling-rate conversion on the MI355X (csrc/resample.hip): audio of any common rate to the 16 kHz the path runs at, and
16 kHz (or a file's own rate) to the 44.1 kHz of the reference's wav cuts.

Reference seam: segment_laughter.py:134 (`librosa.load(audio_path, sr=44100)`) and laugh_segmenter.py:157-185
(`librosa.load(sr=8000)`): both resample on the host.  The convention here is scipy.signal.resample_poly with its defaults
(librosa's default is a different filter: same instants, same length, another low-pass):

    up / down = sr_out / sr_in reduced;  half = zeros * max(up, down);  h = firwin(2 * half + 1, 1 / max(up, down),
    window=('kaiser', beta)) * up;  y[n] = sum_j x[j] * h[half + n * down - j * up],  n < ceil(n_in * up / down)

The filter is designed here in float64 (numpy only); the kernel sums float32 products of the float32-rounded taps.  There is no
CPU fallback: a ratio beyond the kernel's limits raises ValueError.
"""
import math

import numpy as np
import torch

import _hip

LAD_RESAMPLE_F32, LAD_RESAMPLE_I16 = 0, 1     # enum lad_resample_dtype (include/lad_hip.h)


def ratio(sr_in, sr_out):
    """(up, down) with up / down = sr_out / sr_in in lowest terms."""
    sr_in, sr_out = int(sr_in), int(sr_out)
    if sr_in < 1 or sr_out < 1:
        raise ValueError(f"sampling rates must be positive, got {sr_in} -> {sr_out}")
    g = math.gcd(sr_in, sr_out)
    return sr_out // g, sr_in // g


def design_lowpass(up, down, zeros=10, beta=5.0):
    """(h float64 of 2 * half + 1 taps, half): Kaiser-windowed sinc with cutoff 1 / max(up, down) of Nyquist, unit sum, times up
    (scipy.signal.resample_poly's default filter for zeros=10, beta=5.0; more zeros / a larger beta give a steeper filter)."""
    m = max(int(up), int(down))
    half = int(zeros) * m
    k = np.arange(-half, half + 1, dtype=np.float64)
    h = np.sinc(k / m) / m * np.kaiser(2 * half + 1, float(beta))
    h /= h.sum()
    return h * up, half


def polyphase_table(h, half, up, down=None):
    """(float32 table (up, K), K) in the layout of include/lad_hip.h: table[p][t] = h[half + p - (t - L) * up] where that index
    exists, 0 elsewhere, L = half // up, K = 2 * L + 1 + (half % up != 0).  `down` plays no part in the layout."""
    h = np.asarray(h, dtype=np.float64)
    assert h.shape == (2 * half + 1,)
    L = half // up
    K = 2 * L + 1 + (1 if half % up else 0)
    idx = half + np.arange(up)[:, None] - (np.arange(K)[None, :] - L) * up
    ok = (idx >= 0) & (idx <= 2 * half)
    table = np.where(ok, h[np.clip(idx, 0, 2 * half)], 0.0).astype(np.float32)
    return np.ascontiguousarray(table), K


def out_len(n_in, up, down):
    """ceil(n_in * up / down) (lad_resample_out_len: host only)."""
    n = _hip.lib().lad_resample_out_len(int(n_in), int(up), int(down))
    if n < 0:
        raise ValueError(_hip.lib().lad_last_error().decode("utf-8", "replace"))
    return n


def limits():
    """The kernel's limits as a dictionary (host only)."""
    l = _hip.lib()
    return {"max_up": l.lad_resample_max_up(), "max_down": l.lad_resample_max_down(), "max_taps": l.lad_resample_max_taps(),
            "max_lds_bytes": l.lad_resample_max_lds_bytes(), "tile_outputs": l.lad_resample_tile_outputs()}


def _limits_text(lim):
    return (f"up <= {lim['max_up']}, down <= {lim['max_down']}, taps per output <= {lim['max_taps']}, table + tile span <= "
            f"{lim['max_lds_bytes']} bytes of LDS")


class Resampler:
    """sr_in -> sr_out for 1-D GPU tensors of float32 or int16 PCM; the polyphase table is built once and kept on `device`."""

    def __init__(self, sr_in, sr_out, device="cuda", zeros=10, beta=5.0):
        self.sr_in, self.sr_out = int(sr_in), int(sr_out)
        self.up, self.down = ratio(sr_in, sr_out)
        self.device = torch.device(device)
        self.identity = self.up == 1 and self.down == 1
        self.K, self.table = 0, None
        if self.identity:
            return
        lim = limits()
        if self.up > lim["max_up"] or self.down > lim["max_down"]:
            raise ValueError(f"{self.sr_in} -> {self.sr_out} Hz is {self.up}/{self.down}: beyond the resampling kernel's limits ("
                             f"{_limits_text(lim)})")
        h, half = design_lowpass(self.up, self.down, zeros=zeros, beta=beta)
        table, self.K = polyphase_table(h, half, self.up, self.down)
        need = _hip.lib().lad_resample_lds_bytes(self.up, self.down, self.K) if self.K <= lim["max_taps"] else -1
        if need < 0 or need > lim["max_lds_bytes"]:
            raise ValueError(f"{self.sr_in} -> {self.sr_out} Hz is {self.up}/{self.down} with {self.K} taps per output"
                             f"{'' if need < 0 else f' and {need} bytes of LDS'}: beyond the resampling kernel's limits ("
                             f"{_limits_text(lim)})")
        self.table = torch.from_numpy(table).to(self.device)

    def out_len(self, n_in):
        return int(n_in) if self.identity else out_len(n_in, self.up, self.down)

    def __call__(self, pcm, start=None, stop=None):
        """Outputs [start, stop) (default: all of them) of the converted signal as a float32 GPU tensor."""
        _hip.require_cuda(pcm, "pcm")
        if pcm.dim() != 1 or pcm.dtype not in (torch.float32, torch.int16):
            raise _hip.LadHipError(f"pcm must be a 1-D float32 or int16 tensor, got {tuple(pcm.shape)} {pcm.dtype}")
        total = self.out_len(pcm.numel())
        a = 0 if start is None else int(start)
        b = total if stop is None else int(stop)
        if not 0 <= a <= b <= total:
            raise ValueError(f"outputs [{a}, {b}) outside the {total} the signal has at {self.sr_out} Hz")
        if self.identity:
            x = pcm if pcm.dtype == torch.float32 else pcm.to(torch.float32) / 32768.0
            return x[a:b]
        if pcm.device != self.table.device:
            raise _hip.LadHipError(f"pcm is on {pcm.device}, the resampler's table on {self.table.device}")
        y = torch.empty(b - a, dtype=torch.float32, device=pcm.device)
        dtype = LAD_RESAMPLE_I16 if pcm.dtype == torch.int16 else LAD_RESAMPLE_F32
        with torch.cuda.device(pcm.device):
            _hip.launch("lad_resample", pcm, dtype, pcm.numel(), self.table, self.up, self.down, self.K, a, b - a, y)
        return y


_CACHE = {}
_CACHE_SIZE = 8


def get_resampler(sr_in, sr_out, device="cuda"):
    """A cached Resampler for (sr_in, sr_out, device) (the few most recent ones are kept)."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (int(sr_in), int(sr_out), str(device))
    r = _CACHE.pop(key, None)
    if r is None:
        r = Resampler(sr_in, sr_out, device)
        while len(_CACHE) >= _CACHE_SIZE:
            _CACHE.pop(next(iter(_CACHE)))
    _CACHE[key] = r
    return r


def resample(pcm, sr_in, sr_out):
    """pcm (1-D GPU tensor, float32 or int16) at sr_in -> float32 at sr_out."""
    return get_resampler(sr_in, sr_out, pcm.device)(pcm)
