"""Second implementation of the augmentation convention, in numpy: written from the text next to `lad_gather_segments_aug` in
include/lad_hip.h, not from the kernel.  Philox in Python integers; the stages in float64 except where the text fixes fp32
(`unit`, `frac`, and the fp32 struct fields the gates and ranges are read from)."""
import numpy as np

M32 = 0xFFFFFFFF
f32 = np.float32


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11): counter = 4 words, key = 2 words -> 4 words."""
    c0, c1, c2, c3 = (int(v) & M32 for v in counter)
    k0, k1 = (int(v) & M32 for v in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def mulhi(u, n):
    return (int(u) * int(n)) >> 32


def unit(u):
    return f32(int(u) >> 8) * f32(2.0 ** -24)   # exact in fp32


def block(cfg, epoch, chan, first, k):
    return philox4x32_10((int(first) & M32, int(chan), int(epoch), k), (cfg.seed & M32, cfg.seed >> 32))


def draws(cfg, epoch, chan, first, T, F, n_noise=0, noise_frames=None, noise_list=None):
    """Everything a segment draws, as a dict (cfg: any object with the AugmentConfig fields)."""
    r = block(cfg, epoch, chan, first, 0)
    d = {"spec": bool(unit(r[0]) < f32(cfg.p)), "mix_gate": bool(unit(r[1]) < f32(cfg.mix_p))}
    d["snr_db"] = float(f32(cfg.snr_lo)) + (float(f32(cfg.snr_hi)) - float(f32(cfg.snr_lo))) * float(unit(r[2]))
    d["gain_db"] = float(f32(cfg.gain_lo)) + (float(f32(cfg.gain_hi)) - float(f32(cfg.gain_lo))) * float(unit(r[3]))
    r = block(cfg, epoch, chan, first, 1)
    if n_noise:
        d["noise_slot"] = mulhi(r[0], n_noise)
        if noise_list is not None:
            d["noise_chan"] = int(noise_list[d["noise_slot"]])
            d["noise_first"] = mulhi(r[1], int(noise_frames[d["noise_chan"]]) - T + 1)
    W = cfg.W
    if W > 0:
        d["c"] = W + mulhi(r[2], T - 2 * W)
        d["w"] = mulhi(r[3], 2 * W - 1) - (W - 1)
        d["c2"] = d["c"] + d["w"]
    d["time"], d["freq"] = [], []
    for m in range(max(cfg.n_time, cfg.n_freq)):
        r = block(cfg, epoch, chan, first, 2 + m)
        if m < cfg.n_time:
            width = mulhi(r[0], cfg.Wt + 1)
            d["time"].append((mulhi(r[1], T - width + 1), width))
        if m < cfg.n_freq:
            width = mulhi(r[2], cfg.Wf + 1)
            d["freq"].append((mulhi(r[3], F - width + 1), width))
    return d


def gather(mats, chan, first, count, T, pad):
    """Stage 1 for one segment: float32 (T, F), rows past `count` or outside the channel are `pad`."""
    m = mats[chan]
    out = np.full((T, m.shape[1]), f32(pad), f32)
    for t in range(min(int(count), T)):
        st = int(first) + t
        if 0 <= st < m.shape[0]:
            out[t] = m[st]
    return out


def warp_rows(T, c, c2):
    """Per output row: (i0, i1, rem, den) of stage 3."""
    rows = []
    for t in range(T):
        if t < c2:
            num, den, base = t * c, c2, 0
        else:
            num, den, base = (t - c2) * (T - c), T - c2, c
        q, rem = divmod(num, den)
        i0 = base + q
        rows.append((i0, min(i0 + 1, T - 1), rem, den))
    return rows


def augment_segment(cfg, epoch, mats, chan, first, count, T, pad, noise_list=None):
    """One segment through all four stages -> dict with the float64 result and what the tests need to know about the way there:
    x (T, F) float64; filled (T, F) bool: the mask entries; warp: the (i0, i1, rem, den) rows of stage 3 or None; mixed: whether
    stage 2 ran; mean: the fill value (float64) or None; before_masks: the float64 values after stage 3; gathered: stage 1 (float32)."""
    g = gather(mats, chan, first, count, T, pad)
    F = g.shape[1]
    n_noise = len(noise_list) if noise_list is not None else 0
    frames = [m.shape[0] for m in mats]
    d = draws(cfg, epoch, chan, first, T, F, n_noise, frames, noise_list)
    x = g.astype(np.float64)
    mix = d["mix_gate"] and n_noise > 0
    gain_on = not (cfg.gain_lo == 0 and cfg.gain_hi == 0)
    mixed = mix or gain_on
    if mixed:
        G = 10.0 ** (d["gain_db"] / 10.0)
        y = G * np.exp(x)
        if mix:
            b = mats[d["noise_chan"]][d["noise_first"]:d["noise_first"] + T].astype(np.float64)
            assert b.shape == (T, F)
            k = G * np.exp(x).sum() / (10.0 ** (d["snr_db"] / 10.0) * np.exp(b).sum())
            y = y + k * np.exp(b)
        x = np.log(np.maximum(1e-10, y))
    rows = None
    if d["spec"] and cfg.W > 0:
        rows = warp_rows(T, d["c"], d["c2"])
        src = x
        x = np.empty_like(src)
        for t, (i0, i1, rem, den) in enumerate(rows):
            if rem == 0:
                x[t] = src[i0]
            else:
                frac = float(f32(rem) / f32(den))
                x[t] = src[i0] + frac * (src[i1] - src[i0])
    filled = np.zeros((T, F), bool)
    mean, before = None, x
    if d["spec"]:
        mean = float(x.mean())
        for start, width in d["time"]:
            filled[start:start + width, :] = True
        for start, width in d["freq"]:
            filled[:, start:start + width] = True
        x = np.where(filled, mean, x)
    return {"x": x, "before_masks": before, "filled": filled, "warp": rows, "mixed": mixed, "mean": mean, "draws": d, "gathered": g}
