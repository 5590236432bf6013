"""Shared helpers of the low-pass tests (no GPU): scipy's result, a numpy float64 model of the kernel's blocked scan, the error bar
and the plateau track of the decision tests."""
import numpy as np

PAD = 9
WAVE = 64


def reference(x, cutoff):
    """The reference's exact calls (laugh_segmenter.py:49-55)."""
    from scipy import signal
    return signal.filtfilt(*signal.butter(2, cutoff, output='ba'), x)


def tol(x, a):
    """64 ulps of max(1, max|x|), amplified by 1 / (1 - r)^2 with r the pole radius: a rounding error of one ulp in a carried state
    decays like r^n (n + 1) at worst through the double pole pair, which sums to at most about 1 / (1 - r)^2; 64 ulps are allowed
    for FMA contraction and a different association in the scan.  2.1e3 at cutoff 0.01, 2.0e5 at 0.001."""
    r = np.sqrt(a[2])
    return 64 * 2.0 ** -52 * max(1.0, float(np.max(np.abs(x)))) / (1 - r) ** 2


def make_track(seed, n):
    rng = np.random.default_rng(seed)
    out = np.empty(0)
    while out.size < n:
        out = np.concatenate([out, np.full(int(rng.integers(20, 400)), rng.uniform(-0.3, 1.3))])
    return out[:n] + 0.05 * rng.standard_normal(n)


def odd_ext(x):
    x = np.asarray(x, dtype=np.float64)
    return np.concatenate([2 * x[0] - x[PAD:0:-1], x, 2 * x[-1] - x[-2:-PAD - 2:-1]])


def _powers(a, first, count):
    """A^(2^k) for k = first .. first + count - 1, A = [[-a1, 1], [-a2, 0]], by multiplying with A one frame at a time as the
    kernel's host side does (repeated squaring loses digits to cancellation: 9e-10 from scipy at cutoff 0.001 instead of 2e-11);
    a power whose entries have all decayed below 1e-40 is taken as zero."""
    a1, a2 = float(a[1]), float(a[2])
    m, n, out = (1.0, 0.0, 0.0, 1.0), 0, []
    for k in range(first, first + count):
        while n < 1 << k:
            m = (-a1 * m[0] + m[2], -a1 * m[1] + m[3], -a2 * m[0], -a2 * m[1])
            n += 1
            if max(abs(v) for v in m) < 1e-40:
                m, n = (0.0, 0.0, 0.0, 0.0), 1 << k
        out.append(np.array(m).reshape(2, 2))
    return out


def _run(seg, b, a, z):
    """seg (..., L), z (..., 2) -> y (..., L), end state: direct form II transposed along the last axis."""
    z0, z1 = z[..., 0].copy(), z[..., 1].copy()
    y = np.empty_like(seg)
    for j in range(seg.shape[-1]):
        x = seg[..., j]
        y[..., j] = b[0] * x + z0
        z0 = b[1] * x + z1 - a[1] * y[..., j]
        z1 = b[2] * x - a[2] * y[..., j]
    return y, np.stack([z0, z1], axis=-1)


def _scan(s, pw):
    """Inclusive Hillis-Steele scan over axis -2 (64 spans) of the constants s (..., 64, 2) with pw[j] = A^(span 2^j)."""
    s = s.copy()
    for j, m in enumerate(pw):
        d = 1 << j
        s[..., d:, :] = s[..., :-d, :] @ m.T + s[..., d:, :]
    return s


def _pass(seq, b, a, zi, L):
    """One direction of the blocked algorithm over `seq` from the state zi * seq[0]."""
    assert L & (L - 1) == 0, "the model's squaring ladder needs a power of two"
    lg = L.bit_length() - 1
    seg_pw, tile_pw = _powers(a, lg, 6), _powers(a, lg + 6, 6)
    tile = WAVE * L
    n_tiles = -(-seq.size // tile)
    x = np.zeros(n_tiles * tile)
    x[:seq.size] = seq
    x = x.reshape(n_tiles, WAVE, L)
    # local: every lane from zero state, composed over the wave
    _, end = _run(x, b, a, np.zeros((n_tiles, WAVE, 2)))
    const = _scan(end, seg_pw)[:, -1, :]
    # carry: tile to tile
    start = np.empty((n_tiles, 2))
    s = zi * seq[0]
    for t in range(n_tiles):
        start[t] = s
        s = tile_pw[0] @ s + const[t]
    # apply: lane 0 from the true state, the scan gives the others theirs
    z = np.zeros((n_tiles, WAVE, 2))
    z[:, 0, :] = start
    _, end = _run(x, b, a, z)
    incl = _scan(end, seg_pw)
    z[:, 1:, :] = incl[:, :-1, :]
    y, _ = _run(x, b, a, z)
    return y.reshape(-1)[:seq.size]


def blocked(x, b, a, L):
    """numpy float64 model of csrc/lowpass.hip: filtfilt of one biquad as a scan of affine maps, a lane running L frames."""
    import lowpass
    zi = lowpass.zi2(b, a)
    ext = odd_ext(x)
    fwd = _pass(ext, b, a, zi, L)
    back = _pass(fwd[::-1].copy(), b, a, zi, L)
    return back[::-1][PAD:-PAD].copy()


def gpu_lengths(L):
    return [T for T in (10, 11, 19, L - 18, L - 17, L - 9, L, L + 1, 2 * L - 18, 2 * L + 5, 64 * L - 18, 64 * L - 17, 64 * L + 3,
                        130 * L + 7) if T > PAD]


SWEEP_THRESHOLDS = np.concatenate((np.linspace(0, .9, 19).round(2), np.linspace(.91, 1, 10).round(2)))
SWEEP_MIN_LENGTHS = [0, 0.1, 0.2]
