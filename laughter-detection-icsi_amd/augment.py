"""Train-time augmentation of a batch on the GPU: SpecAugment and a noise mix inside the gather launch (csrc/augment.hip).

Neither the reference nor Lhotse's PrecomputedFeatures path behind its LadDataset (datasets.py:49-68) augments a training batch;
the model here is what Lhotse does to precomputed features elsewhere -- `SpecAugment` (time warp, frame masks, feature masks, mean
fill) and the feature-domain mixer behind `MixedCut`, log(exp(a) + gain * exp(b)) with the gain taken from an SNR over summed
energies.  Parity with Lhotse is [UPSTREAM-UNVERIFIED]: the convention is written out next to `lad_gather_segments_aug` in
include/lad_hip.h, and that text is the specification.

This module is host-side only: the configuration, its validation and the named presets (config.AUGMENT).  A segment's augmentation
is a pure function of (seed, epoch, channel, first frame), so data-parallel ranks only have to agree on the seed.
"""
import dataclasses
import operator

import _hip

MAX_MASKS = 16               # of each kind (csrc/augment.hip)
MAX_LDS_BYTES = 160 * 1024   # a segment and its noise excerpt are staged in one CU's LDS
SCRATCH_BYTES = 304          # draws, mask tables and reduction slots in front of them


def _in_unit(x):
    return 0.0 <= x <= 1.0   # (False for NaN)


@dataclasses.dataclass(frozen=True)
class AugmentConfig:
    """The fields of `lad_augment_params` but the epoch, which the dataset supplies.  Validates on construction (ValueError)."""
    seed: int = 0
    p: float = 0.0            # SpecAugment gate: warp and masks apply to a segment with this probability
    mix_p: float = 0.0        # a segment is mixed with an excerpt of a noise channel with this probability
    snr_lo: float = 0.0       # dB, signal over noise, both summed over the segment
    snr_hi: float = 0.0
    gain_lo: float = 0.0      # dB; (0, 0) = no gain stage
    gain_hi: float = 0.0
    W: int = 0                # time warp: the centre frame moves by less than W frames (0: no warp)
    n_time: int = 0           # time masks: how many, each 0..Wt frames wide
    Wt: int = 0
    n_freq: int = 0           # feature masks: how many, each 0..Wf filters wide
    Wf: int = 0

    def __post_init__(self):
        for name in ("seed", "W", "n_time", "Wt", "n_freq", "Wf"):
            try:
                object.__setattr__(self, name, operator.index(getattr(self, name)))   # (numpy integers too)
            except TypeError:
                raise ValueError(f"{name} must be an integer, got {getattr(self, name)!r}") from None
        if not 0 <= self.seed < 2 ** 64:
            raise ValueError(f"augmentation seed must lie in [0, 2^64), got {self.seed}")
        if not (_in_unit(self.p) and _in_unit(self.mix_p)):
            raise ValueError(f"probabilities must lie in [0, 1] (p = {self.p}, mix_p = {self.mix_p})")
        if not (self.snr_lo <= self.snr_hi and self.gain_lo <= self.gain_hi):
            raise ValueError(f"a range needs lo <= hi (snr {self.snr_lo}..{self.snr_hi} dB, gain {self.gain_lo}..{self.gain_hi} dB)")
        for name in ("W", "n_time", "Wt", "n_freq", "Wf"):
            if getattr(self, name) < 0:
                raise ValueError(f"{name} must not be negative, got {getattr(self, name)}")
        if self.n_time > MAX_MASKS or self.n_freq > MAX_MASKS:
            raise ValueError(f"at most {MAX_MASKS} masks of each kind (got {self.n_time} time, {self.n_freq} feature)")

    @property
    def mixes(self):
        return self.mix_p > 0.0

    def validate_for(self, n_frames, num_filters, noise_frames=None):
        """What depends on the batch geometry, refused before any launch: noise_frames = frame counts of the noise channels."""
        T, F = int(n_frames), int(num_filters)
        if F < 4 or F % 4 != 0:
            raise ValueError(f"the number of filters must be a multiple of 4, got {F}")
        if T <= 2 * self.W:
            raise ValueError(f"the time warp needs n_frames > 2 W (n_frames = {T}, W = {self.W})")
        if self.Wt > T or self.Wf > F:
            raise ValueError(f"mask widths must fit the segment (Wt = {self.Wt} of {T} frames, Wf = {self.Wf} of {F} filters)")
        if SCRATCH_BYTES + 2 * T * F * 4 > MAX_LDS_BYTES:
            raise ValueError(f"a {T} x {F} segment and its noise excerpt need {SCRATCH_BYTES + 2 * T * F * 4} bytes of LDS, a CU has "
                             f"{MAX_LDS_BYTES}")
        if self.mixes and (noise_frames is None or len(noise_frames) == 0):
            raise ValueError("mix_p > 0 needs noise channels (noise='self', audio paths or a directory)")
        if noise_frames is not None and len(noise_frames) and min(int(n) for n in noise_frames) < T:
            raise ValueError(f"every noise channel needs at least n_frames = {T} frames (shortest: {min(int(n) for n in noise_frames)})")

    def params(self, epoch):
        """The C struct for one launch."""
        epoch = int(epoch)
        if not 0 <= epoch < 2 ** 32:
            raise ValueError(f"epoch must lie in [0, 2^32), got {epoch}")
        return _hip.AugmentParams(seed=self.seed, epoch=epoch, p=self.p, mix_p=self.mix_p, snr_lo=self.snr_lo, snr_hi=self.snr_hi,
                                  gain_lo=self.gain_lo, gain_hi=self.gain_hi, W=self.W, n_time=self.n_time, Wt=self.Wt,
                                  n_freq=self.n_freq, Wf=self.Wf)


def from_preset(name, seed=0):
    """AugmentConfig of a named preset of config.AUGMENT; 'none' / None -> None."""
    if name is None or name == "none":
        return None
    import config
    if name not in config.AUGMENT:
        raise ValueError(f"unknown augmentation preset {name!r}: one of none, {', '.join(config.AUGMENT)}")
    return AugmentConfig(seed=int(seed), **config.AUGMENT[name])
