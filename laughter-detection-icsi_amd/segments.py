"""Segment index: the table that says which frames of which channel form a training example, and its label.

Reference: compute_features.py:114-195 (`compute_features_for_cuts`: one cut per data-frame row =
`track.truncate(offset=sub_start, duration=sub_duration).pad(duration=1.0)` + supervision `is_laugh = label`, then
`CutSet.shuffle()`), compute_features.py:197-261 (`compute_features_for_single_audio_track`: consecutive 1 s windows,
last partial window dropped), analysis/utils.py:8-15 (`to_frames`: round(t * 1000 / frame_duration)).
Row schema (create_data_df.py:171-172, data/icsi/data_dfs/samples/*.csv):
    start, duration, sub_start, sub_duration, audio_path, meeting_id, chan_id, label

Everything here is integer bookkeeping on the host (bit-exact by construction, tests/test_host_logic.py, tests/test_properties.py); the frames
themselves are gathered on the GPU (csrc/gather.hip).
"""
import csv
from dataclasses import dataclass, field

import numpy as np

FRAME_SHIFT = 0.01        # the frame shift at the default FEAT['num_samples'] = 100 (configured_frame_shift() reads the configured one)
MIN_SEG_DURATION = 1.0


def configured_frame_shift():
    """Frame shift of the configured features, 1 / FEAT['num_samples'] (utils/utils.py:15 of the reference), read at call time:
    0.01 at the default 100 frames per second, 1/128 s at the reference's original 128."""
    import config
    return 1.0 / config.FEAT['num_samples']


def frames_per_segment():
    """Frames of one MIN_SEG_DURATION segment at the configured frame shift (100, or 128 at FEAT['num_samples'] = 128)."""
    return int(round(MIN_SEG_DURATION / configured_frame_shift()))


def seconds_to_frame(t, frame_shift=None):
    """Frame index of a time stamp: round-half-even of t / frame_shift on the 2-decimal values of the data frames
    (create_data_df.py:182 rounds every time to 2 decimals, so t / 0.01 is an integer up to float noise).  frame_shift None: the
    configured one (configured_frame_shift()).  At other frame shifts (1/128 s) the same rule applies; Lhotse's own time -> frame rounding of
    such cuts is a restatement like the rest of this module, parity unpinned."""
    if frame_shift is None:
        frame_shift = configured_frame_shift()
    return int(round(round(float(t), 2) / frame_shift))


@dataclass
class SegmentTable:
    channel: np.ndarray      # int32 (N,)  index into `channels`
    first_frame: np.ndarray  # int64 (N,)
    n_frames: np.ndarray     # int32 (N,)  <= frames_per_segment; the rest is padding
    label: np.ndarray        # int32 (N,)
    channels: list           # channel keys, e.g. "Bmr021/chan3.sph"
    frames_per_segment: int = field(default_factory=frames_per_segment)
    # a table whose windows are redrawn (sampling.py, datasets.LadDataset(redraw=)): the region each row's window is drawn in and the
    # row's place in the table before any permutation or sharding (None: its place in this table).  None: a table as it always was.
    region_first: np.ndarray = None   # int64 (N,)
    region_frames: np.ndarray = None  # int64 (N,)
    row_id: np.ndarray = None         # int64 (N,)

    def __len__(self):
        return len(self.label)

    def _take(self, sel):
        """The rows `sel` (a permutation or a slice); the optional arrays come along, row_id keeps each row's original place."""
        extra = {}
        if self.region_first is not None or self.row_id is not None:
            ids = self.row_id if self.row_id is not None else np.arange(len(self), dtype=np.int64)
            extra = dict(region_first=None if self.region_first is None else self.region_first[sel],
                         region_frames=None if self.region_frames is None else self.region_frames[sel], row_id=ids[sel])
        return SegmentTable(self.channel[sel], self.first_frame[sel], self.n_frames[sel], self.label[sel], self.channels,
                            self.frames_per_segment, **extra)

    def shuffled(self, seed=None):
        rng = np.random.default_rng(seed)
        perm = rng.permutation(len(self))
        return self._take(perm)

    def shard(self, rank, world):
        per = (len(self) + world - 1) // world
        sl = slice(min(len(self), rank * per), min(len(self), (rank + 1) * per))
        return self._take(sl)


def table_from_rows(rows, min_seg_duration=MIN_SEG_DURATION, frame_shift=None, keep_regions=False):
    """rows: iterable of dicts with the data-frame columns -> SegmentTable (one segment per row, row order kept).
    frame_shift None: 1 / FEAT['num_samples'] (configured_frame_shift()).
    keep_regions: also read the `start` / `duration` columns (create_data_df.py:104-105: the region the stored window was sampled
    in) into region_first / region_frames, by the same seconds_to_frame, widened where needed to contain the row's own window."""
    if frame_shift is None:
        frame_shift = configured_frame_shift()
    fps = int(round(min_seg_duration / frame_shift))
    chans, chan_idx = [], {}
    channel, first, count, label = [], [], [], []
    region_first, region_frames = [], []
    for r in rows:
        key = r["audio_path"]
        if key not in chan_idx:
            chan_idx[key] = len(chans)
            chans.append(key)
        sub_start, sub_dur = float(r["sub_start"]), float(r["sub_duration"])
        if sub_start < 0 or sub_dur < 0:
            raise ValueError(f"negative time in segment row {r}")  # create_data_df.py:185-186 asserts the same
        lab = int(r["label"])
        if lab not in (0, 1):
            raise ValueError(f"label must be 0 or 1, got {lab}")   # create_data_df.py:189-190
        channel.append(chan_idx[key])
        first.append(seconds_to_frame(sub_start, frame_shift))
        count.append(min(fps, seconds_to_frame(sub_dur, frame_shift)))
        label.append(lab)
        if keep_regions:
            start, dur = float(r["start"]), float(r["duration"])
            if start < 0 or dur < 0:
                raise ValueError(f"negative time in segment row {r}")
            lo = min(seconds_to_frame(start, frame_shift), first[-1])
            hi = max(seconds_to_frame(start, frame_shift) + seconds_to_frame(dur, frame_shift), first[-1] + count[-1])
            region_first.append(lo)
            region_frames.append(hi - lo)
    extra = {}
    if keep_regions:
        extra = dict(region_first=np.asarray(region_first, np.int64), region_frames=np.asarray(region_frames, np.int64),
                     row_id=np.arange(len(label), dtype=np.int64))
    return SegmentTable(np.asarray(channel, np.int32), np.asarray(first, np.int64), np.asarray(count, np.int32),
                        np.asarray(label, np.int32), chans, fps, **extra)


def table_from_csv(path, **kw):
    with open(path, newline="") as f:
        return table_from_rows(list(csv.DictReader(f)), **kw)


def whole_track_table(n_frames_total, channel_key, laugh_intervals_ms=(), min_seg_duration=MIN_SEG_DURATION,
                      frame_shift=None, index=None, device=None):
    """Consecutive windows over one channel (compute_features.py:228-243): window w = [w, w+1) s; the last partial
    window is dropped; label 1 iff the open-closed interval (start_ms, end_ms] overlaps a laugh interval of the
    channel's participant.  laugh_intervals_ms: iterable of (lo_ms, hi_ms] integer pairs (the `portion` index of
    analysis/preprocess.py, in 1 ms frames).
    index: a sweep_eval.TranscriptIndex -- the laugh intervals are those of its channel (meeting_id, chan) = channel_key, or of the
    key "<meeting_id>/<chan>.sph".  device: the labels are computed there (sampling.window_coverage: lad_window_coverage, no host
    loop; one-second windows only); the default, None, is the host loop below and its output is what it always was."""
    if frame_shift is None:
        frame_shift = configured_frame_shift()
    fps = int(round(min_seg_duration / frame_shift))
    n_win = n_frames_total // fps
    first = np.arange(n_win, dtype=np.int64) * fps
    label = np.zeros(n_win, np.int32)
    if index is not None:
        mc = tuple(channel_key) if not isinstance(channel_key, str) else (channel_key.split("/", 1)[0],
                                                                         channel_key.split("/", 1)[1].rsplit(".", 1)[0])
        sets = index.intervals(*mc)
        laugh_intervals_ms = [] if sets is None else [(int(a), int(b)) for a, b in sets["laugh"]]
        if not isinstance(channel_key, str):
            channel_key = f"{mc[0]}/{mc[1]}.sph"
    if device is not None:
        import torch

        import sampling
        import sweep_eval
        if min_seg_duration != 1.0:
            raise ValueError("the device route labels one-second windows (their millisecond hulls are the windows' own bounds)")
        cover = sampling.window_coverage([[sweep_eval.normalise(list(laugh_intervals_ms))]], [channel_key],
                                         torch.zeros(n_win, dtype=torch.int32, device=device), torch.from_numpy(first).to(device),
                                         torch.full((n_win,), fps, dtype=torch.int32, device=device), fps)
        label = (cover[:, 0] > 0).to(torch.int32).cpu().numpy()
        return SegmentTable(np.zeros(n_win, np.int32), first, np.full(n_win, fps, np.int32), label, [channel_key], fps)
    for w in range(n_win):
        lo, hi = int(round(w * min_seg_duration * 1000)), int(round((w + 1) * min_seg_duration * 1000))
        for a, b in laugh_intervals_ms:  # (lo, hi] overlaps (a, b]  <=>  max(lo, a) < min(hi, b)
            if max(lo, a) < min(hi, b):
                label[w] = 1
                break
    return SegmentTable(np.zeros(n_win, np.int32), first, np.full(n_win, fps, np.int32), label, [channel_key], fps)
