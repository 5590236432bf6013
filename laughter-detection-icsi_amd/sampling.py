"""The segment sampler: from the transcript tables to a training table, and a fresh table every epoch.

Reference: create_data_df.py:32-63 (get_random_non_laughter_segment), :65-81 (get_random_segment_from_df), :84-95 (get_subsample),
:98-206 (create_data_df: per laugh row so many negatives and so many windows of the row, negatives first; the schema and the
asserts), compute_features.py:228-243 (the label rule of whole-track windows).  The reference samples once, on the host, when it
writes {split}_df.csv ("Later either the sampled values can be used or resampling can happen", :104-105); here the table is
redrawn on the device before every epoch (csrc/sample.hip), one launch for the whole table.

    SegmentPools       regions and pools of one corpus in frames, built once on the host from the tables TranscriptIndex takes
    Plan               the row descriptors (kind, src, label) of a table: SegmentPools.plan(preset, meetings)
    DrawTable          the device arrays lad_sample_segments reads + .draw(seed, epoch)
    Sampler            pools + plan + seed: .draw(epoch) device arrays, .rows(epoch) the eight reference columns
    window_coverage    milliseconds of each transcript class under a list of windows (lad_window_coverage)

The convention (frames and milliseconds, regions, pools, kinds, the Philox counter) is written out in include/lad_hip.h next to
lad_sample_segments.  The host side here is integer bookkeeping; every draw happens on the device.  No CPU fallback.
"""
import math
from dataclasses import dataclass

import numpy as np

import sweep_eval

FIXED, POOL_ROW, POOL_MEASURE = 0, 1, 2                    # include/lad_hip.h: enum lad_sample_kind
COLUMNS = ["start", "duration", "sub_start", "sub_duration", "audio_path", "meeting_id", "chan_id", "label"]   # create_data_df.py:171-172
FLOAT_DECIMALS = 2                                          # config.py:60 of the reference, create_data_df.py:182


def channel_key(meeting_id, chan):
    """create_data_df.py:161-162"""
    return f"{meeting_id}/{chan}.sph"


def frames_of(lo_ms, hi_ms, fps, frames_c):
    """The frames [a, b) of the millisecond interval (lo, hi] on a channel of frames_c rows (b <= a: none)."""
    lo_ms, hi_ms, fps = int(lo_ms), int(hi_ms), int(fps)
    return -((-lo_ms * fps) // 1000), min(hi_ms * fps // 1000, int(frames_c))


@dataclass
class Plan:
    kind: np.ndarray       # int32 (N,)
    src: np.ndarray        # int32 (N,)  a region (FIXED) or a pool
    label: np.ndarray      # int32 (N,)
    meeting: list          # meeting id per row

    def __len__(self):
        return len(self.kind)


class SegmentPools:
    """Regions (chan, lo, hi) in frames and pools of them: per meeting a POOL_ROW pool of the speech rows and one of the noise
    rows, a POOL_MEASURE pool `silence` and one `any` (the channels minus laugh and invalid), and one FIXED region per laugh row."""

    def __init__(self, channels, frames, fps, T, regions, pool_off, pool_names, laugh_rows, dropped):
        self.channels, self.frames, self.fps, self.T = list(channels), np.asarray(frames, np.int64), int(fps), int(T)
        self.regions = np.ascontiguousarray(regions, dtype=np.int32).reshape(-1, 3)
        self.pool_off = np.ascontiguousarray(pool_off, dtype=np.int32)
        self.pool_names = list(pool_names)                  # [(meeting, class)] per pool
        self.pool_index = {k: p for p, k in enumerate(self.pool_names)}
        self.laugh_rows = list(laugh_rows)                  # [(meeting, region index)] in table order
        self.dropped = int(dropped)
        self.meetings = sorted({m for m, _ in self.pool_names})
        # pool_cum / pool_total: windows of T frames inside the regions (regions shorter than T count none; measure pools hold none)
        width = np.maximum(self.regions[:, 2].astype(np.int64) - self.regions[:, 1] - self.T + 1, 0)
        self.pool_cum = np.zeros(len(self.regions), np.int64)
        self.pool_total = np.zeros(len(self.pool_names), np.int64)
        for p in range(len(self.pool_names)):
            o0, o1 = int(self.pool_off[p]), int(self.pool_off[p + 1])
            self.pool_cum[o0:o1] = np.cumsum(width[o0:o1]) - width[o0:o1]
            self.pool_total[p] = int(width[o0:o1].sum())

    @classmethod
    def from_transcripts(cls, rows, channels, fps, T, frames=None, noise_pool="noise"):
        if noise_pool not in ("noise", "speech"):
            raise ValueError(f"noise_pool must be 'noise' or 'speech', got {noise_pool!r}")
        fps, T = int(fps), int(T)
        if fps < 1 or T < 1:
            raise ValueError(f"fps and T must be positive, got {fps}, {T}")
        index = sweep_eval.TranscriptIndex(rows, channels)
        recs = sweep_eval._records(rows, sweep_eval.ROW_COLUMNS)
        chans = sweep_eval._records(channels, sweep_eval.CHANNEL_COLUMNS)
        keys, nframes, by_part, by_chan = [], [], {}, {}
        for c in chans:
            if c["part_id"] in (None, ""):
                continue                                     # (no participant: no transcript, nothing to draw from)
            key = channel_key(c["meeting_id"], c["chan"])
            n = int(frames[key]) if frames is not None else int(math.floor(float(c["length"]) * fps))
            by_part[(c["meeting_id"], c["part_id"])] = by_chan[(c["meeting_id"], c["chan"])] = len(keys)
            keys.append(key)
            nframes.append(n)
        regions, pool_off, names = [], [0], []

        def row_region(r):
            ci = by_part.get((r["meeting_id"], r["part_id"]))
            if ci is None:
                return None
            a, b = frames_of(sweep_eval.to_frames(float(r["start"])), sweep_eval.to_frames(float(r["end"])), fps, nframes[ci])
            return (ci, a, b) if b > a and a >= 0 else None

        meetings = index.meetings
        for m in meetings:
            mrows = [r for r in recs if r["meeting_id"] == m]
            for name, kind in (("speech", "speech"), ("noise", noise_pool)):
                regions += [g for g in (row_region(r) for r in mrows if r["type"] == kind) if g is not None]
                pool_off.append(len(regions))
                names.append((m, name))
            mchans = [(mc, by_chan[mc]) for mc in index.channels(m) if mc in by_chan]
            for name in ("silence", "any"):
                for mc, ci in mchans:
                    sets = index.intervals(*mc)
                    if name == "silence":
                        iv = sets["silence"]
                    else:
                        full = sweep_eval.normalise([(0, int(sweep_eval.to_frames(index._length[(m, index.participant(*mc))])))])
                        iv = sweep_eval.subtract(sweep_eval.subtract(full, sets["laugh"]), sets["invalid"])
                    for lo, hi in iv:
                        a, b = frames_of(lo, hi, fps, nframes[ci])
                        if b - a >= T:
                            regions.append((ci, a, b))
                pool_off.append(len(regions))
                names.append((m, name))
        laugh_rows, dropped = [], 0
        for r in recs:
            if r["type"] != "laugh":
                continue
            g = row_region(r)
            if g is None:
                dropped += 1
                continue
            laugh_rows.append((r["meeting_id"], len(regions)))
            regions.append(g)
        if len(regions) >= 2 ** 30:
            raise ValueError("more than 2^30 regions")
        return cls(keys, nframes, fps, T, np.asarray(regions, np.int64).reshape(-1, 3), pool_off, names, laugh_rows, dropped)

    def pool(self, meeting_id, name):
        """(index, regions int32 (n, 3), total measure) of one pool."""
        p = self.pool_index[(meeting_id, name)]
        return p, self.regions[self.pool_off[p]:self.pool_off[p + 1]], int(self.pool_total[p])

    def plan(self, preset, meetings):
        """Row descriptors for the listed meetings, laugh row by laugh row (create_data_df.py:133-168): per laugh row the negatives
        (speech, noise, silence -- or `any` with random=True), then its windows; all negatives first, then all positives
        (:177-180).  preset: a name in config.SAMPLING or such a dictionary."""
        if isinstance(preset, str):
            import config
            preset = config.SAMPLING[preset]
        if float(preset.get("subsample_duration", 1.0)) * self.fps != self.T:
            raise ValueError(f"the preset's subsample_duration {preset.get('subsample_duration')} s is not the pools' T = {self.T} frames "
                             f"at {self.fps} fps")
        n_pos, n_non = int(preset["num_laugh_samples"]), int(preset["num_non_laugh_samples"])
        if preset.get("random", False):
            per = [("any", POOL_MEASURE, n_non)]
        else:
            n_sil = math.floor(n_non * preset.get("silence_share", 0.7))          # create_data_df.py:124-126
            n_noise = math.floor(n_non * preset.get("noise_share", 0.1))
            per = [("speech", POOL_ROW, n_non - n_sil - n_noise), ("noise", POOL_ROW, n_noise), ("silence", POOL_MEASURE, n_sil)]
        neg, pos = [], []
        for m in meetings:
            mine = [j for mm, j in self.laugh_rows if mm == m]
            if not mine:
                continue
            for name, kind, n in per:
                if n == 0:
                    continue
                if (m, name) not in self.pool_index:
                    raise ValueError(f"meeting {m} has no {name} pool (it is not in the transcript tables)")
                p, reg, total = self.pool(m, name)
                if len(reg) == 0 or (kind == POOL_MEASURE and total == 0):
                    raise ValueError(f"meeting {m} has an empty {name} pool: the preset asks for {n} {name} rows per laugh row")
                if total >= 2 ** 32:
                    raise ValueError(f"the {name} pool of meeting {m} holds {total} windows: the draw holds 2^32 - 1")
            for j in mine:
                for name, kind, n in per:
                    neg += [(kind, self.pool_index[(m, name)], 0, m)] * n
                pos += [(FIXED, j, 1, m)] * n_pos
        rows = neg + pos
        return Plan(np.asarray([r[0] for r in rows], np.int32), np.asarray([r[1] for r in rows], np.int32),
                    np.asarray([r[2] for r in rows], np.int32), [r[3] for r in rows])


class DrawTable:
    """What lad_sample_segments reads, on the device, with the host copies its entry point checks.  The arrays are checked here
    once (ValueError, before anything is uploaded), so a draw hands the library only the small pool tables to check."""

    def __init__(self, kind, src, regions, pool_off, pool_cum, pool_total, T, row_id=None, device="cuda"):
        import torch
        self.kind = np.ascontiguousarray(kind, dtype=np.int32)
        self.src = np.ascontiguousarray(src, dtype=np.int32)
        self.regions = np.ascontiguousarray(regions, dtype=np.int32).reshape(-1, 3)
        self.pool_off = np.ascontiguousarray(pool_off, dtype=np.int32)
        self.pool_cum = np.ascontiguousarray(pool_cum, dtype=np.int64)
        self.pool_total = np.ascontiguousarray(pool_total, dtype=np.int64)
        self.row_id = None if row_id is None else np.ascontiguousarray(row_id, dtype=np.int64)
        self.T = int(T)
        self.validate()
        self.device = torch.device(device)
        up = lambda a: torch.from_numpy(a if a.size else np.zeros(1, a.dtype)).to(self.device)   # noqa: E731  (never a null pointer)
        self.d_kind, self.d_src, self.d_regions = up(self.kind), up(self.src), up(self.regions.reshape(-1))
        self.d_pool_off, self.d_pool_cum = up(self.pool_off), up(self.pool_cum)
        self.d_row_id = None if self.row_id is None else up(self.row_id)

    def __len__(self):
        return len(self.kind)

    def validate(self):
        n_regions, n_pools = len(self.regions), len(self.pool_off) - 1
        if self.T < 1:
            raise ValueError(f"T = {self.T} frames per segment, at least 1")
        if len(self.src) != len(self.kind) or (self.row_id is not None and len(self.row_id) != len(self.kind)):
            raise ValueError("kind, src and row_id differ in length")
        if n_pools < 0 or self.pool_off[0] != 0 or np.any(np.diff(self.pool_off) < 0) or self.pool_off[-1] > n_regions:
            raise ValueError("pool offsets must ascend from 0 and stay within the regions")
        if len(self.pool_cum) != n_regions or len(self.pool_total) != n_pools:
            raise ValueError("pool_cum has one entry per region, pool_total one per pool")
        if np.any(self.pool_total < 0) or np.any(self.pool_total >= 2 ** 32):
            raise ValueError("a pool's measure must lie in 0 .. 2^32 - 1")
        if n_regions and np.any(self.regions[:, 2] <= self.regions[:, 1]):
            raise ValueError("a region must hold at least one frame (hi > lo)")
        k, s = self.kind, self.src.astype(np.int64)
        if np.any((k < FIXED) | (k > POOL_MEASURE)):
            raise ValueError("row kinds are 0 (FIXED), 1 (POOL_ROW) or 2 (POOL_MEASURE)")
        if np.any((s < 0) | (s >= np.where(k == FIXED, n_regions, n_pools))):
            raise ValueError("a row's src lies outside the regions (FIXED) or the pools")
        sp = s[k != FIXED]
        if np.any(self.pool_off[sp + 1] == self.pool_off[sp]):
            raise ValueError("a row draws from an empty pool")
        if np.any(self.pool_total[s[k == POOL_MEASURE]] < 1):
            raise ValueError("a POOL_MEASURE row draws from a pool of measure 0")

    def draw(self, seed, epoch, out=None, region=False):
        """One launch: (chan int32, first int64, count int32[, region int32]) device tensors of len(self) rows.  out: the first
        three, written in place.  No synchronisation, no host copy."""
        import torch

        import _hip
        n = len(self)
        if out is None:
            out = (torch.empty(n, dtype=torch.int32, device=self.device), torch.empty(n, dtype=torch.int64, device=self.device),
                   torch.empty(n, dtype=torch.int32, device=self.device))
        chan, first, count = out
        for t, dt, name in ((chan, torch.int32, "chan"), (first, torch.int64, "first"), (count, torch.int32, "count")):
            _hip.require_cuda(t, name, dt)
            if t.numel() != n:
                raise ValueError(f"{name} holds {t.numel()} rows, the table {n}")
        reg = torch.empty(n, dtype=torch.int32, device=self.device) if region else None
        if not 0 <= int(seed) < 2 ** 64 or not 0 <= int(epoch) < 2 ** 32:
            raise ValueError("seed is 64 bits, epoch 32 bits, neither negative")
        with torch.cuda.device(self.device):
            _hip.launch("lad_sample_segments", self.d_kind, self.d_src, n, self.d_row_id, self.d_regions, len(self.regions), self.d_pool_off,
                        self.d_pool_cum, len(self.pool_off) - 1, None, None, self.pool_off, self.pool_total, self.T, int(seed), int(epoch),
                        chan, first, count, reg)
        return (chan, first, count, reg) if region else (chan, first, count)


class Sampler:
    """A table that is redrawn: pools + plan + seed.  take(idx) reorders / selects rows and keeps each row's row_id, so a row's
    window stays a function of (seed, epoch, its place in the plan)."""

    def __init__(self, pools, plan, seed, device="cuda", row_id=None):
        self.pools, self.plan, self.seed, self.device = pools, plan, int(seed), device
        self.row_id = None if row_id is None else np.asarray(row_id, np.int64)
        self._tables, self._label = {}, None

    def __len__(self):
        return len(self.plan)

    def take(self, idx):
        idx = np.asarray(idx)
        ids = (np.arange(len(self), dtype=np.int64) if self.row_id is None else self.row_id)[idx]
        plan = Plan(self.plan.kind[idx], self.plan.src[idx], self.plan.label[idx], [self.plan.meeting[i] for i in idx])
        return Sampler(self.pools, plan, self.seed, self.device, ids)

    def draw_table(self, chan_map=None, device=None):
        """The DrawTable of this sampler; chan_map: int array, pools channel index -> the caller's (a FeatureStore's)."""
        device = self.device if device is None else device
        key = (None if chan_map is None else tuple(int(c) for c in chan_map), str(device))
        if key not in self._tables:
            regions = self.pools.regions.copy()
            if chan_map is not None and len(regions):
                regions[:, 0] = np.asarray(chan_map, np.int32)[regions[:, 0]]
            self._tables[key] = DrawTable(self.plan.kind, self.plan.src, regions, self.pools.pool_off, self.pools.pool_cum,
                                          self.pools.pool_total, self.pools.T, self.row_id, device)
        return self._tables[key]

    def draw(self, epoch, out=None):
        """(chan, first, count, label) device tensors; chan indexes pools.channels."""
        import torch
        t = self.draw_table()
        chan, first, count = t.draw(self.seed, epoch, out=out)
        if self._label is None:
            self._label = torch.from_numpy(self.plan.label).to(t.device)
        return chan, first, count, self._label

    def table(self, epoch=0):
        """The draw of one epoch as a segments.SegmentTable (one device -> host copy)."""
        import segments
        chan, first, count, _ = self.draw(epoch)
        ids = np.arange(len(self), dtype=np.int64) if self.row_id is None else self.row_id
        return segments.SegmentTable(chan.cpu().numpy(), first.cpu().numpy(), count.cpu().numpy(), self.plan.label.copy(),
                                     list(self.pools.channels), self.pools.T, row_id=ids.copy())

    def rows(self, epoch):
        """The eight reference columns (create_data_df.py:171-172), times rounded to 2 decimals (:182).  A FIXED or POOL_ROW row's
        (start, duration) is the region it was drawn in, a POOL_MEASURE row's is its window (:47-49, :63)."""
        chan, first, count, reg = (t.cpu().numpy() for t in self.draw_table().draw(self.seed, epoch, region=True))
        fps = float(self.pools.fps)
        out = []
        for i in range(len(self)):
            lo, hi = (int(first[i]), int(first[i]) + int(count[i])) if self.plan.kind[i] == POOL_MEASURE else \
                (int(v) for v in self.pools.regions[reg[i], 1:])
            key = self.pools.channels[chan[i]]
            out.append([round(lo / fps, FLOAT_DECIMALS), round((hi - lo) / fps, FLOAT_DECIMALS), round(int(first[i]) / fps, FLOAT_DECIMALS),
                        round(int(count[i]) / fps, FLOAT_DECIMALS), key, self.plan.meeting[i], key.split("/", 1)[1][:-len(".sph")],
                        int(self.plan.label[i])])
        return out


def window_coverage(index_or_sets, channels, chan, first, count, fps):
    """int32 (n, S) device tensor: the milliseconds of set s of channel chan[i] inside the hull of window i (lad_window_coverage).
    index_or_sets: a sweep_eval.TranscriptIndex -- the S = 5 sets of TranscriptIndex.intervals in sweep_eval.CLASSES order for
    every (meeting_id, chan) of `channels` -- or, per channel, a list of S normalised (n, 2) interval arrays.  chan (int32, into
    `channels`), first (int64), count (int32): GPU tensors, as lad_gather_segments takes them."""
    import torch

    import _hip
    _hip.require_cuda(chan, "chan", torch.int32)
    _hip.require_cuda(first, "first", torch.int64)
    _hip.require_cuda(count, "count", torch.int32)
    channels = list(channels)
    if hasattr(index_or_sets, "intervals"):
        per = []
        for mc in channels:
            sets = index_or_sets.intervals(*mc)
            per.append([sets[k] if sets is not None else sweep_eval._EMPTY for k in sweep_eval.CLASSES])
    else:
        per = [[np.asarray(s, np.int64).reshape(-1, 2) for s in sets] for sets in index_or_sets]
    if len(per) != len(channels) or not per or len({len(p) for p in per}) != 1 or not per[0]:
        raise ValueError("one list of S >= 1 interval sets per channel, the same S for every channel")
    S = len(per[0])
    parts = [s for p in per for s in p]
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    bounds = np.concatenate(parts) if offsets[-1] else sweep_eval._EMPTY
    if offsets[-1] >= 2 ** 30 or (len(bounds) and (bounds.max() >= 2 ** 31 or bounds.min() < 0)):
        raise ValueError("the sets hold more than 2^30 intervals or a millisecond value outside int32")
    n = int(chan.numel())
    if first.numel() != n or count.numel() != n:
        raise ValueError("chan, first and count differ in length")
    dix = sweep_eval.DeviceIndex(channels, bounds, offsets, chan.device)
    out = torch.empty((n, S), dtype=torch.int32, device=chan.device)
    with torch.cuda.device(chan.device):
        _hip.launch("lad_window_coverage", chan, first, count, n, int(fps), dix.bounds, dix.offsets, dix.bounds_host, dix.offsets_host,
                    dix.n_intervals, len(channels), S, out)
    return out
