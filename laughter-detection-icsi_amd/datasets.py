"""Drop-in for the reference's datasets.py on HBM-resident features.

Reference: datasets.py:23-68 `LadDataset` (item = {'inputs': (B,T,F) f32, 'input_lens': (B,), 'is_laugh': (B,) int32,
'cut': cuts}; built on Lhotse's PrecomputedFeatures: per-cut lilcom read + decompress + pad + stack on the host),
datasets.py:72-93 `InferenceDataset` (item i = feats[i:i+100], zero right-pad at the end of the file).

Here whole-channel feature matrices stay resident in HBM (`FeatureStore`: one hour of audio is 63 MB, the whole ICSI
corpus ~28 GB of the 288 GB) and a batch is one gather launch (csrc/gather.hip) driven by the integer segment table
(segments.py).  There is no lilcom stage: parity is defined against the raw extractor output.
"""
import ctypes

import numpy as np
import torch

import _hip
import config as cfg

# value Lhotse pads short cuts with in the log-mel domain (log(1e-10)); [UPSTREAM-UNVERIFIED], SURVEY.md section 5
LOG_EPSILON = -23.025850929940457


class FeatureStore:
    """Whole-channel (T, F) float32 feature matrices on the GPU + the device-side tables the gather kernel reads."""

    def __init__(self, extractor=None, device="cuda"):
        self.extractor = extractor
        self.device = torch.device(device)
        self.keys, self.mats = [], []
        self._tables = None

    def add_features(self, key, feats):
        f = torch.as_tensor(feats, dtype=torch.float32).to(self.device).contiguous()
        if f.dim() != 2 or f.shape[1] % 4 != 0:
            raise ValueError("features must be (T, F) with F a multiple of 4")
        self.keys.append(key)
        self.mats.append(f)
        self._tables = None
        return len(self.keys) - 1

    def add_audio(self, key, pcm):
        """Featurise one whole channel on the GPU (compute_features.py:66-111, one launch per channel)."""
        if self.extractor is None:
            raise ValueError("FeatureStore needs an extractor to add audio")
        x = torch.as_tensor(np.asarray(pcm) if not isinstance(pcm, torch.Tensor) else pcm).to(self.device, torch.float32)
        return self.add_features(key, self.extractor.extract_long(x.contiguous().view(-1)))

    def index_of(self, key):
        return self.keys.index(key)

    def tables(self):
        if self._tables is None:
            ptrs = torch.tensor([m.data_ptr() for m in self.mats], dtype=torch.int64, device=self.device)
            frames = torch.tensor([m.shape[0] for m in self.mats], dtype=torch.int64, device=self.device)
            self._tables = (ptrs, frames)
        return self._tables

    @property
    def num_filters(self):
        return self.mats[0].shape[1]


def gather_segments(store, chan, first, count, n_frames, pad, out=None):
    """(B, n_frames, F) batch: segment b = frames [first[b], first[b]+count[b]) of channel chan[b], padded with `pad`."""
    ptrs, frames = store.tables()
    n = int(chan.shape[0])
    F = store.num_filters
    if out is None:
        out = torch.empty((n, n_frames, F), device=store.device, dtype=torch.float32)
    _hip.launch("lad_gather_segments", ptrs, frames, chan, first, count, n, n_frames, F, float(pad), out, device=store.device)
    return out


class NoiseChannels:
    """The channels of a store that segments may be mixed with (augment.AugmentConfig.mix_p): their indices on the device for the
    kernel, their frame counts on the host for the validation.  channels: store indices or keys."""

    def __init__(self, store, channels):
        idx = [store.index_of(c) if isinstance(c, str) else int(c) for c in channels]
        if any(not 0 <= i < len(store.mats) for i in idx):
            raise ValueError(f"noise channel index outside the store's {len(store.mats)} channels")
        self.store = store
        self.index = torch.tensor(idx, dtype=torch.int32, device=store.device)
        self.frames = [int(store.mats[i].shape[0]) for i in idx]

    def __len__(self):
        return len(self.frames)


def gather_segments_augmented(store, chan, first, count, n_frames, pad, cfg, epoch, noise, out=None, check_first=True):
    """gather_segments with train-time augmentation in the same launch (csrc/augment.hip; the convention: include/lad_hip.h).
    cfg: augment.AugmentConfig; epoch: part of the random counter, so an epoch's batches differ from the last one's; noise: a
    NoiseChannels, a list of store indices / keys, or None (no mixing).  Refusals are ValueErrors raised before the launch.
    check_first: read first.min() / .max() back to check 0 <= first < 2^32 (the counter holds 32 bits of it) -- a device
    synchronisation; LadDataset checks its table once instead."""
    if noise is not None and not isinstance(noise, NoiseChannels):
        noise = NoiseChannels(store, noise)
    if noise is not None and len(noise) == 0:
        noise = None
    F = store.num_filters
    cfg.validate_for(n_frames, F, noise.frames if noise is not None else None)
    params = cfg.params(epoch)
    n = int(chan.shape[0])
    if check_first and n and not (int(first.min()) >= 0 and int(first.max()) < 2 ** 32):
        raise ValueError("augmented segments need 0 <= first frame < 2^32")
    ptrs, frames = store.tables()
    if out is None:
        out = torch.empty((n, n_frames, F), device=store.device, dtype=torch.float32)
    _hip.launch("lad_gather_segments_aug", ptrs, frames, chan, first, count, n, n_frames, F, float(pad), ctypes.byref(params),
                noise.index if noise is not None else None, len(noise) if noise is not None else 0,
                min(noise.frames) if noise is not None else 0, out, device=store.device)
    return out


class LadDataset(torch.utils.data.Dataset):
    """Laugh-activity-detection dataset: indexing with a batch of segment ids returns the reference's batch dict.

    augment: an augment.AugmentConfig -- the batches are augmented in the gather launch, differently in every epoch
    (`set_epoch`); None: the plain gather.  noise: what mixing draws from -- 'self' (the channels this table names that hold at
    least a segment's frames: other speech, no extra data, and never a channel that only another split sharing the store uses), a
    list of store keys / indices, or a NoiseChannels.
    redraw: the windows are drawn afresh by `set_epoch` (csrc/sample.hip; the convention: include/lad_hip.h next to
    lad_sample_segments) -- 'window': every row inside its own region (a table with region_first / region_frames:
    segments.table_from_rows(keep_regions=True)); a sampling.Sampler of len(table) rows whose pools name the table's channels: every
    row by its kind.  One launch per epoch into the arrays the gather reads, no synchronisation, no host copy.  Until the first
    `set_epoch` the table's own windows stand.  redraw_seed: the seed of a 'window' redraw (a Sampler
    brings its own).  None (the default): the table as it is, and nothing here runs."""

    def __init__(self, store, table, pad_value=LOG_EPSILON, augment=None, noise=None, redraw=None, redraw_seed=0):
        super().__init__()
        self.store, self.table, self.pad_value = store, table, pad_value
        self.redraw, self._draw_table, self._draw_seed = redraw, None, int(redraw_seed)
        self.augment, self.noise, self.epoch = augment, None, 0
        if augment is not None:
            T = table.frames_per_segment
            if isinstance(noise, str):
                if noise != 'self':
                    raise ValueError(f"noise must be 'self', a list of channels or a NoiseChannels, got {noise!r}")
                noise = [i for i in sorted({store.index_of(k) for k in table.channels}) if store.mats[i].shape[0] >= T]
            if noise is not None and not isinstance(noise, NoiseChannels):
                noise = NoiseChannels(store, noise)
            self.noise = noise if noise is not None and len(noise) else None
            augment.validate_for(T, store.num_filters, self.noise.frames if self.noise is not None else None)
            if len(table) and not (int(table.first_frame.min()) >= 0 and int(table.first_frame.max()) < 2 ** 32):
                raise ValueError("augmented segments need 0 <= first frame < 2^32")
        remap = np.asarray([store.index_of(k) for k in table.channels], np.int32)
        dev = store.device
        if redraw is not None:
            # (with augmentation as well: every first frame a draw can give lies below its region's upper end, and _make_draw_table
            # keeps those within int32 -- the check on 0 <= first < 2^32 is made there, once, not per epoch)
            self._draw_table, self._draw_seed = self._make_draw_table(redraw, remap)
        self._chan = torch.from_numpy(remap[table.channel]).to(dev)
        self._first = torch.from_numpy(table.first_frame).to(dev)
        self._count = torch.from_numpy(table.n_frames).to(dev)
        self._label = torch.from_numpy(table.label).to(dev)

    def __len__(self):
        return len(self.table)

    def _make_draw_table(self, redraw, remap):
        """(sampling.DrawTable with channels as the store counts them, seed)."""
        import sampling
        table, store = self.table, self.store
        frames = np.asarray([m.shape[0] for m in store.mats], np.int64)
        if isinstance(redraw, str):
            if redraw != 'window':
                raise ValueError(f"redraw must be None, 'window' or a sampling.Sampler, got {redraw!r}")
            if table.region_first is None or table.region_frames is None:
                raise ValueError("redraw='window' needs a table with regions (segments.table_from_rows(..., keep_regions=True))")
            chan = remap[table.channel]
            lo = np.minimum(table.region_first, table.first_frame)
            own_end = table.first_frame + table.n_frames
            hi = np.maximum(np.minimum(table.region_first + table.region_frames, frames[chan]), own_end)
            if len(table) and (int(lo.min()) < 0 or int(hi.max()) >= 2 ** 31 or np.any(hi <= lo)):
                raise ValueError("redraw='window': a region is empty or lies outside 0 .. 2^31 - 1 frames")
            n = len(table)
            return sampling.DrawTable(np.zeros(n, np.int32), np.arange(n, dtype=np.int32), np.stack([chan, lo, hi], axis=1),
                                      np.zeros(1, np.int32), np.zeros(n, np.int64), np.zeros(0, np.int64), table.frames_per_segment,
                                      table.row_id, store.device), self._draw_seed
        if len(redraw) != len(table) or list(redraw.pools.channels) != list(table.channels) or redraw.pools.T != table.frames_per_segment:
            raise ValueError("the Sampler and the table differ in rows, channels or frames per segment (table = sampler.table())")
        if len(redraw.pools.regions) and np.any(redraw.pools.regions[:, 2] > frames[remap[redraw.pools.regions[:, 0]]]):
            raise ValueError("a region of the Sampler's pools ends past its channel's features in the store")
        return redraw.draw_table(remap, store.device), redraw.seed

    def set_epoch(self, epoch):
        """The epoch number of the batches to come: part of the augmentation's random counter, and with `redraw` the table's windows
        are drawn for it now."""
        self.epoch = int(epoch)
        if self._draw_table is not None:
            self._draw_table.draw(self._draw_seed, self.epoch, out=(self._chan, self._first, self._count))

    def __getitem__(self, cuts):
        idx = torch.as_tensor(cuts, dtype=torch.int64, device=self.store.device).view(-1)
        chan, first, count = self._chan[idx].contiguous(), self._first[idx].contiguous(), self._count[idx].contiguous()
        if self.augment is None:
            inputs = gather_segments(self.store, chan, first, count, self.table.frames_per_segment, self.pad_value)
        else:
            inputs = gather_segments_augmented(self.store, chan, first, count, self.table.frames_per_segment, self.pad_value,
                                               self.augment, self.epoch, self.noise, check_first=False)
        return {"inputs": inputs, "input_lens": count, "is_laugh": self._label[idx].contiguous(), "cut": cuts}


class InferenceDataset(torch.utils.data.Dataset):
    """Stride-one-frame windows over the features of a whole file (datasets.py:72-93)."""

    def __init__(self, feats, n_frames=None) -> None:
        super().__init__()
        self.feats = feats
        # (read when the dataset is made, not when this module is imported: a caller may set FEAT['num_samples'] = 128 first)
        self.n_frames = cfg.FEAT['num_samples'] if n_frames is None else n_frames

    def __len__(self):
        return len(self.feats)

    def __getitem__(self, index):
        ret = self.feats[index:index + self.n_frames]
        if ret.shape[0] != self.n_frames:
            pad_amount = self.n_frames - ret.shape[0]
            if isinstance(ret, torch.Tensor):
                ret = torch.nn.functional.pad(ret, (0, 0, 0, pad_amount))
            else:
                ret = np.pad(ret, ((0, pad_amount), (0, 0)))
        return ret

    def batch(self, start, size):
        """Windows [start, start+size) as one (n, n_frames, F) GPU tensor through the gather kernel."""
        if not (isinstance(self.feats, torch.Tensor) and self.feats.is_cuda):
            raise _hip.LadHipError("InferenceDataset.batch needs GPU-resident features")
        T = self.feats.shape[0]
        n = max(0, min(size, T - start))
        store = FeatureStore(device=self.feats.device)
        store.add_features("file", self.feats)
        dev = self.feats.device
        first = torch.arange(start, start + n, dtype=torch.int64, device=dev)
        count = torch.clamp(T - first, max=self.n_frames).to(torch.int32)
        return gather_segments(store, torch.zeros(n, dtype=torch.int32, device=dev), first, count, self.n_frames, 0.0)
