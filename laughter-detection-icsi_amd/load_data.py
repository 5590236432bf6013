"""Drop-in for the reference's load_data.py: same two factory functions, data resident on the MI355X.

Reference: load_data.py:12-34 `create_training_dataloader(cutset_dir, split, shuffle=False)` (Lhotse CutSet +
SingleCutSampler(max_cuts=32) + DataLoader(batch_size=None); the loop reads `.sampler.num_cuts`, train.py:305-306),
load_data.py:37-54 `create_inference_dataloader(audio_path)` (whole file -> features -> InferenceDataset ->
DataLoader(batch_size=32)).

Lhotse manifests are replaced by the data-frame CSVs the reference itself produces (create_data_df.py:171-172 schema,
`{split}_df.csv`) plus the audio files they name: channels are featurised once on the GPU and kept in HBM.
Audio: 16 kHz mono .wav (int16/float) or .npy float arrays; NIST .sph needs external conversion (sph2pipe), as in
the reference's own tooling (analysis/output_processing/laughs_to_wav.py).  Files at another sampling rate are refused unless
the caller asks for `resample=True` (load_audio_device: converted on the GPU, csrc/resample.hip).
"""
import os
import sys

import numpy as np
import torch

import config as cfg
from datasets import FeatureStore, InferenceDataset, LadDataset
import parallel
import segments

sys.path.append(os.path.join(os.path.dirname(os.path.abspath(__file__)), "utils"))
from utils import get_feat_extractor  # noqa: E402


def load_audio(path, sampling_rate=16000):
    """Mono float32 in [-1, 1] at `sampling_rate`."""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".npy":
        return np.load(path).astype(np.float32).reshape(-1)
    if ext == ".wav":
        from scipy.io import wavfile
        sr, x = wavfile.read(path)
        if sr != sampling_rate:
            raise ValueError(f"{path}: expected {sampling_rate} Hz audio, got {sr}")
        if x.ndim > 1:
            x = x[:, 0]
        if x.dtype == np.int16:
            return (x.astype(np.float32) / 32768.0)
        if x.dtype == np.int32:
            return (x.astype(np.float32) / 2147483648.0)
        return x.astype(np.float32)
    raise ValueError(f"unsupported audio format {ext!r} ({path}): convert NIST sphere files with sph2pipe first")


def load_audio_device(path, sampling_rate=16000, device="cuda", resample=False, source_rate=None):
    """Mono float32 GPU tensor at `sampling_rate`: the file is read, uploaded and, with resample=True and a file at another
    rate, converted on the device (resample.Resampler; 16-bit PCM stays int16 until the kernel scales it, exactly as load_audio
    does).  Without resample=True a file at another rate raises the ValueError of load_audio.  `.npy` arrays carry no rate:
    `source_rate` says it (default: `sampling_rate`)."""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".npy":
        sr, x = int(source_rate or sampling_rate), np.load(path).astype(np.float32).reshape(-1)
    elif ext == ".wav":
        from scipy.io import wavfile
        sr, x = wavfile.read(path)
        if x.ndim > 1:
            x = x[:, 0]
    else:
        raise ValueError(f"unsupported audio format {ext!r} ({path}): convert NIST sphere files with sph2pipe first")
    if sr != sampling_rate and not resample:
        raise ValueError(f"{path}: expected {sampling_rate} Hz audio, got {sr}")
    if x.dtype == np.int32:
        x = x.astype(np.float32) / 2147483648.0
    elif x.dtype != np.int16:
        x = x.astype(np.float32)
    pcm = torch.from_numpy(np.ascontiguousarray(x)).to(device)
    if sr == sampling_rate:
        return pcm if pcm.dtype == torch.float32 else pcm.to(torch.float32) / 32768.0
    import resample as resample_mod
    return resample_mod.get_resampler(sr, sampling_rate, pcm.device)(pcm)


class SegmentSampler:
    """Index batches of at most `max_cuts` segments (SingleCutSampler(max_cuts=32), load_data.py:32).

    With world > 1 the segments are dealt round-robin to the ranks and the number of batches is the same on every rank
    (parallel.train_step_count): each training step issues one all-reduce, so ranks must never disagree on the count.
    A ragged last batch is dropped on ALL ranks when any rank would see fewer than `min_batch` segments in it."""

    def __init__(self, n, max_cuts=32, rank=0, world=1, min_batch=1):
        self.n, self.max_cuts = n, max_cuts
        self.num_cuts = n
        self.rank, self.world, self.min_batch = rank, world, min_batch

    def __iter__(self):
        return parallel.train_batches(self.n, self.max_cuts, self.rank, self.world, self.min_batch)

    def __len__(self):
        return parallel.train_step_count(self.n, self.max_cuts, self.world, self.min_batch)


class SegmentLoader:
    """Iterable of batch dicts with the attributes the reference loop reads (`.sampler.num_cuts`, `.dataset`)."""

    def __init__(self, dataset, sampler):
        self.dataset, self.sampler = dataset, sampler

    def __iter__(self):
        for idx in self.sampler:
            yield self.dataset[idx]

    def __len__(self):
        return len(self.sampler)


INDEX_SHUFFLE_SEED = 0


def load_segment_table(cutset_dir, split, shuffle=False, seed=None, world=1, index_seed=INDEX_SHUFFLE_SEED, keep_regions=False):
    """The epoch's segment order for `split` (host integers only, no GPU): `{split}_df.csv` -> index-time permutation
    (compute_features.py:191-193) -> optional loader-time shuffle (load_data.py:27-28).  Identical on every rank.
    keep_regions: the table also carries each row's (start, duration) region and its place in the CSV (redraw='window')."""
    if split not in ['train', 'dev', 'test']:
        raise ValueError(
            f"Unexpected value for split. Needs to be one of 'train, dev, test'. Found {split}")
    table = segments.table_from_csv(os.path.join(cutset_dir, f'{split}_df.csv'), keep_regions=keep_regions)
    if index_seed is not None:
        table = table.shuffled(index_seed)
    if shuffle:
        if seed is None and world > 1:
            raise ValueError("shuffle=True in a data-parallel job needs an explicit seed (every rank must draw the same order)")
        table = table.shuffled(seed)
    return table


def read_feats_manifest(path):
    """`{split}_feats.jsonl` of compute_features.compute_features_per_split -> {key: record}; a recording is found by the
    absolute path of its audio file, by that path without its extension, or by its id."""
    import json
    by_key = {}
    if os.path.isdir(path):
        files = sorted(os.path.join(path, f) for f in os.listdir(path) if f.endswith('.jsonl'))
    else:
        # a data-parallel compute_features run leaves one manifest per rank next to the name asked for
        stem = path[:-len('.jsonl')] if path.endswith('.jsonl') else path
        d = os.path.dirname(path) or '.'
        files = [path] if os.path.isfile(path) else []
        files += sorted(os.path.join(d, f) for f in os.listdir(d)
                        if f.startswith(os.path.basename(stem) + '.rank') and f.endswith('.jsonl'))
    if not files:
        raise FileNotFoundError(f"no feature manifest at {path}")
    for fpath in files:
        with open(fpath) as f:
            for line in f:
                line = line.strip()
                if not line:
                    continue
                rec = json.loads(line)
                ap = os.path.abspath(rec['audio_path'])
                by_key[ap] = rec
                by_key[os.path.splitext(ap)[0]] = rec
                by_key.setdefault('id:' + rec['id'], rec)
    return by_key


def extractor_signature(extractor):
    """What decides the numbers an extractor writes: its configuration without the device (feats.HipFbankConfig).  Stored with
    every manifest record by compute_features.py and compared here before stored features are trained on."""
    d = dict(extractor.config.to_dict())
    d.pop('device', None)
    return d


def _stored_features(manifest, path, num_filters, extractor=None):
    """The stored (T, F) matrix of the recording whose audio is `path`, or None when the manifest does not list it.
    extractor: the configured feature extractor; stored features that another configuration produced (frame shift, filter
    bank, window, ...) are refused -- they would be trained on silently otherwise."""
    ap = os.path.abspath(path)
    rec = manifest.get(ap) or manifest.get(os.path.splitext(ap)[0])
    if rec is None:
        return None
    if extractor is not None:
        want = extractor_signature(extractor)
        have = rec.get('extractor')
        if have is not None:
            diff = sorted(k for k in set(want) | set(have) if want.get(k) != have.get(k))
            if diff:
                raise ValueError(f"{rec['features_path']}: stored features come from another extractor configuration (differs in "
                                 f"{', '.join(diff)}); re-run compute_features.py or train from the audio")
        elif abs(float(rec.get('frame_shift', want['frame_shift'])) - float(want['frame_shift'])) > 1e-12:
            raise ValueError(f"{rec['features_path']}: stored features have frame shift {rec['frame_shift']}, the configured extractor "
                             f"{want['frame_shift']}")
    feats = np.load(rec['features_path'])
    if feats.ndim != 2 or feats.shape[0] != rec['num_frames'] or feats.shape[1] != num_filters:
        raise ValueError(f"{rec['features_path']}: stored features {feats.shape} do not match the manifest "
                         f"({rec['num_frames']}, {rec['num_features']}) / the configured {num_filters} filters")
    return feats.astype(np.float32, copy=False)


def create_training_dataloader(cutset_dir, split, shuffle=False, batch_size=32, audio_root=None, seed=None, rank=0,
                               world=1, store=None, index_seed=INDEX_SHUFFLE_SEED, feats_manifest=None, resample=False,
                               augment=None, noise=None, redraw=None, transcripts=None, channels=None, redraw_seed=None):
    '''
    Create a dataloader for the provided split
        - split needs to be one of 'train', 'dev' and 'test'
        - cutset_dir holds `{split}_df.csv` (segment rows) ; audio paths are resolved against `audio_root`
        - shuffle shuffles the segment table before batching (CutSet.shuffle(), load_data.py:27-28)
        - index_seed: the data-frame CSVs list every speech row, then every laugh row (create_data_df.py:177-179); the
          reference mixes them ONCE when it builds the segment index (`cuts.shuffle()`, compute_features.py:191-193) and
          its loaders then read that stored order.  The same one-off permutation is applied here, with a fixed seed so
          that every rank of a data-parallel job derives the same order BEFORE the segments are dealt to the ranks.
          None keeps the CSV order (single-class batches on the reference's tables: only for tests).
        - feats_manifest: a `{split}_feats.jsonl` written by compute_features.compute_features_per_split (or a directory of
          them).  Channels it lists are loaded from their stored (T, F) matrices instead of being featurised again -- the
          reference trains from stored features too (compute_features.py:105-111 writes them, load_data.py:24-25 and
          datasets.py:56 read them).  The stored matrices are the extractor's raw float32 output (no lilcom stage), so the
          batches are bit-equal to those of the audio path; channels the manifest does not list fall back to their audio.
        - resample: audio files at another rate than 16 kHz are converted on the GPU (load_audio_device) instead of refused
        - augment: an augment.AugmentConfig -- the batches are augmented inside the gather launch (csrc/augment.hip); the loop
          calls `loader.dataset.set_epoch(e)` before each epoch.  None (the default): today's batches, bit for bit.
        - noise: what augment.mix_p mixes in.  'self': the channels of this split that hold at least a segment's frames (other
          speech, no extra data); a directory or a list of audio / .npy paths: featurised into the same store under the keys
          `noise:<file name without extension>`
        - redraw: the training windows are drawn afresh on the GPU before every epoch (`loader.dataset.set_epoch(e)`: one launch of
          csrc/sample.hip, a pure function of (redraw_seed, epoch, the row's place in the table)).  'window': the rows of
          `{split}_df.csv`, each inside its own (start, duration) region, as Gillick et al. did.  'transcripts': the table is
          sampling.SegmentPools.plan(config.SAMPLING['reference'], the meetings the CSV's meeting_id column names) over the
          `transcripts` / `channels` tables (as sweep_eval.TranscriptIndex takes them); the CSV only says which meetings the
          split holds and how its channels are keyed.  The index_seed / shuffle permutation is applied to the rows once; every
          rank redraws the whole table from the same (seed, epoch), nothing is communicated.  Only for split 'train'.
          None (the default): today's batches, bit for bit.  (`resample` is the audio's sampling rate, hence the name.)
        - redraw_seed: default `seed`, or 0
    '''
    if noise is not None and augment is None:
        raise ValueError("noise channels without an augmentation config: pass augment=")
    if redraw is not None:
        if redraw not in ('window', 'transcripts'):
            raise ValueError(f"redraw must be None, 'window' or 'transcripts', got {redraw!r}")
        if split != 'train':
            raise ValueError(f"redraw is for the training split only (the {split} batches are never redrawn)")
        if (redraw == 'transcripts') != (transcripts is not None and channels is not None):
            raise ValueError("redraw='transcripts' needs the transcripts and channels tables, and only it takes them")
        if redraw_seed is None:
            redraw_seed = seed if seed is not None else 0
    elif transcripts is not None or channels is not None or redraw_seed is not None:
        raise ValueError("transcripts / channels / redraw_seed without redraw=")
    table = load_segment_table(cutset_dir, split, shuffle=shuffle, seed=seed, world=world, index_seed=index_seed,
                               keep_regions=redraw == 'window')
    if store is None:
        extractor = get_feat_extractor(num_samples=cfg.FEAT['num_samples'], num_filters=cfg.FEAT['num_filters'])
        store = FeatureStore(extractor)
    root = audio_root if audio_root is not None else cutset_dir
    manifest = read_feats_manifest(feats_manifest) if feats_manifest is not None else None

    def load_channels(keys):
        for key in keys:
            if key not in store.keys:
                path = key if os.path.isabs(key) else os.path.join(root, key)
                if not os.path.exists(path):
                    for alt in (".wav", ".npy"):
                        if os.path.exists(os.path.splitext(path)[0] + alt):
                            path = os.path.splitext(path)[0] + alt
                            break
                stored = _stored_features(manifest, path, cfg.FEAT['num_filters'], getattr(store, 'extractor', None)) if manifest is not None else None
                if stored is not None:
                    store.add_features(key, stored)
                elif resample:
                    store.add_audio(key, load_audio_device(path, device=store.device, resample=True))
                else:
                    store.add_audio(key, load_audio(path))

    sampler = None
    if redraw == 'transcripts':
        sampler, table = _transcript_sampler(os.path.join(cutset_dir, f'{split}_df.csv'), table.frames_per_segment, transcripts, channels,
                                             store, load_channels, redraw_seed, shuffle, seed, world, index_seed)
    load_channels(table.channels)
    if redraw is not None:
        dataset = LadDataset(store, table, augment=augment, noise=_noise_channels(store, noise, resample) if augment is not None else None,
                             redraw=sampler if sampler is not None else 'window', redraw_seed=redraw_seed)
    elif augment is None:
        dataset = LadDataset(store, table)
    else:
        dataset = LadDataset(store, table, augment=augment, noise=_noise_channels(store, noise, resample))
    # train-mode BatchNorm needs two segments per batch on every rank: a shorter ragged tail is dropped on all ranks alike
    return SegmentLoader(dataset, SegmentSampler(len(table), max_cuts=batch_size, rank=rank, world=world,
                                                 min_batch=2 if split == 'train' else 1))


def _transcript_sampler(csv_path, T, transcripts, channels, store, load_channels, redraw_seed, shuffle, seed, world, index_seed):
    """(sampling.Sampler, its epoch-0 SegmentTable) for redraw='transcripts': the plan of config.SAMPLING['reference'] for the
    meetings the CSV's meeting_id column names, over pools that end where the channels' features in the store end, permuted once as
    load_segment_table permutes the CSV's rows."""
    import csv

    import sampling
    import sweep_eval
    with open(csv_path, newline="") as f:
        meetings = list(dict.fromkeys(r["meeting_id"] for r in csv.DictReader(f)))
    rows = [r for r in sweep_eval._records(transcripts, sweep_eval.ROW_COLUMNS) if r["meeting_id"] in meetings]
    chans = [c for c in sweep_eval._records(channels, sweep_eval.CHANNEL_COLUMNS) if c["meeting_id"] in meetings]
    unknown = [m for m in meetings if m not in {c["meeting_id"] for c in chans}]
    if unknown:
        raise ValueError(f"the split names meetings the channel table does not hold: {unknown}")
    keys = [sampling.channel_key(c["meeting_id"], c["chan"]) for c in chans if c["part_id"] not in (None, "")]
    load_channels(keys)
    frames = {k: int(store.mats[store.index_of(k)].shape[0]) for k in keys}
    pools = sampling.SegmentPools.from_transcripts(rows, chans, fps=cfg.FEAT['num_samples'], T=T, frames=frames)
    sampler = sampling.Sampler(pools, pools.plan('reference', meetings), redraw_seed, device=store.device)
    if index_seed is not None:
        sampler = sampler.take(np.random.default_rng(index_seed).permutation(len(sampler)))
    if shuffle:
        if seed is None and world > 1:
            raise ValueError("shuffle=True in a data-parallel job needs an explicit seed (every rank must draw the same order)")
        sampler = sampler.take(np.random.default_rng(seed).permutation(len(sampler)))
    return sampler, sampler.table(0)


def _noise_channels(store, noise, resample=False):
    """`noise` of create_training_dataloader -> what LadDataset takes: 'self' as it is, files featurised into the store."""
    if noise is None or noise == 'self':
        return noise
    if isinstance(noise, (str, os.PathLike)):
        d = os.fspath(noise)
        if not os.path.isdir(d):
            raise ValueError(f"noise: {d} is neither 'self' nor a directory")
        paths = sorted(os.path.join(d, f) for f in os.listdir(d) if os.path.splitext(f)[1].lower() in ('.wav', '.npy'))
        if not paths:
            raise ValueError(f"noise: no .wav / .npy files in {d}")
    else:
        paths = [os.fspath(p) for p in noise]
    keys = []
    for path in paths:
        key = 'noise:' + os.path.splitext(os.path.basename(path))[0]
        if key not in store.keys:
            if resample:
                store.add_audio(key, load_audio_device(path, device=store.device, resample=True))
            else:
                store.add_audio(key, load_audio(path))
        keys.append(key)
    return keys


class InferenceLoader:
    """Batches of <= batch_size stride-one-frame windows, (n, FEAT['num_samples'], F) GPU float32 (DataLoader(batch_size=32))."""

    def __init__(self, dataset, batch_size=32):
        self.dataset, self.batch_size = dataset, batch_size

    def __iter__(self):
        for s in range(0, len(self.dataset), self.batch_size):
            yield self.dataset.batch(s, self.batch_size)

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size


def create_inference_dataloader(audio_path, batch_size=32, resample=False):
    '''
    Create inference dataloader for the audio file `audio_path`: the whole file is featurised in one GPU launch and the
    windows are read out of that (T, F) matrix.  `loader.dataset.feats` is the matrix itself, for
    `model.engine.predict_windows`, which skips the window materialisation altogether.
    resample=True: a file at another rate than 16 kHz is converted on the GPU first (load_audio_device) instead of refused.
    '''
    extractor = get_feat_extractor(num_samples=cfg.FEAT['num_samples'], num_filters=cfg.FEAT['num_filters'])
    if resample:
        pcm = load_audio_device(audio_path, device=extractor.config.device, resample=True)
    else:
        pcm = torch.from_numpy(load_audio(audio_path)).to(extractor.config.device)
    feats_all = extractor.extract_long(pcm.contiguous())
    dataset = InferenceDataset(feats_all)
    return InferenceLoader(dataset, batch_size=batch_size)
