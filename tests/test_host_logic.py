"""CPU tests of the host-side integer logic: segmenter vs reference goldens, segment table vs the oracle restatement
and the reference's own sample tables, InferenceDataset window semantics."""
import csv
import json
import os

import numpy as np
import pytest

from oracle import recipe, segmenter_oracle as so, segments_oracle as sgo


def test_segmenter_matches_reference_golden(golden_dir):
    import laugh_segmenter as ls
    cases = json.load(open(os.path.join(golden_dir, "segmenter.json")))
    assert len(cases) >= 3
    for c in cases:
        p = recipe.make_prob_track(c["seed"], c["n"]) if "seed" in c else np.array(c["probs"])
        d = ls.get_laughter_instances(p, c["thresholds"], c["min_lengths"], c["fps"])
        ref = {tuple(k): [tuple(s) for s in v] for k, v in c["result"]}
        assert list(d.keys()) == list(ref.keys())
        for k in ref:
            assert d[k] == ref[k], (c.get("seed", c.get("name")), k)


@pytest.mark.parametrize("n,seed", [(1, 0), (2, 1), (1000, 2), (36000, 3)])
def test_segmenter_run_indices_bit_exact_vs_oracle(n, seed):
    import laugh_segmenter as ls
    p = recipe.make_prob_track(seed, n) if n >= 100 else np.random.default_rng(seed).random(n)
    for thr in (0.0, 0.3, 0.5, 0.99, 1.0):
        got = [tuple(int(v) for v in r) for r in ls.get_laughter_frame_spans(p, thr)]
        assert got == so.run_indices(p, thr)
    # float32 probabilities straight from the GPU head behave the same
    p32 = p.astype(np.float32)
    assert [tuple(int(v) for v in r) for r in ls.get_laughter_frame_spans(p32, 0.5)] == so.run_indices(p32, 0.5)


def test_segmenter_edge_cases():
    import laugh_segmenter as ls
    assert ls.get_laughter_instances([], [0.5], [0.2], 100.0) == {(0.5, 0.2): []}
    d = ls.get_laughter_instances([0.9] * 30, [0.5], [0.2, 0.3], 100.0)
    assert d[(0.5, 0.2)] == [(0.0, 0.29)] and d[(0.5, 0.3)] == []  # 0.29 - 0.0 > 0.2 only
    d = ls.get_laughter_instances([0.0, -1.0, 2.0, 0.0], [0.0], [0.0], 1.0)
    assert d[(0.0, 0.0)] == [(0.0, 3.0)]  # p <= 0 becomes 1e-7 > 0; p > 1 becomes 1
    assert ls.fix_over_underflow(1.5) == 1 and ls.fix_over_underflow(0) == 0.0000001 and ls.fix_over_underflow(0.3) == 0.3


@pytest.mark.parametrize("name", ["sample_df.csv", "tiny_sample.csv"])
def test_segment_table_matches_oracle_on_reference_sample_tables(golden_dir, name):
    import segments
    path = os.path.join(golden_dir, "data_dfs", name)
    rows = list(csv.DictReader(open(path)))
    assert list(rows[0].keys()) == ["start", "duration", "sub_start", "sub_duration", "audio_path", "meeting_id", "chan_id", "label"]
    t = segments.table_from_csv(path)
    chans, ref = sgo.rows_to_segments(rows)
    assert t.channels == chans and len(t) == len(ref)
    got = list(zip(t.channel.tolist(), t.first_frame.tolist(), t.n_frames.tolist(), t.label.tolist()))
    assert got == ref
    assert t.n_frames.max() <= 100 and t.first_frame.dtype == np.int64 and t.label.dtype == np.int32
    # first row of the sample table: sub_start 1478.92 s -> frame 147892, one full second
    assert got[0][1:3] == (147892, 100)


def test_segment_table_short_ragged_and_bad_rows():
    import segments
    rows = [dict(start=0, duration=0.5, sub_start=0.0, sub_duration=0.37, audio_path="a.wav", meeting_id="m", chan_id="c", label=1),
            dict(start=3, duration=2, sub_start=3.29, sub_duration=1.0, audio_path="b.wav", meeting_id="m", chan_id="d", label=0)]
    t = segments.table_from_rows(rows)
    assert t.n_frames.tolist() == [37, 100] and t.first_frame.tolist() == [0, 329]  # 3.29 / 0.01 = 328.99999999999994 -> 329
    assert segments.table_from_rows([]).label.shape == (0,)
    with pytest.raises(ValueError):
        segments.table_from_rows([dict(rows[0], label=2)])
    with pytest.raises(ValueError):
        segments.table_from_rows([dict(rows[0], sub_start=-1.0)])
    sh = t.shuffled(3)
    assert sorted(sh.first_frame.tolist()) == [0, 329]
    assert len(t.shard(0, 2)) == 1 and len(t.shard(1, 2)) == 1 and len(t.shard(2, 3)) == 0


def test_whole_track_windows_and_labels():
    import segments
    laughs = [(1500, 1800), (3000, 3001), (5999, 7000)]
    t = segments.whole_track_table(799, "Bmr021/chan3.sph", laughs)
    ref = sgo.whole_track_windows(799, laughs)
    assert len(t) == 7 == len(ref)  # the 8th window is partial and dropped
    assert list(zip(t.first_frame.tolist(), t.n_frames.tolist(), t.label.tolist())) == ref
    # (1000,2000] overlaps (1500,1800]; (3000,4000] overlaps (3000,3001]; (2000,3000] does NOT touch (3000,3001]
    assert t.label.tolist() == [0, 1, 0, 1, 0, 1, 1]


def test_inference_dataset_window_semantics():
    import datasets
    feats = np.arange(250 * 44, dtype=np.float32).reshape(250, 44)
    ds = datasets.InferenceDataset(feats)
    assert len(ds) == 250
    assert np.array_equal(ds[0], feats[:100])
    last = ds[249]
    assert last.shape == (100, 44) and np.array_equal(last[0], feats[249]) and np.all(last[1:] == 0.0)
    mid = ds[200]
    assert np.array_equal(mid[:50], feats[200:]) and np.all(mid[50:] == 0.0)


def test_parallel_window_shards_cover_track():
    import parallel
    T = 360000
    seen = 0
    for r in range(8):
        sh = parallel.shard_indices(T, r, 8)
        assert sh.start == seen
        seen = sh.stop
    assert seen == T


def test_get_audio_length_reads_header_only(tmp_path):
    """audio_utils.get_audio_length (reference audio_utils.py:7-9): samples / rate, also for a ragged sample count."""
    import audio_utils
    import load_data
    from scipy.io import wavfile
    n = 16000 * 2 + 37
    x = (np.sin(np.arange(n) * 0.01) * 0.3).astype(np.float32)
    wavfile.write(str(tmp_path / "a.wav"), 16000, (x * 32767).astype(np.int16))
    wavfile.write(str(tmp_path / "f.wav"), 16000, x)  # IEEE-float wav: the `wave` module rejects it
    np.save(str(tmp_path / "a.npy"), x)
    for name in ("a.wav", "f.wav", "a.npy"):
        p = str(tmp_path / name)
        assert audio_utils.get_audio_length(p) == n / 16000.0
        assert load_data.load_audio(p).shape == (n,)
    with pytest.raises(ValueError):
        audio_utils.get_audio_length(str(tmp_path / "a.sph"))


def test_rank_manifests_of_a_data_parallel_featurisation_are_found_and_foreign_features_refused(tmp_path):
    """compute_features.py under N ranks leaves {split}_feats.rank<r>.jsonl (no {split}_feats.jsonl): train.find_feats_manifests
    must find them (it silently re-featurised from audio), load_data.read_feats_manifest gathers them, and a record
    written by ANOTHER extractor configuration (frame shift, filter bank, ...) is refused instead of being trained on."""
    import argparse
    import json
    import types

    import load_data
    import train
    cut = tmp_path / "lhotse" / "cutsets"
    cut.mkdir(parents=True)
    cfg_now = {"sampling_rate": 16000, "frame_shift": 0.01, "num_filters": 44, "mel_variant": "kaldi"}
    ext = types.SimpleNamespace(config=types.SimpleNamespace(to_dict=lambda: dict(cfg_now, device="cuda")))
    assert load_data.extractor_signature(ext) == cfg_now   # the device does not decide the numbers
    feats = np.arange(300 * 44, dtype=np.float32).reshape(300, 44)
    for r, name in enumerate(("a", "b")):
        np.save(tmp_path / f"{name}.npy", feats + r)
        rec = {"id": name, "audio_path": str(tmp_path / f"{name}.wav"), "features_path": str(tmp_path / f"{name}.npy"),
               "num_frames": 300, "num_features": 44, "frame_shift": 0.01, "extractor": cfg_now}
        (cut / f"train_feats.rank{r}.jsonl").write_text(json.dumps(rec) + "\n")
    args = argparse.Namespace(feats_manifest_dir=None, data_root=str(tmp_path), lhotse_dir="lhotse")
    found = train.find_feats_manifests(args)
    assert found == {"train": str(cut / "train_feats.jsonl")}            # the stem stands for the rank files
    assert train.find_feats_manifests(argparse.Namespace(feats_manifest_dir=str(cut), data_root="x", lhotse_dir="y")) == found
    with pytest.raises(SystemExit):
        train.find_feats_manifests(argparse.Namespace(feats_manifest_dir=str(tmp_path), data_root="x", lhotse_dir="y"))
    man = load_data.read_feats_manifest(found["train"])
    got = load_data._stored_features(man, str(tmp_path / "b.wav"), 44, ext)
    assert np.array_equal(got, feats + 1)
    assert load_data._stored_features(man, str(tmp_path / "nobody.wav"), 44, ext) is None
    other = types.SimpleNamespace(config=types.SimpleNamespace(to_dict=lambda: dict(cfg_now, frame_shift=0.0125, device="cuda")))
    with pytest.raises(ValueError, match="another extractor configuration.*frame_shift"):
        load_data._stored_features(man, str(tmp_path / "a.wav"), 44, other)
    # a manifest of round 4 (no extractor record) is still checked for what it does hold: the frame shift
    old = {k: v for k, v in json.loads((cut / "train_feats.rank0.jsonl").read_text()).items() if k != "extractor"}
    (cut / "train_feats.rank0.jsonl").write_text(json.dumps(old) + "\n")
    man = load_data.read_feats_manifest(found["train"])
    assert load_data._stored_features(man, str(tmp_path / "a.wav"), 44, ext) is not None
    with pytest.raises(ValueError, match="frame shift"):
        load_data._stored_features(man, str(tmp_path / "a.wav"), 44, other)


def _read_laughter_textgrid(path):
    """What analysis/analyse.py:39-46 takes from a file: `grid['laughter']` of praat-textgrids, every interval's xmin / xmax / text
    (long "ooTextFile" format: `item [k]:` -> `name`, `intervals [i]:` -> `xmin`, `xmax`, `text`), kept iff text == 'laugh'."""
    import re
    text = open(path).read()
    assert text.startswith('File type = "ooTextFile"\nObject class = "TextGrid"\n')
    head, *items = re.split(r"\n\s*item \[\d+\]:\n", text)
    tiers = {}
    for item in items:
        assert re.search(r'class = "IntervalTier"', item)
        name = re.search(r'name = "([^"]*)"', item).group(1)
        n = int(re.search(r"intervals: size = (\d+)", item).group(1))
        ivs = [(float(a), float(b), t) for a, b, t in
               re.findall(r'intervals \[\d+\]:\s*xmin = (\S+)\s*xmax = (\S+)\s*text = "([^"]*)"', item)]
        assert len(ivs) == n
        tiers[name] = ivs
    xmax = float(re.search(r"\nxmax = (\S+)", head).group(1))
    assert int(re.search(r"\nsize = (\d+)", head).group(1)) == len(tiers)
    grid = tiers["laughter"]
    # a tier praat accepts: contiguous from 0 to xmax, no empty or reversed interval
    t = 0.0
    for a, b, _ in grid:
        assert a == t and b > a
        t = b
    assert t == xmax or not grid
    return [(a, b) for a, b, txt in grid if str(txt) == "laugh"], xmax


def test_textgrid_round_trip_gives_back_the_instances(tmp_path):
    """The TextGrid the path writes (segment_laughter.py:150-161) read back the way the reference's evaluation reads it
    (analysis/analyse.py:39-46): exactly the instances of get_laughter_instances, bit for bit."""
    import laugh_segmenter as ls
    import textgrid
    p = recipe.make_prob_track(5, 3000)
    p[-40:] = 0.99                                       # a laugh that runs to the last frame of the file
    fps, file_length = 100.0, 30.0
    d = ls.get_laughter_instances(p, [0.2, 0.5, 0.8], [0.0, 0.2], fps)
    assert any(v and v[-1][1] == (len(p) - 1) / fps for v in d.values())
    cases = list(d.items()) + [(("empty", 0), []), (("to_xmax", 0), [(1.25, 2.5), (29.0, file_length)]),
                               (("from_zero", 0), [(0.0, 0.31)]), (("touching", 0), [(1.0, 2.0), (2.0, 3.5)])]
    for key, instances in cases:
        path = tmp_path / f"{key[0]}_{key[1]}.TextGrid"
        textgrid.write_laughter_textgrid(str(path), instances, xmax=file_length)
        got, xmax = _read_laughter_textgrid(str(path))
        assert got == [(float(a), float(b)) for a, b in instances], key
        assert xmax == file_length
    # no file length given: the tier ends at the last instance; nothing at all: an empty tier
    textgrid.write_laughter_textgrid(str(tmp_path / "a.TextGrid"), [(0.5, 0.75)])
    assert _read_laughter_textgrid(str(tmp_path / "a.TextGrid")) == ([(0.5, 0.75)], 0.75)
    textgrid.write_laughter_textgrid(str(tmp_path / "b.TextGrid"), [])
    assert _read_laughter_textgrid(str(tmp_path / "b.TextGrid")) == ([], 0.0)


def test_format_outputs_is_the_references():
    """laugh_segmenter.py:141-149."""
    import laugh_segmenter as ls
    inst = [(0.5, 1.25), (3.0, 3.5)]
    assert ls.format_outputs(inst) == [{'start': 0.5, 'end': 1.25}, {'start': 3.0, 'end': 3.5}]
    out = ls.format_outputs(inst, ["a.wav", "b.wav"])
    assert out == [{'filename': "a.wav", 'start': 0.5, 'end': 1.25}, {'filename': "b.wav", 'start': 3.0, 'end': 3.5}]
    assert list(out[0]) == ['filename', 'start', 'end']
    assert ls.format_outputs([]) == []
    with pytest.raises(IndexError):
        ls.format_outputs(inst, ["a.wav"])


def test_librosa_convention_host_tables_are_the_third_party_goldens(golden_dir):
    """The product's librosa-convention tables (feats.slaney_mel_bank, hann_window_periodic, dct2_ortho: the only place the
    convention enters -- the kernel is the same) against tests/golden/librosa_conv.npz (transformers.audio_utils) and
    scipy.fft.dct.  Host arithmetic only: nothing here needs the GPU."""
    import feats
    g = np.load(os.path.join(golden_dir, "librosa_conv.npz"))
    for n_mels in (44, 40, 128):
        assert np.abs(feats.slaney_mel_bank(n_mels, 16000) - g[f"bank_{n_mels}"]).max() < 1e-15
    scipy_fft = pytest.importorskip("scipy.fft")
    eye = np.eye(44)
    assert np.abs(feats.dct2_ortho(44, 20) - scipy_fft.dct(eye, type=2, norm="ortho", axis=0)[:20].T).max() < 1e-14
    sig = pytest.importorskip("scipy.signal")
    assert np.abs(feats.hann_window_periodic(400) - sig.get_window("hann", 400, fftbins=True)).max() < 1e-15


# ------------------------------------------------------------------------------------------ the training schedule (engine.train_schedule)
_ALL_ON = dict(bf16x3=True, bf16x3_32=True, f16x2=True, f16x2_32=True, relu_bits=True, virtual_a1=True, fuse_bn_bwd=False, fuse_bn_bwd_b3=True,
               fuse_bn_bwd_wgrad=True, fuse_s2_shortcut=True, fuse_s2_shortcut_wgrad=True, s2_b3=True)   # ResNetEngine's defaults


def _rows(sched):
    """A schedule as one dict per block; a convolution as "<forward / data-gradient arithmetic>/<weight-gradient kernel>[+bn]"."""
    def conv(c):
        return None if c is None else f"{c.arith}/{c.wgrad}{'+bn' if c.wgrad_bn else ''}"

    return [dict(entry=b.entry, a1_virtual=b.a1_virtual, bits=b.bits, dgrad2_bn=b.dgrad2_bn, dgrad1_bn=b.dgrad1_bn, sc_wgrad_fused=b.sc_wgrad_fused,
                 c1=conv(b.conv1), c2=conv(b.conv2), sc=conv(b.sc)) for b in sched.blocks]


def _row(entry, a1_virtual, bits, dgrad2_bn, dgrad1_bn, sc_wgrad_fused, c1, c2, sc):
    return dict(entry=entry, a1_virtual=a1_virtual, bits=bits, dgrad2_bn=dgrad2_bn, dgrad1_bn=dgrad1_bn, sc_wgrad_fused=sc_wgrad_fused, c1=c1, c2=c2, sc=sc)


def _launchable(engine, blocks, sched):
    """Every stride-1 convolution and weight-gradient launch the engine makes from this schedule has an entry point."""
    mask = {None: None, "split": "bits", "f32": "y"}
    for b, ch in zip(blocks, sched.blocks):
        if b.conv1.stride == 1:
            engine.conv_s1_entry(ch.conv1.arith, b.conv1.cin)
            engine.conv_wgrad_entry(ch.conv1.wgrad, bn=ch.conv1.wgrad_bn)
            engine.conv_s1_entry("f32" if ch.dgrad1_bn == "f32" else ch.conv1.arith, b.conv1.cin, gated=ch.bits, bn=mask[ch.dgrad1_bn])
            if ch.sc is not None:
                engine.conv_s1_entry(ch.sc.arith, b.sc_conv.cin)
                engine.conv_wgrad_entry(ch.sc.wgrad)
        engine.conv_s1_entry(ch.conv2.arith, b.conv2.cin, in_coef=ch.a1_virtual)
        engine.conv_wgrad_entry(ch.conv2.wgrad, in_coef=ch.a1_virtual, bn=ch.bits and ch.conv2.wgrad_bn)
        engine.conv_s1_entry("f32" if ch.dgrad2_bn == "f32" else ch.conv2.arith, b.conv2.cin, bn="x" if ch.dgrad2_bn else None)


def test_train_schedule_of_resnet_base_and_of_the_augmentation_widths():
    """engine.train_schedule: the kernels of a training step as a literal table -- resnet_base on (100, 44) with the default flags at
    four batch sizes (past 2 GiB per tensor the 32-channel layers leave the split-operand kernels, the 64-channel ones do not), every
    flag flipped alone at batch 512 (which fields move, and no others), resnet_with_augmentation on (128, 44) (exact f32, nothing
    fused).  No schedule asks for a launch the library has no entry point for; such a combination is an error."""
    import _hip
    import engine
    base = engine.block_geometry(64, [64, 32, 16, 16], 100, 44, True)
    assert [(b.name, b.conv1.cin, b.conv1.cout, b.conv1.stride, b.conv1.h_in, b.conv1.w_in, b.sc_conv is not None) for b in base] == [
        ("block1.0", 64, 64, 1, 100, 44, False), ("block1.1", 64, 64, 1, 100, 44, False),
        ("block2.0", 64, 32, 2, 100, 44, True), ("block2.1", 32, 32, 1, 50, 22, False),
        ("block3.0", 32, 16, 2, 50, 22, True), ("block3.1", 16, 16, 1, 25, 11, False),
        ("block4.0", 16, 16, 2, 25, 11, True), ("block4.1", 16, 16, 1, 13, 6, False)]
    small = [_row("s2_fused", False, False, None, None, True, "f32/f32", "f32/f32", "f32/f32"),
             _row("plain", False, False, None, None, False, "f32/f32", "f32/f32", None)] * 2
    default = [_row("plain", True, True, "split", None, False, "h2/h2+bn", "h2/h2+bn", None),
               _row("plain", True, True, "split", "split", False, "h2/h2+bn", "h2/h2+bn", None),
               _row("s2b3", True, False, "split", "split", True, "f32/f32", "h2/b3c", "f32/f32"),
               _row("plain", True, False, "split", None, False, "h2/b3c", "h2/b3c", None)] + small
    for B in (32, 512, 2048):
        sched = engine.train_schedule(base, B, _ALL_ON, True)
        assert _rows(sched) == default, B
        assert sched.stem_onepass is True and dict(sched.opts) == _ALL_ON
        assert sched.images == {("h2", n) for n in ("block1.0.conv1", "block1.0.conv2", "block1.1.conv1", "block1.1.conv2", "block2.0.conv2",
                                                    "block2.1.conv1", "block2.1.conv2")} | {("s2b3", "block2.0.conv1")}
        _launchable(engine, base, sched)
    labels = [(b.conv1.label_fwd, b.conv1.label_dgrad, b.conv2.label_fwd, b.conv2.label_dgrad) for b in sched.blocks]
    assert labels[:4] == [("conv_h2<64,64,9>",) * 4, ("conv_h2<64,64,9>",) * 4,
                          ("conv_s2b3<64,32,9>", "conv_s1<32,64,9>", "conv_h2<32,32,9>", "conv_h2<32,32,9>"), ("conv_h2<32,32,9>",) * 4]
    assert labels[4] == ("conv_s2<32,16,9>", "conv_s1<16,32,9>", "conv_s1<16,16,9>", "conv_s1<16,16,9>") and sched.blocks[4].sc.label_fwd == "conv_s2<32,16,1>"
    # batch 16000: 32 x 50 x 22 floats per item pass 2 GiB (the 32-channel kernels' 32-bit byte offsets); 64 channels count rows
    sched = engine.train_schedule(base, 16000, _ALL_ON, True)
    assert _rows(sched) == default[:2] + [_row("s2b3", False, False, None, "split", True, "f32/f32", "f32/f32", "f32/f32"),
                                          _row("plain", False, False, None, None, False, "f32/f32", "f32/f32", None)] + small
    assert sched.images == {("h2", n) for n in ("block1.0.conv1", "block1.0.conv2", "block1.1.conv1", "block1.1.conv2")} | {("s2b3", "block2.0.conv1")}
    _launchable(engine, base, sched)
    # one flag flipped at batch 512: {block: fields that move}
    f32 = dict(c1="f32/f32", c2="f32/f32")
    moves = {
        "bf16x3": {0: dict(a1_virtual=False, bits=False, dgrad2_bn=None, **f32), 1: dict(a1_virtual=False, bits=False, dgrad2_bn=None, dgrad1_bn=None, **f32),
                   2: dict(entry="s2_fused", a1_virtual=False, dgrad2_bn=None, dgrad1_bn=None, c2="f32/f32"), 3: dict(a1_virtual=False, dgrad2_bn=None, **f32)},
        "bf16x3_32": {2: dict(a1_virtual=False, dgrad2_bn=None, c2="f32/f32"), 3: dict(a1_virtual=False, dgrad2_bn=None, **f32)},
        "f16x2": {0: dict(c1="b3/b3c", c2="b3/b3c"), 1: dict(c1="b3/b3c", c2="b3/b3c"), 2: dict(c2="b3/b3c"), 3: dict(c1="b3/b3c", c2="b3/b3c")},
        "f16x2_32": {2: dict(c2="b3/b3c"), 3: dict(c1="b3/b3c", c2="b3/b3c")},
        "relu_bits": {0: dict(bits=False), 1: dict(bits=False, dgrad1_bn=None), 2: dict(dgrad1_bn=None)},
        "virtual_a1": {i: dict(a1_virtual=False) for i in range(4)},
        # (on: exact-f32 epilogues wherever a BatchNorm's x and y are both in HBM; no sign bits then)
        "fuse_bn_bwd": {0: dict(bits=False, dgrad2_bn="f32"), 1: dict(bits=False, dgrad2_bn="f32", dgrad1_bn="f32"), 2: dict(dgrad2_bn="f32", dgrad1_bn=None),
                        3: dict(dgrad2_bn="f32"), 4: dict(dgrad2_bn="f32"), 5: dict(dgrad2_bn="f32"), 6: dict(dgrad2_bn="f32"), 7: dict(dgrad2_bn="f32")},
        "fuse_bn_bwd_b3": {0: dict(dgrad2_bn=None), 1: dict(dgrad2_bn=None, dgrad1_bn=None), 2: dict(dgrad2_bn=None, dgrad1_bn=None), 3: dict(dgrad2_bn=None)},
        "fuse_bn_bwd_wgrad": {0: dict(c1="h2/h2", c2="h2/h2"), 1: dict(c1="h2/h2", c2="h2/h2")},
        "fuse_s2_shortcut": {2: dict(entry="plain", dgrad1_bn=None), 4: dict(entry="plain"), 6: dict(entry="plain")},
        "fuse_s2_shortcut_wgrad": {i: dict(sc_wgrad_fused=False) for i in (2, 4, 6)},
        "s2_b3": {2: dict(entry="s2_fused")},
    }
    assert sorted(moves) == sorted(engine.ResNetEngine.KERNEL_OPTIONS)
    for flag, moved in moves.items():
        sched = engine.train_schedule(base, 512, {**_ALL_ON, flag: not _ALL_ON[flag]}, True)
        assert _rows(sched) == [{**row, **moved.get(i, {})} for i, row in enumerate(default)], flag
        assert sched.stem_onepass is True
        _launchable(engine, base, sched)
    assert engine.train_schedule(base, 512, {**_ALL_ON, "fuse_bn_bwd": True}, True).blocks[1].conv1.label_dgrad == "conv_s1<64,64,9>"
    sched = engine.train_schedule(base, 512, _ALL_ON, False)
    assert sched.stem_onepass is False and _rows(sched) == default
    # resnet_with_augmentation: whatever the flags say, exact f32 and no split-operand fusion; with the engine's own (all off) nothing at all
    aug = engine.block_geometry(64, [128, 64, 32, 32], 128, 44, False)
    assert [(b.conv1.cin, b.conv1.cout, b.conv1.stride, b.sc_conv is not None) for b in aug][:3] == [(64, 128, 1, True), (128, 128, 1, False), (128, 64, 2, True)]
    sched = engine.train_schedule(aug, 32, dict.fromkeys(_ALL_ON, False), True)
    assert _rows(sched) == [_row("plain", False, False, None, None, False, "f32/f32", "f32/f32", "f32/f32"),
                            _row("plain", False, False, None, None, False, "f32/f32", "f32/f32", None)] * 4
    assert sched.images == frozenset()
    _launchable(engine, aug, sched)
    sched = engine.train_schedule(aug, 32, _ALL_ON, True)
    assert all(c is None or c == "f32/f32" for r in _rows(sched) for c in (r["c1"], r["c2"], r["sc"]))
    assert not any(r["a1_virtual"] or r["bits"] or r["entry"] == "s2b3" or r["dgrad2_bn"] or r["dgrad1_bn"] for r in _rows(sched)) and not sched.images
    _launchable(engine, aug, sched)
    # what the library has no kernel for is refused, not replaced
    assert engine.conv_s1_entry("h2", 64, gated=True, bn="bits") == "lad_conv_h2"
    assert engine.conv_s1_entry("b3", 64, gated=True, bn="bits") == "lad_conv_b3_dgrad_bnstat"
    assert engine.conv_s1_entry("f32", 16, bn="y") == "lad_conv_fwd_bnstat"
    assert engine.conv_wgrad_entry("h2", in_coef=True, bn=True) == "lad_conv_wgrad_h2_bnbwd"
    for bad in (dict(arith="f32", cin=64, gated=True), dict(arith="f32", cin=64, in_coef=True), dict(arith="b3", cin=32, gated=True),
                dict(arith="b3", cin=64, bn="y"), dict(arith="h2", cin=64, bn="y"), dict(arith="f32", cin=64, bn="bits"), dict(arith="f16", cin=64)):
        with pytest.raises(_hip.LadHipError):
            engine.conv_s1_entry(**bad)
    for bad in (dict(kind="f32", in_coef=True), dict(kind="f32", bn=True), dict(kind="b3c", bn=True), dict(kind="b3", bn=False)):
        with pytest.raises(_hip.LadHipError):
            engine.conv_wgrad_entry(**bad)


# ------------------------------------------------------------------------------------------ the inference layout (engine.stream_layout)
_INFER_ON = dict(stream_direct=True, stream_level2=True, stream_super=True, strip_block_fused=True, small_block_fused=True, tail_fused=True,
                 strip2_resident=True, strip_stem_shared=True, f16_s2_shortcut_fused=True)   # ResNetEngine's defaults
_L1 = ("n_strip", "stream_row0", "cat_rows")
_L2 = ("shift2", "n_strip2", "h2s", "img_s2", "stream2_base", "rows2")
# (B, H): the literal table of the shared layouts of resnet_base, fp16, every switch on, no run
_SHARED2 = {
    (8192, 100): (8282, 4099590, 4472866, 76, 8268, 4146, 95381, 2472132, 2662918),
    (201, 100): (291, 144045, 157726, 76, 277, 150, 3473, 82823, 89793),
    (64, 100): (154, 76230, 83746, 76, 140, 82, 1909, 41860, 45702),
    (2, 100): (92, 45540, 50266, 76, 78, 51, 1196, 23322, 25738),
    (64, 96): (150, 74250, 81586, 72, 136, 80, 1863, 40664, 44414),
    (64, 90): (144, 71280, 78346, 66, 130, 77, 1794, 38870, 42482),
    (64, 120): (174, 86130, 94546, 96, 160, 92, 2139, 47840, 52142),
}
_WITH_RUN = [((1200, 600), 600), ((1711, 600), 511)]


def _base_layout(B, H=100, half=True, run=None, **flip):
    import engine
    return engine.stream_layout(engine.block_geometry(64, [64, 32, 16, 16], H, 44, True), B, H, 44, half, {**_INFER_ON, **flip}, run)


def _all_layouts():
    """Every layout the tests below name."""
    import engine
    out = [_base_layout(B, H) for B, H in _SHARED2] + [_base_layout(64, 101), _base_layout(1), _base_layout(64, half=False)]
    out += [_base_layout(B, run=run) for run, B in _WITH_RUN]
    out += [_base_layout(8192, **{k: False}) for k in _INFER_ON] + [_base_layout(B) for B in (165, 166, 435, 436, 511, 512)]
    out.append(engine.stream_layout(engine.block_geometry(64, [128, 64, 32, 32], 128, 44, False), 64, 128, 44, False, _INFER_ON))
    return out


def test_stream_layout_of_resnet_base_as_a_literal_table():
    """engine.stream_layout: where the strips and streams of a group of sliding windows lie, restated by hand -- group sizes from 2 to
    8192, window lengths with every level even, an odd level 2 and an odd level 1, runs of groups with a full and a short last group,
    fp32, the augmentation widths."""
    import engine
    for (B, H), want in _SHARED2.items():
        lay = _base_layout(B, H)
        assert lay.mode == "shared2" and lay.run is None and (lay.B, lay.H, lay.W, lay.half) == (B, H, 44, True)
        assert tuple(getattr(lay, f) for f in _L1 + _L2) == want, (B, H)
        assert (lay.n1, lay.band, lay.Ht, lay.img_t_rows, lay.k3, lay.band2, lay.Ht2, lay.img_t2) == (2, 5, 10, 495, 4, 6, 12, 299)
        assert (lay.Hs, lay.stream_rows, lay.n_strip_max, lay.n_strip2_max) == (B + H - 1, B + H - 1, lay.n_strip, lay.n_strip2)
        assert (lay.H2, lay.W2) == (H // 2, 22)
    odd = _base_layout(64, 101)          # odd at level 1: the phases of level 2 do not exist
    assert odd.mode == "direct" and (odd.n_strip, odd.stream_row0, odd.cat_rows) == (155, 76725, 76725 + 165 * 45 + 46)
    assert all(getattr(odd, f) is None for f in _L2 + ("k3", "H2", "W2", "band2", "Ht2", "img_t2", "n_strip2_max"))
    one = _base_layout(1)
    assert one.mode == "per_window" and (one.n1, one.band) == (2, 5)
    assert all(getattr(one, f) is None for f in _L1 + _L2 + ("Ht", "Hs", "n_strip_max", "img_t_rows"))
    # a run of groups: the stream is the run's, the strips' room is the largest group's
    lay = _base_layout(600, run=(1200, 600))
    assert lay.mode == "shared2" and lay.run == (1200, 600) and lay.stream_rows == 1299 and lay.Hs == 699
    assert (lay.stream_row0, lay.cat_rows, lay.h2s, lay.stream2_base, lay.rows2) == (341550, 400186, 650, 202124, 232094)
    lay = _base_layout(511, run=(1711, 600))                     # the short last group
    assert (lay.n_strip, lay.n_strip_max, lay.n_strip2, lay.n_strip2_max) == (601, 690, 587, 676)
    assert (lay.cat_rows, lay.rows2) == (423181, 243824)
    # a run is a feature of the fully shared path: elsewhere it comes back as None and the layout is the group's own
    assert _base_layout(64, 101, run=(128, 64)) == odd and _base_layout(1, run=(601, 600)) == one
    assert _base_layout(600, run=(1200, 600), stream_level2=False) == _base_layout(600, stream_level2=False)
    assert _base_layout(600, run=(1200, 600), stream_super=False) == _base_layout(600, stream_super=False)
    f32 = _base_layout(64, half=False)
    assert f32.mode == "assembled" and (f32.n_strip, f32.Ht, f32.Hs, f32.stream_row0, f32.cat_rows, f32.rows2) == (154, 10, 163, None, None, None)
    assert not any(f32.window_fused + f32.rides + f32.strip_fused + f32.stream_fused) and not (f32.stem_kept or f32.strip_stem_rows or f32.tail_fused)
    aug = engine.stream_layout(engine.block_geometry(64, [128, 64, 32, 32], 128, 44, False), 64, 128, 44, False, _INFER_ON)
    assert aug.mode == "per_window" and aug.n1 == 0                # (block1.0 changes the width: no identity block at full resolution)


def test_stream_layout_launch_choices_and_switches():
    """Which launches a layout tries: the defaults at 8192 windows, every switch of INFER_OPTIONS flipped alone (which fields move, and
    no others), and the image-count thresholds of the fused blocks."""
    import engine
    F, T = False, True
    default = _base_layout(8192)
    assert default.window_fused == (F, F, F, T, F, T, F, T) and default.rides == (F, F, T, F, F, F, T, F)
    assert (default.stream_fused, default.strip_fused, default.stream2_fused, default.strip2_fused) == ((F, F), (T, T), (F,), (T,))
    assert (default.stem_kept, default.strip_stem_rows, default.strips2_resident, default.tail_fused) == (T, T, T, T)
    none2 = dict.fromkeys(("k3", "H2", "W2", "band2", "Ht2", "shift2", "h2s", "n_strip2", "n_strip2_max", "img_t2", "img_s2", "stream2_base", "rows2"))
    off2 = dict(none2, stream2_fused=(), strip2_fused=(), strips2_resident=F, tail_fused=F)
    moves = {
        "stream_direct": dict(off2, mode="assembled", stream_row0=None, cat_rows=None),
        "stream_level2": dict(off2, mode="direct", cat_rows=4472866 - 90),       # (no spare rows for an odd phase)
        "stream_super": {},                                                       # (moves a layout with a run only: below)
        "strip_block_fused": dict(strip_fused=(F, F), strip_stem_rows=F),
        "small_block_fused": dict(window_fused=(F,) * 8, strip2_fused=(F,)),
        "tail_fused": dict(tail_fused=F),
        "strip2_resident": dict(strips2_resident=F),
        "strip_stem_shared": dict(stem_kept=F, strip_stem_rows=F),
        "f16_s2_shortcut_fused": dict(rides=(F,) * 8, strips2_resident=F),
    }
    assert sorted(moves) == sorted(engine.ResNetEngine.INFER_OPTIONS) == sorted(_INFER_ON)
    for flag, moved in moves.items():
        assert _base_layout(8192, **{flag: False}) == default._replace(**moved), flag
    with_run = _base_layout(8192, run=(16384, 8192))
    assert with_run.run == (16384, 8192) and with_run.stream_rows == 16483 and with_run.n_strip_max == default.n_strip
    assert _base_layout(8192, run=(16384, 8192), stream_super=False) == default
    # 64-channel strip blocks from 256 strips on (and with them the first block with the stem inside)
    a, b = _base_layout(165), _base_layout(166)
    assert (a.n_strip, b.n_strip) == (255, 256)
    assert (a.strip_fused, a.strip_stem_rows, b.strip_fused, b.strip_stem_rows) == ((F, F), F, (T, T), T) and a.stem_kept and b.stem_kept
    # 32-channel blocks of the level-2 strips from 512 strips on
    a, b = _base_layout(435), _base_layout(436)
    assert (a.n_strip2, b.n_strip2) == (511, 512) and (a.strip2_fused, b.strip2_fused) == ((F,), (T,))
    assert a.window_fused == b.window_fused == (F,) * 8
    # 16- / 32-channel blocks of the per-window levels from 512 windows on
    a, b = _base_layout(511), _base_layout(512)
    assert a.window_fused == (F,) * 8 and b.window_fused == (F, F, F, T, F, T, F, T)
    # the rules themselves
    blocks = engine.block_geometry(64, [64, 32, 16, 16], 100, 44, True)
    assert engine._tail_blocks_ok(blocks[4:]) and not engine._tail_blocks_ok(blocks[3:]) and not engine._tail_blocks_ok(blocks[5:])
    assert engine._block_fits_lds(blocks[0], 256, _INFER_ON, (10, 44)) and not engine._block_fits_lds(blocks[0], 256, _INFER_ON, (11, 44))
    assert not engine._block_fits_lds(blocks[0], 256, _INFER_ON) and not engine._block_fits_lds(blocks[2], 4096, _INFER_ON)
    assert [engine._s2_shortcut_rides(b, _INFER_ON) for b in (blocks[2], blocks[4], blocks[6])] == [T, F, T]


def test_stream_layout_regions_are_disjoint_and_inside_their_buffers():
    """In every layout above: cat = [strips][W + 2 zeroed rows behind a short group's strips][stream image][spare rows] and cat2 =
    [strips][zeroed rows][phase-0 stream][phase-1 stream][tail], in order, disjoint, inside cat_rows / rows2; and the last group of a
    run (d = S - B) reads its windows inside the stream image(s)."""
    seen = set()
    for lay in _all_layouts():
        seen.add(lay.mode)
        if lay.cat_rows is None:
            assert lay.mode in ("per_window", "assembled") and lay.stream_row0 is None and lay.rows2 is None
            continue
        Wp, (S, B_max) = lay.W + 1, lay.run or (lay.B, lay.B)
        assert lay.n_strip <= lay.n_strip_max and lay.B <= B_max and lay.n_strip_max == B_max + lay.H - lay.Ht
        strips_end = lay.n_strip * lay.img_t_rows
        zero_end = strips_end + lay.W + 2                     # what the last strip reads below itself
        stream_end = lay.stream_row0 + (lay.stream_rows + 1) * Wp + lay.W + 2   # the image with its border row and tail
        assert lay.stream_row0 == lay.n_strip_max * lay.img_t_rows and lay.stream_rows == S + lay.H - 1
        if lay.n_strip < lay.n_strip_max:
            assert zero_end <= lay.stream_row0                # a short group: the zeroed rows lie in front of the stream
        else:
            assert strips_end == lay.stream_row0              # else they ARE the stream's border row and the first of its rows
        spare = 2 * Wp if lay.mode == "shared2" else 0        # the odd phase reads the stream from its second row on
        assert 0 < strips_end <= lay.stream_row0 < stream_end and stream_end + spare == lay.cat_rows
        d = S - lay.B                                         # the run's last group: its last window's last row
        last_row = lay.stream_row0 + (d + lay.B - 1 + lay.H - 1) * Wp
        assert lay.stream_row0 + d * Wp + (lay.B + lay.H - 1) * Wp <= stream_end - (lay.W + 2) and last_row + Wp <= lay.cat_rows
        if lay.mode != "shared2":
            continue
        Wp2 = lay.W2 + 1
        assert lay.n_strip2 <= lay.n_strip2_max == B_max + lay.shift2 and d % 2 == 0 and lay.h2s == (lay.stream_rows + 1) // 2
        strips2_end = lay.n_strip2 * lay.img_t2
        assert lay.stream2_base == lay.n_strip2_max * lay.img_t2 and lay.img_s2 == (lay.h2s + 1) * Wp2
        if lay.n_strip2 < lay.n_strip2_max:
            assert strips2_end + lay.W2 + 2 <= lay.stream2_base
        else:
            assert strips2_end == lay.stream2_base
        assert lay.stream2_base + 2 * lay.img_s2 + lay.W2 + 2 == lay.rows2
        # window i = 2 j + phase of the group reads rows d / 2 + j .. + H2 of its phase image: the last window of either phase
        for phase in (0, 1):
            if lay.B > phase:
                j = (lay.B - 1 - phase) // 2
                assert (d // 2 + j + lay.H2) * Wp2 <= lay.img_s2
        # the odd-phase stream is the stride-2 block on the level-1 stream from its second row on: inside cat with the spare rows
        assert lay.stream_row0 + Wp + (lay.stream_rows + 1) * Wp + lay.W + 2 <= lay.cat_rows
    assert seen == {"per_window", "assembled", "direct", "shared2"}
