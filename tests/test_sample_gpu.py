"""GPU tests of the segment sampler (csrc/sample.hip) against the Python-integer model of the convention (tests/_sample_model.py),
then through sampling.py, datasets.LadDataset, load_data, train.py and create_data_df.py.  Every comparison is of integers (or of
the bits of gathered features) and exact.  The model's tables are computed once per geometry and shared."""
import csv
import ctypes
import functools
import json

import numpy as np
import pytest
import torch

import _sample_model as sm

pytestmark = pytest.mark.gpu

GEOMETRIES = ((100, 100), (128, 128))       # (fps, T)
N_ROWS = (1, 257, 70000)                    # 70,000: past the kernel's fixed grid of 65,536 lanes
SEEDS = (23, 0x1234567890)                  # the second: above 2^32 (both halves of the key)
PRESET = {"num_laugh_samples": 2, "num_non_laugh_samples": 10, "silence_share": 0.7, "noise_share": 0.1, "subsample_duration": 1.0,
          "random": False}
PAD = -23.025850929940457


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _case(T):
    """Channels of 5 T + 7, 3 T, T and 2 T + 1 frames.  Pools: 0 a row pool with regions shorter than T, of exactly T, longer, and one
    that ends on its channel's last frame; 1 a row pool of one region; 2 a measure pool (a region of exactly T among them, one
    ending on the channel's last frame); 3 a measure pool of one region of exactly T frames: M = 1.  Then the FIXED regions."""
    frames = (5 * T + 7, 3 * T, T, 2 * T + 1)
    pools = [[(0, 3, 3 + T // 3), (0, T, 2 * T), (1, 0, 3 * T), (3, T + 2, 2 * T + 1), (0, 17, 18)],
             [(1, 5, 2 * T)],
             [(0, 0, T), (0, 2 * T, 5 * T + 7), (1, T // 2, 3 * T), (3, 0, 2 * T + 1)],
             [(2, 0, T)]]
    fixed = [(0, 7, 7 + T - 1), (1, T, 2 * T), (0, 4 * T, 5 * T + 7), (3, 0, 2 * T + 1), (2, 0, T), (1, 11, 12)]
    regions = np.asarray([g for p in pools for g in p] + fixed, np.int32)
    pool_off = np.concatenate([[0], np.cumsum([len(p) for p in pools])]).astype(np.int32)
    cum, total = sm.pool_cum_of(regions, pool_off, T)
    assert total[3] == 1
    n = max(N_ROWS)
    rng = np.random.default_rng(T)
    kind = rng.integers(0, 3, n).astype(np.int32)
    src = np.where(kind == sm.FIXED, pool_off[-1] + rng.integers(0, len(fixed), n),
                   np.where(kind == sm.POOL_ROW, rng.integers(0, 2, n), 2 + rng.integers(0, 2, n))).astype(np.int32)
    kind[:3], src[:3] = (0, 1, 2), (pool_off[-1], 0, 3)
    return dict(frames=frames, regions=regions, pool_off=pool_off, cum=cum, total=total, kind=kind, src=src, T=T,
                perm=np.random.default_rng(T + 1).permutation(n).astype(np.int64) + 2 ** 33)     # row ids above 2^32 too


@functools.lru_cache(maxsize=None)
def _model(T, seed, permuted):
    c = _case(T)
    return sm.draw(c["kind"], c["src"], c["regions"], c["pool_off"], c["cum"], T, seed, 3, row_id=c["perm"] if permuted else None, detail=True)[:4]


def _i32p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def _call(c, n, seed, epoch, row_id=None, host=True, kind=None, src=None, T=None, total=None, pool_off_host=None):
    """lad_sample_segments on the first n rows of the case -> (rc, chan, first, count, region) as numpy."""
    import _hip
    kind = np.ascontiguousarray(c["kind"][:n] if kind is None else kind)
    src = np.ascontiguousarray(c["src"][:n] if src is None else src)
    total = np.ascontiguousarray(c["total"] if total is None else total, dtype=np.int64)
    off_host = np.ascontiguousarray(c["pool_off"] if pool_off_host is None else pool_off_host, dtype=np.int32)
    d = [_dev(kind), _dev(src), _dev(c["regions"].reshape(-1)), _dev(c["pool_off"]), _dev(c["cum"])]
    rid = _dev(row_id[:n]) if row_id is not None else None
    out = [torch.full((n,), -7, dtype=dt, device="cuda") for dt in (torch.int32, torch.int64, torch.int32, torch.int32)]
    rc = _hip.lib().lad_sample_segments(_hip.ptr(d[0]), _hip.ptr(d[1]), n, _hip.ptr(rid), _hip.ptr(d[2]), len(c["regions"]), _hip.ptr(d[3]),
                                        _hip.ptr(d[4]), len(c["pool_off"]) - 1, _i32p(kind) if host else None, _i32p(src) if host else None,
                                        _i32p(off_host), total.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), c["T"] if T is None else T,
                                        seed, epoch, *(_hip.ptr(t) for t in out), _hip.stream_handle())
    torch.cuda.synchronize()
    return (rc,) + tuple(t.cpu().numpy() for t in out)


@pytest.mark.parametrize("permuted", [False, True])
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n", N_ROWS)
@pytest.mark.parametrize("fps,T", GEOMETRIES)
def test_sample_segments_equals_model(fps, T, n, seed, permuted):
    c = _case(T)
    want = _model(T, seed, permuted)
    rc, chan, first, count, region = _call(c, n, seed, 3, row_id=c["perm"] if permuted else None, host=(n != 257))
    assert rc == 0
    assert np.array_equal(chan, want[0][:n]) and np.array_equal(first, want[1][:n]) and np.array_equal(count, want[2][:n])
    assert np.array_equal(region, want[3][:n])
    assert np.all(first + count <= np.asarray(c["frames"])[chan]) and np.all(first >= 0)
    if n == max(N_ROWS):
        k = c["kind"]
        short = c["regions"][region, 2] - c["regions"][region, 1] < T
        assert short.any() and np.array_equal(count[short], (c["regions"][region, 2] - c["regions"][region, 1])[short])
        assert np.all(first[(k == sm.POOL_MEASURE) & (c["src"] == 3)] == 0)                    # M = 1: the one window
        assert np.any(first + count == np.asarray(c["frames"])[chan])                          # a window on a channel's last frame
        other = _call(c, n, seed, 4, row_id=c["perm"] if permuted else None, host=False)
        assert not np.array_equal(other[2], first)                                             # another epoch: another table


def test_draw_table_and_permutation():
    """sampling.DrawTable is the same launch; a permuted row_id permutes the table."""
    import sampling
    T = 100
    c = _case(T)
    n = 4099
    want = _model(T, SEEDS[0], False)
    t = sampling.DrawTable(c["kind"][:n], c["src"][:n], c["regions"], c["pool_off"], c["cum"], c["total"], T)
    got = [x.cpu().numpy() for x in t.draw(SEEDS[0], 3, region=True)]
    assert all(np.array_equal(g, w[:n]) for g, w in zip(got, want))
    perm = np.random.default_rng(9).permutation(n)
    p = sampling.DrawTable(c["kind"][:n][perm], c["src"][:n][perm], c["regions"], c["pool_off"], c["cum"], c["total"], T, row_id=perm)
    out = (torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int64, device="cuda"),
           torch.empty(n, dtype=torch.int32, device="cuda"))
    assert p.draw(SEEDS[0], 3, out=out)[1] is out[1]
    assert all(np.array_equal(o.cpu().numpy(), w[:n][perm]) for o, w in zip(out, want))


def test_bad_inputs_are_refused_before_any_launch():
    import _hip
    import sampling
    T = 100
    c = _case(T)
    n = 64
    bad_src = c["src"][:n].copy()
    bad_src[5] = len(c["regions"]) if c["kind"][5] == sm.FIXED else len(c["pool_off"]) - 1
    bad_kind = c["kind"][:n].copy()
    bad_kind[9] = 3
    big = c["total"].copy()
    big[2] = 2 ** 32
    off = c["pool_off"].copy()
    off[2] = off[1] - 1
    for kw in (dict(src=bad_src), dict(kind=bad_kind), dict(T=0), dict(total=big), dict(pool_off_host=off)):
        rc, chan, first, count, region = _call(c, n, 1, 0, **kw)
        assert rc == _hip.LAD_ERR_INVALID, kw
        assert _hip.lib().lad_last_error().decode().startswith("lad_sample_segments")
        assert np.all(chan == -7) and np.all(first == -7) and np.all(count == -7)              # nothing was written
    args = (c["regions"], c["pool_off"], c["cum"], c["total"])
    for kind, src, rest, T_ in ((c["kind"][:n], bad_src, args, T), (bad_kind, c["src"][:n], args, T), (c["kind"][:n], c["src"][:n], args, 0),
                                (c["kind"][:n], c["src"][:n], args[:3] + (big,), T)):
        with pytest.raises(ValueError):
            sampling.DrawTable(kind, src, *rest, T_)
    empty = np.asarray([0, 0, 1], np.int32)                                                    # pool 0 is empty
    with pytest.raises(ValueError, match="empty pool"):
        sampling.DrawTable([1], [0], [(0, 0, 50)], empty, [0], [0, 0], T)
    with pytest.raises(ValueError, match="measure 0"):
        sampling.DrawTable([2], [1], [(0, 0, 50)], empty, [0], [0, 0], T)


# ---- transcript coverage ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _corpus():
    import sweep_eval
    rows, chans = sm.corpus()
    chans = chans + [{"meeting_id": "Bmr001", "part_id": "", "chan": "chanX", "length": 60.0}]   # no participant: five empty sets
    return rows, chans, sweep_eval.TranscriptIndex(rows, chans)


@pytest.mark.parametrize("fps", [100, 128])
def test_window_coverage_equals_coverage_differences(fps):
    import sampling
    import sweep_eval
    rows, chans, index = _corpus()
    channels = [(c["meeting_id"], c["chan"]) for c in chans]
    rng = np.random.default_rng(fps)
    n = 2000
    chan = rng.integers(0, len(channels), n).astype(np.int32)
    first = rng.integers(0, 60 * fps, n).astype(np.int64)
    count = rng.integers(0, 3 * fps, n).astype(np.int32)
    count[::9] = 0
    first[::50] += 70 * fps                                     # past the last interval of every set
    first[1], count[1] = 0, 64 * fps                            # the whole channel
    got = sampling.window_coverage(index, channels, _dev(chan), _dev(first), _dev(count), fps).cpu().numpy()
    assert got.shape == (n, 5) and got.dtype == np.int32
    hulls = np.asarray([sm.hull(f, k, fps) for f, k in zip(first, count)], np.int64)
    sets = [index.intervals(*mc) for mc in channels]
    for s, name in enumerate(sweep_eval.CLASSES):
        want = np.zeros(n, np.int64)
        for ci in range(len(channels)):
            sel = chan == ci
            iv = sets[ci][name] if sets[ci] is not None else sweep_eval._EMPTY
            want[sel] = sweep_eval.coverage(iv, hulls[sel, 1]) - sweep_eval.coverage(iv, hulls[sel, 0])
        assert np.array_equal(got[:, s], want), name
    assert got[chan == len(channels) - 1].max() == 0 and got.max() > 0
    laugh = [[sets[ci]["laugh"] if sets[ci] is not None else sweep_eval._EMPTY] for ci in range(len(channels))]
    one = sampling.window_coverage(laugh, channels, _dev(chan), _dev(first), _dev(count), fps).cpu().numpy()       # S = 1
    assert one.shape == (n, 1) and np.array_equal(one[:, 0], got[:, 1])


@pytest.mark.parametrize("fps", [100, 128])
def test_whole_track_labels_on_the_device(fps):
    import segments
    rows, chans, index = _corpus()
    for c in chans[:2]:
        laugh = [(int(a), int(b)) for a, b in index.intervals(c["meeting_id"], c["chan"])["laugh"]]
        n_frames = int(c["length"] * fps) + 3
        key = f"{c['meeting_id']}/{c['chan']}.sph"
        host = segments.whole_track_table(n_frames, key, laugh, frame_shift=1.0 / fps)
        dev = segments.whole_track_table(n_frames, key, laugh, frame_shift=1.0 / fps, device="cuda")
        via_index = segments.whole_track_table(n_frames, key, frame_shift=1.0 / fps, index=index, device="cuda")
        assert 0 < host.label.sum() < len(host)
        for t in (dev, via_index):
            assert np.array_equal(t.label, host.label) and np.array_equal(t.first_frame, host.first_frame)
            assert np.array_equal(t.n_frames, host.n_frames) and t.channels == host.channels and t.label.dtype == host.label.dtype


# ---- LadDataset ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _store_and_table():
    """Three channels of random features (the store lists them in another order than the table) and a table of 203 rows with
    regions: shorter than a segment, of exactly a segment, long, and one that ends on its channel's last frame."""
    import datasets
    import segments
    rng = np.random.default_rng(4)
    frames = {"A/chan0.sph": 1200, "A/chan1.sph": 900, "B/chan2.sph": 400}
    store = datasets.FeatureStore()
    for k in ("B/chan2.sph", "A/chan0.sph", "A/chan1.sph"):
        store.add_features(k, (3.0 * rng.standard_normal((frames[k], 44)) - 6.0).astype(np.float32))
    keys = list(frames)
    rows = []
    for i in range(203):
        key = keys[i % 3]
        total = frames[key] / 100.0
        dur = (0.37, 1.0, 2.5, 4.0)[(i // 3) % 4]
        start = round(float(rng.uniform(0, total - dur)), 2)
        if i == 5:
            start = round(total - dur, 2)                         # ends on the channel's last frame
        sub_dur = min(dur, 1.0)
        sub = round(float(rng.uniform(start, max(start, start + dur - sub_dur))), 2)
        rows.append({"start": start, "duration": dur, "sub_start": sub, "sub_duration": sub_dur, "audio_path": key, "label": i % 2})
    return store, rows, segments.table_from_rows(rows, frame_shift=0.01, keep_regions=True), segments.table_from_rows(rows, frame_shift=0.01)


def _batches(ds, batch=64):
    return [ds[list(range(s, min(s + batch, len(ds))))] for s in range(0, len(ds), batch)]


def _same(a, b):
    return all(torch.equal(x[k], y[k]) for x, y in zip(a, b) for k in ("inputs", "input_lens", "is_laugh")) and len(a) == len(b)


def _window_model(store, table, seed, epoch):
    """The model's draw for redraw='window' -> the gathered batch of the whole table."""
    import datasets
    remap = np.asarray([store.index_of(k) for k in table.channels], np.int32)
    regions = np.stack([remap[table.channel], table.region_first, table.region_first + table.region_frames], axis=1)
    n = len(table)
    chan, first, count = sm.draw(np.zeros(n, np.int32), np.arange(n), regions, np.zeros(1, np.int32), np.zeros(n, np.int64), 100, seed, epoch,
                                 row_id=table.row_id)
    return datasets.gather_segments(store, _dev(chan), _dev(first), _dev(count), 100, PAD), count


def test_off_is_off_and_regions_equal_to_windows_change_nothing():
    import datasets
    import segments
    store, rows, table, old = _store_and_table()
    assert old.region_first is None
    remap = np.asarray([store.index_of(k) for k in old.channels], np.int32)
    parent = datasets.gather_segments(store, _dev(remap[old.channel]), _dev(old.first_frame), _dev(old.n_frames), 100, PAD)
    plain = datasets.LadDataset(store, old)
    assert plain.redraw is None and plain._draw_table is None
    got = plain[list(range(len(old)))]
    assert torch.equal(got["inputs"], parent) and torch.equal(got["is_laugh"].cpu(), torch.from_numpy(old.label))
    plain.set_epoch(3)
    assert torch.equal(plain[list(range(len(old)))]["inputs"], parent)
    assert _same(_batches(datasets.LadDataset(store, table)), _batches(plain))                 # regions carried along, not used
    tight = segments.SegmentTable(table.channel, table.first_frame, table.n_frames, table.label, table.channels, 100,
                                  region_first=table.first_frame.copy(), region_frames=table.n_frames.astype(np.int64), row_id=table.row_id)
    ds = datasets.LadDataset(store, tight, redraw="window", redraw_seed=11)
    for e in (0, 5):
        ds.set_epoch(e)
        assert _same(_batches(ds), _batches(plain))
    with pytest.raises(ValueError, match="regions"):
        datasets.LadDataset(store, old, redraw="window")
    with pytest.raises(ValueError):
        datasets.LadDataset(store, table, redraw="rows")


def test_window_redraw_equals_model_whatever_the_order_or_the_rank():
    import datasets
    store, rows, table, old = _store_and_table()
    seed = SEEDS[1]
    ds = datasets.LadDataset(store, table, redraw="window", redraw_seed=seed)
    shuffled = table.shuffled(2)
    ds_shuffled = datasets.LadDataset(store, shuffled, redraw="window", redraw_seed=seed)
    everything = list(range(len(table)))
    per_epoch = []
    for e in (0, 1):
        want, count = _window_model(store, table, seed, e)
        ds.set_epoch(e)
        got = ds[everything]
        assert torch.equal(got["inputs"], want) and np.array_equal(got["input_lens"].cpu().numpy(), count)
        assert np.all(count == np.minimum(100, table.region_frames))
        ds_shuffled.set_epoch(e)
        assert torch.equal(ds_shuffled[everything]["inputs"], want[_dev(shuffled.row_id)])     # the draw follows the row, not its place
        for rank in range(4):                                                                  # table sharding: world = 4
            part = shuffled.shard(rank, 4)
            dr = datasets.LadDataset(store, part, redraw="window", redraw_seed=seed)
            dr.set_epoch(e)
            assert torch.equal(dr[list(range(len(part)))]["inputs"], want[_dev(part.row_id)])
        per_epoch.append(want)
    assert not torch.equal(per_epoch[0], per_epoch[1])
    # the loader's round-robin dealing of one full table: a rank's batches are those rows of the single-rank table
    import load_data
    ds.set_epoch(1)
    for rank in range(4):
        for idx in load_data.SegmentSampler(len(table), max_cuts=16, rank=rank, world=4, min_batch=2):
            assert torch.equal(ds[idx]["inputs"], per_epoch[1][_dev(np.asarray(idx, np.int64))])


def test_redraw_with_augmentation_is_reproducible():
    import augment
    import datasets
    store, rows, table, old = _store_and_table()
    runs = []
    for _ in range(2):
        ds = datasets.LadDataset(store, table, augment=augment.from_preset("spec", 7), redraw="window", redraw_seed=7)
        out = []
        for e in (0, 1):
            ds.set_epoch(e)
            out.append(ds[list(range(len(table)))]["inputs"].clone())
        runs.append(out)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(*runs))
    assert not torch.equal(runs[0][0], runs[0][1])
    plain = datasets.LadDataset(store, table, redraw="window", redraw_seed=7)
    plain.set_epoch(0)
    assert not torch.equal(plain[list(range(len(table)))]["inputs"], runs[0][0])               # (it was augmented)


def _synthetic_corpus(root, seconds=12):
    """Two meetings of two channels each as audio + transcript rows with room for every class; returns (rows, channels)."""
    import synth
    from scipy.io import wavfile
    clips = synth.make_clips(4, n_samples=16000 * seconds, seed=78).cpu().numpy()
    rows, chans = [], []
    for mi, m in enumerate(("Btr001", "Bdv002")):
        (root / m).mkdir(parents=True, exist_ok=True)
        for ci in range(2):
            part, chan = f"p{mi}{ci}", f"chan{ci}"
            wavfile.write(root / m / f"{chan}.wav", 16000, (np.clip(clips[2 * mi + ci], -1, 1) * 32767).astype(np.int16))
            chans.append({"meeting_id": m, "part_id": part, "chan": chan, "length": float(seconds)})
            shift = 0.13 * ci
            for kind, spans in (("laugh", [(1.0, 2.2), (6.0, 6.5), (10.2, 10.204)]), ("speech", [(3.0, 4.5), (7.7, 8.9)]),
                                ("noise", [(5.0, 5.4)]), ("invalid", [(9.9, 10.1)])):
                for a, b in spans:
                    rows.append({"meeting_id": m, "part_id": part, "chan": chan, "start": round(a + shift, 3), "end": round(b + shift, 3),
                                 "length": round(b - a, 3), "type": kind, "laugh_type": "laugh" if kind == "laugh" else ""})
    return rows, chans


def test_sampler_dataset_equals_model_and_create_data_df_round_trip(tmp_path, monkeypatch):
    import config
    import create_data_df
    import datasets
    import sampling
    import segments
    monkeypatch.setitem(config.FEAT, "num_samples", 100)
    rows, chans = _synthetic_corpus(tmp_path / "audio")
    pools = sampling.SegmentPools.from_transcripts(rows, chans, 100, 100)
    assert pools.dropped == 4                                                                  # the 4 ms laughs hold no whole frame
    plan = pools.plan(PRESET, pools.meetings)
    sampler = sampling.Sampler(pools, plan, SEEDS[1])
    want = {e: sm.draw(plan.kind, plan.src, pools.regions, pools.pool_off, pools.pool_cum, 100, SEEDS[1], e) for e in (0, 1)}
    chan, first, count, label = sampler.draw(1)
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip((chan, first, count), want[1]))
    assert np.array_equal(label.cpu().numpy(), plan.label)
    # a dataset over a store that lists the channels in another order, rows permuted
    rng = np.random.default_rng(1)
    store = datasets.FeatureStore()
    for k in reversed(pools.channels):
        store.add_features(k, (3.0 * rng.standard_normal((int(pools.frames[pools.channels.index(k)]), 44)) - 6.0).astype(np.float32))
    perm = rng.permutation(len(plan))
    taken = sampler.take(perm)
    ds = datasets.LadDataset(store, taken.table(0), redraw=taken)
    remap = np.asarray([store.index_of(k) for k in pools.channels], np.int32)
    for e in (0, 1):
        ds.set_epoch(e)
        got = ds[list(range(len(plan)))]
        ref = datasets.gather_segments(store, _dev(remap[want[e][0]][perm]), _dev(want[e][1][perm]), _dev(want[e][2][perm]), 100, PAD)
        assert torch.equal(got["inputs"], ref) and np.array_equal(got["is_laugh"].cpu().numpy(), plan.label[perm])
    with pytest.raises(ValueError):
        datasets.LadDataset(store, sampler.take(perm[:-1]).table(0), redraw=taken)
    # create_data_df: the CSV gives the draw back, and the reference's asserts hold on it
    splits = {"train": ["Btr001"], "dev": ["Bdv002"]}
    written, dropped = create_data_df.create_data_df(rows, chans, splits, str(tmp_path / "dfs"), preset=PRESET, seed=23, epoch=2)
    assert dropped == 4
    for split, meetings in splits.items():
        p = pools.plan(PRESET, meetings)
        w = sm.draw(p.kind, p.src, pools.regions, pools.pool_off, pools.pool_cum, 100, 23, 2)
        t = segments.table_from_csv(str(tmp_path / "dfs" / f"{split}_df.csv"), frame_shift=0.01, keep_regions=True)
        assert written[split] == len(p) == len(t) > 0
        assert [t.channels[c] for c in t.channel] == [pools.channels[c] for c in w[0]]
        assert np.array_equal(t.first_frame, w[1]) and np.array_equal(t.n_frames, w[2]) and np.array_equal(t.label, p.label)
        assert np.all(t.region_first <= t.first_frame) and np.all(t.first_frame + t.n_frames <= t.region_first + t.region_frames)
        with open(tmp_path / "dfs" / f"{split}_df.csv", newline="") as f:
            recs = list(csv.DictReader(f))
        assert list(recs[0]) == sampling.COLUMNS
        for r in recs:
            assert min(float(r[k]) for k in ("start", "duration", "sub_start", "sub_duration")) >= 0
            assert r["label"] in ("0", "1") and r["meeting_id"] in meetings and r["audio_path"].split("/")[0] in meetings
            assert r["audio_path"] == f"{r['meeting_id']}/{r['chan_id']}.sph"


def _write_tables(tmp_path, rows, chans):
    for name, cols, recs in (("transcripts.csv", ["meeting_id", "part_id", "chan", "start", "end", "length", "type", "laugh_type"], rows),
                             ("channels.csv", ["meeting_id", "part_id", "chan", "length"], chans)):
        with open(tmp_path / name, "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=cols)
            w.writeheader()
            w.writerows(recs)


@pytest.mark.parametrize("mode", ["window", "transcripts"])
def test_train_script_with_redraw(tmp_path, capsys, monkeypatch, mode):
    """train.py --redraw on a synthetic corpus: finite losses, the training table is redrawn, the dev batches are bit-equal to those
    of a loader built without redraw."""
    import config
    import create_data_df
    import load_data
    import train
    monkeypatch.setitem(config.FEAT, "num_samples", 100)
    root = tmp_path / "data"
    rows, chans = _synthetic_corpus(root)
    _write_tables(tmp_path, rows, chans)
    (tmp_path / "splits.json").write_text(json.dumps({"train": ["Btr001"], "dev": ["Bdv002"]}))
    create_data_df.main(["--transcripts", str(tmp_path / "transcripts.csv"), "--channels", str(tmp_path / "channels.csv"), "--splits",
                         str(tmp_path / "splits.json"), "--out_dir", str(root / "data_dfs")])
    made = []
    orig = load_data.create_training_dataloader

    def spy(*a, **kw):
        made.append(orig(*a, **kw))
        return made[-1]
    monkeypatch.setattr(load_data, "create_training_dataloader", spy)
    ck = tmp_path / "ck"
    extra = ["--transcripts", str(tmp_path / "transcripts.csv"), "--channels", str(tmp_path / "channels.csv")] if mode == "transcripts" else []
    train.main(["--config", "resnet_base", "--checkpoint_dir", str(ck), "--data_root", str(root), "--batch_size", "16", "--log_frequency", "1",
                "--max_steps", "3", "--seed", "5", "--redraw", mode, "--redraw_seed", "9"] + extra)
    monkeypatch.undo()
    assert f"Redraw: {mode} (seed 9)" in capsys.readouterr().out
    with open(ck / "metrics.csv") as f:
        table = list(csv.reader(f))
    losses = [float(r[5]) for r in table[1:]] + [float(r[9]) for r in table[1:]]
    assert len(table) == 4 and all(np.isfinite(losses))
    dev, trn = made
    assert dev.dataset.redraw is None and trn.dataset.redraw is not None and trn.dataset._draw_seed == 9
    data_dir = str(root / "data_dfs")
    plain_dev = orig(data_dir, "dev", shuffle=True, seed=5, batch_size=16, audio_root=str(root))
    pairs = list(zip(dev, plain_dev))
    assert len(pairs) >= 1 and all(torch.equal(x["inputs"], y["inputs"]) and torch.equal(x["is_laugh"], y["is_laugh"]) for x, y in pairs)
    before = trn.dataset._first.clone()
    trn.dataset.set_epoch(1)
    assert not torch.equal(before, trn.dataset._first)                                         # epoch 0 (the run's) against epoch 1
    frames = torch.tensor([m.shape[0] for m in trn.dataset.store.mats], device="cuda")
    assert bool(torch.all(trn.dataset._first + trn.dataset._count <= frames[trn.dataset._chan.long()]))
    with pytest.raises(ValueError, match="training split"):
        orig(data_dir, "dev", audio_root=str(root), redraw="window")
    with pytest.raises(SystemExit):
        train.main(["--config", "resnet_base", "--checkpoint_dir", str(ck), "--data_root", str(root), "--redraw", "transcripts"])
