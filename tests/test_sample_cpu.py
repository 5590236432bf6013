"""The segment sampler without a GPU: the model of the convention (tests/_sample_model.py) has the properties the convention
promises, and sampling.SegmentPools -- the host half of the product -- builds the regions and pools the brute-force
per-millisecond sets say it should.  The kernels are pinned to the model in tests/test_sample_gpu.py."""
import math

import numpy as np
import pytest

import _sample_model as sm
import _score_model
import sampling
import sweep_eval

N_MS = 70000
CASES = [(100, 100), (128, 128)]
PRESET = {"num_laugh_samples": 3, "num_non_laugh_samples": 10, "silence_share": 0.7, "noise_share": 0.1, "subsample_duration": 1.0,
          "random": False}
SEED = 5            # chosen so that the model passes the uniformity bounds (they are 4-sigma bounds: most seeds do)


@pytest.fixture(scope="module")
def world():
    rows, chans = sm.corpus()
    model = _score_model.Model(rows, chans, N_MS)
    sets = {}                                                   # (meeting, part) -> {class: bool per millisecond}
    for c in chans:
        m, p = c["meeting_id"], c["part_id"]
        d = {"invalid": model.get(model.invalid, m, p), "laugh": model.get(model.laugh, m, p), "speech": model.get(model.speech, m, p),
             "noise": model.get(model.noise, m, p), "silence": model.silence[m][p]}
        d["any"] = model.oc(0, _score_model.to_frames(c["length"])) & ~d["laugh"] & ~d["invalid"]
        sets[(m, p)] = d
    pools = {ft: sampling.SegmentPools.from_transcripts(rows, chans, *ft) for ft in CASES}
    return {"rows": rows, "chans": chans, "sets": sets, "pools": pools, "index": sweep_eval.TranscriptIndex(rows, chans)}


def _chan_index(pools, c):
    return pools.channels.index(sampling.channel_key(c["meeting_id"], c["chan"]))


@pytest.mark.parametrize("fps,T", CASES)
def test_frame_rule_matches_per_millisecond_membership(world, fps, T):
    pools = world["pools"][(fps, T)]
    for c in world["chans"]:
        ci = _chan_index(pools, c)
        frames_c = int(pools.frames[ci])
        assert frames_c == math.floor(c["length"] * fps)
        iv = world["index"].intervals(c["meeting_id"], c["chan"])
        for name in sweep_eval.CLASSES:
            want = sm.frames_inside(world["sets"][(c["meeting_id"], c["part_id"])][name], fps, frames_c)
            got = np.zeros(frames_c, bool)
            for lo, hi in iv[name]:
                a, b = sampling.frames_of(lo, hi, fps, frames_c)
                got[a:max(a, b)] = True
            assert np.array_equal(got, want), (c, name)
        # the measure pools of the meeting hold, for this channel, exactly the runs of >= T such frames
        for name in ("silence", "any"):
            want = [r for r in sm.runs(sm.frames_inside(world["sets"][(c["meeting_id"], c["part_id"])][name], fps, frames_c)) if r[1] - r[0] >= T]
            _, reg, total = pools.pool(c["meeting_id"], name)
            got = [(int(a), int(b)) for ch, a, b in reg if ch == ci]
            assert got == want, (c, name)
        assert all(int(b) <= pools.frames[ch] and 0 <= a < b for ch, a, b in pools.regions)


def _laugh_regions(world, pools, fps):
    """Per laugh row of the table, in order: its region by brute force, or None where it holds no whole frame."""
    out = []
    part_chan = {(c["meeting_id"], c["part_id"]): c for c in world["chans"]}
    for r in world["rows"]:
        if r["type"] != "laugh":
            continue
        ci = _chan_index(pools, part_chan[(r["meeting_id"], r["part_id"])])
        lo, hi = _score_model.to_frames(r["start"]), _score_model.to_frames(r["end"])
        rr = sm.runs(sm.frames_inside(sm.member_of([(lo, hi)] if hi > lo else [], N_MS), fps, int(pools.frames[ci])))
        assert len(rr) <= 1
        out.append((r, (ci,) + rr[0]) if rr else (r, None))
    return out


@pytest.mark.parametrize("fps,T", CASES)
def test_laugh_rows_become_fixed_regions(world, fps, T):
    pools = world["pools"][(fps, T)]
    want = _laugh_regions(world, pools, fps)
    kept = [g for _, g in want if g is not None]
    assert pools.dropped == len(want) - len(kept) and pools.dropped > 0
    assert [tuple(int(v) for v in pools.regions[j]) for _, j in pools.laugh_rows] == kept
    assert [m for m, _ in pools.laugh_rows] == [r["meeting_id"] for r, g in want if g is not None]


def _table(pools, n):
    """n rows of each kind / class: FIXED over the laugh regions, POOL_ROW speech and noise, POOL_MEASURE silence and any."""
    kind, src, what = [], [], []
    laugh = [j for _, j in pools.laugh_rows]
    for name, k in (("laugh", sm.FIXED), ("speech", sm.POOL_ROW), ("noise", sm.POOL_ROW), ("silence", sm.POOL_MEASURE), ("any", sm.POOL_MEASURE)):
        for i in range(n):
            m = pools.meetings[i % len(pools.meetings)]
            kind.append(k)
            src.append(laugh[i % len(laugh)] if name == "laugh" else pools.pool_index[(m, name)])
            what.append(name)
    return np.asarray(kind, np.int32), np.asarray(src, np.int32), what


@pytest.mark.parametrize("fps,T", CASES)
def test_draws_land_where_the_convention_says(world, fps, T):
    pools = world["pools"][(fps, T)]
    kind, src, what = _table(pools, 4096)
    cum, total = sm.pool_cum_of(pools.regions, pools.pool_off, T)
    assert np.array_equal(cum[:pools.pool_off[-1]], pools.pool_cum[:pools.pool_off[-1]]) and np.array_equal(total, pools.pool_total)
    chan, first, count, reg, _ = sm.draw(kind, src, pools.regions, pools.pool_off, cum, T, SEED, 0, detail=True)
    key_part = {sampling.channel_key(c["meeting_id"], c["chan"]): (c["meeting_id"], c["part_id"]) for c in world["chans"]}
    assert np.all(first >= 0) and np.all(first + count <= pools.frames[chan])
    for i in range(len(kind)):
        sets = world["sets"][key_part[pools.channels[chan[i]]]]
        lo, hi, f, n = int(pools.regions[reg[i], 1]), int(pools.regions[reg[i], 2]), int(first[i]), int(count[i])
        assert lo <= f and f + n <= hi
        assert n == min(T, hi - lo)
        cover = {k: sm.coverage_ms(sets[k], f, n, fps) for k in sweep_eval.CLASSES}
        h = sm.hull(f, n, fps)
        if what[i] == "silence":
            assert n == T and cover["silence"] == h[1] - h[0] and all(cover[k] == 0 for k in sweep_eval.CLASSES[:4])
        elif what[i] == "any":
            assert n == T and cover["laugh"] == 0 and cover["invalid"] == 0
        elif what[i] == "laugh":
            assert kind[i] == sm.FIXED and reg[i] == src[i]
    # every positive lies inside its laugh row, by the frame rule on the row's own milliseconds
    regions_of_rows = [(r, g) for r, g in _laugh_regions(world, pools, fps) if g is not None]
    for i in np.flatnonzero(kind == sm.FIXED):
        r, g = regions_of_rows[[j for _, j in pools.laugh_rows].index(int(src[i]))]
        lo_ms, hi_ms = _score_model.to_frames(r["start"]), _score_model.to_frames(r["end"])
        assert 1000 * int(first[i]) >= lo_ms * fps and 1000 * (int(first[i]) + int(count[i])) <= hi_ms * fps
        assert chan[i] == g[0]


@pytest.mark.parametrize("fps,T", CASES)
def test_draws_are_uniform(world, fps, T):
    pools = world["pools"][(fps, T)]
    n = 4096
    bound = lambda q: 4 * math.sqrt(q * (1 - q) / n)          # noqa: E731
    m = pools.meetings[0]
    for name in ("silence", "any"):
        p, reg, M = pools.pool(m, name)
        _, _, _, _, us = sm.draw(np.full(n, sm.POOL_MEASURE, np.int32), np.full(n, p, np.int32), pools.regions, pools.pool_off, pools.pool_cum, T,
                                 SEED, 0, detail=True)
        bins = np.bincount([u * 8 // M for u in us], minlength=8) / n
        sizes = np.bincount([u * 8 // M for u in range(M)], minlength=8) / M
        for b in range(8):
            assert abs(bins[b] - sizes[b]) <= bound(sizes[b]), (name, b, bins[b], sizes[b])
    for name in ("speech", "noise"):
        p, reg, _ = pools.pool(m, name)
        cnt = len(reg)
        _, _, _, rj, _ = sm.draw(np.full(n, sm.POOL_ROW, np.int32), np.full(n, p, np.int32), pools.regions, pools.pool_off, pools.pool_cum, T, SEED,
                                 1, detail=True)
        rel = rj - pools.pool_off[p]
        assert rel.min() >= 0 and rel.max() < cnt
        assert len(set(rel.tolist())) == cnt                     # every region of a small pool is drawn at least once
        bins = np.bincount(rel * 8 // cnt, minlength=8) / n
        sizes = np.bincount(np.arange(cnt) * 8 // cnt, minlength=8) / cnt
        for b in range(8):
            assert abs(bins[b] - sizes[b]) <= bound(sizes[b]), (name, b, bins[b], sizes[b])


def test_draws_are_a_function_of_seed_epoch_and_row_id(world):
    pools = world["pools"][(100, 100)]
    kind, src, _ = _table(pools, 64)
    args = (kind, src, pools.regions, pools.pool_off, pools.pool_cum, 100)
    a = sm.draw(*args, 7, 0)
    assert all(np.array_equal(x, y) for x, y in zip(a, sm.draw(*args, 7, 0)))
    assert not np.array_equal(a[1], sm.draw(*args, 7, 1)[1])
    assert not np.array_equal(a[1], sm.draw(*args, 8, 0)[1])
    assert not np.array_equal(a[1], sm.draw(*args, 7 + 2 ** 32, 0)[1])      # (the high half of the seed is part of the key)
    perm = np.random.default_rng(0).permutation(len(kind))
    b = sm.draw(kind[perm], src[perm], pools.regions, pools.pool_off, pools.pool_cum, 100, 7, 0, row_id=perm)
    assert all(np.array_equal(x[perm], y) for x, y in zip(a, b))


@pytest.mark.parametrize("random", [False, True])
def test_plan_counts_follow_the_floor_rule(world, random):
    pools = world["pools"][(100, 100)]
    preset = dict(PRESET, random=random, num_non_laugh_samples=13)
    plan = pools.plan(preset, pools.meetings)
    n_rows = len(pools.laugh_rows)
    n_sil, n_noise = math.floor(13 * 0.7), math.floor(13 * 0.1)
    assert (n_sil, n_noise) == (9, 1)
    n_neg = 13 * n_rows
    assert len(plan) == n_neg + 3 * n_rows
    assert np.all(plan.label[:n_neg] == 0) and np.all(plan.label[n_neg:] == 1)          # negatives first, then positives
    assert np.all(plan.kind[n_neg:] == sm.FIXED)
    assert plan.src[n_neg:].tolist() == [j for m in pools.meetings for mm, j in pools.laugh_rows if mm == m for _ in range(3)]
    per_row = plan.kind[:n_neg].reshape(n_rows, 13)
    srcs = plan.src[:n_neg].reshape(n_rows, 13)
    meetings = [mm for m in pools.meetings for mm, _ in pools.laugh_rows if mm == m]
    for i in range(n_rows):
        names = [pools.pool_names[s][1] for s in srcs[i]]
        assert {pools.pool_names[s][0] for s in srcs[i]} == {meetings[i]}
        if random:
            assert names == ["any"] * 13 and np.all(per_row[i] == sm.POOL_MEASURE)
        else:
            assert names == ["speech"] * 3 + ["noise"] * 1 + ["silence"] * 9
            assert per_row[i].tolist() == [sm.POOL_ROW] * 4 + [sm.POOL_MEASURE] * 9
    one = pools.plan(preset, pools.meetings[1:])
    assert set(one.meeting) == set(pools.meetings[1:])


def test_reference_preset():
    import config
    p = config.SAMPLING["reference"]
    assert p["random"] is False and p["subsample_duration"] == 1.0
    assert (p["silence_share"], p["noise_share"]) == (0.7, 0.1)
    assert p["num_laugh_samples"] >= 1 and p["num_non_laugh_samples"] >= 1


def test_an_empty_pool_of_a_requested_class_is_refused(world):
    rows = [r for r in world["rows"] if not (r["type"] == "noise" and r["meeting_id"] == "Bed002")]
    pools = sampling.SegmentPools.from_transcripts(rows, world["chans"], 100, 100)
    with pytest.raises(ValueError, match="Bed002.*noise"):
        pools.plan(PRESET, pools.meetings)
    assert len(pools.plan(PRESET, ["Bmr001"])) > 0                                       # the other meeting is fine
    assert len(pools.plan(dict(PRESET, random=True), pools.meetings)) > 0                # and `any` does not need the noise rows
    # a segment longer than every silence gap: the silence pool has measure 0
    long_pools = sampling.SegmentPools.from_transcripts(world["rows"], world["chans"], 100, 3000)
    with pytest.raises(ValueError, match="silence"):
        long_pools.plan(dict(PRESET, subsample_duration=30.0), long_pools.meetings)
    with pytest.raises(ValueError):
        pools.plan(dict(PRESET, subsample_duration=2.0), pools.meetings)                 # (not the pools' T)
    with pytest.raises(ValueError):
        sampling.SegmentPools.from_transcripts(rows, world["chans"], 100, 100, noise_pool="music")


def test_noise_pool_speech_reproduces_the_reference(world):
    a = world["pools"][(100, 100)]
    b = sampling.SegmentPools.from_transcripts(world["rows"], world["chans"], 100, 100, noise_pool="speech")
    for m in a.meetings:
        assert np.array_equal(b.pool(m, "noise")[1], a.pool(m, "speech")[1])
        assert np.array_equal(b.pool(m, "speech")[1], a.pool(m, "speech")[1])
        assert not np.array_equal(a.pool(m, "noise")[1], a.pool(m, "speech")[1])
        assert np.array_equal(b.pool(m, "silence")[1], a.pool(m, "silence")[1])


def test_table_keeps_regions_only_when_asked():
    import segments
    rows = [{"start": 1.0, "duration": 2.5, "sub_start": 1.7, "sub_duration": 1.0, "audio_path": "A/chan0.sph", "label": 1},
            {"start": 4.0, "duration": 0.4, "sub_start": 4.0, "sub_duration": 0.4, "audio_path": "A/chan1.sph", "label": 0},
            {"start": 9.0, "duration": 0.5, "sub_start": 8.9, "sub_duration": 1.0, "audio_path": "A/chan0.sph", "label": 0}]
    old = segments.table_from_rows(rows, frame_shift=0.01)
    assert old.region_first is None and old.region_frames is None and old.row_id is None
    assert old.shuffled(3).row_id is None and old.shard(0, 2).region_first is None
    t = segments.table_from_rows(rows, frame_shift=0.01, keep_regions=True)
    for name in ("channel", "first_frame", "n_frames", "label"):
        assert np.array_equal(getattr(t, name), getattr(old, name))
    assert t.region_first.tolist() == [100, 400, 890] and t.region_frames.tolist() == [250, 40, 100]   # the last one widened to its window
    assert t.row_id.tolist() == [0, 1, 2]
    s = t.shuffled(3)
    assert np.array_equal(s.first_frame, t.first_frame[s.row_id]) and np.array_equal(s.region_first, t.region_first[s.row_id])
    assert np.array_equal(s.first_frame, old.shuffled(3).first_frame)
    assert s.shard(1, 2).row_id.tolist() == s.row_id[2:].tolist()
