"""What the engine hands to liblad_hip.so, and what comes back, is what it was at the commit before every launch went through
_hip.launch: per case of tools/launch_digests.py (a fused train step at batch 4 under one changed option each, predict_windows in
both precisions and under one changed switch each, the per-label event counts) the SHA-256 of the recorded call sequence (entry
point, every value that is no pointer, NULL or not for every pointer) and of the bytes of the results.  The digests of
tests/golden/launch_parent.json were recorded from that commit on an MI355X, twice with the same outcome; the library and the
launches are the same, so no tolerance applies.  The largest launch is a group of 512 windows."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import launch_digests as rec  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = rec.cases()


@pytest.fixture(scope="module")
def golden():
    with open(rec.GOLDEN) as f:
        return json.load(f)


def test_every_case_has_a_recorded_digest(golden):
    assert set(CASES) == set(golden)
    # bit-identical paths share their results and the event counts share their launches: the pair tells every case apart
    assert len({(d["calls"], d["results"]) for d in golden.values()}) == len(golden)


@pytest.mark.parametrize("name", list(CASES))
def test_the_launches_and_the_results_are_the_parent_commits(name, golden):
    got, reached = rec.run(CASES[name])
    print(name, got, sorted(reached))
    assert got["calls"] == golden[name]["calls"]
    assert got["results"] == golden[name]["results"]


def test_the_cases_reach_the_try_and_fall_back_entry_points():
    """What the digests cover: the four entry points that may decline are tried, and every label asked for has its event pairs."""
    with rec.recording() as r:
        counts = dict(eval(rec.predict("fp16", {}, events=True, T=rec.T_LARGE, chunk=rec.CHUNK_LARGE)))
    print(counts)
    assert {"lad_f16_block_fwd_stem_rows", "lad_f16_conv_s2_strips_fwd", "lad_f16_tail_fwd"} <= {name for name, _ in r.calls}
    assert "lad_f16_block_fwd" in rec.run(CASES["predict/fp16/groups512/no_strip_stem_shared"])[1]
    assert sum(counts.values()) > 0
