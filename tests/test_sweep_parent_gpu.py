"""The device half of tests/test_sweep_parent_cpu.py: the device forms of the three span families (the *_instances_device and
*_frame_spans_device of laugh_segmenter.py, sweep_eval.score_sweep_device with and without events= and lowpass=, evaluate_sweep.py
--scorer device, segment_laughter.load_and_pred with segmenter="device") return, write and refuse what they did at the commit
before they were put behind one Decoder record.  The cases are those of tools/sweep_digests.py (gpu_cases), the digests the "gpu"
part of tests/golden/sweep_parent.json, recorded from that commit on an MI355X.  The largest launch is 3 x 3000 frames x 64
settings."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import sweep_digests as rec  # noqa: E402

pytestmark = pytest.mark.gpu

PART = "gpu"
CASES = rec.gpu_cases()


@pytest.fixture(scope="module")
def golden():
    with open(rec.GOLDEN) as f:
        return json.load(f)[PART]


def test_every_case_has_a_recorded_digest(golden):
    assert set(CASES) == set(golden)
    assert len(set(golden.values())) == len(golden)


@pytest.mark.parametrize("name", list(CASES))
def test_the_result_is_the_parent_commits(name, golden):
    got = CASES[name]()
    if name.startswith("refusals/"):
        print(got)
    digest = rec.sha(got)
    print(name, digest)
    assert digest == golden[name]


def test_the_outputs_are_not_trivial():
    """What the digests cover: in every family some cells of the dictionaries are empty and some are not."""
    for family, (filled, cells) in rec.cell_counts(device=True).items():
        print(family, filled, cells)
        assert 0 < filled < cells, family
