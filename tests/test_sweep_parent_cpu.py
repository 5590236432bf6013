"""The sweep's Python layer after its three span families were put behind one Decoder record (laugh_segmenter.py, sweep_eval.py,
evaluate_sweep.py, segment_laughter.py): the host forms return, write and refuse what they did at the commit before the change.

tools/sweep_digests.py holds the cases, the seeded inputs and the serialisation; tests/golden/sweep_parent.json holds the SHA-256
digests recorded from that commit.  Dictionaries are compared with their key order and float reprs, the scripts by the bytes of
every file they write; the refusals are recorded as the exception's type and message."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import sweep_digests as rec  # noqa: E402

PART = "cpu"
CASES = rec.cpu_cases()


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
    for family, (filled, cells) in rec.cell_counts().items():
        print(family, filled, cells)
        assert 0 < filled < cells, family
