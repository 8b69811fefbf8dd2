"""The cell-sorted gather backward (cell_gather.hpp) and the operators around it give the bits they gave before the three operators
came to share it: every forward result and every gradient of tests/cell_gather_cases.py has the SHA-256 that
tests/golden/gen_cell_gather_bits.py recorded from the library of the commit before.  The order of every sum is a contract
(DESIGN.md §6i); the fp64 bounds of the operators' own tests would not notice a changed one.  Digests are exact: no tolerance."""
import json
import os

import pytest

from tests import cell_gather_cases

pytestmark = pytest.mark.gpu
WANT = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cell_gather_bits.json")))


@pytest.fixture(scope="module")
def got(cuda):
    return cell_gather_cases.digests(cuda)


def test_the_same_cases_were_recorded(got):
    assert set(got) == set(WANT) and len(WANT) == 21
    for case in WANT:
        assert set(got[case]) == set(WANT[case]), case


@pytest.mark.parametrize("case", sorted(WANT))
def test_bits_equal_the_recorded_ones(got, case):
    differ = [k for k in WANT[case] if got[case][k] != WANT[case][k]]
    assert not differ, "%s: %s changed" % (case, ", ".join(differ))
