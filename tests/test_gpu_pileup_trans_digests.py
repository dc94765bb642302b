"""The single-pair inter-chromosomal pile-up (pileup.pileup_trans_records, a batch of one pair) against the bits of the
single-pair kernels it replaced: tests/golden/pileup_trans_pair_digests.json holds the SHA-256 of every output of
scripts/pileup_trans_digests.py's cases, written at the last commit that had those kernels.  Every case, every output; the
fixture is never regenerated from later code."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(os.path.join(ROOT, "scripts"))
import pileup_trans_digests as ptd                          # noqa: E402

pytestmark = pytest.mark.gpu

with open(os.path.join(ROOT, "tests", "golden", "pileup_trans_pair_digests.json")) as fh:
    GOLDEN = json.load(fh)
CASES = ptd.cases()


def test_the_cases_are_the_fixtures():
    assert [c[0] for c in CASES] and sorted(c[0] for c in CASES) == sorted(GOLDEN)
    for c in CASES:                                          # "enrich_sums" exactly where the window leaves room for the peak box
        assert set(GOLDEN[c[0]]) == set(("valid_rows", "valid_cols", "expected", "obs", "oe") + ptd.KEYS
                                        + (("enrich_sums",) if c[8] > ptd.PEAK else ())), c[0]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_every_output_has_the_bits_of_the_single_pair_kernels(case):
    got, want = ptd.digests(case), GOLDEN[case[0]]
    assert set(got) == set(want)
    assert {k: got[k] for k in sorted(got)} == {k: want[k] for k in sorted(want)}
