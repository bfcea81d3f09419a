"""The host weight packers write what they wrote before they moved into conv_pack.cpp and were built from shared steps.

Every digest in tests/golden/conv_pack_sha256.json was recorded from a library built at the PARENT commit of that change
(tests/golden/make_conv_pack_golden.py TREE), never from the library under test.  The cases are tests/conv_pack_cases.py;
this test only recomputes and compares.
"""
import json
import os

import pytest

from read_amd import _lib
from tests import conv_pack_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rec():
    with open(os.path.join(ROOT, "tests", "golden", "conv_pack_sha256.json")) as f:
        return json.load(f)


def test_fixture_covers_every_case(rec):
    assert rec["seed"] == cases.SEED
    assert sorted(rec["sha256"]) == sorted([cases.case_id(c) for c in cases.CASES] + [f"params-cout{co}" for co in cases.PARAM_COUTS])


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_packer_output_is_bit_identical(rec, case):
    assert cases.pack_digest(_lib.lib(), case) == rec["sha256"][cases.case_id(case)]


@pytest.mark.parametrize("cout", cases.PARAM_COUTS)
def test_params_output_is_bit_identical(rec, cout):
    assert cases.params_digest(_lib.lib(), cout) == rec["sha256"][f"params-cout{cout}"]
