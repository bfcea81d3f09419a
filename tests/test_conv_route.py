"""The gated-conv dispatcher answers what it answered before it was rewritten around one routing function and one knob table.

Every expectation in tests/golden/conv_route.json was recorded from a library built at the PARENT commit of that change
(tests/golden/make_route_golden.py TREE), never from the library under test.  The sweep itself is tests/route_cases.py.
"""
import ctypes as C
import json
import os

import pytest

from read_amd import _lib
from tests import route_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The ONE permitted difference class of the outcome sweep.  The old launch_gated_conv ran the tile-table lookup and its checks for
# every launch, so a launch that a persistent F(4x4)-family / split-operand kernel takes (family 4, 5 or 6) was refused when the
# table's Winograd F(2x2) entry would have been the table's choice and ITS operand was misaligned — an operand the launch never
# reads.  Such a launch is now treated as the same launch with that operand aligned: the answer must be what the PARENT recorded
# for that sibling (variant 0 of the operand set: on this GPU-less machine READ_EHIP from the runtime, or a later refusal).
EXEMPT = {
    "wino_operand_of_a_kernel_not_taken": {
        "parent": [-22, "read_gated_conv_forward: config k3s1c16_p1q1_wino needs wpacked_wino"],
        "families": (4, 5, 6),
        "set": "operands",
        "variant": ((), ("wpacked_wino",)),
    },
}


@pytest.fixture(scope="module")
def rec():
    with open(os.path.join(ROOT, "tests", "golden", "conv_route.json")) as f:
        return json.load(f)


def _defaults_guard():
    """The sweeps assume the default tuning state: a library loaded with READ_TUNE / READ_CONV_WAVE would shift every record."""
    assert not os.environ.get("READ_TUNE") and not os.environ.get("READ_CONV_WAVE")


def test_route_table_matches_the_parent(rec):
    """read_conv_kernel_family over shapes x sources x modes x configs, operand presence / alignment and every routing knob."""
    _defaults_guard()
    sweep, total = rc.Sweep(_lib), 0
    for name, cases in sweep.sets():
        want = rc.unpack(rec["sets"], name, "family")
        got = [sweep.family(c) for c in cases]
        assert len(got) == rec["sets"][name]["n"] == len(want), name
        wrong = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
        assert not wrong, f"{name}: {len(wrong)} of {len(got)} families differ, first at case {wrong[0]}: {got[wrong[0]]} != {want[wrong[0]]}"
        total += len(got)
    assert total > 150000


def test_route_anchors():
    """The families the issue lists, all operands present (they are part of the record too; spelled out here to be readable)."""
    _defaults_guard()
    L = _lib.lib()
    for (cin, cout, k, s), by_config in (((64, 64, 3, 1), {-1: 5, -5: 4, -7: 5, -12: 5, -8: 6}), ((32, 3, 3, 1), {-1: 1}),
                                         ((64, 128, 3, 2), {-1: 6}), ((128, 64, 1, 1), {-1: 7}), ((24, 56, 1, 1), {-1: 0}),
                                         ((48, 64, 3, 1), {-1: 4, -7: 2})):
        for cfg, fam in by_config.items():
            d, _ = rc.make_desc(_lib, cin, cout, k, s, config=cfg)
            assert L.read_conv_kernel_family(C.byref(d)) == fam, (cin, cout, k, s, cfg)
    assert L.read_conv_kernel_family(None) == -1


def test_launch_outcomes_match_the_parent(rec):
    """(rc, message) of read_gated_conv_forward and read_gated_conv_forward_f4x1 for the same descriptors: refusals with their text,
    READ_EHIP by its code alone (its text carries file:line).  Fake pointers: skipped, before any descriptor is built, where a GPU
    is visible."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("the descriptors carry fake pointers: run on a machine without a GPU")
    _defaults_guard()
    sweep, outcomes, used, total = rc.Sweep(_lib), rec["outcomes"], {k: 0 for k in EXEMPT}, 0
    for name, cases in sweep.sets():
        fams = rc.unpack(rec["sets"], name, "family")
        want = {f: rc.unpack(rec["sets"], name, f) for f in ("forward", "forward_f4x1")}
        n = 0
        for i, case in enumerate(cases):
            for field, f4x1 in (("forward", False), ("forward_f4x1", True)):
                got, parent = list(sweep.outcome(case, f4x1)), outcomes[want[field][i]]
                if got == parent:
                    continue
                variants = rc.operand_variants()
                klass = [k for k, e in EXEMPT.items() if parent == e["parent"] and fams[i] in e["families"] and name == e["set"] and
                         variants[i % len(variants)] == e["variant"] and got == outcomes[want[field][i - i % len(variants)]]]
                assert klass, f"{name} case {i} ({field}): {got} but the parent answered {parent} (family {fams[i]})"
                used[klass[0]] += 1
            n += 1
        assert n == rec["sets"][name]["n"], name
        total += n
    # every exemption is of a named class, and the class is real (the record holds such refusals)
    assert used["wino_operand_of_a_kernel_not_taken"] > 0 and total > 150000
    print("exempted:", used, "of", 2 * total)


def test_tuning_keys_and_normalisation_match_the_parent(rec):
    _defaults_guard()
    L = _lib.lib()
    keys = rc.tuning_keys(_lib)
    # the record was taken while "unet_streams" was a key; it is retired since (tests/test_splat_knobs.py holds it to "unknown key")
    assert keys == [k for k in rec["tuning_keys"] if k != "unet_streams"]
    assert rec["knob_values"] == list(rc.KNOB_VALUES)
    table = rc.knob_table(_lib)
    assert table == rec["knobs"]
    assert rc.knob_table(_lib) == table                              # ... and the defaults came back
    v = C.c_int()
    for key in ("conv_nope", "conv_", "") + rc.RETIRED_KEYS:
        assert L.read_tuning_set(key.encode(), 1) == -22
        assert L.read_last_error().decode() == f"read_tuning_set: unknown key '{key}'"
        assert L.read_tuning_get(key.encode(), C.byref(v)) == -22
        assert L.read_last_error().decode() == f"read_tuning_get: unknown key '{key}'"
    assert L.read_tuning_key(-1) is None and L.read_tuning_key(len(keys)) is None


def test_plans_match_the_parent(rec):
    """read_unet_create_layout on the CPU for each layout at both sizes, default knobs and with the F(4x4) family switched off."""
    _defaults_guard()
    assert rc.plans(_lib) == rec["plans"]
    assert any(p[4] == -22 for p in rec["plans"]) and any(p[4] == 0 and p[6] == 105 for p in rec["plans"])
