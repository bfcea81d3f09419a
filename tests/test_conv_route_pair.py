"""Config -13 (f4x1_pair_conv_kernel, two resident workgroups per CU) is accepted and refused exactly where config -12
(gated_conv_f4x1h_kernel) is: same family, same return code, the same refusal text but for the config's number.  Swept over the
anchor shapes of tests/route_cases.py with every operand absent, misaligned or alone.  Fake pointers: the launch half is skipped where
a GPU is visible (tests/route_cases.py)."""
import ctypes as C
import itertools

import pytest

from read_amd import _lib
from tests import route_cases as rc

PAIR, F4X1 = -13, -12
MODES = ("plain", "linear", "mul", "residual")


def _cases():
    for (cin, cout, k, s), mode, (absent, mis) in itertools.product(rc.ANCHOR_SHAPES, MODES, rc.operand_variants()):
        yield (cin, cout, k, s, mode, absent, mis), [rc.make_desc(_lib, cin, cout, k, s, "one", mode, cfg, absent, mis) for cfg in (F4X1, PAIR)]


def test_pair_config_reports_the_family_of_config_12():
    L, n5 = _lib.lib(), 0
    for key, (one, two) in _cases():
        f1, f2 = L.read_conv_kernel_family(C.byref(one[0])), L.read_conv_kernel_family(C.byref(two[0]))
        assert f1 == f2, (key, f1, f2)
        n5 += f2 == 5
    assert n5 > 0
    d, _ = rc.make_desc(_lib, 64, 64, 3, 1, config=PAIR)
    assert L.read_conv_kernel_family(C.byref(d)) == 5
    d, _ = rc.make_desc(_lib, 32, 32, 3, 1, config=PAIR)
    assert L.read_conv_kernel_family(C.byref(d)) == 5


def test_pair_config_is_accepted_and_refused_as_config_12():
    import torch
    if torch.cuda.is_available():
        pytest.skip("the descriptors carry fake pointers: run on a machine without a GPU")
    sweep, accepted, refused_by_name = rc.Sweep(_lib), 0, 0
    for key, (one, two) in _cases():
        for f4x1 in (False, True):
            o1, o2 = sweep.outcome(one, f4x1), sweep.outcome(two, f4x1)
            want = (o1[0], o1[1].replace("config -12 ", "config -13 ") if o1[1] else None)
            assert o2 == want, (key, f4x1, o1, o2)
            accepted += o2[0] != -22
            refused_by_name += bool(o2[1] and "config -13 " in o2[1])
    assert accepted > 0 and refused_by_name > 0


def test_pair_config_is_refused_by_name_on_a_launch_outside_the_family():
    import torch
    if torch.cuda.is_available():
        pytest.skip("the descriptors carry fake pointers: run on a machine without a GPU")
    sweep = rc.Sweep(_lib)
    for shape in ((128, 64, 1, 1), (64, 128, 3, 2), (48, 64, 3, 1)):             # a 1x1 layer, a stride-2 layer, Cin % 32 != 0
        for f4x1 in (False, True):
            rc_, msg = sweep.outcome(rc.make_desc(_lib, *shape, config=PAIR), f4x1)
            assert rc_ == -22 and msg.startswith("read_gated_conv_forward: config -13 takes the launches of the split-operand 3x3/s1 family"), (shape, msg)
    # the family's own shape without the operand beside the descriptor
    rc_, msg = sweep.outcome(rc.make_desc(_lib, 64, 64, 3, 1, config=PAIR), False)
    assert rc_ == -22 and "config -13 " in msg and "read_gated_conv_forward_f4x1" in msg
