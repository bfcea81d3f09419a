"""Config -14 (f4x1_wide_conv_kernel, two channel groups on one input transform) is accepted exactly where config -12
(gated_conv_f4x1h_kernel) is and Cout % 64 == 0: there it has the family, the return code and the refusal text of -12 but for the
config's number; everywhere else it is refused by name.  Swept over the anchor shapes of tests/route_cases.py with every operand
absent, misaligned or alone.  Fake pointers: the launch half is skipped where a GPU is visible (tests/route_cases.py)."""
import ctypes as C
import itertools

import pytest

from read_amd import _lib
from tests import route_cases as rc

WIDE, F4X1 = -14, -12
MODES = ("plain", "linear", "mul", "residual")
REFUSAL = "read_gated_conv_forward: config -14 takes the launches of the split-operand 3x3/s1 family"


def _cases():
    for (cin, cout, k, s), mode, (absent, mis) in itertools.product(rc.ANCHOR_SHAPES, MODES, rc.operand_variants()):
        yield (cin, cout, k, s, mode, absent, mis), [rc.make_desc(_lib, cin, cout, k, s, "one", mode, cfg, absent, mis) for cfg in (F4X1, WIDE)]


def test_wide_config_reports_the_family_of_config_12():
    L, n5 = _lib.lib(), 0
    for key, (one, two) in _cases():
        if key[1] % 64:
            continue
        f1, f2 = L.read_conv_kernel_family(C.byref(one[0])), L.read_conv_kernel_family(C.byref(two[0]))
        assert f1 == f2, (key, f1, f2)
        n5 += f2 == 5
    assert n5 > 0
    for shape in ((64, 64, 3, 1), (128, 128, 3, 1)):
        d, _ = rc.make_desc(_lib, *shape, config=WIDE)
        assert L.read_conv_kernel_family(C.byref(d)) == 5, shape


def test_wide_config_is_accepted_and_refused_as_config_12_where_groups_pair_up():
    import torch
    if torch.cuda.is_available():
        pytest.skip("the descriptors carry fake pointers: run on a machine without a GPU")
    sweep, accepted, refused_by_name, refused_elsewhere = rc.Sweep(_lib), 0, 0, 0
    for key, (one, two) in _cases():
        for f4x1 in (False, True):
            o1, o2 = sweep.outcome(one, f4x1), sweep.outcome(two, f4x1)
            if key[1] % 64 == 0:
                want = (o1[0], o1[1].replace("config -12 ", "config -14 ") if o1[1] else None)
                assert o2 == want, (key, f4x1, o1, o2)
                accepted += o2[0] != -22
                refused_by_name += bool(o2[1] and "config -14 " in o2[1])
            else:
                # refused by name; a descriptor that config -12 refuses for something other than its config (a null or misaligned
                # pointer, found before a kernel is chosen) is refused with that same text
                assert o2[0] == -22, (key, f4x1, o2)
                other = o1[0] == -22 and "config -12 " not in o1[1] and o2 == o1
                assert o2[1].startswith(REFUSAL) or other, (key, f4x1, o1, o2)
                refused_elsewhere += o2[1].startswith(REFUSAL)
    assert accepted > 0 and refused_by_name > 0 and refused_elsewhere > 0


def test_wide_config_is_refused_by_name_without_a_group_pair_or_outside_the_family():
    import torch
    if torch.cuda.is_available():
        pytest.skip("the descriptors carry fake pointers: run on a machine without a GPU")
    sweep = rc.Sweep(_lib)
    # one group, three groups; then a 1x1 layer, a stride-2 layer, Cin % 32 != 0
    for shape in ((32, 32, 3, 1), (64, 32, 3, 1), (64, 96, 3, 1), (128, 64, 1, 1), (64, 128, 3, 2), (48, 64, 3, 1)):
        for f4x1 in (False, True):
            rc_, msg = sweep.outcome(rc.make_desc(_lib, *shape, config=WIDE), f4x1)
            assert rc_ == -22 and msg.startswith(REFUSAL), (shape, f4x1, msg)
    # the family's own shape without the operand beside the descriptor
    rc_, msg = sweep.outcome(rc.make_desc(_lib, 64, 64, 3, 1, config=WIDE), False)
    assert rc_ == -22 and "config -14 " in msg and "read_gated_conv_forward_f4x1" in msg
    # ... and with it the launch passes validation (on a machine without a GPU it then fails in the runtime)
    rc_, msg = sweep.outcome(rc.make_desc(_lib, 64, 64, 3, 1, config=WIDE), True)
    assert rc_ != -22, msg
