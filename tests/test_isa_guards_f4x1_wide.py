"""CPU (hipcc cross-compiles): properties of the generated gfx950 code of f4x1_wide_conv_kernel (read_amd/csrc/conv.hip) that
eight waves on one CU rest on, found in the ISA like those of tests/test_isa_guards_f4x1_pair.py:

  * one instance, and its symbol does not match gated_conv_*kernel (tests/test_isa_guards.py counts that pattern);
  * no scratch;
  * at most 256 registers per wave (two waves per SIMD), the 96 accumulator registers in the accumulation file;
  * at most 160 KiB of static LDS (two V images of 61,440 bytes + the two groups' epilogue parameters);
  * a multiple of 216 MFMAs (recorded: ONE stage instance, the accumulators are cleared in front of a unit), nothing on the fp32
    matrix path;
  * the converts of the transform.  An item is one row segment of a thread: six frequencies x (hi, lo) = 12 v_cvt_pk_f16_f32.  The code
    of a transform instance holds the three items a gh = 0 wave carries (i = 0, 1, 2; a gh = 1 wave runs the first two of them for its
    i = 3, 4 and branches round the third): 36.  There are two instances, the prologue's and the one beside the stage's MFMAs: 72.
"""
import re

import pytest

from tests.test_isa_guards import _asm, _function, _meta

KERNEL = "f4x1_wide_conv_kernel"
STAGE_INSTANCES = 1
ITEMS_IN_CODE = 3
TRANSFORM_INSTANCES = 2
N_CVT = 12 * ITEMS_IN_CODE * TRANSFORM_INSTANCES


@pytest.fixture(scope="module")
def conv_asm(tmp_path_factory):
    return _asm("conv.hip", tmp_path_factory)


def test_wide_kernel_is_one_instance_outside_the_census(conv_asm):
    names = set(re.findall(r"^(_Z\S*" + KERNEL + r"\S*):\s*;", conv_asm, flags=re.M))
    assert len(names) == 1, names
    name = next(iter(names))
    assert KERNEL + "I" not in name                                             # not a template
    assert not re.search(r"gated_conv_\w*kernel", name)


def test_wide_kernel_fits_eight_waves_on_a_cu(conv_asm):
    name, body = _function(conv_asm, KERNEL)
    assert _meta(conv_asm, name, "private_seg_size") == 0, "scratch in the wide kernel"
    vgpr, agpr = _meta(conv_asm, name, "num_vgpr"), _meta(conv_asm, name, "num_agpr")
    m = re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\n(?:.*\n)*?\s*\.amdhsa_group_segment_fixed_size (\d+)", conv_asm)
    assert m, "kernel descriptor not found"
    lds = int(m.group(1))
    n_mfma, n_cvt = body.count("v_mfma_f32_16x16x32_f16"), body.count("v_cvt_pk_f16_f32")
    print(f"{KERNEL}: num_vgpr {vgpr} + num_agpr {agpr} = {vgpr + agpr}, LDS {lds} B, {n_mfma} MFMAs, {n_cvt} converts")
    assert vgpr + agpr <= 256, "two waves per SIMD"
    assert agpr >= 96, "the 24 accumulators live in the accumulation file"
    assert lds <= 163840
    assert n_mfma % 216 == 0 and n_mfma == STAGE_INSTANCES * 216
    assert "v_mfma_f32_16x16x4_f32" not in body
    assert n_cvt == N_CVT
