"""CPU (hipcc cross-compiles): properties of the generated gfx950 code of gated_conv_f4x1h_kernel (read_amd/csrc/conv.hip) that its
measurements rest on, found in the ISA like those of tests/test_isa_guards.py:

  * no scratch (the F(4x4) sibling once ran 720 us instead of 60 with 1.4 KB of it);
  * one wave per SIMD by design (__launch_bounds__(256, 1)): the register count is recorded, and it needs more than the 256 that two
    waves per SIMD would leave — the 24 accumulators, the ring of nine weight fragments and the 60 patch registers;
  * 216 MFMAs per stage, first and steady instance: 2 x 216 in the body, nothing duplicated, nothing on the fp32 matrix path;
  * 30 split stores (hi and lo: 60 v_cvt_pk_f16_f32) per transform instance: prologue + two stage instances;
  * the unit loop does not drain the memory pipeline at its head (the weight and patch loads of the next unit are in flight there);
  * no probe variants: the release library holds exactly one instance of the kernel, not a template.
"""
import re

import pytest

from tests.test_isa_guards import _asm, _function, _meta


@pytest.fixture(scope="module")
def conv_asm(tmp_path_factory):
    return _asm("conv.hip", tmp_path_factory)


def test_f4x1_kernel_registers_and_pipeline(conv_asm):
    name, body = _function(conv_asm, "gated_conv_f4x1h_kernel")
    assert _meta(conv_asm, name, "private_seg_size") == 0, "scratch in the F(4,3)-by-rows kernel"
    vgpr, agpr = _meta(conv_asm, name, "num_vgpr"), _meta(conv_asm, name, "num_agpr")
    print(f"gated_conv_f4x1h_kernel: num_vgpr {vgpr} + num_agpr {agpr} = {vgpr + agpr}")
    assert 256 < vgpr + agpr <= 512, "one wave per SIMD by design"
    assert agpr >= 96, "the 24 accumulators live in the accumulation file"
    assert body.count("v_mfma_f32_16x16x32_f16") == 2 * 216                     # first + steady stage instance
    assert "v_mfma_f32_16x16x4_f32" not in body
    assert body.count("v_cvt_pk_f16_f32") == 3 * 60                             # prologue + two stage instances: hi and lo of 5 items x 6 frequencies
    lines = body.split("\n")
    heads = [i for i, l in enumerate(lines) if "Loop Header: Depth=1" in l]
    assert heads, "unit loop not found"
    head = "\n".join(lines[heads[0]:heads[0] + 12])
    assert "vmcnt(0)" not in head, "the unit loop drains the previous unit's stores and loads:\n" + head
    mf = [i for i, l in enumerate(lines) if l.strip().startswith("v_mfma_f32_16x16x32_f16")]
    stage = [l.strip() for l in lines[mf[0]:mf[-1]]]
    assert sum(1 for l in stage if l.startswith("s_waitcnt") and "vmcnt(0)" in l) == 0, "a stage drains its weight or patch loads"


def test_f4x1_kernel_has_no_probe_variants(conv_asm):
    names = set(re.findall(r"^(_Z\S*gated_conv_f4x1h_kernel\S*):\s*;", conv_asm, flags=re.M))
    assert len(names) == 1, names
    assert "gated_conv_f4x1h_kernelILi" not in conv_asm                         # not a template over probe bits
    for old in ("wino4h2", "wino4x2"):
        assert old not in next(iter(names))
