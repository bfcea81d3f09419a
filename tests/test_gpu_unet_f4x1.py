"""GPU: the UNet plan with the split-operand 3x3/s1 layers on the F(4,3)-by-rows kernel (gated_conv_f4x1h_kernel), and where its
operand comes from.  tests/test_gpu_unet.py holds the plan to the oracle and the lean blob to the full one; here:

  * the lean blob carries the order, the full blob (laid out as it always was) gets it as a side buffer derived from its exact
    weights: both render the same bits;
  * a lean blob packed before the kernel existed (READ_UNET_LAYOUT_LEAN_W4H) still renders, on the F(4x4) split-operand kernel — bit
    for bit what the new blobs render with read_tuning_set("conv_f4x1", 0) — and agrees with the default plan at the network guard;
  * the default plan and the conv_f4x1 = 0 plan are two different arithmetic paths (their frames differ in bits), and
    conv_f4x1 = 128 (levels 2 and 3 only) is a third.
"""
import numpy as np
import pytest
import torch

from oracle import unet_torch
from read_amd import synthetic
from tests.unet_spec import UNET_SPEC
from tests.test_gpu_unet import _check_rgb

pytestmark = pytest.mark.gpu


def test_old_blobs_render_and_the_knob_selects_the_kernel(hip):
    from read_amd import _lib
    from read_amd.unet import LAYOUT_FULL, LAYOUT_LEAN, LAYOUT_LEAN_W4H, UNetEngine, layout_of, pack_state
    H, W = 96, 160
    state = synthetic.make_unet_state(UNET_SPEC, 12)
    torch.manual_seed(5)
    xs = [torch.rand(H >> l, W >> l, 8, device="cuda") for l in range(4)]
    with torch.no_grad():
        ref = unet_torch.unet_forward(state, *[x.permute(2, 0, 1)[None].cpu() for x in xs])[0]
    outs, blobs = {}, {}
    for layout in (LAYOUT_FULL, LAYOUT_LEAN, LAYOUT_LEAN_W4H):
        blobs[layout] = packed = torch.from_numpy(pack_state(state, layout=layout)).cuda()
        assert layout_of(packed) == layout
        eng = UNetEngine(packed, H, W)
        kinds = [k for (_, _, _, k) in eng.profile(*xs)]
        assert kinds.count(5) >= 70 and kinds.count(6) == 3 and kinds.count(4) == 0
        outs[layout] = eng.forward(*xs).clone()
        _check_rgb(outs[layout].permute(2, 0, 1).cpu(), ref, f"layout {layout}")
    assert torch.equal(outs[LAYOUT_FULL], outs[LAYOUT_LEAN])
    assert not torch.equal(outs[LAYOUT_FULL], outs[LAYOUT_LEAN_W4H])           # F(4,3) by rows against F(4x4): different bits
    _check_rgb(outs[LAYOUT_FULL].permute(2, 0, 1).cpu(), outs[LAYOUT_LEAN_W4H].permute(2, 0, 1).cpu(), "new plan against the old blob's plan")
    try:
        _lib.check(hip.read_tuning_set(b"conv_f4x1", 0))
        for layout in (LAYOUT_FULL, LAYOUT_LEAN):                                 # both carry the F(4x4) split operand too
            assert torch.equal(UNetEngine(blobs[layout], H, W).forward(*xs), outs[LAYOUT_LEAN_W4H])
        _lib.check(hip.read_tuning_set(b"conv_f4x1", 128))                        # per-level dispatch: levels 2 and 3 only
        mixed = UNetEngine(blobs[LAYOUT_FULL], H, W).forward(*xs).clone()
        assert torch.equal(mixed, UNetEngine(blobs[LAYOUT_LEAN], H, W).forward(*xs))
        _check_rgb(mixed.permute(2, 0, 1).cpu(), ref, "conv_f4x1 = 128")
        assert not torch.equal(mixed, outs[LAYOUT_FULL]) and not torch.equal(mixed, outs[LAYOUT_LEAN_W4H])
    finally:
        _lib.check(hip.read_tuning_set(b"conv_f4x1", 32))
    # a full-layout plan without its side buffer (a host that does not know the kernel): the F(4x4) kernel
    eng = UNetEngine(blobs[LAYOUT_FULL], H, W)
    _lib.check(hip.read_unet_set_f4x1(eng.handle, None))
    assert torch.equal(eng.forward(*xs), outs[LAYOUT_LEAN_W4H])
