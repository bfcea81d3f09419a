"""GPU: f4x1_wide_conv_kernel (config -14), the F(4,3)-by-rows kernel with one input transform for two channel groups, against
gated_conv_f4x1h_kernel (config -12).  The two run the same arithmetic in the same order per accumulator, so the check is equality
of bits, not a tolerance; one shape is also held to the torch-fp32 oracle at the tolerance of tests/test_gpu_conv_f4x1_pair.py, which
guards against a mistake the two launches would share (the harness, the packer).

What each shape is there for:
    C =  64,   8 x  32   one wide unit, two chunks: both V buffers and both group halves
    C =  64,  13 x  37   clipped rows and columns: halo zeros on all four borders, stores outside the image suppressed
    C = 128,  16 x  64   two group pairs, four chunks, four blocks
    C = 256,  16 x  64   four pairs, eight chunks
    C =  64, 200 x 704   550 wide units on at most CUs workgroups: the walk wraps twice; V, the patch cursor and the weight ring carry
                         over into the next unit
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import conv_ref64 as R64

pytestmark = pytest.mark.gpu

TOL = 10.0 * 5e-6                     # tests/test_gpu_conv_f4x1_pair.py
WIDE, F4X1 = -14, -12
SHAPES = [(64, 8, 32), (64, 13, 37), (128, 16, 64), (256, 16, 64), (64, 200, 704)]


def _pack(L):
    from read_amd.gated_conv import PackedGatedConv
    return PackedGatedConv(L["wf"], L["bf"], L["wm"], L["bm"], L["gamma"], L["beta"], L["mean"], L["var"], src_channels=[L["wf"].shape[1]])


def _nhwc(a_chw):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a_chw).transpose(1, 2, 0))).cuda()


def _inputs(c, H, W, seed):
    rng = np.random.default_rng([seed, c, H, W])
    return rng.standard_normal((c, H, W)).astype(np.float32), rng.standard_normal((c, H, W)).astype(np.float32)


@pytest.mark.parametrize("c,H,W", SHAPES)
def test_wide_equals_single_workgroup_kernel(hip, c, H, W):
    from read_amd.gated_conv import conv_desc, gated_conv
    L = R64.tame_layer(c, c, 3, 1800 + c)
    pk = _pack(L)
    x, res = _inputs(c, H, W, 1800)
    xd, rd = _nhwc(x), _nhwc(res)
    assert hip.read_conv_kernel_family(ctypes.byref(conv_desc(pk, [(xd, 0)], config=WIDE))) == 5
    for elu in (True, False):
        for r in (rd, None):
            one = gated_conv(pk, [(xd, 0)], elu=elu, residual=r, config=F4X1)
            two = gated_conv(pk, [(xd, 0)], elu=elu, residual=r, config=WIDE)
            torch.cuda.synchronize()
            assert torch.equal(one.view(torch.int32), two.view(torch.int32)), \
                f"C={c} {H}x{W} elu={elu} residual={r is not None}: {int((one.view(torch.int32) != two.view(torch.int32)).sum())} of {one.numel()} values differ"
            again = gated_conv(pk, [(xd, 0)], elu=elu, residual=r, config=WIDE)
            torch.cuda.synchronize()
            assert torch.equal(two.view(torch.int32), again.view(torch.int32)), "two launches of the wide kernel differ"


def test_wide_concat_slot_and_oracle(hip):
    """out_cstride > Cout: the kernel writes its channels of a wider tensor and nothing else, the same bits as config -12; the result is
    also within TOL (1 + |ref|) of the torch-fp32 oracle."""
    from read_amd.gated_conv import gated_conv
    c, H, W = 64, 24, 96
    L = R64.tame_layer(c, c, 3, 1864)
    pk = _pack(L)
    x, res = _inputs(c, H, W, 1864)
    xd, rd = _nhwc(x), _nhwc(res)
    wide = {}
    for cfg in (F4X1, WIDE):
        wide[cfg] = torch.full((H, W, c + 32), -7.0, device="cuda")
        gated_conv(pk, [(xd, 0)], residual=rd, config=cfg, out=wide[cfg], out_channels=c + 32)
    torch.cuda.synchronize()
    assert bool((wide[WIDE][..., c:] == -7.0).all()), "wrote outside its channels"
    assert torch.equal(wide[WIDE].view(torch.int32), wide[F4X1].view(torch.int32))
    got = wide[WIDE][..., :c].cpu().numpy()
    oracle = R64.oracle_fp32(L, x, residual=res).transpose(1, 2, 0)
    err = np.abs(got - oracle)
    print(f"wide {c} {H}x{W}: max |diff| vs torch fp32 {err.max():.3e} (tol {TOL:.1e} (1 + |ref|))")
    assert np.all(err <= TOL * (1.0 + np.abs(oracle)))


@pytest.mark.parametrize("cout", [32, 96, 24])
def test_wide_refused_where_no_group_pair_exists(hip, cout):
    """Cout % 64 != 0 leaves a channel group without a partner (32, 96) or is no launch of the family at all (24): config -14 is
    refused by name, not mis-launched."""
    from read_amd import _lib
    from read_amd.gated_conv import conv_desc
    L = R64.tame_layer(32, cout, 3, 1824 + cout)
    pk = _pack(L)
    x, _ = _inputs(32, 9, 33, 1824)
    xd = _nhwc(x)
    out = torch.full((9, 33, cout), -7.0, device="cuda")
    d = conv_desc(pk, [(xd, 0)], config=WIDE, out=out)
    f4 = getattr(pk, "wpacked_f4x1", None)
    rc = (hip.read_gated_conv_forward_f4x1(ctypes.byref(d), f4.data_ptr(), _lib.stream_ptr()) if f4 is not None
          else hip.read_gated_conv_forward(ctypes.byref(d), _lib.stream_ptr()))
    msg = hip.read_last_error().decode()
    assert rc == -22 and "config -14 " in msg, (cout, rc, msg)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()), "a refused launch wrote"
