"""GPU: f4x1_pair_conv_kernel (config -13), the F(4,3)-by-rows kernel as two resident workgroups per CU, against
gated_conv_f4x1h_kernel (config -12).  The two run the same arithmetic in the same order per accumulator, so the check is equality
of bits, not a tolerance; one shape is also held to the torch-fp32 oracle at the tolerance of tests/test_gpu_conv_f4x1.py, which
guards against a mistake the two launches would share (the harness, the packer).

What each shape is there for:
    C =  32,   8 x  32   one unit, one chunk: the V image is written once and nothing is reused
    C =  32,  13 x  37   clipped rows and columns: halo zeros on all four borders, stores outside the image suppressed
    C =  64,  24 x  96   two chunks, two channel groups: the single V image is rewritten between chunks (both barriers)
    C = 256,  16 x  64   eight chunks, eight groups
    C =  32, 200 x 704   550 units on at most 2 x CUs workgroups: the walk wraps, V and the patch cursor carry over into the next unit
    C =  64, 136 x 512   544 units with two groups
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import conv_ref64 as R64

pytestmark = pytest.mark.gpu

TOL = 10.0 * 5e-6                     # tests/test_gpu_conv_f4x1.py
PAIR, F4X1 = -13, -12
SHAPES = [(32, 8, 32), (32, 13, 37), (64, 24, 96), (256, 16, 64), (32, 200, 704), (64, 136, 512)]


def _pack(L):
    from read_amd.gated_conv import PackedGatedConv
    return PackedGatedConv(L["wf"], L["bf"], L["wm"], L["bm"], L["gamma"], L["beta"], L["mean"], L["var"], src_channels=[L["wf"].shape[1]])


def _nhwc(a_chw):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a_chw).transpose(1, 2, 0))).cuda()


def _inputs(c, H, W, seed):
    rng = np.random.default_rng([seed, c, H, W])
    return rng.standard_normal((c, H, W)).astype(np.float32), rng.standard_normal((c, H, W)).astype(np.float32)


def test_pair_kernel_occupancy(hip):
    """Two workgroups of the kernel are resident on a CU: what the kernel exists for (62,208 bytes of LDS, at most 256 registers)."""
    assert hip.read_conv_f4x1_pair_occupancy() == 2


@pytest.mark.parametrize("c,H,W", SHAPES)
def test_pair_equals_single_workgroup_kernel(hip, c, H, W):
    from read_amd.gated_conv import conv_desc, gated_conv
    L = R64.tame_layer(c, c, 3, 1700 + c)
    pk = _pack(L)
    x, res = _inputs(c, H, W, 1700)
    xd, rd = _nhwc(x), _nhwc(res)
    assert hip.read_conv_kernel_family(ctypes.byref(conv_desc(pk, [(xd, 0)], config=PAIR))) == 5
    for elu in (True, False):
        for r in (rd, None):
            one = gated_conv(pk, [(xd, 0)], elu=elu, residual=r, config=F4X1)
            two = gated_conv(pk, [(xd, 0)], elu=elu, residual=r, config=PAIR)
            torch.cuda.synchronize()
            assert torch.equal(one.view(torch.int32), two.view(torch.int32)), \
                f"C={c} {H}x{W} elu={elu} residual={r is not None}: {int((one.view(torch.int32) != two.view(torch.int32)).sum())} of {one.numel()} values differ"
            again = gated_conv(pk, [(xd, 0)], elu=elu, residual=r, config=PAIR)
            torch.cuda.synchronize()
            assert torch.equal(two.view(torch.int32), again.view(torch.int32)), "two launches of the pair kernel differ"


def test_pair_concat_slot_and_oracle(hip):
    """out_cstride > Cout: the kernel writes its channels of a wider tensor and nothing else, the same bits as config -12; the result is
    also within TOL (1 + |ref|) of the torch-fp32 oracle."""
    from read_amd.gated_conv import gated_conv
    c, H, W = 64, 24, 96
    L = R64.tame_layer(c, c, 3, 1764)
    pk = _pack(L)
    x, res = _inputs(c, H, W, 1764)
    xd, rd = _nhwc(x), _nhwc(res)
    wide = {}
    for cfg in (F4X1, PAIR):
        wide[cfg] = torch.full((H, W, c + 32), -7.0, device="cuda")
        gated_conv(pk, [(xd, 0)], residual=rd, config=cfg, out=wide[cfg], out_channels=c + 32)
    torch.cuda.synchronize()
    assert bool((wide[PAIR][..., c:] == -7.0).all()), "wrote outside its channels"
    assert torch.equal(wide[PAIR].view(torch.int32), wide[F4X1].view(torch.int32))
    got = wide[PAIR][..., :c].cpu().numpy()
    oracle = R64.oracle_fp32(L, x, residual=res).transpose(1, 2, 0)
    err = np.abs(got - oracle)
    print(f"pair {c} {H}x{W}: max |diff| vs torch fp32 {err.max():.3e} (tol {TOL:.1e} (1 + |ref|))")
    assert np.all(err <= TOL * (1.0 + np.abs(oracle)))


def test_pair_refused_where_the_single_workgroup_kernel_is(hip):
    """Cout that is no multiple of 32 is not a launch of the family: config -12 refuses it, and so does config -13."""
    from read_amd import _lib
    from read_amd.gated_conv import conv_desc
    L = R64.tame_layer(32, 24, 3, 1724)
    pk = _pack(L)
    x, _ = _inputs(32, 9, 33, 1724)
    xd = _nhwc(x)
    out = torch.empty(9, 33, 24, device="cuda")
    rcs = {}
    for cfg in (F4X1, PAIR):
        d = conv_desc(pk, [(xd, 0)], config=cfg, out=out)
        f4 = getattr(pk, "wpacked_f4x1", None)
        rcs[cfg] = (hip.read_gated_conv_forward_f4x1(ctypes.byref(d), f4.data_ptr(), _lib.stream_ptr()) if f4 is not None
                    else hip.read_gated_conv_forward(ctypes.byref(d), _lib.stream_ptr()))
        msg = hip.read_last_error().decode()
        assert rcs[cfg] == -22 and f"config {cfg} " in msg, (cfg, rcs[cfg], msg)
    torch.cuda.synchronize()
