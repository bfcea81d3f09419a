"""GPU: gated_conv_f4x1h_kernel (Winograd F(4,3) along x, the three ky taps direct, split operands on the f16 matrix cores; config -12 /
read_tuning_set("conv_f4x1", min Cin); read_gated_conv_forward_f4x1) against the torch-fp32 oracle on the CPU and against float64.

Tolerance of the parity check: |diff| <= 10 x 5e-6 x (1 + |ref|) — the scale of 10 is the one tests/test_gpu_conv.py gives this family
(test_winograd_f4_split_operand_kernel: `_close(..., scale=10.0)`), on a base of 5e-6 where that file uses 2e-5: four times TIGHTER than
the F(4x4) kernel is held to.  On amplified inputs the tolerance scales with the amplitude, as in that file's direct-kernel range check.

Range: the input transform multiplies by at most 10 (tests/test_f4x1_model.py asserts it from the matrix), so the f16 pieces overflow
at 65504 / 10 = 6550.  Checked at half of that (3275: a margin of two) and at 5,000; F(4x4) overflows at about 650.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import conv_ref64 as R64

pytestmark = pytest.mark.gpu

TOL = 10.0 * 5e-6
F4X1, W4H = -12, -7


def _pack(L):
    from read_amd.gated_conv import PackedGatedConv
    return PackedGatedConv(L["wf"], L["bf"], L["wm"], L["bm"], L["gamma"], L["beta"], L["mean"], L["var"], src_channels=[L["wf"].shape[1]])


def _nhwc(a_chw):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a_chw).transpose(1, 2, 0))).cuda()


def _launch(pk, x, config, elu=True, residual=None, **kw):
    from read_amd.gated_conv import gated_conv
    out = gated_conv(pk, [(_nhwc(x), 0)], elu=elu, residual=_nhwc(residual) if residual is not None else None, config=config, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _case(c, H, W, seed, amp=1.0, residual=True):
    L = R64.tame_layer(c, c, 3, seed)
    rng = np.random.default_rng([seed, c, H, W])
    x = (rng.standard_normal((c, H, W)) * amp).astype(np.float32)
    res = (rng.standard_normal((c, H, W)) * amp).astype(np.float32) if residual else None
    return L, x, res


# the four C -> C shapes of the network at an eighth of its 1216 x 352 frame per side, and odd sizes that clip the 8 x 32 units and the 1 x 4
# tiles on all four borders (one unit, several units side by side and below each other, a single pixel, widths 4 k + 1 .. 4 k + 3).  Every
# workgroup runs ONE unit here: the grid is min(units, compute units) rounded down to a multiple of the channel groups, and the largest
# entry has 32 units.  The persistent walk (a workgroup's second and third unit) is run by shape in
# tests/test_gpu_conv_accuracy.py::test_persistent_walk_against_fp64, and the kernel is held to a float64 reference and its derived bound
# there (family "f4x1" of test_split_operand_family_against_fp64); the checks below are parity, dispatch and plumbing.
SHAPES = [(32, 44, 152), (64, 22, 76), (128, 11, 38), (256, 6, 19), (32, 41, 130), (64, 13, 37), (128, 9, 17), (256, 11, 35), (96, 23, 70),
          (160, 3, 65), (64, 1, 1), (32, 5, 3), (32, 64, 96)]


def test_f4x1_parity_and_float64(hip):
    """Every shape with residual on / off and ELU on / off against the torch-fp32 oracle at TOL; against float64 the kernel's E_max and
    E_rms (tests/conv_ref64.py: error in units of fp32 round-off of the condition term) do not exceed those of the F(4x4) split-operand
    kernel it replaces, launched here on the same inputs."""
    from read_amd.gated_conv import conv_desc
    fam = hip.read_conv_kernel_family
    worse = []
    for j, (c, H, W) in enumerate(SHAPES):
        elu, with_res = j % 2 == 0, j % 4 < 2
        L, x, res = _case(c, H, W, 1200 + j, residual=with_res)
        pk = _pack(L)
        assert pk.wpacked_f4x1 is not None
        assert fam(ctypes.byref(conv_desc(pk, [(_nhwc(x), 0)], elu=elu, config=F4X1))) == 5
        got = _launch(pk, x, F4X1, elu=elu, residual=res).transpose(2, 0, 1)
        old = _launch(pk, x, W4H, elu=elu, residual=res).transpose(2, 0, 1)
        oracle = R64.oracle_fp32(L, x, elu=elu, residual=res)
        err = np.abs(got - oracle)
        tol = TOL * (1.0 + np.abs(oracle))
        ref = R64.reference(L, x, elu=elu, residual=res)
        e_new, e_old = R64.measure_gated(got, ref), R64.measure_gated(old, ref)
        print(f"f4x1 {c:3d} {H}x{W} elu={int(elu)} res={int(with_res)}: max |diff| vs torch {err.max():.3e} (tol {TOL:.1e} (1 + |ref|))   "
              f"E_max / E_rms  f4x1 {e_new[0]:.2f} / {e_new[1]:.3f}   w4h {e_old[0]:.2f} / {e_old[1]:.3f}")
        assert np.all(err <= tol), f"{c} {H}x{W}: {int((err > tol).sum())} of {err.size} off, max {err.max():.3e}"
        if e_new[0] > e_old[0] or e_new[1] > e_old[1]:
            worse.append((c, H, W, e_new, e_old))
    assert not worse, f"less accurate than the F(4x4) split-operand kernel against float64: {worse}"


def test_f4x1_channel_stride_and_repeatability(hip):
    """out_cstride > Cout: the kernel writes its channels of a wider tensor and nothing else; two launches on the same input are bit-identical."""
    for c, H, W in ((64, 13, 37), (128, 24, 40)):
        L, x, res = _case(c, H, W, 1300 + c)
        pk = _pack(L)
        wide = torch.full((H, W, c + 32), -7.0, device="cuda")
        got = _launch(pk, x, F4X1, residual=res, out=wide, out_channels=c + 32)
        assert np.all(got[..., c:] == -7.0), "wrote outside its channels"
        plain = _launch(pk, x, F4X1, residual=res)
        assert np.array_equal(got[..., :c], plain)
        again = _launch(pk, x, F4X1, residual=res)
        assert np.array_equal(plain.view(np.uint32), again.view(np.uint32)), "two launches differ"
        oracle = R64.oracle_fp32(L, x, residual=res).transpose(1, 2, 0)
        assert np.all(np.abs(plain - oracle) <= TOL * (1.0 + np.abs(oracle)))


@pytest.mark.parametrize("amp", [3275.0, 5000.0])
def test_f4x1_range(hip, amp):
    """Activations of amplitude `amp` (uniform in [-amp, amp]: B^T d stays below 10 amp < 65504): finite, within the same relative
    tolerance.  (The F(4x4) kernel overflows at about 650.)"""
    c, H, W = 64, 24, 40
    L = R64.tame_layer(c, c, 3, 77)
    rng = np.random.default_rng(1400)
    x = rng.uniform(-amp, amp, (c, H, W)).astype(np.float32)
    x[:, 5, 8:14] = amp * np.array([1, -1, -1, 1, 1, 1], np.float32)[None]      # the worst signs for B^T's rows with |row| sum 10
    got = _launch(_pack(L), x, F4X1).transpose(2, 0, 1)
    assert np.isfinite(got).all()
    oracle = R64.oracle_fp32(L, x)
    err = np.abs(got - oracle)
    print(f"f4x1 range amp {amp}: max |diff| {err.max():.3e}, tolerance {TOL * amp:.3e} (1 + |ref|)")
    assert np.all(err <= TOL * amp * (1.0 + np.abs(oracle)))


def test_f4x1_dispatch(hip):
    """The predicate decides: config -12 and read_tuning_set("conv_f4x1", min Cin) send a family-5 launch to the new kernel (results equal
    config -12's, bit for bit), everything else leaves it on the F(4x4) kernel (results equal config -7's); both report family 5; FAM's
    x1 * x2 and launches without the operand never take it; a host that packed ONLY the new order is refused where F(4x4) is needed."""
    from read_amd import _lib
    from read_amd.gated_conv import conv_desc, gated_conv, _desc
    fam = hip.read_conv_kernel_family
    get = lambda: (lambda v: (_lib.check(hip.read_tuning_get(b"conv_f4x1", ctypes.byref(v))), v.value)[1])(ctypes.c_int(-1))   # noqa: E731
    default = get()
    try:
        for c in (32, 64, 128):
            L, x, res = _case(c, 19, 45, 1500 + c)
            pk = _pack(L)
            new, old = _launch(pk, x, F4X1, residual=res), _launch(pk, x, W4H, residual=res)
            assert not np.array_equal(new, old)                                   # different arithmetic: the two kernels are told apart by their bits
            for knob in (0, 32, 64, 128, 256):
                _lib.check(hip.read_tuning_set(b"conv_f4x1", knob))
                assert get() == knob
                assert fam(ctypes.byref(conv_desc(pk, [(_nhwc(x), 0)]))) == 5
                auto = _launch(pk, x, -1, residual=res)
                assert np.array_equal(auto, new if (knob and c >= knob) else old), (c, knob)
            _lib.check(hip.read_tuning_set(b"conv_f4x1", 32))
            xm = _nhwc(x)
            assert fam(ctypes.byref(conv_desc(pk, [(xm, 0)], mul=xm))) == 6      # FAM stays on the direct kernel
            pk.wpacked_f4x1 = None                                                # no operand: the F(4x4) kernel, whatever the knob says
            assert np.array_equal(_launch(pk, x, -1, residual=res), old)
        # only the new order packed (wpacked_w4h NULL): runs on the new kernel, refused when the knob sends it to F(4x4)
        L, x, res = _case(64, 19, 45, 1564)
        pk = _pack(L)
        new = _launch(pk, x, F4X1, residual=res)
        f4 = pk.wpacked_f4x1
        pk.wpacked_w4h = pk.wpacked_w4 = pk.wpacked_wino = pk.wpacked_w16 = pk.wpacked_d3h = None
        assert np.array_equal(_launch(pk, x, -1, residual=res), new)
        _lib.check(hip.read_tuning_set(b"conv_f4x1", 0))
        d, _ = _desc(pk, [(_nhwc(x), 0)])
        d.wpacked = None
        assert hip.read_gated_conv_forward_f4x1(ctypes.byref(d), f4.data_ptr(), _lib.stream_ptr()) != 0
        assert hip.read_gated_conv_forward(ctypes.byref(conv_desc(_pack(L), [(_nhwc(x), 0)], config=F4X1)), _lib.stream_ptr()) != 0   # -12 without the operand
    finally:
        _lib.check(hip.read_tuning_set(b"conv_f4x1", default))
        torch.cuda.synchronize()
