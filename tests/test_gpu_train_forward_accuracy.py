"""GPU: the forward linear launches of the training step — read_gated_conv_forward with linear = 1 as read_amd/train.py issues it
(layer_route, _packed_for, _linear_conv), on the workgroup-tiled direct fp32 kernel (family 0; 64 -> 56 k1 reports family 0 on the fp32
pixel-lane kernel), the fp32 Winograd F(2x2,3x3) kernel (family 2) and the fp32 Winograd F(4x4,3x3) kernel (family 4) — against the float64 references of tests/conv_ref64.py and
tests/train_ref64.py in units of fp32 round-off, under the rules of tests/test_gpu_train_accuracy.py (`judge`):
  1. the pre-activations fm = [f | m] elementwise under train_ref64.conv_forward_bound and under the yardstick cap (torch-fp32 and a
     sequential fp32 sum on the CPU), cond = sum |x| |w| + |b| (direct) or A_w + |b| (Winograd); a guard band after fm untouched; on the
     direct kernel impulses read the integer weights back exactly; with all-zero weights fm is the bias, bit for bit;
  2. the fused gated output y of the Winograd kernels (out_gated), (i) against the float64 gate of the device's own fm under the gate
     kernel's bound and (ii) against the float64 layer under gated_bound composed from the bounds of 1, with and without ELU, with
     eval-mode BatchNorm parameters and with identity_bn;
  3. stacked geometries: separator rows of y are +0.0, valid rows and all of fm bit-identical to the unstacked launch; one layer per
     kernel through GatedConvFn.apply with nb = 3 must reproduce the launch with the block geometry of its OUTPUT rows;
  4. the fused gate and read_gate_forward on the same fm, each within the gate's bound of the float64 gate;
  5. the launches that take_out_gated refuses on the host.
The cases and the assertions over a launch's buffers live in tests/train_forward_cases.py, shared with the CPU mutation catalogue.
Run with -s to see the table; lines start with "TACC|" (families fwd_direct, fwd_w2, fwd_w4, fwd_gate)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from read_amd import _lib
from tests import conv_ref64 as R64
from tests import train_forward_cases as FC
from tests import train_ref64 as T
from tests.test_gpu_train_accuracy import FAILED, finish, judge
from tests.train_fp32 import GUARD, SENTINEL, conv_direct32, gate32

pytestmark = pytest.mark.gpu
f32 = np.float32
FAMILY_OF_KIND = {_lib.PACK_DIRECT: "direct", _lib.PACK_WINO: "w2", _lib.PACK_W4: "w4"}
READ_EINVAL = -22


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=f32)).cuda()


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


class _switched:
    """read_amd.train with one module switch off (USE_WINOGRAD / USE_W4), restored on the way out."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        from read_amd import train
        if self.name:
            self.old = getattr(train, self.name)
            setattr(train, self.name, False)
        return train

    def __exit__(self, *exc):
        from read_amd import train
        if self.name:
            setattr(train, self.name, self.old)


class _Layer:
    """The device side of one case: the layer's tensors, its input, its route and the packed entries of both parameter blocks."""

    def __init__(self, train, case, family):
        self.case, self.family = case, family
        L = case.L
        self.ts = tuple(_dev(L[key]) for key in ("wf", "bf", "wm", "bm", "gamma", "beta", "mean", "var"))
        self.x = _dev(case.x.transpose(1, 2, 0))
        self.route = train.layer_route(case.cin, case.cout, case.k, case.stride)
        assert FAMILY_OF_KIND[self.route.fwd] == family, (case.name, self.route)
        self.train = train

    def launch(self, elu, identity, block_h=0, valid_h=0):
        """-> (fm buffer, y buffer) on the host, each with its guard band; the kernel family of the descriptor is asserted."""
        train, case = self.train, self.case
        entry = train._packed_for(self.route, self.ts, identity_bn=identity)
        n_fm, n_y = case.oh * case.ow * 2 * case.cout, case.oh * case.ow * case.cout
        fm_buf = torch.full((n_fm + GUARD,), float(SENTINEL), device="cuda")
        y_buf = torch.full((n_y + GUARD,), float(SENTINEL), device="cuda")
        fm, y = fm_buf[:n_fm].view(case.oh, case.ow, 2 * case.cout), y_buf[:n_y].view(case.oh, case.ow, case.cout)
        train.FLOP_LOG = []                                          # _linear_conv records read_conv_kernel_family of ITS descriptor
        try:
            train._linear_conv(self.x, case.cin, entry.fwd, entry.params, case.cout, case.k, case.stride, fm, wino=entry.wino,
                               gated=(y, elu, block_h, valid_h), w4=self.route.fwd == _lib.PACK_W4)
        finally:
            log, train.FLOP_LOG = train.FLOP_LOG, None
        assert log[-1][2] == T.FORWARD_FAMILY[self.family], f"{case.name}: the launch took kernel family {log[-1][2]}"
        return _host(fm_buf), _host(y_buf)


def _torch_gate(fm2, cout, bn, elu, identity):
    t = torch.from_numpy(np.ascontiguousarray(fm2))
    g = (F.elu(t[:, :cout]) if elu else t[:, :cout]) * torch.sigmoid(t[:, cout:])
    if identity:
        return g.numpy()
    par = [torch.from_numpy(np.asarray(bn[key], f32)) for key in ("mean", "var", "gamma", "beta")]
    return F.batch_norm(g.t()[None], *par, training=False, eps=T.EPS)[0].t().numpy()


def _seq_gate(fm2, cout, sc, sh, elu):
    a, _, s = gate32(fm2, cout, elu)
    return (((a * s).astype(f32) * sc[None]).astype(f32) + sh[None]).astype(f32)


def _own_yard(case, fm, elu, identity, valid):
    fm2 = fm.reshape(-1, 2 * case.cout)
    sc, sh = FC.scale_shift32(case.L, identity)
    v = valid[:, None]
    return {"torch": _torch_gate(fm2, case.cout, FC.bn_of(case.L, identity), elu, identity) * v, "seq": _seq_gate(fm2, case.cout, sc, sh, elu) * v}


def _layer_yard(case, elu, identity, fm_seq):
    """The layer end to end on the CPU: torch fp32, and the sequential fp32 pre-activations fm_seq (2 cout, oh, ow) through gate32."""
    L = dict(case.L)
    L.update(FC.bn_of(case.L, identity))
    sc, sh = FC.scale_shift32(case.L, identity)
    seq = _seq_gate(np.ascontiguousarray(fm_seq.transpose(1, 2, 0)).reshape(-1, 2 * case.cout), case.cout, sc, sh, elu)
    return {"torch": R64.oracle_fp32(L, case.x, stride=case.stride, elu=elu), "seq": seq.reshape(case.oh, case.ow, case.cout).transpose(2, 0, 1)}


def _fm_yard(case):
    L = case.L
    return {"torch": R64.oracle_fp32(L, case.x, stride=case.stride, linear=True),
            "seq": np.concatenate([(conv_direct32(case.x, L["w" + fm], case.stride) + L["b" + fm][:, None, None]).astype(f32) for fm in "fm"])}


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


LAUNCHES = [(family, layer) for family in ("direct", "w2", "w4") for layer in FC.LAYERS[family]]


@pytest.mark.parametrize("family,layer", LAUNCHES, ids=[f"{fam}-{FC.layer_name(l).replace(' ', '_')}" for fam, l in LAUNCHES])
def test_forward_linear_launch(hip, family, layer):
    """Assertions 1 and 2 for one layer at both sizes, every input class."""
    _forward_rows(family, layer, FC.SIZES[layer[3]])


@pytest.mark.parametrize("family,layer", LAUNCHES, ids=[f"{fam}-{FC.layer_name(l).replace(' ', '_')}" for fam, l in LAUNCHES])
def test_forward_linear_launch_at_degenerate_sizes(hip, family, layer):
    """The same at 2 x 2, 4 x 4 and 1 x 1 (FC.SIZES_TINY: the coarse levels of a 16-pixel crop; an impulse at every pixel), the guard
    bands behind fm and y included.  A 4x4 / stride-2 layer has no output at 1 x 1: that size is not a launch."""
    _forward_rows(family, layer, [hw for hw in FC.SIZES_TINY if 0 not in T.out_hw(layer[2], layer[3], *hw)])


def _forward_rows(family, layer, sizes):
    with _switched(layer[4]) as train:
        for hw in sizes:
            for case in FC.cases(layer, hw):
                dev = _Layer(train, case, family)
                first, yard_fm = None, _fm_yard(case)
                for elu, identity in ((True, False), (False, True), (True, True), (False, False)):
                    fm_buf, y_buf = dev.launch(elu, identity)
                    if first is None:
                        first = fm_buf
                        fm = FC.check_preactivations(case, family, fm_buf, judge, FAILED.append, yard_fm)
                    assert _same_bits(fm_buf, first), f"{case.name}: fm changed with the epilogue's parameters"
                    if family == "direct":                       # no fused gate: out_gated is not even passed on
                        assert _same_bits(y_buf, np.full_like(y_buf, SENTINEL)), f"{case.name}: a direct launch wrote y"
                        break
                    valid = np.ones(case.oh * case.ow, bool)
                    FC.check_gated(case, family, fm, y_buf, elu, identity, 0, 0, judge, FAILED.append,
                                   _own_yard(case, fm, elu, identity, valid), _layer_yard(case, elu, identity, yard_fm["seq"]))
    finish()


@pytest.mark.parametrize("family", ["w2", "w4"])
def test_separator_rows_of_the_fused_gate(hip, family):
    """Assertion 3: stacked geometries whose separators cross the kernels' tile boundaries, every layer of the family."""
    for layer in FC.LAYERS[family]:
        with _switched(layer[4]) as train:
            for (H, W, bh, vh) in FC.GEOMETRIES:
                case = next(FC.cases(layer, (H, W), classes="a"))
                dev = _Layer(train, case, family)
                for elu, identity in ((True, False), (False, True)):
                    fm0_buf, y0_buf = dev.launch(elu, identity)
                    fm0, y0 = fm0_buf[:-GUARD].reshape(case.oh, case.ow, -1), y0_buf[:-GUARD].reshape(case.oh, case.ow, -1)
                    fm_buf, y_buf = dev.launch(elu, identity, bh, vh)
                    valid = T.valid_rows(case.oh * case.ow, case.ow, bh, vh)
                    assert 0 < valid.sum() < valid.size or bh == vh
                    fm = fm_buf[:-GUARD].reshape(case.oh, case.ow, -1)
                    FC.check_gated(case, family, fm, y_buf, elu, identity, bh, vh, judge, FAILED.append,
                                   _own_yard(case, fm, elu, identity, valid), None, unstacked=(fm0, y0))
    finish()


@pytest.mark.parametrize("layer,hw,nb,v", [((32, 64, 3, 2), (24, 12), 3, (3, 4)), ((64, 32, 4, 2), (20, 12), 2, (3, 5)),
                                           ((32, 32, 3, 1), (21, 9), 3, (5, 7)), ((16, 32, 3, 1), (10, 21), 2, (3, 5))])
def test_gated_conv_fn_takes_the_block_geometry_at_the_output_scale(hip, layer, hw, nb, v):
    """GatedConvFn.apply(..., nb, v_num, v_den) against the launch (and, on the direct kernel, read_gate_forward) with the block geometry
    of the layer's OUTPUT rows, bit for bit."""
    from read_amd import train
    case = next(FC.cases(layer, hw, classes="a"))
    family = FAMILY_OF_KIND[train.layer_route(*layer).fwd]
    dev = _Layer(train, case, family)
    bh, vh = T.block_geometry(case.oh, nb, *v)
    if layer[3] == 2:
        assert (bh, vh) != T.block_geometry(case.H, nb, *v)          # the input scale would give another geometry
    for elu in (True, False):
        fm_buf, y_buf = dev.launch(elu, False, bh, vh)
        want = y_buf[:-GUARD].reshape(case.oh, case.ow, case.cout)
        if family == "direct":
            entry = train._packed_for(dev.route, dev.ts)
            fm_d, y_d = _dev(fm_buf[:-GUARD]), torch.full((case.oh, case.ow, case.cout), float(SENTINEL), device="cuda")
            _lib.check(hip.read_gate_forward(fm_d.data_ptr(), case.oh * case.ow, case.cout, entry.params.data_ptr(), int(elu), None, y_d.data_ptr(),
                                             case.ow, bh, vh, _lib.stream_ptr()))
            want = _host(y_d)
        with torch.no_grad():
            got = _host(train.GatedConvFn.apply(dev.x, *dev.ts, case.k, case.stride, elu, nb, v[0], v[1]))
        assert _same_bits(got, want), f"{case.name} nb {nb} valid {v}: GatedConvFn's y differs from the launch with block {bh}/{vh}"
        valid = T.valid_rows(case.oh * case.ow, case.ow, bh, vh)
        assert not got.reshape(valid.size, -1)[~valid].view(np.uint32).any() and (~valid).any() and got.reshape(valid.size, -1)[valid].any()


@pytest.mark.parametrize("family", ["w2", "w4"])
def test_fused_gate_and_gate_forward_agree_with_the_float64_gate(hip, family):
    """Assertion 4: on the same fm, the fused y and read_gate_forward's y are each within the gate's bound of the float64 gate.  The two
    kernels contract differently: the number of elements that differ is printed, not asserted."""
    st = _lib.stream_ptr()
    for layer in FC.LAYERS[family]:
        with _switched(layer[4]) as train:
            (H, W, bh, vh) = FC.GEOMETRIES[0]
            for case in FC.cases(layer, (H, W), classes="abd"):
                dev = _Layer(train, case, family)
                P, cout = case.oh * case.ow, case.cout
                for elu, identity in ((True, False), (False, True)):
                    fm_buf, y_buf = dev.launch(elu, identity, bh, vh)
                    entry = train._packed_for(dev.route, dev.ts, identity_bn=identity)
                    fm_d, y_d = _dev(fm_buf[:-GUARD]), torch.full((P, cout), float(SENTINEL), device="cuda")
                    _lib.check(hip.read_gate_forward(fm_d.data_ptr(), P, cout, entry.params.data_ptr(), int(elu), None, y_d.data_ptr(), case.ow, bh, vh, st))
                    fused, plain = y_buf[:-GUARD].reshape(P, cout), _host(y_d)
                    fm2 = fm_buf[:-GUARD].reshape(P, 2 * cout)
                    y_ref, B, bound, _ = T.gate_forward_ref(fm2, cout, FC.bn_of(case.L, identity), elu, None, case.ow, bh, vh)
                    yard = _own_yard(case, fm2, elu, identity, T.valid_rows(P, case.ow, bh, vh))
                    tag = f"{case.name} [{family}] {'elu' if elu else 'lin'} {'identity' if identity else 'eval'}"
                    differ = int((fused.view(np.uint32) != plain.view(np.uint32)).sum())
                    judge("fwd_gate", case.cls, tag + " fused", fused, y_ref, B, bound, yard)
                    judge("fwd_gate", case.cls, tag + " gate_forward", plain, y_ref, B, bound, yard, extra=f" {differ} of {fused.size} differ from the fused y |")
    finish()


def _desc(dev, entry, fm, **fields):
    """The descriptor of _linear_conv for this layer, with `fields` on top."""
    case = dev.case
    d = _lib.ConvDesc()
    d.n_src = 1
    d.src[0].data = dev.x.data_ptr()
    d.src[0].C, d.src[0].srcH, d.src[0].srcW, d.src[0].shift = case.cin, case.H, case.W, 0
    d.inH, d.inW, d.Cout, d.ksize, d.stride, d.elu = case.H, case.W, case.cout, case.k, case.stride, 0
    d.wpacked, d.params, d.out, d.out_cstride = entry.fwd.data_ptr(), entry.params.data_ptr(), fm.data_ptr(), 2 * case.cout
    d.config, d.linear = -1, 1
    if dev.route.fwd == _lib.PACK_W4:
        d.wpacked_w4 = entry.fwd.data_ptr()
    elif dev.route.fwd == _lib.PACK_WINO:
        d.wpacked_wino = entry.fwd.data_ptr()
    for key, value in fields.items():
        setattr(d, key, value)
    return d


REFUSALS = [("out_gated on a direct launch", (8, 16, 3, 1), dict()),
            ("out_gated without linear", (16, 32, 3, 1), dict(linear=0)),
            ("out_gated without linear (F(4x4))", (32, 32, 3, 1), dict(linear=0)),
            ("a misaligned out_gated", (16, 32, 3, 1), dict(misalign=4)),
            ("a misaligned out_gated (F(4x4))", (32, 32, 3, 1), dict(misalign=4)),
            ("valid_h > block_h", (16, 32, 3, 1), dict(block_h=4, valid_h=5)),
            ("valid_h > block_h (F(4x4))", (32, 32, 3, 1), dict(block_h=4, valid_h=5))]


@pytest.mark.parametrize("what,layer,fields", REFUSALS, ids=[r[0].replace(" ", "_") for r in REFUSALS])
def test_out_gated_is_refused_on_the_host(hip, what, layer, fields):
    """Assertion 5 (take_out_gated): the argument error, and neither buffer touched — every pointer of these descriptors is valid."""
    from read_amd import train
    case = next(FC.cases(layer, (9, 21), classes="a"))
    dev = _Layer(train, case, FAMILY_OF_KIND[train.layer_route(*layer).fwd])
    entry = train._packed_for(dev.route, dev.ts)
    n_fm, n_y = case.oh * case.ow * 2 * case.cout, case.oh * case.ow * case.cout
    fm = torch.full((n_fm + GUARD,), float(SENTINEL), device="cuda")
    y = torch.full((n_y + GUARD,), float(SENTINEL), device="cuda")
    fields = dict(fields)
    d = _desc(dev, entry, fm, out_gated=y.data_ptr() + fields.pop("misalign", 0), **fields)
    rc = hip.read_gated_conv_forward(ctypes.byref(d), _lib.stream_ptr())
    assert rc == READ_EINVAL, f"{what}: read_gated_conv_forward returned {rc}"
    assert b"out_gated" in hip.read_last_error()
    assert bool((_host(fm) == SENTINEL).all()) and bool((_host(y) == SENTINEL).all()), f"{what}: a refused launch wrote"
