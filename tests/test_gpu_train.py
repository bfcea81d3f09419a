"""Parity of the native training step with torch.autograd through the oracle (oracle/unet_torch.py,
the functional restatement of the reference's modules): per-layer gradients of every BasicConv flavour, the bilinear x4
adjoint, the Huber loss, the full UNet backward on a crop, the sparse descriptor RMSprop against torch.optim.RMSprop, and
one whole optimisation step through TexturePipeline.  Stated tolerance: gradients rtol 1e-4 of the largest gradient entry of
the tensor (fp32, different summation orders; wgrad sums ~10^4..10^5 products per weight).
This file stays the END-TO-END parity test (autograd through GatedConvFn / UNet.backward, the UNet's own geometry).  What each kernel
costs per element — every C entry point called directly, float64 references, derived bounds, the shapes and value ranges where the
kernels can go wrong — lives in tests/test_gpu_train_accuracy.py (tests/train_ref64.py, profiles/train_accuracy_fp64.md)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import unet_torch
from read_amd import synthetic
from read_amd.train import GatedConvFn, SparseDescriptorRMSprop, Up4Fn, huber_loss, unet_forward_train
from read_amd.unet import UNet
from tests.unet_spec import UNET_SPEC

pytestmark = pytest.mark.gpu

RTOL = 1e-4


def _close(got, ref, what, rtol=RTOL):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = max(float(ref.abs().max()), 1e-30)
    err = float((got - ref).abs().max()) / scale
    assert err <= rtol, f"{what}: max error {err:.3e} of the largest entry ({scale:.3e})"
    return err


@pytest.mark.parametrize("cin,cout,k,stride,elu,H,W", [
    (32, 32, 3, 1, True, 24, 40), (64, 64, 3, 1, False, 17, 33), (8, 32, 3, 1, True, 32, 48), (32, 3, 3, 1, False, 16, 32),
    (48, 40, 3, 1, True, 9, 21),          # F(4x4) linear launches with a padded last channel group, odd image size
    (64, 64, 3, 1, False, 16, 36), (128, 32, 3, 1, True, 8, 8), (32, 64, 3, 1, True, 136, 32),    # Winograd-domain wgrad: partial tile group, one tile row, several splits
    (480, 32, 1, 1, True, 16, 24), (64, 56, 1, 1, True, 12, 20), (16, 32, 1, 1, True, 9, 31), (128, 64, 1, 1, False, 10, 18),
    (32, 64, 3, 2, True, 32, 48), (128, 256, 3, 2, True, 16, 16), (256, 128, 4, 2, True, 16, 24), (64, 32, 4, 2, True, 32, 32),
])
def test_gated_conv_layer_gradients(hip, cin, cout, k, stride, elu, H, W):
    rng = np.random.default_rng(cin * 1000 + cout + k)
    b = 1.0 / np.sqrt(cin * k * k)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32))
    p = dict(wf=t(rng.uniform(-b, b, (cout, cin, k, k))), bf=t(rng.uniform(-b, b, cout)), wm=t(rng.uniform(-b, b, (cout, cin, k, k))),
             bm=t(rng.uniform(-b, b, cout)), gamma=t(rng.uniform(0.5, 1.5, cout)), beta=t(0.1 * rng.standard_normal(cout)),
             mean=t(0.1 * rng.standard_normal(cout)), var=t(rng.uniform(0.5, 1.5, cout)))
    x = t(rng.standard_normal((1, cin, H, W)))
    pad = (k - 1) // 2
    # oracle: the reference's BasicConv arithmetic under torch.autograd
    ref_in = {n: v.clone().requires_grad_(n not in ("mean", "var")) for n, v in p.items()}
    xr = x.clone().requires_grad_(True)
    f = F.conv2d(xr, ref_in["wf"], ref_in["bf"], stride=stride, padding=pad)
    m = F.conv2d(xr, ref_in["wm"], ref_in["bm"], stride=stride, padding=pad)
    yr = F.batch_norm((F.elu(f) if elu else f) * torch.sigmoid(m), ref_in["mean"], ref_in["var"], ref_in["gamma"], ref_in["beta"],
                      training=False, eps=1e-5)
    g = t(rng.standard_normal(tuple(yr.shape)))
    yr.backward(g)
    # HIP
    dev = {n: v.cuda().requires_grad_(n not in ("mean", "var")) for n, v in p.items()}
    xd = x[0].permute(1, 2, 0).contiguous().cuda().requires_grad_(True)
    y = GatedConvFn.apply(xd, dev["wf"], dev["bf"], dev["wm"], dev["bm"], dev["gamma"], dev["beta"], dev["mean"], dev["var"], k, stride, elu)
    _close(y.permute(2, 0, 1)[None], yr, "forward", rtol=2e-5)
    y.backward(g[0].permute(1, 2, 0).contiguous().cuda())
    _close(xd.grad.permute(2, 0, 1)[None], xr.grad, "dx")
    for n in ("wf", "wm", "bf", "bm", "gamma", "beta"):
        _close(dev[n].grad, ref_in[n].grad, "d" + n)


def test_winograd_domain_wgrad_equals_the_direct_kernel(hip):
    """read_conv_wgrad on 3x3 / stride-1 layers: the F(4x4,3x3)-domain kernel (dg = G^T [sum_tiles (B^T d B) . (A dY A^T)] G; 4x
    fewer multiplications) against the direct MFMA kernel (knob wgrad_wino = 0) and against torch's conv2d weight gradient, on the
    UNet's channel counts, with partial tile groups (W / 4 not a multiple of 8), a padded d[f|m] tile (Cout = 3), accumulation."""
    from read_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(77)
    for (cin, cout, H, W) in ((32, 32, 128, 64), (64, 64, 64, 96), (128, 128, 32, 36), (256, 256, 16, 16), (32, 3, 32, 64), (64, 40, 20, 28)):
        cp = (cout + 7) // 8 * 8
        x = torch.from_numpy(rng.standard_normal((H, W, cin)).astype(np.float32)).cuda()
        dfm = torch.zeros((H, W, 2 * cp), dtype=torch.float32)
        dfm[:, :, :cout] = torch.from_numpy(rng.standard_normal((H, W, cout)).astype(np.float32))
        dfm[:, :, cp:cp + cout] = torch.from_numpy(rng.standard_normal((H, W, cout)).astype(np.float32))
        dfm = dfm.cuda()
        n_scr = L.read_conv_wgrad_scratch_floats(cin, cout, 3, H)
        scratch = torch.empty(n_scr, dtype=torch.float32, device="cuda")
        got = {}
        try:
            for knob in (1, 0):
                _lib.check(L.read_tuning_set(b"wgrad_wino", knob))
                dwf = torch.full((cout, cin, 3, 3), 7.0, device="cuda")
                dwm = torch.full((cout, cin, 3, 3), -3.0, device="cuda")
                _lib.check(L.read_conv_wgrad(x.data_ptr(), H, W, cin, dfm.data_ptr(), cout, 3, 1, dwf.data_ptr(), dwm.data_ptr(), 0,
                                             scratch.data_ptr(), n_scr, _lib.stream_ptr()))
                got[knob] = (dwf.clone(), dwm.clone())
                _lib.check(L.read_conv_wgrad(x.data_ptr(), H, W, cin, dfm.data_ptr(), cout, 3, 1, dwf.data_ptr(), dwm.data_ptr(), 1,
                                             scratch.data_ptr(), n_scr, _lib.stream_ptr()))            # accumulate: twice the gradient
                _close(dwf, 2 * got[knob][0], f"accumulate {cin}->{cout} knob {knob}", rtol=1e-6)
        finally:
            _lib.check(L.read_tuning_set(b"wgrad_wino", 1))
        xc = x.cpu().permute(2, 0, 1)[None].double()
        for half, name in ((0, "dwf"), (1, "dwm")):
            g = dfm.cpu()[:, :, half * cp:half * cp + cout].permute(2, 0, 1)[None].double()
            ref = torch.nn.grad.conv2d_weight(xc, (cout, cin, 3, 3), g, padding=1)
            e1 = _close(got[1][half], ref, f"winograd {name} {cin}->{cout} {H}x{W}", rtol=2e-5)
            e0 = _close(got[0][half], ref, f"direct {name} {cin}->{cout} {H}x{W}", rtol=2e-5)
            print(f"{cin}->{cout} {H}x{W} {name}: winograd {e1:.2e} direct {e0:.2e} of the largest entry")
        assert not torch.equal(got[1][0], got[0][0])                     # the knob really switches kernels


def test_up4_and_huber(hip):
    rng = np.random.default_rng(1)
    x = torch.from_numpy(rng.standard_normal((1, 16, 9, 13)).astype(np.float32))
    xr = x.clone().requires_grad_(True)
    yr = F.interpolate(xr, scale_factor=4, mode="bilinear", align_corners=False)
    g = torch.from_numpy(rng.standard_normal(tuple(yr.shape)).astype(np.float32))
    yr.backward(g)
    xd = x[0].permute(1, 2, 0).contiguous().cuda().requires_grad_(True)
    y = Up4Fn.apply(xd)
    _close(y.permute(2, 0, 1)[None], yr, "up4 forward", rtol=1e-6)
    y.backward(g[0].permute(1, 2, 0).contiguous().cuda())
    _close(xd.grad.permute(2, 0, 1)[None], xr.grad, "up4 backward", rtol=1e-5)
    out = torch.from_numpy((2.0 * rng.standard_normal((2, 3, 20, 24))).astype(np.float32))       # both Huber branches
    tgt = torch.from_numpy(rng.random((2, 3, 20, 24)).astype(np.float32))
    o_r = out.clone().requires_grad_(True)
    l_r = F.huber_loss(o_r, tgt)
    (1e4 * l_r).backward()                                                                          # huber_ratio, train.py:549
    o_d = out.cuda().requires_grad_(True)
    l_d = huber_loss(o_d, tgt.cuda())
    (1e4 * l_d).backward()
    assert abs(float(l_d.detach()) - float(l_r.detach())) <= 1e-6 * abs(float(l_r.detach()))
    _close(o_d.grad, o_r.grad, "huber grad", rtol=1e-6)


def test_unet_training_graph_vs_oracle_autograd(hip):
    """The whole UNet on a batch of three 64x96 crops (stacked into one tall image with zero separator rows by the HIP
    graph): output, input gradients (they become descriptor gradients) and all 594 parameter gradients against
    torch.autograd through the oracle's functional restatement of the reference modules, which sees a plain batch."""
    H, W, B = 64, 96, 3
    state = synthetic.make_unet_state(UNET_SPEC, 13)
    net = UNet()
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    net.cuda().eval()
    rng = np.random.default_rng(3)
    xs = [torch.from_numpy(rng.random((B, 8, H >> l, W >> l)).astype(np.float32)) for l in range(4)]
    # oracle
    st_r = {k: torch.from_numpy(np.asarray(v)).clone().requires_grad_(np.asarray(v).dtype == np.float32 and "running" not in k)
            for k, v in state.items()}
    xs_r = [x.clone().requires_grad_(True) for x in xs]
    out_r = unet_torch.unet_forward(st_r, *xs_r)
    g = torch.from_numpy(rng.standard_normal(tuple(out_r.shape)).astype(np.float32))
    out_r.backward(g)
    # HIP
    xs_d = [x.cuda().requires_grad_(True) for x in xs]
    out = net(*xs_d)
    assert out.shape == (B, 3, H, W) and out.grad_fn is not None
    _close(out, out_r, "forward", rtol=2e-5)
    out.backward(g.cuda())
    for l in range(4):
        _close(xs_d[l].grad, xs_r[l].grad, f"dx level {l}")
    worst = 0.0
    n = 0
    for name, p in net.named_parameters():
        ref = st_r[name].grad
        if name.startswith("ConvsOut."):                            # never executed (unet.py:181-186): no gradient on either side
            assert p.grad is None and ref is None, name
            continue
        assert p.grad is not None and ref is not None, name
        worst = max(worst, _close(p.grad, ref, name, rtol=2e-4))
        n += 1
    # 99 executed BasicConvs x 6 trainable tensors (ConvsOut.* are never executed: no gradient, unet.py:181-186)
    print(f"{n} parameter gradients, worst relative error {worst:.2e}")
    assert n >= 594
    # a single item takes the unstacked graph and gives the same numbers
    one = net(*[x[1:2].cuda().requires_grad_(True) for x in xs])
    _close(one, out_r[1:2], "single-item training forward", rtol=2e-5)
    # inference afterwards still uses the fused plan and sees the same weights
    with torch.no_grad():
        y2 = net(*[x.cuda() for x in xs])
    _close(y2, out_r, "fused forward after training forward", rtol=2e-5)


@pytest.mark.parametrize("cin,cout,k,stride,elu,H,W,nb", [
    (32, 32, 3, 1, True, 24, 40, 1), (64, 64, 3, 1, False, 2 * (16 + 4), 32, 2), (8, 32, 3, 1, True, 32, 48, 1),
    (64, 56, 1, 1, True, 12, 20, 1), (32, 64, 3, 2, True, 32, 48, 1), (256, 128, 4, 2, True, 16, 24, 1), (32, 3, 3, 1, False, 16, 32, 1),
    # negative nb: |nb| stacked items, each its OWN BatchNorm batch (the net called once per item, compose.py:137-176)
    (32, 32, 3, 1, True, 16, 24, -3), (8, 32, 3, 1, True, 16, 40, -2), (64, 56, 1, 1, False, 16, 20, -4),
])
def test_gated_conv_layer_batch_statistics_batchnorm(hip, cin, cout, k, stride, elu, H, W, nb):
    """One BasicConv with nn.BatchNorm2d in .train() (unet.py:40,51; the reference's default, train.py:271-279): output, every
    gradient and the running-buffer update against torch's F.batch_norm(training=True).  nb = 2: two items stacked with
    separator rows — the statistics count the items' pixels only."""
    rng = np.random.default_rng(cin * 77 + cout + k)
    b = 1.0 / np.sqrt(cin * k * k)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32))
    p = dict(wf=t(rng.uniform(-b, b, (cout, cin, k, k))), bf=t(rng.uniform(-b, b, cout)), wm=t(rng.uniform(-b, b, (cout, cin, k, k))),
             bm=t(rng.uniform(-b, b, cout)), gamma=t(rng.uniform(0.5, 1.5, cout)), beta=t(0.1 * rng.standard_normal(cout)),
             mean=t(0.1 * rng.standard_normal(cout)), var=t(rng.uniform(0.5, 1.5, cout)))
    pad = (k - 1) // 2
    per_item, nb = nb < 0, abs(nb)
    if nb == 1:
        x = t(rng.standard_normal((1, cin, H, W)))
        xb = x
    else:                                                     # items of 16 rows + 4 zero separator rows each
        items = t(rng.standard_normal((nb, cin, 16, W)))
        xb = items
        x = torch.nn.functional.pad(items, (0, 0, 0, 4)).permute(1, 0, 2, 3).reshape(1, cin, nb * 20, W)
    ref_in = {n: v.clone().requires_grad_(n not in ("mean", "var")) for n, v in p.items()}
    xr = xb.clone().requires_grad_(True)
    f = F.conv2d(xr, ref_in["wf"], ref_in["bf"], stride=stride, padding=pad)
    m = F.conv2d(xr, ref_in["wm"], ref_in["bm"], stride=stride, padding=pad)
    rm, rv = p["mean"].clone(), p["var"].clone()
    gated = (F.elu(f) if elu else f) * torch.sigmoid(m)
    if per_item:      # one F.batch_norm call per item, in order: own statistics, the running buffers move nb times
        yr = torch.cat([F.batch_norm(gated[b:b + 1], rm, rv, ref_in["gamma"], ref_in["beta"], training=True, momentum=0.1, eps=1e-5)
                        for b in range(nb)], 0)
    else:
        yr = F.batch_norm(gated, rm, rv, ref_in["gamma"], ref_in["beta"], training=True, momentum=0.1, eps=1e-5)
    g = t(rng.standard_normal(tuple(yr.shape)))
    yr.backward(g)
    dev = {n: v.cuda().requires_grad_(n not in ("mean", "var")) for n, v in p.items()}
    xd = x[0].permute(1, 2, 0).contiguous().cuda().requires_grad_(True)
    blk = (1, 1, 1) if nb == 1 else (nb, 16, 20)
    y = GatedConvFn.apply(xd, dev["wf"], dev["bf"], dev["wm"], dev["bm"], dev["gamma"], dev["beta"], dev["mean"], dev["var"], k,
                          stride, elu, *blk, 2 if per_item else True)
    if nb == 1:
        y_cmp, unstack = y.permute(2, 0, 1)[None], lambda a: a.permute(2, 0, 1)[None]
        gd = g[0].permute(1, 2, 0).contiguous()
    else:
        unstack = lambda a: a.reshape(nb, 20, W, -1)[:, :16].permute(0, 3, 1, 2)
        y_cmp = unstack(y)
        assert float(y.detach().reshape(nb, 20, W, -1)[:, 16:].abs().max()) == 0.0          # separators stay zero
        gd = torch.nn.functional.pad(g.permute(0, 2, 3, 1), (0, 0, 0, 0, 0, 4)).reshape(nb * 20, W, cout).contiguous()
    _close(y_cmp, yr, "forward", rtol=5e-5)
    _close(dev["mean"], rm, "running_mean", rtol=1e-5)
    _close(dev["var"], rv, "running_var", rtol=1e-5)
    y.backward(gd.cuda())
    _close(unstack(xd.grad), xr.grad, "dx")
    for n in ("wf", "wm", "bf", "bm", "gamma", "beta"):
        _close(dev[n].grad, ref_in[n].grad, "d" + n, rtol=2e-4)


def test_unet_batch_statistics_mode_vs_oracle(hip):
    """model.train() — the reference's DEFAULT training mode (train.py:271-279,450): the whole UNet on a stacked batch with
    batch-statistics BatchNorm in every BasicConv against the oracle with training=True (itself pinned against the reference's
    own UNet in .train(), tests/test_oracle_unet.py): output, input gradients, parameter gradients, running buffers; and
    the eval-mode fused plan afterwards sees the moved running statistics."""
    H, W, B = 48, 64, 3
    state = synthetic.make_unet_state(UNET_SPEC, 17)
    net = UNet()
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    net.cuda().train()
    rng = np.random.default_rng(5)
    xs = [torch.from_numpy(rng.random((B, 8, H >> l, W >> l)).astype(np.float32)) for l in range(4)]
    st_r = {k: torch.from_numpy(np.asarray(v)).clone().requires_grad_(np.asarray(v).dtype == np.float32 and "running" not in k)
            for k, v in state.items()}
    xs_r = [x.clone().requires_grad_(True) for x in xs]
    out_r = unet_torch.unet_forward(st_r, *xs_r, training=True)
    g = torch.from_numpy(rng.standard_normal(tuple(out_r.shape)).astype(np.float32))
    out_r.backward(g)
    xs_d = [x.cuda().requires_grad_(True) for x in xs]
    out = net(*xs_d)
    _close(out, out_r, "forward (batch statistics)", rtol=1e-4)
    out.backward(g.cuda())
    for l in range(4):
        _close(xs_d[l].grad, xs_r[l].grad, f"dx level {l}", rtol=5e-4)
    worst, n = 0.0, 0
    for name, p in net.named_parameters():
        if name.startswith("ConvsOut."):
            continue
        worst = max(worst, _close(p.grad, st_r[name].grad, name, rtol=1e-3))
        n += 1
    print(f"{n} parameter gradients in batch-statistics mode, worst relative error {worst:.2e}")
    assert n >= 594
    sd = net.state_dict()
    for k in sd:
        if "running_" in k and not k.startswith("ConvsOut."):
            _close(sd[k].cpu(), st_r[k], k, rtol=1e-4)
        if k.endswith("num_batches_tracked") and not k.startswith("ConvsOut."):
            assert int(sd[k]) == 1, k
    # eval afterwards: the fused plan re-packs and uses the running statistics the training pass just moved
    net.eval()
    with torch.no_grad():
        y_eval = net(*[x.cuda() for x in xs])
        ref_eval = unet_torch.unet_forward(st_r, *xs)
    _close(y_eval, ref_eval, "fused eval forward after a train-mode pass", rtol=2e-5)


@pytest.mark.parametrize("train_mode", [False, True], ids=["eval", "batch-statistics"])
@pytest.mark.parametrize("B,H,W", [(3, 16, 16), (1, 32, 16)])
def test_unet_training_graph_at_16_pixel_crops_vs_fp64_autograd(hip, B, H, W, train_mode):
    """The two graph tests above at the smallest crops the library accepts: three stacked 16 x 16 crops (levels 16 x 16 ... 2 x 2 per
    item, feat_extract.7 writes ONE pixel per item) and one 32 x 16 crop, against torch.autograd through the oracle in FLOAT64.  The
    same measure (_close) and the same tolerances: 2e-5 forward / 1e-4 input gradients / 2e-4 parameter gradients in eval mode,
    1e-4 / 5e-4 / 1e-3 with batch statistics; all 594 parameter gradients and the four input gradients.  Every miss is collected and
    reported together."""
    f_tol, x_tol, p_tol = (1e-4, 5e-4, 1e-3) if train_mode else (2e-5, RTOL, 2e-4)
    state = synthetic.make_unet_state(UNET_SPEC, 13 if not train_mode else 17)
    net = UNet()
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    net.cuda()
    net.train() if train_mode else net.eval()
    rng = np.random.default_rng([3, B, H, W])
    xs = [torch.from_numpy(rng.random((B, 8, H >> l, W >> l)).astype(np.float32)) for l in range(4)]
    st_r = {k: torch.from_numpy(np.asarray(v)).double().requires_grad_("running" not in k) for k, v in state.items() if np.asarray(v).dtype == np.float32}
    xs_r = [x.double().requires_grad_(True) for x in xs]
    out_r = unet_torch.unet_forward(st_r, *xs_r, training=train_mode)
    assert out_r.dtype == torch.float64
    g = torch.from_numpy(rng.standard_normal(tuple(out_r.shape)).astype(np.float32))
    out_r.backward(g.double())
    xs_d = [x.cuda().requires_grad_(True) for x in xs]
    out = net(*xs_d)
    assert out.shape == (B, 3, H, W) and out.grad_fn is not None
    missed = []

    def close(got, ref, what, rtol):
        try:
            return _close(got, ref, what, rtol=rtol)
        except AssertionError as e:
            missed.append(str(e))
            return float("nan")

    close(out, out_r, "forward", f_tol)
    out.backward(g.cuda())
    for l in range(4):
        close(xs_d[l].grad, xs_r[l].grad, f"dx level {l}", x_tol)
    errs = []
    for name, p in net.named_parameters():
        if name.startswith("ConvsOut."):                            # never executed (unet.py:181-186)
            continue
        assert p.grad is not None and st_r[name].grad is not None, name
        errs.append(close(p.grad, st_r[name].grad, name, p_tol))
    print(f"B={B} {H}x{W} {'batch statistics' if train_mode else 'eval'}: {len(errs)} parameter gradients, worst relative error {np.nanmax(errs):.2e}, {len(missed)} missed")
    assert len(errs) >= 594
    if train_mode:
        # the running statistics the pass moved (over 1 - 4 pixels per item at the coarse levels), then the fused eval plan on them
        sd = net.state_dict()
        for k in sd:
            if "running_" in k and not k.startswith("ConvsOut."):
                close(sd[k].cpu(), st_r[k], k, 1e-4)
            if k.endswith("num_batches_tracked") and not k.startswith("ConvsOut."):
                assert int(sd[k]) == 1, k
        net.eval()
        with torch.no_grad():
            y_eval = net(*[x.cuda() for x in xs])
            ref_eval = unet_torch.unet_forward(st_r, *[x.double() for x in xs])
        close(y_eval, ref_eval, "fused eval forward after a train-mode pass", 2e-5)
    else:
        # a single item takes the unstacked graph; inference afterwards still uses the fused plan and sees the same weights
        one = net(*[x[B - 1:B].cuda().requires_grad_(True) for x in xs])
        close(one, out_r[B - 1:B], "single-item training forward", 2e-5)
        with torch.no_grad():
            y2 = net(*[x.cuda() for x in xs])
        close(y2, out_r, "fused forward after training forward", 2e-5)
    assert not missed, f"{len(missed)} tensors outside their tolerance: " + "; ".join(missed[:12])


def test_batch_statistics_over_one_pixel_on_a_single_16_pixel_crop(hip):
    """One 16 x 16 crop in .train(): feat_extract.7 writes ONE pixel, so its BatchNorm has one value per channel.  The reference
    refuses that (torch's F.batch_norm raises ValueError; asserted on the oracle), so there is no graph to compare with; what the
    library does there is stated and held: it runs, the batch variance of that layer is 0 (its running_var moves to 0.9 of the old
    value: momentum 0.1, unbiased = biased at a count of one), and output and gradients are finite.  The kernels at a count of one
    against float64: tests/test_gpu_train_accuracy.py, the degenerate batch-statistics rows."""
    H = W = 16
    state = synthetic.make_unet_state(UNET_SPEC, 17)
    net = UNet()
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    net.cuda().train()
    rng = np.random.default_rng([5, H, W])
    xs = [torch.from_numpy(rng.random((1, 8, H >> l, W >> l)).astype(np.float32)) for l in range(4)]
    st_r = {k: torch.from_numpy(np.asarray(v)).clone() for k, v in state.items()}
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        unet_torch.unet_forward(st_r, *xs, training=True)
    xs_d = [x.cuda().requires_grad_(True) for x in xs]
    out = net(*xs_d)
    out.backward(torch.ones_like(out))
    assert bool(torch.isfinite(out).all()) and all(bool(torch.isfinite(x.grad).all()) for x in xs_d)
    assert all(bool(torch.isfinite(p.grad).all()) for n, p in net.named_parameters() if not n.startswith("ConvsOut."))
    key = "feat_extract.7.block.norm.running_var"
    _close(net.state_dict()[key].cpu(), 0.9 * torch.from_numpy(np.asarray(state[key])), key, rtol=1e-6)


def test_sparse_rmsprop_equals_dense_torch_rmsprop(hip):
    """Rows touched in some steps only: the lazily decayed sparse update must follow torch.optim.RMSprop's dense trajectory."""
    from read_amd.texture import PointTexture
    N, Cc = 4000, 8
    rng = np.random.default_rng(4)
    init = rng.random((1, Cc, N)).astype(np.float32)
    tex = PointTexture(Cc, N, init_method='zeros')
    with torch.no_grad():
        tex.texture_.copy_(torch.from_numpy(init))
    tex.cuda()
    tex.sparse_training = True
    opt = SparseDescriptorRMSprop([tex], lr=0.1)
    ref_p = torch.nn.Parameter(torch.from_numpy(init.copy()))
    ref_opt = torch.optim.RMSprop([ref_p], lr=0.1)
    for step in range(6):
        ids_np = rng.integers(0, N if step != 2 else N // 10, (2, 1, 24, 32))
        if step == 3:
            ids_np.reshape(-1)[rng.permutation(ids_np.size)[:800]] = 0         # background: one run of > 512 equal ids
        ids = torch.from_numpy(ids_np.astype(np.float32))
        w = torch.from_numpy(rng.standard_normal((2, Cc, 24, 32)).astype(np.float32))
        (tex(ids.cuda()) * w.cuda()).sum().backward()
        if step == 4:       # the dense gradient rows on request (then the optimizer consumes them instead of the sorted pairs)
            dense = torch.zeros(N, Cc).index_add_(0, ids.reshape(2, -1).long().reshape(-1),
                                                  w.permute(0, 2, 3, 1).reshape(-1, Cc))
            _close(tex.grad_rows(), dense, "dense gradient rows", rtol=1e-5)
        opt.step()
        opt.zero_grad()
        ref_opt.zero_grad()
        (ref_p[0][:, ids[:, 0].long()].permute(1, 0, 2, 3) * w).sum().backward()
        ref_opt.step()
        assert tex.texture_.grad is None
    got = tex.state_dict()["texture_"].cpu()                       # state_dict() writes the rows back into texture_
    _close(got, ref_p.detach(), "descriptors after 6 sparse steps", rtol=1e-5)
    assert float(tex.grad_rows().abs().max()) == 0.0               # gradient rows are clean again
    # forward after the steps serves the updated rows
    ids = torch.arange(64, dtype=torch.float32).view(1, 1, 8, 8)
    with torch.no_grad():
        _close(tex(ids.cuda()), ref_p.detach()[0][:, ids[0, 0].long()][None], "lookup after training", rtol=1e-5)


def test_texture_pipeline_training_step(hip):
    """B5: TexturePipeline.create in training mode (datasets + criterion supplied like the reference's args), two full
    optimisation steps (HIP forward/backward, Adam on the net, sparse RMSprop on the descriptors) against the same steps done
    with torch modules of the oracle and torch optimizers."""
    from types import SimpleNamespace
    from read_amd.pipeline import TexturePipeline
    H, W, N = 32, 48, 3000
    rng = np.random.default_rng(6)

    class DS:
        id, name = 0, "scene0"
        scene_data = {'pointcloud': {'xyz': np.zeros((N, 3), np.float32)}}
        def load(self): pass
        def unload(self): pass

    class Crit(torch.nn.Module):
        def forward(self, out, target):
            return huber_loss(out, target)

    args = SimpleNamespace(inference=False, descriptor_size=8, texture_activation='none', use_mesh=False, supersampling=1,
                           lr=1e-3, texture_lr=1e-1, texture_ckpt=None, get_datasets=lambda a: ([DS()], [DS()]),
                           criterion_module=Crit, criterion_args={}, pipeline='READ.pipelines.ogl.TexturePipeline')
    pipe = TexturePipeline()
    pipe.create(args)
    state = synthetic.make_unet_state(UNET_SPEC, 2)
    pipe.net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    tex = pipe.textures[0]
    init = rng.random((1, 8, N)).astype(np.float32)
    with torch.no_grad():
        tex.texture_.copy_(torch.from_numpy(init))
    model = pipe.model.cuda()
    pipe.dataset_load([DS()])
    model.cuda().eval()                                             # eval_in_train: True (train.py:271-277)
    extra = pipe.extra_optimizer([DS()])
    assert isinstance(extra, SparseDescriptorRMSprop)
    # oracle twin
    st_r = {k: torch.nn.Parameter(torch.from_numpy(np.asarray(v)).clone()) if (np.asarray(v).dtype == np.float32 and "running" not in k)
            else torch.from_numpy(np.asarray(v)).clone() for k, v in state.items()}
    tex_r = torch.nn.Parameter(torch.from_numpy(init.copy()))
    opt_r = torch.optim.Adam([p for p in st_r.values() if isinstance(p, torch.nn.Parameter)], lr=1e-3)
    ext_r = torch.optim.RMSprop([tex_r], lr=1e-1)
    keys = "uv_1d_p1, uv_1d_p1_ds1, uv_1d_p1_ds2, uv_1d_p1_ds3, uv_1d_p1_ds4".replace(' ', '').split(',')
    g_ref = []
    for step in range(2):
        maps = [rng.integers(0, N, (2, 1, H >> l, W >> l)) for l in range(5)]
        target = torch.from_numpy(rng.random((2, 3, H, W)).astype(np.float32))
        inputs = {'id': torch.tensor([0, 0])}
        inputs.update({k: torch.from_numpy(m).float().cuda() for k, m in zip(keys, maps)})
        out = model(inputs)
        loss = pipe.criterion(out, target.cuda()) * 1e4
        loss.backward()
        pipe.optimizer.step()
        pipe.optimizer.zero_grad()
        extra.step()
        extra.zero_grad()
        outs = []
        for b in range(2):
            feats = [tex_r[:, :, torch.from_numpy(m[b, 0]).long()] for m in maps]
            outs.append(unet_torch.unet_forward(st_r, *feats[:4]))
        loss_r = F.huber_loss(torch.cat(outs, 0), target) * 1e4
        loss_r.backward()
        g_ref.append(tex_r.grad.detach().clone())
        opt_r.step(); opt_r.zero_grad(); ext_r.step(); ext_r.zero_grad()
        assert abs(float(loss) - float(loss_r)) <= 1e-4 * abs(float(loss_r)), (step, float(loss), float(loss_r))
    # RMSprop's first steps move a descriptor by lr * g / (sqrt(0.01 g^2) + 1e-8) ~ 10 lr sign(g): an entry whose gradient is at
    # round-off level takes an update that depends on the last bits of g — ill-conditioned by construction.  So: entries whose
    # reference gradient is above 1e-4 of the largest one in both steps (or exactly zero: untouched rows) are compared at 2e-3 of
    # the largest entry; the others only against the size of the steps themselves (2 steps x 10 lr).  The gradients themselves are
    # held to 1e-4 by the tests above.
    got, ref = tex.state_dict()["texture_"].cpu().double(), tex_r.detach().double()
    gmax = max(float(g.abs().max()) for g in g_ref)
    well = torch.ones_like(ref, dtype=torch.bool)
    for g in g_ref:
        well &= (g.abs() > 1e-4 * gmax) | (g == 0)
    assert float(well.double().mean()) > 0.5, "the well-conditioned set must be most of the table"
    scale = float(ref.abs().max())
    err_well = float(((got - ref).abs() * well).max()) / scale
    assert err_well <= 2e-3, f"descriptors after two steps (well-conditioned entries): {err_well:.3e} of the largest entry"
    assert float((got - ref).abs().max()) <= 2 * 10 * 1e-1 + 1e-6, "an ill-conditioned entry moved by more than the two steps can"
    sd = pipe.net.state_dict()
    for name in ("feat_extract.0.block.conv_f.weight", "Encoder.3.layers.2.main.0.block.conv_m.weight", "feat_extract.5.block.norm.weight",
                 "AFFs.1.conv.0.block.conv_f.bias"):
        _close(sd[name].cpu(), st_r[name].detach(), name, rtol=2e-3)   # Adam divides by sqrt(v): early steps amplify round-off


def test_sparse_descriptors_survive_unload_and_load(hip):
    """the train loop moves the texture off the device between train and eval (train.py:271-305 ->
    dataset_unload -> unload_textures -> .cpu(), then dataset_load / model.cuda()).  Rows stepped by the sparse optimizer must
    be written back into texture_ BEFORE it leaves the device, so eval, checkpoints and the next epoch see the trained rows."""
    from read_amd.net_texture import NetAndTexture
    from read_amd.texture import PointTexture
    N, Cc = 3000, 8
    rng = np.random.default_rng(11)
    init = rng.random((1, Cc, N)).astype(np.float32)
    tex = PointTexture(Cc, N, init_method='zeros')
    with torch.no_grad():
        tex.texture_.copy_(torch.from_numpy(init))
    tex.sparse_training = True
    model = NetAndTexture(UNet(), {0: tex})
    model.load_textures(0)
    model.cuda()
    opt = SparseDescriptorRMSprop([tex], lr=0.1)
    ref_p = torch.nn.Parameter(torch.from_numpy(init.copy()))
    ref_opt = torch.optim.RMSprop([ref_p], lr=0.1)

    def one_step():
        ids = torch.from_numpy(rng.integers(0, N, (2, 1, 16, 24)).astype(np.float32))
        w = torch.from_numpy(rng.standard_normal((2, Cc, 16, 24)).astype(np.float32))
        (tex(ids.cuda()) * w.cuda()).sum().backward()
        opt.step()
        ref_opt.zero_grad()
        (ref_p[0][:, ids[:, 0].long()].permute(1, 0, 2, 3) * w).sum().backward()
        ref_opt.step()
    one_step()
    one_step()
    model.unload_textures()                                        # epoch boundary: texture -> CPU
    assert not tex.texture_.is_cuda
    _close(tex.texture_.detach(), ref_p.detach(), "texture_ on the CPU after unload", rtol=1e-5)     # trained values, not the initial ones
    _close(tex.state_dict()["texture_"], ref_p.detach(), "checkpoint after unload", rtol=1e-5)
    model.load_textures(0)                                         # eval / next epoch: back to the device
    model.cuda()
    probe = torch.arange(128, dtype=torch.float32).view(1, 1, 8, 16)
    with torch.no_grad():
        _close(tex(probe.cuda()), ref_p.detach()[0][:, probe[0, 0].long()][None], "lookup after reload", rtol=1e-5)
    one_step()                                                     # the optimizer state carried over (same trajectory as dense)
    _close(tex.state_dict()["texture_"].cpu(), ref_p.detach(), "descriptors after unload / load / one more step", rtol=1e-5)


def test_wgrad_when_gradients_accumulate_or_are_frozen(hip):
    """weight gradients come from a side stream; with an existing .grad (gradient accumulation) autograd adds
    on the main stream, which must wait for them; with frozen weights no wgrad is computed at all."""
    rng = np.random.default_rng(21)
    cin, cout, H, W = 32, 32, 40, 56
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32))
    b = 1.0 / np.sqrt(cin * 9)
    p = dict(wf=t(rng.uniform(-b, b, (cout, cin, 3, 3))), bf=t(rng.uniform(-b, b, cout)), wm=t(rng.uniform(-b, b, (cout, cin, 3, 3))),
             bm=t(rng.uniform(-b, b, cout)), gamma=t(rng.uniform(0.5, 1.5, cout)), beta=t(0.1 * rng.standard_normal(cout)),
             mean=t(0.1 * rng.standard_normal(cout)), var=t(rng.uniform(0.5, 1.5, cout)))
    xs = [t(rng.standard_normal((1, cin, H, W))) for _ in range(3)]
    gs = [t(rng.standard_normal((1, cout, H, W))) for _ in range(3)]
    ref_in = {n: v.clone().requires_grad_(n not in ("mean", "var")) for n, v in p.items()}
    for x, g in zip(xs, gs):
        f = F.conv2d(x, ref_in["wf"], ref_in["bf"], padding=1)
        m = F.conv2d(x, ref_in["wm"], ref_in["bm"], padding=1)
        F.batch_norm(F.elu(f) * torch.sigmoid(m), ref_in["mean"], ref_in["var"], ref_in["gamma"], ref_in["beta"], training=False,
                     eps=1e-5).backward(g)
    dev = {n: v.cuda().requires_grad_(n not in ("mean", "var")) for n, v in p.items()}
    for x, g in zip(xs, gs):                                       # three backward passes into the same .grad
        y = GatedConvFn.apply(x[0].permute(1, 2, 0).contiguous().cuda(), dev["wf"], dev["bf"], dev["wm"], dev["bm"], dev["gamma"],
                              dev["beta"], dev["mean"], dev["var"], 3, 1, True)
        y.backward(g[0].permute(1, 2, 0).contiguous().cuda())
    for n in ("wf", "wm", "bf", "bm", "gamma", "beta"):
        _close(dev[n].grad, ref_in[n].grad, "accumulated d" + n)
    frozen = {n: v.cuda() for n, v in p.items()}
    xd = xs[0][0].permute(1, 2, 0).contiguous().cuda().requires_grad_(True)
    y = GatedConvFn.apply(xd, frozen["wf"], frozen["bf"], frozen["wm"], frozen["bm"], frozen["gamma"], frozen["beta"], frozen["mean"],
                          frozen["var"], 3, 1, True)
    y.backward(gs[0][0].permute(1, 2, 0).contiguous().cuda())
    assert xd.grad is not None and all(v.grad is None for v in frozen.values())


def test_src_train_py_loop_body_with_dict_results(hip):
    """the body of the reference's headless loop (src/train.py:150-266) with its own names and call order —
    ``renderer = MyRender(); renderer.update_ds(ds_list)``, ``ModelAndLoss(pipeline.model, criterion)``,
    ``data['input'], depths = renderer.render(data)``, ``out, loss_dict = model(data_input, target, label=label, mask=mask)``,
    ``out['im_out']``, ``loss = vgg + huber * 1e4 (+ reg_loss)``, backward, both optimizers — under the src tree's result
    convention ({'im_out'}, loss dict; src/READ/models/unet.py:280, src/READ/models/compose.py:29-40), against the oracle:
    raster bit-exact, image, both loss entries, the updated net weights and descriptors."""
    from types import SimpleNamespace
    import oracle
    from read_amd import _alias, camera
    from READ.gl.myrender import MyRender                                     # the names src/train.py imports (:29, :596)
    from READ.models.compose import ModelAndLoss
    from READ.pipelines.ogl import TexturePipeline
    W, H, N, B = 64, 48, 20_000, 2
    FMT = "uv_1d_p1, uv_1d_p1_ds1, uv_1d_p1_ds2, uv_1d_p1_ds3, uv_1d_p1_ds4"
    keys = FMT.replace(' ', '').split(',')
    rng = np.random.default_rng(12)
    xyz = synthetic.make_cloud(N)

    class DS:
        id, name, tgt_sh, input_format = 0, "scene0", (W, H), FMT
        scene_data = {'pointcloud': {'xyz': xyz}}
        def load(self): pass
        def unload(self): pass

    class Crit(torch.nn.Module):                       # stands in for the VGG criterion (its weights are a download)
        def forward(self, out, target):
            return (out - target).abs().mean()

    huber_ratio = 1e4                                  # src/train.py:550
    args = SimpleNamespace(inference=False, descriptor_size=8, texture_activation='none', use_mesh=False, supersampling=1,
                           lr=1e-3, texture_lr=1e-1, texture_ckpt=None, merge_loss=True, use_mask=False, headless=True,
                           # src/READ/pipelines/ogl.py:94: get_datasets returns (train, val, {id: texture checkpoint})
                           get_datasets=lambda a: ([DS()], [DS()], {0: None}),
                           criterion_module=Crit, criterion_args={}, pipeline='READ.pipelines.ogl.TexturePipeline')
    _alias.set_result_convention('dict')
    try:
        pipeline = TexturePipeline()
        pipeline.create(args)
        assert pipeline.texture_ckpts == {0: None}
        state = synthetic.make_unet_state(UNET_SPEC, 5)
        pipeline.get_net().load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
        init = rng.random((1, 8, N)).astype(np.float32)
        with torch.no_grad():
            pipeline.textures[0].texture_.copy_(torch.from_numpy(init))
        # ---- run_epoch (src/train.py:130-152)
        model = ModelAndLoss(pipeline.model, pipeline.criterion, use_mask=args.use_mask)
        ds_list = pipeline.ds_train
        renderer = MyRender()
        renderer.update_ds(ds_list)
        pipeline.dataset_load(ds_list)
        extra_optimizer = pipeline.extra_optimizer(ds_list)
        model.cuda()
        pipeline.model.eval()                          # eval_in_train (src/train.py:311-314)
        # oracle twin
        st_r = {k: torch.nn.Parameter(torch.from_numpy(np.asarray(v)).clone()) if (np.asarray(v).dtype == np.float32 and "running" not in k)
                else torch.from_numpy(np.asarray(v)).clone() for k, v in state.items()}
        tex_r = torch.nn.Parameter(torch.from_numpy(init.copy()))
        opt_r = torch.optim.Adam([p for p in st_r.values() if isinstance(p, torch.nn.Parameter)], lr=1e-3)
        ext_r = torch.optim.RMSprop([tex_r], lr=1e-1)
        for it in range(2):
            proj = np.stack([synthetic.make_proj(W, H, f=60.0)] * B)
            view = np.stack([synthetic.sweep_pose(3 + 7 * it), synthetic.sweep_pose(21 + 5 * it)])
            data = {'input': {'id': torch.tensor([0] * B)}, 'view_matrix': torch.from_numpy(view),
                    'proj_matrix': torch.from_numpy(proj), 'target': torch.from_numpy(rng.random((B, 3, H, W)).astype(np.float32))}
            # ---- run_sub (src/train.py:153-266)
            data['input'], depths = renderer.render(data)
            inputs = data['input']
            data_input = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in inputs.items()}      # to_device
            target = data['target'].cuda()
            label, mask = None, None
            out, loss_dict = model(data_input, target, label=label, mask=mask)
            im_out = out['im_out']
            assert set(out) == {'im_out'} and set(loss_dict) == {'vgg_loss', 'huber_loss'}
            assert depths['uv_1d_p1'].shape == (B, 1, H, W)
            loss = loss_dict['vgg_loss'] + loss_dict['huber_loss'] * huber_ratio
            if hasattr(pipeline.model, 'reg_loss'):
                loss = loss + pipeline.model.reg_loss()
            loss.backward(create_graph=False)
            pipeline.optimizer.step()
            pipeline.optimizer.zero_grad()
            extra_optimizer.step()
            extra_optimizer.zero_grad()
            # ---- the same iteration on the host
            tm = camera.total_matrix(proj, view)
            outs = []
            for b in range(B):
                oi, od = oracle.raster_multiscale(xyz, tm[b], W, H, 5)
                for l, k in enumerate(keys):
                    assert np.array_equal(inputs[k][b, 0].cpu().numpy(), oracle.index_to_float(oi[l])), (it, b, k)
                    assert np.array_equal(depths[k][b, 0].cpu().numpy().view(np.uint32), od[l].view(np.uint32))
                feats = [tex_r[:, :, torch.from_numpy(oi[l].astype(np.int64))] for l in range(4)]
                outs.append(unet_torch.unet_forward(st_r, *feats))
            im_r = torch.cat(outs, 0)
            vgg_r, hub_r = (im_r - data['target']).abs().mean(), F.huber_loss(im_r, data['target'])
            (vgg_r + hub_r * huber_ratio).backward()
            opt_r.step(); opt_r.zero_grad(); ext_r.step(); ext_r.zero_grad()
            _close(im_out, im_r, f"im_out, iteration {it}", rtol=2e-3 if it else 2e-5)    # Adam's first step amplifies round-off
            for name, got, ref in (("vgg_loss", loss_dict['vgg_loss'], vgg_r), ("huber_loss", loss_dict['huber_loss'], hub_r)):
                assert abs(float(got) - float(ref)) <= (1e-3 if it else 1e-5) * abs(float(ref)), (it, name, float(got), float(ref))
        pipeline.model.check_ids()
        sd = pipeline.get_net().state_dict()
        for name in ("feat_extract.0.block.conv_f.weight", "Decoder.3.layers.3.main.1.block.conv_m.weight",
                     "feat_extract.5.block.norm.bias", "SCM1.conv.block.conv_f.bias"):
            _close(sd[name].cpu(), st_r[name].detach(), name, rtol=2e-3)
        pipeline.dataset_unload(ds_list)
        assert not pipeline.textures[0].texture_.is_cuda
        # eval through the same model object, as EvalIterCb / OGL.infer(input_dict) read it (src/READ/gl/nn.py:130)
        pipeline.dataset_load(ds_list)
        model.cuda()
        with torch.no_grad():
            probe = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in renderer.render(data)[0].items()}
            res = pipeline.model(probe)
        assert isinstance(res, dict) and res['im_out'].shape == (B, 3, H, W)
    finally:
        _alias.set_result_convention(None)


def test_two_forwards_before_a_backward_keep_their_own_activations(hip):
    """Two forwards of one net before any backward (.eval(), 32 x 48, B = 2): the second one must not disturb what the first one's
    nodes saved — its input gradients equal those of a lone forward over the same inputs — and the second still backpropagates."""
    H, W, B = 32, 48, 2
    state = synthetic.make_unet_state(UNET_SPEC, 23)
    rng = np.random.default_rng(31)
    xs = [torch.from_numpy(rng.random((B, 8, H >> l, W >> l)).astype(np.float32)).cuda() for l in range(4)]
    g = torch.from_numpy(rng.standard_normal((B, 3, H, W)).astype(np.float32)).cuda()
    net = UNet()
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    net = net.cuda().eval()
    ins_a = [x.clone().requires_grad_(True) for x in xs]
    ins_b = [(x * 0.5).clone().requires_grad_(True) for x in xs]
    out_a = net(*ins_a)
    out_b = net(*ins_b)
    net.zero_grad()
    (out_a * g).sum().backward()
    ga = [i.grad.clone() for i in ins_a]
    ins_c = [x.clone().requires_grad_(True) for x in xs]
    (net(*ins_c) * g).sum().backward()
    for l in range(4):
        _close(ga[l], ins_c[l].grad, f"first forward's gradients after an interleaved second forward, level {l}", rtol=1e-4)
    (out_b * g).sum().backward()
    assert all(i.grad is not None for i in ins_b)


def test_pack_plan_equals_the_per_layer_packers_and_follows_the_optimizer(hip):
    """One read_conv_pack_batch launch (read_amd/train.py _PackPlan) against the per-layer device packers it replaces: parameter
    block, forward fragments and dgrad fragments of every executed layer bit for bit, in eval-mode and identity (batch-statistics)
    form; and after a FUSED Adam step (which does not advance torch's version counters by itself) the next refresh
    packs the stepped weights."""
    from read_amd import train as T
    from read_amd.pipeline import _DeviceAdam
    state = synthetic.make_unet_state(UNET_SPEC, 41)
    net = UNet()
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    net.cuda()
    for identity in (False, True):
        plan = T._PackPlan(net, identity)
        plan.refresh()
        torch.cuda.synchronize()
        assert len(plan.layers) == 99 and plan.njobs == 99 * 2 + sum(1 for _ts, e in plan.layers if e.dgrad is not None)
        for ts, planned in plan.layers:
            wf, wm, route = ts[0], ts[2], planned.route
            T._PACK_CACHE.pop(id(wf), None)                                   # force the per-layer path
            ref = T._packed_for(route, ts, identity_bn=identity)
            assert ref is not planned and ref.route == route
            assert torch.equal(ref.params, planned.params), ("parameter block", route)
            assert (ref.wino is None) == (planned.wino is None) and torch.equal(ref.fwd, planned.fwd), ("forward fragments", route)
            assert (planned.dgrad is None) == (route.dgrad is None)
            if planned.dgrad is not None:
                T._pack_dgrad(ref, wf, wm)
                assert torch.equal(ref.dgrad, planned.dgrad), ("dgrad fragments", route)
            T._PACK_CACHE.pop(id(wf), None)
    # a fused Adam step: versions bumped by _DeviceAdam, so the plan's signature changes and the refresh repacks
    net.eval()
    plan = T._pack_plan(net, False)
    plan.refresh()
    _ts, first = plan.layers[0]
    before = first.fwd.clone()
    opt = _DeviceAdam(net.parameters(), lr=1e-2)
    xs = [torch.rand(1, 8, 32 >> l, 48 >> l, device="cuda") for l in range(4)]
    net(*xs).sum().backward()
    sig = plan.signature
    opt.step()
    assert opt.param_groups[0]['fused'] is True and opt._step_supports_amp_scaling
    plan.refresh()
    assert plan.signature != sig and not torch.equal(first.fwd, before)


def test_model_and_loss_under_dataparallel_on_one_gpu(hip):
    """src/train.py:147-148 wraps the merged model in nn.DataParallel by default (--multigpu True).  On one visible GPU DataParallel
    hands the call to the module itself: the result and the losses must be those of the direct call (more than one GPU — replicas
    of the HIP-backed modules — is not rebuilt)."""
    from read_amd import _alias
    from read_amd.net_texture import ModelAndLoss, NetAndTexture
    from read_amd.texture import PointTexture
    H, W, N, B = 32, 48, 2000, 2
    rng = np.random.default_rng(3)
    state = synthetic.make_unet_state(UNET_SPEC, 8)
    net = UNet()
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    tex = PointTexture(8, N, init_method='rand')
    model = NetAndTexture(net, {0: tex})
    model.load_textures(0)
    merged = ModelAndLoss(model, torch.nn.L1Loss()).cuda().eval()
    keys = "uv_1d_p1,uv_1d_p1_ds1,uv_1d_p1_ds2,uv_1d_p1_ds3,uv_1d_p1_ds4".split(',')
    maps = [torch.from_numpy(rng.integers(0, N, (B, 1, H >> l, W >> l)).astype(np.float32)).cuda() for l in range(5)]
    target = torch.rand(B, 3, H, W, device="cuda")

    def inputs():
        d = {'id': torch.zeros(B, dtype=torch.long)}
        d.update(dict(zip(keys, maps)))
        return d
    _alias.set_result_convention('dict')
    try:
        with torch.no_grad():
            out, losses = merged(inputs(), target, label=None, mask=None)
            out_dp, losses_dp = torch.nn.DataParallel(merged, device_ids=[0])(inputs(), target, label=None, mask=None)
        assert torch.equal(out['im_out'], out_dp['im_out'])
        assert set(losses) == set(losses_dp) == {'vgg_loss', 'huber_loss'}
        for k in losses:                                   # the reductions sum with atomics: equal to round-off, not bit for bit
            assert abs(float(losses[k]) - float(losses_dp[k])) <= 1e-6 * abs(float(losses[k])), k
    finally:
        _alias.set_result_convention(None)


def test_data_parallel_step_on_a_single_rank_rccl_group(hip):
    """SURVEY 8e "Training" / VERDICT r4 #7: the data-parallel exchange (read_amd/ddp.py) on the device — a 1-rank RCCL group with
    the collectives forced on: the flat gradient arena is all-reduced by RCCL, fused Adam consumes the arena views, the gathered
    (id, row) pairs feed read_rmsprop_sorted.  With one rank the mean is the identity, so two optimisation steps through
    DataParallelStep.reduce() must leave the weights and descriptors of the same two steps without it (up to the run-to-run
    round-off of the step itself).  (World size 2
    on gloo: tests/test_ddp_gloo.py.)"""
    import socket
    from types import SimpleNamespace
    import torch.distributed as dist
    from read_amd import ddp
    from read_amd.pipeline import TexturePipeline
    H, W, N = 32, 48, 3000

    class DS:
        id, name = 0, "scene0"
        scene_data = {'pointcloud': {'xyz': np.zeros((N, 3), np.float32)}}
        def load(self): pass
        def unload(self): pass

    class Crit(torch.nn.Module):
        def forward(self, out, target):
            return huber_loss(out, target)

    keys = "uv_1d_p1, uv_1d_p1_ds1, uv_1d_p1_ds2, uv_1d_p1_ds3, uv_1d_p1_ds4".replace(' ', '').split(',')

    def run(with_ddp):
        rng = np.random.default_rng(16)
        args = SimpleNamespace(inference=False, descriptor_size=8, texture_activation='none', use_mesh=False, supersampling=1,
                               lr=1e-3, texture_lr=1e-1, texture_ckpt=None, get_datasets=lambda a: ([DS()], [DS()]),
                               criterion_module=Crit, criterion_args={}, pipeline='READ.pipelines.ogl.TexturePipeline')
        pipe = TexturePipeline()
        pipe.create(args)
        state = synthetic.make_unet_state(UNET_SPEC, 2)
        pipe.net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
        tex = pipe.textures[0]
        with torch.no_grad():
            tex.texture_.copy_(torch.from_numpy(rng.random((1, 8, N)).astype(np.float32)))
        model = pipe.model.cuda()
        pipe.dataset_load([DS()])
        model.cuda().eval()
        extra = pipe.extra_optimizer([DS()])
        step = ddp.DataParallelStep(pipe.net, pipe.textures) if with_ddp else None
        for it in range(2):
            maps = [rng.integers(0, N, (2, 1, H >> l, W >> l)) for l in range(5)]
            target = torch.from_numpy(rng.random((2, 3, H, W)).astype(np.float32))
            inputs = {'id': torch.tensor([0, 0])}
            inputs.update({k: torch.from_numpy(m).float().cuda() for k, m in zip(keys, maps)})
            loss = pipe.criterion(model(inputs), target.cuda()) * 1e4
            loss.backward()
            if step is not None:
                step.reduce()
                assert all(p.grad is None or p.grad.data_ptr() == v.data_ptr() for p, v in zip(step.arena.params, step.arena.views))   # None: no gradient on any rank (ConvsOut)
            pipe.optimizer.step()
            pipe.optimizer.zero_grad()
            extra.step()
            extra.zero_grad()
        torch.cuda.synchronize()
        return ({k: v.detach().cpu().clone() for k, v in pipe.net.state_dict().items()},
                tex.state_dict()["texture_"].cpu().clone(), None if step is None else step.arena.nbytes)

    want_net, want_tex, _ = run(False)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    ddp.FORCE_COLLECTIVES = True
    try:
        got_net, got_tex, nbytes = run(True)
    finally:
        ddp.FORCE_COLLECTIVES = False
        dist.destroy_process_group()
    assert nbytes >= 4 * sum(v.numel() for k, v in want_net.items() if v.dtype == torch.float32 and "running" not in k and "num_batches" not in k)
    # Two runs of the SAME step are not bit-equal (the gate backward accumulates its per-channel sums with fp32 atomics), and the
    # first Adam / RMSprop steps move an entry by ~lr * sign(g): an entry whose gradient is at round-off level may go either way.
    # So: nearly every entry must agree to a fraction of a step, and none may differ by more than the two steps can move it.
    lr_net, lr_tex = 1e-3, 1e-1
    for k, v in want_net.items():
        if v.dtype != torch.float32 or "num_batches" in k:
            continue
        d = (got_net[k].double() - v.double()).abs()
        assert float(d.max()) <= 2 * 2 * lr_net + 1e-6, f"{k}: differs by {float(d.max()):.3e} from the plain step"
        assert float((d <= 0.02 * lr_net).double().mean()) >= 0.97, f"{k}: {float((d > 0.02 * lr_net).double().mean()):.3f} of the entries off"
    d = (got_tex.double() - want_tex.double()).abs()
    assert float(d.max()) <= 2 * 10 * lr_tex + 1e-6
    assert float((d <= 1e-3).double().mean()) >= 0.97, f"descriptors: {float((d > 1e-3).double().mean()):.3f} of the entries off"
