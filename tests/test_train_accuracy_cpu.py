"""CPU: tests/train_ref64.py checked before anything runs on the device.
  * the float64 references agree with torch double autograd to 1e-12 relative;
  * NumPy fp32 restatements of the gate / BatchNorm chain (modes 0 / 1 / 2, bn_bwd_coeff, bn_stats in fp64, bn_finalize, bn_apply) and of
    both weight-gradient kernels (pixel pairs, per-split partials, the reduce; the two transform passes and the G^T . G step), in the
    kernels' own order of operations and without fused multiply-adds, stay inside the derived bounds on every input class;
  * the restatements reproduce the class (d) behaviour DESIGN.md quotes (the dgamma error in units of the centred condition term grows
    with |mean| / std; a constant channel misses beta by about u |mean| scale);
  * the generators do what they claim;
  * the forward's linear launches (tests/train_forward_cases.py): the fp32 restatement of the three convolution kernels and the fused gate
    passes every assertion of tests/test_gpu_train_forward_accuracy.py, each seeded defect of the mutation catalogue fails one, and
    conv_forward_bound restates conv_dgrad_bound."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_ref64 as R64
from tests import train_ref64 as T
from tests import train_forward_cases as FC
from tests.train_fp32 import (GUARD, MUTATIONS, bn_bwd_coeff32, bn_forward32, bn_grads32, gate32, gate_backward32,  # noqa: F401
                              linear_launch32, wgrad_direct32, wgrad_wino32)

f32 = np.float32


# ------------------------------------------------------------------------------------------ cases
GEOM = [(91, 13, 0, 0, 1), (105, 7, 5, 3, 1), (105, 7, 5, 3, 3)]                                 # (P, W, block_h, valid_h, groups)


def _cases(C):
    for cls, mk in (("a", T.unit_case), ("b", T.checkpoint_case), ("d", lambda P, C_, s: T.range_edge_case(P, C_, s)[:3])):
        for (P, W, bh, vh, groups) in GEOM:
            yield cls, P, W, bh, vh, groups, mk(P, C, 5)


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# ------------------------------------------------------------------------------------------ references against torch double
def test_gate_references_agree_with_torch_double_autograd():
    C = 9
    for cls, P, W, bh, vh, groups, (fm, dy, L) in _cases(C):
        if cls == "d":
            continue                                       # exp(-m) of |m| > 100: torch's sigmoid and 1 / (1 + exp) part ways at 1e-44
        v = T.valid_rows(P, W, bh, vh)[:, None]
        t = torch.from_numpy(fm.astype(np.float64)).requires_grad_(True)
        par = {k: torch.from_numpy(L[k].astype(np.float64)).requires_grad_(k in ("gamma", "beta")) for k in ("gamma", "beta", "mean", "var")}
        g = F.elu(t[:, :C]) * torch.sigmoid(t[:, C:])
        y = F.batch_norm(g.t()[None], par["mean"], par["var"], par["gamma"], par["beta"], training=False, eps=T.EPS)[0].t()
        y_ref, _, _, _ = T.gate_forward_ref(fm, C, L, True, None, W, bh, vh)
        assert _rel(y_ref, (y.detach().numpy() * v)) <= 1e-12
        (y * torch.from_numpy(dy.astype(np.float64) * v)).sum().backward()
        ref = T.GateBackwardEval(dy, fm, C, L, True, W, bh, vh)
        assert _rel(ref.df, t.grad[:, :C].numpy()) <= 1e-12 and _rel(ref.dm, t.grad[:, C:].numpy()) <= 1e-12
        assert _rel(ref.dgamma, par["gamma"].grad.numpy()) <= 1e-11 and _rel(ref.sums[2], par["beta"].grad.numpy()) <= 1e-12
        # batch statistics: the reference with the exact statistics is BatchNorm's backward
        df, dm, dgam, dbeta, stat = T.bn_backward_torch64(dy, fm, C, L["gamma"], True, W, bh, vh, groups)
        refb = T.GateBackwardBn(dy, fm, C, L["gamma"], True, W, bh, vh, groups, stat)          # stat in float64: the exact statistics
        assert _rel(refb.df, df) <= 1e-10 and _rel(refb.dm, dm) <= 1e-10, (cls, groups)
        assert _rel(refb.dgamma, dgam) <= 1e-10 and _rel(refb.dbeta, dbeta) <= 1e-12


def test_bn_forward_reference_agrees_with_torch_double():
    C = 9
    for cls, P, W, bh, vh, groups, (fm, dy, L) in _cases(C):
        g = fm[:, :C]
        rm0, rv0 = L["mean"].copy(), L["var"].copy()
        ref = T.BnForward(g, L, W, bh, vh, groups, 0.1, rm0, rv0)
        v, grp = T.valid_rows(P, W, bh, vh), T.group_of(P, W, bh, groups)
        rm, rv = torch.from_numpy(rm0.astype(np.float64)), torch.from_numpy(rv0.astype(np.float64))
        for j in range(groups):
            sel = v & (grp == j)
            y = F.batch_norm(torch.from_numpy(g[sel].astype(np.float64)).t()[None], rm, rv, torch.from_numpy(L["gamma"].astype(np.float64)),
                             torch.from_numpy(L["beta"].astype(np.float64)), training=True, momentum=0.1, eps=T.EPS)[0].t().numpy()
            assert np.abs(ref.y[sel] - y).max() <= 1e-12 * max(1.0, np.abs(y).max())
        assert _rel(ref.running_mean, rm.numpy()) <= 1e-12 and _rel(ref.running_var, rv.numpy()) <= 1e-12
        assert not ref.y[~v].any()


def test_huber_and_up4_references_agree_with_torch_double():
    rng = np.random.default_rng(2)
    o, t = rng.standard_normal(257).astype(f32) * 2, rng.standard_normal(257).astype(f32)
    ot = torch.from_numpy(o.astype(np.float64)).requires_grad_(True)
    loss = F.huber_loss(ot, torch.from_numpy(t.astype(np.float64)), reduction="sum")
    loss.backward()
    ref = T.huber_ref(o, t, 1.0)
    assert abs(ref["loss_sum"] - float(loss.detach())) <= 1e-12 * float(loss.detach()) and _rel(ref["grad"], ot.grad.numpy()) <= 1e-12
    # up4 backward is the adjoint of the forward: <up(x), d> = <x, up^T(d)>
    x, d = rng.standard_normal((10, 3, 4)).astype(f32), rng.standard_normal((40, 12, 4)).astype(f32)
    for bh, vh in ((0, 0), (5, 3)):
        out, _, _ = T.up4_forward_ref(x, bh, vh)
        din, _, _ = T.up4_backward_ref(d, 10, 3, bh, vh)
        assert abs((out * d).sum() - (x * din).sum()) <= 1e-12 * np.abs(out * d).sum()
        if bh:
            assert not out.reshape(2, 20, -1)[:, 12:].any() and not din.reshape(2, 5, -1)[:, 3:].any()


# ------------------------------------------------------------------------------------------ restatements inside the bounds
@pytest.mark.parametrize("C", [3, 9, 32])
def test_fp32_restatement_of_the_gate_chain_stays_inside_the_derived_bounds(C):
    _gate_chain_inside_bounds(C, _cases(C))


# 1 (batch statistics over one value: var = 0, y = beta), 4 and 12 pixels and three stacked 2 x 2 items with one separator row each (statistics over the batch, and per item over 4 values):
# the coarse levels of a 16-pixel crop, the geometries of tests/test_gpu_train_accuracy.py's degenerate rows
TINY_GEOM = ((1, 1, 0, 0, 1), (4, 2, 0, 0, 1), (12, 6, 0, 0, 1), (18, 2, 3, 2, 1), (18, 2, 3, 2, 3))


@pytest.mark.parametrize("C", [3, 9, 256])
def test_fp32_restatement_of_the_gate_chain_at_degenerate_sizes(C):
    """The references and bounds of the gate / BatchNorm chain are right at a handful of pixels before any kernel is blamed there."""
    _gate_chain_inside_bounds(C, ((cls, P, W, bh, vh, groups, mk(P, C, 6)) for cls, mk in (("a", T.unit_case), ("b", T.checkpoint_case))
                                  for (P, W, bh, vh, groups) in TINY_GEOM))


def _gate_chain_inside_bounds(C, cases):
    for cls, P, W, bh, vh, groups, (fm, dy, L) in cases:
        what = f"class {cls} C {C} P {P} block {bh}/{vh} groups {groups}"
        v = T.valid_rows(P, W, bh, vh)
        sc = (L["gamma"] / np.sqrt((L["var"] + f32(T.EPS)).astype(f32)).astype(f32)).astype(f32)
        sh = (L["beta"] - (L["mean"] * sc).astype(f32)).astype(f32)
        a, da, s = gate32(fm, C, True)
        y = (((a * s).astype(f32) * sc[None]).astype(f32) + sh[None]).astype(f32) * v[:, None]
        y_ref, B, bound, _ = T.gate_forward_ref(fm, C, L, True, None, W, bh, vh)
        assert T.worst(np.abs(y - y_ref), bound) <= 1.0, what + " gate forward"
        if groups == 1:
            df, dm, sums = gate_backward32(dy, fm, C, sc, True, v, 0)
            ref = T.GateBackwardEval(dy, fm, C, L, True, W, bh, vh)
            assert T.worst(np.abs(df - ref.df), ref.bound_df) <= 1.0 and T.worst(np.abs(dm - ref.dm), ref.bound_dm) <= 1.0, what + " mode 0"
            assert T.worst(np.abs(sums - ref.sums), ref.bound_sums) <= 1.0, what + " sums"
            assert T.worst(np.abs(bn_grads32(sums, L["mean"], L["var"]) - ref.dgamma), ref.bound_dgamma) <= 1.0, what + " dgamma"
        # batch statistics: forward, then backward with the forward's fp32 statistics
        grp = T.group_of(P, W, bh, groups)
        g = (a * s).astype(f32)
        fwd = T.BnForward(g, L, W, bh, vh, groups, 0.1, L["mean"], L["var"])
        rm, rv = L["mean"].copy(), L["var"].copy()
        stat = np.zeros((groups, 2, C), f32)
        yb = np.zeros((P, C), f32)
        for j in range(groups):
            sel = v & (grp == j)
            yb[sel], stat[j, 0], stat[j, 1], rm, rv = bn_forward32(g[sel], L["gamma"], L["beta"], 0.1, rm, rv)
        assert T.worst(np.abs(yb - fwd.y), fwd.bound_y) <= 1.0, what + " bn forward y"
        assert T.worst(np.abs(stat - fwd.stat), fwd.bound_stat) <= 1.0, what + " stat"
        assert T.worst(np.abs(rm - fwd.running_mean), fwd.bound_rm) <= 1.0 and T.worst(np.abs(rv - fwd.running_var), fwd.bound_rv) <= 1.0, what
        refb = T.GateBackwardBn(dy, fm, C, L["gamma"], True, W, bh, vh, groups, stat)
        df, dm = np.zeros((P, C), f32), np.zeros((P, C), f32)
        dgam = np.zeros(C, f32)
        for j in range(groups):
            idx = np.nonzero(grp == j)[0]
            vj = v[idx]
            _, _, sums = gate_backward32(dy[idx], fm[idx], C, sc, True, vj, 1)
            abc = bn_bwd_coeff32(sums, stat[j, 0], stat[j, 1], L["gamma"], int(vj.sum()))
            df[idx], dm[idx], sums2 = gate_backward32(dy[idx], fm[idx], C, sc, True, vj, 2, abc)
            dgam = dgam + bn_grads32(sums2, stat[j, 0], stat[j, 1])
        assert T.worst(np.abs(df - refb.df), refb.bound_df) <= 1.0 and T.worst(np.abs(dm - refb.dm), refb.bound_dm) <= 1.0, what + " mode 2"
        assert T.worst(np.abs(dgam - refb.dgamma), refb.bound_dgamma) <= 1.0, what + " dgamma (groups)"


def test_fp32_restatements_of_both_wgrad_kernels_stay_inside_the_derived_bounds():
    _wgrad_inside_bounds(np.random.default_rng(9), ((8, 3, 3, 1, 7, 9), (8, 5, 4, 2, 13, 5), (16, 4, 1, 1, 7, 9), (8, 3, 3, 2, 7, 9)), ((32, 3, 8, 12), (32, 4, 44, 8)))


def test_fp32_restatements_of_both_wgrad_kernels_at_degenerate_sizes():
    """The direct kernel at 1 x 1 and 2 x 2 (stride 1, k3 / stride 2, k4 / stride 2: one output pixel), the Winograd-domain one at a
    single tile row (4 x 4, 4 x 12): the smallest image read_conv_wgrad_family gives it."""
    direct = [(8, 3, 3, 1, h, h) for h in (1, 2)] + [(8, 3, 3, 2, h, h) for h in (1, 2)] + [(8, 5, 4, 2, 2, 2)]
    _wgrad_inside_bounds(np.random.default_rng(19), direct, ((32, 3, 4, 4), (32, 4, 4, 12)), impulse=(1, 2))


def _wgrad_inside_bounds(rng, direct, wino, impulse=(3, 4)):
    for (cin, cout, k, stride, H, W) in direct:
        for cls in "abc":
            oh, ow = T.out_hw(k, stride, H, W)
            sx, sd = (T.scales_b(cin, rng), T.scales_b(cout, rng)) if cls == "b" else (np.ones(cin), np.ones(cout))
            x = (rng.standard_normal((H, W, cin)) * sx).astype(f32)
            d = (rng.standard_normal((oh, ow, cout)) * sd).astype(f32)
            if cls == "c":                                           # checkerboard under random d; then an impulse over integers: exact
                x = R64.checkerboard(cin, H, W).transpose(1, 2, 0).copy()
            ref, A = T.wgrad_ref(x, d, k, stride)
            got = wgrad_direct32(x, d, k, stride, T.wgrad_plan(cin, cout, k, oh))
            assert T.worst(np.abs(got - ref), T.wgrad_direct_bound(A, cin, cout, k, oh, ow)) <= 1.0, (cin, cout, k, stride, cls)
            if cls == "c":
                x = T.small_integers((H, W, cin), rng)
                for (py, px) in T.impulse_pixels(oh, ow)[:6]:
                    d = np.zeros((oh, ow, cout), f32)
                    d[py, px] = 2.0 ** -10
                    assert np.array_equal(wgrad_direct32(x, d, k, stride, T.wgrad_plan(cin, cout, k, oh)).astype(np.float64), T.wgrad_ref(x, d, k, stride)[0])
    for (cin, cout, H, W) in wino:
        for cls in "abc":
            sx, sd = (T.scales_b(cin, rng), T.scales_b(cout, rng)) if cls == "b" else (np.ones(cin), np.ones(cout))
            x = (rng.standard_normal((H, W, cin)) * sx).astype(f32)
            d = (rng.standard_normal((H, W, cout)) * sd).astype(f32)
            if cls == "c":                                           # an impulse of d on a tile boundary over small integers
                x, d = T.small_integers((H, W, cin), rng), np.zeros((H, W, cout), f32)
                d[impulse] = 1.0
            ref, A = T.wgrad_ref(x, d, 3, 1)
            Aw = T.wgrad_wino_Aw(x, d)
            assert (Aw >= A * (1 - 1e-12)).all()                       # the transformed-domain condition term dominates the direct one
            got = wgrad_wino32(x, d, T.wgrad4_plan(cin, cout, H))
            assert T.worst(np.abs(got - ref), T.wgrad_wino_bound(Aw, cin, cout, H, W)) <= 1.0, (cin, cout, H, W, cls)


# ------------------------------------------------------------------------------------------ the forward's linear launches
VARIANTS = ((True, False), (False, True), (True, True), (False, False))                          # (elu, identity_bn), as the GPU test launches them


def _run_assertions(case, family, elu_identity, block_h=0, valid_h=0, mut=None, unstacked=None):
    """The restatement's buffers of one launch per variant through the assertions the GPU test applies to the device's.
    -> (failures, err / bound of every judged row, (fm, y) of the last variant)."""
    fails = []
    judge = FC.bound_judge(fails)
    out = None
    for elu, identity in elu_identity:
        sc, sh = FC.scale_shift32(case.L, identity)
        fm_buf, y_buf = linear_launch32(case.L, case.x, case.stride, family, elu, sc, sh, block_h, valid_h, mut=mut)
        fm = FC.check_preactivations(case, family, fm_buf, judge, fails.append)
        if family == "direct":
            return fails, judge.ratios, (fm, None)
        y = FC.check_gated(case, family, fm, y_buf, elu, identity, block_h, valid_h, judge, fails.append,
                           unstacked=None if unstacked is None else unstacked[(elu, identity)])
        out = (fm, y)
    return fails, judge.ratios, out


@pytest.mark.parametrize("family", ["direct", "w2", "w4"])
def test_fp32_restatement_of_the_forward_launches_stays_inside_the_derived_bound(family):
    """tests/train_fp32.py linear_launch32 — the direct kernel as a sequential fp32 sum over (tap, channel), F(2x2) and F(4x4) through
    their fp32 transforms, the fused gate with fast_exp32 — on classes (a), (b), (d) at the GPU test's layers and sizes: every assertion
    of the GPU test holds, and the closest approach to the derived bounds is printed."""
    _forward_restatement_inside_bounds(family, lambda layer: FC.SIZES[layer[3]], "abd")


@pytest.mark.parametrize("family", ["direct", "w2", "w4"])
def test_fp32_restatement_of_the_forward_launches_at_degenerate_sizes(family):
    """... at 2 x 2, 4 x 4 and 1 x 1 (FC.SIZES_TINY), class (c) with its impulse at every pixel included: the references, the bounds and
    the exactness assertions are right at those sizes before any kernel is blamed."""
    _forward_restatement_inside_bounds(family, lambda layer: [hw for hw in FC.SIZES_TINY if 0 not in T.out_hw(layer[2], layer[3], *hw)], "abcd")


def _forward_restatement_inside_bounds(family, sizes_of, classes):
    worst = {}
    for layer in FC.LAYERS[family]:
        for hw in sizes_of(layer):
            for case in FC.cases(layer, hw, classes=classes):
                fails, ratios, _ = _run_assertions(case, family, VARIANTS[:2])
                assert not fails, fails
                for fam, cls, _name, q in ratios:
                    worst[(fam, cls)] = max(worst.get((fam, cls), 0.0), q)
    print(f"forward restatement [{family}], worst err / bound:", {f"{k[0]} ({k[1]})": round(v, 3) for k, v in sorted(worst.items())})
    assert max(worst.values()) <= 1.0


def test_every_seeded_defect_of_the_forward_launch_breaks_an_assertion():
    """The mutation catalogue: each defect built into the restatement must fail at least one assertion of the GPU test on at least one
    of its cases (and the unmutated restatement none).  A defect that passes means the cases are too weak."""
    flat = {"w2": [((32, 3, 3, 1), (9, 21), "a"), ((48, 20, 3, 1), (9, 21), "b")],
            "w4": [((48, 40, 3, 1), (9, 21), "a"), ((48, 40, 3, 1), (12, 20), "b"), ((64, 24, 3, 1), (9, 21), "d")],
            "direct": [((8, 16, 3, 1), (9, 21), "a"), ((64, 56, 1, 1), (9, 21), "b")]}
    stacked = {"w2": [((16, 32, 3, 1), FC.GEOMETRIES[1])], "w4": [((32, 8, 3, 1), FC.GEOMETRIES[0])]}
    runs = []                                                        # (family, case, block_h, valid_h, unstacked)
    for family, rows in flat.items():
        for layer, hw, cls in rows:
            runs.append((family, next(FC.cases(layer + (None,), hw, classes=cls)), 0, 0, None))
    for family, rows in stacked.items():
        for layer, (H, W, bh, vh) in rows:
            case = next(FC.cases(layer + (None,), (H, W), classes="a"))
            plain = {}
            for variant in VARIANTS:
                fails, _, plain[variant] = _run_assertions(case, family, (variant,))
                assert not fails, fails
            runs.append((family, case, bh, vh, plain))
    for family, case, bh, vh, plain in runs:
        fails, _, _ = _run_assertions(case, family, VARIANTS, bh, vh, unstacked=plain)
        assert not fails, ("the unmutated restatement", case.name, fails)
    for mut in MUTATIONS:
        caught = [case.name for family, case, bh, vh, plain in runs if _run_assertions(case, family, VARIANTS, bh, vh, mut=mut, unstacked=plain)[0]]
        print(f"mutation {mut}: caught on {len(caught)} of {len(runs)} cases")
        assert caught, f"no assertion of the forward tests sees the defect '{mut}'"
    # block geometry taken at the input scale of a stride-2 layer: GatedConvFn's y against the launch with T.block_geometry(out rows)
    layer, (H, W), nb, v = (32, 64, 3, 2), (24, 12), 3, (3, 4)
    case = next(FC.cases(layer + (None,), (H, W), classes="a"))
    sc, sh = FC.scale_shift32(case.L, False)
    fm = linear_launch32(case.L, case.x, 2, "direct", True, sc, sh, 0, 0)[0][:-GUARD].reshape(case.oh * case.ow, -1)
    a, _, s = gate32(fm, case.cout, True)
    y = (((a * s).astype(f32) * sc[None]).astype(f32) + sh[None]).astype(f32)
    want = y * T.valid_rows(len(y), case.ow, *T.block_geometry(case.oh, nb, *v))[:, None]
    wrong = y * T.valid_rows(len(y), case.ow, *T.block_geometry(H, nb, *v))[:, None]
    assert T.block_geometry(case.oh, nb, *v) == (4, 3) and not np.array_equal(want.view(np.uint32), wrong.view(np.uint32))


def test_forward_bound_restates_the_dgrad_bound_and_the_bias_cases_are_exact():
    """A 32 -> 16 layer with zero bias is the dgrad's virtual layer of a 32-channel layer: conv_forward_bound gives conv_dgrad_bound's
    numbers.  Class (d): the float64 reference's pre-activations ARE the biases."""
    rng = np.random.default_rng(12)
    H, W = 9, 21
    L = R64.tame_layer(32, 16, 3, 5)
    L["bf"], L["bm"] = np.zeros(16, f32), np.zeros(16, f32)
    x = rng.standard_normal((32, H, W)).astype(f32)
    ref = R64.reference(L, x)
    for which, val, A in (("f", ref.f, ref.Af), ("m", ref.m, ref.Am)):
        wv = L["w" + which].astype(np.float64)
        d_hwc, value = np.ascontiguousarray(x.transpose(1, 2, 0)), val.transpose(1, 2, 0)
        b, cond = T.conv_forward_bound(L, x, ref, "direct", which)
        assert np.array_equal(b.transpose(1, 2, 0), T.conv_dgrad_bound(d_hwc, wv, A.transpose(1, 2, 0), value, "direct")) and np.array_equal(cond, A)
        for fam in ("w2", "w4"):
            b, cond = T.conv_forward_bound(L, x, ref, fam, which)
            b0, Aw = T.conv_dgrad_bound(d_hwc, wv, None, value, fam)
            assert np.array_equal(b.transpose(1, 2, 0), b0) and np.array_equal(cond.transpose(1, 2, 0), Aw)
    for layer in ((32, 3, 3, 1, None), (48, 40, 3, 1, None), (64, 32, 4, 2, None)):
        case = next(FC.cases(layer, FC.SIZES[layer[3]][0], classes="d"))
        r = case.ref()
        assert np.array_equal(r.f, np.broadcast_to(case.L["bf"].astype(np.float64)[:, None, None], r.f.shape))
        assert np.array_equal(r.m, np.broadcast_to(case.L["bm"].astype(np.float64)[:, None, None], r.m.shape))
        assert {float(b) for b in case.L["bf"]} <= {float(f32(e)) for e in FC.F_EDGES} and (np.abs(case.L["bm"]) >= 88).any()
        for fam in ("direct",) if layer[3] == 2 else ("w2", "w4"):
            df, dm, cf, cm = case.bounds(fam)
            assert np.array_equal(cf, np.abs(r.f)) and np.array_equal(cm, np.abs(r.m))         # no product in the condition terms either


# ------------------------------------------------------------------------------------------ class (d)
def test_class_d_numbers_of_the_restatement():
    """What DESIGN.md quotes: against the centred condition term (what torch's formulation is held to) the kernels' dgamma error grows
    with |mean| / std, and a constant channel of value 100 misses beta = 0.2 by about u |mean| scale."""
    C, P, W = 7, 1536, 32
    fm, dy, L, kinds = T.range_edge_case(P, C, 11)
    v = np.ones(P, bool)
    sc = np.ones(C, f32)
    a, da, s = gate32(fm, C, True)
    g = (a * s).astype(f32)
    fwd = T.BnForward(g, L, W, 0, 0, 1, 0.1, L["mean"], L["var"])
    y, mf, vf, _, _ = bn_forward32(g, L["gamma"], L["beta"], 0.1, L["mean"], L["var"])
    stat = np.stack([mf, vf])[None]
    refb = T.GateBackwardBn(dy, fm, C, L["gamma"], True, W, 0, 0, 1, stat)
    _, _, sums = gate_backward32(dy, fm, C, sc, True, v, 1)
    dgam = bn_grads32(sums, mf, vf)
    E = {kinds[c]: abs(dgam[c] - refb.dgamma[c]) / max(T.U * refb.cond_dgamma["centered"][c], 1e-300) for c in range(C)}
    print("class (d), restatement: E(dgamma, centred) =", {k: round(float(e), 1) for k, e in E.items() if k.startswith("ratio")})
    # the quoted behaviour: about one unit at |mean| / std = 1, growing with the ratio, and never above the leading term of the bound
    lead = {kinds[c]: refb.lead_dgamma[c] / (T.U * refb.cond_dgamma["centered"][c]) for c in range(C) if kinds[c].startswith("ratio")}
    assert E["ratio1"] <= 2.0 and E["ratio256"] > 4 * max(E["ratio1"], 1.0)
    assert all(E[k] <= lead[k] for k in lead), (E, lead)
    assert E["ratio32"] <= 2.0 * 32 and E["ratio256"] <= 2.0 * 256        # sequential-order worst case of u |mean| sum |dy| over cond: ~ ratio
    c = kinds.index("constant")
    miss = np.abs(y[:, c].astype(np.float64) - 0.2).max()
    scale = abs(L["gamma"][c]) / np.sqrt(T.EPS)
    print("class (d), restatement: constant channel y - beta =", miss, "u |mean| scale =", T.U * 100 * scale)
    assert miss <= 8 * T.U * 100 * scale and T.worst(np.abs(y - fwd.y), fwd.bound_y) <= 1.0
    assert abs(dgam[c]) <= refb.bound_dgamma[c]                        # dgamma of the constant channel is 0 within the bound


# ------------------------------------------------------------------------------------------ generators
def test_generators_do_what_they_claim():
    C, P = 14, 1536
    fm, dy, L, kinds = T.range_edge_case(P, C, 3)
    gt = T.Gate(fm, C, True)
    for c, kind in enumerate(kinds):
        g = gt.g[:, c]
        if kind.startswith("ratio"):
            want = float(kind[5:])
            assert abs(abs(g.mean()) / g.std() / want - 1) < 0.15, (kind, abs(g.mean()) / g.std())
        elif kind == "constant":
            assert g.std() == 0 and fm[:, c].std() == 0
        elif kind == "elu_saturated":
            assert fm[:, c].max() < -20 and np.abs(gt.a[:, c] + 1).max() < 3e-9
        elif kind == "gate_overflow":
            assert np.abs(fm[:, C + c]).min() > 100
        elif kind == "tiny_f":
            assert np.abs(fm[:, c]).max() < 1e-5
    rng = np.random.default_rng(1)
    for n in (2, 3, 40):
        s = T.scales_b(n, rng)
        assert s.max() / s.min() >= 2.0 ** 12
    _, dyb, Lb = T.checkpoint_case(64, 40, 1)
    rms = np.sqrt((dyb.astype(np.float64) ** 2).mean(0))
    assert rms.max() / rms.min() >= 2.0 ** 12 and (Lb["gamma"] == 0).any() and (Lb["gamma"] < 0).any()
    pos = T.impulse_pixels(13, 9, splits_rows=(3, 6))
    for want in ((0, 0), (12, 8), (2, 3), (3, 3), (1, 3), (1, 4), (3, 1), (4, 1), (6, 8)):
        assert want in pos, want
    x = T.small_integers((5, 7, 3), rng)
    assert (x == np.round(x)).all() and x.min() >= 1


def test_virtual_layers_of_the_convolution_kernel_dgrad_equal_the_input_gradient():
    """T.virtual_weights (the flipped, transposed layer the stride-1 dgrad runs) and T.poly_pseudo_weights (the four parities of a
    stride-2 layer) reproduce conv2d's input gradient, and the Winograd condition term dominates the direct one."""
    rng = np.random.default_rng(4)
    cin, cout, H, W = 8, 3, 9, 7
    cp = T.pad8(cout)
    for k in (1, 3):
        wf, wm = (rng.standard_normal((cout, cin, k, k)).astype(f32) for _ in range(2))
        dfm = np.zeros((H, W, 2 * cp), f32)
        dfm[:, :, :cout], dfm[:, :, cp:cp + cout] = rng.standard_normal((2, H, W, cout))
        ref, cond = T.dgrad_ref(dfm, cout, wf, wm, k, 1, H, W)
        wv = T.virtual_weights(wf, wm)
        y = F.conv2d(torch.from_numpy(dfm.astype(np.float64).transpose(2, 0, 1).copy())[None], torch.from_numpy(wv), padding=(k - 1) // 2)[0]
        assert np.abs(y.numpy().transpose(1, 2, 0) - ref).max() <= 1e-12 * np.abs(ref).max()
        if k == 3:
            for fam in ("w2", "w4"):
                bound, Aw = T.conv_dgrad_bound(dfm, wv, cond, ref, fam)
                assert (Aw >= cond * (1 - 1e-12)).all() and (bound > 0).all()
    for k in (3, 4):
        H, W = 8, 12
        oh, ow = T.out_hw(k, 2, H, W)
        wf, wm = (rng.standard_normal((cout, cin, k, k)).astype(f32) for _ in range(2))
        dfm = np.zeros((oh, ow, 2 * cp), f32)
        dfm[:, :, :cout], dfm[:, :, cp:cp + cout] = rng.standard_normal((2, oh, ow, cout))
        ref, _ = T.dgrad_ref(dfm, cout, wf, wm, k, 2, H, W)
        pf, pm = T.poly_pseudo_weights(wf, k), T.poly_pseudo_weights(wm, k)
        for par in range(4):
            r, _ = T.dgrad_ref(dfm, cout, pf[par], pm[par], 3, 1, oh, ow)
            assert np.abs(r - ref[par >> 1::2, par & 1::2]).max() <= 1e-12 * np.abs(ref).max()
