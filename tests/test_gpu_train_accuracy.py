"""GPU: the training kernels of read_amd/csrc/train.hip, each called directly through the C entry points, against the float64 references
of tests/train_ref64.py in units of fp32 round-off (E = |got - ref| / (u cond)), on unit-scale (a), checkpoint-like (b), structured (c)
and range-edge (d) inputs.  Every element of every case is measured.  Each launch is held to
  1. the derived bound, elementwise (tests/train_ref64.py counts the roundings): a case over it is a kernel bug or a flaw in the derivation;
  2. the yardstick cap  E_rms <= 2 max(R_torch_rms, R_seq_rms, 0.5),  E_max <= 2 max(R_torch_max, R_seq_max, 1)  with R the same statistic
     of the torch-fp32 operation and of a NumPy fp32 restatement that sums sequentially, both on the CPU on the same inputs.  Rows that
     legitimately need more (`raised`; profiles/train_accuracy_fp64.md explains each) are capped by the leading term of the derived bound;
  3. exactness where no product reaches the output: separator rows are 0, padded channels of d[f|m] are 0, impulse rows of the direct dW
     are the integers of x, accumulate after a zero gradient leaves the buffer bit-identical.
Run with -s to see the table; lines start with "TACC|".  tests/test_gpu_train.py stays the end-to-end parity test."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from read_amd import _lib
from tests import conv_ref64 as R64
from tests import train_ref64 as T
from tests.train_fp32 import bn_bwd_coeff32, bn_forward32, bn_grads32, gate32, gate_backward32

pytestmark = pytest.mark.gpu
f32 = np.float32


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _params(hip, C, gamma, beta, mean, var, eps):
    p = torch.zeros(hip.read_conv_param_floats(C), dtype=torch.float32, device="cuda")
    keep = [_dev(a) for a in (gamma, beta, mean, var)]
    _lib.check(hip.read_conv_pack_params_device(C, None, None, *[t.data_ptr() for t in keep], eps, p.data_ptr(), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return p


def _identity_params(hip, C):
    return _params(hip, C, np.ones(C, f32), np.zeros(C, f32), np.zeros(C, f32), np.ones(C, f32), 0.0)


MEASURE_FLOOR = 2.0 ** -100        # E does not count differences below this: results that small are in or next to fp32's subnormal range
                                   # (sigmoid(-150) is 0 in fp32), where u cond is no yardstick; rule 1 still sees them (FLUSH, TINY)


def judge(family, cls, name, got, ref, cond, bound, yard, lead=None, extra="", zero_cond_by_bound=False):
    """One TACC line and the three assertions.  yard: {"torch": array, "seq": array} (either may be missing); lead: the leading term of
    the derived bound, elementwise: the cap of a row that misses the yardstick cap (module docstring, 2.; printed as `raised`).  zero_cond_by_bound: entries whose condition
    term is 0 but whose formulation on the device is not an exact constant (dgamma of a constant channel) are held to rule 1 alone."""
    got = np.asarray(got, np.float64)
    finite = bool(np.isfinite(got).all())
    err = np.abs(np.nan_to_num(got, nan=3e38, posinf=3e38, neginf=-3e38) - ref)
    q = T.worst(err, bound)
    keep = Ellipsis
    if zero_cond_by_bound:
        keep = np.asarray(cond) > 0
        ref, cond, err = np.asarray(ref)[keep], np.asarray(cond)[keep], err[keep]
        lead = None if lead is None else np.asarray(lead)[keep]
    meas = lambda e: T.stats(np.where(e <= MEASURE_FLOOR, 0.0, e), cond) if np.size(e) else (0.0, 0.0)      # noqa: E731
    e_max, e_rms = meas(err)
    R = {k: meas(np.abs(np.asarray(v, np.float64)[keep] - ref)) for k, v in yard.items()}
    rt, rs = R.get("torch", (float("nan"),) * 2), R.get("seq", (float("nan"),) * 2)
    fin = [r for r in R.values() if np.isfinite(r[0])]
    cap_max = 2 * max([r[0] for r in fin] + [1.0])
    cap_rms = 2 * max([r[1] for r in fin] + [0.5])
    raised = False
    if lead is not None and not (e_max <= cap_max and e_rms <= cap_rms):      # only a row that needs more than the yardsticks allow
        l_max, l_rms = T.stats(lead, cond) if np.size(lead) else (0.0, 0.0)
        cap_max, cap_rms, raised = max(cap_max, l_max), max(cap_rms, l_rms), True
    print("TACC| %-12s | %s | %-46s | E_max %10.2f | E_rms %9.3f | R_torch max %8.2f rms %7.3f | R_seq max %8.2f rms %7.3f | err/bound %6.3f |%s%s" % (
        family, cls, name, e_max, e_rms, rt[0], rt[1], rs[0], rs[1], q, " raised |" if raised else "", extra))
    what = f"{family} ({cls}) {name}"
    if not finite:
        FAILED.append(f"{what}: non-finite output inside the documented range")
    if not q <= 1.0:
        FAILED.append(f"{what}: {q:.3f} x the derived bound (E_max {e_max:.1f}, E_rms {e_rms:.2f})")
    if not (e_max <= cap_max and e_rms <= cap_rms):
        FAILED.append(f"{what}: E_max {e_max:.2f} E_rms {e_rms:.3f} against the caps {cap_max:.2f} / {cap_rms:.3f}")
    return e_max, e_rms


FAILED = []                # every row of a test is measured and printed before the test fails on the rows that missed an assertion


def finish():
    msgs = list(FAILED)
    del FAILED[:]
    assert not msgs, "%d rows failed:\n" % len(msgs) + "\n".join(msgs)


# ------------------------------------------------------------------------------------------ gate and BatchNorm
GATE_C = (3, 8, 9, 40, 56, 32, 64, 128, 256, 96, 160)
GATE_GEOM = ((7 * 13, 13, 0, 0, (1,)), (5, 5, 0, 0, (1,)), (3 * 5 * 7, 7, 5, 3, (1, 3)))            # (P, W, block_h, valid_h, groups)
UNET_GEOM = (2 * 20 * 8, 8, 20, 16, (1, 2))


def _centred(ref):
    """cond_dgamma in the centred form; a channel whose deviations from its mean are below 2^-30 of its values (a constant channel: the
    float64 gate leaves one ulp of 100) has no centred scale that fp32 tensors could express: 0, i.e. held to the derived bound alone."""
    c, k = ref.cond_dgamma["centered"], ref.cond_dgamma["kernel"]
    return np.where(c <= 2.0 ** -30 * k, 0.0, c)


def _gate_inputs(cls, P, C, seed):
    if cls == "a":
        return T.unit_case(P, C, seed)
    if cls == "b":
        return T.checkpoint_case(P, C, seed)
    return T.range_edge_case(P, C, seed)[:3]


def _gate_cases():
    for C in GATE_C:
        for cls in "abd":
            for geom in GATE_GEOM:
                yield C, cls, geom
    yield 32, "a", UNET_GEOM
    yield 7, "d", (1536, 32, 0, 0, (1,))                             # one channel of every kind at the pixel count DESIGN.md quotes
    yield 32, "d", (1536, 32, 0, 0, (1,))                            # the same through gate_backward4_kernel


def _torch32_eval(fm, dy, C, L, elu, residual, v):
    t = torch.from_numpy(fm).requires_grad_(True)
    par = {k: torch.from_numpy(L[k]).requires_grad_(k in ("gamma", "beta")) for k in ("gamma", "beta", "mean", "var")}
    f = t[:, :C]
    g = (F.elu(f) if elu else f) * torch.sigmoid(t[:, C:])
    y = F.batch_norm(g.t()[None], par["mean"], par["var"], par["gamma"], par["beta"], training=False, eps=T.EPS)[0].t()
    if residual is not None:
        y = y + torch.from_numpy(residual)
    vm = torch.from_numpy(v.astype(f32))[:, None]
    (y * torch.from_numpy(dy) * vm).sum().backward()
    return (y.detach() * vm).numpy(), t.grad[:, :C].numpy(), t.grad[:, C:].numpy(), par["gamma"].grad.numpy(), par["beta"].grad.numpy()


# Degenerate sizes: 1, 4 and 12 pixels (the coarse levels of a 16-pixel crop: 1 x 1, 2 x 2, 2 x 6) and three stacked 2 x 2 items with
# one separator row each, at 3, 9 and 256 channels.  Batch statistics over ONE value per channel (what feat_extract.7 sees on a single
# 16 x 16 crop) are refused by torch's F.batch_norm, so the torch yardstick does not exist for that geometry; the library computes them
# (mean = the value, var = 0, y = beta, running_var moves towards 0) and is held there to the float64 reference of tests/train_ref64.py,
# which has no such restriction, to the derived bounds and to the sequential yardstick alone.
TINY_GEOM = ((1, 1, 0, 0, (1,)), (4, 2, 0, 0, (1,)), (12, 6, 0, 0, (1,)), (3 * 3 * 2, 2, 3, 2, (1, 3)))


def _tiny_gate_cases(batch_statistics):
    for C in (3, 9, 256):
        for cls in "ab":
            for geom in TINY_GEOM:
                yield C, cls, geom


def test_gate_forward_and_eval_backward(hip):
    """read_gate_forward, read_gate_backward, read_bn_param_grads."""
    _gate_eval_rows(hip, _gate_cases())


def test_gate_forward_and_eval_backward_at_degenerate_sizes(hip):
    _gate_eval_rows(hip, _tiny_gate_cases(False))


def _gate_eval_rows(hip, cases):
    st = _lib.stream_ptr()
    for C, cls, (P, W, bh, vh, _groups) in cases:
        fm, dy, L = _gate_inputs(cls, P, C, 21)
        if cls == "d":                                               # eval mode after training: the running statistics are the channels' own
            g64 = T.Gate(fm, C, True).g
            L["mean"], L["var"] = g64.mean(0).astype(f32), g64.var(0).astype(f32)
        rng = np.random.default_rng([C, P])
        res = rng.standard_normal((P, C)).astype(f32)
        cp = T.pad8(C)
        v = T.valid_rows(P, W, bh, vh)
        name = f"C {C} P {P} W {W} block {bh}/{vh}"
        params = _params(hip, C, L["gamma"], L["beta"], L["mean"], L["var"], T.EPS)
        fm_d, dy_d, res_d = _dev(fm), _dev(dy), _dev(res)
        sc = (L["gamma"] / np.sqrt((L["var"] + f32(T.EPS)).astype(f32)).astype(f32)).astype(f32)
        sh = (L["beta"] - (L["mean"] * sc).astype(f32)).astype(f32)
        a, da, s = gate32(fm, C, True)
        for residual in (None, res):
            y = torch.full((P, C), 7.0, device="cuda")
            _lib.check(hip.read_gate_forward(fm_d.data_ptr(), P, C, params.data_ptr(), 1, res_d.data_ptr() if residual is not None else None,
                                             y.data_ptr(), W, bh, vh, st))
            y_ref, B, bound, cond = T.gate_forward_ref(fm, C, L, True, residual, W, bh, vh)
            yt = _torch32_eval(fm, dy, C, L, True, residual, v)[0]
            ys = (((a * s).astype(f32) * sc[None]).astype(f32) + sh[None]).astype(f32)
            ys = ((ys + residual).astype(f32) if residual is not None else ys) * v[:, None]
            got = _host(y)
            judge("gate_fwd", cls, name + (" +res" if residual is not None else ""), got, y_ref, B, bound, {"torch": yt, "seq": ys})
            assert not got[~v].any(), name + ": separator rows of y are not zero"
            const = (cond == 0) & v[:, None]                        # gamma = 0: the shift (+ residual), exactly
            if const.any():
                want = (np.broadcast_to(sh[None], (P, C)) + (residual if residual is not None else 0)).astype(f32)
                assert np.array_equal(got[const], want[const]), name + ": outputs that no product reaches differ from the constant"
        # backward
        dfm = torch.full((P, 2 * cp), 7.0, device="cuda")
        sums = torch.zeros((4, C), device="cuda")
        _lib.check(hip.read_gate_backward(dy_d.data_ptr(), fm_d.data_ptr(), P, C, params.data_ptr(), 1, dfm.data_ptr(), sums.data_ptr(), W, bh, vh, st))
        grads = torch.zeros((4, C), device="cuda")                   # dbf, dbm, dgamma, dbeta
        mean_d, var_d = _dev(L["mean"]), _dev(L["var"])
        _lib.check(hip.read_bn_param_grads(C, sums.data_ptr(), mean_d.data_ptr(), var_d.data_ptr(), T.EPS, grads[0].data_ptr(), grads[1].data_ptr(),
                                           grads[2].data_ptr(), grads[3].data_ptr(), st))
        dfm_h, sums_h, grads_h = _host(dfm), _host(sums), _host(grads)
        ref = T.GateBackwardEval(dy, fm, C, L, True, W, bh, vh)
        _, dft, dmt, dgt, dbt = _torch32_eval(fm, dy, C, L, True, None, v)
        dfs, dms, sums_s = gate_backward32(dy, fm, C, sc, True, v, 0, geometry=(1, 1))
        judge("gate_bwd df", cls, name, dfm_h[:, :C], ref.df, ref.cond_df, ref.bound_df, {"torch": dft, "seq": dfs})
        judge("gate_bwd dm", cls, name, dfm_h[:, cp:cp + C], ref.dm, ref.cond_dm, ref.bound_dm, {"torch": dmt, "seq": dms})
        assert not dfm_h[:, C:cp].any() and not dfm_h[:, cp + C:].any(), name + ": padded channels of d[f|m] are not zero"
        assert not dfm_h[~v].any(), name + ": separator rows of d[f|m] are not zero"
        judge("gate_bwd sums", cls, name, sums_h, ref.sums, ref.cond_sums, ref.bound_sums,
              {"torch": np.stack([dft.sum(0), dmt.sum(0), dbt, sums_s[3]]), "seq": sums_s}, lead=ref.lead_sums)
        assert np.array_equal(grads_h[0], sums_h[0]) and np.array_equal(grads_h[1], sums_h[1]) and np.array_equal(grads_h[3], sums_h[2])
        lead = ref.lead_dgamma if cls == "d" else ref.lead_dgamma_terms
        judge("bn_grads dgamma", cls, name, grads_h[2], ref.dgamma, _centred(ref), ref.bound_dgamma,
              {"torch": dgt, "seq": bn_grads32(sums_s, L["mean"], L["var"])}, lead=lead, zero_cond_by_bound=True,
              extra=" E(kernel form) max %.2f |" % T.stats(np.abs(grads_h[2] - ref.dgamma), ref.cond_dgamma["kernel"])[0])
    finish()


def _torch32_bn(fm, dy, C, L, v, grp, groups, momentum):
    """torch fp32: F.batch_norm(training) per statistic group over the gate's output, and its autograd."""
    t = torch.from_numpy(fm).requires_grad_(True)
    ga, be = torch.from_numpy(L["gamma"]).requires_grad_(True), torch.from_numpy(L["beta"]).requires_grad_(True)
    g = F.elu(t[:, :C]) * torch.sigmoid(t[:, C:])
    rm, rv = torch.from_numpy(L["mean"].copy()), torch.from_numpy(L["var"].copy())
    y_all = np.zeros(dy.shape, f32)
    tot = 0.0
    for j in range(groups):
        idx = torch.from_numpy(np.nonzero(v & (grp == j))[0])
        y = F.batch_norm(g[idx].t()[None], rm, rv, ga, be, training=True, momentum=momentum, eps=T.EPS)[0].t()
        y_all[idx.numpy()] = y.detach().numpy()
        tot = tot + (y * torch.from_numpy(dy)[idx]).sum()
    tot.backward()
    return y_all, rm.numpy(), rv.numpy(), t.grad[:, :C].numpy(), t.grad[:, C:].numpy(), ga.grad.numpy(), be.grad.numpy()


def test_batch_statistics_batchnorm_forward_and_backward(hip):
    """read_bn_train_forward, read_gate_backward_bn, read_bn_param_grads_groups: both group modes."""
    _bn_rows(hip, _gate_cases())


def test_batch_statistics_batchnorm_at_degenerate_sizes(hip):
    """... statistics over 4 and 12 values per channel, and per item over the 4 valid pixels of each of three stacked 2 x 2 items.
    dbeta is given the rule's second yardstick here, a sequential fp32 sum of dy (the larger tests pass torch's alone): over 12 terms
    autograd's reduction can land within one unit where any other order of the same additions is at two (measured on the CPU on the
    (b) case of C = 256: both the sequential sum and torch.sum are at 2.03, autograd's dbeta at 1.03), and the cap 2 max(R, 1) is meant
    to be taken over the orders a correct sum may use."""
    _bn_rows(hip, _tiny_gate_cases(True), dbeta_seq=True)


def _bn_rows(hip, cases, dbeta_seq=False):
    st = _lib.stream_ptr()
    mom = 0.1
    for C, cls, (P, W, bh, vh, group_modes) in cases:
        fm, dy, L = _gate_inputs(cls, P, C, 22)
        cp, cpad = T.pad8(C), (C + 31) // 32 * 32
        v = T.valid_rows(P, W, bh, vh)
        ident = _identity_params(hip, C)
        fm_d, dy_d, gamma_d, beta_d = _dev(fm), _dev(dy), _dev(L["gamma"]), _dev(L["beta"])
        gt = T.Gate(fm, C, True)
        for groups in group_modes:
            name = f"C {C} P {P} W {W} block {bh}/{vh} groups {groups}"
            grp = T.group_of(P, W, bh, groups)
            # forward: g from the device's own gate (identity BatchNorm), normalised in place
            y = torch.full((P, C), 7.0, device="cuda")
            _lib.check(hip.read_gate_forward(fm_d.data_ptr(), P, C, ident.data_ptr(), 1, None, y.data_ptr(), W, bh, vh, st))
            g_dev = _host(y).copy()
            rm_d, rv_d = _dev(L["mean"]), _dev(L["var"])
            stat = torch.zeros((groups, 2, C), device="cuda")
            ss = torch.zeros((groups, 2, cpad), device="cuda")
            scratch = torch.zeros(2 * C * groups, dtype=torch.float64, device="cuda")
            _lib.check(hip.read_bn_train_forward(y.data_ptr(), P, C, W, bh, vh, groups, gamma_d.data_ptr(), beta_d.data_ptr(), T.EPS, mom,
                                                 rm_d.data_ptr(), rv_d.data_ptr(), stat.data_ptr(), ss.data_ptr(), scratch.data_ptr(), st))
            y_h, stat_h, rm_h, rv_h = _host(y), _host(stat), _host(rm_d), _host(rv_d)
            fwd = T.BnForward(g_dev, L, W, bh, vh, groups, mom, L["mean"], L["var"])          # the reference of THIS kernel: its own input g
            yt = np.zeros((P, C), f32)
            ys, rm_s, rv_s = np.zeros((P, C), f32), L["mean"].copy(), L["var"].copy()
            rm_t, rv_t = torch.from_numpy(L["mean"].copy()), torch.from_numpy(L["var"].copy())
            torch_ok = min(int((v & (grp == j)).sum()) for j in range(groups)) > 1     # F.batch_norm refuses one value per channel
            only = (lambda d: d) if torch_ok else (lambda d: {k_: v_ for k_, v_ in d.items() if k_ != "torch"})
            for j in range(groups):
                sel = v & (grp == j)
                ys[sel], _, _, rm_s, rv_s = bn_forward32(g_dev[sel], L["gamma"], L["beta"], mom, rm_s, rv_s)
                if torch_ok:
                    yt[sel] = F.batch_norm(torch.from_numpy(g_dev[sel]).t()[None], rm_t, rv_t, torch.from_numpy(L["gamma"]), torch.from_numpy(L["beta"]),
                                           training=True, momentum=mom, eps=T.EPS)[0].t().numpy()
            judge("bn_fwd y", cls, name, y_h, fwd.y, fwd.cond_y, fwd.bound_y, only({"torch": yt, "seq": ys}),
                  extra=" E(xhat) max %.2f torch %.2f |" % (T.stats(np.abs(y_h - fwd.y), fwd.cond_y_centered)[0], T.stats(np.abs(yt - fwd.y), fwd.cond_y_centered)[0]))
            assert not y_h[~v].any(), name + ": separator rows of y are not zero"
            judge("bn_fwd stat", cls, name, stat_h, fwd.stat, fwd.cond_stat, fwd.bound_stat, {})
            judge("bn_fwd running", cls, name, np.stack([rm_h, rv_h]), np.stack([fwd.running_mean, fwd.running_var]),
                  np.stack([fwd.cond_rm, fwd.cond_rv]), np.stack([fwd.bound_rm, fwd.bound_rv]),
                  only({"torch": np.stack([rm_t.numpy(), rv_t.numpy()]), "seq": np.stack([rm_s, rv_s])}))
            # backward with the forward's statistics
            dfm = torch.full((P, 2 * cp), 7.0, device="cuda")
            sums = torch.zeros((groups, 4, C), device="cuda")
            abc = torch.zeros((groups, 3, C), device="cuda")
            _lib.check(hip.read_gate_backward_bn(dy_d.data_ptr(), fm_d.data_ptr(), P, C, ident.data_ptr(), 1, dfm.data_ptr(), sums.data_ptr(), W, bh, vh,
                                                 groups, stat.data_ptr(), gamma_d.data_ptr(), T.EPS, abc.data_ptr(), st))
            grads = torch.zeros((4, C), device="cuda")
            _lib.check(hip.read_bn_param_grads_groups(C, groups, sums.data_ptr(), stat.data_ptr(), T.EPS, grads[0].data_ptr(), grads[1].data_ptr(),
                                                      grads[2].data_ptr(), grads[3].data_ptr(), st))
            dfm_h, grads_h = _host(dfm), _host(grads)
            ref = T.GateBackwardBn(dy, fm, C, L["gamma"], True, W, bh, vh, groups, stat_h)
            zc = np.zeros(C, f32)
            _, _, _, dft, dmt, dgt, dbt = _torch32_bn(fm, dy, C, L, v, grp, groups, mom) if torch_ok else (None, None, None, np.zeros((P, C), f32), np.zeros((P, C), f32), zc, zc)
            dfs, dms, dgs = np.zeros((P, C), f32), np.zeros((P, C), f32), np.zeros(C, f32)
            one = np.ones(C, f32)
            for j in range(groups):
                idx = np.nonzero(grp == j)[0]
                _, _, s1 = gate_backward32(dy[idx], fm[idx], C, one, True, v[idx], 1, geometry=(1, 1))
                coeff = bn_bwd_coeff32(s1, stat_h[j, 0], stat_h[j, 1], L["gamma"], int(v[idx].sum()))
                dfs[idx], dms[idx], s2 = gate_backward32(dy[idx], fm[idx], C, one, True, v[idx], 2, coeff, geometry=(1, 1))
                dgs = dgs + bn_grads32(s2, stat_h[j, 0], stat_h[j, 1])
            raised = cls == "d"
            # df, dm: the condition term of dg carried through the gate's factors
            cdf, cdm = ref.cond_dg * gt.sig * gt.da_abs, ref.cond_dg * gt.a_abs * gt.sig * (1 + gt.sig)
            cdf_dg = (gt.f > 0) & (gt.sig == 1.0) & v[:, None]       # where df IS dg (the ratio and constant channels of class (d))
            dg_dev = np.where(cdf_dg, dfm_h[:, :C], ref.dg)
            judge("bn_bwd df", cls, name, dfm_h[:, :C], ref.df, cdf, ref.bound_df, only({"torch": dft, "seq": dfs}), lead=ref.lead_df if raised else None)
            judge("bn_bwd dm", cls, name, dfm_h[:, cp:cp + C], ref.dm, cdm, ref.bound_dm, only({"torch": dmt, "seq": dms}), lead=ref.lead_dm if raised else None)
            assert not dfm_h[:, C:cp].any() and not dfm_h[:, cp + C:].any() and not dfm_h[~v].any(), name + ": padding / separator rows of d[f|m]"
            per_kind = ""
            if raised and P == 1536:
                e = np.where(_centred(ref) > 0, np.abs(grads_h[2] - ref.dgamma) / np.maximum(T.U * ref.cond_dgamma["centered"], 1e-300), np.nan)
                eg = np.where(cdf_dg > 0, np.abs(dg_dev - ref.dg) / np.maximum(T.U * ref.cond_dg, 1e-300), 0.0).max(0)
                per_kind = " per kind E(dgamma) / worst E(dg): " + ", ".join("%s %.1f / %.1f" % (k_, max(e[c] for c in range(C) if c % 7 == i), max(eg[c] for c in range(C) if c % 7 == i))
                                                                                 for i, k_ in enumerate(T.D_CHANNELS)) + " |"
            judge("bn_bwd dgamma", cls, name, grads_h[2], ref.dgamma, _centred(ref), ref.bound_dgamma, only({"torch": dgt, "seq": dgs}),
                  lead=ref.lead_dgamma_terms + (ref.lead_dgamma if raised else 0), zero_cond_by_bound=True, extra=per_kind)
            yard_dbeta = only({"torch": dbt})
            if dbeta_seq:
                yard_dbeta["seq"] = np.add.accumulate(dy * v[:, None].astype(f32), axis=0, dtype=f32)[-1]
            judge("bn_bwd dbeta", cls, name, grads_h[3], ref.dbeta, ref.cond_dbeta, ref.bound_dbeta, yard_dbeta)
            judge("bn_bwd dbf", cls, name, grads_h[0], ref.dbf, cdf.sum(0), ref.bound_dbf, only({"torch": dft.sum(0), "seq": np.add.accumulate(dfs, axis=0, dtype=f32)[-1]}),
                  lead=ref.lead_dbf + (ref.lead_df.sum(0) if raised else 0))
            judge("bn_bwd dbm", cls, name, grads_h[1], ref.dbm, cdm.sum(0), ref.bound_dbm, only({"torch": dmt.sum(0), "seq": np.add.accumulate(dms, axis=0, dtype=f32)[-1]}),
                  lead=ref.lead_dbm + (ref.lead_dm.sum(0) if raised else 0))
    finish()


# ------------------------------------------------------------------------------------------ weight gradients
def _knob(hip, value=None):
    """The wgrad_wino knob: its value, or set it."""
    import ctypes
    if value is None:
        v = ctypes.c_int()
        _lib.check(hip.read_tuning_get(b"wgrad_wino", ctypes.byref(v)))
        return v.value
    _lib.check(hip.read_tuning_set(b"wgrad_wino", value))


def _dfm(d_f, d_m, cout):
    cp = T.pad8(cout)
    out = np.zeros(d_f.shape[:2] + (2 * cp,), f32)
    out[:, :, :cout], out[:, :, cp:cp + cout] = d_f, d_m
    return out


def _wgrad(hip, x, dfm, cout, k, stride, accumulate=0, init=None):
    H, W, cin = x.shape
    oh, _ = T.out_hw(k, stride, H, W)
    n_scr = hip.read_conv_wgrad_scratch_floats(cin, cout, k, oh)
    scratch = torch.empty(n_scr, dtype=torch.float32, device="cuda")
    dw = [torch.full((cout, cin, k, k), 7.0, device="cuda") if init is None else _dev(init[i]) for i in range(2)]
    x_d, d_d = _dev(x), _dev(dfm)
    _lib.check(hip.read_conv_wgrad(x_d.data_ptr(), H, W, cin, d_d.data_ptr(), cout, k, stride, dw[0].data_ptr(), dw[1].data_ptr(), accumulate,
                                   scratch.data_ptr(), n_scr, _lib.stream_ptr()))
    return _host(dw[0]), _host(dw[1])


def _wgrad_inputs(cls, cin, cout, H, W, oh, ow, rng):
    sx, sd = (T.scales_b(cin, rng), T.scales_b(2 * cout, rng)) if cls == "b" else (np.ones(cin), np.ones(2 * cout))
    if cls == "const":
        x = R64.constant_image(cin, H, W).transpose(1, 2, 0).copy()
    elif cls == "checker":
        x = R64.checkerboard(cin, H, W).transpose(1, 2, 0).copy()
    else:
        x = (rng.standard_normal((H, W, cin)) * sx).astype(f32)
    d = (rng.standard_normal((oh, ow, 2 * cout)) * sd).astype(f32)
    return x, d[:, :, :cout].copy(), d[:, :, cout:].copy()


DIRECT_LAYERS = ((8, 3, 3, 1), (48, 20, 3, 1), (64, 40, 3, 1), (32, 64, 3, 2), (64, 32, 4, 2), (16, 32, 1, 1), (96, 32, 1, 1), (192, 32, 1, 1),
                 (128, 64, 1, 1), (160, 56, 1, 1))


def _judge_wgrad(family, cls, name, got, x, dparts, k, stride, bound_fn, cond_fn=None, previous=None, yard=True):
    for half, (g, d) in enumerate(zip(got, dparts)):
        ref, A = T.wgrad_ref(x, d, k, stride)
        cond = A if cond_fn is None else cond_fn(x, d)
        extra = ""
        if cond_fn is not None:
            extra = " E(A) max %.2f rms %.3f |" % T.stats(np.abs(g - ref), A)
        prev = None if previous is None else previous[half]
        if prev is not None:
            ref, cond = ref + prev, cond + np.abs(prev)
        y = {}
        if yard:
            y = {"torch": T.wgrad_torch32(x, d, k, stride), "seq": T.wgrad_seq32(x, d, k, stride)}
            if prev is not None:
                y = {n: (v + prev).astype(f32) for n, v in y.items()}
        judge(family, cls, name + (" dWf", " dWm")[half], g, ref, cond, bound_fn(cond, prev), y, extra=extra)


def test_direct_weight_gradient(hip):
    """read_conv_wgrad on wgrad_mfma_kernel + wgrad_reduce_kernel (knob wgrad_wino = 0)."""
    rng = np.random.default_rng(31)
    knob = _knob(hip)
    _knob(hip, 0)
    try:
        cases = [(l, hw, cls) for l in DIRECT_LAYERS for hw in ((7, 9), (13, 5)) for cls in "ab"]
        cases += [((8, 3, 3, 1), (7, 9), "const"), ((64, 32, 4, 2), (13, 5), "checker"), ((256, 256, 3, 1), (40, 8), "a"), ((256, 256, 3, 1), (40, 8), "b")]
        for (cin, cout, k, stride), (H, W), cls in cases:
            oh, ow = T.out_hw(k, stride, H, W)
            assert hip.read_conv_wgrad_family(cin, k, stride, H, W) == 0
            x, df, dm = _wgrad_inputs(cls, cin, cout, H, W, oh, ow, rng)
            name = f"{cin}->{cout} k{k} s{stride} {H}x{W}"
            dfm = _dfm(df, dm, cout)
            got = _wgrad(hip, x, dfm, cout, k, stride)
            _judge_wgrad("wgrad", "c" if cls in ("const", "checker") else cls, name, got, x, (df, dm), k, stride,
                         lambda A, prev: T.wgrad_direct_bound(A, cin, cout, k, oh, ow))
            # accumulate = 1 onto a previous gradient, and onto the result with a zero d[f|m]: bit-identical
            prev = [rng.standard_normal(got[0].shape).astype(f32) for _ in range(2)]
            acc = _wgrad(hip, x, dfm, cout, k, stride, accumulate=1, init=prev)
            _judge_wgrad("wgrad acc", "c" if cls in ("const", "checker") else cls, name, acc, x, (df, dm), k, stride,
                         lambda A, p: T.wgrad_direct_bound(A - np.abs(p), cin, cout, k, oh, ow, True, p), previous=prev)
            same = _wgrad(hip, x, np.zeros_like(dfm), cout, k, stride, accumulate=1, init=got)
            assert np.array_equal(same[0], got[0]) and np.array_equal(same[1], got[1]), name + ": accumulating a zero gradient changed the buffer"
    finally:
        _knob(hip, knob)
    finish()


def test_direct_weight_gradient_reads_impulses_back_exactly(hip):
    """Class (c): one non-zero pixel of d[f|m] (1, then 2^-10) over an x of small integers: every entry of dW is that multiple of one entry
    of x, exactly."""
    rng = np.random.default_rng(32)
    knob = _knob(hip)
    _knob(hip, 0)
    try:
        for (cin, cout, k, stride), (H, W) in (((8, 3, 3, 1), (7, 9)), ((32, 64, 3, 2), (13, 5)), ((64, 32, 4, 2), (7, 9)), ((192, 32, 1, 1), (13, 5)),
                                               ((256, 256, 3, 1), (40, 8))):
            oh, ow = T.out_hw(k, stride, H, W)
            plan = T.wgrad_plan(cin, cout, k, oh)
            x = T.small_integers((H, W, cin), rng)
            pad = (k - 1) // 2
            xp = np.zeros((H + 2 * pad + k, W + 2 * pad + k, cin), f32)
            xp[pad:pad + H, pad:pad + W] = x
            pos = T.impulse_pixels(oh, ow, splits_rows=range(plan["rows_per_split"], oh, plan["rows_per_split"]))
            if cin == 256:
                pos = [p for p in pos if p[1] == ow // 3 or p in ((0, 0), (oh - 1, ow - 1))]
            for (py, px) in pos:
                for amp in (1.0, 2.0 ** -10):
                    d = np.zeros((oh, ow, cout), f32)
                    d[py, px] = amp
                    got = _wgrad(hip, x, _dfm(d, d, cout), cout, k, stride)
                    want = np.broadcast_to((f32(amp) * xp[py * stride:py * stride + k, px * stride:px * stride + k]).transpose(2, 0, 1)[None], got[0].shape)
                    assert np.array_equal(got[0], want) and np.array_equal(got[1], want), f"{cin}->{cout} k{k} s{stride} {H}x{W}: impulse at {(py, px)} x {amp}"
            print("TACC| %-12s | c | %-46s | %d impulse positions x 2 amplitudes read back exactly" % ("wgrad", f"{cin}->{cout} k{k} s{stride} {H}x{W}", len(pos)))
    finally:
        _knob(hip, knob)


def test_winograd_domain_weight_gradient(hip):
    """read_conv_wgrad on wgrad_wino4_kernel, wgrad_wino4_sum_kernel, wgrad_wino4_reduce_kernel: E against A_w asserted, E(A) printed."""
    rng = np.random.default_rng(33)
    knob = _knob(hip)
    _knob(hip, 1)
    try:
        _winograd_wgrad_cases(hip, rng)
    finally:
        _knob(hip, knob)
    finish()


def _winograd_wgrad_cases(hip, rng):
    for (cin, cout, H, W) in ((32, 32, 4, 4), (128, 128, 44, 36), (32, 3, 8, 12), (64, 40, 12, 20)):
        # class (c): one non-zero pixel of d[f|m] (1, then 2^-10) over an x of small integers, at the corners, the edges and both sides
        # of every 4 x 4 tile boundary and of every boundary between two splits of tile rows; judged against A_w (the transforms round)
        plan = T.wgrad4_plan(cin, cout, H)
        pos = T.impulse_pixels(H, W, splits_rows=range(4 * plan["rows_per_split"], H, 4 * plan["rows_per_split"]))
        if cin == 128:
            pos = [p for p in pos if p[1] == W // 3 or p in ((0, 0), (H - 1, W - 1), (3, 1), (4, 1), (1, 31), (1, 32))]
        xi = T.small_integers((H, W, cin), rng)
        for (py, px) in pos:
            for amp in ((1.0,) if cin == 128 else (1.0, 2.0 ** -10)):
                d = np.zeros((H, W, cout), f32)
                d[py, px] = amp
                got = _wgrad(hip, xi, _dfm(d, d, cout), cout, 3, 1)
                _judge_wgrad("wgrad_wino", "c", f"{cin}->{cout} {H}x{W} impulse {py},{px} x {amp:g}", got, xi, (d, d), 3, 1,
                             lambda Aw, prev: T.wgrad_wino_bound(Aw, cin, cout, H, W), cond_fn=T.wgrad_wino_Aw, yard=cin < 128)
        for cls in ("a", "b", "const", "checker"):
            if cls in ("const", "checker") and cin == 128:
                continue
            assert hip.read_conv_wgrad_family(cin, 3, 1, H, W) == 4
            x, df, dm = _wgrad_inputs(cls, cin, cout, H, W, H, W, rng)
            name = f"{cin}->{cout} {H}x{W}"
            dfm = _dfm(df, dm, cout)
            got = _wgrad(hip, x, dfm, cout, 3, 1)
            c = "c" if cls in ("const", "checker") else cls
            # the yardsticks sum in the pixel domain: they lack the 8 + 10 transform roundings and the amplification of |B^T|, |A|, |G|
            # that A_w already carries; against A_w they sit far below 1, so the floors of the yardstick cap are what holds these rows
            _judge_wgrad("wgrad_wino", c, name, got, x, (df, dm), 3, 1, lambda Aw, prev: T.wgrad_wino_bound(Aw, cin, cout, H, W), cond_fn=T.wgrad_wino_Aw)
            same = _wgrad(hip, x, np.zeros_like(dfm), cout, 3, 1, accumulate=1, init=got)
            assert np.array_equal(same[0], got[0]) and np.array_equal(same[1], got[1]), name + ": accumulating a zero gradient changed the buffer"


def test_weight_gradient_at_degenerate_sizes(hip):
    """read_conv_wgrad at the sizes of a 16-pixel crop's coarse levels.  With the Winograd-domain knob on, C -> C 3x3 / stride-1 layers
    (32, 128, 256) at 2 x 2, 1 x 1, 2 x 6 and 4 x 12: read_conv_wgrad_family sends an image of fewer than four rows to the direct kernels
    (family 0: it has no whole 4 x 4 tile) and 4 x 12 to the Winograd-domain kernels (family 4); each row is held to the bound of the
    family that the route names — class (a), a constant, and impulses of d[f|m] at every pixel of the 2 x 2.  With the knob off, one
    stride-1, one k3 / stride-2 and one k4 / stride-2 layer at 1 x 1 and 2 x 2 (k4 at 1 x 1 has an empty output: left out), class (a)
    and every impulse read back exactly."""
    rng = np.random.default_rng(131)
    knob = _knob(hip)
    try:
        _knob(hip, 1)
        for c in (32, 128, 256):
            for (H, W) in ((2, 2), (1, 1), (2, 6), (4, 12)):
                fam = hip.read_conv_wgrad_family(c, 3, 1, H, W)
                assert fam == (4 if H >= 4 else 0), (c, H, W, fam)
                wino = fam == 4
                bound = (lambda Aw, prev: T.wgrad_wino_bound(Aw, c, c, H, W)) if wino else (lambda A, prev: T.wgrad_direct_bound(A, c, c, 3, H, W))
                kw = dict(cond_fn=T.wgrad_wino_Aw) if wino else {}
                rows = [(cls, "", _wgrad_inputs(cls, c, c, H, W, H, W, rng)) for cls in ("a", "const")]
                if (H, W) == (2, 2):
                    xi = T.small_integers((H, W, c), rng)
                    for (py, px) in ((0, 0), (0, 1), (1, 0), (1, 1)):
                        d = np.zeros((H, W, c), f32)
                        d[py, px] = 1.0
                        rows.append(("impulse", f" impulse {py},{px}", (xi, d, d)))
                for cls, tag, (x, df, dm) in rows:
                    got = _wgrad(hip, x, _dfm(df, dm, c), c, 3, 1)
                    _judge_wgrad("wgrad_wino" if wino else "wgrad", "a" if cls == "a" else "c", f"{c}->{c} {H}x{W}{tag} [family {fam}]", got, x, (df, dm), 3, 1,
                                 bound, **kw)
        _knob(hip, 0)
        for (cin, cout, k, stride) in ((48, 20, 3, 1), (32, 64, 3, 2), (64, 32, 4, 2)):
            for (H, W) in ((1, 1), (2, 2)):
                oh, ow = T.out_hw(k, stride, H, W)
                if oh == 0:
                    continue
                assert hip.read_conv_wgrad_family(cin, k, stride, H, W) == 0
                name = f"{cin}->{cout} k{k} s{stride} {H}x{W}"
                x, df, dm = _wgrad_inputs("a", cin, cout, H, W, oh, ow, rng)
                got = _wgrad(hip, x, _dfm(df, dm, cout), cout, k, stride)
                _judge_wgrad("wgrad", "a", name, got, x, (df, dm), k, stride, lambda A, prev: T.wgrad_direct_bound(A, cin, cout, k, oh, ow))
                xi = T.small_integers((H, W, cin), rng)
                pad = (k - 1) // 2
                xp = np.zeros((H + 2 * pad + k, W + 2 * pad + k, cin), f32)
                xp[pad:pad + H, pad:pad + W] = xi
                for py in range(oh):
                    for px in range(ow):
                        for amp in (1.0, 2.0 ** -10):
                            d = np.zeros((oh, ow, cout), f32)
                            d[py, px] = amp
                            got = _wgrad(hip, xi, _dfm(d, d, cout), cout, k, stride)
                            want = np.broadcast_to((f32(amp) * xp[py * stride:py * stride + k, px * stride:px * stride + k]).transpose(2, 0, 1)[None], got[0].shape)
                            assert np.array_equal(got[0], want) and np.array_equal(got[1], want), f"{name}: impulse at {(py, px)} x {amp}"
                print("TACC| %-12s | c | %-46s | %d impulse positions x 2 amplitudes read back exactly" % ("wgrad", name, oh * ow))
    finally:
        _knob(hip, knob)
    finish()


# ------------------------------------------------------------------------------------------ generic input gradient
def test_generic_input_gradient(hip):
    """read_conv_dgrad_generic: (k3, s2) and (k4, s2) at odd sizes."""
    _generic_dgrad_rows(hip, np.random.default_rng(34), ((9, 13), (7, 7)))
    finish()


def test_generic_input_gradient_at_degenerate_sizes(hip):
    """... at 2 x 2 (output 1 x 1) and 3 x 1 (k3: output 2 x 1; k4: 1 x 0, an empty d[f|m]: left out)."""
    _generic_dgrad_rows(hip, np.random.default_rng(134), ((2, 2), (3, 1)))
    finish()


def _generic_dgrad_rows(hip, rng, sizes):
    st = _lib.stream_ptr()
    for k in (3, 4):
        for (H, W) in sizes:
            if 0 in T.out_hw(k, 2, H, W):
                continue
            for cin in (8, 32):
                for cout in (3, 40):
                    for cls in "abc":
                        oh, ow = T.out_hw(k, 2, H, W)
                        sd = T.scales_b(2 * cout, rng) if cls == "b" else np.ones(2 * cout)
                        sw = T.scales_b(cin, rng) if cls == "b" else np.ones(cin)
                        w = [(rng.standard_normal((cout, cin, k, k)) * sw[None, :, None, None] / np.sqrt(cin * k * k)).astype(f32) for _ in range(2)]
                        d = (rng.standard_normal((oh, ow, 2 * cout)) * sd).astype(f32)
                        if cls == "c":                               # an impulse of d[f|m] over integer weights: dx is read back exactly
                            w = [T.small_integers((cout, cin, k, k), rng) for _ in range(2)]
                            d[:] = 0
                            d[oh - 1, ow // 2, cout - 1], d[0, 0, cout] = 1.0, 2.0 ** -10
                        dfm = _dfm(d[:, :, :cout], d[:, :, cout:], cout)
                        ws = torch.empty(hip.read_conv_dgrad_generic_floats(cin, cout, k), dtype=torch.float32, device="cuda")
                        dx = torch.full((H, W, cin), 7.0, device="cuda")
                        dfm_d, wf_d, wm_d = _dev(dfm), _dev(w[0]), _dev(w[1])
                        _lib.check(hip.read_conv_dgrad_generic(dfm_d.data_ptr(), oh, ow, cin, cout, k, 2, wf_d.data_ptr(), wm_d.data_ptr(), ws.data_ptr(),
                                                               H, W, dx.data_ptr(), st))
                        got = _host(dx)
                        ref, cond = T.dgrad_ref(dfm, cout, w[0], w[1], k, 2, H, W)
                        name = f"{cin}->{cout} k{k} s2 {H}x{W}"
                        judge("dgrad_generic", cls, name, got, ref, cond, T.dgrad_bound(cond, cout, k, 2),
                              {"torch": T.dgrad_torch32(dfm, cout, w[0], w[1], k, 2, H, W), "seq": T.dgrad_seq32(dfm, cout, w[0], w[1], k, 2, H, W)})
                        if cls == "c":
                            assert np.array_equal(got.astype(np.float64), ref), name + ": the impulse's weights are not read back exactly"


# ------------------------------------------------------------------------------------------ input gradient through the convolution kernels
_METHOD = {"s1": "conv", "dilated": "dilated", "poly": "poly"}


def _conv_dgrad(dfm_h, wf_h, wm_h, route, H, W, branch):
    """The three non-generic methods of read_amd.train.GatedConvFn.backward, driven with a chosen d[f|m] through the helper the backward
    pass itself calls (train._dgrad): "s1" stride 1, "dilated" 3x3 / stride 2 as the stride-1 dgrad of the zero-dilated d[f|m], "poly" one
    3x3 / stride-1 dgrad per pixel parity.  The case names the method; the route function must offer it for this layer (with the
    polyphase method switched off for "dilated", which it otherwise precedes).  -> dx (H, W, cin) on the host."""
    from read_amd import train
    assert train.dgrad_method(route, H, W, polyphase=branch != "dilated") == _METHOD[branch], (branch, route)
    dfm, wf, wm = _dev(dfm_h), _dev(wf_h), _dev(wm_h)
    dx = torch.full((H, W, route.cin), 7.0, device="cuda")
    assert train._dgrad(_METHOD[branch], route, dfm, H, W, wf, wm, out=dx) is dx
    return _host(dx)


def _conv_family(route, branch):
    """The kernel family of the fragments the method reads, as the route function decides it."""
    kind = route.poly if branch == "poly" else route.dgrad
    return {_lib.PACK_DIRECT: "direct", _lib.PACK_WINO: "w2", _lib.PACK_W4: "w4"}[kind]


def test_input_gradient_through_the_convolution_kernels(hip):
    """Stride 1 (k1, k3; 2 pad8(Cout) = 16, 48, 80, 112, 128 virtual input channels), dilated 3x3 / stride 2, polyphase k3 / k4: the fp32
    convolution kernels in linear mode over d[f|m] with flipped, transposed weights.  cond = sum |d| |w|; the Winograd launches are held
    to the transformed-domain term A_w (asserted), E against cond is printed as E(A)."""
    cases = [("s1", k, 1, cout, hw) for k in (1, 3) for cout in (3, 20, 40, 56, 64) for hw in ((9, 21), (12, 20))]
    cases += [(br, k, 2, cout, (8, 12)) for (br, k) in (("dilated", 3), ("poly", 3), ("poly", 4)) for cout in (3, 40)]
    _conv_dgrad_rows(np.random.default_rng(37), cases)
    finish()


def test_input_gradient_through_the_convolution_kernels_at_degenerate_sizes(hip):
    """... "s1" at 1 x 1, 2 x 2 and 2 x 6; "dilated" and "poly" (k3, k4) at inputs of 2 x 2 (d[f|m] is one pixel: three of the four
    parity planes of the polyphase form are empty or one pixel) and 4 x 4."""
    cases = [("s1", k, 1, cout, hw) for k in (1, 3) for cout in (3, 40, 64) for hw in ((1, 1), (2, 2), (2, 6))]
    cases += [(br, k, 2, cout, hw) for (br, k) in (("dilated", 3), ("poly", 3), ("poly", 4)) for cout in (3, 40) for hw in ((2, 2), (4, 4))]
    _conv_dgrad_rows(np.random.default_rng(137), cases)
    finish()


def _conv_dgrad_rows(rng, cases):
    from read_amd import train
    cin = 32
    for branch, k, stride, cout, (H, W) in cases:
        for cls in "ab":
            oh, ow = T.out_hw(k, stride, H, W)
            sd = T.scales_b(2 * cout, rng) if cls == "b" else np.ones(2 * cout)
            sw = T.scales_b(cin, rng) if cls == "b" else np.ones(cin)
            w = [(rng.standard_normal((cout, cin, k, k)) * sw[None, :, None, None] / np.sqrt(cin * k * k)).astype(f32) for _ in range(2)]
            d = (rng.standard_normal((oh, ow, 2 * cout)) * sd).astype(f32)
            dfm = _dfm(d[:, :, :cout], d[:, :, cout:], cout)
            route = train.layer_route(cin, cout, k, stride)
            got = _conv_dgrad(dfm, w[0], w[1], route, H, W, branch)
            ref, cond = T.dgrad_ref(dfm, cout, w[0], w[1], k, stride, H, W)
            fam = _conv_family(route, branch)
            name = f"{branch} {cin}->{cout} k{k} s{stride} {H}x{W} [{fam}]"
            yard = {"torch": T.dgrad_torch32(dfm, cout, w[0], w[1], k, stride, H, W), "seq": T.dgrad_seq32(dfm, cout, w[0], w[1], k, stride, H, W)}
            if fam == "direct":
                judge("dgrad_conv", cls, name, got, ref, cond, T.conv_dgrad_bound(dfm, T.virtual_weights(w[0], w[1]), cond, ref, fam), yard)
                continue
            # the virtual stride-1 3x3 layer(s) the Winograd kernel sees
            bound, Aw = np.zeros_like(ref), np.zeros_like(ref)
            if branch == "poly":
                pf, pm = T.poly_pseudo_weights(w[0], k), T.poly_pseudo_weights(w[1], k)
                for par in range(4):
                    sl = (slice(par >> 1, None, 2), slice(par & 1, None, 2))
                    bound[sl], Aw[sl] = T.conv_dgrad_bound(dfm, T.virtual_weights(pf[par], pm[par]), None, ref[sl], fam)
            else:
                d_in = dfm
                if branch == "dilated":
                    d_in = np.zeros((H, W, dfm.shape[2]), f32)
                    d_in[::2, ::2] = dfm
                bound, Aw = T.conv_dgrad_bound(d_in, T.virtual_weights(w[0], w[1]), None, ref, fam)
            judge("dgrad_conv", cls, name, got, ref, Aw, bound, yard, extra=" E(A) max %.2f rms %.3f |" % T.stats(np.abs(got - ref), cond))


# ------------------------------------------------------------------------------------------ bilinear x 4
def test_bilinear_up4_forward_and_backward(hip):
    """read_bilinear_up4_blocks, read_bilinear_up4_backward.  No R_seq: the only sums are the backward's <= 36 terms per thread."""
    _up4_rows(hip, np.random.default_rng(35), ((1, 1, 0, 0), (2, 5, 0, 0), (5, 3, 0, 0), (10, 3, 5, 3)))
    finish()


def test_bilinear_up4_on_stacked_one_and_four_pixel_items(hip):
    """... three stacked items of 1 x 1 and of 2 x 2 valid pixels, one separator row each (what a batch of three 16 x 16 crops gives
    feat_extract.7 and feat_extract.3)."""
    _up4_rows(hip, np.random.default_rng(135), ((6, 1, 2, 1), (9, 2, 3, 2)))
    finish()


def _up4_rows(hip, rng, geometries):
    st = _lib.stream_ptr()
    for (H, W, bh, vh) in geometries:
        for C in (4, 8):
            for cls in "ab":
                sc = T.scales_b(C, rng) if cls == "b" else np.ones(C)
                x = (rng.standard_normal((H, W, C)) * sc).astype(f32)
                d = (rng.standard_normal((4 * H, 4 * W, C)) * sc).astype(f32)
                name = f"{H}x{W} C {C} block {bh}/{vh}"
                out = torch.full((4 * H, 4 * W, C), 7.0, device="cuda")
                x_d, d_d = _dev(x), _dev(d)
                _lib.check(hip.read_bilinear_up4_blocks(x_d.data_ptr(), H, W, C, out.data_ptr(), bh, vh, st))
                ref, cond, bound = T.up4_forward_ref(x, bh, vh)
                got = _host(out)
                judge("up4_fwd", cls, name, got, ref, cond, bound, {"torch": T.up4_torch32(x, H, W, bh, vh, False)})
                din = torch.full((H, W, C), 7.0, device="cuda")
                _lib.check(hip.read_bilinear_up4_backward(d_d.data_ptr(), H, W, C, din.data_ptr(), bh, vh, st))
                refb, condb, boundb = T.up4_backward_ref(d, H, W, bh, vh)
                gotb = _host(din)
                judge("up4_bwd", cls, name, gotb, refb, condb, boundb, {"torch": T.up4_torch32(d, H, W, bh, vh, True)})
                if bh:
                    assert not got.reshape(H // bh, 4 * bh, -1)[:, 4 * vh:].any() and not gotb.reshape(H // bh, bh, -1)[:, vh:].any(), name + ": separator rows"


# ------------------------------------------------------------------------------------------ Huber
def test_huber_loss_and_gradient(hip):
    """read_huber_loss: the per-element gradient and the summed loss."""
    rng = np.random.default_rng(36)
    st = _lib.stream_ptr()
    for n in (1, 3, 255, 257, 1000):
        for cls in "ab":
            t = (rng.standard_normal(n) * (2.0 ** rng.uniform(-8, 6, n) if cls == "b" else 1.0)).astype(f32)
            o = (t + rng.standard_normal(n) * 1.5).astype(f32)
            edge = np.array([0.0, 1.0, -1.0, np.nextafter(f32(1), f32(0)), np.nextafter(f32(1), f32(2)), -np.nextafter(f32(1), f32(0)), -np.nextafter(f32(1), f32(2))], f32)
            m = min(n, len(edge))
            t[:m] = f32(0.25)                                        # 0.25 + d is exact for these d: the difference is exactly the edge value
            o[:m] = f32(0.25) + edge[:m]
            scale = 1.0 / n
            o_d, t_d = _dev(o), _dev(t)
            loss, grad = torch.full((1,), 7.0, device="cuda"), torch.full((n,), 7.0, device="cuda")
            _lib.check(hip.read_huber_loss(o_d.data_ptr(), t_d.data_ptr(), n, scale, loss.data_ptr(), grad.data_ptr(), st))
            ref = T.huber_ref(o, t, f32(scale))
            ot = torch.from_numpy(o).requires_grad_(True)
            lt = F.huber_loss(ot, torch.from_numpy(t), reduction="sum")
            (lt * f32(scale)).backward()
            d32 = o - t
            l32 = np.where(np.abs(d32) < 1, (f32(0.5) * d32 * d32).astype(f32), np.abs(d32) - f32(0.5)).astype(f32)
            g32 = (f32(scale) * np.where(np.abs(d32) < 1, d32, np.sign(d32))).astype(f32)
            judge("huber grad", cls, f"n {n}", _host(grad), ref["grad"], np.abs(ref["grad"]), ref["bound_grad"], {"torch": ot.grad.numpy(), "seq": g32})
            judge("huber loss", cls, f"n {n}", _host(loss), np.array([ref["loss_sum"]]), np.array([ref["cond_loss"]]), np.array([ref["bound_loss"]]),
                  {"torch": np.array([float(lt.detach())]), "seq": np.add.accumulate(l32, dtype=f32)[-1:]})
    finish()


# ------------------------------------------------------------------------------------------ RMSprop over the touched rows
def _rms_schedule(N, rng):
    """Six steps of pixel ids: runs of 1, 2, 512, 513 (the LONG_RUN boundary) and 5000 pairs, ids -1 and N; 70 runs of 513 (more than the
    MAX_LONG = 64 slots: the rest are summed in the head thread); rows left alone for 1 step (row 101) and for 50 (row 100)."""
    run = lambda row, n: np.full(n, row, np.int64)                                                  # noqa: E731
    s1 = np.concatenate([run(10, 1), run(11, 2), run(12, 512), run(13, 513), run(0, 5000), run(-1, 3), run(N, 2), run(100, 4), run(101, 1), np.arange(300, 340)])
    s2 = np.concatenate([run(r, 513) for r in range(200, 270)] + [run(100, 2), run(N, 1)])
    s3 = np.concatenate([run(101, 3), rng.integers(0, N, 700)])
    s4 = rng.integers(-1, N + 1, 900)
    s5 = np.concatenate([run(0, 600), rng.integers(0, N, 200)])
    s6 = np.concatenate([run(100, 5), run(13, 513), rng.integers(0, N, 50)])
    return [rng.permutation(s) for s in (s1, s2, s3, s4, s5, s6)]


@pytest.mark.parametrize("C", [1, 8, 16])
def test_rmsprop_sorted_and_sparse_follow_the_dense_float64_trajectory(hip, C):
    """read_rmsprop_sorted and read_rmsprop_sparse against dense float64 RMSprop (alpha 0.99, eps 1e-8) over 6 steps, the last one after 50
    idle steps (the lazy powf decay)."""
    N, lr = 600, np.float32(0.05)
    alpha, eps = np.float32(0.99), np.float32(1e-8)
    rng = np.random.default_rng([41, C])
    st = _lib.stream_ptr()
    rows0 = rng.standard_normal((N, C)).astype(f32)
    sched = _rms_schedule(N, rng)
    grads = [(rng.standard_normal((len(ids), C)) * 2.0 ** rng.uniform(-6, 2, (len(ids), 1))).astype(f32) for ids in sched]
    for kernel in ("sorted", "sparse"):
        traj = T.RmspropTrajectory(rows0, float(alpha), float(eps))
        rows, sq = _dev(rows0), torch.zeros((N, C), device="cuda")
        stamp = torch.zeros(N, dtype=torch.int32, device="cuda")
        scratch = torch.zeros(int(hip.read_rmsprop_sorted_scratch_ints()), dtype=torch.int32, device="cuda")
        p_t = torch.nn.Parameter(torch.from_numpy(rows0.copy()))
        opt = torch.optim.RMSprop([p_t], lr=float(lr), alpha=float(alpha), eps=float(eps))
        p_s, sq_s = rows0.copy(), np.zeros((N, C), f32)
        step = 0
        for k, (ids, g) in enumerate(zip(sched, grads)):
            idle = 50 if k == 5 else 0
            if idle:
                traj.idle(idle)
                for _ in range(idle):
                    p_t.grad = torch.zeros_like(p_t)
                    opt.step()
                    sq_s = (alpha * sq_s).astype(f32)
            step += idle + 1
            ok = (ids >= 0) & (ids < N)
            table = np.zeros((N, C), f32)
            for i in np.nonzero(ok)[0]:                              # fp32, the pairs one after the other
                table[ids[i]] = table[ids[i]] + g[i]
            if kernel == "sorted":
                order = np.argsort(ids, kind="stable")
                s_ids, perm, g_d = _dev(ids[order], torch.int32), _dev(order, torch.int64), _dev(g)
                _lib.check(hip.read_rmsprop_sorted(rows.data_ptr(), sq.data_ptr(), stamp.data_ptr(), C, N, s_ids.data_ptr(), perm.data_ptr(), g_d.data_ptr(),
                                                   len(ids), step, float(lr), float(alpha), float(eps), scratch.data_ptr(), st))
                touched = traj.apply(ids, g, float(lr))
            else:
                tab_d, ids_d = _dev(table), _dev(ids, torch.int32)
                _lib.check(hip.read_rmsprop_sparse(rows.data_ptr(), sq.data_ptr(), tab_d.data_ptr(), stamp.data_ptr(), C, N, ids_d.data_ptr(), len(ids), step,
                                                   float(lr), float(alpha), float(eps), st))
                uniq = np.unique(ids[ok])
                touched = traj.apply(uniq, table[uniq], float(lr))
                assert not _host(tab_d)[uniq].any(), "read_rmsprop_sparse left gradient rows of touched ids behind"
            p_t.grad = torch.from_numpy(table.copy())
            opt.step()
            sq_s = ((alpha * sq_s).astype(f32) + ((f32(1) - alpha) * table * table).astype(f32)).astype(f32)
            p_s = (p_s - ((lr * table).astype(f32) / (np.sqrt(sq_s) + eps).astype(f32)).astype(f32)).astype(f32)
            name = f"C {C} step {step} ({int(touched.sum())} rows, {len(ids)} pairs)"
            judge("rmsprop " + kernel, "a", name + " rows", _host(rows), traj.p, traj.cond_p, traj.e_p, {"torch": p_t.detach().numpy(), "seq": p_s})
            t = touched
            judge("rmsprop " + kernel, "a", name + " sq", _host(sq)[t], traj.sq[t], traj.cond_v[t], traj.e_v[t] + T.TINY, {"seq": sq_s[t]})
            assert np.array_equal(_host(stamp)[t], np.full(int(t.sum()), step)), name + ": stamps of the touched rows"
        if kernel == "sorted":                                        # ids outside 0 .. N - 1 change nothing
            before = [_host(x).copy() for x in (rows, sq, stamp)]
            bad = np.concatenate([np.full(5, -1), np.full(600, N)]).astype(np.int64)
            g_d, bad_d, perm_d = _dev(rng.standard_normal((len(bad), C)).astype(f32)), _dev(bad, torch.int32), _dev(np.arange(len(bad)), torch.int64)
            _lib.check(hip.read_rmsprop_sorted(rows.data_ptr(), sq.data_ptr(), stamp.data_ptr(), C, N, bad_d.data_ptr(), perm_d.data_ptr(), g_d.data_ptr(),
                                               len(bad), step + 1, float(lr), float(alpha), float(eps), scratch.data_ptr(), st))
            for b, x in zip(before, (rows, sq, stamp)):
                assert np.array_equal(b, _host(x)), "out-of-range ids changed the optimizer state"
    finish()
