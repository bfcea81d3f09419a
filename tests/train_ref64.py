"""float64 references of the training kernels (read_amd/csrc/train.hip), the error measure in units of fp32 round-off, the derived
error bounds with the roundings they count, two fp32 yardsticks, and the inputs on which these kernels can go wrong.  Plain NumPy and
torch-float64 on the CPU; nothing from read_amd or oracle/ takes part in the arithmetic.  u, EPS, TINY, `gated_bound` and the
generators come from tests/conv_ref64.py.  tests/test_train_accuracy_cpu.py runs NumPy fp32 restatements of the kernels through the
measure, tests/test_gpu_train_accuracy.py the kernels themselves.  The forward's linear launches on the fp32 convolution kernels
(`conv_forward_bound`, derivation in front of it) are run by tests/test_gpu_train_forward_accuracy.py.

LAYOUT.  As the device sees it: pixel-major, fm (P, 2 C) = [f | m], dy / y / g (P, C), d[f|m] (P, 2 Cp) with Cp = C padded to 8; a
stacked batch is `block_h` rows per item of which the first `valid_h` are valid, the rest separator rows (`valid_rows`).

THE MEASURE.  E = |got - ref| / (u cond), u = 2^-24, cond = the reference's formula with every summand replaced by its absolute value
(a product has cond = |product|).  Where cond = 0 no product reaches the output and the kernel must return the exact constant.

THE DERIVED BOUNDS (absolute, per element).  Roundings are counted without fused multiply-adds (hipcc contracts a * b + c: a contraction
only removes a rounding).  FLUSH = 2^-126: v_exp_f32 / v_rcp_f32 may flush a result below the normal range.

Gate, shared by all modes (gate_forward_kernel :261-267, gate_backward_kernel :310-321, gate_backward4_kernel :387-397):
  s = v_rcp_f32(1 + v_exp_f32(-m log2e)): the rounded constant and the product 2 u |m| in the exponent, exp 1 ulp = 2 u, the add u, rcp 2 u
      d_s   <= sigma (1 - sigma) u (3 |m| + 2) + 3 u sigma + FLUSH                       (conv_ref64.gated_bound's d_sigma with d_m = 0)
      1 - s : exact for s >= 1/2 (Sterbenz), one rounding below:   d_1ms <= d_s + u (1 - sigma)
  a = f > 0 ? f : v_exp_f32(f log2e) - 1:   d_a <= [f <= 0] (u (e^f (2 |f| + 2) + |a|) + FLUSH)      (the exp - 1 cancellation: u |a|)
  da = f > 0 ? 1 : a + 1:                   d_da <= [f <= 0] (d_a + u e^f)
  g = a s:                                  d_g <= |a| d_s + sigma d_a + u |g|
Gate forward  y = (a s) sc + sh (+ residual): conv_ref64.gated_bound with d_f = d_m = 0, A_f = |f|, A_m = |m| — the params block is
  produced by pack_params_body (:40-44) with the same expressions as the host packer.
Gate backward, eval BatchNorm (mode 0): gs = dy sc (sc: 3.5 u as in gated_bound; the product 1), df = (gs s) da, dm = ((gs a) s)(1 - s)
      d_df <= 6.5 u |df| + |gs| (da d_s + sigma d_da)
      d_dm <= 7.5 u |dm| + |gs| (sigma (1 - sigma) d_a + |a| (1 - sigma) d_s + |a| sigma d_1ms)
  cond_df = |dy| S sigma (f <= 0 ? e^f + 2 : 1),  cond_dm = |dy| S (f <= 0 ? e^f + 1 : |f|) sigma (1 + sigma).
The four sums (:306-339 / :394-417): a thread adds its pixels in fp32 (ceil(span / (blocks ROWS)) of them), thread 0..CW-1 adds the
  ROWS LDS slots, the workgroups meet in fp32 atomics: a value passes through at most
      depth = ceil(span / (blocks ROWS)) + ROWS + blocks       additions (`sum_depth`; blocks, ROWS from read_gate_backward :1302-1313)
      d_sum <= sum_i d_term_i + depth u sum_i |term_i|
  the terms of S3 = sum dy g carry d_term = |dy| (d_g + u |g|).
bn_grads_kernel (:427-431)  dgamma = (S3 - mean S2) rstd, rstd = 1 / sqrtf(var + eps): 3.5 u (add, sqrt, divide, eps as a float):
      d_dgamma <= r (d_S3 + |mean| d_S2 + u |mean S2| + u |S3 - mean S2|) + 4.5 u |dgamma|
  cond_dgamma = r sum |dy| |g - mean|   (`form` "centered", what torch's formulation costs), or with the term the kernel's formulation
  adds, r (sum |dy| |g| + |mean| sum |dy|)  (`form` "kernel").  The bound above is of the second kind: depth u r |mean| sum |dy| is its
  leading term for |mean| >> std.
Batch-statistics forward (bn_stats_kernel in fp64 :489-503, bn_finalize_kernel :517-527, bn_apply_kernel :541):
  mean, var = E g^2 - mean^2 in fp64: d_var64 <= 2^-40 E g^2 (fp64 sums of < 2^12 terms and the cancellation, generously);
  stat = (float) of both: u |mean|, u var + d_var64;  sc = gamma / sqrtf(vf + eps): 3.5 u + the variance's rounding, <= 5 u S + dS_var,
  dS_var = S d_var64 / (2 (var + eps));  sh = beta - mf sc: 7 u |mean| S + u |T| + |mean| dS_var;  y = g sc + sh:
      d_y <= u (7 S |g| + 7 S |mean| + |T| + |y|) + (|g| + |mean|) dS_var        cond_y = S |g| + S |mean| + |beta|
  (cond in the kernel's formulation; the centered form S |g - mean| + |beta| is what torch's costs: E against it is E(xhat).)
  running buffers rm = (1 - mom) rm + mom mf: 1 - mom, two products, one add and the cast: 5 u (|(1 - mom) rm| + |mom mean|) per group.
Batch-statistics backward (bn_bwd_coeff_kernel :554-559, mode 2 :315 / :391): with e2 = d_S2, e3 = d_S3 as above, n = count,
      dgamma as above: e_dg;   A = gamma r: 4.5 u;   Cc = ((-A r) dgamma) / n: 11 u |Cc| + |A| r e_dg / n =: e_C
      B = (-A dbeta) / n - Cc mean:  e_B = 6.5 u |A dbeta / n| + |A| e2 / n + |mean| e_C + u |Cc mean| + u |B|
      gs = A dy + B + Cc g:          e_gs = 5.5 u |A dy| + u |A dy + B| + e_B + |g| e_C + |Cc| d_g + u |Cc g| + u |gs|
      d_df <= 2 u |df| + e_gs sigma da + |gs| (da d_s + sigma d_da),   d_dm likewise with 3 u
  cond_dg = |A| (|dy| + mean|dy| + |xhat| mean(|dy| |xhat|)) (the centred formulation); |mean| e_C + |g| e_C is what the kernel's
  formulation adds when |mean| >> std.
Direct wgrad (wgrad_mfma_kernel :715-722, wgrad_reduce_kernel :753-762): v_mfma_f32_32x32x2_f32 adds two products to the accumulator:
  a split of `rows_per_split` rows and ceil(outW / 2) pixel pairs is a chain of N = 2 rows_per_split ceil(outW / 2) terms, each product
  rounded at most once; the splits are summed in fours, then sequentially: at most `splits` additions; accumulate adds one rounding:
      d_dW <= u ((N + 1 + splits) A + [accumulate] (A + |previous|)),   A = sum_pixels |x| |d|      (`wgrad_plan` restates :1481-1502)
Winograd-domain wgrad (wg4_bt6 :789-799, wg4_a4 :801-811, the MFMA loop :911-915, wgrad_wino4_sum_kernel :935-944,
  wgrad_wino4_reduce_kernel :966-982): each transform pass is at most two roundings deep (an fma over an fma; an add of two fmas): 4 u on
  V against |B^T| |d| |B|, 4 u on M against |A| |dY| |A^T|; the product 1; a split is a chain of N = 8 n_it terms (8 tiles per iteration,
  padded tiles are zeros); the sum over splits at most `splits`; the G^T . G step per pass: the sum / difference, the rounded constant
  1/6, 1/12 or 1/24, the product, two additions: 5 u per pass against |G^T| |U| |G|:
      d_dW <= u (4 + 4 + 1 + N + splits + 10) A_w + [accumulate] u (A_w + |previous|)
  A_w = |G^T| [sum_tiles (|B^T| |d| |B|) . (|A| |dY| |A^T|)] |G|.  No bound in terms of A exists; E against A is printed as E(A).
Generic dgrad (dgrad_generic_kernel :578-597): one thread adds ceil(k / stride)^2 taps x 2 Cp products sequentially:
      d_dx <= u (ceil(k / stride)^2 2 Cp + 1) cond,   cond = sum |d| |w|
Bilinear x4 (bilinear_up4_blocks_kernel :1026, bilinear_up4_backward_kernel :1051-1068): the weights are multiples of 1/8, exact, and so
  are their products; forward: product, product, add, product, add: 5 u cond; backward: at most 36 terms in sequence: 37 u cond.
Huber (huber_kernel :1086-1097): d = out - target one rounding, grad = scale d or +-scale: 2 u |grad|;  l = (0.5 d) d or |d| - 0.5:
      d_l <= u (2 |d| min(|d|, 1) + 2 l);  the sum: a thread's ceil(n / (256 blocks)) terms, the 8-level LDS tree, `blocks` atomics.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests import conv_ref64 as R64
from tests.conv_ref64 import EPS, SECOND_ORDER, TINY, U
from tests.test_train_identities import AT, BT, G

FLUSH = 2.0 ** -126
LOG2E32 = np.float32(1.44269504088896341)


def pad8(c):
    return (c + 7) // 8 * 8


def valid_rows(P, W, block_h, valid_h):
    """-> (P,) bool: pixel p is not in a separator row (separator_row, train.hip:243)."""
    rows = np.arange(P) // W
    return np.ones(P, bool) if block_h <= 0 else (rows % block_h) < valid_h


def group_of(P, W, block_h, groups):
    return np.zeros(P, np.int64) if groups == 1 else (np.arange(P) // W) // block_h


def grid_for(items, per_block=256, cap=256 * 16):
    return int(min(max((items + per_block - 1) // per_block, 1), cap))


def stats(err, den):
    """(E_max, E_rms) of err / (u den); an error where den = 0 counts as infinite."""
    return R64._stats(np.asarray(err, np.float64), np.asarray(den, np.float64))


def worst(err, bound):
    """max err / bound over all elements; 0 / 0 = 0, x / 0 = inf."""
    err, bound = np.broadcast_arrays(np.asarray(err, np.float64), np.asarray(bound, np.float64))
    q = np.zeros(err.shape)
    nz = bound > 0
    q[nz] = err[nz] / bound[nz]
    q[~nz & (err > 0)] = np.inf
    return float(q.max()) if q.size else 0.0


# ------------------------------------------------------------------------------------------ gate
class Gate:
    """float64 pieces of the gate at every (pixel, channel), and the error bounds of their fp32 evaluation (module docstring)."""

    def __init__(self, fm, C, elu):
        f, m = fm[:, :C].astype(np.float64), fm[:, C:2 * C].astype(np.float64)
        self.f, self.m, self.elu = f, m, elu
        with np.errstate(over="ignore", under="ignore"):
            self.sig = 1.0 / (1.0 + np.exp(-m))
            self.oms = 1.0 / (1.0 + np.exp(m))                       # 1 - sigma without the cancellation
            ef = np.exp(np.minimum(f, 0.0))
            self.a = np.where(f > 0, f, np.expm1(np.minimum(f, 0.0))) if elu else f
        self.neg = (f <= 0) if elu else np.zeros(f.shape, bool)
        self.da = np.where(self.neg, ef, 1.0)
        self.g = self.a * self.sig
        self.d_s = self.sig * self.oms * U * (3 * np.abs(m) + 2) + 3 * U * self.sig + FLUSH
        self.d_oms = self.d_s + U * self.oms
        self.d_a = self.neg * (U * (ef * (2 * np.abs(f) + 2) + np.abs(self.a)) + FLUSH)
        self.d_da = self.neg * (self.d_a + U * ef)
        self.d_g = np.abs(self.a) * self.d_s + self.sig * self.d_a + U * np.abs(self.g)
        self.a_abs = np.where(self.neg, ef + 1.0, np.abs(f))
        self.da_abs = np.where(self.neg, ef + 2.0, 1.0)

    def through(self, gs, e_gs, n_f, n_m):
        """df = gs s da, dm = gs a s (1 - s) and their bounds from gs's own bound e_gs; n_f, n_m: relative roundings u |df|, u |dm|."""
        s, a, da, oms = self.sig, self.a, self.da, self.oms
        df, dm = gs * s * da, gs * a * s * oms
        ags = np.abs(gs)
        b_f = n_f * U * np.abs(df) + e_gs * s * da + ags * (da * self.d_s + s * self.d_da)
        b_m = n_m * U * np.abs(dm) + e_gs * np.abs(a) * s * oms + ags * (s * oms * self.d_a + np.abs(a) * (oms * self.d_s + s * self.d_oms))
        return df, dm, SECOND_ORDER * b_f + TINY, SECOND_ORDER * b_m + TINY


def bn_scale(gamma, var):
    return np.asarray(gamma, np.float64) / np.sqrt(np.asarray(var, np.float64) + EPS)


def gate_forward_ref(fm, C, L, elu, residual, W, block_h, valid_h):
    """read_gate_forward.  L: gamma, beta, mean, var (float32).  -> (y, cond B, bound), (P, C) float64; separator rows 0 / 0 / 0."""
    P = fm.shape[0]
    gt = Gate(fm, C, elu)
    r = R64.Ref()
    r.f, r.m, r.elu, r.g, r.sig, r.dact = gt.f, gt.m, elu, gt.a, gt.sig, gt.da
    r.Af, r.Am = np.abs(gt.f), np.abs(gt.m)
    Ss = bn_scale(L["gamma"], L["var"])[None]
    r.S = np.abs(Ss)
    r.T = np.asarray(L["beta"], np.float64)[None] - np.asarray(L["mean"], np.float64)[None] * Ss
    r.mean_S = np.abs(np.asarray(L["mean"], np.float64))[None] * r.S
    r.res = np.zeros_like(gt.f) if residual is None else residual.astype(np.float64)
    r.y = Ss * gt.a * gt.sig + r.T + r.res
    cond = r.S * (np.abs(gt.da) * gt.sig * r.Af + np.abs(gt.a) * gt.sig * gt.oms * r.Am)
    B = cond + np.abs(r.y)
    bound = R64.gated_bound(r, 0.0, 0.0) + FLUSH * r.S * (1 + np.abs(gt.a))
    v = valid_rows(P, W, block_h, valid_h)[:, None]
    return np.where(v, r.y, 0.0), np.where(v, B, 0.0), np.where(v, bound, 0.0), np.where(v, cond, 0.0)


def gate_bwd_geometry(span, C):
    """(blocks, ROWS) of the gate-backward launch over `span` pixels (read_gate_backward / read_gate_backward_bn)."""
    if C % 32 == 0 and C <= 256:
        return grid_for(span, 1024 // C, 2048), 256 // (C // 4)
    if pad8(C) <= 8:
        return grid_for(span, 32, 2048), 32
    return grid_for(span, 8, 2048), 8


def sum_depth(span, C):
    blocks, rows = gate_bwd_geometry(span, C)
    return -(-span // (blocks * rows)) + rows + blocks


def _gsum(a, grp, groups):
    return np.stack([a[grp == j].sum(0) for j in range(groups)])


class GateBackwardEval:
    """read_gate_backward + read_bn_param_grads: df, dm (P, C), sums (4, C), dbf, dbm, dbeta, dgamma (C,), each with cond_* and bound_*."""

    def __init__(self, dy, fm, C, L, elu, W, block_h, valid_h):
        P = fm.shape[0]
        gt = Gate(fm, C, elu)
        v = valid_rows(P, W, block_h, valid_h)[:, None]
        dy64 = dy.astype(np.float64) * v
        Ss = bn_scale(L["gamma"], L["var"])[None]
        mean, r = np.asarray(L["mean"], np.float64), 1.0 / np.sqrt(np.asarray(L["var"], np.float64) + EPS)
        gs = dy64 * Ss
        self.df, self.dm, self.bound_df, self.bound_dm = gt.through(gs, 4.5 * U * np.abs(gs), 2, 3)
        self.bound_df, self.bound_dm = self.bound_df * v, self.bound_dm * v
        self.cond_df = np.abs(gs) * gt.sig * gt.da_abs
        self.cond_dm = np.abs(gs) * gt.a_abs * gt.sig * (1 + gt.sig)
        depth = sum_depth(P, C)
        terms = [self.df, self.dm, dy64, dy64 * gt.g]
        d_terms = [self.bound_df, self.bound_dm, 0.0 * dy64, np.abs(dy64) * (gt.d_g + U * np.abs(gt.g))]
        self.sums = np.stack([t.sum(0) for t in terms])
        self.cond_sums = np.stack([np.abs(t).sum(0) for t in terms])
        self.bound_sums = np.stack([d.sum(0) for d in d_terms]) + depth * U * self.cond_sums + TINY
        # the part of that bound the terms bring with them (v_exp_f32 / v_rcp_f32 at 1 ulp, the gate's products) and one rounding of the sum
        self.lead_sums = np.stack([d.sum(0) for d in d_terms]) + U * self.cond_sums + TINY
        S2, S3 = self.sums[2], self.sums[3]
        self.dgamma = (S3 - mean * S2) * r
        self.cond_dgamma = {"centered": r * (np.abs(dy64) * np.abs(gt.g - mean[None])).sum(0),
                            "kernel": r * (self.cond_sums[3] + np.abs(mean) * self.cond_sums[2])}
        self.bound_dgamma = SECOND_ORDER * (r * (self.bound_sums[3] + np.abs(mean) * self.bound_sums[2] + U * np.abs(mean * S2) + U * np.abs(S3 - mean * S2))
                                            + 4.5 * U * np.abs(self.dgamma)) + TINY
        # the same bound with depth = 1 and exact terms: what a formulation without the |mean| sum |dy| term would be held to
        # the leading term of that bound where |mean| >> std (the kernel's formulation): the summation error of S3 and of mean S2
        self.lead_dgamma_terms = r * self.lead_sums[3]
        self.lead_dgamma = self.lead_dgamma_terms + depth * U * self.cond_dgamma["kernel"]


# ------------------------------------------------------------------------------------------ batch-statistics BatchNorm
class BnForward:
    """read_bn_train_forward: y (P, C), stat (groups, 2, C), running mean / var (C,), with cond_* and bound_*."""

    def __init__(self, g, L, W, block_h, valid_h, groups, momentum, rm0, rv0):
        P, C = g.shape
        v = valid_rows(P, W, block_h, valid_h)
        grp = group_of(P, W, block_h, groups)
        g64 = g.astype(np.float64)
        gamma, beta = np.asarray(L["gamma"], np.float64), np.asarray(L["beta"], np.float64)
        self.y, self.cond_y, self.cond_y_centered, self.bound_y = (np.zeros((P, C)) for _ in range(4))
        self.stat, self.bound_stat, self.cond_stat = np.zeros((groups, 2, C)), np.zeros((groups, 2, C)), np.zeros((groups, 2, C))
        rm, rv = rm0.astype(np.float64), rv0.astype(np.float64)
        e_rm, e_rv = np.zeros(C), np.zeros(C)
        for j in range(groups):
            sel = v & (grp == j)
            x = g64[sel]
            n = x.shape[0]
            mean, ex2 = x.mean(0), (x * x).mean(0)
            var = ((x - mean[None]) ** 2).mean(0)
            d_var = 2.0 ** -40 * ex2
            self.stat[j, 0], self.stat[j, 1] = mean, var
            self.cond_stat[j, 0], self.cond_stat[j, 1] = np.abs(x).mean(0), ex2 + mean * mean
            self.bound_stat[j, 0], self.bound_stat[j, 1] = U * np.abs(mean) + TINY, U * var + d_var + TINY
            S = gamma / np.sqrt(var + EPS)
            aS = np.abs(S)
            dS_var = aS * d_var / (2 * (var + EPS))
            T = beta - mean * S
            y = x * S[None] + T[None]
            self.y[sel] = y
            self.cond_y[sel] = aS[None] * np.abs(x) + (aS * np.abs(mean) + np.abs(beta))[None]
            self.cond_y_centered[sel] = aS[None] * np.abs(x - mean[None]) + np.abs(beta)[None]
            self.bound_y[sel] = SECOND_ORDER * (U * (7 * aS[None] * np.abs(x) + (7 * aS * np.abs(mean) + np.abs(T))[None] + np.abs(y))
                                                + (np.abs(x) + np.abs(mean)[None]) * dS_var[None]) + TINY
            unb = var * n / (n - 1) if n > 1 else var
            c_rm, c_rv = np.abs((1 - momentum) * rm) + np.abs(momentum * mean), np.abs((1 - momentum) * rv) + np.abs(momentum * unb)
            e_rm = (1 - momentum) * e_rm + 5 * U * c_rm + TINY
            e_rv = (1 - momentum) * e_rv + 5 * U * c_rv + momentum * d_var * 2 + TINY
            rm, rv = (1 - momentum) * rm + momentum * mean, (1 - momentum) * rv + momentum * unb
            self.cond_rm, self.cond_rv = c_rm, c_rv
        self.running_mean, self.running_var, self.bound_rm, self.bound_rv = rm, rv, e_rm, e_rv


class GateBackwardBn:
    """read_gate_backward_bn + read_bn_param_grads_groups.  stat (groups, 2, C) float32 is an INPUT (the forward pass's mean and biased
    variance): the reference is the function of (dy, fm, stat) the kernels state, which is BatchNorm's backward when stat is exact."""

    def __init__(self, dy, fm, C, gamma, elu, W, block_h, valid_h, groups, stat):
        P = fm.shape[0]
        gt = Gate(fm, C, elu)
        v = valid_rows(P, W, block_h, valid_h)
        grp = group_of(P, W, block_h, groups)
        dy64 = dy.astype(np.float64) * v[:, None]
        gamma = np.asarray(gamma, np.float64)
        span = P if groups == 1 else block_h * W
        depth = sum_depth(span, C)
        self.df, self.dm, self.bound_df, self.bound_dm, self.cond_dg, self.dg, self.bound_dg = (np.zeros((P, C)) for _ in range(7))
        self.dgamma, self.dbeta, self.dbf, self.dbm = (np.zeros(C) for _ in range(4))
        self.lead_df, self.lead_dm, self.lead_dgamma = np.zeros((P, C)), np.zeros((P, C)), np.zeros(C)
        self.lead_dbf, self.lead_dbm, self.lead_dgamma_terms = np.zeros(C), np.zeros(C), np.zeros(C)
        self.bound_dgamma, self.bound_dbeta, self.bound_dbf, self.bound_dbm = (np.zeros(C) for _ in range(4))
        self.cond_dgamma = {"centered": np.zeros(C), "kernel": np.zeros(C)}
        self.cond_dbeta, self.cond_dbf, self.cond_dbm = np.zeros(C), np.zeros(C), np.zeros(C)
        for j in range(groups):
            sel = v & (grp == j)
            n = int(sel.sum())
            mean, var = stat[j, 0].astype(np.float64), stat[j, 1].astype(np.float64)
            r = 1.0 / np.sqrt(var + EPS)
            d, g, d_g = dy64[sel], gt.g[sel], gt.d_g[sel]
            xh = (g - mean[None]) * r[None]
            S2, S3 = d.sum(0), (d * g).sum(0)
            c2, c3 = np.abs(d).sum(0), np.abs(d * g).sum(0)
            e2 = depth * U * c2 + TINY
            e3 = (np.abs(d) * (d_g + U * np.abs(g))).sum(0) + depth * U * c3 + TINY
            dgam = (d * xh).sum(0)
            e_dg = r * (e3 + np.abs(mean) * e2 + U * np.abs(mean * S2) + U * np.abs(S3 - mean * S2)) + 4.5 * U * np.abs(dgam) + TINY
            A = gamma * r
            Cc = -A * r * dgam / n
            B = -A * S2 / n - Cc * mean
            e_C = 11 * U * np.abs(Cc) + np.abs(A) * r * e_dg / n
            e_B = 6.5 * U * np.abs(A * S2 / n) + np.abs(A) * e2 / n + np.abs(mean) * e_C + U * np.abs(Cc * mean) + U * np.abs(B)
            gs = A[None] * (d - S2[None] / n - xh * dgam[None] / n)
            e_gs = (5.5 * U * np.abs(A[None] * d) + U * np.abs(A[None] * d + B[None]) + e_B[None] + np.abs(g) * e_C[None]
                    + np.abs(Cc)[None] * d_g + U * np.abs(Cc[None] * g) + U * np.abs(gs))
            sub = Gate.__new__(Gate)
            for k_, val in gt.__dict__.items():
                setattr(sub, k_, val[sel] if isinstance(val, np.ndarray) else val)
            df, dm, b_f, b_m = sub.through(gs, e_gs, 2, 3)
            self.dg[sel], self.bound_dg[sel] = gs, e_gs
            lead_C = np.abs(A) * r * r * depth * U * (c3 + np.abs(mean) * c2) / n      # of e_C: the summation error of S3 - mean S2
            lead_gs = (np.abs(mean)[None] + np.abs(g)) * lead_C[None]
            self.lead_df[sel], self.lead_dm[sel] = lead_gs * sub.sig * sub.da, lead_gs * np.abs(sub.a) * sub.sig * sub.oms
            self.lead_dgamma_terms += r * ((np.abs(d) * (d_g + U * np.abs(g))).sum(0) + U * c3) + TINY
            self.lead_dgamma += depth * U * r * (c3 + np.abs(mean) * c2)
            self.lead_dbf += b_f.sum(0) + U * np.abs(df).sum(0)
            self.lead_dbm += b_m.sum(0) + U * np.abs(dm).sum(0)
            self.df[sel], self.dm[sel], self.bound_df[sel], self.bound_dm[sel] = df, dm, b_f, b_m
            self.cond_dg[sel] = np.abs(A)[None] * (np.abs(d) + c2[None] / n + np.abs(xh) * (np.abs(d) * np.abs(xh)).sum(0)[None] / n)
            self.dgamma += dgam
            self.dbeta += S2
            self.dbf += df.sum(0)
            self.dbm += dm.sum(0)
            self.cond_dgamma["centered"] += r * (np.abs(d) * np.abs(g - mean[None])).sum(0)
            self.cond_dgamma["kernel"] += r * (c3 + np.abs(mean) * c2)
            self.cond_dbeta += c2
            self.cond_dbf += np.abs(df).sum(0)
            self.cond_dbm += np.abs(dm).sum(0)
            self.bound_dgamma += e_dg
            self.bound_dbeta += e2
            self.bound_dbf += b_f.sum(0) + depth * U * np.abs(df).sum(0)
            self.bound_dbm += b_m.sum(0) + depth * U * np.abs(dm).sum(0)
        for name in ("dgamma", "dbeta", "dbf", "dbm"):               # the groups' contributions are added in fp32, in order
            b = getattr(self, "bound_" + name)
            setattr(self, "bound_" + name, SECOND_ORDER * (b + groups * U * (self.cond_dgamma["kernel"] if name == "dgamma" else getattr(self, "cond_" + name))) + TINY)


def bn_backward_torch64(dy, fm, C, gamma, elu, W, block_h, valid_h, groups):
    """torch double autograd of act(f) sigmoid(m) -> F.batch_norm(training) per statistic group: (df, dm, dgamma, dbeta, stat)."""
    P = fm.shape[0]
    v = valid_rows(P, W, block_h, valid_h)
    grp = group_of(P, W, block_h, groups)
    t = torch.from_numpy(fm.astype(np.float64)).requires_grad_(True)
    ga = torch.from_numpy(np.asarray(gamma, np.float64)).requires_grad_(True)
    be = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    f, m = t[:, :C], t[:, C:]
    g = (F.elu(f) if elu else f) * torch.sigmoid(m)
    tot = 0.0
    stat = np.zeros((groups, 2, C))
    for j in range(groups):
        idx = torch.from_numpy(np.nonzero(v & (grp == j))[0])
        gj = g[idx]
        stat[j, 0], stat[j, 1] = gj.mean(0).detach().numpy(), gj.var(0, unbiased=False).detach().numpy()
        y = F.batch_norm(gj.t()[None], None, None, ga, be, training=True, eps=EPS)[0].t()
        tot = tot + (y * torch.from_numpy(dy.astype(np.float64))[idx]).sum()
    tot.backward()
    return t.grad[:, :C].numpy(), t.grad[:, C:].numpy(), ga.grad.numpy(), be.grad.numpy(), stat


# ------------------------------------------------------------------------------------------ weight gradients
def out_hw(k, stride, H, W):
    pad = (k - 1) // 2
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def wgrad_plan(cin, cout, k, outH):
    """wgrad_plan of train.hip: -> dict NT, splits, rows_per_split."""
    taps = k * k
    NT = 1 if taps == 1 else (9 if taps == 9 else 8)
    tap_groups = (taps + NT - 1) // NT
    tiles_ci = (cin + 31) // 32
    if taps == 1 and cin % 32 == 0 and tiles_ci > 1:
        NT = 5 if tiles_ci % 5 == 0 else (4 if tiles_ci % 4 == 0 else (2 if tiles_ci % 2 == 0 else 1))
        tiles_ci //= NT
    tiles_co = (2 * pad8(cout) + 31) // 32
    waves = tiles_ci * tiles_co * tap_groups
    splits = max(1, min((2048 + waves - 1) // waves, outH))
    rps = (outH + splits - 1) // splits
    return dict(NT=NT, splits=(outH + rps - 1) // rps, rows_per_split=rps)


def wgrad4_plan(cin, cout, H):
    wgs = (cin // 32) * ((2 * pad8(cout) + 31) // 32)
    tiles_y = H // 4
    splits = max(1, min((256 + wgs - 1) // wgs, tiles_y))
    rps = (tiles_y + splits - 1) // splits
    return dict(splits=(tiles_y + rps - 1) // rps, rows_per_split=rps)


def wgrad_ref(x_hwc, d_hwc, k, stride):
    """x (H, W, Cin), d (outH, outW, Co) -> (dW, A), (Co, Cin, k, k) float64."""
    pad = (k - 1) // 2
    x = torch.from_numpy(np.ascontiguousarray(x_hwc.transpose(2, 0, 1))).double()[None]
    d = torch.from_numpy(np.ascontiguousarray(d_hwc.transpose(2, 0, 1))).double()[None]
    shape = (d.shape[1], x.shape[1], k, k)
    return (torch.nn.grad.conv2d_weight(x, shape, d, stride=stride, padding=pad).numpy(),
            torch.nn.grad.conv2d_weight(x.abs(), shape, d.abs(), stride=stride, padding=pad).numpy())


def wgrad_direct_bound(A, cin, cout, k, outH, outW, accumulate=False, previous=None):
    p = wgrad_plan(cin, cout, k, outH)
    N = 2 * p["rows_per_split"] * ((outW + 1) // 2)
    b = U * (N + 1 + p["splits"]) * A
    if accumulate:
        b = b + U * (A + np.abs(previous))
    return SECOND_ORDER * b + TINY


def wgrad_wino_Aw(x_hwc, d_hwc):
    """A_w (Co, Cin, 3, 3) of the module docstring."""
    H, W, cin = x_hwc.shape
    ty, tx = H // 4, W // 4
    xp = np.zeros((H + 2, W + 2, cin))
    xp[1:-1, 1:-1] = np.abs(x_hwc)
    iy = (4 * np.arange(ty))[:, None] + np.arange(6)[None]
    ix = (4 * np.arange(tx))[:, None] + np.arange(6)[None]
    patch = xp[iy[:, None, :, None], ix[None, :, None, :]]                                       # (ty, tx, 6, 6, C)
    V = np.einsum("ia,tuabc,jb->tuijc", np.abs(BT), patch, np.abs(BT)).reshape(ty * tx, 36, cin)
    dt = np.abs(d_hwc.astype(np.float64)).reshape(ty, 4, tx, 4, -1)
    M = np.einsum("ia,taubo,jb->tuijo", np.abs(AT.T), dt, np.abs(AT.T)).reshape(ty * tx, 36, -1)
    Uw = np.einsum("tfc,tfo->ocf", V, M).reshape(M.shape[2], cin, 6, 6)
    return np.einsum("xa,ocxn,nb->ocab", np.abs(G), Uw, np.abs(G))


def wgrad_wino_bound(Aw, cin, cout, H, W, accumulate=False, previous=None):
    p = wgrad4_plan(cin, cout, H)
    N = 8 * p["rows_per_split"] * ((W // 4 + 7) // 8)
    b = U * (19 + N + p["splits"]) * Aw
    if accumulate:
        b = b + U * (Aw + np.abs(previous))
    return SECOND_ORDER * b + TINY


def wgrad_torch32(x_hwc, d_hwc, k, stride):
    pad = (k - 1) // 2
    x = torch.from_numpy(np.ascontiguousarray(x_hwc.transpose(2, 0, 1)))[None]
    d = torch.from_numpy(np.ascontiguousarray(d_hwc.transpose(2, 0, 1)))[None]
    return torch.nn.grad.conv2d_weight(x, (d.shape[1], x.shape[1], k, k), d, stride=stride, padding=pad).numpy()


def wgrad_seq32(x_hwc, d_hwc, k, stride):
    """fp32, every entry summed over the output pixels in raster order, one rounded product and one rounded addition per pixel."""
    pad = (k - 1) // 2
    H, W, cin = x_hwc.shape
    oh, ow, co = d_hwc.shape
    xp = np.zeros((H + 2 * pad + k, W + 2 * pad + k, cin), np.float32)
    xp[pad:pad + H, pad:pad + W] = x_hwc
    acc = np.zeros((co, cin, k, k), np.float32)
    for oy in range(oh):
        for ox in range(ow):
            patch = xp[oy * stride:oy * stride + k, ox * stride:ox * stride + k]                   # (k, k, cin)
            acc = acc + (d_hwc[oy, ox][:, None, None, None] * patch.transpose(2, 0, 1)[None]).astype(np.float32)
    return acc


# ------------------------------------------------------------------------------------------ input gradient, generic
def dgrad_ref(dfm, cout, wf, wm, k, stride, inH, inW):
    """dfm (outH, outW, 2 Cp) -> (dx, cond) (inH, inW, Cin) float64."""
    cp, pad, cin = pad8(cout), (k - 1) // 2, wf.shape[1]
    out = []
    for fn in (lambda a: a, np.abs):
        tot = 0.0
        for half, w in ((0, wf), (1, wm)):
            d = torch.from_numpy(np.ascontiguousarray(fn(dfm[:, :, half * cp:half * cp + cout].astype(np.float64)).transpose(2, 0, 1)))[None]
            tot = tot + torch.nn.grad.conv2d_input((1, cin, inH, inW), torch.from_numpy(fn(w.astype(np.float64))), d, stride=stride, padding=pad)[0]
        out.append(tot.numpy().transpose(1, 2, 0))
    return out


def dgrad_bound(cond, cout, k, stride):
    return SECOND_ORDER * U * (math.ceil(k / stride) ** 2 * 2 * pad8(cout) + 1) * cond + TINY


def dgrad_torch32(dfm, cout, wf, wm, k, stride, inH, inW):
    cp, pad, cin = pad8(cout), (k - 1) // 2, wf.shape[1]
    tot = 0.0
    for half, w in ((0, wf), (1, wm)):
        d = torch.from_numpy(np.ascontiguousarray(dfm[:, :, half * cp:half * cp + cout].transpose(2, 0, 1)))[None]
        tot = tot + torch.nn.grad.conv2d_input((1, cin, inH, inW), torch.from_numpy(w), d, stride=stride, padding=pad)[0]
    return tot.numpy().transpose(1, 2, 0)


def dgrad_seq32(dfm, cout, wf, wm, k, stride, inH, inW):
    """fp32 in the kernel's loop order (taps, then the 2 Cp channels), one rounded product and one rounded addition per term."""
    cp, pad, cin = pad8(cout), (k - 1) // 2, wf.shape[1]
    oh, ow = dfm.shape[:2]
    acc = np.zeros((inH + 2 * k, inW + 2 * k, cin), np.float32)                                   # origin shifted by k
    for ky in range(k):
        for kx in range(k):
            ys = k + np.arange(oh) * stride + ky - pad
            xs = k + np.arange(ow) * stride + kx - pad
            for c in range(2 * cp):
                co = c % cp
                if co >= cout:
                    continue
                w = (wf if c < cp else wm)[co, :, ky, kx]
                acc[np.ix_(ys, xs)] = acc[np.ix_(ys, xs)] + (dfm[:, :, c][:, :, None] * w[None, None, :]).astype(np.float32)
    return acc[k:k + inH, k:k + inW]


# ------------------------------------------------------------------------------------------ bilinear x 4
def _items(H, block_h, valid_h):
    return [(0, H)] if block_h <= 0 else [(b * block_h, valid_h) for b in range(H // block_h)]


def up4_forward_ref(x_hwc, block_h, valid_h):
    """-> (out, cond, bound) (4 H, 4 W, C) float64; separator rows zero."""
    H, W, C = x_hwc.shape
    out, cond = np.zeros((4 * H, 4 * W, C)), np.zeros((4 * H, 4 * W, C))
    for y0, n in _items(H, block_h, valid_h):
        for dst, fn in ((out, lambda a: a), (cond, np.abs)):
            t = torch.from_numpy(np.ascontiguousarray(fn(x_hwc[y0:y0 + n].astype(np.float64)).transpose(2, 0, 1)))[None]
            dst[4 * y0:4 * (y0 + n)] = F.interpolate(t, scale_factor=4, mode="bilinear", align_corners=False)[0].numpy().transpose(1, 2, 0)
    return out, cond, SECOND_ORDER * 5 * U * cond + TINY * (cond > 0)


def up4_backward_ref(dout_hwc, H, W, block_h, valid_h):
    """dout (4 H, 4 W, C) -> (din, cond, bound) (H, W, C): torch double autograd of F.interpolate per item."""
    C = dout_hwc.shape[2]
    din, cond = np.zeros((H, W, C)), np.zeros((H, W, C))
    for y0, n in _items(H, block_h, valid_h):
        for dst, fn in ((din, lambda a: a), (cond, np.abs)):
            t = torch.zeros((1, C, n, W), dtype=torch.float64, requires_grad=True)
            d = torch.from_numpy(np.ascontiguousarray(fn(dout_hwc[4 * y0:4 * (y0 + n)].astype(np.float64)).transpose(2, 0, 1)))[None]
            (F.interpolate(t, scale_factor=4, mode="bilinear", align_corners=False) * d).sum().backward()
            dst[y0:y0 + n] = t.grad[0].numpy().transpose(1, 2, 0)
    return din, cond, SECOND_ORDER * 37 * U * cond + TINY * (cond > 0)


def up4_torch32(a_hwc, H, W, block_h, valid_h, backward):
    """The torch-fp32 yardstick of either direction."""
    C = a_hwc.shape[2]
    out = np.zeros((H, W, C) if backward else (4 * H, 4 * W, C), np.float32)
    for y0, n in _items(H, block_h, valid_h):
        if backward:
            t = torch.zeros((1, C, n, W), requires_grad=True)
            d = torch.from_numpy(np.ascontiguousarray(a_hwc[4 * y0:4 * (y0 + n)].transpose(2, 0, 1)))[None]
            (F.interpolate(t, scale_factor=4, mode="bilinear", align_corners=False) * d).sum().backward()
            out[y0:y0 + n] = t.grad[0].numpy().transpose(1, 2, 0)
        else:
            t = torch.from_numpy(np.ascontiguousarray(a_hwc[y0:y0 + n].transpose(2, 0, 1)))[None]
            out[4 * y0:4 * (y0 + n)] = F.interpolate(t, scale_factor=4, mode="bilinear", align_corners=False)[0].numpy().transpose(1, 2, 0)
    return out


# ------------------------------------------------------------------------------------------ Huber
def huber_ref(out, target, scale):
    """-> dict grad, bound_grad (n,), loss_sum, cond_loss, bound_loss (the SUM of the elements' losses, as the kernel returns it)."""
    n = out.size
    d = out.astype(np.float64) - target.astype(np.float64)
    ad = np.abs(d)
    grad = scale * np.where(ad < 1, d, np.sign(d))
    l = np.where(ad < 1, 0.5 * d * d, ad - 0.5)
    blocks = grid_for(n, 256, 1024)
    depth = -(-n // (256 * blocks)) + 8 + blocks
    d_l = U * (2 * ad * np.minimum(ad, 1.0) + 2 * l)
    return dict(grad=grad, bound_grad=SECOND_ORDER * 2 * U * np.abs(grad) + TINY * (grad != 0), loss_sum=l.sum(), cond_loss=np.abs(l).sum(),
                bound_loss=SECOND_ORDER * (d_l.sum() + depth * U * np.abs(l).sum()) + TINY * n)


# ------------------------------------------------------------------------------------------ inputs
def unit_case(P, C, seed):
    """Class (a): fm, dy standard normal; BatchNorm parameters as conv_ref64.tame_layer."""
    rng = np.random.default_rng([seed, P, C, 0])
    L = R64.tame_layer(8, C, 1, seed)
    return rng.standard_normal((P, 2 * C)).astype(np.float32), rng.standard_normal((P, C)).astype(np.float32), L


def scales_b(C, rng):
    """Class (b): per-channel scales 2^U(-8, 6), the two extremes always present (a span of 2^14)."""
    s = 2.0 ** rng.uniform(-8, 6, C)
    if C >= 2:
        s[rng.permutation(C)[:2]] = (2.0 ** -8, 2.0 ** 6)
    return s


def checkpoint_case(P, C, seed):
    """Class (b): the BatchNorm statistics of conv_ref64.checkpoint_like (var 1e-4 .. 1e2, gamma of both signs and 0); f, m unit scale
    times 2^U(-3, 3) per channel (the gate saturates above), dy per-channel scales 2^U(-8, 6)."""
    rng = np.random.default_rng([seed, P, C, 1])
    L, _ = R64.checkpoint_like(8, C, 1, 2, 2, seed, edge_rows=False)
    fm = (rng.standard_normal((P, 2 * C)) * (2.0 ** rng.uniform(-3, 3, 2 * C))[None]).astype(np.float32)
    dy = (rng.standard_normal((P, C)) * scales_b(C, rng)[None]).astype(np.float32)
    return fm, dy, L


D_CHANNELS = ("ratio1", "ratio32", "ratio256", "constant", "elu_saturated", "gate_overflow", "tiny_f")


def range_edge_case(P, C, seed):
    """Class (d): channel c is of kind D_CHANNELS[c % 7].  ratioN: ELU off the table (f > 0), m = 40 (sigmoid = 1 in fp32 and 1 - 4e-18 in
    fp64): g = f with |mean| / std = N (N = 1: an exponential distribution, to within the sample's own scatter); constant: f = 100, m = 40: var = 0; elu_saturated: f in
    [-60, -20]; gate_overflow: m = +-(100 .. 200); tiny_f: |f| ~ 1e-6.  -> (fm, dy, L, kinds)."""
    rng = np.random.default_rng([seed, P, C, 3])
    fm, dy, L = unit_case(P, C, seed)
    kinds = [D_CHANNELS[c % len(D_CHANNELS)] for c in range(C)]
    z = rng.standard_normal((P, C))
    z = (z - z.mean(0)) / z.std(0)
    for c, kind in enumerate(kinds):
        if kind.startswith("ratio"):
            n = float(kind[5:])
            e = rng.exponential(1.0, P)                              # ratio 1 with f > 0: a positive distribution whose mean is its std
            fm[:, c] = (0.03 * e / e.mean() if n == 1 else 0.03 * (n + z[:, c])).astype(np.float32)
            fm[:, C + c] = 40.0
        elif kind == "constant":
            fm[:, c], fm[:, C + c] = 100.0, 40.0
        elif kind == "elu_saturated":
            fm[:, c] = rng.uniform(-60, -20, P).astype(np.float32)
        elif kind == "gate_overflow":
            fm[:, C + c] = (rng.choice([-1.0, 1.0], P) * rng.uniform(100, 200, P)).astype(np.float32)
        elif kind == "tiny_f":
            fm[:, c] = (1e-6 * rng.standard_normal(P)).astype(np.float32)
    L["beta"] = np.full(C, 0.2, np.float32)
    return fm, dy, L, kinds


def small_integers(shape, rng, lo=1, hi=60):
    """Distinct-looking small integers (exact in fp32, and so are their sums over a few thousand pixels)."""
    return rng.integers(lo, hi, shape).astype(np.float32)


def impulse_pixels(H, W, splits_rows=(), tile=4):
    """Positions (y, x) for an impulse of d: corners, edges, both sides of every split boundary and of every 4 x 4 tile boundary, and the
    last (odd) pixel of a row."""
    pos = {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1), (H // 2, W - 1 - (W % 2 == 0))}
    for r in splits_rows:
        for y in (r - 1, r):
            if 0 <= y < H:
                pos.add((y, W // 3))
    for b in range(tile, max(H, W), tile):
        for q in (b - 1, b):
            if q < H:
                pos.add((q, min(W - 1, 1)))
            if q < W:
                pos.add((min(H - 1, 1), q))
    return sorted(pos)


# ------------------------------------------------------------------------------------------ RMSprop over the touched rows
LONG_RUN, MAX_LONG, LONG_SUB = 512, 64, 64


def run_sum_depth(length, long_slot):
    """Additions a gradient row passes through in rmsprop_sorted_kernel (:1647-1652, one thread, in sorted order) or, for a run above
    LONG_RUN that got one of the MAX_LONG slots, in rmsprop_long_partial_kernel / _final_kernel (:1667-1695)."""
    if length > LONG_RUN and long_slot:
        return -(-(-(-length // LONG_SUB)) // 256) + 8 + LONG_SUB
    return length


class RmspropTrajectory:
    """Dense float64 RMSprop (alpha, eps; no momentum, not centred) over the rows, step by step, with the bound of the sparse kernels' fp32
    trajectory carried along.  Per touched row (rmsprop_row :1608-1615): decay = powf(alpha, missed) (2 ulp = 4 u assumed), v = alpha (sq decay)
    + (1 - alpha) g g: 8 roundings on positive terms, 8 u v;  the update lr g / (sqrtf(v) + eps): product, sqrt, add, divide: 4 u, and the
    subtraction from the row u |p|.  First-order sensitivities carry e_g (the run's sum: depth u sum |rows|) and e_v forward:
        e_v   = alpha decay e_v(last) + 8 u v + 2 (1 - alpha) |g| e_g
        e_upd = lr (e_g / (sqrt v + eps) + |g| (e_v / (2 sqrt v) + 2 u sqrt v) / (sqrt v + eps)^2) + 4 u |upd|
        e_p   = e_p(previous) + e_upd + u |p|
    cond is the same with u = 1 per input: cond_upd = lr (cond_g / (sqrt v + eps) + |g| (v + 2 (1 - alpha) |g| cond_g) / (2 sqrt v (sqrt v + eps)^2)),
    cond_v = alpha decay sq + (1 - alpha) (sum |rows|)^2."""

    def __init__(self, rows, alpha=0.99, eps=1e-8):
        self.p = rows.astype(np.float64)
        self.sq = np.zeros_like(self.p)
        self.alpha, self.eps = alpha, eps
        self.e_p, self.e_v, self.cond_v = np.zeros_like(self.p), np.zeros_like(self.p), np.zeros_like(self.p)
        self.cond_p = np.abs(self.p)
        self.last = np.zeros(rows.shape[0], np.int64)
        self.step = 0

    def idle(self, steps):
        """`steps` steps in which no row is touched: the dense optimizer only decays sq."""
        self.step += steps
        self.sq = self.alpha ** steps * self.sq

    def apply(self, ids, g_rows, lr, long_slots=True):
        """ids (n,) int (out-of-range ids are skipped), g_rows (n, C) float32.  -> the set of touched rows."""
        self.step += 1
        N, C = self.p.shape
        a = self.alpha
        ok = (ids >= 0) & (ids < N)
        g, cg = np.zeros((N, C)), np.zeros((N, C))
        np.add.at(g, ids[ok], g_rows[ok].astype(np.float64))
        np.add.at(cg, ids[ok], np.abs(g_rows[ok].astype(np.float64)))
        count = np.bincount(ids[ok], minlength=N)
        n_long = int((count > LONG_RUN).sum())
        depth = np.array([run_sum_depth(int(c), long_slots and n_long <= MAX_LONG) for c in count], np.float64)
        e_g = depth[:, None] * U * cg
        touched = count > 0
        missed = (self.step - 1 - self.last)[:, None]
        decay = a ** missed
        self.sq = a * self.sq                                          # the dense optimizer decays every row
        self.e_v = np.where(touched[:, None], a * decay * self.e_v, self.e_v)      # the stored sq is as old as the row's last touch
        v = self.sq + (1 - a) * g * g
        self.cond_v = np.where(touched[:, None], self.sq + (1 - a) * cg * cg, self.cond_v)       # every summand of the run's sum by its absolute value
        e_v = self.e_v + 8 * U * v + 2 * (1 - a) * np.abs(g) * e_g + U * U * cg * cg
        rt = np.sqrt(v)
        den = rt + self.eps
        safe = np.where(rt > 0, rt, 1.0)
        upd = lr * g / den
        e_upd = lr * (e_g / den + np.abs(g) * (e_v / (2 * safe) + 2 * U * rt) / den ** 2) + 4 * U * np.abs(upd)
        c_upd = lr * (cg / den + np.abs(g) * (v + 2 * (1 - a) * np.abs(g) * cg) / (2 * safe * den ** 2))
        t = touched[:, None]
        self.sq = np.where(t, v, self.sq)
        self.e_v = np.where(t, e_v, self.e_v)
        self.p = np.where(t, self.p - upd, self.p)
        self.e_p = np.where(t, SECOND_ORDER * (self.e_p + e_upd + U * np.abs(self.p)) + TINY, self.e_p)
        self.cond_p = np.where(t, self.cond_p + c_upd, self.cond_p)
        self.last = np.where(touched, self.step, self.last)
        return touched


# ------------------------------------------------------------------------------------------ input gradient through the convolution kernels
# The stride-1 dgrad is the layer's own fp32 convolution kernel over d[f|m] with flipped, transposed weights (pack_weights_kernel /
# pack_wino_kernel / pack_w4_kernel mode 1, train.hip:52-182): a virtual layer of 2 Cp input channels and Cin outputs.
F2_BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float64)
F2_G = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], np.float64)
F2_AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float64)


def virtual_weights(wf, wm, taps=None):
    """(Cin, 2 Cp, k, k): Wv[ci][c'][a][b] = W{c' < Cp ? f : m}[c' % Cp][ci][k - 1 - a][k - 1 - b], zero rows for the padded channels."""
    cout, cin, k, _ = wf.shape
    cp = pad8(cout)
    wv = np.zeros((cin, 2 * cp, k, k), np.float64)
    for half, w in ((0, wf), (1, wm)):
        wv[:, half * cp:half * cp + cout] = w.astype(np.float64)[:, :, ::-1, ::-1].transpose(1, 0, 2, 3)
    return wv


def wino_forward_terms(x_chw, w, m):
    """F(m x m, 3 x 3), m = 2 or 4: -> (A_w, A_in) (Cout, H, W): A_w = |A^T| (sum_c (|G| |g| |G^T|) . |B^T d B|) |A|, A_in the same with
    |B^T| |d| |B| — the transformed-domain condition terms of tests/conv_ref64.py, the filter transform taken by absolute values too
    (pack_wino_body forms it in fp32)."""
    from tests.wino4_ref import AT as AT4, BT as BT4, G as G4
    At, Bt, Gm = (F2_AT, F2_BT, F2_G) if m == 2 else (AT4.astype(np.float64), BT4.astype(np.float64), np.asarray(G4, np.float64))
    cin, H, W = x_chw.shape
    p = m + 2
    ty, tx = -(-H // m), -(-W // m)
    xp = np.zeros((cin, m * ty + 2, m * tx + 2))
    xp[:, 1:H + 1, 1:W + 1] = x_chw
    iy = (m * np.arange(ty))[:, None] + np.arange(p)[None]
    ix = (m * np.arange(tx))[:, None] + np.arange(p)[None]
    d = xp[:, iy[:, None, :, None], ix[None, :, None, :]]
    V = np.abs(np.einsum("ia,ctuab,jb->tuijc", Bt, d, Bt))
    Vin = np.einsum("ia,ctuab,jb->tuijc", np.abs(Bt), np.abs(d), np.abs(Bt))
    Uabs = R64.filter_memo(w, ("fp32 wino", m), lambda a: np.einsum("ia,ocab,jb->ijco", np.abs(Gm), np.abs(a), np.abs(Gm)))
    out = []
    for Vx in (V, Vin):
        M = np.einsum("tuijc,ijco->tuijo", Vx, Uabs)
        Y = np.einsum("pi,tuijo,qj->otpuq", np.abs(At), M, np.abs(At)).reshape(w.shape[0], m * ty, m * tx)
        out.append(Y[:, :H, :W])
    return out


def conv_dgrad_bound(d_hwc, wv, cond, value, family):
    """|got - dx| <= this, (H, W, Cin).  family "direct" (the workgroup-tiled fp32 MFMA kernel): k k 2 Cp rounded products added in some
    order: u (k k 2 Cp + 1) cond.  "w2" / "w4" (the fp32 Winograd kernels F(2x2) / F(4x4)): the filter transform 4 u (two fp32 passes of
    two roundings; F(4x4): evaluated in double, rounded once), the input transform 2 u (F(2x2): one difference per pass) or 4 u (bt6)
    against A_in, the product 1, the channel sum 2 Cp, the output transform 4 u (F(2x2): two additions per pass) or 6 u, the store:
        u ((2 Cp + 1 + 4 + 6) A_w + 4 A_in + |dx|)."""
    c2, k = wv.shape[1], wv.shape[2]
    if family == "direct":
        return SECOND_ORDER * U * (k * k * c2 + 1) * cond + TINY
    Aw, Ain = wino_forward_terms(np.ascontiguousarray(d_hwc.astype(np.float64).transpose(2, 0, 1)), wv, 2 if family == "w2" else 4)
    return SECOND_ORDER * U * ((c2 + 11) * Aw + 4 * Ain + np.abs(value.transpose(2, 0, 1))).transpose(1, 2, 0) + TINY, Aw.transpose(1, 2, 0)


# ------------------------------------------------------------------------------------------ the forward's linear launches
# GatedConvFn.forward -> _linear_conv: the layer's OWN filters through the same three fp32 kernels (read_amd/csrc/conv.hip), linear = 1.
# The count is conv_dgrad_bound's with Cin in the place of 2 Cp, and the bias, which the dgrad's virtual layer does not have:
#   direct (the workgroup-tiled kernel): k k Cin rounded products added in some order by the MFMAs (and, with WK > 1, over the waves'
#     LDS partials, conv.hip:358-364), then ONE addition f += bf + pf (conv.hip:369-370; pf = 0 without an addend, so bf + pf is exact):
#         |got - f| <= u (k k Cin + 1) A_f,      A_f = sum |x| |w| + |b|     (every partial sum and the biased value are bounded by A_f)
#     A 1x1 layer whose Cout is no multiple of 32 (64 -> 56) also reports family 0 but runs on the fp32 pixel-lane kernel
#     (conv_uses_px; gated_conv_px_kernel, linear epilogue at conv.hip:3999): Cin fused multiply-adds and the bias: the same count.
#   F(2x2) (gated_conv_wino_kernel): the filter transform 4 u (pack_wino_body: two fp32 passes of two roundings), the input transform 2 u
#     against A_in (one difference per pass), the product 1, the channel sum Cin, the output transform 4 u (conv.hip:953-954 and 965-966:
#     r0 = acc0 + acc1 + acc2, Y = R0 + R1 + R2: two additions per pass), then f = Y + bf (conv.hip:981, 984): one rounding of the
#     biased value, u |f|;
#   F(4x4) (gated_conv_wino4_kernel<false, 1>): the filter transform 4 u (evaluated in double and rounded once: generous), the input
#     transform 4 u against A_in (bt6: two roundings per pass), the product 1, the channel sum Cin (v_mfma_f32_16x16x4_f32: four
#     products per instruction, Cin / 4 instructions per frequency), the output transform 6 u (conv.hip:1894-1908: R[0] = acc + s1 + s2,
#     three additions on the longest path per pass), then Y[p][px] + bb (conv.hip:1922): u |f|;
#         |got - f| <= u ((Cin + 1 + 4 + 6) A_w + 4 A_in + |f|),       A_w, A_in of wino_forward_terms, the bias in neither.
#   With b = 0 these ARE conv_dgrad_bound's numbers: its `+ 1` (direct) and its |dx| term (Winograd) are the epilogue's addition, which
#   the dgrad performs with a zero bias.  Where every weight of a row is zero (class (d) of the forward tests) A_w = A_in = 0 and the
#   accumulators are +0: the stored value is the exact sum 0 + b — b itself, except that (+0) + (-0) is +0.
# The measure takes cond = A_f (direct) or A_w + |b| (Winograd), as tests/test_gpu_conv_accuracy.py does for the split-operand kernels.
FORWARD_FAMILY = {"direct": 0, "w2": 2, "w4": 4}                   # read_conv_kernel_family of the three kernels


def conv_forward_bound(L, x_chw, ref, family, which):
    """|got - f| (which = "f") or |got - m| <= bound, elementwise, for the linear launch of the layer L on x: -> (bound, cond), each
    (Cout, outH, outW).  ref = conv_ref64.reference(L, x, stride); family "direct" / "w2" / "w4"."""
    w, b = R64.filter_memo(L["w" + which], "f64", lambda a: np.asarray(a, np.float64)), np.abs(np.asarray(L["b" + which], np.float64))[:, None, None]
    cin, k = w.shape[1], w.shape[2]
    A, val = (ref.Af, ref.f) if which == "f" else (ref.Am, ref.m)
    if family == "direct":
        return SECOND_ORDER * U * (k * k * cin + 1) * A + TINY, A
    Aw, Ain = wino_forward_terms(np.asarray(x_chw, np.float64), w, 2 if family == "w2" else 4)
    return SECOND_ORDER * U * ((cin + 11) * Aw + 4 * Ain + np.abs(val)) + TINY, Aw + b


def block_geometry(out_h, nb, v_num, v_den):
    """(block_h, valid_h) of a stacked batch of nb items at a layer whose OUTPUT has out_h rows (read_amd/train.py, GatedConvFn.forward:
    `bh = Ho // nb if nb > 1 else 0`, `vh = bh * v_num // v_den`) — the rule gate_forward_kernel's separator_row applies to output rows."""
    bh = out_h // nb if nb > 1 else 0
    return bh, bh * v_num // v_den


def poly_pseudo_weights(w, k):
    """The four 3 x 3 pseudo-layers of read_amd/train.py _poly_fragments: (parity 2 py + px, Cout, Cin, 3, 3); tap index k = the zero tap."""
    taps = np.array([[4, 1, 3], [0, 2, 4]] if k == 4 else [[3, 1, 3], [0, 2, 3]])
    w5 = np.pad(w, ((0, 0), (0, 0), (0, 1), (0, 1)))
    return np.stack([w5[:, :, taps[par >> 1]][:, :, :, taps[par & 1]] for par in range(4)])
