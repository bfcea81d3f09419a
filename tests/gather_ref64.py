"""float64 definitions of the descriptor path (read_amd/csrc/gather.hip, ten entry points), the derived error bounds with the roundings
they count, two fp32 yardsticks, a catalogue of deliberately wrong fp32 models, and the case set the CPU test
(tests/test_gather_accuracy_cpu.py) and the GPU test (tests/test_gpu_gather_accuracy.py) share.  Plain NumPy; the table pair is
tests/joint_texture_model.py (select, act_apply, act_slope, adjoint_*), the stitch merge tests/stitch_model.py — neither is restated.

THE MEASURE, as in tests/train_ref64.py.  E = |got - ref| / (u cond), u = 2^-24, cond = the reference's formula with every summand
replaced by its absolute value; for an activation cond = |act(v)|.  Where cond = 0 the kernel must return the exact constant.

THE DEFINITIONS.  clamp(id) = min(max(id, 0), n - 1) everywhere an id addresses a row, forward and backward alike.
  read_texture_to_rows / read_rows_to_texture   the transpose, compared as uint32
  read_gather_forward                           act(rows[clamp(id)])
  read_gather_forward_ss                        the four samples around (o + 1/2) ss - 1/2 with the edge clamp (index + 1 only where it
                                                stays inside the image), activated first, blended with the weights (1 - l, l) per axis;
                                                l = 0 for odd ss (the output IS the activated centre sample), l = 1/2 for even ss
  read_gather_forward_tables / _backward_tables joint_texture_model
  read_stitch_gather_forward                    stitch_model.merge for the winner, act_s(rows_s[clamp(local id)]) for the row
  read_gather_backward                          np.add.at in float64, with the hits k per row and sum |g| per row element
  read_bilinear_down / _backward                the same four-sample rule on NCHW planes, and its transpose

THE DERIVED BOUNDS (absolute, per element; SECOND_ORDER = 1 + 2^-10 on first-order terms; FLUSH = 2^-126 per operation that may
flush a result below the normal range).
  Activations.  ASSUMED, not measured: the accuracy of the device library's expf and tanhf is documented nowhere we can read, so the
      relative-error figures of the OpenCL C specification the device library is written to are used: exp <= 3 ulp, tanh <= 5 ulp
      (1 ulp <= 2 u relative).  Division and addition are correctly rounded under hipcc's default.  These figures may be tightened only
      by reading the expansion of expf / tanhf in the cross-compiled ISA of gather.hip and counting, never from what the device returns.
      sigmoid y = 1 / (1 + e), e = expf(-v): 6 u on e reaches y with the factor e / (1 + e) = 1 - y; the add and the divide u each:
          d_y <= u y (6 (1 - y) + 2) + FLUSH            (expf overflows to inf from |v| = 88.73: y = 0 against a true y < 2^-126)
      tanh:  d_y <= 10 u |y| + FLUSH.      none: 0, the row's bits.      v = +-inf: exactly 0 / 1 / +-1.      NaN: NaN.
  Bilinear blends (even ss).  wy0 (wx0 v0 + lx v1) + ly (wx0 v2 + lx v3): the weights are 1/2, products by 1/2 are exact; three
      additions remain (two if the compiler fuses one: gather.hip is built with default contraction; a fusion only removes a rounding),
      each of a partial sum no larger than cond.  The kernel's additions are two deep, which would give 2 u cond; torch's fp32
      interpolate adds the four products in a chain three deep, and the bound has to hold the yardsticks as well:
          d_out <= 1/4 sum_k d_act(v_k) + 3 u cond + 3 FLUSH,   cond = 1/4 sum_k |act(v_k)|
      Odd ss: the kernel returns the activated centre sample: d_out = d_act(v_0); 0 with activation none.  read_bilinear_down at odd ss
      blends with the weights 1 and 0: finite inputs give the centre sample's value, bound 0.
  read_bilinear_down_backward: the weights are 1/4, or 1 and 0: exact, bound 0 (inputs are kept 2^24 above the subnormal range).
  Scatter-add.  A row element hit k times is a chain of k - 1 rounded additions of partial sums no larger than (1 + u)^(k-1) sum |g|, in
      any order (the atomics commit in any order); -munsafe-fp-atomics gives hardware float adds, which may flush, once per addend:
          d <= ((1 + u)^(k-1) - 1) sum |g| + k FLUSH       (first order: (k - 1) u sum |g|);  k = 1: the gradient's bits;  k = 0: +0
  Table adjoint.  g = d slope(y), y the DEVICE's own forward output: the definition is d slope64(y_device).
      sigmoid: 1 - y, y (1 - y), the product with d: 3 u |d slope|.   tanh: y y (u y^2 absolute), 1 - y y (u slope), the product:
          d_g <= |d| u (y^2 + 2 slope) + FLUSH   (tanh),      3 u |d| slope + FLUSH   (sigmoid),      0   (none)
      dense mode adds the scatter-add bound over sum |g| and the k terms' own d_g.
      The distance to the true derivative at x is printed by the GPU test and asserted nowhere.

THE YARDSTICKS.  (1) the torch CPU fp32 operation: index_select, sigmoid / tanh, F.interpolate(scale_factor = 1 / ss, 'bilinear'),
index_add_, autograd for the adjoints; (2) a NumPy fp32 restatement of the kernel's expressions, collisions summed in pixel order.
The cap, as in the training harness: E_rms <= 2 max(R_torch_rms, R_seq_rms, 0.5), E_max <= 2 max(R_torch_max, R_seq_max, 1).  A row
that misses the cap but sits under the leading term of its derived bound is `raised`; every raised row needs a line
"- raised `family (class)`: ..." in profiles/gather_accuracy_fp64.md, or it fails."""
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

from tests import joint_texture_model as jm
from tests.conv_ref64 import SECOND_ORDER, U
from tests.train_ref64 import FLUSH, scales_b, stats, worst

f32 = np.float32
ACTS = ("none", "sigmoid", "tanh")
ACT_ID = jm.ACT
GRID_ITEMS = 2048 * 256                 # every launcher caps the grid at 2048 blocks of 256 threads
EXP_ULP, TANH_ULP = 3, 5                # assumed (module docstring)
SENTINEL = 0x7FC5E175                   # the NaN bit pattern output buffers are prefilled with
GUARD = 0x7FCBA9D5                      # ... and the one of the guard bands
GUARD_FLOATS = 64
MEASURE_FLOOR = 2.0 ** -100


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ------------------------------------------------------------------------------------------ activations
def act64(x, act):
    with np.errstate(all="ignore"):
        return jm.act_apply(np.asarray(x, np.float64), act)


def act_bound(x, act):
    """-> (lead, bound) of act(x) elementwise; 0 at +-inf (the exact constants) and at NaN (judged apart)."""
    x = np.asarray(x, np.float64)
    y = np.nan_to_num(act64(x, act), nan=0.0)
    if act == "sigmoid":
        lead = U * y * (2 * EXP_ULP * (1.0 - y) + 2)
    elif act == "tanh":
        lead = 2 * TANH_ULP * U * np.abs(y)
    else:
        return np.zeros(x.shape), np.zeros(x.shape)
    fin = np.isfinite(x)
    return np.where(fin, lead, 0.0), np.where(fin, SECOND_ORDER * lead + FLUSH, 0.0)


def act32_torch(x, act):
    t = torch.from_numpy(np.ascontiguousarray(x, f32))
    return (torch.sigmoid(t) if act == "sigmoid" else torch.tanh(t) if act == "tanh" else t).numpy()


def act32_seq(x, act, mut=None):
    """The kernel's expressions in NumPy fp32: 1 / (1 + expf(-v)), tanhf(v)."""
    x = np.ascontiguousarray(x, f32)
    with np.errstate(all="ignore"):
        if act == "sigmoid":
            e = np.exp(-x)
            if mut == "exp_rel_2^-18":
                e = (e * f32(1 + 2.0 ** -18)).astype(f32)
            return (f32(1) / (f32(1) + e)).astype(f32)
        if act == "tanh":
            if mut == "tanh_by_exp":
                e = np.exp((f32(2) * x).astype(f32))
                return np.where(np.isinf(e), f32(1), (e - f32(1)) / (e + f32(1))).astype(f32)
            return np.tanh(x)
    return x


def slope_bound(d, y, act):
    """The table adjoint's per-pixel bound: -> (g64 = d slope64(y), bound)."""
    d, y = np.asarray(d, np.float64), np.asarray(y, np.float64)
    s = jm.act_slope(y, act)
    g = d * s
    if act == "sigmoid":
        return g, SECOND_ORDER * 3 * U * np.abs(g) + FLUSH
    if act == "tanh":
        return g, SECOND_ORDER * U * np.abs(d) * (y * y + 2 * np.abs(s)) + FLUSH
    return g, np.zeros(g.shape)


def slope32_seq(d, y, act, mut=None):
    d, y = np.ascontiguousarray(d, f32), np.ascontiguousarray(y, f32)
    if act == "sigmoid":
        return (d * (y * (f32(1) - y)).astype(f32)).astype(f32)
    if act == "tanh":
        s = (f32(1) - y) if mut == "tanh_slope_1-y" else (f32(1) - (y * y).astype(f32))
        return (d * s.astype(f32)).astype(f32)
    return d


# ------------------------------------------------------------------------------------------ the plain gather
def clamp(ids, n, mut=None):
    ids = np.asarray(ids, np.int64)
    if mut == "clamp_to_n":
        return np.clip(ids, 0, n)                      # the caller pads the table with a NaN row at n
    if mut == "negative_wrap":
        return np.where(ids < 0, ids % n, np.minimum(ids, n - 1))
    return np.clip(ids, 0, n - 1)


def gather_ref(rows, ids, act):
    """rows (n, C) fp32, ids (P,) -> (y, cond, lead, bound, x) float64, x the raw samples (NaN where the row holds NaN)."""
    x = np.asarray(rows, np.float64)[clamp(ids, len(rows))]
    y = act64(x, act)
    lead, bound = act_bound(x, act)
    return y, np.abs(np.nan_to_num(y, nan=0.0)), lead, bound, x


def gather_torch32(rows, ids, act):
    t = torch.index_select(torch.from_numpy(np.ascontiguousarray(rows, f32)), 0, torch.from_numpy(clamp(ids, len(rows))))
    return act32_torch(t.numpy(), act)


def decode_items(counts, C, mut=None):
    """The kernels' item -> (level, pixel, quad) decode, for every item of a launch: -> (level, pix, q, written) int arrays; `written`
    is False for an item the (mutated) decode sends outside its level (the restatement then leaves the sentinel in place)."""
    qpp = C // 4
    end = np.cumsum(np.asarray(counts, np.int64) * qpp)
    item = np.arange(int(end[-1]), dtype=np.int64)
    if mut == "stop_at_grid":
        item = item[item < GRID_ITEMS]
    lvl, base = np.zeros(item.shape, np.int64), np.zeros(item.shape, np.int64)
    for k in range(len(counts) - 1):
        adv = item >= end[k]
        if mut == "empty_level_base" and counts[k] == 0:
            adv = np.zeros(item.shape, bool)
        lvl, base = np.where(adv, k + 1, lvl), np.where(adv, end[k], base)
    local = item - base
    div = 2 if mut == "quad_div_2" else qpp
    pix = local // div
    q = local - pix * div
    ok = (pix < np.asarray(counts, np.int64)[lvl]) & (q < qpp) & (pix >= 0)
    return lvl, pix, q, ok


def gather_seq32(rows, levels, C, act, mut=None):
    """The NumPy fp32 restatement of gather_forward_kernel over a level table: -> one (P_l, C) fp32 array per level (None for an empty
    level), prefilled with the sentinel."""
    n = len(rows)
    rows = np.ascontiguousarray(rows, f32)
    if mut == "clamp_to_n":
        rows = np.concatenate([rows, np.full((1, C), np.nan, f32)])
    counts = [0 if ids is None else len(ids) for ids in levels]
    out = [None if ids is None else np.full((len(ids), C), np.uint32(SENTINEL).view(f32)) for ids in levels]
    lvl, pix, q, ok = decode_items(counts, C, mut)
    for l, ids in enumerate(levels):
        m = ok & (lvl == l)
        if ids is None or not m.any():
            continue
        r = clamp(np.asarray(ids)[pix[m]], n, mut)
        col = 4 * q[m][:, None] + np.arange(4)[None]
        out[l][pix[m][:, None], col] = act32_seq(rows[r[:, None], col], act, mut)
    return out


# ------------------------------------------------------------------------------------------ the four-sample rule
def ss_axis(count, ss):
    """Output positions 0 .. count - 1 of an axis -> (i0, i1, l): the two source samples and the weight of the second."""
    s = (np.arange(count) + 0.5) * ss - 0.5
    i0 = np.floor(s).astype(np.int64)
    return i0, i0 + (i0 < count * ss - 1), s - i0


def _samples(S, h, w, ss, mut=None):
    """S (P, ss h, ss w, ...) -> [v00, v01, v10, v11], (ly, lx) shaped to broadcast."""
    y0, y1, ly = ss_axis(h, ss)
    x0, x1, lx = ss_axis(w, ss)
    tail = (1,) * (S.ndim - 3)
    if mut == "no_edge_clamp":
        # x0 + 1 read from the flat image, NaN past its end.  Since odd ss returns the centre sample, the clamp can no longer show in a
        # device OUTPUT: even ss never reaches the edge, odd ss discards the neighbours.  What the clamp still prevents is the read past
        # the end of the index image; this model keeps blending at ss = 1 and meets the NaN there, which stands for that read.
        P, sh, sw = S.shape[:3]
        flat = np.concatenate([S.reshape((P * sh * sw,) + S.shape[3:]), np.full((1,) + S.shape[3:], np.nan, S.dtype)])
        at = lambda ya, xa: flat[(np.arange(P)[:, None, None] * sh + ya[None, :, None]) * sw + xa[None, None, :]]       # noqa: E731
        v = [at(y0, x0), at(y0, x0 + 1), at(y1, x0), at(y1, x0 + 1)]
    else:
        v = [S[:, ya][:, :, xa] for ya in (y0, y1) for xa in (x0, x1)]
    if mut == "blend_reads_v00_twice":
        v[1] = v[0]
    return v, ly.reshape((1, h, 1) + tail), lx.reshape((1, 1, w) + tail)


def blend(S, h, w, ss, mut=None, centre_odd=True):
    """The blend in S's own precision and the kernel's order of operations (float64: the definition; float32: the restatement)."""
    v, ly, lx = _samples(S, h, w, ss, mut)
    if (ss & 1) and centre_odd and mut != "no_edge_clamp":
        return v[0].copy()
    t = S.dtype.type
    ly, lx = ly.astype(S.dtype), lx.astype(S.dtype)
    with np.errstate(all="ignore"):
        return (t(1) - ly) * ((t(1) - lx) * v[0] + lx * v[1]) + ly * ((t(1) - lx) * v[2] + lx * v[3])


def gather_ss_ref(rows, idx, ss, act):
    """idx (B, ss h, ss w) -> (out, cond, lead, bound) (B, h, w, C) float64."""
    B, sh, sw = idx.shape
    h, w = sh // ss, sw // ss
    y, cond_s, lead_s, bound_s, _ = gather_ref(rows, idx.reshape(-1), act)
    shp = (B, sh, sw, rows.shape[1])
    out, cond = blend(y.reshape(shp), h, w, ss), blend(cond_s.reshape(shp), h, w, ss)
    lead, bound = blend(lead_s.reshape(shp), h, w, ss), blend(bound_s.reshape(shp), h, w, ss)
    if ss & 1:
        return out, cond, lead, bound
    return out, cond, lead + 3 * U * cond, bound + SECOND_ORDER * 3 * U * cond + 3 * FLUSH


def interp_torch(S_nchw, ss):
    if ss == 1:
        return S_nchw.clone()
    return F.interpolate(S_nchw, scale_factor=1.0 / ss, mode="bilinear", align_corners=False)


def gather_ss_torch(rows, idx, ss, act, dtype=torch.float32):
    """torch: index_select, the activation, F.interpolate(scale_factor = 1 / ss) -> (B, h, w, C).  A table with non-finite rows (odd ss
    only) takes the centre samples by a strided slice instead: interpolate multiplies the neighbours by 0, and 0 inf = NaN is not the
    definition."""
    B, sh, sw = idx.shape
    t = torch.index_select(torch.from_numpy(np.ascontiguousarray(rows)).to(dtype), 0, torch.from_numpy(clamp(idx.reshape(-1), len(rows))))
    t = torch.sigmoid(t) if act == "sigmoid" else torch.tanh(t) if act == "tanh" else t
    if not np.isfinite(rows).all():
        assert ss & 1, "non-finite rows have no place in the blends of even ss"
        return t.reshape(B, sh, sw, -1)[:, (ss - 1) // 2::ss, (ss - 1) // 2::ss].contiguous().numpy()
    return interp_torch(t.reshape(B, sh, sw, -1).permute(0, 3, 1, 2), ss).permute(0, 2, 3, 1).contiguous().numpy()


def gather_ss_seq32(rows, idx, ss, act, mut=None):
    B, sh, sw = idx.shape
    rows = np.ascontiguousarray(rows, f32)
    x = rows[clamp(idx.reshape(-1), len(rows))].reshape(B, sh, sw, -1)
    if mut == "act_after_blend":
        return act32_seq(blend(x, sh // ss, sw // ss, ss), act)
    return blend(act32_seq(x, act), sh // ss, sw // ss, ss, mut).astype(f32)


def down_ref(x, ss):
    """read_bilinear_down: x (planes, ss h, ss w) -> (out, cond, bound) float64."""
    P, sh, sw = x.shape
    x64 = np.asarray(x, np.float64)
    out, cond = blend(x64, sh // ss, sw // ss, ss), blend(np.abs(x64), sh // ss, sw // ss, ss)
    return out, cond, np.zeros(out.shape) if ss & 1 else SECOND_ORDER * 3 * U * cond + 3 * FLUSH


def down_seq32(x, ss, mut=None):
    P, sh, sw = x.shape
    return blend(np.ascontiguousarray(x, f32), sh // ss, sw // ss, ss, mut, centre_odd=False).astype(f32)


def down_torch(x, ss, dtype=torch.float32):
    return interp_torch(torch.from_numpy(np.ascontiguousarray(x)).to(dtype)[None], ss)[0].numpy()


def down_backward_ref(dout, ss, dtype=np.float64):
    """The transpose: dout (planes, h, w) -> din (planes, ss h, ss w).  For ss >= 2 the footprints are disjoint."""
    P, h, w = dout.shape
    y0, y1, ly = ss_axis(h, ss)
    x0, x1, lx = ss_axis(w, ss)
    d = np.asarray(dout, dtype)
    din = np.zeros((P, h * ss, w * ss), dtype)
    for ya, wy in ((y0, 1 - ly), (y1, ly)):
        for xa, wx in ((x0, 1 - lx), (x1, lx)):
            wgt = (wy[:, None] * wx[None, :]).astype(dtype)
            cur = din[:, ya[:, None], xa[None, :]]
            din[:, ya[:, None], xa[None, :]] = cur + np.where(wgt != 0, wgt * d, 0).astype(dtype)
    return din


def down_backward_torch(dout, ss, dtype=torch.float32):
    P, h, w = dout.shape
    t = torch.zeros((1, P, h * ss, w * ss), dtype=dtype, requires_grad=True)
    (interp_torch(t, ss) * torch.from_numpy(np.ascontiguousarray(dout)).to(dtype)[None]).sum().backward()
    return t.grad[0].numpy()


def down_backward_footprint(h, w, ss):
    """-> bool (ss h, ss w): the samples that receive a gradient (the 2 x 2 footprints of even ss, the centres of odd ss)."""
    y0, y1, ly = ss_axis(h, ss)
    x0, x1, lx = ss_axis(w, ss)
    my, mx = np.zeros(h * ss, bool), np.zeros(w * ss, bool)
    my[y0], mx[x0] = True, True
    if not ss & 1:
        my[y1], mx[x1] = True, True
    return my[:, None] & mx[None, :]


# ------------------------------------------------------------------------------------------ the scatter-add
def scatter_ref(n, C, levels, grads, dtype=np.float64, mut=None):
    """levels: ids per level (None = empty), grads: (P_l, C) per level -> (drows (n, C), hits (n,), mass (n, C)).  dtype float32: the
    restatement, collisions summed in pixel order."""
    acc, mass, hits = np.zeros((n, C), dtype), np.zeros((n, C)), np.zeros(n, np.int64)
    for ids, g in zip(levels, grads):
        if ids is None:
            continue
        r = clamp(ids, n, mut if mut == "negative_wrap" else None)
        np.add.at(acc, r, np.asarray(g).astype(dtype))
        np.add.at(mass, r, np.abs(np.asarray(g, np.float64)))
        hits += np.bincount(r, minlength=n)
    return acc, hits, mass


def scatter_bound(hits, mass):
    k = np.asarray(hits, np.float64)[:, None]
    return np.where(k > 0, np.expm1(np.maximum(k - 1, 0) * np.log1p(U)) * mass * SECOND_ORDER + k * FLUSH, 0.0)


def scatter_lead(hits, mass):
    """The leading term (k - 1) u sum |g|: the cap of a row whose atomics happened to commit in a less lucky order than the pixel order
    both yardsticks sum in (`raised`)."""
    return np.maximum(np.asarray(hits, np.float64)[:, None] - 1, 0) * U * mass


def scatter_torch32(n, C, levels, grads):
    acc = torch.zeros((n, C))
    for ids, g in zip(levels, grads):
        if ids is not None:
            acc.index_add_(0, torch.from_numpy(clamp(ids, n)), torch.from_numpy(np.ascontiguousarray(g, f32)))
    return acc.numpy()


# ------------------------------------------------------------------------------------------ stitch
def stitch_ref(parts, visible=None):
    """parts: [(rows (n_s, C), idx_levels, depth_levels, id_base, act)], idx / depth flat per level (None = empty level) ->
    (idx, depth, part, y, bound, lead) per level through stitch_model.merge; empty levels are None."""
    from tests import stitch_model as sm
    levels = len(parts[0][1])
    live = [l for l in range(levels) if parts[0][1][l] is not None]
    mi, md, mp, ml = sm.merge([([p[1][l] for l in live], [p[2][l] for l in live], p[3]) for p in parts], visible)
    out = [None] * levels
    for j, l in enumerate(live):
        C = parts[0][0].shape[1]
        y, lead, bound = np.zeros((len(mp[j]), C)), np.zeros((len(mp[j]), C)), np.zeros((len(mp[j]), C))
        src = np.where(mp[j] == 255, 0, mp[j])
        for s, p in enumerate(parts):
            m = src == s
            y[m], _, lead[m], bound[m], _ = gather_ref(p[0], ml[j][m], p[4])
        out[l] = (mi[j], md[j], mp[j], y, bound, lead)
    return out


# ------------------------------------------------------------------------------------------ the measure
def raised_explanations():
    """The `family (class)` keys profiles/gather_accuracy_fp64.md explains."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "gather_accuracy_fp64.md")
    if not os.path.exists(path):
        return set()
    with open(path) as f:
        return set(re.findall(r"^- raised `([^`]+)`: \S", f.read(), re.M))


FAILED = []                # every row of a test is measured and printed before the test fails on the rows that missed an assertion
ROWS = []                  # (family, cls, name, e_max, e_rms, rt, rs, q, raised) of every judged row, for the profile table


def judge(family, cls, name, got, ref, cond, bound, yard, lead=None, extra="", prefix="GACC|", failed=None, quiet=False):
    """One table line and the assertions of rules 1 and 2 (module docstring).  got must be finite: NaN outputs that a NaN input
    demands are checked and zeroed by the caller (`split_nan`)."""
    failed = FAILED if failed is None else failed
    got = np.asarray(got, np.float64)
    finite = bool(np.isfinite(got).all())
    err = np.abs(np.nan_to_num(got, nan=3e38, posinf=3e38, neginf=-3e38) - ref)
    q = worst(err, bound)
    meas = lambda e: stats(np.where(e <= MEASURE_FLOOR, 0.0, e), cond) if np.size(e) else (0.0, 0.0)      # noqa: E731
    e_max, e_rms = meas(err)
    R = {k: meas(np.abs(np.asarray(v, np.float64) - ref)) for k, v in yard.items()}
    rt, rs = R.get("torch", (float("nan"),) * 2), R.get("seq", (float("nan"),) * 2)
    fin = [r for r in R.values() if np.isfinite(r[0])]
    cap_max = 2 * max([r[0] for r in fin] + [1.0])
    cap_rms = 2 * max([r[1] for r in fin] + [0.5])
    raised = False
    if lead is not None and not (e_max <= cap_max and e_rms <= cap_rms):
        l_max, l_rms = stats(lead, cond) if np.size(lead) else (0.0, 0.0)
        cap_max, cap_rms, raised = max(cap_max, l_max), max(cap_rms, l_rms), True
    if not quiet:
        print("%s %-14s | %s | %-52s | E_max %9.2f | E_rms %8.3f | R_torch max %8.2f rms %7.3f | R_seq max %8.2f rms %7.3f | err/bound %6.3f |%s%s" % (
            prefix, family, cls, name, e_max, e_rms, rt[0], rt[1], rs[0], rs[1], q, " raised |" if raised else "", extra))
    ROWS.append((family, cls, name, e_max, e_rms, rt, rs, q, raised))
    what = f"{family} ({cls}) {name}"
    if not finite:
        failed.append(f"{what}: non-finite output where the inputs are finite")
    if not q <= 1.0:
        failed.append(f"{what}: {q:.3f} x the derived bound (E_max {e_max:.1f}, E_rms {e_rms:.2f})")
    if not (e_max <= cap_max and e_rms <= cap_rms):
        failed.append(f"{what}: E_max {e_max:.2f} E_rms {e_rms:.3f} against the caps {cap_max:.2f} / {cap_rms:.3f}")
    if raised and f"{family} ({cls})" not in raised_explanations():
        failed.append(f"{what}: raised, and profiles/gather_accuracy_fp64.md has no line explaining `{family} ({cls})`")
    return e_max, e_rms


def finish(failed=None):
    failed = FAILED if failed is None else failed
    msgs = list(failed)
    del failed[:]
    assert not msgs, "%d rows failed:\n" % len(msgs) + "\n".join(msgs)


def sentinel_free(a):
    return not (bits(a) == np.uint32(SENTINEL)).any()


# ------------------------------------------------------------------------------------------ the case set: values
SUBNORMAL = 2.0 ** -140
EDGE = np.array([0.0, -0.0, SUBNORMAL, -SUBNORMAL, 1e-4, -1e-4, 1e-2, -1e-2, 9, -9, 17, -17, 88.7, -88.7, 88.8, -88.8, 104, -104, 1e30, -1e30,
                 np.inf, -np.inf, np.nan], f32)
EDGE_FINITE = EDGE[:20]
NAN_PAYLOAD = 0x7FC12345


def value_rows(cls, n, C, rng):
    """(a) unit scale; (b) per-channel scales 2^U(-8, 6) (train_ref64.scales_b); (d) the domain edge: row r holds EDGE[(r + c) % 23] in
    channel c, so every row meets every value ("df": the 20 finite values only, for the blends)."""
    if cls == "a":
        return rng.standard_normal((n, C)).astype(f32)
    if cls == "b":
        return (rng.standard_normal((n, C)) * scales_b(C, rng)[None]).astype(f32)
    vals = EDGE if cls == "d" else EDGE_FINITE
    rows = vals[(np.arange(n)[:, None] + np.arange(C)[None]) % len(vals)].copy()
    rows.view(np.uint32)[np.isnan(rows)] = NAN_PAYLOAD
    return rows


def required_ids(n):
    return [0, n - 1, -1, -2 ** 31, n, 2 ** 31 - 1]


def level_ids(P, n, rng, k=0, hot=None):
    """The ids of one level of P pixels over a table of n rows: the six required ids (a level of fewer than six pixels takes as many as
    fit, starting at the k-th, so that the levels of a table cover them between them), random rows elsewhere; hot = every pixel that
    is not a required id addresses this row (the background id)."""
    if P == 0:
        return None
    req = required_ids(n)
    req = (req[k % 6:] + req[:k % 6])[:min(P, 6)]
    rest = np.full(P - len(req), hot, np.int64) if hot is not None else rng.integers(0, n, P - len(req))
    return rng.permutation(np.concatenate([np.asarray(req, np.int64), rest])).astype(np.int32)


CHANNELS = (4, 8, 12, 20, 64)
TABLE_N = (1, 2, 257)
LEVEL_TABLES = {"one": (37,), "7-0-1-130-3": (7, 0, 1, 130, 3), "0-5-0-0-9": (0, 5, 0, 0, 9), "64-64-0-0-0": (64, 64, 0, 0, 0)}
BIG_N = 2 ** 20 + 3
GRID_STRIDE = {"C64 part of the grid": (64, (32768 + 37,)), "C8 second trip": (8, (262144 + 5,)),
               "C12 boundary inside a pixel": (12, (100000, 74762, 50))}
assert (100000 + 74762) * 3 < GRID_ITEMS < (100000 + 74762) * 3 + 3          # item 524 288 is the third quad of pixel 0 of level 2


def _stable(s):
    return sum((i + 1) * ord(c) for i, c in enumerate(s)) % (2 ** 31)


def gather_cases(which="small"):
    """-> dicts name, cls, C, n, rows, levels (ids per level or None), act.  small: every C x n x level table x activation in class (a),
    every C x activation in classes (b) and (d); grid: the three grid-stride launches."""
    if which == "grid":
        for name, (C, counts) in GRID_STRIDE.items():
            rng = np.random.default_rng([7, C])
            rows = value_rows("a", 257, C, rng)
            yield dict(name=name, cls="a", C=C, n=257, rows=rows, levels=[level_ids(P, 257, rng, k) for k, P in enumerate(counts)],
                       act="tanh" if C == 12 else "none")
        return
    for C in CHANNELS:
        for tname, counts in LEVEL_TABLES.items():
            for n in TABLE_N:
                for act in ACTS:
                    rng = np.random.default_rng([1, C, n, _stable(tname), _stable(act)])
                    yield dict(name=f"C{C} n{n} levels {tname} {act}", cls="a", C=C, n=n, rows=value_rows("a", n, C, rng),
                               levels=[level_ids(P, n, rng, k) for k, P in enumerate(counts)], act=act)
        for cls in "bd":
            for act in ACTS:
                rng = np.random.default_rng([2, C, _stable(cls), _stable(act)])
                n = 257 if cls == "b" else len(EDGE)
                yield dict(name=f"C{C} n{n} levels 7-0-1-130-3 {act}", cls=cls, C=C, n=n, rows=value_rows(cls, n, C, rng),
                           levels=[level_ids(P, n, rng, k) for k, P in enumerate(LEVEL_TABLES["7-0-1-130-3"])], act=act)


def big_table_case():
    """n = 2^20 + 3 rows of C = 64 (a 268 MB table nobody materialises on the host: on the device it is one uninitialised allocation,
    and a zeroed one for the scatter-add): the case carries the addressed rows only.  The largest element offset is 2^26 floats =
    2^28 bytes: the case shows that ids above 2^20 address their rows, NOT that the row offset is formed in 64 bits (that would take
    a table of 8 GB).
    -> (n, C, ids, {row: values})."""
    rng = np.random.default_rng(9)
    n, C = BIG_N, 64
    ids = np.concatenate([required_ids(n), n - 1 - rng.integers(0, 40, 58)]).astype(np.int64)
    ids = rng.permutation(ids).astype(np.int32)
    addressed = np.unique(clamp(ids, n))
    return n, C, ids, {int(r): rng.standard_normal(C).astype(f32) for r in addressed}


SS_SIZES = ((1, 1), (1, 9), (9, 1), (5, 7))
SS_ALL = (1, 2, 3, 4, 5, 6, 7, 8)


def ss_cases(which="small"):
    """-> dicts name, cls, C, n, rows, B, ss, sizes [(h, w) per level], idx [(B, ss h, ss w) per level], act.  Two levels of different
    aspect per launch.  Class (d): at odd ss (ss = 1 included) the whole domain-edge table, +-inf and NaN with its payload among the
    centre samples and among their neighbours: the output is the activated centre sample whatever the neighbours hold.  At even ss
    the 20 finite edge values only: a non-finite sample has no place in a blend (inf - inf, 0 inf = NaN)."""
    if which == "grid":
        rng = np.random.default_rng(17)
        C, n, B, ss, sizes = 64, 257, 1, 2, [(129, 255)]
        yield dict(name="C64 129x255 ss2 second trip", cls="a", C=C, n=n, rows=value_rows("a", n, C, rng), B=B, ss=ss, sizes=sizes,
                   idx=[rng.integers(-1, n + 1, (B, ss * h, ss * w)).astype(np.int32) for h, w in sizes], act="sigmoid")
        return
    pairs = (((1, 1), (1, 9)), ((9, 1), (5, 7)))
    for ss in SS_ALL:
        for B in (1, 3):
            for k, sizes in enumerate(pairs):
                for act in ACTS:
                    for cls in ("a", "b", "d" if ss & 1 else "df"):
                        C = CHANNELS[(ss + B + k + ACTS.index(act)) % len(CHANNELS)]
                        if cls != "a" and (B, k) != (3, 1):
                            continue
                        rng = np.random.default_rng([3, ss, B, k, _stable(act), _stable(cls)])
                        n = 257 if cls in "ab" else len(EDGE) if cls == "d" else len(EDGE_FINITE)
                        idx = [rng.integers(-1, n + 1, (B, ss * h, ss * w)).astype(np.int32) for h, w in sizes]
                        yield dict(name=f"ss{ss} B{B} C{C} {sizes[0][0]}x{sizes[0][1]}+{sizes[1][0]}x{sizes[1][1]} {act}", cls=cls[0], C=C, n=n,
                                   rows=value_rows(cls, n, C, rng), B=B, ss=ss, sizes=list(sizes), idx=idx, act=act)


def down_cases(which="small"):
    """read_bilinear_down and its adjoint: -> dicts name, cls, ss, x (planes, ss h, ss w), dout (planes, h, w)."""
    if which == "grid":
        rng = np.random.default_rng(19)
        yield dict(name="forward 3x419x418 ss2 second trip", cls="a", ss=2, x=rng.standard_normal((3, 838, 836)).astype(f32), dout=None)
        yield dict(name="adjoint 1x363x362 ss2 second trip", cls="a", ss=2, x=None, dout=rng.standard_normal((1, 363, 362)).astype(f32))
        return
    for ss in SS_ALL[1:]:
        for planes in (1, 3):
            for (h, w) in SS_SIZES:
                for cls in "ab":
                    rng = np.random.default_rng([4, ss, planes, h, w, _stable(cls)])
                    sc = scales_b(planes, rng)[:, None, None] if cls == "b" else 1.0
                    yield dict(name=f"ss{ss} planes {planes} {h}x{w}", cls=cls, ss=ss, x=(rng.standard_normal((planes, ss * h, ss * w)) * sc).astype(f32),
                               dout=(rng.standard_normal((planes, h, w)) * sc).astype(f32))


HITS = (1, 2, 64, 65, 4096)


def scatter_cases(which="small"):
    """-> dicts name, cls, C, n, levels, grads.  hits: rows 1..5 of n = 257 are hit 1, 2, 64, 65 and 4096 times, the clamped ids land on
    rows 0 and n - 1, every other row stays untouched; background: one row hit by every pixel of every level; the level tables at
    every C; grid: the three grid-stride launches."""
    def grads(levels, C, cls, rng):
        sc = scales_b(C, rng)[None] if cls == "b" else 1.0
        return [None if ids is None else (rng.standard_normal((len(ids), C)) * sc).astype(f32) for ids in levels]
    if which == "grid":
        for name, (C, counts) in GRID_STRIDE.items():
            rng = np.random.default_rng([8, C])
            levels = [level_ids(P, 257, rng, k) for k, P in enumerate(counts)]
            yield dict(name=name, cls="a", C=C, n=257, levels=levels, grads=grads(levels, C, "a", rng))
        return
    for cls in "ab":
        for C in (8, 20):
            rng = np.random.default_rng([5, C, _stable(cls)])
            n = 257
            ids = np.concatenate([np.full(k, r + 1) for r, k in enumerate(HITS)] + [[-1, -2 ** 31, -7], [n, 2 ** 31 - 1]]).astype(np.int64)
            ids = rng.permutation(ids).astype(np.int32)
            cut = (len(ids) // 3, 2 * len(ids) // 3)
            levels = [ids[:cut[0]], None, ids[cut[0]:cut[1]], ids[cut[1]:]]
            yield dict(name=f"hits 1/2/64/65/4096 C{C}", cls=cls, C=C, n=n, levels=levels, grads=grads(levels, C, cls, rng))
        rng = np.random.default_rng([6, _stable(cls)])
        levels = [level_ids(P, 257, rng, k, hot=0) for k, P in enumerate(LEVEL_TABLES["7-0-1-130-3"])]
        yield dict(name="background id 0 C12", cls=cls, C=12, n=257, levels=levels, grads=grads(levels, 12, cls, rng))
    for C in CHANNELS:
        for tname, counts in LEVEL_TABLES.items():
            for n in TABLE_N:
                rng = np.random.default_rng([10, C, n, _stable(tname)])
                levels = [level_ids(P, n, rng, k) for k, P in enumerate(counts)]
                yield dict(name=f"C{C} n{n} levels {tname}", cls="a", C=C, n=n, levels=levels, grads=grads(levels, C, "a", rng))


EIGHT_SIZES = (3, 1, 4, 1, 5, 9, 2, 6)
EIGHT_BASES = (0, 3, 6, 10, 11, 20, 29, 40)
EIGHT_ACTS = ("none", "sigmoid", "tanh", "none", "tanh", "sigmoid", "none", "tanh")


def table_cases():
    """joint_texture_model's layouts at C = 12 and 64, the eight-table launch, a level table with empty levels, one grid-stride launch:
    -> dicts name, C, sizes, bases, acts, tables [(n_t, C)], levels (flat ids or None), d (gradients per level)."""
    def make(name, C, sizes, bases, acts, levels, rng):
        tables = [rng.standard_normal((n, C)).astype(f32) for n in sizes]
        d = [None if ids is None else rng.standard_normal((len(ids), C)).astype(f32) for ids in levels]
        return dict(name=name, C=C, sizes=tuple(sizes), bases=tuple(bases), acts=tuple(acts), tables=tables, levels=levels, d=d)
    for C in (12, 64):
        for layout, bases in jm.LAYOUTS.items():
            for aname, acts in jm.ACTS.items():
                rng = np.random.default_rng([12, C, len(layout), len(aname)])
                yield make(f"C{C} {layout} {aname}", C, jm.SIZES, bases, acts, [m.reshape(-1) for m in jm.draw_ids(bases, rng)], rng)
    rng = np.random.default_rng(13)
    fixed, end8 = jm.required_ids(EIGHT_BASES, EIGHT_SIZES), EIGHT_BASES[-1] + EIGHT_SIZES[-1]
    ids = [rng.permutation(np.concatenate([fixed, [EIGHT_BASES[2] + 1] * hot, rng.integers(-1, end8 + 2, P - len(fixed) - hot)])).astype(np.int32)
           for P, hot in ((96, jm.HOT_HITS), (40, 0))]
    yield make("C12 eight tables", 12, EIGHT_SIZES, EIGHT_BASES, EIGHT_ACTS, ids, rng)
    end = jm.LAYOUTS["gapped"][-1] + jm.SIZES[-1]
    lv = [None if P == 0 else np.concatenate([jm.required_ids(jm.LAYOUTS["gapped"])[:P], rng.integers(-1, end + 2, max(P - 11, 0))]).astype(np.int32)
          for P in LEVEL_TABLES["7-0-1-130-3"]]
    yield make("C20 gapped mixed levels 7-0-1-130-3", 20, jm.SIZES, jm.LAYOUTS["gapped"], jm.ACTS["mixed"], lv, rng)
    C, counts = GRID_STRIDE["C12 boundary inside a pixel"]
    yield make("C12 gapped mixed, boundary inside a pixel", C, jm.SIZES, jm.LAYOUTS["gapped"], jm.ACTS["mixed"],
               [rng.integers(-1, end + 2, P).astype(np.int32) for P in counts], rng)


def stitch_cases():
    """-> dicts name, C, counts, parts [(rows, idx_levels, depth_levels, id_base, act)], visible, want_feat.  Depths from a set of eight
    values, so ties are everywhere; about a third of the candidates are the empty pattern; local ids stay inside their tables."""
    def make(name, C, S, counts, seed, want_feat=True, hidden=()):
        rng = np.random.default_rng([14, seed])
        sizes = [int(rng.integers(1, 40)) for _ in range(S)]
        parts, base = [], 0
        for s in range(S):
            idx, dep = [], []
            for P in counts:
                if P == 0:
                    idx.append(None), dep.append(None)
                    continue
                i = rng.integers(0, sizes[s], P).astype(np.int32)
                d = (rng.integers(1, 9, P) * 0.25).astype(f32)
                empty = rng.random(P) < 0.35
                i[empty], d[empty] = 0, 0.0
                idx.append(i), dep.append(d)
            parts.append((rng.standard_normal((sizes[s], C)).astype(f32), idx, dep, base, ACTS[(s + seed) % 3]))
            base += sizes[s]
        return dict(name=name, C=C, counts=tuple(counts), parts=parts, visible=[s not in hidden for s in range(S)], want_feat=want_feat)
    yield make("C12 three parts", 12, 3, LEVEL_TABLES["7-0-1-130-3"], 1)
    yield make("C64 three parts, part 1 hidden", 64, 3, LEVEL_TABLES["0-5-0-0-9"], 2, hidden=(1,))
    yield make("C12 eight parts", 12, 8, LEVEL_TABLES["7-0-1-130-3"], 3)
    yield make("C64 one part", 64, 1, LEVEL_TABLES["64-64-0-0-0"], 4)
    yield make("C8 three parts, no features (one lane per pixel)", 8, 3, LEVEL_TABLES["7-0-1-130-3"], 5, want_feat=False)
    yield make("C12 two parts, boundary inside a pixel", 12, 2, GRID_STRIDE["C12 boundary inside a pixel"][1], 6)


# ------------------------------------------------------------------------------------------ the layout change
def transpose_cases():
    for n in (1, 255, 256, 257):
        for C in (4, 12, 64):
            rng = np.random.default_rng([15, n, C])
            tex = rng.standard_normal((C, n)).astype(f32)
            tex.reshape(-1)[:len(EDGE)] = EDGE[:tex.size]
            tex.view(np.uint32)[np.isnan(tex)] = NAN_PAYLOAD
            yield dict(name=f"n{n} C{C}", n=n, C=C, tex=tex)


def rows_to_texture_seq(rows, mut=None):
    tex = np.ascontiguousarray(np.asarray(rows, f32).T)
    if mut == "swap_channels" and tex.shape[0] == 12:
        tex[[5, 6]] = tex[[6, 5]]
    return tex


# ------------------------------------------------------------------------------------------ a launch's reference, bounds and yardsticks
def cat(levels):
    """Per-level arrays (None = empty level) -> one (sum P_l, C) array."""
    return np.concatenate([np.asarray(x).reshape(-1, np.asarray(x).shape[-1]) for x in levels if x is not None])


def clean(what, got, ref, failed=None):
    """Where the reference is not finite (NaN in, NaN out; act none hands +-inf through) the output must be the same non-finite value;
    those entries are then zeroed in both.  -> (got, ref) float64."""
    failed = FAILED if failed is None else failed
    got, ref = np.array(got, np.float64), np.array(ref, np.float64)
    odd = ~np.isfinite(ref)
    if not np.array_equal(got[odd], ref[odd], equal_nan=True) or np.isnan(got[~odd]).any():
        failed.append(f"{what}: non-finite outputs do not coincide with the non-finite values the definition hands through")
    got[odd | np.isnan(got)], ref[odd] = 0, 0
    return got, ref


def gather_launch(case, mut=None):
    """The plain gather of one case: ref, cond, lead, bound, want_bits (act none), yardsticks as thunks."""
    ids = np.concatenate([i for i in case["levels"] if i is not None])
    y, cond, lead, bound, x = gather_ref(case["rows"], ids, case["act"])
    want = bits(np.asarray(case["rows"], f32)[clamp(ids, case["n"])]) if case["act"] == "none" else None
    return dict(ref=y, cond=cond, lead=lead if case["act"] != "none" else None, bound=bound, want_bits=want,
                torch=lambda: gather_torch32(case["rows"], ids, case["act"]),
                seq=lambda m=None: cat(gather_seq32(case["rows"], case["levels"], case["C"], case["act"], m)))


def ss_launch(case):
    refs = [gather_ss_ref(case["rows"], idx, case["ss"], case["act"]) for idx in case["idx"]]
    ref, cond, lead, bound = (cat([r[k] for r in refs]) for k in range(4))
    centre = None
    if case["ss"] & 1:                                   # the activated centre sample; at ss = 1 the plain gather of the same ids
        centre = [idx[:, (case["ss"] - 1) // 2::case["ss"], (case["ss"] - 1) // 2::case["ss"]] for idx in case["idx"]]
    return dict(ref=ref, cond=cond, lead=lead, bound=bound, centre_ids=centre,
                torch=lambda: cat([gather_ss_torch(case["rows"], idx, case["ss"], case["act"]) for idx in case["idx"]]),
                seq=lambda m=None: cat([gather_ss_seq32(case["rows"], idx, case["ss"], case["act"], m) for idx in case["idx"]]))


def scatter_launch(case):
    ref, hits, mass = scatter_ref(case["n"], case["C"], case["levels"], case["grads"])
    return dict(ref=ref, cond=mass, lead=scatter_lead(hits, mass), bound=scatter_bound(hits, mass), hits=hits,
                torch=lambda: scatter_torch32(case["n"], case["C"], case["levels"], case["grads"]),
                seq=lambda m=None: scatter_seq32(case, m))


def scatter_seq32(case, mut=None):
    levels, grads = case["levels"], case["grads"]
    if mut == "drop_one_addend":                         # the first pixel that addresses the 4096-fold row is skipped
        hot = 1 + HITS.index(4096)
        l = next(k for k, ids in enumerate(levels) if ids is not None and (ids == hot).any())
        keep = np.ones(len(levels[l]), bool)
        keep[np.nonzero(levels[l] == hot)[0][0]] = False
        levels = [ids[keep] if k == l else ids for k, ids in enumerate(levels)]
        grads = [g[keep] if k == l else g for k, g in enumerate(grads)]
    acc = scatter_ref(case["n"], case["C"], levels, grads, f32, mut)[0]
    if mut == "untouched_row_nonzero":
        acc[np.nonzero(scatter_ref(case["n"], case["C"], levels, grads)[1] == 0)[0][:1]] = f32(1e-30)
    return acc


def table_select(case, ids):
    return jm.select(ids, case["bases"], case["sizes"])


def tables_forward_launch(case):
    ids = np.concatenate([i for i in case["levels"] if i is not None])
    t, local = table_select(case, ids)
    C = case["C"]
    x = np.zeros((len(ids), C))
    lead, bound = np.zeros((len(ids), C)), np.zeros((len(ids), C))
    seq, tor = np.zeros((len(ids), C), f32), np.zeros((len(ids), C), f32)
    for s, (rows, act) in enumerate(zip(case["tables"], case["acts"])):
        m = t == s
        x[m] = rows[local[m]]
        lead[m], bound[m] = act_bound(x[m], act)
        seq[m], tor[m] = act32_seq(rows[local[m]], act), act32_torch(rows[local[m]], act)
    y = jm.forward(ids, case["tables"], case["bases"], case["acts"])
    plain = np.array([a == "none" for a in case["acts"]])[t]
    return dict(ref=y, cond=np.abs(y), lead=lead, bound=bound, plain=plain, want_bits=bits(x.astype(f32)), ids=ids, torch=lambda: tor, seq=lambda m=None: seq)


def tables_backward_launch(case, y, mut=None):
    """y (P, C) fp32: the forward output the adjoint reads (the device's own on the GPU).  -> pairs and dense bundles."""
    ids = np.concatenate([i for i in case["levels"] if i is not None])
    d = cat(case["d"])
    t, local = table_select(case, ids)
    g, gb, gc = np.zeros(d.shape), np.zeros(d.shape), np.zeros(d.shape)
    seq, tor = np.zeros(d.shape, f32), np.zeros(d.shape, f32)
    for s, act in enumerate(case["acts"]):
        m = t == s
        g[m], gb[m] = slope_bound(d[m], y[m], act)
        y64 = np.asarray(y[m], np.float64)               # cond: the summands of the slope by absolute value: 1 - y y -> 1 + y y, y - y y -> |y| + y y
        gc[m] = np.abs(d[m]) * (1.0 if act == "none" else np.abs(y64) + y64 * y64 if act == "sigmoid" else 1 + y64 * y64)
        seq[m] = slope32_seq(d[m], y[m], act, mut)
        dt, yt = torch.from_numpy(np.ascontiguousarray(d[m], f32)), torch.from_numpy(np.ascontiguousarray(y[m], f32))
        tor[m] = (torch.ops.aten.sigmoid_backward(dt, yt) if act == "sigmoid" else torch.ops.aten.tanh_backward(dt, yt) if act == "tanh" else dt).numpy()
    assert np.array_equal(g, jm.adjoint_pairs(ids, d, y, case["bases"], case["sizes"], case["acts"]))
    pairs = dict(ref=g, cond=gc, lead=None, bound=gb, plain=np.array([a == "none" for a in case["acts"]])[t], torch=lambda: tor, seq=lambda m=None: seq)
    drows, hits, mass = jm.adjoint_dense(ids, d, y, case["bases"], case["sizes"], case["acts"])
    dense = []
    for s, n in enumerate(case["sizes"]):
        m = t == s
        carried = np.zeros((n, d.shape[1]))
        np.add.at(carried, local[m], gb[m])
        dense.append(dict(ref=drows[s], cond=mass[s], lead=scatter_lead(hits[s], mass[s]) + carried, bound=scatter_bound(hits[s], mass[s]) + carried, hits=hits[s],
                          torch=lambda m=m, n=n: scatter_torch32(n, d.shape[1], [local[m]], [tor[m]]),
                          seq=lambda _=None, m=m, n=n: scatter_ref(n, d.shape[1], [local[m]], [seq[m]], f32)[0]))
    return pairs, dense


def run_judge(family, case, got, L, name=None, yard_mut=None, failed=None, quiet=False, against=("torch", "seq")):
    """Judge `got` against the launch bundle L: non-finite hand-through, sentinel, rules 1 and 2."""
    failed = FAILED if failed is None else failed
    name = case["name"] if name is None else name
    what = f"{family} ({case['cls'] if 'cls' in case else 'a'}) {name}"
    if not sentinel_free(got):
        failed.append(f"{what}: the sentinel survives inside the output buffer")
    got, ref = clean(what, got, L["ref"], failed)
    yard = {k: np.nan_to_num(np.asarray(L[k](), np.float64), nan=0.0, posinf=0.0, neginf=0.0) * np.isfinite(L["ref"]) for k in against}
    return judge(family, case.get("cls", "a"), name, got, ref, L["cond"], L["bound"], yard, lead=L["lead"], failed=failed, quiet=quiet)
