"""NumPy fp32 restatements of the training kernels (read_amd/csrc/train.hip) in the kernels' own order of operations, without fused
multiply-adds: the gate / BatchNorm chain (modes 0 / 1 / 2, bn_bwd_coeff, bn_stats in fp64, bn_finalize, bn_apply) and both
weight-gradient kernels; and of the forward's linear launches on the three fp32 convolution kernels of read_amd/csrc/conv.hip with the
Winograd kernels' fused gate (linear_launch32, which can also carry one seeded defect: MUTATIONS).  tests/test_train_accuracy_cpu.py
holds them to the derived bounds of tests/train_ref64.py; tests/test_gpu_train_accuracy.py and tests/test_gpu_train_forward_accuracy.py
use them, summing sequentially, as the yardstick R_seq."""
import numpy as np

from tests import train_ref64 as T

f32 = np.float32


# ------------------------------------------------------------------------------------------ fp32 restatements
def fast_exp32(x):
    with np.errstate(over="ignore", under="ignore"):
        return np.exp2((x * T.LOG2E32).astype(f32).astype(np.float64)).astype(f32)


def gate32(fm, C, elu):
    f, m = fm[:, :C], fm[:, C:2 * C]
    with np.errstate(over="ignore", invalid="ignore"):
        a = np.where(f > 0, f, fast_exp32(np.minimum(f, f32(0))) - f32(1)).astype(f32) if elu else f
        da = np.where(f > 0, f32(1), a + f32(1)).astype(f32) if elu else np.ones_like(f)
        s = (1.0 / (f32(1) + fast_exp32(-m)).astype(np.float64)).astype(f32)
    return a, da, s


# ------------------------------------------------------------------------------------------ the forward's linear launches
def conv_direct32(x_chw, w, stride, drop=()):
    """The convolution WITHOUT its bias as a sequential fp32 sum over (tap, channel): one rounded product and one rounded addition per
    term — the direct kernel's arithmetic in one of the orders the MFMAs may take, and the yardstick R_seq.  drop: channels left out
    (the mutation catalogue).  -> (Cout, outH, outW) float32."""
    cout, cin, k, _ = w.shape
    pad = (k - 1) // 2
    H, W = x_chw.shape[1:]
    oh, ow = T.out_hw(k, stride, H, W)
    xp = np.zeros((cin, H + 2 * pad + k, W + 2 * pad + k), f32)
    xp[:, pad:pad + H, pad:pad + W] = x_chw
    acc = np.zeros((cout, oh, ow), f32)
    for ky in range(k):
        for kx in range(k):
            win = xp[:, ky:ky + stride * oh:stride, kx:kx + stride * ow:stride]
            for c in range(cin):
                if c not in drop:
                    acc = acc + w[:, c, ky, kx][:, None, None] * win[c][None]
    return acc


def _at4(a):
    """The output transform of gated_conv_wino4_kernel along axis 0 (conv.hip: s1, d1, s2, d2, R[0] = acc + s1 + s2, ...)."""
    s1, d1, s2, d2 = a[1] + a[2], a[1] - a[2], a[3] + a[4], a[3] - a[4]
    return np.stack([(a[0] + s1) + s2, d1 + f32(2) * d2, s1 + f32(4) * s2, (d1 + f32(8) * d2) + a[5]]).astype(f32)


def _at2(a):
    """F(2x2): r0 = acc0 + acc1 + acc2, r1 = acc1 - acc2 - acc3."""
    return np.stack([(a[0] + a[1]) + a[2], (a[1] - a[2]) - a[3]]).astype(f32)


def _bt4(d):
    """F(2x2) input transform along axis 0: one difference (or sum) per output."""
    return np.stack([d[0] - d[2], d[1] + d[2], d[2] - d[1], d[1] - d[3]]).astype(f32)


def conv_wino32(x_chw, w, m, drop=()):
    """The convolution WITHOUT its bias through F(m x m, 3 x 3), m = 2 / 4, every step in fp32: the filter transform of
    tests/wino_ref.py (fp32) / tests/wino4_ref.py (double, rounded once, as the packers do), the input transform B^T d B in two fp32
    passes, the channel sum sequentially, the output transform in the kernels' order of additions.  -> (Cout, H, W) float32."""
    from tests import wino4_ref, wino_ref
    cout, cin = w.shape[:2]
    H, W = x_chw.shape[1:]
    p = m + 2
    ty, tx = -(-H // m), -(-W // m)
    xp = np.zeros((cin, m * ty + 2, m * tx + 2), f32)
    xp[:, 1:H + 1, 1:W + 1] = x_chw
    iy = (m * np.arange(ty))[:, None] + np.arange(p)[None]
    ix = (m * np.arange(tx))[:, None] + np.arange(p)[None]
    d = xp[:, iy[:, None, :, None], ix[None, :, None, :]].transpose(3, 4, 0, 1, 2)                # (p, p, cin, ty, tx)
    bt, at = (_bt4, _at2) if m == 2 else (_bt6, _at4)
    Uw = (wino_ref.filter_transform if m == 2 else wino4_ref.filter_transform4)(w)                # (p, p, cin, cout)
    V = bt(bt(d).transpose(1, 0, 2, 3, 4)).transpose(1, 0, 2, 3, 4)
    M = np.zeros((p, p, cout, ty, tx), f32)
    for c in range(cin):
        if c not in drop:
            M = M + Uw[:, :, c, :, None, None] * V[:, :, c, None]
    Y = at(at(M).transpose(1, 0, 2, 3, 4)).transpose(1, 0, 2, 3, 4)                               # (m, m, cout, ty, tx)
    return np.ascontiguousarray(Y.transpose(2, 3, 0, 4, 1).reshape(cout, m * ty, m * tx)[:, :H, :W])


MUTATIONS = ("bm_added_to_f", "bias_at_next_channel", "scale_of_channel_mod_32", "separator_gt", "separator_on_tile_row", "m_stored_at_cp",
             "column_past_width", "elu_after_sigmoid", "exp_without_minus_one", "dropped_chunk")
SENTINEL = f32(7.0)
GUARD = 64


def linear_launch32(L, x_chw, stride, family, elu, sc, sh, block_h, valid_h, mut=None):
    """One linear launch of read_gated_conv_forward as the training forward issues it, restated in fp32 with the stores into flat
    buffers that end in a guard band of GUARD sentinels: -> (fm buffer, y buffer or None).  family "direct" (no fused gate) / "w2" /
    "w4"; sc, sh (Cout,) float32: the scale and shift of the params block.  mut: one of MUTATIONS — the defects the GPU test's
    assertions must see (tests/test_train_accuracy_cpu.py)."""
    wf, wm = L["wf"], L["wm"]
    cout, cin, k, _ = wf.shape
    cp32 = (cout + 31) // 32 * 32
    pad = lambda a: np.concatenate([np.asarray(a, f32), np.zeros(cp32 + 1 - cout, f32)])             # noqa: E731  (one past the block: zero)
    bf, bm, scp, shp = pad(L["bf"]), pad(L["bm"]), pad(sc), pad(sh)
    drop = tuple(range(32, 48)) if mut == "dropped_chunk" and cin == 48 else ()
    conv = (lambda w: conv_direct32(x_chw, w, stride, drop)) if family == "direct" else (lambda w: conv_wino32(x_chw, w, 2 if family == "w2" else 4, drop))
    Yf, Ym = conv(wf), conv(wm)
    _, oh, ow = Yf.shape
    c = np.arange(cout)
    bi = np.where((c >= cout // 32 * 32) & (cout % 32 != 0), c + 1, c) if mut == "bias_at_next_channel" else c
    f = (Yf + (bm if mut == "bm_added_to_f" else bf)[bi][:, None, None]).astype(f32)
    mm = (Ym + bm[bi][:, None, None]).astype(f32)
    n = oh * ow * 2 * cout
    fm_buf = np.full(n + GUARD, SENTINEL, f32)
    pix = (np.arange(oh)[:, None] * ow + np.arange(ow)[None]) * (2 * cout)                           # (oh, ow)
    fm_buf[pix[None] + c[:, None, None]] = f
    fm_buf[pix[None] + ((cout + 7) // 8 * 8 if mut == "m_stored_at_cp" else cout) + c[:, None, None]] = mm
    tile = {"direct": 4, "w2": 2, "w4": 4}[family]
    past = mut == "column_past_width" and ow % tile != 0

    def store_past(buf, idx, vals):                                   # the partial tile's next column lands on the next row's first pixel
        ok = idx < buf.size
        buf[idx[ok]] = vals[ok]

    if past:
        store_past(fm_buf, (pix[:, -1] + 2 * cout)[None] + c[:, None], f[:, :, -1])
    if family == "direct":
        return fm_buf, None
    with np.errstate(over="ignore", invalid="ignore"):
        e = fast_exp32(np.minimum(f, f32(0)))
        act = (lambda v: np.where(v > 0, v, (fast_exp32(np.minimum(v, f32(0))) - f32(1)).astype(f32))) if elu else (lambda v: v)
        a = np.where(f > 0, f, e if mut == "exp_without_minus_one" else (e - f32(1)).astype(f32)).astype(f32) if elu else f
        s = (1.0 / (f32(1) + fast_exp32(-mm)).astype(np.float64)).astype(f32)
        g = act((f * s).astype(f32)).astype(f32) if mut == "elu_after_sigmoid" else (a * s).astype(f32)
    ci = c % 32 if mut == "scale_of_channel_mod_32" else c
    v = ((g * scp[ci][:, None, None]).astype(f32) + shp[ci][:, None, None]).astype(f32)
    rows = np.arange(oh)
    if block_h > 0:
        r = rows // tile * tile if mut == "separator_on_tile_row" else rows
        sep = (r % block_h > valid_h) if mut == "separator_gt" else (r % block_h >= valid_h)
        v[:, sep] = 0.0
    y_buf = np.full(oh * ow * cout + GUARD, SENTINEL, f32)
    ypix = (rows[:, None] * ow + np.arange(ow)[None]) * cout
    y_buf[ypix[None] + c[:, None, None]] = v
    if past:
        store_past(y_buf, (ypix[:, -1] + cout)[None] + c[:, None], v[:, :, -1])
    return fm_buf, y_buf


def kernel_sum32(vals, blocks, rows):
    """Per-thread sequential sums, the LDS column sum, the workgroups in block order (one of the orders the atomics may take)."""
    P, C = vals.shape
    K = -(-P // (blocks * rows))
    v = np.zeros((K * blocks * rows, C), f32)
    v[:P] = vals
    v = v.reshape(K, blocks, rows, C)
    acc = np.zeros((blocks, rows, C), f32)
    for k in range(K):
        acc = acc + v[k]
    col = np.zeros((blocks, C), f32)
    for r in range(rows):
        col = col + acc[:, r]
    tot = np.zeros(C, f32)
    for b in range(blocks):
        tot = tot + col[b]
    return tot


def gate_backward32(dy, fm, C, sc, elu, valid, mode, abc=None, geometry=None):
    """gate_backward_kernel over one statistic group's pixels: -> (df, dm, sums (4, C)) in fp32.  geometry (blocks, ROWS): (1, 1) sums
    every channel over the pixels one after the other."""
    a, da, s = gate32(fm, C, elu)
    g = (a * s).astype(f32)
    gs = ((abc[0][None] * dy).astype(f32) + abc[1][None]).astype(f32) + (abc[2][None] * g).astype(f32) if mode == 2 else dy * sc[None]
    gs = gs.astype(f32)
    df = ((gs * s).astype(f32) * da).astype(f32) * valid[:, None]
    dm = (((gs * a).astype(f32) * s).astype(f32) * (f32(1) - s)).astype(f32) * valid[:, None]
    blocks, rows = geometry or T.gate_bwd_geometry(fm.shape[0], C)
    terms = [df, dm, dy * valid[:, None], (dy * g).astype(f32) * valid[:, None]]
    return df.astype(f32), dm.astype(f32), np.stack([kernel_sum32(t.astype(f32), blocks, rows) for t in terms])


def rstd32(var):
    return (f32(1) / np.sqrt((var + f32(T.EPS)).astype(f32)).astype(f32)).astype(f32)


def bn_grads32(sums, mean, var):
    return ((sums[3] - (mean * sums[2]).astype(f32)).astype(f32) * rstd32(var)).astype(f32)


def bn_bwd_coeff32(sums, mean, var, gamma, n):
    r = rstd32(var)
    dgamma = ((sums[3] - (mean * sums[2]).astype(f32)).astype(f32) * r).astype(f32)
    A = (gamma * r).astype(f32)
    Cc = (((-A * r).astype(f32) * dgamma).astype(f32) / f32(n)).astype(f32)
    B = (((-A * sums[2]).astype(f32) / f32(n)).astype(f32) - (Cc * mean).astype(f32)).astype(f32)
    return np.stack([A, B, Cc])


def bn_forward32(g, gamma, beta, momentum, rm, rv):
    """One statistic group: -> (y, mean, var, rm, rv) as bn_stats / bn_finalize / bn_apply compute them."""
    n = g.shape[0]
    s1, s2 = g.astype(np.float64).sum(0), (g.astype(np.float64) ** 2).sum(0)
    mean = s1 / n
    var = np.maximum(s2 / n - mean * mean, 0.0)
    mf, vf = mean.astype(f32), var.astype(f32)
    sc = (gamma / np.sqrt((vf + f32(T.EPS)).astype(f32)).astype(f32)).astype(f32)
    sh = (beta - (mf * sc).astype(f32)).astype(f32)
    one_m = f32(1) - f32(momentum)
    rm = ((one_m * rm).astype(f32) + (f32(momentum) * mf).astype(f32)).astype(f32)
    rv = ((one_m * rv).astype(f32) + (f32(momentum) * (var * n / (n - 1) if n > 1 else var).astype(f32)).astype(f32)).astype(f32)
    return ((g * sc[None]).astype(f32) + sh[None]).astype(f32), mf, vf, rm, rv


def wgrad_direct32(x, d, k, stride, plan):
    """wgrad_mfma_kernel + wgrad_reduce_kernel: per split the pixel pairs of its rows in order, two rounded products added to the
    accumulator one after the other; the splits in fours, then one by one."""
    pad = (k - 1) // 2
    H, W, cin = x.shape
    oh, ow, co = d.shape
    xp = np.zeros((H + 2 * pad + k, W + 2 * pad + k, cin), f32)
    xp[pad:pad + H, pad:pad + W] = x
    parts = []
    for y0 in range(0, oh, plan["rows_per_split"]):
        acc = np.zeros((co, cin, k, k), f32)
        for oy in range(y0, min(oh, y0 + plan["rows_per_split"])):
            for ox in range(ow):
                patch = xp[oy * stride:oy * stride + k, ox * stride:ox * stride + k]
                acc = acc + (d[oy, ox][:, None, None, None] * patch.transpose(2, 0, 1)[None]).astype(f32)
        parts.append(acc)
    assert len(parts) == plan["splits"]
    s, i = np.zeros_like(parts[0]), 0
    while i + 4 <= len(parts):
        s = s + ((parts[i] + parts[i + 1]) + (parts[i + 2] + parts[i + 3]))
        i += 4
    for p in parts[i:]:
        s = s + p
    return s


def _bt6(d):
    a, b, c, e = (f32(-4) * d[2] + d[4]), (f32(-4) * d[1] + d[3]), d[4] - d[2], d[3] - d[1]
    return np.stack([f32(4) * d[0] + (f32(-5) * d[2] + d[4]), a + b, a - b, f32(2) * e + c, f32(-2) * e + c, f32(4) * d[1] + (f32(-5) * d[3] + d[5])]).astype(f32)


def _a4(y):
    s02, s13, p, q = y[0] + y[2], y[1] + y[3], f32(4) * y[2] + y[0], f32(8) * y[3] + f32(2) * y[1]
    return np.stack([y[0], s02 + s13, s02 - s13, p + q, p - q, y[3]]).astype(f32)


def _gt(u):
    s12, d12, s34, d34 = u[1] + u[2], u[2] - u[1], u[3] + u[4], u[3] - u[4]
    c6, c12, c24 = f32(1.0 / 6.0), f32(1.0 / 12.0), f32(1.0 / 24.0)
    return np.stack([f32(0.25) * u[0] - s12 * c6 + s34 * c24, d12 * c6 + d34 * c12, -s12 * c6 + s34 * c6 + u[5]]).astype(f32)


def wgrad_wino32(x, d, plan):
    """wgrad_wino4_kernel + sum + reduce in fp32: transforms as wg4_bt6 / wg4_a4 (columns, then rows), tiles accumulated in order within
    a split of tile rows, the splits in four lanes, then G^T . G as the reduce kernel writes it."""
    H, W, cin = x.shape
    co = d.shape[2]
    ty, tx = H // 4, W // 4
    xp = np.zeros((H + 2, W + 2, cin), f32)
    xp[1:-1, 1:-1] = x
    parts = []
    for t0 in range(0, ty, plan["rows_per_split"]):
        acc = np.zeros((6, 6, cin, co), f32)
        for t in range(t0, min(ty, t0 + plan["rows_per_split"])):
            for u_ in range(tx):
                patch = xp[4 * t:4 * t + 6, 4 * u_:4 * u_ + 6]                                    # (6, 6, cin)
                V = _bt6(_bt6(patch).transpose(1, 0, 2)).transpose(1, 0, 2)                       # columns first (u[.][j]), then rows
                M = _a4(_a4(d[4 * t:4 * t + 4, 4 * u_:4 * u_ + 4]).transpose(1, 0, 2)).transpose(1, 0, 2)
                acc = acc + (V[:, :, :, None] * M[:, :, None, :]).astype(f32)
        parts.append(acc)
    lanes = [np.zeros_like(parts[0]) for _ in range(4)]
    i = 0
    while i + 4 <= len(parts):
        for j in range(4):
            lanes[j] = lanes[j] + parts[i + j]
        i += 4
    for p in parts[i:]:
        lanes[0] = lanes[0] + p
    Us = (lanes[0] + lanes[1]) + (lanes[2] + lanes[3]) if len(parts) > 1 else parts[0]
    gtu = _gt(Us)                                                                                 # (3, 6, cin, co)
    return _gt(gtu.transpose(1, 0, 2, 3)).transpose(3, 2, 1, 0)                                   # (co, cin, a, b)
