"""NumPy fp32 restatements of the training kernels (read_amd/csrc/train.hip) in the kernels' own order of operations, without fused
multiply-adds: the gate / BatchNorm chain (modes 0 / 1 / 2, bn_bwd_coeff, bn_stats in fp64, bn_finalize, bn_apply) and both
weight-gradient kernels.  tests/test_train_accuracy_cpu.py holds them to the derived bounds of tests/train_ref64.py;
tests/test_gpu_train_accuracy.py uses them, summing sequentially, as the yardstick R_seq."""
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
