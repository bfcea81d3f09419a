"""float64 reference of one gated convolution (BasicConv), an error measure in units of fp32 round-off, the derived error bounds of
the split-operand kernels, and the inputs on which those kernels can go wrong.  Plain torch / NumPy on the CPU; nothing from read_amd
or oracle/ takes part in the arithmetic.  tests/test_conv_accuracy_cpu.py runs the NumPy restatements of the kernels through it,
tests/test_gpu_conv_accuracy.py the kernels themselves.

THE MEASURE.  u = 2^-24.  From the fp32 inputs, in float64:  f = conv_f x + b_f,  m = conv_m x + b_m,  y = S act(f) sigma(m) + T + r
with S = gamma / sqrt(var + eps), T = beta - mean S, r the residual.  Condition terms  A_f = conv(|x|, |w_f|) + |b_f|  (A_m likewise),
    B = S (|act'(f)| sigma A_f + |act(f)| sigma (1 - sigma) A_m) + |y|.
    linear launches   E = |got - f| / (u A_f)              gated launches   E = |got - y| / (u B)
A correctly rounded fp32 dot product in any order has E of order 1 .. sqrt(K); a lost f16 piece shows as hundreds to thousands.
R is the same statistic for the torch-fp32 oracle (oneDNN) on the same inputs.

THE DERIVED BOUND (absolute, per element; `preact_bound_*` and `gated_bound`).  Operands (read_amd/csrc/conv.hip, comment above
gated_conv_wino4h_kernel, "every operand is split into TWO f16 pieces"):  x = xh + 2^-11 xl, w s = wh + wl, product = (2^-11 wh) xl +
wl xh + wh xh.  Round-to-nearest f16 (11-bit significand) leaves |x - xh| <= 2^-11 |x|, and the low piece carries that residual to
2^-11 of itself: each operand to 2^-22 = 4 u; the dropped pair wl (2^-11 xl) is at most 2^-11 2^-11 = 4 u: 12 u |w| |x| per product.
That is only true while the low pieces are NORMAL f16 numbers.  f16 has a fixed quantum of 2^-24 below 2^-14, so
  * wl (any value) and 2^-11 wh (for |wh| < 2^-3) are rounded to 2^-24: up to 2^-25 each in units of w s, i.e. an ABSOLUTE error of
    2 . 2^-25 / s per weight, times |x| (|xl| <= |x|).  With max |w s| in [2^14, 2^15) this is 2^-38 .. 2^-39 of the row's largest
    weight: invisible while the entries of a row lie within 2^14 of each other, the limit of the format beyond.  W_FLOOR;
  * xl = f16((x - xh) 2^11) likewise: 2^-25 2^-11 = 2^-36 absolute per activation, times |w| — the "absolute error floor of ~1e-11"
    the kernel comment quotes for |V| below ~1e-4.  X_FLOOR.
Accumulation: every v_mfma adds one k-block of exact products (an f16 x f16 product has 22 significant bits) to the fp32 accumulator and
rounds once; three MFMAs (one per piece pair) per k-block, partial sums bounded by A: 3 nb u A with nb k-blocks.  The epilogue forms
fma(acc, 1 / s, b) — one rounding, 1 / s a power of two.  Hence
    |got_f - f|  <=  u (12 + 3 nb + 1) A_f  +  W_FLOOR conv(|x|, 1) / s  +  X_FLOOR conv(1, |w_f|)  +  TINY
(TINY = 2^-126 for results in the fp32 subnormal range.)  nb per family: see K_BLOCKS.  FAM's x1 * x2 is rounded to fp32 before the
split (lwrite1 of gated_conv_d3h_kernel): one more u per product.
Winograd (gated_conv_wino4h_kernel): the same in the transformed domain with A_w = |A^T| (sum_c |U_c| . |V_c|) |A^T|^T, the 36
frequencies each one MFMA chain over Cin / 32 k-blocks.  Input transform bt6: every output is an add followed by an fma or two fmas = 2
roundings per pass, two passes: 4 u against |B^T| |d| |B^T|^T (not |V|: the pattern cancels), propagated as
A_in = |A^T| (sum_c |U_c| . (|B^T| |d_c| |B^T|^T)) |A^T|^T.  Output transform (R / Y of the epilogue): the longest path is three
additions per pass (R[0] = acc + s1 + s2; the factors 2, 4, 8 are exact): 6 u A_w.  Then the fma with 1 / s and the bias: 1.
    |got_f - f|  <=  u ((12 + 3 Cin / 32 + 6) A_w + 4 A_in + |f|)  +  floors in the transformed domain  +  TINY
F(4,3) by rows (gated_conv_f4x1h_kernel, family "f4x1"): Winograd along x only, the three ky taps direct.  With the patch columns
4 t - 1 .. 4 t + 4 of segment t:  V[r] = B^T d_r,  U[ky] = G w[ky][:],  M[y][fq] = sum_ky sum_c U[ky][fq][c] V[y + ky - 1][fq][c],
Y = A^T M, and the absolute-value images  A_w = |A^T| (sum_ky sum_c |U| . |V|),  A_in = the same with |B^T| |d| in the place of |V|.
  * input transform, the lambda `bt6`: every output is an add followed by an fma (x1 = fma(q, -4, p), x3 = fma(f, 2, h), ...) or two
    fmas (y0, y5) = 2 roundings, ONE pass: 2 u against |B^T| |d|, carried through the sum as 2 u A_in;
  * split operands, `split_store` (hi = v_cvt_pk_f16_f32, the residual by v_fma_mix_f32 is exact, times 2048, v_cvt_pk_f16_f32) and
    read_conv_pack_f4x1_host (hi = f16_bits_rtn(us), lo = f16_bits_rtn(us - hi)); the three piece pairs of `stage_body` (pc = 0: Ws x Bl,
    pc = 1: Wl x Bh, pc = 2: Wh x Bh): 12 u |U| |V| per product, as above;
  * accumulation, `stage_body`: per 32-channel chunk and frequency an accumulator acc[nb][fq] takes 3 taps x 3 piece pairs = 9
    v_mfma_f32_16x16x32_f16, one rounding each, partial sums bounded by the frequency's share of A_w: 9 (Cin / 32) u A_w;
  * output transform, the unit epilogue: Y[nb][0] = acc[0] + s1 + s2 with s1 = acc[1] + acc[2], s2 = acc[3] + acc[4] — three additions
    on the longest path, as Y[nb][3] = d1 + 8 dd2 + acc[5] (8 dd2 is exact, or fused): 3 u A_w;
  * f = fma(Yf, isf, bf): 1 u |f|.
The floors are the Winograd kernel's, in the 1-D transformed domain (V1 = |A^T| sum_ky sum_c |V|, U1 = |A^T| sum_ky sum_c |U| over the
taps whose row is inside the image: a row outside loads zeros, and zero has no pieces to lose) — with one term more.  The 4 u allowed
for the dropped pair Ul (2^-11 Vl) assume |V - Vh| <= 2^-11 |V|.  Where Vh is SUBNORMAL (|V| < 2^-14) the residual is bounded by the
f16 quantum instead, |V - Vh| <= 2^-25 absolute, so the dropped pair is up to 2^-11 |U| 2^-25 = X_FLOOR |U| per product however small
V is: of the size of the Vl floor itself.  In general |Ul| 2^-11 |Vl| <= 2^-11 |U| (2^-11 |V| + 2^-25): the relative part is in the
12 u, the absolute part doubles the X_FLOOR term.  (On activations of 1e-6 the NumPy model of this kernel still reaches 0.88 of the
bound.  That is not a floor: the worst element has f = b_f + 1e-6-sized products, u |f| is 0.92 of its bound and 2 X_FLOOR U1 0.06,
and the one rounding of fma(Yf, isf, bf) is half an ulp of f, which IS u |f| for f just above a power of two.  The term is tight by
nature; the other families hide it under (12 + 3 nb + 1) u A with |b| inside A.)
    |got_f - f|  <=  u ((12 + 9 Cin / 32 + 3) A_w + 2 A_in + |f|)  +  W_FLOOR V1 / s  +  2 X_FLOOR U1  +  TINY
s: one power of two per output row over all (ky, frequency, cin), `mx` of read_conv_pack_f4x1_host (f4x1_filter_inv_scale).
Range: the largest row sum of |B^T| is 10 (rows 0, 1, 2, 5): |V| <= 10 max |x|, finite in f16 up to max |x| = 6550 (65500 rounds to
65504, the last finite f16; 65600 rounds to Inf).  f4x1_range_edge attains it.
Gate epilogue (the `epilogue` lambdas of the kernels: mm = fma(acc_m, -log2e / s, -log2e b_m), t = v_exp_f32(mm) + 1, sg = v_rcp_f32(t),
fe = f log2e, e = v_exp_f32(fe) - 1, v = (f sg) sc + sh + res; v_exp_f32 / v_rcp_f32 1 ulp = 2 u):
  d_sigma <= sigma (1 - sigma) (d_m + u (3 A_m + 2))  +  3 u sigma        (rounded log2e constant, the rounded product log2e b_m and the
                                                                          fma: 3 u A_m in the exponent; exp 2 u; the add 1 u, rcp 2 u)
  d_g     <= act'(f) (d_f + [f <= 0] u (2 |f| + 2))  +  [f <= 0] u |g|    (fe = f log2e: constant + rounding; exp 2 u; the - 1: u |g|)
  d_y     <= S (sigma d_g + |g| d_sigma)  +  u (6.5 S |g sigma| + 4.5 S |mean| + 2 |T| + |y|)
             (product g sigma 1; sc = gamma / sqrtf(var + eps) computed in fp32 on the host, eps as a float: 3.5; the multiply 1, the
              add of sh 1 — against S |g sigma| + |T| —; sh = beta - mean sc: 4.5 S |mean| + |T|; the residual add |y|)
(gated_conv_pxh_kernel forms m = fma(acc, 1 / s, b_m) first and then m (-log2e): three roundings of at most u |m| <= u A_m, the same 3 u A_m.)
First order; the neglected second-order terms are below 2^-10 of these while d_f, d_m < 2^-10: the factor SECOND_ORDER.
"""
import numpy as np
import torch
import torch.nn.functional as F

from tests.wino4_ref import AT, BT, G

U = 2.0 ** -24
EPS = 1e-5
W_FLOOR = 2.0 * 2.0 ** -25          # per weight, in units of w s
X_FLOOR = 2.0 ** -36                # per activation
TINY = 2.0 ** -126
SECOND_ORDER = 1.0 + 2.0 ** -10

# Measured caps (profiles/conv_accuracy_fp64.md, column c): E_rms <= c R_rms and E_max <= c R_max against the torch-fp32 oracle's own
# error on the same case; per family, launch mode AND class (tighter than one number per family): c = twice the largest ratio E / R
# measured on an MI355X over the cases of that row of the table, rounded up to a power of two, and never below 1 (a kernel is not asked
# to beat the oracle) — twice, because the ratio of two round-off statistics over 10^5 - 10^6 outputs moves by tens of percent between
# seeds, not by a factor.  Winograd (w4h): E against A_w (module docstring).  The d3h / d3h_s2 / w4h kernels have no linear launches;
# the NumPy restatements of their pre-activations (tests/test_conv_accuracy_cpu.py) are held to the pxh kernel's linear row — the same
# three-piece-pair arithmetic, measured without an epilogue.
C_MEASURED = {"d3h": {"gated": {"a": 4.0, "b": 16.0, "c": 16.0, "d": 8.0}}, "d3h_s2": {"gated": {"a": 4.0, "b": 8.0, "c": 16.0, "d": 8.0}}, "pxh": {"gated": {"a": 4.0, "b": 4.0, "c": 8.0, "d": 4.0}, "linear": {"a": 4.0, "b": 2.0, "c": 2.0, "d": 1.0}}, "t3h": {"gated": {"a": 4.0, "b": 2.0, "c": 16.0, "d": 8.0}, "linear": {"a": 4.0, "b": 8.0, "c": 2.0, "d": 2.0}}, "w4h": {"gated": {"a": 1.0, "b": 8.0, "c": 16.0, "d": 8.0}},
              "f4x1": {"gated": {"a": 4.0, "b": 16.0, "c": 16.0, "d": 8.0}}}      # f4x1: E against A_w, as w4h


def measured_cap(family, mode, cls):
    by_mode = C_MEASURED[family]
    return by_mode[mode][cls] if mode in by_mode else C_MEASURED["pxh"][mode][cls]


def k_blocks(family, cin, k):
    """MFMA k-blocks per output element: gated_conv_d3h_kernel / _s2 run one v_mfma_f32_16x16x32_f16 triple per (tap, 32-channel chunk)
    (`stage`: 9 taps x 4 pixel blocks, three MFMAs each); gated_conv_pxh_kernel one v_mfma_f32_32x32x16_f16 triple per k16 step of
    K = taps Cin padded to 16 (read_conv_pack_t3h_host); the Winograd kernel one triple per 32-channel chunk and frequency; the
    F(4,3)-by-rows kernel three triples (one per ky tap) per 32-channel chunk and frequency: its bound counts 9 per block."""
    if family in ("d3h", "d3h_s2"):
        return k * k * cin // 32
    if family in ("pxh", "t3h"):
        return (k * k * cin + 15) // 16
    if family in ("w4h", "f4x1"):
        return cin // 32
    raise ValueError(family)


# ------------------------------------------------------------------------------------------ reference
def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def _conv(x, w, b, stride):
    pad = (w.shape[-1] - 1) // 2
    return F.conv2d(x[None], w, b, stride=stride, padding=pad)[0]


class Ref:
    """All float64 CHW numpy arrays: f, m, Af, Am, y, B, and what the derived bound needs."""


def reference(L, x, stride=1, elu=True, residual=None, mul=None):
    """L: dict wf, bf, wm, bm, gamma, beta, mean, var (float32 arrays); x (C, H, W) float32 (concatenated / resampled as the layer sees
    it); mul: FAM's second factor; residual (Cout, outH, outW)."""
    r = Ref()
    x64 = _t64(x) * (_t64(mul) if mul is not None else 1.0)
    wf, wm, bf, bm = _t64(L["wf"]), _t64(L["wm"]), _t64(L["bf"]), _t64(L["bm"])
    ones_w = torch.ones((1,) + tuple(wf.shape[1:]), dtype=torch.float64)
    ones_x = torch.ones_like(x64)
    r.f = _conv(x64, wf, bf, stride).numpy()
    r.m = _conv(x64, wm, bm, stride).numpy()
    r.Af = _conv(x64.abs(), wf.abs(), bf.abs(), stride).numpy()
    r.Am = _conv(x64.abs(), wm.abs(), bm.abs(), stride).numpy()
    r.X1 = _conv(x64.abs(), ones_w, None, stride).numpy()[0]                                     # (outH, outW): sum of |x| under the taps
    r.W1f = _conv(ones_x, wf.abs(), None, stride).numpy()                                        # sum of |w| over the taps inside the image
    r.W1m = _conv(ones_x, wm.abs(), None, stride).numpy()
    g64, be, mu, va = (np.asarray(L[k], np.float64)[:, None, None] for k in ("gamma", "beta", "mean", "var"))
    r.S = np.abs(g64) / np.sqrt(va + EPS)
    Ssigned = g64 / np.sqrt(va + EPS)
    r.T = be - mu * Ssigned
    r.mean_S = np.abs(mu) * r.S
    with np.errstate(over="ignore"):
        r.sig = 1.0 / (1.0 + np.exp(-r.m))
        r.g = np.where(r.f > 0, r.f, np.expm1(np.minimum(r.f, 0.0))) if elu else r.f
        r.dact = np.where(r.f > 0, 1.0, np.exp(np.minimum(r.f, 0.0))) if elu else np.ones_like(r.f)
    r.elu = elu
    r.res = np.zeros_like(r.f) if residual is None else np.asarray(residual, np.float64)
    r.y = Ssigned * r.g * r.sig + r.T + r.res
    r.cond = r.S * (np.abs(r.dact) * r.sig * r.Af + np.abs(r.g) * r.sig * (1.0 - r.sig) * r.Am)  # the part of B that comes from the products
    r.B = r.cond + np.abs(r.y)
    r.mul = mul is not None
    return r


def oracle_fp32(L, x, stride=1, elu=True, residual=None, mul=None, linear=False):
    """The torch-fp32 restatement of BasicConv on the same inputs (what oracle.unet_torch.basic_conv computes): -> (Cout or 2 Cout, H, W)."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))       # noqa: E731
    xx = t(x) * t(mul) if mul is not None else t(x)
    f = _conv(xx, t(L["wf"]), t(L["bf"]), stride)
    m = _conv(xx, t(L["wm"]), t(L["bm"]), stride)
    if linear:
        return torch.cat([f, m]).numpy()
    if elu:
        f = F.elu(f)
    y = F.batch_norm((f * torch.sigmoid(m))[None], t(L["mean"]), t(L["var"]), t(L["gamma"]), t(L["beta"]), training=False, eps=EPS)[0]
    if residual is not None:
        y = y + t(residual)
    return y.numpy()


# ------------------------------------------------------------------------------------------ measure
def _stats(err, den):
    nz = den > 0
    e = np.zeros_like(err)
    e[nz] = err[nz] / (U * den[nz])
    e[~nz & (err > 0)] = np.inf
    return float(e.max()), float(np.sqrt(np.mean(e ** 2)))


def measure_linear(got_2c, ref):
    """got (2 Cout, H, W) = [f | m] -> (E_max, E_rms) over both halves."""
    c = ref.f.shape[0]
    err = np.abs(np.concatenate([got_2c[:c].astype(np.float64) - ref.f, got_2c[c:].astype(np.float64) - ref.m]))
    return _stats(err, np.concatenate([ref.Af, ref.Am]))


def measure_gated(got, ref):
    return _stats(np.abs(got.astype(np.float64) - ref.y), ref.B)


# ------------------------------------------------------------------------------------------ derived bounds
def row_inv_scale(w_rows):
    """1 / s of the packers: s = 2^ex puts the row's largest |entry| in [2^14, 2^15), ex clamped to +-60, 1 for an all-zero row."""
    mx = np.abs(np.asarray(w_rows, np.float64)).reshape(w_rows.shape[0], -1).max(axis=1)
    ex = np.zeros(mx.shape, np.int64)
    nz = mx > 0
    _, e = np.frexp(mx[nz])
    ex[nz] = np.clip(15 - e, -60, 60)
    return np.ldexp(1.0, -ex)


def preact_bound_direct(L, ref, family, which):
    """|got - f| (which = 'f') or |got - m| <= this, elementwise, for the direct split-operand families."""
    w = L["w" + which]
    A, W1 = (ref.Af, ref.W1f) if which == "f" else (ref.Am, ref.W1m)
    cin, k = w.shape[1], w.shape[2]
    n = 12 + (1 if ref.mul else 0) + 3 * k_blocks(family, cin, k) + 1
    inv_s = row_inv_scale(w)[:, None, None]
    return U * n * A + W_FLOOR * inv_s * ref.X1[None] + X_FLOOR * W1 + TINY


def wino_terms(L, x, which):
    """-> (A_w, A_in, V1 = |A^T| (sum_c |V_c|) |A^T|^T, U1 = |A^T| (sum_c |U_c|) |A^T|^T), each (Cout, H, W), float64, bias not included."""
    w = np.asarray(L["w" + which], np.float64)
    cout, cin = w.shape[:2]
    _, H, W = x.shape
    ty, tx = (H + 3) // 4, (W + 3) // 4
    xp = np.zeros((cin, 4 * ty + 2, 4 * tx + 2))
    xp[:, 1:H + 1, 1:W + 1] = x
    iy = (4 * np.arange(ty))[:, None] + np.arange(6)[None]
    ix = (4 * np.arange(tx))[:, None] + np.arange(6)[None]
    d = xp[:, iy[:, None, :, None], ix[None, :, None, :]]                                        # (C, ty, tx, 6, 6)
    B64, A64 = BT.astype(np.float64), AT.astype(np.float64)
    V = np.abs(np.einsum("ia,ctuab,jb->tuijc", B64, d, B64, optimize=True))
    Vin = np.einsum("ia,ctuab,jb->tuijc", np.abs(B64), np.abs(d), np.abs(B64), optimize=True)
    Uabs = np.ascontiguousarray(np.abs(np.einsum("ia,ocab,jb->ijco", G, w, G)))

    def per_frequency(Vt):                                                                       # sum_c |V_c| |U_c|: one matrix product per frequency
        Vf = np.ascontiguousarray(Vt.transpose(2, 3, 0, 1, 4)).reshape(6, 6, ty * tx, cin)
        M = np.stack([np.stack([Vf[i, j] @ Uabs[i, j] for j in range(6)]) for i in range(6)])
        return M.reshape(6, 6, ty, tx, cout).transpose(2, 3, 0, 1, 4)

    out = []
    for M in (per_frequency(V), per_frequency(Vin),
              np.repeat(V.sum(-1)[..., None], cout, -1), np.repeat(Uabs.sum(2)[None, None], ty, 0).repeat(tx, 1)):
        Y = np.einsum("pi,tuijo,qj->otpuq", np.abs(A64), M, np.abs(A64), optimize=True).reshape(cout, 4 * ty, 4 * tx)
        out.append(Y[:, :H, :W])
    return out


def wino_filter_inv_scale(w):
    Uf = np.einsum("ia,ocab,jb->oijc", G, np.asarray(w, np.float64), G)
    return row_inv_scale(Uf)


def preact_bound_wino(L, x, ref, which):
    Aw, Ain, V1, U1 = wino_terms(L, x, which)
    w = L["w" + which]
    n = 12 + 3 * k_blocks("w4h", w.shape[1], 3) + 6
    inv_s = wino_filter_inv_scale(w)[:, None, None]
    val = np.abs(ref.f if which == "f" else ref.m)
    return U * (n * Aw + 4 * Ain + val) + W_FLOOR * inv_s * V1 + X_FLOOR * U1 + TINY, Aw


def _f4x1_images(x):
    """-> (|V|, |B^T| |d|), each (6, H + 2, segments, Cin): the transformed rows of the zero-padded image, row index y + 1."""
    cin, H, W = x.shape
    nt = (W + 3) // 4
    xp = np.zeros((H + 2, 4 * nt + 2, cin))
    xp[1:H + 1, 1:W + 1] = np.asarray(x, np.float64).transpose(1, 2, 0)
    d = np.stack([xp[:, j:j + 4 * nt:4] for j in range(6)]).reshape(6, -1)                       # [patch column 4 t - 1 + j][(row, segment, cin)]
    B64 = BT.astype(np.float64)
    return np.abs(B64 @ d).reshape(6, H + 2, nt, cin), (np.abs(B64) @ np.abs(d)).reshape(6, H + 2, nt, cin)


def f4x1_terms(L, x, which):
    """The 1-D analogue of wino_terms for gated_conv_f4x1h_kernel -> (A_w, A_in, V1, U1), each (Cout, H, W), float64, bias not included
    (module docstring, "F(4,3) by rows").  Every contraction over cin is one matrix product per (frequency, ky)."""
    w = np.asarray(L["w" + which], np.float64)
    cout, cin = w.shape[:2]
    _, H, W = x.shape
    nt = (W + 3) // 4
    Uabs = np.ascontiguousarray(np.abs(np.einsum("fb,ocab->faco", G.astype(np.float64), w)))      # [fq][ky][cin][co]
    absAT = np.abs(AT).astype(np.float64)
    inside = np.array([[0 <= y + ky - 1 < H for ky in range(3)] for y in range(H)], np.float64)   # (y, ky): the tap's row is in the image
    out = []
    V, Vin = _f4x1_images(x)
    for img in (V, Vin):
        M = np.stack([sum(img[fq, ky:ky + H].reshape(H * nt, cin) @ Uabs[fq, ky] for ky in range(3)) for fq in range(6)])   # (fq, (y, t), co)
        out.append(np.einsum("pf,fno->onp", absAT, M).reshape(cout, H, 4 * nt)[:, :, :W])
    X1 = sum(V[:, ky:ky + H].sum(axis=3) for ky in range(3))                                      # (fq, y, t)
    V1 = np.einsum("pf,fyt->ytp", absAT, X1).reshape(H, 4 * nt)[:, :W]
    out.append(np.broadcast_to(V1[None], (cout, H, W)).copy())
    U1 = np.einsum("pf,yk,fko->oyp", absAT, inside, Uabs.sum(axis=2))                             # (co, y, pixel of the segment)
    out.append(np.tile(U1, (1, 1, nt))[:, :, :W])
    return out


def f4x1_filter_inv_scale(w):
    """1 / s of read_conv_pack_f4x1_host: one scale per output row over all (ky, frequency, cin) of U[ky] = G w[ky][:]."""
    Uf = np.einsum("fb,ocab->oafc", G.astype(np.float64), np.asarray(w, np.float64))
    return row_inv_scale(Uf)


def preact_bound_f4x1(L, x, ref, which):
    """-> (|got - f| or |got - m| <= this, elementwise; A_w) for gated_conv_f4x1h_kernel (module docstring, "F(4,3) by rows")."""
    Aw, Ain, V1, U1 = f4x1_terms(L, x, which)
    w = L["w" + which]
    n = 12 + 9 * k_blocks("f4x1", w.shape[1], 3) + 3
    inv_s = f4x1_filter_inv_scale(w)[:, None, None]
    val = np.abs(ref.f if which == "f" else ref.m)
    return U * (n * Aw + 2 * Ain + val) + W_FLOOR * inv_s * V1 + 2 * X_FLOOR * U1 + TINY, Aw


def gated_bound(ref, df, dm):
    """|got - y| <= this, from the pre-activation bounds df, dm (module docstring, "Gate epilogue")."""
    neg = (ref.f <= 0) if ref.elu else np.zeros(ref.f.shape, bool)
    near0 = np.abs(ref.f) <= df                                  # the branch of the device may differ from the reference's: both are within d_f
    dact = np.where(near0, 1.0, ref.dact)
    dg = dact * (df + neg * U * (2 * np.abs(ref.f) + 2)) + neg * U * np.abs(ref.g)
    dsig = ref.sig * (1 - ref.sig) * (dm + U * (3 * ref.Am + 2)) + 3 * U * ref.sig
    epi = U * (6.5 * ref.S * np.abs(ref.g * ref.sig) + 4.5 * ref.mean_S + 2 * np.abs(ref.T) + np.abs(ref.y))
    return SECOND_ORDER * (ref.S * (ref.sig * dg + np.abs(ref.g) * dsig) + epi) + TINY * (1 + ref.S)


def constant_outputs(L, ref):
    """Where no product reaches the output (S = 0: gamma = 0; or A_f = 0: an all-zero conv_f row with zero bias, act(0) = 0) the kernel
    must store the epilogue constant sh (+ residual) exactly.  -> (mask, candidates): sh = beta - mean * sc in fp32, with or without a
    fused multiply-add on the host (both are correct roundings of the packer's expression)."""
    g, be, mu, va = (np.asarray(L[k], np.float32) for k in ("gamma", "beta", "mean", "var"))
    sc = g / np.sqrt(va + np.float32(EPS))
    sh_a = (be - mu * sc).astype(np.float32)
    sh_b = (be.astype(np.float64) - mu.astype(np.float64) * sc.astype(np.float64)).astype(np.float32)
    mask = np.broadcast_to(ref.S == 0, ref.f.shape) | (ref.Af == 0)
    res = ref.res.astype(np.float32)
    return mask, [(s[:, None, None] + res).astype(np.float32) for s in (sh_a, sh_b)]


# ------------------------------------------------------------------------------------------ inputs
def tame_layer(cin, cout, k, seed):
    """Class (a): the distribution every other test uses (read_amd.synthetic.make_unet_state: Conv2d default init, gamma and var in
    [0.5, 1.5]), restated here so the helper stands alone."""
    rng = np.random.default_rng([seed, cin, cout, k])
    b = 1.0 / np.sqrt(cin * k * k)
    return dict(wf=rng.uniform(-b, b, (cout, cin, k, k)).astype(np.float32), bf=rng.uniform(-b, b, cout).astype(np.float32),
                wm=rng.uniform(-b, b, (cout, cin, k, k)).astype(np.float32), bm=rng.uniform(-b, b, cout).astype(np.float32),
                gamma=rng.uniform(0.5, 1.5, cout).astype(np.float32), beta=(0.1 * rng.standard_normal(cout)).astype(np.float32),
                mean=(0.1 * rng.standard_normal(cout)).astype(np.float32), var=rng.uniform(0.5, 1.5, cout).astype(np.float32))


EDGE_ROWS = ("zero", "single", "pow2", "below_pow2", "denormal", "neg_zero")


def edge_row(kind, cin, k, rng):
    """One weight row (cin, k, k) of the packers' edge cases; the largest entry sits at the last tap, which the Winograd filter transform
    copies unchanged into frequency (5, 5) (G[5] = [0, 0, 1]): it stays the row's largest there too."""
    w = (rng.uniform(-1, 1, (cin, k, k)) * 2.0 ** -6).astype(np.float32)
    if kind == "zero":
        w[:] = 0.0
    elif kind == "single":
        w[:] = 0.0
        w[cin // 2, k - 1, k - 1] = np.float32(-0.7)
    elif kind == "pow2":
        w[3 % cin, k - 1, k - 1] = np.float32(0.125)                       # frexp gives e with max = 2^(e-1): the boundary of the scale rule
    elif kind == "below_pow2":
        w[5 % cin, k - 1, k - 1] = np.nextafter(np.float32(0.125), np.float32(0))    # s w rounds UP into the next f16 binade (f16_bits_rtn's carry)
    elif kind == "denormal":
        w[:] = (rng.uniform(-1, 1, (cin, k, k)) * 1e-40).astype(np.float32)  # ex = 15 - e > 60: the clamp
    elif kind == "neg_zero":
        w[::2] = np.float32(-0.0)
    return w


def checkpoint_like(cin, cout, k, H, W, seed, edge_rows=True):
    """Class (b): -> (L, x).  Per-input-channel activation scales 2^U(-8, 8) with that channel's weights scaled by the inverse; per-row
    weight scales 2^U(-12, 6); three entries of every row 2^10 x the rest; var log-uniform 1e-4 .. 1e2; gamma of both signs and 0; |bias|
    up to 10; the edge rows of EDGE_ROWS in conv_f (rows 0 ..) and conv_m (rows 8 ..); -0.0 among the activations."""
    rng = np.random.default_rng([seed, cin, cout, k, 1])
    L = tame_layer(cin, cout, k, seed)
    a = 2.0 ** rng.uniform(-8, 8, cin)
    x = (rng.standard_normal((cin, H, W)) * a[:, None, None]).astype(np.float32)
    x[rng.random(x.shape) < 0.01] = np.float32(-0.0)
    for key in ("wf", "wm"):
        w = L[key].astype(np.float64) / a[None, :, None, None]
        flat = w.reshape(cout, -1)
        for o in range(cout):
            flat[o, rng.choice(flat.shape[1], 3, replace=False)] *= 2.0 ** 10
        w = flat.reshape(w.shape) * (2.0 ** rng.uniform(-12, 6, cout))[:, None, None, None]
        L[key] = w.astype(np.float32)
    L["var"] = np.exp(rng.uniform(np.log(1e-4), np.log(1e2), cout)).astype(np.float32)
    L["gamma"] = (L["gamma"] * rng.choice([-1.0, 1.0], cout)).astype(np.float32)
    L["gamma"][rng.choice(cout, max(1, cout // 16), replace=False)] = 0.0
    L["bf"] = (L["bf"] + (rng.random(cout) < 0.25) * rng.uniform(-10, 10, cout)).astype(np.float32)
    L["bm"] = (L["bm"] + (rng.random(cout) < 0.25) * rng.uniform(-10, 10, cout)).astype(np.float32)
    if edge_rows:
        for j, kind in enumerate(EDGE_ROWS):
            if j < cout:
                L["wf"][j] = edge_row(kind, cin, k, rng)
            if 8 + j < cout:
                L["wm"][8 + j] = edge_row(kind, cin, k, rng)
        L["bf"][0] = 0.0                                          # the all-zero conv_f row with zero bias: act(0) = 0, the output is the BN constant
    return L, x


def impulse(cin, H, W, c, y, x_, amp):
    x = np.zeros((cin, H, W), np.float32)
    x[c, y, x_] = amp
    return x


def impulse_positions(cin, H, W):
    """(channel, y, x): every position of the 6 x 6 Winograd patch of tile (1, 1) (origin 4 t - 1 = 3), the four corners, the last
    partial tile / unit in x and in y, and the k-block / lane-quad boundary channels."""
    pos = [(1 % cin, 3 + i, 3 + j) for i in range(6) for j in range(6) if 3 + i < H and 3 + j < W]
    pos += [(2 % cin, 0, 0), (2 % cin, 0, W - 1), (2 % cin, H - 1, 0), (2 % cin, H - 1, W - 1), (4 % cin, H - 1, W // 2), (4 % cin, H // 2, W - 1)]
    pos += [(c, min(5, H - 1), min(6, W - 1)) for c in sorted({0, 7 % cin, 8 % cin, 31 % cin, 32 % cin, cin - 1})]
    return pos


def impulse_positions_f4x1(cin, H, W):
    """impulse_positions plus what the geometry of gated_conv_f4x1h_kernel adds (units of 8 rows x 32 columns = 8 segments of 4): the
    unit seam in x (columns 31, 32, 33) inside a unit's rows, the halo rows of a unit (7, 8) at that seam, and every column of the last
    partial segment.  A list of its own: the cases of the other families do not change."""
    pos = list(impulse_positions(cin, H, W))
    seam = [x_ for x_ in (31, 32, 33) if x_ < W]
    pos += [(1 % cin, min(3, H - 1), x_) for x_ in seam]
    pos += [(1 % cin, y, x_) for y in (7, 8) if y < H for x_ in seam]
    pos += [(3 % cin, H // 2, x_) for x_ in range(4 * ((W - 1) // 4), W)]
    return list(dict.fromkeys(pos))


def constant_image(cin, H, W, value=1.0):
    return np.full((cin, H, W), value, np.float32)


def checkerboard(cin, H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.broadcast_to(np.where((yy + xx) % 2 == 0, 1.0, -1.0)[None], (cin, H, W)).astype(np.float32).copy()


def wino_range_edge(cin, H, W, rows=(0, 0), tile=(1, 1), amp=650.0):
    """Class (d): the 6 x 6 sign pattern sign(BT[r]) x sign(BT[r']) (rows of absolute sum 10: 0, 1, 2, 5) that attains |B^T d B| = 100 amp
    at frequency (r, r'), on the patch of an interior tile (origin 4 t - 1), every channel, the rest of the image zero."""
    assert all(np.abs(BT[r]).sum() == 10 for r in rows)
    pat = np.outer(np.sign(BT[rows[0]]), np.sign(BT[rows[1]])).astype(np.float32) * np.float32(amp)
    x = np.zeros((cin, H, W), np.float32)
    y0, x0 = 4 * tile[0] - 1, 4 * tile[1] - 1
    x[:, y0:y0 + 6, x0:x0 + 6] = pat[None]
    return x


def f4x1_range_edge(cin, H, W, row=0, segment=1, amp=6550.0):
    """Class (d) of the F(4,3)-by-rows kernel: sign(BT[row]) amp on the six patch columns 4 t - 1 .. 4 t + 4 of segment t, every image
    row and channel, the rest zero: |B^T d| = 10 amp at frequency `row` (rows of absolute sum 10: 0, 1, 2, 5).  At amp = 6550 the
    transformed value is 65500, which rounds to 65504, the last finite f16."""
    assert np.abs(BT[row]).sum() == 10 and 4 * segment - 1 >= 0 and 4 * segment + 4 < W
    x = np.zeros((cin, H, W), np.float32)
    x[:, :, 4 * segment - 1:4 * segment + 5] = (np.sign(BT[row]).astype(np.float32) * np.float32(amp))[None, None, :]
    return x
