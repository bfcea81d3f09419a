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

RESAMPLED SOURCES (`assemble`).  The loader of gated_conv_pxh_kernel (`load_step`: sy = (ly[pt] << sl) >> sr, sx likewise, one of sl, sr
zero by conv_prepare's SrcDev{..., shift > 0 ? shift : 0, shift < 0 ? -shift : 0}) reads source pixel dst << s of a finer source and
dst >> -s of a coarser one.  Addressing only: the arithmetic and its bound are those of the concatenated image.
A LAUNCH WITH AN ADDEND (`preact_bound_addend`; epilogue of gated_conv_pxh_kernel).  pp = pre + ((y >> pre_shift) pre_W + (x >>
pre_shift)) pre_cstride, af = pp[pre_foff + cc], am = pp[pre_moff + cc] with cc = c0 < Cout ? c0 : Cout - 4 (a padded group reads valid
channels and stores nothing), then
  * f = fma(acc, 1 / s_f, b_f): the `+ 1` of preact_bound_direct, against the launch's OWN A (Af_own = conv(|x|, |w_f|) + |b_f|);
  * f += af[qd]: one more rounding, u |f| of the finished value;
  * the addend's own error d_pre, sampled as the addend is; zero for an addend the host gives.
    |got_f - f|  <=  preact_bound_direct(own weights, own sources)  +  u |f|  +  d_pre          (m likewise; gated_bound on top, unchanged)
The measure takes A_f = Af_own + |pre_f|: where the addend cancels the launch's own sum (|f| << A) the error stays of the size u A.
THE CHAIN (`AFF_PLAN`, `aff_chain_reference`; build() of read_amd/csrc/unet.cpp under g_unet_aff_split).  q3 = W[:, z] z is a plain linear
launch: d(q3) = preact_bound_direct(part 3).  Every later launch reads the coarser one as its addend at (y >> 1, x >> 1):
    d(q_k) = preact_bound_direct(part k) + up(d(q_k+1)) + u |q_k|,     d_f(AFF_i) = preact_bound_direct(own part) + up(d(q)) + u |f|
with up() the same sampling, |q_k| and |f| the float64 values of the UNSPLIT layer on assemble(...) (the chain computes the same sum,
re-associated), each part's 1 / s from row_inv_scale of that part's stacked rows (the packer scales what it is given: `derive` stacks
[f0 f1 f2 | m0 m1 m2] with zero bias), and nb = columns of the part / 16.  E is taken against A of the unsplit 480-channel layer.  The
intermediate tensors are fp32: one stored with an f16 significand (2^-12 |q| relative) exceeds d(q) ~ (13 + 3 nb) u A wherever
|q| > 2^-12 (13 + 3 nb) A — 0.012 A for the 256 columns of q3 —, which a sum of 256 products does on most elements.
THE OUTPUT HEAD (family "sc", gated_conv_smallc_kernel; `preact_bound_sc`).  fp32 operands, no packer: no split terms, no W_FLOOR /
X_FLOOR.  Per accumulator 9 x 32 = 288 v_fmac_f32 in the order (phase of CPH channels, tap, quad of the phase, channel of the quad), each
one fused product-and-add = one rounding of a partial sum that is bounded by A: 288 u A; a tap outside the image arrives as zero
(buffer load out of range) and its fmac is exact.  Then f = fa + params[c] (an add, not an fma): u |f|.
    |got_f - f|  <=  288 u A_f  +  u |f|  +  TINY
elu1 / sigmoidf (fast_exp(x) = v_exp_f32(x log2e), v_rcp_f32) against the gate epilogue above: elu1 is d_g term for term (fe = f log2e:
constant and rounding, exp 2 u, the - 1); sigmoidf(m) forms (-m) log2e — the rounded constant and one rounding, 2 u |m| <= 2 u A_m where
the split kernels have 3 u A_m — then exp, + 1, rcp as there; (f sg) sc + sh has no residual and may contract to an fma.  Every term is
at most its counterpart: gated_bound is used unchanged.  Denormals: read_amd/build.py passes -O3 and no flush option, so the kernels are
compiled with fp32 denormals ON (v_fmac_f32 keeps a subnormal partial sum); TINY stays for the results v_exp_f32 / v_rcp_f32 flush.
bilinear_up4_kernel (`bilinear_up4_bound`).  The weights ly0, ly1, lx0, lx1 are multiples of 1/8 in [0, 1], exact in fp32, and sum to 1
per axis.  o = ly0 (lx0 v00 + lx1 v01) + ly1 (lx0 v10 + lx1 v11) without any contraction: each product lx v one rounding and their sum
one: 2 u (lx0 |v00| + lx1 |v01|); the product with ly one more: 3 u; the final sum u |o| <= u sum w |v|: 4 u sum w |v| (an fma in
the place of a product and a sum only removes roundings).  A constant image of 1.0 comes back exactly: the products k / 8 are exact and sum to 1.
CLASS (e): DEGENERATE SIZES (`SHAPES_E_*`, `degenerate_positions`, `degenerate_images`).  The library accepts every viewport that is a
positive multiple of 16; at 16 x 16 the four UNet levels are 16 x 16, 8 x 8, 4 x 4 and 2 x 2.  Class (e) holds every family to the same
measure and the same derived bounds at those levels and below: an image smaller than one 8 x 32 unit / 4 x 4 tile / 4-pixel segment in
both directions, a stride-2 parity plane of one pixel, a nearest-resampled source or an addend of 2 x 2 or a single pixel, a 6 x 6
Winograd patch that is halo on all four sides.  No term of the bounds depends on the image size: A, A_w, A_in, X1, W1 are sums over the
taps INSIDE the image (a tap outside loads zero and has no pieces to lose), so a corner output of a constant-1 image sees 4 taps, an
edge 6 and the interior 9 in the reference and in the bound alike, and a halo mistake is an error of order 1 against a bound of order
1e-6.  Inputs per shape: unit scale (with a residual where the family takes one, ELU alternating), a constant 1, a checkerboard, and
impulses of 1 and 2^-10 at every pixel where H W <= 16 (else the corners, the mid-edges and the centre) in channels 1 % C and C - 1.
The caps of class (e) are measured as the others are (C_MEASURED), but over a handful of pixels the oracle's own R is noisy: they are
set per family and mode from the class (e) rows of profiles/conv_accuracy_fp64.md and apply where R_max >= 1 only.
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
C_MEASURED = {"d3h": {"gated": {"a": 4.0, "b": 16.0, "c": 16.0, "d": 8.0, "e": 32.0}}, "d3h_s2": {"gated": {"a": 4.0, "b": 8.0, "c": 16.0, "d": 8.0, "e": 32.0}}, "pxh": {"gated": {"a": 4.0, "b": 4.0, "c": 8.0, "d": 4.0, "e": 8.0}, "linear": {"a": 4.0, "b": 2.0, "c": 2.0, "d": 1.0, "e": 4.0}}, "t3h": {"gated": {"a": 4.0, "b": 2.0, "c": 16.0, "d": 8.0, "e": 16.0}, "linear": {"a": 4.0, "b": 8.0, "c": 2.0, "d": 2.0, "e": 4.0}}, "w4h": {"gated": {"a": 1.0, "b": 8.0, "c": 16.0, "d": 8.0, "e": 32.0}},
              "f4x1": {"gated": {"a": 4.0, "b": 16.0, "c": 16.0, "d": 8.0, "e": 32.0}},      # f4x1: E against A_w, as w4h
              # pxh_pre: gated_conv_pxh_kernel with a pre-activation addend; chain: the six launches of the AFF chain against the unsplit layer;
              # sc: gated_conv_smallc_kernel (the output head)
              "pxh_pre": {"gated": {"a": 4.0, "b": 16.0, "c": 8.0, "d": 4.0, "e": 8.0}, "linear": {"a": 2.0, "b": 4.0, "c": 1.0, "d": 4.0}},      # (linear (c): R_max < 1 on every case)
              "chain": {"gated": {"a": 2.0, "b": 4.0, "e": 4.0}, "linear": {"a": 4.0, "b": 8.0, "e": 4.0}},
              # class (e) only: the two other forms of the F(4,3)-by-rows kernel, forced (the bits of f4x1: the same rows, the same cap)
              "f4x1_pair": {"gated": {"e": 32.0}}, "f4x1_wide": {"gated": {"e": 32.0}},
              "sc": {"gated": {"a": 4.0, "b": 4.0, "c": 4.0, "d": 16.0, "e": 8.0}}}


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


_FILTER_MEMO = {}


def filter_memo(w, tag, fn, also=()):
    """fn(w) for a weight array, kept for the last few arrays: the filter-side transforms of a 256 -> 256 layer cost more than
    everything else of a case on a 2 x 2 image, and the cases of one shape share their layer.  Keyed by the IDENTITY of w and of every
    array in `also` (what fn reads besides w), which the memo keeps alive.  The arrays must not be edited in place after their first
    use here — the memo cannot see that; the generators of this module finish a layer before they hand it out."""
    key = (id(w), tag) + tuple(id(a) for a in also)
    hit = _FILTER_MEMO.get(key)
    if hit is None or hit[0] is not w or any(x is not y for x, y in zip(hit[1], also)):
        while len(_FILTER_MEMO) >= 16:
            _FILTER_MEMO.pop(next(iter(_FILTER_MEMO)))
        hit = _FILTER_MEMO[key] = (w, tuple(also), fn(w))
    return hit[2]


# ------------------------------------------------------------------------------------------ reference
def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def _conv(x, w, b, stride):
    pad = (w.shape[-1] - 1) // 2
    return F.conv2d(x[None], w, b, stride=stride, padding=pad)[0]


class Ref:
    """All float64 CHW numpy arrays: f, m, Af, Am, y, B, and what the derived bound needs."""


def reference(L, x, stride=1, elu=True, residual=None, mul=None, pre=None):
    """L: dict wf, bf, wm, bm, gamma, beta, mean, var (float32 arrays); x (C, H, W) float32 (concatenated / resampled as the layer sees
    it: `assemble`); mul: FAM's second factor; residual (Cout, outH, outW); pre = (pre_f, pre_m): the pre-activation addends at OUTPUT
    resolution (`sample_addend`), added in float64: f = conv_f x + b_f + pre_f, A_f = conv(|x|, |w_f|) + |b_f| + |pre_f|; Af_own / Am_own
    keep the launch's own part (without the addend), which is what its products and its accumulation are bounded by."""
    r = Ref()
    x64 = _t64(x) * (_t64(mul) if mul is not None else 1.0)
    wf, wm, bf, bm = _t64(L["wf"]), _t64(L["wm"]), _t64(L["bf"]), _t64(L["bm"])
    ones_w = torch.ones((1,) + tuple(wf.shape[1:]), dtype=torch.float64)
    ones_x = torch.ones_like(x64)
    r.f = _conv(x64, wf, bf, stride).numpy()
    r.m = _conv(x64, wm, bm, stride).numpy()
    r.Af = _conv(x64.abs(), wf.abs(), bf.abs(), stride).numpy()
    r.Am = _conv(x64.abs(), wm.abs(), bm.abs(), stride).numpy()
    r.Af_own, r.Am_own = r.Af, r.Am
    if pre is not None:
        pf, pm = (np.asarray(p, np.float64) for p in pre)
        r.f, r.m = r.f + pf, r.m + pm
        r.Af, r.Am = r.Af + np.abs(pf), r.Am + np.abs(pm)
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


def oracle_fp32(L, x, stride=1, elu=True, residual=None, mul=None, linear=False, pre=None):
    """The torch-fp32 restatement of BasicConv on the same inputs (what oracle.unet_torch.basic_conv computes): -> (Cout or 2 Cout, H, W).
    pre = (pre_f, pre_m): fp32 addends at output resolution, added in fp32 to the fp32 pre-activations."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))       # noqa: E731
    xx = t(x) * t(mul) if mul is not None else t(x)
    f = _conv(xx, t(L["wf"]), t(L["bf"]), stride)
    m = _conv(xx, t(L["wm"]), t(L["bm"]), stride)
    if pre is not None:
        f, m = f + t(pre[0]), m + t(pre[1])
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
    A, W1 = (ref.Af_own, ref.W1f) if which == "f" else (ref.Am_own, ref.W1m)     # (the launch's own products: an addend is not among them)
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
    Uabs = filter_memo(L["w" + which], "wino", lambda a: np.ascontiguousarray(np.abs(np.einsum("ia,ocab,jb->ijco", G, np.asarray(a, np.float64), G))))

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
    inv_s = filter_memo(w, "wino 1/s", wino_filter_inv_scale)[:, None, None]
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
    Uabs = filter_memo(L["w" + which], "f4x1", lambda a: np.ascontiguousarray(np.abs(np.einsum("fb,ocab->faco", G.astype(np.float64), np.asarray(a, np.float64)))))   # [fq][ky][cin][co]
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
    inv_s = filter_memo(w, "f4x1 1/s", f4x1_filter_inv_scale)[:, None, None]
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


# ------------------------------------------------------------------------------------------ resampled sources and addends
def assemble(xs, shifts, H, W):
    """The nearest-resampled concatenation as the loader of gated_conv_pxh_kernel addresses it (sy = (ly << sl) >> sr, one of sl, sr zero:
    conv_prepare): xs[i] (C_i, h_i, w_i), source pixel = dst << s for s > 0 (a finer source, sub-sampled), dst >> -s for s < 0 (a coarser
    one, repeated) -> (sum C_i, H, W).  Plain index arrays: an index past a source raises."""
    out = []
    for x, s in zip(xs, shifts):
        iy, ix = ((np.arange(n) << s) if s >= 0 else (np.arange(n) >> -s) for n in (H, W))
        out.append(np.asarray(x)[:, iy[:, None], ix[None, :]])
    return np.concatenate(out, 0)


def sample_addend(t_hwc, f_off, m_off, cout, shift, H, W):
    """The pre-activation addend as the epilogues address it (pp = pre + ((y >> pre_shift) preW + (x >> pre_shift)) pre_cstride, then
    pre_foff + c, pre_moff + c): t (preH, preW, C) -> (pre_f, pre_m), each (cout, H, W), dtype of t."""
    t = np.asarray(t_hwc)
    px = t[(np.arange(H) >> shift)[:, None], (np.arange(W) >> shift)[None, :]]
    return (np.ascontiguousarray(px[..., off:off + cout].transpose(2, 0, 1)) for off in (f_off, m_off))


def preact_bound_addend(L, ref, family, which, total, d_pre=0.0):
    """|got - f| <= this for a launch with an addend (module docstring, "A launch with an addend"): the launch's own bound, the rounding
    of f1 + pre against the finished value `total`, and the addend's own error d_pre sampled as the addend is (0: given by the host)."""
    return preact_bound_direct(L, ref, family, which) + U * np.abs(total) + d_pre


# The AFF launch chain of the default plan (read_amd/csrc/unet.cpp, `if (g_unet_aff_split)`), one row per launch in the plan's order:
# name, columns of the 480-channel concatenation [res1 32 | res2 64 | res3 128 | z 256] that the launch multiplies, AFF layers whose rows it
# stacks ([f0 f1 f2 | m0 m1 m2]), (source, shift) list, linear, addend (name, f_off, m_off, shift), level of the output, and the sources
# (with shifts) of the UNSPLIT layer restricted to the columns from this launch's first on — what the launch's output stands for.
AFF_PLAN = (("q3", (224, 480), (0, 1, 2), ((3, 0),), True, None, 3, ((3, 0),)),
            ("q2", (96, 224), (0, 1), ((2, 0),), True, ("q3", 0, 224, 1), 2, ((2, 0), (3, -1))),
            ("a2", (0, 224), (2,), ((0, 2), (1, 1), (2, 0)), False, ("q3", 96, 320, 1), 2, ((0, 2), (1, 1), (2, 0), (3, -1))),
            ("q1", (32, 96), (0,), ((1, 0),), True, ("q2", 0, 96, 1), 1, ((1, 0), (2, -1), (3, -2))),
            ("a1", (0, 96), (1,), ((0, 1), (1, 0)), False, ("q2", 32, 128, 1), 1, ((0, 1), (1, 0), (2, -1), (3, -2))),
            ("a0", (0, 32), (0,), ((0, 0),), False, ("q1", 0, 32, 1), 0, ((0, 0), (1, -1), (2, -2), (3, -3))))


def part_layer(layers, c0, c1, own_bias):
    """The rows of `layers` stacked, restricted to input columns c0 .. c1 - 1; zero bias unless own_bias (`derive` of unet.cpp: the bias
    stays with the launch at the layer's own level)."""
    cat = lambda key: np.concatenate([np.asarray(L[key]) for L in layers])                       # noqa: E731
    P = {key: cat(key) for key in ("gamma", "beta", "mean", "var")}
    for fm in "fm":
        P["w" + fm] = np.ascontiguousarray(cat("w" + fm)[:, c0:c1])
        P["b" + fm] = cat("b" + fm) if own_bias else np.zeros(P["w" + fm].shape[0], np.float32)
    return P


def run_aff_chain(layers, xs, launch):
    """The six launches in the plan's order.  launch(name, L_part, [(x_i, shift)], pre, linear, (H, W) of the output) -> the launch's
    output, in whatever form the caller's next launch takes as pre = (that output, f_off, m_off, shift).  -> {name: output}."""
    outs = {}
    for name, (c0, c1), li, srcs, linear, pre, level, _ in AFF_PLAN:
        Lp = part_layer([layers[i] for i in li], c0, c1, own_bias=not linear)
        outs[name] = launch(name, Lp, [(xs[i], s) for i, s in srcs], None if pre is None else (outs[pre[0]],) + tuple(pre[1:]), linear,
                            xs[level].shape[1:])
    return outs


def aff_chain_inputs(cls, sizes=((20, 36), (10, 18), (5, 9), (3, 5))):
    """-> (three AFF layers 480 -> 32 / 64 / 128, the sources res1 32, res2 64, res3 128, z 256 at their levels).  Class (a): tame_layer and
    unit-scale sources.  Class (b): ONE checkpoint_like layer of 224 rows cut into the three (rows 0 .. 31, 32 .. 95, 96 .. 223), so that
    all three share the per-input-channel scales 2^U(-8, 8) that the sources carry.  Without the packers' edge rows: the linear launches
    have zero bias, so the row of fp32-denormal weights gives pre-activations of ~1e-38 with A_f of the same size — there the whole
    result is inside TINY and E against u A_f measures nothing (8e6 on an MI355X, at 0.33 of the derived bound); the edge rows run with
    addends in class (b) of the single launches, where the bias is the layer's own."""
    chans = (32, 64, 128, 256)
    offs = np.cumsum((0,) + chans)
    if cls == "a":
        rng = np.random.default_rng([73, 480])
        layers = [tame_layer(480, 32 << i, 1, 73 + i) for i in range(3)]
        x = rng.standard_normal((480,) + tuple(sizes[0])).astype(np.float32)
    else:
        L, x = checkpoint_like(480, 224, 1, sizes[0][0], sizes[0][1], 74, edge_rows=False)
        rows = np.cumsum((0, 32, 64, 128))
        layers = [{key: np.ascontiguousarray(v[rows[i]:rows[i + 1]]) for key, v in L.items()} for i in range(3)]
    return layers, [np.ascontiguousarray(x[offs[k]:offs[k + 1], :h, :w]) for k, (h, w) in enumerate(sizes)]


def aff_chain_reference(layers, xs, family="pxh"):
    """-> {name: (ref, d_f, d_m, L, x)}: the float64 reference of the UNSPLIT layer L (for q_k: its stacked rows over the columns from part
    k on) on x = assemble(...), and the bound composed level by level (module docstring, "The chain"):
    d(q_k) = preact_bound_direct(part k) + up(d(q_k+1)) + u |q_k|."""
    out = {}
    for name, (c0, c1), li, srcs, linear, pre, level, full_srcs in AFF_PLAN:
        H, W = xs[level].shape[1:]
        Ls = [layers[i] for i in li]
        Lfull, xfull = part_layer(Ls, c0, 480, own_bias=not linear), assemble([xs[i] for i, _ in full_srcs], [s for _, s in full_srcs], H, W)
        full = reference(Lfull, xfull)
        Lp = part_layer(Ls, c0, c1, own_bias=not linear)
        own = reference(Lp, assemble([xs[i] for i, _ in srcs], [s for _, s in srcs], H, W))
        d = []
        for j, fm in enumerate("fm"):
            b = preact_bound_direct(Lp, own, family, fm)
            if pre is not None:
                dq_f, dq_m = out[pre[0]][1:3]
                dq = np.concatenate([dq_f, dq_m]).transpose(1, 2, 0)
                b = b + U * np.abs(full.f if fm == "f" else full.m) + tuple(sample_addend(dq, pre[1], pre[2], b.shape[0], pre[3], H, W))[j]
            d.append(b)
        out[name] = (full, d[0], d[1], Lfull, xfull)
    return out


# ------------------------------------------------------------------------------------------ the output head and the up-sampling
def preact_bound_sc(L, ref, which):
    """|got - f| <= this for gated_conv_smallc_kernel (module docstring, "The output head")."""
    w = L["w" + which]
    A, val = (ref.Af_own, ref.f) if which == "f" else (ref.Am_own, ref.m)
    return SECOND_ORDER * U * (w.shape[1] * w.shape[2] * w.shape[3]) * A + U * np.abs(val) + TINY


def bilinear_up4_ref(x):
    """nn.Upsample(scale_factor=4, mode='bilinear', align_corners=False) restated from the formula (src = 0.25 (dst + 0.5) - 0.5 clamped at
    0, the upper neighbour clamped at the last index): x (C, h, w) float32 -> (value, sum w |v|), each (C, 4 h, 4 w) float64."""
    def axis(n):
        s = np.maximum(0.25 * (np.arange(4 * n) + 0.5) - 0.5, 0.0)
        i0 = np.floor(s).astype(np.int64)
        return i0, i0 + (i0 < n - 1), 1.0 - (s - i0), s - i0

    (y0, y1, ly0, ly1), (x0, x1, lx0, lx1) = axis(x.shape[1]), axis(x.shape[2])

    def interp(v):
        top, bot = (v[:, r][:, :, x0] * lx0 + v[:, r][:, :, x1] * lx1 for r in (y0, y1))
        return ly0[None, :, None] * top + ly1[None, :, None] * bot

    v = np.asarray(x, np.float64)
    return interp(v), interp(np.abs(v))


def bilinear_up4_bound(absum):
    """|got - value| <= this (module docstring, "bilinear_up4_kernel"); absum = sum w |v| of bilinear_up4_ref."""
    return SECOND_ORDER * 4 * U * absum + TINY


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


SENTINEL = -7.0


def source_sizes(shifts, H, W):
    """The size of each source of a resampled concatenation at output size H x W: H << s for a finer source (whole, so that the first
    source's size >> s gives H back), ((H - 1) >> -s) + 1 for a coarser one — the smallest that conv_prepare accepts."""
    return [(H << s, W << s) if s >= 0 else (((H - 1) >> -s) + 1, ((W - 1) >> -s) + 1) for s in shifts]


def split_sources(x_big, split, shifts, H, W):
    """x_big (sum split, H << max shift, W << max shift) -> the sources, each the top-left corner of its channels at its own size."""
    offs = np.cumsum([0] + list(split))
    return [np.ascontiguousarray(x_big[offs[i]:offs[i + 1], :h, :w]) for i, (h, w) in enumerate(source_sizes(shifts, H, W))]


def addend_size(shift, H, W):
    return ((H - 1) >> shift) + 1, ((W - 1) >> shift) + 1


def addend_tensor(rng, shape_hwc, f_off, m_off, cout, scale=1.0):
    """(preH, preW, C) float32: standard normal times `scale` (a number or one value per output channel) in the channels the launch reads,
    SENTINEL in every other one."""
    t = np.full(shape_hwc, SENTINEL, np.float32)
    for off in (f_off, m_off):
        t[..., off:off + cout] = (rng.standard_normal(shape_hwc[:2] + (cout,)) * scale).astype(np.float32)
    return t


def cancelling_addend(t, own_f64, f_off, shift):
    """The f slice of t replaced by -fl32(own pre-activation) of the top-left output pixel of every addend pixel: there the launch's own sum
    and the addend cancel to the rounding of the former, |f| << A_f; the other pixels of the block see an addend of the same size."""
    t = t.copy()
    st = 1 << shift
    t[..., f_off:f_off + own_f64.shape[0]] = -own_f64[:, ::st, ::st].astype(np.float32).transpose(1, 2, 0)
    return t


def addend_impulse_spots(pre_hw, cout):
    """(row, column, channel) of single addend elements: the four corners and the last row / last column (shared by the odd rest of the
    output) at channel 1, and the channels at the quad, half-wave and group boundaries (0, 3, 4, 31, 32, Cout - 1) at the last corner."""
    ph, pw = pre_hw
    spots = [(y, x_, 1) for (y, x_) in ((0, 0), (0, pw - 1), (ph - 1, 0), (ph - 1, pw - 1), (ph - 1, pw // 2), (ph // 2, pw - 1))]
    spots += [(ph - 1, pw - 1, c) for c in sorted({0, 3, 4, 31, 32, cout - 1}) if c < cout]
    return list(dict.fromkeys(spots))


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


# ------------------------------------------------------------------------------------------ class (e): degenerate sizes
# (C, H, W) of the 3x3 / stride-1 C -> C families: the plan's own levels at a 16 x 16 viewport (32 x 16 x 16 ... 256 x 2 x 2), their
# 16 x 48 / 48 x 16 neighbours, and smaller: one pixel, one row, one column, one pixel more than a unit's width, two columns.
SHAPES_E_S1 = [(256, 2, 2), (256, 2, 6), (256, 6, 2), (128, 4, 4), (128, 4, 12), (128, 1, 1), (64, 8, 8), (64, 1, 7), (64, 7, 1), (64, 3, 5),
               (32, 16, 16), (32, 2, 33), (32, 9, 2)]
# (cin, cout, k, input H, W) of the stride-2 family: every output is non-empty (k3: ((H - 1) >> 1) + 1, k4: H >> 1)
SHAPES_E_S2 = [(32, 64, 3, 16, 16), (32, 64, 3, 2, 2), (32, 64, 3, 1, 1), (32, 64, 3, 3, 3), (32, 64, 3, 2, 6), (64, 128, 3, 8, 8), (64, 128, 3, 1, 5),
               (128, 256, 3, 4, 4), (128, 256, 3, 2, 2), (256, 128, 4, 2, 2), (256, 128, 4, 2, 6), (128, 64, 4, 4, 4), (64, 32, 4, 8, 8), (64, 32, 4, 2, 2)]
SHAPES_E_PXH = [([256], 256), ([128, 128], 128), ([8, 56], 64)]           # (sources, cout) at SIZES_E_PXH
SIZES_E_PXH = [(1, 1), (2, 2), (2, 6), (4, 4), (7, 1)]
SHAPES_E_T3H = [(8, 32), (8, 16)]                                          # (cin, cout) at SIZES_E_T3H
SIZES_E_T3H = [(1, 1), (2, 2), (2, 6), (16, 16), (5, 1)]
SIZES_E_SC = [(1, 1), (2, 2), (16, 16), (7, 33), (16, 1)]                  # the 32 -> 3 head
# SHAPES_RESAMPLED's first layout at outputs whose coarse source is 2 x 2 / one pixel (the fine one 8 x 8 / 4 x 4)
SHAPES_E_RESAMPLED = [([32, 64, 128], (1, 0, -1), 64, 4, 4), ([32, 64, 128], (1, 0, -1), 64, 2, 2)]
# the three AFF layouts of SHAPES_PRE at outputs 2 x 2, 4 x 4, 8 x 8: the addend, one level coarser, has 1, 2 and 4 rows
LAYOUTS_E_PRE = [([32], (0,), 32, 64, 0, 32, 1), ([32, 64], (1, 0), 64, 192, 32, 128, 1), ([32, 64, 128], (2, 1, 0), 128, 448, 96, 320, 1)]
SIZES_E_PRE = [(2, 2), (4, 4), (8, 8)]
SIZES_E_CHAIN = ((16, 16), (8, 8), (4, 4), (2, 2))                         # res1, res2, res3, z of a 16 x 16 viewport


def degenerate_positions(H, W):
    """(y, x) of the impulses of class (e): every pixel where H W <= 16, else the four corners, the mid-edges and the centre.  A list
    of its own: impulse_positions assumes an image that holds the patch of tile (1, 1)."""
    if H * W <= 16:
        return [(y, x_) for y in range(H) for x_ in range(W)]
    pos = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1), (H // 2, W // 2)]
    return list(dict.fromkeys(pos))


def degenerate_images(cin, H, W, seed):
    """The inputs of class (e) at one shape: (name, x (cin, H, W) float32, elu, unit_scale).  Unit scale, a constant 1, a checkerboard,
    impulses of 1 and 2^-10 at degenerate_positions in channels 1 % cin and cin - 1; ELU alternates over the list."""
    rng = np.random.default_rng([seed, cin, H, W])
    yield "unit scale", rng.standard_normal((cin, H, W)).astype(np.float32), seed % 2 == 0, True
    yield "constant 1", constant_image(cin, H, W), True, False
    yield "checkerboard +-1", checkerboard(cin, H, W), False, False
    j = 0
    for amp in (1.0, 2.0 ** -10):
        for c in dict.fromkeys((1 % cin, cin - 1)):
            for (y, x_) in degenerate_positions(H, W):
                yield f"impulse {amp:g} at c{c} ({y},{x_})", impulse(cin, H, W, c, y, x_, amp), j % 2 == 0, False
                j += 1
