"""The forward linear launches of the training step (read_amd/train.py: GatedConvFn.forward -> _linear_conv -> read_gated_conv_forward
with linear = 1): the layers, sizes, input classes and stacked geometries the accuracy tests use, the float64 references with the derived
bounds of tests/train_ref64.py, and ONE set of assertions over the buffers a launch leaves behind.  tests/test_gpu_train_forward_accuracy.py
hands those assertions the device's buffers, tests/test_train_accuracy_cpu.py the buffers of the NumPy fp32 restatement
(tests/train_fp32.py: linear_launch32) — unchanged, and with each defect of the mutation catalogue built in.  No GPU, no read_amd.

LAYERS: the distinct (cin, cout, k, stride) of tests/unet_spec.py, one per route and epilogue branch, plus the padded shapes; `switch`
names the module switch of read_amd.train that is turned OFF for the row (None: the defaults)."""
import numpy as np

from tests import conv_ref64 as R64
from tests import train_ref64 as T
from tests.train_fp32 import GUARD, SENTINEL

f32 = np.float32

LAYERS = {
    "direct": [(8, 16, 3, 1, None), (8, 32, 3, 1, None), (8, 64, 3, 1, None),                                   # fwd_kc = 8
               (480, 32, 1, 1, None), (64, 56, 1, 1, None), (256, 128, 1, 1, None), (16, 32, 1, 1, None),        # k1
               (32, 64, 3, 2, None), (128, 256, 3, 2, None), (64, 32, 4, 2, None), (256, 128, 4, 2, None),       # stride 2
               (32, 32, 3, 1, "USE_WINOGRAD")],                                                                  # the 3x3 / s1 layer of all three kernels
    "w2": [(16, 32, 3, 1, None), (32, 3, 3, 1, None), (64, 3, 3, 1, None), (32, 32, 3, 1, "USE_W4"), (48, 20, 3, 1, None)],
    "w4": [(32, 32, 3, 1, None), (64, 64, 3, 1, None), (128, 128, 3, 1, None), (256, 256, 3, 1, None), (48, 40, 3, 1, None),
           (32, 8, 3, 1, None), (64, 24, 3, 1, None)],
}
SIZES = {1: ((9, 21), (12, 20)), 2: ((8, 12), (9, 13))}             # partial tiles in both directions, more than one tile row
GEOMETRIES = ((21, 9, 7, 5), (10, 21, 5, 3), (12, 20, 4, 4))        # (H, W, block_h, valid_h): nb = 3, 2, 3; separators across the 2- / 4- / 8-row tiles
F_EDGES = (-100.0, -0.0, 0.0, 1e-40, 1e4, -60.0, 1e-6, 100.0)       # b_f of class (d): T.range_edge_case's values for f, a subnormal, both zeros
M_EDGES = (150.0, -150.0, 88.0, -88.0, 0.0, 40.0)                   # b_m: past and at the edge of v_exp_f32's range, and range_edge_case's 40


def layer_name(layer):
    cin, cout, k, stride = layer[:4]
    return f"{cin}->{cout} k{k} s{stride}"


class Case:
    """One input of one layer: L (wf, bf, wm, bm, gamma, beta, mean, var: float32), x (cin, H, W) float32; the float64 reference and the
    derived bounds are computed once and shared by every launch of the case."""

    def __init__(self, layer, hw, cls, kind, L, x):
        self.cin, self.cout, self.k, self.stride = layer[:4]
        self.H, self.W = hw
        self.cls, self.kind, self.L, self.x = cls, kind, L, x
        self.oh, self.ow = T.out_hw(self.k, self.stride, self.H, self.W)
        self.name = f"{layer_name(layer)} {self.H}x{self.W} {kind}"
        self._ref, self._bounds = None, {}

    def ref(self):
        if self._ref is None:
            self._ref = R64.reference(self.L, self.x, stride=self.stride)
        return self._ref

    def bounds(self, family):
        """-> (d_f, d_m, cond_f, cond_m), each (cout, oh, ow)."""
        if family not in self._bounds:
            (df, cf), (dm, cm) = (T.conv_forward_bound(self.L, self.x, self.ref(), family, w) for w in "fm")
            self._bounds[family] = (df, dm, cf, cm)
        return self._bounds[family]


def bias_edges(cout, shift):
    c = np.arange(cout) + shift
    return np.array(F_EDGES, f32)[c % len(F_EDGES)], np.array(M_EDGES, f32)[(c // len(F_EDGES) + c) % len(M_EDGES)]


SIZES_TINY = ((2, 2), (4, 4), (1, 1))                               # the coarse levels of a 16-pixel crop: smaller than any tile of the three kernels


def impulse_spots(cin, H, W):
    """(channel, y, x) of the impulses of class (c): the two corners and a pixel of the second tile row; on an image that does not hold
    that pixel (SIZES_TINY) every pixel (R64.degenerate_positions), the channels 0, cin - 1 and an odd middle one in turn."""
    if H > 4 and W > 2:
        return ((0, 0, 0), (cin - 1, H - 1, W - 1), ((cin // 2) | 1, 4, min(16, W - 2)))
    chans = (0, cin - 1, (cin // 2) | 1)
    return tuple((chans[j % 3], y, x_) for j, (y, x_) in enumerate(R64.degenerate_positions(H, W)))


def cases(layer, hw, classes="abcd"):
    """The cases of one layer at one size: (a) unit scale; (b) checkpoint-like: per-channel scales T.scales_b on the inputs and on the 2 Cout
    weight rows (the biases follow their rows), BatchNorm statistics of R64.checkpoint_like; (c) impulses of 1.0 over small-integer weights,
    a constant image, a checkerboard; (d) all-zero weights under the bias edges F_EDGES x M_EDGES."""
    cin, cout, k, stride = layer[:4]
    H, W = hw
    seed = 1000 * cin + cout + 7 * k + stride
    rng = np.random.default_rng([seed, H, W])
    tame = R64.tame_layer(cin, cout, k, seed)
    if "a" in classes:
        yield Case(layer, hw, "a", "unit scale", dict(tame), rng.standard_normal((cin, H, W)).astype(f32))
    if "b" in classes:
        L = dict(tame)
        s_in, s_row = T.scales_b(cin, rng), T.scales_b(2 * cout, rng)
        level = float(np.sqrt((s_in ** 2).mean()))
        for j, fm in enumerate("fm"):
            rows = s_row[j * cout:(j + 1) * cout]
            L["w" + fm] = (tame["w" + fm] * rows[:, None, None, None]).astype(f32)
            L["b" + fm] = (tame["b" + fm] * rows * level).astype(f32)
        L.update({key: v for key, v in R64.checkpoint_like(8, cout, 1, 2, 2, seed, edge_rows=False)[0].items() if key in ("gamma", "beta", "mean", "var")})
        yield Case(layer, hw, "b", "checkpoint-like", L, (rng.standard_normal((cin, H, W)) * s_in[:, None, None]).astype(f32))
    if "c" in classes:
        L = dict(tame)
        L["wf"], L["wm"] = T.small_integers((cout, cin, k, k), rng), T.small_integers((cout, cin, k, k), rng)
        for (c, y, x_) in impulse_spots(cin, H, W):
            yield Case(layer, hw, "c", f"impulse c{c} ({y},{x_})", L, R64.impulse(cin, H, W, c, y, x_, 1.0))
        yield Case(layer, hw, "c", "constant 1", dict(tame), R64.constant_image(cin, H, W))
        yield Case(layer, hw, "c", "checkerboard", dict(tame), R64.checkerboard(cin, H, W))
    if "d" in classes:
        L = dict(tame)
        L["wf"], L["wm"] = np.zeros_like(tame["wf"]), np.zeros_like(tame["wm"])
        L["bf"], L["bm"] = bias_edges(cout, H)
        yield Case(layer, hw, "d", "bias edges", L, rng.standard_normal((cin, H, W)).astype(f32))


def bn_of(L, identity):
    """The BatchNorm parameters a launch's params block stands for: the layer's own (eval mode), or scale 1 / shift 0 (identity_bn, what the
    batch-statistics mode packs: gamma 1, var 1, eps 0 — restated for references that add EPS as var = 1 - EPS)."""
    cout = L["wf"].shape[0]
    if not identity:
        return {key: L[key] for key in ("gamma", "beta", "mean", "var")}
    return dict(gamma=np.ones(cout, f32), beta=np.zeros(cout, f32), mean=np.zeros(cout, f32), var=np.full(cout, 1.0 - T.EPS, np.float64))


def scale_shift32(L, identity):
    """(sc, sh) as the packer's params block holds them (pack_params_body of train.hip, the host packer's expressions)."""
    cout = L["wf"].shape[0]
    if identity:
        return np.ones(cout, f32), np.zeros(cout, f32)
    sc = (L["gamma"] / np.sqrt((L["var"] + f32(T.EPS)).astype(f32)).astype(f32)).astype(f32)
    return sc, (L["beta"] - (L["mean"] * sc).astype(f32)).astype(f32)


def regate(ref, bn, elu):
    """The reference of the same pre-activations under other BatchNorm parameters / another activation: conv_ref64.reference's gate part."""
    r = R64.Ref()
    r.__dict__.update(ref.__dict__)
    g64, be, mu, va = (np.asarray(bn[key], np.float64)[:, None, None] for key in ("gamma", "beta", "mean", "var"))
    Ss = g64 / np.sqrt(va + T.EPS)
    r.S, r.T, r.mean_S = np.abs(Ss), be - mu * Ss, np.abs(mu) * np.abs(Ss)
    r.elu = elu
    r.g = np.where(r.f > 0, r.f, np.expm1(np.minimum(r.f, 0.0))) if elu else r.f
    r.dact = np.where(r.f > 0, 1.0, np.exp(np.minimum(r.f, 0.0))) if elu else np.ones_like(r.f)
    r.y = Ss * r.g * r.sig + r.T
    return r


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _hwc(a_chw):
    return np.ascontiguousarray(a_chw.transpose(1, 2, 0))


TABLE = {"direct": "fwd_direct", "w2": "fwd_w2", "w4": "fwd_w4"}


def check_preactivations(case, family, fm_buf, judge, fail, yard=None):
    """Assertion 1 on the flat buffer of a launch (oh ow 2 cout floats, then GUARD sentinels): the guard band, every pre-activation under
    the derived bound (and what else `judge` holds a row to), the exact rows of classes (c) and (d).  -> fm (oh, ow, 2 cout)."""
    cout, n = case.cout, case.oh * case.ow * 2 * case.cout
    what = f"{TABLE[family]} ({case.cls}) {case.name}"
    if fm_buf.size != n + GUARD or not np.array_equal(_bits(fm_buf[n:]), _bits(np.full(GUARD, SENTINEL))):
        fail(f"{what}: the launch wrote past the end of fm")
    fm = fm_buf[:n].reshape(case.oh, case.ow, 2 * cout)
    ref = case.ref()
    df, dm, cf, cm = case.bounds(family)
    got = fm.transpose(2, 0, 1)
    judge(TABLE[family], case.cls, case.name, got, np.concatenate([ref.f, ref.m]), np.concatenate([cf, cm]), np.concatenate([df, dm]), yard or {})
    bias = np.concatenate([case.L["bf"], case.L["bm"]]).astype(f32)[:, None, None]
    if case.kind.startswith("impulse") and family == "direct":
        # one product of 1.0 and an integer weight per output: the integer plus the bias, one rounding
        whole = np.rint(np.concatenate([ref.f, ref.m]) - bias.astype(np.float64)).astype(f32)
        if not np.array_equal(got, (whole + bias).astype(f32)):
            fail(f"{what}: the impulse does not read the integer weights back exactly")
    if case.cls == "d":
        # no product reaches the output: the accumulators are +0 and the stored value is the fp32 sum 0 + b (b itself; +0 for b = -0)
        want = np.broadcast_to((f32(0) + bias).astype(f32), got.shape)
        if not np.array_equal(_bits(got), _bits(want)):
            fail(f"{what}: fm differs from the bias where every weight is zero")
    return fm


def check_gated(case, family, fm, y_buf, elu, identity, block_h, valid_h, judge, fail, yard_own=None, yard_layer=None, unstacked=None):
    """Assertions 2 and 3 on the fused gate's flat buffer (oh ow cout floats, then GUARD sentinels) of a launch whose pre-activations are
    fm: (i) against the float64 gate of fm itself under the gate kernel's bound, (ii) against the float64 layer under gated_bound composed
    from the pre-activation bounds, the separator rows +0.0, the constants where no product reaches y, and — unstacked = (fm, y) of the
    same input without block geometry — every valid row bit-identical to it.  -> y (oh, ow, cout)."""
    cout, P = case.cout, case.oh * case.ow
    tag = f"{'elu' if elu else 'lin'} {'identity' if identity else 'eval'} block {block_h}/{valid_h}"
    what = f"fwd_gate[{family}] ({case.cls}) {case.name} {tag}"
    if y_buf.size != P * cout + GUARD or not np.array_equal(_bits(y_buf[P * cout:]), _bits(np.full(GUARD, SENTINEL))):
        fail(f"{what}: the launch wrote past the end of y")
    y = y_buf[:P * cout].reshape(case.oh, case.ow, cout)
    bn = bn_of(case.L, identity)
    fm2, y2 = fm.reshape(P, 2 * cout), y.reshape(P, cout)
    valid = T.valid_rows(P, case.ow, block_h, valid_h)
    # (i) the epilogue alone
    y_ref, B, bound, _ = T.gate_forward_ref(fm2, cout, bn, elu, None, case.ow, block_h, valid_h)
    gt = T.Gate(fm2, cout, elu)
    Ss = T.bn_scale(bn["gamma"], bn["var"])[None]
    mean_S, shift = np.abs(np.asarray(bn["mean"], np.float64))[None] * np.abs(Ss), np.asarray(bn["beta"], np.float64)[None] - np.asarray(bn["mean"], np.float64)[None] * Ss
    lead = T.U * (6.5 * np.abs(Ss * gt.g) + 4.5 * mean_S + 2 * np.abs(shift) + np.abs(y_ref)) * valid[:, None]
    judge("fwd_gate", case.cls, f"{case.name} [{family}] {tag} (i)", y2, y_ref, B, bound, yard_own or {}, lead=lead)
    if _bits(y2[~valid]).any():
        fail(f"{what}: separator rows of y are not +0.0")
    sc, sh = scale_shift32(case.L, identity)
    const = ((np.asarray(bn["gamma"]) == 0)[None] | (fm2[:, :cout] == 0)) & valid[:, None]      # sc = 0, or act(f) = 0: no product reaches y
    sh_fused = (np.asarray(bn["beta"], np.float64) - np.asarray(bn["mean"], np.float64) * sc.astype(np.float64)).astype(f32)     # beta - mean sc as one fma
    if const.any() and not (np.equal(y2, sh[None]) | np.equal(y2, sh_fused[None]))[const].all():
        fail(f"{what}: outputs that no product reaches differ from the shift")
    # (ii) the layer end to end: gated_bound from the pre-activation bounds, plus the flush of v_exp_f32 / v_rcp_f32 results below the
    # normal range as gate_forward_ref allows it (FLUSH S (1 + |act(f)|): sigmoid(-88) is subnormal and f reaches 1e4 in class (d))
    ref = regate(case.ref(), bn, elu)
    df, dm, cf, cm = case.bounds(family)
    v3 = valid.reshape(case.oh, case.ow)[None]
    b2 = (R64.gated_bound(ref, df, dm) + T.FLUSH * ref.S * (1 + np.abs(ref.g))) * v3
    Bw = (ref.S * (np.abs(ref.dact) * ref.sig * cf + np.abs(ref.g) * ref.sig * (1.0 - ref.sig) * cm) + np.abs(ref.y)) * v3
    lead = T.U * (6.5 * ref.S * np.abs(ref.g * ref.sig) + 4.5 * ref.mean_S + 2 * np.abs(ref.T) + np.abs(ref.y)) * v3
    judge("fwd_gate", case.cls, f"{case.name} [{family}] {tag} (ii)", y.transpose(2, 0, 1), ref.y * v3, Bw, b2, yard_layer or {}, lead=lead)
    if unstacked is not None:
        fm0, y0 = unstacked
        if not np.array_equal(_bits(fm), _bits(fm0)):
            fail(f"{what}: fm changed with the block geometry (the kernel must not mask it)")
        if not np.array_equal(_bits(y2[valid]), _bits(y0.reshape(P, cout)[valid])):
            fail(f"{what}: valid rows of y differ from the unstacked launch")
    return y


def bound_judge(fails):
    """A `judge` for buffers that did not come from the device: rule 1 alone (the derived bound, elementwise) and finiteness.  Records
    err / bound of every row in .ratios."""
    def judge(family, cls, name, got, ref, cond, bound, yard, lead=None, **_):
        got = np.asarray(got, np.float64)
        q = T.worst(np.abs(np.nan_to_num(got, nan=3e38, posinf=3e38, neginf=-3e38) - ref), bound)
        judge.ratios.append((family, cls, name, q))
        if not (q <= 1.0 and np.isfinite(got).all()):
            fails.append(f"{family} ({cls}) {name}: {q:.3f} x the derived bound")
    judge.ratios = []
    return judge
