"""CPU: the NumPy restatements of the split-operand convolution kernels (tests/d3h_ref.py, tests/wino4h_ref.py, the F(4,3)-by-rows
model of tests/test_f4x1_model.py, with the library's own host packers) held to the float64 reference, the derived bounds and the measured caps of tests/conv_ref64.py — on unit-scale,
checkpoint-like, structured and range-edge inputs — and the DETECTION POWER of those caps: the same arithmetic with one seeded defect
each must exceed them.  The restatements sum in float64 where the device rounds per MFMA, so the intact models sit well inside the caps;
what this module establishes is that the inputs are such that correct split arithmetic passes (floors included) and that broken split
arithmetic does not.  The kernels themselves: tests/test_gpu_conv_accuracy.py."""
import numpy as np
import pytest

from tests import conv_ref64 as R64
from tests.d3h_ref import pack_d1h_blob, pack_d3h_blob, split_conv_model, split_conv_model_taps


# ------------------------------------------------------------------------------------------ plumbing
def im2col(x_chw, k, stride, clamped=False):
    """-> (outH, outW, k k Cin), index tap * Cin + ci (the order of read_conv_pack_t3h_host), zero padding (k - 1) // 2.  clamped: a
    seeded defect — the border taken by clamping the coordinate instead of padding with zeros."""
    cin, H, W = x_chw.shape
    pad = (k - 1) // 2
    oh, ow = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    xp = np.zeros((cin, H + 2 * pad + stride, W + 2 * pad + stride), np.float32)
    xp[:, pad:pad + H, pad:pad + W] = x_chw
    if clamped:
        xp = np.pad(x_chw, ((0, 0), (pad, pad + stride), (pad, pad + stride)), mode="edge").astype(np.float32)
    taps = [xp[:, ky:ky + stride * oh:stride, kx:kx + stride * ow:stride] for ky in range(k) for kx in range(k)]
    return np.ascontiguousarray(np.concatenate(taps, 0).transpose(1, 2, 0))


def w_matrix(w):
    return np.ascontiguousarray(w.transpose(0, 2, 3, 1).reshape(w.shape[0], -1))


def split_model(cols, w2, defect=None):
    """tests/d3h_ref.split_conv_model_taps, copied so that ONE line at a time can be broken (defect = None: the same arithmetic)."""
    cout, K = w2.shape
    mx = np.abs(w2.astype(np.float64)).max(axis=1)
    ex = np.zeros(cout, np.int64)
    nz = mx > 0
    ex[nz] = np.clip(15 - np.frexp(mx[nz])[1], -60, 60)
    if defect == "scale_binade":
        ex[nz] += 1                                              # the row's largest entry lands in [2^15, 2^16)
    ws = np.ldexp(w2.astype(np.float64), ex[:, None])
    with np.errstate(over="ignore", invalid="ignore"):
        wh = ws.astype(np.float16)
        r = ws - wh.astype(np.float64)
        wl = r.astype(np.float16)
        if defect == "wl_truncated":                             # toward zero instead of to nearest
            over = np.abs(wl.astype(np.float64)) > np.abs(r)
            wl = np.where(over, np.nextafter(wl, np.float16(0)), wl)
        wl = wl.astype(np.float64)
        whs = (wh * np.float16(2.0 ** -11)).astype(np.float16).astype(np.float64)
        wh = wh.astype(np.float64)
        xh = cols.astype(np.float16)
        if defect == "xl_unscaled":                              # the low piece kept at its own scale: it underflows f16
            xl = (cols - xh.astype(np.float32)).astype(np.float16).astype(np.float64)
            whs = wh
        else:
            xl = ((cols - xh.astype(np.float32)) * np.float32(2048.0)).astype(np.float16).astype(np.float64)
        xh = xh.astype(np.float64)
        t_hl = xl @ whs.T if defect != "drop_wh_xl" else 0.0
        t_lh = xh @ wl.T if defect != "drop_wl_xh" else 0.0
        out = t_hl + t_lh + xh @ wh.T
        return (out * np.ldexp(1.0, -ex)[None, None, :]).astype(np.float32)


GEOMETRY_DEFECTS = ("border_clamped", "ragged_unwritten")      # of the launch around the arithmetic: class (e) must catch them


def run_direct(L, x, k, stride, family, model=split_model, defect=None, cls="a"):
    """One layer's pre-activations [f | m] through a model -> dict of E, R, the worst err / derived bound, finiteness.  The defects of
    GEOMETRY_DEFECTS leave the arithmetic alone: the border by clamping; the outputs of a ragged last 4 x 4 tile left as they were
    (R64.SENTINEL, what the tests fill an output with)."""
    ref = R64.reference(L, x, stride=stride)
    cols = im2col(x, k, stride, clamped=defect == "border_clamped")
    kw = {} if defect is None or defect in GEOMETRY_DEFECTS else {"defect": defect}
    got = [(model(cols, w_matrix(L["w" + fm]), **kw) + L["b" + fm][None, None, :]).transpose(2, 0, 1) for fm in "fm"]
    got = np.concatenate(got)
    if defect == "ragged_unwritten":
        got[:, got.shape[1] // 4 * 4:], got[:, :, got.shape[2] // 4 * 4:] = R64.SENTINEL, R64.SENTINEL
    finite = bool(np.isfinite(got).all())
    bound = np.concatenate([R64.preact_bound_direct(L, ref, family, fm) for fm in "fm"])
    err = np.abs(np.nan_to_num(got.astype(np.float64), nan=1e300, posinf=1e300, neginf=-1e300) - np.concatenate([ref.f, ref.m]))
    clean = np.nan_to_num(got, nan=3e38, posinf=3e38, neginf=-3e38)
    e_max, e_rms = R64.measure_linear(clean, ref)
    r_max, r_rms = R64.measure_linear(R64.oracle_fp32(L, x, stride=stride, linear=True), ref)
    zero = np.concatenate([ref.Af, ref.Am]) == 0
    return dict(E_max=e_max, E_rms=e_rms, R_max=r_max, R_rms=r_rms, q=float((err / bound).max()), finite=finite,
                zero_exact=bool((got[zero] == 0).all()), cls=cls)


def inside_caps(s, family):
    """The two kinds of cap of tests/conv_ref64.py: the derived bound (q <= 1, hard) and the measured one against the oracle's own error
    (only where the oracle has an error to compare with: R_max >= 1)."""
    c = R64.measured_cap(family, "linear", s["cls"])
    ok = s["finite"] and s["q"] <= 1.0 and s["zero_exact"]
    if s["R_max"] >= 1.0:
        ok = ok and s["E_rms"] <= c * s["R_rms"] and s["E_max"] <= c * s["R_max"]
    return ok


# the direct families at CPU-sized shapes: (family, cin, cout, k, stride, H, W)
DIRECT = [("d3h", 64, 32, 3, 1, 9, 21), ("d3h_s2", 32, 32, 3, 2, 10, 14), ("d3h_s2", 32, 32, 4, 2, 10, 14), ("pxh", 96, 40, 1, 1, 7, 13),
          ("t3h", 8, 32, 3, 1, 9, 21)]


def direct_inputs(family, cin, cout, k, stride, H, W):
    """(class, name, L, x) over classes (a) - (d) of tests/conv_ref64.py."""
    rng = np.random.default_rng([cin, cout, k, 3])
    tame = R64.tame_layer(cin, cout, k, 11)
    yield "a", "unit scale", tame, rng.standard_normal((cin, H, W)).astype(np.float32)
    Lb, xb = R64.checkpoint_like(cin, cout, k, H, W, 12)
    yield "b", "checkpoint-like", Lb, xb
    for amp in (1.0, 2.0 ** -10):
        for (c, y, x_) in R64.impulse_positions(cin, H, W)[::5]:
            yield "c", f"impulse {amp:g} at c{c} ({y},{x_})", tame, R64.impulse(cin, H, W, c, y, x_, amp)
    yield "c", "constant", tame, R64.constant_image(cin, H, W)
    yield "c", "checkerboard", tame, R64.checkerboard(cin, H, W)
    for amp in (2.0 ** -14, 1e-6):
        yield "d", f"small scale {amp:g}", tame, (rng.standard_normal((cin, H, W)) * amp).astype(np.float32)


@pytest.mark.parametrize("shape", DIRECT, ids=lambda s: f"{s[0]}-k{s[3]}s{s[4]}")
def test_direct_split_models_stay_inside_the_caps(shape):
    """The intact three-piece-pair arithmetic on every class: finite, inside the derived bound |err| <= u (12 + 3 nb + 1) A + floors
    (tests/conv_ref64.py; on the small-scale cases of class (d) the floors ARE the promise: ~1e-11 absolute per product, not fp32-relative
    accuracy), inside the measured caps, exact zeros where A = 0."""
    family = shape[0]
    for cls, name, L, x in direct_inputs(*shape):
        s = run_direct(L, x, shape[3], shape[4], family, model=split_conv_model_taps, cls=cls)
        print("%-7s %s %-34s E_max %8.2f E_rms %7.3f  R_max %8.2f R_rms %7.3f  err/bound %.3f" % (family, cls, name, s["E_max"], s["E_rms"], s["R_max"], s["R_rms"], s["q"]))
        assert inside_caps(s, family), (family, cls, name, s)
    # the 3x3 restatement with its own padding and tap loop is the same arithmetic as the im2col form used here
    if family == "d3h":
        L, x = R64.checkpoint_like(shape[1], shape[2], 3, shape[5], shape[6], 12)
        a = split_conv_model(np.ascontiguousarray(x.transpose(1, 2, 0)), L["wf"])
        b = split_conv_model_taps(im2col(x, 3, 1), w_matrix(L["wf"]))
        assert float(np.abs(a.astype(np.float64) - b).max()) <= 2 * R64.U * float(R64.reference(L, x).Af.max())


# Which classes must catch which defect (direct arithmetic; "a" unit scale, "b" checkpoint-like, "c" impulses / constant /
# checkerboard, "d" small scales):
#   drop_wh_xl    the pair (2^-11 wh) xl is lost: up to 2^-11 |w x| per product wherever x is not an f16 number — (a) and (b).  The
#                 impulses, the constant and the checkerboard of (c) ARE f16 numbers (xl = 0): (c) is blind to this one by construction.
#   drop_wl_xh    the pair wl xh is lost: up to 2^-11 |w x| per product for every x: (a), (b), and every impulse of (c) (hundreds to
#                 thousands of units at one pixel).
#   xl_unscaled   x - xh underflows f16 (quantum 2^-24) instead of being carried at 2^11: an absolute 2^-25 per activation — (b) (the
#                 channels whose scale is small: E_rms seven times the intact model's, over the measured cap) and (d) (over both).
#   scale_binade  nothing is lost until an entry reaches 65520: the row of (b) whose largest weight is the fp32 number just below a power
#                 of two rounds to 2^16 = Inf in f16: (b), non-finite.
#   wl_truncated  |wh + wl - w s| grows from half an ulp of wl to a whole one: still within the 4 u per operand that the bound must allow
#                 for round-to-nearest's worst case, so no sum can show it; it is caught where it lives, in the packer:
#                 test_packers_on_edge_rows holds every stored wl to HALF an ulp of the exact residual, and
#                 test_truncated_low_piece_breaks_the_packer_property shows truncated pieces breaking exactly that.
EXPECT = {"drop_wh_xl": {"a", "b"}, "drop_wl_xh": {"a", "b", "c"}, "xl_unscaled": {"b", "d"}, "scale_binade": {"b"}}


@pytest.mark.parametrize("defect", sorted(EXPECT))
def test_seeded_defects_exceed_the_caps(defect):
    shape = DIRECT[0]
    caught = {}
    for cls, name, L, x in direct_inputs(*shape):
        s = run_direct(L, x, shape[3], shape[4], shape[0], defect=defect, cls=cls)
        intact = run_direct(L, x, shape[3], shape[4], shape[0], cls=cls)
        assert inside_caps(intact, shape[0]), (cls, name, intact)                # the copy without a defect is the real arithmetic
        hit = not inside_caps(s, shape[0])
        caught.setdefault(cls, []).append((name, hit))
        print("%-13s %s %-34s E_max %10.2f E_rms %9.3f  R_max %8.2f R_rms %7.3f  err/bound %9.3f  %s" % (
            defect, cls, name, s["E_max"], s["E_rms"], s["R_max"], s["R_rms"], s["q"], "CAUGHT" if hit else "-"))
    for cls in EXPECT[defect]:
        assert any(h for _, h in caught[cls]), f"{defect}: class ({cls}) did not catch it: {caught}"
    if defect == "drop_wl_xh":
        assert all(h for n, h in caught["c"] if n.startswith("impulse")), "every impulse must show a lost weight piece"


def half_ulp_f16(v):
    """Half the f16 spacing at |v| (2^-25 in the subnormal range)."""
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -14)))
    return 2.0 ** (e - 11)


def test_truncated_low_piece_breaks_the_packer_property():
    """wl_truncated of EXPECT: round-to-nearest pieces satisfy |wh + wl - w s| <= half an ulp of wl; truncated ones do not."""
    L, _ = R64.checkpoint_like(64, 32, 3, 4, 4, 21)
    w2 = w_matrix(L["wf"]).astype(np.float64)
    ex = np.round(np.log2(1.0 / R64.row_inv_scale(w2))).astype(np.int64)
    ws = np.ldexp(w2, ex[:, None])
    wh = ws.astype(np.float16).astype(np.float64)
    r = ws - wh
    rtn = r.astype(np.float16)
    assert np.all(np.abs(rtn.astype(np.float64) - r) <= half_ulp_f16(r))
    trunc = np.where(np.abs(rtn.astype(np.float64)) > np.abs(r), np.nextafter(rtn, np.float16(0)), rtn).astype(np.float64)
    assert np.any(np.abs(trunc - r) > half_ulp_f16(r))


# ------------------------------------------------------------------------------------------ the library's packers on the edge rows
def _halfs(blob, n_inv):
    return blob[:-n_inv].view(np.float16), blob[-n_inv:]


def test_packers_on_edge_rows():
    """read_conv_pack_dkh_host (3x3, 4x4, 1x1), read_conv_pack_t3h_host and read_conv_pack_w4h_host against the NumPy packers BIT FOR BIT
    on checkpoint-like layers with the edge rows (all zeros, a single weight, largest |w| a power of two and the fp32 number just below
    one, fp32 denormals, -0.0), and the properties the arithmetic rests on, from the library's own output: 1 / s as the rule says, every
    piece finite, hi + lo within half an f16 ulp of the exact residual.  read_conv_pack_f4x1_host has no NumPy packer beside it: its
    output is decoded (tests/test_f4x1_model.decode_rows) and held to the same properties against G w in float64."""
    from read_amd import _lib
    from tests import test_f4x1_model as F4
    from tests.wino4_ref import G
    from tests.wino4h_ref import pack_w4h_blob
    L_ = _lib.lib()
    for cin, cout in ((64, 40), (32, 32)):
        L, _ = R64.checkpoint_like(cin, cout, 3, 4, 4, 31)
        wf, wm = np.ascontiguousarray(L["wf"]), np.ascontiguousarray(L["wm"])
        cp = (cout + 31) // 32 * 32
        # direct 3x3
        got = np.zeros(L_.read_conv_dkh_floats(cin, cout, 3), np.float32)
        assert L_.read_conv_pack_dkh_host(cin, cout, 3, wf.ctypes.data, wm.ctypes.data, got.ctypes.data) == 0
        want = pack_d3h_blob(wf, wm)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "direct 3x3 packer != model packer on the edge rows"
        h, inv = _halfs(got, 2 * cp)
        assert np.isfinite(h.astype(np.float32)).all()
        assert np.array_equal(inv[:cout], R64.row_inv_scale(wf).astype(np.float32)) and np.array_equal(inv[cp:cp + cout], R64.row_inv_scale(wm).astype(np.float32))
        assert inv[0] == 1.0 and inv[4] == np.float32(2.0 ** -60)           # the all-zero row; the denormal row at the clamp (s = 2^60)
        assert inv[2] == np.float32(2.0 ** -17) and inv[3] == np.float32(2.0 ** -18)   # 0.125 = 0.5 x 2^-2: ex = 17; the number just below it: ex = 18
        # Winograd F(4x4)
        got = np.zeros(L_.read_conv_w4h_floats(cin, cout), np.float32)
        assert L_.read_conv_pack_w4h_host(cin, cout, wf.ctypes.data, wm.ctypes.data, got.ctypes.data) == 0
        want = pack_w4h_blob(wf, wm)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "Winograd packer != model packer on the edge rows"
        h, inv = _halfs(got, 2 * cp)
        assert np.isfinite(h.astype(np.float32)).all()
        assert np.array_equal(inv[:cout], R64.wino_filter_inv_scale(wf).astype(np.float32))
        # F(4,3) by rows
        halfs, inv = F4.pack_f4x1(wf, wm)
        assert inv.shape == (2, cp) and np.isfinite(halfs.astype(np.float32)).all()
        Uh, Ul = F4.decode_rows(halfs, cin, cp)
        for fm, w in enumerate((wf, wm)):
            assert np.array_equal(inv[fm, :cout], R64.f4x1_filter_inv_scale(w).astype(np.float32)), "1 / s of the F(4,3)-by-rows packer"
            z, dn = (0, 4) if fm == 0 else (8, 12)                            # the all-zero row; the denormal row at the clamp (s = 2^60)
            assert inv[fm, z] == 1.0 and inv[fm, dn] == np.float32(2.0 ** -60)
            w64 = w.astype(np.float64).transpose(0, 2, 1, 3)                  # (co, ky, cin, kx)
            Us = sum(G[None, None, :, None, b] * w64[:, :, None, :, b] for b in range(3)) / inv[fm, :cout].astype(np.float64)[:, None, None, None]
            hi, lo = Uh[fm, :cout], Ul[fm, :cout]                             # (co, ky, frequency, cin)
            assert np.abs(Us).max() < 2.0 ** 15 and np.isfinite(hi).all() and np.isfinite(lo).all()
            assert np.all(np.abs(hi - Us) <= half_ulp_f16(Us)) and np.all(np.abs(hi + lo - Us) <= half_ulp_f16(Us - hi)), "pieces of the F(4,3)-by-rows packer"
            assert not Uh[fm, cout:].any() and not Ul[fm, cout:].any() and np.all(inv[fm, cout:] == 1.0)     # padded rows: zero, scale 1
        # 1x1
        w1f, w1m = np.ascontiguousarray(wf[:, :, 0, 0]), np.ascontiguousarray(wm[:, :, 0, 0])
        got = np.zeros(L_.read_conv_dkh_floats(cin, cout, 1), np.float32)
        assert L_.read_conv_pack_dkh_host(cin, cout, 1, w1f.ctypes.data, w1m.ctypes.data, got.ctypes.data) == 0
        assert np.array_equal(got.view(np.uint32), pack_d1h_blob(w1f, w1m).view(np.uint32)), "1x1 packer != model packer on the edge rows"
    L, _ = R64.checkpoint_like(32, 32, 4, 4, 4, 33)                          # the 4 x 4 / stride-2 operand: the piece property from the library's halfs
    wf, wm = np.ascontiguousarray(L["wf"]), np.ascontiguousarray(L["wm"])
    got = np.zeros(L_.read_conv_dkh_floats(32, 32, 4), np.float32)
    assert L_.read_conv_pack_dkh_host(32, 32, 4, wf.ctypes.data, wm.ctypes.data, got.ctypes.data) == 0
    h, inv = _halfs(got, 64)
    h = h.reshape(1, 2, 1, 16, 2, 2, 64, 8).astype(np.float64)               # [group][rh][chunk][tap][rb][piece][lane][e]
    for rh in range(2):
        for rb in range(2):
            for i in range(16):
                co, fm = 16 * rh + 8 * rb + (i & 7), i >> 3
                w = (wm if fm else wf)[co].astype(np.float64)                # (cin, 4, 4)
                s = 1.0 / float(inv[32 * fm + co])
                for kq in range(4):
                    ws = w[8 * kq:8 * kq + 8].reshape(8, 16).T * s            # (tap, e)
                    hi, lo = h[0, rh, 0, :, rb, 0, i + 16 * kq], h[0, rh, 0, :, rb, 1, i + 16 * kq]
                    assert np.all(np.abs(hi - ws) <= half_ulp_f16(ws)) and np.all(np.abs(hi + lo - ws) <= half_ulp_f16(ws - hi))
    for cin, cout in ((8, 32), (32, 8)):                                      # the implicit-GEMM form of 3x3 weights
        L, _ = R64.checkpoint_like(cin, cout, 3, 4, 4, 35)
        wf, wm = np.ascontiguousarray(L["wf"]), np.ascontiguousarray(L["wm"])
        K = (9 * cin + 15) // 16 * 16
        mat = lambda w: np.concatenate([w_matrix(w), np.zeros((cout, K - 9 * cin), np.float32)], 1)   # noqa: E731
        got = np.zeros(L_.read_conv_t3h_floats(cin, cout), np.float32)
        assert L_.read_conv_pack_t3h_host(cin, cout, wf.ctypes.data, wm.ctypes.data, got.ctypes.data) == 0
        assert np.array_equal(got.view(np.uint32), pack_d1h_blob(mat(wf), mat(wm)).view(np.uint32)), "implicit-GEMM packer != model packer on the edge rows"


# ------------------------------------------------------------------------------------------ Winograd
def run_wino(L, x, halfs_edit=None, cls="a"):
    """The lane-exact model of gated_conv_wino4h_kernel (tests/wino4h_ref.py) on the LIBRARY's packed operand -> statistics as run_direct;
    E against the transformed-domain condition term A_w and (EA) against A: that number shows what Winograd costs."""
    from read_amd import _lib
    from tests.wino4h_ref import wino4h_conv_model
    cout, cin = L["wf"].shape[:2]
    cp = (cout + 31) // 32 * 32
    wf, wm = np.ascontiguousarray(L["wf"]), np.ascontiguousarray(L["wm"])
    def pack(_):
        blob = np.zeros(_lib.lib().read_conv_w4h_floats(cin, cout), np.float32)
        assert _lib.lib().read_conv_pack_w4h_host(cin, cout, wf.ctypes.data, wm.ctypes.data, blob.ctypes.data) == 0
        return blob

    blob = R64.filter_memo(L["wf"], "w4h blob", pack, also=(L["wm"],))   # (the cases of one class (e) shape share their layer)
    halfs = blob[:-2 * cp].view(np.float16).reshape(cp // 32, 4, cin // 32, 36, 2, 64, 8).copy()
    inv = blob[-2 * cp:].reshape(2, cp).copy()
    if halfs_edit is not None:
        halfs_edit(halfs, inv)
    with np.errstate(over="ignore", invalid="ignore"):
        f, m = wino4h_conv_model(np.ascontiguousarray(x.transpose(1, 2, 0)), halfs, inv, cin, cout)
        got = np.concatenate([(f + L["bf"][None, None]).transpose(2, 0, 1), (m + L["bm"][None, None]).transpose(2, 0, 1)])
    ref = R64.reference(L, x)
    bf_, Awf = R64.preact_bound_wino(L, x, ref, "f")
    bm_, Awm = R64.preact_bound_wino(L, x, ref, "m")
    bound = np.concatenate([bf_, bm_])
    truth = np.concatenate([ref.f, ref.m])
    finite = bool(np.isfinite(got).all())
    err = np.abs(np.nan_to_num(got.astype(np.float64), nan=1e300, posinf=1e300, neginf=-1e300) - truth)
    Aw = np.concatenate([Awf + np.abs(L["bf"].astype(np.float64))[:, None, None], Awm + np.abs(L["bm"].astype(np.float64))[:, None, None]])
    clean = np.nan_to_num(got, nan=3e38, posinf=3e38, neginf=-3e38)
    e_max, e_rms = R64._stats(np.abs(clean.astype(np.float64) - truth), Aw)
    ea_max, ea_rms = R64.measure_linear(clean, ref)
    r_max, r_rms = R64.measure_linear(R64.oracle_fp32(L, x, linear=True), ref)
    return dict(E_max=e_max, E_rms=e_rms, EA_max=ea_max, EA_rms=ea_rms, R_max=r_max, R_rms=r_rms, q=float((err / bound).max()), finite=finite,
                zero_exact=bool((got[Aw == 0] == 0).all()), cls=cls)


def wino_inside_caps(s):
    c = R64.C_MEASURED["w4h"]["gated"][s["cls"]]            # (the device has no linear Winograd launch to measure)
    ok = s["finite"] and s["q"] <= 1.0 and s["zero_exact"]
    if s["R_max"] >= 1.0:                                        # the measured cap: E against A_w, as tests/test_gpu_conv_accuracy.py
        ok = ok and s["E_rms"] <= c * s["R_rms"] and s["E_max"] <= c * s["R_max"]
    return ok


def wino_inputs(cin, cout, H, W):
    rng = np.random.default_rng([cin, cout, 5])
    tame = R64.tame_layer(cin, cout, 3, 41)
    yield "a", "unit scale", tame, rng.standard_normal((cin, H, W)).astype(np.float32)
    Lb, xb = R64.checkpoint_like(cin, cout, 3, H, W, 42)
    yield "b", "checkpoint-like", Lb, xb
    for amp, (c, y, x_) in ((1.0, (1, 3, 3)), (2.0 ** -10, (31, 5, 6)), (1.0, (2, H - 1, W - 1)), (2.0 ** -10, (0, 8, 8))):
        yield "c", f"impulse {amp:g} at c{c} ({y},{x_})", tame, R64.impulse(cin, H, W, c, y, x_, amp)
    yield "c", "constant", tame, R64.constant_image(cin, H, W)
    yield "d", "range edge 650, rows (0, 0)", tame, R64.wino_range_edge(cin, H, W, rows=(0, 0))
    yield "d", "range edge 650, rows (1, 5)", tame, R64.wino_range_edge(cin, H, W, rows=(1, 5))
    yield "d", "small scale 2^-14", tame, (rng.standard_normal((cin, H, W)) * 2.0 ** -14).astype(np.float32)


def test_winograd_split_model_stays_inside_the_caps_and_defects_do_not():
    """The lane-exact Winograd model on classes (a) - (d) (one 8 x 32 unit and a partial one below it, 32 channels): inside the
    transformed-domain bound of tests/conv_ref64.py (the model's input transform rounds once, the bound allows the kernel's four), finite
    at the documented range edge (amplitude 650 on the pattern that attains |B^T d B| = 100 x), exact zeros.
    Defects, on the operand the model consumes: the Ul pieces zeroed (= the pair Ul Vh dropped) — caught on (a), (b) and on every impulse;
    the row scale one binade up — caught on (b) (the just-below-a-power-of-two row overflows f16)."""
    cin, cout, H, W = 32, 32, 11, 13

    def drop_ul(halfs, inv):
        halfs[:, :, :, :, 1] = 0

    def binade(halfs, inv):
        with np.errstate(over="ignore"):
            halfs *= np.float16(2.0)
        inv *= 0.5

    caught = {"drop_ul": {}, "binade": {}}
    for cls, name, L, x in wino_inputs(cin, cout, H, W):
        s = run_wino(L, x, cls=cls)
        print("w4h     %s %-30s E(A_w) max %8.2f rms %7.3f  E(A) max %9.2f rms %8.3f  R_max %7.2f R_rms %6.3f  err/bound %.3f" % (
            cls, name, s["E_max"], s["E_rms"], s["EA_max"], s["EA_rms"], s["R_max"], s["R_rms"], s["q"]))
        assert wino_inside_caps(s), (cls, name, s)
        if name in ("unit scale", "checkpoint-like") or name.startswith("impulse"):
            for dname, edit in (("drop_ul", drop_ul), ("binade", binade)):
                d = run_wino(L, x, halfs_edit=edit, cls=cls)
                caught[dname].setdefault(cls, []).append(not wino_inside_caps(d))
                print("   %-8s E(A) max %10.2f rms %9.3f  err/bound %9.3f finite %s" % (dname, d["EA_max"], d["EA_rms"], d["q"], d["finite"]))
    assert any(caught["drop_ul"]["a"]) and any(caught["drop_ul"]["b"]) and all(caught["drop_ul"]["c"]), caught
    assert any(caught["binade"]["b"]), caught


# ------------------------------------------------------------------------------------------ F(4,3) by rows
def run_f4x1(L, x, halfs_edit=None, cls="a"):
    """The NumPy model of gated_conv_f4x1h_kernel (tests/test_f4x1_model.f4x1_conv_model) on the LIBRARY's packed operand -> statistics as
    run_wino: E against the transformed-domain condition term A_w, (EA) against A; `got` = [f | m] for the checks that look at elements."""
    from tests import test_f4x1_model as F4
    cout, cin = L["wf"].shape[:2]
    halfs, inv = R64.filter_memo(L["wf"], "f4x1 blob", lambda _: F4.pack_f4x1(np.ascontiguousarray(L["wf"]), np.ascontiguousarray(L["wm"])), also=(L["wm"],))
    halfs, inv = halfs.copy(), inv.copy()
    if halfs_edit is not None:
        halfs_edit(halfs, inv)
    with np.errstate(over="ignore", invalid="ignore"):
        Uh, Ul = F4.decode_rows(halfs, cin, inv.shape[1])
        f, m = F4.f4x1_conv_model(np.ascontiguousarray(x.transpose(1, 2, 0)), Uh, Ul, inv, cout)
        got = np.concatenate([(f + L["bf"][None, None]).transpose(2, 0, 1), (m + L["bm"][None, None]).transpose(2, 0, 1)])
    ref = R64.reference(L, x)
    bf_, Awf = R64.preact_bound_f4x1(L, x, ref, "f")
    bm_, Awm = R64.preact_bound_f4x1(L, x, ref, "m")
    bound = np.concatenate([bf_, bm_])
    truth = np.concatenate([ref.f, ref.m])
    finite = bool(np.isfinite(got).all())
    err = np.abs(np.nan_to_num(got.astype(np.float64), nan=1e300, posinf=1e300, neginf=-1e300) - truth)
    Aw = np.concatenate([Awf + np.abs(L["bf"].astype(np.float64))[:, None, None], Awm + np.abs(L["bm"].astype(np.float64))[:, None, None]])
    clean = np.nan_to_num(got, nan=3e38, posinf=3e38, neginf=-3e38)
    e_max, e_rms = R64._stats(np.abs(clean.astype(np.float64) - truth), Aw)
    ea_max, ea_rms = R64.measure_linear(clean, ref)
    r_max, r_rms = R64.measure_linear(R64.oracle_fp32(L, x, linear=True), ref)
    return dict(E_max=e_max, E_rms=e_rms, EA_max=ea_max, EA_rms=ea_rms, R_max=r_max, R_rms=r_rms, q=float((err / bound).max()), finite=finite,
                zero_exact=bool((got[Aw == 0] == 0).all()), cls=cls, got=got)


def f4x1_inside_caps(s):
    """Finite, inside preact_bound_f4x1, exact zeros where A_w + |b| = 0, and inside the linear caps this file uses for models
    (measured_cap falls back to the pxh kernel's linear row for a family without linear launches)."""
    return inside_caps(s, "f4x1")


F4X1_SHAPE = (32, 32, 11, 37)        # one full 8 x 32 unit, partial units to the right (5 columns, a last segment of 1) and below (3 rows)


def f4x1_inputs(cin, cout, H, W):
    rng = np.random.default_rng([cin, cout, 7])
    tame = R64.tame_layer(cin, cout, 3, 51)
    yield "a", "unit scale", tame, rng.standard_normal((cin, H, W)).astype(np.float32)
    Lb, xb = R64.checkpoint_like(cin, cout, 3, H, W, 52)
    yield "b", "checkpoint-like", Lb, xb
    base = R64.impulse_positions(cin, H, W)
    own = [p for p in R64.impulse_positions_f4x1(cin, H, W) if p not in base]           # the seam, the halo rows, the last partial segment
    for amp in (1.0, 2.0 ** -10):
        for (c, y, x_) in base[::5] + own:
            yield "c", f"impulse {amp:g} at c{c} ({y},{x_})", tame, R64.impulse(cin, H, W, c, y, x_, amp)
    yield "c", "constant", tame, R64.constant_image(cin, H, W)
    yield "c", "checkerboard", tame, R64.checkerboard(cin, H, W)
    yield "d", "range edge 6550, row 1, segment 3", tame, R64.f4x1_range_edge(cin, H, W, row=1, segment=3)
    yield "d", "range edge 6550, row 5, segment 8", tame, R64.f4x1_range_edge(cin, H, W, row=5, segment=8)      # the last full segment, right of the seam
    for amp, label in ((2.0 ** -14, "2^-14"), (1e-6, "1e-6")):
        yield "d", f"small scale {label}", tame, (rng.standard_normal((cin, H, W)) * amp).astype(np.float32)


def test_f4x1_model_stays_inside_the_caps():
    """The intact arithmetic of gated_conv_f4x1h_kernel on classes (a) - (d): finite (at amplitude 6550 on the pattern that attains
    |B^T d| = 10 x), inside preact_bound_f4x1, inside the linear caps, exact zeros where A_w + |b| = 0."""
    for cls, name, L, x in f4x1_inputs(*F4X1_SHAPE):
        s = run_f4x1(L, x, cls=cls)
        print("f4x1    %s %-36s E(A_w) max %8.2f rms %7.3f  E(A) max %9.2f rms %8.3f  R_max %7.2f R_rms %6.3f  err/bound %.3f" % (
            cls, name, s["E_max"], s["E_rms"], s["EA_max"], s["EA_rms"], s["R_max"], s["R_rms"], s["q"]))
        assert s["finite"], (cls, name)
        assert s["q"] <= 1.0, (cls, name, s["q"])
        assert s["zero_exact"], (cls, name)
        assert f4x1_inside_caps(s), (cls, name, {k: v for k, v in s.items() if k != "got"})


def _f4x1_drop_ul(halfs, inv):
    halfs[:, :, :, :, :, 1] = 0                                  # = the pair Ul Vh dropped


def _f4x1_binade(halfs, inv):
    with np.errstate(over="ignore"):
        halfs *= np.float16(2.0)                                 # the row's largest entry lands in [2^15, 2^16)
    inv *= 0.5


def _f4x1_no_ky0(halfs, inv):
    halfs[:, :, :, 0] = 0                                        # the fragments of tap ky = 0: the row above never reaches the output


# Which classes must catch which defect of the operand the model consumes:
#   drop_ul  up to 2^-11 |U V| per product for every V: (a), (b), and EVERY impulse of (c);
#   binade   nothing is lost until an entry reaches 65520: the row of (b) whose largest weight is the fp32 number just below a power of two
#            (its G[5] w = w at frequency 5) rounds to 2^16 = Inf in f16: (b), non-finite;
#   no_ky0   a third of the taps: every class.  On an impulse at (y, x) it is visible EXACTLY: the output row y + 1 sees the impulse
#            through tap ky = 0 alone, so the broken model returns the bias there, bit for bit, where the reference does not — for the
#            impulses on row 7 that is row 8, the top row of the unit below.
F4X1_DEFECTS = {"drop_ul": (_f4x1_drop_ul, {"a", "b", "c"}), "binade": (_f4x1_binade, {"b"}), "no_ky0": (_f4x1_no_ky0, {"a", "b", "c", "d"})}


@pytest.mark.parametrize("defect", sorted(F4X1_DEFECTS))
def test_f4x1_seeded_defects_exceed_the_caps(defect):
    edit, classes = F4X1_DEFECTS[defect]
    cin, cout, H, W = F4X1_SHAPE
    caught = {}
    for cls, name, L, x in f4x1_inputs(*F4X1_SHAPE):
        s = run_f4x1(L, x, halfs_edit=edit, cls=cls)
        hit = not f4x1_inside_caps(s)
        caught.setdefault(cls, []).append((name, hit))
        print("%-8s %s %-36s E(A) max %10.2f rms %9.3f  err/bound %9.3f finite %s  %s" % (defect, cls, name, s["EA_max"], s["EA_rms"], s["q"], s["finite"], "CAUGHT" if hit else "-"))
        if defect == "binade" and cls == "b":
            assert not s["finite"], "the row just below a power of two must overflow f16 one binade up"
        if defect == "no_ky0" and name.startswith("impulse"):
            y = int(name.split("(")[1].split(",")[0])
            if y + 1 < H:
                ref = R64.reference(L, x)
                row = s["got"][:cout, y + 1]
                assert np.array_equal(row, np.broadcast_to(L["bf"][:, None], row.shape)) and np.any(ref.f[:, y + 1] != L["bf"].astype(np.float64)[:, None]), name
    for cls in classes:
        assert any(h for _, h in caught[cls]), f"{defect}: class ({cls}) did not catch it: {caught}"
    if defect in ("drop_ul", "no_ky0"):
        # (an impulse on the last image row reaches no output through tap ky = 0: nothing to lose there)
        assert all(h for n, h in caught["c"] if n.startswith("impulse") and (defect == "drop_ul" or int(n.split("(")[1].split(",")[0]) + 1 < H)), caught["c"]


def test_f4x1_model_overflows_just_past_the_documented_range():
    """Written to fail the finiteness check: amplitude 6560 on the range-edge pattern gives |B^T d| = 65600, which rounds to Inf in f16 —
    so the 6550 cases of the tests above and of tests/test_gpu_conv_accuracy.py really sit on the edge."""
    cin, cout, H, W = F4X1_SHAPE
    tame = R64.tame_layer(cin, cout, 3, 51)
    for row, segment in ((1, 3), (5, 8)):
        assert run_f4x1(tame, R64.f4x1_range_edge(cin, H, W, row=row, segment=segment, amp=6550.0), cls="d")["finite"]
        s = run_f4x1(tame, R64.f4x1_range_edge(cin, H, W, row=row, segment=segment, amp=6560.0), cls="d")
        assert not s["finite"] and not f4x1_inside_caps(s), (row, segment)


# ------------------------------------------------------------------------------------------ addends, resampled sources, the AFF chain, the head
def _sample(t, f_off, m_off, cout, shift, H, W, defect=None):
    """R64.sample_addend, copied so that ONE line at a time can be broken."""
    if defect == "m_from_f_offset":
        m_off = f_off
    if defect == "pre_shift_off_by_one":
        shift += 1
    iy, ix = np.arange(H) >> shift, np.arange(W) >> shift
    if defect == "row_clamped":
        iy = np.minimum(iy, t.shape[0] - 2)
    px = t[iy[:, None], ix[None, :]]
    return px[..., f_off:f_off + cout].transpose(2, 0, 1), px[..., m_off:m_off + cout].transpose(2, 0, 1)


def _assemble(srcs, H, W, defect=None):
    """R64.assemble, copied likewise: the first finer source read with >> where << is meant."""
    out = []
    for x, s in srcs:
        wrong = defect == "shift_direction" and s > 0
        iy, ix = ((np.arange(n) << s) if (s >= 0 and not wrong) else (np.arange(n) >> abs(s)) for n in (H, W))
        out.append(x[:, iy[:, None], ix[None, :]])
    return np.concatenate(out, 0)


def pxh_launch_model(L, srcs, H, W, pre=None, defect=None):
    """One launch of gated_conv_pxh_kernel up to its pre-activations, on tests/d3h_ref.split_conv_model_taps (acc / s as fp32):
    fl32(fl32(acc / s + b) + pre), pre = (tensor (preH, preW, C), f_off, m_off, shift) -> [f | m] (H, W, 2 Cout) float32."""
    x = np.ascontiguousarray(_assemble(srcs, H, W, defect).transpose(1, 2, 0))
    cout = L["wf"].shape[0]
    add = _sample(pre[0], pre[1], pre[2], cout, pre[3], H, W, defect) if pre is not None else (None, None)
    out = []
    for fm, p in zip("fm", add):
        w2 = w_matrix(L["w" + fm])
        acc = split_conv_model_taps(x, w2).astype(np.float64)
        b = L["b" + fm].astype(np.float64)[None, None]
        if p is None:
            f = (acc + b).astype(np.float32)
        elif defect == "addend_before_scaling":                  # fma(acc_s + pre, 1 / s, b)
            f = (acc + p.transpose(1, 2, 0).astype(np.float64) * R64.row_inv_scale(w2)[None, None] + b).astype(np.float32)
        else:
            f = ((acc + b).astype(np.float32).astype(np.float64) + p.transpose(1, 2, 0)).astype(np.float32)
        out.append(f)
    return np.concatenate(out, 2)


def _q(got_hwc, truth, bound):
    return float((np.abs(got_hwc.transpose(2, 0, 1).astype(np.float64) - truth) / bound).max())


ADDEND_SHAPE = ([32], (0,), 32, 13, 37, 64, 0, 32, 1)          # the AFF0 launch of the plan at an odd size: the last addend row and column are shared
RESAMPLED_SHAPE = ([32, 64, 128], (1, 0, -1), 64, 13, 37)


def addend_inputs(shape, cls):
    """-> (L, srcs, pre) of class (a), (b) or (b) in its cancelling form ("bc")."""
    split, shifts, cout, H, W, C, f_off, m_off, sh = shape
    cin, big = sum(split), max(max(shifts), 0)
    rng = np.random.default_rng([71, cin, cout, H])
    if cls == "a":
        L, xb = R64.tame_layer(cin, cout, 1, 71), rng.standard_normal((cin, H << big, W << big)).astype(np.float32)
    else:
        L, xb = R64.checkpoint_like(cin, cout, 1, H << big, W << big, 72)
    xs = R64.split_sources(xb, split, shifts, H, W)
    t = R64.addend_tensor(rng, R64.addend_size(sh, H, W) + (C,), f_off, m_off, cout, 1.0 if cls == "a" else 2.0 ** rng.uniform(-8, 8, cout))
    if cls == "bc":
        t = R64.cancelling_addend(t, R64.reference(L, R64.assemble(xs, shifts, H, W)).f, f_off, sh)
    return L, list(zip(xs, shifts)), (t, f_off, m_off, sh)


def addend_q(L, srcs, pre, H, W, defect=None):
    """err / derived bound of the launch model's pre-activations, and of the torch-fp32 oracle's on the same inputs."""
    cout = L["wf"].shape[0]
    x = R64.assemble([s[0] for s in srcs], [s[1] for s in srcs], H, W)
    add = tuple(R64.sample_addend(pre[0], pre[1], pre[2], cout, pre[3], H, W)) if pre is not None else None
    ref = R64.reference(L, x, pre=add)
    truth = np.concatenate([ref.f, ref.m])
    if add is None:
        bound = np.concatenate([R64.preact_bound_direct(L, ref, "pxh", fm) for fm in "fm"])
    else:
        bound = np.concatenate([R64.preact_bound_addend(L, ref, "pxh", fm, tot) for fm, tot in (("f", ref.f), ("m", ref.m))])
    got = pxh_launch_model(L, srcs, H, W, pre, defect)
    ora = R64.oracle_fp32(L, x, linear=True, pre=add)
    return _q(got, truth, bound), float((np.abs(ora.astype(np.float64) - truth) / bound).max())


@pytest.mark.parametrize("cls", ["a", "b", "bc"])
def test_addend_epilogue_model_stays_inside_the_bound(cls):
    """fl32(fl32(acc / s + b) + pre) on unit-scale and checkpoint-like inputs (the addend scaled per channel by 2^U(-8, 8), and the
    cancelling form): inside preact_bound_direct(own) + u |f|; so is the torch-fp32 oracle: the inputs are fair."""
    H, W = ADDEND_SHAPE[3:5]
    q, q_oracle = addend_q(*addend_inputs(ADDEND_SHAPE, cls), H, W)
    print("addend (%s): model err/bound %.3f, oracle %.3f" % (cls, q, q_oracle))
    assert q <= 1.0 and q_oracle <= 1.0, (q, q_oracle)


def test_resampled_concatenation_model_stays_inside_the_bound():
    split, shifts, cout, H, W = RESAMPLED_SHAPE
    for cls in "ab":
        L, srcs, _ = addend_inputs((split, shifts, cout, H, W, 2 * cout, 0, cout, 1), cls)
        q, q_oracle = addend_q(L, srcs, None, H, W)
        print("resampled (%s): model err/bound %.3f, oracle %.3f" % (cls, q, q_oracle))
        assert q <= 1.0 and q_oracle <= 1.0, (cls, q, q_oracle)


def _round_to_11_bits(a):
    m, e = np.frexp(a.astype(np.float64))
    return np.ldexp(np.round(np.ldexp(m, 11)), e - 11).astype(np.float32)


def chain_inputs(cls, sizes=((20, 36), (10, 18), (5, 9), (3, 5))):
    """Three AFF layers 480 -> 32 / 64 / 128 and the four sources res1 32, res2 64, res3 128, z 256 at their levels; class (b): the layers
    checkpoint-like with the sources scaled per channel as their weights are (inversely)."""
    return R64.aff_chain_inputs(cls, sizes)


def chain_q(layers, xs, defect=None):
    """-> {launch: err / composed bound of its pre-activations [f | m]} for the six launches on the launch model."""
    def launch(name, Lp, srcs, pre, linear, hw):
        out = pxh_launch_model(Lp, srcs, hw[0], hw[1], pre)
        return _round_to_11_bits(out) if (defect == "q_rounded_to_11_bits" and name == "q3") else out

    outs = R64.run_aff_chain(layers, xs, launch)
    refs = R64.aff_chain_reference(layers, xs)
    return {name: _q(outs[name], np.concatenate([ref.f, ref.m]), np.concatenate([df, dm])) for name, (ref, df, dm, _, _) in refs.items()}


@pytest.mark.parametrize("cls", ["a", "b"])
def test_aff_chain_model_stays_inside_the_composed_bound(cls):
    """The six launches of the plan on the launch model, every intermediate tensor fp32: each of q3, q2, q1 and the pre-activations of
    the three gated launches inside d(q_k) = B_lin(part k) + up(d(q_k+1)) + u |q_k| against the UNSPLIT layer in float64."""
    q = chain_q(*chain_inputs(cls))
    print("chain (%s): " % cls + "  ".join("%s %.3f" % kv for kv in q.items()))
    assert max(q.values()) <= 1.0, q


def head_model(L, x, cph=8, defect=None):
    """gated_conv_smallc_kernel up to its pre-activations: per accumulator a sequential fp32 fma chain in the kernel's order (phase of cph
    channels, tap, quad of the phase, channel of the quad), then fl32(acc + b) -> [f | m] (2 Cout, H, W) float32.  (The fma is formed in
    float64 — the product of two fp32 numbers is exact there — and rounded to fp32.)"""
    cin, H, W = x.shape
    xp = np.zeros((cin, H + 2, W + 2))
    xp[:, 1:-1, 1:-1] = x
    out = []
    for fm in "fm":
        w = L["w" + fm].astype(np.float64)
        acc = np.zeros((w.shape[0], H, W), np.float32)
        for ph in range(cin // cph):
            for tap in range(9):
                ky, kx = divmod(tap, 3)
                for ch in range(ph * cph, (ph + 1) * cph):          # (quad, channel of the quad) = consecutive channels of the phase
                    v = xp[ch, ky:ky + H, kx:kx + W]
                    if defect == "tap_row_dropped" and tap == 7:
                        v = v.copy()
                        v[H - 2] = 0.0                               # tap (2, 1) of output row H - 2 reads the last image row: dropped
                    acc = (w[:, ch, ky, kx][:, None, None] * v[None] + acc.astype(np.float64)).astype(np.float32)
        out.append((acc.astype(np.float64) + L["b" + fm].astype(np.float64)[:, None, None]).astype(np.float32))
    return np.concatenate(out)


def head_q(cls, defect=None, shape=(3, 9, 33)):
    cout, H, W = shape
    if cls == "a":
        L, x = R64.tame_layer(32, cout, 3, 75), np.random.default_rng(75).standard_normal((32, H, W)).astype(np.float32)
    else:
        L, x = R64.checkpoint_like(32, cout, 3, H, W, 76)
    ref = R64.reference(L, x)
    truth, bound = np.concatenate([ref.f, ref.m]), np.concatenate([R64.preact_bound_sc(L, ref, fm) for fm in "fm"])
    got = head_model(L, x, defect=defect)
    ora = R64.oracle_fp32(L, x, linear=True)
    return float((np.abs(got.astype(np.float64) - truth) / bound).max()), float((np.abs(ora.astype(np.float64) - truth) / bound).max())


@pytest.mark.parametrize("cls", ["a", "b"])
def test_head_model_stays_inside_the_bound(cls):
    q, q_oracle = head_q(cls)
    print("head (%s): model err/bound %.3f, oracle %.3f" % (cls, q, q_oracle))
    assert q <= 1.0 and q_oracle <= 1.0, (q, q_oracle)


# One seeded defect per case; each must EXCEED the derived bound on classes (a) and (b) while the intact model (tests above) stays inside.
NEW_DEFECTS = ["m_from_f_offset", "addend_before_scaling", "row_clamped", "q_rounded_to_11_bits", "pre_shift_off_by_one", "shift_direction", "tap_row_dropped"]


@pytest.mark.parametrize("defect", NEW_DEFECTS)
def test_seeded_addend_chain_and_head_defects_exceed_the_bound(defect):
    for cls in "ab":
        if defect == "q_rounded_to_11_bits":
            q = chain_q(*chain_inputs(cls), defect=defect)
            print("%s (%s): " % (defect, cls) + "  ".join("%s %.3f" % kv for kv in q.items()))
            assert all(v > 1.0 for v in q.values()), q            # q3 itself and everything downstream of it
        elif defect == "tap_row_dropped":
            q, _ = head_q(cls, defect)
            assert q > 1.0, (defect, cls, q)
        elif defect == "shift_direction":
            split, shifts, cout, H, W = RESAMPLED_SHAPE
            L, srcs, _ = addend_inputs((split, shifts, cout, H, W, 2 * cout, 0, cout, 1), cls)
            q, _ = addend_q(L, srcs, None, H, W, defect)
            assert q > 1.0, (defect, cls, q)
        else:
            H, W = ADDEND_SHAPE[3:5]
            q, _ = addend_q(*addend_inputs(ADDEND_SHAPE, cls), H, W, defect)
            print("%s (%s): err/bound %.3f" % (defect, cls, q))
            assert q > 1.0, (defect, cls, q)


def test_oracle_stays_inside_the_derived_bound_on_every_new_gpu_case():
    """The inputs of the resampled-source, addend, chain and head cases of tests/test_gpu_conv_accuracy.py are fair: the torch-fp32 oracle
    alone — a correctly rounded fp32 evaluation in another order — is inside the derived bound on every element of every one of them."""
    from tests import test_gpu_conv_accuracy as G
    todo = [(c, False, "pxh") for c in G.cases_resampled()]
    todo += [(c, lin, "pxh_pre") for cls in "abcd" for c, lin in G.cases_pre(cls)]
    todo += [(c, False, "sc") for cls in "abcd" for c in G.cases_sc(cls)]
    worst = {}
    for case, linear, family in todo:
        ref = case.ref()
        ora = R64.oracle_fp32(case.L, case.x, elu=case.elu, residual=case.residual, linear=linear, pre=case.addend())
        df, dm, _ = G._bounds(case, family)
        truth, bound = (np.concatenate([ref.f, ref.m]), np.concatenate([df, dm])) if linear else (ref.y, R64.gated_bound(ref, df, dm))
        q = float((np.abs(ora.astype(np.float64) - truth) / bound).max())
        worst[(family, case.cls)] = max(worst.get((family, case.cls), 0.0), q)
        assert q <= 1.0, (family, case.cls, case.name, q)
    for cls in "ab":
        layers, xs = R64.aff_chain_inputs(cls)
        for name, (ref, df, dm, Lfull, xfull) in R64.aff_chain_reference(layers, xs).items():
            linear = name.startswith("q")
            ora = R64.oracle_fp32(Lfull, xfull, linear=linear)
            truth, bound = (np.concatenate([ref.f, ref.m]), np.concatenate([df, dm])) if linear else (ref.y, R64.gated_bound(ref, df, dm))
            q = float((np.abs(ora.astype(np.float64) - truth) / bound).max())
            worst[("chain", cls)] = max(worst.get(("chain", cls), 0.0), q)
            assert q <= 1.0, ("chain", cls, name, q)
    print("oracle err / derived bound, worst per family and class: " + "  ".join("%s (%s) %.3f" % (f, c, q) for (f, c), q in sorted(worst.items())))


# ------------------------------------------------------------------------------------------ class (e): degenerate sizes
def degenerate_direct_cases():
    """(family, k, stride, L, name, x, (outH, outW)) over the class (e) shapes of the direct split-operand families."""
    for j, (c, H, W) in enumerate(R64.SHAPES_E_S1):
        L = R64.tame_layer(c, c, 3, 1100 + j)
        for name, x, _, _ in R64.degenerate_images(c, H, W, 1100 + j):
            yield "d3h", 3, 1, L, f"{c} {H}x{W} {name}", x
    for j, (cin, cout, k, H, W) in enumerate(R64.SHAPES_E_S2):
        L = R64.tame_layer(cin, cout, k, 1200 + j)
        for name, x, _, _ in R64.degenerate_images(cin, H, W, 1200 + j):
            yield "d3h_s2", k, 2, L, f"{cin}->{cout} k{k}s2 {H}x{W} {name}", x
    for family, layers in (("pxh", [(sum(s), co, 1, R64.SIZES_E_PXH) for s, co in R64.SHAPES_E_PXH]), ("t3h", [(ci, co, 3, R64.SIZES_E_T3H) for ci, co in R64.SHAPES_E_T3H])):
        for j, (cin, cout, k, sizes) in enumerate(layers):
            L = R64.tame_layer(cin, cout, k, 1300 + j)
            for (H, W) in sizes:
                for name, x, _, _ in R64.degenerate_images(cin, H, W, 1300 + j):
                    yield family, k, 1, L, f"{cin}->{cout} {H}x{W} {name}", x


def test_direct_split_models_on_degenerate_sizes():
    """Class (e) (tests/conv_ref64.py): the three-piece-pair arithmetic at 16 x 16 down to 1 x 1, every shape and input the GPU test
    runs, inside the derived bound, finite, exact zeros — the references and the bounds are right there before any kernel is blamed."""
    worst = {}
    for family, k, stride, L, name, x in degenerate_direct_cases():
        s = run_direct(L, x, k, stride, family, model=split_conv_model_taps, cls="e")
        worst[family] = max(worst.get(family, 0.0), s["q"])
        assert inside_caps(s, family), (family, name, s)
    print("class (e), direct split models, worst err / bound: " + "  ".join("%s %.3f" % kv for kv in sorted(worst.items())))


@pytest.mark.parametrize("defect", GEOMETRY_DEFECTS)
def test_geometry_defects_exceed_the_bound_on_degenerate_sizes(defect):
    """The border by clamping instead of zero padding; the outputs of a ragged last 4 x 4 tile left unwritten.  On every class (e) shape
    of the 3x3 / 4x4 families that has a border tap / a ragged tile, the unit-scale case, the constant and the checkerboard must each
    exceed the caps (on a constant 1 a corner sees 9 taps where 4 are due: an error of order 1), and so must an impulse on a border
    pixel / every impulse; the intact model stays inside them (the test above)."""
    seen = 0
    for family, k, stride, L, name, x in degenerate_direct_cases():
        if k == 1 or x.shape[0] > 64:                                      # (the geometry is the same at every channel count)
            continue
        oh, ow = (x.shape[1] + 2 * ((k - 1) // 2) - k) // stride + 1, (x.shape[2] + 2 * ((k - 1) // 2) - k) // stride + 1
        if defect == "ragged_unwritten" and oh % 4 == 0 and ow % 4 == 0:
            continue
        dense = "impulse" not in name
        if defect == "border_clamped" and not dense:
            _, y, x_ = np.argwhere(x != 0)[0].tolist()
            # a clamped coordinate re-reads a border pixel where a tap of some output falls outside on that side: always above and to
            # the left (pad >= 1); below / to the right iff the last output's last tap, (o - 1) stride - pad + k - 1, passes the image —
            # at stride 1 always, at stride 2 for some sizes only.  An impulse elsewhere (interior, or on a far border that no tap
            # leaves) is read exactly as with zero padding: not a case of this defect.
            pad, Hh, Ww = (k - 1) // 2, x.shape[1], x.shape[2]
            below, right = (oh - 1) * stride - pad + k - 1 >= Hh, (ow - 1) * stride - pad + k - 1 >= Ww
            assert stride == 2 or (below and right)
            if not (y == 0 or x_ == 0 or (y == Hh - 1 and below) or (x_ == Ww - 1 and right)):
                continue
        s = run_direct(L, x, k, stride, family, model=split_conv_model_taps, defect=defect, cls="e")
        hit = not inside_caps(s, family)
        seen += 1
        print("%-16s %-7s %-44s err/bound %10.3g  %s" % (defect, family, name, s["q"], "CAUGHT" if hit else "-"))
        assert hit, (defect, family, name, s)                            # (intact: test_direct_split_models_on_degenerate_sizes)
    assert seen > 100, seen


def test_winograd_models_on_degenerate_sizes():
    """The lane-exact model of gated_conv_wino4h_kernel and the model of gated_conv_f4x1h_kernel, on the library's packed operands, over
    the 3x3 / stride-1 shapes of class (e): a 6 x 6 patch that is halo on all four sides, segments and tiles that hang over the image
    in both directions.  F(4,3) by rows: every input of every shape.  F(4x4): the unit-scale case and the constant 1 (on which a halo
    mistake is an error of order 1) at every shape, every input at C = 32 — the lane-exact model takes seconds per case at C = 256."""
    worst = {"w4h": 0.0, "f4x1": 0.0}
    for j, (c, H, W) in enumerate(R64.SHAPES_E_S1):
        L = R64.tame_layer(c, c, 3, 1100 + j)
        for name, x, _, _ in R64.degenerate_images(c, H, W, 1100 + j):
            s = run_f4x1(L, x, cls="e")
            worst["f4x1"] = max(worst["f4x1"], s["q"])
            assert f4x1_inside_caps(s), ("f4x1", c, H, W, name, {k: v for k, v in s.items() if k != "got"})
            if c == 32 or name in ("unit scale", "constant 1"):
                s = run_wino(L, x, cls="e")
                worst["w4h"] = max(worst["w4h"], s["q"])
                assert wino_inside_caps(s), ("w4h", c, H, W, name, s)
    print("class (e), Winograd models, worst err / bound: " + "  ".join("%s %.3f" % kv for kv in sorted(worst.items())))


def test_launch_models_on_degenerate_sizes():
    """pxh_launch_model on the resampled-source and addend cases of class (e) (a coarse source of 2 x 2 / one pixel, addends of one,
    two and four rows), head_model on the head's, and the chain on the levels of a 16 x 16 viewport: inside the derived bounds."""
    from tests import test_gpu_conv_accuracy as G
    worst = {}
    for group, family in (("resampled", "pxh"), ("pxh_pre", "pxh_pre"), ("sc", "sc")):
        for cases in G.cases_e(group):
            for case in cases:
                ref = case.ref()
                df, dm, _ = G._bounds(case, family)
                H, W = case.x.shape[1:]
                got = head_model(case.L, case.x).transpose(1, 2, 0) if family == "sc" else pxh_launch_model(case.L, list(zip(case.xs, case.shifts)), H, W, case.pre)
                q = _q(got, np.concatenate([ref.f, ref.m]), np.concatenate([df, dm]))
                worst[group] = max(worst.get(group, 0.0), q)
                assert q <= 1.0, (group, case.name, q)
    for cls in "ab":
        q = chain_q(*chain_inputs(cls, R64.SIZES_E_CHAIN))
        worst["chain " + cls] = max(q.values())
        assert max(q.values()) <= 1.0, (cls, q)
    print("class (e), launch models, worst err / bound: " + "  ".join("%s %.3f" % kv for kv in sorted(worst.items())))
