"""CPU: NumPy model of the exact arithmetic of gated_conv_f4x1h_kernel (read_amd/csrc/conv.hip) — Winograd F(4,3) along x only, the three
ky taps direct, split fp32 operands on v_mfma_f32_16x16x32_f16 — fed by the LIBRARY's host packer (read_conv_pack_f4x1_host):

    M[y][f] = sum_ky sum_c U[ky][f][c] V[y + ky - 1][f][c],   V[r] = B^T d_r,   U[ky] = G w[ky][:],   Y = A^T M
    V = Vh + 2^-11 Vl,  U s = Uh + Ul,  product = (2^-11 Uh) Vl + Ul Vh + Uh Vh  (fp32 accumulator),  result / s

  * packer output -> split pieces -> three products -> 1-D output transform against a float64 direct convolution (C = 32 and 256);
  * the packed fragment order [group][wave][chunk][ky 3][frequency 6][Uh | Ul][lane][8 halfs] decoded back to G w;
  * the transform's amplification bound, from the matrix: the largest row sum of |B^T| is 10.

THE BOUND of the first check (derived, per output element; u = 2^-24, the counting of tests/conv_ref64.py carried over to one
transform pass).  With A_in = |A^T| (sum_ky sum_c |U| (|B^T| |d|)) — the absolute-value image of the whole computation —
    input transform bt6: an add followed by an fma, or two fmas = 2 roundings, ONE pass .............  2 u
    split operands: 4 u per operand + 4 u for the dropped pair .......................................  12 u
    accumulation: 9 MFMAs (3 taps x 3 piece pairs) per 32-channel block, one rounding each ..........  9 (Cin / 32) u
    output transform: the longest path is three additions (Y0 = M0 + s1 + s2; 2, 4, 8 are exact) ....  3 u
    the product with 1 / s is exact (a power of two).
    |model - f64|  <=  u (2 + 12 + 9 Cin / 32 + 3) A_in  +  floors
floors: the f16 quantum 2^-24 of the low pieces (conv_ref64.W_FLOOR per weight in units of U s, X_FLOOR per transformed activation).
"""
import numpy as np
import pytest

from tests.conv_ref64 import U as U32, W_FLOOR, X_FLOOR
from tests.wino4_ref import AT, BT, G

LANE = np.arange(64)


def _lib():
    from read_amd import _lib as L_
    return L_.lib()


def pack_f4x1(wf, wm):
    """The library's packer -> (halfs float16 [group][wave 4][chunk][ky 3][frequency 6][piece 2][lane 64][8], inv float32 [2][CoutPad])."""
    L = _lib()
    cout, cin = wf.shape[:2]
    cp = (cout + 31) // 32 * 32
    n = L.read_conv_f4x1_floats(cin, cout)
    assert n == cin * 18 * 2 * cp + 2 * cp                         # half the F(4x4) order
    assert 2 * (n - 2 * cp) == L.read_conv_w4h_floats(cin, cout) - 2 * cp
    blob = np.zeros(n, np.float32)
    assert L.read_conv_pack_f4x1_host(cin, cout, np.ascontiguousarray(wf).ctypes.data, np.ascontiguousarray(wm).ctypes.data, blob.ctypes.data) == 0
    halfs = blob[:n - 2 * cp].view(np.float16).reshape(cp // 32, 4, cin // 32, 3, 6, 2, 64, 8)
    return halfs, blob[n - 2 * cp:].reshape(2, cp)


def decode_rows(halfs, cin, cp):
    """-> (Uh, Ul) float64 [fm 2][co CoutPad][ky 3][frequency 6][cin]: the A operand's lane map undone (lane = i + 16 kq: row i =
    co % 8 + 8 fm of wave (co % 32) / 8, input channels 32 chunk + 8 kq + e)."""
    out = np.zeros((2, 2, cp, 3, 6, cin))
    for g in range(cp // 32):
        for w in range(4):
            for c in range(cin // 32):
                blk = halfs[g, w, c].astype(np.float64)            # (ky, fq, piece, lane, e)
                for lane in range(64):
                    i, kq = lane & 15, lane >> 4
                    co, fm = 32 * g + 8 * w + (i & 7), i >> 3
                    for piece in range(2):
                        out[piece, fm, co, :, :, 32 * c + 8 * kq:32 * c + 8 * kq + 8] = blk[:, :, piece, lane, :]
    return out[0], out[1]


def f4x1_conv_model(x_hwc, Uh, Ul, inv, cout):
    """-> (f, m) float32 (H, W, cout): the kernel's arithmetic on x (H, W, Cin) float32."""
    H, W, cin = x_hwc.shape
    nt = (W + 3) // 4
    xp = np.zeros((H + 2, 4 * nt + 2, cin), np.float32)
    xp[1:H + 1, 1:W + 1] = x_hwc
    d = np.stack([xp[:, j:j + 4 * nt:4] for j in range(6)], axis=2)              # (row, tile, 6, cin): columns 4 t - 1 + j
    V = np.einsum("fj,rtjc->rtfc", BT.astype(np.float32), d).astype(np.float32)   # fp32 transform
    Vh = V.astype(np.float16)
    Vl = ((V - Vh.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    Vh, Vl = Vh.astype(np.float64), Vl.astype(np.float64)
    outs = []
    for fm in range(2):
        acc = np.zeros((H, nt, 6, cout), np.float32)
        uh, ul = Uh[fm, :cout], Ul[fm, :cout]                                     # (co, ky, f, cin)
        us = uh * 2.0 ** -11                                                      # v_pk_mul_f16: exact for these magnitudes or rounded to the f16 quantum
        us = us.astype(np.float16).astype(np.float64)
        for c0 in range(0, cin, 32):                                              # one fp32 rounding per 32-channel block and tap triple
            blk = np.zeros((H, nt, 6, cout))
            for ky in range(3):
                vh, vl = Vh[ky:ky + H, :, :, c0:c0 + 32], Vl[ky:ky + H, :, :, c0:c0 + 32]
                blk += np.einsum("ofc,ytfc->ytfo", us[:, ky, :, c0:c0 + 32], vl) + np.einsum("ofc,ytfc->ytfo", ul[:, ky, :, c0:c0 + 32], vh) + \
                    np.einsum("ofc,ytfc->ytfo", uh[:, ky, :, c0:c0 + 32], vh)
            acc = (acc.astype(np.float64) + blk).astype(np.float32)
        Y = np.einsum("pf,ytfo->ytpo", AT.astype(np.float32), acc).astype(np.float32)
        outs.append((Y.reshape(H, 4 * nt, cout)[:, :W] * inv[fm, :cout][None, None, :]).astype(np.float32))
    return outs


def conv64(x_hwc, w):
    H, W, _ = x_hwc.shape
    xp = np.zeros((H + 2, W + 2, x_hwc.shape[2]))
    xp[1:H + 1, 1:W + 1] = x_hwc
    out = np.zeros((H, W, w.shape[0]))
    for ky in range(3):
        for kx in range(3):
            out += np.einsum("hwc,oc->hwo", xp[ky:ky + H, kx:kx + W], w[:, :, ky, kx].astype(np.float64))
    return out


def bound(x_hwc, w, inv_rows):
    """u (26 + 9 Cin / 32) A_in + floors, A_in in the transformed domain (module docstring)."""
    H, W, cin = x_hwc.shape
    cout = w.shape[0]
    nt = (W + 3) // 4
    xp = np.zeros((H + 2, 4 * nt + 2, cin))
    xp[1:H + 1, 1:W + 1] = np.abs(x_hwc)
    d = np.stack([xp[:, j:j + 4 * nt:4] for j in range(6)], axis=2)
    Vabs = np.einsum("fj,rtjc->rtfc", np.abs(BT).astype(np.float64), d)
    Uabs = np.abs(np.einsum("fb,ocab->oafc", G, w.astype(np.float64)))            # (co, ky, f, cin)
    A = np.zeros((H, nt, 6, cout))
    X1 = np.zeros((H, nt, 6))
    for ky in range(3):
        A += np.einsum("ofc,ytfc->ytfo", Uabs[:, ky], Vabs[ky:ky + H])
        X1 += Vabs[ky:ky + H].sum(axis=3)
    W1 = Uabs.sum(axis=(1, 3))                                                    # (co, f)
    absAT = np.abs(AT).astype(np.float64)
    Ain = np.einsum("pf,ytfo->ytpo", absAT, A).reshape(H, 4 * nt, cout)[:, :W]
    floor = np.einsum("pf,ytf->ytp", absAT, X1).reshape(H, 4 * nt)[:, :W, None] * W_FLOOR * inv_rows[None, None, :] + \
        np.tile(np.einsum("pf,of->po", absAT, W1), (nt, 1))[None, :W] * X_FLOOR
    return U32 * (2 + 12 + 9 * (cin // 32) + 3) * Ain + floor


@pytest.mark.parametrize("cin,cout,H,W", [(32, 32, 11, 21), (256, 40, 7, 14)])
def test_f4x1_model_against_float64(cin, cout, H, W):
    rng = np.random.default_rng([41, cin])
    b = 1.0 / np.sqrt(cin * 9)
    wf = rng.uniform(-b, b, (cout, cin, 3, 3)).astype(np.float32)
    wm = rng.uniform(-b, b, (cout, cin, 3, 3)).astype(np.float32) * np.float32(0.25)
    wm[3] = 0.0                                                                   # an all-zero row keeps scale 1
    x = rng.standard_normal((H, W, cin)).astype(np.float32)
    halfs, inv = pack_f4x1(wf, wm)
    cp = inv.shape[1]
    Uh, Ul = decode_rows(halfs, cin, cp)
    f, m = f4x1_conv_model(x, Uh, Ul, inv, cout)
    for got, w, fm in ((f, wf, 0), (m, wm, 1)):
        ref = conv64(x, w)
        err = np.abs(got.astype(np.float64) - ref)
        bd = bound(x, w, inv[fm, :cout].astype(np.float64)) + U32 * np.abs(ref)   # + the final rounding of the result to fp32
        print(f"f4x1 model C={cin} {'fm'[fm]}: max err {err.max():.3e}  max err / bound {float((err / np.maximum(bd, 1e-300)).max()):.3f}")
        assert np.all(err <= bd), (cin, fm, float((err / np.maximum(bd, 1e-300)).max()))
    assert inv[1, 3] == 1.0 and not m[..., 3].any()


def test_f4x1_fragment_order_decodes_to_G_w():
    rng = np.random.default_rng(43)
    cin, cout = 64, 40
    wf = (rng.standard_normal((cout, cin, 3, 3)) * 0.2).astype(np.float32)
    wm = (rng.standard_normal((cout, cin, 3, 3)) * 0.05).astype(np.float32)
    halfs, inv = pack_f4x1(wf, wm)
    cp = inv.shape[1]
    Uh, Ul = decode_rows(halfs, cin, cp)
    for fm, w in enumerate((wf, wm)):
        w64 = w.astype(np.float64).transpose(0, 2, 1, 3)                          # (co, ky, cin, kx)
        want = sum(G[None, None, :, None, b] * w64[:, :, None, :, b] for b in range(3))   # U[ky] = G w[ky][:]: (co, ky, f, cin), summed in the packer's order
        s = 1.0 / inv[fm, :cout].astype(np.float64)
        top = np.abs(want).reshape(cout, -1).max(axis=1) * s
        assert np.all((top >= 2.0 ** 14) & (top < 2.0 ** 15))                     # the scale rule
        Us = want * s[:, None, None, None]
        hi = Us.astype(np.float16).astype(np.float64)
        lo = (Us - hi).astype(np.float16).astype(np.float64)
        assert np.array_equal(Uh[fm, :cout], hi) and np.array_equal(Ul[fm, :cout], lo), "fragment order or pieces"
        assert np.abs(hi + lo - Us).max() <= 2.0 ** -22 * 2.0 ** 15
        assert not Uh[fm, cout:].any() and not Ul[fm, cout:].any() and np.all(inv[fm, cout:] == 1.0)   # padded rows
    assert _lib().read_conv_f4x1_floats(48, 32) == 0                              # whole 32-channel chunks only


def test_f4x1_amplification_and_swizzle():
    """The input transform multiplies by at most 10 (F(4x4): 10 x 10), so the f16 pieces overflow at 65504 / 10 = 6550; and the V image's
    slot swizzle keeps the four 16-lane groups of ds_read_b128 on 16 different 16-byte bank quads for even AND odd row pairs."""
    assert np.abs(BT).sum(axis=1).max() == 10.0
    assert 5000.0 * 10.0 < 65504.0 and 2.0 * 3275.0 * 10.0 <= 65504.0
    t, kl = LANE & 15, LANE >> 4
    for odd in (0, 1):
        key = (t >> 2) ^ (2 * odd)                                                # 2 (row & 1) + (segment >> 2) of the row the lane reads
        addr16 = (t & 7) * 4 + (kl ^ ((-key) & 3))                                # 16-byte units; the row stride is a multiple of 256 bytes
        for grp in ([0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]):
            for half in (0, 32):
                assert len({int(addr16[l + half]) % 16 for l in grp}) == 16
    # the transform's stores: a wave writes (row, frequency, piece) as 64 different dwords of one 256-byte row
    for wv in range(4):
        cp_, sg = LANE & 15, (wv & 1) * 4 + (LANE >> 4)
        dw = sg * 16 + (((cp_ >> 2) ^ ((-wv) & 3)) << 2) + (cp_ & 3)
        assert len(set((dw % 64).tolist())) == 64
        # ... and what a reader of that row finds under its key is the slot the writer used: key = 2 (row & 1) + (segment >> 2) = wave
        assert np.all((2 * ((wv >> 1) & 1) + (sg >> 2)) == wv)


def test_f4x1_order_in_the_unet_blobs():
    """The lean blob carries the order of every split-operand 3x3/s1 layer the plan launches (70), the full blob is laid out as before
    and a host derives the same bits from its direct fragments (read_conv_unpack_weights_host is the exact inverse of the packer);
    the lean layout without the order is still known, by its length."""
    import ctypes as C
    from read_amd.unet import LAYOUT_FULL, LAYOUT_LEAN, LAYOUT_LEAN_W4H, layout_of
    from tests.weight_order_cases import blob
    L = _lib()
    n_side = L.read_unet_f4x1_floats()
    assert L.read_unet_packed_floats_layout(LAYOUT_LEAN) == L.read_unet_packed_floats_layout(LAYOUT_LEAN_W4H) + n_side
    assert L.read_unet_packed_floats_layout(LAYOUT_FULL) == L.read_unet_packed_floats()
    full, lean, old = (blob(l) for l in (LAYOUT_FULL, LAYOUT_LEAN, LAYOUT_LEAN_W4H))     # pack_state(make_unet_state(UNET_SPEC, 3)), shared
    assert layout_of(old) == LAYOUT_LEAN_W4H and layout_of(lean) == LAYOUT_LEAN
    lean_b = lean.tobytes()
    w_off, s_off, cin, cout = C.c_size_t(), C.c_size_t(), C.c_int(), C.c_int()
    j, total = 0, 0
    while L.read_unet_f4x1_layer(j, C.byref(w_off), C.byref(s_off), C.byref(cin), C.byref(cout)) == 0:
        assert s_off.value == total and cin.value % 32 == 0 and cout.value % 32 == 0
        n = L.read_conv_packed_floats(cin.value, cout.value, 3)
        wf = np.zeros((cout.value, cin.value, 3, 3), np.float32)
        wm = np.zeros_like(wf)
        assert L.read_conv_unpack_weights_host(cin.value, cout.value, 3, 16, full[w_off.value:w_off.value + n].ctypes.data, wf.ctypes.data, wm.ctypes.data) == 0
        if j in (0, 17, 40, 69):                                                  # the derived order is in the lean blob, bit for bit
            f4 = np.zeros(L.read_conv_f4x1_floats(cin.value, cout.value), np.float32)
            assert L.read_conv_pack_f4x1_host(cin.value, cout.value, wf.ctypes.data, wm.ctypes.data, f4.ctypes.data) == 0
            assert f4.tobytes() in lean_b and f4[:256].tobytes() not in old.tobytes()
            again = np.zeros(n, np.float32)
            assert L.read_conv_pack_weights_host(cin.value, cout.value, 3, 16, wf.ctypes.data, wm.ctypes.data, again.ctypes.data) == 0
            assert np.array_equal(again.view(np.uint32), full[w_off.value:w_off.value + n].view(np.uint32))
        total += L.read_conv_f4x1_floats(cin.value, cout.value)
        j += 1
    assert j == 70 and total == n_side
