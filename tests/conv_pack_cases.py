"""The host weight packers on small shapes, as sha256 digests of their output bytes: shared by tests/test_conv_pack_golden.py
and tests/golden/make_conv_pack_golden.py (which records tests/golden/conv_pack_sha256.json from the PARENT's library).

Weights come from one fixed NumPy seed per case.  The rows (conv_f and conv_m of every output channel) are scaled by powers of
two from 2^-70 to 2^20; row 1 of conv_f is all zero and row 1 of conv_m is a row of fp32 denormals (the +-60 clamp of the
split-operand row scale).  Every output buffer is prefilled with 0xA5 bytes and hashed whole, padded rows included.
"""
import ctypes as C
import hashlib

import numpy as np

SEED = 20261019
FILL = 0xA5

# (order, Cin, Cout, ksize, kc): ksize / kc are 0 where the order has none
CASES = (
    [("direct", 8, 5, k, 8) for k in (1, 3, 4)] + [("direct", 32, 40, 1, 16), ("direct", 32, 40, 1, 32), ("direct", 32, 40, 3, 16)]
    + [(o, ci, co, 3, 0) for o in ("wino", "w16", "w4") for ci, co in ((16, 8), (32, 40))]
    + [(o, ci, co, 3, 0) for o in ("w4h", "f4x1", "d3h") for ci, co in ((32, 3), (32, 40), (64, 32))]
    + [("dkh", ci, co, 3, 0) for ci, co in ((32, 3), (32, 40), (64, 32))]
    + [("dkh", 32, 32, 4, 0), ("dkh", 16, 4, 1, 0), ("dkh", 48, 40, 1, 0)]
    + [("t3h", 8, 12, 3, 0), ("t3h", 32, 3, 3, 0), ("sc", 32, 3, 3, 0)]
)
PARAM_COUTS = (3, 40)


def case_id(case):
    o, ci, co, k, kc = case
    return f"{o}-cin{ci}-cout{co}-k{k}" + (f"-kc{kc}" if kc else "")


def weights(case):
    """(wf, wm), each (Cout, Cin, k, k) fp32."""
    o, ci, co, k, kc = case
    rng = np.random.default_rng([SEED, ci, co, k])
    w = rng.standard_normal((2, co, ci, k, k)).astype(np.float32)
    exps = np.linspace(-70, 20, 2 * co).round().astype(np.int64).reshape(2, co)
    rng.shuffle(exps.reshape(-1))
    w = np.ldexp(w, exps[:, :, None, None, None].astype(np.int32)).astype(np.float32)
    if co > 1:
        w[0, 1] = 0.0
        w[1, 1] = (rng.integers(-4000, 4000, size=(ci, k, k)).astype(np.float32) * np.float32(2.0 ** -149)).astype(np.float32)
        assert np.all(np.abs(w[1, 1]) < np.finfo(np.float32).tiny) and np.any(w[1, 1] != 0)
    return np.ascontiguousarray(w[0]), np.ascontiguousarray(w[1])


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _out(nfloats):
    assert nfloats > 0
    return np.full(int(nfloats) * 4, FILL, np.uint8)


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def pack_digest(L, case):
    o, ci, co, k, kc = case
    wf, wm = weights(case)
    if o == "direct":
        out = _out(L.read_conv_packed_floats(ci, co, k))
        assert L.read_conv_pack_weights_host(ci, co, k, kc, _p(wf), _p(wm), _p(out)) == 0
        # ... and back: the unpacked weights are the weights, bit for bit, and go into the digest as the library returned them
        bf, bm = np.full_like(wf, np.nan), np.full_like(wm, np.nan)
        assert L.read_conv_unpack_weights_host(ci, co, k, kc, _p(out), _p(bf), _p(bm)) == 0
        assert np.array_equal(bf.view(np.uint32), wf.view(np.uint32)) and np.array_equal(bm.view(np.uint32), wm.view(np.uint32))
        return _sha(out, bf, bm)
    if o == "dkh":
        out = _out(L.read_conv_dkh_floats(ci, co, k))
        assert L.read_conv_pack_dkh_host(ci, co, k, _p(wf), _p(wm), _p(out)) == 0
        return _sha(out)
    size = {"wino": L.read_conv_wino_floats, "w16": L.read_conv_wino_floats, "w4": L.read_conv_w4_floats, "w4h": L.read_conv_w4h_floats,
            "f4x1": L.read_conv_f4x1_floats, "d3h": L.read_conv_d3h_floats, "t3h": L.read_conv_t3h_floats, "sc": L.read_conv_sc_floats}[o]
    out = _out(size(ci, co))
    assert getattr(L, f"read_conv_pack_{o}_host")(ci, co, _p(wf), _p(wm), _p(out)) == 0
    return _sha(out)


def params_digest(L, cout):
    rng = np.random.default_rng([SEED, cout])
    bf, bm, gamma, beta, mean = (rng.standard_normal(cout).astype(np.float32) for _ in range(5))
    var = rng.uniform(0.01, 4.0, cout).astype(np.float32)
    out = _out(L.read_conv_param_floats(cout))
    assert L.read_conv_pack_params_host(cout, _p(bf), _p(bm), _p(gamma), _p(beta), _p(mean), _p(var), C.c_float(1e-5), _p(out)) == 0
    return _sha(out)


def digests(L):
    """{case id: sha256} for every case, with the library L (read_amd._lib.lib())."""
    d = {case_id(c): pack_digest(L, c) for c in CASES}
    d.update({f"params-cout{co}": params_digest(L, co) for co in PARAM_COUTS})
    return d
