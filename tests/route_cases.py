"""The descriptor sweep behind tests/test_conv_route.py, and what is asked of a library for each descriptor.

tests/golden/make_route_golden.py runs it against a library built at the PARENT of a dispatcher change and stores the answers
(tests/golden/conv_route.json); the test runs it against the current library and compares.  Every pointer is fake (aligned,
non-null, never dereferenced): read_conv_kernel_family only reads the descriptor, and on a machine without a GPU a launch that
passes validation fails in the HIP runtime (READ_EHIP) before anything is touched.  NEVER run the outcome sweep where a GPU is
visible.
"""
import ctypes as C
import itertools

import numpy as np

CINS = (8, 16, 24, 32, 48, 64, 128, 256, 480)
COUTS = (3, 4, 32, 56, 64, 128)
KS = ((1, 1), (3, 1), (3, 2), (4, 2))                    # (ksize, stride)
SOURCES = ("one", "one_shift", "two", "two_shift")
MODES = ("plain", "linear", "linear_gated", "mul", "residual", "pre", "pre_bilinear", "fill")
# every forced config, then table indices: a 3x3/s1 tile entry, a 1x1 entry, a wave-autonomous entry, the Winograd entry, out of range
CONFIGS = tuple(range(-1, -13, -1)) + (0, 14, 25, 33, 99)
OPERANDS = ("wpacked", "wpacked_wino", "wpacked_w16", "wpacked_w4", "wpacked_sc", "wpacked_w4h", "wpacked_d3h", "wpacked_t3h", "f4x1")
# the shapes the issue anchors, plus the descriptor pyramid's first layer, a decoder 4x4/s2 and the 32 -> 32 ResBlock
ANCHOR_SHAPES = ((64, 64, 3, 1), (32, 3, 3, 1), (64, 128, 3, 2), (128, 64, 1, 1), (24, 56, 1, 1), (48, 64, 3, 1), (8, 32, 3, 1),
                 (64, 64, 4, 2), (32, 32, 3, 1))
# routing knobs: (key, default, one other value); each is also swept at 0
KNOBS = (("conv_wave", 1, 1), ("conv_px", 1, 3), ("conv_kc32", 1, 1), ("conv_sc", 8, 16), ("conv_wino", 1 << 30, 32), ("conv_w16", 0, 1),
         ("conv_w4", 32, 64), ("conv_w4h", 32, 64), ("conv_f4x1", 32, 64), ("conv_d3h", 0, 64), ("conv_d3h_fam", 32, 64),
         ("conv_d3h_s2", 32, 64), ("conv_pxh", 16, 64), ("conv_t3h", 8, 32))
KNOB_VALUES = (-5, -1, 0, 1, 2, 3, 4, 5, 8, 16, 32, 64, 1 << 30)
# retired keys (attribution probes and two measured-slower kernels, removed from the sources): "unknown key" in every library
RETIRED_KEYS = ("conv_ablate", "conv_abl", "conv_w4x2", "conv_w4h_waves")
PLAN_SIZES = ((352, 1216), (256, 256))
PLAN_KNOBS = ({}, {"conv_w4": 0, "conv_w4h": 0, "conv_d3h_fam": 0})

_BASE = 0x10000000          # fake device addresses, 16 MiB apart, 256-byte aligned
_SLOT = {n: _BASE + (i + 1) * 0x1000000 for i, n in enumerate(
    OPERANDS + ("params", "out", "mul", "residual", "pre", "out_gated", "src0", "src1"))}


def _up4(v):
    return (v + 3) // 4 * 4


def make_desc(_lib, cin, cout, ksize, stride, sources="one", mode="plain", config=-1, absent=(), misaligned=(), H=96, W=192):
    """(descriptor, f4x1 operand) or None where the case does not exist (two sources of 8 channels in all)."""
    def ptr(name):
        if name in absent:
            return None
        return _SLOT[name] + (4 if name in misaligned else 0)

    if sources.startswith("two"):
        if cin < 16:
            return None
        chans = (cin // 2, cin // 2) if cin % 32 == 0 else (8, cin - 8)
    else:
        chans = (cin,)
    d = _lib.ConvDesc()
    d.n_src = len(chans)
    for i, c in enumerate(chans):
        coarse = sources.endswith("shift") and i == len(chans) - 1      # the last source at half resolution (nearest up-sampling)
        d.src[i].data = ptr("src%d" % i)
        d.src[i].C = c
        d.src[i].shift = -1 if coarse else 0
        d.src[i].srcH = ((H - 1) >> 1) + 1 if coarse else H
        d.src[i].srcW = ((W - 1) >> 1) + 1 if coarse else W
    pad = (ksize - 1) // 2
    outH, outW = (H + 2 * pad - ksize) // stride + 1, (W + 2 * pad - ksize) // stride + 1
    linear = mode.startswith("linear")
    d.inH, d.inW, d.Cout, d.ksize, d.stride, d.elu = H, W, cout, ksize, stride, 1
    d.linear = 1 if linear else 0
    d.out_cstride = _up4((2 if linear else 1) * cout) + (4 if mode == "fill" else 0)
    d.params, d.out, d.config = ptr("params"), ptr("out"), config
    for name in OPERANDS[:-1]:
        setattr(d, name, ptr(name))
    if mode == "linear_gated":
        d.out_gated, d.block_h, d.valid_h = ptr("out_gated"), 0, 0
    if mode == "mul":
        d.mul = ptr("mul")
    if mode == "residual":
        d.residual = ptr("residual")
    if mode == "fill":
        d.fill_pad, d.out_fill = 1, 1.0
    if mode.startswith("pre"):
        d.pre, d.pre_shift = ptr("pre"), 2
        d.pre_f_off, d.pre_m_off, d.pre_cstride = 0, _up4(cout), 2 * _up4(cout)
        d.preH, d.preW = ((outH - 1) >> 2) + 1, ((outW - 1) >> 2) + 1
        d.pre_bilinear = 1 if mode == "pre_bilinear" else 0
    return d, ptr("f4x1")


def shape_cases(_lib):
    """Set A: every shape x sources x mode x config, all operands present."""
    for (cin, cout), (k, s), src, mode, cfg in itertools.product(itertools.product(CINS, COUTS), KS, SOURCES, MODES, CONFIGS):
        c = make_desc(_lib, cin, cout, k, s, src, mode, cfg)
        if c:
            yield c


def operand_variants():
    """(absent, misaligned) operand names; variant 0 = everything present and aligned."""
    variants = [((), ())]
    variants += [((n,), ()) for n in OPERANDS] + [((), (n,)) for n in OPERANDS + ("mul", "out", "params")]
    variants += [(tuple(m for m in OPERANDS if m != n), ()) for n in OPERANDS]
    variants += [(tuple(m for m in OPERANDS if m not in (n, "wpacked")), ()) for n in OPERANDS[1:]]
    return variants


def operand_cases(_lib):
    """Set B: each operand pointer absent, misaligned, or the only one present (the variants are the innermost axis)."""
    for (cin, cout, k, s), mode, cfg, (absent, mis) in itertools.product(ANCHOR_SHAPES, ("plain", "linear", "mul"), CONFIGS, operand_variants()):
        yield make_desc(_lib, cin, cout, k, s, "one", mode, cfg, absent, mis)


def knob_cases(_lib):
    """Set C (run once per knob setting): every shape under the automatic choice, one and two sources, at two image sizes."""
    for (cin, cout), (k, s), src, mode in itertools.product(itertools.product(CINS, COUTS), KS, ("one", "two"), ("plain", "linear", "mul")):
        for (H, W) in ((96, 192), (44, 152)):
            c = make_desc(_lib, cin, cout, k, s, src, mode, -1, H=H, W=W)
            if c:
                yield c


def knob_settings():
    yield None
    for key, default, other in KNOBS:
        for v in sorted({0, other} - {default}):
            yield key, v


class Sweep:
    """Runs the three sets against a loaded library: families (read_conv_kernel_family) and, on request, launch outcomes."""

    def __init__(self, _lib):
        self._lib, self.L = _lib, _lib.lib()

    def _set_knob(self, setting):
        for key, default, _ in KNOBS:
            self._lib.check(self.L.read_tuning_set(key.encode(), default))
        if setting:
            self._lib.check(self.L.read_tuning_set(setting[0].encode(), setting[1]))

    def sets(self):
        """(name, iterator of cases); the knob is set while the iterator is consumed and reset afterwards."""
        yield "shapes", shape_cases(self._lib)
        yield "operands", operand_cases(self._lib)
        for setting in knob_settings():
            self._set_knob(setting)
            try:
                yield ("knob:%s=%d" % setting if setting else "knob:defaults"), knob_cases(self._lib)
            finally:
                self._set_knob(None)

    def family(self, case):
        return self.L.read_conv_kernel_family(C.byref(case[0]))

    def outcome(self, case, f4x1):
        """(rc, message): the message of a refusal (READ_EINVAL); None otherwise — a HIP error's text carries file:line."""
        d, wp = case
        rc = self.L.read_gated_conv_forward_f4x1(C.byref(d), wp, None) if f4x1 else self.L.read_gated_conv_forward(C.byref(d), None)
        return rc, (self.L.read_last_error().decode() if rc == -22 else None)


def rle(seq):
    """[v, n, v, n, ...]: run-length encoding of a sequence of small integers."""
    out = []
    for v in seq:
        if out and out[-2] == v:
            out[-1] += 1
        else:
            out += [v, 1]
    return out


def unrle(flat):
    return [v for v, n in zip(flat[::2], flat[1::2]) for _ in range(n)]


def pack(seq, block):
    """A sequence as a table of its distinct blocks (the innermost sweep axis) and the run-length-encoded block numbers."""
    assert len(seq) % block == 0
    table, ids = [], []
    for i in range(0, len(seq), block):
        b = seq[i:i + block]
        if b not in table:
            table.append(b)
        ids.append(table.index(b))
    return {"block": block, "table": table, "ids": rle(ids)}


def diff(seq, base, of):
    """A sequence as its differences [i, v, i, v, ...] from another recorded one (`of` = [set, field])."""
    assert len(seq) == len(base)
    return {"of": of, "diff": [x for i, (v, w) in enumerate(zip(seq, base)) if v != w for x in (i, v)]}


def unpack(sets, name, field):
    e = sets[name][field]
    if "of" in e:
        seq = unpack(sets, *e["of"])
        for i, v in zip(e["diff"][::2], e["diff"][1::2]):
            seq[i] = v
        return seq
    return [v for b in unrle(e["ids"]) for v in e["table"][b]]


def knob_table(_lib):
    """{key: [read_tuning_get after read_tuning_set(key, v) for v in KNOB_VALUES]} over every conv key; defaults restored."""
    L, keys, table = _lib.lib(), tuning_keys(_lib), {}
    for key in (k for k in keys if k.startswith("conv_")):
        v0, got = C.c_int(), []
        _lib.check(L.read_tuning_get(key.encode(), C.byref(v0)))
        for v in KNOB_VALUES:
            g = C.c_int()
            _lib.check(L.read_tuning_set(key.encode(), v))
            _lib.check(L.read_tuning_get(key.encode(), C.byref(g)))
            got.append(g.value)
        _lib.check(L.read_tuning_set(key.encode(), v0.value))
        table[key] = [v0.value] + got
    return table


def tuning_keys(_lib):
    L, keys = _lib.lib(), []
    while L.read_tuning_key(len(keys)):
        keys.append(L.read_tuning_key(len(keys)).decode())
    return keys


def plans(_lib):
    """[[layout, H, W, knobs, rc, error text, launch count]] of read_unet_create_layout on the CPU (fake blob and workspace)."""
    L, out = _lib.lib(), []
    for knobs in PLAN_KNOBS:
        saved = {}
        for k, v in knobs.items():
            g = C.c_int()
            _lib.check(L.read_tuning_get(k.encode(), C.byref(g)))
            saved[k] = g.value
            _lib.check(L.read_tuning_set(k.encode(), v))
        try:
            for layout, (H, W) in itertools.product((0, 1, 2), PLAN_SIZES):
                h = C.c_void_p()
                need = L.read_unet_workspace_bytes(H, W)
                ws = np.empty(need + 256, np.uint8)              # never touched: the plan only takes addresses inside it
                rc = L.read_unet_create_layout(C.byref(h), _BASE, H, W, (ws.ctypes.data + 255) // 256 * 256, need, layout)
                err = L.read_last_error().decode() if rc else ""
                n = L.read_unet_launch_count(h) if rc == 0 else 0
                if rc == 0:
                    L.read_unet_destroy(h)
                out.append([layout, H, W, knobs, rc, err, n])
        finally:
            for k, v in saved.items():
                _lib.check(L.read_tuning_set(k.encode(), v))
    return out
