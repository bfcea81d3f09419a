"""What tests/test_weight_orders.py holds against tests/golden/weight_orders.json, and the packed UNet blobs the CPU tests share.

Everything here goes through whichever `read_amd` is importable: the tests' own, or — in tests/golden/make_weight_orders_golden.py —
the reference tree's.  The blobs are packed once per process and handed out read-only (flags.writeable is off).
"""
import functools
import hashlib

import numpy as np

LAYOUTS = {"full": 0, "lean": 1, "lean_w4h": 2}          # READ_UNET_LAYOUT_*
BLOB_SEED = 3

# (Cin, Cout, k) of the single-layer packer: every presence boundary of PackedGatedConv — Cin 8 / 16 / 32 / not a multiple of 16,
# Cout 3 / 24 / a multiple of 32, k 1 / 3 / 4, Cin above 256
SHAPES = [(8, 32, 3), (16, 8, 3), (32, 3, 3), (32, 32, 3), (40, 32, 3), (48, 64, 3), (64, 64, 3), (64, 128, 3), (64, 24, 3), (128, 64, 4),
          (64, 64, 1), (24, 56, 1), (272, 32, 1), (480, 32, 1)]
# the attributes of PackedGatedConv that hold one weight order each (None: the layer does not carry it)
ORDER_ATTRS = ("wpacked", "params", "wpacked_wino", "wpacked_w16", "wpacked_w4", "wpacked_w4h", "wpacked_f4x1", "wpacked_d3h", "wpacked_t3h",
               "wpacked_sc")


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a)).hexdigest()


@functools.lru_cache(maxsize=None)
def blob(layout):
    """pack_state(make_unet_state(UNET_SPEC, 3), layout) as a host ndarray (zero-filled first: the alignment gaps are part of it)."""
    from read_amd import synthetic
    from read_amd.unet import pack_state
    from tests.unet_spec import UNET_SPEC
    b = pack_state(synthetic.make_unet_state(UNET_SPEC, BLOB_SEED), layout=layout)
    b.flags.writeable = False
    return b


@functools.lru_cache(maxsize=None)
def side_buffer():
    """The F(4,3)-by-rows side buffer a host derives from the FULL blob, as a host ndarray."""
    import warnings
    import torch
    from read_amd.unet import f4x1_side_buffer
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)              # torch warns that the blob is not writable; f4x1_side_buffer only reads it
        s = f4x1_side_buffer(torch.from_numpy(blob(LAYOUTS["full"]))).numpy()
    s.flags.writeable = False
    return s


def layer_inputs(cin, cout, k):
    """wf, bf, wm, bm, gamma, beta, mean, var of one BasicConv, from default_rng([Cin, Cout, k])."""
    r = np.random.default_rng([cin, cout, k])
    w = lambda: r.standard_normal((cout, cin, k, k)).astype(np.float32)
    v = lambda: r.standard_normal(cout).astype(np.float32)
    pos = lambda: r.uniform(0.5, 1.5, cout).astype(np.float32)
    wf, wm = w(), w()
    bf, bm = v(), v()
    return wf, bf, wm, bm, pos(), v(), v(), pos()


def layer_record(cin, cout, k):
    """{"kc", "orders": {attribute: sha256}} of PackedGatedConv on the CPU: the orders present and their bytes."""
    from read_amd.gated_conv import PackedGatedConv
    p = PackedGatedConv(*layer_inputs(cin, cout, k), device="cpu")
    return {"kc": p.kc, "orders": {a: sha256(getattr(p, a).numpy()) for a in ORDER_ATTRS if getattr(p, a) is not None}}


def blob_record(name):
    b = blob(LAYOUTS[name])
    return {"floats": int(b.size), "sha256": sha256(b)}


def side_record():
    s = side_buffer()
    return {"floats": int(s.size), "sha256": sha256(s)}
