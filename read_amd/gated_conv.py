"""Single-layer front end of ``read_gated_conv_forward`` (READ's BasicConv, unet.py:22-53).

Used by the layer-level parity tests and the tile-configuration sweeps; the full network goes
through ``read_unet_forward`` instead (one C call per frame)."""
import ctypes as C

import numpy as np
import torch

from . import _lib


def kc_for(src_channels):
    """Input-channel chunk of the kernel: 16 when every concatenated source has C % 16 == 0, else 8."""
    return 8 if any(c % 16 for c in src_channels) else 16


def _wino(cin, cout, k):
    return k == 3 and cin % 16 == 0


def _w4(cin, cout, k):
    return _wino(cin, cout, k) and cout % 32 == 0 and cin >= 32


def _w4h(cin, cout, k):
    return _w4(cin, cout, k) and cin % 32 == 0


# The weight orders of one layer, one row each: attribute of PackedGatedConv, whether read_conv_desc has a field of that name, the size
# function and the packer with the arguments each takes (a packer's are followed by wf, wm, dst), and the rule carried(Cin, Cout, k).
# A layer carries an order when its rule holds and the size function answers non-zero.  These rules are the single-layer packer's
# own — every order a kernel could take — not the UNet blob's.
_CC, _CCK, _CCKK = ("cin", "cout"), ("cin", "cout", "k"), ("cin", "cout", "k", "kc")
WEIGHT_ORDERS = (
    ("wpacked", True, "read_conv_packed_floats", _CCK, "read_conv_pack_weights_host", _CCKK, lambda cin, cout, k: True),
    ("wpacked_wino", True, "read_conv_wino_floats", _CC, "read_conv_pack_wino_host", _CC, _wino),        # Winograd F(2x2,3x3)
    ("wpacked_w16", True, "read_conv_wino_floats", _CC, "read_conv_pack_w16_host", _CC, _wino),          # ... in the wave-autonomous kernel's order
    ("wpacked_w4", True, "read_conv_w4_floats", _CC, "read_conv_pack_w4_host", _CC, _w4),                # Winograd F(4x4,3x3)
    ("wpacked_w4h", True, "read_conv_w4h_floats", _CC, "read_conv_pack_w4h_host", _CC, _w4h),            # ... split into f16 piece pairs
    ("wpacked_f4x1", False, "read_conv_f4x1_floats", _CC, "read_conv_pack_f4x1_host", _CC, _w4h),        # F(4,3) by rows: travels beside the descriptor
    ("wpacked_d3h", True, "read_conv_dkh_floats", _CCK, "read_conv_pack_dkh_host", _CCK, lambda cin, cout, k: k in (1, 3, 4)),   # plain weights as f16 piece pairs
    ("wpacked_t3h", True, "read_conv_t3h_floats", _CC, "read_conv_pack_t3h_host", _CC, lambda cin, cout, k: k == 3),             # 8 - 32 input channels
    ("wpacked_sc", True, "read_conv_sc_floats", _CC, "read_conv_pack_sc_host", _CC, lambda cin, cout, k: k == 3),                # Cout <= 4
)


class PackedGatedConv:
    """Weights of one BasicConv packed for the MFMA kernel and resident on the device."""

    def __init__(self, wf, bf, wm, bm, gamma, beta, mean, var, src_channels=None, eps=1e-5, device=None, kc=None):
        device = device if device is not None else _lib.require_gpu()
        f32 = lambda a: np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype=np.float32)
        wf, wm, bf, bm, gamma, beta, mean, var = map(f32, (wf, wm, bf, bm, gamma, beta, mean, var))
        self.cout, self.cin, self.k, _ = wf.shape
        self.kc = kc if kc is not None else kc_for(src_channels if src_channels is not None else [self.cin])
        L = _lib.lib()
        pp = np.empty(L.read_conv_param_floats(self.cout), np.float32)
        _lib.check(L.read_conv_pack_params_host(self.cout, bf.ctypes.data, bm.ctypes.data, gamma.ctypes.data,
                                                beta.ctypes.data, mean.ctypes.data, var.ctypes.data, eps,
                                                pp.ctypes.data), "read_conv_pack_params_host")
        self.params = torch.from_numpy(pp).to(device)
        dims = {"cin": self.cin, "cout": self.cout, "k": self.k, "kc": self.kc}
        for attr, _, size, size_args, packer, pack_args, carried in WEIGHT_ORDERS:
            n = getattr(L, size)(*(dims[a] for a in size_args)) if carried(self.cin, self.cout, self.k) else 0
            buf = np.empty(n, np.float32)
            if n:
                _lib.check(getattr(L, packer)(*(dims[a] for a in pack_args), wf.ctypes.data, wm.ctypes.data, buf.ctypes.data), packer)
            setattr(self, attr, torch.from_numpy(buf).to(device) if n else None)


def gated_conv(packed, sources, **kw):
    """One BasicConv launch (read_gated_conv_forward); arguments as conv_desc.  Returns the NHWC output (outH,outW,Cout)."""
    d, out = _desc(packed, sources, **kw)
    f4 = getattr(packed, "wpacked_f4x1", None)
    if f4 is not None:                 # the same launch with the F(4,3)-by-rows operand beside the descriptor (conv_f4x1 / config -12 decide)
        _lib.check(_lib.lib().read_gated_conv_forward_f4x1(C.byref(d), f4.data_ptr(), _lib.stream_ptr()), "read_gated_conv_forward_f4x1")
        return out
    _lib.check(_lib.lib().read_gated_conv_forward(C.byref(d), _lib.stream_ptr()), "read_gated_conv_forward")
    return out


def conv_desc(packed, sources, **kw):
    """The filled read_conv_desc of a launch (for read_conv_kernel_family and friends); the tensors it points at stay alive with it."""
    d, out = _desc(packed, sources, **kw)
    d._keep = (packed, sources, kw, out)
    return d


def _desc(packed, sources, stride=1, elu=True, mul=None, residual=None, config=-1, out=None,
          out_channels=None, fill=None, linear=False, pre=None):
    """sources: list of (NHWC tensor (h,w,C), shift).

    linear: plain convolution, output channels [conv_f + b_f | conv_m + b_m] (2*Cout).
    pre: (NHWC tensor, f_off, m_off, shift[, bilinear]) pre-activation addend sampled at (y >> shift, x >> shift), or — with
    bilinear = True and shift 2 — as nn.Upsample(x4, bilinear, align_corners=False) of the tensor (include/read_hip.h)."""
    t0, s0 = sources[0]
    inH = (t0.shape[0] >> s0) if s0 >= 0 else (t0.shape[0] << -s0)
    inW = (t0.shape[1] >> s0) if s0 >= 0 else (t0.shape[1] << -s0)
    pad = (packed.k - 1) // 2
    outH = (inH + 2 * pad - packed.k) // stride + 1
    outW = (inW + 2 * pad - packed.k) // stride + 1
    cs = out_channels if out_channels is not None else packed.cout * (2 if linear else 1)
    if out is None:
        out = torch.empty((outH, outW, cs), dtype=torch.float32, device=t0.device)
    d = _lib.ConvDesc()
    d.n_src = len(sources)
    for i, (t, sh) in enumerate(sources):
        assert t.is_contiguous() and t.dtype == torch.float32
        d.src[i].data = t.data_ptr()
        d.src[i].C = t.shape[2]
        d.src[i].srcH, d.src[i].srcW = t.shape[0], t.shape[1]
        d.src[i].shift = sh
    d.mul = mul.data_ptr() if mul is not None else None
    d.inH, d.inW = inH, inW
    d.Cout, d.ksize, d.stride = packed.cout, packed.k, stride
    d.elu = 1 if elu else 0
    d.params = packed.params.data_ptr()
    d.residual = residual.data_ptr() if residual is not None else None
    d.out, d.out_cstride = out.data_ptr(), cs
    d.fill_pad = 0 if fill is None else 1
    d.out_fill = 0.0 if fill is None else float(fill)
    d.config = config
    for attr, in_desc, *_ in WEIGHT_ORDERS:
        buf = getattr(packed, attr, None)
        if in_desc:
            setattr(d, attr, buf.data_ptr() if buf is not None else None)
    d.linear = 1 if linear else 0
    if pre is not None:
        pt, f_off, m_off, psh = pre[:4]
        d.pre_bilinear = 1 if (len(pre) > 4 and pre[4]) else 0
        assert pt.is_contiguous() and pt.dtype == torch.float32
        d.pre, d.pre_cstride, d.pre_f_off, d.pre_m_off, d.pre_shift = pt.data_ptr(), pt.shape[2], f_off, m_off, psh
        d.preH, d.preW = pt.shape[0], pt.shape[1]
    return d, out


def bilinear_up4(x):
    """NHWC (h,w,C) -> (4h,4w,C), align_corners=False (unet.py:200)."""
    h, w, c = x.shape
    out = torch.empty((4 * h, 4 * w, c), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().read_bilinear_up4(x.data_ptr(), h, w, c, out.data_ptr(), _lib.stream_ptr()),
               "read_bilinear_up4")
    return out


def config_names():
    L = _lib.lib()
    return [L.read_conv_config_name(i).decode() for i in range(L.read_conv_config_count())]
