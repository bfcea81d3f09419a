"""Native training step of READ's render path (BASELINE configs[4]).

What the reference gets from torch.autograd + cuDNN under ``src/train.py:132-203`` — backward of every ``BasicConv``
(READ/models/unet.py:22-53), of the ×4 bilinear upsample, of the descriptor lookup (READ/models/texture.py:61), the Huber
loss (src/READ/models/compose.py:35,38) and the descriptor optimizer (READ/pipelines/ogl.py:16,99-100) — runs here on the
HIP kernels of csrc/train.hip + csrc/conv.hip:

  GatedConvFn     forward  = MFMA convolution in linear mode (pre-activations f|m kept) + gate kernel
                  backward = gate backward (+ bias / BatchNorm-affine sums), dgrad (the same MFMA kernel over d[f|m] with
                             flipped, transposed weights; the six stride-2 layers as four stride-1 dgrads, one per pixel
                             parity), wgrad (3x3/s1: in the Winograd F(4x4,3x3) domain; the others direct MFMA)
  Up4Fn           bilinear x4 and its adjoint
  huber_loss      loss value + gradient in one launch
  SparseDescriptorRMSprop   RMSprop over the descriptor rows a step touched (the reference sweeps all N rows: 960 MB of
                             gradient + state at 30 M points every step)

Routing lives in ONE place: ``layer_route`` says which fragment orders a layer's launches read (forward, dgrad, polyphase),
``dgrad_method`` which dgrad runs it; both are pure.  ``_layer_jobs`` turns a route into the layer's packing jobs — the step's
``_PackPlan`` runs all of them in one launch, the per-layer path (``_packed_for`` / ``_pack_dgrad``) the same jobs one by one.

The graph around the convolutions (torch.cat, nearest resampling, FAM's product, residual adds) is expressed with torch
tensor ops on the device so that autograd does the bookkeeping of the 99-layer graph; every FLOP-carrying node is HIP.
BatchNorm: with the net in ``.eval()`` (configs/train_example.yaml ``eval_in_train: True``; train.py:271-277) it is the
eval-mode affine map with trainable gamma/beta; with the net in ``.train()`` (the reference's default, train.py:450) every
layer normalises with the statistics of the batch and moves its running buffers (``read_bn_train_forward`` /
``read_gate_backward_bn``), exactly what nn.BatchNorm2d does in the reference's BasicConv (unet.py:40,51).
"""
import ctypes as C
import os
import weakref
from typing import NamedTuple, Optional

import torch

from . import _lib

BN_EPS = 1e-5
BN_MOMENTUM = 0.1          # nn.BatchNorm2d default (unet.py:40)
BN_PER_ITEM = 2            # GatedConvFn's bn_train: 0 eval, 1 batch statistics over the stacked batch, 2 per stacked item


def _ptr(t):
    return t.data_ptr() if t is not None else None


# -----------------------------------------------------------------------------------------------------------------------
# One route per layer: which fragment orders its launches read, and which dgrad runs it
# -----------------------------------------------------------------------------------------------------------------------
class LayerRoute(NamedTuple):
    """What a layer's training launches read, decided ONCE from its shape and the module switches (layer_route).  Kinds are the
    packing kinds of read_pack_job (_lib.PACK_DIRECT / PACK_WINO / PACK_W4); ONE fragment order per layer, direction and step: the
    Winograd order where that kernel runs the launch (3x3 / stride 1), the direct order everywhere else — packing both cost 64 us
    per layer and step for fragments nobody read."""
    cin: int
    cout: int
    k: int
    stride: int
    fwd: int                 # forward fragments (the layer's own weights, mode 0) ...
    fwd_kc: int              # ... and the channel chunk of the direct order (16 with the Winograd orders)
    dgrad: Optional[int]     # dgrad fragments (flipped / transposed, mode 1); None: the dgrad is no convolution launch over them
    dgrad_kc: int
    poly: Optional[int]      # fragments of the four polyphase pseudo-layers (_poly_fragments); None: no polyphase dgrad


def layer_route(cin, cout, k, stride):
    """The route of a (cin -> cout, k x k, stride) layer under USE_WINOGRAD / USE_W4.  Pure: no library call, no tensor."""
    if cin % 8:
        raise ValueError(f"the HIP convolution needs input channels in multiples of 8 (got {cin})")

    def wino_kind(c_in, c_out):
        # F(4x4,3x3) for the layers that kernel takes in linear mode (csrc/conv.hip conv_uses_w4): at least two 16-channel chunks,
        # output channels in multiples of 8 (the dgrad of a 32-channel layer is a 64 -> 16 + 16 virtual layer: half a group; a
        # padded last group is masked); F(2x2,3x3) for the rest
        return _lib.PACK_W4 if USE_W4 and c_in % 16 == 0 and c_in >= 32 and c_out % 8 == 0 else _lib.PACK_WINO

    virtual = (2 * ((cout + 7) // 8 * 8), cin // 2)         # the dgrad's virtual layer: 2 * cp -> cin / 2 gated channels (always % 16)
    if USE_WINOGRAD and k == 3 and stride == 1 and cin % 16 == 0:
        fwd, fwd_kc = wino_kind(cin, cout), 16
    else:
        fwd, fwd_kc = _lib.PACK_DIRECT, 16 if cin % 16 == 0 else 8
    dgrad = None
    if stride == 1 or (stride == 2 and k == 3):              # 3x3 / stride 2: the stride-1 dgrad over the zero-dilated d[f|m]
        dgrad = wino_kind(*virtual) if USE_WINOGRAD and k == 3 else _lib.PACK_DIRECT   # the stride-1 dgrad of a 3x3 layer always runs on that kernel
    poly = wino_kind(*virtual) if USE_WINOGRAD and stride == 2 and k in (3, 4) and cin % 16 == 0 else None
    return LayerRoute(cin, cout, k, stride, fwd, fwd_kc, dgrad, 16, poly)


def dgrad_method(route, H, W, polyphase=None):
    """How the input gradient of a layer over an (H, W) input is computed (_dgrad runs it):
      'conv'     stride 1: the convolution kernel over d[f|m] with the layer's dgrad fragments
      'poly'     stride 2, even H and W: four 3x3 / stride-1 dgrads, one per pixel parity (_poly_fragments)
      'dilated'  3x3 / stride 2, even H and W: 'conv' over the zero-dilated d[f|m]
      'generic'  the vector kernel (read_conv_dgrad_generic)
    polyphase: POLYPHASE_DGRAD unless given.  Pure, like layer_route."""
    if route.stride == 1:
        return 'conv'
    even = H % 2 == 0 and W % 2 == 0
    if (POLYPHASE_DGRAD if polyphase is None else polyphase) and route.poly is not None and even:
        return 'poly'
    return 'dilated' if route.dgrad is not None and even else 'generic'


def _linear_conv(x, cin, wpacked, params, cout, k, stride, out, wino=None, gated=None, w4=False):
    """x (H,W,cin) NHWC -> out (Ho,Wo,2*cout): [conv_f + b_f | conv_m + b_m] through the MFMA kernel (linear epilogue);
    with Winograd fragments (3x3 / stride 1, cin % 16 == 0) through the Winograd F(2x2,3x3) kernel — which can store the
    layer's gated output in the same pass: gated = (y (Ho,Wo,cout), elu, block_h, valid_h)."""
    H, W = int(x.shape[0]), int(x.shape[1])
    d = _lib.ConvDesc()
    d.n_src = 1
    d.src[0].data = x.data_ptr()
    d.src[0].C, d.src[0].srcH, d.src[0].srcW, d.src[0].shift = cin, H, W, 0
    d.inH, d.inW, d.Cout, d.ksize, d.stride, d.elu = H, W, cout, k, stride, 0
    d.wpacked, d.params, d.out, d.out_cstride = wpacked.data_ptr(), params.data_ptr(), out.data_ptr(), 2 * cout
    d.config, d.linear = -1, 1
    if wino is not None:
        if w4:
            d.wpacked_w4 = wino.data_ptr()
        else:
            d.wpacked_wino = wino.data_ptr()
        if gated is not None:
            y, elu, bh, vh = gated
            d.out_gated, d.elu, d.block_h, d.valid_h = y.data_ptr(), int(elu), int(bh), int(vh)
    if FLOP_LOG is not None:                                 # bench.py: MFMA flops this launch EXECUTES (Winograd gains counted)
        pad = (k - 1) // 2
        Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        FLOP_LOG.append(("conv", 2.0 * Ho * Wo * cin * 2 * cout * k * k, int(_lib.lib().read_conv_kernel_family(C.byref(d)))))
    _lib.check(_lib.lib().read_gated_conv_forward(C.byref(d), _lib.stream_ptr()), "read_gated_conv_forward(linear)")
    return out


# bench.py sets this to a list for one instrumented step: (kind, direct-convolution flops of the launch as issued — padded /
# dilated operands included —, kernel family 4 = F(4x4,3x3) executes 1/4 of them, 2 = F(2x2,3x3) 1/2.25, 0 = all)
FLOP_LOG = None


# packed copies of a layer's weights, reused by every image of a batch (weights only change at optimizer steps, which bump
# the parameters' _version): key = id of the conv_f weight -> _PackEntry
_PACK_CACHE = {}
USE_W4 = True                # ... and through the F(4x4,3x3) kernel where its units fit (cin >= 32, cout % 8 == 0; layer_route)
USE_WINOGRAD = True          # 3x3 / stride-1 layers with cin % 16 == 0: forward pre-activations and dgrad through the Winograd kernel


WGRAD_SIDE_STREAM = os.environ.get("READ_AMD_WGRAD_SIDE", "1") != "0"   # weight gradients on a side stream, joined at the end of the backward pass
_SIDE = {}                   # device -> [streams, join queued for the running backward pass, layer counter]


WGRAD_STREAMS = max(1, int(os.environ.get("READ_AMD_WGRAD_STREAMS", "1")))     # side streams the layers' weight gradients rotate over


def _side_stream(dev):
    """The side stream of the NEXT layer's weight gradient (round robin over WGRAD_STREAMS streams)."""
    e = _SIDE.get(dev)
    if e is None:
        e = _SIDE[dev] = [[torch.cuda.Stream(dev) for _ in range(WGRAD_STREAMS)], False, 0]
    e[2] += 1
    return e[0][e[2] % len(e[0])]


def _queue_join(dev):
    e = _SIDE[dev]
    if e[1]:
        return
    e[1] = True

    def join():
        e[1] = False
        cur = torch.cuda.current_stream(dev)
        for st_ in e[0]:
            cur.wait_stream(st_)
    torch.autograd.Variable._execution_engine.queue_callback(join)


_ZERO_PARAMS = {}


def _bump_version(*tensors):
    inc = getattr(torch._C, '_increment_version', None)
    if inc is not None:
        inc(list(tensors))
    else:
        for t in tensors:
            t.add_(0)


_CONST_VECS = {}


def _const_vec(n, value, dev):
    v = _CONST_VECS.get((n, value, dev))
    if v is None:
        v = _CONST_VECS[(n, value, dev)] = torch.full((n,), value, dtype=torch.float32, device=dev)
    return v


def _zero_params(n, dev):
    """An all-zero parameter block (bias / scale / shift of the dgrad's virtual layer): read-only, one per size and device."""
    z = _ZERO_PARAMS.get((n, dev))
    if z is None:
        z = _ZERO_PARAMS[(n, dev)] = torch.zeros(n, dtype=torch.float32, device=dev)
    return z


def _pack_version(route, ts, identity_bn):
    wf, bf, wm, bm = ts[:4]
    if identity_bn:
        return tuple(t._version for t in (wf, bf, wm, bm)) + (wf.data_ptr(), wm.data_ptr(), 'identity', route)
    return tuple(t._version for t in ts) + (wf.data_ptr(), wm.data_ptr(), route)


class _PackEntry:
    """The packed copies of ONE layer: what _PACK_CACHE holds, what a GatedConvFn node keeps (ctx.pack), what the pack plan fills."""
    __slots__ = ("version", "route", "params", "fwd", "dgrad", "dgrad_event", "event", "ref")

    def __init__(self, version=None, route=None, params=None, fwd=None, dgrad=None, event=None):
        self.version, self.route = version, route           # _pack_version of the tensors packed; LayerRoute
        self.params, self.fwd = params, fwd                 # parameter block; forward fragments in the order route.fwd
        self.dgrad, self.dgrad_event = dgrad, None          # dgrad fragments in the order route.dgrad (None: not packed) + their event
        self.event = event                                  # params / fwd are packed; None: by the step's pack plan
        self.ref = None                                     # weakref of the conv_f weight the cache key is the id of (_cache_put)

    @property
    def wino(self):          # the forward fragments where they are in a Winograd order (read_conv_desc.wpacked_wino / _w4), else None
        return self.fwd if self.route.fwd != _lib.PACK_DIRECT else None


def _cache_put(wf, entry):
    """entry becomes the cache entry of the parameter wf and dies with it: ONE finalizer per parameter object, however many
    versions of it pass through the cache."""
    key = id(wf)
    old = _PACK_CACHE.get(key)
    if old is not None and old.ref() is wf:
        entry.ref = old.ref                                   # same parameter, new version: keep its finalizer's handle
    else:
        entry.ref = weakref.ref(wf)
        weakref.finalize(wf, _drop_pack, key, entry.ref)      # the entry dies with its parameter
    _PACK_CACHE[key] = entry


def _drop_pack(key, ref):
    e = _PACK_CACHE.get(key)
    if e is not None and e.ref is ref:
        del _PACK_CACHE[key]


# -----------------------------------------------------------------------------------------------------------------------
# One job builder: a layer's packing jobs, for the step's one batch launch and for the per-layer launches alike
# -----------------------------------------------------------------------------------------------------------------------
_FRAGMENT_FLOATS = {(_lib.PACK_DIRECT, 0): "read_conv_packed_floats", (_lib.PACK_DIRECT, 1): "read_conv_dgrad_packed_floats",
                    (_lib.PACK_WINO, 0): "read_conv_wino_floats", (_lib.PACK_WINO, 1): "read_conv_dgrad_wino_floats",
                    (_lib.PACK_W4, 0): "read_conv_w4_floats", (_lib.PACK_W4, 1): "read_conv_dgrad_w4_floats"}


def _fragment_floats(kind, mode, cin, cout, k):
    size = getattr(_lib.lib(), _FRAGMENT_FLOATS[(kind, mode)])
    return size(cin, cout, k) if kind == _lib.PACK_DIRECT else size(cin, cout)


def _job(kind, mode, cin, cout, k, kc, out, wf=None, wm=None, par=None, eps=BN_EPS):
    """One validated read_pack_job (include/read_hip.h) writing `out`; par = (bf, bm, gamma, beta, mean, var) of a params job."""
    j = _lib.PackJob()
    j.kind, j.mode, j.Cin, j.Cout, j.ksize, j.kc, j.eps = kind, mode, cin, cout, k, kc, eps
    j.out = out.data_ptr()
    if wf is not None:
        j.wf, j.wm = wf.data_ptr(), wm.data_ptr()
    if par is not None:
        j.bf, j.bm, j.gamma, j.beta, j.mean, j.var = (_ptr(t) for t in par)
    _lib.check(_lib.lib().read_conv_pack_job_prepare(C.byref(j)), "read_conv_pack_job_prepare")
    return j


def _layer_jobs(route, wf, wm, ts=None, identity_bn=False, fwd=True, dgrad=True):
    """The packing jobs of one layer with the tensors they fill, in the order params, fwd, dgrad: {name: (PackJob, out)}.
    wf, wm: the contiguous weights; ts: the layer's eight tensors for the parameter block (None: no params job).
    identity_bn (batch-statistics mode): the params block carries the two biases and scale 1 / shift 0 — the launch then
    stores g = act(f) * sigmoid(m) itself and read_bn_train_forward normalises it."""
    dev = wf.device
    cin, cout, k = route.cin, route.cout, route.k
    jobs = {}
    if ts is not None:
        _wf, bf, _wm, bm, gamma, beta, mean, var = ts
        eps = BN_EPS
        if identity_bn:
            one, zero = _const_vec(cout, 1.0, dev), _const_vec(cout, 0.0, dev)
            gamma, beta, mean, var, eps = one, zero, zero, one, 0.0       # scale = 1 / sqrt(1 + 0)
        out = torch.empty(_lib.lib().read_conv_param_floats(cout), dtype=torch.float32, device=dev)
        jobs['params'] = (_job(_lib.PACK_PARAMS, 0, cin, cout, k, 0, out, par=(bf, bm, gamma, beta, mean, var), eps=eps), out)
    for name, want, kind, kc in (('fwd', fwd, route.fwd, route.fwd_kc), ('dgrad', dgrad, route.dgrad, route.dgrad_kc)):
        if want and kind is not None:
            mode = int(name == 'dgrad')
            out = torch.empty(_fragment_floats(kind, mode, cin, cout, k), dtype=torch.float32, device=dev)
            jobs[name] = (_job(kind, mode, cin, cout, k, kc, out, wf, wm), out)
    return jobs


def _launch_jobs(jobs):
    """One launch per job on the current stream: the path of a standalone GatedConvFn and of weights the step's plan does not take."""
    L, st = _lib.lib(), _lib.stream_ptr()
    for j in jobs:
        _lib.check(L.read_conv_pack_job(C.byref(j), st), "read_conv_pack_job")


def _packed_for(route, ts, identity_bn=False):
    """The layer's entry with the parameter block and the forward fragments of its CURRENT tensors ts = (wf, bf, wm, bm, gamma, beta,
    running mean, running var), from the cache or packed now."""
    wf, wm = ts[0], ts[2]
    ver = _pack_version(route, ts, identity_bn)
    hit = _PACK_CACHE.get(id(wf))
    if hit is not None and hit.ref() is not wf:             # the id was recycled by another tensor: not this layer's entry
        hit = None
    if hit is not None and hit.version == ver:
        if hit.event is not None:                           # None: the step's pack plan filled it on this stream, into buffers it keeps
            cur = torch.cuda.current_stream()
            cur.wait_event(hit.event)                       # packed on another item's stream
            hit.params.record_stream(cur)
            hit.fwd.record_stream(cur)
        return hit
    jobs = _layer_jobs(route, wf.detach().contiguous(), wm.detach().contiguous(), ts, identity_bn, dgrad=False)
    _launch_jobs(j for j, _out in jobs.values())
    ev = torch.cuda.Event()
    ev.record()
    entry = _PackEntry(ver, route, jobs['params'][1], jobs['fwd'][1], event=ev)
    _cache_put(wf, entry)
    return entry


def _pack_dgrad(entry, wf, wm):
    """Flipped / transposed fragments of the layer for its dgrad (direct or, for 3x3, Winograd) on the current stream."""
    jobs = _layer_jobs(entry.route, wf.detach().contiguous(), wm.detach().contiguous(), fwd=False)
    _launch_jobs(j for j, _out in jobs.values())
    ev = torch.cuda.Event()
    ev.record()
    entry.dgrad, entry.dgrad_event = jobs['dgrad'][1], ev


# -----------------------------------------------------------------------------------------------------------------------
# dgrad of the 4x4 / stride-2 layers (feat_extract.7 / .3 / .4, READ/models/unet.py:198-200) on the Winograd kernel
# -----------------------------------------------------------------------------------------------------------------------
# y[o] = sum_a W[a] x[2 o + a - 1]  =>  dx[2 u + p] = sum_{t in 0..2} K_p[t] dy[u + t - 1] with K_0 = [W3, W1, 0], K_1 = [0, W2, W0]
# (per axis): each of the four pixel parities of dx is a 3x3 / stride-1 correlation over the HALF-resolution d[f|m] — i.e. the
# stride-1 dgrad of a 3x3 pseudo-layer whose weights are Wp = [0, W1, W3] (even positions) / [W0, W2, 0] (odd positions) along
# each axis.  Four launches of the F(4x4,3x3) kernel on a quarter of the pixels replace the generic vector kernel (690 us per
# layer, three layers on the critical path of the backward pass).
POLYPHASE_DGRAD = os.environ.get("READ_AMD_POLYPHASE", "1") != "0"
_POLY = {}                   # id(conv_f weight) -> _PolyEntry
_POLY_SEL = {}               # device -> index tensors of the four parities


class _PolyEntry(NamedTuple):
    version: tuple
    frags: torch.Tensor      # [4][n]: the fragments of the four pseudo-layers, parity 2 py + px
    event: torch.cuda.Event
    stream: int              # the stream they were packed on


def _poly_fragments(wf, wm, route):
    """-> fragments [4][n] in the order route.poly, one row per pixel parity.
    k = 3 (stride 2, pad 1) the same way: dx[2 u] = W1 dy[u], dx[2 u + 1] = W2 dy[u] + W0 dy[u + 1] — pseudo-weights
    [0, W1, 0] / [W0, W2, 0]; instead of the stride-1 dgrad over a zero-dilated d[f|m] (4x the pixels, 3/4 of them zeros)."""
    cin, cout, k = route.cin, route.cout, route.k
    key = id(wf)
    ver = (wf._version, wm._version, wf.data_ptr(), wm.data_ptr(), route)
    hit = _POLY.get(key)
    if hit is not None and hit.version == ver:
        cur = torch.cuda.current_stream(wf.device)
        if hit.stream != cur.cuda_stream:                         # packed on another stream (a caller that runs its steps on several)
            cur.wait_event(hit.event)
            hit.frags.record_stream(cur)
        return hit.frags
    dev = wf.device
    sel = _POLY_SEL.get((dev, k))
    if sel is None:                                                            # parity -> source tap of the pseudo taps (k: the zero tap)
        taps = torch.tensor([[4, 1, 3], [0, 2, 4]] if k == 4 else [[3, 1, 3], [0, 2, 3]], device=dev)
        sel = _POLY_SEL[(dev, k)] = (taps[[0, 0, 1, 1]][:, :, None], taps[[0, 1, 0, 1]][:, None, :])
    w5 = torch.nn.functional.pad(torch.stack((wf.detach(), wm.detach())), (0, 1, 0, 1))      # (2, cout, cin, k + 1, k + 1)
    wp = w5[:, :, :, sel[0], sel[1]].permute(3, 0, 1, 2, 4, 5).contiguous()                    # (parity 2 py + px, f|m, cout, cin, 3, 3)
    buf = torch.empty((4, _fragment_floats(route.poly, 1, cin, cout, 3)), dtype=torch.float32, device=dev)
    # the dgrad jobs of four 3x3 pseudo-layers, one launch each
    _launch_jobs(_job(route.poly, 1, cin, cout, 3, route.dgrad_kc, buf[par], wp[par, 0], wp[par, 1]) for par in range(4))
    ev = torch.cuda.Event()
    ev.record()
    if key not in _POLY:
        weakref.finalize(wf, _POLY.pop, key, None)
    _POLY[key] = _PolyEntry(ver, buf, ev, torch.cuda.current_stream(dev).cuda_stream)
    return buf


# -----------------------------------------------------------------------------------------------------------------------
# Every packing job of a step in one launch
# -----------------------------------------------------------------------------------------------------------------------
# The optimizer changes every weight every step, so a step re-packs the parameter block, the forward fragments and the dgrad
# fragments of all 99 layers.  Layer by layer that was 297 launches of 2 .. 5 us kernels per step, each with its allocation, its
# event and its record_stream calls on the host and ~8 us of launch gap on the device (bench.py, round 4 before the wgrad work: ~1200 launches per step).  The net's tensors keep their addresses across optimizer steps, so the jobs are tabulated
# ONCE per (net, BatchNorm mode) — outputs in buffers the plan keeps — and a step is one read_conv_pack_batch launch at the head of
# the forward pass; the per-layer cache then hits for every layer.
PACK_BATCH = os.environ.get("READ_AMD_PACK_BATCH", "1") != "0"


class _NotBatchPackable(Exception):
    pass


class _PackPlan:
    """Assumptions a caller may rely on: (1) the fragments are packed on the stream of the refresh() that saw the weights change; a
    forward on ANOTHER stream waits for that launch (the event below) even when its own refresh() returns early; (2) the buffers are
    overwritten in place by the next refresh, so a backward pass uses the fragments of the weights AS THEY ARE when it runs —
    i.e. between a forward and its backward the weights must not be stepped (the usual order: backward, then optimizer.step())."""

    def __init__(self, net, identity_bn):
        from .unet import layer_table
        dev = next(net.parameters()).device
        self.identity_bn = bool(identity_bn)
        self.layers = []            # (tensors of the layer, its _PackEntry: the buffers the jobs fill)
        self.jobs = []              # (layer path, PackJob) in table order
        for (path, cin, cout, k, stride, _elu) in layer_table():
            if path.startswith("ConvsOut."):                 # in the state dict, never executed (unet.py:181-186)
                continue
            node = net
            for p_ in path.split('.'):
                node = node._modules[p_]
            b = node.block
            n = b['norm']
            ts = (b['conv_f'].weight, b['conv_f'].bias, b['conv_m'].weight, b['conv_m'].bias, n.weight, n.bias, n.running_mean,
                  n.running_var)
            if not (ts[0].is_contiguous() and ts[2].is_contiguous()):
                raise _NotBatchPackable("non-contiguous weights")
            route = layer_route(cin, cout, k, stride)
            jobs = _layer_jobs(route, ts[0], ts[2], ts, self.identity_bn)
            out = {name: o for name, (_j, o) in jobs.items()}
            self.layers.append((ts, _PackEntry(None, route, out['params'], out['fwd'], out.get('dgrad'))))
            self.jobs += [(path, j) for j, _o in jobs.values()]
        first = 0
        for _path, j in self.jobs:
            j.first_block = first
            first += j.nblocks
        self.total_blocks, self.njobs = first, len(self.jobs)
        table = (_lib.PackJob * self.njobs)(*(j for _path, j in self.jobs))
        self.table = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
        self.signature = None
        self.stream = self.event = None

    def refresh(self):
        """Pack every layer with its current weights — one launch — unless nothing changed since the last one."""
        sig = tuple(t._version for ts, _entry in self.layers for t in ts)
        cur = torch.cuda.current_stream()
        if sig == self.signature:
            if cur != self.stream:
                cur.wait_event(self.event)                # packed on another stream: order this one behind that launch
            return
        _lib.check(_lib.lib().read_conv_pack_batch(self.table.data_ptr(), self.njobs, self.total_blocks, _lib.stream_ptr()),
                   "read_conv_pack_batch")
        self.signature = sig
        self.stream, self.event = cur, torch.cuda.Event()
        self.event.record(cur)
        for ts, entry in self.layers:                     # the per-layer cache then hits for every layer (entry.event stays None)
            entry.version = _pack_version(entry.route, ts, self.identity_bn)
            _cache_put(ts[0], entry)


def _net_tensors(net):
    """The net's parameters and buffers, listed once: their addresses key what is built per net (the pack plans)."""
    ts = net.__dict__.get('_flat_tensors')
    if ts is None:
        ts = net.__dict__['_flat_tensors'] = list(net.parameters()) + list(net.buffers())
    return ts


def _pack_plan(net, identity_bn):
    """The net's plan for this BatchNorm mode; rebuilt when a tensor has moved (.cuda() / .to() / a new parameter object)."""
    key = (bool(identity_bn), hash(tuple(t.data_ptr() for t in _net_tensors(net))), USE_W4, USE_WINOGRAD)
    plans = net.__dict__.setdefault('_pack_plans', {})
    if key in plans:
        return plans[key]
    if len(plans) >= 4:
        plans.clear()
    try:
        plan = _PackPlan(net, identity_bn)
    except _NotBatchPackable:
        plan = None                # e.g. channels_last weights: every layer packs itself (_packed_for calls .contiguous())
    plans[key] = plan
    return plan


class _GradArena:
    """The bias / BatchNorm-parameter gradients of every layer of ONE step live in one tensor, zero-filled by ONE launch when the
    step's first backward node asks for its slice (read_bn_param_grads accumulates): 99 `torch.zeros((4, cout))` per step otherwise."""

    def __init__(self):
        self.size, self.buf, self.taken = 0, None, set()

    def reserve(self, n):
        off = self.size
        self.size += (n + 63) // 64 * 64                    # 256-byte slices
        return off

    def take(self, off, n, dev):
        if off in self.taken:                               # a second backward over the same graph (retain_graph): fresh zeros
            return torch.zeros(n, dtype=torch.float32, device=dev)
        self.taken.add(off)
        if self.buf is None:
            self.buf = torch.zeros(self.size, dtype=torch.float32, device=dev)
        return self.buf[off:off + n]


def _dgrad(method, route, dfm, H, W, wf, wm, entry=None, live=None, out=None):
    """d[f|m] (Ho, Wo, 2 * pad8(cout)) -> dx (H, W, cin) by `method` (dgrad_method): the input gradient of GatedConvFn.backward, and
    what tests/test_gpu_train_accuracy.py drives method by method.  wf, wm: the contiguous weights; entry: the layer's _PackEntry —
    its dgrad fragments are packed here when nobody has yet; live: the parameter objects the polyphase fragments are cached under
    (wf, wm themselves when not given); out: write dx here."""
    L = _lib.lib()
    dev = dfm.device
    cin, cout, k = route.cin, route.cout, route.k
    Ho, Wo = int(dfm.shape[0]), int(dfm.shape[1])
    cp = (cout + 7) // 8 * 8
    dx = out if out is not None else torch.empty((H, W, cin), dtype=torch.float32, device=dev)
    if method == 'poly':
        # four 3x3 / stride-1 dgrads over the half-resolution d[f|m], one per pixel parity of dx (_poly_fragments)
        frags = _poly_fragments(*(live or (wf, wm)), route)            # of the CURRENT weights (cache: packed in forward)
        zero = _zero_params(L.read_conv_param_floats(cin // 2), dev)
        for par in range(4):
            dxp = torch.empty((Ho, Wo, cin), dtype=torch.float32, device=dev)
            _linear_conv(dfm, 2 * cp, frags[par], zero, cin // 2, 3, 1, dxp, wino=frags[par], w4=route.poly == _lib.PACK_W4)
            dx[par >> 1::2, par & 1::2] = dxp
    elif method in ('conv', 'dilated'):
        # dgrad = the same MFMA convolution over d[f|m] with flipped, transposed weights; the two "gate halves" of
        # the kernel's output tile are simply the two halves of the input channels.  A 3x3 / stride-2 layer is the
        # stride-1 layer sampled at the even positions, so its dgrad is the stride-1 dgrad of d[f|m] spread onto the
        # even positions of a zero image — 4x the necessary MFMAs, still 7x faster than the generic VALU kernel
        # (1.34 ms per layer) because it runs on the Winograd kernel.
        d_in = dfm
        if method == 'dilated':
            d_in = torch.zeros((H, W, 2 * cp), dtype=torch.float32, device=dev)
            d_in[::2, ::2] = dfm
        if entry is None:
            entry = _PackEntry(route=route)
        if entry.dgrad is None:
            _pack_dgrad(entry, wf, wm)
        wd, ev = entry.dgrad, entry.dgrad_event
        wdw = wd if route.dgrad != _lib.PACK_DIRECT else None
        if ev is not None:                   # None: packed by the step's pack plan, whose refresh() ordered this stream behind it
            torch.cuda.current_stream().wait_event(ev)
            wd.record_stream(torch.cuda.current_stream())
        zero = _zero_params(L.read_conv_param_floats(cin // 2), dev)
        _linear_conv(d_in, 2 * cp, wd, zero, cin // 2, k, 1, dx, wino=wdw, w4=route.dgrad == _lib.PACK_W4)
    else:
        if FLOP_LOG is not None:
            FLOP_LOG.append(("dgrad_valu", 2.0 * Ho * Wo * cin * 2 * cout * k * k, 0))
        ws = torch.empty(L.read_conv_dgrad_generic_floats(cin, cout, k), dtype=torch.float32, device=dev)
        _lib.check(L.read_conv_dgrad_generic(dfm.data_ptr(), Ho, Wo, cin, cout, k, route.stride, wf.data_ptr(), wm.data_ptr(),
                                             ws.data_ptr(), H, W, dx.data_ptr(), _lib.stream_ptr()))
    return dx


class GatedConvFn(torch.autograd.Function):
    """y = BN_eval(act(conv_f(x) + b_f) * sigmoid(conv_m(x) + b_m)) for ONE image, x (H,W,Cin) NHWC -> (Ho,Wo,Cout)."""

    @staticmethod
    def forward(ctx, x, wf, bf, wm, bm, gamma, beta, mean, var, k, stride, elu, nb=1, v_num=1, v_den=1, bn_train=False, arena=None):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("read_amd.train: the training nodes cache packed weights and record events, so they cannot be captured "
                               "into a HIP graph — a replay would run on the weights of the capture step")
        L = _lib.lib()
        st = _lib.stream_ptr()
        x = x.contiguous()
        H, W, cin = (int(v) for v in x.shape)
        cout = int(wf.shape[0])
        pad = (k - 1) // 2
        Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        dev = x.device
        wf_c, wm_c = wf.detach().contiguous(), wm.detach().contiguous()
        route = layer_route(cin, cout, k, stride)
        entry = _packed_for(route, (wf, bf, wm, bm, gamma, beta, mean, var), identity_bn=bn_train)
        params, wp = entry.params, entry.fwd
        ctx.pack, ctx.route = entry, route
        # stride-2 layers: dgrad as four stride-1 dgrads, one per pixel parity (_poly_fragments)
        ctx.method = method = dgrad_method(route, H, W)
        ctx.side = WGRAD_SIDE_STREAM
        # the dgrad's fragments too, now: in the backward pass the wgrad kernels of the layers above fill the chip from their side
        # stream and a small packing launch between two dgrads waits 200 us for its turn (10 us here)
        if x.requires_grad:
            if method in ('conv', 'dilated') and entry.dgrad is None:
                _pack_dgrad(entry, wf, wm)
            elif method == 'poly':
                _poly_fragments(wf, wm, route)
        side = _SIDE.get(dev)
        if side is not None:
            side[1] = False          # a backward pass that died before its join callback ran must not mute the next one's
        fm = torch.empty((Ho, Wo, 2 * cout), dtype=torch.float32, device=dev)
        y = torch.empty((Ho, Wo, cout), dtype=torch.float32, device=dev)
        # a batch is one tall image of nb stacked items; separator rows (block geometry at THIS layer's output scale) stay zero
        bh = Ho // nb if nb > 1 else 0
        vh = bh * v_num // v_den
        wino = entry.wino
        # the Winograd kernel writes the gated output next to the pre-activations; the other kernels leave it to the gate pass
        _linear_conv(x, cin, wp, params, cout, k, stride, fm, wino=wino, gated=(y, elu, bh, vh), w4=route.fwd == _lib.PACK_W4)
        if wino is None:
            _lib.check(L.read_gate_forward(fm.data_ptr(), Ho * Wo, cout, params.data_ptr(), int(elu), None, y.data_ptr(), Wo, bh, vh, st))
        stat, groups = None, 1
        if bn_train:
            # y holds g = act(f) * sigmoid(m) so far: normalise it with the batch statistics, in place; the module's running
            # buffers (mean, var ARE the buffers) move as nn.BatchNorm2d's do — no autograd through them.
            # bn_train == 2 (BN_PER_ITEM): every stacked item is its own BatchNorm batch (the net called once per item,
            # READ/models/compose.py:137-176) — per-item statistics, the buffers move nb times in item order
            groups = nb if (int(bn_train) == BN_PER_ITEM and nb > 1) else 1
            stat = torch.empty((groups, 2, cout), dtype=torch.float32, device=dev)
            scale_shift = torch.empty((groups, 2, (cout + 31) // 32 * 32), dtype=torch.float32, device=dev)
            scratch = torch.empty(groups * 2 * cout, dtype=torch.float64, device=dev)
            _lib.check(L.read_bn_train_forward(y.data_ptr(), Ho * Wo, cout, Wo, bh, vh, groups, gamma.detach().data_ptr(),
                                               beta.detach().data_ptr(), BN_EPS, BN_MOMENTUM, mean.data_ptr(), var.data_ptr(),
                                               stat.data_ptr(), scale_shift.data_ptr(), scratch.data_ptr(), st), "read_bn_train_forward")
            _bump_version(mean, var)                 # written through raw pointers: caches keyed on ._version must see it
            mean = var = stat                        # the backward pass needs the groups' {mean, biased var}, not the buffers
        ctx.bn_train = bool(bn_train)
        ctx.bn_groups = groups
        ctx.arena = (arena, arena.reserve(8 * cout)) if arena is not None else None      # eval mode: sums + gradients; .train(): gradients
        # the weights ride on the context, not in save_for_backward: the backward's dgrad reads the packed fragments, which hold the
        # weights as they are when it runs (_PackPlan, assumption 2), and the generic dgrad reads wf / wm the same way.  Saved tensors
        # are version-checked: a backward walked after an in-place update of a parameter (retain_graph across an optimizer step)
        # would raise "modified by an inplace operation" for these two tensors alone
        ctx.weights = (wf_c, wm_c, gamma.detach() if bn_train else None, mean, var)      # mean / var: running buffers or batch statistics
        ctx.save_for_backward(x, fm, params)
        ctx.cfg = (k, stride, int(elu), H, W, cin, cout, Ho, Wo, bh, vh)
        ctx.wrefs = (weakref.ref(wf), weakref.ref(wm))
        return y

    @staticmethod
    def backward(ctx, dy):
        L = _lib.lib()
        st = _lib.stream_ptr()
        x, fm, params = ctx.saved_tensors
        wf, wm, gamma_d, mean, var = ctx.weights
        k, stride, elu, H, W, cin, cout, Ho, Wo, bh, vh = ctx.cfg
        dev = x.device
        dy = dy.contiguous()
        cp = (cout + 7) // 8 * 8
        dfm = torch.empty((Ho, Wo, 2 * cp), dtype=torch.float32, device=dev)
        groups = ctx.bn_groups
        # eval-mode BatchNorm: sums[4][cout] and the four parameter-gradient rows are one zero-filled slice [8][cout] — of the step's
        # arena (ONE fill for all layers) or of a tensor of its own; read_gate_backward / read_bn_param_grads accumulate into it
        zeroed = None
        if not ctx.bn_train:
            zeroed = (ctx.arena[0].take(ctx.arena[1], 8 * cout, dev) if ctx.arena is not None
                      else torch.zeros(8 * cout, dtype=torch.float32, device=dev)).view(8, cout)
        sums = zeroed[:4] if zeroed is not None else torch.empty((groups, 4, cout), dtype=torch.float32, device=dev)
        if ctx.bn_train:
            stat = mean                                               # [groups][2][cout]: batch mean / biased variance of the forward pass
            abc = torch.empty((groups, 3, cout), dtype=torch.float32, device=dev)
            _lib.check(L.read_gate_backward_bn(dy.data_ptr(), fm.data_ptr(), Ho * Wo, cout, params.data_ptr(), elu, dfm.data_ptr(),
                                               sums.data_ptr(), Wo, bh, vh, groups, stat.data_ptr(), gamma_d.data_ptr(), BN_EPS,
                                               abc.data_ptr(), st), "read_gate_backward_bn")
        else:
            _lib.check(L.read_gate_backward(dy.data_ptr(), fm.data_ptr(), Ho * Wo, cout, params.data_ptr(), elu, dfm.data_ptr(),
                                            sums.data_ptr(), Wo, bh, vh, st))
        # The side stream's outputs are allocated BEFORE the event it waits for: a block the caching allocator hands out here was
        # freed by main-stream work that precedes the event.  Allocated after the dgrad below, dwf could be the block of a dgrad
        # temporary whose kernels are still queued on the main stream — the wgrad, ordered only behind ev_dfm, then wrote into memory
        # the main stream was still using (seen as a garbage dW_f of feat_extract.7 once the dgrad had freed tensors of that size).
        want_w = ctx.needs_input_grad[1] or ctx.needs_input_grad[3]
        dwf = dwm = scratch = None
        if want_w:
            dwf, dwm = torch.empty_like(wf), torch.empty_like(wm)
            n_scr = L.read_conv_wgrad_scratch_floats(cin, cout, k, Ho)
            scratch = torch.empty(n_scr, dtype=torch.float32, device=dev)
        ev_dfm = None
        if ctx.side:
            ev_dfm = torch.cuda.Event()
            ev_dfm.record(torch.cuda.current_stream(dev))              # d[f|m] (and everything before it) is complete here
        if zeroed is not None:
            dbf, dbm, dgamma, dbeta = zeroed[4:].unbind(0)
        elif ctx.arena is not None:                     # the step's ONE zero-filled tensor for every layer's bias / BatchNorm gradients
            dbf, dbm, dgamma, dbeta = ctx.arena[0].take(ctx.arena[1], 4 * cout, dev).view(4, cout).unbind(0)
        else:
            dbf, dbm, dgamma, dbeta = torch.zeros((4, cout), dtype=torch.float32, device=dev).unbind(0)     # one fill, four rows
        if ctx.bn_train:
            _lib.check(L.read_bn_param_grads_groups(cout, groups, sums.data_ptr(), stat.data_ptr(), BN_EPS, dbf.data_ptr(),
                                                    dbm.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), st))
        else:
            _lib.check(L.read_bn_param_grads(cout, sums.data_ptr(), mean.data_ptr(), var.data_ptr(), BN_EPS, dbf.data_ptr(),
                                             dbm.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), st))
        dx = None
        if ctx.needs_input_grad[0]:
            method, live = ctx.method, (ctx.wrefs[0](), ctx.wrefs[1]())
            if method == 'poly' and (live[0] is None or live[1] is None):      # the parameters are gone: from the weights the context holds
                method = dgrad_method(ctx.route, H, W, polyphase=False)
            dx = _dgrad(method, ctx.route, dfm, H, W, wf, wm, ctx.pack, live)
        if not want_w:                                                      # frozen net: nobody asked for weight gradients
            return dx, None, dbf, None, dbm, dgamma, dbeta, None, None, None, None, None, None, None, None, None, None
        if FLOP_LOG is not None:
            FLOP_LOG.append(("wgrad", 2.0 * Ho * Wo * cin * 2 * cout * k * k, int(L.read_conv_wgrad_family(cin, k, stride, H, W))))
        if ctx.side:
            # nothing downstream of this layer needs its weight gradient before the optimizer step, so it is computed on a
            # side stream while the main stream goes on with the dgrad chain of the layers below; the end of the backward
            # pass joins the streams (_join_side_stream, queued once per pass on the autograd engine)
            main, side = torch.cuda.current_stream(dev), _side_stream(dev)
            side.wait_event(ev_dfm)
            with torch.cuda.stream(side):
                _lib.check(L.read_conv_wgrad(x.data_ptr(), H, W, cin, dfm.data_ptr(), cout, k, stride, dwf.data_ptr(), dwm.data_ptr(),
                                             0, scratch.data_ptr(), n_scr, _lib.stream_ptr()))
            for t in (x, dfm, dwf, dwm, scratch):
                t.record_stream(side)
            # Returning dwf / dwm before the side stream has produced them is only safe when AccumulateGrad STEALS the
            # tensors (``.grad`` is None, no hooks): otherwise ``grad += dwf`` runs on the main stream right away — gradient
            # accumulation over several backward() calls, zero_grad(set_to_none=False), a layer used twice in one graph, a
            # tensor hook.  Then the main stream waits for this layer's wgrad here.
            stealable = True
            for r in ctx.wrefs:
                p = r()
                if p is None or p.grad is not None or getattr(p, '_backward_hooks', None) or getattr(p, '_post_accumulate_grad_hooks', None):
                    stealable = False
            if stealable:
                _queue_join(dev)
            else:
                ev_w = torch.cuda.Event()
                ev_w.record(side)
                main.wait_event(ev_w)
        else:
            _lib.check(L.read_conv_wgrad(x.data_ptr(), H, W, cin, dfm.data_ptr(), cout, k, stride, dwf.data_ptr(), dwm.data_ptr(), 0,
                                         scratch.data_ptr(), n_scr, st))
        return dx, dwf, dbf, dwm, dbm, dgamma, dbeta, None, None, None, None, None, None, None, None, None, None


class Up4Fn(torch.autograd.Function):
    """nn.Upsample(scale_factor=4, mode='bilinear') (unet.py:200) on an (H,W,C) NHWC image — or on nb vertically stacked
    items, each interpolated on its own — and its adjoint."""

    @staticmethod
    def forward(ctx, x, nb=1, v_num=1, v_den=1):
        x = x.contiguous()
        H, W, c = (int(v) for v in x.shape)
        bh = H // nb if nb > 1 else 0
        vh = bh * v_num // v_den
        out = torch.empty((4 * H, 4 * W, c), dtype=torch.float32, device=x.device)
        _lib.check(_lib.lib().read_bilinear_up4_blocks(x.data_ptr(), H, W, c, out.data_ptr(), bh, vh, _lib.stream_ptr()))
        ctx.shape = (H, W, c, bh, vh)
        return out

    @staticmethod
    def backward(ctx, dout):
        H, W, c, bh, vh = ctx.shape
        dout = dout.contiguous()
        din = torch.empty((H, W, c), dtype=torch.float32, device=dout.device)
        _lib.check(_lib.lib().read_bilinear_up4_backward(dout.data_ptr(), H, W, c, din.data_ptr(), bh, vh, _lib.stream_ptr()))
        return din, None, None, None


class _HuberFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, out, target):
        out, target = out.contiguous(), target.contiguous().to(out.device, torch.float32)
        n = out.numel()
        loss = torch.empty(1, dtype=torch.float32, device=out.device)
        grad = torch.empty_like(out)
        _lib.check(_lib.lib().read_huber_loss(out.data_ptr(), target.data_ptr(), n, 1.0 / n, loss.data_ptr(), grad.data_ptr(),
                                              _lib.stream_ptr()))
        ctx.save_for_backward(grad)
        return loss[0] / n

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None


def huber_loss(out, target):
    """``F.huber_loss(out, target)`` (delta 1, mean) with value and gradient from one HIP launch."""
    return _HuberFn.apply(out, target)


# -----------------------------------------------------------------------------------------------------------------------
# the UNet graph in training mode (READ/models/unet.py:202-285), one image, NHWC
# -----------------------------------------------------------------------------------------------------------------------
def _bc(net, path, x, k, stride=1, elu=True, blk=(1, 1, 1)):
    node = net
    for p in path.split('.'):
        node = node._modules[p]
    b = node.block
    n = b['norm']
    bn_train = int(bool(net.training))
    if bn_train and net.__dict__.get('_bn_per_item') and blk[0] > 1:
        bn_train = BN_PER_ITEM
    if bn_train and n.num_batches_tracked is not None:
        # nn.BatchNorm2d bookkeeping (momentum is fixed, so only a counter): one forward call per statistic group
        n.num_batches_tracked += blk[0] if bn_train == BN_PER_ITEM else 1
    return GatedConvFn.apply(x, b['conv_f'].weight, b['conv_f'].bias, b['conv_m'].weight, b['conv_m'].bias, n.weight, n.bias,
                             n.running_mean, n.running_var, k, stride, elu, *blk, bn_train, net.__dict__.get('_grad_arena'))


def _res_blocks(net, prefix, x, blk):
    for j in range(4):
        p = f"{prefix}.layers.{j}.main."
        x = _bc(net, p + "1", _bc(net, p + "0", x, 3, blk=blk), 3, elu=False, blk=blk) + x
    return x


def _scm(net, name, x, blk):
    y = _bc(net, name + ".main.0", x, 3, blk=blk)
    y = _bc(net, name + ".main.1", y, 1, blk=blk)
    y = _bc(net, name + ".main.2", y, 3, blk=blk)
    y = _bc(net, name + ".main.3", y, 1, blk=blk)
    return _bc(net, name + ".conv", torch.cat([x, y], -1), 1, elu=False, blk=blk)


def _down(x, s):                       # F.interpolate(scale_factor=1/s), nearest: source index = dst * s
    return x[::s, ::s]


def _up(x, s):                         # nearest up: source index = dst // s
    return x.repeat_interleave(s, 0).repeat_interleave(s, 1)


def unet_forward_train(net, x, x2, x4, x8, blk=(1, 1, 1)):
    """(h,w,8) NHWC pyramids -> (H,W,3); every tensor carries autograd history.  blk = (nb, v_num, v_den): the tensors hold
    nb items stacked vertically, v_num of every v_den rows of an item's block are valid (the rest: zero separator rows;
    ``stack_batch``).  Nearest resampling, concatenation, products and sums keep the separators zero by themselves."""
    if PACK_BATCH:
        plan = _pack_plan(net, bool(net.training))         # every layer's parameter block and fragments: one launch
        if plan is not None:                               # None: a layout the batch packer does not take -> the per-layer packers
            plan.refresh()
    net.__dict__['_grad_arena'] = _GradArena()
    z2, z4, z8 = _scm(net, "SCM2", x2, blk), _scm(net, "SCM1", x4, blk), _scm(net, "SCM0", x8, blk)
    res1 = _res_blocks(net, "Encoder.0", _bc(net, "feat_extract.0", x, 3, blk=blk), blk)
    z = _bc(net, "feat_extract.1", res1, 3, stride=2, blk=blk)
    z = z + _bc(net, "FAM2.merge", z * z2, 3, elu=False, blk=blk)
    res2 = _res_blocks(net, "Encoder.1", z, blk)
    z = _bc(net, "feat_extract.2", res2, 3, stride=2, blk=blk)
    z = z + _bc(net, "FAM1.merge", z * z4, 3, elu=False, blk=blk)
    res3 = _res_blocks(net, "Encoder.2", z, blk)
    z = _bc(net, "feat_extract.6", res3, 3, stride=2, blk=blk)
    z = z + _bc(net, "FAM0.merge", z * z8, 3, elu=False, blk=blk)
    z = _res_blocks(net, "Encoder.3", z, blk)
    z12, z13 = _down(res1, 2), _down(res1, 4)
    z21, z23 = _up(res2, 2), _down(res2, 2)
    z32, z31 = _up(res3, 2), _up(res3, 4)
    z43 = _up(z, 2)
    z42 = _up(z43, 2)
    z41 = _up(z42, 2)

    def aff(name, xs):
        return _bc(net, name + ".conv.1", _bc(net, name + ".conv.0", torch.cat(xs, -1), 1, blk=blk), 3, elu=False, blk=blk)
    r1, r2, r3 = aff("AFFs.0", [res1, z21, z31, z41]), aff("AFFs.1", [z12, res2, z32, z42]), aff("AFFs.2", [z13, z23, res3, z43])
    z = _res_blocks(net, "Decoder.0", z, blk)
    z = Up4Fn.apply(_bc(net, "feat_extract.7", z, 4, stride=2, blk=blk), *blk)
    z = _res_blocks(net, "Decoder.1", _bc(net, "Convs.0", torch.cat([z, r3], -1), 1, blk=blk), blk)
    z = Up4Fn.apply(_bc(net, "feat_extract.3", z, 4, stride=2, blk=blk), *blk)
    z = _res_blocks(net, "Decoder.2", _bc(net, "Convs.1", torch.cat([z, r2], -1), 1, blk=blk), blk)
    z = Up4Fn.apply(_bc(net, "feat_extract.4", z, 4, stride=2, blk=blk), *blk)
    z = _res_blocks(net, "Decoder.3", _bc(net, "Convs.2", torch.cat([z, r1], -1), 1, blk=blk), blk)
    return _bc(net, "feat_extract.5", z, 3, elu=False, blk=blk)


SEPARATOR_ROWS = 16        # zero rows between the items of a stacked batch at full resolution (1 row at the 1/16 scale)


def stack_batch(x_nchw, level):
    """(B,C,h,w) -> (B * (h + gap), w, C) NHWC: the items of a batch stacked vertically with SEPARATOR_ROWS >> level zero
    rows after each — the zero padding every convolution expects between neighbours, so one launch covers the batch."""
    B, c, h, w = x_nchw.shape
    x = x_nchw.permute(0, 2, 3, 1)
    if B > 1:
        x = torch.nn.functional.pad(x, (0, 0, 0, 0, 0, SEPARATOR_ROWS >> level))
    return x.reshape(-1, w, c).contiguous()


# bench.py is the reader of both: LAST_STEP_PATH after its timed steps, GRAPH_TRAIN (saved, cleared, restored) around its instrumented step
GRAPH_TRAIN = False
LAST_STEP_PATH = None


def unet_forward_train_batch(net, xs, per_item_statistics=False):
    """xs: four (B,8,h,w) pyramids -> (B,3,H,W) through ONE stacked image.  In ``.train()`` the BatchNorm layers normalise with
    the statistics of the whole batch — ``nn.BatchNorm2d`` on a (B,C,h,w) tensor — unless ``per_item_statistics``: then every item
    is its own batch of one and the running buffers move B times in item order, which is what B separate calls of the net do
    (``NetAndTexture.forward``, READ/models/compose.py:137-176)."""
    global LAST_STEP_PATH
    LAST_STEP_PATH = 'eager'
    B, _, H, W = xs[0].shape
    if H % 16 or W % 16:
        raise ValueError(f"training crops must be multiples of 16, got {W}x{H}")
    blk = (B, H, H + SEPARATOR_ROWS) if B > 1 else (1, 1, 1)
    net.__dict__['_bn_per_item'] = bool(per_item_statistics)
    try:
        out = unet_forward_train(net, *[stack_batch(x, l) for l, x in enumerate(xs)], blk=blk)
    finally:
        net.__dict__['_bn_per_item'] = False
    out = out.reshape(B, -1, W, 3)[:, :H]
    return out.permute(0, 3, 1, 2)


# -----------------------------------------------------------------------------------------------------------------------
# descriptor optimizer
# -----------------------------------------------------------------------------------------------------------------------
class SparseDescriptorRMSprop:
    """RMSprop (torch defaults, READ/pipelines/ogl.py:16: alpha 0.99, eps 1e-8, no momentum) over the descriptor ROWS that
    the step's index maps touched.  The dense optimizer of the reference reads and writes all N rows of gradient, state
    and parameter every step; rows without a pixel have zero gradient, so only their second-moment decay is owed — it is
    applied lazily when the row is touched again (csrc/train.hip), which makes every row's trajectory equal the dense one.

    Duck-types what ``train.py`` uses of a torch optimizer: ``step()``, ``zero_grad()``, ``param_groups`` (lr),
    ``state_dict()`` / ``load_state_dict()``.

    ``textures`` may hold ``JointTexture`` modules: a joint with queued pairs does one sort of its merged ids and one
    ``read_rmsprop_sorted_tables`` over its parts.  The state (sq, stamp, step) is kept per PART, where a part trained alone keeps
    it, so a part may be stepped through a joint in one iteration and alone in the next.  When a joint steps, every trainable
    part's step advances, touched or not: the dense optimizer on the concatenated parameter.  A list without joints takes the
    single-table path unchanged."""

    def __init__(self, textures, lr=1e-1, alpha=0.99, eps=1e-8):
        self.textures = list(textures)
        self.param_groups = [{'params': [t.texture_ for t in self._tables()], 'lr': lr, 'alpha': alpha, 'eps': eps}]
        self.state = {}
        self._joint_scratch = {}

    def _tables(self):
        """The PointTextures that carry state, once each: the list's own and the joints' parts, in order of first appearance."""
        out, seen = [], set()
        for tex in self.textures:
            for t in getattr(tex, 'parts', None) or [tex]:
                if id(t) not in seen:
                    seen.add(id(t))
                    out.append(t)
        return out

    def _step_joint(self, joint, g):
        pend = joint.take_pending()
        live = joint.trainable_parts()
        if pend is None or not live:
            return
        L = _lib.lib()
        table = (_lib.RmspropTable * len(joint.parts))()
        for t, (part, base) in enumerate(zip(joint.parts, joint.id_bases)):
            table[t].n, table[t].id_base = part.num_ids(), int(base)
            if not part.wants_grad():
                continue                                      # frozen: trainable 0, no pointers, no state
            s = self._state(part)
            s['step'] += 1
            rows = part.training_rows()
            table[t].rows, table[t].sq, table[t].stamp = rows.data_ptr(), s['sq'].data_ptr(), s['stamp'].data_ptr()
            table[t].step, table[t].trainable = s['step'], 1
        pids, pg = pend
        sorted_ids, perm = torch.sort(pids, stable=True)
        scratch = self._joint_scratch.get(pids.device)
        if scratch is None:
            scratch = self._joint_scratch[pids.device] = torch.zeros(int(L.read_rmsprop_sorted_scratch_ints()), dtype=torch.int32,
                                                                     device=pids.device)
        _lib.check(L.read_rmsprop_sorted_tables(table, len(joint.parts), int(pg.shape[1]), sorted_ids.data_ptr(), perm.data_ptr(),
                                                pg.data_ptr(), int(pids.numel()), float(g['lr']), float(g['alpha']), float(g['eps']),
                                                scratch.data_ptr(), _lib.stream_ptr()), "read_rmsprop_sorted_tables")
        for part in live:
            part.rows_changed()

    def _state(self, tex):
        s = self.state.get(id(tex))
        if s is None:
            rows = tex.training_rows()
            s = self.state[id(tex)] = {'step': 0, 'sq': torch.zeros_like(rows),
                                       'stamp': torch.zeros(rows.shape[0], dtype=torch.int32, device=rows.device)}
        return s

    def step(self, closure=None):
        g = self.param_groups[0]
        L = _lib.lib()
        for tex in self.textures:
            if hasattr(tex, 'parts'):             # a JointTexture: one sorted update over its parts' tables
                self._step_joint(tex, g)
                continue
            if tex._touched:                      # someone asked for the dense gradient rows: everything goes through them
                tex.grad_rows()
            pend = tex.take_pending()
            ids = tex.take_touched()
            if pend is None and ids is None:
                continue
            s = self._state(tex)
            s['step'] += 1
            rows = tex.training_rows()
            if pend is not None:
                # pairs sorted by id, runs summed in order, each row updated once (no gradient table, deterministic)
                pids, pg = pend
                sorted_ids, perm = torch.sort(pids, stable=True)
                if 'scratch' not in s:
                    s['scratch'] = torch.zeros(int(L.read_rmsprop_sorted_scratch_ints()), dtype=torch.int32, device=rows.device)
                _lib.check(L.read_rmsprop_sorted(rows.data_ptr(), s['sq'].data_ptr(), s['stamp'].data_ptr(), int(rows.shape[1]),
                                                 int(rows.shape[0]), sorted_ids.data_ptr(), perm.data_ptr(), pg.data_ptr(),
                                                 int(pids.numel()), s['step'], float(g['lr']), float(g['alpha']), float(g['eps']),
                                                 s['scratch'].data_ptr(), _lib.stream_ptr()), "read_rmsprop_sorted")
            else:
                grad = tex.grad_rows()
                _lib.check(L.read_rmsprop_sparse(rows.data_ptr(), s['sq'].data_ptr(), grad.data_ptr(), s['stamp'].data_ptr(),
                                                 int(rows.shape[1]), int(rows.shape[0]), ids.data_ptr(), ids.numel(),
                                                 s['step'], float(g['lr']), float(g['alpha']), float(g['eps']),
                                                 _lib.stream_ptr()), "read_rmsprop_sparse")
            tex.rows_changed()

    def zero_grad(self, set_to_none=True):
        pass                                      # step() leaves every touched gradient row zero again

    def state_dict(self):
        return {'param_groups': [{k: v for k, v in self.param_groups[0].items() if k != 'params'}],
                'state': [{k: (v.cpu() if torch.is_tensor(v) else v) for k, v in self._state(t).items() if k != 'scratch'}
                          for t in self._tables()]}

    def load_state_dict(self, sd):
        self.param_groups[0].update(sd['param_groups'][0])
        for t, s in zip(self._tables(), sd['state']):
            cur = self._state(t)
            cur['step'] = s['step']
            cur['sq'].copy_(s['sq'])
            cur['stamp'].copy_(s['stamp'])
