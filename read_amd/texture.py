"""Neural point descriptors (mirror of READ/models/texture.py:14-70).

``PointTexture`` keeps the reference's parameter (``texture_`` of shape (1, C, N), same
state-dict key) so checkpoints interchange, and serves lookups from an N x C row-major copy in
HBM through the HIP gather (one 32-byte row per point at C = 8 instead of C reads at stride 4N).
"""
import ctypes as C

import torch
import torch.nn as nn

from . import _lib

_ACT = {"none": 0, "sigmoid": 1, "tanh": 2}


def texture_to_rows(texture_cn):
    """(C, N) channel-major CUDA tensor -> (N, C) row-major CUDA tensor."""
    Cc, n = texture_cn.shape
    rows = torch.empty((n, Cc), dtype=torch.float32, device=texture_cn.device)
    _lib.check(_lib.lib().read_texture_to_rows(texture_cn.data_ptr(), n, Cc, rows.data_ptr(), _lib.stream_ptr()),
               "read_texture_to_rows")
    return rows


def rows_to_texture(rows_nc):
    n, Cc = rows_nc.shape
    tex = torch.empty((Cc, n), dtype=torch.float32, device=rows_nc.device)
    _lib.check(_lib.lib().read_rows_to_texture(rows_nc.data_ptr(), n, Cc, tex.data_ptr(), _lib.stream_ptr()),
               "read_rows_to_texture")
    return tex


def gather_pyramid(rows_nc, idx_levels, activation="none", out=None, ss=1):
    """rows (N,C) + int32 index maps [(B,h,w)...] -> NHWC feature maps [(B,h,w,C)...].
    ss > 1: the index maps were rendered at ss x the feature size (READ/gl/nn.py:100-101) and the samples are reduced by
    the bilinear downscale of READ/models/compose.py:162-163 inside the same launch -> [(B,h/ss,w/ss,C)...]."""
    n, Cc = rows_nc.shape
    levels = len(idx_levels)
    if ss > 1:
        B = int(idx_levels[0].shape[0])
        hs = [int(i.shape[1]) // ss for i in idx_levels]
        wsz = [int(i.shape[2]) // ss for i in idx_levels]
        for i, h, w in zip(idx_levels, hs, wsz):
            if i.shape[0] != B or h * ss != i.shape[1] or w * ss != i.shape[2]:
                raise ValueError(f"index map {tuple(i.shape)} is not a multiple of supersampling {ss}")
        if out is None:
            out = [torch.empty((B, h, w, Cc), dtype=torch.float32, device=rows_nc.device) for h, w in zip(hs, wsz)]
        _lib.check(_lib.lib().read_gather_forward_ss(
            rows_nc.data_ptr(), n, Cc, levels, B, _lib.ptr_array([i.data_ptr() for i in idx_levels]),
            (C.c_int * levels)(*hs), (C.c_int * levels)(*wsz), int(ss), _lib.ptr_array([o.data_ptr() for o in out]),
            _ACT[activation], _lib.stream_ptr()), "read_gather_forward_ss")
        return out
    if out is None:
        out = [torch.empty(tuple(i.shape) + (Cc,), dtype=torch.float32, device=rows_nc.device) for i in idx_levels]
    counts = (C.c_int64 * levels)(*[int(i.numel()) for i in idx_levels])
    _lib.check(_lib.lib().read_gather_forward(
        rows_nc.data_ptr(), n, Cc, levels, _lib.ptr_array([i.data_ptr() for i in idx_levels]), counts,
        _lib.ptr_array([o.data_ptr() for o in out]), _ACT[activation], _lib.stream_ptr()), "read_gather_forward")
    return out


def gather_tables_pyramid(tables, idx_levels, out=None):
    """The gather over several descriptor tables (read_gather_forward_tables), one launch for all levels.

    tables: [(rows_nc, id_base, activation), ...], 1..8 of them: table t, an (n_t, C) CUDA tensor, serves the ids
    [id_base_t, id_base_t + n_t) with its own activation; id_base_0 = 0, bases ascend, ranges do not overlap
    (``PointCloudRasterizer.id_ranges``).  An id below 0 reads row 0 of table 0; an id in no range the last row of the last table
    whose base is <= id.  -> NHWC feature maps [(B,h,w,C)...] as ``gather_pyramid``'s."""
    if not 1 <= len(tables) <= _lib.READ_GATHER_MAX_TABLES:
        raise ValueError(f"the table gather takes 1..{_lib.READ_GATHER_MAX_TABLES} tables, got {len(tables)}")
    Cc = int(tables[0][0].shape[1])
    table = (_lib.GatherTable * len(tables))()
    for t, (rows, id_base, activation) in enumerate(tables):
        if not torch.is_tensor(rows) or rows.dim() != 2 or int(rows.shape[1]) != Cc or not rows.is_contiguous():
            raise ValueError(f"table {t}: descriptor rows must be a contiguous (n, {Cc}) tensor")
        table[t].rows_nc, table[t].n = rows.data_ptr(), int(rows.shape[0])
        table[t].id_base, table[t].activation = int(id_base), _ACT[activation]
    levels = len(idx_levels)
    if out is None:
        out = [torch.empty(tuple(i.shape) + (Cc,), dtype=torch.float32, device=tables[0][0].device) for i in idx_levels]
    counts = (C.c_int64 * levels)(*[int(i.numel()) for i in idx_levels])
    _lib.check(_lib.lib().read_gather_forward_tables(
        table, len(tables), Cc, levels, _lib.ptr_array([i.data_ptr() for i in idx_levels]), counts,
        _lib.ptr_array([o.data_ptr() for o in out]), _lib.stream_ptr()), "read_gather_forward_tables")
    return out


def gather_tables_backward(tables, idx_levels, dfeat_levels, feat_levels=None, pairs=False, drows=None):
    """The adjoint of ``gather_tables_pyramid`` (read_gather_backward_tables): g = dfeat * act'(y) per pixel, one launch.

    tables: [(n_t, id_base, activation), ...] — n_t the table's row count, or its (n_t, C) rows (only the count is used);
    dfeat_levels / feat_levels: NHWC gradients and the forward's own outputs [(B,h,w,C)...] (feat_levels may be None when every
    activation is 'none').  pairs=True -> [(B*h*w, C)...], g of every pixel (no atomics; with the ids: the sorted optimizer's
    pairs).  drows: None, or one (n_t, C) gradient-row tensor per table to ADD into (None entries: that table is frozen).
    -> the pairs' levels (or None)."""
    if not 1 <= len(tables) <= _lib.READ_GATHER_MAX_TABLES:
        raise ValueError(f"the table gather takes 1..{_lib.READ_GATHER_MAX_TABLES} tables, got {len(tables)}")
    Cc = int(dfeat_levels[0].shape[-1])
    table = (_lib.GatherTable * len(tables))()
    for t, (rows, id_base, activation) in enumerate(tables):
        table[t].rows_nc, table[t].n = None, int(rows.shape[0]) if torch.is_tensor(rows) else int(rows)
        table[t].id_base, table[t].activation = int(id_base), _ACT[activation]
    if drows is not None:
        if len(drows) != len(tables):
            raise ValueError(f"drows has {len(drows)} entries for {len(tables)} tables")
        for t, d in enumerate(drows):
            if d is not None and (tuple(d.shape) != (table[t].n, Cc) or not d.is_contiguous() or d.dtype != torch.float32):
                raise ValueError(f"table {t}: gradient rows must be a contiguous fp32 ({table[t].n}, {Cc}) tensor")
    levels = len(idx_levels)
    dfeat_levels = [d.contiguous() for d in dfeat_levels]
    g = [torch.empty((int(i.numel()), Cc), dtype=torch.float32, device=dfeat_levels[0].device) for i in idx_levels] if pairs else None
    counts = (C.c_int64 * levels)(*[int(i.numel()) for i in idx_levels])
    arr = lambda ts: None if ts is None else _lib.ptr_array([None if t is None else t.data_ptr() for t in ts])
    _lib.check(_lib.lib().read_gather_backward_tables(
        table, len(tables), Cc, levels, arr(idx_levels), counts, arr(dfeat_levels), arr(feat_levels), arr(g), arr(drows),
        _lib.stream_ptr()), "read_gather_backward_tables")
    return g


def stitch_gather_pyramid(parts, out=None, want_index=False, want_depth=False, want_part=False, want_feat=True, ss=1):
    """Scene stitching (read_stitch_gather_forward): merge the parts' pyramids and gather from the winner's table, one launch.

    parts: list of ``(rows_nc, idx_levels, depth_levels, id_base, activation)``, 1..8 of them — rows (n_s, C) CUDA tensor (with
    want_feat=False the part's point count n_s, an int, does as well), int32 local-id maps and fp32 depth maps [(1,h,w)...] of
    this part's rasteriser (both None = the part is hidden: it keeps its number and its id range, and part 0 still serves the
    pixels nobody covers), id_base added to its ids in the merged index image, activation 'none' / 'sigmoid' / 'tanh'.
    out: None, a list of NHWC feature tensors to fill (as gather_pyramid's), or a dict with any of 'feat', 'index', 'depth', 'part'
    (lists of tensors per level) to fill instead of allocating.
    -> the feature maps [(1,h,w,C)...] alone when no merged image is requested, otherwise the tuple (features, then the
    requested ones of: merged index int32, merged depth fp32, part image uint8 (255 = no candidate)), each [(1,h,w)...];
    features are None with want_feat=False."""
    if ss > 1:
        raise NotImplementedError("stitch_gather_pyramid: supersampling (ss > 1) is not supported with stitching")
    if not 1 <= len(parts) <= _lib.READ_STITCH_MAX_PARTS:
        raise ValueError(f"a stitched frame has 1..{_lib.READ_STITCH_MAX_PARTS} parts, got {len(parts)}")
    if not isinstance(out, dict):
        out = {} if out is None else {'feat': out}
    shown = next((p for p in parts if p[1] is not None), None)
    like = shown[1] if shown is not None else next((v for v in out.values() if v is not None), None)
    if like is None:
        raise ValueError("every part is hidden and no output buffers were given: the image sizes are unknown")
    levels = len(like)
    shapes = [tuple(t.shape[:3]) for t in like]
    device = like[0].device
    rows0 = parts[0][0]
    Cc = int(rows0.shape[1]) if torch.is_tensor(rows0) else 4
    keep, table = [], (_lib.StitchPart * len(parts))()
    for s, (rows, idx, dep, id_base, activation) in enumerate(parts):
        if (idx is None) != (dep is None):
            raise ValueError(f"part {s}: index and depth pyramids go together (both None = hidden)")
        if want_feat and (not torch.is_tensor(rows) or int(rows.shape[1]) != Cc):
            raise ValueError(f"part {s}: descriptor rows missing or not {Cc} channels wide")
        if idx is not None:
            if len(idx) != levels or len(dep) != levels or any(tuple(i.shape) != sh or tuple(d.shape) != sh
                                                               for i, d, sh in zip(idx, dep, shapes)):
                raise ValueError(f"part {s}: pyramid shapes differ from {shapes}")
            ip, dp = _lib.ptr_array([i.data_ptr() for i in idx]), _lib.ptr_array([d.data_ptr() for d in dep])
            keep += [ip, dp]
            table[s].idx_levels, table[s].depth_levels = ip, dp
        table[s].rows_nc = rows.data_ptr() if torch.is_tensor(rows) else None
        table[s].n = int(rows.shape[0]) if torch.is_tensor(rows) else int(rows)
        table[s].id_base = int(id_base)
        table[s].activation = _ACT[activation]

    def buffers(name, want, dtype, tail=()):
        if not want:
            return None
        if out.get(name) is None:
            out[name] = [torch.empty(sh + tail, dtype=dtype, device=device) for sh in shapes]
        return out[name]
    feat = buffers('feat', want_feat, torch.float32, (Cc,))
    index = buffers('index', want_index, torch.int32)
    depth = buffers('depth', want_depth, torch.float32)
    part = buffers('part', want_part, torch.uint8)
    counts = (C.c_int64 * levels)(*[sh[0] * sh[1] * sh[2] for sh in shapes])
    arr = lambda ts: None if ts is None else _lib.ptr_array([t.data_ptr() for t in ts])
    _lib.check(_lib.lib().read_stitch_gather_forward(table, len(parts), Cc, levels, counts, arr(index), arr(depth), arr(part),
                                                     arr(feat), _lib.stream_ptr()), "read_stitch_gather_forward")
    extra = tuple(x for x, w in ((index, want_index), (depth, want_depth), (part, want_part)) if w)
    return (feat,) + extra if extra else feat


def scatter_pyramid(dfeat_levels, idx_levels, n):
    """Backward of gather_pyramid: -> (N, C) gradient rows (fp32 atomics)."""
    Cc = dfeat_levels[0].shape[-1]
    drows = torch.zeros((n, Cc), dtype=torch.float32, device=dfeat_levels[0].device)
    levels = len(idx_levels)
    dfeat_levels = [d.contiguous() for d in dfeat_levels]
    counts = (C.c_int64 * levels)(*[int(i.numel()) for i in idx_levels])
    _lib.check(_lib.lib().read_gather_backward(
        drows.data_ptr(), n, Cc, levels, _lib.ptr_array([i.data_ptr() for i in idx_levels]), counts,
        _lib.ptr_array([d.data_ptr() for d in dfeat_levels]), _lib.stream_ptr()), "read_gather_backward")
    return drows


class _BilinearDownFn(torch.autograd.Function):
    """(B,C,ss*h,ss*w) -> (B,C,h,w): F.interpolate(scale_factor=1/ss, mode='bilinear') (READ/models/compose.py:162-163)."""

    @staticmethod
    def forward(ctx, x, ss):
        x = x.contiguous()
        B, c, H, W = (int(v) for v in x.shape)
        if H % ss or W % ss:
            raise ValueError(f"input {W}x{H} is not a multiple of supersampling {ss}")
        out = torch.empty((B, c, H // ss, W // ss), dtype=torch.float32, device=x.device)
        _lib.check(_lib.lib().read_bilinear_down(x.data_ptr(), B * c, H // ss, W // ss, int(ss), out.data_ptr(), _lib.stream_ptr()),
                   "read_bilinear_down")
        ctx.cfg = (B, c, H, W, int(ss))
        return out

    @staticmethod
    def backward(ctx, g):
        B, c, H, W, ss = ctx.cfg
        g = g.contiguous()
        din = torch.empty((B, c, H, W), dtype=torch.float32, device=g.device)
        _lib.check(_lib.lib().read_bilinear_down_backward(g.data_ptr(), B * c, H // ss, W // ss, ss, din.data_ptr(),
                                                          _lib.stream_ptr()), "read_bilinear_down_backward")
        return din, None


def bilinear_down(x, ss):
    """HIP replacement of ``F.interpolate(x, scale_factor=1/ss, mode='bilinear')`` for integer ss >= 2 (differentiable)."""
    _lib.require_gpu()
    if not x.is_cuda:
        raise _lib.ReadHipError("bilinear_down runs on the GPU")
    return _BilinearDownFn.apply(x.float(), int(ss))


class _RangeCheck:
    """Out-of-range point ids without a device->host sync per lookup.  The reference's index_select (texture.py:61) reports
    them through an asynchronous device assert; here every lookup queues `max(ids) >= n` into pinned host memory and the
    NEXT lookup (or ``flush()``) raises IndexError once that copy has landed — the gather itself clamps, so nothing reads
    out of bounds in the meantime."""

    def __init__(self):
        self.pending = []          # (event, pinned flag tensor, n)
        self.free = []             # pinned one-int buffers whose copy has landed

    def queue(self, ids, n, signed=False):
        """signed: ids may also be negative (ids that did not come from the rasteriser) — a negative id counts as id n."""
        if ids.numel() == 0:                               # an empty lookup has nothing out of range (and no .max())
            return
        flag = self.free.pop() if self.free else torch.empty(1, dtype=torch.int32).pin_memory()
        worst = (torch.where(ids < 0, n, ids) if signed else ids).max()
        flag.copy_(worst.to(torch.int32).reshape(1), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.pending.append((ev, flag, n))

    def poll(self, wait=False):
        keep = []
        for ev, flag, n in self.pending:
            if wait:
                ev.synchronize()
            if ev.query():
                worst = int(flag[0])
                self.free.append(flag)
                if worst >= n:
                    self.pending = []
                    raise IndexError(f"point id {worst} out of range for a descriptor table of {n} points "
                                     f"(wrong texture for this scene?)")
            else:
                keep.append((ev, flag, n))
        self.pending = keep

    def flush(self):
        self.poll(wait=True)


class _GatherFn(torch.autograd.Function):
    """texture_ (1,C,N) x int32 ids (B,H,W) -> NHWC (B,H,W,C); backward = HIP scatter-add."""

    @staticmethod
    def forward(ctx, texture, ids):
        rows = texture_to_rows(texture[0])
        ctx.save_for_backward(ids)
        ctx.n = texture.shape[-1]
        return gather_pyramid(rows, [ids])[0]

    @staticmethod
    def backward(ctx, grad):
        (ids,) = ctx.saved_tensors
        drows = scatter_pyramid([grad], [ids], ctx.n)
        return rows_to_texture(drows)[None], None


class _GatherRowsFn(torch.autograd.Function):
    """Sparse-training lookup: the live (N,C) rows are the master copy.  Backward only QUEUES its (ids, gradient rows) pair on
    the texture (``take_pending``): SparseDescriptorRMSprop sorts the step's pairs by id, sums runs of equal ids and updates
    each touched row once — no N x C gradient table is written (scatter-adding into one cost 10.5 ms per iteration at
    30 M points: random fp32 atomics into 320 MB).  ``grad_rows()`` still materialises the dense gradient rows on request
    (then the optimizer takes them plus the touched ids).  ``texture_`` itself gets no dense (1,C,N) gradient — at 30 M
    points that tensor alone is 960 MB per step."""

    @staticmethod
    def forward(ctx, texture, ids, module):
        ctx.module = module
        ctx.save_for_backward(ids)
        return gather_pyramid(module.training_rows(), [ids])[0]

    @staticmethod
    def backward(ctx, grad):
        (ids,) = ctx.saved_tensors
        m = ctx.module
        g = grad.contiguous()
        m._pending.append((ids.reshape(-1), g.reshape(-1, g.shape[-1])))
        ev = torch.cuda.Event()                     # backward may run on a batch item's own stream (NetAndTexture.forward)
        ev.record()
        m._scatter_events.append(ev)
        return None, None, None


class Texture(nn.Module):
    def null_grad(self):
        raise NotImplementedError()

    def reg_loss(self):
        return 0.


class PointTexture(Texture):
    """Same constructor, parameter name/shape and ``forward`` contract as the reference."""

    def __init__(self, num_channels, size, activation='none', checkpoint=None, init_method='zeros', reg_weight=0.):
        super().__init__()
        assert isinstance(size, int), 'size must be int'
        shape = 1, num_channels, size
        if checkpoint:
            self.texture_ = torch.load(checkpoint, map_location='cpu')['texture'].texture_
        else:
            if init_method == 'rand':
                texture = torch.rand(shape)
            elif init_method == 'zeros':
                texture = torch.zeros(shape)
            else:
                raise ValueError(init_method)
            self.texture_ = nn.Parameter(texture.float())
        if activation not in _ACT:
            raise ValueError(activation)
        self.activation = activation
        self.reg_weight = reg_weight
        self._rows = None
        self._rows_version = None
        self.sparse_training = False        # True: gradients go to grad_rows() + touched ids (SparseDescriptorRMSprop)
        self._range_check = _RangeCheck()   # asynchronous id range check of forward() (raises at the next lookup / check_ids())
        self._grad_rows = None
        self._touched = []
        self._pending = []                  # (ids, gradient rows) pairs of backward passes the optimizer has not consumed
        self._scatter_events = []
        self._rows_newer = False            # the rows were stepped by the sparse optimizer; texture_ is stale until synced

    def null_grad(self):
        self.texture_.grad = None
        self._touched = []
        self._pending = []
        self._scatter_events = []

    # ---- sparse training state ---------------------------------------------------------------------------------------
    def training_rows(self):
        return self.rows()

    def _join_streams(self):
        cur = torch.cuda.current_stream()
        for ev in self._scatter_events:             # gradients produced on other streams must have landed
            cur.wait_event(ev)
        self._scatter_events = []

    def grad_rows(self):
        """Dense (N,C) gradient rows (zero where no pixel pointed).  Queued pairs are scatter-added on the way."""
        rows = self.rows()
        if self._grad_rows is None or self._grad_rows.shape != rows.shape or self._grad_rows.device != rows.device:
            self._grad_rows = torch.zeros_like(rows)
        if self._pending:
            self._join_streams()
            drows = self._grad_rows
            for ids, g in self._pending:
                counts = (C.c_int64 * 1)(int(ids.numel()))
                _lib.check(_lib.lib().read_gather_backward(drows.data_ptr(), drows.shape[0], drows.shape[1], 1,
                                                           _lib.ptr_array([ids.data_ptr()]), counts,
                                                           _lib.ptr_array([g.data_ptr()]), _lib.stream_ptr()),
                           "read_gather_backward")
                self._touched.append(ids)
            self._pending = []
        return self._grad_rows

    def take_pending(self):
        """(ids (n,) int32, gradient rows (n,C)) of every backward pass since the last optimizer step, or None."""
        if not self._pending:
            return None
        self._join_streams()
        ids = torch.cat([p[0] for p in self._pending]).contiguous()
        g = torch.cat([p[1] for p in self._pending]).contiguous()
        self._pending = []
        return ids, g

    def take_touched(self):
        if not self._touched:
            return None
        self._join_streams()
        ids = torch.cat(self._touched).contiguous()
        self._touched = []
        return ids

    def rows_changed(self):
        self._rows_newer = True

    def sync_texture(self):
        """Write the (N,C) rows back into ``texture_`` (checkpoints, dense consumers) after sparse optimizer steps."""
        if self._rows_newer and self._rows is not None:
            self.texture_.data.copy_(rows_to_texture(self._rows)[None])     # .data: no version bump, the row cache stays valid
            self._rows_newer = False

    def state_dict(self, *args, **kwargs):
        self.sync_texture()
        return super().state_dict(*args, **kwargs)

    def _apply(self, fn, *args, **kwargs):
        """``.cpu()`` / ``.cuda()`` / ``.to()`` (NetAndTexture.unload_textures, READ/models/compose.py:118-123; the train loop
        moves the texture off the device between train and eval, train.py:271-305): rows stepped by the sparse optimizer are
        written back into ``texture_`` BEFORE the parameter leaves the device, and the row cache is dropped — the next lookup
        rebuilds it from the (now current) parameter wherever it lives."""
        self.sync_texture()
        out = super()._apply(fn, *args, **kwargs)
        self._rows = None
        self._rows_version = None
        self._rows_newer = False
        self._grad_rows = None
        return out

    def invalidate(self):
        """Drop the cached rows (call after editing ``texture_`` through ``.data`` or other version-blind paths)."""
        self._rows = None
        self._rows_newer = False

    def reg_loss(self):
        return self.reg_weight * torch.mean(torch.pow(self.texture_, 2))

    def rows(self):
        """Cached (N, C) row-major copy of texture_ on its device; refreshed when the parameter changes."""
        t = self.texture_
        key = (t._version, t.data_ptr(), t.device)
        if self._rows is None or self._rows_version != key:
            _lib.require_gpu()
            if not t.is_cuda:
                raise _lib.ReadHipError("PointTexture lookups run on the GPU: move the module with .cuda()")
            self._rows = texture_to_rows(t.detach()[0].contiguous())
            self._rows_version = key
        return self._rows

    @staticmethod
    def _ids(inputs):
        if isinstance(inputs, dict):
            ids = None
            for f, x in inputs.items():
                if 'uv' in f:
                    ids = x[:, 0]
            assert ids is not None, 'Input format does not have uv'
        else:
            ids = inputs[:, 0]                      # B x H x W
        if ids.dtype != torch.int32:
            ids = ids.to(torch.int32)               # float ids are integer valued (texture.py:53 .long())
        return ids.contiguous()

    def forward(self, inputs):
        """ids (B,1|3,H,W) float or int -> (B,C,H,W) view of an NHWC tensor (values as texture.py:55-63)."""
        ids = self._ids(inputs)
        if not self.texture_.is_cuda:
            raise _lib.ReadHipError("PointTexture lookups run on the GPU: move the module with .cuda()")
        ids = ids.to(self.texture_.device)
        # out-of-range ids are reported one lookup late (or at check_ids()): two int(ids.max()) / int(ids.min()) round trips per
        # lookup were 80 device -> host synchronisations per training iteration (8 items x 5 levels); the kernels clamp
        self._range_check.poll()
        self._range_check.queue(ids, self.texture_.shape[-1], signed=True)
        if torch.is_grad_enabled() and self.texture_.requires_grad:
            sample = (_GatherRowsFn.apply(self.texture_, ids, self) if self.sparse_training
                      else _GatherFn.apply(self.texture_, ids))
            if self.activation == 'sigmoid':
                sample = torch.sigmoid(sample)
            elif self.activation == 'tanh':
                sample = torch.tanh(sample)
        else:
            sample = gather_pyramid(self.rows(), [ids], self.activation)[0]
        return sample.permute(0, 3, 1, 2)

    def forward_pyramid(self, idx_levels):
        """Fast path: int32 index maps of all scales -> NHWC feature maps, one launch."""
        return gather_pyramid(self.rows(), idx_levels, self.activation)

    # ---- what NetAndTexture asks of a texture (JointTexture answers the same four) ----------------------------------------------
    @property
    def device(self):
        return self.texture_.device

    def wants_grad(self):
        return self.texture_.requires_grad

    def num_ids(self):
        """Ids 0 .. num_ids() - 1 are valid for this texture."""
        return int(self.texture_.shape[-1])

    def lookup_pyramid(self, idx_levels, ss=1):
        """The no-gradient lookup of all scales in one launch; ss > 1: the fused bilinear reduce of gather_pyramid."""
        return gather_pyramid(self.rows(), idx_levels, self.activation, ss=ss)

    def check_ids(self):
        """Wait for the queued id range checks of forward() and raise IndexError if one of them failed."""
        self._range_check.flush()


class _JointGatherFn(torch.autograd.Function):
    """JointTexture's lookup with a gradient: merged ids (B,H,W) -> NHWC (B,H,W,C) through the table gather (the activations are
    applied inside the launch), backward through its adjoint read_gather_backward_tables.  Sparse mode queues (merged ids, g) on the
    joint as _GatherRowsFn does on a PointTexture; dense mode returns every trainable part's (1,C,N) gradient.  ``params`` are the
    trainable parts' ``texture_`` — present so that autograd calls backward at all."""

    @staticmethod
    def forward(ctx, ids, joint, *params):
        ctx.joint = joint
        y = gather_tables_pyramid(joint.tables(), [ids])[0]
        ctx.save_for_backward(ids, y)
        return y

    @staticmethod
    def backward(ctx, grad):
        ids, y = ctx.saved_tensors
        m = ctx.joint
        meta = m.tables(rows=False)
        feat = [y] if any(p.activation != 'none' for p in m.parts) else None
        if m.sparse_training:
            g = gather_tables_backward(meta, [ids], [grad], feat, pairs=True)[0]
            m._pending.append((ids.reshape(-1), g))
            ev = torch.cuda.Event()                 # backward may run on a batch item's own stream (NetAndTexture.forward)
            ev.record()
            m._scatter_events.append(ev)
            return (None, None) + (None,) * len(m.trainable_parts())
        drows = [torch.zeros_like(p.rows()) if p.wants_grad() else None for p in m.parts]
        gather_tables_backward(meta, [ids], [grad], feat, drows=drows)
        return (None, None) + tuple(rows_to_texture(d)[None] for d in drows if d is not None)


class JointTexture(Texture):
    """1..8 ``PointTexture`` parts of equal channel count served as ONE texture of merged ids: part t owns the ids
    [id_base_t, id_base_t + n_t) (``stitch.id_bases`` of the parts' sizes by default; explicit ascending, non-overlapping bases
    with gaps are accepted — the rule of read_gather_forward_tables).  With equal activations and contiguous ranges, looking up
    and training through the joint is looking up and training the concatenated table; nothing is concatenated or copied.

    The parts stay ordinary modules: they may be registered elsewhere under their own ids, trained alone in another iteration, and
    saved by their own ``state_dict``.  A part with ``texture_.requires_grad == False`` is frozen.  ``sparse_training`` is set on
    the joint and forwarded to the parts; in that mode backward queues (merged ids, gradient rows) on the JOINT (``take_pending``)
    for ``SparseDescriptorRMSprop``.  Ids below 0 or in a gap are clamped by the lookup as the table gather documents and are never
    trained; ids past the last range are reported by ``check_ids`` one lookup late, as PointTexture's."""

    def __init__(self, textures, id_bases=None):
        super().__init__()
        textures = list(textures)
        if not 1 <= len(textures) <= _lib.READ_GATHER_MAX_TABLES:
            raise ValueError(f"a JointTexture has 1..{_lib.READ_GATHER_MAX_TABLES} parts, got {len(textures)}")
        for t, p in enumerate(textures):
            if not isinstance(p, PointTexture):
                raise ValueError(f"part {t}: a JointTexture joins PointTexture modules, got {type(p).__name__}")
        chans = [int(p.texture_.shape[1]) for p in textures]
        if len(set(chans)) != 1:
            raise ValueError(f"the parts' descriptor tables differ in their channel count: {chans}")
        sizes = [p.num_ids() for p in textures]
        if id_bases is None:
            from .stitch import id_bases as prefix_bases
            id_bases = prefix_bases(sizes)
        id_bases = [int(b) for b in id_bases]
        if len(id_bases) != len(textures):
            raise ValueError(f"id_bases has {len(id_bases)} entries for {len(textures)} parts")
        if id_bases[0] != 0:
            raise ValueError(f"id_bases[0] must be 0 (got {id_bases[0]})")
        for t in range(1, len(id_bases)):
            if id_bases[t] < id_bases[t - 1] + sizes[t - 1]:
                raise ValueError(f"part {t}: id_base {id_bases[t]} overlaps the range of part {t - 1}, which ends at "
                                 f"{id_bases[t - 1] + sizes[t - 1]}")
        if id_bases[-1] + sizes[-1] > (1 << 31) - 1:
            raise ValueError(f"merged ids up to {id_bases[-1] + sizes[-1]} leave the int32 id range")
        self.parts = nn.ModuleList(textures)
        self.id_bases = id_bases
        self.num_channels = chans[0]
        self._range_check = _RangeCheck()
        self._pending = []                  # (merged ids, gradient rows) pairs the optimizer has not consumed
        self._scatter_events = []
        self.sparse_training = any(p.sparse_training for p in textures)

    @property
    def sparse_training(self):
        return self._sparse_training

    @sparse_training.setter
    def sparse_training(self, flag):
        self._sparse_training = bool(flag)
        for p in self.parts:
            p.sparse_training = bool(flag)

    # ---- the parts as a table list ------------------------------------------------------------------------------------------------
    def tables(self, rows=True):
        """[(rows_t | n_t, id_base_t, activation_t), ...]: gather_tables_pyramid's / gather_tables_backward's table list."""
        return [(p.rows() if rows else p.num_ids(), b, p.activation) for p, b in zip(self.parts, self.id_bases)]

    def trainable_parts(self):
        return [p for p in self.parts if p.wants_grad()]

    @property
    def device(self):
        return self.parts[0].device

    def wants_grad(self):
        return any(p.wants_grad() for p in self.parts)

    def num_ids(self):
        """The end of the last part's id range."""
        return self.id_bases[-1] + self.parts[-1].num_ids()

    def _on_gpu(self):
        for t, p in enumerate(self.parts):
            if not p.texture_.is_cuda:
                raise ValueError(f"JointTexture: part {t} is not loaded on the GPU (move the joint, or the module it is registered "
                                 "in, with .cuda(); NetAndTexture.load_textures takes the joint's own id)")

    def lookup_pyramid(self, idx_levels, ss=1):
        if ss > 1:
            raise NotImplementedError(f"supersampling {ss} with a JointTexture: the table gather has no fused bilinear reduce")
        self._on_gpu()
        return gather_tables_pyramid(self.tables(), idx_levels)

    def forward_pyramid(self, idx_levels):
        """Fast path: int32 maps of merged ids at all scales -> NHWC feature maps, one launch."""
        return self.lookup_pyramid(idx_levels)

    def forward(self, inputs):
        """merged ids (B,1|3,H,W) float or int -> (B,C,H,W) view of an NHWC tensor."""
        ids = PointTexture._ids(inputs)
        self._on_gpu()
        ids = ids.to(self.device)
        self._range_check.poll()
        self._range_check.queue(ids, self.num_ids(), signed=True)
        if torch.is_grad_enabled() and self.wants_grad():
            sample = _JointGatherFn.apply(ids, self, *[p.texture_ for p in self.trainable_parts()])
        else:
            sample = gather_tables_pyramid(self.tables(), [ids])[0]
        return sample.permute(0, 3, 1, 2)

    # ---- training state -----------------------------------------------------------------------------------------------------------
    def null_grad(self):
        for p in self.parts:
            p.null_grad()
        self._pending = []
        self._scatter_events = []

    def take_pending(self):
        """(merged ids (n,) int32, gradient rows (n,C)) of every backward pass since the last optimizer step, or None."""
        if not self._pending:
            return None
        cur = torch.cuda.current_stream()
        for ev in self._scatter_events:             # gradients produced on other streams must have landed
            cur.wait_event(ev)
        self._scatter_events = []
        ids = torch.cat([p[0] for p in self._pending]).contiguous()
        g = torch.cat([p[1] for p in self._pending]).contiguous()
        self._pending = []
        return ids, g

    def reg_loss(self):
        return sum((p.reg_loss() for p in self.parts), 0.)

    def check_ids(self):
        """Wait for the queued id range checks (the joint's and the parts') and raise IndexError if one of them failed."""
        self._range_check.flush()
        for p in self.parts:
            p.check_ids()
