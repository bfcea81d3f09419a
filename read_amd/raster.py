"""Device-resident multi-scale point rasteriser (front end of ``read_splat_forward``).

Replaces the reference's per-call upload + 5 x B kernel launches + download
(MyRender/CloudProjection/pcpr_cuda.cpp:23-42, point_render.cu:169-200,
src/READ/gl/myrender.py:32-40) with a cloud that stays in HBM, one pass over it per frame
for all cameras and all scales, and outputs that stay on the device.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .camera import level_sizes


class PointCloudRasterizer:
    """Holds xyz (N,3) fp32 in HBM plus the persistent 64-bit key image.

    ``render(total_m, W, H, levels)`` -> (idx_levels, depth_levels): lists of int32 / fp32 CUDA
    tensors shaped (B, h_l, w_l).  Deterministic: per pixel min depth, ties -> min point id;
    empty pixels are (0, 0.0)."""

    CELLS_MIN_POINTS = 1 << 20      # below this the plain pass is used (read_splat_forward_cells falls back anyway)

    def __init__(self, xyz, device=None, cells=True, labels=None):
        """cells: True = build the cell-ordered copy here (on the device, from self.xyz); False = plain path only; a uint8
        CUDA tensor = a blob built elsewhere (e.g. by rank 0 and broadcast over RCCL, read_amd/sweep.py).

        labels: None, or one object label per point (ints in [0, MAX_LABEL]; 0 = the static scene) — scene editing: label k >= 1
        is drawn with M_0 @ P_k (``set_object_pose``) and can be hidden (``set_object_visible``), see ``render``.  The cloud is
        split once on the device: the static part gets its own id-mapped cell blob, the objects' points are compacted label
        after label.  Index images keep the original ids.  New labels mean a new rasteriser; poses and visibility never do.
        Objects are ADDED with ``add_instance`` (one more copy of a label) and ``add_object`` (points from elsewhere with ids past
        the cloud's, also on a cloud without labels).

        A rasteriser is either plain (``_inst is None``: the whole cloud, read_splat_forward_cells) or a range list (``_inst`` =
        {handle: instance}: a static part plus ranges of a point pool, each with its pose and visible flag, drawn in handle order
        by read_splat_forward_instances).  A labelled cloud is a range list from the start — label k is instance k - 1 — and a
        plain cloud becomes one at its first ``add_object`` / ``add_instance``."""
        self.device = device if device is not None else _lib.require_gpu()
        xyz = torch.as_tensor(np.ascontiguousarray(xyz, dtype=np.float32) if not torch.is_tensor(xyz) else xyz)
        if xyz.dim() != 2 or xyz.shape[1] != 3:
            raise ValueError(f"xyz must be (N,3), got {tuple(xyz.shape)}")
        self.xyz = xyz.to(device=self.device, dtype=torch.float32).contiguous()
        self.n = int(self.xyz.shape[0])
        self._workspaces = {}
        self._ws = None
        self.labels = None
        self._foreign = []            # add_object: (xyz tensor, id_base) of every foreign object, in order
        self._inst = None             # None: a plain cloud; else {handle: instance}, drawn in handle order
        if labels is not None:
            if torch.is_tensor(cells):
                raise ValueError("a cloud with object labels builds its own cell blob (the static part's)")
            self._init_objects(labels, cells)
            return
        # cell-ordered copy (Morton-sorted chunks of 1024 points + bounding boxes), built once per cloud on the device
        self.cells = None
        if torch.is_tensor(cells):
            if cells.dtype != torch.uint8 or cells.numel() != _lib.lib().read_splat_cells_bytes(self.n):
                raise ValueError("cells blob does not belong to a cloud of this size")
            self.cells = cells.to(self.device)
        elif cells and self.n >= self.CELLS_MIN_POINTS:
            self.cells = build_cells_device(self.xyz)
        if self.cells is not None:           # a fresh blob at an address the allocator may have handed out before
            _lib.check(_lib.lib().read_splat_cells_invalidate(self.cells.data_ptr(), self.n), "read_splat_cells_invalidate")

    def _init_objects(self, labels, cells):
        lab = torch.as_tensor(labels)
        if lab.dim() != 1 or lab.numel() != self.n:
            raise ValueError(f"labels must hold one entry per point ({self.n}), got shape {tuple(lab.shape)}")
        static_ids, obj_ids, begin = label_layout(lab.to(self.device))
        self.labels = lab.to(self.device, torch.int32)
        self.n_static, self.n_objects = int(static_ids.numel()), len(begin) - 1
        self._static_ids = static_ids
        self._static_xyz = self.xyz[static_ids.long()].contiguous()
        self.cells = None
        if cells and self.n_static >= self.CELLS_MIN_POINTS:
            self.cells = build_cells_device(self._static_xyz, ids=self._static_ids)
            _lib.check(_lib.lib().read_splat_cells_invalidate(self.cells.data_ptr(), self.n_static), "read_splat_cells_invalidate")
        self._start_ranges(self.xyz[obj_ids.long()].contiguous(), obj_ids, begin)

    def _start_ranges(self, own_xyz, own_ids, begin):
        """The range list of a cloud whose K = len(begin) - 1 own objects are the compacted points own_xyz / own_ids, object k at
        [begin[k-1], begin[k]): each starts as one instance, the object itself (handle k - 1, identity pose, visible)."""
        b = begin.tolist()
        self._own_xyz, self._own_ids = own_xyz, own_ids
        self._own_ranges = [(b[k], b[k + 1] - b[k]) for k in range(len(b) - 1)]
        self._inst = {k: {'k': k + 1, 'own': True, 'P': None, 'visible': True} for k in range(len(b) - 1)}
        self._next_handle = len(b) - 1
        self._rebuild_pool()

    def _object_index(self, k):
        if self.labels is None:
            raise ValueError("this rasteriser was built without object labels")
        k = int(k)
        if not 1 <= k <= self.n_objects:
            raise ValueError(f"no object {k}: labels 1..{self.n_objects} (0 is the static scene)")
        return k - 1

    def set_object_pose(self, k, P):
        """P (4x4, None = identity) maps object k's points, in the cloud's coordinates, to their new place; applies from the next
        frame enqueued (the matrices travel in kernel arguments)."""
        self._inst[self._object_index(k)]['P'] = _pose44(P)     # object k itself is instance k - 1

    def set_object_visible(self, k, flag):
        self._inst[self._object_index(k)]['visible'] = bool(flag)

    # ---- scene editing, third verb: add ------------------------------------------------------------------------------------
    def _as_range_list(self):
        """A plain cloud at its first add_object / add_instance: every point is static — the ids the range kernel needs, no copy
        of the positions — and there is no own object."""
        if self._inst is None:
            self._static_xyz, self.n_static = self.xyz, self.n
            self._static_ids = torch.arange(self.n, dtype=torch.int32, device=self.device)
            self._start_ranges(None, None, np.zeros(1, np.int64))

    def _rebuild_pool(self):
        """The point pool the ranges index: the own objects' compacted points, then the foreign objects'; ids alongside."""
        K = len(self._own_ranges)
        xyz = [self._own_xyz] if K else []
        ids = [self._own_ids] if K else []
        ranges = list(self._own_ranges)
        at = sum(self._own_ranges[-1]) if K else 0
        for fx, base in self._foreign:
            m = int(fx.shape[0])
            xyz.append(fx)
            ids.append(torch.arange(base, base + m, dtype=torch.int32, device=self.device))
            ranges.append((at, m))
            at += m
        self._pool_xyz = torch.cat(xyz).contiguous() if xyz else torch.empty((0, 3), dtype=torch.float32, device=self.device)
        self._pool_ids = torch.cat(ids).contiguous() if ids else torch.empty(0, dtype=torch.int32, device=self.device)
        self._ranges = ranges          # object k = pool points [first, first + n) = self._ranges[k - 1]

    def add_object(self, xyz):
        """A foreign object: m points (m,3) with descriptors of their own (typically a labelled object cut out of another fitted
        scene).  Uploaded once; its point j carries id id_base + j, id_base = N for the first foreign object, each next one
        following the previous (``id_ranges``).  -> k, continuing the label numbering.  It starts with no instance."""
        x = torch.as_tensor(np.ascontiguousarray(xyz, dtype=np.float32) if not torch.is_tensor(xyz) else xyz)
        if x.dim() != 2 or x.shape[1] != 3 or x.shape[0] < 1:
            raise ValueError(f"a foreign object is (m,3) points with m >= 1, got {tuple(x.shape)}")
        base = self.n + sum(int(f.shape[0]) for f, _ in self._foreign)
        if base + int(x.shape[0]) > _INT32_MAX:
            raise ValueError(f"ids {base}..{base + int(x.shape[0])} of the new object leave the int32 index image")
        self._as_range_list()
        self._foreign.append((x.to(device=self.device, dtype=torch.float32).contiguous(), base))
        self._rebuild_pool()
        return len(self._ranges)

    def id_ranges(self):
        """[(id_base, n), ...]: the scene's own ids, then every foreign object's — the tables of the gather, in order."""
        return [(0, self.n)] + [(base, int(f.shape[0])) for f, base in self._foreign]

    def _instance(self, handle):
        if self._inst is None or handle not in self._inst:
            raise ValueError(f"no instance {handle!r}")
        return self._inst[handle]

    def add_instance(self, k, P=None, visible=True):
        """One more copy of object k (an own label or a foreign object) drawn with M_0 @ P from the next frame enqueued.  Nothing
        is rebuilt: the list travels in kernel arguments.  -> a handle for the setters and remove_instance."""
        self._as_range_list()
        k = int(k)
        if not 1 <= k <= len(self._ranges):
            raise ValueError(f"no object {k}: objects 1..{len(self._ranges)}")
        h = self._next_handle
        self._next_handle += 1
        self._inst[h] = {'k': k, 'own': False, 'P': _pose44(P), 'visible': bool(visible)}
        return h

    def set_instance_pose(self, handle, P):
        self._instance(handle)['P'] = _pose44(P)

    def set_instance_visible(self, handle, flag):
        self._instance(handle)['visible'] = bool(flag)

    def remove_instance(self, handle):
        if self._instance(handle)['own']:
            raise ValueError(f"instance {handle} is object {self._inst[handle]['k']} itself: hide it (set_object_visible)")
        del self._inst[handle]

    def _instance_list(self):
        """[(k, P, visible)] of the frame being enqueued, in handle order (handles only grow, so that is the dict's order)."""
        return [(i['k'], i['P'], i['visible']) for i in self._inst.values()]

    def instance_matrices(self, total_m):
        """The (I,16) float32 matrices M_i = object_matrix(M_0, P_i) of the instances, in handle order, for the camera total_m."""
        return object_matrices(total_m, [P for _, P, _ in self._instance_list()]).reshape(-1, 16)

    def _instance_rows(self, cam, floats):
        """(cam as ``floats`` float32, an (I,16) array of zeros with ``object_matrix(R4, P_i)[:3]`` in floats 0..11 of instance i):
        R4 = cam's three rows with (0, 0, 0, 1) beneath, the instances in handle order."""
        cam = np.asarray(cam, np.float32).reshape(floats)
        R4 = np.concatenate([cam[:12].reshape(3, 4), np.array([[0, 0, 0, 1]], np.float32)], 0)
        lst = self._instance_list()
        out = np.zeros((len(lst), 16), np.float32)
        out[:, :12] = object_matrices(R4, [P for _, P, _ in lst])[:, :3].reshape(-1, 12)
        return cam, out

    def pano_instance_cameras(self, cam):
        """The (I,16) float32 panorama cameras of the instances, in handle order, for the camera ``cam`` (camera.pano_camera): the
        rows are ``object_matrix(R4, P_i)[:3]``, R4 = cam's three rows with (0, 0, 0, 1) beneath; kx, ky, za, zb repeat."""
        cam, out = self._instance_rows(cam, 16)
        out[:, 12:] = cam[12:]
        return out

    def lens_instance_cameras(self, cam):
        """The (I,16) float32 rows of the instances, in handle order, for the lens camera ``cam`` (camera.lens_camera): floats
        0..11 are ``object_matrix(R4, P_i)[:3]``, R4 = cam's three rows with (0, 0, 0, 1) beneath; the other 4 are ignored (0
        here) — the twenty scalars belong to the frame and travel once."""
        return self._instance_rows(cam, 32)[1]

    def _instances_struct(self, matrices):
        """The read_splat_instances of this frame: its host arrays (first, npts, visible, M) are built here and kept on self
        until the next frame."""
        lst = self._instance_list()
        first = np.array([self._ranges[k - 1][0] for k, _, _ in lst], np.int64)
        npts = np.array([self._ranges[k - 1][1] for k, _, _ in lst], np.int64)
        vis = np.array([v for _, _, v in lst], np.uint8)
        M = np.ascontiguousarray(matrices, np.float32)
        self._inst_host = (first, npts, vis, M)
        return _lib.SplatInstances(self._pool_xyz.data_ptr() or None, self._pool_ids.data_ptr() or None,
                                   int(self._pool_ids.numel()), len(lst), first.ctypes.data, npts.ctypes.data, M.ctypes.data,
                                   vis.ctypes.data)

    def _render_ranges(self, M, W, H, levels, idx, dep, ws, stream):
        inst = self._instances_struct(self.instance_matrices(M))
        _lib.check(_lib.lib().read_splat_forward_instances(
            self._static_xyz.data_ptr() or None, self._static_ids.data_ptr() or None,
            self.cells.data_ptr() if self.cells is not None else None, self.n_static, M.ctypes.data_as(C.POINTER(C.c_float)),
            W, H, levels, C.byref(inst), idx, dep, ws.data_ptr(), ws.numel(), stream), "read_splat_forward_instances")

    def annotate(self, total_m, W, H, idx0, depth0):
        """Frame annotations (read_amd/annotate.py) of the level-0 frame (idx0, depth0) that ``render(total_m, W,
        H, ...)`` wrote with the CURRENT instance list: -> ``Annotation`` — per pixel the object and the handle of the instance
        that drew it, per instance the visible and amodal boxes, counts and nearest depth.  The matrices are the same host
        arithmetic as the frame's (``instance_matrices``), so the bits agree.  Stream-ordered; ``Annotation.check()`` tells
        whether frame and list belonged together."""
        from . import annotate as ann
        M0 = _host_f32(total_m).reshape(-1, 16)
        if M0.shape[0] != 1:
            raise NotImplementedError(f"more than one camera ({M0.shape[0]}) with annotate: an edited frame has one")
        if self._inst is None:                                   # a plain cloud: every pixel is static or empty
            return ann.annotate_frame(self.xyz, None, 0, [], self.xyz[:0], [], [], [], np.zeros((0, 16), np.float32), [], [],
                                      W, H, idx0, depth0)
        lst = self._instance_list()
        K_own = len(self._own_ranges)
        foreign = [(base, int(f.shape[0]), self._ranges[K_own + j][0]) for j, (f, base) in enumerate(self._foreign)]
        return ann.annotate_frame(self.xyz, self.labels, K_own, foreign, self._pool_xyz,
                                  [self._ranges[k - 1][0] for k, _, _ in lst], [self._ranges[k - 1][1] for k, _, _ in lst],
                                  [k for k, _, _ in lst], self.instance_matrices(M0[0]), [v for _, _, v in lst],
                                  list(self._inst.keys()), W, H, idx0, depth0)

    def frame_state(self, total_m, W, H, idx0, depth0):
        """The snapshot the frame flow works from (read_amd/flow.py): the camera, the CURRENT instance list with
        its matrices (``instance_matrices``: the frame's own host arithmetic) and the level-0 frame (idx0, depth0) that
        ``render(total_m, W, H, ...)`` wrote with them, by reference -> ``FrameState``.  No device work."""
        from . import flow as fl
        M0 = _host_f32(total_m).reshape(-1, 16)
        if M0.shape[0] != 1:
            raise NotImplementedError(f"more than one camera ({M0.shape[0]}) with frame_state: an edited frame has one")
        W, H = int(W), int(H)
        for name, t, dt in (("idx0", idx0, torch.int32), ("depth0", depth0, torch.float32)):
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dt and t.numel() == W * H and t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous {dt} CUDA tensor of {H}x{W} pixels")
        if self._inst is None:
            return fl.FrameState(self, M0[0], [], [], np.zeros((0, 16), np.float32), [], W, H, idx0, depth0)
        lst = self._instance_list()
        return fl.FrameState(self, M0[0], list(self._inst.keys()), [k for k, _, _ in lst], self.instance_matrices(M0[0]),
                             [v for _, _, v in lst], W, H, idx0, depth0)

    def flow(self, a, b):
        """Frame flow from ``FrameState`` a to b, both this rasteriser's: -> ``FrameFlow`` — per pixel of a's frame the motion of
        its surface point to b's frame, its depth there and whether it is still seen (visible / occluded / off_image / clipped /
        hidden), per instance the counts.  B's instances are matched to A's list positions by handle; a handle removed since A is
        hidden in B.  ValueError when the states come from different rasterisers or the pool or object count changed between
        them.  Stream-ordered; ``FrameFlow.check()`` tells whether frame A and its list belonged together."""
        from . import flow as fl
        if a.raster is not self or b.raster is not self:
            raise ValueError("flow: the two frame states come from different rasterisers (this one made "
                             f"{'neither' if a.raster is not self and b.raster is not self else 'only one'} of them)")
        return fl.flow_between(a, b)

    def _outputs(self, B, W, H, levels, want_depth, out):
        """The level lists (idx, depth | None) of a frame — fresh ones, or the caller's ``out`` — and the host arrays of their
        device pointers."""
        if out is None:
            sizes = level_sizes(W, H, levels)
            idx = [torch.empty((B, h, w), dtype=torch.int32, device=self.device) for (w, h) in sizes]
            dep = [torch.empty((B, h, w), dtype=torch.float32, device=self.device) for (w, h) in sizes] if want_depth else None
        else:
            idx, dep = out
        return (idx, dep) + _level_ptrs(idx, dep)

    def _workspace(self, B, W, H):
        """One persistent workspace per (min(B,8), W, H): key images, hi-z bounds and the previous frame's
        winners (the warm start of the next frame rendered at that size)."""
        key = (min(B, 8), W, H)
        ws = self._workspaces.get(key)
        if ws is None:
            need = _lib.lib().read_splat_workspace_bytes(B, W, H)
            ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            _lib.check(_lib.lib().read_splat_workspace_init(ws.data_ptr(), ws.numel(), _lib.stream_ptr()),
                       "read_splat_workspace_init")
            self._workspaces[key] = ws
        self._ws = ws
        return ws

    def render(self, total_m, W, H, levels=5, want_depth=True, out=None, next_total=None):
        """total_m: (B,4,4) or (4,4) fp32 host array/tensor = proj @ inv(view).
        next_total: the matrix the NEXT call at this size will use, when the caller knows it (a sweep, a trajectory replay): this
        frame's last launch then also prepares the next frame's chunk lists and depth seeds (read_splat_hint_next_camera —
        4 dependent launches per frame instead of 5; results identical, a wrong announcement only costs two small memsets)."""
        M = _host_f32(total_m).reshape(-1, 16)
        B = M.shape[0]
        if self._inst is not None and B != 1:
            raise ValueError("a cloud with object labels or added objects renders one camera per call")
        idx, dep, idx_p, dep_p = self._outputs(B, W, H, levels, want_depth, out)
        ws = self._workspace(B, W, H)
        L = _lib.lib()
        if next_total is not None and B == 1 and self.cells is not None:
            Mn = _host_f32(next_total).reshape(-1, 16)
            _lib.check(L.read_splat_hint_next_camera(ws.data_ptr(), Mn.ctypes.data_as(C.POINTER(C.c_float))),
                       "read_splat_hint_next_camera")
        if self._inst is not None:
            self._render_ranges(M, W, H, levels, idx_p, dep_p, ws, _lib.stream_ptr())
            return idx, dep
        _lib.check(L.read_splat_forward_cells(self.xyz.data_ptr(),
                                              self.cells.data_ptr() if self.cells is not None else None, self.n,
                                              M.ctypes.data_as(C.POINTER(C.c_float)), B, W, H, levels, idx_p, dep_p,
                                              ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "read_splat_forward_cells")
        return idx, dep

    def render_pano(self, cam, W, H, levels=5, want_depth=True, out=None):
        """One panorama (cylindrical) frame: ``cam`` = the 16 floats of ``camera.pano_camera`` -> (idx_levels, depth_levels) as
        ``render`` gives them.  One camera per call; object labels, poses and visibility are honoured.  The whole cloud is read
        every frame (no chunk culling under a cylinder); without labels the previous frame's winners warm-start the pass.
        Pinhole and panorama frames may alternate on one rasteriser."""
        return self._render_whole(cam, 16, self.pano_instance_cameras, "read_splat_forward_pano", "render_pano", W, H, levels,
                                  want_depth, out)

    def render_lens(self, cam, W, H, levels=5, want_depth=True, out=None):
        """One frame under a lens camera — a distorted pinhole or a fisheye: ``cam`` = the 32 floats of ``camera.lens_camera``
        -> (idx_levels, depth_levels) as ``render`` gives them.  One camera per call; object labels, instances, poses and
        visibility are honoured.  The whole cloud is read every frame (no chunk culling under a lens); without labels the
        previous frame's winners warm-start the pass.  Pinhole, panorama and lens frames may alternate on one rasteriser."""
        return self._render_whole(cam, 32, self.lens_instance_cameras, "read_splat_forward_lens", "render_lens", W, H, levels,
                                  want_depth, out)

    def _render_whole(self, cam, floats, instance_cameras, symbol, who, W, H, levels, want_depth, out):
        """One frame of a camera that reads the whole cloud: ``floats`` host floats, ``symbol`` (+ ``_instances`` with ranges)."""
        cam = _host_f32(cam).reshape(-1, floats)
        if cam.shape[0] != 1:
            raise ValueError(f"{who} renders one camera per call")
        idx, dep, idx_p, dep_p = self._outputs(1, W, H, levels, want_depth, out)
        ws = self._workspace(1, W, H)
        cam_p = cam.ctypes.data_as(C.POINTER(C.c_float))
        if self._inst is not None:
            inst = self._instances_struct(instance_cameras(cam[0]))
            # a cloud without labels is static as a whole: its points' indices are their ids, and none are passed
            ids = (self._static_ids.data_ptr() or None) if self.labels is not None else None
            _lib.check(getattr(_lib.lib(), symbol + "_instances")(
                self._static_xyz.data_ptr() or None, ids, self.n_static, cam_p, W, H, levels, C.byref(inst), idx_p, dep_p,
                ws.data_ptr(), ws.numel(), _lib.stream_ptr()), symbol + "_instances")
        else:
            _lib.check(getattr(_lib.lib(), symbol)(self.xyz.data_ptr() or None, None, self.n, cam_p, W, H, levels, None, idx_p,
                                                   dep_p, ws.data_ptr(), ws.numel(), _lib.stream_ptr()), symbol)
        return idx, dep

    def lidar_instance_cameras(self, cam):
        """The (I,16) float32 sensors of the instances, in handle order, for the sensor ``cam`` (camera.lidar_camera): the layout
        is the panorama's — rows ``object_matrix(R4, P_i)[:3]``, the four scalars (kx, rmin, rmax, half-width) repeat."""
        return self.pano_instance_cameras(cam)

    def _lidar_workspace(self, B, W):
        """The sweeps' own workspace, apart from the frames': one for every sensor (a sweep leaves it as init did), grown when a
        larger sensor comes."""
        need = _lib.lib().read_lidar_workspace_bytes(B, W)
        ws = getattr(self, '_lidar_ws', None)
        if ws is None or ws.numel() < need:
            ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            _lib.check(_lib.lib().read_lidar_workspace_init(ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "read_lidar_workspace_init")
            self._lidar_ws = ws
        return ws

    def _return_labels(self):
        """labels[id] for every id a return can carry: the cloud's labels, then every foreign object's number (K + 1 + ordinal,
        as in ``annotate``); None for a cloud without labels and foreign objects."""
        if self.labels is None and not self._foreign:
            return None
        K = len(self._own_ranges) if self._inst is not None else 0
        own = self.labels if self.labels is not None else torch.zeros(self.n, dtype=torch.int32, device=self.device)
        return torch.cat([own] + [torch.full((int(f.shape[0]),), K + 1 + j, dtype=torch.int32, device=self.device)
                                  for j, (f, _) in enumerate(self._foreign)])

    def sweep_lidar(self, sensor, cam, out=None):
        """One LiDAR sweep (read_amd/lidar.py): ``sensor`` = a ``LidarSensor``, ``cam`` = its 16 floats at the
        sensor's pose (``sensor.camera(view)``) -> a ``LidarSweep`` (``out``: one to write into).  Object labels, poses, visibility
        and instances are honoured as in ``render_pano``; the whole cloud is read every sweep.  Stream-ordered, nothing is
        synchronised; sweeps use a workspace of their own, so frames and sweeps interleave freely."""
        from . import lidar
        out = lidar.LidarSweep(sensor, device=self.device) if out is None else out
        ws = self._lidar_workspace(sensor.B, sensor.W)
        cam = _host_f32(cam).reshape(16)
        if self._inst is not None:
            inst = self._instances_struct(self.lidar_instance_cameras(cam))
            # a cloud without labels is static as a whole: its points' indices are their ids, and none are passed
            ids = (self._static_ids.data_ptr() or None) if self.labels is not None else None
            lidar.sweep(sensor, cam, self._static_xyz.data_ptr() or None, ids, self.n_static, C.pointer(inst), ws, out)
        else:
            lidar.sweep(sensor, cam, self.xyz.data_ptr() or None, None, self.n, None, ws, out)
        out._label_table = self._return_labels()
        return out

    def bind(self, W, H, levels, out, totals):
        """A pre-bound frame call for loops that must not be host-bound (benchmark stages): every ctypes argument is built ONCE —
        the outputs ``out`` = (idx levels, depth levels or None) and the list of camera matrices ``totals`` — and
        ``call(k, next_k=None)`` then costs two foreign calls (hint + forward), ~5 us of host time instead of the ~80 us of
        ``render()``'s argument marshalling.  Same C entry points, same results."""
        idx, dep = out
        ws = self._workspace(1, W, H)
        L = _lib.lib()
        Ms = [_host_f32(t).reshape(16) for t in totals]
        Mp = [m.ctypes.data_as(C.POINTER(C.c_float)) for m in Ms]
        idx_p, dep_p = _level_ptrs(idx, dep)
        xyz_p, cells_p, ws_p, ws_n = self.xyz.data_ptr(), self.cells.data_ptr() if self.cells is not None else None, ws.data_ptr(), ws.numel()
        fwd, hint, n, check = L.read_splat_forward_cells, L.read_splat_hint_next_camera, self.n, _lib.check
        keep = (Ms, idx, dep, ws)

        def call(k, next_k=None, stream=None):
            st = _lib.stream_ptr() if stream is None else stream
            if next_k is not None and cells_p is not None:
                hint(ws_p, Mp[next_k])
            if self._inst is not None:                                 # scene editing: the matrices of the current poses
                self._render_ranges(Ms[k], W, H, levels, idx_p, dep_p, ws, st)
                return
            check(fwd(xyz_p, cells_p, n, Mp[k], 1, W, H, levels, idx_p, dep_p, ws_p, ws_n, st), "read_splat_forward_cells")
        call.keep = keep
        return call

    def render_gl(self, total_m, W, H, point_size=1.0, relative=False, min_point_size=1.0, discard=None, drop=None,
                  perturb=None, perturb_hash=None, want_depth=True, point_sizes=None, pano=None, lens=None):
        """ONE level of ONE camera at its own size with the GL twin's point options (read_splat_forward_gl):
        point_size / relative ("pN" / "psN" tokens, READ/gl/programs.py:183-192), discard = bool/uint8 (N,) array or
        tensor (set_point_discard), drop = (p, seed) seeded drop, perturb = (N,2) clip-space offsets
        (set_point_perturb), perturb_hash = (amp, seed), point_sizes = (N,) per-point sizes (set_point_sizes; they replace
        point_size as in the shader, programs.py:183-187).  -> (idx (1,H,W) int32, depth (1,H,W) fp32 | None).
        pano = a panorama camera (camera.pano_camera) is refused: the GL twin is a pinhole; so is lens = a lens camera
        (camera.lens_camera)."""
        if self.labels is not None:
            raise NotImplementedError("render_gl (GL-twin point options) with object labels")
        if getattr(self, '_inst', None) is not None:
            raise NotImplementedError("render_gl (GL-twin point options) with added objects or instances (add_object / add_instance)")
        if pano is not None:
            raise NotImplementedError("render_gl (GL-twin point options) with a panorama camera: render_pano draws 1-px point ids")
        if lens is not None:
            raise NotImplementedError("render_gl (GL-twin point options) with a lens camera: render_lens draws 1-px point ids")
        M = _host_f32(total_m).reshape(-1, 16)
        if M.shape[0] != 1:
            raise ValueError("render_gl renders one camera per call")
        o = _lib.SplatGlOpts(float(point_size), int(bool(relative)), float(min_point_size), None, 0, 0, None, 0.0, 0, None)
        keep = []
        if point_sizes is not None:         # per-point sizes (NNScene.set_point_sizes): they replace the token's global size
            ps = torch.as_tensor(point_sizes).to(self.device, torch.float32).contiguous().reshape(-1)
            if ps.numel() != self.n:
                raise ValueError(f"point_sizes has {ps.numel()} entries for {self.n} points")
            keep.append(ps)
            o.point_sizes = ps.data_ptr()
            o.point_size = 0.0
        if discard is not None:
            d = torch.as_tensor(discard).to(self.device, torch.uint8).contiguous()
            if d.numel() != self.n:
                raise ValueError(f"discard mask has {d.numel()} entries for {self.n} points")
            keep.append(d)
            o.discard = d.data_ptr()
        if drop is not None:
            o.drop_threshold, o.drop_seed = drop_threshold(drop[0]), int(drop[1]) & 0xffffffff
        if perturb is not None:
            pt = torch.as_tensor(perturb).to(self.device, torch.float32).contiguous()
            if tuple(pt.shape) != (self.n, 2):
                raise ValueError(f"perturb must be ({self.n}, 2), got {tuple(pt.shape)}")
            keep.append(pt)
            o.perturb = pt.data_ptr()
        if perturb_hash is not None:
            o.perturb_amp, o.perturb_seed = float(perturb_hash[0]), int(perturb_hash[1]) & 0xffffffff
        idx = torch.empty((1, H, W), dtype=torch.int32, device=self.device)
        dep = torch.empty((1, H, W), dtype=torch.float32, device=self.device) if want_depth else None
        ws = self._workspace(1, W, H)
        _lib.check(_lib.lib().read_splat_forward_gl(self.xyz.data_ptr(), self.n, M.ctypes.data_as(C.POINTER(C.c_float)), W, H,
                                                    C.byref(o), idx.data_ptr(), dep.data_ptr() if dep is not None else None,
                                                    ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "read_splat_forward_gl")
        return idx, dep


def drop_threshold(p):
    """Probability -> u32 threshold of the seeded drop (point i dropped iff rnd(i, seed) < threshold)."""
    return int(min(max(float(p), 0.0), 1.0) * 4294967295.0)


def build_cells(xyz):
    """Host blob of ``read_splat_cells_build_host`` for an (N,3) float32 array (uint8 ndarray, upload as is)."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    L = _lib.lib()
    nbytes = L.read_splat_cells_bytes(xyz.shape[0])
    if nbytes == 0:
        raise ValueError(f"cannot build cells for {xyz.shape[0]} points")
    blob = np.empty(nbytes, np.uint8)
    _lib.check(L.read_splat_cells_build_host(xyz.ctypes.data, xyz.shape[0], blob.ctypes.data, nbytes),
               "read_splat_cells_build_host")
    return blob


def build_cells_device(xyz, ids=None):
    """Device blob of ``read_splat_cells_build`` for an (N,3) float32 CUDA tensor: a uint8 CUDA tensor, byte for byte the blob of
    ``build_cells`` (up to the sign of a zero in a box bound).  Its scratch comes from the torch allocator; the call waits for
    the build on the current stream (it reports a non-finite point as the host builder does).
    ids: None, or (N,) ids the records carry instead of the point's index (read_splat_cells_build_ids: a subset of a cloud keeps
    its original ids)."""
    if not (torch.is_tensor(xyz) and xyz.is_cuda) or xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError("build_cells_device takes an (N,3) CUDA tensor")
    xyz = xyz.detach().to(torch.float32).contiguous()
    n = int(xyz.shape[0])
    if ids is not None:
        ids = torch.as_tensor(ids).to(xyz.device, torch.int32).contiguous()
        if ids.numel() != n:
            raise ValueError(f"ids has {ids.numel()} entries for {n} points")
    L = _lib.lib()
    nbytes, sbytes = L.read_splat_cells_bytes(n), L.read_splat_cells_build_scratch_bytes(n)
    if nbytes == 0 or sbytes == 0:
        raise ValueError(f"cannot build cells for {n} points")
    with torch.cuda.device(xyz.device):
        blob = torch.empty(nbytes, dtype=torch.uint8, device=xyz.device)
        scratch = torch.empty(sbytes, dtype=torch.uint8, device=xyz.device)
        if ids is None:
            _lib.check(L.read_splat_cells_build(xyz.data_ptr(), n, blob.data_ptr(), nbytes, scratch.data_ptr(), sbytes,
                                                _lib.stream_ptr()), "read_splat_cells_build")
        else:
            _lib.check(L.read_splat_cells_build_ids(xyz.data_ptr(), ids.data_ptr(), n, blob.data_ptr(), nbytes, scratch.data_ptr(),
                                                    sbytes, _lib.stream_ptr()), "read_splat_cells_build_ids")
    return blob


# ---- scene editing: labels and poses ---------------------------------------------------------------------------------------
MAX_LABEL = (1 << 16) - 1
_EYE4 = np.eye(4, dtype=np.float32)
_INT32_MAX = (1 << 31) - 1


def _level_ptrs(idx, dep):
    """The host arrays of device pointers a frame call takes for its index and depth levels (depth may be None)."""
    return _lib.ptr_array([t.data_ptr() for t in idx]), _lib.ptr_array([t.data_ptr() for t in dep]) if dep is not None else None


def _host_f32(a):
    """A host array or a tensor (any device) -> a contiguous float32 numpy array; the input itself where it already is one."""
    return np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype=np.float32)


def _pose44(P):
    """A pose as the rasteriser keeps it: None (the identity), or a 4x4 float32 array of its own (a copy: the caller may go on
    writing to what it passed)."""
    return None if P is None else np.array(_host_f32(P)).reshape(4, 4)


def object_matrix(M0, P):
    """M_k = M_0 @ P_k on the host in float32 — the one helper the product and the tests use.  P None or exactly the identity:
    M_0 itself (not a product).  Otherwise the row-by-column sums in float32, left to right (j = 0..3), no fused operations."""
    M0 = np.asarray(M0, np.float32).reshape(4, 4)
    if P is None:
        return M0
    P = np.asarray(P, np.float32).reshape(4, 4)
    if np.array_equal(P, _EYE4):
        return M0
    out = M0[:, 0:1] * P[0:1, :]
    for j in range(1, 4):
        out = out + M0[:, j:j + 1] * P[j:j + 1, :]
    return out.astype(np.float32)


def object_matrices(M0, poses):
    """``object_matrix(M0, P)`` for a list of poses in one go -> (n,4,4) float32, bit for bit: the same float32 products and
    sums in the same order, element by element; None and the exact identity yield M_0 itself."""
    M0 = np.asarray(M0, np.float32).reshape(4, 4)
    out = np.empty((len(poses), 4, 4), np.float32)
    out[:] = M0
    moved = [i for i, P in enumerate(poses) if P is not None and not np.array_equal(np.asarray(P, np.float32).reshape(4, 4), _EYE4)]
    if moved:
        P = np.stack([np.asarray(poses[i], np.float32).reshape(4, 4) for i in moved])
        acc = M0[None, :, 0:1] * P[:, 0:1, :]
        for j in range(1, 4):
            acc = acc + M0[None, :, j:j + 1] * P[:, j:j + 1, :]
        out[moved] = acc.astype(np.float32)
    return out


def label_layout(labels):
    """One label per point (0 = static; 1..K objects) -> (static_ids, object_ids, begin): int32 tensors on the labels' device
    holding the original ids of the static points (ascending) and of the object points, label after label (ascending ids
    within a label), and begin (host int64, K + 1 entries): object k = object_ids[begin[k-1]:begin[k]].  K = the largest
    label; a label without points is an empty range."""
    lab = torch.as_tensor(labels)
    if lab.dim() != 1:
        raise ValueError(f"labels must be 1-D, got shape {tuple(lab.shape)}")
    if lab.dtype.is_floating_point or lab.dtype == torch.bool:
        raise ValueError(f"labels must be integers, got {lab.dtype}")
    lab = lab.to(torch.int64)
    if lab.numel() and (int(lab.min()) < 0 or int(lab.max()) > MAX_LABEL):
        raise ValueError(f"labels must lie in [0, {MAX_LABEL}]")
    K = int(lab.max()) if lab.numel() else 0
    static_ids = torch.nonzero(lab == 0).flatten().to(torch.int32)
    oids = torch.nonzero(lab > 0).flatten()
    order = torch.argsort(lab[oids], stable=True)
    object_ids = oids[order].to(torch.int32)
    counts = torch.bincount(lab, minlength=K + 1)[1:].cpu().numpy().astype(np.int64)
    begin = np.zeros(K + 1, np.int64)
    begin[1:] = np.cumsum(counts)
    return static_ids, object_ids, begin


def index_to_float(idx):
    """The reference's float32 index image (point_render.cu:158): ids >= 2**24 round."""
    out = torch.empty(idx.shape, dtype=torch.float32, device=idx.device)
    _lib.check(_lib.lib().read_index_to_float(idx.data_ptr(), idx.numel(), out.data_ptr(), _lib.stream_ptr()),
               "read_index_to_float")
    return out
