"""Frame flow (extension): per-pixel motion between two states of one edited scene — where each pixel's surface point
goes in the next frame (optical flow), its depth there, and whether it is still seen, covered, beside the image, cut by a plane or
hidden: the ground truth a rendered sequence exists to provide.

``PointCloudRasterizer.frame_state`` / ``Scene.capture_frame`` / ``OGL.infer_tracked`` snapshot a frame as a ``FrameState``;
``PointCloudRasterizer.flow`` / ``Scene.flow_between`` turn two of them into a ``FrameFlow``.  Everything in it stays on the device and
nothing synchronises until ``check()`` or ``summary()`` is called.  The contract is tests/flow_model.py.

Level-0 pinhole frames only: no panorama or lens camera, no stitched scene, no supersampling.  The labels live on frame A; what frame
B newly shows (disocclusion) is the other direction, ``flow(b, a)``.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .annotate import MAX_FOREIGN, object_lists

STATES = _lib.READ_FLOW_STATES
STATS = _lib.READ_FLOW_STATS
EMPTY, VISIBLE, OCCLUDED, OFF_IMAGE, CLIPPED, HIDDEN, UNMATCHED = range(7)
STATE_NAMES = ("empty", "visible", "occluded", "off_image", "clipped", "hidden", "unmatched")
STAT_NAMES = ("px", "visible", "occluded", "outside")


class FrameState:
    """One frame of an edited scene as the flow needs it: the camera ``M0`` (16 float32), the instance list it was drawn with —
    ``handles``, ``objects`` (the object each draws), ``matrices`` (I,16) = ``object_matrix(M0, P_i)``, ``visible`` — and the level-0
    frame tensors ``idx0`` / ``depth0`` BY REFERENCE (render the next frame into other tensors).  ``raster`` is the rasteriser that
    made it, ``n`` / ``pool_n`` / ``n_objects`` its cloud, pool and object count at that moment: two states are comparable only when
    all four agree."""

    def __init__(self, raster, M0, handles, objects, matrices, visible, W, H, idx0, depth0):
        self.raster = raster
        self.n, self.pool_n, self.n_objects = raster_identity(raster)
        self.M0 = np.array(M0, np.float32).reshape(16)
        self.handles = list(handles)
        self.objects = np.array(objects, np.int32).reshape(-1)
        self.matrices = np.array(matrices, np.float32).reshape(-1, 16)
        self.visible = np.array(visible, np.uint8).reshape(-1)
        self.W, self.H = int(W), int(H)
        self.idx0, self.depth0 = idx0, depth0
        if not (len(self.handles) == self.objects.size == self.matrices.shape[0] == self.visible.size):
            raise ValueError("frame state: the instance table's columns differ in length")


def raster_identity(raster):
    """(n, pool length, object count) of a rasteriser now: what must not change between two states."""
    if raster._inst is None:
        return raster.n, 0, 0
    return raster.n, int(raster._pool_xyz.shape[0]), len(raster._ranges)


class FrameFlow:
    """``flow`` (H,W,2) float32: (u_b - u_a, v_b - v_a) in pixels; ``depth_next`` (H,W) float32: the point's depth in frame B;
    ``state`` (H,W) int32 (``STATE_NAMES``); ``counts`` (8,) int32: pixels per state; ``stats`` (I,4) int32, one row per instance of
    frame A in list order (``STAT_NAMES``); ``handles``: the I handles in that order; ``unmatched``: the device counter.  Flow and
    depth are +0 except where the state is visible, occluded or off_image."""

    def __init__(self, flow, depth_next, state, counts, stats, handles, unmatched):
        self.flow, self.depth_next, self.state, self.counts, self.stats = flow, depth_next, state, counts, stats
        self.handles = list(handles)
        self.unmatched = unmatched
        self._call = None

    def refresh(self):
        """Enqueue the same call again on the current stream: the same tables over the same frame tensors, for a loop that renders
        both frames into fixed outputs with unchanged lists and cameras (every argument was marshalled once)."""
        a, dev, _ = self._call
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().read_flow_frame(C.byref(a), _lib.stream_ptr()), "read_flow_frame")
        return self

    def check(self):
        """Reads the counter (the only synchronising call besides ``summary``): a pixel that its drawer does not reproduce means
        that frame A and its instance list or camera do not belong together."""
        n = int(self.unmatched.item())
        if n:
            raise RuntimeError(f"flow: {n} pixels match no drawer: frame A was not drawn with this instance list and camera")
        return self

    def summary(self):
        """{'counts': {state name: pixels}, 'instances': {handle: {px, visible, occluded, outside}}} on the host."""
        counts = self.counts.cpu().numpy()
        rows = self.stats.cpu().numpy()
        return {'counts': {name: int(counts[s]) for s, name in enumerate(STATE_NAMES)},
                'instances': {h: dict(zip(STAT_NAMES, (int(v) for v in r))) for h, r in zip(self.handles, rows)}}


def flow_frames(xyz, labels, K_own, foreign, pool_xyz, objs, handles, M, visible, M_next, visible_next, M0, M0_next, W, H,
                idx0, depth0, idx0_next, depth0_next):
    """read_flow_frame on the current stream.  xyz (N,3), labels (N,) int32 or None, pool_xyz (n,3): CUDA tensors; foreign =
    [(id_base, n, pool_first)]; objs, handles, visible, visible_next: host sequences of I entries; M, M_next: (I,16) float32 host
    arrays (frame A's and frame B's matrices, both by A's list positions); M0, M0_next: 16 floats each; the four frame tensors:
    contiguous int32 / float32 CUDA tensors of W * H pixels.  -> FrameFlow."""
    W, H = int(W), int(H)
    if W < 1 or H < 1 or W * H >= 1 << 31:
        raise ValueError(f"flow: bad viewport {W}x{H}")
    dev = xyz.device
    for name, t, dt in (("idx0", idx0, torch.int32), ("depth0", depth0, torch.float32), ("idx0_next", idx0_next, torch.int32),
                        ("depth0_next", depth0_next, torch.float32)):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dt and t.numel() == W * H and t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous {dt} CUDA tensor of {H}x{W} pixels")
    if len(foreign) > MAX_FOREIGN:
        raise ValueError(f"at most {MAX_FOREIGN} foreign objects, got {len(foreign)}")
    I = len(objs)
    K = int(K_own) + len(foreign)
    begin, order = object_lists(objs, K)
    objs32 = np.ascontiguousarray(objs, np.int32).reshape(-1)
    vis = np.ascontiguousarray(visible, np.uint8).reshape(-1)
    vis_next = np.ascontiguousarray(visible_next, np.uint8).reshape(-1)
    M = np.ascontiguousarray(M, np.float32).reshape(-1, 16)
    M_next = np.ascontiguousarray(M_next, np.float32).reshape(-1, 16)
    M0 = np.ascontiguousarray(M0, np.float32).reshape(16)
    M0_next = np.ascontiguousarray(M0_next, np.float32).reshape(16)
    if not (vis.size == vis_next.size == M.shape[0] == M_next.shape[0] == len(handles) == I):
        raise ValueError("flow: the instance table's columns differ in length")
    # one upload for the integer columns (visible | visible_next | begin | order) and one for the matrices (M | M_next)
    ints = np.concatenate([vis.astype(np.int32), vis_next.astype(np.int32), begin, order])
    with torch.cuda.device(dev):
        d_ints = torch.from_numpy(ints).to(dev)
        d_M = torch.from_numpy(np.concatenate([M, M_next])).to(dev)
        flow = torch.empty((H, W, 2), dtype=torch.float32, device=dev)
        depth_next = torch.empty((H, W), dtype=torch.float32, device=dev)
        state = torch.empty((H, W), dtype=torch.int32, device=dev)
        counts = torch.empty(STATES, dtype=torch.int32, device=dev)
        stats = torch.empty((I, STATS), dtype=torch.int32, device=dev)
        unmatched = torch.empty(1, dtype=torch.int32, device=dev)
        fr = (_lib.AnnotateForeign * max(len(foreign), 1))()
        for f, (base, n, pf) in enumerate(foreign):
            fr[f] = _lib.AnnotateForeign(int(base), int(n), int(pf))
        p0, m0 = d_ints.data_ptr(), d_M.data_ptr()
        a = _lib.FlowArgs(
            xyz.data_ptr() or None, int(xyz.shape[0]), None if labels is None else labels.data_ptr() or None, int(K_own),
            len(foreign), fr, pool_xyz.data_ptr() or None, int(pool_xyz.shape[0]), I, objs32.ctypes.data,
            m0 if I else None, p0 if I else None, p0 + 8 * I if I else None, p0 + 8 * I + 4 * (K + 1) if I else None,
            m0 + 64 * I if I else None, p0 + 4 * I if I else None, M0.ctypes.data, M0_next.ctypes.data,
            idx0.data_ptr(), depth0.data_ptr(), idx0_next.data_ptr(), depth0_next.data_ptr(), W, H,
            flow.data_ptr(), depth_next.data_ptr(), state.data_ptr(), counts.data_ptr(), stats.data_ptr() or None,
            unmatched.data_ptr())
    out = FrameFlow(flow, depth_next, state, counts, stats, handles, unmatched)
    out._call = (a, dev, (fr, objs32, M0, M0_next, d_ints, d_M, xyz, labels, pool_xyz, idx0, depth0, idx0_next, depth0_next))
    return out.refresh()


def flow_between(a, b):
    """The flow from state ``a`` to state ``b`` of one rasteriser.  B's instances are matched to A's list positions by handle; a
    handle B no longer has is hidden in B.  ValueError unless both states come from the same rasteriser with the same cloud, pool
    and object count (a rebuilt rasteriser — new labels, say — numbers its objects and pool anew)."""
    if a.raster is not b.raster:
        raise ValueError("flow: the two frame states come from different rasterisers (a rebuild — new labels, a new cloud — "
                         "between them numbers objects and pool points anew)")
    if (a.n, a.pool_n, a.n_objects) != (b.n, b.pool_n, b.n_objects):
        raise ValueError(f"flow: the pool or the object count changed between the two states (points {a.n} -> {b.n}, pool "
                         f"{a.pool_n} -> {b.pool_n}, objects {a.n_objects} -> {b.n_objects}): ids and object numbers no longer "
                         "mean the same")
    if (a.W, a.H) != (b.W, b.H):
        raise ValueError(f"flow: the two frames differ in size ({a.W}x{a.H} and {b.W}x{b.H})")
    r = a.raster
    where = {h: j for j, h in enumerate(b.handles)}
    M_next = a.matrices.copy()
    vis_next = np.zeros(len(a.handles), np.uint8)
    for i, h in enumerate(a.handles):
        j = where.get(h)
        if j is not None:                                        # the objects themselves are always there: they cannot be removed
            if b.objects[j] != a.objects[i]:
                raise ValueError(f"flow: instance {h} draws object {a.objects[i]} in one state and {b.objects[j]} in the other")
            M_next[i] = b.matrices[j]
            vis_next[i] = b.visible[j]
    if r._inst is None:                                          # a plain cloud: every pixel is static or empty
        return flow_frames(r.xyz, None, 0, [], r.xyz[:0], [], [], np.zeros((0, 16), np.float32), [], np.zeros((0, 16), np.float32),
                           [], a.M0, b.M0, a.W, a.H, a.idx0, a.depth0, b.idx0, b.depth0)
    K_own = len(r._own_ranges)
    foreign = [(base, int(f.shape[0]), r._ranges[K_own + j][0]) for j, (f, base) in enumerate(r._foreign)]
    return flow_frames(r.xyz, r.labels, K_own, foreign, r._pool_xyz, a.objects, a.handles, a.matrices, a.visible, M_next, vis_next,
                       a.M0, b.M0, a.W, a.H, a.idx0, a.depth0, b.idx0, b.depth0)
