"""Frame annotations (extension): which object and which instance drew each pixel of an edited frame, and
per-instance 2-D boxes — the back end of scene editing, what a perception data set wants beside the RGB frame.

``PointCloudRasterizer.annotate`` / ``Scene.annotate_frame`` / ``OGL.infer_annotated`` return an ``Annotation``; everything in it
stays on the device and nothing synchronises until ``check()`` or ``boxes()`` is called.  The contract is tests/annotate_model.py.

Level-0 pinhole frames only: no panorama camera, no stitched scene, no supersampling.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib

STATS = _lib.READ_ANNOTATE_STATS
STAT_NAMES = ("vis_px", "vx0", "vy0", "vx1", "vy1", "in_pts", "ax0", "ay0", "ax1", "ay1", "near_bits", "n_pts")
MAX_FOREIGN = _lib.READ_GATHER_MAX_TABLES - 1


class Annotation:
    """``objects`` (H,W) int32: -1 empty, 0 the static scene, k the object; ``instances`` (H,W) int32: the handle of the instance that
    drew the pixel, -1 where none did; ``depth`` (H,W) float32: the frame's level-0 depth; ``stats`` (I,12) int32, one row per
    instance in list order (``STAT_NAMES``); ``handles``: the I handles in that order; ``unmatched``: the device counter."""

    def __init__(self, objects, instances, depth, stats, handles, unmatched):
        self.objects, self.instances, self.depth, self.stats = objects, instances, depth, stats
        self.handles = list(handles)
        self.unmatched = unmatched
        self._call = None

    def refresh(self):
        """Enqueue the same call again on the current stream: the same tables over the same frame tensors, for a loop that renders
        into fixed outputs with an unchanged instance list and camera (every argument was marshalled once)."""
        a, dev, _ = self._call
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().read_annotate_frame(C.byref(a), _lib.stream_ptr()), "read_annotate_frame")
        return self

    def check(self):
        """Reads the counter (the only synchronising call besides ``boxes``): a pixel of an object that no listed instance
        reproduces means that frame and instance list do not belong together."""
        n = int(self.unmatched.item())
        if n:
            raise RuntimeError(f"annotation: {n} pixels match no instance of their object: the frame was not drawn with this "
                               "instance list and camera")
        return self

    def boxes(self):
        """{handle: dict} on the host: vis_px, visible_box and amodal_box as (x0, y0, x1, y1) inclusive or None, in_pts, n_pts,
        nearest_depth (float or None), truncation = 1 - in_pts / n_pts (None without points)."""
        rows = self.stats.cpu().numpy()
        out = {}
        for h, r in zip(self.handles, rows):
            s = dict(zip(STAT_NAMES, (int(v) for v in r)))
            out[h] = {
                'vis_px': s['vis_px'],
                'visible_box': (s['vx0'], s['vy0'], s['vx1'], s['vy1']) if s['vis_px'] else None,
                'in_pts': s['in_pts'], 'n_pts': s['n_pts'],
                'amodal_box': (s['ax0'], s['ay0'], s['ax1'], s['ay1']) if s['in_pts'] else None,
                'nearest_depth': float(np.array(s['near_bits'], np.int32).view(np.float32)) if s['in_pts'] else None,
                'truncation': 1.0 - s['in_pts'] / s['n_pts'] if s['n_pts'] else None,
            }
        return out


def object_lists(objs, K):
    """objs[i] = the object (1..K) instance i draws -> (begin (K+1,), order (I,)) int32: object k's instances are
    order[begin[k-1]:begin[k]], list positions ascending."""
    objs = np.asarray(objs, np.int64).reshape(-1)
    if objs.size and (int(objs.min()) < 1 or int(objs.max()) > K):
        raise ValueError(f"instances draw objects {int(objs.min())}..{int(objs.max())}, the scene has objects 1..{K}")
    order = np.argsort(objs, kind='stable').astype(np.int32)
    begin = np.zeros(K + 1, np.int32)
    begin[1:] = np.cumsum(np.bincount(objs - 1, minlength=K)[:K]) if objs.size else 0
    return begin, order


def annotate_frame(xyz, labels, K_own, foreign, pool_xyz, first, npts, objs, M, visible, values, W, H, idx0, depth0):
    """read_annotate_frame on the current stream.  xyz (N,3), labels (N,) int32 or None, pool_xyz (n,3): CUDA tensors; foreign =
    [(id_base, n, pool_first)]; first, npts, objs, visible, values: host sequences of I entries; M: (I,16) float32 host array;
    idx0, depth0: contiguous int32 / float32 CUDA tensors of W * H pixels.  -> Annotation (handles = values)."""
    W, H = int(W), int(H)
    if W < 1 or H < 1 or W * H >= 1 << 31:
        raise ValueError(f"annotate: bad viewport {W}x{H}")
    dev = xyz.device
    for name, t, dt in (("idx0", idx0, torch.int32), ("depth0", depth0, torch.float32)):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dt and t.numel() == W * H and t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous {dt} CUDA tensor of {H}x{W} pixels")
    if len(foreign) > MAX_FOREIGN:
        raise ValueError(f"at most {MAX_FOREIGN} foreign objects, got {len(foreign)}")
    I = len(objs)
    K = int(K_own) + len(foreign)
    begin, order = object_lists(objs, K)
    first = np.ascontiguousarray(first, np.int64).reshape(-1)
    npts = np.ascontiguousarray(npts, np.int64).reshape(-1)
    objs32 = np.ascontiguousarray(objs, np.int32).reshape(-1)
    vis = np.ascontiguousarray(visible, np.uint8).reshape(-1)
    M = np.ascontiguousarray(M, np.float32).reshape(-1, 16)
    values = np.ascontiguousarray(values, np.int32).reshape(-1)
    if not (first.size == npts.size == vis.size == M.shape[0] == values.size == I):
        raise ValueError("annotate: the instance table's columns differ in length")
    # one upload for the integer columns: visible | value | npts | begin | order
    ints = np.concatenate([vis.astype(np.int32), values, npts.astype(np.int32), begin, order])
    with torch.cuda.device(dev):
        d_ints = torch.from_numpy(ints).to(dev)
        d_M = torch.from_numpy(M).to(dev)
        out_obj = torch.empty((H, W), dtype=torch.int32, device=dev)
        out_inst = torch.empty((H, W), dtype=torch.int32, device=dev)
        stats = torch.empty((I, STATS), dtype=torch.int32, device=dev)
        unmatched = torch.empty(1, dtype=torch.int32, device=dev)
        fr = (_lib.AnnotateForeign * max(len(foreign), 1))()
        for f, (base, n, pf) in enumerate(foreign):
            fr[f] = _lib.AnnotateForeign(int(base), int(n), int(pf))
        p0 = d_ints.data_ptr()
        a = _lib.AnnotateArgs(
            xyz.data_ptr() or None, int(xyz.shape[0]), None if labels is None else labels.data_ptr() or None, int(K_own),
            len(foreign), fr, pool_xyz.data_ptr() or None, int(pool_xyz.shape[0]), I,
            first.ctypes.data, npts.ctypes.data, objs32.ctypes.data, M.ctypes.data, vis.ctypes.data,
            d_M.data_ptr() or None, p0 if I else None, p0 + 4 * I if I else None, p0 + 8 * I if I else None,
            p0 + 12 * I if I else None, p0 + 12 * I + 4 * (K + 1) if I else None,
            idx0.data_ptr(), depth0.data_ptr(), W, H, out_obj.data_ptr(), out_inst.data_ptr(), stats.data_ptr() or None,
            unmatched.data_ptr())
    ann = Annotation(out_obj, out_inst, depth0.reshape(H, W), stats, values.tolist(), unmatched)
    ann._call = (a, dev, (fr, first, npts, objs32, M, vis, d_ints, d_M, xyz, labels, pool_xyz, idx0, depth0))
    return ann.refresh()
