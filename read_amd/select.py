"""Object selection (extension): per-point labels made on the device — the front end of scene editing.

``label_boxes``   labels from oriented 3-D boxes (KITTI tracklets, a detector's output): read_select_boxes
``MaskVotes``     labels lifted from 2-D label images on posed views, with an occlusion test against the view's own level-0 frame
                  and a vote over the views: read_select_near / read_select_vote / read_select_finish
``box_matrix``    the 12 floats of a box from centre, extents and rotation
``counts``        points per label

The results feed ``Scene.set_object_labels`` / ``PointCloudRasterizer(labels=...)`` / ``FrameRenderer(object_labels=...)``;
``Scene.select_boxes`` and ``Scene.select_masks`` do both steps.

Limitation of the vote, by contract: a point's candidate is the label of the FIRST view that names one; later views can only agree
(hit) or not (seen).  It is not a majority over labels — order the views so that the most trusted comes first.
Pinhole views only: the occlusion window compares clip w, which is no depth under the panorama camera.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .raster import MAX_LABEL

MAX_BOXES = 1024
MAX_VIEWS = 255


def box_matrix(center, size, R=None, yaw=None):
    """The 3x4 float32 matrix A = diag(2 / size) @ R.T @ [I | -center] that takes cloud coordinates to the unit cube of a box:
    ``size`` = its full extents along its own axes, ``R`` = 3x3 rotation box -> cloud, or ``yaw`` = angle in radians about +y (the
    up axis of the project's clouds); not both.  Formed in float64, rounded once."""
    center = np.asarray(center, np.float64).reshape(-1)
    size = np.asarray(size, np.float64).reshape(-1)
    if center.shape != (3,) or size.shape != (3,):
        raise ValueError(f"center and size are 3 numbers each, got {center.shape} and {size.shape}")
    if not (np.isfinite(center).all() and np.isfinite(size).all() and (size > 0).all()):
        raise ValueError(f"a box needs a finite center and positive finite extents, got center {center}, size {size}")
    if R is not None and yaw is not None:
        raise ValueError("R and yaw are mutually exclusive")
    if yaw is not None:
        c, s = np.cos(float(yaw)), np.sin(float(yaw))
        R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float64)
    R = np.eye(3) if R is None else np.asarray(R, np.float64)
    if R.shape != (3, 3) or not np.isfinite(R).all():
        raise ValueError(f"R is a finite 3x3 rotation, got shape {R.shape}")
    S = np.diag(2.0 / size) @ R.T
    return np.ascontiguousarray(np.concatenate([S, -(S @ center)[:, None]], 1).astype(np.float32))


def _device_xyz(xyz):
    dev = _lib.require_gpu()
    x = torch.as_tensor(np.ascontiguousarray(xyz, dtype=np.float32) if not torch.is_tensor(xyz) else xyz)
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError(f"xyz must be (N,3), got {tuple(x.shape)}")
    return x.to(device=dev if not x.is_cuda else x.device, dtype=torch.float32).contiguous()


def _device_labels(labels, n, device, what="labels"):
    """None, or (n,) integer labels in [0, MAX_LABEL] -> int32 CUDA tensor (the caller's tensor itself when it already is one)."""
    if labels is None:
        return None
    lab = torch.as_tensor(labels)
    if lab.dim() != 1 or lab.numel() != n:
        raise ValueError(f"{what} must hold one entry per point ({n}), got shape {tuple(lab.shape)}")
    if lab.dtype.is_floating_point or lab.dtype == torch.bool:
        raise ValueError(f"{what} must be integers, got {lab.dtype}")
    if n and (int(lab.min()) < 0 or int(lab.max()) > MAX_LABEL):
        raise ValueError(f"{what} must lie in [0, {MAX_LABEL}]")
    return lab.to(device=device, dtype=torch.int32).contiguous()


def label_boxes(xyz, boxes, label_of=None, labels=None):
    """xyz (N,3) (a CUDA tensor stays where it is) and K <= 1024 boxes ((K,12) or (K,3,4), see ``box_matrix``) -> int32 CUDA tensor
    (N,): label_of[k] (default k + 1) of the first box that contains the point, else ``labels`` (default 0).  Faces are inclusive;
    several boxes may share a label; label 0 carves points back into the static scene."""
    x = _device_xyz(xyz)
    n = int(x.shape[0])
    b = np.ascontiguousarray(boxes.detach().cpu().numpy() if torch.is_tensor(boxes) else boxes, dtype=np.float32)
    if b.size == 0:
        b = b.reshape(0, 12)
    if b.ndim == 3 and b.shape[1:] == (3, 4):
        b = b.reshape(-1, 12)
    if b.ndim != 2 or b.shape[1] != 12:
        raise ValueError(f"boxes must be (K,12) or (K,3,4), got {b.shape}")
    K = b.shape[0]
    if K > MAX_BOXES:
        raise ValueError(f"at most {MAX_BOXES} boxes per call, got {K}")
    lo = np.arange(1, K + 1, dtype=np.int64) if label_of is None else np.asarray(label_of)
    if lo.shape != (K,) or lo.dtype.kind not in 'iu':
        raise ValueError(f"label_of must hold one integer per box ({K}), got shape {lo.shape} of {lo.dtype}")
    if K and (int(lo.min()) < 0 or int(lo.max()) > MAX_LABEL):
        raise ValueError(f"label_of must lie in [0, {MAX_LABEL}]")
    lab_in = _device_labels(labels, n, x.device)
    out = torch.empty(n, dtype=torch.int32, device=x.device)
    with torch.cuda.device(x.device):
        b_d = torch.from_numpy(b).to(x.device)
        lo_d = torch.from_numpy(lo.astype(np.int32)).to(x.device)
        _lib.check(_lib.lib().read_select_boxes(x.data_ptr() or None, n, b_d.data_ptr() or None, lo_d.data_ptr() or None, K,
                                                None if lab_in is None else lab_in.data_ptr() or None, out.data_ptr() or None,
                                                _lib.stream_ptr()), "read_select_boxes")
    return out


class MaskVotes:
    """Labels lifted from label images on posed pinhole views.  ``add_view`` applies one view after another on the current stream
    (at most 255); ``labels`` reads the vote out.  ``state`` holds one word per point, cand << 16 | hit << 8 | seen (int32 storage
    of the uint32 bits)."""

    def __init__(self, xyz):
        self.xyz = _device_xyz(xyz)
        self.n = int(self.xyz.shape[0])
        self.state = torch.zeros(self.n, dtype=torch.int32, device=self.xyz.device)
        self.n_views = 0
        self._near = None

    def add_view(self, total_m, W, H, idx0, depth0, mask, rel=0.05, slack=0.0):
        """total_m: the pinhole total matrix (16 floats) exactly as ``PointCloudRasterizer.render`` takes it; idx0, depth0: the
        level-0 images of the unedited cloud under it, as ``render`` returns them; mask: (H,W) integer label image, values in
        [0, MAX_LABEL], 0 = no object.  A point counts as seen when its clip w is at most near * (1 + rel) + slack, near = the clip w
        of its pixel's winner (metric distance along the camera axis for ``get_proj_matrix`` projections)."""
        if self.n_views >= MAX_VIEWS:
            raise ValueError(f"at most {MAX_VIEWS} views per MaskVotes: the counters are 8 bits wide")
        W, H = int(W), int(H)
        M = np.ascontiguousarray(total_m.detach().cpu().numpy() if torch.is_tensor(total_m) else total_m, dtype=np.float32)
        if M.size != 16:
            raise ValueError(f"total_m is one 4x4 matrix, got shape {M.shape}")
        M = M.reshape(16)
        if not (np.isfinite(rel) and rel >= 0 and np.isfinite(slack) and slack >= 0):
            raise ValueError(f"rel and slack must be finite and >= 0, got {rel!r}, {slack!r}")
        dev = self.xyz.device
        for name, t, dt in (("idx0", idx0, torch.int32), ("depth0", depth0, torch.float32)):
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dt and t.numel() == W * H and t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous {dt} CUDA tensor of {H}x{W} pixels")
        m = torch.as_tensor(mask)
        if tuple(m.shape) != (H, W):
            raise ValueError(f"mask must be ({H}, {W}), got {tuple(m.shape)}")
        if m.dtype.is_floating_point or m.dtype == torch.bool:
            raise ValueError(f"mask must be integers, got {m.dtype}")
        if m.numel() and (int(m.min()) < 0 or int(m.max()) > MAX_LABEL):
            raise ValueError(f"mask values must lie in [0, {MAX_LABEL}]")
        m = m.to(device=dev, dtype=torch.int32).contiguous()
        if self._near is None or self._near.numel() != W * H:
            self._near = torch.empty(W * H, dtype=torch.float32, device=dev)
        L = _lib.lib()
        Mp = M.ctypes.data_as(C.POINTER(C.c_float))
        with torch.cuda.device(dev):
            st = _lib.stream_ptr()
            _lib.check(L.read_select_near(self.xyz.data_ptr() or None, self.n, Mp, W, H, idx0.data_ptr(), depth0.data_ptr(),
                                          self._near.data_ptr(), st), "read_select_near")
            _lib.check(L.read_select_vote(self.xyz.data_ptr() or None, self.n, Mp, W, H, self._near.data_ptr(), m.data_ptr(),
                                          float(np.float32(1.0 + rel)), float(np.float32(slack)), self.state.data_ptr() or None, st),
                       "read_select_vote")
        self.n_views += 1

    def labels(self, min_hits=1, ratio=(1, 2), labels=None):
        """-> int32 CUDA tensor (N,): the candidate where it was hit in at least ``min_hits`` views and in at least num / den =
        ``ratio`` of the views that saw the point; else ``labels`` (default 0)."""
        num, den = int(ratio[0]), int(ratio[1])
        if not 1 <= int(min_hits) <= 255:
            raise ValueError(f"min_hits must lie in [1, 255], got {min_hits!r}")
        if den < 1 or not 0 <= num <= den:
            raise ValueError(f"ratio = (num, den) needs den >= 1 and 0 <= num <= den, got {ratio!r}")
        lab_in = _device_labels(labels, self.n, self.xyz.device)
        out = torch.empty(self.n, dtype=torch.int32, device=self.xyz.device)
        with torch.cuda.device(self.xyz.device):
            _lib.check(_lib.lib().read_select_finish(self.state.data_ptr() or None, self.n, int(min_hits), num, den,
                                                     None if lab_in is None else lab_in.data_ptr() or None,
                                                     out.data_ptr() or None, _lib.stream_ptr()), "read_select_finish")
        return out


def counts(labels):
    """Points per label 0..max: bincount on the device -> host int64 array."""
    lab = torch.as_tensor(labels).reshape(-1)
    if lab.numel() == 0:
        return np.zeros(1, np.int64)
    return torch.bincount(lab.to(torch.int64)).cpu().numpy().astype(np.int64)
