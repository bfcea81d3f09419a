"""LiDAR sweeps of the fitted scene (front end of ``read_lidar_sweep``): the sensor — a beam table, azimuth
columns, a range gate and the see-through filter — and the result of one sweep, a range image plus the return list a LiDAR
consumer reads.  The definition of every number is tests/lidar_model.py; the kernels are read_amd/csrc/lidar.hip.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .camera import lidar_camera

MAX_BEAMS = 128
MAX_WINDOW = 4


def beam_table(elev):
    """(B, 2) float32: (cos, sin) of the float32 elevations (radians), formed in float64 and rounded once."""
    e = np.asarray(elev, np.float32).astype(np.float64)
    return np.ascontiguousarray(np.stack([np.cos(e), np.sin(e)], 1).astype(np.float32))


def column_table(W, kx):
    """(W, 2) float32: (sin, cos) of every column's centre azimuth ((c + 0.5) / W * 2 - 1) / kx under the float32 kx, formed in
    float64 and rounded once."""
    th = ((np.arange(int(W), dtype=np.float64) + 0.5) / int(W) * 2.0 - 1.0) / float(np.float32(kx))
    return np.ascontiguousarray(np.stack([np.sin(th), np.cos(th)], 1).astype(np.float32))


class LidarSensor:
    """A spinning LiDAR: ``elevations_deg`` (1..128 beams, strictly ascending; row b of every image is beam b, row 0 the lowest),
    ``columns`` azimuth columns over ``hfov_deg`` in (0, 360], returns gated to [rmin, rmax] metres.

    half_width_deg: a beam accepts points within this angle of its elevation; None = half the smallest beam spacing (every
    elevation inside the table belongs to a beam; a single beam needs a number).
    window = (wb, wc), rel, slack: the see-through filter — a return is dropped when it lies beyond near * (1 + rel) + slack, near
    the closest return among the cells within wb beams and wc columns (a cloud has gaps, and a far surface seen through a near
    one is no return); (0, 0) keeps everything.  wrap: whether the window's columns wrap round the seam; None = iff hfov_deg == 360.

    The sensor owns the host tables and their device copies; it is placed by ``camera(view_matrix)``."""

    def __init__(self, elevations_deg, columns, hfov_deg=360., rmin=0.5, rmax=120., half_width_deg=None, window=(1, 2), rel=0.05,
                 slack=0.0, wrap=None, device=None):
        self.device = device if device is not None else _lib.require_gpu()
        deg = np.asarray(elevations_deg, np.float64).reshape(-1)
        self.elev = np.ascontiguousarray(np.deg2rad(deg).astype(np.float32))
        self.B, self.W = int(self.elev.shape[0]), int(columns)
        if not 1 <= self.B <= MAX_BEAMS:
            raise ValueError(f"a sensor has 1..{MAX_BEAMS} beams, got {self.B}")
        if not (np.isfinite(self.elev).all() and (np.diff(self.elev) > 0).all()):
            raise ValueError("elevations_deg must be finite and strictly ascending")
        if self.W < 1 or self.B * self.W >= 1 << 31:
            raise ValueError(f"columns must be >= 1 with beams * columns < 2^31, got {columns!r}")
        if half_width_deg is None:
            if self.B == 1:
                raise ValueError("half_width_deg=None means half the smallest beam spacing: a single beam needs a number")
            half_width = 0.5 * float(np.diff(self.elev.astype(np.float64)).min())
        else:
            half_width = float(np.deg2rad(float(half_width_deg)))
        self.hfov_deg, self.rmin, self.rmax, self.half_width = float(hfov_deg), float(rmin), float(rmax), half_width
        lidar_camera(np.eye(4), self.hfov_deg, self.rmin, self.rmax, self.half_width)          # its checks, now
        self.wb, self.wc = int(window[0]), int(window[1])
        if not (0 <= self.wb <= MAX_WINDOW and 0 <= self.wc <= MAX_WINDOW):
            raise ValueError(f"window = (beams, columns) must lie in 0..{MAX_WINDOW} each, got {window!r}")
        if not (float(rel) >= 0.0 and np.isfinite(rel) and float(slack) >= 0.0 and np.isfinite(slack)):
            raise ValueError(f"rel and slack must be finite and >= 0, got {rel!r}, {slack!r}")
        self.scale, self.slack = float(np.float32(1.0 + float(rel))), float(slack)
        self.wrap = (self.hfov_deg == 360.0) if wrap is None else bool(wrap)
        self.kx = lidar_camera(np.eye(4), self.hfov_deg, self.rmin, self.rmax, self.half_width)[12]
        self.beam_dir_host, self.col_dir_host = beam_table(self.elev), column_table(self.W, self.kx)
        self.beam_dir = torch.from_numpy(self.beam_dir_host).to(self.device)
        self.col_dir = torch.from_numpy(self.col_dir_host).to(self.device)

    def camera(self, view_matrix):
        """The 16 floats of ``camera.lidar_camera`` for this sensor at ``view_matrix`` (sensor -> world)."""
        return lidar_camera(view_matrix, self.hfov_deg, self.rmin, self.rmax, self.half_width)


class LidarSweep:
    """One sweep, on the device.  ``range`` (B, W) float32 and ``ids`` (B, W) int32: the range image and the point ids (empty
    cells 0.0 / 0).  The return list, in ascending cell order: ``cells`` (the cell b * W + column), ``return_ids`` and, through
    ``points``, xyz in the sensor frame along the beam — tensors of ``capacity`` entries of which the first
    min(count, capacity) belong to this sweep.  ``labels``: the object label of every listed return when the cloud is labelled
    (foreign objects numbered after the labels), else None.  ``count`` (all returns, also beyond the capacity) and ``points``
    (trimmed to the returns) are the only accessors that synchronise."""

    def __init__(self, sensor, capacity=None, device=None):
        dev = device if device is not None else sensor.device
        self.B, self.W = sensor.B, sensor.W
        self.capacity = self.B * self.W if capacity is None else int(capacity)
        if self.capacity < 0:
            raise ValueError(f"capacity must be >= 0, got {capacity!r}")
        self.range = torch.empty((self.B, self.W), dtype=torch.float32, device=dev)
        self.ids = torch.empty((self.B, self.W), dtype=torch.int32, device=dev)
        self.cells = torch.zeros(self.capacity, dtype=torch.int32, device=dev)
        self.return_ids = torch.zeros(self.capacity, dtype=torch.int32, device=dev)
        self._xyz = torch.zeros((self.capacity, 3), dtype=torch.float32, device=dev)
        self._count = torch.zeros(1, dtype=torch.int32, device=dev)
        self._label_table = None

    @property
    def count(self):
        return int(self._count.item())

    @property
    def points(self):
        return self._xyz[:min(self.count, self.capacity)]

    @property
    def labels(self):
        if self._label_table is None:
            return None
        t = self._label_table
        return t[self.return_ids.long().clamp_(0, t.numel() - 1)]          # entries past the returns hold earlier ids: clamped


def sweep(sensor, cam, xyz, ids, n, inst, ws, out):
    """read_lidar_sweep on the current stream into ``out`` (a LidarSweep)."""
    cam = np.ascontiguousarray(np.asarray(cam, np.float32).reshape(16))
    if cam[12] != sensor.kx:
        raise ValueError("this camera was not formed by the sensor (sensor.camera(view)): its field differs from the sensor's columns")
    if (out.B, out.W) != (sensor.B, sensor.W):
        raise ValueError(f"out is a sweep of {out.B} x {out.W} cells, the sensor has {sensor.B} x {sensor.W}")
    args = _lib.LidarArgs(
        xyz, ids, n, inst, cam.ctypes.data, sensor.elev.ctypes.data, sensor.B, sensor.W, sensor.beam_dir.data_ptr(),
        sensor.col_dir.data_ptr(), sensor.wb, sensor.wc, int(sensor.wrap), sensor.scale, sensor.slack, out.range.data_ptr(),
        out.ids.data_ptr(), out._count.data_ptr(), out.cells.data_ptr() or None, out.return_ids.data_ptr() or None,
        out._xyz.data_ptr() or None, out.capacity, ws.data_ptr(), ws.numel())
    _lib.check(_lib.lib().read_lidar_sweep(C.byref(args), _lib.stream_ptr()), "read_lidar_sweep")
    return out
