"""The fused per-frame path: camera -> point-index pyramids -> descriptor pyramids -> RGB.

This is the hot loop of the reference's viewer (viewer.py:263-285 -> READ/gl/nn.py:113-129 ->
READ/datasets/dynamic.py:66-99 -> READ/models/compose.py:125-181) with every stage resident on
one MI355X: the rasteriser's launches + 1 gather launch + the UNet plan's launches (counts: DESIGN.md §3), three C calls,
no host round trips, no per-frame allocation.
"""
import numpy as np
import torch

from . import _lib
from .camera import lens_camera, level_sizes, pano_camera, total_matrix
from .raster import PointCloudRasterizer
from .texture import gather_pyramid, gather_tables_pyramid, texture_to_rows
from .unet import LAYOUT_FULL, UNetEngine, default_layout, layout_of, pack_state

LEVELS = 5          # the reference rasterises and gathers 5 scales; the UNet consumes 4 (unet.py:209-212)


def unet_engine(unet_state, device, H, W):
    """unet_state (see FrameRenderer) -> (packed fp32 blob on the device, its UNetEngine for H x W): what FrameRenderer and
    StitchedFrameRenderer (read_amd/stitch.py) both start from."""
    if torch.is_tensor(unet_state):
        packed = unet_state.to(device, torch.float32).contiguous()       # full or lean: read off its length
        return packed, UNetEngine(packed, H, W)
    # the lean blob (451 of 952 MB: the F(4x4) layers carry their F(4x4) order only) unless the plan cannot be served by it
    packed = torch.from_numpy(pack_state(unet_state, layout=default_layout())).to(device)
    try:
        return packed, UNetEngine(packed, H, W)
    except _lib.ReadHipError:
        if layout_of(packed) == LAYOUT_FULL:
            raise
        packed = torch.from_numpy(pack_state(unet_state, layout=LAYOUT_FULL)).to(device)
        return packed, UNetEngine(packed, H, W)


class FrameRenderer:
    def __init__(self, xyz, texture_cn, unet_state, W, H, proj_matrix=None, device=None, levels=LEVELS, cells=True,
                 frames_in_flight=1, object_labels=None):
        """xyz (N,3); texture_cn (C,N) descriptors (PointTexture.texture_[0]); unet_state: state dict (tensors or
        ndarrays) under the reference's names, or an already packed fp32 blob (1-D tensor, e.g. received from rank 0);
        W,H multiples of 16; cells: see PointCloudRasterizer.

        frames_in_flight > 1 (throughput mode for pose sweeps): ``render_total`` rasterises and gathers on one stream, in
        call order (the rasteriser warm-starts from the previous call), and runs the UNet of call i on stream i mod F with its
        own plan and feature buffers — the launches of consecutive frames overlap, so the workgroups of one frame fill the
        CUs that the last, partly filled round of the other frame's layer leaves idle.  The returned tensor is then
        complete on ``frame_done`` (an event; ``sync()`` waits for everything), not on the caller's stream.

        object_labels: one label per point for scene editing (PointCloudRasterizer): ``set_object_pose`` /
        ``set_object_visible`` apply to the frames enqueued after the call, also with frames_in_flight > 1 (the matrices travel in
        kernel arguments)."""
        self.device = device if device is not None else _lib.require_gpu()
        if W % 16 or H % 16:
            raise ValueError(f"set width {16 * (W // 16)} / height {16 * (H // 16)}")    # READ/gl/nn.py:107-109
        self.W, self.H, self.levels = W, H, levels
        self.raster = PointCloudRasterizer(xyz, self.device, cells=cells, labels=object_labels)
        if self.raster.n != int(torch.as_tensor(texture_cn).shape[-1]):
            raise ValueError(f"descriptor table has {int(torch.as_tensor(texture_cn).shape[-1])} columns for a cloud of "
                             f"{self.raster.n} points")
        tex = torch.as_tensor(texture_cn, dtype=torch.float32).to(self.device).contiguous()
        self.rows = texture_to_rows(tex)
        self.foreign_rows = []           # add_object: (rows (m,C), activation) of every foreign object, in id order
        self.packed, self.unet = unet_engine(unet_state, self.device, H, W)
        self.proj = None if proj_matrix is None else np.asarray(proj_matrix, np.float32)
        sizes = level_sizes(W, H, levels)
        self.idx = [torch.empty((1, h, w), dtype=torch.int32, device=self.device) for (w, h) in sizes]
        self.depth = [torch.empty((1, h, w), dtype=torch.float32, device=self.device) for (w, h) in sizes]
        self.feat = [torch.empty((1, h, w, self.rows.shape[1]), dtype=torch.float32, device=self.device)
                     for (w, h) in sizes]
        self.rgba = torch.empty((H, W, 4), dtype=torch.float32, device=self.device)
        self.frame_done = None
        self._slots = []
        self._calls = 0
        self._raster_stream = None
        self.set_frames_in_flight(frames_in_flight)

    def set_frames_in_flight(self, frames_in_flight):
        """1 = one frame at a time on the caller's stream (the viewer's mode); F > 1 = F UNet plans / streams (see __init__).
        Waits for the frames in flight before switching."""
        self.sync()
        self._slots = []
        self._calls = 0
        self.frame_done = None
        if frames_in_flight > 1:
            if self._raster_stream is None:
                self._raster_stream = torch.cuda.Stream(self.device)
            for _ in range(int(frames_in_flight)):
                slot = {"feat": [torch.empty_like(f) for f in self.feat], "unet": UNetEngine(self.packed, self.H, self.W),
                        "stream": torch.cuda.Stream(self.device), "ready": torch.cuda.Event(), "done": torch.cuda.Event()}
                slot["done"].record(torch.cuda.current_stream(self.device))
                self._slots.append(slot)

    def set_object_pose(self, k, P):
        self.raster.set_object_pose(k, P)

    def set_object_visible(self, k, flag):
        self.raster.set_object_visible(k, flag)

    def add_object(self, xyz, texture_cn, activation='none'):
        """A foreign object (PointCloudRasterizer.add_object): (m,3) points and their (C,m) descriptors.  -> k for add_instance."""
        tex = torch.as_tensor(texture_cn, dtype=torch.float32).to(self.device).contiguous()
        if tex.dim() != 2 or int(tex.shape[0]) != int(self.rows.shape[1]) or int(tex.shape[1]) != int(np.shape(xyz)[0]):
            raise ValueError(f"a foreign object of {int(np.shape(xyz)[0])} points takes ({int(self.rows.shape[1])}, m) descriptors, "
                             f"got {tuple(tex.shape)}")
        if len(self.foreign_rows) + 2 > _lib.READ_GATHER_MAX_TABLES:
            raise ValueError(f"the table gather serves {_lib.READ_GATHER_MAX_TABLES - 1} foreign objects")
        k = self.raster.add_object(xyz)
        self.foreign_rows.append((texture_to_rows(tex), activation))
        return k

    def add_instance(self, k, P=None, visible=True):
        """One more copy of object k from the next frame enqueued (also with frames_in_flight > 1).  -> a handle."""
        return self.raster.add_instance(k, P, visible)

    def set_instance_pose(self, handle, P):
        self.raster.set_instance_pose(handle, P)

    def set_instance_visible(self, handle, flag):
        self.raster.set_instance_visible(handle, flag)

    def remove_instance(self, handle):
        self.raster.remove_instance(handle)

    def rasterize(self, total_m, next_total=None):
        return self.raster.render(total_m, self.W, self.H, self.levels, out=(self.idx, self.depth), next_total=next_total)

    def _rasterize_with(self, render, cam):
        return render(cam, self.W, self.H, self.levels, out=(self.idx, self.depth))

    def rasterize_pano(self, cam):
        return self._rasterize_with(self.raster.render_pano, cam)

    def rasterize_lens(self, cam):
        return self._rasterize_with(self.raster.render_lens, cam)

    def gather(self, out=None):
        out = self.feat if out is None else out
        if self.foreign_rows:
            ranges = self.raster.id_ranges()
            tables = [(self.rows, 0, 'none')] + [(r, base, act) for (r, act), (base, _) in zip(self.foreign_rows, ranges[1:])]
            return gather_tables_pyramid(tables, self.idx, out=out)
        return gather_pyramid(self.rows, self.idx, out=out)

    def refine(self, out=None, channels=4):
        f = self.feat
        return self.unet.forward(f[0][0], f[1][0], f[2][0], f[3][0], out=self.rgba if out is None else out,
                                 channels=channels)

    def render_total(self, total_m, out=None, channels=4, next_total=None):
        """total_m = proj @ inv(view) (4x4 fp32) -> (H,W,channels) fp32 frame on the device.
        next_total: the NEXT call's matrix when the caller knows it (PointCloudRasterizer.render): one launch less per frame."""
        return self._frame(lambda: self.rasterize(total_m, next_total), out, channels)

    def render_pano_total(self, cam, out=None, channels=4):
        """render_total's twin for a panorama camera (the 16 floats of camera.pano_camera): only the raster step differs."""
        return self._frame(lambda: self._rasterize_with(self.raster.render_pano, cam), out, channels)

    def render_lens_total(self, cam, out=None, channels=4):
        """render_total's twin for a lens camera (the 32 floats of camera.lens_camera): only the raster step differs."""
        return self._frame(lambda: self._rasterize_with(self.raster.render_lens, cam), out, channels)

    def _frame(self, rasterize, out, channels):
        if not self._slots:
            rasterize()
            self.gather()
            return self.refine(out, channels)
        slot = self._slots[self._calls % len(self._slots)]
        self._calls += 1
        if out is None:
            out = torch.empty((self.H, self.W, channels), dtype=torch.float32, device=self.device)
        # whatever the caller's stream has waited for (e.g. the exchange that last read `out`) the writer waits for too
        entered = torch.cuda.Event()
        entered.record(torch.cuda.current_stream(self.device))
        rs = self._raster_stream
        with torch.cuda.stream(rs):
            rs.wait_event(slot["done"])                  # this slot's features were last read by the frame F calls ago
            rasterize()
            self.gather(slot["feat"])
            slot["ready"].record(rs)
        us = slot["stream"]
        with torch.cuda.stream(us):
            us.wait_event(slot["ready"])
            us.wait_event(entered)
            f = slot["feat"]
            slot["unet"].forward(f[0][0], f[1][0], f[2][0], f[3][0], out=out, channels=channels)
            slot["done"].record(us)
        out.record_stream(us)
        self.frame_done = slot["done"]
        return out

    def sync(self):
        """Wait (on the host) for every frame in flight."""
        if self._slots:
            self._raster_stream.synchronize()
            for slot in self._slots:
                slot["stream"].synchronize()

    def _proj(self, proj_matrix):
        """The caller's projection matrix, or the one set at construction."""
        proj = self.proj if proj_matrix is None else np.asarray(proj_matrix, np.float32)
        if proj is None:
            raise ValueError("no projection matrix set")
        return proj

    def render(self, view_matrix, proj_matrix=None, out=None, channels=4):
        """view_matrix: camera->world 4x4 (the reference's convention); -> H x W x 4 RGBA (alpha = 1)."""
        return self.render_total(total_matrix(self._proj(proj_matrix), view_matrix), out, channels)

    def render_pano(self, view_matrix, hfov_deg, proj_matrix=None, out=None, channels=4):
        """A panorama (cylindrical) frame with a horizontal field of hfov_deg in (0, 360]: view_matrix camera->world; of the
        projection matrix only the vertical scale / offset and the depth entries are used (camera.pano_camera).  Object edits
        apply; frames_in_flight as for ``render_total``."""
        return self.render_pano_total(pano_camera(self._proj(proj_matrix), view_matrix, hfov_deg), out, channels)

    def render_lens(self, view_matrix, model, coeffs, limit=None, proj_matrix=None, out=None, channels=4):
        """A frame through a lens: model 0 = a pinhole with Brown-Conrady distortion (coeffs k1, k2, p1, p2, k3), model 1 = a
        Kannala-Brandt fisheye (coeffs k1..k4); limit as in camera.lens_camera (None: just inside where the distortion folds
        back).  view_matrix camera->world.  Object edits apply; frames_in_flight as for ``render_total``."""
        return self.render_lens_total(lens_camera(self._proj(proj_matrix), view_matrix, model, coeffs, limit), out, channels)
