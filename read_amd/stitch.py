"""Scene stitching: several fitted scenes ("parts") rendered into one frame.

Each part keeps what a fitted scene has — its cloud with its own cell blob, workspace and (optionally) object labels, its
descriptor table and texture activation — plus a placement P_s (4x4, default identity) and a visible flag.  A frame rasterises
every visible part with the unchanged single-scene path and the camera M_s = object_matrix(M_0, P_s), then ONE launch
(read_stitch_gather_forward) picks per level and pixel the nearest candidate (smallest depth bit pattern, ties to the lowest part),
gathers from the winner's table and, on request, writes the merged index / depth / part images.  Merged ids are
id_base[s] + local id with id_base[s] = sum of n_t over t < s, hidden parts included: hiding a part never renumbers another.

Placements and visibility apply to the next frame enqueued and never rebuild anything.  One camera per call, one frame at a time
(DESIGN.md §10.2)."""
import numpy as np
import torch

from . import _lib
from .camera import level_sizes, total_matrix
from .frame import LEVELS, unet_engine
from .raster import PointCloudRasterizer, _host_f32, object_matrix
from .texture import _ACT, stitch_gather_pyramid, texture_to_rows

MAX_PARTS = _lib.READ_STITCH_MAX_PARTS
_INT32_MAX = (1 << 31) - 1


def id_bases(counts):
    """Point counts of the parts -> id_base per part (exclusive prefix sum); the total must fit the int32 index image."""
    counts = [int(c) for c in counts]
    if not 1 <= len(counts) <= MAX_PARTS:
        raise ValueError(f"a stitched frame has 1..{MAX_PARTS} parts, got {len(counts)}")
    if sum(counts) > _INT32_MAX:
        raise ValueError(f"{sum(counts)} points in all: merged ids must fit int32")
    return [int(b) for b in np.concatenate([[0], np.cumsum(counts)[:-1]])]


def _pose(P):
    return None if P is None else np.array(_host_f32(P)).reshape(4, 4)


def _one_camera(total_m):
    M = _host_f32(total_m)
    if M.size != 16:
        raise ValueError("a stitched frame renders one camera per call")
    return M.reshape(4, 4)


class StitchedRasterizer:
    """One PointCloudRasterizer per part + the parts' placements and visibility.

    clouds: list of (n_s,3) arrays / tensors, or PointCloudRasterizer objects built elsewhere (taken as they are);
    labels: None, or one entry per part (None or that part's object labels, see PointCloudRasterizer)."""

    def __init__(self, clouds, device=None, cells=True, labels=None):
        self.device = device if device is not None else _lib.require_gpu()
        if not 1 <= len(clouds) <= MAX_PARTS:
            raise ValueError(f"a stitched frame has 1..{MAX_PARTS} parts, got {len(clouds)}")
        if labels is not None and len(labels) != len(clouds):
            raise ValueError(f"labels has {len(labels)} entries for {len(clouds)} parts")
        self.parts = [c if isinstance(c, PointCloudRasterizer) else
                      PointCloudRasterizer(c, self.device, cells=cells, labels=None if labels is None else labels[s])
                      for s, c in enumerate(clouds)]
        self.counts = [r.n for r in self.parts]
        self.id_base = id_bases(self.counts)
        self.n = sum(self.counts)
        self.poses = [None] * len(self.parts)
        self.visible = [True] * len(self.parts)

    def part(self, s):
        """Part s's own rasteriser (set_object_pose / set_object_visible / add_instance of a part with object labels; foreign
        objects, add_object, are refused: the stitched gather has one descriptor table per part)."""
        return self.parts[self._index(s)]

    def _index(self, s):
        s = int(s)
        if not 0 <= s < len(self.parts):
            raise ValueError(f"no part {s}: parts 0..{len(self.parts) - 1}")
        return s

    def set_part_pose(self, s, P):
        """P (4x4, None = identity) maps part s's points, in its own coordinates, into the frame's; from the next frame enqueued."""
        self.poses[self._index(s)] = _pose(P)

    def set_part_visible(self, s, flag):
        self.visible[self._index(s)] = bool(flag)

    def part_matrices(self, total_m):
        M0 = _one_camera(total_m)
        return [object_matrix(M0, P) for P in self.poses]

    def render(self, total_m, W, H, levels=5, next_total=None, out=None):
        """-> one entry per part: (idx_levels, depth_levels) of LOCAL ids from that part's rasteriser, or None for a hidden part
        (not rasterised).  out: None or a list of per-part (idx, depth) buffers to fill.  next_total: the next call's camera, when
        known — every part is told object_matrix(next_total, P_s)."""
        for s, r in enumerate(self.parts):
            if r._foreign:
                raise NotImplementedError(f"foreign objects (add_object) in part {s} of a stitched frame: the stitched gather has one "
                                          "descriptor table per part")
        Ms = self.part_matrices(total_m)
        Mn = None if next_total is None else self.part_matrices(next_total)
        frames = []
        for s, r in enumerate(self.parts):
            if not self.visible[s]:
                frames.append(None)
                continue
            frames.append(r.render(Ms[s], W, H, levels, out=None if out is None else out[s],
                                   next_total=None if Mn is None else Mn[s]))
        return frames

    def gather_parts(self, frames, tables=None):
        """The ``parts`` argument of stitch_gather_pyramid for ``render``'s result; tables: per part (rows, activation), or None
        for an ids-only merge."""
        return [(self.counts[s] if tables is None else tables[s][0], None if f is None else f[0], None if f is None else f[1],
                 self.id_base[s], 'none' if tables is None else tables[s][1]) for s, f in enumerate(frames)]

    def render_merged(self, total_m, W, H, levels=5, next_total=None, want_depth=True, want_part=False, out=None):
        """The merged frame without features: (idx_levels, depth_levels | None[, part_levels]) of GLOBAL ids, the images a
        PointCloudRasterizer over the concatenated cloud returns when every placement is the identity."""
        frames = self.render(total_m, W, H, levels, next_total)
        if out is None:
            sizes = level_sizes(W, H, levels)
            out = {'index': [torch.empty((1, h, w), dtype=torch.int32, device=self.device) for (w, h) in sizes]}
        res = stitch_gather_pyramid(self.gather_parts(frames), out=out, want_index=True, want_depth=want_depth,
                                    want_part=want_part, want_feat=False)
        idx = res[1]
        dep = res[2] if want_depth else None
        return (idx, dep, res[-1]) if want_part else (idx, dep)


class StitchedFrameRenderer:
    """FrameRenderer for a stitched frame: rasterise every part, one stitched gather, the UNet.

    parts: list of dicts {xyz, texture_cn, pose=None, object_labels=None, activation='none'} (1..8); the other arguments as
    FrameRenderer's.  Frames run one at a time on the caller's stream.  merged_images: also keep the merged index / depth / part
    images of the last frame in ``idx`` / ``depth`` / ``part_image`` (9 more bytes per pixel and level)."""

    def __init__(self, parts, unet_state, W, H, proj_matrix=None, device=None, levels=LEVELS, cells=True, frames_in_flight=1,
                 merged_images=False):
        if frames_in_flight != 1:
            raise ValueError(f"frames_in_flight={frames_in_flight}: stitched frames run one at a time")
        if not 1 <= len(parts) <= MAX_PARTS:
            raise ValueError(f"a stitched frame has 1..{MAX_PARTS} parts, got {len(parts)}")
        self.device = device if device is not None else _lib.require_gpu()
        if W % 16 or H % 16:
            raise ValueError(f"set width {16 * (W // 16)} / height {16 * (H // 16)}")    # READ/gl/nn.py:107-109
        self.W, self.H, self.levels = W, H, levels
        for s, p in enumerate(parts):
            n, cols = int(np.shape(p['xyz'])[0]), int(torch.as_tensor(p['texture_cn']).shape[-1])
            if n != cols:
                raise ValueError(f"part {s}: descriptor table has {cols} columns for a cloud of {n} points")
            if p.get('activation', 'none') not in _ACT:
                raise ValueError(f"part {s}: activation {p['activation']!r}")
        self.raster = StitchedRasterizer([p['xyz'] for p in parts], self.device, cells=cells,
                                         labels=[p.get('object_labels') for p in parts])
        self.tables = [(texture_to_rows(torch.as_tensor(p['texture_cn'], dtype=torch.float32).to(self.device).contiguous()),
                        p.get('activation', 'none')) for p in parts]
        if len({int(t[0].shape[1]) for t in self.tables}) != 1:
            raise ValueError("the parts' descriptor tables differ in their channel count")
        for s, p in enumerate(parts):
            self.raster.set_part_pose(s, p.get('pose'))
        self.packed, self.unet = unet_engine(unet_state, self.device, H, W)
        self.proj = None if proj_matrix is None else np.asarray(proj_matrix, np.float32)
        sizes = level_sizes(W, H, levels)
        img = lambda dtype, tail=(): [torch.empty((1, h, w) + tail, dtype=dtype, device=self.device) for (w, h) in sizes]
        self._part_out = [(img(torch.int32), img(torch.float32)) for _ in parts]
        self.feat = img(torch.float32, (int(self.tables[0][0].shape[1]),))
        self.merged_images = bool(merged_images)
        self.idx = img(torch.int32) if merged_images else None
        self.depth = img(torch.float32) if merged_images else None
        self.part_image = img(torch.uint8) if merged_images else None
        self.rgba = torch.empty((H, W, 4), dtype=torch.float32, device=self.device)
        self._frames = None
        self.frame_done = None

    def set_part_pose(self, s, P):
        self.raster.set_part_pose(s, P)

    def set_part_visible(self, s, flag):
        self.raster.set_part_visible(s, flag)

    def part(self, s):
        return self.raster.part(s)

    def rasterize(self, total_m, next_total=None):
        self._frames = self.raster.render(total_m, self.W, self.H, self.levels, next_total=next_total, out=self._part_out)
        return self._frames

    def gather(self):
        if self._frames is None:
            raise ValueError("gather() before rasterize()")
        m = self.merged_images
        out = {'feat': self.feat, 'index': self.idx, 'depth': self.depth, 'part': self.part_image}
        stitch_gather_pyramid(self.raster.gather_parts(self._frames, self.tables), out=out, want_index=m, want_depth=m, want_part=m)
        return self.feat

    def refine(self, out=None, channels=4):
        f = self.feat
        return self.unet.forward(f[0][0], f[1][0], f[2][0], f[3][0], out=self.rgba if out is None else out, channels=channels)

    def render_total(self, total_m, out=None, channels=4, next_total=None):
        """total_m = proj @ inv(view) (4x4 fp32, = M_0) -> (H,W,channels) fp32 frame on the device, on the caller's stream."""
        self.rasterize(total_m, next_total)
        self.gather()
        return self.refine(out, channels)

    def render(self, view_matrix, proj_matrix=None, out=None, channels=4):
        """view_matrix: camera->world 4x4 (the reference's convention); -> H x W x 4 RGBA (alpha = 1)."""
        proj = self.proj if proj_matrix is None else np.asarray(proj_matrix, np.float32)
        if proj is None:
            raise ValueError("no projection matrix set")
        return self.render_total(total_matrix(proj, view_matrix), out, channels)

    def sync(self):
        """Nothing is in flight beyond the caller's stream (the counterpart of FrameRenderer.sync)."""
