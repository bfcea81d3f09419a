"""Rasteriser front ends with the reference's interfaces.

``MyRender``          src/READ/gl/myrender.py:12-43  (headless training path; global in src/train.py:596-598)
``Scene``             the camera/cloud state of READ/gl/programs.py::NNScene that the render path reads
``MultiscaleRender``  READ/datasets/dynamic.py:50-99  (viewer / dataset path; GL FBOs replaced by the HIP splat)

``uv_1d_p1[_dsK]`` tokens (point ids, 1-px points: the layout TexturePipeline trains and renders with) take the single-pass
pyramid rasteriser.  Every other token of the input-format DSL (READ/gl/dataset.py:39-82) that makes sense for a point cloud
— ``pN`` point sizes, ``psN`` perspective splats, ``colors``, ``normals_{m,r,l,d}``, ``xyz``, ``depth``, ``labels`` — plus
the dataset augmentations ``set_point_discard`` / ``set_point_perturb`` (READ/gl/programs.py:347-357) is rendered level by
level through ``read_splat_forward_gl`` (the GL twin restated in oracle/raster.c): the z-buffer decides the winning point
of every pixel, the vertex colour of that point (programs.py:133-181, flat shading) is looked up on the device.  Tokens
that need triangles (no ``p``: mesh rendering, ``uv_2d`` mesh textures) and per-point size arrays raise
NotImplementedError.
"""
import re

import numpy as np
import torch

from . import _lib
from .camera import lens_camera, level_sizes, pano_camera, total_matrix
from .raster import PointCloudRasterizer, index_to_float


MODE_COLOR, MODE_NORMALS, MODE_DEPTH, MODE_UV, MODE_XYZ, MODE_LABEL = 0, 1, 2, 3, 4, 5      # NNScene.MODE_* (programs.py:16-21)
UV_TYPE_1D, UV_TYPE_2D = 0, 1
_NORMALS = ('normals_m', 'normals_r', 'normals_l', 'normals_d')


def parse_input_string(string):
    """The input-format DSL of READ/gl/dataset.py:39-82: ``<what>[_<variant>][_pN|_psN][_dsK]``.
    -> {'mode': (mode0, mode1), 'draw_points', 'flat_color', 'point_size', 'splat_mode'[, 'downscale']}."""
    config = {}
    if re.search('^colors', string):
        config['mode'] = (MODE_COLOR, None)
    elif re.search('^uv', string):
        kinds = re.findall('uv_1d|uv_2d', string)
        if not kinds:
            raise ValueError(string)
        config['mode'] = (MODE_UV, UV_TYPE_1D if kinds[-1] == 'uv_1d' else UV_TYPE_2D)
    elif re.search('^normals', string):
        kinds = re.findall('|'.join(_NORMALS), string)
        if not kinds:
            raise ValueError(string)
        config['mode'] = (MODE_NORMALS, _NORMALS.index(kinds[-1]))
    elif re.search('^xyz', string):
        config['mode'] = (MODE_XYZ, None)
    elif re.search('^depth', string):
        config['mode'] = (MODE_DEPTH, None)
    elif re.search('^labels', string):
        config['mode'] = (MODE_LABEL, None)
    else:
        raise ValueError(string)
    sizes = re.findall('ps[0-9]+|p[0-9]+', string)
    config['draw_points'] = config['flat_color'] = bool(sizes)
    config['point_size'] = int(re.search('[0-9]+', sizes[-1]).group()) if sizes else 1
    config['splat_mode'] = bool(sizes) and sizes[-1].startswith('ps')
    scales = re.findall('ds[0-5]+', string)
    if scales:
        config['downscale'] = int(re.search('[0-9]+', scales[-1]).group())
    return config


_WHAT = {MODE_COLOR: 'colors', MODE_UV: 'uv', MODE_NORMALS: 'normals', MODE_XYZ: 'xyz', MODE_DEPTH: 'depth', MODE_LABEL: 'labels'}
_VARIANT = {MODE_UV: ('_1d', '_2d'), MODE_NORMALS: ('_m', '_r', '_l', '_d')}


def generate_input_string(config):
    """Inverse of ``parse_input_string`` (READ/gl/dataset.py:85-122): a draw configuration -> its token,
    ``<what>[_<variant>][_p<N>|_ps<N>][_ds<K>]``.  An unknown uv type raises ValueError like the reference; an unknown normals
    variant is left out like the reference.  ``MODE_LABEL`` gives ``labels`` (the reference function has no branch for it and
    returns a token that does not parse), so ``parse(generate(c)) == c`` holds for every mode ``parse_input_string`` knows."""
    m0, m1 = config['mode']
    s = _WHAT.get(m0, '')
    if m0 == MODE_UV:
        if m1 not in (UV_TYPE_1D, UV_TYPE_2D):
            raise ValueError
        s += _VARIANT[MODE_UV][m1]
    elif m0 == MODE_NORMALS and m1 in (0, 1, 2, 3):
        s += _VARIANT[MODE_NORMALS][m1]
    if config['draw_points']:
        s += ('_ps' if config['splat_mode'] else '_p') + str(config['point_size'])
    if 'downscale' in config:
        s += f"_ds{config['downscale']}"
    return s


def is_point_id_pyramid(input_format):
    """True when the tokens are exactly ``uv_1d_p1`` at downscale 0, 1, 2, ... — the layout served by ONE pass over the
    cloud (pyramid identity)."""
    try:
        cfgs = [parse_input_string(t) for t in input_format.replace(' ', '').split(',')]
    except (ValueError, NotImplementedError):
        return False
    return all(c['mode'] == (MODE_UV, UV_TYPE_1D) and c['draw_points'] and c['point_size'] == 1 and not c['splat_mode']
               and c.get('downscale', 0) == i for i, c in enumerate(cfgs))


class MyRender:
    """Same constructor / update_ds / render contract as src/READ/gl/myrender.py.

    ``render(data)`` returns ``(out_dict, depth_dict)``: ``out_dict['id']`` plus one (B,1,h,w) float32
    tensor per input_format token (scale = position in the list, myrender.py:32).  Tensors are CPU
    tensors like the reference's unless ``device_outputs=True`` (then they stay in HBM, int32 ids
    available as ``last_index``)."""

    def __init__(self, ds_list=None, device_outputs=False):
        self.device_outputs = device_outputs
        self.rasterizers = {}
        if ds_list:
            self.update_ds(ds_list)

    def update_ds(self, ds_list):
        self.ds_list = ds_list
        self.ds_ids = [d.id for d in ds_list]
        self.tgt_sh = self.ds_list[0].tgt_sh
        self.rasterizers = {ds.id: PointCloudRasterizer(np.asarray(ds.scene_data['pointcloud']['xyz'], np.float32))
                            for ds in ds_list}

    def render(self, data):
        input_format = self.ds_list[0].input_format.replace(' ', '').split(',')
        ids = data['input']['id']
        ids_t = torch.as_tensor(ids)
        B = len(ids)
        W, H = int(self.tgt_sh[0]), int(self.tgt_sh[1])
        levels = len(input_format)
        proj = data['proj_matrix'].numpy() if torch.is_tensor(data['proj_matrix']) else np.asarray(data['proj_matrix'])
        view = data['view_matrix'].numpy() if torch.is_tensor(data['view_matrix']) else np.asarray(data['view_matrix'])
        tm = total_matrix(proj, view)                                          # myrender.py:28-30
        dev = _lib.require_gpu()
        sizes = level_sizes(W, H, levels)
        if len(self.ds_ids) == 1 and bool((ids_t == self.ds_ids[0]).all()):
            # one scene (the usual batch): the rasteriser's outputs ARE the batch — no index tensors on the device, no copies
            # (a host -> device copy of a pageable tensor blocks the host until the stream has drained: ten of them per call
            # serialised the training loop's host and device sides)
            index, depth = self.rasterizers[self.ds_ids[0]].render(tm, W, H, levels)
            index, depth = list(index), list(depth)
        else:
            index = [torch.zeros((B, h, w), dtype=torch.int32, device=dev) for (w, h) in sizes]
            depth = [torch.zeros((B, h, w), dtype=torch.float32, device=dev) for (w, h) in sizes]
            for ds_id in self.ds_ids:
                sel = torch.where(ids_t == ds_id)[0]
                if sel.numel() == 0:
                    continue
                i_l, d_l = self.rasterizers[ds_id].render(tm[sel.numpy()], W, H, levels)
                sel_d = sel.to(dev)
                for l in range(levels):
                    index[l][sel_d] = i_l[l]
                    depth[l][sel_d] = d_l[l]
        self.last_index = index
        out_dict, depth_dict = {'id': ids}, {}
        for l, k in enumerate(input_format):
            f = index_to_float(index[l]).unsqueeze(1)
            d = depth[l].unsqueeze(1)
            out_dict[k] = f if self.device_outputs else f.cpu()
            depth_dict[k] = d if self.device_outputs else d.cpu()
        return out_dict, depth_dict


class Scene:
    """Camera + cloud state with NNScene's setter names (READ/gl/programs.py:300-415), no GL: positions and the
    per-point attributes the vertex shader reads, the discard / perturb augmentation buffers, the draw parameters
    ``set_params(**parse_input_string(token))`` sets."""

    # the mode constants callers reach through the class (``NNScene.MODE_UV`` ..., READ/gl/programs.py:61-75)
    MODE_COLOR, MODE_NORMALS, MODE_DEPTH, MODE_UV, MODE_XYZ, MODE_LABEL = (MODE_COLOR, MODE_NORMALS, MODE_DEPTH, MODE_UV,
                                                                            MODE_XYZ, MODE_LABEL)
    NORMALS_MODE_MODEL, NORMALS_MODE_REFLECTION, NORMALS_MODE_LOCAL, NORMALS_MODE_DIRECTION, NORMALS_MODE_RAW = 0, 1, 2, 3, 4
    UV_TYPE_1D, UV_TYPE_2D = UV_TYPE_1D, UV_TYPE_2D

    def __init__(self, xyz=None, flat_color=True):
        self.model_matrix = np.eye(4, dtype=np.float32)
        self.view_matrix = np.eye(4, dtype=np.float32)        # camera -> world
        self.proj_matrix = np.eye(4, dtype=np.float32)
        self._raster = None
        self._dirty = True
        self.xyz = None
        self.colors = self.normals = None
        self._dev = {}
        self.point_discard = None         # bool (N,)  set_point_discard  (programs.py:347-351)
        self.point_perturb = None         # float (N,2) set_point_perturb (programs.py:353-357)
        self.point_sizes = None           # float (N,) set_point_sizes (programs.py:339-345)
        self.point_drop = None            # (p, seed): seeded drop evaluated on the device
        self.point_perturb_seeded = None  # (amp, seed)
        self.object_labels = None         # scene editing (extension): int (N,) labels, 0 = static
        self.object_poses = {}            # label -> 4x4
        self.object_hidden = set()        # labels not drawn
        self.panorama = None              # set_panorama: horizontal field in degrees of the cylindrical camera, None = pinhole
        self.lens = None                  # set_lens: (model, coeffs, limit) of the lens camera, None = the ideal pinhole
        self.foreign_objects = []         # scene editing, add: [(xyz (m,3), PointTexture)] of add_foreign_object, in order
        self.instances = {}               # handle -> {'k', 'P', 'visible'} of add_object_instance, replayed into a rebuilt rasteriser
        self._next_instance = 0
        self.params = {'mode': (MODE_UV, UV_TYPE_1D), 'draw_points': True, 'flat_color': True, 'point_size': 1,
                       'splat_mode': False}
        if xyz is not None:
            self.set_vertices(xyz)

    def set_vertices(self, positions, colors=None, normals=None, uv1d=None, uv2d=None, texture=None):
        positions = np.asarray(positions)
        for name, a in (('colors', colors), ('normals', normals), ('uv1d', uv1d), ('uv2d', uv2d)):
            assert a is None or positions.shape[0] == np.asarray(a).shape[0], 'arrays must have the same shape[0]'
        self.xyz = np.ascontiguousarray(positions, dtype=np.float32)
        self.colors = None if colors is None else np.ascontiguousarray(colors, dtype=np.float32)
        self.normals = None if normals is None else np.ascontiguousarray(normals, dtype=np.float32)
        if uv1d is not None and not np.array_equal(np.asarray(uv1d).reshape(-1), np.arange(positions.shape[0])):
            raise NotImplementedError("uv1d other than the point index (import_model3d's arange) is not supported")
        self.xyz_min, self.xyz_max = self.xyz.min(axis=0), self.xyz.max(axis=0)          # programs.py:334-335
        self.point_discard = self.point_perturb = self.point_sizes = None
        self.object_labels, self.object_poses, self.object_hidden = None, {}, set()
        self.foreign_objects, self.instances = [], {}
        self._dev = {}
        self._dirty = True

    def set_object_labels(self, labels):
        """Extension (not in NNScene): one object label per point (0 = the static scene, k >= 1 = object k), None = no objects.
        Objects are moved by ``set_object_pose`` and hidden by ``set_object_visible`` without rebuilding anything; new labels
        rebuild the rasteriser.  The point-id pyramid (OGL.infer's fast path, MultiscaleRender's id tokens) honours the edits;
        every other token raises NotImplementedError while objects are set."""
        if labels is not None:
            labels = np.ascontiguousarray(labels).reshape(-1)
            if self.xyz is None or labels.shape[0] != self.xyz.shape[0]:
                raise ValueError(f"labels has {labels.shape[0]} entries for {0 if self.xyz is None else self.xyz.shape[0]} points")
        K_old = self._own_objects()
        self.object_labels = labels
        self.object_poses, self.object_hidden = {}, set()
        # foreign objects follow the labels (k = K + 1 + ordinal), so their instances move with them; an instance of an own label
        # that no longer exists is dropped
        K = self._own_objects()
        kept = {}
        for h, inst in self.instances.items():
            if inst['k'] > K_old:
                kept[h] = dict(inst, k=inst['k'] - K_old + K)
            elif inst['k'] <= K:
                kept[h] = inst
        self.instances = kept
        self._dirty = True

    def set_object_pose(self, k, P):
        """Extension: P (4x4, None = identity) maps object k's points, in the cloud's coordinates, to their new place; it is
        applied before the model matrix (M_k = proj @ inv(view) @ model @ P)."""
        self._require_objects()
        if self._raster is not None and not self._dirty:
            self._raster.set_object_pose(k, P)
        if P is None:
            self.object_poses.pop(int(k), None)
        else:
            self.object_poses[int(k)] = np.array(P, np.float32).reshape(4, 4)

    def set_object_visible(self, k, flag):
        """Extension: hide (False) or show object k."""
        self._require_objects()
        if self._raster is not None and not self._dirty:
            self._raster.set_object_visible(k, flag)
        (self.object_hidden.discard if flag else self.object_hidden.add)(int(k))

    def _require_objects(self):
        if self.object_labels is None:
            raise ValueError("no object labels set (set_object_labels)")

    def edited(self):
        return self.object_labels is not None or bool(self.foreign_objects) or bool(self.instances)

    # ---- scene editing, third verb: add (PointCloudRasterizer.add_object / add_instance) -----------------------------------
    def _own_objects(self):
        return 0 if self.object_labels is None or self.object_labels.size == 0 else int(self.object_labels.max())

    def _live_raster(self):
        return self._raster if self._raster is not None and not self._dirty else None

    def has_foreign(self):
        return bool(self.foreign_objects)

    def extract_object(self, k):
        """-> (xyz (m,3) float32, ids (m,) int64) of object k: the points of label k with their ids in this scene — what
        ``add_foreign_object`` of ANOTHER scene takes, with the rows ``ids`` of this scene's descriptor table as its texture."""
        self._require_objects()
        ids = np.flatnonzero(self.object_labels == int(k))
        if not 1 <= int(k) <= self._own_objects():
            raise ValueError(f"no object {k}: labels 1..{self._own_objects()}")
        return self.xyz[ids].copy(), ids

    def add_foreign_object(self, xyz, texture):
        """Extension: an object that is not part of this cloud — m points with their own descriptors, a ``PointTexture`` of size m
        (its own activation).  Its ids follow the scene's: id_base = N for the first, each next one after the previous.  -> k,
        continuing the label numbering (new labels renumber it to follow them).  It is drawn once per ``add_object_instance``."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        if self.xyz is None:
            raise ValueError("scene has no point cloud (set_vertices)")
        if xyz.ndim != 2 or xyz.shape[1] != 3 or xyz.shape[0] < 1:
            raise ValueError(f"a foreign object is (m,3) points with m >= 1, got {xyz.shape}")
        if not hasattr(texture, 'texture_') or int(texture.texture_.shape[-1]) != xyz.shape[0]:
            raise ValueError(f"a foreign object of {xyz.shape[0]} points takes a PointTexture of that size")
        self.foreign_objects.append((xyz, texture))
        r = self._live_raster()
        if r is not None:
            r.add_object(xyz)
        return self._own_objects() + len(self.foreign_objects)

    def add_object_instance(self, k, P=None, visible=True):
        """Extension: one more copy of object k (a label, or a foreign object) placed by P (4x4, None = identity; applied before
        the model matrix, like set_object_pose).  -> a handle.  Nothing is rebuilt."""
        k = int(k)
        if not 1 <= k <= self._own_objects() + len(self.foreign_objects):
            raise ValueError(f"no object {k}: objects 1..{self._own_objects() + len(self.foreign_objects)}")
        h = self._next_instance
        self._next_instance += 1
        inst = {'k': k, 'P': None if P is None else np.array(P, np.float32).reshape(4, 4), 'visible': bool(visible)}
        r = self._live_raster()
        if r is not None:
            inst['raster'] = r.add_instance(k, inst['P'], inst['visible'])
        self.instances[h] = inst
        return h

    def _scene_instance(self, handle):
        if handle not in self.instances:
            raise ValueError(f"no instance {handle!r}")
        return self.instances[handle]

    def set_instance_pose(self, handle, P):
        inst = self._scene_instance(handle)
        inst['P'] = None if P is None else np.array(P, np.float32).reshape(4, 4)
        if self._live_raster() is not None:
            self._raster.set_instance_pose(inst['raster'], inst['P'])

    def set_instance_visible(self, handle, flag):
        inst = self._scene_instance(handle)
        inst['visible'] = bool(flag)
        if self._live_raster() is not None:
            self._raster.set_instance_visible(inst['raster'], flag)

    def remove_instance(self, handle):
        inst = self._scene_instance(handle)
        if self._live_raster() is not None:
            self._raster.remove_instance(inst['raster'])
        del self.instances[handle]

    def gather_tables(self, texture):
        """[(rows, id_base, activation)] for texture.gather_tables_pyramid: the scene's table, then every foreign object's, each
        checked against the rasteriser's id ranges."""
        ranges = self.rasterizer().id_ranges()
        tables = []
        for t, ((base, n), tex) in enumerate(zip(ranges, [texture] + [f[1] for f in self.foreign_objects])):
            if int(tex.texture_.shape[-1]) != n:
                what = "the scene cloud" if t == 0 else f"foreign object {t}"
                raise ValueError(f"descriptor table {t} has {int(tex.texture_.shape[-1])} points, {what} {n}")
            if not tex.texture_.is_cuda:
                tex.cuda()
            tables.append((tex.rows(), base, tex.activation))
        return tables

    def set_point_sizes(self, point_sizes):
        """Per-point sizes (READ/gl/programs.py:339-345, scene yaml 'point_sizes'): from now on every token is drawn with the
        point's own size instead of the token's N — the reference sets global_point_size to 0 and set_params skips
        'point_size' (programs.py:404-406); "ps" tokens still divide by clip z."""
        ps = np.ascontiguousarray(point_sizes, dtype=np.float32).reshape(-1)
        if self.xyz is not None and ps.shape[0] != self.xyz.shape[0]:
            raise ValueError(f"point_sizes has {ps.shape[0]} entries for {self.xyz.shape[0]} points")
        self.point_sizes = ps

    def set_point_discard(self, arr):
        self.point_discard = None if arr is None else np.ascontiguousarray(arr).astype(bool)

    def set_point_perturb(self, arr):
        self.point_perturb = None if arr is None else np.ascontiguousarray(arr, dtype=np.float32).reshape(-1, 2)

    def set_point_drop(self, p, seed=0):
        """Seeded form of ``set_point_discard(np.random.rand(N) < p)`` (READ/datasets/dynamic.py:235-236): evaluated on
        the device from a hash of (point id, seed), restated bit for bit by oracle.drop_mask."""
        self.point_drop = (float(p), int(seed)) if p else None

    def set_point_perturb_seeded(self, amp, seed=0):
        """Seeded form of ``set_point_perturb(amp * (rand(N,2) - 0.5))`` (dynamic.py:176-179,238-239)."""
        self.point_perturb_seeded = (float(amp), int(seed)) if amp else None

    def set_model_view(self, m):
        self.model_matrix = np.asarray(m, np.float32)

    def set_camera_view(self, m):
        """m: camera->world pose (viewer.py:264); the GL scene stores inv(m).T, we keep m."""
        self.view_matrix = np.asarray(m, np.float32)

    def announce_next_camera_view(self, m):
        """Extension (not in NNScene): the pose the NEXT frame will be rendered from, when the caller knows it — a trajectory replay,
        a sweep, a viewer that extrapolates its camera.  The rasteriser then prepares that frame inside this frame's last launch
        (PointCloudRasterizer.render(next_total=...)); a wrong announcement costs two small memsets, never a wrong pixel.
        Consumed by the next render; None withdraws it."""
        self.next_view_matrix = None if m is None else np.asarray(m, np.float32)

    def take_next_total_matrix(self):
        m = getattr(self, 'next_view_matrix', None)
        self.next_view_matrix = None
        if m is None:
            return None
        return (self.proj_matrix @ np.linalg.inv(m.astype(np.float32)) @ self.model_matrix).astype(np.float32)[None]

    def set_proj_matrix(self, m):
        self.proj_matrix = np.asarray(m, np.float32)

    def set_panorama(self, hfov_deg):
        """Extension (not in NNScene): a cylindrical camera with a horizontal field of hfov_deg in (0, 360] at the current view;
        None returns to the pinhole.  ``OGL.infer`` stays on its fast path and rasterises with
        ``PointCloudRasterizer.render_pano``; of the projection matrix only the vertical scale / offset and the depth entries
        are used (camera.pano_camera).  Object edits apply; an announced next camera is ignored; everything that is not the
        point-id pyramid on the fast path raises NotImplementedError while a panorama is set."""
        if hfov_deg is not None and not 0.0 < float(hfov_deg) <= 360.0:
            raise ValueError(f"hfov_deg must lie in (0, 360], got {hfov_deg!r}")
        if hfov_deg is not None and self.lens is not None:
            raise ValueError("set_panorama with a lens camera set (set_lens): a scene has one camera; set_lens(None) first")
        self.panorama = None if hfov_deg is None else float(hfov_deg)

    def pano_camera(self):
        """The 16 floats of camera.pano_camera for the current view, model and projection matrices (points are taken to the
        camera by inv(view) @ model, as in ``total_matrix``)."""
        if self.panorama is None:
            raise ValueError("no panorama set (set_panorama)")
        view = np.linalg.inv(self.model_matrix.astype(np.float64)) @ self.view_matrix.astype(np.float64)
        return pano_camera(self.proj_matrix, view, self.panorama)

    def set_lens(self, model, coeffs=None, limit=None):
        """Extension (not in NNScene): the scene's camera gets a lens at the current view — model 0 a pinhole with Brown-Conrady
        distortion (coeffs = OpenCV's k1, k2, p1, p2, k3), model 1 a Kannala-Brandt fisheye (coeffs = OpenCV's fisheye k1..k4);
        ``set_lens(None)`` returns to the ideal pinhole.  limit as in camera.lens_camera (None: just inside where the distortion
        folds back; smaller: a field mask).  ``OGL.infer`` stays on its fast path and rasterises with
        ``PointCloudRasterizer.render_lens``, and ``MultiscaleRender.render`` serves the point-id pyramid under the lens, so a
        scene is fitted through it as through the pinhole.  Object edits apply; an announced next camera is ignored; everything
        that is not the point-id pyramid raises NotImplementedError while a lens is set."""
        if model is None:
            self.lens = None
            return
        if self.panorama is not None:
            raise ValueError("set_lens with a panorama camera set (set_panorama): a scene has one camera; set_panorama(None) first")
        coeffs = () if coeffs is None else tuple(float(c) for c in np.asarray(coeffs, np.float64).reshape(-1))
        lens_camera(np.eye(4), np.eye(4), model, coeffs, limit)                  # the checks of camera.lens_camera, now
        self.lens = (int(model), coeffs, None if limit is None else float(limit))

    def lens_camera(self):
        """The 32 floats of camera.lens_camera for the current view, model and projection matrices (points are taken to the
        camera by inv(view) @ model, as in ``total_matrix``)."""
        if self.lens is None:
            raise ValueError("no lens set (set_lens)")
        view = np.linalg.inv(self.model_matrix.astype(np.float64)) @ self.view_matrix.astype(np.float64)
        return lens_camera(self.proj_matrix, view, *self.lens)

    def lidar_sweep(self, sensor, view_matrix=None):
        """Extension (not in NNScene): one sweep of the ``lidar.LidarSensor`` placed at ``view_matrix`` (sensor -> world; None =
        the scene's camera view) -> a ``lidar.LidarSweep``: range image, point ids and the return list, with the current object
        edits.  Points are taken to the sensor by inv(view) @ model, as in ``pano_camera``; the LiDAR is a sensor of its own, so
        the projection matrix, ``set_panorama`` and ``set_lens`` play no part."""
        if self.xyz is None:
            raise ValueError("scene has no point cloud (set_vertices)")
        if self.augmented():
            raise NotImplementedError("GL-twin augmentation (point sizes, discard, drop, perturb) with lidar_sweep: a sweep ranges "
                                      "the cloud's points as they are")
        view = self.view_matrix if view_matrix is None else np.asarray(view_matrix, np.float32)
        view = np.linalg.inv(self.model_matrix.astype(np.float64)) @ view.astype(np.float64)
        return self.rasterizer().sweep_lidar(sensor, sensor.camera(view))

    def set_use_light(self, use_light):
        if use_light:
            raise NotImplementedError("the viewer's lighting pass is not part of the render path")

    def set_params(self, skip=(), **kwargs):
        """programs.py:404-416: every key with a setter is applied; here the draw parameters are simply recorded."""
        for k, v in kwargs.items():
            if k not in skip:
                self.params[k] = v

    def delete(self):
        """NNScene.delete() (READ/gl/programs.py; DynamicDataset.unload, dynamic.py:181-183): drop the device copies."""
        self._raster = None
        self._dev = {}
        self._dirty = True

    def augmented(self):
        return (self.point_discard is not None or self.point_perturb is not None or self.point_drop is not None
                or self.point_perturb_seeded is not None or self.point_sizes is not None)

    def device_array(self, name):
        """colors / normals / xyz as (N,3) CUDA tensors, uploaded on first use."""
        if name not in self._dev:
            a = getattr(self, name)
            if a is None:
                a = np.zeros((self.xyz.shape[0], 3), np.float32)        # programs.py:326-327: missing attributes are zeros
            self._dev[name] = torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(_lib.require_gpu())
        return self._dev[name]

    def rasterizer(self):
        if self._raster is None or self._dirty:
            if self.xyz is None:
                raise ValueError("scene has no point cloud (set_vertices)")
            self._raster = PointCloudRasterizer(self.xyz, labels=self.object_labels)
            for k, P in self.object_poses.items():
                self._raster.set_object_pose(k, P)
            for k in self.object_hidden:
                self._raster.set_object_visible(k, False)
            for xyz, _ in self.foreign_objects:
                self._raster.add_object(xyz)
            for _, inst in sorted(self.instances.items()):
                inst['raster'] = self._raster.add_instance(inst['k'], inst['P'], inst['visible'])
            self._dirty = False
        return self._raster

    def total_matrix(self, view_matrix=None):
        # clip = P * inv(cam->world) * model * x   (programs.py:121-125 with column vectors); view_matrix: another camera -> world
        # pose in place of the scene's
        view = np.linalg.inv((self.view_matrix if view_matrix is None else np.asarray(view_matrix, np.float32)).astype(np.float32))
        return (self.proj_matrix @ view @ self.model_matrix).astype(np.float32)[None]

    # ---- object selection: where the labels come from (read_amd/select.py) --------------------------------
    def _selected(self, labels):
        from . import select
        n = select.counts(labels)
        self.set_object_labels(labels.cpu().numpy())
        return n

    def select_boxes(self, boxes, label_of=None, keep=False):
        """Extension: label the cloud on the device from K <= 1024 oriented boxes (``select.box_matrix``; (K,12) or (K,3,4)) — box k
        gives label_of[k] (default k + 1), the first box that contains a point wins, faces inclusive — and hand the result to
        ``set_object_labels``.  keep: start from the current labels instead of 0 (label 0 then carves points back into the static
        scene).  -> points per label (host int64, index = label)."""
        from . import select
        if self.xyz is None:
            raise ValueError("scene has no point cloud (set_vertices)")
        return self._selected(select.label_boxes(self.device_array('xyz'), boxes, label_of,
                                                 self.object_labels if keep else None))

    def select_masks(self, view_matrices, masks, viewport_size, rel=0.05, slack=0.0, min_hits=1, ratio=(1, 2), keep=False):
        """Extension: label the cloud on the device from 2-D label images (``masks[v]``: (H,W) ints, 0 = no object) seen from the
        camera -> world poses ``view_matrices[v]`` with the scene's projection and model matrices, viewport_size = (W, H), at most
        255 views.  Each view renders level 0 of the UNEDITED cloud, keeps the points within near * (1 + rel) + slack of their
        pixel's winner and votes (``select.MaskVotes``: the candidate is the label of the first view that names one); the result
        goes to ``set_object_labels``.  keep: points without a label keep their current one.  -> points per label."""
        from . import select
        if self.xyz is None:
            raise ValueError("scene has no point cloud (set_vertices)")
        if self.panorama is not None:
            raise NotImplementedError("a panorama camera (set_panorama) with select_masks: the occlusion window compares clip w, "
                                      "which is no depth under the cylindrical camera; select from pinhole views")
        if self.lens is not None:
            raise NotImplementedError("a lens camera (set_lens) with select_masks: the views are projected with the ideal pinhole; "
                                      "select from undistorted views")
        if self.augmented():
            raise NotImplementedError("GL-twin augmentation (point sizes, discard, drop, perturb) with select_masks: the views are "
                                      "level-0 frames of the plain cloud")
        if len(view_matrices) != len(masks):
            raise ValueError(f"{len(view_matrices)} view matrices for {len(masks)} masks")
        W, H = int(viewport_size[0]), int(viewport_size[1])
        votes = select.MaskVotes(self.device_array('xyz'))
        # the frames must carry the cloud's own ids under one matrix: the live rasteriser while nothing is edited, else a temporary
        # unlabelled one
        raster = self.rasterizer() if not self.edited() else PointCloudRasterizer(self.xyz)
        for view, mask in zip(view_matrices, masks):
            M = self.total_matrix(view)[0]
            idx, dep = raster.render(M, W, H, 1)
            votes.add_view(M, W, H, idx[0], dep[0], mask, rel, slack)
        labels = votes.labels(min_hits, ratio, self.object_labels if keep else None)
        del raster
        return self._selected(labels)


    # ---- frame annotations: what drew each pixel (read_amd/annotate.py) ------------------------------------
    def annotation_handle(self, handle):
        """The value ``Annotation.instances`` / ``.handles`` carry for the instance ``add_object_instance`` returned ``handle`` for
        (the live rasteriser's own handle).  Object k itself — the labelled points where they are — is k - 1."""
        self.rasterizer()
        return self._scene_instance(handle)['raster']

    def annotate_frame(self, viewport_size):
        """Extension: render level 0 with depth of the current camera and edits through the live rasteriser and annotate it -> an
        ``annotate.Annotation``: per pixel the object and the instance that drew it, per instance boxes and counts.  Pinhole
        frames of the 1-px point-id raster only."""
        if self.xyz is None:
            raise ValueError("scene has no point cloud (set_vertices)")
        if self.panorama is not None:
            raise NotImplementedError("a panorama camera (set_panorama) with annotate_frame: the instance match re-projects with the "
                                      "pinhole projection")
        if self.lens is not None:
            raise NotImplementedError("a lens camera (set_lens) with annotate_frame: the instance match re-projects with the "
                                      "pinhole projection")
        if self.augmented():
            raise NotImplementedError("GL-twin augmentation (point sizes, discard, drop, perturb) with annotate_frame: annotations "
                                      "describe the 1-px point-id frame")
        W, H = int(viewport_size[0]), int(viewport_size[1])
        raster = self.rasterizer()
        M = self.total_matrix()
        if M.shape[0] != 1:
            raise NotImplementedError("more than one camera with annotate_frame")
        idx, dep = raster.render(M, W, H, 1)
        return raster.annotate(M[0], W, H, idx[0], dep[0])

    # ---- frame flow: per-pixel motion between two edited frames (read_amd/flow.py) ---------------------------
    def capture_frame(self, viewport_size, level=0):
        """Extension: render level 0 with depth of the current camera and edits through the live rasteriser into tensors of its own
        and snapshot it with the instance list -> a ``flow.FrameState`` for ``flow_between``.  Pinhole frames of the 1-px point-id
        raster only."""
        if self.xyz is None:
            raise ValueError("scene has no point cloud (set_vertices)")
        if self.panorama is not None:
            raise NotImplementedError("a panorama camera (set_panorama) with capture_frame: the flow re-projects with the pinhole "
                                      "projection")
        if self.lens is not None:
            raise NotImplementedError("a lens camera (set_lens) with capture_frame: the flow re-projects with the pinhole projection")
        if self.augmented():
            raise NotImplementedError("GL-twin augmentation (point sizes, discard, drop, perturb) with capture_frame: the flow "
                                      "describes the 1-px point-id frame")
        if int(level) != 0:
            raise NotImplementedError(f"level {int(level)} with capture_frame: levels above 0 hold the 2x2 minima of level 0, not "
                                      "points drawn at their own pixel")
        W, H = int(viewport_size[0]), int(viewport_size[1])
        raster = self.rasterizer()
        M = self.total_matrix()
        if M.shape[0] != 1:
            raise NotImplementedError("more than one camera with capture_frame")
        idx, dep = raster.render(M, W, H, 1)
        return raster.frame_state(M[0], W, H, idx[0], dep[0])

    def flow_between(self, a, b):
        """Extension: the frame flow from ``capture_frame`` state a to state b -> a ``flow.FrameFlow``: per pixel of a's frame the
        motion of its surface point, its depth in b and whether it is still seen; per instance the counts
        (``annotation_handle`` maps the scene's handles).  Camera moves, poses, visibility, added and removed instances between
        the two captures are followed; what rebuilds the rasteriser (new labels, a new cloud, a new foreign object) is refused
        with ValueError."""
        from . import flow as fl
        return fl.flow_between(a, b)


class StitchedScene:
    """Extension (not in NNScene): several ``Scene`` objects ("parts", 1..8) drawn into one frame — scene stitching
    (read_amd/stitch.py).  Part s is placed by ``set_part_pose(s, P)`` (M_s = M_0 @ P_s, P None = identity) and hidden or shown by
    ``set_part_visible``; neither rebuilds anything.  The camera setters fan out to every part, and the frame's camera M_0 is
    part 0's.  Object edits of a part go through that part's own ``Scene`` (``scenes[s].set_object_pose`` ...).  Merged point ids
    are id_base[s] + local id, id_base[s] = the point count of the parts before s, hidden ones included."""

    stitched = True

    def __init__(self, scenes, poses=None):
        scenes = list(scenes)
        if not 1 <= len(scenes) <= 8:
            raise ValueError(f"a stitched frame has 1..8 parts, got {len(scenes)}")
        if poses is not None and len(poses) != len(scenes):
            raise ValueError(f"poses has {len(poses)} entries for {len(scenes)} parts")
        self.scenes = scenes
        self.part_poses = [None] * len(scenes)
        self.part_hidden = set()
        self._raster = None
        for s, P in enumerate(poses or ()):
            self.set_part_pose(s, P)

    def _index(self, s):
        s = int(s)
        if not 0 <= s < len(self.scenes):
            raise ValueError(f"no part {s}: parts 0..{len(self.scenes) - 1}")
        return s

    def counts(self):
        return [0 if sc.xyz is None else int(sc.xyz.shape[0]) for sc in self.scenes]

    def id_base(self):
        """First merged id of every part: the counts of the parts before it, whether or not they are visible."""
        c = self.counts()
        return [sum(c[:s]) for s in range(len(c))]

    def joint_texture(self, textures):
        """The parts' PointTextures (one per part, in part order) as ONE ``JointTexture`` over this scene's merged ids — what
        NetAndTexture looks up and trains with the id pyramid MultiscaleRender draws of this scene."""
        from .texture import JointTexture
        textures = list(textures)
        counts = self.counts()
        if len(textures) != len(counts):
            raise ValueError(f"{len(textures)} textures for {len(counts)} parts")
        for s, (tex, n) in enumerate(zip(textures, counts)):
            if not hasattr(tex, 'num_ids') or tex.num_ids() != n:
                have = tex.num_ids() if hasattr(tex, 'num_ids') else type(tex).__name__
                raise ValueError(f"part {s}: a descriptor table whose size does not match: the table has {have} points, the "
                                 f"part's cloud {n}")
        return JointTexture(textures, self.id_base())

    def set_part_pose(self, s, P):
        s = self._index(s)
        self.part_poses[s] = None if P is None else np.array(P, np.float32).reshape(4, 4)
        if self._raster is not None:
            self._raster.set_part_pose(s, self.part_poses[s])

    def set_part_visible(self, s, flag):
        s = self._index(s)
        (self.part_hidden.discard if flag else self.part_hidden.add)(s)
        if self._raster is not None:
            self._raster.set_part_visible(s, flag)

    def part_visible(self, s):
        return self._index(s) not in self.part_hidden

    # ---- the camera state of every part moves together ---------------------------------------------------------------------
    def set_camera_view(self, m):
        for sc in self.scenes:
            sc.set_camera_view(m)

    def set_proj_matrix(self, m):
        for sc in self.scenes:
            sc.set_proj_matrix(m)

    def set_panorama(self, hfov_deg):
        if hfov_deg is not None:
            raise NotImplementedError("a panorama camera on a StitchedScene: stitched frames are pinhole frames")
        for sc in self.scenes:
            sc.set_panorama(None)

    @property
    def panorama(self):
        return next((sc.panorama for sc in self.scenes if sc.panorama is not None), None)

    def set_lens(self, model, coeffs=None, limit=None):
        if model is not None:
            raise NotImplementedError("a lens camera on a StitchedScene: stitched frames are pinhole frames")
        for sc in self.scenes:
            sc.set_lens(None)

    @property
    def lens(self):
        return next((sc.lens for sc in self.scenes if sc.lens is not None), None)

    def set_model_view(self, m):
        for sc in self.scenes:
            sc.set_model_view(m)

    def announce_next_camera_view(self, m):
        for sc in self.scenes:
            sc.announce_next_camera_view(m)

    def set_use_light(self, use_light):
        for sc in self.scenes:
            sc.set_use_light(use_light)

    def total_matrix(self):
        return self.scenes[0].total_matrix()

    def capture_frame(self, *args, **kwargs):
        raise NotImplementedError("capture_frame on a StitchedScene: instances belong to a part and the merged frame carries "
                                  "stitched ids; take the flow of the parts' own frames")

    def flow_between(self, *args, **kwargs):
        raise NotImplementedError("flow_between on a StitchedScene: instances belong to a part and the merged frame carries "
                                  "stitched ids; take the flow of the parts' own frames")

    def annotate_frame(self, *args, **kwargs):
        raise NotImplementedError("annotate_frame on a StitchedScene: instances belong to a part and the merged frame carries "
                                  "stitched ids; annotate the parts' own frames")

    def lidar_sweep(self, *args, **kwargs):
        raise NotImplementedError("lidar_sweep on a StitchedScene: a sweep ranges one cloud and its instances; sweep the parts "
                                  "(scenes[s].lidar_sweep)")

    def select_boxes(self, *args, **kwargs):
        raise NotImplementedError("select_boxes on a StitchedScene: labels belong to a part; select on the parts "
                                  "(scenes[s].select_boxes)")

    def select_masks(self, *args, **kwargs):
        raise NotImplementedError("select_masks on a StitchedScene: labels belong to a part; select on the parts "
                                  "(scenes[s].select_masks)")

    def take_next_total_matrix(self):
        nxt = [sc.take_next_total_matrix() for sc in self.scenes]          # consumed on every part; the frame's is part 0's
        return nxt[0]

    def augmented(self):
        return any(sc.augmented() for sc in self.scenes)

    def edited(self):
        return any(sc.edited() for sc in self.scenes)

    def delete(self):
        for sc in self.scenes:
            sc.delete()
        self._raster = None

    def rasterizer(self):
        """The StitchedRasterizer over the parts' own rasterisers, built lazily like ``Scene.rasterizer()`` and rebuilt only when
        a part rebuilt its own (new vertices, new labels)."""
        from .stitch import StitchedRasterizer
        for s, sc in enumerate(self.scenes):
            if getattr(sc, 'foreign_objects', None):
                raise NotImplementedError(f"foreign objects (add_foreign_object) in part {s} of a StitchedScene: the stitched gather "
                                          "has one descriptor table per part")
        rs = [sc.rasterizer() for sc in self.scenes]
        if self._raster is None or any(a is not b for a, b in zip(self._raster.parts, rs)):
            self._raster = StitchedRasterizer(rs)
            for s, P in enumerate(self.part_poses):
                self._raster.set_part_pose(s, P)
            for s in self.part_hidden:
                self._raster.set_part_visible(s, False)
        return self._raster


class MultiscaleRender:
    """READ/datasets/dynamic.py:50-99 without OpenGL: one HIP pass fills all five scales; the
    result dict maps each input_format token to an (h, w, 3) float tensor with the point id in
    channel 0 (GL's RGBA32F colour target, programs.py:164-167), row 0 = image top unless gl_frame."""

    def __init__(self, scene, input_format, viewport_size, proj_matrix=None, out_buffer_location='numpy',
                 gl_frame=False, supersampling=1, clear_color=None):
        self.scene = scene
        self.input_format = input_format
        self.proj_matrix = proj_matrix
        self.gl_frame = gl_frame
        self.viewport_size = viewport_size
        self.ss = supersampling
        self.out_buffer_location = out_buffer_location
        self.last_index = None

    def render(self, view_matrix=None, proj_matrix=None, input_format=None):
        if view_matrix is not None:
            self.scene.set_camera_view(view_matrix)
        proj_matrix = self.proj_matrix if proj_matrix is None else proj_matrix
        if proj_matrix is not None:
            self.scene.set_proj_matrix(proj_matrix)
        self.scene.set_use_light(False)
        input_format = input_format if input_format else self.input_format
        fmts = input_format.replace(' ', '').split(',')
        scene = self.scene
        W, H = self.ss * self.viewport_size[0], self.ss * self.viewport_size[1]
        out = {}
        if getattr(scene, 'panorama', None) is not None:
            what = "a StitchedScene" if getattr(scene, 'stitched', False) else "MultiscaleRender (the dict path)"
            raise NotImplementedError(f"a panorama camera (set_panorama) on {what}: only OGL.infer's fast path and "
                                      "FrameRenderer.render_pano draw it")
        if getattr(scene, 'lens', None) is not None:
            return self._render_lens(scene, input_format, fmts, W, H)
        if getattr(scene, 'stitched', False):
            return self._render_stitched(scene, input_format, fmts, W, H)
        if getattr(scene, 'foreign_objects', None):
            raise NotImplementedError("foreign objects (add_foreign_object) on MultiscaleRender (the dict path): its id tokens would "
                                      "carry ids past the scene's descriptor table; only OGL.infer's fast path and FrameRenderer "
                                      "draw them")
        pyramid = is_point_id_pyramid(input_format) and W % (1 << (len(fmts) - 1)) == 0 and H % (1 << (len(fmts) - 1)) == 0
        if scene.edited() and scene.augmented():
            raise NotImplementedError("scene objects (set_object_labels, add_object_instance) with GL-twin augmentation (point sizes, discard, drop, "
                                      "perturb)")
        if scene.edited() and not pyramid:
            bad = next((f for i, f in enumerate(fmts) if not is_point_id_pyramid(','.join(fmts[:i + 1]))), None)
            if bad is None:
                raise NotImplementedError(f"scene objects (set_object_labels) at {W}x{H}: the point-id pyramid needs sizes that "
                                          f"are multiples of {1 << (len(fmts) - 1)}")
            raise NotImplementedError(f"token {bad!r} with scene objects (set_object_labels): only the point-id pyramid "
                                      "honours object poses and visibility")
        if pyramid and not scene.augmented():
            # the layout of TexturePipeline: one pass over the cloud feeds every scale
            idx, _ = scene.rasterizer().render(scene.total_matrix(), W, H, len(fmts), want_depth=False)
            self.last_index = idx
            for fmt, ids_l in zip(fmts, idx):
                out[fmt] = self._package(self._id_image(ids_l[0]), fmt)
            return out
        self.last_index = []
        for fmt in fmts:
            cfg = parse_input_string(fmt)
            scene.set_params(**cfg)
            s = cfg.get('downscale', 0)
            w, h = W // 2 ** s, H // 2 ** s                       # dynamic.py:61: ss * viewport // 2**i
            x = self._render_token(cfg, w, h)
            out[fmt] = self._package(x, fmt)
        return out

    def _render_lens(self, scene, input_format, fmts, W, H):
        """A lens camera (Scene.set_lens): the plain point-id pyramid through ``render_lens`` — what TexturePipeline trains
        with; everything else is refused by name."""
        what = "a lens camera (set_lens)"
        if getattr(scene, 'stitched', False):
            raise NotImplementedError(f"{what} on a StitchedScene: stitched frames are pinhole frames")
        if getattr(scene, 'foreign_objects', None):
            raise NotImplementedError("foreign objects (add_foreign_object) on MultiscaleRender (the dict path): its id tokens would "
                                      "carry ids past the scene's descriptor table; only OGL.infer's fast path and FrameRenderer "
                                      "draw them")
        if self.ss > 1:
            raise NotImplementedError(f"supersampling {self.ss} with {what}")
        if scene.augmented():
            raise NotImplementedError(f"GL-twin augmentation (point sizes, discard, drop, perturb) with {what}")
        if not is_point_id_pyramid(input_format):
            bad = next(f for i, f in enumerate(fmts) if not is_point_id_pyramid(','.join(fmts[:i + 1])))
            raise NotImplementedError(f"token {bad!r} with {what}: only the point-id pyramid is drawn through a lens")
        if W % (1 << (len(fmts) - 1)) or H % (1 << (len(fmts) - 1)):
            raise NotImplementedError(f"{what} at {W}x{H}: the point-id pyramid needs sizes that are multiples of "
                                      f"{1 << (len(fmts) - 1)}")
        idx, _ = scene.rasterizer().render_lens(scene.lens_camera(), W, H, len(fmts), want_depth=False)
        self.last_index = idx
        return {fmt: self._package(self._id_image(ids_l[0]), fmt) for fmt, ids_l in zip(fmts, idx)}

    def _render_stitched(self, scene, input_format, fmts, W, H):
        """A StitchedScene: the point-id pyramid of merged global ids; everything else is refused by name."""
        if self.ss > 1:
            raise NotImplementedError(f"supersampling {self.ss} with scene stitching (StitchedScene)")
        if scene.augmented():
            raise NotImplementedError("GL-twin augmentation (point sizes, discard, drop, perturb) with scene stitching")
        if not is_point_id_pyramid(input_format):
            bad = next(f for i, f in enumerate(fmts) if not is_point_id_pyramid(','.join(fmts[:i + 1])))
            raise NotImplementedError(f"token {bad!r} with scene stitching (StitchedScene): only the point-id pyramid is merged")
        if W % (1 << (len(fmts) - 1)) or H % (1 << (len(fmts) - 1)):
            raise NotImplementedError(f"scene stitching at {W}x{H}: the point-id pyramid needs sizes that are multiples of "
                                      f"{1 << (len(fmts) - 1)}")
        idx, _ = scene.rasterizer().render_merged(scene.total_matrix(), W, H, len(fmts), want_depth=False)
        self.last_index = idx
        return {fmt: self._package(self._id_image(ids_l[0]), fmt) for fmt, ids_l in zip(fmts, idx)}

    # ---- one token = one GL draw of the reference (READ/gl/render.py:52-85) -------------------------------------------
    def _id_image(self, ids):
        x = torch.zeros(ids.shape + (3,), dtype=torch.float32, device=ids.device)
        x[..., 0] = index_to_float(ids)
        return x

    def _package(self, x, fmt):
        if self.gl_frame:
            x = x.flip([0])
        if ('depth' in fmt and 'depth3' not in fmt) or 'label' in fmt:          # dynamic.py:92-95
            x = x[..., :1]
        return x if self.out_buffer_location == 'torch' else x.cpu().numpy()

    def _render_token(self, cfg, w, h):
        scene = self.scene
        if not cfg['draw_points']:
            raise NotImplementedError("tokens without a point size draw triangles (mesh rendering); a point cloud needs pN / psN")
        mode0, mode1 = cfg['mode']
        if mode0 == MODE_UV and mode1 == UV_TYPE_2D:
            raise NotImplementedError("uv_2d (mesh textures) is outside the point-cloud render path")
        M = scene.total_matrix()
        idx, dep = scene.rasterizer().render_gl(M, w, h, point_size=cfg['point_size'], relative=cfg['splat_mode'],
                                                min_point_size=1.0, discard=scene.point_discard, drop=scene.point_drop,
                                                perturb=scene.point_perturb, perturb_hash=scene.point_perturb_seeded,
                                                point_sizes=scene.point_sizes)
        self.last_index.append(idx)
        ids, covered = idx[0], (dep[0] != 0) | (idx[0] != 0)
        if mode0 == MODE_UV:
            return self._id_image(ids)
        lid = ids.long()
        if mode0 == MODE_COLOR:
            col = scene.device_array('colors')[lid]
        elif mode0 == MODE_LABEL:                                                # programs.py:176-178
            col = torch.zeros(ids.shape + (3,), dtype=torch.float32, device=ids.device)
            col[..., 0] = scene.device_array('normals')[lid][..., 0] / 255.
        elif mode0 == MODE_XYZ:                                                  # programs.py:172-175
            lo = torch.from_numpy(scene.xyz_min).to(ids.device)
            hi = torch.from_numpy(scene.xyz_max).to(ids.device)
            col = (scene.device_array('xyz')[lid] - lo) / (hi - lo + 1e-9)
        elif mode0 == MODE_DEPTH:                                                # programs.py:160-164: gl_Position.z
            pos = scene.device_array('xyz')[lid]
            m2 = torch.from_numpy(M[0, 2].copy()).to(ids.device)
            d = m2[0] * pos[..., 0] + m2[1] * pos[..., 1] + m2[2] * pos[..., 2] + m2[3]
            col = d[..., None].expand(-1, -1, 3)
        else:                                                                    # programs.py:137-159
            nrm = scene.device_array('normals')[lid]
            cam = torch.from_numpy(np.ascontiguousarray(scene.view_matrix[:3, 3])).to(ids.device)
            unit = lambda v: v / v.norm(dim=-1, keepdim=True)
            if mode1 == 0:
                col = nrm * 0.5 + 0.5
            else:
                vdir = unit(cam - scene.device_array('xyz')[lid])
                if mode1 == 1:                                                   # reflect(I, N) = I - 2 dot(N, I) N
                    col = unit(vdir - 2.0 * (nrm * vdir).sum(-1, keepdim=True) * nrm) * 0.5 + 0.5
                elif mode1 == 2:                                                 # normal in the camera frame
                    w2c = torch.from_numpy(np.linalg.inv(scene.view_matrix.astype(np.float32))).to(ids.device)
                    p = cam + nrm
                    local = p @ w2c[:3, :3].T + w2c[:3, 3]
                    col = unit(local) * 0.5 + 0.5
                else:
                    col = vdir * 0.5 + 0.5
        return torch.where(covered[..., None], col.float(), torch.zeros((), device=ids.device))
