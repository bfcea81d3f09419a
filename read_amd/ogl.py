"""Viewer-side glue with the interface of READ/gl/nn.py:76-129 (``OGL``): rasterise the scene's
current camera, look up descriptors, run the net, hand back an ``H x W x 4`` RGBA frame.

``OGL(scene, scene_data, viewport_size, net_ckpt, texture_ckpt, ...)`` loads a pipeline checkpoint
exactly like the reference; ``OGL.from_model(scene, model, input_format, viewport_size)`` wraps an
already-built ``NetAndTexture`` (used when no checkpoint file exists, e.g. synthetic scenes).
``infer()`` keeps every stage on the device: int32 index pyramids -> one gather launch -> one UNet
plan, no ToTensor / host copies (nn.py:115-117)."""
import torch

from . import _lib
from .render import MultiscaleRender, is_point_id_pyramid
from .texture import gather_pyramid, gather_tables_pyramid, stitch_gather_pyramid


class OGL:
    def __init__(self, scene, scene_data, viewport_size, net_ckpt, texture_ckpt, out_buffer_location='numpy',
                 supersampling=1, gpu=True, clear_color=None, temporal_average=False):
        from .pipeline import load_pipeline
        args_upd = {'inference': True}
        if texture_ckpt:
            args_upd['texture_ckpt'] = texture_ckpt
            if 'pointcloud' in scene_data:
                args_upd['n_points'] = scene_data['pointcloud']['xyz'].shape[0]
        pipeline, args = load_pipeline(net_ckpt, args_to_update=args_upd)
        model = pipeline.model
        model.load_textures(0)
        self._setup(scene, model, args.input_format, viewport_size, out_buffer_location, supersampling, gpu,
                    clear_color, temporal_average)

    @classmethod
    def from_model(cls, scene, model, input_format, viewport_size, out_buffer_location='torch', supersampling=1,
                   temporal_average=False, texture_ids=None):
        """texture_ids: for a ``render.StitchedScene`` the loaded texture of every part, in part order (default: the model's
        loaded textures in their order)."""
        self = cls.__new__(cls)
        self._setup(scene, model, input_format, viewport_size, out_buffer_location, supersampling, True, None,
                    temporal_average, texture_ids)
        return self

    def _setup(self, scene, model, input_format, viewport_size, out_buffer_location, supersampling, gpu, clear_color,
               temporal_average, texture_ids=None):
        if not gpu:
            raise _lib.ReadHipError("OGL(gpu=False): the render path has no CPU implementation")
        self.gpu = True
        self.model = model.cuda().eval()
        if supersampling > 1:
            self.model.ss = supersampling
        self.model.temporal_average = temporal_average
        factor = 16
        assert viewport_size[0] % 16 == 0, f'set width {factor * (viewport_size[0] // factor)}'
        assert viewport_size[1] % 16 == 0, f'set height {factor * (viewport_size[1] // factor)}'
        self.viewport_size = viewport_size
        self.input_format = input_format
        self.renderer = MultiscaleRender(scene, input_format, viewport_size, out_buffer_location='torch',
                                         supersampling=self.model.ss, clear_color=clear_color)
        # the device-resident fast path of infer() serves exactly the layout TexturePipeline trains with: >= 4 tokens,
        # token i = 1-px point ids at downscale i; anything else goes through the checked dict path
        fmts = input_format.replace(' ', '').split(',')
        self._fast_format = len(fmts) >= 4 and is_point_id_pyramid(input_format)
        self.last_path = None                # 'fast' / 'dict': which branch the last infer() took (asserted by the tests)
        self.texture_ids = None if texture_ids is None else list(texture_ids)
        if getattr(scene, 'stitched', False):
            ids = list(model._loaded_textures) if texture_ids is None else self.texture_ids
            if len(ids) != len(scene.scenes):
                raise ValueError(f"{len(ids)} textures for a stitched scene of {len(scene.scenes)} parts")
            missing = [t for t in ids if str(t) not in self.model._modules]
            if missing:
                raise ValueError(f"textures {missing} are not loaded (model.load_textures)")
            self.texture_ids = ids
        elif texture_ids is not None:
            raise ValueError("texture_ids goes with a StitchedScene (one texture per part)")

    def infer(self, input_dict=None):
        """-> {'output': H x W x 4 float tensor (RGB + alpha 1), 'net_input': list of NCHW feature maps}; a caller-supplied
        ``input_dict`` (it must carry its own 'id') is rendered as it is and echoed under 'input', as the src tree's
        ``OGL.infer(input_dict)`` does (src/READ/gl/nn.py:115-137)."""
        model = self.model
        if getattr(self.renderer.scene, 'stitched', False):
            return self._infer_stitched(input_dict)
        texture = model._modules[str(model._loaded_textures[0])] if model._loaded_textures else model._modules['0']
        fast = (input_dict is None and not model.temporal_average and self._fast_format
                and not self.renderer.scene.augmented() and hasattr(model.net, 'engine'))
        pano = getattr(self.renderer.scene, 'panorama', None) is not None
        if pano:
            self._require_fast("a panorama camera (set_panorama)", input_dict)
        lens = getattr(self.renderer.scene, 'lens', None) is not None
        if lens:
            self._require_fast("a lens camera (set_lens)", input_dict)
        foreign = bool(getattr(self.renderer.scene, 'foreign_objects', None))
        if foreign:
            self._require_fast("foreign objects (add_foreign_object)", input_dict, ": the table gather has no supersampled form")
        self.last_path = 'fast' if fast else 'dict'
        with torch.set_grad_enabled(False):
            if fast:
                scene = self.renderer.scene
                W, H = self.viewport_size
                fmts = self.input_format.replace(' ', '').split(',')
                raster = scene.rasterizer()
                if raster.n != texture.texture_.shape[-1]:
                    raise ValueError(f"descriptor table has {texture.texture_.shape[-1]} points, the scene cloud {raster.n}")
                ss = int(model.ss)                               # supersampling: raster at ss x, reduce in the gather
                if pano:                                         # Scene.set_panorama: only the raster step differs
                    scene.take_next_total_matrix()               # an announced next camera is ignored (and consumed)
                    idx, _ = raster.render_pano(scene.pano_camera(), W, H, len(fmts), want_depth=False)
                elif lens:                                       # Scene.set_lens: likewise
                    scene.take_next_total_matrix()
                    idx, _ = raster.render_lens(scene.lens_camera(), W, H, len(fmts), want_depth=False)
                else:
                    idx, _ = raster.render(scene.total_matrix(), ss * W, ss * H, len(fmts), want_depth=False,
                                           next_total=scene.take_next_total_matrix())      # Scene.announce_next_camera_view
                if foreign:                                      # ids >= N live in the foreign objects' own tables
                    feats = gather_tables_pyramid(scene.gather_tables(texture), idx)
                else:
                    feats = gather_pyramid(texture.rows(), idx, texture.activation, ss=ss)
                out = model.net.engine(H, W).forward(feats[0][0], feats[1][0], feats[2][0], feats[3][0], channels=4)
                net_input = [f.permute(0, 3, 1, 2) for f in feats]
            else:
                given = input_dict is not None
                if not given:
                    input_dict = {k: v.permute(2, 0, 1)[None] for k, v in self.renderer.render().items()}
                feed = dict(input_dict)                          # the model removes 'id' from the dict it is handed
                if not given or 'id' not in feed:
                    feed['id'] = 0
                o, net_input = model(feed, return_input=True)
                if isinstance(o, dict):                          # src tree: the net returns {'im_out': image}
                    o = o['im_out']
                o = o[0].detach().permute(1, 2, 0)
                out = torch.cat([o, torch.ones_like(o[:, :, :1])], 2).contiguous()
        res = {'output': out, 'net_input': net_input}
        if input_dict is not None:
            res['input'] = input_dict
        return res

    def infer_annotated(self):
        """``infer()``'s fast path with the frame's depth kept, plus the frame's annotation: -> {'output', 'net_input',
        'annotation'}; 'annotation' is an ``annotate.Annotation`` of the level-0 frame the output was painted from (per pixel the
        object and the instance handle, per instance boxes and counts; ``Scene.annotation_handle`` maps the scene's handles).
        'output' is ``infer()``'s frame bit for bit.  What the annotation does not cover is refused by name."""
        model, scene = self.model, self.renderer.scene
        what = "frame annotations (infer_annotated)"
        if getattr(scene, 'stitched', False):
            raise NotImplementedError(f"{what} on a StitchedScene: instances belong to a part; annotate the parts' own frames")
        if getattr(scene, 'panorama', None) is not None:
            raise NotImplementedError(f"a panorama camera (set_panorama) with {what}: the instance match re-projects with the "
                                      "pinhole projection")
        if getattr(scene, 'lens', None) is not None:
            raise NotImplementedError(f"a lens camera (set_lens) with {what}: the instance match re-projects with the pinhole "
                                      "projection")
        self._require_fast(what, None, ": annotations describe the level-0 frame at the output size")
        texture = model._modules[str(model._loaded_textures[0])] if model._loaded_textures else model._modules['0']
        W, H = self.viewport_size
        fmts = self.input_format.replace(' ', '').split(',')
        raster = scene.rasterizer()
        if raster.n != texture.texture_.shape[-1]:
            raise ValueError(f"descriptor table has {texture.texture_.shape[-1]} points, the scene cloud {raster.n}")
        M = scene.total_matrix()
        if M.shape[0] != 1:
            raise NotImplementedError(f"more than one camera with {what}")
        self.last_path = 'fast'
        with torch.set_grad_enabled(False):
            idx, dep = raster.render(M, W, H, len(fmts), want_depth=True, next_total=scene.take_next_total_matrix())
            if scene.has_foreign():
                feats = gather_tables_pyramid(scene.gather_tables(texture), idx)
            else:
                feats = gather_pyramid(texture.rows(), idx, texture.activation, ss=1)
            out = model.net.engine(H, W).forward(feats[0][0], feats[1][0], feats[2][0], feats[3][0], channels=4)
            annotation = raster.annotate(M[0], W, H, idx[0], dep[0])
        return {'output': out, 'net_input': [f.permute(0, 3, 1, 2) for f in feats], 'annotation': annotation}

    def infer_tracked(self):
        """``infer_annotated``'s fast path with the frame snapshot for the frame flow in place of the annotation: -> {'output',
        'net_input', 'state'}; 'state' is a ``flow.FrameState`` of the level-0 frame the output was painted from, for
        ``Scene.flow_between`` with the state of another call.  'output' is ``infer()``'s frame bit for bit.  What the flow does not
        cover is refused by name."""
        model, scene = self.model, self.renderer.scene
        what = "frame flow (infer_tracked)"
        if getattr(scene, 'stitched', False):
            raise NotImplementedError(f"{what} on a StitchedScene: instances belong to a part; take the flow of the parts' own frames")
        if getattr(scene, 'panorama', None) is not None:
            raise NotImplementedError(f"a panorama camera (set_panorama) with {what}: the flow re-projects with the pinhole "
                                      "projection")
        if getattr(scene, 'lens', None) is not None:
            raise NotImplementedError(f"a lens camera (set_lens) with {what}: the flow re-projects with the pinhole projection")
        self._require_fast(what, None, ": the flow describes the level-0 frame at the output size")
        texture = model._modules[str(model._loaded_textures[0])] if model._loaded_textures else model._modules['0']
        W, H = self.viewport_size
        fmts = self.input_format.replace(' ', '').split(',')
        raster = scene.rasterizer()
        if raster.n != texture.texture_.shape[-1]:
            raise ValueError(f"descriptor table has {texture.texture_.shape[-1]} points, the scene cloud {raster.n}")
        M = scene.total_matrix()
        if M.shape[0] != 1:
            raise NotImplementedError(f"more than one camera with {what}")
        self.last_path = 'fast'
        with torch.set_grad_enabled(False):
            idx, dep = raster.render(M, W, H, len(fmts), want_depth=True, next_total=scene.take_next_total_matrix())
            if scene.has_foreign():
                feats = gather_tables_pyramid(scene.gather_tables(texture), idx)
            else:
                feats = gather_pyramid(texture.rows(), idx, texture.activation, ss=1)
            out = model.net.engine(H, W).forward(feats[0][0], feats[1][0], feats[2][0], feats[3][0], channels=4)
            state = raster.frame_state(M[0], W, H, idx[0], dep[0])
        return {'output': out, 'net_input': [f.permute(0, 3, 1, 2) for f in feats], 'state': state}

    def _require_fast(self, what, input_dict, ss_note=''):
        """``what`` — foreign objects, a panorama or lens camera, scene stitching — is drawn on the fast path only (for foreign objects:
        the dict path's single-table lookup would see ids >= N).  What would leave the fast path is refused by name."""
        model, scene = self.model, self.renderer.scene
        if input_dict is not None:
            raise NotImplementedError(f"a caller-supplied input_dict with {what}")
        if model.temporal_average:
            raise NotImplementedError(f"temporal_average with {what}")
        if int(model.ss) > 1:
            raise NotImplementedError(f"supersampling {int(model.ss)} with {what}{ss_note}")
        if scene.augmented():
            raise NotImplementedError(f"GL-twin augmentation (point sizes, discard, drop, perturb) with {what}")
        if not self._fast_format or not hasattr(model.net, 'engine'):
            raise NotImplementedError(f"input format {self.input_format!r} with {what}: only the point-id pyramid of at least four "
                                      "scales on the HIP UNet is served")

    def _infer_stitched(self, input_dict):
        """A StitchedScene: per-part raster with depth -> one stitched gather -> the engine.  Always the fast path; what it does
        not serve is refused by name."""
        model, scene = self.model, self.renderer.scene
        if scene.panorama is not None:
            raise NotImplementedError("a panorama camera (set_panorama) on a StitchedScene: stitched frames are pinhole frames")
        if scene.lens is not None:
            raise NotImplementedError("a lens camera (set_lens) on a StitchedScene: stitched frames are pinhole frames")
        self._require_fast("scene stitching (StitchedScene)", input_dict)
        textures = [model._modules[str(t)] for t in self.texture_ids]
        raster = scene.rasterizer()
        for s, tex in enumerate(textures):
            if hasattr(tex, 'parts'):
                raise NotImplementedError(f"a JointTexture as the texture of part {s} on OGL's fast path: the stitched gather takes one "
                                          "PointTexture per part; pass the parts' own texture ids (the joint serves the dict path)")
            if raster.part(s).n != tex.texture_.shape[-1]:
                raise ValueError(f"part {s}: descriptor table has {tex.texture_.shape[-1]} points, the part's cloud "
                                 f"{raster.part(s).n}")
        self.last_path = 'fast'
        W, H = self.viewport_size
        fmts = self.input_format.replace(' ', '').split(',')
        with torch.set_grad_enabled(False):
            frames = raster.render(scene.total_matrix(), W, H, len(fmts), next_total=scene.take_next_total_matrix())
            rows = [t.rows() for t in textures]
            feats = [torch.empty((1, H >> l, W >> l, rows[0].shape[1]), dtype=torch.float32, device=rows[0].device)
                     for l in range(len(fmts))]
            stitch_gather_pyramid(raster.gather_parts(frames, [(r, t.activation) for r, t in zip(rows, textures)]), out=feats)
            out = model.net.engine(H, W).forward(feats[0][0], feats[1][0], feats[2][0], feats[3][0], channels=4)
        return {'output': out, 'net_input': [f.permute(0, 3, 1, 2) for f in feats]}
