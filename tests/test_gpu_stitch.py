"""GPU: scene stitching — several fitted scenes in one frame (read_stitch_gather_forward, read_amd/stitch.py, StitchedScene).

The contract is the NumPy model of tests/stitch_model.py (checked against the oracle on the CPU, tests/test_stitch_cpu.py).  Every
comparison here is exact: torch.equal on ids, depth bit patterns, part bytes and features.  Activated features are compared with
read_gather_forward's on the winner's local ids (the two kernels share act_apply), plain ones also with the rows themselves."""
import functools

import numpy as np
import pytest
import torch

import oracle
from read_amd import _lib, camera, synthetic
from read_amd.frame import FrameRenderer
from read_amd.net_texture import NetAndTexture
from read_amd.ogl import OGL
from read_amd.raster import PointCloudRasterizer, object_matrix
from read_amd.render import MultiscaleRender, Scene, StitchedScene
from read_amd.stitch import StitchedFrameRenderer, StitchedRasterizer
from read_amd.texture import PointTexture, gather_pyramid, stitch_gather_pyramid
from read_amd.unet import UNet, weight_spec
from tests import stitch_model as sm
from tests.test_gpu_objects import about, cluster_labels, oracle_edit, rot_z

pytestmark = pytest.mark.gpu

LEVELS = sm.LEVELS
ACTS = ("none", "sigmoid", "tanh")
FMT = "uv_1d_p1, uv_1d_p1_ds1, uv_1d_p1_ds2, uv_1d_p1_ds3, uv_1d_p1_ds4"


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def up_levels(levels):
    return [up(a)[None] for a in levels]


def bits(t):
    return t.view(torch.int32)


def assert_images(got, want, what):
    """got: device tensors per level (1,h,w[,C]); want: arrays per level; bit for bit."""
    for l, (g, w) in enumerate(zip(got, want)):
        w = up(w).reshape(g.shape)
        same = torch.equal(bits(g), bits(w)) if g.dtype == torch.float32 else torch.equal(g, w)
        assert same, f"{what}: level {l}: {int((g != w).sum())} entries differ"


def rows_of(n, Cc, seed):
    return (np.random.default_rng(100 + seed).random((n, Cc), dtype=np.float32) * 4.0 - 2.0).astype(np.float32)


def feature_reference(rows_dev, acts, part_levels, local_levels):
    """The activated features of the contract from read_gather_forward: part s's plain gather on the winner's local ids where part s
    won, part 0's descriptor 0 where nobody did."""
    out = None
    for s, (rows, act) in enumerate(zip(rows_dev, acts)):
        mine = [up(np.where(p == s, loc, 0).astype(np.int32))[None] for p, loc in zip(part_levels, local_levels)]
        plain = gather_pyramid(rows, mine, act)
        if out is None:
            out = [f.clone() for f in plain]                  # part 0: also the pixels without a candidate (id 0)
        else:
            for o, f, p in zip(out, plain, part_levels):
                sel = up(p == s)[None]
                o[sel] = f[sel]
    return out


@functools.lru_cache(maxsize=None)
def small_parts(S, w, h):
    """S clouds of 3000 points seen by the union camera, the first 200 points of each being points 200..399 of the part before
    it (exact ties across parts), and their oracle pyramids."""
    clouds = [synthetic.make_cloud(3000, seed=10 + s).copy() for s in range(S)]
    for s in range(1, S):
        clouds[s][:200] = clouds[s - 1][200:400]
    M = sm.union_camera(w, h)
    return clouds, M, [oracle.raster_multiscale(c, M, w, h, LEVELS) for c in clouds]


def run_kernel(pyramids, base, rows_dev, acts, visible=None, **want):
    parts = []
    for s, (pi, pd) in enumerate(pyramids):
        shown = visible is None or visible[s]
        parts.append((rows_dev[s], up_levels(pi) if shown else None, up_levels(pd) if shown else None, base[s], acts[s]))
    return stitch_gather_pyramid(parts, **want)


# ---- 1. the kernel against the NumPy model, on pyramids of the oracle ------------------------------------------------------------
@pytest.mark.parametrize("size", [(64, 48), (48, 32)])
@pytest.mark.parametrize("Cc", [4, 8])
@pytest.mark.parametrize("S", [1, 2, 3, 8])
def test_kernel_equals_the_model(hip, S, Cc, size):
    w, h = size
    clouds, _, pyramids = small_parts(S, w, h)
    counts = [c.shape[0] for c in clouds]
    base = sm.id_bases(counts)
    rows = [rows_of(n, Cc, s) for s, n in enumerate(counts)]
    rows_dev = [up(r) for r in rows]
    acts = [ACTS[s % 3] for s in range(S)]
    for visible in ([True] * S,) + (([True, False] + [True] * (S - 2),) if S >= 3 else ()):
        mi, md, mp, ml = sm.merge([(pi, pd, base[s]) for s, (pi, pd) in enumerate(pyramids)], visible)
        feat, idx, dep, part = run_kernel(pyramids, base, rows_dev, acts, visible, want_index=True, want_depth=True, want_part=True)
        torch.cuda.synchronize()
        what = f"S={S} C={Cc} {w}x{h} visible={visible}"
        assert_images(idx, mi, what + " index")
        assert_images(dep, md, what + " depth")
        assert_images(part, mp, what + " part")
        ref = feature_reference(rows_dev, acts, mp, ml)
        for l in range(LEVELS):
            assert torch.equal(bits(feat[l]), bits(ref[l])), f"{what} features level {l}"
        plain = run_kernel(pyramids, base, rows_dev, ["none"] * S, visible)                 # features alone, no activation
        assert_images(plain, sm.features(rows, mp, ml), what + " plain features")
        if S >= 2 and all(visible):                      # later parts win pixels, and exact cross-part ties occur
            assert int((mp[0] == 1).sum()) > 0 and sm.tie_and_empty_counts(pyramids)[0][0] >= 1


def test_every_subset_of_outputs(hip):
    S, Cc, (w, h) = 3, 8, (64, 48)
    clouds, _, pyramids = small_parts(S, w, h)
    base = sm.id_bases([c.shape[0] for c in clouds])
    rows_dev = [up(rows_of(c.shape[0], Cc, s)) for s, c in enumerate(clouds)]
    full = run_kernel(pyramids, base, rows_dev, ACTS, want_index=True, want_depth=True, want_part=True)
    for mask in range(1, 16):
        wf, wi, wd, wp = bool(mask & 1), bool(mask & 2), bool(mask & 4), bool(mask & 8)
        got = run_kernel(pyramids, base, rows_dev if wf else [c.shape[0] for c in clouds], ACTS, want_feat=wf, want_index=wi,
                         want_depth=wd, want_part=wp)
        got = got if isinstance(got, tuple) else (got,)
        assert (got[0] is None) == (not wf) and len(got) == 1 + wi + wd + wp
        want = [full[0] if wf else None] + [x for x, on in ((full[1], wi), (full[2], wd), (full[3], wp)) if on]
        for g, x in zip(got, want):
            if g is not None:
                for l in range(LEVELS):
                    assert torch.equal(bits(g[l]) if g[l].dtype == torch.float32 else g[l],
                                       bits(x[l]) if x[l].dtype == torch.float32 else x[l]), f"outputs {mask:04b} level {l}"
    with pytest.raises(_lib.ReadHipError, match="no outputs"):
        run_kernel(pyramids, base, rows_dev, ACTS, want_feat=False)


def test_hand_built_pyramid_with_every_pixel_class(hip):
    """Classes per pixel: 0 nobody; 1 one candidate; 2 parts 0 and 2 tie; 3 parts 1 and 3 tie and part 1 is hidden; 4 local id 0 at a
    non-zero depth (a candidate); 5 a non-zero id at depth bits 0 (a candidate, and nothing is nearer); 6 all four, distinct."""
    S, Cc, (w, h) = 4, 8, (64, 48)
    rng = np.random.default_rng(7)
    counts = [500, 400, 300, 200]
    base = sm.id_bases(counts)
    visible = [True, False, True, True]
    pyramids, classes = [([], []) for _ in range(S)], []
    for l in range(LEVELS):
        shape = (h >> l, w >> l)
        cls = rng.integers(0, 7, shape)
        cls.reshape(-1)[:7] = np.arange(7)                                  # every class on every level
        ids = [rng.integers(1, n, shape).astype(np.int32) for n in counts]
        dep = [rng.uniform(0.1, 0.9, shape).astype(np.float32) for _ in counts]
        on = [np.zeros(shape, bool) for _ in counts]
        one = rng.integers(0, S, shape)
        for s in range(S):
            on[s] |= (cls == 1) & (one == s) | (cls == 6)
        on[0] |= (cls == 2) | (cls == 4) | (cls == 5)
        on[2] |= (cls == 2) | (cls == 5)
        on[1] |= cls == 3
        on[3] |= cls == 3
        dep[2] = np.where(cls == 2, dep[0], dep[2])
        dep[3] = np.where(cls == 3, dep[1], dep[3])
        ids[0] = np.where(cls == 4, 0, ids[0]).astype(np.int32)
        dep[2] = np.where(cls == 5, 0.0, dep[2]).astype(np.float32)
        for s in range(S):
            pyramids[s][0].append(np.where(on[s], ids[s], 0).astype(np.int32))
            pyramids[s][1].append(np.where(on[s], dep[s], 0.0).astype(np.float32))
        classes.append(cls)
    rows = [rows_of(n, Cc, s) for s, n in enumerate(counts)]
    rows_dev = [up(r) for r in rows]
    acts = ["tanh", "none", "sigmoid", "none"]
    mi, md, mp, ml = sm.merge([(pi, pd, base[s]) for s, (pi, pd) in enumerate(pyramids)], visible)
    for l, cls in enumerate(classes):                                       # the model does what the class says
        assert (mp[l][cls == 0] == 255).all() and (mp[l][cls == 2] == 0).all() and (mp[l][cls == 3] == 3).all()
        assert (mp[l][cls == 4] == 0).all() and (mi[l][cls == 4] == 0).all() and (mp[l][cls == 5] == 2).all()
        assert (mi[l][cls == 3] >= base[3]).all() and (md[l][cls == 5].view(np.uint32) == 0).all()
    ref = feature_reference(rows_dev, acts, mp, ml)
    empties = [(np.zeros_like(i), np.zeros_like(d)) for i, d in zip(*pyramids[1])]
    as_empties = [pyramids[0], tuple(map(list, zip(*empties))), pyramids[2], pyramids[3]]
    for name, pyr, vis in (("hidden part passed without a pyramid", pyramids, visible),
                           ("hidden part passed as a pyramid of empties", as_empties, None)):
        feat, idx, dep, part = run_kernel(pyr, base, rows_dev, acts, vis, want_index=True, want_depth=True, want_part=True)
        assert_images(idx, mi, name + ": index")
        assert_images(dep, md, name + ": depth")
        assert_images(part, mp, name + ": part")
        for l in range(LEVELS):
            assert torch.equal(bits(feat[l]), bits(ref[l])), f"{name}: features level {l}"
    # part 0 hidden and nobody else there: the pixel still samples part 0's descriptor 0, with part 0's activation
    feat = run_kernel(pyramids, base, rows_dev, acts, [False, False, False, False],
                      out=[torch.empty((1, h >> l, w >> l, Cc), device="cuda") for l in range(LEVELS)])
    want = torch.tanh(rows_dev[0][0])
    assert torch.equal(bits(feat[0][0, 0, 0]), bits(gather_pyramid(rows_dev[0], [torch.zeros((1, 1, 1), dtype=torch.int32,
                                                                                      device="cuda")], "tanh")[0][0, 0, 0]))
    assert all(torch.equal(f, f[0, 0, 0].expand_as(f)) for f in feat) and torch.allclose(feat[0][0, 0, 0], want, atol=1e-6)


# ---- 2. one part = the plain path --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ACTS)
def test_one_part_equals_the_plain_gather(hip, act):
    (w, h), Cc = (64, 48), 8
    clouds, _, pyramids = small_parts(1, w, h)
    rows = up(rows_of(clouds[0].shape[0], Cc, 0))
    idx, dep = up_levels(pyramids[0][0]), up_levels(pyramids[0][1])
    feat, mi, md, mp = stitch_gather_pyramid([(rows, idx, dep, 0, act)], want_index=True, want_depth=True, want_part=True)
    plain = gather_pyramid(rows, idx, act)
    for l in range(LEVELS):
        assert torch.equal(bits(feat[l]), bits(plain[l])) and torch.equal(mi[l], idx[l]) and torch.equal(bits(md[l]), bits(dep[l]))
        empty = (idx[l] == 0) & (bits(dep[l]) == 0)
        assert bool(empty.any()) and torch.equal(mp[l] == 255, empty) and bool((mp[l][~empty] == 0).all())


# ---- 3. the whole rasteriser, identity placements ------------------------------------------------------------------------------
def test_identity_placements_equal_the_concatenated_cloud_plain_path(hip):
    clouds, M = sm.union_scene()
    (whole_i, whole_d), _ = sm.union_oracle()
    st = StitchedRasterizer(list(clouds))
    assert all(r.cells is None for r in st.parts) and st.id_base == sm.id_bases(sm.COUNTS) and st.n == sum(sm.COUNTS)
    idx, dep, part = st.render_merged(M, sm.W, sm.H, LEVELS, want_part=True)
    one = PointCloudRasterizer(np.concatenate(clouds)).render(M, sm.W, sm.H, LEVELS)
    torch.cuda.synchronize()
    assert_images(idx, whole_i, "stitched vs oracle: index")
    assert_images(dep, whole_d, "stitched vs oracle: depth")
    for l in range(LEVELS):
        assert torch.equal(idx[l], one[0][l]) and torch.equal(bits(dep[l]), bits(one[1][l])), f"level {l} vs the concatenation"
    assert int((part[0] == 1).sum()) > 0 and int((part[0] == 2).sum()) > 0 and int((part[0] == 255).sum()) > 0


def test_identity_placements_equal_the_concatenated_cloud_cell_path(hip):
    W, H = 256, 128
    big = synthetic.make_cloud((1 << 20) + 4096, seed=1)
    clouds = [big, synthetic.make_cloud(15_000, seed=2).copy(), synthetic.make_cloud(5_000, seed=3).copy()]
    front = np.unique(oracle.raster_multiscale(big, camera.total_matrix(synthetic.make_proj(W, H, f=120.0),
                                                                        synthetic.sweep_pose(1))[0], W, H, 1, threads=16)[0][0])
    clouds[1][:64] = big[front[front > 0][:64]]                              # exact ties across parts
    st = StitchedRasterizer(clouds)
    one = PointCloudRasterizer(np.concatenate(clouds))
    assert st.part(0).cells is not None and st.part(1).cells is None and one.cells is not None
    proj = synthetic.make_proj(W, H, f=120.0)
    totals = [camera.total_matrix(proj, synthetic.sweep_pose(k))[0] for k in range(4)]
    won = 0
    for k in range(3):
        a = st.render_merged(totals[k], W, H, LEVELS, next_total=totals[k + 1], want_part=True)
        b = one.render(totals[k], W, H, LEVELS, next_total=totals[k + 1])
        for l in range(LEVELS):
            assert torch.equal(a[0][l], b[0][l]), f"pose {k} index level {l}: {int((a[0][l] != b[0][l]).sum())} pixels differ"
            assert torch.equal(bits(a[1][l]), bits(b[1][l])), f"pose {k} depth level {l}"
        won += int(((a[2][0] == 1) | (a[2][0] == 2)).sum())
    assert won > 0


# ---- 4. placements, hiding, an edited part --------------------------------------------------------------------------------------
def test_placements_hiding_and_an_edited_part(hip):
    clouds, M0 = sm.union_scene()
    W, H = sm.W, sm.H
    base = sm.id_bases(sm.COUNTS)
    labels = cluster_labels(clouds[0], 2, 1_500, 21)
    cent = lambda xyz: xyz.astype(np.float64).mean(0)
    obj_pose = {1: about(cent(clouds[0][labels == 1]), rot_z(0.4), (2.0, 1.0, -1.0))}
    P1 = about(cent(clouds[1]), rot_z(0.3), (3.0, 1.0, -2.0))
    st = StitchedRasterizer(list(clouds), labels=[labels, None, None])
    st.part(0).set_object_pose(1, obj_pose[1])
    st.set_part_pose(1, P1)
    Ms = [object_matrix(M0, P) for P in (None, P1, None)]
    assert not np.array_equal(Ms[1], M0) and Ms[0] is not None
    pyr = [oracle_edit(clouds[0], labels, Ms[0], W, H, obj_pose),
           oracle.raster_multiscale(clouds[1], Ms[1], W, H, LEVELS), oracle.raster_multiscale(clouds[2], Ms[2], W, H, LEVELS)]
    tab = [(pi, pd, base[s]) for s, (pi, pd) in enumerate(pyr)]

    def frame(visible, what):
        for s, v in enumerate(visible):
            st.set_part_visible(s, v)
        idx, dep, part = st.render_merged(M0, W, H, LEVELS, want_part=True)
        mi, md, mp, _ = sm.merge(tab, visible)
        assert_images(idx, mi, what + ": index")
        assert_images(dep, md, what + ": depth")
        assert_images(part, mp, what + ": part")
        return [t.clone() for t in idx], mp
    all_idx, all_part = frame([True, True, True], "all parts")
    assert all(int((all_part[0] == s).sum()) > 0 for s in range(3))
    moved = sm.merge([(pi, pd, base[s]) for s, (pi, pd) in enumerate(sm.union_oracle()[1])])[0]
    assert not np.array_equal(moved[0], all_idx[0][0].cpu().numpy())            # the placement and the object pose change the frame
    frame([True, True, False], "part 2 hidden")
    no1_idx, no1_part = frame([True, False, True], "part 1 hidden, part 2 shown")
    keep = up(all_part[0] == 2)[None]                                         # part 2's pixels keep their ids when part 1 hides
    assert bool(keep.any()) and torch.equal(no1_idx[0][keep], all_idx[0][keep])
    assert bool((no1_idx[0][up(no1_part[0] == 2)[None]] >= base[2]).all())
    again, _ = frame([True, True, True], "all parts again")
    assert all(torch.equal(a, b) for a, b in zip(again, all_idx))


# ---- 5. frames -------------------------------------------------------------------------------------------------------------------
def _descriptors():
    return [synthetic.make_descriptors(n, seed=40 + s) for s, n in enumerate(sm.COUNTS)]


def test_stitched_frame_equals_the_frame_of_the_concatenation(hip):
    clouds, M0 = sm.union_scene()
    W, H = sm.W, sm.H
    desc = _descriptors()
    state = synthetic.make_unet_state(weight_spec())
    sf = StitchedFrameRenderer([{'xyz': c, 'texture_cn': d} for c, d in zip(clouds, desc)], state, W, H, merged_images=True)
    fr = FrameRenderer(np.concatenate(clouds), np.concatenate(desc, 1), state, W, H)
    a = sf.render_total(M0).clone()
    b = fr.render_total(M0)
    torch.cuda.synchronize()
    for l in range(LEVELS):
        assert torch.equal(sf.idx[l], fr.idx[l]) and torch.equal(bits(sf.depth[l]), bits(fr.depth[l])), f"level {l}"
        assert torch.equal(bits(sf.feat[l]), bits(fr.feat[l])), f"features level {l}"
    assert torch.equal(bits(a), bits(b))
    sf.set_part_visible(1, False)                                              # a hidden part changes the frame, showing it restores it
    c = sf.render_total(M0).clone()
    sf.set_part_visible(1, True)
    d = sf.render_total(M0)
    sf.sync()
    torch.cuda.synchronize()
    assert not torch.equal(c, a) and torch.equal(bits(d), bits(a))


def _net_and_textures(tables, state):
    net = UNet()
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    textures = {}
    for tid, t in enumerate(tables):
        tex = PointTexture(8, t.shape[1])
        tex.texture_.data.copy_(torch.from_numpy(t)[None])
        textures[tid] = tex
    model = NetAndTexture(net, textures)
    model.load_textures(list(textures))
    return model.cuda().eval()


def test_ogl_on_a_stitched_scene_takes_the_fast_path(hip):
    clouds, _ = sm.union_scene()
    W, H = sm.W, sm.H
    desc = _descriptors()
    state = synthetic.make_unet_state(weight_spec())
    view = np.eye(4, dtype=np.float32)
    view[1, 3], view[2, 3] = 4.0, 60.0                                         # sm.union_camera's pose
    proj = synthetic.make_proj(W, H, f=60.0)
    st = StitchedScene([Scene(c) for c in clouds])
    st.set_proj_matrix(proj)
    st.set_camera_view(view)
    ogl = OGL.from_model(st, _net_and_textures(desc, state), FMT, (W, H), texture_ids=[0, 1, 2])
    out = ogl.infer()['output']
    assert ogl.last_path == 'fast'
    whole = Scene(np.concatenate(clouds))
    whole.set_proj_matrix(proj)
    whole.set_camera_view(view)
    ref_ogl = OGL.from_model(whole, _net_and_textures([np.concatenate(desc, 1)], state), FMT, (W, H))
    ref = ref_ogl.infer()['output']
    assert ref_ogl.last_path == 'fast'
    sf = StitchedFrameRenderer([{'xyz': c, 'texture_cn': d} for c, d in zip(clouds, desc)], state, W, H, proj_matrix=proj)
    frame = sf.render(view)
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(ref)), "stitched OGL vs OGL on the concatenation"
    torch.testing.assert_close(out, frame, rtol=0, atol=1e-6)                 # the engine of the model vs the frame renderer's
    (whole_i, _), _ = sm.union_oracle()
    maps = MultiscaleRender(st, FMT, (W, H), out_buffer_location='torch').render()
    for l, k in enumerate(FMT.replace(' ', '').split(',')):
        assert torch.equal(maps[k][..., 0].cpu(), torch.from_numpy(oracle.index_to_float(whole_i[l]))), k
    raster = st.rasterizer()
    st.set_part_visible(2, False)                                              # reaches the next frame without a rebuild
    hidden = ogl.infer()['output']
    assert st.rasterizer() is raster and not torch.equal(hidden, out)
    st.set_part_visible(2, True)
    assert torch.equal(bits(ogl.infer()['output']), bits(out))
    with pytest.raises(NotImplementedError, match="stitching"):
        MultiscaleRender(st, "uv_1d_p1, xyz_p1_ds1", (W, H), out_buffer_location='torch').render()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(hip):
    W, H = sm.W, sm.H
    clouds = [synthetic.make_cloud(300, seed=s) for s in range(9)]
    desc = [synthetic.make_descriptors(300, seed=s) for s in range(9)]
    state = synthetic.make_unet_state(weight_spec())
    parts = [{'xyz': c, 'texture_cn': d} for c, d in zip(clouds, desc)]
    with pytest.raises(ValueError, match="stitched frames run one at a time"):
        StitchedFrameRenderer(parts[:2], state, W, H, frames_in_flight=2)
    bad = [parts[0], {'xyz': clouds[1], 'texture_cn': desc[1][:, :299]}, parts[2]]
    with pytest.raises(ValueError, match="part 1: descriptor table has 299 columns for a cloud of 300 points"):
        StitchedFrameRenderer(bad, state, W, H)
    with pytest.raises(ValueError, match="1..8 parts, got 9"):
        StitchedFrameRenderer(parts, state, W, H)
    with pytest.raises(ValueError, match="1..8 parts, got 9"):
        StitchedRasterizer(clouds)
    st = StitchedScene([Scene(c) for c in clouds[:3]])
    st.set_proj_matrix(synthetic.make_proj(W, H, f=60.0))
    model = _net_and_textures([desc[0], desc[1][:, :299], desc[2]], state)
    with pytest.raises(ValueError, match="part 1: descriptor table has 299 points"):
        OGL.from_model(st, model, FMT, (W, H), texture_ids=[0, 1, 2]).infer()
    with pytest.raises(ValueError, match="2 textures for a stitched scene of 3 parts"):
        OGL.from_model(st, model, FMT, (W, H), texture_ids=[0, 1])
    with pytest.raises(NotImplementedError, match="temporal_average with scene stitching"):
        OGL.from_model(st, model, FMT, (W, H), texture_ids=[0, 1, 2], temporal_average=True).infer()
