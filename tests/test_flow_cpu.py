"""CPU: the frame-flow contract (tests/flow_model.py) — its projection pinned to the oracle's pixel and depth bits, the state pairs
of tests/flow_cases.py (each generator asserts what its pair is for), the conventions of the outputs, and the Python refusals that
need no device."""
import numpy as np
import pytest

import oracle
from read_amd import flow
from read_amd.raster import object_matrix
from tests import flow_cases as fc
from tests import flow_model as fm

SIZES = fc.SIZES
# EMPTY and HIDDEN depend on frame A alone (annotate_cases.edited); "outside" = OFF_IMAGE + CLIPPED and VISIBLE + OCCLUDED do not depend
# on where instance 2 is re-posed to.  Figures of an independent prototype of the model.
PROTOTYPE = {(80, 48): dict(empty=1639, seen_or_covered=1167 + 482, outside=419, hidden=133),
             (64, 32): dict(empty=688, seen_or_covered=643 + 355, outside=273, hidden=89),
             (75, 37): dict(empty=1020, seen_or_covered=838 + 438, outside=361, hidden=118)}


def _same_as_oracle(xyz, M, W, H):
    xyz = np.ascontiguousarray(xyz, np.float32)
    pix, dep = oracle.project_points(xyz, M, W, H)
    pr = fm.project(xyz, M, W, H)
    assert np.array_equal(pr['pix'], pix)
    ok = pix >= 0
    assert np.array_equal(pr['depth'][ok].view(np.uint32), dep[ok].view(np.uint32))
    # the pixel is the integer part of (u, v)
    assert np.array_equal(pr['u'][ok].astype(np.int32) + W * pr['v'][ok].astype(np.int32), pix[ok])
    return int(ok.sum())


@pytest.mark.parametrize("W,H", SIZES)
def test_projection_is_the_oracles_in_pixel_and_depth_bits(W, H):
    c = fc.moved(W, H)
    rng = np.random.default_rng(11)
    clouds = [c['xyz'], c['foreign'][0], rng.uniform((-40, -25, -60), (40, 25, 12), (20000, 3)).astype(np.float32)]
    mats = [c['M0_a'], c['M0_b']] + [object_matrix(c['M0_b'], P) for _, P, _ in c['inst_b'] if P is not None]
    inside = 0
    for M in mats:
        for xyz in clouds:
            inside += _same_as_oracle(xyz, M, W, H)
    assert inside > 20000
    # points placed on the image edges and on the two planes: the camera at the origin looks down -z with f = W, so at distance d the
    # image is d wide and d * H / W high; nx = +-1 and ny = +-1 exactly, and steps of one ulp around them
    d = np.float32(16.0)
    edge = []
    for sx in (-0.5, 0.5, 0.0):
        for sy in (-0.5, 0.5, 0.0):
            x, y = np.float32(sx) * d, np.float32(sy) * d * np.float32(H) / np.float32(W)
            for ex in (-1, 0, 1):
                for ey in (-1, 0, 1):
                    edge.append((np.nextafter(x, np.float32(ex * 1e9)) if ex else x, np.nextafter(y, np.float32(ey * 1e9)) if ey else y, -d))
    for z in (-0.1, -1000.0, 0.0, 1e-30, -1e-30, 0.05, -0.0999, -1001.0, -999.0):      # the near and far planes (0.1 / 1000), the eye
        for zz in (np.float32(z), np.nextafter(np.float32(z), np.float32(1e9)), np.nextafter(np.float32(z), np.float32(-1e9))):
            edge.append((0.0, 0.0, zz))
            edge.append((np.float32(0.25) * zz, np.float32(0.1) * zz, zz))
    edge = np.array(edge, np.float32)
    with np.errstate(all='ignore'):
        n_in = _same_as_oracle(edge, c['M0_a'], W, H)
    assert 0 < n_in < edge.shape[0]
    pr = fm.project(edge, c['M0_a'], W, H)
    assert (pr['pix'][pr['nx'] == 1] == -1).all() and (pr['nx'] == 1).any(), "nx = 1 is inside the cube and outside the image"


@pytest.mark.parametrize("W,H", SIZES)
def test_moved_holds_every_state(W, H):
    c = fc.moved(W, H)                                               # the generator's own assertions: >= 20 pixels per state, >= 10 ties
    out, cnt = c['out'], c['out']['counts']
    want = PROTOTYPE[(W, H)]
    assert cnt[fm.EMPTY] == want['empty'] and cnt[fm.HIDDEN] == want['hidden']
    assert cnt[fm.OFF_IMAGE] + cnt[fm.CLIPPED] == want['outside']
    assert cnt[fm.VISIBLE] + cnt[fm.OCCLUDED] == want['seen_or_covered']
    assert out['unmatched'] == 0 and cnt[fm.UNMATCHED] == 0 and cnt[7] == 0
    st, fl, dn = out['state'], out['flow'], out['depth_next']
    still = ~np.isin(st, (fm.VISIBLE, fm.OCCLUDED, fm.OFF_IMAGE))
    assert not fl[still].view(np.uint32).any() and not dn[still].view(np.uint32).any(), "+0.0f outside the three moving states"
    assert out['state'].dtype == np.int32 and fl.dtype == np.float32 and fl.shape == (H, W, 2) and out['stats'].dtype == np.int32
    # VISIBLE means what it says: the pixel the point lands on in B holds the same id at the depth the model gives
    q = _target(c, out).reshape(H, W)
    vis = st == fm.VISIBLE
    assert (q[vis] >= 0).all() and np.array_equal(c['idx_b'].reshape(-1)[q[vis]], c['idx_a'][vis])
    assert np.array_equal(dn[vis].view(np.uint32), c['depth_b'].reshape(-1)[q[vis]].view(np.uint32))
    occ = st == fm.OCCLUDED
    assert (q[occ] >= 0).all() and (q[np.isin(st, (fm.OFF_IMAGE, fm.CLIPPED))] == -1).all()
    covered = c['depth_b'].reshape(-1)[q[occ]].view(np.uint32) <= dn[occ].view(np.uint32)
    assert covered.all(), "an occluded point lies at or behind what B shows at its pixel"


def _target(c, out):
    """The pixel q of frame B per pixel of A, from the model's own projection under B's drawer matrices."""
    W, H = c['W'], c['H']
    _, _, pt = fm.resolve(c['xyz'], c['labels'], c['foreign'], c['idx_a'].reshape(-1), c['depth_a'].reshape(-1).view(np.uint32))
    Mb = np.broadcast_to(c['M0_b'].reshape(16), (W * H, 16)).copy()
    for i, (_, P, _) in enumerate(c['inst_b']):
        Mb[out['won'].reshape(-1) == i] = object_matrix(c['M0_b'], P).reshape(16)
    return fm.project(pt, Mb, W, H)['pix']


@pytest.mark.parametrize("W,H", SIZES)
def test_consistency_of_counts_and_rows(W, H):
    for name in ("moved", "foreign_moves", "identity", "one_moved_instance", "no_instances"):
        c = getattr(fc, name)(W, H)
        out = c['out']
        assert out['counts'].sum() == W * H and out['counts'][7] == 0
        assert np.array_equal(out['counts'][:7], np.bincount(out['state'].reshape(-1), minlength=7))
        for i, row in enumerate(out['stats']):
            assert row[fm.PX] == (out['won'] == i).sum()
            if c['inst_b'][i][2]:
                assert row[fm.N_VISIBLE] + row[fm.N_OCCLUDED] + row[fm.N_OUTSIDE] == row[fm.PX], (name, i, row)
            else:
                assert row[1:].sum() == 0 and (out['state'][out['won'] == i] == fm.HIDDEN).all(), "hidden in B: px only"
        assert out['stats'][:, fm.PX].sum() == (out['won'] >= 0).sum()


@pytest.mark.parametrize("W,H", SIZES)
def test_identity_static_camera_and_no_instances(W, H):
    c = fc.identity(W, H)
    assert c['out']['counts'][fm.VISIBLE] + c['out']['counts'][fm.EMPTY] == W * H
    c = fc.one_moved_instance(W, H)
    assert c['out']['stats'][6, fm.PX] > 0 and c['out']['counts'][fm.HIDDEN] == 0
    c = fc.no_instances(W, H)
    assert c['out']['counts'][fm.VISIBLE] > 0 and c['out']['counts'][fm.OFF_IMAGE] > 0 and c['out']['unmatched'] == 0
    c = fc.foreign_moves(W, H)
    assert c['out']['stats'][5, fm.N_VISIBLE] + c['out']['stats'][5, fm.N_OCCLUDED] >= fc.MIN_PIXELS


def test_the_wide_case_reaches_past_one_turn():
    c = fc.wide()
    assert c['W'] * c['H'] > 512 * 256 and c['out']['counts'].sum() == c['W'] * c['H'] and c['out']['unmatched'] == 0


def test_a_mismatched_list_and_a_wrong_camera_are_counted():
    W, H = 80, 48
    c = fc.moved(W, H)
    a, b = fc.mismatched(c)
    out = fm.flow(c['xyz'], c['labels'], c['foreign'], a, b, c['M0_a'], c['M0_b'], W, H, c['idx_a'], c['depth_a'], c['idx_b'], c['depth_b'])
    px5 = c['out']['stats'][5, fm.PX]
    assert out['unmatched'] == px5 > 0 and out['counts'][fm.UNMATCHED] == px5 and out['stats'][5, fm.PX] == 0
    sel = out['state'] == fm.UNMATCHED
    assert np.array_equal(sel, c['out']['won'] == 5) and not out['flow'][sel].view(np.uint32).any()
    # the static check: another camera for A than its frame was drawn with leaves static pixels without a drawer
    out = fm.flow(c['xyz'], c['labels'], c['foreign'], c['inst_a'], c['inst_b'], c['M0_b'], c['M0_b'], W, H, c['idx_a'], c['depth_a'],
                  c['idx_b'], c['depth_b'])
    assert out['unmatched'] > 1000
    # an id that no range holds
    idx = c['idx_a'].copy()
    filled = np.flatnonzero(~((idx.reshape(-1) == 0) & (c['depth_a'].reshape(-1).view(np.uint32) == 0)))
    idx.reshape(-1)[filled[:3]] = c['xyz'].shape[0] + 400 + 5
    out = fm.flow(c['xyz'], c['labels'], c['foreign'], c['inst_a'], c['inst_b'], c['M0_a'], c['M0_b'], W, H, idx, c['depth_a'],
                  c['idx_b'], c['depth_b'])
    assert out['unmatched'] == 3 and (out['state'].reshape(-1)[filled[:3]] == fm.UNMATCHED).all()


def test_count_zero_on_a_frame_with_objects():
    """count = 0 on the edited frame: object pixels are UNMATCHED, static pixels still flow."""
    W, H = 64, 32
    c = fc.moved(W, H)
    out = fm.flow(c['xyz'], c['labels'], c['foreign'], [], [], c['M0_a'], c['M0_b'], W, H, c['idx_a'], c['depth_a'], c['idx_b'], c['depth_b'])
    ref = c['out']
    assert out['unmatched'] == (ref['won'] >= 0).sum() > 0 and out['stats'].shape == (0, 4)
    static = ref['won'] < 0
    assert np.array_equal(out['state'][static], ref['state'][static])
    assert np.array_equal(out['flow'][static].view(np.uint32), ref['flow'][static].view(np.uint32))


def test_names_and_python_refusals_without_a_device():
    from read_amd.render import Scene, StitchedScene
    assert flow.STATE_NAMES == ("empty", "visible", "occluded", "off_image", "clipped", "hidden", "unmatched")
    assert (flow.EMPTY, flow.VISIBLE, flow.OCCLUDED, flow.OFF_IMAGE, flow.CLIPPED, flow.HIDDEN, flow.UNMATCHED) == tuple(range(7))
    assert (fm.EMPTY, fm.VISIBLE, fm.OCCLUDED, fm.OFF_IMAGE, fm.CLIPPED, fm.HIDDEN, fm.UNMATCHED) == tuple(range(7))
    assert flow.STATES == fm.STATES == 8 and flow.STATS == fm.STATS == 4 and flow.STAT_NAMES[fm.N_OUTSIDE] == "outside"
    s = Scene(np.zeros((4, 3), np.float32))
    s.set_panorama(200.0)
    with pytest.raises(NotImplementedError, match="panorama.*capture_frame"):
        s.capture_frame((64, 32))
    s.set_panorama(None)
    s.set_lens(0, (0.1, 0.0, 0.0, 0.0, 0.0))
    with pytest.raises(NotImplementedError, match="lens.*capture_frame"):
        s.capture_frame((64, 32))
    s.set_lens(None)
    s.set_point_drop(0.5, 1)
    with pytest.raises(NotImplementedError, match="GL-twin.*capture_frame"):
        s.capture_frame((64, 32))
    s.set_point_drop(0.0)
    with pytest.raises(NotImplementedError, match="level 1 with capture_frame"):
        s.capture_frame((64, 32), level=1)
    with pytest.raises(ValueError, match="no point cloud"):
        Scene().capture_frame((64, 32))
    st = object.__new__(StitchedScene)
    with pytest.raises(NotImplementedError, match="capture_frame on a StitchedScene"):
        st.capture_frame((64, 32))
    with pytest.raises(NotImplementedError, match="flow_between on a StitchedScene"):
        st.flow_between(None, None)
    f = flow.FrameFlow(None, None, None, None, None, [3, 4], None)
    assert f.handles == [3, 4]
