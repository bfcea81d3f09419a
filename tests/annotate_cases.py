"""The scenes of the annotation tests (tests/test_annotate_cpu.py, tests/test_gpu_annotate.py).  Each generator asserts on the
MODEL's output (tests/annotate_model.py) that the frame holds what it is for, so a test cannot pass vacuously.

A case is a dict: xyz, labels (or None), foreign (list of (m,3) arrays), inst = [(k, P, visible)], M0, W, H and the model's frame
(idx, depth) and annotation (obj, inst_img, stats, unmatched, won)."""
import functools

import numpy as np

from read_amd import camera, synthetic
from tests import annotate_model as am


def translation(t):
    P = np.eye(4, dtype=np.float32)
    P[:3, 3] = np.asarray(t, np.float32)
    return P


def _blob(rng, n, centre, r):
    v = rng.standard_normal((n, 3))
    v *= (r * rng.random(n) ** (1 / 3) / np.linalg.norm(v, axis=1))[:, None]
    return (v + np.asarray(centre)).astype(np.float32)


def _camera(W, H):
    """The camera at the origin looking down -z with f = W: at distance d the image is d wide and d * H / W high."""
    return camera.total_matrix(synthetic.make_proj(W, H, f=float(W)), synthetic.sweep_pose(0))[0]


def _finish(case):
    W, H = case['W'], case['H']
    case['idx'], case['depth'] = am.render(case['xyz'], case['labels'], case['foreign'], case['inst'], case['M0'], W, H)
    obj, inst_img, stats, unmatched, won = am.annotate(case['xyz'], case['labels'], case['foreign'], case['inst'], case['M0'], W, H,
                                                       case['idx'], case['depth'], case.get('values'))
    case.update(obj=obj, inst_img=inst_img, stats=stats, unmatched=unmatched, won=won)
    assert unmatched == 0, unmatched
    return case


def _cloud(n_static, seed):
    """Object 1 = ids 0..599 (point 0 at its front), then the static wall (top of the image left empty), then object 2."""
    rng = np.random.default_rng(seed)
    o1 = _blob(rng, 600, (-4.0, -1.0, -20.0), 1.5)
    o1[0] = (-4.0, -1.0, -18.0)
    wall = np.empty((n_static, 3), np.float32)
    wall[:, 0] = rng.uniform(-15, 15, n_static)
    wall[:, 1] = rng.uniform(-9, 2, n_static)
    wall[:, 2] = rng.uniform(-31, -29, n_static)
    o2 = _blob(rng, 500, (5.0, -2.0, -22.0), 1.5)
    xyz = np.concatenate([o1, wall, o2]).astype(np.float32)
    labels = np.concatenate([np.full(600, 1), np.zeros(n_static), np.full(500, 2)]).astype(np.int32)
    return xyz, labels, _blob(rng, 400, (0.0, 0.0, 0.0), 1.0)


SEVEN = [(1, None, True),                                    # 0 object 1 where it is
         (2, None, True),                                    # 1 object 2 where it is
         (1, translation((8.0, 3.0, 4.0)), True),            # 2 a copy of object 1 ...
         (1, translation((8.0, 3.0, 4.0)), True),            # 3 ... and its identical twin: every pixel of the pair is a tie
         (2, translation((-9.0, 1.0, 12.0)), False),         # 4 hidden, close to the camera: would win pixels
         (3, translation((-1.0, -1.5, -12.0)), True),        # 5 the foreign object
         (2, translation((-15.0, 0.0, 2.0)), True)]          # 6 object 2 across the left image edge: 0 < in_pts < n_pts


@functools.lru_cache(maxsize=None)
def edited(W, H, n_static=4500):
    """Two labelled clusters, one foreign object, seven instances: every situation of the contract in one frame."""
    xyz, labels, cut = _cloud(n_static, 3)
    case = _finish(dict(xyz=xyz, labels=labels, foreign=[cut], inst=list(SEVEN), M0=_camera(W, H), W=W, H=H,
                        values=np.array([10, 11, 12, 13, 14, 15, 16], np.int32)))
    obj, won, stats = case['obj'], case['won'], case['stats']
    assert (obj == -1).sum() > 20 and (obj == 0).sum() > 20 and (obj >= 1).sum() > 20, "empty, static and object pixels"
    twin = am.key_matches(xyz, labels, [cut], SEVEN, case['M0'], W, H, 3)          # where instance 3 holds the frame's key too
    ties = int(((won == 2) & twin).sum())
    assert ties >= 10 and stats[3, am.VIS_PX] == 0, f"{ties} tie pixels go to the lower list entry"
    shown = list(SEVEN)
    shown[4] = (2, SEVEN[4][1], True)
    won_shown = am.first_instance_by_key_image(xyz, labels, [cut], shown, case['M0'], W, H)
    assert (won_shown == 4).sum() > 0 and (won == 4).sum() == 0 and stats[4, am.N_PTS] == 500, "the hidden instance would win pixels"
    assert np.array_equal(stats[4], am.empty_row(500))
    assert 0 < stats[6, am.IN_PTS] < stats[6, am.N_PTS], "an instance cut by the image edge"
    assert stats[5, am.VIS_PX] > 0 and stats[0, am.VIS_PX] > 0, "a foreign and an own instance are both seen"
    assert (case['idx'] >= xyz.shape[0]).sum() > 0
    filled = ~((case['idx'] == 0) & (case['depth'].view(np.uint32) == 0))
    assert labels[0] >= 1 and ((case['idx'] == 0) & filled).sum() >= 1, "point id 0 belongs to an object and wins a pixel"
    assert (case['inst_img'][won >= 0] == case['values'][won[won >= 0]]).all()
    return case


@functools.lru_cache(maxsize=None)
def unlabelled(W, H):
    """A cloud without labels plus a foreign object drawn twice (one copy hidden)."""
    xyz, _, cut = _cloud(4500, 5)
    inst = [(1, translation((2.0, -1.0, -14.0)), True), (1, translation((-3.0, 0.0, -10.0)), False),
            (1, translation((-6.0, -2.0, -25.0)), True)]
    case = _finish(dict(xyz=xyz, labels=None, foreign=[cut], inst=inst, M0=_camera(W, H), W=W, H=H))
    assert case['stats'][0, am.VIS_PX] > 0 and case['stats'][2, am.VIS_PX] > 0 and (case['obj'] == 0).sum() > 0
    assert set(np.unique(case['obj'])) == {-1, 0, 1}
    return case


@functools.lru_cache(maxsize=None)
def no_instances(W, H):
    """I = 0: a cloud without labels, objects or instances."""
    xyz, _, _ = _cloud(4500, 7)
    case = _finish(dict(xyz=xyz, labels=None, foreign=[], inst=[], M0=_camera(W, H), W=W, H=H))
    assert case['stats'].shape == (0, 12) and set(np.unique(case['obj'])) == {-1, 0} and (case['inst_img'] == -1).all()
    return case


@functools.lru_cache(maxsize=None)
def seventy(W, H):
    """70 instances: the seven above and 63 more copies of object 1, so the extents walk takes three launches; four hidden ones at
    the batch boundaries."""
    xyz, labels, cut = _cloud(4500, 3)
    rng = np.random.default_rng(9)
    inst = list(SEVEN) + [(1, translation((rng.uniform(-2, 16), rng.uniform(-3, 4), rng.uniform(-6, 8))), i not in (31, 32, 33, 64))
                          for i in range(7, 70)]
    case = _finish(dict(xyz=xyz, labels=labels, foreign=[cut], inst=inst, M0=_camera(W, H), W=W, H=H))
    assert len(inst) == 70 and (case['stats'][7:, am.VIS_PX] > 0).sum() > 20 and case['stats'][31:34, am.IN_PTS].sum() == 0
    return case
