"""CPU: object selection — the NumPy model (tests/select_model.py) against a plain per-point loop, the edge cases
of the contract on the model, box_matrix, the C ABI's argument checks (no GPU needed: they precede every launch), and the conditions
on the inputs of the GPU vote test (tests/select_cases.py), so that it cannot pass on a trivial case.  The kernels are held to the
model on the GPU (tests/test_gpu_select.py)."""
import ctypes as C

import numpy as np
import pytest

import oracle
from read_amd import _lib, synthetic
from read_amd.select import MAX_BOXES, MAX_VIEWS, box_matrix
from tests import select_cases as sc
from tests import select_model as sm

f32 = np.float32
FAKE = 1 << 20          # a 256-byte aligned non-null address: the calls below fail on their arguments and never touch it


# ---- the model against a per-point loop --------------------------------------------------------------------------------------------
def _dot4(M, r, p):
    return M[4 * r] * p[0] + M[4 * r + 1] * p[1] + M[4 * r + 2] * p[2] + M[4 * r + 3] * f32(1)


def _loop_boxes(xyz, boxes, label_of, labels_in):
    out = np.empty(len(xyz), np.int32)
    for i, p in enumerate(xyz):
        out[i] = 0 if labels_in is None else labels_in[i]
        for k, A in enumerate(boxes):
            if all(abs(_dot4(A, r, p)) <= f32(1) for r in range(3)):
                out[i] = label_of[k]
                break
    return out


def _loop_project(M, p, W, H):
    c = [_dot4(M, r, p) for r in range(4)]
    nx, ny, nz = c[0] / c[3], c[1] / c[3], c[2] / c[3]
    if not (nx >= -1 and nx <= 1 and ny >= -1 and ny <= 1 and nz >= -1 and nz <= 1):
        return -1, c[3]
    xx, yy = int((f32(W) * (nx + f32(1))) * f32(0.5)), int((f32(H) * (f32(1) - ny)) * f32(0.5))
    return (yy * W + xx if 0 <= xx < W and 0 <= yy < H else -1), c[3]


def _loop_view(state, xyz, M, W, H, idx0, depth0, mask, scale, slack):
    idx0, bits, mask = idx0.reshape(-1), depth0.reshape(-1).view(np.uint32), mask.reshape(-1)
    near = np.array([f32(np.inf) if idx0[p] == 0 and bits[p] == 0 else _dot4(M, 3, xyz[idx0[p]]) for p in range(W * H)], f32)
    out = state.copy()
    for i, p in enumerate(xyz):
        pix, w = _loop_project(M, p, W, H)
        if pix < 0:
            continue
        lim = near[pix] * scale + slack
        if not w <= lim:
            continue
        cand, hit, seen = int(state[i]) >> 16, (int(state[i]) >> 8) & 255, int(state[i]) & 255
        seen += 1
        m = int(mask[pix])
        if m != 0 and cand == 0:
            cand, hit = m, 1
        elif m != 0 and m == cand:
            hit += 1
        out[i] = cand << 16 | hit << 8 | seen
    return near, out


def _loop_finish(state, min_hits, num, den, labels_in):
    out = np.empty(len(state), np.int32)
    for i, s in enumerate(state):
        cand, hit, seen = int(s) >> 16, (int(s) >> 8) & 255, int(s) & 255
        ok = cand != 0 and hit >= min_hits and hit * den >= num * seen
        out[i] = cand if ok else (0 if labels_in is None else labels_in[i])
    return out


def test_model_equals_a_per_point_loop():
    n = 2000
    rng = np.random.default_rng(5)
    with np.errstate(all='ignore'):
        cloud = synthetic.make_cloud(n, 4)
        boxes, _ = sc.random_boxes(5, 9)
        label_of = np.array([3, 1, 0, 3, 7], np.int32)
        labels_in = rng.integers(0, 4, n).astype(np.int32)
        want = _loop_boxes(cloud, boxes, label_of, labels_in)
        assert 0.01 * n <= int((want != labels_in).sum())
        assert np.array_equal(sm.label_boxes(cloud, boxes, label_of, labels_in), want)
        assert np.array_equal(sm.label_boxes(cloud, boxes), _loop_boxes(cloud, boxes, np.arange(1, 6), None))
        # three posed views of a street
        case = sc.vote_case(n_views=3)
        W, H = case['W'], case['H']
        xyz = synthetic.make_street_cloud(n)
        scale, slack = sm.scale_of(case['rel']), f32(case['slack'])
        state_m = np.zeros(n, np.uint32)
        state_l = np.zeros(n, np.uint32)
        for M, mask in zip(case['totals'], case['masks']):
            idx, dep = oracle.raster_multiscale(xyz, M.reshape(4, 4), W, H, 1)
            near_l, state_l = _loop_view(state_l, xyz, M, W, H, idx[0], dep[0], mask, scale, slack)
            near_m = sm.near_image(xyz, M, idx[0], dep[0])
            assert np.array_equal(near_m.view(np.uint32), near_l.view(np.uint32))
            state_m = sm.vote(state_m, xyz, M, W, H, near_m, mask, scale, slack)
            assert np.array_equal(state_m, state_l)
        assert len(np.unique(state_m)) > 6 and (state_m >> 16).max() == 2
        for min_hits, ratio in ((1, (0, 1)), (2, (1, 2)), (3, (1, 1)), (1, (2, 3))):
            assert np.array_equal(sm.finish(state_m, min_hits, ratio, labels_in), _loop_finish(state_l, min_hits, *ratio, labels_in))
            assert np.array_equal(sm.finish(state_m, min_hits, ratio), _loop_finish(state_l, min_hits, *ratio, None))


# ---- boxes: the edges of the contract -------------------------------------------------------------------------------------------------
def test_faces_are_inclusive_and_the_next_float_is_outside():
    box, pts, inside = sc.face_points()
    assert np.array_equal(box.reshape(3, 4), np.concatenate([0.5 * np.eye(3, dtype=f32), np.zeros((3, 1), f32)], 1))
    assert pts[0, 0] == f32(2) and pts[1, 0] == np.nextafter(f32(2), f32(3)) and len(pts) == 12
    assert np.array_equal(sm.inside_box(pts, box[0]), inside)
    assert np.array_equal(sm.label_boxes(pts, box), inside.astype(np.int32))


def test_nonfinite_points_are_outside():
    box, _, _ = sc.face_points()
    pts = sc.nonfinite_points()
    assert len(pts) == 9 and not sm.inside_box(pts, box[0]).any()
    # also under a rotated box, where an infinity meets a zero or an opposite infinity
    rot = box_matrix((0, 0, 0), (4, 4, 4), yaw=0.7)
    assert not sm.inside_box(pts, rot).any()
    assert np.array_equal(sm.label_boxes(pts, box, labels_in=np.full(9, 5)), np.full(9, 5))


def test_overlap_goes_to_the_smallest_k_and_labels_repeat_and_zero_carves():
    xyz = np.array([[0, 0, 0], [3, 0, 0], [-3, 0, 0], [9, 9, 9]], f32)
    big, left, right = box_matrix((0, 0, 0), (8, 2, 2)), box_matrix((-3, 0, 0), (2, 2, 2)), box_matrix((3, 0, 0), (2, 2, 2))
    assert sm.label_boxes(xyz, [left, big, right]).tolist() == [2, 2, 1, 0]          # -3 lies in left (k = 0) and big (k = 1)
    assert sm.label_boxes(xyz, [big, left, right]).tolist() == [1, 1, 1, 0]
    assert sm.label_boxes(xyz, [left, right, big], label_of=[4, 4, 9]).tolist() == [9, 4, 4, 0]      # two boxes, one label
    # label 0 carves the middle back out of the big box; elsewhere labels_in stays
    assert sm.label_boxes(xyz, [box_matrix((0, 0, 0), (2, 2, 2)), big], label_of=[0, 6], labels_in=[7, 7, 7, 7]).tolist() == \
        [0, 6, 6, 7]
    assert sm.label_boxes(xyz, np.zeros((0, 12), f32), labels_in=[1, 2, 3, 4]).tolist() == [1, 2, 3, 4]
    assert sm.label_boxes(xyz, np.zeros((0, 12), f32)).tolist() == [0, 0, 0, 0]


# ---- box_matrix ------------------------------------------------------------------------------------------------------------------------
def test_box_matrix_r_and_yaw_agree():
    for yaw in (0.0, 0.3, -1.2, 2.9):
        c, s = np.cos(yaw), np.sin(yaw)
        R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
        a, b = box_matrix((1, 2, 3), (2, 3, 4), yaw=yaw), box_matrix((1, 2, 3), (2, 3, 4), R=R)
        assert a.dtype == f32 and a.shape == (3, 4) and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # yaw turns the box's x axis towards -z, like synthetic.sweep_pose
    A = box_matrix((0, 0, 0), (2, 2, 2), yaw=np.pi / 2)
    assert np.allclose(A[:, :3] @ np.array([0, 0, -1.0]), [1, 0, 0], atol=1e-6)
    assert np.array_equal(box_matrix((0, 0, 0), (4, 4, 4)), box_matrix((0, 0, 0), (4, 4, 4), R=np.eye(3)))


def test_rotated_box_contains_its_shrunk_corners_and_not_the_grown_ones():
    rng = np.random.default_rng(8)
    for _ in range(20):
        center, size = rng.uniform(-50, 50, 3), rng.uniform(0.5, 20, 3)
        R, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        A = box_matrix(center, size, R=R)
        signs = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64)
        for grow, want in ((1 - 1e-3, True), (1 + 1e-3, False)):
            corners = (center + (signs * 0.5 * size * grow) @ R.T).astype(f32)
            assert (sm.inside_box(corners, A) == want).all()


def test_box_matrix_refusals():
    for size in ((1, 0, 1), (1, -2, 1), (1, np.nan, 1), (1, 1), (1, np.inf, 1)):
        with pytest.raises(ValueError):
            box_matrix((0, 0, 0), size)
    with pytest.raises(ValueError, match="mutually exclusive"):
        box_matrix((0, 0, 0), (1, 1, 1), R=np.eye(3), yaw=0.1)
    with pytest.raises(ValueError):
        box_matrix((0, 0), (1, 1, 1))
    with pytest.raises(ValueError):
        box_matrix((0, 0, 0), (1, 1, 1), R=np.eye(4))
    assert MAX_BOXES == sm.MAX_BOXES == 1024 and MAX_VIEWS == sm.MAX_VIEWS == 255


# ---- voting: hand-built views ------------------------------------------------------------------------------------------------------------
W2, H2 = 4, 2
M_ID = synthetic.make_proj(W2, H2, f=2.0).reshape(16)          # camera at the origin looking down -z: clip w = -z


def _view_of(xyz):
    idx, dep = oracle.raster_multiscale(np.asarray(xyz, f32), M_ID.reshape(4, 4), W2, H2, 1)
    return idx[0], dep[0]


def _run(xyz, masks, scale=f32(1), slack=f32(0)):
    xyz = np.asarray(xyz, f32)
    idx, dep = _view_of(xyz)
    near = sm.near_image(xyz, M_ID, idx, dep)
    state = np.zeros(len(xyz), np.uint32)
    for m in masks:
        state = sm.vote(state, xyz, M_ID, W2, H2, near, np.full((H2, W2), m, np.int32), scale, slack)
    return state


def test_first_candidate_rule_conflict_and_thresholds():
    front = [[0.1, 0.1, -2.0]]
    assert _run(front, [0, 0]).tolist() == [2]                                         # seen twice, never named
    assert _run(front, [5, 5, 0]).tolist() == [5 << 16 | 2 << 8 | 3]
    assert _run(front, [0, 5, 5]).tolist() == [5 << 16 | 2 << 8 | 3]                   # the candidate may come late
    # the first label stays the candidate although a later one is named more often: seen, not hit
    s = _run(front, [5, 7, 7, 7])
    assert s.tolist() == [5 << 16 | 1 << 8 | 4]
    assert sm.finish(s, 1, (0, 1)).tolist() == [5] and sm.finish(s, 1, (1, 2)).tolist() == [0]
    assert sm.finish(s, 1, (1, 4)).tolist() == [5]                                     # hit * den >= num * seen at equality
    assert sm.finish(s, 2, (0, 1)).tolist() == [0]                                     # min_hits
    assert sm.finish(s, 2, (0, 1), labels_in=[9]).tolist() == [9]
    s = _run(front, [5, 5, 0, 0])
    assert sm.finish(s, 2, (1, 2)).tolist() == [5] and sm.finish(s, 3, (1, 2)).tolist() == [0]
    assert sm.finish(s, 2, (2, 3)).tolist() == [0] and sm.finish(s, 2, (1, 1)).tolist() == [0]
    assert sm.finish(np.array([0], np.uint32), 1, (0, 1), labels_in=[4]).tolist() == [4]      # no candidate: cand != 0 fails


def test_empty_pixel_is_infinitely_far_and_the_window_is_inclusive():
    # point 0 wins its pixel at distance 2; point 1 lies behind it in the same pixel at distance 2.5; point 2 is off screen
    xyz = np.array([[0.1, 0.1, -2.0], [0.125, 0.125, -2.5], [0.0, 50.0, -2.0]], f32)
    idx, dep = _view_of(xyz)
    near = sm.near_image(xyz, M_ID, idx, dep)
    assert np.isposinf(near).sum() == W2 * H2 - 1 and near[np.isfinite(near)].tolist() == [2.0]
    pix = sm.project(xyz, M_ID, W2, H2)
    assert pix[0] == pix[1] >= 0 and pix[2] == -1
    assert _run(xyz, [3]).tolist() == [3 << 16 | 1 << 8 | 1, 0, 0]
    # c3 == lim passes, one ulp less does not: slack alone (2 + 0.5), rel alone (2 * 1.25)
    assert _run(xyz, [3], slack=f32(0.5)).tolist()[1] == 3 << 16 | 1 << 8 | 1
    assert _run(xyz, [3], slack=f32(0.5) - f32(2.0 ** -22)).tolist()[1] == 0          # one ulp of [2, 4) less: 2.4999998
    assert _run(xyz, [3], scale=sm.scale_of(0.25)).tolist()[1] == 3 << 16 | 1 << 8 | 1
    assert _run(xyz, [3], scale=np.nextafter(f32(1.25), f32(1))).tolist()[1] == 0
    # a point alone in a frame rendered without it: its pixel is empty there, near = +inf, it is seen
    lone = np.array([[0.1, 0.1, -2.0], [-0.3, -0.2, -900.0]], f32)
    idx, dep = _view_of(lone[:1])
    near = sm.near_image(lone, M_ID, idx, dep)
    assert sm.vote(np.zeros(2, np.uint32), lone, M_ID, W2, H2, near, np.ones((H2, W2), np.int32), f32(1), f32(0)).tolist() == \
        [1 << 16 | 1 << 8 | 1] * 2


# ---- the C ABI: exported, bound, refusing bad arguments before any device work -----------------------------------------------------------
NEW = ("read_select_boxes", "read_select_near", "read_select_vote", "read_select_finish")
_M = np.eye(4, dtype=f32).reshape(16)
_MP = _M.ctypes.data_as(C.POINTER(C.c_float))


def _einval(rc, name, word):
    msg = _lib.lib().read_last_error().decode()
    assert rc == -22 and name in msg and word in msg, (rc, msg)


def test_symbols_are_exported_and_bound():
    L = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
    assert _lib.lib().read_abi_version() == 3


def test_select_boxes_refuses_bad_arguments():
    L = _lib.lib()
    for xyz, boxes, lab, out in ((None, FAKE, FAKE, FAKE), (FAKE, None, FAKE, FAKE), (FAKE, FAKE, None, FAKE), (FAKE, FAKE, FAKE, None)):
        _einval(L.read_select_boxes(xyz, 10, boxes, lab, 2, None, out, None), "read_select_boxes", "null")
    for K in (-1, 1025):
        _einval(L.read_select_boxes(FAKE, 10, FAKE, FAKE, K, None, FAKE, None), "read_select_boxes", "K =")
    _einval(L.read_select_boxes(FAKE, -1, FAKE, FAKE, 1, None, FAKE, None), "read_select_boxes", "n =")
    assert L.read_select_boxes(None, 0, None, None, 0, None, None, None) == 0
    assert L.read_select_boxes(None, 0, None, None, 1024, None, None, None) == 0


def test_select_near_and_vote_refuse_bad_arguments():
    L = _lib.lib()
    for args in ((None, FAKE, FAKE, FAKE), (FAKE, None, FAKE, FAKE), (FAKE, FAKE, None, FAKE), (FAKE, FAKE, FAKE, None)):
        _einval(L.read_select_near(args[0], 10, _MP, 64, 48, args[1], args[2], args[3], None), "read_select_near", "null")
        _einval(L.read_select_vote(args[0], 10, _MP, 64, 48, args[1], args[2], 1.05, 0.0, args[3], None), "read_select_vote", "null")
    _einval(L.read_select_near(FAKE, 10, None, 64, 48, FAKE, FAKE, FAKE, None), "read_select_near", "M_host")
    _einval(L.read_select_vote(FAKE, 10, None, 64, 48, FAKE, FAKE, 1.05, 0.0, FAKE, None), "read_select_vote", "M_host")
    for W, H in ((65536, 32768), (0, 48), (64, -1)):                                   # W * H >= 2^31, or no image
        _einval(L.read_select_near(FAKE, 10, _MP, W, H, FAKE, FAKE, FAKE, None), "read_select_near", "W/H")
        _einval(L.read_select_vote(FAKE, 10, _MP, W, H, FAKE, FAKE, 1.05, 0.0, FAKE, None), "read_select_vote", "W/H")
    for scale in (0.999, float('nan'), float('inf'), -2.0):
        _einval(L.read_select_vote(FAKE, 10, _MP, 64, 48, FAKE, FAKE, scale, 0.0, FAKE, None), "read_select_vote", "scale")
    for slack in (-0.001, float('nan'), float('inf')):
        _einval(L.read_select_vote(FAKE, 10, _MP, 64, 48, FAKE, FAKE, 1.0, slack, FAKE, None), "read_select_vote", "slack")
    assert L.read_select_near(None, 0, _MP, 64, 48, None, None, None, None) == 0
    assert L.read_select_vote(None, 0, _MP, 64, 48, None, None, 1.0, 0.0, None, None) == 0


def test_select_finish_refuses_bad_arguments():
    L = _lib.lib()
    _einval(L.read_select_finish(None, 10, 1, 1, 2, None, FAKE, None), "read_select_finish", "null")
    _einval(L.read_select_finish(FAKE, 10, 1, 1, 2, None, None, None), "read_select_finish", "null")
    for min_hits in (0, 256, -3):
        _einval(L.read_select_finish(FAKE, 10, min_hits, 1, 2, None, FAKE, None), "read_select_finish", "min_hits")
    for den in (0, -1):
        _einval(L.read_select_finish(FAKE, 10, 1, 0, den, None, FAKE, None), "read_select_finish", "den")
    for num, den in ((-1, 2), (3, 2)):
        _einval(L.read_select_finish(FAKE, 10, 1, num, den, None, FAKE, None), "read_select_finish", "num")
    assert L.read_select_finish(None, 0, 1, 1, 2, None, None, None) == 0
    assert L.read_select_finish(None, 0, 255, 2, 2, None, None, None) == 0


def test_python_layer_refuses_before_the_device():
    from read_amd.render import Scene, StitchedScene
    scene = Scene(synthetic.make_cloud(100, 1))
    stitched = StitchedScene([scene])
    with pytest.raises(NotImplementedError, match="StitchedScene"):
        stitched.select_boxes(np.zeros((1, 12), f32))
    with pytest.raises(NotImplementedError, match="StitchedScene"):
        stitched.select_masks([np.eye(4)], [np.zeros((48, 64), np.int32)], (64, 48))
    scene.set_panorama(180.0)
    with pytest.raises(NotImplementedError, match="panorama"):
        scene.select_masks([np.eye(4)], [np.zeros((48, 64), np.int32)], (64, 48))
    scene.set_panorama(None)
    scene.set_point_drop(0.5, 1)
    with pytest.raises(NotImplementedError, match="augmentation"):
        scene.select_masks([np.eye(4)], [np.zeros((48, 64), np.int32)], (64, 48))


# ---- the inputs of the GPU vote test are not trivial -----------------------------------------------------------------------------------------
def test_vote_case_exercises_every_class():
    case = sc.vote_case()
    xyz, W, H = case['xyz'], case['W'], case['H']
    n = len(xyz)
    assert n == 100_003 and (W, H) == (64, 48) and len(case['totals']) == 4
    scale, slack = sm.scale_of(case['rel']), f32(case['slack'])
    state = np.zeros(n, np.uint32)
    best = dict.fromkeys(('out of view', 'occluded', 'seen without a hit', 'hit', 'conflict'), 0.0)
    for v, (M, mask) in enumerate(zip(case['totals'], case['masks'])):
        idx, dep = oracle.raster_multiscale(xyz, M.reshape(4, 4), W, H, 1)
        near = sm.near_image(xyz, M, idx[0], dep[0])
        pix, vis = sm.classify(xyz, M, W, H, near, scale, slack)
        m = mask.reshape(-1)[np.maximum(pix, 0)]
        cand = (state >> 16).astype(np.int64)
        hit = vis & (m != 0) & ((cand == 0) | (cand == m))
        conflict = vis & (m != 0) & (cand != 0) & (cand != m)
        share = {'out of view': (pix < 0).mean(), 'occluded': ((pix >= 0) & ~vis).mean(), 'seen without a hit': (vis & ~hit).mean(),
                 'hit': hit.mean(), 'conflict': conflict.mean()}
        print(f"view {v}: " + ", ".join(f"{k} {100 * s:.1f} %" for k, s in share.items()) + f", seen {100 * vis.mean():.1f} %")
        best = {k: max(best[k], share[k]) for k in best}
        state = sm.vote(state, xyz, M, W, H, near, mask, scale, slack)
    assert all(s >= 0.005 for s in best.values()), best
    labels = sm.finish(state, case['min_hits'], case['ratio'])
    count = np.bincount(labels, minlength=4)
    rejected = int(((state >> 16 != 0) & (labels == 0)).sum())
    print(f"final: {count[1]} of label 1, {count[2]} of label 2, {count[3]} of label 3, {rejected} rejected")
    assert count[1] >= 500 and count[2] >= 500 and count[3] == 0 and rejected >= 500


def test_box_cases_label_a_fair_share():
    xyz = synthetic.make_cloud(100_003)
    for K in sc.BOX_K[1:]:
        boxes, label_of = sc.random_boxes(K, 31)
        share = (sm.label_boxes(xyz, boxes, label_of, np.full(len(xyz), -1)) >= 0).mean()
        print(f"K = {K}: {100 * share:.1f} % of the points lie in a box")
        assert 0.01 <= share <= 0.30, (K, share)
