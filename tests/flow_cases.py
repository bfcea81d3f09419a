"""The state pairs of the frame-flow tests (tests/test_flow_cpu.py, tests/test_gpu_flow.py).  Each generator asserts on the MODEL's
output (tests/flow_model.py) that the pair holds what it is for, so a test cannot pass vacuously.

A case is a dict: xyz, labels, foreign, W, H; inst_a / inst_b = [(k, P, visible)] by A's list positions; M0_a / M0_b; the model's
frames idx_a, depth_a, idx_b, depth_b; and ``out``, the model's flow (flow, depth_next, state, counts, stats, unmatched, won)."""
import functools

import numpy as np

from read_amd import camera, synthetic
from tests import annotate_cases as ac
from tests import annotate_model as am
from tests import flow_model as fm

SIZES = [(80, 48), (64, 32), (75, 37)]         # 75 x 37 = 2775 pixels: no multiple of a wave, the last wave has tail lanes
CAMERA_STEP = (1.5, 0.3, -2.0)
MIN_PIXELS = 20
MIN_TIES = 10


def camera_b(W, H, step=CAMERA_STEP):
    """A's camera (annotate_cases._camera) moved by ``step`` in the world."""
    pose = synthetic.sweep_pose(0).astype(np.float64)
    T = np.eye(4)
    T[:3, 3] = step
    return camera.total_matrix(synthetic.make_proj(W, H, f=float(W)), (T @ pose).astype(np.float32))[0]


def _compose(P, t):
    """The pose P (None = identity) followed by the translation t."""
    T = ac.translation(t)
    return T if P is None else (T @ np.asarray(P, np.float32)).astype(np.float32)


def _finish(base, inst_b, M0_b):
    case = dict(xyz=base['xyz'], labels=base['labels'], foreign=base['foreign'], W=base['W'], H=base['H'], inst_a=list(base['inst']),
                inst_b=list(inst_b), M0_a=base['M0'], M0_b=np.asarray(M0_b, np.float32), idx_a=base['idx'], depth_a=base['depth'])
    W, H = case['W'], case['H']
    case['idx_b'], case['depth_b'] = fm.render(case['xyz'], case['labels'], case['foreign'], case['inst_b'], case['M0_b'], W, H)
    case['out'] = fm.flow(case['xyz'], case['labels'], case['foreign'], case['inst_a'], case['inst_b'], case['M0_a'], case['M0_b'], W, H,
                          case['idx_a'], case['depth_a'], case['idx_b'], case['depth_b'])
    out = case['out']
    assert out['unmatched'] == 0 and out['counts'].sum() == W * H and out['counts'][7] == 0
    return case


def moved_list(inst):
    """State B of ``moved``: instance 0 behind the wall, 1 behind the camera, 2 re-posed (the twins part), 5 hidden."""
    b = list(inst)
    b[0] = (b[0][0], _compose(b[0][1], (0.0, 0.0, -14.0)), b[0][2])
    b[1] = (b[1][0], _compose(b[1][1], (-5.0, 2.0, 30.0)), b[1][2])
    b[2] = (b[2][0], ac.translation((6.0, 2.0, 3.0)), b[2][2])
    b[5] = (b[5][0], b[5][1], False)
    return b


@functools.lru_cache(maxsize=None)
def moved(W, H, n_static=4500):
    """A = annotate_cases.edited; B: the camera stepped by CAMERA_STEP, instance 0 pushed behind the wall, instance 1 sent behind the
    camera, instance 2 re-posed, instance 5 hidden: every state of the contract in one pair."""
    base = ac.edited(W, H, n_static)
    case = _finish(base, moved_list(base['inst']), camera_b(W, H))
    out, st, won = case['out'], case['out']['state'], case['out']['won']
    for s in (fm.EMPTY, fm.VISIBLE, fm.OCCLUDED, fm.OFF_IMAGE, fm.CLIPPED, fm.HIDDEN):
        assert out['counts'][s] >= MIN_PIXELS, f"state {s}: {out['counts'][s]} pixels"
    twin = am.key_matches(case['xyz'], case['labels'], case['foreign'], case['inst_a'], case['M0_a'], W, H, 3)
    ties = int(((won == 2) & twin & (st == fm.VISIBLE)).sum())
    assert ties >= MIN_TIES, f"{ties} tie pixels of the twins are visible"
    assert out['stats'][5, fm.PX] > 0 and (st[won == 5] == fm.HIDDEN).all(), "the foreign instance of A is the one hidden in B"
    row0 = out['stats'][0]                                   # the wall is a sparse cloud: a few points show through its gaps
    assert row0[fm.N_OCCLUDED] >= MIN_PIXELS and row0[fm.N_OCCLUDED] > 4 * row0[fm.N_VISIBLE], "instance 0 went behind the wall"
    assert (st[won == 1] == fm.CLIPPED).all() and out['stats'][1, fm.N_OUTSIDE] == out['stats'][1, fm.PX] > 0, "instance 1 is behind the camera"
    static = (won < 0) & (st != fm.EMPTY)
    assert (np.abs(out['flow'][static & (st == fm.VISIBLE)]).max(axis=-1) > 0).all(), "the camera moved: static pixels flow"
    return case


@functools.lru_cache(maxsize=None)
def wide(W=600, H=300, turn=512 * 256):
    """``moved``'s pair at a frame of more pixels than one turn of the pixel pass covers (csrc/flow.hip: at most 512 workgroups of
    256 lanes, which then loop): static and object pixels lie past the first turn, and the last turn is partly filled."""
    base = ac.edited(W, H, 60000)
    case = _finish(base, moved_list(base['inst']), camera_b(W, H))
    out = case['out']
    assert turn < W * H < 2 * turn and (W * H) % 256 != 0
    late = np.arange(W * H).reshape(H, W) >= turn
    assert ((out['won'] >= 0) & late).sum() >= MIN_PIXELS and ((out['won'] < 0) & late & (out['state'] == fm.VISIBLE)).sum() >= MIN_PIXELS
    for s in (fm.EMPTY, fm.VISIBLE, fm.OCCLUDED, fm.OFF_IMAGE, fm.CLIPPED, fm.HIDDEN):
        assert out['counts'][s] >= MIN_PIXELS, f"state {s}: {out['counts'][s]} pixels"
    return case


@functools.lru_cache(maxsize=None)
def foreign_moves(W, H):
    """``moved`` with the foreign instance (5) kept visible and shifted: pixels of a foreign object flow (in ``moved`` itself the only
    foreign instance is the hidden one, whose flow is 0 by contract)."""
    base = ac.edited(W, H)
    b = moved_list(base['inst'])
    b[5] = (b[5][0], _compose(base['inst'][5][1], (0.5, 0.25, 0.0)), True)
    case = _finish(base, b, camera_b(W, H))
    st, won = case['out']['state'], case['out']['won']
    sel = (won == 5) & (case['idx_a'] >= case['xyz'].shape[0])
    flowing = sel & ((st == fm.VISIBLE) | (st == fm.OCCLUDED))
    assert flowing.sum() >= MIN_PIXELS and (np.abs(case['out']['flow'][flowing]).sum(axis=-1) > 0).all(), "a foreign instance flows"
    return case


@functools.lru_cache(maxsize=None)
def identity(W, H):
    """B = A: every filled pixel is VISIBLE (the twins' ties included), flow and depth_next - depth are exactly 0."""
    base = ac.edited(W, H)
    case = _finish(base, list(base['inst']), base['M0'])
    case['idx_b'], case['depth_b'] = case['idx_a'], case['depth_a']
    out = case['out']
    filled = ~((case['idx_a'] == 0) & (case['depth_a'].view(np.uint32) == 0))
    assert (out['state'][filled] == fm.VISIBLE).all() and (out['state'][~filled] == fm.EMPTY).all()
    assert not out['flow'].view(np.uint32).any(), "flow bits are +0 everywhere"
    assert np.array_equal(out['depth_next'].view(np.uint32)[filled], case['depth_a'].view(np.uint32)[filled])
    twin = am.key_matches(case['xyz'], case['labels'], case['foreign'], case['inst_a'], case['M0_a'], W, H, 3)
    assert ((out['won'] == 2) & twin & (out['state'] == fm.VISIBLE)).sum() >= MIN_TIES, "a genuine tie of two copies counts as visible"
    return case


@functools.lru_cache(maxsize=None)
def one_moved_instance(W, H):
    """The camera stands still and instance 6 alone moves: static pixels have zero flow."""
    base = ac.edited(W, H)
    b = list(base['inst'])
    b[6] = (b[6][0], _compose(b[6][1], (2.0, 0.5, 0.0)), True)
    case = _finish(base, b, base['M0'])
    out, won = case['out'], case['out']['won']
    static = (won < 0) & (out['state'] != fm.EMPTY)
    assert static.sum() >= MIN_PIXELS and not out['flow'][static].view(np.uint32).any(), "static pixels do not move"
    assert set(np.unique(out['state'][static])) <= {fm.VISIBLE, fm.OCCLUDED}
    moving = (won == 6) & (out['state'] == fm.VISIBLE)
    assert moving.sum() > 0 and (out['flow'][moving][:, 0] > 0).all(), "instance 6 moves to the right"
    others = (won >= 0) & (won != 6)
    assert not out['flow'][others].view(np.uint32).any()
    return case


@functools.lru_cache(maxsize=None)
def no_instances(W, H):
    """I = 0: a cloud without labels, objects or instances under the moved camera — static pixels still flow."""
    base = ac.no_instances(W, H)
    case = _finish(base, [], camera_b(W, H))
    out = case['out']
    assert out['stats'].shape == (0, 4) and out['counts'][fm.VISIBLE] >= MIN_PIXELS and out['counts'][fm.HIDDEN] == 0
    return case


def mismatched(case):
    """The case with A's instance 5 listed at another pose than its frame was drawn with: -> (inst_a, inst_b) of the wrong list."""
    a = list(case['inst_a'])
    a[5] = (3, ac.translation((-1.0, -1.25, -12.0)), True)
    return a, list(case['inst_b'])
