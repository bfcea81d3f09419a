"""CPU: the annotation contract (tests/annotate_model.py) against two independent restatements — the per-instance key images of
tests/instances_model.py for the instance image, a brute-force loop over pixels and points for the statistics —, the conventions for
empty rows, and the argument refusals that need no device."""
import ctypes as C

import numpy as np
import pytest

import oracle
from read_amd import _lib, annotate
from read_amd.raster import object_matrix
from tests import annotate_cases as ac
from tests import annotate_model as am

SIZES = [(80, 48), (64, 32)]


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("case", ["edited", "unlabelled", "seventy", "no_instances"])
def test_instance_image_is_the_first_instance_holding_the_merged_key(case, W, H):
    c = getattr(ac, case)(W, H)
    ref = am.first_instance_by_key_image(c['xyz'], c['labels'], c['foreign'], c['inst'], c['M0'], W, H)
    assert np.array_equal(c['won'], ref)
    assert c['unmatched'] == 0
    if case == "edited":
        twin = am.key_matches(c['xyz'], c['labels'], c['foreign'], c['inst'], c['M0'], W, H, 3)
        assert ((c['won'] == 2) & twin).sum() >= 10 and not (c['won'] == 3).any()       # exact ties go to the lower list entry


@pytest.mark.parametrize("W,H", SIZES)
def test_statistics_against_a_brute_force_loop(W, H):
    c = ac.edited(W, H)
    _, pool, _, lst = am.instance_ranges(c['xyz'], c['labels'], c['foreign'], c['inst'])
    for i, (first, npts, P, visible) in enumerate(lst):
        row = [0, 2 ** 31 - 1, 2 ** 31 - 1, -1, -1, 0, 2 ** 31 - 1, 2 ** 31 - 1, -1, -1, 2 ** 31 - 1, npts]
        for y in range(H):
            for x in range(W):
                if c['won'][y, x] == i:
                    row[0] += 1
                    row[1], row[2], row[3], row[4] = min(row[1], x), min(row[2], y), max(row[3], x), max(row[4], y)
        if visible:
            pix, d = oracle.project_points(pool[0][first:first + npts], object_matrix(c['M0'], P), W, H)
            for q, dd in zip(pix.tolist(), d.view(np.uint32).tolist()):
                if q >= 0:
                    x, y = q % W, q // W
                    row[5] += 1
                    row[6], row[7], row[8], row[9] = min(row[6], x), min(row[7], y), max(row[8], x), max(row[9], y)
                    row[10] = min(row[10], dd)
        assert c['stats'][i].tolist() == row, i
    assert c['stats'].dtype == np.int32


def test_conventions_for_empty_rows_and_a_mismatched_list():
    W, H = 80, 48
    c = ac.edited(W, H)
    assert am.empty_row(7).tolist() == [0, 2 ** 31 - 1, 2 ** 31 - 1, -1, -1, 0, 2 ** 31 - 1, 2 ** 31 - 1, -1, -1, 2 ** 31 - 1, 7]
    assert np.array_equal(c['stats'][4], am.empty_row(500)), "a hidden instance keeps n_pts and is otherwise empty"
    assert c['stats'][3, am.VIS_PX] == 0 and c['stats'][3, am.VX0] == 2 ** 31 - 1 and c['stats'][3, am.VX1] == -1
    assert c['stats'][3, am.IN_PTS] == 600                           # the twin wins nothing but its extents are its own
    assert (c['inst_img'][c['obj'] <= 0] == -1).all() and (c['inst_img'][c['obj'] >= 1] >= 10).all()
    # the frame annotated with another pose for one instance: its pixels match no instance
    moved = list(c['inst'])
    moved[5] = (3, ac.translation((-1.0, -1.25, -12.0)), True)
    _, inst_img, stats, unmatched, _ = am.annotate(c['xyz'], c['labels'], c['foreign'], moved, c['M0'], W, H, c['idx'], c['depth'])
    assert unmatched == c['stats'][5, am.VIS_PX] > 0 and stats[5, am.VIS_PX] == 0
    # an id that no range holds
    idx = c['idx'].copy()
    filled = np.flatnonzero(~((idx.reshape(-1) == 0) & (c['depth'].reshape(-1).view(np.uint32) == 0)))
    idx.reshape(-1)[filled[:3]] = c['xyz'].shape[0] + 400 + 5
    obj, _, _, unmatched, _ = am.annotate(c['xyz'], c['labels'], c['foreign'], c['inst'], c['M0'], W, H, idx, c['depth'])
    assert unmatched >= 3 and (obj.reshape(-1)[filled[:3]] == -1).all()


def test_object_lists():
    begin, order = annotate.object_lists([1, 2, 1, 1, 2, 3, 2], 3)
    assert begin.tolist() == [0, 3, 6, 7] and order.tolist() == [0, 2, 3, 1, 4, 6, 5]
    begin, order = annotate.object_lists([], 2)
    assert begin.tolist() == [0, 0, 0] and order.size == 0
    begin, order = annotate.object_lists([3], 4)                     # objects without instances are empty lists
    assert begin.tolist() == [0, 0, 0, 1, 1]
    with pytest.raises(ValueError, match="objects 1..3"):
        annotate.object_lists([1, 4], 3)
    with pytest.raises(ValueError, match="objects 1..3"):
        annotate.object_lists([0], 3)


def _args(**kw):
    """A call with I = 2, K = 2 (one own, one foreign object) whose pointers are small non-null numbers: nothing is dereferenced on the
    device side before the checks are through, and every check fails before device work."""
    keep = dict(first=np.array([0, 10], np.int64), npts=np.array([10, 5], np.int64), obj=np.array([1, 2], np.int32),
                M=np.zeros((2, 16), np.float32), vis=np.ones(2, np.uint8),
                foreign=(_lib.AnnotateForeign * 1)(_lib.AnnotateForeign(100, 5, 10)))
    a = _lib.AnnotateArgs()
    d = 0x1000
    a.xyz, a.n, a.labels, a.K_own, a.n_foreign, a.foreign = d, 100, d, 1, 1, keep['foreign']
    a.pool_xyz, a.pool_n, a.count = d, 15, 2
    a.first, a.npts, a.obj, a.M, a.visible = (keep[k].ctypes.data for k in ('first', 'npts', 'obj', 'M', 'vis'))
    a.d_M = a.d_visible = a.d_value = a.d_npts = a.d_obj_begin = a.d_obj_list = d
    a.idx0 = a.depth0 = a.out_obj = a.out_inst = a.stats = a.unmatched = d
    a.W, a.H = 80, 48
    for k, v in kw.items():
        if k in keep and v is not None:
            keep[k][...] = v
        else:
            setattr(a, k, v)
    return a, keep


@pytest.mark.parametrize("change,word", [
    (dict(idx0=None), b"null"), (dict(unmatched=None), b"null"), (dict(xyz=None), b"xyz"), (dict(d_obj_list=None), b"device table"),
    (dict(M=None), b"host table"), (dict(stats=None), b"stats"), (dict(pool_xyz=None), b"pool_xyz"),
    (dict(W=1 << 16, H=1 << 15), b"W * H"), (dict(W=0), b"W/H"),
    (dict(n=-1), b"n = -1"), (dict(count=-1), b"count"), (dict(K_own=-1), b"K_own"), (dict(pool_n=-1), b"pool_n"),
    (dict(n_foreign=8), b"n_foreign"),
    (dict(obj=[1, 3]), b"object 3 outside [1, 2]"), (dict(obj=[0, 1]), b"object 0 outside"),
    (dict(n=101), b"ascend from n"),                                  # the foreign base 100 lies inside the cloud's ids
    (dict(npts=[10, 6]), b"past the pool"), (dict(first=[-1, 10]), b"first = -1"),
])
def test_bad_arguments_are_refused_before_any_device_work(change, word):
    a, keep = _args(**change)
    L = _lib.lib()
    assert L.read_annotate_frame(C.byref(a), None) == -22
    msg = L.read_last_error()
    assert b"read_annotate_frame" in msg and word in msg, msg
    assert L.read_annotate_frame(None, None) == -22


def test_python_refusals_without_a_device():
    from read_amd.render import Scene, StitchedScene
    s = Scene(np.zeros((4, 3), np.float32))
    s.set_panorama(200.0)
    with pytest.raises(NotImplementedError, match="panorama"):
        s.annotate_frame((64, 32))
    s.set_panorama(None)
    s.set_point_drop(0.5, 1)
    with pytest.raises(NotImplementedError, match="GL-twin"):
        s.annotate_frame((64, 32))
    with pytest.raises(ValueError, match="no point cloud"):
        Scene().annotate_frame((64, 32))
    with pytest.raises(NotImplementedError, match="StitchedScene"):
        StitchedScene.annotate_frame(object.__new__(StitchedScene), (64, 32))
    a = annotate.Annotation(None, None, None, None, [], None)
    assert a.handles == [] and annotate.STAT_NAMES[am.NEAR_BITS] == "near_bits" and len(annotate.STAT_NAMES) == am.STATS
