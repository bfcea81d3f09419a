"""CPU: scene stitching — the C ABI (read_stitch_gather_forward: exported, bound, its struct laid out as the header says, bad
arguments refused before any device work), the NumPy model of the merge contract against the oracle on the concatenated cloud,
and the host bookkeeping of StitchedScene.  The kernel and the frames are checked on the GPU (tests/test_gpu_stitch.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from read_amd import _lib
from read_amd.render import MultiscaleRender, Scene, StitchedScene
from tests import stitch_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 1 << 20          # a 256-byte aligned non-null address: the calls below fail on their arguments and never touch it
EINVAL = -22


def test_symbol_is_exported_and_bound():
    L = C.CDLL(_lib.LIB_PATH)
    assert hasattr(L, "read_stitch_gather_forward") and "read_stitch_gather_forward" in _lib.SIGNATURES
    assert _lib.lib().read_abi_version() == 3
    assert _lib.READ_STITCH_MAX_PARTS == 8


def test_struct_layout_matches_the_header(tmp_path):
    fields = [f for f, _ in _lib.StitchPart._fields_]
    assert fields == ["idx_levels", "depth_levels", "rows_nc", "n", "id_base", "activation"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "read_hip.h"\n'
                   'int main(void) { printf("%d %zu", READ_STITCH_MAX_PARTS, sizeof(read_stitch_part));\n'
                   + "".join(f'printf(" %zu", offsetof(read_stitch_part, {f}));\n' for f in fields) + 'return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call([os.environ.get("CC", "cc"), "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [_lib.READ_STITCH_MAX_PARTS, C.sizeof(_lib.StitchPart)] + [getattr(_lib.StitchPart, f).offset for f in fields]


class _Call:
    """A valid read_stitch_gather_forward call over fake addresses whose pieces can be broken one at a time."""

    def __init__(self, count=2, levels=5):
        self.count, self.levels, self.C = count, levels, 8
        self.keep = [_lib.ptr_array([FAKE] * max(levels, 1)) for _ in range(2 * max(count, 1))]
        self.parts = (_lib.StitchPart * max(count, 1))()
        for s in range(max(count, 1)):
            self.parts[s].idx_levels, self.parts[s].depth_levels = self.keep[2 * s], self.keep[2 * s + 1]
            self.parts[s].rows_nc, self.parts[s].n, self.parts[s].id_base, self.parts[s].activation = FAKE, 1000, 1000 * s, 0
        self.counts = (C.c_int64 * max(levels, 1))(*[64 * 48 >> (2 * l) for l in range(max(levels, 1))])
        self.outs = [_lib.ptr_array([FAKE] * max(levels, 1)) for _ in range(4)]
        self.null_parts = False

    def run(self):
        L = _lib.lib()
        rc = L.read_stitch_gather_forward(None if self.null_parts else self.parts, self.count, self.C, self.levels, self.counts,
                                          *self.outs, None)
        return rc, L.read_last_error().decode()


def _broken(case):
    c = _Call(count={"count0": 0, "count9": 9}.get(case, 2), levels={"levels0": 0, "levels6": 6}.get(case, 5))
    if case == "C":
        c.C = 6
    elif case == "null_parts":
        c.null_parts = True
    elif case == "null_counts":
        c.counts = None
    elif case == "rows":
        c.parts[1].rows_nc = None
    elif case == "id_base_negative":
        c.parts[1].id_base = -1
    elif case == "id_base_overflow":
        c.parts[1].id_base, c.parts[1].n = (1 << 31) - 1000, 1000        # id_base + n = INT32_MAX + 1
    elif case == "no_outputs":
        c.outs = [None] * 4
    elif case == "half_hidden":
        c.parts[0].depth_levels = None
    return c


@pytest.mark.parametrize("case,text", [
    ("count0", "count must be 1..8"), ("count9", "count must be 1..8"), ("C", "multiple of 4"), ("levels0", "levels must be 1..5"),
    ("levels6", "levels must be 1..5"), ("null_parts", "null part table"), ("null_counts", "null part table"),
    ("rows", "part 1: rows_nc is null while features are requested"), ("id_base_negative", "part 1: id_base -1"),
    ("id_base_overflow", "leaves the int32 id range"), ("no_outputs", "no outputs"), ("half_hidden", "part 0: index and depth")])
def test_bad_arguments_are_refused_before_any_device_work(case, text):
    rc, msg = _broken(case).run()                     # no GPU here: anything past the checks would fail differently
    assert rc == EINVAL and "read_stitch_gather_forward" in msg and text in msg, (case, rc, msg)


def test_limits_that_are_still_valid_pass_the_checks():
    # zero pixels on every level: READ_OK without a launch, so only the checks run (the addresses are never touched)
    c = _Call()
    c.counts = (C.c_int64 * 5)(0, 0, 0, 0, 0)
    assert c.run()[0] == 0
    c.parts[1].id_base, c.parts[1].n, c.parts[1].rows_nc = (1 << 31) - 1001, 1000, None      # id_base + n == INT32_MAX exactly,
    c.outs[3] = None                                                                          # rows NULL without features,
    c.parts[0].idx_levels = c.parts[0].depth_levels = None                                    # part 0 hidden
    rc, msg = c.run()
    assert rc == 0, msg


# ---- the contract, in NumPy, against the oracle ---------------------------------------------------------------------------------
def test_model_equals_the_oracle_on_the_concatenated_cloud():
    clouds, M = sm.union_scene()
    assert tuple(c.shape[0] for c in clouds) == sm.COUNTS
    (whole_i, whole_d), parts = sm.union_oracle()
    base = sm.id_bases(sm.COUNTS)
    got_i, got_d, got_p, _ = sm.merge([(pi, pd, base[s]) for s, (pi, pd) in enumerate(parts)])
    stats = sm.tie_and_empty_counts(parts)
    for l in range(sm.LEVELS):
        assert np.array_equal(got_i[l], whole_i[l]), f"index level {l}: {int((got_i[l] != whole_i[l]).sum())} pixels differ"
        assert np.array_equal(got_d[l].view(np.uint32), whole_d[l].view(np.uint32)), f"depth level {l}"
        ties, empty = stats[l]
        assert ties >= 1 and empty >= 1, f"level {l}: {ties} exact cross-part ties, {empty} empty pixels"
        assert int((got_p[l] == 255).sum()) == empty
    later = (got_p[0] >= 1) & (got_p[0] != 255)                                  # later parts really win, and sky really exists
    assert int(later.sum()) >= 100 and int((got_p[0] == 255).sum()) >= 0.2 * got_p[0].size


def test_model_hiding_keeps_ids_and_features_follow_the_winner():
    _, parts = sm.union_oracle()
    base = sm.id_bases(sm.COUNTS)
    tab = [(pi, pd, base[s]) for s, (pi, pd) in enumerate(parts)]
    full = sm.merge(tab)
    hid = sm.merge(tab, visible=[True, False, True])
    keep = full[2][0] == 2                                                       # pixels part 2 owned stay part 2's, same ids
    assert keep.any() and np.array_equal(hid[0][0][keep], full[0][0][keep]) and (hid[2][0][keep] == 2).all()
    assert not (hid[2][0] == 1).any() and (hid[0][0][hid[2][0] == 2] >= base[2]).all()
    rows = [np.random.default_rng(s).random((n, 4), dtype=np.float32) for s, n in enumerate(sm.COUNTS)]
    feat = sm.features(rows, hid[2], hid[3])
    allrows = np.concatenate(rows)
    assert np.array_equal(feat[0], allrows[hid[0][0]])                         # = gathering the concatenated table by merged id


# ---- StitchedScene on the host ------------------------------------------------------------------------------------------------
def _scenes():
    return [Scene(np.random.default_rng(s).standard_normal((n, 3)).astype(np.float32)) for s, n in enumerate((100, 60, 40))]


def test_stitched_scene_bookkeeping():
    scenes = _scenes()
    P = np.eye(4, dtype=np.float32)
    P[:3, 3] = (1.0, 2.0, 3.0)
    st = StitchedScene(scenes, poses=[None, P, None])
    assert st.counts() == [100, 60, 40] and st.id_base() == [0, 100, 160]
    st.set_part_visible(0, False)
    st.set_part_visible(1, False)
    assert st.id_base() == [0, 100, 160] and not st.part_visible(1) and st.part_visible(2)       # stable under hiding
    st.set_part_visible(1, True)
    assert st.part_visible(1) and np.array_equal(st.part_poses[1], P) and st.part_poses[0] is None
    st.set_part_pose(1, None)
    assert st.part_poses[1] is None
    view, proj, model = (np.random.default_rng(k).standard_normal((4, 4)).astype(np.float32) for k in (1, 2, 3))
    st.set_camera_view(view), st.set_proj_matrix(proj), st.set_model_view(model), st.announce_next_camera_view(view)
    for sc in scenes:
        assert np.array_equal(sc.view_matrix, view) and np.array_equal(sc.proj_matrix, proj)
        assert np.array_equal(sc.model_matrix, model) and np.array_equal(sc.next_view_matrix, view)
    assert np.array_equal(st.total_matrix(), scenes[0].total_matrix())
    assert st.take_next_total_matrix() is not None and all(sc.next_view_matrix is None for sc in scenes)
    assert not st.augmented() and not st.edited()
    scenes[2].set_point_discard(np.zeros(40, bool))
    assert st.augmented()
    scenes[1].set_object_labels(np.arange(60) % 2)
    assert st.edited()
    for bad in (-1, 3):
        with pytest.raises(ValueError, match="no part"):
            st.set_part_pose(bad, None)
    with pytest.raises(ValueError, match="1..8 parts"):
        StitchedScene([Scene(np.zeros((1, 3), np.float32)) for _ in range(9)])
    with pytest.raises(ValueError, match="poses"):
        StitchedScene(_scenes(), poses=[None])


def test_stitched_scene_refuses_what_stitching_does_not_serve():
    st = StitchedScene(_scenes())
    fmt = "uv_1d_p1, uv_1d_p1_ds1, uv_1d_p1_ds2, uv_1d_p1_ds3"
    for bad in ("xyz_p1_ds1", "colors_p1_ds1", "uv_1d_p2_ds1", "depth_p1_ds1"):
        with pytest.raises(NotImplementedError, match="stitching"):
            MultiscaleRender(st, f"uv_1d_p1, {bad}", (64, 64), out_buffer_location='torch').render()
    with pytest.raises(NotImplementedError, match="supersampling 2 with scene stitching"):
        MultiscaleRender(st, fmt, (64, 64), out_buffer_location='torch', supersampling=2).render()
    with pytest.raises(NotImplementedError, match="multiples of 8"):
        MultiscaleRender(st, fmt, (68, 64), out_buffer_location='torch').render()
    st.scenes[1].set_point_discard(np.zeros(60, bool))
    with pytest.raises(NotImplementedError, match="augmentation"):
        MultiscaleRender(st, fmt, (64, 64), out_buffer_location='torch').render()


def test_python_layer_refuses_before_the_device():
    from read_amd.stitch import id_bases
    from read_amd.texture import stitch_gather_pyramid
    assert id_bases([5, 7, 9]) == [0, 5, 12]
    with pytest.raises(ValueError, match="1..8 parts"):
        id_bases([1] * 9)
    with pytest.raises(ValueError, match="int32"):
        id_bases([1 << 30, 1 << 30])
    with pytest.raises(NotImplementedError, match="supersampling"):
        stitch_gather_pyramid([(None, None, None, 0, 'none')], ss=2)
    with pytest.raises(ValueError, match="1..8 parts"):
        stitch_gather_pyramid([(None, None, None, 0, 'none')] * 9)
    with pytest.raises(ValueError, match="hidden"):
        stitch_gather_pyramid([(10, None, None, 0, 'none')])

