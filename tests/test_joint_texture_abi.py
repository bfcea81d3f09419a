"""CPU, library built, no GPU: the C ABI of training through the table gather — read_gather_backward_tables and
read_rmsprop_sorted_tables are exported and bound and refuse bad arguments with READ_EINVAL and a message before any device work —
and the host-side refusals of JointTexture, StitchedScene.joint_texture, NetAndTexture and DataParallelStep.  The kernels are held to
their references on the GPU (tests/test_gpu_joint_texture.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from read_amd import _lib

FAKE = 1 << 20          # a 256-byte aligned non-null address: the calls below fail on their arguments and never touch it
NEW = ("read_gather_backward_tables", "read_rmsprop_sorted_tables")


def test_symbols_are_exported_and_bound():
    L = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
    assert _lib.lib().read_abi_version() == 3


def test_struct_layouts():
    # float *, float *, int32_t *, int64_t, int64_t, int, int
    assert C.sizeof(_lib.RmspropTable) == 48
    assert [getattr(_lib.RmspropTable, f).offset for f in ("rows", "sq", "stamp", "n", "id_base", "step", "trainable")] == \
        [0, 8, 16, 24, 32, 40, 44]


def _tables(spec):
    t = (_lib.GatherTable * len(spec))()
    for k, (n, base, act) in enumerate(spec):
        t[k].rows_nc, t[k].n, t[k].id_base, t[k].activation = None, n, base, act
    return t


GOOD = ((5, 0, 0), (1, 5, 1), (7, 6, 2))


def _backward(spec=GOOD, count=None, Cc=8, levels=2, idx=FAKE, dfeat=FAKE, feat=FAKE, g=FAKE, drows=(FAKE, None, FAKE), counts=(96, 24),
              tables=True):
    L = _lib.lib()
    arr = lambda p, n: None if p is None else _lib.ptr_array([p] * n)              # noqa: E731
    rc = L.read_gather_backward_tables(_tables(spec) if tables else None, len(spec) if count is None else count, Cc, levels,
                                       arr(idx, levels), (C.c_int64 * len(counts))(*counts), arr(dfeat, levels), arr(feat, levels),
                                       arr(g, levels), None if drows is None else _lib.ptr_array(list(drows)), None)
    return rc, L.read_last_error().decode()


@pytest.mark.parametrize("kwargs,word", [
    (dict(count=0), "count"), (dict(spec=GOOD * 3, count=9), "count"), (dict(Cc=6), "multiple of 4"), (dict(levels=6), "levels"),
    (dict(tables=False), "null"), (dict(idx=None), "null"), (dict(dfeat=None), "null"),
    (dict(spec=((5, 0, 0), (0, 5, 0))), "empty"), (dict(spec=((5, 0, 3),)), "activation"), (dict(spec=((5, 1, 0),)), "id_base must be 0"),
    (dict(spec=((5, 0, 0), (1, 0, 0))), "ascend"), (dict(spec=((5, 0, 0), (1, 4, 0))), "overlaps"),
    (dict(spec=((5, 0, 0), (2, (1 << 31) - 2, 0))), "int32"),
    (dict(feat=None), "feat_levels is null"),                                            # an activation is set and y is missing
    (dict(g=None, drows=None), "no outputs"), (dict(g=None, drows=(None, None, None)), "no outputs"),
    (dict(dfeat=FAKE + 4), "dfeat level 0 misaligned"), (dict(feat=FAKE + 8), "feat level 0 misaligned"), (dict(g=FAKE + 4), "g level 0 misaligned"),
    (dict(drows=(FAKE, None, FAKE + 4)), "table 2: gradient rows misaligned"), (dict(counts=(96, -1)), "negative"),
])
def test_gather_backward_tables_refuses_bad_arguments(kwargs, word):
    rc, msg = _backward(**kwargs)
    assert rc == -22 and "read_gather_backward_tables" in msg and word in msg, (kwargs, msg)


def test_gather_backward_tables_accepts_what_it_documents():
    # no pixels: every check passes and nothing is launched (there is no GPU here)
    for kwargs in (dict(), dict(g=None), dict(drows=None), dict(spec=((5, 0, 0), (3, 9, 0)), feat=None, drows=(FAKE, FAKE))):
        rc, msg = _backward(counts=(0, 0), **kwargs)
        assert rc == 0, (kwargs, msg)


def _rms(spec=((600, 0, 1, 1), (1, 600, 1, 1), (40, 601, 1, 1)), count=None, Cc=8, ids=FAKE, perm=FAKE, g=FAKE, n=0, scratch=FAKE, ptr=FAKE,
         tables=True):
    L = _lib.lib()
    t = (_lib.RmspropTable * len(spec))()
    for k, (rows_n, base, step, trainable) in enumerate(spec):
        t[k].rows, t[k].sq, t[k].stamp = (ptr, ptr, ptr) if trainable != 2 else (None, None, None)
        t[k].n, t[k].id_base, t[k].step, t[k].trainable = rows_n, base, step, int(bool(trainable))
    rc = L.read_rmsprop_sorted_tables(t if tables else None, len(spec) if count is None else count, Cc, ids, perm, g, n, 0.1, 0.99, 1e-8,
                                      scratch, None)
    return rc, L.read_last_error().decode()


@pytest.mark.parametrize("kwargs,word", [
    (dict(count=0), "count"), (dict(spec=((1, 0, 1, 1),) * 9), "count"), (dict(tables=False), "null"), (dict(ids=None), "null"),
    (dict(perm=None), "null"), (dict(g=None), "null"), (dict(scratch=None), "null"), (dict(Cc=0), "bad sizes"), (dict(Cc=17), "bad sizes"),
    (dict(n=-1), "bad sizes"), (dict(spec=((0, 0, 1, 1),)), "empty"), (dict(spec=((5, 2, 1, 1),)), "id_base must be 0"),
    (dict(spec=((5, 0, 1, 1), (5, 0, 1, 1))), "ascend"), (dict(spec=((5, 0, 1, 1), (5, 3, 1, 1))), "overlaps"),
    (dict(spec=((5, 0, 1, 1), (2, (1 << 31) - 2, 1, 1))), "int32"), (dict(spec=((5, 0, 0, 1),)), "step"),
    (dict(spec=((5, 0, 1, 2),)), "null rows"),
])
def test_rmsprop_sorted_tables_refuses_bad_arguments(kwargs, word):
    rc, msg = _rms(**kwargs)
    assert rc == -22 and "read_rmsprop_sorted_tables" in msg and word in msg, (kwargs, msg)


def test_rmsprop_sorted_tables_accepts_what_it_documents():
    # n = 0 returns after the checks; a frozen table needs neither pointers nor a step, and gaps between the ranges are allowed
    for spec in (((600, 0, 1, 1), (1, 600, 1, 1), (40, 601, 1, 1)), ((5, 0, 3, 1), (1, 8, 0, 0), (7, 20, 9, 1))):
        rc, msg = _rms(spec=spec)
        assert rc == 0, msg
    t = (_lib.RmspropTable * 1)()
    t[0].n, t[0].trainable = 5, 0
    assert _lib.lib().read_rmsprop_sorted_tables(t, 1, 8, FAKE, FAKE, FAKE, 0, 0.1, 0.99, 1e-8, FAKE, None) == 0


# ---- host-side refusals ---------------------------------------------------------------------------------------------------------
def _tex(n, Cc=8, act='none'):
    from read_amd.texture import PointTexture
    return PointTexture(Cc, n, activation=act)


def test_joint_texture_construction():
    from read_amd.texture import JointTexture
    j = JointTexture([_tex(5), _tex(1), _tex(7)])
    assert j.id_bases == [0, 5, 6] and j.num_ids() == 13 and j.num_channels == 8 and len(j.trainable_parts()) == 3
    assert JointTexture([_tex(5), _tex(1), _tex(7)], [0, 8, 20]).num_ids() == 27              # gaps are accepted
    with pytest.raises(ValueError, match="channel count"):
        JointTexture([_tex(5), _tex(5, Cc=4)])
    with pytest.raises(ValueError, match="1..8 parts, got 0"):
        JointTexture([])
    with pytest.raises(ValueError, match="1..8 parts, got 9"):
        JointTexture([_tex(2) for _ in range(9)])
    with pytest.raises(ValueError, match="overlaps"):
        JointTexture([_tex(5), _tex(3)], [0, 4])
    with pytest.raises(ValueError, match="id_bases"):
        JointTexture([_tex(5), _tex(3)], [1, 6])
    with pytest.raises(ValueError, match="id_bases"):
        JointTexture([_tex(5), _tex(3)], [0])
    with pytest.raises(ValueError, match="PointTexture"):
        JointTexture([torch.nn.Linear(2, 2)])


def test_joint_texture_forwards_the_training_mode_and_freezes_by_part():
    from read_amd.texture import JointTexture
    a, b = _tex(5), _tex(3)
    j = JointTexture([a, b])
    assert not j.sparse_training
    j.sparse_training = True
    assert a.sparse_training and b.sparse_training
    b.texture_.requires_grad_(False)
    assert j.wants_grad() and j.trainable_parts() == [a]
    a.texture_.requires_grad_(False)
    assert not j.wants_grad()
    assert [k for k, _ in j.named_parameters()] == ["parts.0.texture_", "parts.1.texture_"]


def test_optimizer_keeps_one_state_per_part():
    from read_amd.texture import JointTexture
    from read_amd.train import SparseDescriptorRMSprop
    a, b, c = _tex(5), _tex(3), _tex(4)
    j = JointTexture([a, b])
    opt = SparseDescriptorRMSprop([j, a, c])
    assert [id(t) for t in opt._tables()] == [id(a), id(b), id(c)]                            # the parts once each, then the rest
    assert [id(p) for p in opt.param_groups[0]['params']] == [id(a.texture_), id(b.texture_), id(c.texture_)]
    assert [id(t) for t in SparseDescriptorRMSprop([a, c])._tables()] == [id(a), id(c)]       # no joint: the list itself


def test_stitched_scene_joint_texture():
    from read_amd.render import Scene, StitchedScene
    rng = np.random.default_rng(0)
    st = StitchedScene([Scene(rng.standard_normal((n, 3)).astype(np.float32)) for n in (30, 12)])
    j = st.joint_texture([_tex(30), _tex(12)])
    assert j.id_bases == st.id_base() == [0, 30] and j.num_ids() == 42
    with pytest.raises(ValueError, match="size does not match"):
        st.joint_texture([_tex(30), _tex(13)])
    with pytest.raises(ValueError, match="1 textures for 2 parts"):
        st.joint_texture([_tex(30)])


def test_refusals_name_what_is_refused():
    from read_amd import ddp
    from read_amd.net_texture import NetAndTexture
    from read_amd.texture import JointTexture
    a, b = _tex(5), _tex(3)
    j = JointTexture([a, b])
    with pytest.raises(NotImplementedError, match="JointTexture under DataParallelStep"):
        ddp.DataParallelStep(torch.nn.Linear(2, 2), {0: a, 'ab': j})
    ids = {'uv_1d_p1': torch.zeros(1, 1, 4, 4)}
    model = NetAndTexture(torch.nn.Identity(), {'ab': j}, supersampling=2)
    model.load_textures(['ab'])
    with pytest.raises(NotImplementedError, match="supersampling 2 with a JointTexture"):
        model(dict(ids, id=['ab']))
    with pytest.raises(NotImplementedError, match="supersampling 2 with a JointTexture"):
        j.lookup_pyramid([torch.zeros(1, 4, 4, dtype=torch.int32)], ss=2)
    # a joint whose parts are not on the GPU (nobody loaded it) says so, with or without a gradient
    with pytest.raises(ValueError, match="part 0 is not loaded on the GPU"):
        j(torch.zeros(1, 1, 4, 4))
    with torch.no_grad(), pytest.raises(ValueError, match="part 0 is not loaded on the GPU"):
        j.forward_pyramid([torch.zeros(1, 4, 4, dtype=torch.int32)])
