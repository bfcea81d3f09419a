"""CPU: the float64 model of the table gather's adjoint (tests/joint_texture_model.py) against torch.autograd through
act_t(cat(tables)[clamped ids]) — table selection, the clamp and act' — in pairs mode and dense mode, on the case set the GPU tests use.
This pins the contract; the device is held to the model in tests/test_gpu_joint_texture.py."""
import numpy as np
import pytest
import torch

from tests import joint_texture_model as jm

_T_ACT = {"none": lambda x: x, "sigmoid": torch.sigmoid, "tanh": torch.tanh}


def _case(Cc, layout, acts, seed):
    rng = np.random.default_rng([7, Cc, seed])
    bases = jm.LAYOUTS[layout]
    tables = [rng.standard_normal((n, Cc)) for n in jm.SIZES]
    ids = np.concatenate([m.reshape(-1) for m in jm.draw_ids(bases, rng)])
    d = rng.standard_normal((ids.size, Cc))
    return bases, jm.ACTS[acts], tables, ids, d


def test_case_set_contains_what_it_promises():
    for layout, bases in jm.LAYOUTS.items():
        rng = np.random.default_rng(1)
        for m in jm.draw_ids(bases, rng):
            flat = m.reshape(-1)
            assert set(jm.required_ids(bases)) <= set(flat.tolist()), layout
            t, local = jm.select(flat, bases, jm.SIZES)
            assert max(np.bincount(local[t == 2])) >= jm.HOT_HITS
        if layout == "gapped":
            assert any(all(not b <= i < b + n for b, n in zip(bases, jm.SIZES)) and 0 <= i < bases[-1] for i in jm.required_ids(bases))


def test_select_clamps_as_the_forward_documents():
    t, local = jm.select([-3, 0, 4, 5, 7, 8, 9, 19, 20, 26, 27, 1000], (0, 8, 20), (5, 1, 7))
    assert t.tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 2, 2, 2, 2]
    assert local.tolist() == [0, 0, 4, 4, 4, 0, 0, 0, 0, 6, 6, 6]


@pytest.mark.parametrize("Cc,layout,acts", jm.cases())
def test_adjoint_model_is_autograd_of_the_concatenated_table(Cc, layout, acts):
    bases, act_names, tables, ids, d = _case(Cc, layout, acts, 0)
    t, local = jm.select(ids, bases, jm.SIZES)
    offset = np.concatenate([[0], np.cumsum(jm.SIZES)[:-1]])
    cat = torch.from_numpy(np.concatenate(tables)).requires_grad_(True)
    picked = cat[torch.from_numpy(offset[t] + local)]                       # (P, C): the row every pixel reads
    picked.retain_grad()
    y = torch.empty_like(picked)
    for s, name in enumerate(act_names):
        m = torch.from_numpy(t == s)
        y = torch.where(m[:, None], _T_ACT[name](picked), y)
    (y * torch.from_numpy(d)).sum().backward()
    y64 = jm.forward(ids, tables, bases, act_names)
    np.testing.assert_allclose(y64, y.detach().numpy(), rtol=1e-13, atol=1e-15)
    g = jm.adjoint_pairs(ids, d, y64, bases, jm.SIZES, act_names)
    np.testing.assert_allclose(g, picked.grad.numpy(), rtol=1e-12, atol=1e-14)
    drows, hits, _ = jm.adjoint_dense(ids, d, y64, bases, jm.SIZES, act_names)
    np.testing.assert_allclose(np.concatenate(drows), cat.grad.numpy(), rtol=1e-12, atol=1e-13)
    assert sum(int(h.sum()) for h in hits) == ids.size
    if acts == "none":
        assert np.array_equal(g, d)


def test_frozen_table_receives_nothing_and_changes_nothing_else():
    bases, act_names, tables, ids, d = _case(4, "gapped", "mixed", 1)
    y = jm.forward(ids, tables, bases, act_names)
    full, _, _ = jm.adjoint_dense(ids, d, y, bases, jm.SIZES, act_names)
    part, _, _ = jm.adjoint_dense(ids, d, y, bases, jm.SIZES, act_names, frozen=(1,))
    assert part[1] is None and np.array_equal(part[0], full[0]) and np.array_equal(part[2], full[2])
