"""CPU: tests/gather_ref64.py checked before anything runs on the device.
  * every float64 reference equals the torch float64 CPU operation or its autograd on the shared cases: gathers bit for bit, blends and
    sums to 1e-15 relative, <A x, y> = <x, A^T y> for both adjoint pairs;
  * on every shared case the NumPy fp32 restatement and the torch fp32 yardstick stay under the derived bound elementwise, and each
    meets the yardstick cap against the other;
  * a catalogue of deliberately wrong fp32 models: each is rejected by the shared case its test id names."""
import numpy as np
import pytest
import torch

from tests import gather_ref64 as G
from tests import joint_texture_model as jm

f32 = np.float32


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)) if a.size else 0.0


def _act_t(t, act):
    return torch.sigmoid(t) if act == "sigmoid" else torch.tanh(t) if act == "tanh" else t


# ------------------------------------------------------------------------------------------ the references against torch float64
def test_gather_and_scatter_references_equal_torch_float64():
    for case in list(G.gather_cases()) + list(G.gather_cases("grid")):
        L = G.gather_launch(case)
        ids = torch.from_numpy(G.clamp(np.concatenate([i for i in case["levels"] if i is not None]), case["n"]))
        raw = torch.index_select(torch.from_numpy(case["rows"].astype(np.float64)), 0, ids)
        if case["act"] == "none":
            assert np.array_equal(L["ref"].view(np.uint64), raw.numpy().view(np.uint64)), case["name"]
            continue
        want, got = _act_t(raw, case["act"]).numpy(), L["ref"]
        fin = np.isfinite(want)
        assert np.array_equal(np.isnan(want), np.isnan(got)) and np.abs(got[fin] - want[fin]).max() <= 1e-15 * np.abs(want[fin]).max(), case["name"]
        tiny = fin & (np.abs(want) > 1e-300)                                  # relative, element by element, where tanh keeps it
        assert (np.abs(got[tiny] - want[tiny]) <= 4e-15 * np.abs(want[tiny])).all(), case["name"]
    for case in list(G.scatter_cases()) + list(G.scatter_cases("grid")):
        L = G.scatter_launch(case)
        acc = torch.zeros((case["n"], case["C"]), dtype=torch.float64)
        for ids, g in zip(case["levels"], case["grads"]):
            if ids is not None:
                acc.index_add_(0, torch.from_numpy(G.clamp(ids, case["n"])), torch.from_numpy(g.astype(np.float64)))
        # np.add.at and index_add_ both add a level's pixels in pixel order: the same float64 sum, rounding for rounding
        assert (np.abs(L["ref"] - acc.numpy()) <= 1e-15 * L["cond"]).all(), case["name"]
        assert not L["ref"][L["hits"] == 0].any()
        # <gather(rows), g> = <rows, scatter(g)>
        rows = np.random.default_rng(1).standard_normal((case["n"], case["C"]))
        ids = np.concatenate([i for i in case["levels"] if i is not None])
        lhs = float((rows[G.clamp(ids, case["n"])] * G.cat(case["grads"]).astype(np.float64)).sum())
        assert abs(lhs - float((rows * L["ref"]).sum())) <= 1e-12 * float((np.abs(rows) * L["cond"]).sum()), case["name"]


def test_blend_references_equal_torch_float64():
    for case in list(G.ss_cases()) + list(G.ss_cases("grid")):
        for idx in case["idx"]:
            ref = G.gather_ss_ref(case["rows"], idx, case["ss"], case["act"])[0]
            want = G.gather_ss_torch(case["rows"].astype(np.float64), idx, case["ss"], case["act"], torch.float64)
            odd = ~np.isfinite(want)                      # odd ss, class (d): NaN and +-inf centre samples come through as they are
            assert ref.shape == want.shape and np.array_equal(ref[odd], want[odd], equal_nan=True), case["name"]
            assert _rel(np.where(odd, 0.0, ref), np.where(odd, 0.0, want)) <= 1e-15, case["name"]
    rng = np.random.default_rng(2)
    for case in list(G.down_cases()) + list(G.down_cases("grid")):
        ss = case["ss"]
        if case["x"] is not None:
            ref = G.down_ref(case["x"], ss)[0]
            assert _rel(ref, G.down_torch(case["x"].astype(np.float64), ss, torch.float64)) <= 1e-15, case["name"]
        if case["dout"] is not None:
            din = G.down_backward_ref(case["dout"], ss)
            assert _rel(din, G.down_backward_torch(case["dout"].astype(np.float64), ss, torch.float64)) <= 1e-15, case["name"]
            x = rng.standard_normal(din.shape)
            lhs, rhs = float((G.down_ref(x, ss)[0] * case["dout"]).sum()), float((x * din).sum())
            assert abs(lhs - rhs) <= 1e-13 * float((np.abs(x) * np.abs(din)).sum() + 1e-300), case["name"]
            foot = G.down_backward_footprint(case["dout"].shape[1], case["dout"].shape[2], ss)
            assert not din[:, ~foot].any() and (din[:, foot] != 0).all(), case["name"]


def test_table_pair_and_stitch_references_equal_torch_float64():
    for case in G.table_cases():
        L = G.tables_forward_launch(case)
        ids = L["ids"]
        t, local = G.table_select(case, ids)
        leaves = [torch.from_numpy(r.astype(np.float64)).requires_grad_(True) for r in case["tables"]]
        y = torch.zeros((len(ids), case["C"]), dtype=torch.float64)
        for s, act in enumerate(case["acts"]):
            m = torch.from_numpy(t == s)
            y = y.index_put((torch.nonzero(m)[:, 0],), _act_t(torch.index_select(leaves[s], 0, torch.from_numpy(local[t == s])), act))
        assert _rel(L["ref"], y.detach().numpy()) <= 1e-15, case["name"]
        d = G.cat(case["d"])
        (y * torch.from_numpy(d.astype(np.float64))).sum().backward()
        drows, _, _ = jm.adjoint_dense(ids, d, L["ref"], case["bases"], case["sizes"], case["acts"])
        for s in range(len(case["sizes"])):
            # the same sum in the same order; the terms differ by the two roundings of y (1 - y) d against d (1 - y) y: 1e-15 of sum |d|
            mass = jm.adjoint_dense(ids, d, L["ref"], case["bases"], case["sizes"], case["acts"])[2][s]
            assert (np.abs(drows[s] - leaves[s].grad.numpy()) <= 1e-15 * mass).all(), (case["name"], s)
    for case in G.stitch_cases():
        ref = G.stitch_ref(case["parts"], case["visible"])
        whole = np.concatenate([p[0] for p in case["parts"]]).astype(np.float64)
        for l, P in enumerate(case["counts"]):
            assert (ref[l] is None) == (P == 0)
            if P == 0:
                continue
            mi, md, mp, y, _, _ = ref[l]
            raw = torch.index_select(torch.from_numpy(whole), 0, torch.from_numpy(mi.astype(np.int64)))      # the merged id addresses the concatenation
            for s, p in enumerate(case["parts"]):
                m = np.where(mp == 255, 0, mp) == s
                assert _rel(y[m], _act_t(raw[torch.from_numpy(m)], p[4]).numpy()) <= 1e-15, case["name"]
            assert not case["visible"].count(False) or not np.isin(mp, [s for s, v in enumerate(case["visible"]) if not v]).any()


# ------------------------------------------------------------------------------------------ the yardsticks inside every rule
def _both(family, case, L, failed):
    """Both yardsticks under the derived bound, and each under the cap the other sets."""
    G.run_judge(family, case, L["seq"](), L, failed=failed, quiet=True, against=("torch",))
    G.run_judge(family, case, L["torch"](), L, failed=failed, quiet=True, against=("seq",))


@pytest.mark.parametrize("which", ["small", "grid"])
def test_yardsticks_stay_inside_every_rule_gathers(which):
    failed = []
    for case in G.gather_cases(which):
        _both("gather_fwd", case, G.gather_launch(case), failed)
    for case in G.ss_cases(which):
        L = G.ss_launch(case)
        _both("gather_ss", case, L, failed)
        if case["ss"] & 1:                                   # odd ss: the activated centre sample, bit for bit
            want = G.cat([G.act32_seq(case["rows"][G.clamp(c.reshape(-1), case["n"])], case["act"]) for c in L["centre_ids"]])
            assert np.array_equal(G.bits(L["seq"]()), G.bits(want)), case["name"]
    for case in G.down_cases(which):
        if case["x"] is not None:
            ref, cond, bound = G.down_ref(case["x"], case["ss"])
            L = dict(ref=ref, cond=cond, lead=None, bound=bound, seq=lambda: G.down_seq32(case["x"], case["ss"]), torch=lambda: G.down_torch(case["x"], case["ss"]))
            _both("down", case, L, failed)
        if case["dout"] is not None:
            ref = G.down_backward_ref(case["dout"], case["ss"])
            for got in (G.down_backward_ref(case["dout"], case["ss"], f32), G.down_backward_torch(case["dout"], case["ss"])):
                assert np.array_equal(got.astype(np.float64), ref), case["name"]
    G.finish(failed)


@pytest.mark.parametrize("which", ["small", "grid"])
def test_yardsticks_stay_inside_every_rule_scatter(which):
    failed = []
    for case in G.scatter_cases(which):
        L = G.scatter_launch(case)
        _both("scatter", case, L, failed)
        once = L["hits"] == 1                                # a row hit once: the gradient's bits; an untouched row: +0
        for y in (L["seq"](), L["torch"]()):
            assert np.array_equal(y[once].astype(np.float64), L["ref"][once]) and not G.bits(y[L["hits"] == 0]).any(), case["name"]
    G.finish(failed)


def test_yardsticks_stay_inside_every_rule_table_pair_and_stitch():
    failed = []
    for case in G.table_cases():
        L = G.tables_forward_launch(case)
        _both("tables_fwd", case, L, failed)
        y = L["seq"]()
        pairs, dense = G.tables_backward_launch(case, y)
        _both("tables_bwd pairs", case, pairs, failed)
        for s, D in enumerate(dense):
            G.run_judge("tables_bwd dense", case, D["seq"](), D, name=f"{case['name']} table {s}", failed=failed, quiet=True, against=("torch",))
            G.run_judge("tables_bwd dense", case, D["torch"](), D, name=f"{case['name']} table {s}", failed=failed, quiet=True, against=("seq",))
    for case in G.stitch_cases():
        for l, lv in enumerate(G.stitch_ref(case["parts"], case["visible"])):
            if lv is None:
                continue
            mi, md, mp, y, bound, lead = lv
            src = np.where(mp == 255, 0, mp)
            loc = mi - np.asarray([p[3] for p in case["parts"]])[src]
            seq, tor = np.zeros(y.shape, f32), np.zeros(y.shape, f32)
            for s, p in enumerate(case["parts"]):
                seq[src == s], tor[src == s] = G.act32_seq(p[0][loc[src == s]], p[4]), G.act32_torch(p[0][loc[src == s]], p[4])
            L = dict(ref=y, cond=np.abs(y), lead=lead, bound=bound, seq=lambda: seq, torch=lambda: tor)
            _both("stitch", dict(case, cls="a"), L, failed)
    G.finish(failed)


def test_layout_change_restatement_is_the_transpose():
    for case in G.transpose_cases():
        rows = np.ascontiguousarray(case["tex"].T)
        assert np.array_equal(G.bits(G.rows_to_texture_seq(rows)), G.bits(case["tex"]))


# ------------------------------------------------------------------------------------------ the harness would notice
def _find(gen, name):
    return next(c for c in gen if c["name"] == name)


def _gather_mut(name, mut, which="small"):
    case = _find(G.gather_cases(which), name)
    return "gather_fwd", case, G.gather_launch(case), mut


def _ss_mut(name, mut):
    """name without its channel count (the case set cycles C over the launches)."""
    head, tail = name.split(" C* ")
    case = next(c for c in G.ss_cases() if c["name"].startswith(head + " C") and c["name"].endswith(" " + tail) and c["cls"] == "a")
    return "gather_ss", case, G.ss_launch(case), mut


MUTATIONS = {
    "quad_div_2": lambda: _gather_mut("C12 n257 levels 7-0-1-130-3 none", "quad_div_2"),
    "empty_level_base": lambda: _gather_mut("C8 n257 levels 7-0-1-130-3 none", "empty_level_base"),
    "stop_at_grid": lambda: _gather_mut("C64 part of the grid", "stop_at_grid", "grid"),
    "no_edge_clamp": lambda: _ss_mut("ss1 B1 C* 9x1+5x7 none", "no_edge_clamp"),
    "blend_reads_v00_twice": lambda: _ss_mut("ss2 B1 C* 9x1+5x7 none", "blend_reads_v00_twice"),
    "clamp_to_n": lambda: _gather_mut("C4 n2 levels one none", "clamp_to_n"),
    "negative_wrap": lambda: _gather_mut("C20 n257 levels 0-5-0-0-9 none", "negative_wrap"),
    "act_after_blend": lambda: _ss_mut("ss4 B3 C* 9x1+5x7 sigmoid", "act_after_blend"),
    "exp_rel_2^-18": lambda: _gather_mut("C8 n257 levels 7-0-1-130-3 sigmoid", "exp_rel_2^-18"),
    "tanh_by_exp": lambda: _gather_mut("C8 n23 levels 7-0-1-130-3 tanh", "tanh_by_exp"),
}


def test_the_named_mutation_cases_exist():
    names = {c["name"] for c in G.gather_cases()} | {c["name"] for c in G.gather_cases("grid")} | {c["name"] for c in G.ss_cases()}
    for make in MUTATIONS.values():
        assert make()[1]["name"] in names


@pytest.mark.parametrize("mutation", [f"{k}@{v()[0]}/{v()[1]['cls']}/{v()[1]['name'].replace(' ', '_')}" for k, v in MUTATIONS.items()])
def test_harness_rejects_a_wrong_decode_clamp_blend_or_activation(mutation):
    family, case, L, mut = MUTATIONS[mutation.split("@")[0]]()
    failed = []
    G.run_judge(family, case, L["seq"](), L, failed=failed, quiet=True)
    assert not failed, "the unmutated restatement must pass: " + "; ".join(failed)
    got = L["seq"](mut)
    G.run_judge(family, case, got, L, failed=failed, quiet=True)
    if L.get("want_bits") is not None and not np.array_equal(G.bits(got), L["want_bits"]):
        failed.append("bits differ from the addressed rows")
    assert failed, f"{mut} passed the harness on {case['name']}"


def test_harness_rejects_tanh_slope_1_minus_y__tables_bwd_pairs_C12_gapped_mixed():
    case = _find(G.table_cases(), "C12 gapped mixed")
    y = G.tables_forward_launch(case)["seq"]()
    failed = []
    pairs, _ = G.tables_backward_launch(case, y)
    G.run_judge("tables_bwd pairs", case, pairs["seq"](), pairs, failed=failed, quiet=True)
    assert not failed
    wrong, _ = G.tables_backward_launch(case, y, mut="tanh_slope_1-y")
    G.run_judge("tables_bwd pairs", case, wrong["seq"](), pairs, failed=failed, quiet=True)
    assert failed


@pytest.mark.parametrize("mut", ["drop_one_addend", "untouched_row_nonzero"])
def test_harness_rejects_a_wrong_sum__scatter_a_hits_C20(mut):
    case = _find(G.scatter_cases(), "hits 1/2/64/65/4096 C20")
    assert case["cls"] == "a"
    L = G.scatter_launch(case)
    failed = []
    G.run_judge("scatter", case, L["seq"](), L, failed=failed, quiet=True)
    assert not failed
    got = L["seq"](mut)
    G.run_judge("scatter", case, got, L, failed=failed, quiet=True)
    if G.bits(got[L["hits"] == 0]).any():
        failed.append("an untouched row is not +0")
    assert failed, f"{mut} passed the harness"


def test_harness_rejects_swapped_channels__rows_to_texture_n257_C12():
    case = _find(G.transpose_cases(), "n257 C12")
    rows = np.ascontiguousarray(case["tex"].T)
    assert not np.array_equal(G.bits(G.rows_to_texture_seq(rows, "swap_channels")), G.bits(case["tex"]))
