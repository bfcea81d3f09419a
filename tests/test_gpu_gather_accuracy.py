"""GPU: the ten entry points of read_amd/csrc/gather.hip, each called directly through its C symbol, against the float64 definitions of
tests/gather_ref64.py in units of fp32 round-off (E = |got - ref| / (u cond)) on the case set tests/test_gather_accuracy_cpu.py has
already put through both yardsticks.  Every element of every case is measured.  Each launch is held to
  1. the derived bound, elementwise (tests/gather_ref64.py counts the roundings); outputs are finite wherever inputs are finite;
  2. the yardstick cap  E_rms <= 2 max(R_torch_rms, R_seq_rms, 0.5),  E_max <= 2 max(R_torch_max, R_seq_max, 1);  a row that needs more
     is `raised` to the leading term of its derived bound and must be explained in profiles/gather_accuracy_fp64.md;
  3. exactness, compared as uint32, where the code promises it: activation none hands the addressed row's bits through (-0, subnormals
     and NaN payloads included); ss = 1 and odd ss are the plain gather of the centre sample; one table / one part are the plain
     gather; read_bilinear_down_backward is dout / 4 on the footprint (dout on the centre of odd ss) and +0 elsewhere; a row hit once
     by the scatter-add holds the gradient's bits, an untouched row +0; y = 1.0f gives g = 0 through the table adjoint; clamped ids
     address rows 0 and n - 1 forward and backward; texture_to_rows o rows_to_texture is the identity;
  4. the 4096-fold row is summed twice: both runs obey rule 1, their difference is printed and asserted nowhere.
Every output buffer is prefilled with a NaN bit pattern and sits between two guard bands of 64 floats: the bands must come back
bit-identical and no sentinel may survive inside.  Run with -s to see the table; lines start with "GACC|"."""
import ctypes as C

import numpy as np
import pytest
import torch

from read_amd import _lib
from tests import gather_ref64 as G
from tests import joint_texture_model as jm

pytestmark = pytest.mark.gpu
f32 = np.float32
BAND = G.GUARD_FLOATS


def _i32(pattern):
    return int(np.uint32(pattern).view(np.int32))


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


class Guarded:
    """A device buffer of `numel` 4-byte elements (or bytes, kind "u8") between two guard bands; filled with the sentinel, or zeroed."""

    def __init__(self, numel, kind="f32", zero=False):
        self.kind, self.numel = kind, int(numel)
        words = self.numel if kind != "u8" else (self.numel + 3) // 4
        self.buf = torch.full((words + 2 * BAND,), 0 if zero else _i32(G.SENTINEL), dtype=torch.int32, device="cuda")
        self.buf[:BAND] = _i32(G.GUARD)
        self.buf[BAND + words:] = _i32(G.GUARD)
        self.words = words

    def ptr(self):
        return self.buf.data_ptr() + 4 * BAND

    def host(self, shape=None):
        """Synchronise, check the guard bands, -> the payload on the host."""
        torch.cuda.synchronize()
        h = self.buf.cpu().numpy()
        assert (h[:BAND] == _i32(G.GUARD)).all() and (h[BAND + self.words:] == _i32(G.GUARD)).all(), "a guard band was written"
        body = h[BAND:BAND + self.words]
        out = body.view(np.uint8)[:self.numel] if self.kind == "u8" else body.view(f32) if self.kind == "f32" else body
        return out.copy() if shape is None else out.reshape(shape).copy()


def _counts(levels):
    return (C.c_int64 * len(levels))(*[0 if x is None else len(x) for x in levels])


def _ptrs(bufs):
    return _lib.ptr_array([None if b is None else (b.ptr() if isinstance(b, Guarded) else b.data_ptr()) for b in bufs])


def _level_outputs(levels, width, kind="f32", zero=False):
    return [None if ids is None else Guarded(len(ids) * width, kind, zero) for ids in levels]


def _collect(outs, width):
    return [None if o is None else o.host((-1, width) if width else None) for o in outs]


def plain_gather(hip, rows_d, n, Cc, levels, act):
    """read_gather_forward -> per-level host arrays (P_l, C), None for an empty level (passed as null pointers)."""
    ids_d = [None if ids is None else _dev(ids, torch.int32) for ids in levels]
    outs = _level_outputs(levels, Cc)
    _lib.check(hip.read_gather_forward(rows_d.data_ptr(), n, Cc, len(levels), _ptrs(ids_d), _counts(levels), _ptrs(outs), G.ACT_ID[act],
                                       _lib.stream_ptr()), "read_gather_forward")
    return _collect(outs, Cc)


def _exact(what, got, want):
    if not np.array_equal(G.bits(got), G.bits(want)):
        bad = int((G.bits(got) != G.bits(want)).sum())
        G.FAILED.append(f"{what}: {bad} of {np.size(got)} elements differ in their bits")


# ------------------------------------------------------------------------------------------ the layout change
def test_layout_change_is_the_transpose_on_bits(hip):
    st = _lib.stream_ptr()
    for case in G.transpose_cases():
        n, Cc, tex = case["n"], case["C"], case["tex"]
        tex_d = _dev(tex)
        rows = Guarded(n * Cc)
        _lib.check(hip.read_texture_to_rows(tex_d.data_ptr(), n, Cc, rows.ptr(), st))
        got = rows.host((n, Cc))
        _exact(f"texture_to_rows {case['name']}", got, tex.T)
        back = Guarded(n * Cc)
        _lib.check(hip.read_rows_to_texture(rows.ptr(), n, Cc, back.ptr(), st))
        _exact(f"rows_to_texture o texture_to_rows {case['name']}", back.host((Cc, n)), tex)
        _exact(f"rows_to_texture {case['name']}", back.host((Cc, n)), G.rows_to_texture_seq(got))
        print("GACC| %-14s | - | %-52s | both directions and the round trip are the transpose on bits" % ("layout", case["name"]))
    G.finish()


# ------------------------------------------------------------------------------------------ the plain gather
def test_plain_gather_forward(hip):
    """read_gather_forward: every C x n x level table x activation, the value classes, the grid-stride launches, the 2^20-row table."""
    for which in ("small", "grid"):
        for case in G.gather_cases(which):
            L = G.gather_launch(case)
            got = G.cat(plain_gather(hip, _dev(case["rows"]), case["n"], case["C"], case["levels"], case["act"]))
            G.run_judge("gather_fwd", case, got, L)
            if L["want_bits"] is not None:                           # the addressed (clamped) row's bits: -0, subnormals, NaN payloads
                if not np.array_equal(G.bits(got), L["want_bits"]):
                    G.FAILED.append(f"gather_fwd {case['name']}: activation none does not hand the addressed row's bits through")
    n, Cc, ids, sparse = G.big_table_case()
    rows_d = torch.empty((n, Cc), dtype=torch.float32, device="cuda")
    for r, v in sparse.items():
        rows_d[r] = _dev(v)
    got = plain_gather(hip, rows_d, n, Cc, [ids], "none")[0]
    _exact(f"gather_fwd n {n} C {Cc}: ids near the top of the table", got, np.stack([sparse[int(r)] for r in G.clamp(ids, n)]))
    print("GACC| %-14s | a | %-52s | %d ids near the top read back on bits" % ("gather_fwd", f"n 2^20+3 C{Cc}", len(ids)))
    G.finish()


# ------------------------------------------------------------------------------------------ the supersampled gather
def ss_gather(hip, case):
    Cc, B, ss = case["C"], case["B"], case["ss"]
    rows_d = _dev(case["rows"])
    idx_d = [_dev(i, torch.int32) for i in case["idx"]]
    outs = [Guarded(B * h * w * Cc) for h, w in case["sizes"]]
    hs, ws = (C.c_int * len(outs))(*[h for h, _ in case["sizes"]]), (C.c_int * len(outs))(*[w for _, w in case["sizes"]])
    _lib.check(hip.read_gather_forward_ss(rows_d.data_ptr(), case["n"], Cc, len(outs), B, _ptrs(idx_d), hs, ws, ss, _ptrs(outs), G.ACT_ID[case["act"]],
                                          _lib.stream_ptr()), "read_gather_forward_ss")
    return _collect(outs, Cc), rows_d


def test_supersampled_gather(hip):
    """read_gather_forward_ss through the C entry point: ss 1..8, B 1 and 3, sizes with h = 1 and w = 1, every activation."""
    for which in ("small", "grid"):
        for case in G.ss_cases(which):
            L = G.ss_launch(case)
            got, rows_d = ss_gather(hip, case)
            G.run_judge("gather_ss", case, G.cat(got), L)
            if case["ss"] & 1:                                       # ss = 1 and odd ss: the plain gather of the centre samples, bit for bit
                centre = plain_gather(hip, rows_d, case["n"], case["C"], [c.reshape(-1) for c in L["centre_ids"]], case["act"])
                _exact(f"gather_ss {case['name']}: odd ss against read_gather_forward of the centre samples", G.cat(got), G.cat(centre))
    G.finish()


# ------------------------------------------------------------------------------------------ the bilinear down-scale and its adjoint
def test_bilinear_down_and_its_adjoint(hip):
    st = _lib.stream_ptr()
    for which in ("small", "grid"):
        for case in G.down_cases(which):
            ss = case["ss"]
            if case["x"] is not None:
                P, sh, sw = case["x"].shape
                x_d, out = _dev(case["x"]), Guarded(P * (sh // ss) * (sw // ss))
                _lib.check(hip.read_bilinear_down(x_d.data_ptr(), P, sh // ss, sw // ss, ss, out.ptr(), st), "read_bilinear_down")
                ref, cond, bound = G.down_ref(case["x"], ss)
                L = dict(ref=ref, cond=cond, lead=None, bound=bound, torch=lambda: G.down_torch(case["x"], ss), seq=lambda: G.down_seq32(case["x"], ss))
                G.run_judge("down", case, out.host(ref.shape), L)
            if case["dout"] is not None:
                P, h, w = case["dout"].shape
                d_d, din = _dev(case["dout"]), Guarded(P * h * w * ss * ss)
                _lib.check(hip.read_bilinear_down_backward(d_d.data_ptr(), P, h, w, ss, din.ptr(), st), "read_bilinear_down_backward")
                got = din.host((P, h * ss, w * ss))
                # dout / 4 on the footprint of even ss, dout on the centre of odd ss, +0 everywhere else: the fp32 transpose is exact
                _exact(f"down_bwd {case['name']}", got, G.down_backward_ref(case["dout"], ss, f32))
                foot = G.down_backward_footprint(h, w, ss)
                if G.bits(got[:, ~foot]).any():
                    G.FAILED.append(f"down_bwd {case['name']}: a sample outside the footprint is not +0")
                print("GACC| %-14s | %s | %-52s | exact on bits: %d footprint samples, %d zeros" % ("down_bwd", case["cls"], case["name"], P * int(foot.sum()),
                                                                                                  P * int((~foot).sum())))
    G.finish()


# ------------------------------------------------------------------------------------------ the scatter-add
def scatter(hip, n, Cc, levels, grads, drows=None):
    ids_d = [None if ids is None else _dev(ids, torch.int32) for ids in levels]
    g_d = [None if g is None else _dev(g) for g in grads]
    drows = Guarded(n * Cc, zero=True) if drows is None else drows
    _lib.check(hip.read_gather_backward(drows.ptr() if isinstance(drows, Guarded) else drows.data_ptr(), n, Cc, len(levels), _ptrs(ids_d), _counts(levels),
                                        _ptrs(g_d), _lib.stream_ptr()), "read_gather_backward")
    return drows


def _scatter_exact(name, case, L, got):
    once = L["hits"] == 1
    ids = np.concatenate([i for i in case["levels"] if i is not None])
    r = G.clamp(ids, case["n"])
    g = G.cat(case["grads"])
    first = {int(row): k for k, row in reversed(list(enumerate(r)))}
    want = np.stack([g[first[int(row)]] for row in np.nonzero(once)[0]]) if once.any() else np.zeros((0, case["C"]), f32)
    _exact(f"scatter {name}: rows hit once hold the gradient's bits", got[once], want)
    if G.bits(got[L["hits"] == 0]).any():
        G.FAILED.append(f"scatter {name}: an untouched row is not +0")


def test_scatter_add(hip):
    """read_gather_backward: hits 1 / 2 / 64 / 65 / 4096, the background row, clamped ids, every C and level table, the grid-stride
    launches; the 4096-fold rows are summed twice."""
    for which in ("small", "grid"):
        for case in G.scatter_cases(which):
            L = G.scatter_launch(case)
            got = scatter(hip, case["n"], case["C"], case["levels"], case["grads"]).host((case["n"], case["C"]))
            G.run_judge("scatter", case, got, L)
            _scatter_exact(case["name"], case, L, got)
            if case["name"].startswith("hits"):
                assert L["hits"][[0, case["n"] - 1]].tolist() == [3, 2]                 # the clamped ids landed on rows 0 and n - 1
                again = scatter(hip, case["n"], case["C"], case["levels"], case["grads"]).host((case["n"], case["C"]))
                G.run_judge("scatter", case, again, L, name=case["name"] + " (second run)")
                hot = 1 + G.HITS.index(4096)
                diff = np.abs(again[hot].astype(np.float64) - got[hot]) / (G.U * L["cond"][hot])
                print("GACC| %-14s | %s | %-52s | run-to-run spread of the 4096-fold row: max %.2f u cond, %d of %d elements differ" % (
                    "scatter", case["cls"], case["name"], diff.max(), int((again[hot] != got[hot]).sum()), case["C"]))
    # the 2^20-row table: gradients land near the top and on row 0, nothing else is touched
    n, Cc, ids, sparse = G.big_table_case()
    rng = np.random.default_rng(21)
    g = rng.standard_normal((len(ids), Cc)).astype(f32)
    drows = torch.zeros((n, Cc), dtype=torch.float32, device="cuda")
    scatter(hip, n, Cc, [ids], [g], drows)
    torch.cuda.synchronize()
    touched = torch.nonzero((drows.view(torch.int32) != 0).any(dim=1))[:, 0].cpu().numpy()
    uniq, compact = np.unique(G.clamp(ids, n), return_inverse=True)
    assert np.array_equal(touched, uniq), "the 2^20-row table: the rows touched are not the rows addressed"
    case = dict(name=f"n 2^20+3 C{Cc} ids near the top", cls="a", C=Cc, n=len(uniq), levels=[compact.astype(np.int32)], grads=[g])
    G.run_judge("scatter", case, drows[torch.from_numpy(uniq).cuda()].cpu().numpy(), G.scatter_launch(case))
    G.finish()


# ------------------------------------------------------------------------------------------ the table pair
def _tables(case, rows_d=None):
    t = (_lib.GatherTable * len(case["sizes"]))()
    for k, (n, b, a) in enumerate(zip(case["sizes"], case["bases"], case["acts"])):
        t[k].rows_nc = None if rows_d is None else rows_d[k].data_ptr()
        t[k].n, t[k].id_base, t[k].activation = int(n), int(b), G.ACT_ID[a]
    return t


def tables_forward(hip, case, rows_d):
    ids_d = [None if ids is None else _dev(ids, torch.int32) for ids in case["levels"]]
    outs = _level_outputs(case["levels"], case["C"])
    _lib.check(hip.read_gather_forward_tables(_tables(case, rows_d), len(case["sizes"]), case["C"], len(case["levels"]), _ptrs(ids_d), _counts(case["levels"]),
                                              _ptrs(outs), _lib.stream_ptr()), "read_gather_forward_tables")
    return outs, ids_d


def tables_backward(hip, case, ids_d, d, y_d, pairs, dense):
    """y_d: per-level device pointers of the forward's output (Guarded buffers or tensors).  -> (g per level | None, drows per table | None)."""
    d_d = [None if x is None else _dev(x) for x in d]
    g = _level_outputs(case["levels"], case["C"]) if pairs else None
    drows = [Guarded(n * case["C"], zero=True) for n in case["sizes"]] if dense else None
    any_act = any(a != "none" for a in case["acts"])
    _lib.check(hip.read_gather_backward_tables(_tables(case), len(case["sizes"]), case["C"], len(case["levels"]), _ptrs(ids_d), _counts(case["levels"]), _ptrs(d_d),
                                               _ptrs(y_d) if any_act else None, _ptrs(g) if pairs else None, _ptrs(drows) if dense else None,
                                               _lib.stream_ptr()), "read_gather_backward_tables")
    return g, drows


def test_table_gather_and_its_adjoint(hip):
    """read_gather_forward_tables / read_gather_backward_tables at C 12, 20 and 64, eight tables, empty levels, the grid-stride boundary."""
    for case in G.table_cases():
        Cc = case["C"]
        rows_d = [_dev(r) for r in case["tables"]]
        L = G.tables_forward_launch(case)
        outs, ids_d = tables_forward(hip, case, rows_d)
        y = G.cat(_collect(outs, Cc))
        G.run_judge("tables_fwd", case, y, L)
        _exact(f"tables_fwd {case['name']}: activation none hands the addressed row's bits through", y[L["plain"]], L["want_bits"].view(f32)[L["plain"]])
        # the adjoint reads the device's own y
        pairs, dense = G.tables_backward_launch(case, y)
        g, drows = tables_backward(hip, case, ids_d, case["d"], outs, True, True)
        got = G.cat(_collect(g, Cc))
        ids = L["ids"]
        t, local = G.table_select(case, ids)
        true = np.zeros(got.shape)                                   # d act'(x) at the raw row: printed, asserted nowhere
        for s, (rows, act) in enumerate(zip(case["tables"], case["acts"])):
            x = rows.astype(np.float64)[local[t == s]]
            true[t == s] = G.cat(case["d"])[t == s] * jm.act_slope(G.act64(x, act), act)
        away = G.stats(np.abs(got - true), pairs["cond"])[0]
        G.run_judge("tables_bwd pairs", case, got, pairs)
        print("GACC| %-14s | a | %-52s | distance to d act'(x) at the raw row: max %.2f u cond" % ("tables_bwd", case["name"], away))
        _exact(f"tables_bwd {case['name']}: activation none, g is d", got[pairs["plain"]], G.cat(case["d"])[pairs["plain"]])
        for s, D in enumerate(dense):
            got_s = drows[s].host((case["sizes"][s], Cc))
            G.run_judge("tables_bwd dense", case, got_s, D, name=f"{case['name']} table {s}")
            if G.bits(got_s[D["hits"] == 0]).any():
                G.FAILED.append(f"tables_bwd dense {case['name']} table {s}: an untouched row is not +0")
    G.finish()


def test_one_table_and_one_part_are_the_plain_gather(hip):
    for Cc in (12, 64):
        for act in G.ACTS:
            rng = np.random.default_rng([31, Cc])
            n = 23
            rows = G.value_rows("d", n, Cc, rng)
            levels = [G.level_ids(P, n, rng, k) for k, P in enumerate(G.LEVEL_TABLES["7-0-1-130-3"])]
            rows_d = _dev(rows)
            plain = G.cat(plain_gather(hip, rows_d, n, Cc, levels, act))
            case = dict(C=Cc, sizes=(n,), bases=(0,), acts=(act,), levels=levels)
            outs, _ = tables_forward(hip, case, [rows_d])
            _exact(f"one table C{Cc} {act} against read_gather_forward", G.cat(_collect(outs, Cc)), plain)
            # one part: local ids inside the table, depth 1 everywhere, so every pixel is a candidate
            inside = [None if ids is None else G.clamp(ids, n).astype(np.int32) for ids in levels]
            part = dict(C=Cc, counts=G.LEVEL_TABLES["7-0-1-130-3"], want_feat=True, visible=[True],
                        parts=[(rows, inside, [None if i is None else np.ones(len(i), f32) for i in inside], 0, act)])
            feat = stitch(hip, part)[3]
            _exact(f"one part C{Cc} {act} against read_gather_forward", G.cat(feat), plain)
            print("GACC| %-14s | d | %-52s | one table and one part equal read_gather_forward on bits" % ("tables / stitch", f"C{Cc} {act}"))
    G.finish()


def test_saturated_output_gives_a_zero_gradient(hip):
    """y = 1.0f through the table adjoint: g = 0 for sigmoid and tanh (y = -1.0f for tanh as well), whatever d is."""
    Cc, P = 12, 70
    rng = np.random.default_rng(33)
    d = (rng.standard_normal((P, Cc)) * 2.0 ** rng.uniform(-20, 20, (P, Cc))).astype(f32)
    for act, yv in (("sigmoid", 1.0), ("tanh", 1.0), ("tanh", -1.0)):
        case = dict(C=Cc, sizes=(5,), bases=(0,), acts=(act,), levels=[rng.integers(-1, 7, P).astype(np.int32)])
        ids_d = [_dev(case["levels"][0], torch.int32)]
        g, drows = tables_backward(hip, case, ids_d, [d], [_dev(np.full((P, Cc), yv, f32))], True, True)
        got, rows = g[0].host((P, Cc)), drows[0].host((5, Cc))
        if (G.bits(got) & np.uint32(0x7FFFFFFF)).any() or (G.bits(rows) & np.uint32(0x7FFFFFFF)).any():
            G.FAILED.append(f"tables_bwd {act} y = {yv}: the gradient is not 0")
        print("GACC| %-14s | d | %-52s | g = 0 on all %d elements, pairs and dense" % ("tables_bwd", f"{act} y = {yv}", P * Cc))
    G.finish()


# ------------------------------------------------------------------------------------------ stitch
def stitch(hip, case):
    """read_stitch_gather_forward -> (idx, depth, part, feat) per level (feat None without features)."""
    Cc, counts, parts = case["C"], case["counts"], case["parts"]
    table = (_lib.StitchPart * len(parts))()
    keep = []
    for s, (rows, idx, dep, base, act) in enumerate(parts):
        rows_d = _dev(rows)
        keep.append(rows_d)
        if case["visible"][s]:
            i_d = [None if i is None else _dev(i, torch.int32) for i in idx]
            d_d = [None if x is None else _dev(x) for x in dep]
            ip, dp = _ptrs(i_d), _ptrs(d_d)
            keep += [i_d, d_d, ip, dp]
            table[s].idx_levels, table[s].depth_levels = ip, dp
        table[s].rows_nc = rows_d.data_ptr() if case["want_feat"] else None
        table[s].n, table[s].id_base, table[s].activation = len(rows), int(base), G.ACT_ID[act]
    lv = [None if P == 0 else np.zeros(P) for P in counts]
    o_i, o_d, o_p = _level_outputs(lv, 1, "i32"), _level_outputs(lv, 1), _level_outputs(lv, 1, "u8")
    o_f = _level_outputs(lv, Cc) if case["want_feat"] else None
    _lib.check(hip.read_stitch_gather_forward(table, len(parts), Cc, len(counts), (C.c_int64 * len(counts))(*counts), _ptrs(o_i), _ptrs(o_d), _ptrs(o_p),
                                              _ptrs(o_f) if o_f else None, _lib.stream_ptr()), "read_stitch_gather_forward")
    return _collect(o_i, 0), _collect(o_d, 0), _collect(o_p, 0), _collect(o_f, Cc) if o_f else None


def test_stitch_gather(hip):
    """read_stitch_gather_forward at C 12 and 64, eight parts, a hidden part, empty levels, the launch without features."""
    for case in G.stitch_cases():
        ref = G.stitch_ref(case["parts"], case["visible"])
        gi, gd, gp, gf = stitch(hip, case)
        for l, lv in enumerate(ref):
            if lv is None:
                continue
            mi, md, mp, y, bound, lead = lv
            what = f"stitch {case['name']} level {l}"
            if not (np.array_equal(gi[l], mi) and np.array_equal(G.bits(gd[l]), G.bits(md)) and np.array_equal(gp[l], mp)):
                G.FAILED.append(what + ": the merged index / depth / part images differ from the merge contract")
            if gf is None:
                continue
            src = np.where(mp == 255, 0, mp)
            loc = mi - np.asarray([p[3] for p in case["parts"]])[src]
            seq, tor = np.zeros(y.shape, f32), np.zeros(y.shape, f32)
            for s, p in enumerate(case["parts"]):
                seq[src == s], tor[src == s] = G.act32_seq(p[0][loc[src == s]], p[4]), G.act32_torch(p[0][loc[src == s]], p[4])
                if p[4] == "none":
                    _exact(what + f": part {s} (activation none) hands its rows' bits through", gf[l][src == s], p[0][loc[src == s]])
            L = dict(ref=y, cond=np.abs(y), lead=lead, bound=bound, seq=lambda: seq, torch=lambda: tor)
            G.run_judge("stitch", dict(case, cls="a"), gf[l], L, name=f"{case['name']} level {l}")
        if gf is None:
            print("GACC| %-14s | a | %-52s | merged images exact, no features" % ("stitch", case["name"]))
    G.finish()
