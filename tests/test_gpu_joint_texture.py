"""GPU: training through the table gather — read_gather_backward_tables against the float64 model of tests/joint_texture_model.py,
read_rmsprop_sorted_tables against the dense float64 trajectory of the CONCATENATED table (tests/train_ref64.RmspropTrajectory, the
harness of tests/test_gpu_train_accuracy.py), then JointTexture, SparseDescriptorRMSprop and NetAndTexture on top of them.

Bounds (u = 2^-24), each derived, none fitted:
  pairs   |g - d act'(y)| <= 4 u |d| per element, float64 from the fp32 d and y: act' is in [0, 1]; y y (or 1 - y), the difference
          from 1 and the product with d round once each, every one of them bounded by u against 1; one unit of slack.  Absolute,
          because 1 - y y cancels.  Activation none: g == d bit for bit.  Two runs: bit-identical (no atomics).
  dense   |drows - sum64 g| <= (k + 4) u sum |d| per row element with k contributing pixels: the 3 u of each g and k - 1 fp32 additions
          of partial sums no larger than sum |d| (in any order: the atomics commute up to round-off).  Rows nobody addressed: exactly 0.
  rmsprop |rows - traj.p| <= traj.e_p (0 for a row that was never touched: bit-unchanged), |sq - traj.sq| <= traj.e_v on touched rows.
Run with -s to see the worst ratio of every check; lines start with "JTEX|".

Worst error / bound seen on the MI355X: pairs 0.32, dense 0.26, rmsprop rows 0.40 and sq 0.29, the module-level step 0.90 (DESIGN.md
§10.2, "Training on stitched scenes")."""
import numpy as np
import pytest
import torch

from read_amd import _lib, synthetic
from read_amd.texture import JointTexture, PointTexture, gather_tables_backward, gather_tables_pyramid
from read_amd.train import SparseDescriptorRMSprop, huber_loss
from tests import joint_texture_model as jm
from tests import train_ref64 as T

pytestmark = pytest.mark.gpu
f32 = np.float32
U = 2.0 ** -24


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _report(name, err, bound):
    q = T.worst(err, bound)
    print("JTEX| %-70s | err/bound %.3f" % (name, q))
    return q


# ------------------------------------------------------------------------------------------ the adjoint of the table gather
def _adjoint_case(Cc, layout, acts):
    rng = np.random.default_rng([11, Cc, len(layout), len(acts)])
    bases, act_names = jm.LAYOUTS[layout], jm.ACTS[acts]
    tables = [rng.standard_normal((n, Cc)).astype(f32) for n in jm.SIZES]
    ids = jm.draw_ids(bases, rng)
    d = [rng.standard_normal(m.shape + (Cc,)).astype(f32) for m in ids]
    return bases, act_names, tables, ids, d


@pytest.mark.parametrize("Cc,layout,acts", jm.cases())
def test_adjoint_of_the_table_gather(hip, Cc, layout, acts):
    bases, act_names, tables, ids, d = _adjoint_case(Cc, layout, acts)
    rows_d = [_dev(t) for t in tables]
    ids_d = [_dev(m, torch.int32) for m in ids]
    d_d = [_dev(x) for x in d]
    y_d = gather_tables_pyramid([(r, b, a) for r, b, a in zip(rows_d, bases, act_names)], ids_d)      # the device's own forward
    meta = [(n, b, a) for n, b, a in zip(jm.SIZES, bases, act_names)]
    feat = None if acts == "none" else y_d
    flat_ids = np.concatenate([m.reshape(-1) for m in ids])
    flat_d = np.concatenate([x.reshape(-1, Cc) for x in d])
    flat_y = np.concatenate([_host(y).reshape(-1, Cc) for y in y_d])
    # the forward itself addresses the rows the model says (the clamp rules): act none reads them back bit for bit
    if acts == "none":
        t, local = jm.select(flat_ids, bases, jm.SIZES)
        want = np.stack([tables[a][b] for a, b in zip(t, local)])
        assert np.array_equal(_bits(flat_y), _bits(want))
    # ---- pairs mode
    g1 = gather_tables_backward(meta, ids_d, d_d, feat, pairs=True)
    g2 = gather_tables_backward(meta, ids_d, d_d, feat, pairs=True)
    got = np.concatenate([_host(g) for g in g1])
    assert np.array_equal(_bits(got), _bits(np.concatenate([_host(g) for g in g2]))), "pairs mode: two runs differ"
    ref = jm.adjoint_pairs(flat_ids, flat_d, flat_y, bases, jm.SIZES, act_names)
    q = _report(f"pairs C {Cc} {layout} {acts}", np.abs(got - ref), 4 * U * np.abs(flat_d.astype(np.float64)))
    assert q <= 1.0, f"pairs mode: {q:.3f} x the bound"
    t, _ = jm.select(flat_ids, bases, jm.SIZES)
    plain = np.array([a == "none" for a in act_names])[t]
    assert np.array_equal(_bits(got[plain]), _bits(flat_d[plain])), "activation none: g must be d bit for bit"
    # ---- dense mode: one flat buffer [table 0 | table 1 | table 2]; in the second run table 1 is frozen and its slice poisoned
    sizes = np.array(jm.SIZES)
    off = np.concatenate([[0], np.cumsum(sizes)])
    for frozen in ((), (1,)):
        flat = torch.zeros((int(off[-1]), Cc), device="cuda")
        views = [flat[off[s]:off[s + 1]] for s in range(3)]
        for s in frozen:
            views[s].fill_(float("nan"))
        assert gather_tables_backward(meta, ids_d, d_d, feat, drows=[None if s in frozen else v for s, v in enumerate(views)]) is None
        ref_rows, hits, mass = jm.adjoint_dense(flat_ids, flat_d, flat_y, bases, jm.SIZES, act_names, frozen)
        for s in range(3):
            got_s = _host(views[s])
            if s in frozen:
                assert np.isnan(got_s).all(), "a frozen table's gradient rows were written"
                continue
            k = hits[s][:, None]
            q = _report(f"dense C {Cc} {layout} {acts} table {s} frozen {frozen}", np.abs(got_s - ref_rows[s]), (k + 4) * U * mass[s])
            assert q <= 1.0, f"dense mode, table {s}: {q:.3f} x the bound"
            assert not got_s[hits[s] == 0].any(), "a row nobody addressed is not exactly 0"
        assert hits[2].max() >= jm.HOT_HITS


# ------------------------------------------------------------------------------------------ the sorted RMSprop over a table list
RMS_SIZES = (600, 1, 40)
RMS_BASES = (0, 600, 601)
RMS_N = 641


def _rms_schedule(rng):
    """Four steps of 1400 merged ids: 520 pairs of id 0 and 520 of the first row of table 2 (two long runs in different tables), runs on
    both sides of every table boundary, negative and past-the-end ids, random ids elsewhere."""
    run = lambda row, n: np.full(n, row, np.int64)                                                  # noqa: E731
    steps = []
    for _ in range(4):
        fixed = np.concatenate([run(0, 520), run(RMS_BASES[2], 520), run(RMS_BASES[1] - 1, 3), run(RMS_BASES[1], 2), run(RMS_BASES[2] + 1, 2),
                                run(-1, 3), run(-7, 1), run(RMS_N, 2), run(RMS_N + 59, 1)])
        ids = np.concatenate([fixed, rng.integers(0, RMS_N, 1400 - len(fixed))])
        steps.append(rng.permutation(ids))
    return steps


def _rms_tables(rows, sq, stamp, step, frozen=()):
    t = (_lib.RmspropTable * len(rows))()
    for k in range(len(rows)):
        t[k].rows, t[k].sq, t[k].stamp = rows[k].data_ptr(), sq[k].data_ptr(), stamp[k].data_ptr()
        t[k].n, t[k].id_base = int(rows[k].shape[0]), int(sum(r.shape[0] for r in rows[:k]))
        t[k].step, t[k].trainable = (0, 0) if k in frozen else (step, 1)
    return t


@pytest.mark.parametrize("variant", ["three tables", "table 1 frozen", "one table"])
@pytest.mark.parametrize("Cc", [8, 16])
def test_rmsprop_sorted_tables_follows_the_dense_float64_trajectory(hip, Cc, variant):
    lr, alpha, eps = f32(0.05), f32(0.99), f32(1e-8)
    rng = np.random.default_rng([43, Cc])
    rows0 = rng.standard_normal((RMS_N, Cc)).astype(f32)
    sched = _rms_schedule(rng)
    grads = [(rng.standard_normal((len(ids), Cc)) * 2.0 ** rng.uniform(-6, 2, (len(ids), 1))).astype(f32) for ids in sched]
    sizes = (RMS_N,) if variant == "one table" else RMS_SIZES
    frozen = (1,) if variant == "table 1 frozen" else ()
    off = np.concatenate([[0], np.cumsum(sizes)])
    rows = [_dev(rows0[off[k]:off[k + 1]]) for k in range(len(sizes))]
    sq = [torch.zeros_like(r) for r in rows]
    stamp = [torch.zeros(r.shape[0], dtype=torch.int32, device="cuda") for r in rows]
    scratch = torch.zeros(int(hip.read_rmsprop_sorted_scratch_ints()), dtype=torch.int32, device="cuda")
    traj = T.RmspropTrajectory(rows0, float(alpha), float(eps))
    ever = np.zeros(RMS_N, bool)
    step = 0
    for k, (ids, g) in enumerate(zip(sched, grads)):
        idle = 50 if k == 3 else 0
        if idle:
            traj.idle(idle)
        step += idle + 1
        order = np.argsort(ids, kind="stable")
        s_ids, perm, g_d = _dev(ids[order], torch.int32), _dev(order, torch.int64), _dev(g)
        _lib.check(hip.read_rmsprop_sorted_tables(_rms_tables(rows, sq, stamp, step, frozen), len(sizes), Cc, s_ids.data_ptr(), perm.data_ptr(),
                                                  g_d.data_ptr(), len(ids), float(lr), float(alpha), float(eps), scratch.data_ptr(),
                                                  _lib.stream_ptr()), "read_rmsprop_sorted_tables")
        live = np.ones(len(ids), bool) if not frozen else ids != RMS_BASES[1]           # the dense optimizer never sees a frozen table's gradient
        touched = traj.apply(ids[live], g[live], float(lr))
        ever |= touched
        got_rows, got_sq, got_stamp = (np.concatenate([_host(x) for x in xs]) for xs in (rows, sq, stamp))
        name = f"rmsprop C {Cc} {variant} step {step} ({int(touched.sum())} rows)"
        q = _report(name + " rows", np.abs(got_rows - traj.p), traj.e_p)
        assert q <= 1.0, f"{name}: rows {q:.3f} x the bound"
        q = _report(name + " sq", np.abs(got_sq[touched] - traj.sq[touched]), traj.e_v[touched] + T.TINY)
        assert q <= 1.0, f"{name}: sq {q:.3f} x the bound"
        assert np.array_equal(got_stamp[touched], np.full(int(touched.sum()), step)), name + ": stamps of the touched rows"
        assert touched[0] and touched[RMS_BASES[2]]                                    # the two long runs were applied
    # rows no valid id ever named — and with them everything a negative or past-the-end id could have been clamped to — are bit-unchanged
    assert np.array_equal(_bits(got_rows[~ever]), _bits(rows0[~ever])) and not got_sq[~ever].any() and not got_stamp[~ever].any()
    if frozen:
        k = frozen[0]
        assert np.array_equal(_bits(_host(rows[k])), _bits(rows0[off[k]:off[k + 1]])), "a frozen table's rows changed"
        assert not _host(sq[k]).any() and not _host(stamp[k]).any(), "a frozen table's optimizer state changed"


def test_rmsprop_sorted_tables_with_one_table_is_read_rmsprop_sorted(hip):
    Cc = 8
    rng = np.random.default_rng(47)
    rows0 = rng.standard_normal((RMS_N, Cc)).astype(f32)
    ids = _rms_schedule(rng)[0]
    g = rng.standard_normal((len(ids), Cc)).astype(f32)
    order = np.argsort(ids, kind="stable")
    s_ids, perm, g_d = _dev(ids[order], torch.int32), _dev(order, torch.int64), _dev(g)
    scratch = torch.zeros(int(hip.read_rmsprop_sorted_scratch_ints()), dtype=torch.int32, device="cuda")
    state = []
    for tables in (False, True):
        rows, sq, stamp = _dev(rows0), torch.zeros((RMS_N, Cc), device="cuda"), torch.zeros(RMS_N, dtype=torch.int32, device="cuda")
        if tables:
            _lib.check(hip.read_rmsprop_sorted_tables(_rms_tables([rows], [sq], [stamp], 1), 1, Cc, s_ids.data_ptr(), perm.data_ptr(), g_d.data_ptr(),
                                                      len(ids), 0.05, 0.99, 1e-8, scratch.data_ptr(), _lib.stream_ptr()))
        else:
            _lib.check(hip.read_rmsprop_sorted(rows.data_ptr(), sq.data_ptr(), stamp.data_ptr(), Cc, RMS_N, s_ids.data_ptr(), perm.data_ptr(),
                                               g_d.data_ptr(), len(ids), 1, 0.05, 0.99, 1e-8, scratch.data_ptr(), _lib.stream_ptr()))
        state.append([_host(x) for x in (rows, sq, stamp)])
    for a, b in zip(*state):
        assert np.array_equal(_bits(a.astype(f32)), _bits(b.astype(f32)))


# ------------------------------------------------------------------------------------------ JointTexture and the optimizer
PART_SIZES = (300, 50, 120)


def _parts(rng, Cc=8, sizes=PART_SIZES, sparse=True):
    parts = []
    for n in sizes:
        p = PointTexture(Cc, n)
        p.texture_.data.copy_(torch.from_numpy(rng.standard_normal((1, Cc, n)).astype(f32)))
        parts.append(p)
    joint = JointTexture(parts).cuda()
    joint.sparse_training = sparse
    return parts, joint


def _concat(parts):
    """(N, C) fp32: the parts' rows as the optimizer left them (state_dict() writes them back into texture_)."""
    return np.concatenate([p.state_dict()["texture_"][0].t().cpu().numpy() for p in parts])


def _id_map(rng, N, shape=(2, 1, 32, 24)):
    ids = rng.integers(0, N, shape)
    ids[rng.random(shape) < 0.4] = 0
    return torch.from_numpy(ids.astype(f32)).cuda()


def test_joint_texture_forward_is_the_concatenated_point_texture(hip):
    rng = np.random.default_rng(51)
    parts, joint = _parts(rng)
    N = sum(PART_SIZES)
    whole = PointTexture(8, N)
    whole.texture_.data.copy_(torch.from_numpy(_concat(parts).T.copy())[None])
    whole.cuda()
    ids = _id_map(rng, N)
    with torch.no_grad():
        a, b = joint(ids), whole(ids)
        pyr = joint.forward_pyramid([ids[:, 0].to(torch.int32).contiguous()])[0]
    assert a.shape == (2, 8, 32, 24) and torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(pyr.permute(0, 3, 1, 2), a)
    assert joint.num_ids() == N and joint.id_bases == [0, 300, 350]
    joint.check_ids()
    with torch.no_grad():
        joint(torch.full((1, 1, 2, 2), float(N), device="cuda"))
    with pytest.raises(IndexError):
        joint.check_ids()


@pytest.mark.parametrize("frozen", [None, 1])
def test_joint_texture_sparse_step_follows_the_trajectory(hip, frozen):
    rng = np.random.default_rng(52)
    parts, joint = _parts(rng)
    N, lr = sum(PART_SIZES), 0.05
    if frozen is not None:
        parts[frozen].texture_.requires_grad_(False)
    rows0 = _concat(parts)
    frozen_ckpt = None if frozen is None else {k: v.clone() for k, v in parts[frozen].state_dict().items()}
    opt = SparseDescriptorRMSprop([joint], lr=lr)
    traj = T.RmspropTrajectory(rows0, 0.99, 1e-8)
    ids = _id_map(rng, N)
    ids[0, 0, 0, :4] = torch.tensor([299., 300., 349., 350.], device="cuda")           # both sides of both boundaries
    w = torch.from_numpy(rng.standard_normal((2, 8, 32, 24)).astype(f32)).cuda()
    (joint(ids) * w).sum().backward()
    assert all(p.texture_.grad is None for p in parts), "sparse mode writes no dense gradient"
    pids, pg = joint.take_pending()
    assert joint.take_pending() is None
    ids_h, g_h = _host(pids).astype(np.int64), _host(pg)
    # activation none: the queued rows are the incoming gradient, pixel by pixel
    assert np.array_equal(ids_h, _host(ids[:, 0]).astype(np.int64).reshape(-1))
    assert np.array_equal(_bits(g_h), _bits(_host(w.permute(0, 2, 3, 1).contiguous()).reshape(-1, 8)))
    joint._pending.append((pids.clone(), pg.clone()))                                  # re-queue what the trajectory was fed
    opt.step()
    lo, hi = (0, 0) if frozen is None else (joint.id_bases[frozen], joint.id_bases[frozen] + PART_SIZES[frozen])
    live = ~((ids_h >= lo) & (ids_h < hi))
    touched = traj.apply(ids_h[live], g_h[live], lr)
    got = _concat(parts)
    q = _report(f"joint step (frozen {frozen}) rows, {int(touched.sum())} touched", np.abs(got - traj.p), traj.e_p)
    assert q <= 1.0, f"{q:.3f} x the bound"
    assert np.array_equal(_bits(got[~touched]), _bits(rows0[~touched])), "untouched rows changed"
    assert bool((got[touched] != rows0[touched]).any(axis=1).all()), "a touched row did not move"
    for s, p in enumerate(parts):                                                      # every trainable part's step advances
        assert (id(p) in opt.state) == (s != frozen) and (s == frozen or opt.state[id(p)]['step'] == 1)
    if frozen is not None:
        after = parts[frozen].state_dict()
        assert all(torch.equal(after[k].view(torch.int32), frozen_ckpt[k].view(torch.int32)) for k in frozen_ckpt)
        return
    # ---- the same part alone in the next iteration: one state, the trajectory goes on
    sq_before = opt.state[id(parts[0])]['sq']
    solo = SparseDescriptorRMSprop([joint, parts[0]], lr=lr)
    solo.state = opt.state
    ids2 = _id_map(rng, PART_SIZES[0], (1, 1, 16, 8))
    w2 = torch.from_numpy(rng.standard_normal((1, 8, 16, 8)).astype(f32)).cuda()
    (parts[0](ids2) * w2).sum().backward()
    solo.step()
    assert solo.state[id(parts[0])]['sq'] is sq_before and solo.state[id(parts[0])]['step'] == 2
    assert solo.state[id(parts[1])]['step'] == 1 and solo.state[id(parts[2])]['step'] == 1
    traj.apply(_host(ids2[:, 0]).astype(np.int64).reshape(-1), _host(w2.permute(0, 2, 3, 1).contiguous()).reshape(-1, 8), lr)
    q = _report("part 0 alone after the joint step, rows", np.abs(_concat(parts) - traj.p), traj.e_p)
    assert q <= 1.0, f"{q:.3f} x the bound"
    sd = solo.state_dict()
    assert len(sd['state']) == 3 and [s['step'] for s in sd['state']] == [2, 1, 1]      # the parts once each
    solo.load_state_dict(sd)


def test_joint_texture_dense_mode_gives_every_part_its_gradient(hip):
    rng = np.random.default_rng(53)
    Cc = 8
    parts = []
    for n, act in zip(PART_SIZES, ("none", "sigmoid", "tanh")):
        p = PointTexture(Cc, n, activation=act)
        p.texture_.data.copy_(torch.from_numpy(rng.standard_normal((1, Cc, n)).astype(f32)))
        parts.append(p)
    parts[1].texture_.requires_grad_(False)
    joint = JointTexture(parts).cuda()
    N = sum(PART_SIZES)
    ids = _id_map(rng, N)
    w = torch.from_numpy(rng.standard_normal((2, Cc, 32, 24)).astype(f32)).cuda()
    y = joint(ids)
    (y * w).sum().backward()
    assert parts[1].texture_.grad is None and not joint._pending
    ids_i = ids[:, 0].to(torch.int32).contiguous()
    y_l, d_l = [y.detach().permute(0, 2, 3, 1).contiguous()], [w.permute(0, 2, 3, 1).contiguous()]
    drows = [torch.zeros((n, Cc), device="cuda") if s != 1 else None for s, n in enumerate(PART_SIZES)]
    gather_tables_backward(joint.tables(rows=False), [ids_i], d_l, y_l, drows=drows)
    flat_ids = _host(ids_i).reshape(-1)
    ref, hits, mass = jm.adjoint_dense(flat_ids, _host(d_l[0]).reshape(-1, Cc), _host(y_l[0]).reshape(-1, Cc), joint.id_bases, PART_SIZES,
                                       [p.activation for p in parts], frozen=(1,))
    for s in (0, 2):
        grad = _host(parts[s].texture_.grad)
        assert grad.shape == (1, Cc, PART_SIZES[s])
        got, direct = grad[0].T, _host(drows[s])
        k = hits[s][:, None]
        for what, x in (("module", got), ("kernel", direct)):
            q = _report(f"dense gradient of part {s} ({what})", np.abs(x - ref[s]), (k + 4) * U * mass[s])
            assert q <= 1.0, f"part {s} ({what}): {q:.3f} x the bound"
        few = hits[s] <= 2                 # a sum of at most two terms does not depend on the order of the atomics
        assert few.any() and np.array_equal(_bits(got[few]), _bits(direct[few]))


# ------------------------------------------------------------------------------------------ NetAndTexture end to end
KEYS = "uv_1d_p1,uv_1d_p1_ds1,uv_1d_p1_ds2,uv_1d_p1_ds3,uv_1d_p1_ds4".split(',')
H, W = 32, 48


def _model(textures, seed=8):
    from read_amd.net_texture import NetAndTexture
    from read_amd.unet import UNet, weight_spec
    net = UNet()
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic.make_unet_state(weight_spec(), seed).items()})
    return NetAndTexture(net, textures)


def _inputs(maps, tid, B):
    d = {'id': [tid] * B}
    d.update(dict(zip(KEYS, maps)))
    return d


def test_net_and_texture_with_a_joint(hip):
    rng = np.random.default_rng(54)
    sizes, B = (400, 150), 2
    N = sum(sizes)
    (a, b), joint = _parts(rng, sizes=sizes)
    whole = PointTexture(8, N)
    whole.texture_.data.copy_(torch.from_numpy(_concat([a, b]).T.copy())[None])
    maps = [torch.from_numpy(rng.integers(0, N, (B, 1, H >> l, W >> l)).astype(f32)).cuda() for l in range(5)]
    for m in maps:
        m[:, :, 0, 0] = 0.0
    # ---- eval: the model with the joint is the model with the concatenated PointTexture, bit for bit (one net serves both: the
    # textures dict holds the parts under their own ids, the joint, and the concatenation)
    model = _model({0: a, 1: b, 'ab': joint, 'whole': whole})
    model.load_textures(['ab', 'whole'])
    model.cuda().eval()
    with torch.no_grad():
        out = model(_inputs(maps, 'ab', B))
        ref = model(_inputs(maps, 'whole', B))
        mixed = model(dict(_inputs(maps, 'ab', B), id=['whole', 'ab']))
    assert out.shape == (B, 3, H, W) and torch.equal(out.view(torch.int32), ref.view(torch.int32))
    assert torch.equal(mixed.view(torch.int32), ref.view(torch.int32))
    model.check_ids()
    # ---- one training step: Huber, Adam on the net, the sparse optimizer on the joint; part b frozen
    b.texture_.requires_grad_(False)
    ckpt_b = {k: v.clone() for k, v in b.state_dict().items()}
    rows0 = _concat([a, b])
    adam = torch.optim.Adam(model.net.parameters(), lr=1e-3)
    opt = SparseDescriptorRMSprop([joint], lr=0.1)
    target = torch.rand(B, 3, H, W, device="cuda")
    loss = huber_loss(model(_inputs(maps, 'ab', B)), target) * 1e4
    loss.backward()
    pids, pg = joint.take_pending()
    joint._pending.append((pids, pg))
    adam.step()
    opt.step()
    assert np.isfinite(float(loss.detach()))
    got = _concat([a, b])
    ids_h, g_h = _host(pids), _host(pg)
    named = np.zeros(N, bool)
    named[ids_h] = True
    nonzero = np.zeros(N, bool)
    gsum = np.zeros((N, 8))
    np.add.at(gsum, ids_h, g_h.astype(np.float64))
    nonzero[(gsum != 0).any(axis=1)] = True
    part_a = np.arange(N) < sizes[0]
    moved = (got != rows0).any(axis=1)
    assert not moved[~(named & part_a)].any(), "a row that was not touched, or a row of the frozen part, moved"
    assert moved[named & part_a & nonzero].all() and (named & part_a & nonzero).sum() > 50, "a touched row with a gradient did not move"
    after = b.state_dict()
    assert all(torch.equal(after[k].view(torch.int32), ckpt_b[k].view(torch.int32)) for k in ckpt_b), "the frozen part's checkpoint changed"
    assert opt.state[id(a)]['step'] == 1 and id(b) not in opt.state
    # ---- the per-item branch in training: item 0 through the joint, item 1 through part a on its own
    model.load_textures(['ab', 0])
    maps2 = [torch.cat([m[:1], m[1:] % sizes[0]]) for m in maps]
    model(dict(_inputs(maps2, 'ab', B), id=['ab', 0])).sum().backward()
    (jid, _), (aid, _) = joint.take_pending(), a.take_pending()
    assert jid.numel() == aid.numel() == sum((H >> l) * (W >> l) for l in range(4))     # the UNet reads four of the five scales
    model.check_ids()


def test_stitched_scene_feeds_the_joint_training_step(hip):
    """Shape and plumbing: MultiscaleRender on a two-part StitchedScene -> merged-id pyramid -> NetAndTexture with the scene's joint."""
    from read_amd.render import MultiscaleRender, Scene, StitchedScene
    counts = (3000, 2000)
    clouds = [synthetic.make_cloud(n, seed=s + 1) for s, n in enumerate(counts)]
    view = np.eye(4, dtype=np.float32)
    view[1, 3], view[2, 3] = 4.0, 60.0
    st = StitchedScene([Scene(c) for c in clouds])
    st.set_proj_matrix(synthetic.make_proj(W, H, f=60.0 * W / 64))
    st.set_camera_view(view)
    fmt = ", ".join(KEYS)
    maps = MultiscaleRender(st, fmt, (W, H), out_buffer_location='torch').render()
    parts = [PointTexture(8, n, init_method='rand') for n in counts]
    joint = st.joint_texture(parts)
    joint.sparse_training = True
    parts[0].texture_.requires_grad_(False)
    model = _model({'drive': joint})
    model.load_textures(['drive'])
    model.cuda().eval()
    inputs = {'id': ['drive']}
    inputs.update({k: maps[k].permute(2, 0, 1)[None, :1].contiguous() for k in KEYS})
    assert int(inputs[KEYS[0]].max()) >= counts[0], "the frame shows nothing of part 1"
    adam = torch.optim.Adam(model.net.parameters(), lr=1e-3)
    opt = SparseDescriptorRMSprop([joint], lr=0.1)
    before = [p.rows().clone() for p in parts]
    loss = huber_loss(model(inputs), torch.rand(1, 3, H, W, device="cuda"))
    loss.backward()
    adam.step()
    opt.step()
    model.check_ids()
    assert torch.equal(parts[0].rows(), before[0]) and not torch.equal(parts[1].rows(), before[1])


def test_refusals_on_the_device(hip):
    from read_amd import ddp
    rng = np.random.default_rng(55)
    (a, b), joint = _parts(rng, sizes=(40, 20))
    with pytest.raises(NotImplementedError, match="JointTexture under DataParallelStep"):
        ddp.DataParallelStep(torch.nn.Linear(2, 2).cuda(), [a, joint])
    model = _model({0: a, 1: b, 'ab': joint})
    model.ss = 2
    model.load_textures([0, 1, 'ab'])
    model.cuda().eval()
    maps = [torch.zeros(1, 1, 2 * (H >> l), 2 * (W >> l), device="cuda") for l in range(5)]
    with torch.no_grad(), pytest.raises(NotImplementedError, match="supersampling 2 with a JointTexture"):
        model(_inputs(maps, 'ab', 1))
    # the fast path draws a stitched scene from one PointTexture per part: the joint is no part's texture
    from read_amd.ogl import OGL
    from read_amd.render import Scene, StitchedScene
    model.ss = 1
    st = StitchedScene([Scene(synthetic.make_cloud(n, seed=s + 1)) for s, n in enumerate((300, 200))])
    st.set_proj_matrix(synthetic.make_proj(W, H, f=45.0))
    st.set_camera_view(np.eye(4, dtype=np.float32))
    with pytest.raises(NotImplementedError, match="JointTexture as the texture of part 0"):
        OGL.from_model(st, model, ", ".join(KEYS), (W, H), texture_ids=['ab', 1]).infer()
    model.unload_textures()                                       # the parts are on the CPU again: nobody loaded the joint
    with pytest.raises((NotImplementedError, ValueError), match="not loaded on the GPU"):
        joint(torch.zeros(1, 1, 4, 4))
