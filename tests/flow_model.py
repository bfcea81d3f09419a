"""Frame flow: the NumPy model of the contract (include/read_hip.h, read_flow_frame).  The kernel
(read_amd/csrc/flow.hip) and Python (read_amd/flow.py) are held to it bit for bit.

Two states of one rasteriser: A, the frame the labels live on, and B, the frame they point into.  A state is a camera M0, for every
position i of A's instance list a pose and a visible flag (M_i = object_matrix(M0, P_i)), and the level-0 idx / depth frame drawn
with them.  Cloud, labels, foreign objects, the object each instance draws and W, H are common.

Per pixel p of A: empty (idx == 0 and depth bits == 0) -> EMPTY.  Otherwise id -> (object k, point) as tests/annotate_model.py does.
The drawer: for k == 0 the static scene, matrices M0_a / M0_b, and M0_a must reproduce pixel p and depth_a[p]'s bits; for k >= 1 the
first instance in list order that is visible in A, draws k and under M_i^a projects the point to p with depth_a[p]'s bits.  No
drawer: UNMATCHED, unmatched += 1.  Under A's drawer matrix the point has continuous pixel coordinates (u_a, v_a), under B's
(u_b, v_b), depth d_b and pixel q.  The drawer hidden in B: HIDDEN.  q >= 0: VISIBLE where idx_b[q] == id and depth_b[q]'s bits are
d_b's, else OCCLUDED.  q == -1 with nz in [-1, 1] and nx, ny finite: OFF_IMAGE; any other q == -1: CLIPPED.  flow = (u_b - u_a,
v_b - v_a) and depth_next = d_b for VISIBLE, OCCLUDED and OFF_IMAGE, +0 otherwise.

The projection is computed here, in float32 operation by operation (no contraction, sums left to right, IEEE division), because
oracle.project_points returns no sub-pixel coordinates; tests/test_flow_cpu.py pins it to the oracle's pixel and depth bits."""
import numpy as np

from read_amd.raster import object_matrix
from tests import annotate_model as am

EMPTY, VISIBLE, OCCLUDED, OFF_IMAGE, CLIPPED, HIDDEN, UNMATCHED = range(7)
STATES = 8
STATS = 4
PX, N_VISIBLE, N_OCCLUDED, N_OUTSIDE = range(STATS)
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def project(xyz, M, W, H):
    """xyz (n,3); M (16,), (4,4) or one matrix per point (n,16) -> dict of (n,) arrays: pix (int32, -1 = rejected), depth, u, v, nx, ny,
    nz (float32).  The operations of csrc/project.h's project_one / ndc_pixel, one float32 rounding each."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    M = np.asarray(M, np.float32)
    M = np.broadcast_to(M.reshape(1, 16), (xyz.shape[0], 16)) if M.size == 16 else M.reshape(-1, 16)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    one = F(1.0)
    with np.errstate(all='ignore'):
        c = [M[:, 4 * r] * x + M[:, 4 * r + 1] * y + M[:, 4 * r + 2] * z + M[:, 4 * r + 3] * one for r in range(4)]
        nx, ny, nz = c[0] / c[3], c[1] / c[3], c[2] / c[3]
        inside = (nx >= -1) & (nx <= 1) & (ny >= -1) & (ny <= 1) & (nz >= -1) & (nz <= 1)
        u = (F(W) * (nx + one)) * F(0.5)
        v = (F(H) * (one - ny)) * F(0.5)
        depth = (nz + one) * F(0.5)
        xx = np.where(inside, u, 0).astype(np.int32)             # the C cast truncates; inside, 0 <= u <= W
        yy = np.where(inside, v, 0).astype(np.int32)
    ok = inside & (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
    pix = np.where(ok, yy * W + xx, -1).astype(np.int32)
    assert all(a.dtype == np.float32 for a in (u, v, depth, nx, ny, nz))
    return dict(pix=pix, depth=depth, u=u, v=v, nx=nx, ny=ny, nz=nz)


def resolve(xyz, labels, foreign, idx, dbits):
    """id -> (filled, k_of, pt) per pixel: k_of = -1 where the pixel is empty or no range holds its id."""
    N = xyz.shape[0]
    lab = np.zeros(N, np.int64) if labels is None else np.asarray(labels).astype(np.int64)
    K_own = int(lab.max()) if lab.size else 0
    filled = ~((idx == 0) & (dbits == 0))
    k_of = np.full(idx.size, -1, np.int64)
    pt = np.zeros((idx.size, 3), np.float32)
    own = filled & (idx >= 0) & (idx < N)
    k_of[own] = lab[idx[own]]
    pt[own] = xyz[idx[own]]
    base = N
    for f, fx in enumerate(foreign):
        fx = np.asarray(fx, np.float32)
        sel = filled & (idx >= base) & (idx < base + fx.shape[0])
        k_of[sel] = K_own + 1 + f
        pt[sel] = fx[idx[sel] - base]
        base += fx.shape[0]
    return filled, k_of, pt


def flow(xyz, labels, foreign, inst_a, inst_b, M0_a, M0_b, W, H, idx_a, depth_a, idx_b, depth_b):
    """inst_a = [(k, P, visible)] of state A; inst_b = the same list positions in state B (k unchanged; an instance B no longer has:
    visible False).  -> dict: flow (H,W,2) float32, depth_next (H,W) float32, state (H,W) int32, counts (8,) int32, stats (I,4)
    int32, unmatched int, won (H,W) int32 = the list position of the drawing instance (-1: the static scene or none)."""
    xyz = np.asarray(xyz, np.float32)
    M0_a, M0_b = np.asarray(M0_a, np.float32).reshape(16), np.asarray(M0_b, np.float32).reshape(16)
    I = len(inst_a)
    assert len(inst_b) == I and all(a[0] == b[0] for a, b in zip(inst_a, inst_b))
    P_ = W * H
    idx_a = np.asarray(idx_a, np.int32).reshape(-1)
    idx_b = np.asarray(idx_b, np.int32).reshape(-1)
    bits_a, bits_b = _bits(depth_a).reshape(-1), _bits(depth_b).reshape(-1)
    assert idx_a.size == idx_b.size == bits_a.size == bits_b.size == P_
    filled, k_of, pt = resolve(xyz, labels, foreign, idx_a, bits_a)
    pixel = np.arange(P_)
    Ma = [object_matrix(M0_a, P).reshape(16) for _, P, _ in inst_a]
    Mb = [object_matrix(M0_b, P).reshape(16) for _, P, _ in inst_b]
    # the drawer: the annotation's walk (list order, the first match stays); the static scene checks itself
    won = np.full(P_, -1, np.int32)
    for i in range(I - 1, -1, -1):
        k, _, visible = inst_a[i]
        if not visible:
            continue
        cand = np.flatnonzero(filled & (k_of == k))
        if cand.size == 0:
            continue
        pr = project(pt[cand], Ma[i], W, H)
        hit = (pr['pix'] == cand) & (_bits(pr['depth']) == bits_a[cand])
        won[cand[hit]] = i
    static = filled & (k_of == 0)
    pa0 = project(pt, M0_a, W, H)
    drawn = (static & (pa0['pix'] == pixel) & (_bits(pa0['depth']) == bits_a)) | (won >= 0)
    # one matrix per pixel, A's and B's
    Mpa = np.broadcast_to(M0_a, (P_, 16)).copy()
    Mpb = np.broadcast_to(M0_b, (P_, 16)).copy()
    hidden = np.zeros(P_, bool)
    for i in range(I):
        sel = won == i
        Mpa[sel], Mpb[sel] = Ma[i], Mb[i]
        hidden[sel] = not inst_b[i][2]
    pa, pb = project(pt, Mpa, W, H), project(pt, Mpb, W, H)
    q = pb['pix']
    qc = np.clip(q, 0, P_ - 1)
    same = (q >= 0) & (idx_b[qc] == idx_a) & (bits_b[qc] == _bits(pb['depth']))
    beside = (q < 0) & (pb['nz'] >= -1) & (pb['nz'] <= 1) & np.isfinite(pb['nx']) & np.isfinite(pb['ny'])
    state = np.full(P_, EMPTY, np.int32)
    state[filled] = UNMATCHED
    live = drawn & ~hidden
    state[drawn & hidden] = HIDDEN
    state[live & (q >= 0) & same] = VISIBLE
    state[live & (q >= 0) & ~same] = OCCLUDED
    state[live & (q < 0) & beside] = OFF_IMAGE
    state[live & (q < 0) & ~beside] = CLIPPED
    moves = (state == VISIBLE) | (state == OCCLUDED) | (state == OFF_IMAGE)
    fl = np.zeros((P_, 2), np.float32)
    dn = np.zeros(P_, np.float32)
    with np.errstate(all='ignore'):
        fl[moves, 0] = (pb['u'] - pa['u'])[moves]
        fl[moves, 1] = (pb['v'] - pa['v'])[moves]
    dn[moves] = pb['depth'][moves]
    counts = np.zeros(STATES, np.int32)
    counts[:7] = np.bincount(state, minlength=7)[:7]
    stats = np.zeros((I, STATS), np.int32)
    for i in range(I):
        sel = won == i
        stats[i] = (sel.sum(), (sel & (state == VISIBLE)).sum(), (sel & (state == OCCLUDED)).sum(),
                    (sel & ((state == OFF_IMAGE) | (state == CLIPPED))).sum())
    return dict(flow=fl.reshape(H, W, 2), depth_next=dn.reshape(H, W), state=state.reshape(H, W), counts=counts, stats=stats,
                unmatched=int(counts[UNMATCHED]), won=won.reshape(H, W))


def render(xyz, labels, foreign, inst, M0, W, H):
    """The level-0 frame of a state (tests/annotate_model.render): -> (idx (H,W) int32, depth (H,W) float32)."""
    return am.render(xyz, labels, foreign, inst, M0, W, H)
