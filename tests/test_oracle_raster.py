"""CPU: the rasteriser oracle against (a) the committed golden vectors, which are the output of the
reference's own DepthProject source run serially (tests/golden/make_golden.py), (b) an independent
NumPy restatement, (c) the live reference-source build when it is present (oracle/_ref)."""
import hashlib
import json
import os

import numpy as np
import pytest

import oracle
from oracle import ref_c
from oracle.raster_np import raster_level_np
from read_amd import camera, synthetic


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_golden_config0(golden_dir):
    g = np.load(os.path.join(golden_dir, "raster_256_100k.npz"))
    xyz = synthetic.make_cloud(int(g["N"]), int(g["seed"]))
    for b in range(g["M"].shape[0]):
        idx, dep = oracle.raster_multiscale(xyz, g["M"][b], 256, 256, 5)
        for l in range(5):
            assert np.array_equal(idx[l], g[f"index{l}"][b])
            assert np.array_equal(_bits(dep[l]), _bits(g[f"depth{l}"][b]))


def test_golden_matrix_is_reproducible(golden_dir):
    """total_m itself is an input; the recipe must regenerate the stored one."""
    g = np.load(os.path.join(golden_dir, "raster_256_100k.npz"))
    Ms = camera.total_matrix(synthetic.make_proj(256, 256, f=256.0),
                             np.stack([np.eye(4, dtype=np.float32), synthetic.sweep_pose(40)]))
    assert np.array_equal(Ms, g["M"])


@pytest.mark.parametrize("W,H,N,f", [(256, 256, 100_000, 256.0), (1216, 352, 400_000, 720.0), (77, 33, 9_000, 60.0)])
def test_c_equals_numpy_and_threads(W, H, N, f):
    xyz = synthetic.make_cloud(N, seed=11)
    M = camera.total_matrix(synthetic.make_proj(W, H, f=f), synthetic.sweep_pose(7))[0]
    ci, cd = oracle.raster_level(xyz, M, W, H)
    ni, nd = raster_level_np(xyz, M, W, H)
    assert np.array_equal(ci, ni) and np.array_equal(_bits(cd), _bits(nd))
    ti, td = oracle.raster_level(xyz, M, W, H, threads=4)
    assert np.array_equal(ci, ti) and np.array_equal(_bits(cd), _bits(td))


def test_oracle_equals_reference_source_run_serially(golden_dir):
    """The pin: the reference's own kernel text, compiled for the CPU, one emulated thread per point.  Its maps are stored as
    SHA-256 digests in tests/golden/raster_ref_serial.json (tests/golden/make_ref_raster_golden.py): the comparison is
    bit-exact, so equal digests are equal maps.  Where oracle/_ref is built, the live build must still match the digests."""
    def sha256(a):
        return hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest()

    with open(os.path.join(golden_dir, "raster_ref_serial.json")) as fh:
        g = json.load(fh)
    for case in g["cases"]:
        W, H, N = case["W"], case["H"], case["N"]
        xyz = synthetic.make_cloud(N, seed=g["seed"])
        Ms = camera.total_matrix(synthetic.make_proj(W, H, f=case["f"]), np.stack([synthetic.sweep_pose(k) for k in g["poses"]]))
        if ref_c.available():
            li, ld = ref_c.pcpr_ref_forward(xyz, Ms, W, H)
            for b, want in enumerate(case["maps"]):
                assert (sha256(li[b]), sha256(ld[b])) == (want["index_sha256"], want["depth_sha256"]), (W, H, b)
        for b, want in enumerate(case["maps"]):
            oi, od = oracle.raster_level(xyz, Ms[b], W, H)
            assert not (od[oi > 0] == 0).any()                      # no d == 0 points (documented departure)
            assert int((oi > 0).sum()) == want["covered"], (W, H, b)
            assert sha256(oracle.index_to_float(oi)) == want["index_sha256"], (W, H, b)
            assert sha256(od) == want["depth_sha256"], (W, H, b)


def test_pyramid_identity():
    """level l == 2x2 key-min of level l-1 when W,H are multiples of 16."""
    W, H = 304, 176
    xyz = synthetic.make_cloud(250_000, seed=5)
    M = camera.total_matrix(synthetic.make_proj(W, H, f=200.0), np.eye(4, dtype=np.float32))[0]
    idx, dep = oracle.raster_multiscale(xyz, M, W, H, 5)

    def keys(i, d):
        k = (_bits(d).astype(np.uint64) << np.uint64(32)) | i.astype(np.uint32).astype(np.uint64)
        k[(i == 0) & (d == 0)] = np.uint64(0xFFFFFFFFFFFFFFFF)
        return k
    k = keys(idx[0], dep[0])
    for l in range(1, 5):
        h, w = k.shape
        k = k.reshape(h // 2, 2, w // 2, 2).min(axis=(1, 3))
        assert np.array_equal(k, keys(idx[l], dep[l]))


def test_edge_cases():
    W, H = 64, 32
    M = camera.total_matrix(synthetic.make_proj(W, H, f=64.0), np.eye(4, dtype=np.float32))[0]
    # empty cloud
    i, d = oracle.raster_level(np.zeros((0, 3), np.float32), M, W, H)
    assert not i.any() and not d.any()
    # behind the camera / outside the frustum: nothing lands
    pts = np.array([[0, 0, 5], [1000, 0, -1], [0, 0, -0.01], [0, 0, -5000]], np.float32)
    i, d = oracle.raster_level(pts, M, W, H)
    assert not i.any() and not d.any()
    # exact ties -> smallest index; nearer point wins regardless of order
    pts = np.array([[0.3, 0.2, -9], [0, 0, -10], [0, 0, -10], [0, 0, -4], [0, 0, -10]], np.float32)
    i, d = oracle.raster_level(pts, M, W, H)
    assert i[H // 2, W // 2] == 3
    i, d = oracle.raster_level(pts[[0, 1, 2, 4]], M, W, H)
    assert i[H // 2, W // 2] == 1
    # w == 0 (NaN/inf NDC) is rejected, not UB
    i, d = oracle.raster_level(np.array([[0, 0, 0]], np.float32), M, W, H)
    assert not i.any()


def test_float_index_rounding():
    idx = np.array([0, 1, (1 << 24) - 1, (1 << 24) + 1, 29_999_999], np.int32)
    assert np.array_equal(oracle.index_to_float(idx), idx.astype(np.float32))
    assert oracle.index_to_float(idx)[3] == float(1 << 24)           # ids >= 2^24 round (point_render.cu:158)


def test_gather_and_backward_oracle():
    rng = np.random.default_rng(0)
    tex = rng.random((8, 500), dtype=np.float32)
    idx = rng.integers(0, 500, (12, 20)).astype(np.int32)
    out = oracle.gather_chw(tex, idx)
    assert np.array_equal(out, tex[:, idx])
    g = rng.standard_normal((8, 12, 20)).astype(np.float32)
    gt = oracle.gather_backward_chw(g, idx, 500)
    ref = np.zeros((8, 500), np.float32)
    for c in range(8):
        np.add.at(ref[c], idx.reshape(-1), g[c].reshape(-1))
    np.testing.assert_allclose(gt, ref, rtol=1e-6, atol=1e-6)


def test_gl_coverage_rule_equals_the_opengl_specification_text():
    """Pin of the GL twin's pixel coverage (round-2 verdict: "the pixel-coverage rule for sizes > 1 is the
    builder's own convention"): oracle/raster.c's floor(u +- (s - 1) / 2) rule against oracle/raster_gl_spec.py, an
    independent restatement written from the OpenGL 4.6 core specification's text (13.7 clipping of points by their centre,
    14.4.1 "pixel whose center lies inside a square ... with side length equal to the current point size", 13.8.1 viewport,
    17.3.6 GL_LESS) — odd, EVEN and fractional sizes, "ps" splats that actually exceed one pixel, per-point size arrays,
    discard and perturbation.  Pixels whose centre lies within 1e-4 px of a square's edge are excluded (the spec does not say
    which side owns the edge); everything else must agree bit for bit."""
    from oracle.raster_gl_spec import raster_level_gl_spec
    N, W, H = 2500, 96, 64
    xyz = synthetic.make_cloud(N, seed=5)
    M = camera.total_matrix(synthetic.make_proj(W, H, f=60.0), synthetic.sweep_pose(7))[0]
    rng = np.random.default_rng(1)
    cases = [dict(point_size=1), dict(point_size=2), dict(point_size=3), dict(point_size=4), dict(point_size=7),
             dict(point_size=300, relative=True), dict(point_size=777, relative=True, min_point_size=2.5),
             dict(point_sizes=rng.uniform(0.5, 6.0, N).astype(np.float32)),
             dict(point_sizes=rng.uniform(1, 400, N).astype(np.float32), relative=True),
             dict(point_size=5, discard=rng.random(N) < 0.3, perturb=(0.5 * (rng.random((N, 2)) - 0.5)).astype(np.float32))]
    for kw in cases:
        a_i, a_d = oracle.raster_level_gl(xyz, M, W, H, **kw)
        b_i, b_d, amb = raster_level_gl_spec(xyz, M, W, H, **kw)
        ok = ~amb
        assert amb.mean() < 0.02, kw
        assert ((a_i != 0) | (a_d != 0)).sum() > 1000, kw                    # the case draws something
        assert np.array_equal(a_i[ok], b_i[ok]), kw
        assert np.array_equal(_bits(a_d)[ok], _bits(b_d)[ok]), kw
    # sizes > 1 really cover more than the 1-px rule (the test above is not vacuous), and p1 reduces to the pinned rasteriser
    i1, d1 = oracle.raster_level_gl(xyz, M, W, H, point_size=1)
    i0, d0 = oracle.raster_level(xyz, M, W, H)
    assert np.array_equal(i1, i0) and np.array_equal(_bits(d1), _bits(d0))
    i2, _ = oracle.raster_level_gl(xyz, M, W, H, point_size=2)
    assert (i2 != 0).sum() > 1.5 * (i1 != 0).sum()
