"""Parity of the HIP UNet / full frame with the reference: the committed golden vectors were
produced by the reference's own modules (tests/golden/make_golden.py); larger sizes are checked
against the oracle restatement.

Stated tolerance (fp32 MFMA vs fp32 oneDNN, 40+ gated-conv layers deep; measured 2e-7 / 148 dB): max |diff| <= 5e-6,
PSNR >= 120 dB, and — because the random-weight RGB output has a per-channel spread of only ~0.01-0.03 — the error
RELATIVE to the signal: rms(diff) <= 1e-4 * std(ref) (the north-star budget is 0.5 dB of PSNR)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import oracle
from oracle import unet_torch
from read_amd import camera, synthetic
from read_amd.frame import FrameRenderer
from read_amd.unet import UNet, layer_table, weight_spec
from tests.unet_spec import UNET_SPEC

pytestmark = pytest.mark.gpu

MAX_ABS = 5e-6
MIN_PSNR = 120.0
MAX_REL_RMS = 1e-4          # rms(got - ref) / std(ref)
TAP_REL = 2e-5              # intermediates: |diff| <= TAP_REL * max(1, |ref|) elementwise


def _check_rgb(got, ref, what):
    diff = (got.double() - ref.double())
    err, p = float(diff.abs().max()), unet_torch.psnr(got, ref)
    rel = float(diff.pow(2).mean().sqrt() / ref.double().std())
    print("%s: max|diff| %.3e  PSNR %.1f dB  rms/std %.2e" % (what, err, p, rel))
    assert err <= MAX_ABS, f"{what}: max|diff| {err:.3e}"
    assert p >= MIN_PSNR, f"{what}: PSNR {p:.1f} dB"
    assert rel <= MAX_REL_RMS, f"{what}: relative rms {rel:.3e}"


def test_layer_table_matches_independent_spec(hip):
    assert weight_spec() == UNET_SPEC
    assert len(layer_table()) == 101


def _golden_frame(golden_dir):
    g = np.load(os.path.join(golden_dir, "frame_64x48.npz"))
    W, H, N, seed = int(g["W"]), int(g["H"]), int(g["N"]), int(g["seed"])
    xyz = synthetic.make_cloud(N, seed)
    desc = synthetic.make_descriptors(N, 8, seed)
    state = synthetic.make_unet_state(UNET_SPEC, seed)
    return g, W, H, xyz, desc, state


def test_golden_frame_end_to_end(golden_dir, hip):
    """Same camera, cloud, descriptors and weights as the reference run that produced the golden."""
    g, W, H, xyz, desc, state = _golden_frame(golden_dir)
    fr = FrameRenderer(xyz, desc, state, W, H)
    rgba = fr.render_total(g["M"])
    torch.cuda.synchronize()
    for l in range(5):
        assert np.array_equal(fr.idx[l][0].cpu().numpy(), g[f"idx{l}"]), f"index level {l}"
        assert np.array_equal(fr.depth[l][0].cpu().numpy().view(np.uint32), g[f"depth{l}"].view(np.uint32))
    got = rgba[:, :, :3].permute(2, 0, 1).cpu()
    ref = torch.from_numpy(g["rgb"])
    assert bool((rgba[:, :, 3] == 1).all())
    _check_rgb(got, ref, "golden frame")
    # intermediates (sub-sampled in the golden file to keep it small)
    taps = {"res1": ("Encoder.0.y2", (slice(None, None, 4), slice(None, None, 4))),
            "zb": ("Encoder.3.y2", (slice(None), slice(None))), "z8": ("SCM0.out", (slice(None), slice(None))),
            "aff2": ("aff2.out", (slice(None, None, 2), slice(None, None, 2)))}
    for key, (name, sl) in taps.items():
        t = fr.unet.debug_tensor(name).permute(2, 0, 1).cpu()[(slice(None),) + sl]
        r = torch.from_numpy(g[key])
        bad = float(((t - r).abs() / r.abs().clamp(min=1.0)).max())
        assert bad <= TAP_REL, f"{key}: relative error {bad:.3e}"


def test_unet_module_256_vs_oracle(hip):
    """BASELINE configs[0] geometry (256x256) through the nn.Module mirror, against the oracle."""
    torch.manual_seed(0)
    state = synthetic.make_unet_state(UNET_SPEC, 5)
    net = UNet()
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    net.cuda().eval()
    xs = [torch.rand(1, 8, 256 >> l, 256 >> l) for l in range(5)]
    with torch.no_grad():
        got = net(*[x.cuda() for x in xs]).cpu()
        ref = unet_torch.unet_forward(state, *xs[:4])
    assert got.shape == (1, 3, 256, 256)
    _check_rgb(got, ref, "256x256")
    # state-dict names are the reference's: 909 tensors
    assert len(net.state_dict()) == 909


def test_full_frame_256_100k_vs_oracle(hip):
    """configs[0]: 100 k points, 256x256, the whole path against the whole oracle."""
    W = H = 256
    N = 100_000
    xyz, desc = synthetic.make_cloud(N), synthetic.make_descriptors(N)
    state = synthetic.make_unet_state(UNET_SPEC)
    proj = synthetic.make_proj(W, H, f=256.0)
    fr = FrameRenderer(xyz, desc, state, W, H, proj_matrix=proj)
    pose = synthetic.sweep_pose(12)
    rgba = fr.render(pose).cpu()
    M = camera.total_matrix(proj, pose)[0]
    idx, _ = oracle.raster_multiscale(xyz, M, W, H, 5, threads=8)
    with torch.no_grad():
        ref = unet_torch.net_and_texture_forward(state, desc[None], idx)[0]
    got = rgba[:, :, :3].permute(2, 0, 1)
    _check_rgb(got, ref, "frame 256")


def test_frames_in_flight_equal_sequential_frames(hip):
    """FrameRenderer(frames_in_flight=2): rasteriser + gather on one stream in call order, the UNet of consecutive calls on
    two streams with their own plans and feature buffers.  Every frame of a pose sequence (cell-ordered cloud, warm-started
    rasteriser) must equal the one-at-a-time renderer bit for bit, also when the output buffers are reused two calls later."""
    W, H = 256, 128
    N = (1 << 20) + 4321
    xyz, desc = synthetic.make_cloud(N, 5), synthetic.make_descriptors(N)
    state = synthetic.make_unet_state(UNET_SPEC, 2)
    proj = synthetic.make_proj(W, H, f=200.0)
    seq = FrameRenderer(xyz, desc, state, W, H, proj_matrix=proj)
    pipe = FrameRenderer(xyz, desc, state, W, H, proj_matrix=proj, frames_in_flight=2)
    assert pipe.raster.cells is not None
    poses = [synthetic.sweep_pose(k) for k in (0, 1, 2, 3, 40, 41, 2, 0)]
    want = [seq.render(p).clone() for p in poses]
    bufs = [torch.empty((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
    got = []
    for i, p in enumerate(poses):
        out = pipe.render(p, out=bufs[i & 1])
        assert out is bufs[i & 1]
        pipe.frame_done.synchronize()                    # this frame only; the next call overlaps with nothing here ...
        got.append(out.clone())
    for i, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g, w), f"frame {i} differs"
    # ... and back to back, without waiting in between (the pipelined use): compare after one sync at the end
    outs = [pipe.render(p) for p in poses]
    pipe.sync()
    for i, (g, w) in enumerate(zip(outs, want)):
        assert torch.equal(g, w), f"pipelined frame {i} differs"
    # ... and with every frame announcing the next pose (round 5: the rasteriser prepares it inside this frame's last launch) —
    # truthfully, wrongly (the pose after next) and not at all, through both renderers
    totals = [camera.total_matrix(proj, p) for p in poses]
    for fr_ in (seq, pipe):
        for mode in ("true", "wrong", "mixed"):
            outs = []
            for i, t in enumerate(totals):
                nxt = None
                if mode == "true" and i + 1 < len(totals):
                    nxt = totals[i + 1]
                elif mode == "wrong":
                    nxt = totals[(i + 2) % len(totals)]
                elif mode == "mixed" and i % 2 == 0 and i + 1 < len(totals):
                    nxt = totals[i + 1]
                outs.append(fr_.render_total(t, next_total=nxt).clone() if fr_ is seq else fr_.render_total(t, next_total=nxt))
            fr_.sync()
            for i, (g, w) in enumerate(zip(outs, want)):
                assert torch.equal(g, w), f"announced ({mode}) frame {i} differs"


def test_pipelined_frames_through_the_rccl_exchange(hip):
    """The loop bench.py times at N > 1 — sweep.run_steps with a FrameExchange — on ONE GPU: a single-rank RCCL group with
    the exchange forced on, FrameRenderer(frames_in_flight=2) writing the exchange's send buffers from its UNet streams and
    handing the completion events to post().  Frames coming out of the all-gather must equal the one-at-a-time frames."""
    import socket
    import torch.distributed as dist
    from read_amd import sweep
    W, H = 256, 128
    N = 200_000
    xyz, desc = synthetic.make_cloud(N, 8), synthetic.make_descriptors(N)
    state = synthetic.make_unet_state(UNET_SPEC, 4)
    proj = synthetic.make_proj(W, H, f=200.0)
    seq = FrameRenderer(xyz, desc, state, W, H, proj_matrix=proj)
    pipe = FrameRenderer(xyz, desc, state, W, H, proj_matrix=proj, frames_in_flight=2)
    n = 7
    total = [camera.total_matrix(proj, synthetic.sweep_pose(k)) for k in range(n)]
    want = [seq.render_total(total[k]).clone() for k in range(n)]
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    def render_into(k, out):
        pipe.render_total(total[k], out=out)
        return pipe.frame_done

    results = {}
    try:
        for mode in ('all', 'root'):                       # all-gather to every rank / gather to rank 0 (the viewer process)
            ex = sweep.FrameExchange((H, W, 4), torch.device("cuda", 0), torch.float32, mode, force=True)
            assert ex.mode == mode and ex.world == 1
            got = []
            for i in range(n):
                sweep.run_steps(render_into, ex, i, 1, n)
                if i > 0:
                    got.append(ex.frames(i - 1)[0].clone())
            got.append(ex.frames(n - 1)[0].clone())
            ex.drain()
            torch.cuda.synchronize()
            results[mode] = got
        assert sweep.gather_objects(True) == [True]        # bench.py's verified_ranks at world size 1 with a live process group
    finally:
        dist.destroy_process_group()
    for mode, got in results.items():
        for i, (g, w) in enumerate(zip(got, want)):
            assert torch.equal(g, w), f"exchange mode {mode!r}: frame {i} differs"


def test_winograd_and_direct_conv_paths_agree(hip):
    """The automatic plan runs the 3x3/s1 C -> C layers through the Winograd F(4x4,3x3) kernel and the 32 -> 3 output layer on
    the vector pipe; with conv_w4 = 0 the same layers take the Winograd F(2x2,3x3) kernel, and with conv_wino = conv_sc = 0 as
    well the direct implicit-GEMM kernel (from the FULL weight blob: the lean one carries only the automatic plan's orders).
    All three must meet the tolerance against the oracle, and they must differ in round-off (the knobs really switch kernels)."""
    from read_amd import _lib
    from read_amd.unet import LAYOUT_FULL
    torch.manual_seed(3)
    state = synthetic.make_unet_state(UNET_SPEC, 9)
    net = UNet()
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    net.cuda().eval()
    net.__dict__['_layout'] = LAYOUT_FULL
    xs = [torch.rand(1, 8, 128 >> l, 192 >> l) for l in range(5)]
    ref = unet_torch.unet_forward(state, *xs[:4])
    outs = {}
    L = _lib.lib()
    try:
        for name, (w4, wino, sc) in (("automatic", (32, 1 << 30, 8)), ("winograd F(2x2)", (0, 1 << 30, 8)), ("direct", (0, 0, 0))):
            _lib.check(L.read_tuning_set(b"conv_w4", w4))
            _lib.check(L.read_tuning_set(b"conv_wino", wino))
            _lib.check(L.read_tuning_set(b"conv_sc", sc))
            with torch.no_grad():
                outs[name] = net(*[x.cuda() for x in xs]).cpu()
            _check_rgb(outs[name], ref, name)
    finally:
        _lib.check(L.read_tuning_set(b"conv_w4", 32))
        _lib.check(L.read_tuning_set(b"conv_wino", 1 << 30))
        _lib.check(L.read_tuning_set(b"conv_sc", 8))
    for a, b in (("automatic", "winograd F(2x2)"), ("winograd F(2x2)", "direct"), ("automatic", "direct")):
        assert not torch.equal(outs[a], outs[b]), (a, b)
        assert float((outs[a] - outs[b]).abs().max()) <= 2 * MAX_ABS


def test_plan_variants_agree_with_the_oracle(hip):
    """The plan's two algebraic rewrites — AFF inputs of coarser levels applied at their own level (unet_aff_split) and the
    bilinear x4 up-sampling folded into the Convs.k launches as a pre-activation addend (unet_up_fold, round 5) — against the plan
    wired exactly as the reference (both off: 480-channel AFF concats, three separate Upsample passes): each meets the tolerance
    against the oracle, the launch labels say which plan ran, and the rewrites really change the arithmetic (round-off differs)."""
    from read_amd import _lib
    torch.manual_seed(5)
    state = synthetic.make_unet_state(UNET_SPEC, 13)
    net = UNet()
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    net.cuda().eval()
    xs = [torch.rand(1, 8, 96 >> l, 160 >> l) for l in range(5)]
    ref = unet_torch.unet_forward(state, *xs[:4])
    L = _lib.lib()
    outs = {}
    try:
        for split, fold in ((1, 1), (1, 0), (0, 1), (0, 0)):
            _lib.check(L.read_tuning_set(b"unet_aff_split", split))
            _lib.check(L.read_tuning_set(b"unet_up_fold", fold))
            net.invalidate()                                          # plans are built under the knobs of their creation
            with torch.no_grad():
                outs[(split, fold)] = net(*[x.cuda() for x in xs]).cpu()
            _check_rgb(outs[(split, fold)], ref, f"plan aff_split={split} up_fold={fold}")
            labels = net.launch_labels()
            assert any(l.startswith("up4(") for l in labels) == (fold == 0), labels
            assert ("Convs.2.r" in labels) == (fold == 1) and ("AFFq3" in labels) == (split == 1)
    finally:
        _lib.check(L.read_tuning_set(b"unet_aff_split", 1))
        _lib.check(L.read_tuning_set(b"unet_up_fold", 0))             # the default (the fold measured level-to-slower, csrc/unet.cpp)
        net.invalidate()
    assert not torch.equal(outs[(1, 1)], outs[(1, 0)]) and not torch.equal(outs[(1, 1)], outs[(0, 1)])
    for k in outs:
        assert float((outs[k] - outs[(0, 0)]).abs().max()) <= 2 * MAX_ABS


def test_headline_frame_1216x352_vs_oracle(hip):
    """The configuration bench.py times: the full UNet at 1216x352 (every persistent-scheduling path of the 32/64/128/256
    channel Winograd launches at 352x1216 / 176x608 / 88x304 / 44x152) on the descriptor pyramids of a rasterised
    frame, against the oracle; plus the kitti6 viewport 1216x368 (H not a multiple of 32)."""
    torch.set_num_threads(min(os.cpu_count() or 1, 32))
    state = synthetic.make_unet_state(UNET_SPEC)
    for (W, H, N, pose) in ((1216, 352, 3_000_000, 7), (1216, 368, 1_500_000, 3)):
        xyz = synthetic.make_cloud(N) if H == 352 else synthetic.make_street_cloud(N)
        desc = synthetic.make_descriptors(N)
        proj = synthetic.make_proj(W, H)
        fr = FrameRenderer(xyz, desc, state, W, H, proj_matrix=proj)
        fr.render(synthetic.sweep_pose(pose - 1))                   # warm start, as in the sweep
        rgba = fr.render(synthetic.sweep_pose(pose)).cpu()
        M = camera.total_matrix(proj, synthetic.sweep_pose(pose))[0]
        idx, dep = oracle.raster_multiscale(xyz, M, W, H, 5, threads=8)
        for l in range(5):
            assert np.array_equal(fr.idx[l][0].cpu().numpy(), idx[l]), f"{W}x{H} index level {l}"
            assert np.array_equal(fr.depth[l][0].cpu().numpy().view(np.uint32), dep[l].view(np.uint32))
        with torch.no_grad():
            ref = unet_torch.net_and_texture_forward(state, desc[None], idx)[0]
        _check_rgb(rgba[:, :, :3].permute(2, 0, 1), ref, f"frame {W}x{H}")
        assert bool((rgba[:, :, 3] == 1).all())
        # ... and the frame above came out of the kernels the documents describe: the 73 C -> C 3x3 / stride-1 launches (and the
        # three 3x3 layers of the SCM chains) of the plan run on the Winograd F(4x4,3x3) kernel, none on a silent fallback
        f = fr.feat
        prof = fr.unet.profile(f[0][0], f[1][0], f[2][0], f[3][0], channels=4)
        kinds = [k for (_, _, _, k) in prof]
        # (round 6: 5 = the F(4x4) kernel with split operands on the f16 matrix cores — every launch of the family but FAM's three,
        #  which multiply two tensors in the loader and run on the DIRECT split-operand kernel, 6)
        assert len(prof) == 105 and kinds.count(5) >= 70 and kinds.count(6) == 3 and kinds.count(4) == 0, (len(prof), kinds.count(5), kinds.count(6), kinds.count(4), kinds.count(2))
        assert sum(1 for (lbl, _, fl, k) in prof if abs(fl - 15.778971648e9 * (H / 352)) < 1e6 and k not in (5, 6)) == 0


def test_split_operand_plan_against_the_fp32_plan(hip):
    """Round 6: the default plan runs 70 of the 73 family launches on the split-operand F(4x4) kernel (f16 matrix cores) and FAM's three on the
    direct split-operand kernel; with
    read_tuning_set("conv_w4h", 0) the same blob (full layout) runs them on the fp32-matrix-core kernel.  Both frames against the
    torch-fp32 oracle at the network guard, and against each other; the lean blob carries the split operand only, so the knob is
    refused there (loudly) and the module repacks the full blob."""
    from read_amd import _lib
    from read_amd.unet import LAYOUT_FULL, LAYOUT_LEAN, UNetEngine, layout_of, pack_state
    H, W = 96, 160
    state = synthetic.make_unet_state(UNET_SPEC, 9)
    torch.manual_seed(3)
    xs = [torch.rand(H >> l, W >> l, 8, device="cuda") for l in range(4)]
    with torch.no_grad():
        ref = unet_torch.unet_forward(state, *[x.permute(2, 0, 1)[None].cpu() for x in xs])[0]
    full = torch.from_numpy(pack_state(state, layout=LAYOUT_FULL)).cuda()
    eng = UNetEngine(full, H, W)
    kinds = [k for (_, _, _, k) in eng.profile(*xs)]
    assert kinds.count(5) >= 70 and kinds.count(6) == 3 and kinds.count(4) == 0
    split = eng.forward(*xs).clone()
    _check_rgb(split.permute(2, 0, 1).cpu(), ref, "split-operand plan")
    try:
        _lib.check(_lib.lib().read_tuning_set(b"conv_w4h", 0))
        kinds = [k for (_, _, _, k) in eng.profile(*xs)]
        assert kinds.count(5) == 0 and kinds.count(4) >= 70 and kinds.count(6) == 3        # FAM stays on the direct split-operand kernel
        fp32 = eng.forward(*xs).clone()
        _check_rgb(fp32.permute(2, 0, 1).cpu(), ref, "fp32-matrix-core plan")
        _check_rgb(split.permute(2, 0, 1).cpu(), fp32.permute(2, 0, 1).cpu(), "split-operand plan against the fp32 plan")
        assert not torch.equal(split, fp32)                    # two different arithmetic paths really ran
        lean = torch.from_numpy(pack_state(state, layout=LAYOUT_LEAN)).cuda()
        with pytest.raises(_lib.ReadHipError, match="lean"):
            UNetEngine(lean, H, W)
    finally:
        _lib.check(_lib.lib().read_tuning_set(b"conv_w4h", 32))


def test_lean_weight_blob_renders_the_same_frame(hip):
    """the lean packed blob (the F(4x4) layers carry their F(4x4) order only: 451 of 952 MB) gives the frame of the
    full blob bit for bit — same plan, same kernels, fewer bytes resident —, is what FrameRenderer and the UNet module pack by
    default, and is refused (then replaced by the full blob) when a tuning knob takes a layer off the F(4x4) kernel."""
    from read_amd import _lib
    from read_amd.unet import LAYOUT_FULL, LAYOUT_LEAN, UNetEngine, layout_of, pack_state
    H, W = 64, 96
    state = synthetic.make_unet_state(UNET_SPEC, 4)
    xs = [torch.rand(H >> l, W >> l, 8, device="cuda") for l in range(4)]
    outs = {}
    for layout in (LAYOUT_FULL, LAYOUT_LEAN):
        packed = torch.from_numpy(pack_state(state, layout=layout)).cuda()
        assert layout_of(packed) == layout
        outs[layout] = UNetEngine(packed, H, W).forward(*xs).clone()
    assert torch.equal(outs[LAYOUT_FULL], outs[LAYOUT_LEAN])
    net = UNet()
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    net.cuda().eval()
    with torch.no_grad():
        y = net(*[x.permute(2, 0, 1)[None] for x in xs])
    assert layout_of(net.packed_weights()) == LAYOUT_LEAN
    assert torch.equal(y[0].permute(1, 2, 0), outs[LAYOUT_FULL])
    # F(4x4) switched off: the lean blob cannot serve the plan -> loud refusal at the C level, automatic full blob in the module
    lean = torch.from_numpy(pack_state(state, layout=LAYOUT_LEAN)).cuda()
    live = UNetEngine(lean, H, W)                          # created while the F(4x4) kernel takes its layers ...
    try:
        _lib.check(_lib.lib().read_tuning_set(b"conv_w4", 0))
        with pytest.raises(_lib.ReadHipError, match="lean"):
            UNetEngine(lean, H, W)
        # ... and the knob changes under it: the executor's launches refuse the missing fragment order with
        # READ_EINVAL instead of reading through a NULL wpacked
        with pytest.raises(_lib.ReadHipError, match="wpacked is NULL"):
            live.forward(*xs)
        torch.cuda.synchronize()
        net.invalidate()
        with torch.no_grad():
            y2 = net(*[x.permute(2, 0, 1)[None] for x in xs])
        assert layout_of(net.packed_weights()) == LAYOUT_FULL
        _check_rgb(y2.cpu(), y.cpu(), "F(2x2) kernels from the full blob against F(4x4) from the lean one")
    finally:
        _lib.check(_lib.lib().read_tuning_set(b"conv_w4", 32))


# ------------------------------------------------------------------------------------------ the smallest viewports
# Every viewport that is a positive multiple of 16 is accepted.  At 16 x 16 the four levels are 16 x 16, 8 x 8, 4 x 4 and 2 x 2, the
# 4x4 / stride-2 layer feat_extract.7 writes ONE pixel and the rasteriser's fifth level is 1 x 1: every kernel of the plan runs on an
# image smaller than its unit.  16 x 48 / 48 x 16 / 32 x 16 are ragged in one direction, 80 x 112 has W / 8 = 14 (no multiple of 4)
# and a ragged tile row, 16 x 1216 is one tile row of the headline width.
TINY_VIEWPORTS = [(16, 16), (16, 48), (48, 16), (32, 16), (80, 112), (16, 1216)]
# tap of oracle.unet_torch.unet_forward -> tensor of the plan (read_amd/csrc/unet.cpp, Builder::build: the fourth block of a
# resblocks() ring lands in its ".y2")
ORACLE_TAPS = {"res1": "Encoder.0.y2", "res2": "Encoder.1.y2", "res3": "Encoder.2.y2", "zb": "Encoder.3.y2", "z2": "SCM2.out", "z4": "SCM1.out",
               "z8": "SCM0.out", "aff0": "aff0.out", "aff1": "aff1.out", "aff2": "aff2.out", "d3": "Decoder.3.y2"}
_TINY = {}


def _tiny_net():
    """One seeded state, its float64 copy and its full-layout blob on the device, shared by the tests below."""
    from read_amd.unet import LAYOUT_FULL, pack_state
    if not _TINY:
        state = synthetic.make_unet_state(UNET_SPEC, 9)
        _TINY["state"] = state
        _TINY["st64"] = {k: torch.from_numpy(np.asarray(v)).double() for k, v in state.items() if np.asarray(v).dtype.kind == "f"}
        _TINY["full"] = torch.from_numpy(pack_state(state, layout=LAYOUT_FULL)).cuda()
    return _TINY


def _tiny_case(H, W):
    """-> (inputs (h, w, 8) per level on the host, float64 RGB (3, H, W), float64 taps), computed once per viewport."""
    if (H, W) not in _TINY:
        g = torch.Generator().manual_seed(1000 * H + W)
        xs = [torch.rand(H >> l, W >> l, 8, generator=g) for l in range(4)]
        taps = {}
        with torch.no_grad():
            ref = unet_torch.unet_forward(_tiny_net()["st64"], *[x.permute(2, 0, 1)[None].double() for x in xs], taps=taps)[0]
        assert ref.dtype == torch.float64
        _TINY[(H, W)] = (xs, ref, taps)
    return _TINY[(H, W)]


def _check_taps(eng, taps, what):
    for key, name in ORACLE_TAPS.items():
        t = eng.debug_tensor(name).permute(2, 0, 1).cpu().double()
        r = taps[key][0]
        assert t.shape == r.shape, (what, key, t.shape, r.shape)
        bad = float(((t - r).abs() / r.abs().clamp(min=1.0)).max())
        print("%s: tap %-5s %-14s %s relative error %.3e" % (what, key, name, tuple(t.shape), bad))
        assert bad <= TAP_REL, f"{what}: {key} ({name}): relative error {bad:.3e}"


def _assert_split_operand_plan(eng, xs_dev, what):
    """The default plan's 3x3 / stride-1 launches ran on the split-operand kernels (5; FAM's three on the direct one, 6), none on
    the fp32 Winograd kernel (4): the assertion of test_split_operand_plan_against_the_fp32_plan, so that a silent fallback at a
    small size does not pass for them."""
    kinds = [k for (_, _, _, k) in eng.profile(*xs_dev)]
    assert kinds.count(5) >= 70 and kinds.count(6) == 3 and kinds.count(4) == 0, (what, kinds)


@pytest.mark.parametrize("H,W", TINY_VIEWPORTS)
def test_unet_engine_at_the_smallest_viewports_against_fp64(hip, H, W):
    """UNetEngine (default plan, full layout) against unet_torch.unet_forward in FLOAT64 at the three network guards, and every tap
    the oracle exposes against the plan's tensor at TAP_REL.  read_unet_create writes nothing into the workspace (unet.cpp: the
    Builder only hands out addresses; UNetEngine allocates it with torch.empty), so the workspace is filled with NaN before the
    first forward: a launch that reads what no launch wrote — a halo, a row past a ragged unit — shows in the frame."""
    from read_amd.unet import UNetEngine
    xs, ref, taps = _tiny_case(H, W)
    xs_dev = [x.cuda() for x in xs]
    eng = UNetEngine(_tiny_net()["full"], H, W)
    eng.ws.fill_(0xFF)                                           # every float of it: 0xFFFFFFFF, a NaN
    got = eng.forward(*xs_dev).clone()
    torch.cuda.synchronize()
    what = f"{H}x{W} against fp64"
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite frame from a NaN-filled workspace"
    _check_rgb(got.permute(2, 0, 1).cpu(), ref, what)
    _check_taps(eng, taps, what)
    _assert_split_operand_plan(eng, xs_dev, what)
    again = eng.forward(*xs_dev)
    torch.cuda.synchronize()
    assert torch.equal(got, again), f"{what}: the second frame of the same engine differs"


@pytest.mark.parametrize("H,W", [(16, 16), (80, 112)])
def test_plan_knobs_at_the_smallest_viewports_against_fp64(hip, H, W):
    """The four unet_aff_split x unet_up_fold plans, conv_f4x1 = 0 (the F(4x4) split-operand kernel in the place of F(4,3) by rows) and
    conv_w4h = 0 (the fp32 Winograd kernel, full layout) at 16 x 16 and 80 x 112: each against the float64 network at the three guards.
    A plan is built under the knobs of its creation: one UNetEngine per plan on the shared full-layout blob (what UNet.invalidate()
    leads to, without packing the state again)."""
    from read_amd import _lib
    from read_amd.unet import UNetEngine
    xs, ref, _ = _tiny_case(H, W)
    xs_dev = [x.cuda() for x in xs]
    L = _lib.lib()
    default = {}
    for key in (b"unet_aff_split", b"unet_up_fold", b"conv_f4x1", b"conv_w4h"):     # what the knobs hold now is what they go back to
        val = ctypes.c_int(-1)
        _lib.check(L.read_tuning_get(key, ctypes.byref(val)))
        default[key] = val.value
    assert default[b"unet_aff_split"] == 1 and default[b"unet_up_fold"] == 0 and default[b"conv_f4x1"] > 0 and default[b"conv_w4h"] > 0, default
    plans = [{b"unet_aff_split": s, b"unet_up_fold": f} for s in (1, 0) for f in (0, 1)] + [{b"conv_f4x1": 0}, {b"conv_w4h": 0}]
    outs = []
    try:
        for plan in plans:
            for key, v in {**default, **plan}.items():
                _lib.check(L.read_tuning_set(key, v))
            eng = UNetEngine(_tiny_net()["full"], H, W)
            what = f"{H}x{W} " + (" ".join(f"{k.decode()}={v}" for k, v in plan.items()))
            outs.append(eng.forward(*xs_dev).permute(2, 0, 1).cpu())
            _check_rgb(outs[-1], ref, what)
            labels = eng.launch_labels()
            assert any(l.startswith("up4(") for l in labels) == (plan.get(b"unet_up_fold", 0) == 0) and ("AFFq3" in labels) == (plan.get(b"unet_aff_split", 1) == 1), (what, labels)
            if plan == plans[0]:
                _assert_split_operand_plan(eng, xs_dev, what)
            elif b"conv_w4h" in plan:
                kinds = [k for (_, _, _, k) in eng.profile(*xs_dev)]
                assert kinds.count(5) == 0 and kinds.count(4) >= 70, (what, kinds)
            del eng
    finally:
        for key, v in default.items():
            _lib.check(L.read_tuning_set(key, v))
    assert not torch.equal(outs[0], outs[4]) and not torch.equal(outs[0], outs[5]), "conv_f4x1 = 0 / conv_w4h = 0 did not change the arithmetic"


@pytest.mark.parametrize("N", [5000, (1 << 20) + 4321], ids=["plain", "cells"])
@pytest.mark.parametrize("W,H", [(16, 16), (48, 16)])
def test_frame_renderer_at_the_smallest_viewports(hip, W, H, N):
    """FrameRenderer at 16 x 16 and 16 rows x 48 columns, on a cloud below the cell-ordering threshold and on one above it: all five
    index / depth levels bit for bit against oracle.raster_multiscale (the fifth is 1 x 1 / 1 x 3), the frame at the network guards
    against net_and_texture_forward, and frames_in_flight = 2 equal to one frame at a time over four poses."""
    if ("cloud", N) not in _TINY:
        _TINY[("cloud", N)] = (synthetic.make_cloud(N, 5), synthetic.make_descriptors(N))
    xyz, desc = _TINY[("cloud", N)]
    state = _tiny_net()["state"]
    proj = synthetic.make_proj(W, H, f=float(W))
    seq = FrameRenderer(xyz, desc, _tiny_net()["full"], W, H, proj_matrix=proj)            # (the packed blob: the state is not packed again)
    assert (seq.raster.cells is not None) == (N > (1 << 20))
    poses = [synthetic.sweep_pose(k) for k in (0, 1, 2, 40)]
    want = []
    for k, pose in enumerate(poses):
        rgba = seq.render(pose).clone()
        want.append(rgba)
        if k not in (1, 3):                                               # (a warm-started frame and one after a jump)
            continue
        M = camera.total_matrix(proj, pose)[0]
        idx, dep = oracle.raster_multiscale(xyz, M, W, H, 5, threads=8)
        assert tuple(seq.idx[4].shape[1:]) == (H >> 4, W >> 4)
        for l in range(5):
            assert np.array_equal(seq.idx[l][0].cpu().numpy(), idx[l]), f"{W}x{H} pose {k}: index level {l}"
            assert np.array_equal(seq.depth[l][0].cpu().numpy().view(np.uint32), dep[l].view(np.uint32)), f"{W}x{H} pose {k}: depth level {l}"
        with torch.no_grad():
            ref = unet_torch.net_and_texture_forward(state, desc[None], idx)[0]
        _check_rgb(rgba[:, :, :3].permute(2, 0, 1).cpu(), ref, f"frame {W}x{H}, {N} points, pose {k}")
        assert bool((rgba[:, :, 3] == 1).all())
    seq.set_frames_in_flight(2)                                           # the same renderer, now with two plans and two streams
    outs = [seq.render(p) for p in poses]
    seq.sync()
    for i, (g, w) in enumerate(zip(outs, want)):
        assert torch.equal(g, w), f"{W}x{H}, {N} points: pipelined frame {i} differs"
