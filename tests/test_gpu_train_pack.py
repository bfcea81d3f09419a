"""GPU: the one packing path of the training step (read_amd/csrc/train.hip pack_job_body) reached three ways — through the
read_conv_pack_*_device entry points, through read_conv_pack_job, and as a one-job read_conv_pack_batch table — must write the same
bits; and the default step must issue the launches it issued before its routing was collected in read_amd.train.layer_route /
dgrad_method (tests/golden/train_step_launches.json, recorded at the parent of that change).  CPU side: tests/test_train_route.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from read_amd import _lib, synthetic
from read_amd.unet import UNet
from tests.unet_spec import UNET_SPEC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS, DIRECT, WINO, W4 = _lib.PACK_PARAMS, _lib.PACK_DIRECT, _lib.PACK_WINO, _lib.PACK_W4
WRAPPER = {(DIRECT, 0): "read_conv_pack_weights_device", (DIRECT, 1): "read_conv_pack_dgrad_device",
           (WINO, 0): "read_conv_pack_wino_device", (WINO, 1): "read_conv_pack_dgrad_wino_device",
           (W4, 0): "read_conv_pack_w4_device", (W4, 1): "read_conv_pack_dgrad_w4_device"}
FLOATS = {(DIRECT, 0): "read_conv_packed_floats", (DIRECT, 1): "read_conv_dgrad_packed_floats",
          (WINO, 0): "read_conv_wino_floats", (WINO, 1): "read_conv_dgrad_wino_floats",
          (W4, 0): "read_conv_w4_floats", (W4, 1): "read_conv_dgrad_w4_floats"}
# (Cin, Cout, k) -> the (kind, mode, kc) the training step packs for such a layer: every kind, mode and padding case
SHAPES = [((32, 32, 3), [(W4, 0, 16), (W4, 1, 16)]),
          ((16, 32, 3), [(WINO, 0, 16)]),
          ((8, 32, 3), [(DIRECT, 0, 8), (WINO, 1, 16)]),
          ((32, 3, 3), [(WINO, 0, 16), (WINO, 1, 16)]),                  # Cout padded to 32 (forward) / to 8 (the dgrad's virtual input)
          ((64, 32, 1), [(DIRECT, 0, 16), (DIRECT, 1, 16)]),
          ((32, 32, 4), [(DIRECT, 0, 16)])]


def _fresh(n):
    return torch.full((n,), float('nan'), dtype=torch.float32, device="cuda")


def _three_ways(hip, job, n, wrapper_call):
    """-> the outputs of the *_device wrapper, of read_conv_pack_job and of a one-job read_conv_pack_batch, each into its own
    NaN-filled buffer of the n floats the order takes."""
    st = _lib.stream_ptr()
    outs = [_fresh(n) for _ in range(3)]
    b = _lib.PackJob.from_buffer_copy(job)
    b.out = outs[2].data_ptr()
    _lib.check(hip.read_conv_pack_job_prepare(C.byref(b)))
    assert b.total == n, "the job writes what the size function promises"          # before anything is launched into n floats
    _lib.check(wrapper_call(outs[0].data_ptr(), st))
    j = _lib.PackJob.from_buffer_copy(job)
    j.out = outs[1].data_ptr()
    _lib.check(hip.read_conv_pack_job(C.byref(j), st))
    assert (j.total, j.nblocks, j.Cp) == (b.total, b.nblocks, b.Cp)
    b.first_block = 0
    table = torch.frombuffer(bytearray(bytes(b)), dtype=torch.uint8).cuda()
    _lib.check(hip.read_conv_pack_batch(table.data_ptr(), 1, b.nblocks, st))
    torch.cuda.synchronize()
    return outs


def _same_bits(outs, what):
    a = outs[0].view(torch.int32)
    assert not torch.isnan(outs[0]).any(), (what, "the packer left part of its output unwritten")
    assert torch.equal(a, outs[1].view(torch.int32)), (what, "read_conv_pack_job differs from the *_device entry point")
    assert torch.equal(a, outs[2].view(torch.int32)), (what, "a one-job read_conv_pack_batch differs from the *_device entry point")


def test_device_wrappers_job_and_batch_pack_the_same_bits(hip):
    rng = np.random.default_rng(53)
    seen = set()
    for (cin, cout, k), jobs in SHAPES:
        wf, wm = (torch.from_numpy(rng.standard_normal((cout, cin, k, k)).astype(np.float32)).cuda() for _ in range(2))
        for kind, mode, kc in jobs:
            job = _lib.PackJob()
            job.kind, job.mode, job.Cin, job.Cout, job.ksize, job.kc = kind, mode, cin, cout, k, kc
            job.wf, job.wm = wf.data_ptr(), wm.data_ptr()
            size = getattr(hip, FLOATS[(kind, mode)])
            n = size(cin, cout, k) if kind == DIRECT else size(cin, cout)
            fn = getattr(hip, WRAPPER[(kind, mode)])
            shape = (cin, cout, k, kc) if kind == DIRECT else (cin, cout)
            assert n > 0, (kind, mode, cin, cout, k)
            outs = _three_ways(hip, job, n, lambda out, st: fn(*shape, wf.data_ptr(), wm.data_ptr(), out, st))
            _same_bits(outs, (kind, mode, cin, cout, k))
            assert outs[0].any()
            seen.add((kind, mode))
    assert seen == set(WRAPPER)
    # the parameter block, with and without biases; Cout 3 pads to 32, 300 takes two workgroups
    for cout in (3, 32, 300):
        bf, bm, gamma, beta, mean = (torch.from_numpy(rng.standard_normal(cout).astype(np.float32)).cuda() for _ in range(5))
        var = torch.from_numpy(rng.uniform(0.5, 1.5, cout).astype(np.float32)).cuda()
        for biases in (True, False):
            job = _lib.PackJob()
            job.kind, job.Cout, job.eps = PARAMS, cout, 1e-5
            job.gamma, job.beta, job.mean, job.var = (t.data_ptr() for t in (gamma, beta, mean, var))
            if biases:
                job.bf, job.bm = bf.data_ptr(), bm.data_ptr()
            ptrs = [t.data_ptr() if (biases or i >= 2) else None for i, t in enumerate((bf, bm, gamma, beta, mean, var))]
            outs = _three_ways(hip, job, hip.read_conv_param_floats(cout), lambda out, st: hip.read_conv_pack_params_device(cout, *ptrs, 1e-5, out, st))
            _same_bits(outs, ("params", cout, biases))
            assert bool(outs[0][:cout].any()) == biases


def test_default_step_issues_the_launches_of_the_parent(hip):
    """One eager forward + backward of the UNet at 32 x 48, B = 2, in .eval() and in .train(): the ordered (kind, flops, kernel
    family) list of train.FLOP_LOG — every convolution, dgrad and wgrad launch with the family that ran it."""
    from read_amd import train
    with open(os.path.join(ROOT, "tests", "golden", "train_step_launches.json")) as f:
        want = json.load(f)
    state = synthetic.make_unet_state(UNET_SPEC, 41)
    net = UNet()
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    net.cuda()
    graph_was, log_was = train.GRAPH_TRAIN, train.FLOP_LOG
    train.GRAPH_TRAIN = False
    try:
        for mode in ("eval", "train"):
            getattr(net, mode)()
            g = torch.Generator().manual_seed(5)
            xs = [torch.rand(2, 8, 32 >> l, 48 >> l, generator=g).cuda().requires_grad_(True) for l in range(4)]
            train.FLOP_LOG = []
            net(*xs).sum().backward()
            torch.cuda.synchronize()
            got = [[kind, float(flops), int(fam)] for (kind, flops, fam) in train.FLOP_LOG]
            assert train.LAST_STEP_PATH == 'eager'
            assert len(got) == len(want[mode]) == 315, mode
            wrong = [i for i, (a, b) in enumerate(zip(got, want[mode])) if a != b]
            assert not wrong, f"{mode}: launch {wrong[0]} is {got[wrong[0]]}, the parent issued {want[mode][wrong[0]]}"
            net.zero_grad()
    finally:
        train.GRAPH_TRAIN, train.FLOP_LOG = graph_was, log_was
