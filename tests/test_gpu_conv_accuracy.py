"""GPU: every split-operand convolution kernel (gated_conv_wino4h_kernel, gated_conv_f4x1h_kernel, gated_conv_d3h_kernel,
gated_conv_d3h_s2_kernel, gated_conv_pxh_kernel and its taps form) against a float64 reference, in units of fp32 round-off, on unit-scale, checkpoint-like,
structured and range-edge inputs (tests/conv_ref64.py: the measure, the derived bounds with the source lines they count, the
generators).  Each case is asserted against
  * the derived bound, elementwise (hard: a case over it is a bug in the kernel or a flaw in the derivation);
  * the measured cap E <= c R against the torch-fp32 oracle's own error on the same inputs, c per family, launch mode and class from
    profiles/conv_accuracy_fp64.md (twice the largest measured ratio, rounded up to a power of two) — not where the oracle's error is
    below one unit (R_max < 1: impulses, where oneDNN is exact);
  * exactness where no product reaches the output (gamma = 0, an all-zero conv_f row with zero bias): the epilogue constant, ==.
Every element of every case is measured.  The fp32 kernels the split kernels replaced (Winograd F(4x4), config -5, family 4; one direct
fp32 configuration, family 0) are still what the full weight layout falls back to (conv_w4h = 0): on the 3x3 / stride-1 cases of classes
(a) - (c) their linear launches are held to the fp32 bound of the training forward (tests/train_ref64.py: conv_forward_bound) and their
gated launches to gated_bound composed from it — families "fp32_w4", "fp32_direct"; no measured cap: the derived bound, the kernel
family, finiteness and the exact constants.  Class (d) is built for the f16 range these kernels do not have: one case at 2e4 must be
finite.
An automatic launch (config -1) of the 3x3 / stride-1 family is attributed BY ITS BITS — the F(4x4) and the F(4,3)-by-rows kernel both
report family 5 — and held to the bound and cap of the kernel that ran.
Plus the persistent walk (shapes with more units than the device has compute units, impulses in a workgroup's second and third unit),
FAM's x1 * x2 launches, the family query against the dispatch order, the loud failure past the documented range, and one whole network
whose residual blocks carry checkpoint-like statistics against the float64 network.
What every frame of the default plan runs around those kernels is held to the same measure (families "pxh_pre", "chain", "sc" of
FAMILY_ID / FORCE; derivations in tests/conv_ref64.py):
  * gated_conv_pxh_kernel on nearest-resampled sources at sizes that are not powers of two apart (SHAPES_RESAMPLED; family pxh's caps);
  * the same kernel with a host-given pre-activation addend in the plan's layouts (SHAPES_PRE: pre_f_off != 0, pre_m_off != Cout,
    pre_cstride > 2 Cout, a shared last addend row / column, a padded channel group, a linear launch) on classes (a) - (d) — (b) also with
    an addend that cancels the launch's own sum, (c) single addend elements over a zero image — with sentinels around what it may write;
  * the six launches of the AFF chain in the plan's order against the float64 UNSPLIT 480-channel layer and the bound composed level by level;
  * the output head gated_conv_smallc_kernel (SHAPES_SC, config -6, family 1), with and without ELU, and its fill channel;
  * bilinear_up4_kernel against a float64 restatement of the formula (SHAPES_UP4).
Every pxh launch of these runs forced (config -10) and automatic (-1) and must report family 7.
Class (e), degenerate sizes: every family above — and the pair and wide forms of the F(4,3)-by-rows kernel — at the plan's levels of a
16 x 16 viewport and below, forced and automatic, every launch also inside guard bands (the section at the end of this file).
Run with -s to see the table; lines start with "ACC|"."""
import ctypes

import numpy as np
import pytest
import torch

from read_amd.gated_conv import PackedGatedConv, config_names, conv_desc, gated_conv
from tests import conv_ref64 as R64
from tests import train_ref64 as T

pytestmark = pytest.mark.gpu

FAMILY_ID = {"w4h": 5, "f4x1": 5, "d3h": 6, "d3h_s2": 6, "pxh": 7, "t3h": 8, "pxh_pre": 7, "chain": 7, "sc": 1, "fp32_w4": 4, "fp32_direct": 0}
FORCE = {"w4h": -7, "f4x1": -12, "d3h": -8, "d3h_s2": -1, "pxh": -10, "t3h": -11,         # stride 2 goes through the automatic choice, family asserted
         "pxh_pre": -10, "chain": -10, "sc": -6}                                           # pxh_pre: gated_conv_pxh_kernel with an addend; chain: the six AFF launches; sc: the head
DIRECT_FP32 = "k3s1c16_p2q1m4n1f1b2"
FP32 = {"fp32_w4": "w4", "fp32_direct": "direct"}                                          # the fp32 kernels: family of T.conv_forward_bound
# class (e) also forces the two other forms of the F(4,3)-by-rows kernel (tests/test_gpu_conv_f4x1_pair.py, _wide.py): the bound of f4x1
FAMILY_ID.update(f4x1_pair=5, f4x1_wide=5)
FORCE.update(f4x1_pair=-13, f4x1_wide=-14)
SAME_BOUND = {"f4x1_pair": "f4x1", "f4x1_wide": "f4x1"}


def fp32_config(family):
    return -5 if family == "fp32_w4" else config_names().index(DIRECT_FP32)


def _pack(L, src_channels):
    return PackedGatedConv(L["wf"], L["bf"], L["wm"], L["bm"], L["gamma"], L["beta"], L["mean"], L["var"], src_channels=src_channels)


def _nhwc(a_chw):
    return torch.from_numpy(np.ascontiguousarray(a_chw.transpose(1, 2, 0))).cuda()


class Case:
    def __init__(self, family, cls, name, L, x, stride=1, elu=True, residual=None, mul=None, split=None, xs=None, shifts=None, pre=None):
        """xs, shifts: the sources at their own sizes and their shifts (x is then their assembly, R64.assemble);
        pre = (tensor (preH, preW, C) float32 on the host, f_off, m_off, shift): the pre-activation addend of the launch."""
        if xs is not None:
            H, W = (xs[0].shape[1] >> shifts[0], xs[0].shape[2] >> shifts[0]) if shifts[0] >= 0 else (xs[0].shape[1] << -shifts[0], xs[0].shape[2] << -shifts[0])
            x, split = R64.assemble(xs, shifts, H, W), [s.shape[0] for s in xs]
        self.family, self.cls, self.name, self.L, self.x = family, cls, name, L, x
        self.stride, self.elu, self.residual, self.mul = stride, elu, residual, mul
        self.split = split if split is not None else [x.shape[0]]           # channels per source (pxh: concatenated sources)
        self.xs, self.shifts, self.pre = xs, shifts, pre
        self.k = L["wf"].shape[2]
        self._ref = None
        self._bounds = {}

    def addend(self):
        """-> (pre_f, pre_m) at output resolution, float32, or None."""
        if self.pre is None:
            return None
        t, f_off, m_off, shift = self.pre
        return tuple(R64.sample_addend(t, f_off, m_off, self.L["wf"].shape[0], shift, self.x.shape[1], self.x.shape[2]))

    def ref(self):
        if self._ref is None:
            self._ref = R64.reference(self.L, self.x, stride=self.stride, elu=self.elu, residual=self.residual, mul=self.mul, pre=self.addend())
        return self._ref

    def launch(self, config, linear=False, **more):
        """-> ((C or 2 C, H, W) float32 on the host, kernel family of the launch).  With an addend the output is a slot of a tensor four
        channels wider, filled with R64.SENTINEL: those four and the whole addend tensor must be unchanged afterwards."""
        pk = _pack(self.L, self.split)
        offs = np.cumsum([0] + self.split)
        if self.xs is not None:
            srcs = [(_nhwc(x), s) for x, s in zip(self.xs, self.shifts)]
        else:
            srcs = [(_nhwc(self.x[offs[i]:offs[i + 1]]), 0) for i in range(len(self.split))]
        kw = dict(stride=self.stride, elu=self.elu, config=config, **more)
        if linear:
            kw["linear"] = True
        else:
            if self.residual is not None:
                kw["residual"] = _nhwc(self.residual)
            if self.mul is not None:
                kw["mul"] = _nhwc(self.mul)
        cs = pt = None
        if self.pre is not None:
            cs = self.L["wf"].shape[0] * (2 if linear else 1)
            pt = torch.from_numpy(self.pre[0]).cuda()
            kw.update(pre=(pt,) + tuple(self.pre[1:]), out=torch.full(self.x.shape[1:] + (cs + 4,), R64.SENTINEL, device="cuda"), out_channels=cs + 4)
        from read_amd import _lib
        fam = _lib.lib().read_conv_kernel_family(ctypes.byref(conv_desc(pk, srcs, **kw)))
        out = gated_conv(pk, srcs, **kw)
        torch.cuda.synchronize()
        if pt is not None:
            assert _same_bits(pt.cpu().numpy(), self.pre[0]), f"{self.name}: the launch changed its addend tensor"
            assert bool((out[..., cs:] == R64.SENTINEL).all()), f"{self.name}: the launch wrote beyond its {cs} channels"
            out = out[..., :cs]
        return out.cpu().numpy().transpose(2, 0, 1), fam


def _bounds(case, family, linear=False):
    """-> (d_f, d_m, B_w): the pre-activation bounds and, for the Winograd family, the condition term B with A_w in the place of A (a
    linear launch of the fp32 Winograd kernel: [A_w + |b_f| | A_w + |b_m|])."""
    family = SAME_BOUND.get(family, family)
    if (family, linear) in case._bounds:
        return case._bounds[(family, linear)]
    if family not in case._bounds:
        ref = case.ref()
        if family in FP32:
            (df, cf), (dm, cm) = (T.conv_forward_bound(case.L, case.x, ref, FP32[family], fm) for fm in "fm")
            Bw = ref.S * (np.abs(ref.dact) * ref.sig * cf + np.abs(ref.g) * ref.sig * (1.0 - ref.sig) * cm) + np.abs(ref.y)
            case._bounds[(family, True)] = (df, dm, np.concatenate([cf, cm]) if family == "fp32_w4" else None)
            case._bounds[family] = (df, dm, Bw if family == "fp32_w4" else None)
        elif family in ("w4h", "f4x1"):
            preact = R64.preact_bound_wino if family == "w4h" else R64.preact_bound_f4x1
            df, Awf = preact(case.L, case.x, ref, "f")
            dm, Awm = preact(case.L, case.x, ref, "m")
            Awf = Awf + np.abs(case.L["bf"].astype(np.float64))[:, None, None]
            Awm = Awm + np.abs(case.L["bm"].astype(np.float64))[:, None, None]
            Bw = ref.S * (np.abs(ref.dact) * ref.sig * Awf + np.abs(ref.g) * ref.sig * (1.0 - ref.sig) * Awm) + np.abs(ref.y)
            case._bounds[family] = (df, dm, Bw)
        elif family == "sc":
            case._bounds[family] = (R64.preact_bound_sc(case.L, ref, "f"), R64.preact_bound_sc(case.L, ref, "m"), None)
        elif family == "pxh_pre":
            df, dm = (R64.preact_bound_addend(case.L, ref, "pxh", fm, tot) for fm, tot in (("f", ref.f), ("m", ref.m)))
            case._bounds[family] = (df, dm, None)
        else:
            df, dm = (R64.preact_bound_direct(case.L, ref, family, fm) for fm in "fm")
            case._bounds[family] = (df, dm, None)
    return case._bounds.get((family, linear), case._bounds[family])


def check(case, config, linear=False, family=None, rows=None, assert_caps=True):
    """Launch, measure, print the table line and assert the caps.  family: the split-operand family whose bound applies (None: a
    comparison kernel, printed only)."""
    ref = case.ref()
    got, fam = case.launch(config, linear)
    ora = R64.oracle_fp32(case.L, case.x, stride=case.stride, elu=case.elu, residual=case.residual, mul=case.mul, linear=linear, pre=case.addend())
    df, dm, Bw = _bounds(case, family, linear) if family is not None else (None, None, None)
    return judge(case.L, ref, got, ora, fam, df, dm, Bw, family, case.cls, case.name, config, linear, rows, assert_caps)


def judge(L, ref, got, ora, fam, df, dm, Bw, family, cls, name, config, linear=False, rows=None, assert_caps=True):
    """Measure one launch's output `got` and the oracle's `ora` against `ref`, print the table line and assert: the kernel family, finiteness,
    the derived bound (d_f, d_m: the pre-activation bounds), the measured cap, the exact constants."""
    finite = bool(np.isfinite(got).all())
    clean = np.nan_to_num(got, nan=3e38, posinf=3e38, neginf=-3e38)
    if linear:
        (e_max, e_rms), (r_max, r_rms) = R64.measure_linear(clean, ref), R64.measure_linear(ora, ref)
        truth = np.concatenate([ref.f, ref.m])
    else:
        (e_max, e_rms), (r_max, r_rms) = R64.measure_gated(clean, ref), R64.measure_gated(ora, ref)
        truth = ref.y
    q = float("nan")
    ea_max, ea_rms = e_max, e_rms
    if family is not None:
        bound = np.concatenate([df, dm]) if linear else R64.gated_bound(ref, df, dm)
        q = float((np.abs(clean.astype(np.float64) - truth) / bound).max())
        if Bw is not None:
            # Winograd: no bound in terms of A exists (the transforms amplify).  The asserted statistic is E against the transformed-domain
            # condition term A_w; E against A is printed as E(A): that number shows what Winograd costs.
            e_max, e_rms = R64._stats(np.abs(clean.astype(np.float64) - truth), Bw)
    row = dict(family=family or f"fp32[{fam}]", cls=cls, name=name, mode="linear" if linear else "gated", config=config, kernel=fam,
               E_max=e_max, E_rms=e_rms, EA_max=ea_max, EA_rms=ea_rms, R_max=r_max, R_rms=r_rms, q=q, finite=finite)
    print("ACC| %-8s | %s | %-44s | %-6s | cfg %3d fam %d | E_max %10.2f | E_rms %9.3f | R_max %8.2f | R_rms %7.3f | E/R max %8.2f rms %8.2f | err/bound %6.3f | E(A) max %10.2f rms %9.3f" % (
        row["family"], cls, name, row["mode"], config, fam, e_max, e_rms, r_max, r_rms, e_max / max(r_max, 1e-30), e_rms / max(r_rms, 1e-30), q, ea_max, ea_rms))
    if rows is not None:
        rows.append(row)
    if family is None or not assert_caps:
        return row
    what = f"{family} ({cls}) {name} {row['mode']} config {config}"
    assert fam == FAMILY_ID[family], f"{what}: the launch took kernel family {fam}"
    assert finite, f"{what}: non-finite output inside the documented range"
    assert q <= 1.0, f"{what}: {q:.3f} x the derived bound (E_max {e_max:.1f}, E_rms {e_rms:.2f})"
    if r_max >= 1.0 and family not in FP32:
        c = R64.measured_cap(family, row["mode"], cls)
        assert e_rms <= c * r_rms and e_max <= c * r_max, f"{what}: E_max {e_max:.2f} E_rms {e_rms:.3f} against {c} x (R_max {r_max:.2f}, R_rms {r_rms:.3f})"
    if not linear:
        mask, cands = R64.constant_outputs(L, ref)
        if mask.any():
            assert bool((np.equal(got, cands[0]) | np.equal(got, cands[1]))[mask].all()), f"{what}: outputs that no product reaches differ from the epilogue constant"
    return row


# ------------------------------------------------------------------------------------------ the cases
def _res(rng, cout, H, W):
    return rng.standard_normal((cout, H, W)).astype(np.float32)


def _out_hw(k, stride, H, W):
    pad = (k - 1) // 2
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


SHAPES_A = {  # a subset of the shapes of tests/test_gpu_conv.py: (cin or source list, cout, k, stride, H, W, elu, residual)
    "w4h": [(128, 128, 3, 1, 9, 17, True, True), (64, 64, 3, 1, 40, 100, False, True), (32, 32, 3, 1, 41, 130, True, False), (96, 96, 3, 1, 14, 37, False, False),
            (256, 256, 3, 1, 8, 32, True, True)],
    # f4x1: ragged 8 x 32 units and 4-pixel segments on all four borders (widths 4 k + 1 .. 4 k + 3, heights 8 k + 1 .. 8 k + 7), a single pixel
    "f4x1": [(32, 32, 3, 1, 41, 130, True, False), (64, 64, 3, 1, 13, 37, True, False), (128, 128, 3, 1, 9, 17, True, True), (256, 256, 3, 1, 11, 35, True, False),
             (96, 96, 3, 1, 23, 70, False, False), (160, 160, 3, 1, 3, 65, True, False), (64, 64, 3, 1, 1, 1, True, False)],
    "d3h": [(128, 128, 3, 1, 9, 17, True, True), (64, 64, 3, 1, 40, 100, False, True), (32, 32, 3, 1, 41, 130, True, False), (32, 64, 3, 1, 19, 45, True, False),
            (256, 256, 3, 1, 8, 32, False, True), (128, 32, 3, 1, 19, 45, True, False)],
    "d3h_s2": [(32, 64, 3, 2, 24, 80, True, False), (64, 128, 3, 2, 13, 37, False, False), (128, 256, 3, 2, 22, 46, True, False),
               (64, 64, 4, 2, 10, 18, True, False), (32, 96, 4, 2, 9, 21, False, False), (256, 128, 4, 2, 22, 76, True, False)],
    "pxh": [([16], 32, 1, 1, 12, 44, True, False), ([32], 56, 1, 1, 12, 44, True, False), ([8, 56], 64, 1, 1, 12, 44, False, False),
            ([128, 128], 128, 1, 1, 12, 44, True, True), ([96], 64, 1, 1, 40, 100, True, False), ([8, 248], 256, 1, 1, 12, 44, False, True)],
    "t3h": [(8, 32, 3, 1, 37, 61, True, False), (8, 16, 3, 1, 22, 76, True, False), (16, 32, 3, 1, 21, 45, True, False), (32, 64, 3, 1, 13, 70, False, False),
            (8, 32, 3, 1, 1, 40, True, False), (32, 32, 3, 1, 21, 45, True, True)],
}
SHAPES_B = {"w4h": [(64, 64, 3, 1, 23, 38), (128, 32, 3, 1, 9, 17)], "f4x1": [(64, 64, 3, 1, 23, 38), (128, 32, 3, 1, 9, 17)], "d3h": [(64, 64, 3, 1, 23, 38), (128, 32, 3, 1, 9, 17)],
            "d3h_s2": [(32, 64, 3, 2, 13, 37), (64, 32, 4, 2, 10, 18)], "pxh": [(64, 56, 1, 1, 12, 44), (256, 64, 1, 1, 9, 33)],
            "t3h": [(8, 32, 3, 1, 21, 45), (32, 32, 3, 1, 13, 37)]}
SHAPE_C = {"w4h": (64, 32, 3, 1, 13, 37), "f4x1": (64, 32, 3, 1, 13, 37), "d3h": (64, 32, 3, 1, 13, 37), "d3h_s2": (64, 32, 3, 2, 13, 37), "pxh": (64, 32, 1, 1, 13, 37), "t3h": (32, 32, 3, 1, 13, 37)}


def cases_a(family):
    for j, (cin, cout, k, s, H, W, elu, with_res) in enumerate(SHAPES_A[family]):
        split = cin if isinstance(cin, list) else [cin]
        c = sum(split)
        rng = np.random.default_rng([100 + j, c, cout])
        oh, ow = _out_hw(k, s, H, W)
        yield Case(family, "a", f"unit scale {split}->{cout} k{k}s{s} {H}x{W}", R64.tame_layer(c, cout, k, 200 + j), rng.standard_normal((c, H, W)).astype(np.float32),
                   stride=s, elu=elu, residual=_res(rng, cout, oh, ow) if with_res else None, split=split)


def cases_b(family):
    for j, (cin, cout, k, s, H, W) in enumerate(SHAPES_B[family]):
        L, x = R64.checkpoint_like(cin, cout, k, H, W, 300 + j)
        rng = np.random.default_rng([300 + j])
        oh, ow = _out_hw(k, s, H, W)
        yield Case(family, "b", f"checkpoint-like {cin}->{cout} k{k}s{s} {H}x{W}", L, x, stride=s, elu=j % 2 == 0,
                   residual=_res(rng, cout, oh, ow) if (j == 1 and family != "d3h_s2") else None)


def cases_c(family):
    cin, cout, k, s, H, W = SHAPE_C[family]
    L = R64.tame_layer(cin, cout, k, 400)
    for amp in (1.0, 2.0 ** -10):
        for (c, y, x_) in (R64.impulse_positions_f4x1 if family == "f4x1" else R64.impulse_positions)(cin, H, W):
            yield Case(family, "c", f"impulse {amp:g} at c{c} ({y},{x_})", L, R64.impulse(cin, H, W, c, y, x_, amp), stride=s)
    yield Case(family, "c", "constant 1", L, R64.constant_image(cin, H, W), stride=s)
    yield Case(family, "c", "checkerboard +-1", L, R64.checkerboard(cin, H, W), stride=s, elu=False)


def cases_d(family):
    cin, cout, k, s, H, W = SHAPE_C[family]
    L = R64.tame_layer(cin, cout, k, 500)
    rng = np.random.default_rng([500, cin])
    if family == "w4h":
        # the documented range edge: |B^T d B| = 100 x 650 = 65000 < 65504 at frequency (r, r'), on interior tiles of both unit rows
        for rows, tile in (((0, 0), (1, 1)), ((1, 2), (1, 1)), ((5, 5), (2, 3)), ((2, 5), (2, 7)), ((0, 5), (1, 8))):
            yield Case(family, "d", f"range edge 650 rows {rows} tile {tile}", L, R64.wino_range_edge(cin, H, W, rows=rows, tile=tile, amp=650.0))
    if family == "f4x1":
        # the documented range edge: |B^T d| = 10 x 6550 = 65500, which rounds to 65504, at frequency `row`, on every image row of an interior
        # segment and of the last full one (right of the unit seam at x = 32)
        for row in (0, 1, 2, 5):
            for segment in (3, W // 4 - 1):
                yield Case(family, "d", f"range edge 6550 row {row} segment {segment}", L, R64.f4x1_range_edge(cin, H, W, row=row, segment=segment, amp=6550.0))
    for amp, label in ((2.0 ** -14, "2^-14"), (1e-6, "1e-6")):
        # hi piece subnormal: the kernel promises an absolute floor of ~1e-11 per product here (X_FLOOR of tests/conv_ref64.py, carried
        # through the sum as conv(1, |w|)), not fp32-relative accuracy; the derived bound contains exactly that floor
        yield Case(family, "d", f"small scale {label}", L, (rng.standard_normal((cin, H, W)) * amp).astype(np.float32), stride=s)


ALL_CLASSES = {"a": cases_a, "b": cases_b, "c": cases_c, "d": cases_d}


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def attribute_auto(case):
    """The split-operand family an automatic launch (config -1) of this case runs on, or None.  The F(4x4) kernel and the F(4,3)-by-rows
    kernel both report family 5: the launch is attributed by its BITS — equal to the forced launch of one and different from the
    other's (different arithmetic: tests/test_gpu_conv_f4x1.test_f4x1_dispatch)."""
    got, fam = case.launch(-1)
    if fam != 5:
        return {6: "d3h", 7: "pxh", 8: "t3h"}.get(fam)
    as_f4x1, as_w4h = (_same_bits(got, case.launch(FORCE[f])[0]) for f in ("f4x1", "w4h"))
    assert as_f4x1 != as_w4h, f"{case.name}: an automatic family-5 launch equals {'both' if as_f4x1 else 'neither'} of config -12 and config -7"
    return "f4x1" if as_f4x1 else "w4h"


def run_family(family, rows=None, assert_caps=True, classes="abcd"):
    linear_too = family in ("pxh", "t3h")
    for cls in classes:
        for case in ALL_CLASSES[cls](family):
            check(case, FORCE[family], family=family, rows=rows, assert_caps=assert_caps)
            if linear_too:
                check(case, FORCE[family], linear=True, family=family, rows=rows, assert_caps=assert_caps)
            if cls in "ab" and FORCE[family] != -1:
                # the automatic choice: held to the bound and caps of whichever split-operand kernel it takes, printed otherwise
                check(case, -1, family=attribute_auto(case), rows=rows, assert_caps=assert_caps)


@pytest.mark.parametrize("family", ["w4h", "f4x1", "d3h", "d3h_s2", "pxh", "t3h"])
def test_split_operand_family_against_fp64(hip, family):
    run_family(family)


def fp32_cases(cls):
    """The 3x3 / stride-1 cases the fp32 kernels have always run on — classes (a), (b) of families w4h and d3h — and class (c) of w4h
    (d3h's structured cases are the same)."""
    for family in ("w4h", "d3h") if cls in "ab" else ("w4h",):
        for case in ALL_CLASSES[cls](family):
            if case.k == 3 and case.stride == 1 and case.x.shape[0] % 16 == 0:
                yield case


@pytest.mark.parametrize("cls", ["a", "b", "c"])
@pytest.mark.parametrize("family", list(FP32))
def test_fp32_kernels_against_fp64(hip, family, cls):
    """The fp32 Winograd F(4x4) kernel (config -5) and the direct fp32 configuration, linear and gated (module docstring)."""
    for case in fp32_cases(cls):
        for linear in (True, False):
            check(case, fp32_config(family), linear=linear, family=family)


# ------------------------------------------------------------------------------------------ resampled sources, addends, the AFF chain
# (sources, shifts, cout, H, W): a source coarser than an ODD-sized output, a finer first source, a padded channel group
SHAPES_RESAMPLED = [([32, 64, 128], (1, 0, -1), 64, 13, 37), ([32, 64], (2, 0), 56, 9, 17)]
# (sources, shifts, cout, H, W, channels of the addend tensor, f_off, m_off, pre_shift, linear): the layouts of the plan's AFF launches
# (build() of read_amd/csrc/unet.cpp) at sizes whose last addend row and column are shared by an odd rest, and a padded channel group
SHAPES_PRE = [([32], (0,), 32, 13, 37, 64, 0, 32, 1, False),
              ([32, 64], (1, 0), 64, 12, 44, 192, 32, 128, 1, False),
              ([32, 64, 128], (2, 1, 0), 128, 9, 17, 448, 96, 320, 1, False),
              ([64], (0,), 56, 11, 38, 112, 0, 56, 2, False),
              ([64], (0,), 96, 5, 9, 448, 0, 224, 1, True)]


def _sources(shape, cls, seed):
    """-> (L, xs) of class (a) / (d) (tame_layer, unit-scale sources times `amp`) or (b) (checkpoint_like)."""
    split, shifts, cout, H, W = shape[:5]
    cin, big = sum(split), max(max(shifts), 0)
    if cls == "b":
        L, xb = R64.checkpoint_like(cin, cout, 1, H << big, W << big, seed)
    else:
        L = R64.tame_layer(cin, cout, 1, seed)
        xb = (np.random.default_rng([seed, cin, H, W]).standard_normal((cin, H << big, W << big)) * (2.0 ** -14 if cls == "d" else 1.0)).astype(np.float32)
    return L, R64.split_sources(xb, split, shifts, H, W)


def cases_resampled():
    for j, shape in enumerate(SHAPES_RESAMPLED):
        for cls in "ab":
            L, xs = _sources(shape, cls, 900 + j)
            yield Case("pxh", cls, f"resampled {shape[0]} shifts {shape[1]}->{shape[2]} {shape[3]}x{shape[4]}", L, None, elu=j == 0, xs=xs, shifts=shape[1])


def cases_pre(cls):
    """The cases of one class over SHAPES_PRE: (case, linear)."""
    for j, shape in enumerate(SHAPES_PRE):
        split, shifts, cout, H, W, C, f_off, m_off, sh, linear = shape
        tag = f"{split}->{cout} {H}x{W} addend C={C} ({f_off},{m_off})>>{sh}"
        rng = np.random.default_rng([910 + j, ord(cls)])
        pre_shape = R64.addend_size(sh, H, W) + (C,)
        mk = lambda name, L, xs, t, **kw: (Case("pxh_pre", cls, f"{name} {tag}", L, None, xs=xs, shifts=shifts, pre=(t, f_off, m_off, sh), **kw), linear)   # noqa: E731
        if cls == "a":
            L, xs = _sources(shape, "a", 910 + j)
            yield mk("unit scale", L, xs, R64.addend_tensor(rng, pre_shape, f_off, m_off, cout), elu=j % 2 == 0,
                     residual=_res(rng, cout, H, W) if (j == 1 and not linear) else None)
        elif cls == "b":
            L, xs = _sources(shape, "b", 920 + j)
            t = R64.addend_tensor(rng, pre_shape, f_off, m_off, cout, 2.0 ** rng.uniform(-8, 8, cout))
            yield mk("checkpoint-like, addend 2^U(-8,8)", L, xs, t, elu=j % 2 == 0)
            own = R64.reference(L, R64.assemble(xs, shifts, H, W)).f
            yield mk("checkpoint-like, cancelling addend", L, xs, R64.cancelling_addend(t, own, f_off, sh), elu=j % 2 == 1)
        elif cls == "d":
            L, xs = _sources(shape, "d", 930 + j)
            yield mk("small scale 2^-14", L, xs, R64.addend_tensor(rng, pre_shape, f_off, m_off, cout, 2.0 ** -14))
        elif cls == "c":
            L = R64.tame_layer(sum(split), cout, 1, 940 + j)
            zeros = [np.zeros((c,) + hw, np.float32) for c, hw in zip(split, R64.source_sizes(shifts, H, W))]
            for (py, px, c) in R64.addend_impulse_spots(pre_shape[:2], cout):
                for off, br in ((f_off, "f"), (m_off, "m")):
                    t = np.full(pre_shape, R64.SENTINEL, np.float32)
                    t[..., f_off:f_off + cout] = 0.0
                    t[..., m_off:m_off + cout] = 0.0
                    t[py, px, off + c] = 1.0
                    yield mk(f"x = 0, addend 1 at ({py},{px}) {br}{c}", L, zeros, t)
            if j == 0:                                                              # the input impulses of the other families, with a constant addend
                t = np.full(pre_shape, R64.SENTINEL, np.float32)
                t[..., f_off:f_off + cout] = 0.5
                t[..., m_off:m_off + cout] = -0.25
                for (c, y, x_) in R64.impulse_positions(sum(split), H, W):
                    yield mk(f"impulse 1 at c{c} ({y},{x_}), constant addend", L, [R64.impulse(sum(split), H, W, c, y, x_, 1.0)], t)


def test_resampled_sources_against_fp64(hip):
    """The (ly << sl) >> sr addressing of gated_conv_pxh_kernel's loader at sizes that are NOT powers of two apart (13 x 37 read from
    7 x 19 and from 26 x 74; 9 x 17 from 36 x 68), forced (config -10) and automatic: family 7 both, the bound and caps of family pxh."""
    for case in cases_resampled():
        for cfg in (FORCE["pxh"], -1):
            check(case, cfg, family="pxh")


@pytest.mark.parametrize("cls", ["a", "b", "c", "d"])
def test_pxh_with_addend_against_fp64(hip, cls):
    """gated_conv_pxh_kernel with a host-given pre-activation addend in the layouts of the plan (pre_f_off != 0, pre_m_off != Cout,
    pre_cstride > 2 Cout, a last addend row / column shared by an odd output size, a padded channel group, pre_shift 2, a linear launch),
    against reference(..., pre=...) and preact_bound_direct(own) + u |f| (tests/conv_ref64.py, "A launch with an addend"), config -10 and
    -1, family 7 both.  The addend tensor and the channels of `out` beyond the launch's own stay as they were (Case.launch)."""
    for case, linear in cases_pre(cls):
        for cfg in (FORCE["pxh_pre"], -1):
            check(case, cfg, linear=linear, family="pxh_pre")


@pytest.mark.parametrize("cls", ["a", "b"])
def test_aff_chain_against_fp64(hip, cls):
    """The six launches of the default plan's AFF chain (R64.AFF_PLAN: q3 -> q2 -> AFF2 -> q1 -> AFF1 -> AFF0) on res1 32 x 20 x 36,
    res2 64 x 10 x 18, res3 128 x 5 x 9, z 256 x 3 x 5: each of q3, q2, q1 and each gated output against the float64 reference of the UNSPLIT
    layer on assemble(...) and the bound composed level by level; config -10 and -1, every launch family 7."""
    _aff_chain(cls, R64.aff_chain_inputs(cls), cls, "")


def _aff_chain(cls, inputs, row_cls, tag, guarded=False, rows=None, assert_caps=True):
    """The chain on `inputs` = (layers, sources), judged as class `row_cls`.  guarded: every launch a second time with its sources and
    its addend inside NaN bands and its output inside sentinel bands (class (e), `Guarded`): the same bits, untouched bands."""
    from read_amd import _lib
    layers, xs = inputs
    refs = R64.aff_chain_reference(layers, xs)
    for cfg in (FORCE["chain"], -1):
        fams = {}

        def launch(name, Lp, srcs, pre, linear, hw):
            pk = _pack(Lp, [x.shape[0] for x, _ in srcs])
            srcs_d = [(_nhwc(x), s) for x, s in srcs]
            kw = dict(config=cfg, linear=linear, pre=pre)
            fams[name] = _lib.lib().read_conv_kernel_family(ctypes.byref(conv_desc(pk, srcs_d, **kw)))
            out = gated_conv(pk, srcs_d, **kw)
            assert tuple(out.shape[:2]) == tuple(hw), (name, out.shape, hw)
            if guarded:
                g = Guarded()
                kw_g = dict(kw, pre=None if pre is None else (g.input(pre[0]),) + tuple(pre[1:]), out=g.output(tuple(out.shape)))
                gated_conv(pk, [(g.input(t), s) for t, s in srcs_d], **kw_g)
                torch.cuda.synchronize()
                bad = g.problems(out)
                assert not bad, f"{name} of the chain {tag} config {cfg}: {bad}"
            return out

        outs = R64.run_aff_chain(layers, xs, launch)
        torch.cuda.synchronize()
        for name, (ref, df, dm, Lfull, xfull) in refs.items():
            linear = name.startswith("q")
            got = outs[name].cpu().numpy().transpose(2, 0, 1)
            judge(Lfull, ref, got, R64.oracle_fp32(Lfull, xfull, linear=linear), fams[name], df, dm, None, "chain", row_cls,
                  f"{name} of the chain ({'tame' if cls == 'a' else 'checkpoint-like'}){tag}", cfg, linear=linear, rows=rows, assert_caps=assert_caps)


# ------------------------------------------------------------------------------------------ the output head and the up-sampling
SHAPES_SC = [(3, 9, 33), (3, 17, 65), (4, 8, 32), (1, 9, 33)]          # (cout, H, W): READ's 32 -> 3 head on partial 8 x 32 tiles, a full tile, one channel


def cases_sc(cls):
    for j, (cout, H, W) in enumerate(SHAPES_SC):
        rng = np.random.default_rng([950 + j, ord(cls)])
        tag = f"32->{cout} {H}x{W}"
        for elu in (True, False):
            if cls == "a":
                yield Case("sc", cls, f"unit scale {tag} elu={elu}", R64.tame_layer(32, cout, 3, 950 + j), rng.standard_normal((32, H, W)).astype(np.float32), elu=elu)
            elif cls == "b":
                L, x = R64.checkpoint_like(32, cout, 3, H, W, 960 + j, edge_rows=(j == 1))        # (the edge rows would be all of a 3-row layer)
                yield Case("sc", cls, f"checkpoint-like {tag} elu={elu}", L, x, elu=elu)
            elif cls == "d":
                for amp, label in ((2.0 ** -14, "2^-14"), (1e-6, "1e-6")):
                    yield Case("sc", cls, f"small scale {label} {tag} elu={elu}", R64.tame_layer(32, cout, 3, 970 + j), (rng.standard_normal((32, H, W)) * amp).astype(np.float32), elu=elu)
            elif cls == "c" and j == 0:
                L = R64.tame_layer(32, cout, 3, 980)
                for amp in (1.0, 2.0 ** -10):
                    for (c, y, x_) in R64.impulse_positions(32, H, W):
                        if elu or (y in (0, H - 1) or x_ in (0, W - 1)):                         # without ELU: the border impulses
                            yield Case("sc", cls, f"impulse {amp:g} at c{c} ({y},{x_}) elu={elu}", L, R64.impulse(32, H, W, c, y, x_, amp), elu=elu)
                yield Case("sc", cls, f"constant 1 elu={elu}", L, R64.constant_image(32, H, W), elu=elu)
                yield Case("sc", cls, f"checkerboard +-1 elu={elu}", L, R64.checkerboard(32, H, W), elu=elu)


@pytest.mark.parametrize("cls", ["a", "b", "c", "d"])
def test_output_head_against_fp64(hip, cls):
    """gated_conv_smallc_kernel (config -6, family 1): 288 sequential v_fmac_f32 per accumulator, against 288 u A + u |f| and the gate
    epilogue's bound (tests/conv_ref64.py, "The output head")."""
    for case in cases_sc(cls):
        check(case, FORCE["sc"], family="sc")


def test_output_head_fill(hip):
    """out_channels = 4, fill = 1.0 on the 32 -> 3 head: the fourth channel is the fill, exactly, and the three real ones are the bits of
    the launch without it."""
    case = next(iter(cases_sc("a")))
    plain, fam = case.launch(FORCE["sc"])
    filled, fam4 = case.launch(FORCE["sc"], out_channels=4, fill=1.0)
    assert fam == 1 and fam4 == 1 and filled.shape[0] == 4
    assert bool((filled[3] == np.float32(1.0)).all()) and _same_bits(np.ascontiguousarray(filled[:3]), plain)


SHAPES_UP4 = [(32, 1, 1), (64, 3, 2), (128, 5, 19), (256, 2, 7)]          # (C, h, w)


def test_bilinear_up4_against_fp64(hip):
    """bilinear_up4_kernel against the float64 restatement of the formula (R64.bilinear_up4_ref) and 4 u sum w |v|, on unit-scale and
    per-channel-scaled inputs; a constant image of 1.0 comes back exactly 1.0."""
    from read_amd.gated_conv import bilinear_up4
    for j, (c, h, w) in enumerate(SHAPES_UP4):
        rng = np.random.default_rng([990 + j])
        for label, scale in (("unit scale", np.ones(c)), ("2^U(-8,8) per channel", 2.0 ** rng.uniform(-8, 8, c))):
            x = (rng.standard_normal((c, h, w)) * scale[:, None, None]).astype(np.float32)
            got = bilinear_up4(_nhwc(x)).cpu().numpy().transpose(2, 0, 1)
            want, absum = R64.bilinear_up4_ref(x)
            err = np.abs(got.astype(np.float64) - want)
            q = float((err / R64.bilinear_up4_bound(absum)).max())
            print("ACC| up4      | %s | %-44s | E_max %6.2f | err/bound %6.3f" % ("a" if label == "unit scale" else "b", f"{label} {c} {h}x{w}", R64._stats(err, absum)[0], q))
            assert got.shape == (c, 4 * h, 4 * w) and q <= 1.0, (c, h, w, label, q)
        ones = bilinear_up4(_nhwc(np.ones((c, h, w), np.float32))).cpu().numpy()
        assert bool((ones == np.float32(1.0)).all()), (c, h, w)


# ------------------------------------------------------------------------------------------ the persistent walk
# The kernels of the 8 x 32-unit family run one workgroup per compute unit, each walking units u = blockIdx, blockIdx + grid, ... with
# grid = min(n_units, CUs) rounded down to a multiple of the Cout / 32 channel groups (persistent_grid of read_amd/csrc/conv.hip; unit u =
# tile u / groups, group u % groups).  The walk has state of its own — step_tile with its single wrap in x, a prefetch cursor that runs
# ahead into the next unit, V buffers whose parity across units depends on whether Cin / 32 is odd, weight rings that keep turning — and
# only a shape with MORE units than compute units reaches it.  (C, H, W): 261 / 513 / 258 / 261 / 264 units on 256 CUs.
WALK_SHAPES = [(32, 72, 900),       # one chunk: the V parity flips per unit; some workgroups walk two units
               (32, 150, 860),      # one workgroup walks three
               (64, 24, 1376),      # two groups
               (96, 20, 920),       # three groups, grid 255, an odd chunk count
               (256, 20, 330)]      # eight groups


def walk_grid(c, H, W):
    """-> (n_units, grid, groups, tiles_x): the rule above, restated from the device's compute-unit count and the shape."""
    groups, tiles_x = (c + 31) // 32, (W + 31) // 32
    n_units = tiles_x * ((H + 7) // 8) * groups
    grid = min(n_units, torch.cuda.get_device_properties(0).multi_processor_count)
    grid = max(grid - grid % groups, groups)
    return n_units, grid, groups, tiles_x


_WALK_CASES = {}


def walk_cases(shape):
    """-> the class (a) case and the class (c) case (one image with two impulses) of one walk shape, built once and shared by the
    families that run it (only the latest shape is kept: the references of 10^5 pixels are large); asserts the conditions that make
    them walk."""
    if shape in _WALK_CASES:
        return _WALK_CASES[shape]
    _WALK_CASES.clear()
    c, H, W = shape
    n_units, grid, groups, tiles_x = walk_grid(c, H, W)
    assert n_units > grid, f"{c} x {H}x{W}: {n_units} units on a grid of {grid}: no workgroup walks a second unit on this device"
    t0 = (grid + groups - 1) // groups                                       # the first tile all of whose units have index >= grid
    spots = [(1 % c, min(8 * (t0 // tiles_x) + 3, H - 1), min(32 * (t0 % tiles_x) + 17, W - 1)), (c - 1, H - 1, W - 1)]
    x = np.zeros((c, H, W), np.float32)
    for (ch, y, x_) in spots:
        unit = ((y // 8) * tiles_x + x_ // 32) * groups
        assert unit >= grid, f"the impulse at ({y},{x_}) lies in units {unit} .. {unit + groups - 1}, the grid is {grid}"
        x[ch, y, x_] = 1.0
    rng = np.random.default_rng([800, c, H, W])
    L = R64.tame_layer(c, c, 3, 800)
    tag = f"walk {n_units} / {grid}: {c} {H}x{W}"
    _WALK_CASES[shape] = [Case("walk", "a", f"{tag} unit scale", L, rng.standard_normal((c, H, W)).astype(np.float32), residual=_res(rng, c, H, W)),
                          Case("walk", "c", f"{tag} impulses at " + " ".join(f"c{ch} ({y},{x_})" for (ch, y, x_) in spots), L, x)]
    return _WALK_CASES[shape]


WALK_RUNS = [(shape, family) for shape in WALK_SHAPES for family in (("f4x1", "w4h", "d3h") if shape in ((32, 72, 900), (256, 20, 330)) else ("f4x1",))]


@pytest.mark.parametrize("shape,family", WALK_RUNS, ids=lambda v: v if isinstance(v, str) else "%dx%dx%d" % v)
def test_persistent_walk_against_fp64(hip, shape, family):
    """Unit-scale inputs (class (a)) and two impulses (class (c)) on shapes with more units than the device has compute units: one
    impulse in the first tile that only a workgroup's SECOND unit reaches, one in the last unit (partial on every shape but 24 x 1376).
    Held to the derived bound and to the caps of classes (a) / (c) of the family, as every other case; config -12 on every shape, -7
    and -8 on two of them (no other kernel-level float64 case walks a second unit for those kernels either).  A device with more compute
    units than a shape has units FAILS here: the shapes must then grow, not the test pass without walking."""
    for case in walk_cases(shape):
        check(case, FORCE[family], family=family)


def test_f4x1_fails_loudly_past_its_range(hip):
    """Activations of ~2e4 (normal x 2e4; |B^T d| far beyond 65504, the documented range ends at 6550 — module docstring of
    tests/conv_ref64.py): the F(4,3)-by-rows kernel returns Inf / NaN, never a plausible wrong number, as
    tests/test_gpu_conv.test_winograd_f4_split_operand_kernel asserts for the F(4x4) kernel."""
    L = R64.tame_layer(64, 64, 3, 78)
    x = (np.random.default_rng(78).standard_normal((64, 24, 40)) * 2.0e4).astype(np.float32)
    got, fam = Case("f4x1", "d", "normal x 2e4", L, x).launch(FORCE["f4x1"])
    assert fam == 5 and not np.isfinite(got).all(), "overflow of the f16 pieces must not pass silently"


def test_fp32_kernels_stay_finite_past_the_f16_range(hip):
    """The counterpart of test_f4x1_fails_loudly_past_its_range: on the same activations of ~2e4 the fp32 kernels have no range to leave —
    finite, and inside the fp32 bound like every other case."""
    L = R64.tame_layer(64, 64, 3, 78)
    x = (np.random.default_rng(78).standard_normal((64, 24, 40)) * 2.0e4).astype(np.float32)
    case = Case("fp32", "d", "normal x 2e4", L, x)
    for fp32 in FP32:
        for linear in (True, False):
            assert check(case, fp32_config(fp32), linear=linear, family=fp32)["finite"]


def test_fam_multiply_through_the_direct_split_kernel(hip):
    """FAM's x1 * x2 launch (automatic choice: family 6 with a multiplier): the product is rounded to fp32 before the split, one more u per
    product in the bound."""
    for j, c in enumerate((64, 128)):
        rng = np.random.default_rng([600, c])
        x1, x2 = rng.standard_normal((c, 12, 40)).astype(np.float32), rng.standard_normal((c, 12, 40)).astype(np.float32)
        case = Case("d3h", "a", f"FAM x1 * x2 C={c}", R64.tame_layer(c, c, 3, 600 + j), x1, elu=False, residual=x1, mul=x2)
        check(case, -1, family="d3h")
    L, x = R64.checkpoint_like(64, 64, 3, 12, 40, 610)
    x2 = (np.random.default_rng(611).standard_normal(x.shape)).astype(np.float32)
    check(Case("d3h", "b", "FAM x1 * x2 checkpoint-like C=64", L, x, elu=False, residual=x, mul=x2), -1, family="d3h")


def test_family_query_agrees_with_the_dispatch_for_small_cout(hip):
    """read_conv_kernel_family tests the small-Cout kernel before the implicit-GEMM form, as launch_gated_conv dispatches: with conv_t3h
    raised to 32 a 32 -> 4 layer still runs (and reports) the vector-pipe kernel, family 1; forced with config -11 it is family 8."""
    from read_amd import _lib
    L_ = _lib.lib()
    L = R64.tame_layer(32, 4, 3, 700)
    pk = _pack(L, [32])
    x = torch.randn(128, 160, 32, device="cuda")
    try:
        assert L_.read_conv_kernel_family(ctypes.byref(conv_desc(pk, [(x, 0)]))) == 1
        _lib.check(L_.read_tuning_set(b"conv_t3h", 32))
        assert L_.read_conv_kernel_family(ctypes.byref(conv_desc(pk, [(x, 0)]))) == 1
        assert L_.read_conv_kernel_family(ctypes.byref(conv_desc(pk, [(x, 0)], config=-11))) == 8
        L64 = R64.tame_layer(32, 64, 3, 701)
        assert L_.read_conv_kernel_family(ctypes.byref(conv_desc(_pack(L64, [32]), [(x, 0)]))) == 8
    finally:
        _lib.check(L_.read_tuning_set(b"conv_t3h", 8))


# ------------------------------------------------------------------------------------------ the whole network
def rescale_like_a_checkpoint(state, seed):
    """A seeded UNet state whose residual blocks x + BC1(BC0(x)) carry checkpoint-like statistics, WITHOUT changing the function:
      * BC0's output channel c is scaled by b_c = 2^U(-8, 6) through its BatchNorm affine (gamma, beta) and BC1's weights of input channel
        c by 1 / b_c: BC1 — a 3x3 / stride-1 layer on the Winograd split-operand kernel — sees activations whose channel scales span 2^14
        against inversely scaled weights (products stay O(1), the f16 pieces do not);
      * BC1 has no ELU, so its conv_f rows (and bias) are scaled by a_o = 2^U(-6, 3) and the inverse is folded into its running
        statistics: mean' = a mean, var' + eps = a^2 (var + eps) (var' from 2e-4 to 1e2)."""
    st = {k: np.array(v, dtype=np.float64 if np.asarray(v).dtype.kind == "f" else None, copy=True) for k, v in state.items()}
    rng = np.random.default_rng(seed)
    for blk in ("Encoder", "Decoder"):
        for i in range(4):
            for j in range(4):
                p0, p1 = f"{blk}.{i}.layers.{j}.main.0.block.", f"{blk}.{i}.layers.{j}.main.1.block."
                c = st[p0 + "norm.weight"].shape[0]
                b = 2.0 ** rng.uniform(-8, 6, c)
                st[p0 + "norm.weight"] *= b
                st[p0 + "norm.bias"] *= b
                for conv in ("conv_f", "conv_m"):
                    st[p1 + conv + ".weight"] /= b[None, :, None, None]
                a = 2.0 ** rng.uniform(-6, 3, c)
                st[p1 + "conv_f.weight"] *= a[:, None, None, None]
                st[p1 + "conv_f.bias"] *= a
                st[p1 + "norm.running_mean"] *= a
                st[p1 + "norm.running_var"] = a * a * (st[p1 + "norm.running_var"] + R64.EPS) - R64.EPS
    return {k: (v.astype(np.float32) if v.dtype.kind == "f" else v) for k, v in st.items()}


def scale_inner_channel(state, block, c, factor):
    """The same exchange for one channel of one residual block: BC0's output channel c times `factor`, BC1's weights of that channel divided."""
    st = dict(state)
    p0, p1 = block + ".main.0.block.", block + ".main.1.block."
    for key in ("norm.weight", "norm.bias"):
        v = st[p0 + key].astype(np.float64)
        v[c] *= factor
        st[p0 + key] = v.astype(np.float32)
    for conv in ("conv_f", "conv_m"):
        v = st[p1 + conv + ".weight"].astype(np.float64)
        v[:, c] /= factor
        st[p1 + conv + ".weight"] = v.astype(np.float32)
    return st


def test_unet_with_checkpoint_like_statistics_against_fp64(hip):
    """UNetEngine at 96 x 160 on a make_unet_state whose 32 residual blocks were rescaled as above, against unet_torch.unet_forward run in
    FLOAT64 (state and inputs cast: the restatement takes its dtype from them), at the three network guards of tests/test_gpu_unet.py
    (MAX_ABS, MIN_PSNR, MAX_REL_RMS).  The input of the Winograd layer Decoder.0.layers.0.main.1, recomputed in float64 from the tap `zb`,
    is brought to a maximum of 300 by scaling its largest channel (the same function-preserving exchange) and must then exceed 100
    somewhere and stay below the documented 650: the split kernel's range is exercised, not just its middle.
    Second pass: the same exchange to a maximum of 3000 — inside the F(4,3)-by-rows kernel's documented ~6500 and outside F(4x4)'s 650 —
    with the engine's default plan, after asserting that this plan is what it names: conv_f4x1 = 32 and the engine holds the
    F(4,3)-by-rows side buffer.  The same three guards."""
    from oracle import unet_torch
    from read_amd import _lib, synthetic
    from read_amd.unet import UNetEngine, pack_state
    from tests.test_gpu_unet import _check_rgb
    from tests.unet_spec import UNET_SPEC
    H, W = 96, 160
    base = rescale_like_a_checkpoint(synthetic.make_unet_state(UNET_SPEC, 9), 17)
    torch.manual_seed(3)
    xs = [torch.rand(H >> l, W >> l, 8) for l in range(4)]
    x64 = [x.permute(2, 0, 1)[None].double() for x in xs]
    to64 = lambda st: {k: torch.from_numpy(np.asarray(v)).double() for k, v in st.items() if np.asarray(v).dtype.kind == "f"}   # noqa: E731
    taps = {}
    with torch.no_grad():
        unet_torch.unet_forward(to64(base), *x64, taps=taps)
        inner = unet_torch.basic_conv(to64(base), "Decoder.0.layers.0.main.0", taps["zb"], 3)[0]
    per_channel = inner.abs().amax(dim=(1, 2))
    c = int(per_channel.argmax())
    L_ = _lib.lib()
    for target, lo, hi in ((300.0, 100.0, 650.0), (3000.0, 1000.0, 6500.0)):
        state = scale_inner_channel(base, "Decoder.0.layers.0", c, target / float(per_channel[c]))
        with torch.no_grad():
            st64 = to64(state)
            ref = unet_torch.unet_forward(st64, *x64, taps=taps)[0]
            top = float(unet_torch.basic_conv(st64, "Decoder.0.layers.0.main.0", taps["zb"], 3).abs().max())
        print("input of Decoder.0.layers.0.main.1: max |x| = %.1f" % top)
        assert ref.dtype == torch.float64 and lo < top < hi, top
        eng = UNetEngine(torch.from_numpy(pack_state(state)).cuda(), H, W)
        if target > 650.0:                                                          # the pass is about the F(4,3)-by-rows kernel: the default plan must run it
            knob = ctypes.c_int(-1)
            _lib.check(L_.read_tuning_get(b"conv_f4x1", ctypes.byref(knob)))
            assert knob.value == 32, knob.value
            assert getattr(eng, "f4x1", None) is not None and eng.f4x1.is_cuda and eng.f4x1.numel() == L_.read_unet_f4x1_floats()
        kinds = [k for (_, _, _, k) in eng.profile(*[x.cuda() for x in xs])]
        assert kinds.count(5) >= 70, kinds                                          # the residual blocks run on the Winograd split-operand kernels
        got = eng.forward(*[x.cuda() for x in xs]).permute(2, 0, 1).cpu()
        _check_rgb(got, ref, "checkpoint-like statistics against fp64, inner maximum %g" % target)


# ------------------------------------------------------------------------------------------ class (e): degenerate sizes
# Every family at the plan's own levels of a 16 x 16 viewport and below (tests/conv_ref64.py, "Class (e)": the shapes, the inputs, why
# the bounds hold unchanged).  Each launch runs twice: on plainly allocated tensors, and with every tensor it reads inside NaN bands
# and the one it writes inside sentinel bands (GUARD floats before and after, tests/train_fp32.py) — the same bits, a finite result,
# untouched bands: a load past a tensor's end may be masked before arithmetic, it may not reach it.  include/read_hip.h documents no
# slack that a caller owes, so none is given.  GUARD floats are 256 bytes: the views keep the alignment of the allocation.
from tests.train_fp32 import GUARD, SENTINEL as BAND          # noqa: E402


class Guarded:
    """The tensors of one guarded launch."""

    def __init__(self):
        self.ins, self.out_flat, self.out = [], None, None

    def input(self, t):
        """A device or host array -> an equal view inside a NaN-filled flat buffer with GUARD floats on either side."""
        t = torch.as_tensor(t).cuda()
        flat = torch.full((t.numel() + 2 * GUARD,), float("nan"), device="cuda")
        view = flat[GUARD:GUARD + t.numel()].view(t.shape)
        view.copy_(t)
        self.ins.append((flat, view, t.clone()))
        return view

    def output(self, shape):
        n = int(np.prod(shape))
        self.out_flat = torch.full((n + 2 * GUARD,), float(BAND), device="cuda")
        self.out = self.out_flat[GUARD:GUARD + n].view(shape)
        return self.out

    def problems(self, plain_out):
        """-> what went wrong, as a list of strings: a band written, an input changed, a non-finite output, other bits than `plain_out`."""
        bad = []
        if not bool((self.out_flat[:GUARD] == float(BAND)).all() and (self.out_flat[-GUARD:] == float(BAND)).all()):
            bad.append("wrote into the band around its output")
        for flat, view, orig in self.ins:
            if not bool(torch.isnan(flat[:GUARD]).all() and torch.isnan(flat[-GUARD:]).all() and torch.equal(view.view(torch.int32), orig.view(torch.int32))):
                bad.append("changed an input or its band")
        if not bool(torch.isfinite(self.out).all()):
            bad.append("a load outside a tensor reached the arithmetic: non-finite output")
        if plain_out is not None and not torch.equal(self.out.view(torch.int32), plain_out.view(torch.int32)):
            bad.append("other bits than on plainly allocated tensors")
        return bad


_PACKS = {}


def _pack_once(L, split):
    key = (id(L), tuple(split))
    if key not in _PACKS:
        _PACKS[key] = (L, _pack(L, list(split)))              # (L is kept alive: its id is the key)
    return _PACKS[key][1]


def launch_e(case, config, linear=False):
    """-> (output (C or 2 C, H, W) of the guarded launch or None, kernel family, message of a refusal or None, problems)."""
    from read_amd import _lib
    L_ = _lib.lib()
    pk = _pack_once(case.L, case.split)
    hwc = lambda a: np.ascontiguousarray(np.asarray(a, np.float32).transpose(1, 2, 0))          # noqa: E731
    offs = np.cumsum([0] + list(case.split))
    src_np = [(hwc(x), s) for x, s in zip(case.xs, case.shifts)] if case.xs is not None else [(hwc(case.x[offs[i]:offs[i + 1]]), 0) for i in range(len(case.split))]
    cout = case.L["wf"].shape[0]
    cs = cout * (2 if linear else 1)
    oh, ow = _out_hw(case.k, case.stride, case.x.shape[1], case.x.shape[2])
    plain = None
    for guarded in (False, True):
        g = Guarded()
        put = g.input if guarded else (lambda a: torch.as_tensor(a).cuda())
        srcs = [(put(a), s) for a, s in src_np]
        kw = dict(stride=case.stride, elu=case.elu, config=config)
        if linear:
            kw["linear"] = True
        else:
            if case.residual is not None:
                kw["residual"] = put(hwc(case.residual))
            if case.mul is not None:
                kw["mul"] = put(hwc(case.mul))
        if case.pre is not None:
            kw["pre"] = (put(case.pre[0]),) + tuple(case.pre[1:])
        out = g.output((oh, ow, cs))
        d = conv_desc(pk, srcs, out=out, **kw)
        fam = L_.read_conv_kernel_family(ctypes.byref(d))
        f4 = getattr(pk, "wpacked_f4x1", None)
        rc = (L_.read_gated_conv_forward_f4x1(ctypes.byref(d), f4.data_ptr(), _lib.stream_ptr()) if f4 is not None
              else L_.read_gated_conv_forward(ctypes.byref(d), _lib.stream_ptr()))
        msg = L_.read_last_error().decode("utf-8", "replace") if rc != 0 else None
        torch.cuda.synchronize()
        if rc != 0:
            # a forced configuration "forces it where the shape fits": a refusal is READ_EINVAL with a message, before any device work
            assert rc == -22 and msg and config != -1, f"{case.name} config {config}: return {rc}, message {msg!r}"
            assert bool((g.out_flat == float(BAND)).all()), f"{case.name} config {config}: a refused launch wrote"
            return None, fam, msg, []
        if guarded:
            return out.cpu().numpy().transpose(2, 0, 1), fam, None, g.problems(plain)
        plain = out.clone()


def check_e(case, config, family, linear=False, rows=None, assert_caps=True):
    """check() for class (e): the guarded launch, judge()'s assertions, and the guard bands.  A refused forced configuration is
    asserted to be a refusal (launch_e) and printed as one."""
    got, fam, refusal, problems = launch_e(case, config, linear)
    mode = "linear" if linear else "gated"
    if refusal is not None:
        print("ACC| %-8s | e | %-44s | %-6s | cfg %3d fam %d | REFUSED: %s" % (family, case.name, mode, config, fam, refusal))
        if rows is not None:
            rows.append(dict(family=family, cls="e", name=case.name, mode=mode, config=config, kernel=fam, refused=refusal))
        return None
    if (linear, "ora") not in case._bounds:
        case._bounds[(linear, "ora")] = R64.oracle_fp32(case.L, case.x, stride=case.stride, elu=case.elu, residual=case.residual, mul=case.mul, linear=linear, pre=case.addend())
    df, dm, Bw = _bounds(case, family, linear)
    row = judge(case.L, case.ref(), got, case._bounds[(linear, "ora")], fam, df, dm, Bw, family, "e", case.name, config, linear, rows, assert_caps)
    row["problems"] = problems
    assert not (problems and assert_caps), f"{family} (e) {case.name} {mode} config {config}: {problems}"
    return row


AUTO_FAMILY = {0: "fp32_direct", 1: "sc", 4: "fp32_w4", 6: "d3h", 7: "pxh", 8: "t3h"}
_CASES_E = {}


def cases_e(group):
    """The cases of one group of class (e), built once and shared by the families that run them: [[the cases of one shape, the
    unit-scale one first]]."""
    if group in _CASES_E:
        return _CASES_E[group]
    shapes = []
    if group == "s1":
        for j, (c, H, W) in enumerate(R64.SHAPES_E_S1):
            L, rng = R64.tame_layer(c, c, 3, 1100 + j), np.random.default_rng([1100 + j])
            shapes.append([Case("s1", "e", f"{c} {H}x{W} {name}", L, x, elu=elu, residual=_res(rng, c, H, W) if unit else None)
                           for name, x, elu, unit in R64.degenerate_images(c, H, W, 1100 + j)])
    elif group == "d3h_s2":
        for j, (cin, cout, k, H, W) in enumerate(R64.SHAPES_E_S2):
            L = R64.tame_layer(cin, cout, k, 1200 + j)
            shapes.append([Case("d3h_s2", "e", f"{cin}->{cout} k{k}s2 {H}x{W} {name}", L, x, stride=2, elu=elu) for name, x, elu, _ in R64.degenerate_images(cin, H, W, 1200 + j)])
    elif group in ("pxh", "t3h", "sc"):
        layers = {"pxh": [(split, cout, 1, R64.SIZES_E_PXH) for split, cout in R64.SHAPES_E_PXH],
                  "t3h": [([cin], cout, 3, R64.SIZES_E_T3H) for cin, cout in R64.SHAPES_E_T3H], "sc": [([32], 3, 3, R64.SIZES_E_SC)]}[group]
        for j, (split, cout, k, sizes) in enumerate(layers):
            L = R64.tame_layer(sum(split), cout, k, 1300 + j)
            for (H, W) in sizes:
                rng = np.random.default_rng([1300 + j, H, W])
                shapes.append([Case(group, "e", f"{split}->{cout} {H}x{W} {name}", L, x, elu=elu, split=split, residual=_res(rng, cout, H, W) if unit and group != "sc" else None)
                               for name, x, elu, unit in R64.degenerate_images(sum(split), H, W, 1300 + j)])
    elif group == "resampled":
        for j, shape in enumerate(R64.SHAPES_E_RESAMPLED):
            split, shifts, cout, H, W = shape
            big = max(max(shifts), 0)
            L = R64.tame_layer(sum(split), cout, 1, 1400 + j)
            shapes.append([Case("pxh", "e", f"resampled {split} {shifts}->{cout} {H}x{W} {name}", L, None, elu=elu, xs=R64.split_sources(xb, split, shifts, H, W), shifts=shifts)
                           for name, xb, elu, _ in R64.degenerate_images(sum(split), H << big, W << big, 1400 + j)])
    elif group == "pxh_pre":
        for j, (split, shifts, cout, C, f_off, m_off, sh) in enumerate(R64.LAYOUTS_E_PRE):
            L = R64.tame_layer(sum(split), cout, 1, 1500 + j)
            big = max(max(shifts), 0)
            for (H, W) in R64.SIZES_E_PRE:
                rng = np.random.default_rng([1500 + j, H, W])
                pre_shape = R64.addend_size(sh, H, W) + (C,)
                flat = np.full(pre_shape, R64.SENTINEL, np.float32)                              # a constant addend: 0.5 to f, -0.25 to m
                flat[..., f_off:f_off + cout], flat[..., m_off:m_off + cout] = 0.5, -0.25
                tag = f"{split}->{cout} {H}x{W} addend C={C}>>{sh}"
                mk = lambda name, xs, t, elu: Case("pxh_pre", "e", f"{tag} {name}", L, None, elu=elu, xs=xs, shifts=shifts, pre=(t, f_off, m_off, sh))   # noqa: E731
                cases = [mk(name, R64.split_sources(xb, split, shifts, H, W), R64.addend_tensor(rng, pre_shape, f_off, m_off, cout) if unit else flat, elu)
                         for name, xb, elu, unit in R64.degenerate_images(sum(split), H << big, W << big, 1500 + j)]
                zeros = [np.zeros((c,) + hw, np.float32) for c, hw in zip(split, R64.source_sizes(shifts, H, W))]
                for amp in (1.0, 2.0 ** -10):                                                    # single addend elements over a zero image
                    for (py, px) in R64.degenerate_positions(*pre_shape[:2]):
                        for off, br in ((f_off, "f"), (m_off, "m")):
                            for c in dict.fromkeys((1 % cout, cout - 1)):
                                t = np.full(pre_shape, R64.SENTINEL, np.float32)
                                t[..., f_off:f_off + cout], t[..., m_off:m_off + cout] = 0.0, 0.0
                                t[py, px, off + c] = amp
                                cases.append(mk(f"x = 0, addend {amp:g} at ({py},{px}) {br}{c}", zeros, t, True))
                shapes.append(cases)
    else:
        raise ValueError(group)
    _CASES_E[group] = shapes
    return shapes


# what runs each group: (family whose bound and cap apply, forced configuration or None: the fp32 kernels' own, linear launches too)
RUNS_E = {"w4h": ("s1", False), "f4x1": ("s1", False), "f4x1_pair": ("s1", False), "f4x1_wide": ("s1", False), "d3h": ("s1", False),
          "fp32_w4": ("s1", True), "fp32_direct": ("s1", True), "d3h_s2": ("d3h_s2", False), "pxh": ("pxh", True), "t3h": ("t3h", True),
          "sc": ("sc", False), "resampled": ("resampled", False), "pxh_pre": ("pxh_pre", False)}


def run_e(family, rows=None, assert_caps=True):
    group, linear_too = RUNS_E[family]
    fam = "pxh" if family == "resampled" else family
    config = fp32_config(fam) if fam in FP32 else -9 if fam == "d3h_s2" else FORCE[fam]
    for cases in cases_e(group):
        for case in cases:
            if fam == "f4x1_wide" and case.L["wf"].shape[0] % 64 != 0:
                continue                                                  # the wide form exists where two channel groups do: not a case of it
            check_e(case, config, fam, rows=rows, assert_caps=assert_caps)
            if linear_too:
                check_e(case, config, fam, linear=True, rows=rows, assert_caps=assert_caps)


def run_e_auto(group, rows=None, assert_caps=True):
    """Every shape of the group on the automatic route (config -1): attributed once per shape, on the unit-scale case (the route looks at
    the shape, not at the data; an impulse can give two kernels the same bits), and held to the bound and cap of the family that ran."""
    for cases in cases_e(group):
        fam = attribute_auto(cases[0])
        if fam is None:
            fam = AUTO_FAMILY[cases[0].launch(-1)[1]]
        if fam == "d3h" and cases[0].stride == 2:
            fam = "d3h_s2"                                                # family 6 both; the stride-2 form has its own rows and cap
        if fam == "pxh" and cases[0].pre is not None:
            fam = "pxh_pre"                                               # the same kernel; the bound of a launch with an addend
        for case in cases:
            row = check_e(case, -1, fam, rows=rows, assert_caps=assert_caps)
            assert row is not None, f"{case.name}: the automatic route refused an accepted shape"


@pytest.mark.parametrize("family", list(RUNS_E))
def test_degenerate_sizes_against_fp64(hip, family):
    """Class (e), every family forced (module comment above; the shapes of tests/conv_ref64.py)."""
    run_e(family)


@pytest.mark.parametrize("group", ["s1", "d3h_s2", "pxh", "t3h", "sc", "resampled", "pxh_pre"])
def test_degenerate_sizes_on_the_automatic_route(hip, group):
    run_e_auto(group)


@pytest.mark.parametrize("cls", ["a", "b"])
def test_aff_chain_degenerate_against_fp64(hip, cls):
    """test_aff_chain_against_fp64 at the levels of a 16 x 16 viewport: res1 32 x 16 x 16, res2 64 x 8 x 8, res3 128 x 4 x 4, z 256 x 2 x 2,
    every launch also guarded."""
    _aff_chain(cls, R64.aff_chain_inputs(cls, R64.SIZES_E_CHAIN), "e", " 16x16..2x2", guarded=True)
