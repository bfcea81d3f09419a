"""Training through a table list, measured: the descriptor half of a training step through a JointTexture of S = 1 / 2 / 4 tables against
the single-table path on the concatenated table.  One JSON line (kept as profiles/joint_texture_probe.json).  No gate.

    python tools/joint_texture_probe.py [--laps 5] [--reps 20] [--points 3000000]

The training batch's pixels: 8 crops of 256 x 256, five levels, C = 8 (698 368 pairs per step).  Ids are uniform over the --points
merged ids, 30 % of them 0 (the background); the gradient is normal(0, 1).  Per step, as the modules issue it:
  single    _GatherRowsFn queues the incoming gradient as it is (no launch); torch.cat of the five levels' ids and rows, one
            torch.sort, read_rmsprop_sorted on the concatenated (N, 8) table
  tables S  read_gather_backward_tables in pairs mode, one launch per level (activation none, as autograd calls it once per lookup);
            the same cat and sort; read_rmsprop_sorted_tables over S tables of N / S rows
  sort      the cat and the sort alone, for scale: both sides pay it
The variants alternate inside one process: one untimed lap of all of them, then --laps laps; a lap of a variant is --reps steps between
two HIP events, enqueued while a sleep kernel holds the GPU, so the lap is device time.  Per variant: mean / min / max microseconds
per step over the laps."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from read_amd import _lib  # noqa: E402
from read_amd.texture import gather_tables_backward  # noqa: E402

CROPS, SIDE, LEVELS, CH = 8, 256, 5, 8
LR, ALPHA, EPS = 1e-3, 0.99, 1e-8


def lap_us(call, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(int(2e8))
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def cat_sort(ids, rows):
    pids = torch.cat([i.reshape(-1) for i in ids])
    pg = torch.cat([r.reshape(-1, CH) for r in rows])
    sorted_ids, perm = torch.sort(pids, stable=True)
    return pids, pg, sorted_ids, perm


class State:
    """rows / sq / stamp of S tables of n rows each and the step counter they share."""

    def __init__(self, S, n, gen):
        self.rows = [torch.randn((n, CH), device="cuda", generator=gen) for _ in range(S)]
        self.sq = [torch.zeros_like(r) for r in self.rows]
        self.stamp = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(S)]
        self.n, self.step = n, 0
        self.scratch = torch.zeros(int(_lib.lib().read_rmsprop_sorted_scratch_ints()), dtype=torch.int32, device="cuda")


def single_step(st, ids, grad):
    L = _lib.lib()

    def call():
        st.step += 1
        pids, pg, sorted_ids, perm = cat_sort(ids, grad)
        _lib.check(L.read_rmsprop_sorted(st.rows[0].data_ptr(), st.sq[0].data_ptr(), st.stamp[0].data_ptr(), CH, st.n, sorted_ids.data_ptr(),
                                         perm.data_ptr(), pg.data_ptr(), int(pids.numel()), st.step, LR, ALPHA, EPS, st.scratch.data_ptr(),
                                         _lib.stream_ptr()), "read_rmsprop_sorted")
    return call


def tables_step(st, ids, grad):
    L, S = _lib.lib(), len(st.rows)
    meta = [(st.n, s * st.n, 'none') for s in range(S)]
    table = (_lib.RmspropTable * S)()
    for s in range(S):
        table[s].rows, table[s].sq, table[s].stamp = st.rows[s].data_ptr(), st.sq[s].data_ptr(), st.stamp[s].data_ptr()
        table[s].n, table[s].id_base, table[s].trainable = st.n, s * st.n, 1

    def call():
        st.step += 1
        g = [gather_tables_backward(meta, [i], [d], None, pairs=True)[0] for i, d in zip(ids, grad)]
        pids, pg, sorted_ids, perm = cat_sort(ids, g)
        for s in range(S):
            table[s].step = st.step
        _lib.check(L.read_rmsprop_sorted_tables(table, S, CH, sorted_ids.data_ptr(), perm.data_ptr(), pg.data_ptr(), int(pids.numel()), LR, ALPHA,
                                                EPS, st.scratch.data_ptr(), _lib.stream_ptr()), "read_rmsprop_sorted_tables")
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--laps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--points", type=int, default=3_000_000)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    gen = torch.Generator("cuda").manual_seed(1)
    N = a.points // 4 * 4
    ids, grad = [], []
    for l in range(LEVELS):
        shape = (CROPS, SIDE >> l, SIDE >> l)
        i = torch.randint(0, N, shape, device="cuda", generator=gen, dtype=torch.int32)
        i[torch.rand(shape, device="cuda", generator=gen) < 0.3] = 0
        ids.append(i)
        grad.append(torch.randn(shape + (CH,), device="cuda", generator=gen))
    pairs = sum(int(i.numel()) for i in ids)
    variants = {"single": single_step(State(1, N, gen), ids, grad), "sort": lambda: cat_sort(ids, grad)}
    for S in (1, 2, 4):
        variants[f"tables{S}"] = tables_step(State(S, N // S, gen), ids, grad)
    # one step of S = 4 computes what the single-table step computes (equal step counters, contiguous ranges): the rows agree bit for bit
    a_st, b_st = State(1, N, torch.Generator("cuda").manual_seed(2)), State(4, N // 4, torch.Generator("cuda").manual_seed(2))
    for s in range(4):
        b_st.rows[s].copy_(a_st.rows[0][s * (N // 4):(s + 1) * (N // 4)])
    single_step(a_st, ids, grad)()
    tables_step(b_st, ids, grad)()
    torch.cuda.synchronize()
    same = bool(torch.equal(a_st.rows[0], torch.cat(b_st.rows)))
    laps = {k: [] for k in variants}
    for lap in range(a.laps + 1):                                # lap 0 warms every variant up and is not kept
        for k, call in variants.items():
            t = lap_us(call, a.reps)
            if lap:
                laps[k].append(t)
    out = {"tool": "joint_texture_probe", "device": torch.cuda.get_device_name(0), "crops": CROPS, "side": SIDE, "levels": LEVELS, "C": CH,
           "points": N, "pairs_per_step": pairs, "laps": a.laps, "reps": a.reps, "tables4_equals_single_bit_for_bit": same, "variants": {}}
    for k, v in laps.items():
        out["variants"][k] = {"us_mean": round(float(np.mean(v)), 2), "us_min": round(min(v), 2), "us_max": round(max(v), 2),
                              "us_laps": [round(x, 2) for x in v]}
    base = out["variants"]["single"]
    out["single_spread_us"] = round(base["us_max"] - base["us_min"], 2)
    for S in (1, 2, 4):
        out[f"tables{S}_minus_single_us"] = round(out["variants"][f"tables{S}"]["us_mean"] - base["us_mean"], 2)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
