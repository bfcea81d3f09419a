"""A/B of two builds of libreadhip.so that must launch the same kernels: the current one against read_amd/libreadhip_v_<variant>.so
(READ_HIP_VARIANT, read_amd/_lib.py).  Used for host-only changes of the conv dispatcher (profiles/route_refactor_ab.md).

    python tools/route_ab.py trace DIR_A DIR_B      # rocprofv3 --kernel-trace csv of `bench.py --steps N`: same ordered launches?
    python tools/route_ab.py detail A.json B.json   # bench.py --full --detail: same per-launch family column?
    python tools/route_ab.py frames DIR_A DIR_B     # bench.py --dump-outputs: bit-identical frames?
    python tools/route_ab.py speed --variant parent --runs 3 --out FILE.md   # alternating default bench.py runs, both modes

Every bench.py run of `speed` is a fresh child process under a time limit; the first failure ends the script.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def launches(d):
    files = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))
    assert files, f"no kernel trace csv under {d}"
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    return [(r["Kernel_Name"], (int(r["Grid_Size_X"]), int(r["Grid_Size_Y"]), int(r["Grid_Size_Z"])),
             (int(r["Workgroup_Size_X"]), int(r["Workgroup_Size_Y"]), int(r["Workgroup_Size_Z"])), int(r["LDS_Block_Size"])) for r in rows]


def cmd_trace(a):
    A, B = launches(a.a), launches(a.b)
    conv = sum(1 for l in A if "gated_conv" in l[0])
    print(f"launches: {len(A)} / {len(B)} ({conv} gated-conv launches, {len(set(l[0] for l in A))} distinct kernels)")
    if A == B:
        print("IDENTICAL: the ordered list of (kernel, grid, workgroup, LDS bytes) is the same")
        return 0
    for i, (x, y) in enumerate(zip(A, B)):
        if x != y:
            print(f"first difference at launch {i}:\n  A {x}\n  B {y}")
            break
    print("same multiset of launches:", sorted(A) == sorted(B))
    return 1


def cmd_detail(a):
    A, B = json.load(open(a.a)), json.load(open(a.b))
    fa, fb = [(r["label"], r["c3s1"]) for r in A], [(r["label"], r["c3s1"]) for r in B]
    hist = {}
    for _, c in fa:
        hist[c] = hist.get(c, 0) + 1
    print(f"launches: {len(fa)} / {len(fb)}; family column histogram of A: {dict(sorted(hist.items()))}")
    print("IDENTICAL family column" if fa == fb else "family columns DIFFER: %r" % [(x, y) for x, y in zip(fa, fb) if x != y][:5])
    return 0 if fa == fb else 1


def cmd_frames(a):
    import numpy as np
    rc = 0
    for f in sorted(os.listdir(a.a)):
        x, y = np.load(os.path.join(a.a, f)), np.load(os.path.join(a.b, f))
        same = x.shape == y.shape and x.tobytes() == y.tobytes()
        print(f"{f}: shape {x.shape} {x.dtype}, finite {bool(np.isfinite(x).all())}, {'BIT-IDENTICAL' if same else 'DIFFERENT'}")
        rc |= 0 if same else 1
    return rc


def bench(variant, extra):
    env = dict(os.environ)
    env.pop("READ_HIP_VARIANT", None)
    if variant:
        env["READ_HIP_VARIANT"] = variant
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, env=env, capture_output=True, text=True, timeout=420)
    if p.returncode != 0:
        print(p.stdout[-2000:], p.stderr[-2000:], sep="\n", flush=True)
        sys.exit(f"bench.py {extra} with variant {variant!r} ended with status {p.returncode}: nothing more is run")
    rec = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    return rec["value"]


def cmd_speed(a):
    modes = (("frames/s, two frames in flight (the headline)", []), ("frames/s, one frame at a time (latency mode)", ["--frames-in-flight", "1"]))
    lines = []
    for title, extra in modes:
        runs = {"variant": [], "current": []}
        for i in range(a.runs):
            for who in ("variant", "current"):
                v = bench(a.variant if who == "variant" else None, extra)
                runs[who].append(v)
                print(f"{title}: run {i} {who} {v:.2f}", flush=True)
        lo, hi = min(runs["variant"]), max(runs["variant"])
        inside = all(lo <= v <= hi for v in runs["current"])
        lines += [f"### {title}", "", f"| run | {a.variant} | current |", "|---|---|---|"]
        lines += [f"| {i} | {x:.2f} | {y:.2f} |" for i, (x, y) in enumerate(zip(runs["variant"], runs["current"]))]
        lines += ["", f"Spread of the {a.variant} library's own repeats: {lo:.2f} .. {hi:.2f} ({100 * (hi - lo) / lo:.2f} %).  Current library: "
                  f"{min(runs['current']):.2f} .. {max(runs['current']):.2f}, mean {sum(runs['current']) / a.runs:.2f} against {sum(runs['variant']) / a.runs:.2f} "
                  f"({100 * (sum(runs['current']) / sum(runs['variant']) - 1):+.2f} %): "
                  + ("every run inside that spread." if inside else "NOT every run inside that spread."), ""]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    return 0


def main():
    p = argparse.ArgumentParser()
    sub = p.add_subparsers(dest="cmd", required=True)
    for name in ("trace", "detail", "frames"):
        s = sub.add_parser(name)
        s.add_argument("a")
        s.add_argument("b")
    s = sub.add_parser("speed")
    s.add_argument("--variant", default="parent")
    s.add_argument("--runs", type=int, default=3)
    s.add_argument("--out", default="")
    a = p.parse_args()
    sys.exit({"trace": cmd_trace, "detail": cmd_detail, "frames": cmd_frames, "speed": cmd_speed}[a.cmd](a))


if __name__ == "__main__":
    main()
