"""Does a source change alter the gfx950 code of a kernel?  One verdict per kernel symbol.

    python tools/isa_diff.py REV [file.hip] [--pair OLD=NEW ...]          (file defaults to conv.hip)

REV's read_amd/csrc/<file> is written into a temporary directory beside REV's headers (csrc/*.h, include/*.h); that copy and the
working tree's file are compiled with the product's flags (read_amd.build.FLAGS + PER_FILE) plus -S --cuda-device-only, and
each kernel's text (its label up to .Lfunc_end) is compared:

    identical       the text is byte-equal
    prologue-only   the text from the first "Loop Header: Depth=1" comment to .Lfunc_end is byte-equal, and num_vgpr, num_agpr,
                    numbered_sgpr, private_seg_size and the LDS size are equal: only code in front of the kernel's loop moved
    differs         anything else (a kernel without a depth-1 loop is identical or differs)

The one thing masked before comparing is the ordinal of the function inside the file in local labels (.LBB<n>_, .Lfunc_end<n>),
which changes when a kernel is added or removed above, and with it the blanks that pad a label line's comment to its column (an ordinal
of three digits where there were two shifts that padding by one).  Exit status 1 if any kernel differs or exists on one side only.

--pair OLD=NEW compares a kernel across a rename: OLD and NEW are substrings of the demangled names, each matching exactly one kernel
of REV and of the working tree; the two are compared as one kernel, with the symbol itself masked in the compared text as well.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from read_amd import build as B  # noqa: E402

META = ("num_vgpr", "num_agpr", "numbered_sgpr", "private_seg_size")
_ORDINAL = re.compile(r"(LBB|Lfunc_end|\bBB)\d+")
_PAD = re.compile(r"[ \t]+;")


def compile_asm(src, include, csrc, out):
    flags = []
    it = iter(B.FLAGS)
    for f in it:                                   # the product's flags with the two -I directories pointed at this side's headers
        if f == "-I":
            next(it)
            continue
        flags.append(f)
    cmd = [B._hipcc()] + flags + ["-I", include, "-I", csrc] + B.PER_FILE.get(os.path.basename(src), []) + ["-S", "--cuda-device-only", src, "-o", out]
    subprocess.check_call(cmd)
    with open(out) as f:
        return f.read().split("\n")


def kernels(lines):
    """{symbol: (text lines, {meta})} for every .amdhsa_kernel of an assembly listing."""
    names = [l.split()[1] for l in lines if l.startswith("\t.amdhsa_kernel ")]
    start = {l.split(":")[0]: i for i, l in enumerate(lines) if l[:1] not in ("\t", " ", ".", "") and ":" in l}
    sets = {}
    for l in lines:
        m = re.match(r"\t\.set (\S+)\.(\w+), (\S+)", l)
        if m:
            sets[(m.group(1), m.group(2))] = m.group(3)
    out = {}
    for n in names:
        i = start[n]
        j = next(k for k in range(i, len(lines)) if lines[k].startswith(".Lfunc_end"))
        text = [_PAD.sub(" ;", _ORDINAL.sub(r"\1", l)) for l in lines[i:j + 1]]
        meta = {k: sets.get((n, k)) for k in META}
        meta["lds"] = next(l.split()[1] for l in text if l.strip().startswith(".amdhsa_group_segment_fixed_size"))
        out[n] = (text, meta)
    return out


def from_loop(text):
    for i, l in enumerate(text):
        if "Loop Header: Depth=1" in l:
            return text[i:]
    return None


def verdict(a, b):
    (ta, ma), (tb, mb) = a, b
    if ta == tb:
        return "identical"
    la, lb = from_loop(ta), from_loop(tb)
    if la is not None and la == lb and ma == mb:
        return "prologue-only"
    return "differs"


def demangle(names):
    """Readable names where a demangler is installed, the symbols themselves otherwise."""
    for tool in ("llvm-cxxfilt", "c++filt"):
        try:
            out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
            return dict(zip(names, out))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def paired(pretty, side, text, which):
    """The one symbol of `side` whose demangled name contains `text`."""
    hits = [n for n in side if text in pretty[n]]
    if len(hits) != 1:
        sys.exit(f"--pair: {text!r} matches {len(hits)} kernels of {which}: " + ", ".join(pretty[n] for n in hits))
    return hits[0]


def main(rev, name="conv.hip", pairs=()):
    with tempfile.TemporaryDirectory() as tmp:
        csrc, inc = os.path.join(tmp, "csrc"), os.path.join(tmp, "include")
        os.makedirs(csrc)
        os.makedirs(inc)
        listing = subprocess.check_output(["git", "-C", ROOT, "ls-tree", "-r", "--name-only", rev, "read_amd/csrc", "include"], text=True).split()
        for path in listing:
            if path.endswith(".h") or path == "read_amd/csrc/" + name:
                dst = os.path.join(inc if path.startswith("include/") else csrc, os.path.basename(path))
                with open(dst, "wb") as f:
                    f.write(subprocess.check_output(["git", "-C", ROOT, "show", f"{rev}:{path}"]))
        with ThreadPoolExecutor(max_workers=2) as ex:
            old = ex.submit(compile_asm, os.path.join(csrc, name), inc, csrc, os.path.join(tmp, "old.s"))
            new = ex.submit(compile_asm, os.path.join(B.CSRC, name), os.path.join(ROOT, "include"), B.CSRC, os.path.join(tmp, "new.s"))
            old, new = kernels(old.result()), kernels(new.result())
    pretty = demangle(sorted(set(old) | set(new)))
    for pair in pairs:                                 # the renamed kernel takes its new symbol on both sides
        o, n = (paired(pretty, side, text, which) for side, text, which in zip((old, new), pair.split("=", 1), (rev, "the working tree")))
        text, meta = old.pop(o)
        old[n] = ([l.replace(o, "<kernel>") for l in text], meta)
        new[n] = ([l.replace(n, "<kernel>") for l in new[n][0]], new[n][1])
        pretty[n] = f"{pretty[o]}  ->  {pretty[n]}"
    pretty = {n: p.replace("(anonymous namespace)::", "") for n, p in pretty.items()}
    count = {}
    print(f"{name}: {rev} against the working tree, {len(old)} / {len(new)} kernels")
    print("verdict | lines old / new | vgpr agpr sgpr scratch lds | kernel")
    for n in sorted(set(old) | set(new), key=lambda n: pretty[n]):
        if n not in old or n not in new:
            v, detail = "differs", "only in " + ("the working tree" if n in new else rev)
        else:
            v = verdict(old[n], new[n])
            mo, mn = old[n][1], new[n][1]
            meta = " ".join(str(mn[k]) if mo[k] == mn[k] else f"{mo[k]}->{mn[k]}" for k in META + ("lds",))
            detail = f"{len(old[n][0])} / {len(new[n][0])} | {meta}"
        count[v] = count.get(v, 0) + 1
        print(f"{v} | {detail} | {pretty[n]}")
    print("total: " + ", ".join(f"{count.get(v, 0)} {v}" for v in ("identical", "prologue-only", "differs")))
    return 1 if count.get("differs") else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(usage=__doc__)
    ap.add_argument("rev")
    ap.add_argument("file", nargs="?", default="conv.hip")
    ap.add_argument("--pair", action="append", default=[], metavar="OLD=NEW")
    a = ap.parse_args()
    sys.exit(main(a.rev, a.file, a.pair))
