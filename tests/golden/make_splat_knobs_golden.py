"""Records tests/golden/splat_knobs.json: what read_tuning_key / read_tuning_set / read_tuning_get answer for every tuning key.

    python tests/golden/make_splat_knobs_golden.py TREE

TREE is a checkout of the commit whose behaviour is the reference (the parent of a change to the knob plumbing), with its
libreadhip.so built (python -m read_amd.build in TREE).  Only the library and its ctypes binding come from TREE.  The keys
in RETIRED are left out of the record; the positions are those of the keys that remain.  Needs no GPU.
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
RETIRED = ["splat_zl2", "splat_kslot", "splat_items", "splat_compact", "unet_streams"]
VALUES = [-5, 0, 1, 3, 17, 300]


def record(_lib):
    """[{key, default, set: [[status, value read back], ...] for VALUES}] in enumeration order; every default restored."""
    L = _lib.lib()
    keys, i = [], 0
    while True:
        k = L.read_tuning_key(i)
        if not k:
            break
        keys.append(k.decode())
        i += 1
    rows, v = [], C.c_int(0)
    for key in keys:
        if key in RETIRED:
            continue
        _lib.check(L.read_tuning_get(key.encode(), C.byref(v)))
        default, sets = v.value, []
        for x in VALUES:
            status = L.read_tuning_set(key.encode(), x)
            _lib.check(L.read_tuning_get(key.encode(), C.byref(v)))
            sets.append([status, v.value])
        _lib.check(L.read_tuning_set(key.encode(), default))
        _lib.check(L.read_tuning_get(key.encode(), C.byref(v)))
        assert v.value == default, (key, default, v.value)
        rows.append({"key": key, "default": default, "set": sets})
    return rows


def main(tree):
    sys.path.insert(0, os.path.abspath(tree))
    from read_amd import _lib                               # TREE's binding, hence TREE's library
    assert os.path.abspath(_lib.LIB_PATH).startswith(os.path.abspath(tree)), _lib.LIB_PATH
    rec = {"values": VALUES, "retired": RETIRED, "keys": record(_lib)}
    path = os.path.join(HERE, "splat_knobs.json")
    with open(path, "w") as f:
        dumps = lambda o: json.dumps(o, separators=(",", ":"))      # one key per line
        f.write('{"values":%s,"retired":%s,"keys":[\n%s\n]}\n' % (dumps(VALUES), dumps(RETIRED), ",\n".join(dumps(r) for r in rec["keys"])))
    print("keys:", len(rec["keys"]), "bytes:", os.path.getsize(path))


if __name__ == "__main__":
    main(sys.argv[1])
