"""Records tests/golden/conv_pack_sha256.json: the sha256 of what every host weight packer writes for the cases of
tests/conv_pack_cases.py.

    python tests/golden/make_conv_pack_golden.py TREE REV

TREE is a checkout of the commit whose behaviour is the reference (the parent of a change to the packers), with its
libreadhip.so built (python -m read_amd.build in TREE); REV names that commit in the fixture's header.  The cases come from
THIS checkout; only the library and its ctypes binding come from TREE.  Needs no GPU.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def main(tree, rev):
    from tests import conv_pack_cases as cases
    sys.path.insert(0, os.path.abspath(tree))
    from read_amd import _lib                               # TREE's binding, hence TREE's library
    assert os.path.abspath(_lib.LIB_PATH).startswith(os.path.abspath(tree)), _lib.LIB_PATH
    rec = {"header": "sha256 of the output bytes of every read_conv_pack_*_host (direct order: with read_conv_unpack_weights_host "
                     "round-tripped), recorded by tests/golden/make_conv_pack_golden.py from the library built at the PARENT commit "
                     "of the change that moved the packers into conv_pack.cpp (%s), before the packers were touched" % rev,
           "seed": cases.SEED, "sha256": cases.digests(_lib.lib())}
    path = os.path.join(HERE, "conv_pack_sha256.json")
    with open(path, "w") as f:
        json.dump(rec, f, indent=0)
        f.write("\n")
    print("cases:", len(rec["sha256"]), "bytes:", os.path.getsize(path))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
