"""Records tests/golden/weight_orders.json: the packed UNet blobs of the three layouts, the F(4,3)-by-rows side buffer and the
single-layer packer's orders (tests/weight_order_cases.py), as sizes and sha256 digests.

    python tests/golden/make_weight_orders_golden.py TREE

TREE is a checkout of the commit whose bytes are the reference (the parent of a change to how weight orders are laid out or packed),
with its libreadhip.so built (python -m read_amd.build in TREE).  The cases come from THIS checkout; the library, its ctypes binding
and the Python packers come from TREE.  No GPU is needed; it takes a minute or two.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def main(tree):
    from tests import weight_order_cases as wc
    sys.path.insert(0, os.path.abspath(tree))
    from read_amd import _lib, gated_conv, unet             # TREE's package, hence TREE's library and packers
    for m in (_lib, gated_conv, unet):
        assert os.path.abspath(m.__file__).startswith(os.path.abspath(tree)), m.__file__
    assert os.path.abspath(_lib.LIB_PATH).startswith(os.path.abspath(tree)), _lib.LIB_PATH
    rec = {"blob_seed": wc.BLOB_SEED, "blobs": {}, "layers": {}}
    for name in wc.LAYOUTS:
        rec["blobs"][name] = wc.blob_record(name)
        print(name, rec["blobs"][name], flush=True)
    rec["side"] = wc.side_record()
    print("side", rec["side"], flush=True)
    for shape in wc.SHAPES:
        rec["layers"]["%d,%d,%d" % shape] = wc.layer_record(*shape)
    with open(os.path.join(HERE, "weight_orders.json"), "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("bytes:", os.path.getsize(os.path.join(HERE, "weight_orders.json")))


if __name__ == "__main__":
    main(sys.argv[1])
