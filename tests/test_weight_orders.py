"""CPU: the weight orders of a layer — which ones a layout or the single-layer packer carries, where they lie and what they hold —
against tests/golden/weight_orders.json, recorded from a library built at the parent of the change that put them into one table
(tests/golden/make_weight_orders_golden.py TREE).  Sizes and sha256 digests: a blob that moves by one float, or one order packed
from the wrong operand, changes a digest."""
import json
import os

import pytest

from tests import weight_order_cases as wc


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "weight_orders.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(wc.LAYOUTS))
def test_unet_blob_is_byte_for_byte_the_recorded_one(golden, name):
    """pack_state of make_unet_state(UNET_SPEC, 3) in each layout (zero-filled first: the alignment gaps count)."""
    assert golden["blob_seed"] == wc.BLOB_SEED
    assert wc.blob_record(name) == golden["blobs"][name]


def test_f4x1_side_buffer_is_byte_for_byte_the_recorded_one(golden):
    """What f4x1_side_buffer derives from the FULL blob on the host (a CPU tensor): read_unet_f4x1_layer's offsets and shapes."""
    assert wc.side_record() == golden["side"]


@pytest.mark.parametrize("shape", wc.SHAPES, ids=lambda s: "%dx%dk%d" % s)
def test_single_layer_packer_carries_the_recorded_orders(golden, shape):
    """PackedGatedConv(device='cpu'): kc, the set of orders present and the bytes of each."""
    assert wc.layer_record(*shape) == golden["layers"]["%d,%d,%d" % shape]
