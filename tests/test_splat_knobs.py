"""CPU: the tuning keys answer as the recorded library did (tests/golden/splat_knobs.json, written by
tests/golden/make_splat_knobs_golden.py): the order read_tuning_key enumerates them in, every default, and for each of a few
values what read_tuning_set returns and what read_tuning_get then reads back.  The retired options are unknown keys."""
import ctypes as C
import json
import os

from read_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "splat_knobs.json")


def _enumerate(L):
    keys = []
    while True:
        k = L.read_tuning_key(len(keys))
        if not k:
            return keys
        keys.append(k.decode())


def test_tuning_keys_answer_as_recorded():
    rec = json.load(open(GOLDEN))
    L, v = _lib.lib(), C.c_int(0)
    keys = _enumerate(L)
    assert keys == [row["key"] for row in rec["keys"]]                 # positions: the enumeration order, nothing more, nothing less
    assert L.read_tuning_key(-1) is None and L.read_tuning_key(len(keys)) is None
    defaults = {}
    for key in keys:
        _lib.check(L.read_tuning_get(key.encode(), C.byref(v)))
        defaults[key] = v.value
    try:
        assert defaults == {row["key"]: row["default"] for row in rec["keys"]}
        for row in rec["keys"]:
            key = row["key"].encode()
            for x, (status, value) in zip(rec["values"], row["set"]):
                assert L.read_tuning_set(key, x) == status, (row["key"], x)
                _lib.check(L.read_tuning_get(key, C.byref(v)))
                assert v.value == value, (row["key"], x)
            _lib.check(L.read_tuning_set(key, row["default"]))
        assert L.read_tuning_set(b"splat_mode", 3) == -22
        assert L.read_last_error() == b"read_tuning_set: splat_mode must be 1 (agent atomics) or 7 (warm start + hi-z)"
    finally:
        for key, d in defaults.items():
            _lib.check(L.read_tuning_set(key.encode(), d))
    assert _lib.tuning_state() == defaults


def test_retired_options_are_unknown_keys():
    rec = json.load(open(GOLDEN))
    L, v = _lib.lib(), C.c_int(0)
    assert sorted(rec["retired"]) == ["splat_compact", "splat_items", "splat_kslot", "splat_zl2", "unet_streams"]
    keys = _enumerate(L)
    for key in rec["retired"]:
        assert key not in keys
        assert L.read_tuning_set(key.encode(), 1) == -22
        assert L.read_last_error() == b"read_tuning_set: unknown key '%s'" % key.encode()
        assert L.read_tuning_get(key.encode(), C.byref(v)) == -22
