"""Records tests/golden/conv_route.json: what a library answers for the descriptor sweep of tests/route_cases.py.

    python tests/golden/make_route_golden.py TREE

TREE is a checkout of the commit whose behaviour is the reference (the parent of a dispatcher change), with its libreadhip.so
built (python -m read_amd.build in TREE).  The sweep comes from THIS checkout; only the library and its ctypes binding come from
TREE.  Run it on a machine WITHOUT a GPU: the launch outcomes are taken with fake pointers.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def main(tree):
    import torch
    assert not torch.cuda.is_available(), "the outcome sweep launches with fake pointers: no GPU may be visible"
    from tests import route_cases as rc
    sys.path.insert(0, os.path.abspath(tree))
    from read_amd import _lib                               # TREE's binding, hence TREE's library
    assert os.path.abspath(_lib.LIB_PATH).startswith(os.path.abspath(tree)), _lib.LIB_PATH
    sweep, messages, sets = rc.Sweep(_lib), [], {}

    def code(outcome):
        outcome = list(outcome)
        if outcome not in messages:
            messages.append(outcome)
        return messages.index(outcome)

    raw = {}
    for name, cases in sweep.sets():
        fam, fwd, fwd_f4x1 = [], [], []
        for case in cases:
            fam.append(sweep.family(case))
            fwd.append(code(sweep.outcome(case, False)))
            fwd_f4x1.append(code(sweep.outcome(case, True)))
        raw[name] = {"family": fam, "forward": fwd, "forward_f4x1": fwd_f4x1}
        # stored compactly: the knob sets as differences from the default state, the f4x1 entry point as differences from the plain one
        block = {"shapes": len(rc.CONFIGS), "knob:defaults": 2}.get(name, len(rc.operand_variants()))
        base = "knob:defaults" if name.startswith("knob:") and name != "knob:defaults" else None
        sets[name] = {"n": len(fam)}
        for field in ("family", "forward"):
            sets[name][field] = rc.diff(raw[name][field], raw[base][field], [base, field]) if base else rc.pack(raw[name][field], block)
        sets[name]["forward_f4x1"] = rc.diff(fwd_f4x1, fwd, [name, "forward"])
        for field in raw[name]:
            assert rc.unpack(sets, name, field) == raw[name][field]
        print(name, len(fam), flush=True)
    rec = {"outcomes": messages, "sets": sets, "tuning_keys": rc.tuning_keys(_lib), "knob_values": list(rc.KNOB_VALUES),
           "knobs": rc.knob_table(_lib), "plans": rc.plans(_lib)}
    with open(os.path.join(HERE, "conv_route.json"), "w") as f:
        json.dump(rec, f, separators=(",", ":"))
    print("outcomes:", len(messages), "bytes:", os.path.getsize(os.path.join(HERE, "conv_route.json")))


if __name__ == "__main__":
    main(sys.argv[1])
