"""Print the forward plan's launch list, built on the CPU (no GPU needed), one line per op: launch or
Sync(src, dst), the entry point, the stream id, every scalar argument and `meta`. Pointer arguments
print as p<k>, k = the order in which that address first appears in the plan (null as p-), so two trees
that wire the same buffers to the same launches print the same text whatever the allocator returns.
For checking that a refactor of the plan-building code leaves the launches as they were:

    python3 profiles/plan_dump.py > new.txt    # and the same on the other tree
    diff old.txt new.txt

usage: python3 profiles/plan_dump.py [B]
"""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pose_estimation_amd import KRRN, make_config  # noqa: E402
from pose_estimation_amd.krrn import KRRNPlan  # noqa: E402
from pose_estimation_amd.runtime import Late, Sync  # noqa: E402
from pose_estimation_amd.synthetic import init_weights  # noqa: E402

# (backbone, classes, S, N): the BASELINE configurations' shapes and a small one
SHAPES = [("lm", 1, 120, 1000), ("w18", 1, 120, 1000), ("w18", 13, 64, 1000), ("w18", 13, 200, 1000),
          ("w18", 5, 256, 1000), ("w32", 1, 320, 4096), ("w18", 1, 64, 256)]


def _fmt(v, ids):
    if isinstance(v, Late):
        return f"Late({v.key})"
    if isinstance(v, ctypes.c_void_p):
        return "p-" if not v.value else f"p{ids.setdefault(v.value, len(ids))}"
    if isinstance(v, ctypes.Array):
        return "[" + ",".join(_fmt(x, ids) for x in v) + "]"
    if isinstance(v, ctypes._SimpleCData):
        return repr(v.value)
    if isinstance(v, float):
        return repr(v)
    if isinstance(v, (list, tuple)):
        return "(" + ",".join(_fmt(x, ids) for x in v) + ")"
    if isinstance(v, (int, str, bool)) or v is None:
        return str(v)
    raise TypeError(f"unexpected plan argument {v!r}")


def dump(plan, out=sys.stdout):
    ids = {}
    for k, op in enumerate(plan.ops):
        if isinstance(op, Sync):
            print(f"{k} {type(op).__name__}({op.src}, {op.dst})", file=out)
            continue
        args = " ".join(_fmt(a, ids) for a in op.args)
        meta = " ".join(f"{key}={_fmt(op.meta[key], ids)}" for key in sorted(op.meta))
        print(f"{k} launch {op.name} sid={op.sid} | {args} | {meta}", file=out)


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    for backbone, C, S, N in SHAPES:
        torch.manual_seed(0)
        m = KRRN(cfg=make_config(num_cls=C, backbone=backbone))
        init_weights(m, 0)
        m.eval()
        kp = KRRNPlan(m, B, S, N, True, torch.device("cpu"))
        print(f"== {backbone} C={C} B={B} S={S} N={N}: {len(kp.plan.ops)} ops")
        dump(kp.plan)


if __name__ == "__main__":
    main()
