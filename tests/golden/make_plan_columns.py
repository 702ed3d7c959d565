"""Record a column of the plan table (tests/_plan_cases.py): what a library does with every row, refusal messages as anchored
regular expressions.  The library must be one built from a commit whose planner is trusted -- the columns in this directory came
from the commit before the planner moved into csrc/bb_plan.h -- never the one under test.
    python tests/golden/make_plan_columns.py emu PATH/libbb_emu.so tests/golden/plan_emu.json
    python tests/golden/make_plan_columns.py gpu PATH/libbarbay_hip.so tests/golden/plan_gpu.json      (on an MI355X)"""
import ctypes
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from barbay_jl_amd import _capi  # noqa: E402
import _plan_cases as pc  # noqa: E402


def main(which, libpath, out):
    lib = _capi._declare(ctypes.CDLL(libpath)) if which == "emu" else _capi.load_library(libpath)
    rx = lambda x: [x[0], "^" + re.escape(x[1]) + "$"]
    res = {}
    for name in pc.rows_for(gpu=which == "gpu"):
        keys = []
        try:
            got = pc.observe(lib, name, lambda k, v: (keys.append(k), os.environ.__setitem__(k, v)))
        finally:
            for k in keys:
                os.environ.pop(k, None)
        if "refused" in got:
            got["refused"] = rx(got["refused"])
        if "enable" in got:
            got["enable"] = [g if g is True else rx(g) for g in got["enable"]]
        res[name] = got
    with open(out, "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in res.items()) + "\n}\n")


if __name__ == "__main__":
    main(*sys.argv[1:4])
