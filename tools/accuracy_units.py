"""Records what tests/_accuracy_cases.py measures into profiles/accuracy/units.json.

    python tools/accuracy_units.py emulation          the host emulation (CPU)
    python tools/accuracy_units.py device [out.json]  the HIP library on the GPU (out.json: write the merged table there instead)
    python tools/accuracy_units.py yardsticks         the trajectory yardsticks (CPU): the literal oracle's ADVI loop against the
                                                      C port's from the posterior-like start, on the engine's own draws; also
                                                      written to tests/golden/accuracy_trajectories.json, which the tests read

units.json: target -> "units": rows [case, geometry, point, quantity, block, oracle units, engine units, bound, entry point of the
engine's worst, max-norm figure]; "trajectories": name_S -> mode -> [max|dmu|, max|domega|] against the literal oracle's loop.
Unlike the tests this asserts nothing: a figure over its bound is recorded as it is.
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

import __graft_entry__ as g  # noqa: E402
import _accuracy_cases as a  # noqa: E402
from barbay_jl_amd import _capi  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "accuracy", "units.json")


def setenv(env):
    for k in ("BB_TUNE_NB", "BB_TUNE_NTHR", "BB_TUNE_STREAM"):
        os.environ.pop(k, None)
    os.environ.update(env)


def emu():
    return _capi._declare(ctypes.CDLL(g.build_emu()))


def units(lib):
    rows = []
    for case in a.CASES:
        for geom, env in a.GEOMETRIES.items():
            setenv(env)
            for r in a.measure(lib, case):
                rows.append([case, geom, r["point"], r["quantity"], r["block"], round(r["oracle"], 3), round(r["engine"], 3),
                             round(a.bound(r["oracle"]), 3), r["entry"], float(f"{r['rel']:.3e}")])
        print(case, flush=True)
    return rows


def trajectories(lib):
    out = {}
    for name in a.TRAJ:
        setenv(a.TRAJ[name][1])
        for S in (1, 2):
            res = {}
            for mode in (1, 2):
                mu, om, kn, eps = a.traj_run(lib, name, S, mode)
                if mode == 1:
                    m2, o2 = a.traj_oracle(name, S, eps)
                res[f"mode{mode}"] = [float(np.abs(mu - m2).max()), float(np.abs(om - o2).max())]
            res["kernel"] = kn
            out[f"{name}_S{S}"] = res
            print(name, S, res, flush=True)
    return out


def yardsticks():
    lib = emu()
    out = {}
    for name in a.TRAJ:
        setenv(a.TRAJ[name][1])
        for S in (1, 2):
            _, _, _, eps = a.traj_run(lib, name, S, 1)            # (the engine only supplies its draws in the caller's order)
            m1, o1 = a.traj_oracle(name, S, eps, "literal")
            m2, o2 = a.traj_oracle(name, S, eps, "port")
            out[f"{name}_S{S}"] = dict(dmu=float(np.abs(m1 - m2).max()), domega=float(np.abs(o1 - o2).max()))
            print(name, S, out[f"{name}_S{S}"], flush=True)
    return out


def main(what, out=OUT):
    doc = json.load(open(OUT)) if os.path.exists(OUT) else {}
    if what == "yardsticks":
        y = yardsticks()
        with open(a.YARDSTICKS, "w") as f:
            json.dump(y, f, indent=1, sort_keys=True)
            f.write("\n")
        doc["trajectory_yardsticks"] = y
    else:
        lib = emu() if what == "emulation" else _capi.load_library()
        doc[what] = dict(units=units(lib), trajectories=trajectories(lib))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("{\n" + ",\n".join(
            f' {json.dumps(k)}: ' + (json.dumps(v, sort_keys=True) if k == "trajectory_yardsticks" else
                                    '{"trajectories": ' + json.dumps(v["trajectories"], sort_keys=True) + ',\n  "units": [\n   ' +
                                    ",\n   ".join(json.dumps(r) for r in v["units"]) + "]}")
            for k, v in sorted(doc.items())) + "\n}\n")


if __name__ == "__main__":
    main(*sys.argv[1:3])
