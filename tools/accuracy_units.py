"""Records what tests/_accuracy_cases.py measures into profiles/accuracy/units.json.

    python tools/accuracy_units.py emulation          the host emulation (CPU)
    python tools/accuracy_units.py device [out.json]  the HIP library on the GPU (out.json: write the merged table there instead)
    python tools/accuracy_units.py yardsticks         the trajectory yardsticks (CPU): the literal oracle's ADVI loop against the
                                                      C port's from the posterior-like start, on the engine's own draws; also
                                                      written to tests/golden/accuracy_trajectories.json, which the tests read

    python tools/accuracy_units.py resident_emulation [commit|parent LIB]     the gradient inside the resident launches
    python tools/accuracy_units.py resident_device [commit|parent LIB] [out.json]   (tests/_accuracy_cases.py, resident_measure), emulation / GPU;
                                                      "parent LIB": the same probe on another build's library (the parent
                                                      commit's libbb_emu.so / libbarbay_hip.so), recorded beside this commit's

units.json: target -> "units": rows [case, geometry, point, quantity, block, oracle units, engine units, bound, entry point of the
engine's worst, max-norm figure]; "trajectories": name_S -> mode -> [max|dmu|, max|domega|] against the literal oracle's loop.
"resident_emulation" / "resident_device": "parent" and "commit" -> one row per kernel and model kind, [kernel<kind, quantity, asserted by the
tests, measured rows, {block: rows over their bound}, then the row nearest its bound: case, config, S, point, block, oracle units, engine
units, bound].
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


def resident(lib, device):
    groups = {}
    for case, config in a.resident_cases(device):
        for r in a.resident_measure(lib, case, config, device):
            key = (r["kernel"].replace("emu:", "").split(",")[0], r["quantity"], r["asserted"])
            g = groups.setdefault(key, dict(n=0, over={}, worst=None))
            g["n"] += 1
            if not r["engine"] <= a.bound(r["oracle"]):
                g["over"][r["block"]] = g["over"].get(r["block"], 0) + 1
            if g["worst"] is None or r["engine"] / a.bound(r["oracle"]) > g["worst"][6] / g["worst"][7]:
                g["worst"] = [case, config, r["S"], r["point"], r["block"], round(r["oracle"], 3), round(r["engine"], 3), round(a.bound(r["oracle"]), 3)]
    print(sum(g["n"] for g in groups.values()), "rows,", sum(sum(g["over"].values()) for k, g in groups.items() if k[2]), "asserted rows over their bound")
    return [list(k) + [g["n"], g["over"]] + g["worst"] for k, g in sorted(groups.items())]


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


def main(what, *rest):
    out = OUT
    if what.startswith("resident_"):
        which, path = "commit", None
        if rest and rest[0] in ("commit", "parent"):
            which, rest = rest[0], rest[1:]
            if which == "parent":
                path, rest = rest[0], rest[1:]
        out = rest[0] if rest else OUT
        if what == "resident_emulation":
            lib = _capi._declare(ctypes.CDLL(path)) if path else emu()
        else:
            lib = _capi._declare(ctypes.CDLL(path)) if path else _capi.load_library()
        doc = json.load(open(out if os.path.exists(out) else OUT))          # (a second run into the same out.json adds to the first)
        doc.setdefault(what, {})[which] = resident(lib, what == "resident_device")
        rest = ()
    elif what == "yardsticks":
        doc = json.load(open(OUT)) if os.path.exists(OUT) else {}
        y = yardsticks()
        with open(a.YARDSTICKS, "w") as f:
            json.dump(y, f, indent=1, sort_keys=True)
            f.write("\n")
        doc["trajectory_yardsticks"] = y
    else:
        out = rest[0] if rest else OUT
        doc = json.load(open(OUT)) if os.path.exists(OUT) else {}
        lib = emu() if what == "emulation" else _capi.load_library()
        doc[what] = dict(units=units(lib), trajectories=trajectories(lib))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("{\n" + ",\n".join(
            f' {json.dumps(k)}: ' + (json.dumps(v, sort_keys=True) if k == "trajectory_yardsticks" else
                                    "{" + ",\n  ".join(f'{json.dumps(w)}: [\n   ' + ",\n   ".join(json.dumps(r) for r in rr) + "]"
                                                        for w, rr in sorted(v.items())) + "}" if k.startswith("resident_") else
                                    '{"trajectories": ' + json.dumps(v["trajectories"], sort_keys=True) + ',\n  "units": [\n   ' +
                                    ",\n   ".join(json.dumps(r) for r in v["units"]) + "]}")
            for k, v in sorted(doc.items())) + "\n}\n")


if __name__ == "__main__":
    main(*sys.argv[1:])
