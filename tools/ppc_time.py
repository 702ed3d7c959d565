#!/usr/bin/env python3
"""Diagnostic: time bb_ppc_bands (posterior predictive bands, barbay.jl_amd/csrc/bb_ppc.h) on C2 (fitness_normal, 50 000 x 8)
and C5 (genotype_fitness_normal, 200 000 x 8) at K = n_samples n_ppc = 10 000, three quantiles.
   python tools/ppc_time.py [--out DIR] [--tag NAME] [--cases C2,C5] [--reps N] [--no-host]
   LIB=barbay.jl_amd/lib/ab/ppc_draw.so python tools/ppc_time.py --tag draw_only     the draw-only floor: the same kernel with the
                                                                                 selection compiled out (tools/xp.py build ppc_draw -DBB_PPC_DRAW_ONLY)
Per case: wall time of the (synchronous) call -- parameter upload, the two launches, the bands' download, and the host count of
observed ratios outside the widest band when asked for -- columns/s and predictive draws/s; k_ppc's registers and spills from the
code object (tools/kernel_resources.py); with the host leg, numpy's time for the same draws and quantiles on 200 rows, extrapolated.
The kernels' own durations come from a rocprofv3 --kernel-trace --stats run of this script."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import barbay_jl_amd as bb  # noqa: E402
from barbay_jl_amd import _capi, synth  # noqa: E402

QS = (0.95, 0.675, 0.05)
NS, NPPC = 1000, 10


def resources(lib):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "k_ppc"], capture_output=True, text=True,
                       env={**os.environ, "LIB": lib})
    out = {}
    for line in r.stdout.splitlines():
        f = line.split()
        if f and f[0] in ("k_ppc", "k_ppc_pop"):
            out[f[0]] = {"vgpr": int(f[2]), "spilled": int(f[4]), "sgpr": int(f[6]), "scratch_B": int(f[8])}
    return out


def host_numpy(n_rows, n_steps, rows=200):
    """numpy's time for the same work on `rows` rows: per row 4 parameter draws x n_samples, per step n_samples n_ppc predictive
    draws and the 2 x 3 quantiles of the column (np.quantile, method="linear" = StatsBase's type 7)."""
    g = np.random.default_rng(0)
    p = [x for q in QS for x in ((1 - q) / 2, 1 - (1 - q) / 2)]
    t0 = time.perf_counter()
    for _ in range(rows):
        s, ls, sbar, lsbar = g.normal(0.1, 0.05, (4, NS))
        for _t in range(n_steps):
            x = g.normal((s - sbar)[:, None], np.exp(ls)[:, None], (NS, NPPC))
            np.quantile(x.reshape(-1), p)
    dt = time.perf_counter() - t0
    return {"rows": rows, "s": dt, "extrapolated_s": dt * n_rows / rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="product")
    ap.add_argument("--cases", default="C2,C5")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    libpath = os.environ.get("LIB") or _capi.LIB_PATH
    lib = _capi.load_library(libpath)
    res = {"tag": a.tag, "lib": os.path.relpath(libpath, ROOT), "K": NS * NPPC, "n_samples": NS, "n_ppc": NPPC, "quantiles": QS,
           "resources": resources(libpath), "cases": {}}
    for name in a.cases.split(","):
        w = synth.fitness_normal() if name == "C2" else synth.genotype_fitness_normal()
        with bb.Engine(w.kind, w.counts, w.n_neutral, w.n_bc, env_idx=w.env_idx, geno_idx=w.geno_idx, seed=1, _lib=lib) as e:
            n_rows, n_steps = e.ppc_shape()
            e.ppc_bands(QS, NS, NPPC, seed=0)                    # warm-up: code object, buffers
            r = {"n_rows": n_rows, "n_steps": n_steps}
            for outside in (False, True):
                ts = []
                for i in range(a.reps):
                    t0 = time.perf_counter()
                    e.ppc_bands(QS, NS, NPPC, seed=i, outside=outside)
                    ts.append(time.perf_counter() - t0)
                key = "with_outside" if outside else "bands_only"
                best = min(ts)
                r[key] = {"ms_min": 1e3 * best, "ms_median": 1e3 * float(np.median(ts)),
                          "columns_per_s": n_rows * n_steps / best, "draws_per_s": n_rows * n_steps * NS * NPPC / best}
            if not a.no_host:
                r["host_numpy"] = host_numpy(n_rows, n_steps)
            res["cases"][name] = r
            print(name, json.dumps(r), flush=True)
    print(json.dumps(res["resources"]))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, f"ppc_time_{a.tag}.json"), "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
