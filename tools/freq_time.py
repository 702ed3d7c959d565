#!/usr/bin/env python3
"""Diagnostic: time bb_freq_bands (frequency-trajectory bands, barbay.jl_amd/csrc/bb_freq.h) on C2 (fitness_normal, 50 000 x 8) at
K = 10 000, three quantiles, in both modes, and bb_ppc_bands in the same process for scale.
   python tools/freq_time.py [--out DIR] [--reps N]
Per call: wall time of the (synchronous) call without the host count of observations outside the band -- parameter upload, the
launches, the bands' download -- and the kernels' registers and spills from the code object (tools/kernel_resources.py).  The kernels'
own durations (the normaliser's share: k_freq_zpart + k_freq_zsum against k_freq) come from a
rocprofv3 --kernel-trace --stats run of this script."""
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


def resources(lib):
    out = {}
    for pat in ("k_freq", "k_ppc"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), pat], capture_output=True, text=True,
                           env={**os.environ, "LIB": lib})
        for line in r.stdout.splitlines():
            f = line.split()
            if f and f[0] in ("k_freq", "k_freq_zpart", "k_freq_zsum", "k_ppc", "k_ppc_pop"):
                out[f[0]] = {"vgpr": int(f[2]), "spilled": int(f[4]), "sgpr": int(f[6]), "scratch_B": int(f[8])}
    return out


def best(f, reps):
    f()                                                          # warm-up: code object, buffers
    ts = []
    for i in range(reps):
        t0 = time.perf_counter()
        f(i)
        ts.append(time.perf_counter() - t0)
    return {"ms_min": 1e3 * min(ts), "ms_median": 1e3 * float(np.median(ts))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    libpath = os.environ.get("LIB") or _capi.LIB_PATH
    lib = _capi.load_library(libpath)
    res = {"lib": os.path.relpath(libpath, ROOT), "quantiles": QS, "resources": resources(libpath)}
    w = synth.fitness_normal()
    with bb.Engine(w.kind, w.counts, w.n_neutral, w.n_bc, seed=1, _lib=lib) as e:
        res["freq_shape"], res["ppc_shape"] = e.freq_shape(), e.ppc_shape()
        res["ppc_bands"] = best(lambda i=0: e.ppc_bands(QS, 1000, 10, seed=i, outside=False), a.reps)
        res["freq_trajectory"] = best(lambda i=0: e.freq_bands(QS, "trajectory", 1000, 10, seed=i, outside=False), a.reps)
        res["freq_posterior"] = best(lambda i=0: e.freq_bands(QS, "posterior", 10_000, 1, seed=i, outside=False), a.reps)
        t0 = time.perf_counter()
        e.freq_bands(QS, "trajectory", 1000, 10, seed=0, outside=True)
        res["freq_trajectory_with_outside_ms"] = 1e3 * (time.perf_counter() - t0)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "freq_time.json"), "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
