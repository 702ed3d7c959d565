#!/usr/bin/env python3
"""Diagnostic: gradients per second of the log-density service an ensemble sampler uses -- bb_logdensity_grad called in a loop (one
point per call) against bb_logdensity_grad_batch at W = 1, 4, 16, 64 -- on data001_single (the reference's 20-barcode fixture) and on
C2 (synth.fitness_normal(50 000, 8)); then the wall time of mcmc_sample with 8 walkers x 50 steps on data001_single, "serial" against
"batched".
   python tools/logp_batch_time.py [--out DIR] [--runs N] [--window SECONDS]
Both calls are synchronous (they end in a download), so a host clock around them times upload, launches and download.  After a
warm-up of every variant the variants are timed in alternating order (forwards, then backwards, ...), `--runs` windows each; a window
repeats the call until `--window` seconds have passed.  Reported per variant: the windows' gradients/s, their median, min and max."""
import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import barbay_jl_amd as bb  # noqa: E402
from barbay_jl_amd import _capi, synth  # noqa: E402

BATCHES = (1, 4, 16, 64)


def window(f, points_per_call, seconds):
    n, t0 = 0, time.perf_counter()
    while True:
        f()
        n += 1
        t = time.perf_counter() - t0
        if t >= seconds:
            return n * points_per_call / t


def rates(e, runs, seconds):
    g = np.random.default_rng(4)
    mean, sigma = e.posterior()
    Z = mean + 0.1 * sigma * g.standard_normal((max(BATCHES), e.D))
    variants = {"single_loop": (lambda: e.logdensity_grad(Z[0]), 1)}
    for W in BATCHES:
        variants[f"batch_W{W}"] = (lambda W=W: e.logdensity_grad_batch(Z[:W]), W)
    lp1, g1 = e.logdensity_grad(Z[0])
    lpb, gb = e.logdensity_grad_batch(Z)
    agree = {"logp_rel": float(abs(lpb[0] - lp1) / abs(lp1)), "grad_rel_to_max": float(np.abs(gb[0] - g1).max() / np.abs(g1).max())}
    for f, _ in variants.values():                                # warm-up: code objects, the handle's buffers at every size
        f()
        f()
    got = {k: [] for k in variants}
    for r in range(runs):
        order = list(variants) if r % 2 == 0 else list(variants)[::-1]
        for k in order:
            f, n = variants[k]
            got[k].append(window(f, n, seconds))
    out = {k: {"grads_per_s": v, "median": float(np.median(v)), "min": min(v), "max": max(v)} for k, v in got.items()}
    return {"D": e.D, "batch_agrees_with_single": agree, "rates": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    a = ap.parse_args()
    libpath = os.environ.get("LIB") or _capi.LIB_PATH
    lib = _capi.load_library(libpath)
    res = {"lib": os.path.relpath(libpath, ROOT), "runs": a.runs, "window_s": a.window, "version": lib.bb_version().decode()}

    df = pd.read_csv(os.path.join(ROOT, "tests", "golden", "data001_single.csv"))
    arr = bb.utils.data_to_arrays(df)
    model = bb.model.fitness_normal(arr.bc_count, arr.bc_total, arr.n_neutral, arr.n_bc)
    with bb.vi.make_engine(model, bb.vi.ADVI(1, 500), bb.vi.TruncatedADAGrad(), 3, 0, _lib=lib) as e:
        e.run(500)
        res["data001_single"] = rates(e, a.runs, a.window)
    w = synth.fitness_normal(50_000, 8)
    with bb.Engine(w.kind, w.counts, w.n_neutral, w.n_bc, seed=1, _lib=lib) as e:
        e.run(200)
        res["fitness_normal_50000x8"] = rates(e, a.runs, a.window)

    kw = dict(data=df, n_walkers=8, n_steps=50, outputname=None, model=bb.model.fitness_normal, advi_steps=500, verbose=False, seed=3,
              engine_kwargs={"_lib": lib})
    wall = {"serial": [], "batched": []}
    bb.mcmc.mcmc_sample(**{**kw, "n_walkers": 2, "n_steps": 4}, ensemble="batched")      # warm-up
    for r in range(a.runs):
        for k in (("serial", "batched") if r % 2 == 0 else ("batched", "serial")):
            t0 = time.perf_counter()
            out = bb.mcmc.mcmc_sample(**kw, ensemble=k)
            wall[k].append(time.perf_counter() - t0)
            assert np.isfinite(out["logp"]).all()
    res["mcmc_sample_8x50_data001_single"] = {k: {"seconds": v, "median": float(np.median(v)), "min": min(v), "max": max(v)}
                                              for k, v in wall.items()}
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "logp_batch_time.json"), "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
