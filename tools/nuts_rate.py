#!/usr/bin/env python3
"""Diagnostic: what a leaf of the device-resident NUTS tree costs (bb_nuts_leaf, csrc/bb_nuts.h) on C2 (synth.fitness_normal(50 000, 8))
at W = 8 and 64 walkers, in one job:
  - leaves per second of `mcmc.nuts_device` (walkers idling behind the deepest tree are not counted: leaves are the evaluations made),
    in the same short run as the host-driven side (a few transitions from the probes' step size: shallow trees, and every kept draw is
    downloaded), and once in a longer run of its own that keeps no chain (`--long-adapt` + `--long-steps` transitions, segments=1,
    keep_chain=False): the step size adapted, trees of the depth a sampler sees, nothing of size D on the host link;
  - leaves per second of bb_nuts_leaf alone, all walkers busy, over doublings of 1, 2, 4, 8 leaves with the driver's ops and a take after
    every second leaf;
  - leapfrogs per second of `mcmc.nuts_ensemble` on bb_logdensity_grad_batch, the host-driven NUTS;
  - leapfrogs per second of bb_hmc_step.
   python tools/nuts_rate.py [--out DIR] [--runs N] [--steps N] [--adapt N] [--long-steps N] [--long-adapt N] [--only-device W]
Every side is synchronous (each call ends in a download), so a host clock around them times everything a sampler would wait for.  After a
warm-up the sides are timed in alternating order, `--runs` times each.  `--only-device W`: nothing but a few doublings of bb_nuts_leaf and
one bb_hmc_step at W walkers, for a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/nuts_rate.py --only-device 64)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import barbay_jl_amd as bb  # noqa: E402
from barbay_jl_amd import _capi, synth  # noqa: E402

EPS = 1e-4          # the raw sides: small enough that no trajectory diverges, the rate does not depend on it
DEPTH = 6           # of both samplers: 5.6 GB of rows at W = 64
TAKE_ALL = _capi.BB_NUTS_TAKE_LEAF | _capi.BB_NUTS_TAKE_SUB | _capi.BB_NUTS_TAKE_STATE


def raw_leaves(e, Z, minv, trees=2):
    """bb_nuts_leaf alone: per tree, doublings j = 0 .. 3 in direction +1, every walker busy; a take of the leaf after every second leaf
    and of the state at the tree's end."""
    W = len(Z)
    with e.hmc_begin(Z, seed=1, inv_mass=minv):
        e.nuts_begin(DEPTH)
        n = 0
        for tree in range(trees + 1):                             # (the first: warm-up, code objects)
            if tree == 1:
                n, t0 = 0, time.perf_counter()
            e.nuts_start(1 + tree, EPS)
            for j in range(4):
                for i in range(1 << j):
                    store, checks = bb.mcmc.nuts_leaf_op(i, j)
                    r = e.nuts_leaf(1, i == 0, i == (1 << j) - 1, store, [checks] * W)
                    n += W
                    if i & 1:
                        e.nuts_take(_capi.BB_NUTS_TAKE_LEAF)
            e.nuts_take(TAKE_ALL)
        t = time.perf_counter() - t0
        assert np.isfinite(r["logp_leaf"]).all() and np.isfinite(r["kinetic"]).all()
    return n / t


def hmc_leapfrogs(e, Z, minv, L=8, transitions=3):
    with e.hmc_begin(Z, seed=1, inv_mass=minv):
        e.hmc_step(0, EPS, L, -np.inf)
        t0 = time.perf_counter()
        for m in range(transitions):
            r = e.hmc_step(1 + m, EPS, L, -np.inf)
        t = time.perf_counter() - t0
        assert np.isfinite(r["h1"]).all()
    return len(Z) * L * transitions / t


def device_long(e, Z, minv, n_steps, n_adapt):
    """nuts_device alone, no chain kept: (leaves per second, mean tree depth, seconds)."""
    rngs = [np.random.default_rng([7, w]) for w in range(len(Z))]
    t0 = time.perf_counter()
    res = bb.mcmc.nuts_device(e, list(Z), n_steps, n_adapt, rngs=rngs, minv=minv, max_depth=DEPTH, seed=1, segments=1, keep_chain=False)
    t = time.perf_counter() - t0
    return sum(r[2]["n_grad"] for r in res) / t, float(np.mean([r[2]["mean_tree_depth"] for r in res])), t


def sampler(e, Z, minv, which, n_steps, n_adapt):
    """(evaluations per second, mean tree depth) of a short run of either sampler from the same starts; the start step size's probes
    are counted on both sides (they are evaluations too)."""
    W = len(Z)
    rngs = [np.random.default_rng([7, w]) for w in range(W)]
    t0 = time.perf_counter()
    if which == "device":
        res = bb.mcmc.nuts_device(e, list(Z), n_steps, n_adapt, rngs=rngs, minv=minv, max_depth=DEPTH, seed=1)
    else:
        res = bb.mcmc.nuts_ensemble(e.logdensity_grad_batch, list(Z), n_steps, n_adapt, rngs=rngs, minv=minv, max_depth=DEPTH)
    t = time.perf_counter() - t0
    assert all(np.isfinite(r[1]).all() for r in res)
    return sum(r[2]["n_grad"] for r in res) / t, float(np.mean([r[2]["mean_tree_depth"] for r in res]))


def headline(lib, runs, n_steps, n_adapt, only_device=0, long_steps=10, long_adapt=30):
    w = synth.fitness_normal()
    res = {}
    with bb.Engine(w.kind, w.counts, w.n_neutral, w.n_bc, seed=1, _lib=lib) as e:
        e.run(200)
        mean, sigma = e.posterior()
        minv = sigma ** 2
        g = np.random.default_rng(4)
        for W in ((only_device,) if only_device else (8, 64)):
            Z = mean + 0.1 * sigma * g.standard_normal((W, e.D))
            if only_device:
                return {"D": e.D, "W": W, "raw_leaves_per_s": raw_leaves(e, Z, minv, 1), "hmc_leapfrogs_per_s": hmc_leapfrogs(e, Z, minv, 8, 1)}
            rows = {k: [] for k in ("nuts_device", "nuts_leaf_raw", "nuts_ensemble_host", "hmc_step")}
            depth = {"nuts_device": [], "nuts_ensemble_host": []}
            raw_leaves(e, Z, minv, 1)                              # warm-up of every code object
            for r in range(runs):
                order = ("nuts_device", "nuts_leaf_raw", "nuts_ensemble_host", "hmc_step")
                for side in (order if r % 2 == 0 else order[::-1]):
                    if side == "nuts_device":
                        v, d = sampler(e, Z, minv, "device", n_steps, n_adapt)
                        depth[side].append(d)
                    elif side == "nuts_ensemble_host":
                        v, d = sampler(e, Z, minv, "host", n_steps, n_adapt)
                        depth[side].append(d)
                    elif side == "nuts_leaf_raw":
                        v = raw_leaves(e, Z, minv)
                    else:
                        v = hmc_leapfrogs(e, Z, minv)
                    rows[side].append(v)
            med = {k: float(np.median(v)) for k, v in rows.items()}
            res[f"W{W}"] = {"per_s": rows, "median_per_s": med, "mean_tree_depth": depth,
                            "device_over_host": med["nuts_device"] / med["nuts_ensemble_host"],
                            "raw_leaf_over_host": med["nuts_leaf_raw"] / med["nuts_ensemble_host"],
                            "leaf_time_over_hmc_leapfrog_time": med["hmc_step"] / med["nuts_leaf_raw"],
                            "driver_leaf_time_over_hmc_leapfrog_time": med["hmc_step"] / med["nuts_device"]}
            v, d, t = device_long(e, Z, minv, long_steps, long_adapt)
            res[f"W{W}"]["nuts_device_no_chain"] = {"leaves_per_s": v, "mean_tree_depth": d, "seconds": t, "n_steps": long_steps, "n_adapt": long_adapt,
                                                   "leaf_time_over_hmc_leapfrog_time": med["hmc_step"] / v}
            print(json.dumps({f"W{W}": res[f"W{W}"]}), flush=True)
        res["D"] = e.D
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--adapt", type=int, default=3)
    ap.add_argument("--long-steps", type=int, default=10)
    ap.add_argument("--long-adapt", type=int, default=30)
    ap.add_argument("--only-device", type=int, default=0)
    a = ap.parse_args()
    libpath = os.environ.get("LIB") or _capi.LIB_PATH
    lib = _capi.load_library(libpath)
    if a.only_device:
        print(json.dumps(headline(lib, 1, a.steps, a.adapt, a.only_device)), flush=True)
        return
    res = {"lib": os.path.relpath(libpath, ROOT), "runs": a.runs, "n_steps": a.steps, "n_adapt": a.adapt, "max_depth": DEPTH,
           "version": lib.bb_version().decode()}
    res["fitness_normal_50000x8"] = headline(lib, a.runs, a.steps, a.adapt, 0, a.long_steps, a.long_adapt)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "nuts_rate.json"), "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
