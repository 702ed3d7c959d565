#!/usr/bin/env python3
"""Diagnostic: what a kept draw costs when its moments are formed on the device (bb_hmc_accum_add, csrc/bb_hmc_accum.h) against what a
user of the session had to do without it -- download the walkers' positions (bb_hmc_get) and take a Welford step of W x D in numpy -- on
C2 (synth.fitness_normal(50 000, 8)) at W = 8 and 64 walkers; also bb_hmc_accum_stats at 2 segments and, for scale, one transition of 16
leapfrogs.
   python tools/hmc_accum_rate.py [--out DIR] [--runs N] [--draws K] [--only-device W]
Every call is synchronous, so a host clock around them times everything a sampler would wait for.  After a warm-up the two sides are
timed in alternating order, `--runs` times each.  `--only-device W`: one transition of 8 leapfrogs, a few adds and one statistics call at
W walkers and nothing else, for a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/hmc_accum_rate.py --only-device 64)."""
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

EPS = 1e-4          # small enough that no trajectory diverges: the times do not depend on it


def host_draws(e, draws, W, D):
    """Per kept draw: bb_hmc_get, then the Welford step of csrc/bb_hmc_accum.h on [W, D] in numpy."""
    mean, m2 = np.zeros((W, D)), np.zeros((W, D))
    t0 = time.perf_counter()
    for n in range(1, draws + 1):
        x, _ = e.hmc_get()
        d = x - mean
        mean += d * (1.0 / n)
        m2 += d * (x - mean)
    return (time.perf_counter() - t0) / draws


def device_draws(e, draws):
    t0 = time.perf_counter()
    for _ in range(draws):
        e.hmc_accum_add(0)
    return (time.perf_counter() - t0) / draws


def timed(f, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        f()
    return (time.perf_counter() - t0) / reps


def headline(lib, runs, draws, only_device=0):
    w = synth.fitness_normal()
    res = {}
    with bb.Engine(w.kind, w.counts, w.n_neutral, w.n_bc, seed=1, _lib=lib) as e:
        e.run(200)
        mean, sigma = e.posterior()
        minv = sigma ** 2
        g = np.random.default_rng(4)
        for W in ((only_device,) if only_device else (8, 64)):
            Z = mean + 0.1 * sigma * g.standard_normal((W, e.D))
            with e.hmc_begin(Z, seed=1, inv_mass=minv):
                e.hmc_accum_begin(2)
                e.hmc_step(0, EPS, 1 if not only_device else 8, -np.inf)      # warm-up: code objects
                for s in (0, 0, 1, 1):
                    e.hmc_accum_add(s)
                e.hmc_accum_stats()
                if only_device:
                    for _ in range(8):
                        e.hmc_accum_add(0)
                    return {"D": e.D, "W": W}
                host, dev = [], []
                for r in range(runs):
                    for side in (("device", "host") if r % 2 == 0 else ("host", "device")):
                        if side == "device":
                            dev.append(device_draws(e, 4 * draws))
                        else:
                            host.append(host_draws(e, draws, W, e.D))
                stats = [timed(e.hmc_accum_stats, 3) for _ in range(runs)]
                step = [timed(lambda: e.hmc_step(1, EPS, 16, -np.inf), 1) for _ in range(runs)]
            res[f"W{W}"] = {"host_get_welford_s_per_draw": host, "device_accum_add_s_per_draw": dev, "accum_stats_s": stats,
                            "transition_16_leapfrogs_s": step, "host_median": float(np.median(host)), "device_median": float(np.median(dev)),
                            "ratio_of_medians": float(np.median(host) / np.median(dev)), "stats_median": float(np.median(stats)),
                            "transition_median": float(np.median(step))}
        res["D"] = e.D
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--draws", type=int, default=3)
    ap.add_argument("--only-device", type=int, default=0)
    a = ap.parse_args()
    libpath = os.environ.get("LIB") or _capi.LIB_PATH
    lib = _capi.load_library(libpath)
    if a.only_device:
        print(json.dumps(headline(lib, 1, a.draws, a.only_device)), flush=True)
        return
    res = {"lib": os.path.relpath(libpath, ROOT), "runs": a.runs, "draws": a.draws, "version": lib.bb_version().decode()}
    res["fitness_normal_50000x8"] = headline(lib, a.runs, a.draws)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "hmc_accum_rate.json"), "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
