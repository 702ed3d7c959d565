#!/usr/bin/env python3
"""Diagnostic: leapfrogs per second of the device-resident HMC session (bb_hmc_step, csrc/bb_hmc.h) against the host-driven way --
`mcmc._leapfrog`'s arithmetic in numpy around bb_logdensity_grad_batch, what `nuts_ensemble` pays per round -- on C2
(synth.fitness_normal(50 000, 8)) at W = 8 and 64 walkers, the same number of leapfrogs on both sides; then, on data001_single, the
smallest effective sample size per gradient evaluation of `hmc_ensemble` against `nuts_ensemble` through bb_chain_summary.
   python tools/hmc_rate.py [--out DIR] [--runs N] [--leapfrogs L] [--only-device W]
Both sides are synchronous (every call ends in a download), so a host clock around them times everything a sampler would wait for.
After a warm-up the two sides are timed in alternating order, `--runs` times each.  `--only-device W`: nothing but a few device
transitions at W walkers, for a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/hmc_rate.py --only-device 64)."""
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

EPS = 1e-4          # small enough that no trajectory diverges: the rate does not depend on it


def device_leapfrogs(e, Z, minv, L, transitions):
    with e.hmc_begin(Z, seed=1, inv_mass=minv):
        e.hmc_step(0, EPS, L, -np.inf)                            # warm-up: code objects
        t0 = time.perf_counter()
        for m in range(transitions):
            r = e.hmc_step(1 + m, EPS, L, -np.inf)
        t = time.perf_counter() - t0
        assert np.isfinite(r["h1"]).all()
    return len(Z) * L * transitions / t


def host_leapfrogs(e, Z, minv, L):
    """`mcmc._leapfrog` for all walkers at once: z, r, g in numpy, one bb_logdensity_grad_batch per leapfrog."""
    lp, g = e.logdensity_grad_batch(Z)
    r = np.random.default_rng(2).standard_normal(Z.shape) / np.sqrt(minv)
    z = Z
    t0 = time.perf_counter()
    for _ in range(L):
        r = r + 0.5 * EPS * g
        z = z + EPS * minv * r
        lp, g = e.logdensity_grad_batch(z)
        r = r + 0.5 * EPS * g
    h = lp - 0.5 * np.einsum("wd,d,wd->w", r, minv, r)
    t = time.perf_counter() - t0
    assert np.isfinite(h).all()
    return len(Z) * L / t


def headline(lib, runs, L, only_device=0):
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
                return {"D": e.D, "W": W, "device_leapfrogs_per_s": device_leapfrogs(e, Z, minv, L, 3)}
            dev, host = [], []
            for r in range(runs):
                for side in (("device", "host") if r % 2 == 0 else ("host", "device")):
                    if side == "device":
                        dev.append(device_leapfrogs(e, Z, minv, L, 3))
                    else:
                        host.append(host_leapfrogs(e, Z, minv, L))
            res[f"W{W}"] = {"device_leapfrogs_per_s": dev, "host_leapfrogs_per_s": host,
                            "device_median": float(np.median(dev)), "host_median": float(np.median(host)),
                            "ratio_of_medians": float(np.median(dev) / np.median(host))}
        res["D"] = e.D
    return res


def ess_per_gradient(lib, n_walkers=4, n_steps=1000, n_adapt=500, advi_steps=3000, seed=3):
    df = pd.read_csv(os.path.join(ROOT, "tests", "golden", "data001_single.csv"))
    arr = bb.utils.data_to_arrays(df)
    model = bb.model.fitness_normal(arr.bc_count, arr.bc_total, arr.n_neutral, arr.n_bc)
    out = {}
    with bb.vi.make_engine(model, bb.vi.ADVI(1, advi_steps), bb.vi.TruncatedADAGrad(), seed, 0, _lib=lib) as e:
        e.run(advi_steps)
        mean, sigma = e.posterior()
        minv = sigma ** 2
        for name in ("hmc", "nuts"):
            rngs = [np.random.default_rng([seed, w]) for w in range(n_walkers)]
            z0s = [mean + sigma * r.standard_normal(e.D) * 0.1 for r in rngs]
            t0 = time.perf_counter()
            if name == "hmc":
                res = bb.mcmc.hmc_ensemble(e, z0s, n_steps, n_adapt, rngs=rngs, minv=minv, seed=seed)
            else:
                res = bb.mcmc.nuts_ensemble(e.logdensity_grad_batch, z0s, n_steps, n_adapt, rngs=rngs, minv=minv)
            t = time.perf_counter() - t0
            s = e.chain_summary(np.stack([r[0] for r in res]), (0.5,))
            n_grad = int(sum(r[2]["n_grad"] for r in res))
            out[name] = {"seconds": t, "n_grad": n_grad, "min_ess": float(s["ess"].min()), "max_rhat": float(s["rhat"].max()),
                         "min_ess_per_gradient": float(s["ess"].min() / n_grad), "min_ess_per_second": float(s["ess"].min() / t),
                         "step_size": [r[2]["step_size"] for r in res]}
            if name == "hmc":
                out[name].update(accept_rate=[r[2]["accept_rate"] for r in res], divergences=[r[2]["divergences"] for r in res])
    out["settings"] = dict(n_walkers=n_walkers, n_steps=n_steps, n_adapt=n_adapt, advi_steps=advi_steps, seed=seed, D=int(mean.shape[0]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--leapfrogs", type=int, default=8)
    ap.add_argument("--only-device", type=int, default=0)
    a = ap.parse_args()
    libpath = os.environ.get("LIB") or _capi.LIB_PATH
    lib = _capi.load_library(libpath)
    if a.only_device:
        print(json.dumps(headline(lib, 1, a.leapfrogs, a.only_device)), flush=True)
        return
    res = {"lib": os.path.relpath(libpath, ROOT), "runs": a.runs, "leapfrogs": a.leapfrogs, "version": lib.bb_version().decode()}
    res["fitness_normal_50000x8"] = headline(lib, a.runs, a.leapfrogs)
    print(json.dumps(res), flush=True)
    res["data001_single"] = ess_per_gradient(lib)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "hmc_rate.json"), "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
