#!/usr/bin/env python3
"""Diagnostic: time bb_dfe_rb (posterior of the fitness distribution of sets of units, barbay.jl_amd/csrc/bb_dfe.h) on C2
(fitness_normal 50 000 x 8) at n_samples = 1000, 32 grid points and three quantiles, for one set of all units and for one set per
1 000 units, phase by phase on the device, against numpy / scipy on the same box's CPUs.
   python tools/dfe_rate.py [--out DIR] [--reps N] [--host-units M] [--host-procs P]
   python tools/xp.py build rb_times -DBB_RB_TIMES      first, for the split: that build drains the stream after every phase and
                                                         prints map+upload / pop / normalisers / part / dfe / download to stderr
Prints: per layout of the sets the wall times of the (synchronous) call on the product library (one warm-up, then --reps calls:
min, median, max); with lib/ab/rb_times.so present, the phases of --phase-reps calls of that build after a warm-up (median, min
and max per phase; run in child processes, before this process opens the GPU); the host
yardstick: the header's formulas for --host-units units of the set of all units -- the draws (Philox as oracle.rng.pairs), the
conditionals, both tails through scipy's erfc at the 32 thresholds, the four sums -- on --host-procs processes, extrapolated to
the 50 000 units (the normalisers, common to every post-fit call and timed by tools/fitness_rb_rate.py, are left out: the
host's numbers are timed, not compared -- the tests compare).  The pool's processes are forked before this process opens the
GPU and are kept until the posterior is known: no process but this one (and, before it, one phase child at a time) ever holds
the device."""
import argparse
import json
import multiprocessing
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NS = 1000
NG = 32
SEED = 7
PROBS = (0.025, 0.5, 0.975)
AB = os.path.join(ROOT, "barbay.jl_amd", "lib", "ab", "rb_times.so")
LAYOUTS = ("one_set", "sets_of_1000")


def layouts(n_units):
    return {"one_set": [np.arange(n_units)], "sets_of_1000": [np.arange(lo, min(lo + 1000, n_units)) for lo in range(0, n_units, 1000)]}


def host_chunk(args):
    """(SL, SU, SV, SC) [NG, NS] of the mutants ms: fitness_rb_rate's conditionals, then the header's tails and sums."""
    from scipy.special import erfc
    from tools.fitness_rb_rate import host_draws
    mean, sigma, lay, T, nn, ms, logZ, sbar, grid = args
    k = len(ms)
    idx = (lay["loglambda"] + (nn + ms)[:, None] * T + np.arange(T)[None, :]).reshape(-1)
    ll = host_draws(mean, sigma, idx).reshape(k, T, NS)
    y = ((ll[:, 1:] - ll[:, :-1]) - (logZ[None, 1:] - logZ[None, :-1]) + sbar[None]).sum(axis=1)
    s = host_draws(mean, sigma, lay["s_bc"] + ms)
    w = np.exp(-2.0 * host_draws(mean, sigma, lay["logsigma_bc"] + ms))
    P = 0.25 + (T - 1) * w
    m, sd = w * y / P, 1.0 / np.sqrt(P)
    out = np.zeros((4, len(grid), NS))
    with np.errstate(all="ignore"):
        for g, x in enumerate(grid):
            v = (m - x) / sd * np.sqrt(0.5)
            pl, pu = 0.5 * erfc(v), 0.5 * erfc(-v)
            out[0, g], out[1, g], out[2, g], out[3, g] = pl.sum(0), pu.sum(0), (pl * pu).sum(0), (s <= x).sum(0)
    return out


def host_warm(_):
    """A pool process's imports, before any timing."""
    import scipy.special  # noqa: F401
    import tools.fitness_rb_rate  # noqa: F401
    return os.getpid()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-units", type=int, default=1600)
    ap.add_argument("--host-procs", type=int, default=16)
    ap.add_argument("--phase-reps", type=int, default=5)
    ap.add_argument("--phases-child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    phases = {}
    if not a.phases_child and os.path.exists(AB):              # the phase children first, one at a time: this process holds no GPU yet
        for name in LAYOUTS:
            c = subprocess.run([sys.executable, os.path.abspath(__file__), "--phases-child", name, "--phase-reps", str(a.phase_reps)], capture_output=True, text=True)
            lines = re.findall(r"\[bb_dfe_rb[^\n]*", c.stderr)[-a.phase_reps:]
            if c.returncode != 0 or len(lines) < a.phase_reps:
                raise RuntimeError("phase run failed:\n" + c.stderr[-2000:])
            per = [{kk: float(v) for kk, v in re.findall(r"(map\+upload|pop|normalisers|part|dfe|download) ([0-9.]+) ms", ln)} for ln in lines]
            phases[name] = {"phase_reps": a.phase_reps, "phases_line": lines[-1],
                            "phases_ms": {kk: {"median": float(np.median([q[kk] for q in per])), "min": min(q[kk] for q in per), "max": max(q[kk] for q in per)} for kk in per[0]}}
    pool = None
    procs = max(1, a.host_procs)
    if not a.phases_child:                                      # numpy's pool forks before this process opens the GPU
        pool = multiprocessing.Pool(procs)
        pool.map(host_warm, range(2 * procs))                   # imports, every process started
    import barbay_jl_amd as bb
    from barbay_jl_amd import _capi
    lib = _capi.load_library(AB if a.phases_child else None)
    w = bb.synth.fitness_normal()
    with bb.Engine(w.kind, w.counts, w.n_neutral, w.n_bc, seed=3, _lib=lib) as e:
        e.run(20)
        n_units = e.fitness_rb_shape()
        own = e.fitness_rb(n_samples=64, probs=(), seed=SEED)
        lo, hi = float((own["q_mean"] - 3 * own["q_sd"]).min()), float((own["q_mean"] + 3 * own["q_sd"]).max())
        grid = np.linspace(lo, hi, NG)
        sets = layouts(n_units)
        call = lambda name: e.dfe_rb(sets[name], grid, probs=PROBS, n_samples=NS, seed=SEED)
        e.dfe_rb(sets["sets_of_1000"][:2], grid, probs=PROBS, n_samples=64, seed=SEED)      # warm-up: code objects, buffers
        if a.phases_child:
            for _ in range(1 + a.phase_reps):                   # one warm-up at size, then the calls whose lines the parent reads
                call(a.phases_child)
            return
        res = {"workload": w.name, "n_samples": NS, "n_grid": NG, "n_quantiles": len(PROBS), "units": n_units, "layouts": {}}
        for name in LAYOUTS:
            r = call(name)                                             # warm-up at size: the buffer grows once
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                r = call(name)
                ts.append(time.perf_counter() - t0)
            cm = r["between_sd"] / r["within_sd"]
            res["layouts"][name] = {"n_sets": len(sets[name]), "reps": a.reps, "call_s_min": min(ts), "call_s_median": float(np.median(ts)), "call_s_max": max(ts),
                                    "erfc_per_s": 2.0 * n_units * NS * NG / min(ts),
                                    "common_mode_after_20_steps": {"median": float(np.median(cm)), "min": float(cm.min()), "max": float(cm.max())}}
            res["layouts"][name].update(phases.get(name, {}))
        mean, sigma = e.posterior()
        lay = {name: lo for name, lo, hi in e.layout()}
    T = w.counts[0].shape[0] if hasattr(w.counts[0], "shape") else len(w.counts[0])
    nn = w.n_neutral
    from tools.fitness_rb_rate import host_draws, host_normalisers
    logZ = np.log(host_normalisers(mean, sigma, lay["loglambda"], T, np.arange(500)))      # (partial sums: timed elsewhere, not compared)
    sbar = host_draws(mean, sigma, lay["s_pop"] + np.arange(T - 1))
    k = min(a.host_units, w.n_bc)
    jobs = [(mean, sigma, lay, T, nn, ms, logZ, sbar, grid) for ms in np.array_split(np.arange(k), procs * 2)]
    with pool:
        pool.map(host_chunk, jobs[:procs])                          # warm-up at size
        ht = []
        for _ in range(3):
            t0 = time.perf_counter()
            sum(pool.map(host_chunk, jobs))
            ht.append(time.perf_counter() - t0)
    res["host_numpy"] = {"procs": procs, "units": k, "units_s_min": min(ht), "units_s_median": float(np.median(ht)), "units_s_max": max(ht),
                         "extrapolated_s": min(ht) * w.n_bc / k, "covers": "the units' part of the call: draws, conditionals, tails, sums over the units"}
    for name in LAYOUTS:
        res["layouts"][name]["host_units_part_over_device_call"] = res["host_numpy"]["extrapolated_s"] / res["layouts"][name]["call_s_min"]
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "dfe_rate.json"), "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
