#!/usr/bin/env python3
"""Diagnostic: time bb_ppc_score (predictive log score and PIT per barcode, barbay.jl_amd/csrc/bb_score.h) on C2
(fitness_normal 50 000 x 8) at n_samples = 1000, against numpy on the host and against bb_ppc_bands on the same handle.
   python tools/ppc_score_rate.py [--out DIR] [--reps N] [--host-rows M]
   python tools/xp.py build score_times -DBB_SCORE_TIMES      first, for the split: that build drains the stream after every phase
                                                               and prints observed / upload / pop / score / download to stderr
Prints: the wall time of the (synchronous) call on the product library; with lib/ab/score_times.so present, the phases of one
call of that build (run in a child process); bb_ppc_bands(n_samples = 1000, n_ppc = 1, three quantiles) on the same handle -- the
same draws, with the selection the score call does not do; numpy's time for the header's formulas, draws included (Philox as
oracle.rng.pairs, scipy's erfc), on --host-rows mutant rows in one process, extrapolated to all rows (the population-mean draws,
shared by every row, are timed apart and counted once)."""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NS = 1000
SEED = 7
QS = (0.95, 0.675, 0.05)
STREAM_PARAM = 0xFFFFFFE0
AB = os.path.join(ROOT, "barbay.jl_amd", "lib", "ab", "score_times.so")


def host_draws(mean, sigma, idx):
    """Parameter draws [len(idx), NS] of the caller's latents idx."""
    from oracle import rng
    j = np.arange(NS, dtype=np.uint64)
    q = np.broadcast_to(np.asarray(idx, dtype=np.uint64)[:, None], (len(idx), NS))
    a, b = rng.pairs(SEED, q, np.broadcast_to(j >> np.uint64(1), q.shape), STREAM_PARAM)
    return mean[idx, None] + sigma[idx, None] * np.where(j & np.uint64(1), b, a)


def host_scores(y, sbar, mean, sigma, lo_s, lo_ls, ms):
    """The header's outputs for the mutants ms (fitness model): y [k, T1], sbar [T1, NS]."""
    from scipy.special import erfc
    n = NS
    s, sd = host_draws(mean, sigma, lo_s + ms), np.exp(host_draws(mean, sigma, lo_ls + ms))
    mu = s[:, None, :] - sbar[None, :, :]
    z = (y[:, :, None] - mu) / sd[:, None, :]
    l = -0.5 * z * z - np.log(sd)[:, None, :] - 0.5 * np.log(2.0 * np.pi)
    pm = mu.mean(-1)
    psd = np.sqrt((sd * sd).mean(-1)[:, None] + ((mu - pm[..., None]) ** 2).mean(-1))
    top = l.max(-1)
    lpd = top + np.log(np.exp(l - top[..., None]).sum(-1)) - np.log(n)
    pw = ((l - l.mean(-1)[..., None]) ** 2).sum(-1) / (n - 1)
    return pm, psd, lpd, pw, (0.5 * erfc(-z / np.sqrt(2.0))).mean(-1), (0.5 * erfc(z / np.sqrt(2.0))).mean(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-rows", type=int, default=200)
    ap.add_argument("--phases-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    import barbay_jl_amd as bb
    from barbay_jl_amd import _capi
    lib = _capi.load_library(AB if a.phases_child else None)
    w = bb.synth.fitness_normal()
    with bb.Engine(w.kind, w.counts, w.n_neutral, w.n_bc, seed=3, _lib=lib) as e:
        e.run(20)
        e.ppc_score(n_samples=64, seed=SEED)                        # warm-up: code objects, buffers
        r = e.ppc_score(n_samples=NS, seed=SEED)
        if a.phases_child:
            return
        ts, tb = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            r = e.ppc_score(n_samples=NS, seed=SEED)
            ts.append(time.perf_counter() - t0)
        e.ppc_bands(QS, n_samples=NS, n_ppc=1, seed=SEED)
        for _ in range(a.reps):
            t0 = time.perf_counter()
            e.ppc_bands(QS, n_samples=NS, n_ppc=1, seed=SEED)
            tb.append(time.perf_counter() - t0)
        mean, sigma = e.posterior()
        lay = {name: lo for name, lo, hi in e.layout()}
    n_rows, n_steps = r["lpd"].shape
    scored = int(r["n_scored"].sum())
    # numpy on the first --host-rows mutants
    nn, k = w.n_neutral, min(a.host_rows, w.n_bc)
    ms = np.arange(k)
    t0 = time.perf_counter()
    sbar = host_draws(mean, sigma, lay["s_pop"] + np.arange(n_steps))
    t_pop = time.perf_counter() - t0
    y = r["observed"][nn:nn + k]
    t0 = time.perf_counter()
    with np.errstate(all="ignore"):
        hs = host_scores(y, sbar, mean, sigma, lay["s_bc"], lay["logsigma_bc"], ms)
    t_rows = time.perf_counter() - t0
    ok = ~np.isnan(y)
    agree = {kk: float(np.nanmax(np.abs(v[ok] - r[kk][nn:nn + k][ok]) / np.maximum(np.abs(v[ok]), 1.0)))
             for kk, v in zip(("pred_mean", "pred_sd", "lpd", "p_waic", "pit", "pit_upper"), hs)}
    res = {"workload": w.name, "n_samples": NS, "rows": n_rows, "steps": n_steps, "scored_cells": scored,
           "call_s_min": min(ts), "call_s_median": float(np.median(ts)), "scored_cells_per_s": scored / min(ts),
           "cell_samples_per_s": scored * NS / min(ts),
           "ppc_bands_n_ppc1": {"rows": 1 + w.n_bc, "call_s_min": min(tb), "call_s_median": float(np.median(tb))},
           "host_numpy": {"rows": k, "procs": 1, "pop_s": t_pop, "rows_s": t_rows, "extrapolated_s": t_pop + t_rows * n_rows / k,
                          "max_rel_difference_from_device": agree}}
    if os.path.exists(AB):
        c = subprocess.run([sys.executable, os.path.abspath(__file__), "--phases-child"], capture_output=True, text=True)
        lines = re.findall(r"\[bb_ppc_score[^\n]*", c.stderr)
        if c.returncode != 0 or not lines:
            raise RuntimeError("phase run failed:\n" + c.stderr[-2000:])
        res["phases_ms"] = {kk: float(v) for kk, v in re.findall(r"(observed|upload|pop|score|download) ([0-9.]+) ms", lines[-1])}
        res["phases_line"] = lines[-1]
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "ppc_score_rate.json"), "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
