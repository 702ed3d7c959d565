#!/usr/bin/env python3
"""Diagnostic: time bb_chain_summary (chain diagnostics, barbay.jl_amd/csrc/bb_chain.h) at W = 4 chains x N = 1 000 draws x
D = 50 000 AR(1) columns (phi drawn per column from 0 .. 0.9), five quantiles, against numpy on the host's CPUs.
   python tools/chain_summary_rate.py [--out DIR] [--cols D] [--reps N] [--host-cols M] [--procs P]
   python tools/xp.py build chain_times -DBB_CHAIN_TIMES      first, for the split: that build drains the stream after every phase
                                                               and prints upload / transpose / stats / download to stderr
Prints: the wall time of the (synchronous) call on the product library; with lib/ab/chain_times.so present, the phases of one
call of that build (run in a child process); numpy's time for the same statistics -- direct lag sums in batches of 32 lags, each
column stopped at its truncation, sort-based quantiles -- on --host-cols columns over --procs processes (forked before the clock
starts, slicing the parent's array: no pool start and no chain through a pipe in the figure), extrapolated to D."""
import argparse
import json
import multiprocessing as mp
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, N = 4, 1000
PROBS = (0.025, 0.25, 0.5, 0.75, 0.975)
AB = os.path.join(ROOT, "barbay.jl_amd", "lib", "ab", "chain_times.so")


def make_chain(D, seed=0):
    g = np.random.default_rng(seed)
    phi = g.uniform(0.0, 0.9, D)
    x = np.empty((W, N, D))
    x[:, 0] = g.standard_normal((W, D)) / np.sqrt(1.0 - phi * phi)
    for n in range(1, N):
        x[:, n] = phi * x[:, n - 1] + g.standard_normal((W, D))
    return x


def host_summary(x):
    """The header's statistics of x[W, N, d], vectorised over the columns."""
    Wn, Nn, d = x.shape
    K = Wn * Nn
    pooled = x.reshape(K, d)
    mean = pooled.mean(0)
    sd = pooled.std(0, ddof=1)
    q = np.quantile(pooled, PROBS, axis=0)
    y = x - x.mean(1, keepdims=True)
    wbar = (y * y).sum(1).mean(0) / (Nn - 1)
    vp = (Nn - 1) / Nn * wbar + (x.mean(1).var(0, ddof=1) if Wn > 1 else 0.0)
    tot, prev, live, t0 = np.zeros(d), np.full(d, np.inf), np.ones(d, bool), 0
    while live.any() and t0 + 1 <= Nn - 1:
        idx = np.flatnonzero(live)
        yy = y[:, :, idx]
        rho = np.stack([1.0 - (wbar[idx] - (yy[:, :Nn - t] * yy[:, t:]).sum(1).mean(0) / Nn) / vp[idx] for t in range(t0, min(t0 + 32, Nn))])
        for k in range(rho.shape[0] // 2):
            pk = rho[2 * k] + rho[2 * k + 1]
            on = live[idx] & (pk > 0)
            live[idx[~on]] = False
            pk = np.minimum(pk, prev[idx])
            tot[idx[on]] += pk[on]
            prev[idx[on]] = pk[on]
        t0 += 32
    ess = np.minimum(K / (-1.0 + 2.0 * tot), K * np.log10(K))
    h = Nn // 2
    hv = np.concatenate([x[:, :h], x[:, Nn - h:]], axis=0)
    w2 = hv.var(1, ddof=1).mean(0)
    rhat = np.sqrt(((h - 1) / h * w2 + hv.mean(1).var(0, ddof=1)) / w2)
    return mean, sd, sd / np.sqrt(ess), ess, rhat, q


_HOST_X = None            # the chain the forked workers slice: set before the pool starts, so nothing of it crosses a pipe


def _host_range(r):
    return host_summary(np.ascontiguousarray(_HOST_X[:, :, r[0]:r[1]]))        # the gather from the column-fastest array is timed


def host_time(x, procs, chunk=250):
    """numpy's time alone: the workers are forked (and have answered once) before the clock starts, they take their columns
    from the parent's array by index range, and only the statistics come back."""
    global _HOST_X
    _HOST_X = x
    ranges = [(i, min(i + chunk, x.shape[2])) for i in range(0, x.shape[2], chunk)]
    with mp.get_context("fork").Pool(procs) as pool:
        pool.map(_host_range, [(0, 1)] * procs)
        t0 = time.perf_counter()
        pool.map(_host_range, ranges, chunksize=1)
        return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cols", type=int, default=50_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-cols", type=int, default=8000)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--phases-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    x = make_chain(a.cols)
    if not a.phases_child:                     # numpy first: the pool forks before this process opens the GPU
        m = min(a.host_cols, a.cols)
        hs = host_time(x[:, :, :m], a.procs)
        host = {"cols": m, "procs": a.procs, "s": hs, "extrapolated_s": hs * a.cols / m}
        print("host numpy", json.dumps(host), flush=True)
    import barbay_jl_amd as bb
    from barbay_jl_amd import _capi
    lib = _capi.load_library(AB if a.phases_child else None)
    w = bb.synth.fitness_normal(2000, 5, 1)
    with bb.Engine(w.kind, w.counts, w.n_neutral, w.n_bc, seed=1, _lib=lib) as e:
        e.chain_summary(x[:, :, :4096], PROBS)                     # warm-up: code objects, buffers
        e.chain_summary(x, PROBS)
        if a.phases_child:
            return
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            r = e.chain_summary(x, PROBS)
            ts.append(time.perf_counter() - t0)
    res = {"W": W, "N": N, "cols": a.cols, "call_s_min": min(ts), "call_s_median": float(np.median(ts)), "columns_per_s": a.cols / min(ts),
           "bytes": x.nbytes, "upload_GB_per_s_if_all_upload": x.nbytes / min(ts) / 1e9, "mean_n_lags": float(r["n_lags"].mean()),
           "max_n_lags": int(r["n_lags"].max()), "host_numpy": host}
    if os.path.exists(AB):
        c = subprocess.run([sys.executable, os.path.abspath(__file__), "--phases-child", "--cols", str(a.cols)], capture_output=True, text=True)
        lines = re.findall(r"\[bb_chain_summary[^\n]*", c.stderr)
        if c.returncode != 0 or not lines:
            raise RuntimeError("phase run failed:\n" + c.stderr[-2000:])
        res["phases_ms"] = {k: float(v) for k, v in re.findall(r"(upload|transpose|stats|download) ([0-9.]+) ms", lines[-1])}
        res["phases_line"] = lines[-1]
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "chain_summary_rate.json"), "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
