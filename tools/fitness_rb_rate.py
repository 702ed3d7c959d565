#!/usr/bin/env python3
"""Diagnostic: time bb_fitness_rb (Rao-Blackwellised fitness marginals, barbay.jl_amd/csrc/bb_rb.h) on C2 (fitness_normal
50 000 x 8) at n_samples = 1000 and three quantiles, phase by phase on the device, against numpy on the same box.
   python tools/fitness_rb_rate.py [--out DIR] [--reps N] [--host-rows M] [--host-cols C]
   python tools/xp.py build rb_times -DBB_RB_TIMES      first, for the split: that build drains the stream after every phase and
                                                         prints upload / pop / normalisers / rb / download to stderr
Prints: the wall time of the (synchronous) call on the product library; with lib/ab/rb_times.so present, the phases of one call of
that build (run in a child process); bb_ppc_score and bb_freq_bands (posterior mode, n_ppc = 1) at the same n_samples on the same
handle, for scale; numpy's time for the header's formulas, draws included (Philox as oracle.rng.pairs, scipy's erfc), in one
process: the normalisers on --host-cols data columns and the units on --host-rows mutants, each extrapolated to the whole problem
(the host's normalisers are then partial sums: its numbers are timed, not compared -- the tests compare)."""
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
PROBS = (0.025, 0.5, 0.975)
QS = (0.95, 0.675, 0.05)
STREAM_PARAM = 0xFFFFFFE0
AB = os.path.join(ROOT, "barbay.jl_amd", "lib", "ab", "rb_times.so")


def host_draws(mean, sigma, idx):
    """Parameter draws [len(idx), NS] of the caller's latents idx."""
    from oracle import rng
    j = np.arange(NS, dtype=np.uint64)
    q = np.broadcast_to(np.asarray(idx, dtype=np.uint64)[:, None], (len(idx), NS))
    a, b = rng.pairs(SEED, q, np.broadcast_to(j >> np.uint64(1), q.shape), STREAM_PARAM)
    return mean[idx, None] + sigma[idx, None] * np.where(j & np.uint64(1), b, a)


def host_normalisers(mean, sigma, lo_l, T, cols):
    """Z [T, NS] over the data columns `cols` (loglambda (t, b) at lo_l + b T + t)."""
    idx = (lo_l + np.asarray(cols)[:, None] * T + np.arange(T)[None, :]).reshape(-1)
    return np.exp(host_draws(mean, sigma, idx)).reshape(len(cols), T, NS).sum(axis=0)


def host_units(mean, sigma, lay, T, nn, ms, logZ, sbar, prior=(0.0, 2.0), threshold=0.0):
    """The header's outputs for the mutants ms (fitness model: one unit each, n_u = T - 1)."""
    from scipy.special import erfc
    k, n = len(ms), NS
    idx = (lay["loglambda"] + (nn + ms)[:, None] * T + np.arange(T)[None, :]).reshape(-1)
    ll = host_draws(mean, sigma, idx).reshape(k, T, n)
    gam = (ll[:, 1:] - ll[:, :-1]) - (logZ[None, 1:] - logZ[None, :-1])
    y = (gam + sbar[None]).sum(axis=1)
    s = host_draws(mean, sigma, lay["s_bc"] + ms)
    w = np.exp(-2.0 * host_draws(mean, sigma, lay["logsigma_bc"] + ms))
    ib2 = 1.0 / (prior[1] * prior[1])
    P = ib2 + (T - 1) * w
    m, sd = (prior[0] * ib2 + w * y) / P, 1.0 / np.sqrt(P)
    rm = m.mean(-1)
    v = (m - threshold) / sd * np.sqrt(0.5)
    out = [s.mean(-1), s.std(-1), rm, np.sqrt((sd * sd).mean(-1) + ((m - rm[:, None]) ** 2).mean(-1)),
           (0.5 * erfc(-v)).mean(-1), (0.5 * erfc(v)).mean(-1)]
    lo = np.repeat((m.min(-1) - 40.0 * sd.max(-1))[:, None], len(PROBS), axis=1)
    hi = np.repeat((m.max(-1) + 40.0 * sd.max(-1))[:, None], len(PROBS), axis=1)
    p = np.asarray(PROBS)[None, :]
    for _ in range(64):
        x = lo + (hi - lo) / 2.0
        F = (0.5 * erfc(-((x[:, :, None] - m[:, None, :]) / sd[:, None, :] * np.sqrt(0.5)))).mean(-1)
        below = F < p
        lo, hi = np.where(below, x, lo), np.where(below, hi, x)
    return out, lo + (hi - lo) / 2.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-rows", type=int, default=200)
    ap.add_argument("--host-cols", type=int, default=500)
    ap.add_argument("--phases-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    import barbay_jl_amd as bb
    from barbay_jl_amd import _capi
    lib = _capi.load_library(AB if a.phases_child else None)
    w = bb.synth.fitness_normal()
    call = lambda e: e.fitness_rb(n_samples=NS, probs=PROBS, threshold=0.0, seed=SEED)
    with bb.Engine(w.kind, w.counts, w.n_neutral, w.n_bc, seed=3, _lib=lib) as e:
        e.run(20)
        e.fitness_rb(n_samples=64, probs=PROBS, seed=SEED)          # warm-up: code objects, buffers
        r = call(e)
        if a.phases_child:
            return
        tr, tm, ts, tf = [], [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            r = call(e)
            tr.append(time.perf_counter() - t0)
        for _ in range(a.reps):                                     # the moments and tails alone
            t0 = time.perf_counter()
            e.fitness_rb(n_samples=NS, probs=(), seed=SEED)
            tm.append(time.perf_counter() - t0)
        e.ppc_score(n_samples=NS, seed=SEED)
        e.freq_bands(QS, mode="posterior", n_samples=NS, n_ppc=1, seed=SEED)
        for _ in range(a.reps):
            t0 = time.perf_counter()
            e.ppc_score(n_samples=NS, seed=SEED)
            ts.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            e.freq_bands(QS, mode="posterior", n_samples=NS, n_ppc=1, seed=SEED)
            tf.append(time.perf_counter() - t0)
        mean, sigma = e.posterior()
        lay = {name: lo for name, lo, hi in e.layout()}
    n_units = int(r["rb_mean"].shape[0])
    T = w.counts[0].shape[0] if hasattr(w.counts[0], "shape") else len(w.counts[0])
    nn, B = w.n_neutral, w.n_neutral + w.n_bc
    k, kc = min(a.host_rows, w.n_bc), min(a.host_cols, B)
    ratio = r["rb_sd"] / r["q_sd"]
    t0 = time.perf_counter()
    Z = host_normalisers(mean, sigma, lay["loglambda"], T, np.arange(kc))
    t_z = time.perf_counter() - t0
    sbar = host_draws(mean, sigma, lay["s_pop"] + np.arange(T - 1))
    t0 = time.perf_counter()
    with np.errstate(all="ignore"):
        host_units(mean, sigma, lay, T, nn, np.arange(k), np.log(Z), sbar)
    t_u = time.perf_counter() - t0
    res = {"workload": w.name, "n_samples": NS, "n_quantiles": len(PROBS), "units": n_units, "time_points": T,
           "latent_draws_touched": int((B * T + 2 * w.n_bc + T - 1) * NS),
           "call_s_min": min(tr), "call_s_median": float(np.median(tr)), "units_per_s": n_units / min(tr),
           "call_no_quantiles_s_min": min(tm),
           "sd_ratio_after_20_steps": {"median": float(np.median(ratio)), "min": float(ratio.min()), "max": float(ratio.max())},
           "ppc_score": {"call_s_min": min(ts)}, "freq_bands_posterior_n_ppc1": {"call_s_min": min(tf)},
           "host_numpy": {"procs": 1, "normaliser_cols": kc, "normalisers_s": t_z, "rows": k, "rows_s": t_u,
                          "extrapolated_s": t_z * B / kc + t_u * w.n_bc / k}}
    if os.path.exists(AB):
        c = subprocess.run([sys.executable, os.path.abspath(__file__), "--phases-child"], capture_output=True, text=True)
        lines = re.findall(r"\[bb_fitness_rb[^\n]*", c.stderr)
        if c.returncode != 0 or not lines:
            raise RuntimeError("phase run failed:\n" + c.stderr[-2000:])
        res["phases_ms"] = {kk: float(v) for kk, v in re.findall(r"(upload|pop|normalisers|rb|download) ([0-9.]+) ms", lines[-1])}
        res["phases_line"] = lines[-1]
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "fitness_rb_rate.json"), "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
