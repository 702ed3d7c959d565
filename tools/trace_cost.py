#!/usr/bin/env python3
"""Diagnostic: what the iterate trace (bb_trace_*, barbay.jl_amd/csrc/bb_trace.h) costs and what it says, on the bench shape
(fitness_normal, 50 000 x 8) and the genotype shape (genotype_fitness_normal, 200 000 x 8).
   python tools/trace_cost.py [--out DIR] [--shapes bench,genotype] [--steps N] [--reps R] [--fit-steps M]
   python tools/trace_cost.py --small                          2 000 barcodes, 200 steps, every = 10: a smoke run of the tool
   python tools/xp.py build trace_times -DBB_TRACE_TIMES       first, for the split: that build drains the stream after every phase
                                                               and prints gather / transpose / stats / collect / verdict / download
Per shape it prints, and with --out writes to DIR/trace_cost.json:
   steps/s untraced and traced at every = 10, 50, 200 (wall time of run(N), the best of R; a traced run is cut at the trace's
   boundaries, so it launches eagerly or in short resident launches where the untraced run replays graphs or stays resident);
   the wall time of one trace_summary over 400 snapshots (4 segments of 100) and, with lib/ab/trace_times.so present, its phases
   (run in a child process);
   the verdict of a fit of M = 10 000 steps at every = 10 over its last 400 snapshots: per block the share of columns with
   split-R-hat above 1.1 and max_mcse_rel (definitions: include/barbay_hip.h, bb_trace_summary)."""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
AB = os.path.join(ROOT, "barbay.jl_amd", "lib", "ab", "trace_times.so")
WINDOW, CHAINS = 400, 4


def workload(shape, small):
    from barbay_jl_amd import synth
    if shape == "bench":
        return synth.fitness_normal(2000 if small else 50_000, 8, seed=42)
    return synth.genotype_fitness_normal(2000 if small else 200_000, 8, 50 if small else 5_000, seed=45)


def engine(wl, lib=None):
    import barbay_jl_amd as bb
    return bb.Engine(wl.kind, wl.counts, wl.n_neutral, wl.n_bc, env_idx=wl.env_idx, geno_idx=wl.geno_idx, seed=42, _lib=lib)


def rate(e, steps, reps):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        e.run(steps)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return steps / best


def verdict_rows(blocks):
    return [dict(name=r["name"], part=r["part"], n_cols=int(r["n_cols"]), n_const=int(r["n_const"]), n_nonfinite=int(r["n_nonfinite"]),
                 share_above=float(r["n_above"]) / max(1, int(r["n_cols"]) - int(r["n_const"])), max_rhat=float(r["max_rhat"]),
                 min_ess=float(r["min_ess"]), max_mcse_rel=float(r["max_mcse_rel"])) for _, r in blocks.iterrows()]


def measure(shape, a):
    wl = workload(shape, a.small)
    every_set = (10,) if a.small else (10, 50, 200)
    window = min(WINDOW, a.steps // 10)
    res = {"shape": shape, "kind": wl.kind, "steps": a.steps, "window": window, "n_chains": CHAINS}
    with engine(wl) as e:
        res["latents"] = e.D
        res["kernel"] = e.kernel_name()
        e.run(min(1000, a.steps))                      # warm-up: code objects, graphs
        res["steps_per_s_untraced"] = rate(e, a.steps, a.reps)
        res["steps_per_s_traced"] = {}
        for every in every_set:
            e.trace_begin(every, max(window, 8))
            e.run(min(200, a.steps))
            res["steps_per_s_traced"][str(every)] = rate(e, a.steps, a.reps)
            e.trace_end()
        print(shape, "rates", json.dumps({k: res[k] for k in ("kernel", "steps_per_s_untraced", "steps_per_s_traced")}), flush=True)
    with engine(wl) as e:                              # the fit: a fresh handle, every = 10
        e.trace_begin(10, max(window, 8))
        t0 = time.perf_counter()
        e.run(a.fit_steps)
        res["fit_s"] = time.perf_counter() - t0
        taken, _ = e.trace_count()
        first = taken - window
        e.trace_summary(first, CHAINS, window // CHAINS)          # warm-up: code objects, buffers
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            s = e.trace_summary(first, CHAINS, window // CHAINS)
            ts.append(time.perf_counter() - t0)
        res["summary_s_min"] = min(ts)
        res["fit_steps"] = a.fit_steps
        res["verdict"] = verdict_rows(s["blocks"])
        n_above = sum(v["share_above"] * (v["n_cols"] - v["n_const"]) for v in res["verdict"])
        res["share_above_all"] = n_above / max(1, sum(v["n_cols"] - v["n_const"] for v in res["verdict"]))
    print(shape, "summary", json.dumps({k: res[k] for k in ("summary_s_min", "share_above_all")}), flush=True)
    for v in res["verdict"]:
        print(f"   {v['name']:13s} {v['part']:5s} {v['n_cols']:8d} cols, above 1.1: {v['share_above']:.4f}, max rhat {v['max_rhat']:.3f}, "
              f"min ess {v['min_ess']:.1f}, max mcse_rel {v['max_mcse_rel']:.3g}", flush=True)
    if os.path.exists(AB) and not a.small:
        c = subprocess.run([sys.executable, os.path.abspath(__file__), "--phases-child", "--shapes", shape], capture_output=True, text=True)
        lines = re.findall(r"\[bb_trace_summary[^\n]*", c.stderr)
        if c.returncode != 0 or not lines:
            raise RuntimeError("phase run failed:\n" + c.stderr[-2000:])
        res["phases_ms"] = {k: float(v) for k, v in re.findall(r"(gather|transpose|stats|collect|verdict|download) ([0-9.]+) ms", lines[-1])}
        res["phases_line"] = lines[-1]
        print(shape, lines[-1], flush=True)
    return res


def phases_child(shape):
    """One warm trace_summary on the BB_TRACE_TIMES build: the phase line goes to stderr."""
    from barbay_jl_amd import _capi
    with engine(workload(shape, False), _capi.load_library(AB)) as e:
        e.trace_begin(1, WINDOW)
        e.run(WINDOW)
        e.trace_summary(0, CHAINS, WINDOW // CHAINS)
        e.trace_summary(0, CHAINS, WINDOW // CHAINS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="bench,genotype")
    ap.add_argument("--steps", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--fit-steps", type=int, default=10_000)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--phases-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    shapes = a.shapes.split(",")
    if a.phases_child:
        return phases_child(shapes[0])
    if a.small:
        a.steps, a.fit_steps, a.reps = 200, 200, 1
    res = {"shapes": [measure(s, a) for s in shapes]}
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "trace_cost.json"), "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
