#!/usr/bin/env python3
"""Diagnostic: time bb_popmean_rb (Rao-Blackwellised population-mean fitness marginals, barbay.jl_amd/csrc/bb_rb.h) beside
bb_fitness_rb on the same handle in the same process, on C2 (fitness_normal 50 000 x 8) and C5 (genotype_fitness_normal
200 000 x 8, 5 000 genotypes), at n_samples = 1000 and three quantiles.
   python tools/popmean_rb_rate.py [--out DIR] [--reps N]
   python tools/xp.py build rb_times -DBB_RB_TIMES      first, for the split: that build drains the stream after every phase and
                                                         prints both calls' phases to stderr
Prints, per workload: the wall time of each (synchronous) call on the product library and, with lib/ab/rb_times.so present, the
phases of one call of each on that build (run in a child process: one handle, bb_fitness_rb then bb_popmean_rb).  bb_fitness_rb is
there for scale; the time is recorded, nothing here is a target."""
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
AB = os.path.join(ROOT, "barbay.jl_amd", "lib", "ab", "rb_times.so")
WORKLOADS = {"C2": "fitness_normal", "C5": "genotype_fitness_normal"}
PHASES = {"bb_fitness_rb": r"(upload|pop|normalisers|rb|download) ([0-9.]+) ms",
          "bb_popmean_rb": r"(upload|normalisers|part|pop|download) ([0-9.]+) ms"}


def run(name, reps, child):
    import barbay_jl_amd as bb
    from barbay_jl_amd import _capi
    lib = _capi.load_library(AB if child else None)
    w = getattr(bb.synth, WORKLOADS[name])()
    calls = {"bb_fitness_rb": lambda e, **kw: e.fitness_rb(n_samples=NS, probs=PROBS, threshold=0.0, seed=SEED, **kw),
             "bb_popmean_rb": lambda e, **kw: e.popmean_rb(n_samples=NS, probs=PROBS, threshold=0.0, seed=SEED, **kw)}
    res = {"workload": w.name, "n_samples": NS, "n_quantiles": len(PROBS)}
    with bb.Engine(w.kind, w.counts, w.n_neutral, w.n_bc, env_idx=w.env_idx, geno_idx=w.geno_idx, seed=3, _lib=lib) as e:
        e.run(20)
        e.fitness_rb(n_samples=64, probs=PROBS, seed=SEED)          # warm-up: code objects, buffers
        e.popmean_rb(n_samples=64, probs=PROBS, seed=SEED)
        for k, call in calls.items():
            r = call(e)
            if child:
                continue
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                r = call(e)
                ts.append(time.perf_counter() - t0)
            ratio = r["rb_sd"] / r["q_sd"]
            res[k] = {"rows": int(r["rb_mean"].shape[0]), "call_s_min": min(ts), "call_s_median": float(np.median(ts)),
                      "sd_ratio_after_20_steps": {"median": float(np.median(ratio)), "min": float(ratio.min()), "max": float(ratio.max())}}
            if k == "bb_popmean_rb":
                res[k]["members"] = int(r["n_members"][0])
                res[k]["member_terms"] = int(r["n_members"].astype(np.int64).sum()) * NS
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--phases-child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.phases_child:
        run(a.phases_child, 0, True)
        return
    out = {}
    for name in WORKLOADS:
        res = run(name, a.reps, False)
        if os.path.exists(AB):
            c = subprocess.run([sys.executable, os.path.abspath(__file__), "--phases-child", name], capture_output=True, text=True)
            for k, pat in PHASES.items():
                lines = re.findall(r"\[" + k + r" [^\n]*", c.stderr)
                if c.returncode != 0 or not lines:
                    raise RuntimeError("phase run failed:\n" + c.stderr[-2000:])
                res[k]["phases_ms"] = {kk: float(v) for kk, v in re.findall(pat, lines[-1])}
                res[k]["phases_line"] = lines[-1]
        print(json.dumps({name: res}), flush=True)
        out[name] = res
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "popmean_rb_rate.json"), "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
