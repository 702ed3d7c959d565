#!/usr/bin/env python3
"""Diagnostic: time bb_logtau_rb (Rao-Blackwellised logtau marginals, barbay.jl_amd/csrc/bb_ltrb.h), both modes, on the replicate
workload of `synth` (replicate_fitness_normal 20 000 x 6 x 3) at n_samples = 1000 and three quantiles, beside bb_logsigma_rb (BC) and
bb_fitness_rb on the same handle, and the numpy restatement of tests/_logtau_rb_cases.py on a small slice of the entries, which also
gives the nodes per draw and the share of draws with two modes.
   python tools/logtau_rb_rate.py [--out DIR] [--reps N] [--slice N]
   python tools/xp.py build rb_times -DBB_RB_TIMES      first, for the split: that build drains the stream after every phase and
                                                         prints the calls' phases to stderr
Prints the wall time of each (synchronous) call on the product library, the same without quantiles (so the bisection's share shows),
and, with lib/ab/rb_times.so present, the phases of one call of each mode on that build (run in a child process).  The time is
recorded, nothing here is a target."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
NS = 1000
SEED = 7
PROBS = (0.025, 0.5, 0.975)
AB = os.path.join(ROOT, "barbay.jl_amd", "lib", "ab", "rb_times.so")
PHASES = r"(upload|normalisers|mixture|download) ([0-9.]+) ms"
MODES = ("full", "collapsed")


def run(reps, child, n_slice):
    import barbay_jl_amd as bb
    from barbay_jl_amd import _capi
    lib = _capi.load_library(AB if child else None)
    w = bb.synth.replicate_fitness_normal()
    res = {"workload": w.name, "n_samples": NS, "n_quantiles": len(PROBS)}
    with bb.Engine(w.kind, w.counts, w.n_neutral, w.n_bc, env_idx=w.env_idx, geno_idx=w.geno_idx, seed=3, _lib=lib) as e:
        e.run(20)
        for m in MODES:                                             # warm-up: code objects, buffers
            e.logtau_rb(mode=m, n_samples=64, probs=PROBS, seed=SEED)
        calls = {"bb_logtau_rb full": lambda **kw: e.logtau_rb(mode="full", n_samples=NS, seed=SEED, **kw),
                 "bb_logtau_rb collapsed": lambda **kw: e.logtau_rb(mode="collapsed", n_samples=NS, seed=SEED, **kw),
                 "bb_logsigma_rb bc": lambda **kw: e.logsigma_rb(block="bc", n_samples=NS, seed=SEED, **kw),
                 "bb_fitness_rb": lambda **kw: e.fitness_rb(n_samples=NS, threshold=0.0, seed=SEED, **kw)}
        for k, call in calls.items():
            r = call(probs=PROBS)
            if child:
                continue
            ts, t0s = [], []
            for _ in range(reps):
                t0 = time.perf_counter()
                r = call(probs=PROBS)
                ts.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                call(probs=())
                t0s.append(time.perf_counter() - t0)
            ratio = r["rb_sd"] / r["q_sd"]
            res[k] = {"rows": int(r["rb_mean"].shape[0]), "call_s_min": min(ts), "call_s_median": float(np.median(ts)),
                      "call_s_min_no_quantiles": min(t0s),
                      "sd_ratio_after_20_steps": {"median": float(np.median(ratio)), "min": float(ratio.min()), "max": float(ratio.max())}}
            if k.startswith("bb_logtau_rb"):
                res[k]["n_terms"] = int(r["n_terms"][0])
                res[k]["two_mode_draws_share"] = float(r["n_two_modes"].mean() / NS)
                res[k]["pool_mean_median"] = float(np.median(r["pool_mean"]))
        if not child and n_slice > 0:                               # the numpy restatement on the first entries: nodes per draw, agreement
            import _logtau_rb_cases as tc
            from oracle.spec import ModelSpec
            cnt = [np.asarray(c) for c in w.counts]
            sp = ModelSpec(kind="replicate", counts=cnt, totals=[c.sum(axis=1) for c in cnt], n_neutral=w.n_neutral, n_bc=w.n_bc)
            mu, om = e.get_params()
            ents = list(range(min(n_slice, tc.n_entries(sp))))
            t0 = time.perf_counter()                                # the per-draw inputs: mostly the normalisers, once whatever the entries
            ci = tc.cond_inputs(sp, tc.lc.draws_of(sp, mu, om, NS, SEED), NS, entries=ents)
            t_in = time.perf_counter() - t0
            for m in MODES:
                t0 = time.perf_counter()
                nodes, rows = [], []
                for u in ents:
                    l, nt, ww, tt, Y, a, ib2 = ci[u]
                    nodes += [c.nleft + c.nright + 1 for c in tc.conds(tc.F64, tc.MODE_ID[m], nt, ww, tt, Y, a, ib2)]
                    rows.append(tc.entry(tc.F64, tc.MODE_ID[m], l, nt, ww, tt, Y, a, ib2, PROBS))
                t_rule = time.perf_counter() - t0
                ref = {k: np.array([float(r[0][i]) for r in rows]) for i, k in enumerate(tc.UNITS)}
                ref["quantiles"] = np.array([[float(q) for q in r[1]] for r in rows])
                got = e.logtau_rb(mode=m, n_samples=NS, probs=PROBS, seed=SEED)
                err = tc.errors(tc.take(got, ents), ref)
                res[f"bb_logtau_rb {m}"]["numpy"] = {"entries": len(ents), "inputs_s": t_in, "rule_s": t_rule, "largest_error": max(err.values()),
                                                     "nodes_per_draw": {"min": int(min(nodes)), "median": float(np.median(nodes)), "max": int(max(nodes))}}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--slice", type=int, default=2, help="entries the numpy restatement is timed on (0: none)")
    ap.add_argument("--phases-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.phases_child:
        run(0, True, 0)
        return
    res = run(a.reps, False, a.slice)
    if os.path.exists(AB):
        c = subprocess.run([sys.executable, os.path.abspath(__file__), "--phases-child"], capture_output=True, text=True)
        for m in MODES:
            lines = re.findall(r"\[bb_logtau_rb " + m + r" [^\n]*", c.stderr)
            if c.returncode != 0 or not lines:
                raise RuntimeError("phase run failed:\n" + c.stderr[-2000:])
            res[f"bb_logtau_rb {m}"]["phases_ms"] = {kk: float(v) for kk, v in re.findall(PHASES, lines[-1])}
            res[f"bb_logtau_rb {m}"]["phases_line"] = lines[-1]
    print(json.dumps({"replicate": res}), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "logtau_rb_rate.json"), "w") as f:
            json.dump({"replicate": res}, f, indent=1)


if __name__ == "__main__":
    main()
