#!/usr/bin/env python3
"""Diagnostic: time bb_fitness_rank (posterior ranks and top-k membership of the units of sets, barbay.jl_amd/csrc/bb_rank.h) on C2
(fitness_normal 50 000 x 8) at n_samples = 1000, two list lengths and three quantiles, for one set of all units (runs of
BB_RANK_RUN merged by search) and for one set per 1 000 units (one workgroup per set and draw), both sources, phase by phase on the
device, against numpy's stable lexsort of a table of the same shape on the same box's CPUs.
   python tools/rank_rate.py [--out DIR] [--reps N] [--host-procs P]
   python tools/xp.py build rank_times -DBB_RB_TIMES                              first, for the split: those builds drain the stream
   python tools/xp.py build rank_times_pm -DBB_RB_TIMES -DBB_RANK_POSITION_MAJOR  after every phase and print map+upload / front /
                                                                                  values / sort / merge / summaries / download
The two builds are the two layouts of the key table: a set's keys [draw][position] (the product's) and [position][draw].
Prints: per source and layout of the sets the wall times of the (synchronous) call on the product library (one warm-up, then
--reps calls: min, median, max); with the lib/ab builds present, the phases of --phase-reps calls of each after a warm-up (median,
min and max per phase; run in child processes, before this process opens the GPU); the host yardstick: np.lexsort (stable, keys
(-v, is NaN)) and the scatter to ranks of a [units, 1000] table of normals, the columns split over --host-procs processes forked
before this process opens the GPU.  The host's numbers are timed, not compared -- the tests compare."""
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
SEED = 7
TOP = (1, 10)
PROBS = (0.025, 0.5, 0.975)
ABS = {"draw_major": os.path.join(ROOT, "barbay.jl_amd", "lib", "ab", "rank_times.so"),
       "position_major": os.path.join(ROOT, "barbay.jl_amd", "lib", "ab", "rank_times_pm.so")}
LAYOUTS = ("one_set", "sets_of_1000")
SOURCES = ("conditional", "draws")
PHASES = "map\\+upload|front|values|sort|merge|summaries|download"


def layouts(n_units):
    return {"one_set": [np.arange(n_units)], "sets_of_1000": [np.arange(lo, min(lo + 1000, n_units)) for lo in range(0, n_units, 1000)]}


def host_columns(args):
    """Ranks of `cols` columns of `n` normals each, set by set: the stable lexsort and the scatter."""
    n, cols, bounds, seed = args
    v = np.random.default_rng(seed).standard_normal((n, cols))
    t0 = time.perf_counter()
    for a, b in bounds:
        x = v[a:b]
        order = np.lexsort((-x, np.isnan(x)), axis=0)
        r = np.empty(x.shape, dtype=np.int32)
        np.put_along_axis(r, order, np.arange(b - a, dtype=np.int32)[:, None], axis=0)
    return time.perf_counter() - t0


def host_warm(_):
    return os.getpid()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-procs", type=int, default=16)
    ap.add_argument("--phase-reps", type=int, default=3)
    ap.add_argument("--phases-child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    phases = {}
    if not a.phases_child:                                      # the phase children first, one at a time: this process holds no GPU yet
        for tab, ab in ABS.items():
            if not os.path.exists(ab):
                continue
            for source in SOURCES:
                for name in LAYOUTS:
                    c = subprocess.run([sys.executable, os.path.abspath(__file__), "--phases-child", f"{tab},{source},{name}", "--phase-reps", str(a.phase_reps)],
                                       capture_output=True, text=True)
                    lines = re.findall(r"\[bb_fitness_rank[^\n]*", c.stderr)[-a.phase_reps:]
                    if c.returncode != 0 or len(lines) < a.phase_reps:
                        raise RuntimeError("phase run failed:\n" + c.stderr[-2000:])
                    per = [{kk: float(v) for kk, v in re.findall(rf"({PHASES}) ([0-9.]+) ms", ln)} for ln in lines]
                    phases.setdefault((source, name), {})[tab] = {
                        "phase_reps": a.phase_reps, "phases_line": lines[-1],
                        "phases_ms": {kk: {"median": float(np.median([q[kk] for q in per])), "min": min(q[kk] for q in per), "max": max(q[kk] for q in per)} for kk in per[0]}}
    pool = None
    procs = max(1, a.host_procs)
    if not a.phases_child:                                      # numpy's pool forks before this process opens the GPU
        pool = multiprocessing.Pool(procs)
        pool.map(host_warm, range(2 * procs))
    import barbay_jl_amd as bb
    from barbay_jl_amd import _capi
    tab, source, child_layout = a.phases_child.split(",") if a.phases_child else (None, None, None)
    lib = _capi.load_library(ABS[tab] if a.phases_child else None)
    w = bb.synth.fitness_normal()
    with bb.Engine(w.kind, w.counts, w.n_neutral, w.n_bc, seed=3, _lib=lib) as e:
        e.run(20)
        n_units = e.fitness_rb_shape()
        sets = layouts(n_units)
        call = lambda src, name: e.fitness_rank(sets[name], top=TOP, probs=PROBS, source=src, n_samples=NS, seed=SEED)
        e.fitness_rank(sets["sets_of_1000"][:2], top=TOP, probs=PROBS, n_samples=64, seed=SEED)      # warm-up: code objects, buffers
        if a.phases_child:
            for _ in range(1 + a.phase_reps):                   # one warm-up at size, then the calls whose lines the parent reads
                call(source, child_layout)
            return
        res = {"workload": w.name, "n_samples": NS, "n_top": len(TOP), "n_quantiles": len(PROBS), "units": n_units, "calls": {}}
        for src in SOURCES:
            for name in LAYOUTS:
                r = call(src, name)                                    # warm-up at size: the buffer grows once
                ts = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    r = call(src, name)
                    ts.append(time.perf_counter() - t0)
                res["calls"][f"{src},{name}"] = {"n_sets": len(sets[name]), "reps": a.reps, "call_s_min": min(ts), "call_s_median": float(np.median(ts)), "call_s_max": max(ts),
                                                 "keys_per_s": n_units * NS / min(ts), "mean_rank_sd_after_20_steps": float(r["rank_sd"].mean()),
                                                 "tables": phases.get((src, name), {})}
    res["host_numpy"] = {"procs": procs}
    with pool:
        for name in LAYOUTS:
            bounds = [(int(s[0]), int(s[-1]) + 1) for s in sets[name]]
            jobs = [(n_units, len(c), bounds, i) for i, c in enumerate(np.array_split(np.arange(NS), procs)) if len(c)]
            ht = []
            for _ in range(2):
                t0 = time.perf_counter()
                inner = pool.map(host_columns, jobs)
                ht.append(time.perf_counter() - t0)
            res["host_numpy"][name] = {"wall_s_min": min(ht), "wall_s_max": max(ht), "sort_s_slowest_process": max(inner),
                                       "covers": "stable lexsort and scatter to ranks of the [units, 1000] table; making the table is in the wall time, not in sort_s"}
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "rank_rate.json"), "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
