#!/usr/bin/env python3
"""Diagnostic: time bb_ppc_loo (PSIS leave-one-out scores per cell and per barcode, barbay.jl_amd/csrc/bb_loo.h) on C2
(fitness_normal 50 000 x 8) at n_samples = 1000, phase by phase, and against bb_ppc_score on the same handle in the same job.
   python tools/ppc_loo_rate.py [--out DIR] [--reps N]
   python tools/xp.py build loo_times -DBB_LOO_TIMES -DBB_SCORE_TIMES      first, for the split: that build drains the stream after
                                                                            every phase and prints the phases of both calls to stderr
Prints one JSON line (and writes DIR/ppc_loo_rate.json): the wall time of the (synchronous) call on the product library, that of
bb_ppc_score at the same n_samples and seed and their ratio; with lib/ab/loo_times.so present, the phases of one call of each in
that build (run in a child process); the spread of khat over the cells and the barcodes, for the record.
   python tools/ppc_loo_rate.py --errors LOG [LOG ...]      gathers the "loo case" lines the tests print (pytest -s) into the table
                                                             of tests/_loo_cases.py: the largest error per parameter set and size"""
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
AB = os.path.join(ROOT, "barbay.jl_amd", "lib", "ab", "loo_times.so")
PHASE = r"(observed|upload|pop|score|loo|download) ([0-9.]+) ms"


def errors_table(logs):
    """label -> (set, n) -> output -> largest error in 1e-16, from the lines `_loo_cases.report` prints."""
    worst = {}
    for path in logs:
        for line in open(path, errors="replace"):
            m = re.match(r".*loo case (\S+)\s+(restatement|emulation|device)\s+(.*)\(1e-16\)", line)
            if not m or "_n" not in m.group(1):
                continue
            name, label, rest = m.groups()
            pset = "tight" if "_tight_" in name else "wide"
            key = (pset, int(name.rsplit("_n", 1)[1]))
            vals = dict(re.findall(r"(\S+)\s+([0-9.]+)", rest))
            d = worst.setdefault(key, {}).setdefault(label, {})
            for k, v in vals.items():
                d[k] = max(d.get(k, 0.0), float(v))
    cols = ("elpd_loo", "p_loo", "khat", "n_eff", "lpd", "row_elpd_loo", "row_khat", "row_n_eff")
    print(f"{'set, n':16s}" + "".join(f"{c:>22s}" for c in cols))
    for key in sorted(worst):
        cell = lambda c: "/".join(f"{worst[key].get(lab, {}).get(c, float('nan')):6.1f}" for lab in ("restatement", "emulation", "device"))
        print(f"{key[0] + ', ' + str(key[1]):16s}" + "".join(f"{cell(c):>22s}" for c in cols))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--errors", nargs="+", default=None)
    ap.add_argument("--phases-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.errors:
        return errors_table(a.errors)
    import barbay_jl_amd as bb
    from barbay_jl_amd import _capi
    lib = _capi.load_library(AB if a.phases_child else None)
    w = bb.synth.fitness_normal()
    with bb.Engine(w.kind, w.counts, w.n_neutral, w.n_bc, seed=3, _lib=lib) as e:
        e.run(20)
        e.ppc_loo(n_samples=64, seed=SEED)                          # warm-up: code objects, buffers
        e.ppc_score(n_samples=64, seed=SEED)
        s = e.ppc_score(n_samples=NS, seed=SEED)
        r = e.ppc_loo(n_samples=NS, seed=SEED)
        if a.phases_child:
            return
        tl, ts = [], []
        for _ in range(a.reps):                                     # alternating, so a drift hits both alike
            t0 = time.perf_counter()
            r = e.ppc_loo(n_samples=NS, seed=SEED)
            tl.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            s = e.ppc_score(n_samples=NS, seed=SEED)
            ts.append(time.perf_counter() - t0)
    assert r["lpd"].tobytes() == s["lpd"].tobytes()
    n_rows, n_steps = r["lpd"].shape
    scored = int(r["n_scored"].sum())
    k, rk = r["khat"][~np.isnan(r["khat"])], r["row_khat"][~np.isnan(r["row_khat"])]
    band = lambda v: {"lt_0.5": int((v < 0.5).sum()), "0.5_to_0.7": int(((v >= 0.5) & (v <= 0.7)).sum()),
                      "gt_0.7": int(((v > 0.7) & np.isfinite(v)).sum()), "inf": int(np.isinf(v).sum())}
    res = {"workload": w.name, "n_samples": NS, "rows": n_rows, "steps": n_steps, "scored_cells": scored,
           "psis_fits_per_call": scored + int((r["n_scored"] > 0).sum()),
           "call_s_min": min(tl), "call_s_median": float(np.median(tl)), "scored_cells_per_s": scored / min(tl),
           "ppc_score": {"call_s_min": min(ts), "call_s_median": float(np.median(ts))},
           "ratio_to_ppc_score": min(tl) / min(ts),
           "khat_cells": band(k), "khat_rows": band(rk), "lpd_bytes_equal_ppc_score": True}
    if os.path.exists(AB):
        c = subprocess.run([sys.executable, os.path.abspath(__file__), "--phases-child"], capture_output=True, text=True)
        ll, ls = re.findall(r"\[bb_ppc_loo[^\n]*", c.stderr), re.findall(r"\[bb_ppc_score[^\n]*", c.stderr)
        if c.returncode != 0 or not ll or not ls:
            raise RuntimeError("phase run failed:\n" + c.stderr[-2000:])
        res["phases_ms"] = {kk: float(v) for kk, v in re.findall(PHASE, ll[-1])}
        res["phases_line"] = ll[-1]
        res["ppc_score"]["phases_ms"] = {kk: float(v) for kk, v in re.findall(PHASE, ls[-1])}
        res["ppc_score"]["phases_line"] = ls[-1]
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "ppc_loo_rate.json"), "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
