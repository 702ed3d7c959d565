#!/usr/bin/env python3
"""Diagnostic: time bb_loglambda_rb (Rao-Blackwellised loglambda marginals, barbay.jl_amd/csrc/bb_llrb.h) on C2 (fitness_normal
50 000 x 8) at n_samples = 1000 and three quantiles, for 1 000 rows spread over the barcodes and for all rows, beside bb_logsigma_rb
(bc) on the same handle.
   python tools/loglambda_rb_rate.py [--out DIR] [--reps N] [--all-quantiles]
   python tools/xp.py build llrb_times -DBB_LLRB_TIMES      first, for the split: that build drains the stream after every phase and
                                                            prints the call's phases to stderr
Prints the wall time of each (synchronous) call on the product library, the same without quantiles (so the bisection's share shows),
and, with lib/ab/llrb_times.so present, the phases of one call of each row set on that build (run in a child process).  All rows
with quantiles is four hundred thousand entries' bisections: it is run only with --all-quantiles.  The time is recorded, nothing
here is a target."""
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
AB = os.path.join(ROOT, "barbay.jl_amd", "lib", "ab", "llrb_times.so")
PHASES = r"(upload|normalisers|tables|entries|download) ([0-9.]+) ms"


def run(reps, child, all_q):
    import barbay_jl_amd as bb
    from barbay_jl_amd import _capi
    lib = _capi.load_library(AB if child else None)
    w = bb.synth.fitness_normal()
    res = {"workload": w.name, "n_samples": NS, "n_quantiles": len(PROBS)}
    with bb.Engine(w.kind, w.counts, w.n_neutral, w.n_bc, env_idx=w.env_idx, geno_idx=w.geno_idx, seed=3, _lib=lib) as e:
        e.run(20)
        n_rows, n_cols = e.loglambda_rb_shape()
        some = np.linspace(0, n_rows - 1, 1000).astype(np.int64)
        e.loglambda_rb(n_samples=64, probs=PROBS, seed=SEED, rows=some[:8])      # warm-up: code objects, buffers
        sets = {"1000 rows": (some, True), "all rows": (None, all_q)}
        for k, (rows, with_q) in sets.items():
            out = res.setdefault(f"bb_loglambda_rb {k}", {"rows": int(n_rows if rows is None else len(rows)), "n_cols": int(n_cols)})
            if child:
                e.loglambda_rb(n_samples=NS, probs=PROBS if with_q else (), seed=SEED, rows=rows)
                continue
            ts, t0s = [], []
            for _ in range(reps):
                if with_q:
                    t0 = time.perf_counter()
                    r = e.loglambda_rb(n_samples=NS, probs=PROBS, seed=SEED, rows=rows)
                    ts.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                r = e.loglambda_rb(n_samples=NS, probs=(), seed=SEED, rows=rows)
                t0s.append(time.perf_counter() - t0)
            ratio = r["rb_sd"] / r["q_sd"]
            low = r["n_reads"] <= 5
            out.update({"call_s_min": min(ts) if ts else None, "call_s_median": float(np.median(ts)) if ts else None, "call_s_min_no_quantiles": min(t0s),
                        "entries_with_5_reads_or_fewer": int(low.sum()),
                        "sd_ratio_after_20_steps": {"median": float(np.median(ratio)), "min": float(ratio.min()), "max": float(ratio.max())}})
        if not child:
            t0 = time.perf_counter()
            e.logsigma_rb(block="bc", n_samples=NS, probs=PROBS, seed=SEED)
            e.logsigma_rb(block="bc", n_samples=NS, probs=PROBS, seed=SEED)
            res["bb_logsigma_rb bc"] = {"call_s": (time.perf_counter() - t0) / 2}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--all-quantiles", action="store_true", help="also time all rows with quantiles")
    ap.add_argument("--phases-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.phases_child:
        run(0, True, a.all_quantiles)
        return
    res = run(a.reps, False, a.all_quantiles)
    if os.path.exists(AB):
        c = subprocess.run([sys.executable, os.path.abspath(__file__), "--phases-child"] + (["--all-quantiles"] if a.all_quantiles else []),
                           capture_output=True, text=True)
        lines = re.findall(r"\[bb_loglambda_rb [^\n]*", c.stderr)
        if c.returncode != 0 or len(lines) < 3:
            raise RuntimeError("phase run failed:\n" + c.stderr[-2000:])
        for k, line in zip(("1000 rows", "all rows"), lines[-2:]):      # (the first line is the warm-up's)
            res[f"bb_loglambda_rb {k}"]["phases_ms"] = {kk: float(v) for kk, v in re.findall(PHASES, line)}
            res[f"bb_loglambda_rb {k}"]["phases_line"] = line
    print(json.dumps({"C2": res}), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "loglambda_rb_rate.json"), "w") as f:
            json.dump({"C2": res}, f, indent=1)


if __name__ == "__main__":
    main()
