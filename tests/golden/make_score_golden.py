"""Generates tests/golden/score_<case>_n<samples>.npz: what bb_ppc_score must return for the cases of tests/_score_cases.py, as a
50-digit mpmath evaluation of the formulas of include/barbay_hip.h on the float64 inputs (y, mu_j, sigma_j) of the numpy
restatement there (`_score_cases.restate` with this file's `score_cell_mp` in place of its float64 cell).  Everything here is
produced by this repository's code from seeded numpy draws; mpmath is needed to generate the files, not to read them.

Usage:  python tests/golden/make_score_golden.py [name ...]        (all: about two minutes on 8 cores)

Stored per file: the seven per-cell outputs [rows, n_steps] (NaN: unscored), row_lpd, row_p_waic [rows] (the 50-digit sums of the
50-digit cells, rounded once) and n_scored, for the rows `_score_cases.golden_cases` names (all rows but for the 16384-sample call).
The largest file is under 40 KB."""
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for _p in (TESTS, os.path.dirname(TESTS)):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import _score_cases as sc  # noqa: E402


def score_cell_mp(y, mu, sd):
    """`_score_cases.score_cell` at 50 digits."""
    import mpmath as mp
    mp.mp.dps = 50
    n = len(mu)
    Y = mp.mpf(y)
    M = [mp.mpf(float(v)) for v in mu]
    S = [mp.mpf(float(v)) for v in sd]
    z = [(Y - m) / s for m, s in zip(M, S)]
    half_log2pi = mp.log(2 * mp.pi) / 2
    l = [-zz * zz / 2 - mp.log(s) - half_log2pi for zz, s in zip(z, S)]
    pm = mp.fsum(M) / n
    psd = mp.sqrt(mp.fsum(s * s for s in S) / n + mp.fsum((m - pm) ** 2 for m in M) / n)
    top = max(l)
    lpd = top + mp.log(mp.fsum(mp.exp(v - top) for v in l)) - mp.log(n)
    lbar = mp.fsum(l) / n
    pw = mp.fsum((v - lbar) ** 2 for v in l) / (n - 1)
    r2 = mp.sqrt(2)
    pit = mp.fsum(mp.erfc(-zz / r2) for zz in z) / (2 * n)
    pit_u = mp.fsum(mp.erfc(zz / r2) for zz in z) / (2 * n)
    return Y, pm, psd, lpd, pw, pit, pit_u


def generate(name):
    case, n, rows = sc.golden_cases()[name]
    sp, mu, om = sc.inputs(case)
    d = sc.restate(sp, mu, om, n, sc.SEED, rows=rows, cell=score_cell_mp)
    np.savez_compressed(sc.golden_path(name), **d)
    return name, os.path.getsize(sc.golden_path(name))


def main(argv):
    names = argv or list(sc.golden_cases())
    names.sort(key=lambda k: -sc.golden_cases()[k][1])          # longest first
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        for name, size in pool.imap_unordered(generate, names):
            print("done", name, size, "bytes", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
