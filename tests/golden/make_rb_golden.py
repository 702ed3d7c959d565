"""Generates tests/golden/rb_<case>_n<samples>.npz: what bb_fitness_rb must return for the cases of tests/_rb_cases.py, as a
50-digit mpmath evaluation of the formulas of include/barbay_hip.h on the float64 inputs (s_j, m_j, sd_j) of the numpy restatement
there (`_rb_cases.restate` with this file's `unit_mp` in place of its float64 unit).  A quantile is the 50-digit ROOT of the
mixture CDF F(x) = p -- Newton's iteration at 50 digits from the float64 bisection's result, stopped when a step is below 1e-40 --
not a replay of the bisection.  Everything here is produced by this repository's code from seeded numpy draws; mpmath is needed to
generate the files, not to read them.

Usage:  python tests/golden/make_rb_golden.py [name ...]        (all: a few minutes on 8 cores)

Stored per file: q_mean, q_sd, rb_mean, rb_sd, p_pos, p_neg [units], quantiles [units, 3], n_steps, for the units
`_rb_cases.golden_cases` names (all units but for the largest call).  The largest file is a few KB.
With --measure: prints, per file, the float64 restatement's error against the stored values (the figure `_rb_cases.Q_MEASURED`
records for the quantiles)."""
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for _p in (TESTS, os.path.dirname(TESTS)):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import _rb_cases as rc  # noqa: E402


def unit_mp(s, m, sd, threshold, probs):
    """`_rb_cases.unit64` at 50 digits."""
    import mpmath as mp
    mp.mp.dps = 50
    n = len(m)
    S = [mp.mpf(float(v)) for v in s]
    M = [mp.mpf(float(v)) for v in m]
    SD = [mp.mpf(float(v)) for v in sd]
    r2 = mp.sqrt(2)
    qm, rm = mp.fsum(S) / n, mp.fsum(M) / n
    q_sd = mp.sqrt(mp.fsum((v - qm) ** 2 for v in S) / n)
    rb_sd = mp.sqrt(mp.fsum(v * v for v in SD) / n + mp.fsum((v - rm) ** 2 for v in M) / n)
    z = [(a - mp.mpf(threshold)) / (b * r2) for a, b in zip(M, SD)]
    p_pos = mp.fsum(mp.erfc(-v) for v in z) / (2 * n)
    p_neg = mp.fsum(mp.erfc(v) for v in z) / (2 * n)
    start = rc.unit64(s, m, sd, threshold, probs)[1]
    qs = []
    for p, x0 in zip(probs, start):
        x = mp.mpf(float(x0))
        for _ in range(60):
            F = mp.fsum(mp.erfc(-(x - a) / (b * r2)) for a, b in zip(M, SD)) / (2 * n)
            f = mp.fsum(mp.exp(-((x - a) / b) ** 2 / 2) / b for a, b in zip(M, SD)) / (n * mp.sqrt(2 * mp.pi))
            dx = (F - mp.mpf(p)) / f
            x -= dx
            if abs(dx) < mp.mpf(10) ** -40:
                break
        else:
            raise RuntimeError("no convergence")
        qs.append(x)
    return [qm, q_sd, rm, rb_sd, p_pos, p_neg], qs


def generate(name):
    case, n, units = rc.golden_cases()[name]
    sp, mu, om = rc.inputs(case)
    d = rc.restate(sp, mu, om, n, rc.SEED, units=units, unit=unit_mp)
    np.savez_compressed(rc.golden_path(name), **d)
    return name, os.path.getsize(rc.golden_path(name))


def measure(name):
    case, n, units = rc.golden_cases()[name]
    sp, mu, om = rc.inputs(case)
    return name, rc.errors(rc.restate(sp, mu, om, n, rc.SEED, units=units), rc.golden(name))


def main(argv):
    meas = "--measure" in argv
    names = [a for a in argv if a != "--measure"] or list(rc.golden_cases())
    names.sort(key=lambda k: -rc.golden_cases()[k][1])          # longest first
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        if meas:
            worst = 0.0
            for name, err in pool.imap_unordered(measure, names):
                rc.report(name, "restatement", err)
                worst = max(worst, err["quantiles"])
            print(f"largest quantile error of the float64 restatement: {worst:.3e}")
            return
        for name, size in pool.imap_unordered(generate, names):
            print(f"{name}: {size} bytes", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
