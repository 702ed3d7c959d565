"""Generates tests/golden/theta_rb_<case>_n<samples>.npz: what bb_theta_rb must return for the cases of tests/_theta_rb_cases.py,
as a 50-digit mpmath evaluation of the formulas of include/barbay_hip.h on the float64 inputs (theta_j, m_j, sd_j) of the numpy
restatement there (`_theta_rb_cases.restate` with `make_rb_golden.unit_mp` in place of its float64 unit; a quantile is the 50-digit
root of the mixture CDF).  Everything here is produced by this repository's code from seeded numpy draws; mpmath is needed to
generate the files, not to read them.

Usage:  python tests/golden/make_theta_rb_golden.py [name ...]        (all: a few minutes on 8 cores)

Stored per file: q_mean, q_sd, rb_mean, rb_sd, p_pos, p_neg [groups], quantiles [groups, 3], n_members, n_steps and threshold
[groups] -- the threshold of a group's p_pos / p_neg, `_theta_rb_cases.nearest` its float64 rb_mean -- for the groups
`_theta_rb_cases.golden_cases` names (all groups but for the largest call).  The largest file is a few KB.
With --measure: prints, per file, the float64 restatement's error against the stored values and the largest over all files (the
figures `_theta_rb_cases.MEASURED` and `Q_MEASURED` record)."""
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for _p in (HERE, TESTS, os.path.dirname(TESTS)):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import _theta_rb_cases as tc  # noqa: E402
from make_rb_golden import unit_mp  # noqa: E402


def generate(name):
    case, n, groups = tc.golden_cases()[name]
    sp, mu, om = tc.inputs(case)
    d = tc.restate(sp, mu, om, n, tc.SEED, threshold=None, groups=groups, unit=unit_mp)
    np.savez_compressed(tc.golden_path(name), **d)
    return name, os.path.getsize(tc.golden_path(name))


def measure(name):
    case, n, groups = tc.golden_cases()[name]
    sp, mu, om = tc.inputs(case)
    ref = tc.golden(name)
    return name, tc.errors(tc.restate(sp, mu, om, n, tc.SEED, threshold=ref["threshold"], groups=groups), ref)


def main(argv):
    meas = "--measure" in argv
    names = [a for a in argv if a != "--measure"] or list(tc.golden_cases())
    names.sort(key=lambda k: -tc.golden_cases()[k][1] * (len(tc.golden_cases()[k][2] or ()) or 40))      # longest first
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        if meas:
            worst, worst_q = 0.0, 0.0
            for name, err in pool.imap_unordered(measure, names):
                tc.report(name, "restatement", err)
                worst = max(worst, max(err[k] for k in tc.UNITS))
                worst_q = max(worst_q, err["quantiles"])
            print(f"largest error of the float64 restatement: moments and tails {worst:.3e}, quantiles {worst_q:.3e}")
            return
        for name, size in pool.imap_unordered(generate, names):
            print(f"{name}: {size} bytes", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
