"""Generates tests/golden/pop_rb_<case>_n<samples>.npz: what bb_popmean_rb must return for the cases of tests/_pop_rb_cases.py,
as a 50-digit mpmath evaluation of the formulas of include/barbay_hip.h on the float64 inputs (sbar_j, m_j, sd_j) of the numpy
restatement there (`_pop_rb_cases.restate` with `make_rb_golden.unit_mp` in place of its float64 unit; a quantile is the 50-digit
root of the mixture CDF).  Everything here is produced by this repository's code from seeded numpy draws; mpmath is needed to
generate the files, not to read them.

Usage:  python tests/golden/make_pop_rb_golden.py [name ...]        (all: a few minutes on 8 cores)

Stored per file: q_mean, q_sd, rb_mean, rb_sd, p_pos, p_neg [groups], quantiles [groups, 3], n_members and threshold [groups] --
the threshold of a group's p_pos / p_neg, `_pop_rb_cases.nearest` its float64 rb_mean -- for the groups
`_pop_rb_cases.golden_cases` names (all groups but for the largest call).  The largest file is a few KB.
Before anything is written the generator checks, on the restatement, that |m_j - s0| / sd_j <= 20 holds for every group.
With --measure: prints, per file, the float64 restatement's error against the stored values and the largest over all files (the
figures `_pop_rb_cases.MEASURED` and `Q_MEASURED` record)."""
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for _p in (HERE, TESTS, os.path.dirname(TESTS)):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import _pop_rb_cases as qc  # noqa: E402
from make_rb_golden import unit_mp  # noqa: E402


def generate(name):
    case, n, groups = qc.golden_cases()[name]
    sp, mu, om = qc.inputs(case)
    quirk = qc.quirk_of(case)
    z = qc.restate(sp, mu, om, n, qc.SEED, threshold=None, probs=(), groups=groups, want_z=True, quirk=quirk)["zmax"]
    assert z.max() <= qc.Z_HI, (name, z.max())
    d = qc.restate(sp, mu, om, n, qc.SEED, threshold=None, groups=groups, unit=unit_mp, quirk=quirk)
    np.savez_compressed(qc.golden_path(name), **d)
    return name, os.path.getsize(qc.golden_path(name))


def measure(name):
    case, n, groups = qc.golden_cases()[name]
    sp, mu, om = qc.inputs(case)
    ref = qc.golden(name)
    return name, qc.errors(qc.restate(sp, mu, om, n, qc.SEED, threshold=ref["threshold"], groups=groups, quirk=qc.quirk_of(case)), ref)


def main(argv):
    meas = "--measure" in argv
    names = [a for a in argv if a != "--measure"] or list(qc.golden_cases())
    names.sort(key=lambda k: -qc.golden_cases()[k][1] * (len(qc.golden_cases()[k][2] or ()) or 10))      # longest first
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        if meas:
            worst, worst_q = 0.0, 0.0
            for name, err in pool.imap_unordered(measure, names):
                qc.report(name, "restatement", err)
                worst = max(worst, max(err[k] for k in qc.UNITS))
                worst_q = max(worst_q, err["quantiles"])
            print(f"largest error of the float64 restatement: moments and tails {worst:.3e}, quantiles {worst_q:.3e}")
            return
        for name, size in pool.imap_unordered(generate, names):
            print(f"{name}: {size} bytes", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
