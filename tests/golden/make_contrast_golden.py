"""Generates tests/golden/contrast_<case>_n<samples>.npz: what bb_contrast_rb must return for the multi-term contrasts of
tests/_contrast_cases.py, as a 50-digit mpmath evaluation (`make_rb_golden.unit_mp`: moments, both tails, the 50-digit ROOT of the
mixture CDF) of the header's formulas on the float64 (d_j, M_j, sd_j) of the numpy restatement there.  A contrast's tails are taken
at the multiple of 1 / `_contrast_cases.GRID` nearest its rb_mean, stored with it.  Everything here is produced by this
repository's code from seeded numpy draws; mpmath is needed to generate the files, not to read them.

Usage:  python tests/golden/make_contrast_golden.py [case_nN ...]        (all: a few minutes on 8 cores)

Stored per file, for each space the case has, prefixed f_ (fitness units) or t_ (theta groups): q_mean, q_sd, rb_mean, rb_sd,
p_pos, p_neg [contrasts], quantiles [contrasts, 3], min_steps, threshold, for the contrasts `_contrast_cases.golden_terms` names.
The largest file is a few KB.
With --measure: prints, per file and space, the float64 restatement's error against the stored values (the figures
`_contrast_cases.MEASURED` and `Q_MEASURED` record)."""
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for _p in (HERE, TESTS, os.path.dirname(TESTS)):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import _contrast_cases as cc  # noqa: E402
from make_rb_golden import unit_mp  # noqa: E402


def files():
    """file stem -> the golden names (one per space) it holds."""
    out = {}
    for name in cc.golden_cases():
        out.setdefault(name.split(":")[1], []).append(name)
    return out


def generate(stem):
    d = {}
    for name in files()[stem]:
        space, case, n = cc.golden_cases()[name]
        res = cc.restate(cc.elements_at(space, case, n), cc.golden_terms(name), unit=unit_mp)
        d.update({f"{space[0]}_{k}": v for k, v in res.items()})
    path = os.path.join(cc.rc.GOLD, f"contrast_{stem}.npz")
    np.savez_compressed(path, **d)
    return stem, os.path.getsize(path)


def measure(name):
    space, case, n = cc.golden_cases()[name]
    ref = dict(cc.golden(name))
    s0 = ref.pop("threshold")
    return name, cc.errors(cc.restate(cc.elements_at(space, case, n), cc.golden_terms(name), threshold=s0), ref)


def main(argv):
    meas = "--measure" in argv
    stems = [a for a in argv if a != "--measure"] or list(files())
    stems.sort(key=lambda k: -int(k.rsplit("_n", 1)[1]))          # longest first
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        if meas:
            worst, qworst = 0.0, 0.0
            for name, err in pool.imap_unordered(measure, [n for s in stems for n in files()[s]]):
                cc.report(name, "restatement", err)
                worst, qworst = max([worst] + [err[k] for k in cc.UNITS]), max(qworst, err["quantiles"])
            print(f"largest error of the float64 restatement: moments and tails {worst:.3e}, quantiles {qworst:.3e}")
            return
        for stem, size in pool.imap_unordered(generate, stems):
            print(f"{stem}: {size} bytes", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
