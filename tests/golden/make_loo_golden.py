"""Generates tests/golden/loo_<case>_<set>_n<samples>.npz: what bb_ppc_loo must return for the cases of tests/_loo_cases.py, as a
50-digit mpmath evaluation of the formulas of include/barbay_hip.h on the float64 inputs (y, mu_j, sigma_j) of the numpy
restatement there (`_loo_cases.restate` with this file's `cell_mp` / `row_mp` in place of its float64 ones).  Everything here is
produced by this repository's code from seeded numpy draws; mpmath is needed to generate the files, not to read them.

Usage:  python tests/golden/make_loo_golden.py [name ...]        (all: about ten minutes on 8 cores)

Stored per file: the five per-cell outputs [rows, n_steps] (NaN: unscored; khat +Inf: unsmoothed), the six per-row outputs
(row_elpd_cells the 50-digit sum of the 50-digit cells, rounded once) and n_scored, for the rows `_loo_cases.golden_cases` names.
Before anything is written the generator asserts what the cases are for (`_loo_cases.check_bands`): cells in each band of khat,
no c within 1 of -690, some beyond it; and that the n = 25 seeds are the ones `find_seed25` finds (--find-seeds prints them)."""
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for _p in (TESTS, os.path.dirname(TESTS)):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import _loo_cases as lc  # noqa: E402


def psis_mp(l):
    """`_loo_cases.psis` at 50 digits on a list of mpf."""
    import mpmath as mp
    n = len(l)

    def lse(v):
        top = max(v)
        return top + mp.log(mp.fsum(mp.exp(x - top) for x in v))

    lpd = lse(l) - mp.log(n)
    a = [-x for x in l]
    A = max(a)
    r = [x - A for x in a]
    M = lc.tail_len(n)
    lw = list(r)
    khat, c = mp.inf, mp.nan
    if M >= 5:
        order = sorted(range(n), key=lambda j: (r[j], j))
        tail = order[n - M:]
        c = r[order[n - M - 1]]
        if c >= -690:
            ec = mp.exp(c)
            x = [mp.exp(r[j]) - ec for j in tail]
            xstar = x[(M + 2) // 4 - 1]
            if xstar > 0:
                m = 30 + int(mp.floor(mp.sqrt(M)))
                th = [1 / x[M - 1] + (1 - mp.sqrt(mp.mpf(m) / (i - mp.mpf(1) / 2))) / (3 * xstar) for i in range(1, m + 1)]

                def kappa(t):
                    return mp.fsum(mp.log1p(-t * xk) for xk in x) / M

                kap = [kappa(t) for t in th]
                L = [M * (mp.log(-t / k) - k - 1) for t, k in zip(th, kap)]
                w = [1 / mp.fsum(mp.exp(Lj - Li) for Lj in L) for Li in L]
                thh = mp.fsum(t * wi for t, wi in zip(th, w))
                kraw = kappa(thh)
                sig = -kraw / thh
                khat = (M * kraw + 5) / (M + 10)
                for i, j in enumerate(tail):
                    p = (mp.mpf(i + 1) - mp.mpf(1) / 2) / M
                    v = mp.log(sig * mp.expm1(-khat * mp.log1p(-p)) / khat + ec)
                    lw[j] = mp.mpf(0) if v > 0 else v
    ls = lse(lw)
    elpd = lse([a_ + b_ for a_, b_ in zip(lw, l)]) - ls
    neff = 1 / mp.fsum(mp.exp(x - ls) ** 2 for x in lw)
    return (elpd, lpd - elpd, khat, neff, lpd), c


def cell_mp(y, mu, sd):
    import mpmath as mp
    mp.mp.dps = 50
    Y = mp.mpf(y)
    half_log2pi = mp.log(2 * mp.pi) / 2
    l = []
    for m, s in zip(mu, sd):
        m, s = mp.mpf(float(m)), mp.mpf(float(s))
        z = (Y - m) / s
        l.append(-z * z / 2 - mp.log(s) - half_log2pi)
    return l, psis_mp(l)


def row_mp(ls):
    import mpmath as mp
    mp.mp.dps = 50
    return psis_mp([mp.fsum(col) for col in zip(*ls)])


def generate(name):
    sp, mu, om, n, rows, seed = lc.case_of(name)
    d = lc.restate(sp, mu, om, n, seed, rows=rows, cell=cell_mp, row=row_mp)
    np.savez_compressed(lc.golden_path(name), **d)
    return name, os.path.getsize(lc.golden_path(name))


def find_seed25(case, pset, limit=5e-14):
    """The first seed >= SEED at which the float64 restatement of the n = 25 rows is within `limit` of the 50-digit values and
    moves by no more than `limit` when every l_j moves by one ulp."""
    sp, mu, om = lc.inputs(case, pset)
    rows = lc.rows25(sp)
    seed = lc.SEED
    while True:
        if lc.sensitivity(sp, mu, om, 25, seed, rows) <= limit:
            ref = lc.restate(sp, mu, om, 25, seed, rows=rows, cell=cell_mp, row=row_mp)
            if max(lc.errors(lc.restate(sp, mu, om, 25, seed, rows=rows), ref).values()) <= limit:
                return seed
        seed += 1


def main(argv):
    if argv == ["--find-seeds"]:
        print({k: find_seed25(*k) for k in lc.SEED25})
        return
    print("bands (khat < 0.5, 0.5 .. 0.7, > 0.7, c < -690):", lc.check_bands(), flush=True)
    for (case, pset), seed in lc.SEED25.items():
        assert find_seed25(case, pset) == seed, (case, pset)
    names = argv or list(lc.golden_cases())
    names.sort(key=lambda k: -lc.golden_cases()[k][2] * (1 if lc.golden_cases()[k][3] is None else 0.1))          # longest first
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        for name, size in pool.imap_unordered(generate, names):
            print("done", name, size, "bytes", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
