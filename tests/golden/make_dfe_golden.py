"""Generates tests/golden/dfe_<case>_n<samples>.npz: what bb_dfe_rb must return for the sets of tests/_dfe_cases.py, as a 50-digit
mpmath evaluation of the header's formulas on the float64 (s_j, m_j, sd_j) of the numpy restatement (`_rb_cases.conditionals`):
both tails of every (unit, threshold, draw) through a 50-digit erfc, every sum exact to 50 digits, the quantiles over the draws
by the type-7 rule on the 50-digit fractions.  The grid of a file is `_dfe_cases.level_grid`, the multiples of 1 / 1024 nearest
the 10 / 25 / 50 / 75 / 90 % points of the units' rb_mean, stored with the values.  Everything here is produced by this
repository's code from seeded numpy draws; mpmath is needed to generate the files, not to read them.

Usage:  python tests/golden/make_dfe_golden.py [case_nN ...]        (all: some ten minutes on 8 cores)

Stored per file: grid [5], below_mean, above_mean, between_sd, within_sd, q_below_mean, q_below_sd [sets, 5], below_bands,
above_bands [sets, 5, 3], n_units [sets], for the sets `_dfe_cases.golden_sets` names.  The largest file is a few KB.
With --measure: prints, per file, the float64 restatement's error against the stored values (the figures `_dfe_cases.MEASURED`
records)."""
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for _p in (HERE, TESTS, os.path.dirname(TESTS)):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import _dfe_cases as dc  # noqa: E402


def unit_tails(args):
    """(pl, pu) [n_grid][n] of one unit, 50 digits."""
    import mpmath as mp
    mp.mp.dps = 50
    m, sd, grid = args
    r2 = mp.sqrt(2)
    pl, pu = [], []
    for x in grid:
        v = [(mp.mpf(float(a)) - mp.mpf(float(x))) / (mp.mpf(float(b)) * r2) for a, b in zip(m, sd)]
        pl.append([mp.erfc(z) / 2 for z in v])
        pu.append([mp.erfc(-z) / 2 for z in v])
    return pl, pu


def quantile7_mp(xs, p):
    """StatsBase.quantile (type 7) of the sorted 50-digit values xs."""
    import mpmath as mp
    K = len(xs)
    h = (K - 1) * mp.mpf(float(p))
    j = min(max(int(mp.floor(h)), 0), K - 2)
    return xs[j] + (h - j) * (xs[j + 1] - xs[j])


def generate(pool, name):
    import mpmath as mp
    mp.mp.dps = 50
    case, n = dc.golden_cases()[name]
    sets = dc.golden_sets(name)
    grid = dc.level_grid(case, n)
    s, m, sd, _ = dc.elements_at(case, n)
    units = sorted({u for st in sets for u in st})
    tails = dict(zip(units, pool.imap(unit_tails, [(m[u], sd[u], grid) for u in units], chunksize=1)))
    ng = len(grid)
    out = {k: np.empty((len(sets), ng)) for k in dc.CELLS}
    out.update({k: np.empty((len(sets), ng, len(dc.PROBS))) for k in dc.BANDS})
    out["n_units"] = np.array([len(st) for st in sets], dtype=np.int64)
    out["grid"] = np.asarray(grid, dtype=np.float64)
    for c, st in enumerate(sets):
        nu = len(st)
        for g, x in enumerate(grid):
            L = [mp.fsum(tails[u][0][g][j] for u in st) / nu for j in range(n)]
            U = [mp.fsum(tails[u][1][g][j] for u in st) / nu for j in range(n)]
            V = [mp.fsum(tails[u][0][g][j] * tails[u][1][g][j] for u in st) / (nu * nu) for j in range(n)]
            Cq = [mp.mpf(int(sum(1 for u in st if s[u][j] <= x))) / nu for j in range(n)]
            lm, cm = mp.fsum(L) / n, mp.fsum(Cq) / n
            out["below_mean"][c, g] = float(lm)
            out["above_mean"][c, g] = float(mp.fsum(U) / n)
            out["between_sd"][c, g] = float(mp.sqrt(mp.fsum((v - lm) ** 2 for v in L) / n))
            out["within_sd"][c, g] = float(mp.sqrt(mp.fsum(V) / n))
            out["q_below_mean"][c, g] = float(cm)
            out["q_below_sd"][c, g] = float(mp.sqrt(mp.fsum((v - cm) ** 2 for v in Cq) / n))
            for k, F in (("below_bands", sorted(L)), ("above_bands", sorted(U))):
                out[k][c, g] = [float(quantile7_mp(F, p)) for p in dc.PROBS]
    path = dc.golden_path(name)
    np.savez_compressed(path, **out)
    return os.path.getsize(path)


def measure(name):
    case, n = dc.golden_cases()[name]
    ref = dict(dc.golden(name))
    grid = ref.pop("grid")
    return name, dc.errors(dc.restate(dc.elements_at(case, n), dc.golden_sets(name), grid), ref)


def main(argv):
    meas = "--measure" in argv
    names = [a for a in argv if a != "--measure"] or sorted(dc.golden_cases())
    names.sort(key=lambda k: -int(k.rsplit("_n", 1)[1]))          # longest first
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        if meas:
            worst = {k: 0.0 for k in dc.VALUES}
            for name in names:
                _, err = measure(name)
                dc.report(name, "restatement", err)
                worst = {k: max(worst[k], err[k]) for k in worst}
            print("largest error of the float64 restatement: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
            return
        for name in names:
            print(f"{name}: {generate(pool, name)} bytes", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
