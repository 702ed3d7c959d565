"""Generates tests/golden/logsigma_rb_<block>_<case>_n<samples>.npz: what bb_logsigma_rb must return for the cases of
tests/_logsigma_rb_cases.py, as a 50-digit mpmath evaluation of the rule of include/barbay_hip.h -- the same rule: the log-domain
Newton with its stopping test, the grid with its refinement and right extent, the Euler-Maclaurin-corrected CDF, the 40-step bisection -- on the float64 per-draw
inputs (l_j, SS_j, n, a, 1 / b^2) of the numpy restatement there.  Everything here is produced by this repository's code from seeded
numpy draws; mpmath is needed to generate the files, not to read them.

Usage:  python tests/golden/make_logsigma_rb_golden.py [name ...]        (all: some minutes on 8 cores)
        python tests/golden/make_logsigma_rb_golden.py --truth            logsigma_rb_truth.npz: mpmath.quad of the density itself
        python tests/golden/make_logsigma_rb_golden.py --measure          the float64 restatement's error against the stored files

Stored per file: q_mean, q_sd, rb_mean, rb_sd, sigma_mean, mode_mean, n_terms for the entries `_logsigma_rb_cases.golden_cases`
names; at n_samples = 2 and 111 also q_entries (three entries, one entry) and quantiles [len(q_entries), 3], the 50-digit bisection (it
costs 120 CDFs of 129 nodes or more per draw: it is made where it is affordable).  The largest file is a few KB.
The truth file: per parameter set (n, SS, a, ib2) the mode, ln Z, E, V by `mpmath.quad` at 40 digits over [l* - 60 delta,
l* + 60 delta'] split at the mode, and the CDF at l* + {-2.3, -0.7, 0.11, 1.9, 4.4} delta; the sets are 14 spanning the ranges of use (n from 0 to
1000, SS from 1e-300 to 1e6, b from 0.2 to 3) and a few per-draw sets of every case."""
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for _p in (HERE, TESTS, os.path.dirname(TESTS)):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import _logsigma_rb_cases as lc  # noqa: E402

QGOLD = {2: 3, 111: 1}     # n_samples -> entries with a 50-digit bisection


def _mp():
    import mpmath
    mpmath.mp.dps = 50
    return mpmath


class CondMp:
    """One draw's conditional about its mode, 50 digits, the rule as it stands."""

    def __init__(self, SS, n, a, ib2):
        mp = _mp()
        f = mp.mpf
        SS, n, a, ib2 = f(float(SS)), f(int(n)), f(float(a)), f(float(ib2))
        if SS == 0:
            lm = a - n / ib2
        else:
            c2 = 2 / ib2
            lnK = mp.log(SS) - 2 * a + c2 * n
            t = mp.log(lnK / c2) if lnK >= c2 else lnK
            for _ in range(50):
                et = mp.exp(t)
                step = ((t + c2 * et) - lnK) / (1 + c2 * et)
                t -= step
                if abs(step) <= f(2) ** -40 * (1 + abs(t)):
                    break
            lm = a + (mp.exp(t) - n) / ib2
        self.mp, self.a, self.ib2, self.n, self.lm = mp, a, ib2, n, lm
        self.W = SS * mp.exp(-2 * lm) if SS != 0 else f(0)
        self.c1 = ib2 * (lm - a) + n
        self.dl = 1 / mp.sqrt(ib2 + 2 * self.W)
        self.m = min(max(1, int(mp.ceil(2 * self.dl))), lc.REFINE_MAX)
        self.r = 1
        while self.r < lc.RIGHT_MAX and mp.log(self.p(lc.RIGHT * self.r * self.dl)[0]) > lc.TAIL:
            self.r *= 2
        self.s = self.dl / (4 * self.m)
        self.nleft, self.nright = lc.LEFT * 4 * self.m, lc.RIGHT * self.r * 4 * self.m
        self.lo, self.hi = lm - 10 * self.dl, lm + self.nright * self.s

    def p(self, u):
        mp = self.mp
        x = mp.expm1(-2 * u)
        return mp.exp(-(u * self.c1) - self.ib2 * (u * u) / 2 - self.W * x / 2), x

    def dh(self, u, em1):
        return -((self.lm + u) - self.a) * self.ib2 - self.n + self.W * (em1 + 1)

    def moments(self):
        mp = self.mp
        s, nodes = self.s, self.nleft + self.nright
        z = m1 = m2 = se = mp.mpf(0)
        for k in range(nodes + 1):
            uk = (k - self.nleft) * s
            p, _ = self.p(uk)
            if k in (0, nodes):
                p = p / 2
            z += p
            m1 += p * uk
            m2 += p * uk * uk
            se += p * mp.exp(uk)
        r1 = m1 / z
        self.Z = s * z
        return self.Z, self.lm + r1, m2 / z - r1 * r1, mp.exp(self.lm) * (se / z)

    def cdf(self, x):
        mp = self.mp
        if x <= self.lo:
            return mp.mpf(0)
        if x >= self.hi:
            return mp.mpf(1)
        ulo, s = -10 * self.dl, self.s
        r = x - (self.lm + ulo)
        N = max(1, int(mp.ceil(r / s)))
        sx = r / N
        p0, e0 = self.p(ulo)
        ux = x - self.lm
        p1, e1 = self.p(ux)
        acc = p0 / 2
        for i in range(1, N):
            acc += self.p(ulo + i * sx)[0]
        acc += p1 / 2
        v = (sx * acc - sx * sx / 12 * (self.dh(ux, e1) * p1 - self.dh(ulo, e0) * p0)) / self.Z
        return min(max(v, mp.mpf(0)), mp.mpf(1))


def entry_mp(l, SS, n, a, ib2, probs, want_q=True):
    mp = _mp()
    f = mp.mpf
    ns = l.shape[0]
    if not (np.all(np.isfinite(SS)) and np.all(np.isfinite(l))):
        raise ValueError("the goldens are made on finite inputs")
    cs = [CondMp(SS[j], n, a, ib2) for j in range(ns)]
    mom = [c.moments() for c in cs]
    lj = [f(float(x)) for x in l]
    qm = mp.fsum(lj) / ns
    rm = mp.fsum(m[1] for m in mom) / ns
    vals = [qm, mp.sqrt(mp.fsum((x - qm) ** 2 for x in lj) / ns), rm,
            mp.sqrt(mp.fsum(m[2] for m in mom) / ns + mp.fsum((m[1] - rm) ** 2 for m in mom) / ns),
            mp.fsum(m[3] for m in mom) / ns, mp.fsum(c.lm for c in cs) / ns]
    qs = []
    for p in (probs if want_q else ()):
        lo, hi = min(c.lo for c in cs), max(c.hi for c in cs)
        for _ in range(lc.ITER):
            x = lo + (hi - lo) / 2
            if mp.fsum(c.cdf(x) for c in cs) / ns < f(float(p)):
                lo = x
            else:
                hi = x
        qs.append(lo + (hi - lo) / 2)
    return vals, qs


def generate(name):
    blk, case, n, entries = lc.golden_cases()[name]
    sp, mu, om = lc.inputs(case)
    ne = lc.n_entries(sp, blk)
    ents = list(range(ne)) if entries is None else list(entries)
    d = lc.restate(sp, blk, mu, om, n, lc.SEED, entries=ents, entry=entry_mp, quirk=lc.quirk_of(case), want_q=False)
    d.pop("quantiles")
    if n in QGOLD:
        qe = [u for u, nt in zip(ents, d["n_terms"]) if nt > 0][:QGOLD[n]]      # (not a prior-only entry: `_logsigma_rb_cases.check_golden`)
        q = lc.restate(sp, blk, mu, om, n, lc.SEED, entries=qe, entry=entry_mp, quirk=lc.quirk_of(case))
        d["q_entries"] = np.array(qe, dtype=np.int64)
        d["quantiles"] = q["quantiles"]
    np.savez_compressed(lc.golden_path(name), **d)
    return name, os.path.getsize(lc.golden_path(name))


def measure(name):
    blk, case, n, entries = lc.golden_cases()[name]
    sp, mu, om = lc.inputs(case)
    ref = lc.golden(name)
    ne = lc.n_entries(sp, blk)
    ents = list(range(ne)) if entries is None else list(entries)
    got = lc.restate(sp, blk, mu, om, n, lc.SEED, entries=ents, quirk=lc.quirk_of(case), want_q=False)
    err = lc.errors(got, {k: ref[k] for k in lc.UNITS + ("n_terms",)}, lc.UNITS)
    if "quantiles" in ref:
        q = lc.restate(sp, blk, mu, om, n, lc.SEED, entries=[int(x) for x in ref["q_entries"]], quirk=lc.quirk_of(case))
        err["quantiles"] = lc.errors({"quantiles": q["quantiles"], "n_terms": 0}, {"quantiles": ref["quantiles"], "n_terms": 0}, ("quantiles",))["quantiles"]
    return name, err


# ---- the rule against the truth ----------------------------------------------------------------------------------------------------
FURTHER_SETS = [(0, 0.0, 0.0, 1.0), (0, 0.0, -1.3, 0.2), (1, 1e-300, 0.0, 1.0), (1, 1e-6, 0.0, 3.0), (2, 0.3, -1.0, 1.0), (4, 1.0, 0.0, 1.0),
              (4, 40.0, 0.5, 0.2), (7, 1e-3, -2.0, 2.0), (10, 1e2, 0.0, 1.0), (50, 3.0, -1.0, 0.5), (260, 12.0, 0.0, 1.0),
              (1000, 1e6, 0.0, 1.0), (1000, 1e-2, 1.0, 3.0), (1000, 250.0, -1.0, 0.2)]      # (n, SS, a, b)


def truth_sets():
    sets = [(n, SS, a, 1.0 / (b * b)) for n, SS, a, b in FURTHER_SETS]
    for blk in lc.BLOCKS:
        for case in lc.SHAPES:
            sp, mu, om = lc.inputs(case)
            ne = lc.n_entries(sp, blk)
            ents = sorted({0, ne // 2, ne - 1})
            ci = lc.cond_inputs(sp, lc.draws_of(sp, mu, om, 2, lc.SEED), 2, blk, entries=ents, quirk=lc.quirk_of(case))
            sets += [(ci[u][2], float(ci[u][1][0]), float(ci[u][3]), float(ci[u][4])) for u in ents]
    return sets


def truth_one(s):
    import mpmath as mp
    mp.mp.dps = 50
    n, SS, a, ib2 = s
    c = CondMp(SS, n, a, ib2)
    mp.mp.dps = 40
    f = mp.mpf
    SSm, nm = f(float(SS)), f(int(n))

    def dens(x):                                                  # exp(h(x) - h(l*)), h as the header writes it
        h = lambda y: -(y - c.a) ** 2 * c.ib2 / 2 - nm * y - SSm / 2 * mp.exp(-2 * y)
        return mp.exp(h(x) - h(c.lm))
    b = 1 / mp.sqrt(c.ib2)
    pts = [c.lm - 60 * c.dl, c.lm - 8 * c.dl, c.lm, c.lm + 8 * c.dl, c.lm + 40 * c.dl, c.lm + 40 * c.dl + 40 * b]
    Z = mp.quad(dens, pts)
    E = mp.quad(lambda x: x * dens(x), pts) / Z
    V = mp.quad(lambda x: (x - E) ** 2 * dens(x), pts) / Z
    C = [mp.quad(dens, [pts[0], pts[1], c.lm + f(m) * c.dl] if m > -8 else [pts[0], c.lm + f(m) * c.dl]) / Z for m in lc.TRUTH_AT]
    return [float(c.lm), float(mp.log(Z)), float(E), float(V)] + [float(x) for x in C]


def main(argv):
    flags = [a for a in argv if a.startswith("--")]
    names = [a for a in argv if not a.startswith("--")] or list(lc.golden_cases())
    cost = lambda k: -lc.golden_cases()[k][2] * (len(lc.golden_cases()[k][3] or ()) or lc.n_entries(lc.spec(lc.golden_cases()[k][1]), lc.golden_cases()[k][0]))
    names.sort(key=cost)                                           # longest first
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        if "--truth" in flags:
            sets = truth_sets()
            rows = np.array(pool.map(truth_one, sets))
            np.savez_compressed(lc.truth_path(), n=np.array([s[0] for s in sets], dtype=np.int64), SS=np.array([s[1] for s in sets]),
                                a=np.array([s[2] for s in sets]), ib2=np.array([s[3] for s in sets]),
                                mode=rows[:, 0], lnZ=rows[:, 1], E=rows[:, 2], V=rows[:, 3], C=rows[:, 4:])
            print(f"{lc.truth_path()}: {len(sets)} parameter sets")
            return
        if "--measure" in flags:
            worst, worst_q = 0.0, 0.0
            for name, err in pool.imap_unordered(measure, names):
                lc.report(name, "restatement", err)
                worst = max(worst, max(err[k] for k in lc.UNITS))
                worst_q = max(worst_q, err.get("quantiles", 0.0))
            print(f"largest error of the float64 restatement: moments {worst:.3e}, quantiles {worst_q:.3e}")
            return
        for name, size in pool.imap_unordered(generate, names):
            print(f"{name}: {size} bytes", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
