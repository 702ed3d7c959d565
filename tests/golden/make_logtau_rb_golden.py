"""Generates tests/golden/logtau_rb_<mode>_<case>_n<samples>.npz: what bb_logtau_rb must return for the cases of
tests/_logtau_rb_cases.py, as a 50-digit mpmath evaluation of the rule of include/barbay_hip.h -- the same statements (`Cond` and
`entry` there, run with the mpmath arithmetic): the segments, the safeguarded mode iteration with its stopping test, the kept modes,
the grid with its refinement and reach, the Euler-Maclaurin-corrected CDF, the 40-step bisection -- on the float64 per-draw inputs
(l_j, n, w_j, tt_j, Y_j, a, 1 / b^2) of the numpy restatement.  Everything here is produced by this repository's code from seeded
numpy draws; mpmath is needed to generate the files, not to read them.

Usage:  python tests/golden/make_logtau_rb_golden.py [name ...]        (all: some minutes on 8 cores)
        python tests/golden/make_logtau_rb_golden.py --truth            logtau_rb_truth.npz: mpmath.quad of the density itself
        python tests/golden/make_logtau_rb_golden.py --measure          the float64 restatement's error against the stored files

Stored per file: q_mean, q_sd, rb_mean, rb_sd, tau_mean, pool_mean, mode_mean, n_terms, n_two_modes for the entries
`_logtau_rb_cases.golden_cases` names; at n_samples = 2 also q_entries (one entry) and quantiles [1, 3], the 50-digit bisection.
The truth file: per parameter set (mode, n, w, tt, Y, a, ib2) the kept modes' number, the global mode, ln Z (about the global
mode), E, V, E[e^l], the pooling expectation by `mpmath.quad` at 40 digits over [a - 12 b - 30, a + 12 b + 30] split at and around
every mode -- the modes found by a scan of h' for sign changes at a step of (24 b + 60) / 20000, not by the rule -- and the CDF
at x = E + {-2.3, -0.7, 0.11, 1.9, 4.4} sd (x stored).  The sets: seven from a sweep over parameters of use (six bimodal), sets
with n = 0, tt = 0, Y = 0, w from 1e-6 to 1e8, b from 0.2 to 3, and per-draw sets of every case in both modes."""
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for _p in (HERE, TESTS, os.path.dirname(TESTS)):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import _logtau_rb_cases as tc  # noqa: E402

F, C = tc.FULL, tc.COLLAPSED
# (mode, n, w, tt, Y, a, b)
FURTHER_SETS = [
    (F, 8, 22.5, 0.035, 2.86, -2, 1), (C, 1, 6.5, 0.0, 3.23, -4, 0.5),
    (F, 3, 1.5, 0.088, 8.0, -2, 1), (F, 2, 178, 0.031, 0.377, -2, 1), (F, 4, 45, 0.16, 3.375, -4, 0.5), (F, 6, 4.0, 0.0205, 2.62, -2, 3),
    (F, 4, 1e4, -1.5, 1.0, -2, 1),
    (F, 0, 1.0, 0.3, 0.0, -2, 1), (C, 0, 1.0, 0.3, 0.0, -1.3, 0.2), (F, 3, 10.0, 0.0, 1.0, -2, 1), (F, 3, 10.0, 0.7, 0.0, -2, 1),
    (C, 3, 10.0, 0.0, 0.0, -2, 1), (F, 2, 1e-6, 1.0, 2.0, 0, 3), (C, 2, 1e-6, 0.0, 2.0, 0, 3), (F, 5, 1e8, 0.5, 0.3, -2, 0.2),
    (C, 5, 1e8, 0.0, 0.3, -2, 0.2), (F, 8, 1e6, 0.02, 1.5, -2, 1), (C, 8, 1e6, 0.0, 1.5, -2, 2), (C, 4, 100.0, 0.0, 0.01, -1, 1),
    (F, 1, 3.0, 1.2, -2.0, 0, 2), (C, 2, 30.0, 0.0, 1.9, -3.5, 0.4), (F, 5, 12.0, -0.05, -2.4, -2, 1),
]


def _mp(dps=50):
    import mpmath
    mpmath.mp.dps = dps
    return mpmath


def generate(name):
    _mp()
    be = tc.MP()
    mode, case, n, ents = tc.golden_cases()[name]
    sp, mu, om = tc.inputs(case)
    d = tc.restate(sp, mode, mu, om, n, tc.SEED, entries=list(ents), be=be, want_q=False)
    d.pop("quantiles")
    if n == 2:
        qe = [u for u, nt in zip(ents, d["n_terms"]) if nt > 0][:1]
        q = tc.restate(sp, mode, mu, om, n, tc.SEED, entries=qe, be=be)
        d["q_entries"] = np.array(qe, dtype=np.int64)
        d["quantiles"] = q["quantiles"]
    np.savez_compressed(tc.golden_path(name), **d)
    return name, os.path.getsize(tc.golden_path(name))


def measure(name):
    mode, case, n, ents = tc.golden_cases()[name]
    sp, mu, om = tc.inputs(case)
    ref = tc.golden(name)
    got = tc.restate(sp, mode, mu, om, n, tc.SEED, entries=list(ents), want_q=False)
    err = tc.errors(got, {k: ref[k] for k in tc.UNITS + ("n_terms", "n_two_modes")}, tc.UNITS)
    if "quantiles" in ref:
        q = tc.restate(sp, mode, mu, om, n, tc.SEED, entries=[int(x) for x in ref["q_entries"]])
        err["quantiles"] = tc.errors({"quantiles": q["quantiles"]}, {"quantiles": ref["quantiles"]}, ("quantiles",))["quantiles"]
    return name, err


# ---- the rule against the truth ----------------------------------------------------------------------------------------------------
def truth_sets():
    sets = [(m, n, float(w), float(tt), float(Y), float(a), 1.0 / (float(b) * float(b))) for m, n, w, tt, Y, a, b in FURTHER_SETS]
    for case in tc.SHAPES + (tc.PRIOR_ONLY,):
        sp, mu, om = tc.inputs(case)
        ne = tc.n_entries(sp)
        ents = sorted({0, ne // 2, ne - 1})
        ci = tc.cond_inputs(sp, tc.lc.draws_of(sp, mu, om, 2, tc.SEED), 2, entries=ents)
        for u in ents:
            l, nt, w, tt, Y, a, ib2 = ci[u]
            sets += [(m, int(nt), float(w[0]), float(tt[0]), float(Y[0]), float(a), float(ib2)) for m in (F, C)]
    return sets


def truth_one(s):
    mp = _mp(40)
    f = mp.mpf
    mode, n, w, tt, Y, a, ib2 = s
    n_, w, tt, Y, a, ib2 = f(n), f(w), f(tt), f(Y), f(a), f(ib2)
    b = 1 / mp.sqrt(ib2)
    if n == 0:
        h = lambda l: -(l - a) ** 2 * ib2 / 2
        d1 = lambda l: -(l - a) * ib2
    elif mode == F:
        A, B = n_ * w * tt * tt / 2, w * tt * Y
        h = lambda l: -(l - a) ** 2 * ib2 / 2 - A * mp.exp(2 * l) + B * mp.exp(l)
        d1 = lambda l: -(l - a) * ib2 + mp.exp(l) * (B - 2 * A * mp.exp(l))
    else:
        v, q = 1 / (n_ * w), (Y / n_) ** 2
        h = lambda l: -(l - a) ** 2 * ib2 / 2 - mp.log(mp.exp(2 * l) + v) / 2 - q / (2 * (mp.exp(2 * l) + v))
        d1 = lambda l: -(l - a) * ib2 + mp.exp(2 * l) * (q - mp.exp(2 * l) - v) / (mp.exp(2 * l) + v) ** 2
    lo, hi = a - 12 * b - 30, a + 12 * b + 30
    xs = [lo + (hi - lo) * i / 20000 for i in range(20001)]
    ds = [d1(x) for x in xs]
    modes = [mp.findroot(d1, (xs[i], xs[i + 1]), solver="anderson", tol=1e-35) for i in range(20000) if ds[i] > 0 and ds[i + 1] <= 0]
    hm = max(h(m) for m in modes)
    glob = [m for m in modes if h(m) == hm][0]
    kept = [m for m in modes if h(m) - hm >= -40]
    dens = lambda x: mp.exp(h(x) - hm)
    pts = sorted({lo, hi} | {m + k * sc for m in modes for sc in (1, b) for k in (-3, -1, -0.3, -0.1, 0, 0.1, 0.3, 1, 3)})
    pts = [p for p in pts if lo <= p <= hi]
    Z = mp.quad(dens, pts)
    E = mp.quad(lambda x: x * dens(x), pts) / Z
    V = mp.quad(lambda x: (x - E) ** 2 * dens(x), pts) / Z
    T = mp.quad(lambda x: mp.exp(x) * dens(x), pts) / Z
    P = mp.quad(lambda x: dens(x) / (1 + n_ * w * mp.exp(2 * x)), pts) / Z if n else f(1)
    sd = mp.sqrt(V)
    xq = [E + f(m) * sd for m in tc.TRUTH_AT]
    Cs = [mp.quad(dens, [p for p in pts if p < x] + [x]) / Z for x in xq]
    return [float(len(kept)), float(glob), float(mp.log(Z)), float(E), float(V), float(T), float(P)] + [float(x) for x in xq] + [float(x) for x in Cs]


def main(argv):
    flags = [a for a in argv if a.startswith("--")]
    gc = tc.golden_cases()
    names = [a for a in argv if not a.startswith("--")] or list(gc)
    names.sort(key=lambda k: -gc[k][2] * len(gc[k][3]))          # longest first
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        if "--truth" in flags:
            sets = truth_sets()
            rows = np.array(pool.map(truth_one, sets, chunksize=1))
            k = len(tc.TRUTH_AT)
            np.savez_compressed(tc.golden_path("truth"), mode=np.array([s[0] for s in sets], dtype=np.int64), n=np.array([s[1] for s in sets], dtype=np.int64),
                                w=np.array([s[2] for s in sets]), tt=np.array([s[3] for s in sets]), Y=np.array([s[4] for s in sets]),
                                a=np.array([s[5] for s in sets]), ib2=np.array([s[6] for s in sets]), n_modes=rows[:, 0].astype(np.int64),
                                glob=rows[:, 1], lnZ=rows[:, 2], E=rows[:, 3], V=rows[:, 4], T=rows[:, 5], P=rows[:, 6], x=rows[:, 7:7 + k], C=rows[:, 7 + k:])
            print(f"{tc.golden_path('truth')}: {len(sets)} parameter sets, {int((rows[:, 0] == 2).sum())} bimodal")
            return
        if "--measure" in flags:
            worst, worst_q = 0.0, 0.0
            for name, err in pool.imap_unordered(measure, names):
                tc.report(name, "restatement", err)
                worst = max(worst, max(err[k] for k in tc.UNITS))
                worst_q = max(worst_q, err.get("quantiles", 0.0))
            print(f"largest error of the float64 restatement: moments {worst:.3e}, quantiles {worst_q:.3e}")
            return
        for name, size in pool.imap_unordered(generate, names):
            print(f"{name}: {size} bytes", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
