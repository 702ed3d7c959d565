#!/usr/bin/env python3
"""Writes tests/golden/llrb_<case>_n<samples>.npz and llrb_truth.npz (mpmath needed here, not by the tests).

    make_loglambda_rb_golden.py [name ...]     the named golden cases of `_loglambda_rb_cases.golden_cases` or `fitness_bimodal` (default: all): a
                                               50-digit evaluation of the rule of include/barbay_hip.h (bb_loglambda_rb) -- the very
                                               functions of the restatement over the `MP` backend -- on the restatement's float64
                                               per-draw inputs; cells without a golden are NaN
    make_loglambda_rb_golden.py --truth        llrb_truth.npz: mpmath.quad of exp(h) itself at 40 digits for `truth_sets`
    make_loglambda_rb_golden.py --measure      the float64 restatement against the goldens: the figures MEASURED / Q_MEASURED
"""
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
import _loglambda_rb_cases as lc      # noqa: E402


class MP:
    num = staticmethod(mp.mpf)
    exp, expm1, log, log1p, sqrt, ceil = (staticmethod(f) for f in (mp.exp, mp.expm1, mp.log, mp.log1p, mp.sqrt, mp.ceil))
    inf = mp.inf
    isfinite = staticmethod(lambda x: bool(mp.isfinite(x)))


def make(name):
    mp.mp.dps = 50
    if name == lc.BIMODAL:                     # the explicit two-mode draws: every entry of the row, moments and quantiles
        np.savez_compressed(lc.golden_path(name), **lc.restate_bimodal(M=MP))
        print("wrote", name, flush=True)
        return
    case, n, rows, gent, qent = lc.golden_cases()[name]
    sp, mu, om = lc.inputs(case)
    out = lc.restate(case, mu, om, n, lc.SEED, list(rows), M=MP, entries=None if gent is None else set(gent), qentries=set(qent))
    np.savez_compressed(lc.golden_path(name), **out)
    print("wrote", name, flush=True)


def truth():
    """ln Z (about the 50-digit global mode, as the rule's Z_j is: about x0 it can be 1e7, whose last double digit is 2e-9), E, V of exp(h) by adaptive quadrature split at the modes and the grid's ends, and the CDF at the float64
    rule's global mode + TRUTH_AT of its curvature scales (the points are stored: the test evaluates its CDF at the same doubles)."""
    mp.mp.dps = 40
    sets = lc.truth_sets()
    T = dict(sets=np.array(sets), lnZ=[], E=[], V=[], C=[], xs=[], n_modes=[])
    for st in sets:
        with np.errstate(all="ignore"):
            c64 = lc.Cond(lc.F64, *st)
            ca64, s64, nl64, nr64, _ = lc.setup(c64)
            dl64 = 1.0 / np.sqrt(-ca64.d12(np.float64(0.0))[1])
            xs = [float(ca64.x + at * dl64) for at in lc.TRUTH_AT]
        c0 = lc.Cond(MP, *st)
        ca, s, nl, nr, modes = lc.setup(c0)
        ustar = ca.x - c0.x
        lo, hi = ustar - nl * s, ustar + nr * s
        span = hi - lo
        pts = sorted({lo - span, lo, hi, hi + span / 4} | set(modes) | {ustar - s * 8, ustar + s * 8})
        g = lambda u: mp.exp(c0.lnp(u)[0])
        Z = mp.quad(g, pts)
        m1 = mp.quad(lambda u: g(u) * u, pts)
        E = m1 / Z
        V = mp.quad(lambda u: g(u) * (u - E) ** 2, pts) / Z
        Cs = []
        for x in xs:
            ux = mp.mpf(x) - c0.x
            sub = [p for p in pts if p < ux] + [ux]
            Cs.append(float(mp.quad(g, sub) / Z) if len(sub) > 1 else 0.0)
        T["lnZ"].append(float(mp.log(Z) - c0.lnp(ustar)[0])); T["E"].append(float(c0.x + E)); T["V"].append(float(V)); T["C"].append(Cs); T["xs"].append(xs)
        T["n_modes"].append(len(modes))
        print(len(T["lnZ"]), "of", len(sets), "modes", len(modes), flush=True)
    np.savez_compressed(lc.truth_path(), **{k: np.array(v) for k, v in T.items()})


def measure():
    worst, worst_q = 0.0, 0.0
    for name, (case, n, rows, gent, qent) in sorted(lc.golden_cases().items()):
        if n > 111:
            continue
        sp, mu, om = lc.inputs(case)
        r64 = lc.restate(case, mu, om, n, lc.SEED, list(rows), entries=None if gent is None else set(gent), qentries=set(qent))
        err = lc.errors(r64, lc.golden(name))
        lc.report(name, "restatement", err)
        worst = max([worst] + [v for k, v in err.items() if k != "quantiles"])
        worst_q = max(worst_q, err["quantiles"])
    print(f"MEASURED {worst:.2e}  Q_MEASURED {worst_q:.2e}")


if __name__ == "__main__":
    args = sys.argv[1:]
    if args == ["--truth"]:
        truth()
    elif args == ["--measure"]:
        measure()
    else:
        for nm in (args or sorted(lc.golden_cases()) + [lc.BIMODAL]):
            make(nm)
