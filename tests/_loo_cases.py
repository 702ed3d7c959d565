"""bb_ppc_loo (Pareto-smoothed importance-sampling leave-one-out scores of the observed log-frequency ratios,
barbay.jl_amd/csrc/bb_loo.h) restated in numpy from the formulas of include/barbay_hip.h, and the cases the emulation and GPU tests
share.  Rows, observed ratios and draws are `_score_cases`'s.

Expected values: tests/golden/loo_<case>_<set>_n<samples>.npz, a 50-digit mpmath evaluation of the same formulas on this
restatement's float64 (y, mu_j, sigma_j), written by tests/golden/make_loo_golden.py; mpmath is not needed to read them.

Parameter sets: "wide" is `_score_cases.params` (cells at 12 <= |z| <= 20, khat in the tens); "tight" is `params_tight` below, a
posterior-like set whose mutants' posterior sds ramp from a tenth of the predictive sd to about it, so that cells with
khat < 0.5, in 0.5 .. 0.7 and above 0.7 all occur, and one mutant whose noise scale is all but unknown (posterior sd 1 on the log
scale) and whose ratios lie 20 predictive sds off: its importance ratios span thousands of nats, c lies far beyond -690 and the
raw branch at M >= 5 is taken.  `check_bands` asserts all of that, and that no cell's c lies within 1 of -690.

Bound: the project's 1e-12, relative to max(|x|, 1), for every real output; the NaN / Inf pattern and n_scored exact.

Why the reference stays inside the bound: on synthetic Gaussian cells at n = 25 / 111 / 1000 (4096 on broader cells) the float64
restatement was within 1.6e-14 (elpd), 7.7e-15 (khat), 4.9e-14 (n_eff) of the 50-digit values, and moving every l_j by one ulp
moved the outputs by at most 1e-14.

Measured on the cases, the largest error over a set's goldens against the 50-digit values, float64 restatement / host emulation /
MI355X, in units of 1e-16 (each test prints its own line; `tools/ppc_loo_rate.py --errors` gathers them):

set, n                        elpd_loo                 p_loo                  khat                 n_eff                   lpd          row_elpd_loo              row_khat             row_n_eff
tight, 2             6.7/  13.7/  13.7    24.4/  24.4/  20.4     0.0/   0.0/   0.0     6.4/   8.2/   8.2     4.5/  11.1/   8.9     8.9/  34.4/  26.6     0.0/   0.0/   0.0     6.5/  12.0/  11.8
tight, 24            8.8/  15.3/  15.3    11.1/  17.4/  17.4     0.0/   0.0/   0.0    29.4/  41.4/  39.6     6.7/   8.3/   8.9    10.0/  17.8/  17.8     0.0/   0.0/   0.0    19.1/  46.7/  46.7
tight, 25            7.4/  22.5/  22.5    10.1/  21.9/  21.9   451.9/ 478.5/ 478.5    30.8/  21.1/  23.2     6.9/   7.8/   7.8     7.8/  27.5/  22.8   312.0/ 147.7/ 126.6    13.3/  19.8/  13.8
tight, 111          18.3/  24.1/  22.8    28.9/  30.7/  30.7   283.7/ 665.0/ 660.6    55.2/  91.3/  87.3    15.0/  16.0/  16.0    26.5/  24.4/  53.1   123.0/ 183.2/ 162.6    47.8/  58.0/  56.2
tight, 1000         70.5/  94.7/ 132.1    71.9/  95.8/ 131.7   138.5/ 171.2/ 176.9   201.8/ 388.3/ 376.6    12.8/  16.4/  16.4    81.5/ 106.0/ 110.5   115.5/ 160.0/ 160.0   171.4/ 266.4/ 236.8
tight, 1025         55.2/  36.3/  53.7    57.5/  39.4/  57.5    70.8/  52.0/  69.2    28.7/  80.8/  51.4     9.3/  11.1/  11.1    12.5/  13.9/  13.9    42.3/  63.3/  88.8     4.5/  10.2/  10.2
tight, 8192        104.1/ 179.4/ 193.0   107.6/ 186.9/ 201.0   126.5/ 172.6/ 184.3    76.8/ 160.8/ 177.8    22.3/  25.5/  25.5    15.3/   4.8/  16.7    15.5/  43.7/  43.1    56.5/  33.1/  10.2
wide, 2              4.2/  11.0/  11.0   222.6/ 501.8/ 643.9     0.0/   0.0/   0.0    70.5/ 178.4/ 201.9     5.8/   9.3/   8.3     8.6/  10.5/  10.5     0.0/   0.0/   0.0    56.2/ 273.8/ 273.8
wide, 24             7.6/   8.2/  11.5    40.5/  50.8/  65.2     0.0/   0.0/   0.0   172.6/ 553.0/ 473.9     6.4/   8.0/   8.0    10.0/   7.8/   9.8     0.0/   0.0/   0.0   133.7/ 120.5/ 374.1
wide, 25             8.3/   9.9/   9.9    48.2/  48.2/  41.6   498.5/1477.7/1477.7    85.0/ 108.7/ 146.0     7.3/   6.2/   8.9     8.3/   9.4/   9.4   273.5/ 663.9/ 663.9    50.7/  61.7/  48.8
wide, 111           17.3/  22.2/  22.2    27.0/  58.2/  43.1   283.7/ 665.0/ 660.6   241.3/ 390.4/ 361.8    13.7/  12.8/  12.8    20.0/  20.0/  23.9   439.6/ 224.3/ 233.1    68.8/  68.8/  68.8
wide, 1000          18.9/  23.7/  23.7    45.3/  72.8/  80.9   183.0/ 383.8/ 385.7   256.2/1011.8/1013.5    12.6/  13.9/  13.9    16.7/  22.2/  22.2   154.3/ 224.9/ 223.5   222.9/ 452.3/ 593.1
(the largest entry, 1477.7e-16, is 0.15 of the bound; khat at n = 25 and 111 is the conditioning of x*, see SEED25)
"""
import ctypes as C
import functools
import math
import os

import numpy as np

import _ppc_cases as pc
import _score_cases as sc
from conftest import make_engine
from barbay_jl_amd import _capi

GOLD = os.path.join(os.path.dirname(__file__), "golden")
CELLS = ("elpd_loo", "p_loo", "khat", "n_eff", "lpd")
ROWS = ("row_elpd_loo", "row_p_loo", "row_khat", "row_n_eff", "row_elpd_cells", "row_khat_max")
TOL = 1e-12
SEED = sc.SEED
NS = (2, 24, 25, 111, 1000)          # M = 0, 4 (the last unsmoothed size), 5 (the smallest fit), 22, 95
SETS = ("tight", "wide")
# name -> (case of _ppc_cases.CASES, parameter set, n_samples, rows with a golden or None for all)
BIG = {
    "fitness_tight_n1025": ("fitness", "tight", 1025, (0, 9, 12, 17, 33, 59)),     # one sample beyond the block
    "fitness_tight_n8192": ("fitness", "tight", 8192, (0, 9, 12, 17, 33, 59)),     # the cap: M = 272, a tail wider than four waves
}
RAW_M = 7                             # the tight set's mutant with the unknown noise scale
# n = 25 (M = 5) is the one size at which x* is x_1 = exp(rho_1) - exp(c), the gap between the tail's smallest draw and the
# largest draw outside it, and x* scales the whole theta grid: its relative rounding error, about ulp(l) / (rho_1 - c), goes
# straight into khat.  Among the 300-odd cells of a case some gap is always a thousand times smaller than the typical one, and
# there the float64 restatement itself is 1e-12 off the 50-digit value (measured: the worst cell of every case at every one of a
# hundred seeds moved by 9e-14 to 4e-12 when every l_j moved by one ulp; from n = 30 on, x* = x_2, the worst is 8e-14).  So the
# n = 25 goldens hold a handful of rows fixed beforehand (`rows25`) at the first seed >= SEED at which the restatement of those rows
# is within 5e-14 of the 50-digit values and moving every l_j by one ulp, up or down by a seeded coin (`sensitivity`), moves no
# output by more than 5e-14 (make_loo_golden.py --find-seeds; the generator asserts that these are the seeds it finds).
SEED25 = {("fitness", "tight"): 13, ("fitness", "wide"): 13, ("genotype_regrouped", "tight"): 11, ("genotype_regrouped", "wide"): 11,
          ("multienv", "tight"): 12, ("multienv", "wide"): 33, ("multienv_replicate", "tight"): 18, ("multienv_replicate", "wide"): 28,
          ("replicate_ragged", "tight"): 17, ("replicate_ragged", "wide"): 17}


def rows25(sp):
    """The rows of an n = 25 golden: neutrals, mutants early, RAW_M and late in the ramp, in the first and the last replicate."""
    nn, B, R = sp.n_neutral, sp.B, sp.n_rep
    return tuple(sorted({0, 3, nn + 3, nn + RAW_M, nn + 12, B - 1, (R - 1) * B + 1, (R - 1) * B + nn + 5, R * B - 1}))


def golden_cases():
    """name -> (case, parameter set, n_samples, rows or None for all or "rows25", seed)."""
    out = {f"{c}_{s}_n{n}": (c, s, n, "rows25" if n == 25 else None, SEED25[(c, s)] if n == 25 else SEED)
           for c in sorted(pc.CASES) for s in SETS for n in NS}
    out.update({k: v + (SEED,) for k, v in BIG.items()})
    return out


def case_of(name):
    """(spec, mu, omega, n_samples, rows, seed) of a golden."""
    case, pset, n, rows, seed = golden_cases()[name]
    sp, mu, om = inputs(case, pset)
    return sp, mu, om, n, (rows25(sp) if rows == "rows25" else rows), seed


def golden_path(name):
    return os.path.join(GOLD, f"loo_{name}.npz")


# ---- parameters ---------------------------------------------------------------------------------------------------------------
def params_tight(sp, seed=sc.PSEED):
    """(mu, omega): `_score_cases.params` without its pushed mutants' push (every mean explains the data), the posterior sd of a
    mutant's fitness latents ramping with the mutant's index from 0.03 to 0.45 (predictive sd 0.3), and mutant RAW_M with
    logsigma's posterior sd 1 and its fitness 20 predictive sds off."""
    mu, om = sc.params(sp, seed)
    mu, om = mu.copy(), om.copy()
    off = sp.offsets()
    nb, R = sp.n_bc, sp.n_rep
    Ek = sp.n_env if sp.kind in ("multienv", "multienv_replicate") else 1
    push = np.zeros(nb)
    push[3::7] = 11.5 * math.exp(-1.2) * np.where(np.arange(len(push[3::7])) % 2 == 0, 1.0, -1.0)
    ramp = 0.03 * (15.0 ** (np.arange(nb) / max(nb - 1, 1)))                     # 0.03 .. 0.45
    inv_softplus = lambda s: np.log(np.expm1(s))
    big = 20.0 * math.exp(-1.2)
    if sp.kind in ("fitness", "multienv"):                                       # flat index e + E m
        lo = off["s_bc"][0]
        mu[lo:lo + nb * Ek] -= np.repeat(push, Ek)
        om[lo:lo + nb * Ek] = inv_softplus(np.repeat(ramp, Ek))
        mu[lo + Ek * RAW_M:lo + Ek * (RAW_M + 1)] += big
        ls = off["logsigma_bc"][0]
        om[ls + Ek * RAW_M:ls + Ek * (RAW_M + 1)] = inv_softplus(1.0)
    else:
        logtau = -3.0
        lo = off["theta_tilde"][0]
        units = nb if sp.kind == "genotype" else Ek * nb * R
        reps = 1 if sp.kind == "genotype" else R
        pushed = push if sp.kind == "genotype" else np.tile(np.repeat(push, Ek), R)
        rampu = ramp if sp.kind == "genotype" else np.tile(np.repeat(ramp, Ek), R)
        mu[lo:lo + units] -= pushed / math.exp(logtau)
        om[lo:lo + units] = inv_softplus(rampu / math.exp(logtau))
        ls = off["logsigma_bc"][0]
        for r in range(reps):
            u0 = RAW_M if sp.kind == "genotype" else Ek * RAW_M + Ek * nb * r
            mu[lo + u0:lo + u0 + Ek] += big / math.exp(logtau)
            om[ls + u0:ls + u0 + Ek] = inv_softplus(1.0)
    return mu, om


@functools.lru_cache(maxsize=None)
def inputs(case, pset):
    """(spec, mu, omega) of a case and parameter set, computed once and read-only."""
    if pset == "wide":
        return sc.inputs(case)
    sp = pc.spec(case)
    mu, om = params_tight(sp)
    mu.setflags(write=False)
    om.setflags(write=False)
    return sp, mu, om


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def tail_len(n):
    c = 0
    while c * c < 9 * n:
        c += 1
    return min(n // 5, c)


def _lse(v):
    m = v.max()
    return m + math.log(np.exp(v - m).sum())


def psis(l):
    """PSIS(l) of the header in float64: (elpd_loo, p_loo, khat, n_eff, lpd) and c (NaN where M < 5)."""
    n = l.shape[0]
    with np.errstate(all="ignore"):
        lpd = _lse(l) - math.log(n)
        if not np.all(np.isfinite(l)):
            return (math.nan, math.nan, math.nan, math.nan, lpd), math.nan
        a = -l
        r = a - a.max()
        M = tail_len(n)
        lw = r.copy()
        khat, c = math.inf, math.nan
        if M >= 5:
            order = np.lexsort((np.arange(n), r))                      # (r_j, j) ascending
            tail = order[n - M:]
            c = float(r[order[n - M - 1]])
            if c >= -690.0:
                x = np.exp(r[tail]) - math.exp(c)
                xstar = x[(M + 2) // 4 - 1]
                if xstar > 0.0:
                    m = 30 + math.isqrt(M)
                    i = np.arange(1, m + 1)
                    th = 1.0 / x[M - 1] + (1.0 - np.sqrt(m / (i - 0.5))) / (3.0 * xstar)
                    kap = np.array([np.log1p(-t * x).sum() / M for t in th])
                    L = M * ((np.log(-th / kap) - kap) - 1.0)
                    w = np.array([1.0 / np.exp(L - Li).sum() for Li in L])
                    thh = (th * w).sum()
                    kraw = np.log1p(-thh * x).sum() / M
                    sig = -kraw / thh
                    khat = (M * kraw + 5.0) / (M + 10.0)
                    p = (np.arange(1, M + 1) - 0.5) / M
                    v = np.log(sig * np.expm1(-khat * np.log1p(-p)) / khat + math.exp(c))
                    lw[tail] = np.where(v > 0.0, 0.0, v)
        ls = _lse(lw)
        elpd = _lse(lw + l) - ls
        neff = 1.0 / (np.exp(lw - ls) ** 2).sum()
    return (float(elpd), float(lpd - elpd), float(khat), float(neff), float(lpd)), c


def logdens(y, mu, sd):
    z = (y - mu) / sd
    return -0.5 * z * z - np.log(sd) - 0.5 * math.log(2.0 * math.pi)


def cell_f64(y, mu, sd):
    """The log densities of a cell from its float64 inputs (what `row` sums) and PSIS of them."""
    l = logdens(y, mu, sd)
    return l, psis(l)


def row_f64(ls):
    acc = ls[0].copy()
    for l in ls[1:]:
        acc = acc + l
    return psis(acc)


def restate(sp, mu, omega, n_samples, seed, rows=None, cell=cell_f64, row=row_f64, want_c=False):
    """bb_ppc_loo at the parameters (mu, omega), caller order, for `rows` (all): a dict as Engine.ppc_loo returns, the rows' entries
    only.  `cell`, `row`: the evaluation of a cell and of a row from its cells' log densities (the golden generator passes its
    50-digit ones); want_c: also 'c' per cell and 'row_c' per row."""
    D = sc.Draws(seed, mu, pc.softplus(omega), n_samples)
    y = sc.observed(sp)
    n_rows, n_steps = y.shape
    rows = np.arange(n_rows) if rows is None else np.asarray(rows)
    out = {k: np.full((len(rows), n_steps), np.nan) for k in CELLS}
    out.update({k: np.full(len(rows), np.nan) for k in ROWS})
    out["n_scored"] = np.zeros(len(rows), dtype=np.int32)
    if want_c:
        out["c"] = np.full((len(rows), n_steps), np.nan)
        out["row_c"] = np.full(len(rows), np.nan)
    for x, rw in enumerate(rows):
        r = int(rw) // sp.B
        ls, acc, kmax = [], 0.0, -math.inf
        for t in range(sp.n_time[r] - 1):
            if np.isnan(y[rw, t]):
                continue
            mj, sj = sc.cell_inputs(sp, D, rw, t)
            l, (vals, c) = cell(float(y[rw, t]), mj, sj)
            ls.append(l)
            for k, v in zip(CELLS, vals):
                out[k][x, t] = float(v)
            acc = acc + vals[0]
            kmax = vals[2] if (vals[2] > kmax or vals[2] != vals[2]) else kmax
            out["n_scored"][x] += 1
            if want_c:
                out["c"][x, t] = c
        if ls:
            vals, c = row(ls)
            for k, v in zip(ROWS[:4], vals[:4]):
                out[k][x] = float(v)
            out["row_elpd_cells"][x], out["row_khat_max"][x] = float(acc), float(kmax)
            if want_c:
                out["row_c"][x] = c
    return out


def sensitivity(sp, mu, om, n, seed, rows):
    """The largest relative move of an output of the restatement when every l_j moves by one ulp, up or down by a seeded coin."""
    g = np.random.default_rng(0)

    def moved(y, m, s):
        l = logdens(y, m, s)
        l = np.where(g.random(l.shape) < 0.5, np.nextafter(l, np.inf), np.nextafter(l, -np.inf))
        return l, psis(l)

    a, b = restate(sp, mu, om, n, seed, rows=rows), restate(sp, mu, om, n, seed, rows=rows, cell=moved)
    worst = 0.0
    for k in CELLS + ROWS:
        ok = np.isfinite(a[k]) & np.isfinite(b[k])
        if ok.any():
            worst = max(worst, float((np.abs(a[k][ok] - b[k][ok]) / np.maximum(np.abs(a[k][ok]), 1.0)).max()))
    return worst


@functools.lru_cache(maxsize=None)
def golden(name):
    with np.load(golden_path(name)) as f:
        g = {k: f[k] for k in f.files}
    for v in g.values():
        v.setflags(write=False)
    return g


# ---- comparison -----------------------------------------------------------------------------------------------------------------
def errors(got, ref):
    """Largest error per output relative to max(|x|, 1); the NaN / Inf pattern and n_scored must be equal."""
    err = {}
    for k in CELLS + ROWS:
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        assert a.shape == b.shape, (k, a.shape, b.shape)
        assert np.array_equal(np.isnan(a), np.isnan(b)), k
        assert np.array_equal(np.isinf(a), np.isinf(b)) and np.array_equal(a[np.isinf(a)], b[np.isinf(b)]), k
        ok = np.isfinite(b)
        if not ok.any():
            err[k] = 0.0
            continue
        err[k] = float(np.max(np.abs(a[ok] - b[ok]) / np.maximum(np.abs(b[ok]), 1.0)))
    assert np.array_equal(got["n_scored"], ref["n_scored"])
    return err


def take(res, rows):
    return res if rows is None else {k: v[list(rows)] for k, v in res.items()}


def report(name, label, err):
    print(f"loo case {name:36s} {label:12s} " + " ".join(f"{k} {err[k] / 1e-16:7.1f}" for k in CELLS + ROWS) + "  (1e-16)")


def same_bytes(a, b):
    return sc.same_bytes(a, b)


def check_golden(lib, name, label):
    """Every output of a call against the golden (and the float64 restatement against it, for the record)."""
    sp, mu, om, n, rows, seed = case_of(name)
    ref = golden(name)
    r64 = restate(sp, mu, om, n, seed, rows=rows)
    e0 = errors(r64, ref)
    report(name, "restatement", e0)
    with pc._handle(lib, sp, mu, om) as e:
        assert e.loo_shape() == e.score_shape() == (sp.n_rep * sp.B, max(sp.n_time) - 1)
        got = e.ppc_loo(n_samples=n, seed=seed)
    y = sc.observed(sp)
    assert np.array_equal(np.isnan(got["lpd"]), np.isnan(y))
    err = errors(take(got, rows), ref)
    report(name, label, err)
    for k in CELLS + ROWS:
        assert e0[k] <= 1e-13, ("restatement", name, k, e0[k])
        assert err[k] <= TOL, (label, name, k, err[k])
    if tail_len(n) < 5:
        assert np.all(np.isinf(got["khat"][~np.isnan(y)])) and np.all(got["khat"][~np.isnan(y)] > 0)
    return got


def check_bands(n=1000):
    """The tight set over the model kinds puts cells in each band of khat, none with c within 1 of -690 and some beyond it (CPU,
    the restatement)."""
    lo = mid = hi = raw = 0
    for case in sorted(pc.CASES):
        sp, mu, om = inputs(case, "tight")
        r = restate(sp, mu, om, n, SEED, want_c=True)
        k = np.concatenate([r["khat"][~np.isnan(r["khat"])], r["row_khat"][~np.isnan(r["row_khat"])]])
        c = np.concatenate([r["c"][~np.isnan(r["c"])], r["row_c"][~np.isnan(r["row_c"])]])
        assert not np.any(np.abs(c + 690.0) <= 1.0), c[np.abs(c + 690.0) <= 1.0]
        lo += np.count_nonzero(k < 0.5)
        mid += np.count_nonzero((k >= 0.5) & (k <= 0.7))
        hi += np.count_nonzero((k > 0.7) & np.isfinite(k))
        raw += np.count_nonzero(c < -690.0)
        assert np.array_equal(np.isinf(k), c < -690.0)
    assert lo >= 4 and mid >= 4 and hi >= 4 and raw >= 1, (lo, mid, hi, raw)
    return lo, mid, hi, raw


def check_shared_bytes(lib, case="replicate_ragged", ns=(2, 25, 111, 1000, 1025)):
    """lpd is bb_ppc_score's lpd, byte for byte, at equal seed and n; n_scored too."""
    for pset in SETS:
        sp, mu, om = inputs(case, pset)
        with pc._handle(lib, sp, mu, om) as e:
            for n in ns:
                a, b = e.ppc_loo(n_samples=n, seed=SEED), e.ppc_score(n_samples=n, seed=SEED)
                assert a["lpd"].tobytes() == b["lpd"].tobytes(), (pset, n)
                assert np.array_equal(a["n_scored"], b["n_scored"])


def check_unsmoothed(lib, case="multienv", ns=(2, 5, 24)):
    """n < 25: elpd_loo = -(LSE(-l) - ln n) of the restatement's l, khat = +Inf."""
    sp, mu, om = inputs(case, "tight")
    y = sc.observed(sp)
    for n in ns:
        D = sc.Draws(SEED, mu, pc.softplus(om), n)
        with pc._handle(lib, sp, mu, om) as e:
            got = e.ppc_loo(n_samples=n, seed=SEED)
        worst = 0.0
        for row in range(y.shape[0]):
            for t in range(sp.n_time[row // sp.B] - 1):
                if np.isnan(y[row, t]):
                    continue
                l = logdens(float(y[row, t]), *sc.cell_inputs(sp, D, row, t))
                want = -(_lse(-l) - math.log(n))
                worst = max(worst, abs(got["elpd_loo"][row, t] - want) / max(abs(want), 1.0))
                assert got["khat"][row, t] == math.inf
        print("unsmoothed n", n, "worst", worst)
        assert worst <= TOL
        assert np.all(np.isinf(got["row_khat"][got["n_scored"] > 0]))


def check_zero_counts(lib, case="replicate_ragged", n=111):
    """Zero counts are unscored, as `_score_cases.check_zero_counts`; a row with no scored cell has NaN row outputs and n_scored = 0;
    a row with one scored cell has row-level outputs byte-identical to that cell's."""
    sp, mu, om = inputs(case, "tight")
    nn = sp.n_neutral
    T0 = sp.n_time[0]
    edits = [(0, 0, 2), (0, 2, nn + 5), (1, sp.n_time[1] - 1, nn + 1), (2, 1, 0)]
    edits += [(0, t, nn + 9) for t in range(1, T0, 2)]                       # every step of this row touches a zero: no scored cell
    edits += [(0, t, nn + 11) for t in range(2, T0)]                         # only step 0 of this row stays
    sp2 = sc.zeroed(sp, edits)
    y2 = sc.observed(sp2)
    with pc._handle(lib, sp2, mu, om) as e:
        got = e.ppc_loo(n_samples=n, seed=SEED)
    for k in CELLS:
        assert np.array_equal(np.isnan(got[k]), np.isnan(y2)), k
    assert np.array_equal(got["n_scored"], (~np.isnan(y2)).sum(axis=1))
    none, one = nn + 9, nn + 11
    assert got["n_scored"][none] == 0 and got["n_scored"][one] == 1
    for k in ROWS:
        assert np.isnan(got[k][none]), k
    for rk, ck in (("row_elpd_loo", "elpd_loo"), ("row_p_loo", "p_loo"), ("row_khat", "khat"), ("row_n_eff", "n_eff"),
                   ("row_elpd_cells", "elpd_loo"), ("row_khat_max", "khat")):
        assert got[rk][one].tobytes() == got[ck][one, 0].tobytes(), rk
    ref = restate(sp2, mu, om, n, SEED)
    err = errors(got, ref)
    report(case + "_zeroed", "vs restated", err)
    for k in CELLS + ROWS:                   # (no golden here: the float64 restatement, itself within 1e-13 of the 50-digit values)
        assert err[k] <= TOL, (k, err[k])
    for row in range(got["lpd"].shape[0]):   # row_elpd_cells: the scored cells in step order
        if got["n_scored"][row]:
            s = 0.0
            for v in got["elpd_loo"][row][~np.isnan(y2[row])]:
                s += v
            assert s == got["row_elpd_cells"][row]


def check_nan_parameter(lib, case="fitness", n=111):
    """One mutant's s_bc mean NaN: its rows are NaN in every real output, every other row keeps its bytes."""
    sp, mu, om = inputs(case, "tight")
    m = 11
    mu2 = mu.copy()
    mu2[sp.offsets()["s_bc"][0] + m] = np.nan
    with pc._handle(lib, sp, mu, om) as e:
        base = e.ppc_loo(n_samples=n, seed=SEED)
    with pc._handle(lib, sp, mu2, om) as e:
        got = e.ppc_loo(n_samples=n, seed=SEED)
        lpd = e.ppc_score(n_samples=n, seed=SEED)["lpd"]
    rows = np.array([r * sp.B + sp.n_neutral + m for r in range(sp.n_rep)])
    rest = np.setdiff1d(np.arange(base["lpd"].shape[0]), rows)
    assert same_bytes({k: v[rest] for k, v in got.items()}, {k: v[rest] for k, v in base.items()})
    scored = ~np.isnan(base["lpd"][rows])
    assert scored.any()
    for k in CELLS:
        assert np.all(np.isnan(got[k][rows][scored])), k
    for k in ROWS:
        assert np.all(np.isnan(got[k][rows])), k
    assert np.array_equal(got["n_scored"], base["n_scored"])
    assert got["lpd"].tobytes() == lpd.tobytes()


def raw_loo(engine, n_samples, seed=SEED, null=(), want=CELLS + ROWS + ("n_scored",)):
    """bb_ppc_loo through ctypes with only the outputs in `want` non-NULL; `null` names arguments passed as NULL (h, o, out)."""
    n_rows, n_steps = engine.loo_shape()
    o = _capi.bb_loo_opts()
    o.n_samples, o.seed = n_samples, seed
    res, out = {}, _capi.bb_loo_out()
    for k in want:
        if k == "n_scored":
            res[k] = np.full(n_rows, -7, dtype=np.int32)
            out.n_scored = res[k].ctypes.data_as(C.POINTER(C.c_int32))
        else:
            res[k] = np.full((n_rows, n_steps) if k in CELLS else n_rows, -7.0)
            setattr(out, k, _capi._ptr(res[k]))
    rc = engine._lib.bb_ppc_loo(None if "h" in null else engine._h, None if "o" in null else C.byref(o),
                                None if "out" in null else C.byref(out))
    return rc, res


def check_errors(lib):
    """Every error code; n = 8193 refused, 8192 taken; every output pointer may be NULL."""
    sp, mu, om = inputs("fitness", "tight")
    with pc._handle(lib, sp, mu, om) as e:
        for null in ("h", "o", "out"):
            assert raw_loo(e, 10, null=(null,))[0] == -1, null
        assert e._lib.bb_loo_shape(None, None, None) == -1
        for n in (0, 1, 8193, 16384, -3):
            assert raw_loo(e, n)[0] == _capi.BB_ERR_UNSUPPORTED, n
        assert raw_loo(e, 64, want=())[0] == 0                             # an all-NULL out
        full = e.ppc_loo(n_samples=64, seed=SEED)
        assert same_bytes(raw_loo(e, 64)[1], full)
        for k in CELLS + ROWS + ("n_scored",):                             # every output NULL except one
            rc, one = raw_loo(e, 64, want=(k,))
            assert rc == 0 and same_bytes(one, {k: full[k]}), k
        try:
            e.ppc_loo(n_samples=8193)
        except _capi.BarBayHipError as ex:
            assert "error -4" in str(ex)
        else:
            raise AssertionError("no error")


def check_buffer_reuse(lib):
    """The call interleaved with other post-fit calls at changing sizes on one handle: every result is byte for byte what a fresh
    handle gives."""
    sp, mu, om = inputs("fitness", "tight")
    qs = (0.95, 0.675, 0.05)
    calls = [lambda e: e.ppc_loo(n_samples=111, seed=SEED),
             lambda e: e.ppc_bands(qs, n_samples=111, n_ppc=7, seed=SEED),
             lambda e: e.ppc_loo(n_samples=1000, seed=SEED),
             lambda e: e.ppc_score(n_samples=2049, seed=SEED),
             lambda e: e.ppc_loo(n_samples=2, seed=SEED),
             lambda e: e.ppc_loo(n_samples=1025, seed=SEED),
             lambda e: e.ppc_loo(n_samples=111, seed=SEED)]
    with pc._handle(lib, sp, mu, om) as e:
        got = [pc._bits(f(e)) for f in calls]
    for i, f in enumerate(calls):
        with pc._handle(lib, sp, mu, om) as e:
            assert got[i] == pc._bits(f(e)), i
    assert got[0] == got[6]


def check_group_handle(lib, case):
    """A device_ids = [0, 0] group handle against a single-device handle."""
    sp, mu, om = inputs(case, "tight")
    with pc._handle(lib, sp, mu, om, device_ids=[0, 0]) as e:
        a = e.ppc_loo(n_samples=111, seed=SEED)
    with pc._handle(lib, sp, mu, om) as e:
        b = e.ppc_loo(n_samples=111, seed=SEED)
    assert same_bytes(a, b)


def check_handle_untouched(lib):
    """run(5) after a call leaves the parameters bit-equal to run(5) on a fresh handle."""
    sp = pc.spec("fitness")
    with make_engine(sp, lib, seed=5) as a, make_engine(sp, lib, seed=5) as b:
        b.ppc_loo(n_samples=111, seed=SEED)
        for x, y in zip(a.get_params(), b.get_params()):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
        a.run(5)
        b.ppc_loo(n_samples=64, seed=1)
        b.run(5)
        for x, y in zip(a.get_params(), b.get_params()):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64))


def check_repeatable(lib, modes=(None,)):
    """Independent of the launch mode and repeatable, bit for bit (the tail list's order on the device is not fixed; the results are)."""
    import barbay_jl_amd as bb
    sp, mu, om = inputs("replicate_ragged", "tight")
    out = []
    for mode in modes:
        kw = {} if mode is None else {"launch_mode": mode}
        with bb.Engine(sp.kind, sp.counts, sp.n_neutral, sp.n_bc, seed=4, _lib=lib, **kw) as e:
            e.set_params(mu, om)
            out.append(e.ppc_loo(n_samples=500, seed=2))
            out.append(e.ppc_loo(n_samples=500, seed=2))
    assert all(same_bytes(out[0], o) for o in out[1:])


# ---- the closed form ------------------------------------------------------------------------------------------------------------
def check_closed_form(lib, n=8192, n_big=400_000):
    """A mutant cell whose sigma and sbar are all but fixed (posterior sd 1e-9) and whose s has posterior sd tau with
    tau^2 / sigma^2 = 0.1: with q(s) = N(m, tau) read as the posterior given y, the leave-one-out posterior is
    N(mu_loo, tau_loo), 1 / tau_loo^2 = 1 / tau^2 - 1 / sigma^2, mu_loo = tau_loo^2 (m / tau^2 - y' / sigma^2) (y' = y + sbar, the
    observation of s), and the exact leave-one-out predictive of y' is N(mu_loo, sigma^2 + tau_loo^2).  The device's elpd_loo at
    n = 8192 lies within 6 Monte-Carlo standard errors of its log density, the standard error from the importance weights of an
    independent numpy sample of 400 000 draws (delta method on the self-normalised estimate), scaled to n."""
    sp, mu, om = inputs("fitness", "tight")
    off = sp.offsets()
    mu, om = mu.copy(), om.copy()
    m_, t = 22, 2
    row = sp.n_neutral + m_
    inv_softplus = lambda s: math.log(math.expm1(s)) if s > 1e-6 else math.log(s)
    sigma = math.exp(mu[off["logsigma_bc"][0] + m_])
    tau = sigma * math.sqrt(0.1)
    om[off["logsigma_bc"][0] + m_] = inv_softplus(1e-9)
    om[off["s_pop"][0] + t] = inv_softplus(1e-9)
    om[off["s_bc"][0] + m_] = inv_softplus(tau)
    with pc._handle(lib, sp, mu, om) as e:
        mean, sd = e.posterior()
        got = e.ppc_loo(n_samples=n, seed=17)
        y = e.ppc_score(n_samples=2, seed=17)["observed"][row, t]
    tau = sd[off["s_bc"][0] + m_]
    sigma = math.exp(mean[off["logsigma_bc"][0] + m_])
    m0 = mean[off["s_bc"][0] + m_]
    yp = y + mean[off["s_pop"][0] + t]
    tl2 = 1.0 / (1.0 / tau ** 2 - 1.0 / sigma ** 2)
    ml = tl2 * (m0 / tau ** 2 - yp / sigma ** 2)
    v = sigma ** 2 + tl2
    exact = -0.5 * (yp - ml) ** 2 / v - 0.5 * math.log(2.0 * math.pi * v)
    g = np.random.default_rng(0)
    s = g.normal(m0, tau, n_big)
    l = logdens(yp, s, sigma)
    w = np.exp(-(l - l.min()))
    w /= w.sum()
    # elpd = -log sum_j w_j' with w' the normalised 1 / p: the variance of the ratio estimator of E[1/p] / 1, per draw
    ip = np.exp(-l)
    rel_var = ip.var() / ip.mean() ** 2
    se = math.sqrt(rel_var / n + rel_var / n_big)
    big = -math.log(ip.mean())
    print("closed form", exact, "device", got["elpd_loo"][row, t], "numpy", big, "se", se, "khat", got["khat"][row, t])
    assert abs(big - exact) < 6 * math.sqrt(rel_var / n_big)
    assert abs(got["elpd_loo"][row, t] - exact) < 6 * se
