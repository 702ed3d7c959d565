"""bb_ppc_score (predictive log score and PIT of the observed log-frequency ratios, barbay.jl_amd/csrc/bb_score.h) restated in
numpy from the formulas of include/barbay_hip.h, and the cases the emulation and GPU tests share.  The keying is the header's:
parameter draw j of the caller's latent i is pairs(seed, i, j >> 1, 0xFFFFFFE0), an even index taking the cosine branch -- the
draw of bb_ppc_bands (`_ppc_cases.restate`).

Expected values: tests/golden/score_<case>_n<samples>.npz, a 50-digit mpmath evaluation of the same formulas on this restatement's
float64 (y, mu_j, sigma_j), written by tests/golden/make_score_golden.py; mpmath is not needed to read them.  Bound: 1e-12, the
figure of `_ppc_cases.assert_bands_close`; for observed, pred_mean, pred_sd, lpd, p_waic and the row sums relative to
max(|x|, 1), for pit and pit_upper relative to the value itself (that binds the tails: the parameters of `params` put cells at
12 <= |z| <= 20, where a tail is 1e-33 .. 1e-89, and none beyond); n_scored and the NaN pattern exact.

Why the reference stays inside the bound: for n <= 1000 and |z| up to about 15 the float64 restatement is within 4.3e-14 (pit)
and 2.7e-15 (lpd) of the 50-digit values, and moving every input by one ulp shifts a pit by at most 8.6e-14 (|z|^2 ulp through
erfc's argument; at |z| = 20 and n = 2 the table below has 6.7e-14); the library's (mu_j, sigma_j)
differ from the restatement's by the few ulp between its exp / log / Box-Muller and numpy's.  The observed ratio is formed with
libm's log on both sides (math.log here), so it is the same double.

Measured, largest error over a case's cells against the golden, float64 restatement / host emulation / MI355X, in units of 1e-16
(relative as above; each test prints its own line):

case                               pred_mean           pred_sd               lpd            p_waic               pit         pit_upper           row_lpd        row_p_waic
fitness_n1000                1.5/  5.2/  5.2   0.6/  1.1/  1.1  11.7/ 11.7/ 11.7  16.9/ 19.9/ 16.6 161.0/109.0/109.0 137.5/ 66.3/ 66.3  29.4/ 29.4/ 29.4  11.1/ 11.1/  9.3
fitness_n111                 2.6/  6.8/  6.8   0.6/  1.1/  1.1  12.6/ 12.3/ 11.6  25.8/ 22.4/ 19.0 238.2/163.1/163.1 103.8/140.2/138.9  27.8/ 28.7/ 28.7  16.1/ 14.1/ 12.1
fitness_n16384               1.4/  2.7/  2.7   0.6/  0.6/  0.6  21.1/ 14.3/ 14.3   2.2/  4.2/  3.7 124.9/111.9/111.9   4.1/  3.4/  3.5  36.6/ 21.1/ 21.1   0.0/  2.1/  0.1
fitness_n2                   0.0/  1.1/  1.1   0.6/  1.1/  1.1   4.4/  6.4/  5.7 166.0/166.0/269.8 276.8/290.9/290.9 249.8/175.7/173.9   8.9/  4.5/  4.5  55.2/ 63.7/157.7
fitness_n2049                1.5/  3.9/  3.9   0.6/  1.1/  1.1  12.8/ 15.5/ 15.5  18.2/ 24.8/ 19.8 148.3/164.7/167.7  94.9/ 68.9/ 68.9  31.1/ 33.3/ 33.3  10.9/ 14.5/ 12.7
genotype_regrouped_n1000     2.5/  5.6/  5.6   0.6/  1.1/  1.1  11.7/ 12.2/ 12.2  14.0/ 18.2/ 16.0 143.4/184.9/397.6 169.6/126.9/142.6  32.2/ 31.6/ 22.8  10.0/ 12.9/ 12.9
genotype_regrouped_n111      4.0/  6.2/  4.9   0.6/  1.1/  1.1  12.5/ 12.2/ 12.2  12.7/ 20.7/ 27.4 180.5/200.8/213.1 200.7/198.5/257.1  26.6/ 27.8/ 27.8   9.0/ 13.5/ 17.9
genotype_regrouped_n2        0.0/  1.5/  3.0   0.6/  2.2/  2.2   3.4/  9.3/  8.3 234.2/234.2/545.5 225.6/218.5/216.7 317.5/371.2/457.6   8.9/  7.8/  7.8  63.3/ 63.3/195.7
multienv_n1000               2.2/  6.6/  6.6   0.6/  1.1/  1.1  11.7/ 11.7/ 11.7  13.5/ 15.0/ 16.4 220.1/184.3/184.3 128.8/150.2/150.2  31.1/ 23.3/ 23.3   8.4/  7.0/  7.0
multienv_n111                3.0/  4.3/  4.3   0.6/  1.1/  1.1  11.5/ 12.8/ 12.8  15.5/ 19.0/ 16.3 149.3/176.0/176.0 215.4/107.8/108.5  32.2/ 26.4/ 34.5  12.5/  7.8/  6.3
multienv_n2                  0.0/  2.6/  2.6   0.6/  1.7/  1.7   5.8/  6.8/  6.8 256.5/722.4/738.3 368.6/359.6/359.6 211.8/257.5/259.2   8.9/  7.8/  8.9  25.2/ 43.4/ 36.9
multienv_replicate_n1000     2.2/  5.3/  5.3   0.6/  1.1/  1.1  12.6/ 13.9/ 13.9  13.1/ 13.5/ 16.2 378.7/334.2/312.6 120.0/119.6/118.1  36.1/ 24.0/ 25.5   7.6/  8.9/ 10.1
multienv_replicate_n111      3.5/  5.6/  5.8   0.6/  1.1/  1.1  13.7/ 11.7/ 11.7  14.8/ 20.2/ 20.2 211.1/471.0/474.5 163.2/261.1/261.1  32.8/ 24.4/ 19.5   8.6/ 14.9/ 16.4
multienv_replicate_n2        0.0/  2.8/  4.1   0.6/  2.8/  3.3   4.1/  5.8/  6.6 175.4/438.5/736.2 479.3/620.1/622.3 265.9/294.6/294.6   8.0/  7.8/  5.6  39.8/197.2/237.7
replicate_ragged_n1000       2.1/  6.4/  6.4   0.6/  1.1/  1.1  12.2/ 11.9/ 11.9  10.9/ 13.3/ 14.0 305.7/233.3/235.5 339.0/285.2/285.2  33.9/ 28.4/ 28.4   8.6/ 10.7/ 12.8
replicate_ragged_n111        5.7/  6.0/  6.0   1.1/  1.1/  1.1  13.5/ 12.6/ 12.6  15.9/ 22.1/ 28.2 237.3/339.5/337.0 311.8/272.3/642.9  34.4/ 24.2/ 24.2   9.0/ 18.0/ 27.0
replicate_ragged_n2          0.0/  2.7/  3.2   0.6/  1.7/  1.7   4.4/  6.7/  6.7 203.7/858.0/703.7 667.8/440.3/442.3 411.3/477.9/477.9   8.9/  7.8/  7.8  77.6/332.5/281.4
(the largest entry, 858.0e-16, is 0.086 of the bound)
(p_waic at n = 2 is the square of one difference l_0 - l_1 of two log densities near -150: their few-ulp errors, not the sum, set it)
"""
import ctypes as C
import functools
import math
import os

import numpy as np

import _ppc_cases as pc
from conftest import make_engine
from barbay_jl_amd import _capi
from oracle import rng
from oracle.spec import ModelSpec

GOLD = os.path.join(os.path.dirname(__file__), "golden")
CELLS = ("observed", "pred_mean", "pred_sd", "lpd", "p_waic", "pit", "pit_upper")
ROWS = ("row_lpd", "row_p_waic")
SELF_RELATIVE = ("pit", "pit_upper")
TOL = 1e-12
SEED = 11
PSEED = 5
NS = (2, 111, 1000)
# name -> (case of _ppc_cases.CASES, n_samples, rows with a golden or None for all)
BIG = {
    "fitness_n2049": ("fitness", 2049, None),          # more samples than the block has threads, no multiple of 64
    "fitness_n16384": ("fitness", 16384, (0, 9, 13, 27, 59)),     # the largest call: two neutrals, the first / a middle / the last mutant
}
Z_LO, Z_HI = 12.0, 20.0


def golden_cases():
    """name -> (case, n_samples, rows) of every golden file."""
    out = {f"{c}_n{n}": (c, n, None) for c in sorted(pc.CASES) for n in NS}
    out.update(BIG)
    return out


def golden_path(name):
    return os.path.join(GOLD, f"score_{name}.npz")


# ---- parameters ---------------------------------------------------------------------------------------------------------------
def observed(sp):
    """y[n_rows, n_steps] (row = r B + b), NaN where a count is 0 or the replicate has no such step; libm's log, as the library."""
    B, n_steps = sp.B, max(sp.n_time) - 1
    y = np.full((sp.n_rep * B, n_steps), np.nan)
    for r, cnt in enumerate(sp.counts):
        n = [float(v) for v in cnt.sum(axis=1)]
        for b in range(B):
            for t in range(sp.n_time[r] - 1):
                c0, c1 = int(cnt[t, b]), int(cnt[t + 1, b])
                if c0 and c1:
                    y[r * B + b, t] = math.log(float(c1) / n[t + 1]) - math.log(float(c0) / n[t])
    return y


def _env(sp, r, t):
    if sp.kind == "multienv":
        return int(sp.env_idx[t + 1])
    if sp.kind == "multienv_replicate":
        return int(sp.env_idx[r][t + 1])
    return 0


def params(sp, seed=PSEED):
    """(mu, omega) of a seeded generator: a posterior that roughly explains the data with a predictive sd near exp(-1.2) = 0.3 --
    s_pop = -(the neutrals' mean ratio), a mutant's fitness = its mean of y + s_pop, logsigma ~ N(-1.2, 0.1), posterior sd
    softplus(N(-3.5, 0.2)) = 0.03 -- and every seventh mutant pushed 11.5 predictive sds off, alternately up and down: the
    cells at 12 <= |z| <= 20 (`check_z_range`)."""
    g = np.random.default_rng(seed)
    off = sp.offsets()
    nn, nb, E, R = sp.n_neutral, sp.n_bc, sp.n_env, sp.n_rep
    Ek = E if sp.kind in ("multienv", "multienv_replicate") else 1
    y = observed(sp)
    mu = g.normal(0.0, 1.0, sp.D)
    om = g.normal(-3.5, 0.2, sp.D)
    spop, m_unit = [], np.zeros((R, nb, Ek))
    for r in range(R):
        T1 = sp.n_time[r] - 1
        yr = y[r * sp.B:(r + 1) * sp.B, :T1]
        st = -np.nanmean(yr[:nn], axis=0)
        spop.append(st)
        for e in range(Ek):
            ts = [t for t in range(T1) if _env(sp, r, t) == e]
            with np.errstate(all="ignore"):
                v = np.nanmean(yr[nn:, ts] + st[ts], axis=1) if ts else np.zeros(nb)
            m_unit[r, :, e] = np.where(np.isfinite(v), v, 0.0)
    mu[slice(*off["s_pop"])] = np.concatenate(spop) + g.normal(0.0, 0.02, sum(len(s) for s in spop))
    mu[slice(*off["logsigma_pop"])] = g.normal(-1.2, 0.1, off["logsigma_pop"][1] - off["logsigma_pop"][0])
    mu[slice(*off["logsigma_bc"])] = g.normal(-1.2, 0.1, off["logsigma_bc"][1] - off["logsigma_bc"][0])
    push = np.zeros(nb)
    push[3::7] = 11.5 * math.exp(-1.2) * np.where(np.arange(len(push[3::7])) % 2 == 0, 1.0, -1.0)
    if sp.kind in ("fitness", "multienv"):                                     # flat index e + E m
        mu[slice(*off["s_bc"])] = (m_unit[0] + push[:, None]).reshape(-1) + g.normal(0.0, 0.05, nb * Ek)
    else:
        logtau = -3.0
        if sp.kind == "genotype":
            gi = np.asarray(sp.geno_idx)
            m = m_unit[0, :, 0]
            theta = np.array([m[gi == k].mean() for k in range(sp.n_geno)])
            units, shared, pushed = m, theta[gi], push
        else:                                                                  # theta[e + E m]; units e + E m + E nb r
            theta = m_unit.mean(axis=0).reshape(-1)
            units, shared, pushed = m_unit.reshape(-1), np.tile(theta, R), np.tile(np.repeat(push, Ek), R)
        mu[slice(*off["theta"])] = theta
        mu[slice(*off["logtau"])] = logtau + g.normal(0.0, 0.05, units.shape[0])
        mu[slice(*off["theta_tilde"])] = (units - shared + pushed) / math.exp(logtau) + g.normal(0.0, 1.0, units.shape[0])
    return mu, om


# ---- the restatement ----------------------------------------------------------------------------------------------------------
class Draws:
    """Parameter draws j < n of the caller's latents at the posterior (mean, sigma), each latent drawn once."""

    def __init__(self, seed, mean, sigma, n):
        self.seed, self.mean, self.sigma = seed, mean, sigma
        self.j = np.arange(n, dtype=np.uint64)
        self.cache = {}

    def __call__(self, i):
        i = int(i)
        if i not in self.cache:
            a, b = rng.pairs(self.seed, np.full(self.j.shape, i, dtype=np.uint64), self.j >> np.uint64(1), pc.STREAM_PARAM)
            self.cache[i] = self.mean[i] + self.sigma[i] * np.where(self.j & np.uint64(1), b, a)
        return self.cache[i]


def cell_inputs(sp, D, row, t):
    """(mu_j, sigma_j) of cell (row, t), t < T_r - 1."""
    off = sp.offsets()
    B, nb, nn, E = sp.B, sp.n_bc, sp.n_neutral, sp.n_env
    r, b = divmod(int(row), B)
    g = sum(T - 1 for T in sp.n_time[:r]) + t
    sbar = D(off["s_pop"][0] + g)
    if b < nn:
        return -sbar, np.exp(D(off["logsigma_pop"][0] + g))
    m = b - nn
    Ek = E if sp.kind in ("multienv", "multienv_replicate") else 1
    e = _env(sp, r, t)
    if sp.kind in ("fitness", "multienv"):
        s, ls = D(off["s_bc"][0] + e + Ek * m), D(off["logsigma_bc"][0] + e + Ek * m)
    else:
        th = int(sp.geno_idx[m]) if sp.kind == "genotype" else e + Ek * m
        u = m if sp.kind == "genotype" else e + Ek * m + Ek * nb * r
        s = D(off["theta"][0] + th) + np.exp(D(off["logtau"][0] + u)) * D(off["theta_tilde"][0] + u)
        ls = D(off["logsigma_bc"][0] + u)
    return s - sbar, np.exp(ls)


def score_cell(y, mu, sd):
    """The seven outputs of a cell from its float64 inputs, the header's formulas as they stand."""
    from scipy.special import erfc
    n = mu.shape[0]
    z = (y - mu) / sd
    l = -0.5 * z * z - np.log(sd) - 0.5 * math.log(2.0 * math.pi)
    pm = mu.sum() / n
    m = l.max()
    lbar = l.sum() / n
    return (y, pm, math.sqrt((sd * sd).sum() / n + ((mu - pm) ** 2).sum() / n), m + math.log(np.exp(l - m).sum()) - math.log(n),
            ((l - lbar) ** 2).sum() / (n - 1), (0.5 * erfc(-z / math.sqrt(2.0))).sum() / n, (0.5 * erfc(z / math.sqrt(2.0))).sum() / n)


def restate(sp, mu, omega, n_samples, seed, rows=None, cell=score_cell, want_z=False):
    """bb_ppc_score at the parameters (mu, omega), caller order, for `rows` (all): a dict as Engine.ppc_score returns, the rows'
    entries only.  `cell`: the evaluation of one cell (the golden generator passes its 50-digit one); want_z: also 'zmax', the
    largest |z_j| per cell."""
    D = Draws(seed, mu, pc.softplus(omega), n_samples)
    y = observed(sp)
    n_rows, n_steps = y.shape
    rows = np.arange(n_rows) if rows is None else np.asarray(rows)
    out = {k: np.full((len(rows), n_steps), np.nan) for k in CELLS}
    out.update({k: np.zeros(len(rows)) for k in ROWS})
    out["n_scored"] = np.zeros(len(rows), dtype=np.int32)
    if want_z:
        out["zmax"] = np.full((len(rows), n_steps), np.nan)
    for x, row in enumerate(rows):
        r = int(row) // sp.B
        acc_l, acc_p = 0.0, 0.0
        for t in range(sp.n_time[r] - 1):
            if np.isnan(y[row, t]):
                continue
            mj, sj = cell_inputs(sp, D, row, t)
            vals = cell(float(y[row, t]), mj, sj)
            for k, v in zip(CELLS, vals):
                out[k][x, t] = float(v)
            acc_l, acc_p = acc_l + vals[3], acc_p + vals[4]
            out["n_scored"][x] += 1
            if want_z:
                out["zmax"][x, t] = np.abs((y[row, t] - mj) / sj).max()
        out["row_lpd"][x], out["row_p_waic"][x] = float(acc_l), float(acc_p)
    return out


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(spec, mu, omega) of a case, computed once and read-only."""
    sp = pc.spec(case)
    mu, om = params(sp)
    mu.setflags(write=False)
    om.setflags(write=False)
    return sp, mu, om


@functools.lru_cache(maxsize=None)
def golden(name):
    case, n, rows = golden_cases()[name]
    with np.load(golden_path(name)) as f:
        g = {k: f[k] for k in f.files}
    for v in g.values():
        v.setflags(write=False)
    return g


# ---- comparison -----------------------------------------------------------------------------------------------------------------
def errors(got, ref):
    """Largest error per output under the rule of the module docstring; the NaN pattern and n_scored must be equal."""
    err = {}
    for k in CELLS + ROWS:
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        assert a.shape == b.shape, (k, a.shape, b.shape)
        assert np.array_equal(np.isnan(a), np.isnan(b)), k
        ok = ~np.isnan(b)
        if not ok.any():
            err[k] = 0.0
            continue
        den = np.abs(b[ok]) if k in SELF_RELATIVE else np.maximum(np.abs(b[ok]), 1.0)
        d = np.abs(a[ok] - b[ok])
        err[k] = float(np.max(np.where(d == 0, 0.0, d / np.where(den == 0, 1.0, den))))
    assert np.array_equal(got["n_scored"], ref["n_scored"])
    return err


def take(res, rows):
    return res if rows is None else {k: v[list(rows)] for k, v in res.items()}


def report(name, label, err):
    print(f"score case {name:28s} {label:12s} " + " ".join(f"{k} {err[k] / 1e-16:7.1f}" for k in CELLS[1:] + ROWS) + "  (1e-16)")


def check_golden(lib, name, label):
    """Case 1: every output of a call against the golden (and the float64 restatement against it, for the record); NaN exactly
    past each replicate's last step and where a count is 0."""
    case, n, rows = golden_cases()[name]
    sp, mu, om = inputs(case)
    ref = golden(name)
    r64 = restate(sp, mu, om, n, SEED, rows=rows)
    e0 = errors(r64, ref)
    report(name, "restatement", e0)
    with pc._handle(lib, sp, mu, om) as e:
        assert e.score_shape() == (sp.n_rep * sp.B, max(sp.n_time) - 1)
        got = e.ppc_score(n_samples=n, seed=SEED)
    y = observed(sp)
    assert np.array_equal(np.isnan(got["lpd"]), np.isnan(y))
    for r, T in enumerate(sp.n_time):
        assert np.all(np.isnan(got["pit"][r * sp.B:(r + 1) * sp.B, T - 1:]))
    err = errors(take(got, rows), ref)
    report(name, label, err)
    for k in CELLS + ROWS:
        assert e0[k] <= TOL, ("restatement", name, k, e0[k])
        assert err[k] <= TOL, (label, name, k, err[k])
    assert np.array_equal(got["observed"][~np.isnan(y)], y[~np.isnan(y)])
    return got


def check_z_range(name):
    """The parameters put cells of a golden at 12 <= |z| <= 20 and none beyond (CPU, the restatement)."""
    case, n, rows = golden_cases()[name]
    sp, mu, om = inputs(case)
    z = restate(sp, mu, om, n, SEED, rows=rows, want_z=True)["zmax"]
    z = z[~np.isnan(z)]
    assert z.max() <= Z_HI, z.max()
    assert np.count_nonzero(z >= Z_LO) >= 4, np.sort(z)[-6:]


def same_bytes(a, b):
    return all(np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes() for k in a) and set(a) == set(b)


def zeroed(sp, cells):
    """A copy of the spec with the counts at cells (r, t, b) set to 0 and the totals recomputed."""
    counts = [c.copy() for c in sp.counts]
    for r, t, b in cells:
        counts[r][t, b] = 0
    return ModelSpec(kind=sp.kind, counts=counts, totals=[c.sum(axis=1) for c in counts], n_neutral=sp.n_neutral, n_bc=sp.n_bc,
                     env_idx=sp.env_idx, geno_idx=sp.geno_idx)


def check_zero_counts(lib, case="replicate_ragged", n=111):
    """Case 2: a few counts set to zero: exactly the steps that touch them are NaN (against the unedited data: those, and what was
    NaN before), n_scored and the row sums follow, and the scored cells match the restatement at the recomputed totals."""
    sp, mu, om = inputs(case)
    nn = sp.n_neutral
    edits = [(0, 0, 2), (0, 2, nn + 5), (1, sp.n_time[1] - 1, nn + 1), (2, 1, 0)]
    sp2 = zeroed(sp, edits)
    y0, y2 = observed(sp), observed(sp2)
    want_nan = np.isnan(y0)
    for r, t, b in edits:
        for s in (t - 1, t):
            if 0 <= s < sp.n_time[r] - 1:
                want_nan[r * sp.B + b, s] = True
    assert np.array_equal(np.isnan(y2), want_nan)
    with pc._handle(lib, sp2, mu, om) as e:
        got = e.ppc_score(n_samples=n, seed=SEED)
    for k in CELLS:
        assert np.array_equal(np.isnan(got[k]), want_nan), k
    assert np.array_equal(got["n_scored"], (~want_nan).sum(axis=1))
    ref = restate(sp2, mu, om, n, SEED)
    err = errors(got, ref)
    report(case + "_zeroed", "vs restated", err)
    for k in CELLS + ROWS:                   # (no golden here: the float64 restatement, itself within 4.3e-14 of the 50-digit values)
        assert err[k] <= TOL, (k, err[k])
    for row in range(got["lpd"].shape[0]):   # the row sums: the scored cells in step order
        s = 0.0
        for v in got["lpd"][row][~want_nan[row]]:
            s += v
        assert s == got["row_lpd"][row]


def check_nan_parameter(lib, case="fitness", n=111):
    """Case 3: one mutant's s_bc mean NaN: its rows are NaN in everything that uses the mean, every other row keeps its bytes."""
    sp, mu, om = inputs(case)
    m = 7
    mu2 = mu.copy()
    mu2[sp.offsets()["s_bc"][0] + m] = np.nan
    with pc._handle(lib, sp, mu, om) as e:
        base = e.ppc_score(n_samples=n, seed=SEED)
    with pc._handle(lib, sp, mu2, om) as e:
        got = e.ppc_score(n_samples=n, seed=SEED)
    rows = np.array([r * sp.B + sp.n_neutral + m for r in range(sp.n_rep)])
    rest = np.setdiff1d(np.arange(base["lpd"].shape[0]), rows)
    assert same_bytes({k: v[rest] for k, v in got.items()}, {k: v[rest] for k, v in base.items()})
    scored = ~np.isnan(base["observed"][rows])
    assert scored.any()
    for k in ("pred_mean", "pred_sd", "lpd", "p_waic", "pit", "pit_upper"):
        assert np.all(np.isnan(got[k][rows][scored])), k
    assert np.all(np.isnan(got["row_lpd"][rows])) and np.all(np.isnan(got["row_p_waic"][rows]))
    assert same_bytes({k: got[k][rows] for k in ("observed", "n_scored")}, {k: base[k][rows] for k in ("observed", "n_scored")})


def raw_score(engine, n_samples, seed=SEED, null=(), want=CELLS + ROWS + ("n_scored",)):
    """bb_ppc_score through ctypes with only the outputs in `want` non-NULL; `null` names arguments passed as NULL (h, o, out)."""
    n_rows, n_steps = engine.score_shape()
    o = _capi.bb_score_opts()
    o.n_samples, o.seed = n_samples, seed
    res, out = {}, _capi.bb_score_out()
    for k in want:
        if k == "n_scored":
            res[k] = np.full(n_rows, -7, dtype=np.int32)
            out.n_scored = res[k].ctypes.data_as(C.POINTER(C.c_int32))
        else:
            res[k] = np.full((n_rows, n_steps) if k in CELLS else n_rows, -7.0)
            setattr(out, k, _capi._ptr(res[k]))
    rc = engine._lib.bb_ppc_score(None if "h" in null else engine._h, None if "o" in null else C.byref(o),
                                  None if "out" in null else C.byref(out))
    return rc, res


def check_errors(lib):
    """Case 4."""
    sp, mu, om = inputs("fitness")
    with pc._handle(lib, sp, mu, om) as e:
        for null in ("h", "o", "out"):
            assert raw_score(e, 10, null=(null,))[0] == -1, null
        for n in (0, 1, 16385, -3):
            assert raw_score(e, n)[0] == _capi.BB_ERR_UNSUPPORTED, n
        rc, big = raw_score(e, 16384)
        assert rc == 0
        assert raw_score(e, 64, want=())[0] == 0                           # an all-NULL out
        full = e.ppc_score(n_samples=64, seed=SEED)
        assert same_bytes(raw_score(e, 64)[1], full) and not same_bytes(big, full)
        for k in CELLS + ROWS + ("n_scored",):                             # every output NULL except one
            rc, one = raw_score(e, 64, want=(k,))
            assert rc == 0 and same_bytes(one, {k: full[k]}), k
        try:
            e.ppc_score(n_samples=1)
        except _capi.BarBayHipError as ex:
            assert "error -4" in str(ex)
        else:
            raise AssertionError("no error")


def check_buffer_reuse(lib):
    """Case 5: the call interleaved with the other post-fit calls at changing sizes on one handle: every result is byte for byte
    what a fresh handle gives."""
    sp, mu, om = inputs("fitness")
    om = np.minimum(om, -2.0)
    qs = (0.95, 0.675, 0.05)
    chain = np.random.default_rng(12).standard_normal((2, 5, 6))
    calls = [lambda e: e.ppc_score(n_samples=111, seed=SEED),
             lambda e: e.ppc_bands(qs, n_samples=111, n_ppc=7, seed=SEED),
             lambda e: e.ppc_score(n_samples=1000, seed=SEED),
             lambda e: e.freq_bands(qs, mode="trajectory", n_samples=111, n_ppc=7, seed=SEED),
             lambda e: e.ppc_score(n_samples=2, seed=SEED),
             lambda e: e.chain_summary(chain),
             lambda e: e.freq_bands(qs, mode="posterior", n_samples=200, n_ppc=1, seed=SEED),
             lambda e: e.ppc_score(n_samples=2049, seed=SEED),
             lambda e: e.ppc_bands(qs, n_samples=1000, n_ppc=1, seed=SEED),
             lambda e: e.ppc_score(n_samples=111, seed=SEED)]
    with pc._handle(lib, sp, mu, om) as e:
        got = [pc._bits(f(e)) for f in calls]
    for i, f in enumerate(calls):
        with pc._handle(lib, sp, mu, om) as e:
            assert got[i] == pc._bits(f(e)), i
    assert got[0] == got[9]


def check_group_handle(lib, case):
    """Case 6: a device_ids = [0, 0] group handle against a single-device handle."""
    sp, mu, om = inputs(case)
    with pc._handle(lib, sp, mu, om, device_ids=[0, 0]) as e:
        a = e.ppc_score(n_samples=111, seed=SEED)
    with pc._handle(lib, sp, mu, om) as e:
        b = e.ppc_score(n_samples=111, seed=SEED)
    assert same_bytes(a, b)


def check_handle_untouched(lib):
    """Case 7: run(5) after a score call leaves the parameters bit-equal to run(5) on a fresh handle."""
    sp = pc.spec("fitness")
    with make_engine(sp, lib, seed=5) as a, make_engine(sp, lib, seed=5) as b:
        b.ppc_score(n_samples=111, seed=SEED)
        for x, y in zip(a.get_params(), b.get_params()):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
        a.run(5)
        b.ppc_score(n_samples=64, seed=1)
        b.run(5)
        for x, y in zip(a.get_params(), b.get_params()):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
