"""bb_dfe_rb (posterior of the fitness distribution of sets of units, barbay.jl_amd/csrc/bb_dfe.h) restated in numpy on top of
`_rb_cases.conditionals`, and the cases the emulation and GPU tests share.  Per draw j and threshold x a unit gives
pl = erfc(v) / 2, pu = erfc(-v) / 2 with v = (m - x) / sd * rsqrt2 and c = [s <= x]; a set's units are summed in the caller's order
in chunks of BB_DFE_CHUNK, each chunk from 0.0, the chunks from 0.0: the header's formulas and order.

Expected values: tests/golden/dfe_<case>_n<samples>.npz, a 50-digit mpmath evaluation on this restatement's float64
(s_j, m_j, sd_j), written by tests/golden/make_dfe_golden.py; the sets of a case are `case_sets`, its grid the multiples of
1 / 1024 nearest the 10 / 25 / 50 / 75 / 90 % points of the units' rb_mean, stored with the values.  The small sets (one and three
units) are made of units that are not sharp (`_rb_cases.params` sharpens every seventh mutant) and lie near the middle of the grid,
so that their tails stay within Z_HI = 20 sds (`check_z_range`): a tail's relative error grows with |z|^2.

Bounds: per output the larger of 1e-12 and 8 x the float64 restatement's own measured error against the golden (MEASURED);
below_mean, above_mean, q_below_mean and the bands relative to the value itself, between_sd, within_sd and q_below_sd absolute
(they are sds of fractions); n_units and the NaN pattern exact.

Measured, largest error over a file's sets and grid points against the golden, float64 restatement / host emulation / MI355X, in
units of 1e-16 (each test prints its own line):

case                                         below_mean         above_mean         between_sd          within_sd       q_below_mean         q_below_sd        below_bands        above_bands
fitness_chunk_n1000                   1.9/  5.5/  5.5    2.2/  5.3/  5.6    0.1/  0.2/  0.2    0.6/  0.6/  0.6    2.7/  6.7/  6.7    0.2/  0.6/  0.6    7.2/ 18.3/ 20.0    5.5/ 26.7/ 26.7
fitness_chunk_n111                    3.7/  5.1/  4.4    3.1/  5.1/  5.9    0.3/  0.4/  0.6    0.6/  0.6/  0.6    4.8/  6.1/  6.1    0.3/  0.3/  0.3    4.4/ 37.9/ 37.9    9.0/ 32.3/ 41.5
fitness_chunk_n2                      4.4/  4.4/  4.4    3.9/  3.9/  3.8    4.1/  4.1/  4.1    0.6/  0.6/  0.6    2.1/  2.1/  2.1    0.2/  0.2/  0.2    6.1/  6.1/  6.1    9.0/  9.0/  8.9
fitness_n1000                         2.0/  2.3/  4.1    1.9/  4.8/  4.8    0.1/  0.2/  0.2    0.6/  0.6/  0.6    1.7/  3.5/  3.5    0.3/  0.4/  0.4    5.0/  5.9/  7.1    4.5/ 22.8/ 22.8
fitness_n111                          3.2/  4.7/  6.0    3.6/  5.5/  5.6    0.1/  0.2/  0.3    0.6/  1.1/  1.1    3.3/ 13.3/ 13.3    0.3/  0.6/  0.6    5.7/  6.9/  6.9   10.1/ 19.7/ 19.7
fitness_n2                            6.5/  6.5/  7.7    3.0/  7.5/  8.1    1.5/  1.7/  1.7    0.6/  1.1/  1.1    1.6/  1.6/  1.6    0.1/  0.1/  0.1    8.2/ 17.1/ 17.1    8.1/ 28.4/ 26.4
fitness_n8672                         2.1/  5.9/  5.9    4.2/  5.8/  5.2    0.0/  0.1/  0.1    0.6/  1.1/  1.1    4.3/  4.3/  4.3    0.3/  0.3/  0.3   18.5/ 22.2/ 22.2   20.8/ 20.8/ 20.8
genotype_regrouped_n1000              2.1/  6.0/  4.4    3.7/  5.6/  6.3    0.3/  0.3/  0.1    0.6/  0.3/  0.6    3.9/  2.6/  2.6    0.1/  0.1/  0.1    7.4/ 11.1/ 23.6    6.2/ 42.3/ 85.4
genotype_regrouped_n111               2.2/  4.0/  2.2    2.8/  7.0/ 10.3    0.3/  0.4/  0.3    0.6/  0.6/  0.6    5.2/  4.2/  4.2    0.1/  0.2/  0.2   12.1/ 98.1/ 98.1   29.4/ 29.4/ 62.3
genotype_regrouped_n2                 4.2/  4.2/  7.2    7.1/  7.1/  7.1    2.4/  2.4/  1.8    0.3/  0.6/  0.3    1.4/  1.4/  1.4    0.3/  0.3/  0.3   21.4/ 19.6/ 19.6   36.7/ 34.6/ 34.6
multienv_env0_only_first_n1000        4.4/  6.6/  6.6    6.9/  6.2/  6.2    0.2/  0.3/  0.3    0.3/  1.1/  0.6    4.0/  3.0/  3.0    0.3/  0.4/  0.4    6.0/ 31.2/ 35.1    9.9/ 70.4/ 71.8
multienv_env0_only_first_n111         8.8/  4.4/  4.4    5.3/  3.2/  3.4    0.3/  0.3/  0.5    1.1/  1.1/  1.1    3.4/ 10.5/ 10.5    0.3/  1.7/  1.7    7.5/  7.5/  7.5    9.6/ 13.7/ 13.7
multienv_env0_only_first_n2           8.2/  8.2/  5.9    5.2/  7.9/  6.7    1.9/  1.9/  1.9    0.6/  0.6/  0.6    1.5/  1.5/  1.5    0.3/  0.3/  0.3    9.9/  9.9/  7.2    6.7/ 10.1/ 10.1
multienv_n1000                        2.1/  6.1/  6.9    3.3/  3.3/  3.3    0.3/  0.2/  0.3    0.6/  1.1/  1.1    3.5/  6.5/  6.5    0.3/  0.3/  0.3    8.0/ 52.9/ 52.9   10.2/ 36.7/ 38.7
multienv_n111                         3.3/  7.1/  6.6    3.8/  6.8/  6.8    0.3/  0.3/  0.4    0.6/  1.1/  1.1    5.1/  6.9/  6.9    0.6/  1.7/  1.7    6.5/  9.5/  9.5    6.0/  8.8/  8.8
multienv_n2                           4.3/ 19.4/ 17.1    3.6/  5.0/  5.0    1.4/  1.9/  1.7    0.6/  1.1/  1.1    1.3/  1.3/  1.3    0.4/  0.4/  0.4    6.6/ 24.1/ 24.1    8.9/ 12.3/ 12.3
multienv_replicate_n1000             20.7/ 22.6/ 24.5   21.8/ 18.6/ 14.0    0.1/  0.3/  0.3    0.1/  0.1/  0.6    4.0/  7.0/  7.0    0.2/  0.2/  0.2   85.5/100.8/200.6   47.7/114.1/114.1
multienv_replicate_n111              41.1/ 41.1/ 39.2   14.9/ 17.1/  9.4    0.3/  0.6/  0.6    0.1/  0.6/  0.6    4.7/ 12.5/ 12.5    0.2/  0.6/  0.6   72.0/221.8/246.0  115.4/ 96.4/140.2
multienv_replicate_n2                69.0/ 54.9/ 54.9   11.6/ 15.4/ 15.4    3.3/  3.3/  3.3    0.6/  1.1/  1.1    2.0/  2.0/  2.0    0.3/  0.3/  0.3   68.8/ 55.6/ 72.9   46.4/ 45.5/ 47.0
replicate_ragged_n1000               24.6/ 22.5/ 51.2   11.4/ 11.8/ 17.2    0.1/  0.1/  0.3    0.1/  0.6/  0.6    3.9/  9.5/  9.5    0.6/  2.8/  2.8  101.4/191.6/114.0  100.4/ 94.2/ 94.2
replicate_ragged_n111                28.2/ 42.3/ 80.6   15.6/  7.8/ 17.9    0.3/  0.2/  0.2    0.1/  0.6/  0.6    4.1/  5.7/  5.7    0.6/  1.7/  1.7  163.1/134.4/248.3   34.4/ 47.2/ 55.5
replicate_ragged_n2                 103.9/106.0/101.8   48.7/ 50.4/ 83.9    2.3/  2.5/  2.5    0.1/  0.6/  2.2    1.7/  1.7/  1.7    0.3/  0.3/  0.3  107.2/181.3/130.9   54.1/ 99.9/113.8
(the largest entry of the emulation and the MI355X, 248.3e-16, is 0.025 of the bound 1e-12; the restatement's own largest,
 163.1e-16 -- a band of a one-unit set of a hierarchical case, a tail far from the unit's mean --, gives 8 x 1.63e-14 = 1.3e-13, below 1e-12: every bound is 1e-12)
"""
import ctypes as C
import functools
import os

import numpy as np

import _contrast_cases as cc
import _ppc_cases as pc
import _rb_cases as rc
import _score_cases as sc
from conftest import make_engine
from barbay_jl_amd import _capi

CELLS = _capi.DFE_CELLS
BANDS = _capi.DFE_BANDS
VALUES = CELLS + BANDS
OUTS = VALUES + ("n_units",)
SELF_RELATIVE = ("below_mean", "above_mean", "q_below_mean") + BANDS
# the float64 restatement's largest error against the goldens, per output: see the table
MEASURED = {"below_mean": 1.04e-14, "above_mean": 4.9e-15, "between_sd": 4.2e-16, "within_sd": 1.2e-16, "q_below_mean": 5.3e-16, "q_below_sd": 6.0e-17,
            "below_bands": 1.64e-14, "above_bands": 1.16e-14}
TOL = {k: max(1e-12, 8.0 * MEASURED[k]) for k in VALUES}
SEED, PROBS, NS, Z_HI = rc.SEED, rc.PROBS, rc.NS, rc.Z_HI
MAXN = _capi.BB_DFE_MAX_SAMPLES
CHUNK = _capi.BB_DFE_CHUNK
MAXG = _capi.BB_DFE_MAX_GRID
GRID = cc.GRID            # thresholds are multiples of 1 / 1024
RSQRT2 = 0.70710678118654752440
LEVELS = (10, 25, 50, 75, 90)
CASES = tuple(rc.all_cases())
BIG = {f"fitness_n{MAXN}": ("fitness", MAXN)}                    # the largest call, a handful of sets


def inputs(case):
    return rc.inputs(case)


def elements_at(case, n):
    return cc.elements_at("fitness", case, n)


# ---- the sets and grid of a case ----------------------------------------------------------------------------------------------------
def plain_units(case):
    """Units that `_rb_cases.params` leaves at their own logsigma_bc (not every seventh mutant), by |rb_mean - median| ascending."""
    sp = inputs(case)[0]
    m = elements_at(case, 111)[1].mean(axis=1)
    E, nb = rc.n_env(sp), sp.n_bc
    nst = elements_at(case, 111)[3]
    u = np.arange(rc.n_units(sp))
    plain = u[((u // E % nb) % 7 != 3) & (nst[u] > 0)]
    return [int(k) for k in plain[np.argsort(np.abs(m[plain] - np.median(m)), kind="stable")]]


@functools.lru_cache(maxsize=None)
def case_sets(case, big=False):
    """The sets of a case, each a list of units: one unit and three units out of order (`plain_units`), every unit, the first
    replicate's units, every unit reversed and, with more than one replicate or environment, the last environment's units across
    the replicates.  fitness_chunk (280 units) instead: 1, 3, all 280 (three chunks), 128 (a full chunk) and 129 descending (the
    boundary).  multienv_replicate: also a set mixing replicates and environments.  multienv_env0_only_first: also a set with
    units of environment 0, whose n_u = 0 (the prior is their conditional).  `big`: the handful of the call at the cap."""
    sp = inputs(case)[0]
    E, nb, R, nu = rc.n_env(sp), sp.n_bc, sp.n_rep, rc.n_units(sp)
    near = plain_units(case)
    sets = [[near[0]], [near[2], near[0], near[1]], list(range(nu))]
    if big:
        return tuple(tuple(s) for s in sets + [list(range(nu))[::-3]])
    if case == "fitness_chunk":
        assert nu == 280
        sets += [list(range(100, 100 + CHUNK)), list(range(151, 151 - (CHUNK + 1), -1))]
    else:
        sets += [list(range(E * nb)), list(range(nu))[::-1]]
        if R > 1 or E > 1:
            sets.append([e + E * m + E * nb * r for r in range(R) for m in range(nb) for e in (E - 1,)])
    if case == "multienv_replicate":
        sets.append([e + E * m + E * nb * r for m in (1, 2, 4, 5) for r in range(R) for e in range(E)])
    if case == "multienv_env0_only_first":
        sets.append([E * m for m in (0, 1, 2)] + [1 + E * 4, 2 + E * 5])
    for s in sets:
        assert len(set(s)) == len(s) and all(0 <= k < nu for k in s)
    return tuple(tuple(s) for s in sets)


def level_grid(case, n, levels=LEVELS):
    """The multiples of 1 / GRID nearest the `levels` % points of the rb_mean of the units that have steps (the others sit on
    their prior mean together); strictly ascending."""
    el = elements_at(case, n)
    m = el[1][el[3] > 0].mean(axis=1)
    x = np.round(np.percentile(m, levels) * GRID) / GRID
    assert np.all(np.diff(x) > 0), x
    return x


def golden_cases():
    """name -> (case, n_samples); the files are tests/golden/dfe_<name>.npz."""
    out = {f"{c}_n{n}": (c, n) for c in CASES for n in NS}
    out.update(BIG)
    return out


def golden_sets(name):
    case, n = golden_cases()[name]
    return [list(s) for s in case_sets(case, big=n > max(NS))]


def golden_path(name):
    return os.path.join(rc.GOLD, f"dfe_{name}.npz")


@functools.lru_cache(maxsize=None)
def golden(name):
    with np.load(golden_path(name)) as f:
        g = {k: f[k] for k in f.files}
    for v in g.values():
        v.setflags(write=False)
    return g


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def fractions(el, idx, grid):
    """(L, U, V, C) [n_grid, n] of the set `idx` from the elements (s, m, sd): the header's order of the sums."""
    from scipy.special import erfc
    s, m, sd, _ = el
    x = np.asarray(grid, dtype=np.float64)[:, None]
    n, shape = len(idx), (len(grid), s.shape[1])
    tot = [np.zeros(shape) for _ in range(4)]
    for c0 in range(0, n, CHUNK):
        part = [np.zeros(shape) for _ in range(4)]
        for u in idx[c0:c0 + CHUNK]:
            v = (m[u] - x) / sd[u] * RSQRT2
            pl, pu = 0.5 * erfc(v), 0.5 * erfc(-v)
            part = [part[0] + pl, part[1] + pu, part[2] + pl * pu, part[3] + (s[u] <= x)]
        tot = [t + p for t, p in zip(tot, part)]
    return tot[0] / n, tot[1] / n, tot[2] / (float(n) * float(n)), tot[3] / n


def restate(el, sets, grid, probs=PROBS, want_z=False):
    """bb_dfe_rb for `sets` on `grid` from the elements `el`: a dict as Engine.dfe_rb returns."""
    with np.errstate(all="ignore"):
        ns, ng = el[0].shape[1], len(grid)
        out = {k: np.empty((len(sets), ng)) for k in CELLS}
        out.update({k: np.empty((len(sets), ng, len(probs))) for k in BANDS})
        out["n_units"] = np.array([len(s) for s in sets], dtype=np.int64)
        if want_z:
            x = np.asarray(grid)[:, None, None]
            out["zmax"] = np.array([np.abs((el[1][list(s)] - x) / el[2][list(s)]).max() for s in sets])
        for c, idx in enumerate(sets):
            L, U, V, Cq = fractions(el, list(idx), grid)
            lm, cm = L.sum(axis=1) / ns, Cq.sum(axis=1) / ns
            out["below_mean"][c], out["above_mean"][c] = lm, U.sum(axis=1) / ns
            out["between_sd"][c] = np.sqrt(((L - lm[:, None]) ** 2).sum(axis=1) / ns)
            out["within_sd"][c] = np.sqrt(V.sum(axis=1) / ns)
            out["q_below_mean"][c], out["q_below_sd"][c] = cm, np.sqrt(((Cq - cm[:, None]) ** 2).sum(axis=1) / ns)
            for k, F in (("below_bands", L), ("above_bands", U)):
                for g in range(ng):
                    bad = len(probs) == 0 or ns < 2 or not np.isfinite(F[g]).all()
                    out[k][c, g] = np.nan if bad else [pc.quantile7(np.sort(F[g]), p) for p in probs]
    return out


# ---- comparison -----------------------------------------------------------------------------------------------------------------
def errors(got, ref, keys=VALUES):
    """Largest error per output under the rule of the module docstring; the NaN pattern and n_units must be equal."""
    err = {}
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        assert a.shape == b.shape, (k, a.shape, b.shape)
        assert np.array_equal(np.isnan(a), np.isnan(b)), k
        ok = ~np.isnan(b)
        if not ok.any():
            err[k] = 0.0
            continue
        d = np.abs(a[ok] - b[ok])
        den = np.abs(b[ok]) if k in SELF_RELATIVE else np.ones(d.shape)
        err[k] = float(np.max(np.where(d == 0, 0.0, d / np.where(den == 0, 1.0, den))))
    if "n_units" in ref:
        assert np.array_equal(got["n_units"], ref["n_units"])
    return err


def assert_within(err, who, tol=TOL):
    for k, v in err.items():
        assert v <= tol[k], (who, k, v)


def report(name, label, err):
    print(f"dfe case {name:36s} {label:12s} " + " ".join(f"{k} {err[k] / 1e-16:7.1f}" for k in err) + "  (1e-16)")


def dfe(e, sets, grid, n, **kw):
    kw.setdefault("probs", PROBS)
    kw.setdefault("seed", SEED)
    return e.dfe_rb([list(s) for s in sets] if not isinstance(sets, tuple) else sets, grid, n_samples=n, **kw)


def cell(res, c, g):
    """The results of set c at grid point g, as bytes."""
    return [np.ascontiguousarray(res[k][c, g]).tobytes() for k in VALUES] + [int(res["n_units"][c])]


def same_bytes(a, b):
    return rc.same_bytes(a, b)


def check_relations(res, tol=1e-12):
    """below_mean non-decreasing and above_mean non-increasing along the grid, below_mean + above_mean = 1, the bands ordered in
    the probabilities; where the set has no NaN."""
    ok = ~np.isnan(res["below_mean"]).any(axis=1)
    lo, hi = res["below_mean"][ok], res["above_mean"][ok]
    assert np.all(np.diff(lo, axis=1) >= 0) and np.all(np.diff(hi, axis=1) <= 0)
    assert np.abs(lo + hi - 1.0).max(initial=0.0) <= tol
    assert np.all((lo >= 0) & (lo <= 1) & (hi >= 0) & (hi <= 1))
    for k in BANDS:
        assert np.all(np.diff(res[k][ok], axis=2) >= 0), k
    for k in ("between_sd", "within_sd", "q_below_sd"):
        assert np.all(res[k][ok] >= 0), k


# ---- 1. golden values ----------------------------------------------------------------------------------------------------------
def check_golden(lib, name, label):
    case, n = golden_cases()[name]
    sp, mu, om = inputs(case)
    sets = golden_sets(name)
    ref = dict(golden(name))
    grid = ref.pop("grid")
    e0 = errors(restate(elements_at(case, n), sets, grid), ref)
    report(name, "restatement", e0)
    with pc._handle(lib, sp, mu, om) as e:
        got = dfe(e, sets, grid, n)
    assert got["below_bands"].shape == (len(sets), len(grid), len(PROBS))
    check_relations(got)
    err = errors(got, ref)
    report(name, label, err)
    assert all(e0[k] <= MEASURED[k] for k in VALUES), "the restatement's own error exceeds what the bounds were derived from"
    assert_within(err, label)
    return got


def check_z_range(name):
    """Pins the |z| = |m_j - x| / sd_j the small sets reach (CPU, the restatement): within Z_HI = 20 sds for the sets of one and
    three units, whose results are single tails; the large sets hold sharp units far from some grid point (|z| beyond 20), whose
    tails vanish beside the other units' in a fraction."""
    case, n = golden_cases()[name]
    sets = golden_sets(name)
    z = restate(elements_at(case, n), sets, golden(name)["grid"], probs=(), want_z=True)["zmax"]
    print(f"dfe z range {name}: small sets {z[:2].max():.2f}, all {z.max():.2f}")
    assert z[:2].max() <= Z_HI, z


# ---- 2. the tie to bb_fitness_rb -------------------------------------------------------------------------------------------------
def check_tie(lib, name, label):
    """Every unit of an `_rb_cases` golden as a one-unit set on the one-point grid {THRESHOLD}: below_mean = p_neg and
    above_mean = p_pos of rb_<name>.npz under that module's bound (relative to the value), within_sd = sqrt(mean_j pl pu) and
    between_sd = the sd over the draws of pl_j from the restatement's draws (absolute, the same bound).  Prints whether the bytes
    of (p_neg, p_pos) agree with fitness_rb on the same handle; the expressions are the same."""
    from scipy.special import erfc
    case, n, which = rc.golden_cases()[name]
    sp, mu, om = inputs(case)
    ref = rc.golden(name)
    which = np.arange(rc.n_units(sp)) if which is None else np.asarray(which)
    with pc._handle(lib, sp, mu, om) as e:
        got = dfe(e, [[int(u)] for u in which], [rc.THRESHOLD], n, probs=())
        own = rc.rb(e, n, probs=())
    _, m, sd, _ = elements_at(case, n)
    v = (m[which] - rc.THRESHOLD) / sd[which] * RSQRT2
    pl, pu = 0.5 * erfc(v), 0.5 * erfc(-v)
    want = {"below_mean": ref["p_neg"], "above_mean": ref["p_pos"], "within_sd": np.sqrt((pl * pu).sum(axis=1) / n),
            "between_sd": np.sqrt(((pl - pl.mean(axis=1)[:, None]) ** 2).sum(axis=1) / n)}
    err = errors({k: got[k][:, 0] for k in want}, want, keys=tuple(want))
    same = np.array_equal(got["below_mean"][:, 0], own["p_neg"][which]) and np.array_equal(got["above_mean"][:, 0], own["p_pos"][which])
    report(f"{name} one-unit", label, err)
    print(f"dfe tie {name}: bytes of (p_neg, p_pos) {'agree' if same else 'DIFFER'}")
    assert np.all(got["n_units"] == 1)
    assert_within(err, label, tol={k: rc.TOL for k in want})
    return same


# ---- 3. composition at one explicit draw ------------------------------------------------------------------------------------------
COMPOSITION_GRID = (-0.25, 0.0, 0.3125)


def check_composition(lib, case):
    """At the three points of `_contrast_cases.check_composition`, each passed as one explicit draw, no quantiles: below_mean =
    mean_u p_neg_u of fitness_rb(draws=z, threshold=x) and within_sd = sqrt(sum p_neg p_pos) / n under `_rb_cases.TOL` (relative
    to the value; absolute); between_sd = q_below_sd = 0 and q_below_mean = the fraction of q_mean <= x exactly."""
    sp = inputs(case)[0]
    sets = [list(s) for s in case_sets(case)]
    g = np.random.default_rng(8)
    with make_engine(sp, lib, seed=1) as e:
        for scale in (0.3, 1.0, 0.3):
            z = g.normal(0.0, scale, sp.D)
            got = e.dfe_rb(sets, COMPOSITION_GRID, probs=(), draws=z)
            assert got["below_bands"].shape == (len(sets), 3, 0)
            worst = 0.0
            for gi, x in enumerate(COMPOSITION_GRID):
                base = e.fitness_rb(probs=(), draws=z, threshold=x)
                for c, s in enumerate(sets):
                    k, n = np.array(s), len(s)
                    want = base["p_neg"][k].sum() / n
                    err = abs(got["below_mean"][c, gi] - want) / (abs(want) if want else 1.0)
                    wsd = np.sqrt((base["p_neg"][k] * base["p_pos"][k]).sum()) / n
                    err = max(err, abs(got["within_sd"][c, gi] - wsd))
                    worst = max(worst, err)
                    assert err <= rc.TOL, (c, x, got["below_mean"][c, gi], want, got["within_sd"][c, gi], wsd)
                    assert got["q_below_mean"][c, gi] == (base["q_mean"][k] <= x).sum() / n
            assert np.all(got["between_sd"] == 0.0) and np.all(got["q_below_sd"] == 0.0)
            print(f"dfe composition {case:28s} sd {scale}: {worst:.2e}")


# ---- 4. the point of the feature ------------------------------------------------------------------------------------------------------
def point_grid(sp, mu, om, n=1000):
    el = rc.conditionals(sp, sc.Draws(SEED, mu, pc.softplus(om), n), n)
    x = np.round(np.percentile(el[1].mean(axis=1), LEVELS) * GRID) / GRID
    return el, x


def point_ratios(res):
    return res["between_sd"][0] / res["within_sd"][0], res["q_below_sd"][0] / res["between_sd"][0]


def check_point_restated():
    """The three conditions of `check_point` on the float64 restatement alone (CPU)."""
    out = []
    for sp, mu, om in (cc.point_inputs(), rc.inputs("fitness")):
        el, x = point_grid(sp, mu, om)
        out.append(point_ratios(restate(el, [list(range(rc.n_units(sp)))], x, probs=())))
    (common, qfrac), (plain, _) = out
    print("dfe point, restatement: between / within", common, "q_below_sd / between_sd", qfrac, "unmodified inputs: between / within", plain)
    assert np.all(common > 2.0) and np.all(qfrac < 0.25) and np.all(plain < 1.0)
    return out


def check_point(lib):
    """With the population mean's posterior sd at 0.3 (`_contrast_cases.point_inputs`), n = 1000, the set of all 50 units, at the
    multiples of 1 / 1024 nearest the 10 / 25 / 50 / 75 / 90 % points of rb_mean: the fraction below x moves between the draws by
    more than twice what the Poisson-binomial spread within a draw gives (between_sd / within_sd > 2; the restatement: 3.6 .. 4.4),
    and q's own draws show less than a quarter of that movement (q_below_sd < 0.25 between_sd; the restatement: 0.10 .. 0.17).  On
    the unmodified inputs (posterior sd 0.03) the first ratio is below 1 (the restatement: 0.42 .. 0.58)."""
    out = []
    for sp, mu, om in (cc.point_inputs(), rc.inputs("fitness")):
        _, x = point_grid(sp, mu, om)
        with pc._handle(lib, sp, mu, om) as e:
            out.append(point_ratios(dfe(e, [list(range(rc.n_units(sp)))], x, 1000, probs=())))
    (common, qfrac), (plain, _) = out
    print("dfe point: between / within", common, "q_below_sd / between_sd", qfrac, "unmodified inputs: between / within", plain)
    assert np.all(common > 2.0), common
    assert np.all(qfrac < 0.25), qfrac
    assert np.all(plain < 1.0), plain
    return out


# ---- 5. determinism ------------------------------------------------------------------------------------------------------------
def wide_grid(case, n, points):
    """`points` multiples of 1 / GRID that hold the case's five grid points."""
    five = level_grid(case, n)
    lo, hi = five[0] - 8 / GRID, five[-1] + 8 / GRID
    extra = np.round(np.linspace(lo, hi, points) * GRID) / GRID
    x = np.unique(np.concatenate([five, extra]))
    drop = [v for v in x if v not in five][:len(x) - points]
    x = np.array([v for v in x if v not in drop])
    assert len(x) == points and np.all(np.diff(x) > 0)
    return x, [int(np.flatnonzero(x == v)[0]) for v in five]


def check_independent_of_the_rest_of_the_call(lib, case, n=111):
    """A cell's bytes do not depend on the call's other sets or grid points, their number or order, a set occurring twice, CSR
    against lists, or the slabs (a slab bound of 1, 3 and 7 tables against the default: sets one at a time, the grid cut);
    permuting the units within a set moves the results by no more than the bounds."""
    sp, mu, om = inputs(case)
    sets = [list(s) for s in case_sets(case)]
    five = level_grid(case, n)
    g64, at64 = wide_grid(case, n, MAXG)
    g9, at9 = wide_grid(case, n, 9)
    perm = np.random.default_rng(3).permutation(len(sets))
    with pc._handle(lib, sp, mu, om) as e:
        base = dfe(e, sets, five, n)
        again = dfe(e, sets, five, n)
        shuffled = dfe(e, [sets[i] for i in perm], five, n)
        more = dfe(e, sets[::2] + sets, five, n)                 # (a set may occur twice in a call)
        alone = [dfe(e, [sets[i]], five, n) for i in (0, len(sets) - 1)]
        csr = dfe(e, (np.cumsum([0] + [len(s) for s in sets]), [k for s in sets for k in s]), five, n)
        one = [dfe(e, sets, [x], n) for x in five]                # grids of one point: the group of 1
        wide = dfe(e, sets, g64, n)                              # BB_DFE_MAX_GRID points: groups of 8
        nine = dfe(e, sets, g9, n)                               # 8 + 1
        slabs = [dfe(e, sets, g9, n, _slab_tables=k) for k in (1, 3, 7, 40)]
        flipped = dfe(e, [s[::-1] for s in sets], five, n)
    assert same_bytes(base, again) and same_bytes(base, csr)
    G = range(len(five))
    for x, i in enumerate(perm):
        assert all(cell(shuffled, x, g) == cell(base, i, g) for g in G), i
    half = len(sets[::2])
    for i in range(len(sets)):
        assert all(cell(more, half + i, g) == cell(base, i, g) for g in G), i
        assert i % 2 or all(cell(more, i // 2, g) == cell(base, i, g) for g in G), i
        for g in G:
            assert cell(one[g], i, 0) == cell(base, i, g), (i, g)
            assert cell(wide, i, at64[g]) == cell(base, i, g), (i, g)
            assert cell(nine, i, at9[g]) == cell(base, i, g), (i, g)
    assert all(cell(alone[0], 0, g) == cell(base, 0, g) and cell(alone[1], 0, g) == cell(base, len(sets) - 1, g) for g in G)
    for s in slabs:
        assert same_bytes(s, nine)
    check_relations(wide)
    err = errors(flipped, base)
    report(f"{case}_n{n}", "units flipped", err)
    assert_within(err, "units flipped")


def check_grid_sizes_against_restatement(lib, case="multienv", n=111):
    """Grids of 1, 5 and BB_DFE_MAX_GRID points against the float64 restatement (itself within MEASURED of a golden on the five)."""
    sp, mu, om = inputs(case)
    sets = [list(s) for s in case_sets(case)][2:]                 # (the large sets: the wide grid leaves the small ones' |z| range)
    el = elements_at(case, n)
    with pc._handle(lib, sp, mu, om) as e:
        for grid in (level_grid(case, n)[2:3], level_grid(case, n), wide_grid(case, n, MAXG)[0]):
            got = dfe(e, sets, grid, n)
            err = errors(got, restate(el, sets, grid))
            report(f"{case}_n{n}_g{len(grid)}", "vs restated", err)
            assert_within(err, f"{len(grid)} grid points")
            check_relations(got)


def check_launch_modes(lib, case="replicate_ragged"):
    import barbay_jl_amd as bb
    sp, mu, om = inputs(case)
    sets, grid = [list(s) for s in case_sets(case)], level_grid(case, 111)
    out = []
    for mode in (1, 0):
        with bb.Engine(sp.kind, sp.counts, sp.n_neutral, sp.n_bc, env_idx=sp.env_idx, geno_idx=sp.geno_idx, seed=4, launch_mode=mode, _lib=lib) as e:
            e.set_params(mu, om)
            out.append(dfe(e, sets, grid, 500, seed=2))
            out.append(dfe(e, sets, grid, 500, seed=2))
    assert all(same_bytes(out[0], o) for o in out[1:])


def check_group_handle(lib, case):
    sp, mu, om = inputs(case)
    sets, grid = [list(s) for s in case_sets(case)], level_grid(case, 111)
    with pc._handle(lib, sp, mu, om, device_ids=[0, 0]) as e:
        a = dfe(e, sets, grid, 111)
    with pc._handle(lib, sp, mu, om) as e:
        b = dfe(e, sets, grid, 111)
    assert same_bytes(a, b)


def check_buffer_reuse(lib):
    """`_rb_cases.check_buffer_reuse` with the call among the other post-fit calls, at changing sizes, sets and grids on one
    handle (the buffer regrows and is reused stale): every result is byte for byte what a fresh handle gives."""
    sp, mu, om = rc.inputs("fitness")
    om = np.minimum(om, -2.0)
    qs = (0.95, 0.675, 0.05)
    chain = np.random.default_rng(12).standard_normal((2, 5, 6))
    dr = rc.materialise(sp, mu, om, 7, 3)
    sets, grid = [list(s) for s in case_sets("fitness")], level_grid("fitness", 111)
    terms = cc.contrast_set("fitness", "fitness")
    calls = [lambda e: dfe(e, sets, grid, 111),
             lambda e: e.ppc_bands(qs, n_samples=111, n_ppc=7, seed=SEED),
             lambda e: dfe(e, sets[:2], grid[:1], 1000),
             lambda e: rc.rb(e, 111),
             lambda e: e.freq_bands(qs, mode="posterior", n_samples=200, n_ppc=1, seed=SEED),
             lambda e: dfe(e, sets + sets, grid, 2),
             lambda e: e.chain_summary(chain),
             lambda e: e.ppc_score(n_samples=111, seed=SEED),
             lambda e: dfe(e, sets[2:], grid, 7, draws=dr),
             lambda e: cc.crb(e, terms, "fitness", 64),
             lambda e: dfe(e, sets[:1], grid, 2049, probs=(0.5,)),
             lambda e: e.popmean_rb(n_samples=64, seed=SEED),
             lambda e: dfe(e, sets, grid, 111)]
    with pc._handle(lib, sp, mu, om) as e:
        got = [pc._bits(f(e)) for f in calls]
    for i, f in enumerate(calls):
        with pc._handle(lib, sp, mu, om) as e:
            assert got[i] == pc._bits(f(e)), i
    assert got[0] == got[-1]


def check_handle_untouched(lib):
    sp = rc.spec("fitness")
    sets, grid = [list(s) for s in case_sets("fitness")], level_grid("fitness", 111)
    with make_engine(sp, lib, seed=5) as a, make_engine(sp, lib, seed=5) as b:
        dfe(b, sets, grid, 111)
        for x, y in zip(a.get_params(), b.get_params()):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
        a.run(5)
        dfe(b, sets, grid, 64, seed=1)
        b.run(5)
        for x, y in zip(a.get_params(), b.get_params()):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64))


def check_internal_against_explicit_draws(lib, case, n=111):
    """The library's own draws against the same draws made on the host and passed in: within the bounds of the goldens."""
    sp, mu, om = inputs(case)
    sets, grid = [list(s) for s in case_sets(case)], level_grid(case, n)
    dr = rc.materialise(sp, mu, om, n, SEED)
    with pc._handle(lib, sp, mu, om) as e:
        a = dfe(e, sets, grid, n)
        b = dfe(e, sets, grid, n, draws=dr)
        c = dfe(e, sets, grid, 5, draws=dr)                      # n_samples is the row count; the argument is ignored
    assert same_bytes(b, c)
    err = errors(a, b)
    report(f"{case}_n{n}", "own/explicit", err)
    assert_within(err, "explicit draws")


# ---- 6. non-finite values and errors ---------------------------------------------------------------------------------------------
RB_VALUES = ("below_mean", "above_mean", "between_sd", "within_sd") + BANDS


def check_nan_parameter(lib, case="multienv", n=111):
    """One mutant's logsigma_bc means NaN: exactly the sets that name one of its units are NaN in the Rao-Blackwellised outputs
    and the bands (q_below_* and n_units are not: the draws' own fitness is finite); every other set keeps its bytes."""
    sp, mu, om = rc.inputs(case)
    E, m = rc.n_env(sp), 4
    sets, grid = [list(s) for s in case_sets(case)] + [[0, 1, 2], [E * 9 + 1]], level_grid(case, n)
    mu2 = mu.copy()
    lo = sp.offsets()["logsigma_bc"][0]
    mu2[lo + E * m:lo + E * (m + 1)] = np.nan
    with pc._handle(lib, sp, mu, om) as e:
        base = dfe(e, sets, grid, n)
    with pc._handle(lib, sp, mu2, om) as e:
        got = dfe(e, sets, grid, n)
    bad = [c for c, s in enumerate(sets) if any(E * m <= k < E * (m + 1) for k in s)]
    assert 0 < len(bad) < len(sets)
    for c in range(len(sets)):
        for g in range(len(grid)):
            if c not in bad:
                assert cell(got, c, g) == cell(base, c, g), (c, g)
                continue
            for k in RB_VALUES:
                assert np.all(np.isnan(got[k][c, g])), (c, g, k)
            for k in ("q_below_mean", "q_below_sd", "n_units"):
                assert np.ascontiguousarray(got[k][c]).tobytes() == np.ascontiguousarray(base[k][c]).tobytes(), (c, k)


def raw(engine, sets, grid=(0.0, 0.25), n_samples=64, probs=PROBS, seed=SEED, draws=None, null=(), want=OUTS, n_quantiles=None, n_sets=None,
        ptr=None, nout=None, n_grid=None, reserved0=0):
    """bb_dfe_rb through ctypes with only the outputs in `want` non-NULL; `null` names arguments passed as NULL (h, o, out, probs,
    grid, set_ptr, set_idx); `ptr`, `n_sets`, `n_grid`: in place of what `sets` and `grid` give."""
    tp = np.ascontiguousarray(np.cumsum([0] + [len(s) for s in sets]) if ptr is None else ptr, dtype=np.int64)
    ti = np.ascontiguousarray([k for s in sets for k in s] + [0], dtype=np.int64)
    p = np.ascontiguousarray(probs, dtype=np.float64)
    x = np.ascontiguousarray(list(grid) + [0.0], dtype=np.float64)
    ng = len(grid) if n_grid is None else n_grid
    nc = len(sets) if n_sets is None else n_sets
    o = _capi.bb_dfe_opts()
    o.n_samples, o.n_quantiles, o.n_grid, o.reserved0, o.seed, o.n_sets = n_samples, len(p) if n_quantiles is None else n_quantiles, ng, reserved0, seed, nc
    o.probs = None if "probs" in null or not len(p) else _capi._ptr(p)
    o.grid = None if "grid" in null else _capi._ptr(x)
    i64 = C.POINTER(C.c_int64)
    o.set_ptr = None if "set_ptr" in null else tp.ctypes.data_as(i64)
    o.set_idx = None if "set_idx" in null else ti.ctypes.data_as(i64)
    if draws is not None:
        o.draws = _capi._ptr(draws)
    nout = max(nc, 0) if nout is None else nout
    res, out = {}, _capi.bb_dfe_out()
    for k in want:
        if k == "n_units":
            res[k] = np.full(nout, -7, dtype=np.int64)
            out.n_units = res[k].ctypes.data_as(i64)
        else:
            res[k] = np.full((nout, len(grid), len(p)) if k in BANDS else (nout, len(grid)), -7.0)
            setattr(out, k, _capi._ptr(res[k]))
    rcode = engine._lib.bb_dfe_rb(None if "h" in null else engine._h, None if "o" in null else C.byref(o), None if "out" in null else C.byref(out))
    return rcode, res


def check_errors(lib):
    """Every BB_ERR_INVALID and BB_ERR_UNSUPPORTED of the contract, with a message that names the set and the position; an
    all-NULL out, each output alone, n_sets == 0.  NOT exercised: BB_ERR_DEVICE (see `_rb_cases.check_errors`), and the 2^31
    indices of BB_ERR_UNSUPPORTED as real arrays -- only through a set_ptr that claims them."""
    sp, mu, om = rc.inputs("fitness")
    INVALID, UNSUPPORTED = -1, _capi.BB_ERR_UNSUPPORTED
    msg = lambda: lib.bb_last_error().decode()
    sets = [list(s) for s in case_sets("fitness")]
    nu = rc.n_units(sp)
    dr = rc.materialise(sp, mu, om, 3, 1)
    with pc._handle(lib, sp, mu, om) as e:
        for null in ("h", "o", "out"):
            assert raw(e, sets, null=(null,))[0] == INVALID and msg(), null
        for null in ("set_ptr", "set_idx"):
            assert raw(e, sets, null=(null,))[0] == INVALID and "null" in msg(), null
        assert raw(e, sets, null=("grid",))[0] == INVALID and "grid" in msg() and "null" in msg()
        assert raw(e, sets, n_sets=-1)[0] == INVALID and "n_sets" in msg()
        assert raw(e, sets, reserved0=-1)[0] == INVALID and "reserved0" in msg()
        for ng in (0, -1, MAXG + 1):
            assert raw(e, sets, n_grid=ng)[0] == INVALID and "n_grid" in msg(), ng
        for bad in (np.inf, -np.inf, np.nan):
            assert raw(e, sets, grid=(0.0, bad))[0] == INVALID and "grid point 1" in msg() and "finite" in msg(), bad
        for grid in ((0.0, 0.0), (0.0, 0.5, 0.25)):
            assert raw(e, sets, grid=grid)[0] == INVALID and f"grid point {len(grid) - 1}" in msg() and "ascending" in msg(), grid
        assert raw(e, sets, ptr=[1] + [2 * (i + 1) for i in range(len(sets))])[0] == INVALID and "set_ptr[0]" in msg()
        assert raw(e, sets[:3], ptr=[0, 2, 1, 3])[0] == INVALID and "set 1" in msg() and "decreases" in msg()
        assert raw(e, [sets[0], [], sets[1]])[0] == INVALID and "set 1" in msg() and "no units" in msg()
        for bad in (-1, nu, 1 << 40):
            assert raw(e, [sets[0], [3, bad]])[0] == INVALID and "set 1, position 1" in msg() and "outside" in msg(), bad
        assert raw(e, [sets[0], sets[1], [3, 5, 3]])[0] == INVALID and "set 2, position 2" in msg() and "twice" in msg()
        for nq in (-1, 9):
            assert raw(e, sets, n_quantiles=nq)[0] == INVALID and "n_quantiles" in msg(), nq
        assert raw(e, sets, null=("probs",), n_quantiles=3)[0] == INVALID and "probs" in msg()
        for bad in (0.0, 1.0, -0.1, 1.5, np.nan):
            assert raw(e, sets, probs=(0.5, bad))[0] == INVALID and "prob" in msg(), bad
        for n in (1, 0, -3, MAXN + 1):
            assert raw(e, sets, n_samples=n)[0] == UNSUPPORTED and "n_samples" in msg(), n
        for n in (0, MAXN + 1):
            assert raw(e, sets, n_samples=n, draws=dr)[0] == UNSUPPORTED and "n_samples" in msg(), n
        assert raw(e, sets, n_samples=1, draws=dr)[0] == UNSUPPORTED and "n_quantiles" in msg()      # quantiles over one draw
        assert raw(e, sets[:1], ptr=[0, 1 << 31], nout=1)[0] == UNSUPPORTED and "2^31" in msg()
        assert raw(e, sets, n_samples=1, draws=dr, probs=())[0] == 0 and raw(e, sets, n_samples=3, draws=dr)[0] == 0      # one explicit draw is served
        rcode, res = raw(e, sets, n_sets=0, nout=2)                                      # nothing computed, nothing written
        assert rcode == 0 and all(np.all(v == -7) for v in res.values())
        assert raw(e, sets, n_sets=0, null=("set_ptr", "set_idx"))[0] == 0
        assert raw(e, sets, want=())[0] == 0                                             # an all-NULL out
        assert raw(e, sets, probs=())[0] == 0                                            # no quantiles
        full = dfe(e, sets, (0.0, 0.25), 64)
        assert same_bytes(raw(e, sets)[1], full)
        for k in OUTS:                                                                   # every output NULL except one
            rcode, one = raw(e, sets, want=(k,))
            assert rcode == 0 and same_bytes(one, {k: full[k]}), k
        for bad, what in ((dict(n_samples=1), "n_samples"), (dict(draws=np.zeros((3, sp.D + 1))), "draws"), (dict(grid=[0.5, 0.25]), "ascending")):
            try:
                e.dfe_rb(sets, **{"grid": (0.0, 0.25), **bad})
            except _capi.BarBayHipError as ex:
                assert what in str(ex)
            else:
                raise AssertionError("no error")
        try:
            e.dfe_rb((np.array([0, 5]), np.arange(3)), (0.0,))
        except _capi.BarBayHipError as ex:
            assert "ptr" in str(ex)
        else:
            raise AssertionError("no error")
