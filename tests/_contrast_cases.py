"""bb_contrast_rb (Rao-Blackwellised fitness contrasts, barbay.jl_amd/csrc/bb_contrast.h) restated in numpy on top of the
restatements of its two element spaces -- `_rb_cases.conditionals` (fitness units) and `_theta_rb_cases.conditionals` (groups) --
and `_rb_cases.unit64`, and the cases the emulation and GPU tests share.  Per draw the contrast's (d_j, M_j, sd_j) are
sum w s, sum w m, sqrt(sum (w sd)(w sd)), each sum from 0.0 in the caller's term order: the header's formulas.

Expected values.  One-term contrasts of weight 1.0: the committed goldens of the two element calls, tests/golden/rb_*.npz and
theta_rb_*.npz, under those modules' own bounds (only sqrt(sd * sd) differs: an ulp at most).  True multi-term mixtures:
tests/golden/contrast_<case>_n<samples>.npz, a 50-digit mpmath evaluation on this restatement's float64 (d_j, M_j, sd_j), written
by tests/golden/make_contrast_golden.py with `make_rb_golden.unit_mp`; a contrast's tails are taken at the multiple of
1 / GRID = 1 / 1024 nearest its rb_mean, since M_j is a difference of O(1) numbers and a tail's relative error grows
with |z|^2 (`check_z_range` pins the |z| reached).

Bounds: per output the larger of 1e-12 and 8 x the float64 restatement's own measured error against the golden (MEASURED for the
six moments and tails, Q_MEASURED for the quantiles), relative to max(|x|, 1) for q_mean, q_sd, rb_mean, rb_sd and the quantiles,
to the value itself for p_pos and p_neg; min_steps and the NaN pattern exact.

Measured, largest error over a file's contrasts against the golden, float64 restatement / host emulation / MI355X, in units of
1e-16 (each test prints its own line):

case                                                       q_mean               q_sd            rb_mean              rb_sd              p_pos              p_neg          quantiles
fitness:fitness_chunk_n1000              1.5/  4.4/  4.4    0.6/  0.6/  0.1    1.5/  2.2/  2.9    0.0/  1.8/  1.8    0.0/  4.4/  4.4    0.0/  4.4/  2.2    4.9/ 12.2/ 12.2 
fitness:fitness_chunk_n111               3.0/  3.0/  3.0    0.0/  0.6/  1.7    3.3/  2.2/  2.2    0.3/  0.3/  1.8    2.2/  4.4/  6.7    1.1/  6.7/  7.8    3.4/ 22.9/ 19.7 
fitness:fitness_chunk_n2                 0.0/  0.0/  6.5    0.0/  2.2/ 20.0    0.0/  0.0/  0.0    0.1/  0.1/  0.1    1.1/  1.1/  2.2    2.2/  2.2/  2.2    1.6/  1.6/  4.9 
fitness:fitness_n1000                    0.1/  5.0/  5.0    0.0/  0.1/  0.1    1.1/  1.1/  1.1    0.3/  0.3/  0.3    2.2/  3.3/  2.2    1.1/  2.2/  2.2    2.2/  5.0/  5.0 
fitness:fitness_n111                     1.7/  5.0/  5.0    0.0/  0.1/  0.1    2.2/  0.6/  0.6    0.1/  0.3/  0.3    2.2/  2.2/  2.2    2.2/  2.2/  2.2    2.2/  5.6/  5.6 
fitness:fitness_n2                       0.0/  0.0/  0.0    0.0/  0.0/  0.0    0.0/  0.0/  0.0    0.3/  0.3/  0.3    2.2/  2.2/  2.2    1.1/  3.3/  3.3    1.1/  1.1/  1.1 
fitness:fitness_n2049                    1.1/  3.4/  3.4    0.0/  0.1/  0.1    0.0/  1.1/  1.1    0.3/  0.3/  0.3    2.2/  4.4/  4.4    1.1/  3.3/  4.4    3.3/  3.3/  3.3 
fitness:fitness_n8672                    1.7/  2.6/  2.6    0.0/  0.1/  0.1    0.6/  1.1/  1.1    0.0/  0.3/  0.3    2.2/  4.4/  4.4    2.2/  3.3/  3.3    1.1/  2.2/  2.2 
fitness:genotype_regrouped_n1000         1.1/  3.6/  3.6    0.3/  0.6/  0.6    0.6/  2.2/  1.1    0.0/  0.1/  0.1    2.2/  4.5/  3.3    2.2/  4.4/  4.4    1.1/  3.9/  3.9 
fitness:genotype_regrouped_n111          1.8/  3.7/  3.7    0.3/  0.6/  0.8    0.1/  2.2/  2.2    0.1/  0.1/  0.1    2.3/  4.5/  4.5    2.2/  4.4/  4.4    2.8/  2.1/  2.9 
fitness:genotype_regrouped_n2            0.0/  0.3/  2.2    0.0/  2.2/  4.4    0.0/  2.2/  2.2    0.1/  0.3/  0.6    2.2/ 15.5/ 15.5    2.2/ 16.7/ 16.7    0.6/  2.2/  2.2 
fitness:multienv_env0_only_first_n1000   1.6/  4.7/  4.7    0.1/  0.1/  0.1    0.1/  1.1/  1.1    0.6/  4.4/  4.4    2.2/  3.3/  4.4    2.2/  4.4/  4.4   13.2/ 35.9/ 35.9 
fitness:multienv_env0_only_first_n111    1.6/  1.6/  1.6    0.1/  0.2/  0.2    0.6/  2.2/  2.2    2.2/  2.2/  2.2    2.2/  2.2/  2.2    1.1/  2.2/  2.2   43.4/ 33.1/ 33.1 
fitness:multienv_env0_only_first_n2      0.0/  0.0/  0.0    0.0/  0.0/  0.0    0.0/  1.1/  1.1    0.6/  0.6/  0.0    2.2/  4.4/  4.4    1.1/  4.4/  4.4    6.4/  6.4/  6.4 
fitness:multienv_n1000                   1.3/  3.3/  3.3    0.1/  0.1/  0.1    0.6/  1.7/  1.1    0.3/  0.6/  0.6    2.2/  3.3/  3.3    2.2/  3.3/  3.3    4.4/ 21.7/ 21.7 
fitness:multienv_n111                    3.3/  2.5/  2.5    0.1/  0.1/  0.1    1.1/  1.1/  1.1    0.6/  0.6/  0.6    2.2/  5.6/  4.4    2.2/  4.5/  4.5   10.0/ 10.0/ 13.1 
fitness:multienv_n2                      0.0/  0.0/  0.0    0.0/  0.3/  0.3    0.0/  0.6/  0.6    0.6/  0.6/  0.3    2.2/  2.2/  2.2    1.1/  1.1/  2.2    3.3/  3.3/  3.3 
fitness:multienv_replicate_n1000         1.3/  2.6/  1.6    0.0/  0.6/  0.6    0.6/  2.2/  2.2    0.1/  0.1/  0.1    2.2/  4.4/  3.3    1.1/  4.4/  2.2    1.1/  2.2/  2.2 
fitness:multienv_replicate_n111          2.6/  4.9/  2.5    0.1/  0.6/  0.8    0.6/  0.7/  0.7    0.1/  0.1/  0.1    2.2/  2.2/  3.3    1.1/  4.4/  4.4    3.3/  3.3/  3.3 
fitness:multienv_replicate_n2            0.0/  2.2/  6.7    0.0/  2.2/  2.2    0.0/  0.6/  1.1    0.1/  0.1/  0.1    2.2/  7.8/ 12.2    1.1/  7.8/ 13.3    1.1/  1.1/  1.7 
fitness:replicate_ragged_n1000           1.2/  4.6/  4.6    0.0/  0.3/  0.6    0.3/  2.2/  2.2    0.1/  0.1/  0.1    1.1/  6.6/  6.6    1.1/  3.4/  4.5    1.7/  1.4/  1.4 
fitness:replicate_ragged_n111            1.2/  2.3/  2.3    0.3/  0.3/  0.8    1.1/  2.2/  2.2    0.1/  0.1/  0.1    2.2/  2.3/  4.4    2.2/  3.3/  2.2    3.1/  4.6/  4.0 
fitness:replicate_ragged_n2              0.0/  0.6/  2.2    0.0/  0.6/  4.4    0.0/  0.3/  0.3    0.1/  0.1/  0.5    2.2/  4.4/  4.4    2.2/  2.2/  5.6    1.1/  1.1/  1.1 
theta:genotype_chunks_n1000              0.3/  0.3/  0.3    0.1/  0.1/  0.1    0.6/  4.8/  4.8    0.3/  0.6/  0.6    1.1/  2.3/  4.4    2.2/  4.4/  4.4    4.4/  7.8/  6.7 
theta:genotype_chunks_n111               0.3/  0.6/  0.6    0.1/  0.1/  0.1    3.9/  6.6/  3.9    0.3/  0.6/  0.6    2.2/  4.4/ 10.1    2.2/  4.5/  4.4    7.8/ 13.3/ 13.3 
theta:genotype_chunks_n2                 0.0/  0.0/  0.0    0.0/  0.0/  0.0    0.0/  0.6/  3.2    0.3/  0.4/  1.0    1.1/ 14.5/ 68.5    2.2/ 15.5/ 68.0    2.2/  2.2/  3.1 
theta:genotype_regrouped_n1000           1.1/  1.1/  1.1    0.0/  0.1/  0.1    2.0/  4.6/  4.0    0.1/  0.3/  0.4    1.1/  6.6/  4.5    2.2/  4.5/  6.7    1.8/  2.8/  1.8 
theta:genotype_regrouped_n111            1.1/  2.2/  2.2    0.1/  0.1/  0.1    3.6/  6.2/  6.2    0.0/  0.1/  0.4    2.4/  4.4/  6.6    2.2/  4.4/  6.7    2.2/  3.4/  3.4 
theta:genotype_regrouped_n2              0.0/  0.3/  0.3    0.0/  0.3/  0.8    0.0/  3.0/  3.3    0.1/  1.8/  3.7    2.2/ 36.8/ 33.0    1.1/ 35.4/ 33.6    2.1/  2.1/  4.4 
theta:multienv_replicate_n1000           0.6/  1.1/  1.1    0.1/  0.1/  0.1    1.1/  2.6/  2.6    0.3/  0.3/  0.3    2.2/  3.3/  3.3    2.2/  6.7/  6.7    4.4/ 24.4/ 24.4 
theta:multienv_replicate_n111            1.1/  0.6/  0.6    0.1/  0.1/  0.1    1.1/  2.2/  3.9    0.3/  0.4/  0.6    2.2/  4.3/  2.2    3.3/  2.3/  4.4    5.0/ 18.9/ 18.9 
theta:multienv_replicate_n2              0.0/  0.6/  1.1    0.0/  0.3/  0.6    0.0/  1.4/  2.2    0.3/  0.3/  3.5    2.2/  6.7/ 28.8    2.2/  6.6/ 28.9    3.3/  3.3/  3.3 
theta:replicate_ragged_n1000             0.6/  1.7/  1.7    0.1/  0.1/  0.1    1.3/  2.6/  3.9    0.1/  0.1/  0.1    1.1/  5.6/ 11.3    0.0/  6.6/  8.8    2.1/  7.8/  7.8 
theta:replicate_ragged_n111              0.6/  1.1/  1.1    0.1/  0.1/  0.1    1.3/  4.3/  4.3    0.1/  0.4/  0.3    1.1/  6.7/ 11.1    2.2/  6.7/ 11.1    4.4/  8.9/  8.9 
theta:replicate_ragged_n2                0.0/  0.6/  0.6    0.0/  0.6/  0.6    0.0/  0.0/  2.0    0.1/  0.1/  1.9    2.2/  2.2/ 37.6    1.1/  1.1/ 36.7    2.2/  2.2/  3.9 
(the largest entry of the first six columns, 68.5e-16, is 0.007 of the bound 1e-12; the largest quantile entry, 43.4e-16,
 is 0.0043 of QTOL = 1e-12; the restatement's own largest are 3.9e-16 (MEASURED) and 43.4e-16 (Q_MEASURED), 8 x which is below
 1e-12 in both, so both bounds are 1e-12)
"""
import ctypes as C
import functools
import os

import numpy as np

import _ppc_cases as pc
import _rb_cases as rc
import _score_cases as sc
import _theta_rb_cases as tr
from conftest import make_engine
from barbay_jl_amd import _capi

UNITS = rc.UNITS
OUTS = UNITS + ("quantiles", "min_steps")
MEASURED = 4.0e-16        # the float64 restatement's largest error of the six moments and tails against the goldens: see the table
Q_MEASURED = 4.4e-15      # ... and of the quantiles
TOL = max(1e-12, 8.0 * MEASURED)
QTOL = max(1e-12, 8.0 * Q_MEASURED)
SEED, PROBS, NS, MAXN, Z_HI = rc.SEED, rc.PROBS, rc.NS, rc.MAXN, rc.Z_HI
GRID = 1024.0             # a contrast's tails are taken at the multiple of 1 / GRID nearest its rb_mean (`nearest`): a contrast of hyper-fitnesses of
                          # the replicate kinds has an sd near 0.001, |z| beyond 20 for every draw on a grid of 1 / 16
SPACES = ("fitness", "theta")
F_CASES = tuple(rc.all_cases())                                   # fitness, genotype_regrouped, multienv, multienv_replicate, replicate_ragged,
                                                                  # multienv_env0_only_first (n_u = 0), fitness_chunk (B = 300: the 256-column chunk)
T_CASES = tr.CASES                                                # genotype_chunks (members 1 / 64 / 65 / rest), genotype_regrouped, multienv_replicate, replicate_ragged
SPACE_CASES = [("fitness", c) for c in F_CASES] + [("theta", c) for c in T_CASES]
BIG = {"fitness_n2049": ("fitness", "fitness", 2049), f"fitness_n{MAXN}": ("fitness", "fitness", MAXN)}      # a handful of contrasts each


def inputs(case):
    return tr.inputs(case) if case == "genotype_chunks" else rc.inputs(case)


def n_space(space, sp):
    return rc.n_units(sp) if space == "fitness" else tr.n_groups(sp)


# ---- the contrasts of a case ------------------------------------------------------------------------------------------------------
def contrast_set(space, case, big=False):
    """The contrasts of a case, each a list of (index, weight): pairs within a replicate (the sharp mutants 3, 10, 17 of
    `_rb_cases.params`), a sum, across environments, across replicates, the same and different genotypes, a 5-term weighted
    mean-minus-mean, and on fitness_chunk one contrast of 130 terms with non-dyadic weights.  `big`: the handful of the 2049 / 8672 calls."""
    sp = inputs(case)[0]
    E, nb, R = rc.n_env(sp), sp.n_bc, sp.n_rep
    cs = []
    if space == "fitness":
        u = lambda r, m, e=0: e + E * m + E * nb * r
        cs += [[(u(0, 10), 1.0), (u(0, 3), -1.0)], [(u(0, 17), 1.0), (u(0, 10), -1.0)], [(u(0, 10), 1.0), (u(0, 3), 1.0)]]
        cs.append([(u(R - 1, m, E - 1), w) for m, w in ((1, 1 / 3), (2, 1 / 3), (3, 1 / 3), (4, -0.5), (5, -0.5))])
        if big:
            return cs + [[(u(0, nb - 1), 1.0), (u(0, 0), -0.7)]]
        for m in (3, 4):                                          # across environments, every pair
            cs += [[(u(0, m, b), 1.0), (u(0, m, a), -1.0)] for a in range(E) for b in range(a + 1, E)]
        for r in range(1, R):                                     # across replicates
            cs += [[(u(r, 3, E - 1), 1.0), (u(0, 3, E - 1), -1.0)], [(u(r, 5), 1.0), (u(r - 1, 6), -1.0)]]
        if sp.kind == "genotype":
            gi = np.asarray(sp.geno_idx)
            same = np.flatnonzero(gi == gi[0])
            other = np.flatnonzero(gi != gi[0])
            cs += [[(int(same[1]), 1.0), (0, -1.0)], [(int(other[0]), 1.0), (0, -1.0)], [(int(other[-1]), 1.0), (int(same[-1]), -1.0)]]
        if case == "fitness_chunk":                               # every other mutant of 260: both sides of the normalisers' chunk boundary
            cs.append([(2 * k, (-1.0) ** k * (0.1 + 0.013 * k)) for k in range(130)])
        cs.append([(u(0, 7), 0.3)])                               # a single term with a weight
    else:
        G = tr.n_groups(sp)
        cs += [[(1, 1.0), (0, -1.0)], [(2, 1.0), (1, -1.0)], [(G - 1, 1.0), (0, -1.0)], [(0, 1.0), (1, 1.0)], [(3, -0.7)]]
        if G >= 5:
            cs.append([(g, w) for g, w in ((1, 1 / 3), (2, 1 / 3), (3, 1 / 3), (4, -0.5), (G - 1, -0.5))])
        else:                                                     # genotype_chunks: one member, a full chunk, a chunk boundary, several chunks
            cs += [[(b, 1.0), (a, -1.0)] for a in range(G) for b in range(a + 2, G)] + [[(0, 1 / 3), (1, 1 / 3), (2, 1 / 3), (3, -1.0)]]
        if E > 1:                                                 # a mutant across its environments, and across mutants within one
            cs += [[(1 + E * m, 1.0), (E * m, -1.0)] for m in (3, 4)] + [[(1 + E * 10, 1.0), (1 + E * 3, -1.0)]]
        else:
            cs.append([(10 % G, 1.0), (3, -1.0)] if 10 % G != 3 else [(5 % G, 1.0), (3, -1.0)])
    for c in cs:
        assert len({k for k, _ in c}) == len(c) and all(0 <= k < n_space(space, sp) for k, _ in c)
    return cs


def golden_cases():
    """name -> (space, case, n_samples); the files are tests/golden/contrast_<case>_n<N>.npz, a space's arrays prefixed f_ / t_."""
    out = {f"{s}:{c}_n{n}": (s, c, n) for s, c in SPACE_CASES for n in NS}
    out.update({f"fitness:{k}": v for k, v in BIG.items()})
    return out


def golden_terms(name):
    space, case, n = golden_cases()[name]
    return contrast_set(space, case, big=n > max(NS))


def golden_path(name):
    return os.path.join(rc.GOLD, f"contrast_{name.split(':')[1]}.npz")


@functools.lru_cache(maxsize=None)
def golden(name):
    pre = name[0] + "_"
    with np.load(golden_path(name)) as f:
        g = {k[2:]: f[k] for k in f.files if k.startswith(pre)}
    for v in g.values():
        v.setflags(write=False)
    return g


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def elements(space, sp, D, n):
    """(s, m, sd) [n_space, n] and n_steps [n_space] of the space's elements."""
    if space == "fitness":
        return rc.conditionals(sp, D, n)
    th, m, sd, _, nst = tr.conditionals(sp, D, n)
    return th, m, sd, nst


@functools.lru_cache(maxsize=8)
def elements_at(space, case, n):
    sp, mu, om = inputs(case)
    with np.errstate(all="ignore"):
        out = elements(space, sp, sc.Draws(SEED, mu, pc.softplus(om), n), n)
    for v in out:
        v.setflags(write=False)
    return out


def nearest(x):
    """The multiple of 1 / GRID nearest to x."""
    return float(np.round(x * GRID) / GRID)


def compose(el, terms):
    """(d, M, sd) [n] and min_steps of one contrast from its space's elements: each sum from 0.0 in the caller's order."""
    s, m, sd, nst = el
    d, M, V = np.zeros(s.shape[1]), np.zeros(s.shape[1]), np.zeros(s.shape[1])
    for k, w in terms:
        ws = w * sd[k]
        d, M, V = d + w * s[k], M + w * m[k], V + ws * ws
    return d, M, np.sqrt(V), min(int(nst[k]) for k, _ in terms)


def restate(el, terms, threshold=None, probs=PROBS, unit=rc.unit64, want_z=False):
    """bb_contrast_rb for the contrasts `terms` from the elements `el`: a dict as Engine.contrast_rb returns, plus the thresholds
    used.  `threshold`: one for all, one per contrast, or None: per contrast the multiple of 1 / GRID nearest to
    the mean of its M_j."""
    with np.errstate(all="ignore"):
        parts = [compose(el, t) for t in terms]
        out = {k: np.empty(len(terms)) for k in UNITS}
        out["quantiles"] = np.empty((len(terms), len(probs)))
        out["min_steps"] = np.array([p[3] for p in parts], dtype=np.int32)
        near = np.array([nearest(p[1].mean()) if np.isfinite(p[1].mean()) else 0.0 for p in parts])
        s0 = np.broadcast_to(np.asarray(near if threshold is None else threshold, dtype=np.float64), (len(terms),))
        out["threshold"] = s0.copy()
        if want_z:
            out["zmax"] = np.array([np.abs((p[1] - s0[x]) / p[2]).max() for x, p in enumerate(parts)])
        for x, (d, M, sd, _) in enumerate(parts):
            vals, qs = unit(d, M, sd, float(s0[x]), probs)
            for k, v in zip(UNITS, vals):
                out[k][x] = float(v)
            out["quantiles"][x] = [float(q) for q in qs]
    return out


# ---- comparison -----------------------------------------------------------------------------------------------------------------
def as_rb(res):
    """A contrast result under the names `_rb_cases.errors` compares."""
    return {**{k: res[k] for k in UNITS + ("quantiles",)}, "n_steps": res["min_steps"]}


def errors(got, ref):
    return rc.errors(as_rb(got), as_rb(ref))


def assert_within(err, who):
    for k in UNITS:
        assert err[k] <= TOL, (who, k, err[k])
    assert err["quantiles"] <= QTOL, (who, "quantiles", err["quantiles"])


def report(name, label, err):
    print(f"contrast case {name:40s} {label:12s} " + " ".join(f"{k} {err[k] / 1e-16:7.1f}" for k in UNITS + ("quantiles",)) + "  (1e-16)")


def crb(e, terms, space, n, **kw):
    kw.setdefault("probs", PROBS)
    kw.setdefault("threshold", 0.0)
    kw.setdefault("seed", SEED)
    return e.contrast_rb(terms, space=space, n_samples=n, **kw)


def at_thresholds(e, terms, space, n, s0, **kw):
    """contrast_rb with contrast c's tails taken at s0[c]: one call per distinct threshold, of the contrasts that take it."""
    out = None
    for t in sorted(set(np.asarray(s0).tolist())):
        sel = np.flatnonzero(np.asarray(s0) == t)
        got = crb(e, [terms[i] for i in sel], space, n, threshold=t, **kw)
        if out is None:
            out = {k: np.full((len(terms),) + v.shape[1:], -7, dtype=v.dtype) for k, v in got.items()}
        for k in got:
            out[k][sel] = got[k]
    return out


def row(res, i):
    """Contrast i's results, as bytes."""
    return [np.ascontiguousarray(res[k][i]).tobytes() for k in OUTS]


# ---- 1. one-term contrasts against the goldens of the element calls ---------------------------------------------------------------
def single_term_cases():
    out = [("fitness", k) for k in sorted(rc.golden_cases())]
    return out + [("theta", k) for k in sorted(tr.golden_cases())]


def check_single_term(lib, space, name, label):
    """Every unit (group) as a one-term contrast of weight 1.0 against rb_<name>.npz (theta_rb_<name>.npz), at the files' own
    thresholds and under `_rb_cases`' (`_theta_rb_cases`') own bounds."""
    mod = rc if space == "fitness" else tr
    case, n, which = mod.golden_cases()[name]
    sp, mu, om = inputs(case)
    ref = dict(mod.golden(name))
    which = np.arange(n_space(space, sp)) if which is None else np.asarray(which)
    s0 = ref.pop("threshold") if space == "theta" else np.full(len(which), rc.THRESHOLD)
    ref.pop("n_members", None)
    with pc._handle(lib, sp, mu, om) as e:
        got = at_thresholds(e, [[(int(k), 1.0)] for k in which], space, n, s0)
    assert np.all(np.diff(got["quantiles"], axis=1) > 0)
    err = rc.errors(as_rb(got), ref)
    report(f"{space}:{name} one-term", label, err)
    mod.assert_within(err, label)


# ---- 2. composition at one explicit draw ------------------------------------------------------------------------------------------
def check_composition(lib, space, case):
    """At the three points of `check_identity`, each passed as one explicit draw: rb_mean = sum w m_k, rb_sd = sqrt(sum w^2 sd_k^2)
    and q_mean = sum w s_k with (s_k, m_k, sd_k) = (q_mean, rb_mean, rb_sd) of fitness_rb / theta_rb at the same draw, TOL relative
    to max(|x|, 1); q_sd = 0 and min_steps exactly.  Those calls are tied to the gradient of the log-joint by their own identity
    tests, so this ties the contrast to it."""
    sp = inputs(case)[0]
    terms = contrast_set(space, case)
    g = np.random.default_rng(8)
    with make_engine(sp, lib, seed=1) as e:
        for scale in (0.3, 1.0, 0.3):
            z = g.normal(0.0, scale, sp.D)
            got = e.contrast_rb(terms, space=space, probs=(), draws=z)
            base = (e.fitness_rb if space == "fitness" else e.theta_rb)(probs=(), draws=z)
            worst = 0.0
            for c, t in enumerate(terms):
                k, w = np.array([k for k, _ in t]), np.array([w for _, w in t])
                want = {"rb_mean": (w * base["rb_mean"][k]).sum(), "rb_sd": np.sqrt(((w * base["rb_sd"][k]) ** 2).sum()),
                        "q_mean": (w * base["q_mean"][k]).sum()}
                for name, x in want.items():
                    err = abs(got[name][c] - x) / max(abs(x), 1.0)
                    worst = max(worst, err)
                    assert err <= rc.TOL, (c, name, got[name][c], x)
                assert got["min_steps"][c] == base["n_steps"][k].min()
            assert np.all(got["q_sd"] == 0.0)
            print(f"contrast composition {space}:{case:28s} sd {scale}: {worst:.2e}")
    if case == "multienv_env0_only_first":                        # a contrast with a unit of environment 0 has a prior among its terms
        assert (got["min_steps"] == 0).any() and (got["min_steps"] > 0).any()


# ---- 3. golden values of multi-term mixtures ----------------------------------------------------------------------------------------
def check_golden(lib, name, label):
    space, case, n = golden_cases()[name]
    sp, mu, om = inputs(case)
    terms = golden_terms(name)
    ref = dict(golden(name))
    s0 = ref.pop("threshold")
    e0 = errors(restate(elements_at(space, case, n), terms, threshold=s0), ref)
    report(name, "restatement", e0)
    with pc._handle(lib, sp, mu, om) as e:
        got = at_thresholds(e, terms, space, n, s0)
    assert got["quantiles"].shape == (len(terms), len(PROBS)) and np.all(np.diff(got["quantiles"], axis=1) > 0)
    err = errors(got, ref)
    report(name, label, err)
    assert e0["quantiles"] <= Q_MEASURED and max(e0[k] for k in UNITS) <= MEASURED, "the restatement's own error exceeds what the bounds were derived from"
    assert_within(err, label)


def check_z_range(name):
    """Pins the |z| = |M_j - s0| / sd_j the cases reach (CPU, the restatement): with the thresholds on the grid every conditional
    stays within Z_HI = 20 of its sds, `_rb_cases`' limit; the hyper-fitness contrasts reach 6 at n >= 1000, the fitness contrasts
    stay below 4 (their deep tails are the one-term contrasts' at `_rb_cases.THRESHOLD`: |z| to 15)."""
    space, case, n = golden_cases()[name]
    ref = golden(name)
    z = restate(elements_at(space, case, n), golden_terms(name), threshold=ref["threshold"], probs=(), want_z=True)["zmax"]
    print(f"contrast z range {name}: {z.max():.2f}")
    assert z.max() <= Z_HI, z.max()
    assert z.max() >= 6.0 if space == "theta" and n >= 1000 else z.max() <= 12.0, z.max()


# ---- 4. the point of the feature ------------------------------------------------------------------------------------------------------
POINT = ([(10, 1.0), (3, -1.0)], [(17, 1.0), (10, -1.0)], [(10, 1.0), (3, 1.0)])


def point_inputs():
    """Case fitness, `_rb_cases.params` with the s_pop block's posterior sd at 0.3."""
    sp, mu, om = rc.inputs("fitness")
    om = om.copy()
    om[slice(*sp.offsets()["s_pop"])] = np.log(np.expm1(0.3))      # softplus^-1(0.3)
    return sp, mu, om


def point_ratios(res, own):
    return [float(res["rb_sd"][c] / np.sqrt(sum((w * own["rb_sd"][k]) ** 2 for k, w in t))) for c, t in enumerate(POINT)]


def check_point_restated():
    """The condition of `check_point` on the float64 restatement alone (CPU)."""
    sp, mu, om = point_inputs()
    el = elements("fitness", sp, sc.Draws(SEED, mu, pc.softplus(om), 1000), 1000)
    res = restate(el, POINT, probs=())
    own = restate(el, [[(u, 1.0)] for u in range(rc.n_units(sp))], probs=())
    r = point_ratios(res, own)
    print("contrast point, restatement: rb_sd / sqrt(sum of marginal variances) =", r)
    assert r[0] < 0.5 and r[1] < 0.5 and r[2] > 1.0, r
    return r


def check_point(lib):
    """A difference of two mutants of one replicate is far sharper than its two marginals say -- the population mean's uncertainty
    (posterior sd 0.3 here) is in both marginals and cancels in the difference: rb_sd / sqrt(rb_sd_a^2 + rb_sd_b^2) < 0.5 for
    s_10 - s_3 and s_17 - s_10 (the float64 restatement gives 0.325 and 0.324), the marginals from fitness_rb on the same handle at
    the same seed; and > 1 for the sum s_10 + s_3 (the restatement, `check_point_restated`: 1.376).  Measured in the emulation and
    on the MI355X: 0.3246, 0.3238, 1.3765."""
    sp, mu, om = point_inputs()
    with pc._handle(lib, sp, mu, om) as e:
        res = crb(e, list(POINT), "fitness", 1000, probs=())
        own = rc.rb(e, 1000, probs=())
    r = point_ratios(res, own)
    print("contrast point: rb_sd / sqrt(sum of marginal variances) =", r)
    assert r[0] < 0.5 and r[1] < 0.5, r
    assert r[2] > 1.0, r
    return r


# ---- 5. determinism ------------------------------------------------------------------------------------------------------------
def check_independent_of_the_other_contrasts(lib, space, case, n=111):
    """A contrast's bytes do not depend on the call's other contrasts, their number or their order; permuting the terms within a
    contrast moves the results by no more than TOL, and the same order twice gives the same bytes."""
    sp, mu, om = inputs(case)
    terms = contrast_set(space, case)
    perm = np.random.default_rng(3).permutation(len(terms))
    with pc._handle(lib, sp, mu, om) as e:
        base = crb(e, terms, space, n)
        again = crb(e, terms, space, n)
        shuffled = crb(e, [terms[i] for i in perm], space, n)
        more = crb(e, terms[::2] + terms, space, n)                # (a contrast may occur twice in a call)
        fewer = crb(e, terms[1::3], space, n)
        alone = [crb(e, [terms[i]], space, n) for i in (0, len(terms) - 1)]
        csr = crb(e, (np.cumsum([0] + [len(t) for t in terms]), [k for t in terms for k, _ in t], [w for t in terms for _, w in t]), space, n)
        flipped = crb(e, [t[::-1] for t in terms], space, n)
        flipped2 = crb(e, [t[::-1] for t in terms], space, n)
    assert rc.same_bytes(base, again) and rc.same_bytes(base, csr) and rc.same_bytes(flipped, flipped2)
    for x, i in enumerate(perm):
        assert row(shuffled, x) == row(base, i), i
    half = len(terms[::2])
    for i in range(len(terms)):
        assert row(more, half + i) == row(base, i), i
        assert i % 2 or row(more, i // 2) == row(base, i), i
    for x, i in enumerate(range(1, len(terms), 3)):
        assert row(fewer, x) == row(base, i), i
    assert row(alone[0], 0) == row(base, 0) and row(alone[1], 0) == row(base, len(terms) - 1)
    err = errors(flipped, base)
    report(f"{space}:{case}_n{n}", "terms flipped", err)
    for k in UNITS + ("quantiles",):
        assert err[k] <= rc.TOL, (k, err[k])


def check_launch_modes(lib, space="theta", case="replicate_ragged"):
    import barbay_jl_amd as bb
    sp, mu, om = inputs(case)
    terms = contrast_set(space, case)
    out = []
    for mode in (1, 0):
        with bb.Engine(sp.kind, sp.counts, sp.n_neutral, sp.n_bc, env_idx=sp.env_idx, geno_idx=sp.geno_idx, seed=4, launch_mode=mode, _lib=lib) as e:
            e.set_params(mu, om)
            out.append(crb(e, terms, space, 500, seed=2))
            out.append(crb(e, terms, space, 500, seed=2))
    assert all(rc.same_bytes(out[0], o) for o in out[1:])


def check_group_handle(lib, space, case):
    sp, mu, om = inputs(case)
    terms = contrast_set(space, case)
    with pc._handle(lib, sp, mu, om, device_ids=[0, 0]) as e:
        a = crb(e, terms, space, 111)
    with pc._handle(lib, sp, mu, om) as e:
        b = crb(e, terms, space, 111)
    assert rc.same_bytes(a, b)


def check_buffer_reuse(lib):
    """`_rb_cases.check_buffer_reuse` with the contrast call among the post-fit calls, at changing sizes and numbers of contrasts
    on one handle (the buffer regrows and is reused stale): every result is byte for byte what a fresh handle gives."""
    sp, mu, om = rc.inputs("fitness")
    om = np.minimum(om, -2.0)
    qs = (0.95, 0.675, 0.05)
    chain = np.random.default_rng(12).standard_normal((2, 5, 6))
    dr = rc.materialise(sp, mu, om, 7, 3)
    terms = contrast_set("fitness", "fitness")
    calls = [lambda e: crb(e, terms, "fitness", 111),
             lambda e: e.ppc_bands(qs, n_samples=111, n_ppc=7, seed=SEED),
             lambda e: crb(e, terms[:2], "fitness", 1000),
             lambda e: rc.rb(e, 111),
             lambda e: e.freq_bands(qs, mode="posterior", n_samples=200, n_ppc=1, seed=SEED),
             lambda e: crb(e, terms + terms, "fitness", 2),
             lambda e: e.chain_summary(chain),
             lambda e: e.ppc_score(n_samples=111, seed=SEED),
             lambda e: crb(e, terms[3:], "fitness", 7, draws=dr),
             lambda e: crb(e, terms[:1], "fitness", 2049, probs=(0.5,)),
             lambda e: e.popmean_rb(n_samples=64, seed=SEED),
             lambda e: crb(e, terms, "fitness", 111)]
    with pc._handle(lib, sp, mu, om) as e:
        got = [pc._bits(f(e)) for f in calls]
    for i, f in enumerate(calls):
        with pc._handle(lib, sp, mu, om) as e:
            assert got[i] == pc._bits(f(e)), i
    assert got[0] == got[-1]


def check_handle_untouched(lib):
    sp = rc.spec("fitness")
    terms = contrast_set("fitness", "fitness")
    with make_engine(sp, lib, seed=5) as a, make_engine(sp, lib, seed=5) as b:
        crb(b, terms, "fitness", 111)
        for x, y in zip(a.get_params(), b.get_params()):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
        a.run(5)
        crb(b, terms, "fitness", 64, seed=1)
        b.run(5)
        for x, y in zip(a.get_params(), b.get_params()):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64))


# ---- 6. non-finite values and errors ---------------------------------------------------------------------------------------------
def check_nan_parameter(lib, case="multienv", n=111):
    """One mutant's logsigma_bc means NaN: exactly the contrasts that name one of its units are NaN in rb_*, p_* and the quantiles
    (the draws' own contrast and min_steps are not); every other contrast keeps its bytes."""
    sp, mu, om = rc.inputs(case)
    E, m = rc.n_env(sp), 4
    terms = contrast_set("fitness", case)
    mu2 = mu.copy()
    lo = sp.offsets()["logsigma_bc"][0]
    mu2[lo + E * m:lo + E * (m + 1)] = np.nan
    with pc._handle(lib, sp, mu, om) as e:
        base = crb(e, terms, "fitness", n)
    with pc._handle(lib, sp, mu2, om) as e:
        got = crb(e, terms, "fitness", n)
    bad = [c for c, t in enumerate(terms) if any(E * m <= k < E * (m + 1) for k, _ in t)]
    assert 0 < len(bad) < len(terms)
    for c in range(len(terms)):
        if c not in bad:
            assert row(got, c) == row(base, c), c
            continue
        for k in ("rb_mean", "rb_sd", "p_pos", "p_neg", "quantiles"):
            assert np.all(np.isnan(got[k][c])), (c, k)
        for k in ("q_mean", "q_sd", "min_steps"):
            assert got[k][c].tobytes() == base[k][c].tobytes(), (c, k)


def raw(engine, terms, space=0, n_samples=64, probs=PROBS, threshold=0.0, seed=SEED, draws=None, null=(), want=OUTS, n_quantiles=None,
        n_contrasts=None, ptr=None, nout=None):
    """bb_contrast_rb through ctypes with only the outputs in `want` non-NULL; `null` names arguments passed as NULL (h, o, out,
    probs, term_ptr, term_idx, term_w); `ptr`, `n_contrasts`: in place of what `terms` gives."""
    tp = np.ascontiguousarray(np.cumsum([0] + [len(t) for t in terms]) if ptr is None else ptr, dtype=np.int64)
    ti = np.ascontiguousarray([k for t in terms for k, _ in t] + [0], dtype=np.int64)
    tw = np.ascontiguousarray([w for t in terms for _, w in t] + [0.0], dtype=np.float64)
    p = np.ascontiguousarray(probs, dtype=np.float64)
    nc = len(terms) if n_contrasts is None else n_contrasts
    o = _capi.bb_contrast_opts()
    o.space, o.n_samples, o.n_quantiles, o.threshold, o.seed, o.n_contrasts = space, n_samples, len(p) if n_quantiles is None else n_quantiles, threshold, seed, nc
    o.probs = None if "probs" in null or not len(p) else _capi._ptr(p)
    i64 = C.POINTER(C.c_int64)
    o.term_ptr = None if "term_ptr" in null else tp.ctypes.data_as(i64)
    o.term_idx = None if "term_idx" in null else ti.ctypes.data_as(i64)
    o.term_w = None if "term_w" in null else _capi._ptr(tw)
    if draws is not None:
        o.draws = _capi._ptr(draws)
    nout = max(nc, 0) if nout is None else nout
    res, out = {}, _capi.bb_contrast_out()
    for k in want:
        if k == "min_steps":
            res[k] = np.full(nout, -7, dtype=np.int32)
            out.min_steps = res[k].ctypes.data_as(C.POINTER(C.c_int32))
        else:
            res[k] = np.full((nout, len(p)) if k == "quantiles" else nout, -7.0)
            setattr(out, k, _capi._ptr(res[k]))
    rcode = engine._lib.bb_contrast_rb(None if "h" in null else engine._h, None if "o" in null else C.byref(o),
                                       None if "out" in null else C.byref(out))
    return rcode, res


def check_errors(lib):
    """Every BB_ERR_INVALID and BB_ERR_UNSUPPORTED of the contract, with a message that names the contrast and the term; an
    all-NULL out, each output alone, n_contrasts == 0.  NOT exercised: BB_ERR_DEVICE (see `_rb_cases.check_errors`), and the 2^31
    terms of BB_ERR_UNSUPPORTED as real arrays -- only through a term_ptr that claims them."""
    sp, mu, om = rc.inputs("fitness")
    INVALID, UNSUPPORTED = -1, _capi.BB_ERR_UNSUPPORTED
    msg = lambda: lib.bb_last_error().decode()
    terms = contrast_set("fitness", "fitness")
    nu = rc.n_units(sp)
    dr = rc.materialise(sp, mu, om, 3, 1)
    with pc._handle(lib, sp, mu, om) as e:
        for null in ("h", "o", "out"):
            assert raw(e, terms, null=(null,))[0] == INVALID and msg(), null
        for null in ("term_ptr", "term_idx", "term_w"):
            assert raw(e, terms, null=(null,))[0] == INVALID and "null" in msg(), null
        assert raw(e, terms, n_contrasts=-1)[0] == INVALID and "n_contrasts" in msg()
        assert raw(e, terms, space=2)[0] == INVALID and "space" in msg()
        assert raw(e, terms, space=-1)[0] == INVALID and "space" in msg()
        assert raw(e, terms, ptr=[1] + [2 * (i + 1) for i in range(len(terms))])[0] == INVALID and "term_ptr[0]" in msg()
        assert raw(e, terms[:3], ptr=[0, 2, 1, 3])[0] == INVALID and "contrast 1" in msg() and "decreases" in msg()
        assert raw(e, [terms[0], [], terms[1]])[0] == INVALID and "contrast 1" in msg() and "no terms" in msg()
        for bad in (-1, nu, 1 << 40):
            assert raw(e, [terms[0], [(3, 1.0), (bad, 1.0)]])[0] == INVALID and "contrast 1, term 1" in msg() and "outside" in msg(), bad
        assert raw(e, [terms[0], terms[1], [(3, 1.0), (5, 2.0), (3, -1.0)]])[0] == INVALID and "contrast 2, term 2" in msg() and "twice" in msg()
        for bad in (np.inf, -np.inf, np.nan):
            assert raw(e, [[(3, 1.0), (5, bad)]])[0] == INVALID and "contrast 0, term 1" in msg() and "weight" in msg(), bad
        for nq in (-1, 9):
            assert raw(e, terms, n_quantiles=nq)[0] == INVALID and "n_quantiles" in msg(), nq
        assert raw(e, terms, null=("probs",), n_quantiles=3)[0] == INVALID and "probs" in msg()
        for bad in (0.0, 1.0, -0.1, 1.5, np.nan):
            assert raw(e, terms, probs=(0.5, bad))[0] == INVALID and "prob" in msg(), bad
        for bad in (np.inf, -np.inf, np.nan):
            assert raw(e, terms, threshold=bad)[0] == INVALID and "threshold" in msg(), bad
        for n in (1, 0, -3, MAXN + 1):
            assert raw(e, terms, n_samples=n)[0] == UNSUPPORTED and "n_samples" in msg(), n
        for n in (0, MAXN + 1):
            assert raw(e, terms, n_samples=n, draws=dr)[0] == UNSUPPORTED and "n_samples" in msg(), n
        assert raw(e, terms, space=1)[0] == UNSUPPORTED and "BB_MODEL_FITNESS" in msg()
        assert raw(e, terms[:1], ptr=[0, 1 << 31], nout=1)[0] == UNSUPPORTED and "2^31" in msg()
        assert raw(e, terms, n_samples=1, draws=dr)[0] == 0 and raw(e, terms, n_samples=3, draws=dr)[0] == 0      # one explicit draw is served
        rcode, res = raw(e, terms, n_contrasts=0, nout=2)                                # nothing computed, nothing written
        assert rcode == 0 and all(np.all(v == -7) for v in res.values())
        assert raw(e, terms, n_contrasts=0, null=("term_ptr", "term_idx", "term_w"))[0] == 0
        assert raw(e, terms, want=())[0] == 0                                            # an all-NULL out
        assert raw(e, terms, probs=())[0] == 0                                           # no quantiles
        full = crb(e, terms, "fitness", 64)
        assert rc.same_bytes(raw(e, terms)[1], full)
        for k in OUTS:                                                                   # every output NULL except one
            rcode, one = raw(e, terms, want=(k,))
            assert rcode == 0 and rc.same_bytes(one, {k: full[k]}), k
        for bad, what in ((dict(n_samples=1), "n_samples"), (dict(draws=np.zeros((3, sp.D + 1))), "draws"), (dict(space="sbar"), "space")):
            try:
                e.contrast_rb(terms, **bad)
            except _capi.BarBayHipError as ex:
                assert what in str(ex)
            else:
                raise AssertionError("no error")
    sp, mu, om = inputs("genotype_regrouped")
    with pc._handle(lib, sp, mu, om) as e:                                               # the spaces have their own ranges
        G = tr.n_groups(sp)
        assert raw(e, [[(G, 1.0)]], space=1)[0] == INVALID and "group" in msg()
        assert raw(e, [[(G - 1, 1.0), (0, -1.0)]], space=1)[0] == 0 and raw(e, [[(G, 1.0)]], space=0)[0] == 0


# ---- 7. own draws against the same draws passed in -------------------------------------------------------------------------------
def check_internal_against_explicit_draws(lib, space, case, n=111):
    """`_rb_cases.check_internal_against_explicit_draws` for the contrasts: numpy's Box-Muller step and the library's differ by
    ulps, so the bounds of the goldens, not the bytes."""
    sp, mu, om = inputs(case)
    terms = contrast_set(space, case)
    dr = rc.materialise(sp, mu, om, n, SEED)
    with pc._handle(lib, sp, mu, om) as e:
        a = crb(e, terms, space, n)
        b = crb(e, terms, space, n, draws=dr)
        c = crb(e, terms, space, 5, draws=dr)                     # n_samples is the row count; the argument is ignored
    assert rc.same_bytes(b, c)
    err = errors(a, b)
    report(f"{space}:{case}_n{n}", "own/explicit", err)
    assert_within(err, "explicit draws")
