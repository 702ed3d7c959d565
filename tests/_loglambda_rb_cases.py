"""bb_loglambda_rb (Rao-Blackwellised loglambda marginals, barbay.jl_amd/csrc/bb_llrb.h) restated from the rule of
include/barbay_hip.h, and the cases the emulation and GPU tests share.  The draws, their keying and the normalisers are `_rb_cases`'.

The rule is written once (`setup`, `moments`, `cdf`) over a small arithmetic backend: `F64` (numpy float64 scalars: the restatement)
and `MP` (mpmath at 50 digits: the goldens, tests/golden/make_loglambda_rb_golden.py; mpmath is not needed to read them).  The
goldens evaluate the SAME rule on this restatement's float64 per-draw inputs (x0, f0, As, Bs, ws, wr, a, 1/b^2, R).

Shapes: the siblings' small specs with a few counts cut down (`low_counts`): per replicate one mutant read 0 times at t = 0, one
read once at t = 1, one read 3 times at its last time point, one whose whole trajectory is 0, 1, 3, 0, 1, .. and a neutral read 3
times at t = 1 -- the skewed end, next to barcodes read hundreds of times.  The rows of a call (`rows_of`) are those barcodes, the
first neutral and the last mutant of every replicate; every time point of a row is an entry, so t = 0 and t = T_r - 1 (one side)
are always among them, and `multienv_replicate` / `replicate_ragged` have the NaN cells of their shorter replicates.

Bounds, by `_rb_cases`' construction (relative to max(|x|, 1)): 1e-12 for the six moments; for the quantiles the larger of that and
8 x the float64 restatement's own measured error against the 50-digit bisection (Q_MEASURED).  n_reads, n_sides and the NaN
pattern are exact.  The quantiles have a 50-digit golden at n_samples = 2 (the entries `golden_cases` names); elsewhere the library
is compared with the float64 restatement at QTOL (one entry; at the sample cap its median).

The rule against the truth (`check_truth`): tests/golden/llrb_truth.npz holds, for per-draw inputs taken from the low-count entries
of the cases and further synthetic sets, `mpmath.quad` of exp(h) itself at 40 digits, split at every mode: ln Z_j, E, V and the CDF
at five points.  The ordinary sets (one mode, tables of ordinary size) are held to what bb_logsigma_rb's rule MEASURED on its own
cases (`LS_TRUTH`: ln Z 9.7e-16 absolute, E 4.0e-14 of the curvature scale, V 1.7e-15 relative, CDF 3.8e-6 absolute): the issue's
"no worse".  bb_logsigma_rb has no counterpart of the hard sets -- two kept modes (V is then the spread between the modes, summed
over a grid of 200 .. 350 nodes that spans both) and the two draws with tables of 1e7 (a curvature scale of 3e-4, coefficients
whose own rounding is 1e-9) -- and they are held to the bounds its rule is held to, `TRUTH_TOL` = 4e-12 and `TRUTH_CTOL` = 3e-5.

Measured, largest error over a case's entries against the golden, float64 restatement / host emulation / MI355X, in units of 1e-16
(each test prints its own line):

case                                         q_mean              q_sd           rb_mean             rb_sd       lambda_mean         mode_mean         quantiles
fitness_bimodal                     1.3/  1.3/  1.3   0.6/  0.6/  0.6   4.8/  4.8/  7.9  11.1/ 13.3/ 17.7   3.7/  3.7/  3.3   2.2/  2.2/  2.2   8.9/  8.9/ 66.3
fitness_chunk_n1000                   -/  2.2/  2.2     -/  0.0/  0.0     -/  0.6/  1.1     -/  0.6/  0.6     -/  1.8/  1.8     -/  0.6/  0.6     -/  0.0/  4.3
fitness_chunk_n111                  3.5/  1.8/  1.8   0.1/  0.1/  0.1   3.2/  1.6/  1.6   0.3/  0.3/  0.3   6.5/  4.6/  4.6   7.1/  4.2/  4.2   0.0/  0.0/  0.0
fitness_chunk_n2                    0.0/  0.0/  0.0   0.0/  0.0/  0.0   1.8/  1.8/  1.8   0.7/  1.4/  0.8   6.6/  6.1/  4.1   1.6/  1.9/  1.9   5.0/  5.0/  5.0
fitness_matrix_prior_n1000            -/  1.1/  1.1     -/  0.0/  0.0     -/  0.6/  0.6     -/  0.3/  0.3     -/  5.2/  5.2     -/  2.2/  2.2     -/  0.0/  0.0
fitness_matrix_prior_n111           4.2/  3.5/  3.5   0.0/  0.2/  0.2   6.2/  4.3/  4.3   0.3/  0.6/  0.6   7.7/  4.7/  4.7   1.5/  3.1/  3.1   0.0/  0.0/  0.0
fitness_matrix_prior_n2             0.0/  1.1/  1.1   0.0/  0.6/  0.6   2.0/  2.0/  2.0   1.1/  1.1/  1.1   5.4/  5.4/  5.4   3.0/  3.0/  2.0   7.6/  7.6/  3.4
fitness_n1000                         -/  1.1/  1.1     -/  0.1/  0.1     -/  0.1/  0.3     -/  0.0/  0.0     -/  2.2/  3.3     -/  0.3/  0.6     -/  8.9/  8.9
fitness_n111                        9.7/  2.2/  2.2   0.1/  0.1/  0.1   1.4/  1.4/  2.8   0.3/  0.6/  0.6   4.4/  4.4/  2.2   1.4/  4.1/  4.1   0.0/  0.0/  0.0
fitness_n2                          0.0/  0.0/  0.0   0.0/  0.0/  0.0   2.2/  2.2/  1.4   0.7/  0.8/  0.7   5.1/  4.9/  5.6   2.1/  2.1/  2.1   5.6/  5.6/  6.3
fitness_tiny_n5781                    -/    -/  0.0     -/    -/  0.0     -/    -/  1.1     -/    -/  0.0     -/    -/  1.1     -/    -/  3.3     -/    -/  0.0
genotype_matrix_prior_n1000           -/  1.1/  1.1     -/  0.0/  0.0     -/  0.6/  0.6     -/  0.3/  0.6     -/  3.3/  3.3     -/  0.1/  0.1     -/  0.0/  0.0
genotype_matrix_prior_n111          3.5/  3.5/  3.5   0.1/  0.1/  0.1   5.5/  4.9/  4.9   0.6/  0.3/  0.3   3.1/  3.9/  2.0   1.7/  3.3/  4.9   0.0/  0.0/  0.0
genotype_matrix_prior_n2            0.0/  0.0/  0.0   0.0/  2.2/  2.2   2.0/  8.5/  8.3   1.7/ 10.5/ 10.5   5.4/ 11.9/ 10.6   1.3/  8.3/  8.9   4.9/  3.6/  3.6
genotype_regrouped_n1000              -/  1.1/  1.1     -/  0.0/  0.0     -/  0.1/  0.1     -/  0.6/  0.6     -/  2.0/  4.0     -/  0.0/  0.1     -/  0.0/  0.0
genotype_regrouped_n111             3.5/  3.5/  3.5   0.1/  0.1/  0.1   8.2/  1.8/  1.8   0.6/  0.6/  0.3   7.6/  5.3/  6.1   3.6/  1.8/  1.8   0.0/  0.0/  0.0
genotype_regrouped_n2               0.0/  0.0/  0.0   0.0/  2.2/  2.2   2.1/  8.3/  8.0   2.5/  9.2/ 13.0   5.2/ 11.7/ 10.8   2.0/  8.6/  8.3   4.8/  4.8/  4.8
multienv_n1000                        -/  1.7/  1.7     -/  0.0/  0.0     -/  1.1/  1.1     -/  0.3/  0.3     -/  2.2/  2.2     -/  0.0/  0.0     -/  0.0/  0.0
multienv_n111                       3.5/  1.8/  1.8   0.1/  0.1/  0.1   3.6/  2.6/  2.6   0.3/  0.3/  0.3   5.3/  2.2/  1.6   5.6/  6.4/  6.4   0.0/  0.0/  0.0
multienv_n2                         0.0/  0.0/  0.0   0.0/  4.4/  4.4   2.0/  2.0/  2.0   0.8/  1.2/  2.2   7.4/  7.0/  8.1   2.2/  2.2/  2.0   4.4/  4.4/  4.4
multienv_replicate_n1000              -/  1.1/  1.1     -/  0.1/  0.1     -/  1.8/  1.8     -/  0.0/  0.0     -/  1.1/  0.0     -/  1.8/  3.6     -/  0.0/  0.0
multienv_replicate_n111             3.3/  5.3/  5.3   0.1/  0.1/  0.1   5.0/  5.0/  5.0   0.6/  0.6/  0.3   6.2/  3.4/  2.3   3.7/  4.4/  5.6   0.0/  0.0/  0.0
multienv_replicate_n2               0.0/  1.8/  1.8   0.0/  4.4/  4.4   1.7/  3.7/  2.2   1.9/  2.1/  2.1   7.4/  8.1/  8.3   2.0/  3.7/  2.0   5.3/  5.3/  5.3
replicate_ragged_method_n1000         -/  1.7/  1.7     -/  0.0/  0.0     -/  2.2/  2.8     -/  0.0/  0.0     -/  2.2/  2.2     -/  1.1/  1.1     -/  0.0/  0.0
replicate_ragged_method_n111        5.6/  8.8/  8.8   0.2/  0.0/  0.0   3.3/  3.4/  3.4   0.3/  0.6/  0.6   4.5/  2.9/  2.9   6.7/  2.3/  2.3   0.0/  0.0/  0.0
replicate_ragged_method_n2          0.0/  1.1/  1.1   0.0/  0.6/  0.6   2.1/  2.1/  2.2   2.2/  2.2/  1.9   7.3/  8.3/  8.0   2.1/  2.0/  2.2   4.3/  4.3/  4.3
replicate_ragged_n1000                -/  1.7/  1.7     -/  0.0/  0.0     -/  1.1/  1.1     -/  0.6/  0.6     -/  2.2/  2.2     -/  2.2/  4.4     -/  0.0/  0.0
replicate_ragged_n111               5.6/  8.8/  8.8   0.2/  0.0/  0.0   7.8/  3.9/  3.9   0.3/  0.3/  0.3   4.4/  2.2/  2.2   3.3/  2.0/  2.4   0.0/  0.0/  0.0
replicate_ragged_n2                 0.0/  1.1/  1.1   0.0/  0.6/  0.6   2.2/  2.2/  2.2   1.9/  1.9/  1.9   9.6/  9.6/  6.7   2.2/  2.2/  2.2   4.3/  4.3/  4.3
(largest entry: restatement 11.1e-16, emulation 13.3e-16, MI355X 66.3e-16; the bound is 1e-12 = 10000e-16.  '-': the restatement is not run whole at n = 1000 and above; the emulation does not run the cap.  The quantile column of the n = 111 and n = 1000 cases is one entry against the float64 restatement, that of the cap the median of one entry against it; fitness_bimodal: the two-mode draws of `check_bimodal`)

The rule against `mpmath.quad` of exp(h), 79 sets.  The 73 ordinary ones (the low-count entries of three cases among them):
ln Z_j 6.7e-16, E 3.2e-15 of the curvature scale, V 9.3e-16, CDF 2.8e-6 -- against bb_logsigma_rb's measured 9.7e-16, 4.0e-14, 1.7e-15, 3.8e-6, the bound.  The 6 hard ones (4 with two kept
modes, sets 75 .. 78 of `truth_sets`, the grid covers both modes of each; 2 draws with tables of 1e7, on which the first bracket
failed on the device): ln Z_j 8.0e-15, E 2.7e-14, V 3.5e-14, CDF 2.8e-6 -- bounds 4e-12 / 3e-5.  The library itself is run on two-mode draws by `check_bimodal`.
"""
import ctypes as C
import functools
import math
import os

import numpy as np

import _ppc_cases as pc
import _rb_cases as rc
import _score_cases as sc
from conftest import make_engine
from barbay_jl_amd import _capi
from oracle import fixtures
from oracle.spec import ModelSpec

UNITS = _capi.LL_UNITS
MAXN = _capi.BB_LOGLAMBDA_RB_MAX_SAMPLES
SEED, PROBS, NS, HIER, GOLD = rc.SEED, rc.PROBS, rc.NS, rc.HIER, rc.GOLD
TOL = 1e-12
MEASURED = 1.1e-15        # the float64 restatement's largest error of the six moments against the goldens (make_loglambda_rb_golden.py --measure)
Q_MEASURED = 8.9e-16      # the float64 restatement's largest quantile error against the 50-digit bisection (make_loglambda_rb_golden.py --measure)
QTOL = max(1e-12, 8.0 * Q_MEASURED)
ITER, TAIL, REACH, REACH_MAX, REFINE_MAX, NODES_MAX = 40, -40.0, 8, 4096, 64, 8192
MODE_ITER, SCAN_MIN, SCAN_MAX, PAD, SLACK, LOW_ITER = 100, 16, 1024, 0.125, 2.0 ** -20, 30
TRUTH_TOL, TRUTH_CTOL = 4e-12, 3e-5      # == _logsigma_rb_cases.TRUTH_TOL / TRUTH_CTOL: what bb_logsigma_rb's rule is held to
LS_TRUTH = dict(lnZ=9.7e-16, E=4.0e-14, V=1.7e-15, C=3.8e-6)      # what bb_logsigma_rb's rule measured on its own cases (_logsigma_rb_cases, bb_lsrb's commit)
TRUTH_AT = (-2.3, -0.7, 0.11, 1.9, 4.4)

SHAPES = ("fitness", "fitness_chunk", "multienv", "genotype_regrouped", "replicate_ragged", "replicate_ragged_method",
          "multienv_replicate", "fitness_matrix_prior", "genotype_matrix_prior")
TINY = "fitness_tiny"
BIMODAL = "fitness_bimodal"


def quirk_of(case):
    return case == "replicate_ragged_method"


def uses_priors(case):
    return case.endswith("matrix_prior")


def low_counts(sp, priors=None):
    """`sp` with the counts of a few barcodes cut down (the module docstring)."""
    nn, counts = sp.n_neutral, []
    for c in sp.counts:
        c = np.array(c, dtype=np.int64)
        T = c.shape[0]
        c[0, nn + 1] = 0
        c[1, nn + 2] = 1
        c[T - 1, nn + 3] = 3
        c[:, nn + 4] = np.array([0, 1, 3] * T)[:T]
        c[1, 0] = 3
        counts.append(c)
    return ModelSpec(kind=sp.kind, counts=counts, totals=[c.sum(axis=1) for c in counts], n_neutral=sp.n_neutral, n_bc=sp.n_bc,
                     env_idx=sp.env_idx, geno_idx=sp.geno_idx, priors=dict(sp.priors) if priors is None else priors)


@functools.lru_cache(maxsize=None)
def spec(case):
    if case in pc.CASES:
        return low_counts(pc.spec(case))
    if case == "replicate_ragged_method":
        return low_counts(pc.spec("replicate_ragged"))
    if case == "fitness_chunk":                                   # B = 300 crosses the 256-column chunk; T = 3: t = 1 has both sides
        return low_counts(rc.spec(case))
    if case == TINY:
        return low_counts(fixtures.synthetic("fitness", B=12, T=4, n_neutral=3, seed=3))
    if case == BIMODAL:                                           # a mutant with no read at t = 1 (`bimodal_draws`)
        sp = spec(TINY)
        counts = [np.array(c) for c in sp.counts]
        counts[0][1, sp.n_neutral + 6] = 0
        return ModelSpec(kind=sp.kind, counts=counts, totals=[c.sum(axis=1) for c in counts], n_neutral=sp.n_neutral, n_bc=sp.n_bc)
    if case == "genotype_matrix_prior":                           # ... on a handle that regroups its mutants: the prior follows its latent
        sp, g = spec("genotype_regrouped"), np.random.default_rng(4)
        n = sp.B * sp.n_time[0]
        return ModelSpec(kind=sp.kind, counts=sp.counts, totals=sp.totals, n_neutral=sp.n_neutral, n_bc=sp.n_bc, geno_idx=sp.geno_idx,
                         priors=dict(loglambda_prior=(g.normal(3.0, 1.0, n), g.uniform(0.5, 3.0, n))))
    if case == "fitness_matrix_prior":                            # Matrix form of the loglambda prior
        sp, g = fixtures.synthetic("fitness", B=30, T=4, n_neutral=5, seed=3), np.random.default_rng(2)
        return low_counts(sp, priors=dict(loglambda_prior=(g.normal(3.0, 1.0, 120), g.uniform(0.5, 3.0, 120))))
    raise KeyError(case)


def rows_of(case):
    sp = spec(case)
    nn, B = sp.n_neutral, sp.B
    return [r * B + b for r in range(sp.n_rep) for b in (0, nn + 1, nn + 2, nn + 3, nn + 4, B - 1)]


def golden_cases():
    """name -> (case, n_samples, rows of the call, entries (x, t) of it with a 50-digit golden of the moments or None for all,
    entries with a 50-digit golden of the quantiles).  A 50-digit evaluation costs about 50 ms a draw, so the calls of many draws
    have a golden for a few entries (always a low-count one, a one-sided and a two-sided one) and the cap for one."""
    out = {}
    for c in SHAPES:
        rows = rows_of(c)
        T0 = spec(c).n_time[0]
        out[f"{c}_n2"] = (c, 2, tuple(rows), None, ((3, 0), (4, 1), (4, 2), (0, 1), (5, T0 - 1)))
        out[f"{c}_n111"] = (c, 111, (rows[0], rows[4], rows[-1]), ((0, 1), (1, 0), (1, 1), (1, 2), (2, spec(c).n_time[-1] - 1)), ())
        out[f"{c}_n1000"] = (c, 1000, (rows[4],), ((0, 0), (0, 1)), ())
    nn = spec(TINY).n_neutral
    out[f"{TINY}_n{MAXN}"] = (TINY, MAXN, (0, nn + 2, nn + 4), ((2, 1),), ())
    return out


def emu_cases():
    return sorted(k for k, v in golden_cases().items() if v[1] <= 1000)


def golden_path(name):
    return os.path.join(GOLD, f"llrb_{name}.npz")


@functools.lru_cache(maxsize=None)
def inputs(case):
    sp = spec(case)
    mu, om = rc.params(sp)
    mu.setflags(write=False)
    om.setflags(write=False)
    return sp, mu, om


def engine(lib, case, mu=None, om=None, **kw):
    if quirk_of(case):
        kw["ragged_method"] = True
    if uses_priors(case):
        kw["use_priors"] = True
    if mu is None:
        return make_engine(spec(case), lib, **kw)
    return pc._handle(lib, spec(case), mu, om, **kw)


def ll(e, n, **kw):
    kw.setdefault("probs", PROBS)
    kw.setdefault("seed", SEED)
    return e.loglambda_rb(n_samples=n, **kw)


# ---- the restatement: per-draw inputs ------------------------------------------------------------------------------------------
def _tables(sp, D, n, r, lo_l, g0, quirk, ks):
    """ln Z_t [T][n], and for the steps `ks` of replicate r: (A_k, B_k) and the per-barcode (w, rho) function."""
    off = sp.offsets()
    B, nb, nn = sp.B, sp.n_bc, sp.n_neutral
    E, hier, T = rc.n_env(sp), sp.kind in HIER, sp.n_time[r]
    lam = lambda b, t: D(lo_l + b * T + t)
    logZ = []
    for t in range(T):                                            # chunks of 256 columns in index order, then the chunks in order
        Z = None
        for b0 in range(0, B, 256):
            part = np.zeros(n)
            for b in range(b0, min(b0 + 256, B)):
                part = part + np.exp(lam(b, t))
            Z = part if Z is None else Z + part
        logZ.append(np.log(Z))

    def wrho(i, k):
        gam = (lam(i, k + 1) - lam(i, k)) - (logZ[k + 1] - logZ[k])
        if i < nn:
            g = g0 + ((i * (T - 1) + k) // nn if quirk else k)
            return np.exp(-2.0 * D(off["logsigma_pop"][0] + g)), gam + D(off["s_pop"][0] + g)
        m, e = i - nn, rc.env_of(sp, r, k)
        em = e + E * m
        u = em + E * nb * r
        if not hier:
            s, ls = D(off["s_bc"][0] + em), D(off["logsigma_bc"][0] + em)
        else:
            th = int(sp.geno_idx[m]) if sp.kind == "genotype" else em
            uu = m if sp.kind == "genotype" else u
            s = D(off["theta"][0] + th) + np.exp(D(off["logtau"][0] + uu)) * D(off["theta_tilde"][0] + uu)
            ls = D(off["logsigma_bc"][0] + uu)
        return np.exp(-2.0 * ls), (gam + D(off["s_pop"][0] + g0 + k)) - s

    AB = {}
    for k in ks:
        SA = SB = None
        for i0 in range(0, B, 256):
            pa, pb = np.zeros(n), np.zeros(n)
            for i in range(i0, min(i0 + 256, B)):
                w, rho = wrho(i, k)
                pa, pb = pa + w, pb + w * rho
            SA, SB = (pa, pb) if SA is None else (SA + pa, SB + pb)
        AB[k] = (SA, SB)
    return logZ, AB, wrho


def cond_inputs(sp, D, n, rows, quirk=False):
    """{(x, t): dict(x0, f0, As, Bs, ws, wr [n]; a, ib2, R)} for the rows[x] (bb_freq_bands rows) from the draws D(i) -> [n] of the
    caller's latents: the header's formulas."""
    off = sp.offsets()
    B = sp.B
    pm, ps = sp.prior_arrays()
    out = {}
    with np.errstate(all="ignore"):
        lo_l, g0 = off["loglambda"][0], 0
        for r in range(sp.n_rep):
            T = sp.n_time[r]
            mine = [(x, row % B) for x, row in enumerate(rows) if row // B == r]
            if mine:
                logZ, AB, wrho = _tables(sp, D, n, r, lo_l, g0, quirk, range(T - 1))
                for x, b in mine:
                    for t in range(T):
                        i = lo_l + b * T + t
                        x0 = D(i)
                        As, Bs, ws, wr = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
                        if t + 1 < T:
                            w, rho = wrho(b, t)
                            As, Bs, ws, wr = AB[t][0], AB[t][1], w, w * rho
                        if t >= 1:
                            w, rho = wrho(b, t - 1)
                            As, Bs, ws, wr = As + AB[t - 1][0], Bs - AB[t - 1][1], ws + w, wr - w * rho
                        out[(x, t)] = dict(x0=x0, f0=np.exp(x0 - logZ[t]), As=As, Bs=Bs, ws=ws, wr=wr, a=float(pm[i]),
                                           ib2=1.0 / (float(ps[i]) * float(ps[i])), R=float(sp.counts[r][t, b]))
            lo_l += T * B
            g0 += T - 1
    return out


# ---- the rule, over an arithmetic backend --------------------------------------------------------------------------------------
class F64:
    """numpy float64 scalars: IEEE results for overflow and NaN, no exceptions."""
    num = staticmethod(np.float64)
    exp, expm1, log, log1p, sqrt, ceil = (staticmethod(f) for f in (np.exp, np.expm1, np.log, np.log1p, np.sqrt, np.ceil))
    inf = np.float64(np.inf)
    isfinite = staticmethod(lambda x: bool(np.isfinite(x)))


class PY:
    """Python floats and libm: the same IEEE doubles as `F64` to an ulp of the library functions, ten times as fast; an overflow
    raises, so it serves only where none can occur (the check at the sample cap)."""
    num = staticmethod(float)
    exp, expm1, log, log1p, sqrt, ceil = (staticmethod(f) for f in (math.exp, math.expm1, math.log, math.log1p, math.sqrt, math.ceil))
    inf = math.inf
    isfinite = staticmethod(math.isfinite)


class Cond:
    """The conditional of one draw about a base point: the header's folded form."""
    __slots__ = ("M", "a", "ib2", "R", "As", "ws", "x", "ex", "f0", "Bs", "wr")

    def __init__(self, M, a, ib2, R, As, ws, x, f0, Bs, wr):
        n = M.num
        self.M, self.a, self.ib2, self.R, self.As, self.ws = M, n(a), n(ib2), n(R), n(As), n(ws)
        self.x, self.f0, self.Bs, self.wr = n(x), n(f0), n(Bs), n(wr)
        self.ex = M.exp(self.x)

    def df(self, u):
        e = self.M.expm1(u)
        y = self.f0 * e
        return e, self.M.log1p(y), self.f0 * (e + 1) / (1 + y)

    def lnp(self, u):
        e, dl, f = self.df(u)
        return (-(self.ib2 / 2) * (u * (u + 2 * (self.x - self.a))) + self.R * u - self.ex * e - self.Bs * dl - (self.As / 2) * (dl * dl)
                - (self.ws / 2) * (u * u) + u * self.wr + self.ws * (u * dl)), e

    def d12(self, u):
        e, dl, f = self.df(u)
        ff, eu = f * (1 - f), self.ex * (e + 1)
        g = -self.ib2 * (u + (self.x - self.a)) + self.R - eu - (self.Bs + self.As * dl) * f - self.ws * u + self.wr + self.ws * (dl + u * f)
        cv = -self.ib2 - eu - self.Bs * ff - self.As * (f * f + dl * ff) - self.ws + self.ws * (2 * f + u * ff)
        return g, cv

    def anchored(self, u):
        e, dl, f = self.df(u)
        return Cond(self.M, self.a, self.ib2, self.R, self.As, self.ws, self.x + u, f, self.Bs + self.As * dl - self.ws * u,
                    self.wr + self.ws * (dl - u))

    def bracket(self):
        M = self.M
        d0 = self.x - self.a
        Bp, Bm = (self.Bs if self.Bs > 0 else M.num(0)), (-self.Bs if self.Bs < 0 else M.num(0))
        C0 = -self.ib2 * d0 + self.R + self.wr + self.ws * M.log1p(-self.f0)
        sl = self.ib2 + self.ws * (1 - self.f0)

        def low(L):
            e = M.expm1(L)
            return (C0 - self.ex * (e + 1) - Bp * (self.f0 * (e + 1) / (1 + self.f0 * e))) / sl - L
        lo = low(M.num(0))
        if lo < 0:
            up = M.num(0)
            for _ in range(LOW_ITER):
                mid = lo + (up - lo) / 2
                if low(mid) >= 0:
                    lo = mid
                else:
                    up = mid
        elif lo == lo:
            lo = M.num(0)
        K = self.R + Bm + self.wr - self.ib2 * d0
        hi = M.num(0)
        if K > 0:
            hi = min(K / self.ib2, M.log(K / self.ex))
            hi = hi if hi > 0 else M.num(0)
        elif K != K:
            hi = K
        return lo - M.num(PAD), hi + M.num(PAD)

    def solve(self, lo, hi, x):
        for _ in range(MODE_ITER):
            g, cv = self.d12(x)
            if g == 0 or g != g:
                return x + g
            if g > 0:
                lo = x
            else:
                hi = x
            xn = x - g / cv
            if not (cv < 0 and lo <= xn <= hi):
                xn = lo + (hi - lo) / 2
            step, x = xn - x, xn
            if abs(step) <= self.M.num(2.0 ** -40) * (1 + abs(x)):
                break
        g, cv = self.d12(x)
        xn = x - g / cv
        return xn if (cv < 0 and lo <= xn <= hi) else x


def _count(M, x):
    return int(M.ceil(x - M.num(SLACK))) if 1 <= x <= 1e9 else 1


def setup(c):
    """(c about the global mode, s, nleft, nright, the kept modes as offsets from x0): the header's mode search and grid."""
    M = c.M
    blo, bhi = c.bracket()
    width = bhi - blo
    modes, kept, gbest = [], [], None
    g0 = c.d12(blo)[0]
    if width != width or g0 != g0:                                # a NaN bracket or g': the mode is NaN
        best = width + g0
    else:
        w8 = width * 8
        nc = SCAN_MIN if not (w8 > SCAN_MIN) else (int(M.ceil(w8)) if w8 < SCAN_MAX else SCAN_MAX)
        cw = width / nc
        edges = [blo + i * cw for i in range(nc)] + [bhi]
        gs = [g0] + [c.d12(e)[0] for e in edges[1:]]
        for i in range(nc):
            if gs[i] > 0 and not (gs[i + 1] > 0):
                m = c.solve(edges[i], edges[i + 1], edges[i] + (edges[i + 1] - edges[i]) / 2)
                modes.append((m, c.lnp(m)[0]))
        if not modes:                                             # no sign change: rounding at an end of the bracket
            best = bhi if g0 > 0 else blo
        else:
            best, gbest = modes[0]
            for m, v in modes[1:]:
                if v > gbest or v != v:
                    best, gbest = m, v
            kept = [(m, 1 / M.sqrt(-c.d12(m)[1])) for m, v in modes if gbest - v <= -TAIL]
    if kept:
        dmin = M.inf
        for _, d in kept:
            if d < dmin:
                dmin = d
    else:
        dmin = 1 / M.sqrt(-c.d12(best)[1])
        kept = [(best, dmin)]
    left, dl0 = kept[0][0] - best, kept[0][1]
    right, dl1 = kept[-1][0] - best, kept[-1][1]
    ca = c.anchored(best)
    m = M.ceil(2 * dmin - M.num(SLACK)) if M.isfinite(dmin) else 1
    m = (m if m <= REFINE_MAX else REFINE_MAX) if m >= 1 else 1
    s = dmin / (4 * m)
    r = 1
    while r < REACH_MAX and ca.lnp(left - (REACH * r) * dl0)[0] > TAIL:
        r *= 2
    e0 = left - (REACH * r) * dl0
    r = 1
    while r < REACH_MAX and ca.lnp(right + (REACH * r) * dl1)[0] > TAIL:
        r *= 2
    e1 = right + (REACH * r) * dl1
    nl, nr = _count(M, -e0 / s), _count(M, e1 / s)
    f = (nl + nr + NODES_MAX - 1) // NODES_MAX
    return ca, s * f, (nl + f - 1) // f, (nr + f - 1) // f, [m for m, _ in kept]


def moments(ca, s, nleft, nright):
    """(Z, E, V, Lam) of one draw on its grid."""
    M = ca.M
    z = m1 = m2 = se = M.num(0)
    nodes = nleft + nright
    for k in range(nodes + 1):
        u = (k - nleft) * s
        v, e = ca.lnp(u)
        p = M.exp(v)
        if k == 0 or k == nodes:
            p = p / 2
        z, m1, m2, se = z + p, m1 + p * u, m2 + p * (u * u), se + p * (e + 1)
    r1 = m1 / z
    return s * z, ca.x + r1, m2 / z - r1 * r1, ca.ex * (se / z)


def cdf_z(ca, s, lo, x):
    """Z_j C_j(x), lo < x < hi: the re-spaced trapezoid less the Euler-Maclaurin end term."""
    M = ca.M
    r, ulo = x - lo, lo - ca.x
    N = M.ceil(r / s)
    N = int(N) if N >= 1 else 1
    sx = r / N
    ux = x - ca.x
    p0, p1 = M.exp(ca.lnp(ulo)[0]), M.exp(ca.lnp(ux)[0])
    acc = p0 / 2
    for i in range(1, N):
        acc = acc + M.exp(ca.lnp(ulo + i * sx)[0])
    acc = acc + p1 / 2
    return sx * acc - sx * sx / 12 * (ca.d12(ux)[0] * p1 - ca.d12(ulo)[0] * p0)


class Entry:
    """One entry's draws worked by the rule: per-draw anchored conditionals, grids and moments."""

    def __init__(self, inp, M=F64):
        n = len(inp["x0"])
        self.M, self.n, self.x0 = M, n, [M.num(v) for v in inp["x0"]]
        self.c, self.s, self.lo, self.hi, self.Z, self.E, self.V, self.L, self.modes = [], [], [], [], [], [], [], [], []
        with np.errstate(all="ignore"):
            for j in range(n):
                c0 = Cond(M, inp["a"], inp["ib2"], inp["R"], inp["As"][j], inp["ws"][j], inp["x0"][j], inp["f0"][j], inp["Bs"][j], inp["wr"][j])
                ca, s, nl, nr, modes = setup(c0)
                Z, E, V, L = moments(ca, s, nl, nr)
                self.c.append(ca); self.s.append(s); self.lo.append(ca.x - nl * s); self.hi.append(ca.x + nr * s)
                self.Z.append(Z); self.E.append(E); self.V.append(V); self.L.append(L); self.modes.append(modes)

    def units(self):
        M, n = self.M, self.n
        tot = lambda v: sum(v[1:], v[0])
        qm, rm = tot(self.x0) / n, tot(self.E) / n
        return [qm, M.sqrt(tot([(v - qm) ** 2 for v in self.x0]) / n), rm,
                M.sqrt(tot(self.V) / n + tot([(v - rm) ** 2 for v in self.E]) / n), tot(self.L) / n, tot([c.x for c in self.c]) / n]

    def mixture(self, x):
        if self.M in (F64, PY):
            return self._mixture64(float(x))
        acc = self.M.num(0)
        for j in range(self.n):
            if x <= self.lo[j]:
                continue
            if x >= self.hi[j]:
                acc = acc + 1
                continue
            C = cdf_z(self.c[j], self.s[j], self.lo[j], x) / self.Z[j]
            acc = acc + (0 if C < 0 else (1 if C > 1 else C))
        return acc / self.n

    def _mixture64(self, x):
        """`mixture` in float64, the draws in play side by side (each draw's own sums in its own order, as `cdf_z`); the sum over
        the draws in index order."""
        if not hasattr(self, "_v"):
            f = lambda k: np.array([float(getattr(c, k)) for c in self.c])
            self._v = {k: f(k) for k in ("a", "ib2", "R", "As", "ws", "x", "ex", "f0", "Bs", "wr")}
            self._v.update(s=np.array(self.s, dtype=np.float64), lo=np.array(self.lo, dtype=np.float64), hi=np.array(self.hi, dtype=np.float64),
                           Z=np.array(self.Z, dtype=np.float64))
        v = self._v
        C = np.where(x >= v["hi"], 1.0, 0.0)
        on = np.flatnonzero((x > v["lo"]) & (x < v["hi"]))
        if len(on):
            P = {k: a[on] for k, a in v.items()}

            def lnp_d1(u):
                e = np.expm1(u)
                y = P["f0"] * e
                dl, f = np.log1p(y), P["f0"] * (e + 1) / (1 + y)
                g = (-(P["ib2"] / 2) * (u * (u + 2 * (P["x"] - P["a"]))) + P["R"] * u - P["ex"] * e - P["Bs"] * dl - (P["As"] / 2) * (dl * dl)
                     - (P["ws"] / 2) * (u * u) + u * P["wr"] + P["ws"] * (u * dl))
                d = (-P["ib2"] * (u + (P["x"] - P["a"])) + P["R"] - P["ex"] * (e + 1) - (P["Bs"] + P["As"] * dl) * f - P["ws"] * u + P["wr"]
                     + P["ws"] * (dl + u * f))
                return g, d
            r, ulo = x - P["lo"], P["lo"] - P["x"]
            N = np.maximum(np.ceil(r / P["s"]), 1.0)
            sx, ux = r / N, x - P["x"]
            g0, d0 = lnp_d1(ulo)
            g1, d1 = lnp_d1(ux)
            p0, p1 = np.exp(g0), np.exp(g1)
            acc = p0 / 2
            for i in range(1, int(N.max())):
                acc = acc + np.where(i < N, np.exp(lnp_d1(ulo + i * sx)[0]), 0.0)
            acc = acc + p1 / 2
            C[on] = np.clip((sx * acc - sx * sx / 12 * (d1 * p1 - d0 * p0)) / P["Z"], 0.0, 1.0)
        tot = np.float64(0.0)
        for c in C:
            tot = tot + c
        return tot / self.n

    def quantiles(self, probs):
        M = self.M
        finite = all(M.isfinite(v) for v in self.Z) and all(M.isfinite(v) for v in self.lo) and all(M.isfinite(v) for v in self.hi)
        if not finite:
            return [float("nan")] * len(probs)
        out = []
        with np.errstate(all="ignore"):
            for p in probs:
                lo, hi = min(self.lo), max(self.hi)
                for _ in range(ITER):
                    x = lo + (hi - lo) / 2
                    if self.mixture(x) < p:
                        lo = x
                    else:
                        hi = x
                out.append(lo + (hi - lo) / 2)
        return out


def draws_of(sp, mu, om, n, seed, draws=None):
    return rc.Rows(draws) if draws is not None else sc.Draws(seed, mu, pc.softplus(om), n)


def restate(case, mu, om, n, seed, rows, probs=PROBS, draws=None, M=F64, entries=None, qentries=None, inputs_only=False):
    """bb_loglambda_rb for `rows`: a dict as Engine.loglambda_rb returns.  `entries`: only these (x, t) are worked (the others
    stay NaN); `qentries`: only these get quantiles."""
    sp = spec(case)
    n_cols = max(sp.n_time)
    inp = cond_inputs(sp, draws_of(sp, mu, om, n, seed, draws), n, rows, quirk_of(case))
    if inputs_only:
        return inp
    out = {k: np.full((len(rows), n_cols), np.nan) for k in UNITS}
    out["quantiles"] = np.full((len(rows), n_cols, len(probs)), np.nan)
    out["n_reads"] = np.zeros((len(rows), n_cols), dtype=np.int64)
    out["n_sides"] = np.zeros((len(rows), n_cols), dtype=np.int32)
    for (x, t), v in inp.items():
        T = sp.n_time[rows[x] // sp.B]
        out["n_reads"][x, t], out["n_sides"][x, t] = int(v["R"]), (t + 1 < T) + (t >= 1)
        if entries is not None and (x, t) not in entries:
            continue
        e = Entry(v, M)
        for k, val in zip(UNITS, e.units()):
            out[k][x, t] = float(val)
        if len(probs) and (qentries is None or (x, t) in qentries):
            out["quantiles"][x, t] = [float(q) for q in e.quantiles(probs)]
    return out


@functools.lru_cache(maxsize=None)
def golden(name):
    with np.load(golden_path(name)) as f:
        g = {k: f[k] for k in f.files}
    for v in g.values():
        v.setflags(write=False)
    return g


# ---- comparison -----------------------------------------------------------------------------------------------------------------
def errors(got, ref, keys=UNITS + ("quantiles",)):
    """Largest error per output, relative to max(|x|, 1), over the cells where `ref` holds a value (there `got` must too)."""
    err = {}
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        assert a.shape == b.shape, (k, a.shape, b.shape)
        ok = ~np.isnan(b)
        assert not np.isnan(a[ok]).any(), k
        d = np.abs(a[ok] - b[ok])
        err[k] = float(np.max(d / np.maximum(np.abs(b[ok]), 1.0))) if ok.any() else 0.0
    return err


def assert_within(err, who):
    for k in err:
        assert err[k] <= (QTOL if k == "quantiles" else TOL), (who, k, err[k])


def report(name, label, err):
    print(f"llrb case {name:36s} {label:12s} " + " ".join(f"{k} {v / 1e-16:7.1f}" for k, v in err.items()) + "  (1e-16)")


same_bytes = rc.same_bytes


def live_cells(case, rows):
    sp = spec(case)
    live = np.zeros((len(rows), max(sp.n_time)), dtype=bool)
    for x, row in enumerate(rows):
        live[x, :sp.n_time[row // sp.B]] = True
    return live


# ---- 1. the identity against the log-joint -----------------------------------------------------------------------------------------
IDENTITY = SHAPES


def check_identity(lib, name, device=False):
    """At 3 random points z, each passed as the one explicit draw.  h'(x0) -- recovered from this restatement's folded coefficients
    at the base point z, g'(0) -- against the literal oracle's gradient entries of the loglambda block (and, device, against
    Engine.logdensity_grad), at `_rb_cases.check_identity`'s tolerance: 1e-9 of the block's largest entry.  The library is tied to
    the same coefficients without a debug route: at n_samples = 1 its mode_mean is x*, and g' built from the restatement's
    coefficients must vanish there to 2^-30 of the curvature scale's inverse (the iteration stops at a step of 2^-40 (1 + |u|)),
    which it does only if the library's tables A, B, its w, rho and its prior are the restatement's."""
    from oracle import literal
    quirk = quirk_of(name)
    sp = spec(name)
    off = sp.offsets()
    blk = slice(*off["loglambda"])
    g = np.random.default_rng(8)
    rows = list(range(sp.n_rep * sp.B))
    with engine(lib, name, seed=1) as e:
        assert e.loglambda_rb_shape() == (sp.n_rep * sp.B, max(sp.n_time))
        for scale in (0.3, 1.0, 0.3):
            z = g.normal(0.0, scale, sp.D)
            z[blk] += 1.5                                          # (rates of a few reads: every term of h' matters)
            inp = cond_inputs(sp, rc.Rows(z[None, :]), 1, rows, quirk)
            grad = literal.logjoint_and_grad(z, sp, **(dict(ragged_quirk=True) if quirk else {}))[1]
            scale_g = np.abs(grad[blk]).max()
            got = e.loglambda_rb(probs=(), draws=z)
            gd = e.logdensity_grad(z)[1] if device else None
            worst = worst_m = 0.0
            lo_l = off["loglambda"][0]
            for r in range(sp.n_rep):
                T = sp.n_time[r]
                for b in range(sp.B):
                    for t in range(T):
                        v = inp[(r * sp.B + b, t)]
                        c = Cond(F64, v["a"], v["ib2"], v["R"], v["As"][0], v["ws"][0], v["x0"][0], v["f0"][0], v["Bs"][0], v["wr"][0])
                        h1 = float(c.d12(np.float64(0.0))[0])
                        i = lo_l + b * T + t
                        worst = max(worst, abs(h1 - grad[i]) / scale_g)
                        if device:
                            assert abs(h1 - gd[i]) <= 1e-9 * np.abs(gd[blk]).max()
                        xs = got["mode_mean"][r * sp.B + b, t]
                        gm, cv = c.d12(np.float64(xs - z[i]))
                        worst_m = max(worst_m, abs(float(gm)) / (2.0 ** -30 * abs(float(cv)) * (1.0 + abs(xs - z[i]))))
                        assert got["q_mean"][r * sp.B + b, t] == z[i] and got["q_sd"][r * sp.B + b, t] == 0.0
                lo_l += T * sp.B
            print(f"llrb identity {name:28s} sd {scale}: restatement {worst:.2e} of max |g| = {scale_g:.3g}; library's mode: |g'(x*)| = {worst_m:.2e} of 2^-30 |g''| (1 + |u|)")
            assert worst <= 1e-9
            assert worst_m <= 1.0
            assert np.array_equal(np.isnan(got["rb_mean"]), ~live_cells(name, rows))


# ---- 2. golden values ----------------------------------------------------------------------------------------------------------
def check_golden(lib, name, label):
    case, n, rows, gent, qent = golden_cases()[name]
    rows = list(rows)
    sp, mu, om = inputs(case)
    ref = golden(name)
    live = live_cells(case, rows)
    with engine(lib, case, mu, om) as e:
        got = ll(e, n, rows=rows)
    assert np.array_equal(got["n_reads"], ref["n_reads"]) and np.array_equal(got["n_sides"], ref["n_sides"])
    for k in UNITS:
        assert np.array_equal(np.isnan(got[k]), ~live), k
    assert np.array_equal(np.isnan(got["quantiles"]), ~(live[..., None] & np.ones(3, dtype=bool)))
    assert np.all(np.diff(got["quantiles"][live], axis=1) > 0)
    err = errors(got, ref)
    if n <= 111:                                                  # the float64 restatement itself, where it is quick
        r64 = restate(case, mu, om, n, SEED, rows, entries=None if gent is None else set(gent), qentries=set(qent))
        e0 = errors(r64, ref)
        report(name, "restatement", e0)
        assert_within(e0, "restatement")
    if not qent and n <= 1000:                                    # no 50-digit quantiles: the float64 restatement's, one entry
        qe = {gent[0]}
        r64 = restate(case, mu, om, n, SEED, rows, entries=qe, qentries=qe)
        err["quantiles"] = errors(got, r64, keys=("quantiles",))["quantiles"]
    elif not qent:                                                # the sample cap: the median of one entry against the restatement
        qe = {gent[0]}
        r64 = restate(case, mu, om, n, SEED, rows, probs=(0.5,), M=PY, entries=qe, qentries=qe)
        assert np.isfinite(r64["quantiles"][gent[0]]).all()
        err["quantiles"] = errors({"quantiles": got["quantiles"][..., 1:2]}, r64, keys=("quantiles",))["quantiles"]
    report(name, label, err)
    assert_within(err, label)
    return got


# ---- 2b. two kept modes in the library itself ------------------------------------------------------------------------------------
BIMODAL_SETS = ((0.35, 6.4, -1.26), (0.35, 6.4, -1.06), (0.15, 6.4, -1.26), (0.25, 7.4, -1.26), (0.35, 7.4, -1.26))


@functools.lru_cache(maxsize=None)
def bimodal_draws():
    """(draws [5, D], row, t): explicit draws of `BIMODAL` at which the conditional of one entry -- mutant 6 at t = 1, which has no
    read there -- has two kept modes in every draw (`truth_sets` 75 .. 78 made from a handle).  Every rate of the draw is about 0.21 but
    the entry's own, 1: it holds 30 % of its time point; its neighbours in time lie `pull` below it, so its own ratio terms (its
    logsigma `own_ls`: a weight of about 1/2 a side) hold a mode near x0 - pull, where delta has levelled off at ln(1 - f0), while
    the other barcodes' terms (weight e^{-2 wo} each, residuals near zero at the draw: s_pop takes up the normaliser's step) hold one
    near the draw.  (draw 0: the right mode is the global one; the others: the left.)"""
    sp = spec(BIMODAL)
    off, nn, B, T = sp.offsets(), sp.n_neutral, sp.B, sp.n_time[0]
    b, t = nn + 6, 1
    g = np.random.default_rng(21)
    out = []
    for own_ls, pull, wo in BIMODAL_SETS:
        z = np.zeros(sp.D)
        lo = off["loglambda"][0]
        z[lo:lo + B * T] = np.log(0.21) + g.normal(0, 0.03, B * T)
        z[lo + b * T + t] = 0.0
        z[lo + b * T + t - 1] = z[lo + b * T + t + 1] = -pull
        z[slice(*off["s_pop"])] = [0.36, -0.36, 0.0]
        z[slice(*off["logsigma_pop"])] = wo
        z[slice(*off["s_bc"])] = g.normal(0, 0.02, sp.n_bc)
        z[slice(*off["logsigma_bc"])] = wo
        z[off["logsigma_bc"][0] + (b - nn)] = own_ls
        out.append(z)
    dr = np.array(out)
    dr.setflags(write=False)
    return dr, b, t


def restate_bimodal(M=F64):
    dr, b, t = bimodal_draws()
    return restate(BIMODAL, None, None, len(dr), 0, [b], draws=dr, M=M)


def check_bimodal(lib, label):
    """The library on draws whose conditional has two kept modes (all five draws of the entry; asserted on the restatement, with
    the grid's ends outside both modes), against a 50-digit golden of moments and quantiles of the row's four entries: a mode
    missed, or the grid laid from the wrong outer mode, moves rb_mean and rb_sd by units, not by 1e-12."""
    dr, b, t = bimodal_draws()
    sp = spec(BIMODAL)
    inp = cond_inputs(sp, rc.Rows(dr), len(dr), [b])[(0, t)]
    assert inp["R"] == 0.0
    e64 = Entry(inp)
    globals_ = []
    for j in range(len(dr)):
        assert len(e64.modes[j]) == 2, (j, e64.modes[j])
        assert all(e64.lo[j] < inp["x0"][j] + m < e64.hi[j] for m in e64.modes[j]), j      # the grid covers both
        globals_.append(int(np.argmin([abs(float(inp["x0"][j] + m - e64.c[j].x)) for m in e64.modes[j]])))
    assert set(globals_) == {0, 1}, globals_                       # the global mode is the left one in some draws, the right one in others
    ref = golden(BIMODAL)
    e0 = errors(restate_bimodal(), ref)
    report(BIMODAL, "restatement", e0)
    with make_engine(sp, lib, seed=1) as e:
        got = e.loglambda_rb(probs=PROBS, draws=dr, rows=[b])
        one = e.loglambda_rb(probs=PROBS, draws=dr[:1], rows=[b])
    err = errors(got, ref)
    report(BIMODAL, label, err)
    assert_within(e0, "restatement")
    assert_within(err, label)
    assert np.all(np.diff(got["quantiles"], axis=2) > 0)
    # one draw alone: the 2.5 % and 97.5 % quantiles of a single two-mode conditional lie on either side of the gap between its modes
    lo_m, hi_m = (float(inp["x0"][0] + m) for m in e64.modes[0])
    assert one["quantiles"][0, t, 0] < lo_m + 1.0 and one["quantiles"][0, t, 2] > hi_m - 1.0, one["quantiles"][0, t]
    return got


# ---- 3. the rule against quadrature of the density -------------------------------------------------------------------------------
def truth_sets():
    """Per-draw inputs (a, ib2, R, As, ws, x0, f0, Bs, wr) the rule is measured on: the low-count entries of three cases (the
    first two draws of each) and synthetic sets -- counts 0 .. 3 against a strong ratio term pulling elsewhere (two modes), a wide
    prior, a count of 1000."""
    sets = []
    for case in ("fitness", "replicate_ragged", "fitness_matrix_prior"):
        sp, mu, om = inputs(case)
        rows = rows_of(case)[:6]
        inp = cond_inputs(sp, draws_of(sp, mu, om, 2, SEED), 2, rows, quirk_of(case))
        for (x, t), v in sorted(inp.items()):
            if v["R"] <= 3:
                for j in (0, 1):
                    sets.append((v["a"], v["ib2"], v["R"], v["As"][j], v["ws"][j], v["x0"][j], v["f0"][j], v["Bs"][j], v["wr"][j]))
    for R in (0.0, 1.0, 3.0):
        for pull in (2.5, 4.0, 5.5):                              # own ratio terms want x near `pull`, the count wants ln R or less
            for w in (2.0, 8.0):
                x0 = 1.0
                sets.append((3.0, 1.0 / 9.0, R, 300.0 * w, w, x0, 1e-3, 0.3 * w, w * (pull - x0)))
    sets.append((3.0, 1.0 / 9.0, 1000.0, 5000.0, 20.0, 6.5, 0.02, -40.0, 3.0))
    sets.append((0.0, 1.0 / 25.0, 0.0, 0.0, 0.0, -1.0, 1e-4, 0.0, 0.0))
    sets.append((3.0, 1.0 / 9.0, 2.0, 4000.0, 30.0, 0.2, 0.3, 900.0, -20.0))      # a frequent barcode: the normaliser terms dominate
    # two draws of a handle 20 steps into its fit (benchmark shape, far from converged: the draw e^9.3 against 62 reads, tables of
    # 1e7): the bracket's lower end must follow e^x down, or the scan's cells are 75 wide and miss the global mode
    sets.append((3.0, 0.1111111111111111, 62.0, 42307991.356019065, 21.418066715192396, 9.326143131923336, 0.0491796448985362,
                 -31652007.60013137, -336.38963138838693))
    sets.append((3.0, 0.1111111111111111, 12.0, 11541964.769153673, 65.87833813444053, 11.461949793656926, 0.27179240661220033,
                 -8905909.595287751, -809.3841785773635))
    # two modes: a barcode that is 30 % of its time point with no reads, its own ratio term pulling 6 .. 7 below the draw -- the
    # normaliser term -As delta^2 / 2 holds one mode near the draw (lowering x there moves every other barcode's residual), the
    # own term one near its target, where delta has levelled off at ln(1 - f0)
    sets.append((0.0, 1.0 / 9.0, 0.0, 300.0, 1.0, 0.0, 0.3, 0.0, -6.0))           # the right mode is the global one
    sets.append((0.0, 1.0 / 9.0, 0.0, 200.0, 1.0, 0.0, 0.3, 0.0, -6.0))           # the left one is
    sets.append((0.0, 1.0 / 9.0, 0.0, 300.0, 1.5, 0.0, 0.3, 0.0, -9.0))
    sets.append((0.0, 1.0 / 9.0, 0.0, 300.0, 1.2, 0.0, 0.3, 0.0, -7.0))
    return sets


def truth_path():
    return os.path.join(GOLD, "llrb_truth.npz")


def check_truth():
    """The float64 rule against mpmath.quad of exp(h) (tests/golden/llrb_truth.npz, written by make_loglambda_rb_golden.py
    --truth): ln Z_j (about the global mode) absolute, E in units of the global mode's curvature scale, V relative, the CDF at the
    global mode + TRUTH_AT curvature scales absolute.  Bounds and measured figures: the module docstring."""
    with np.load(truth_path()) as f:
        T = {k: f[k] for k in f.files}
    sets = truth_sets()
    assert np.array_equal(T["sets"], np.array(sets))
    worst = {grp: dict(lnZ=0.0, E=0.0, V=0.0, C=0.0) for grp in ("ordinary", "hard")}
    two = []
    with np.errstate(all="ignore"):
        for i, st in enumerate(sets):
            c0 = Cond(F64, *st[:5], *st[5:])
            ca, s, nl, nr, modes = setup(c0)
            Z, E, V, L = moments(ca, s, nl, nr)
            dl = 1.0 / np.sqrt(-ca.d12(np.float64(0.0))[1])
            # ln Z_j as the rule defines it, about the global mode (the truth: about the 50-digit mode; h is flat there)
            lnZ = float(np.log(Z))
            w = worst["hard" if len(modes) > 1 or st[3] > 1e6 else "ordinary"]
            w["lnZ"] = max(w["lnZ"], abs(lnZ - T["lnZ"][i]))
            w["E"] = max(w["E"], abs(float(E) - T["E"][i]) / float(dl))
            w["V"] = max(w["V"], abs(float(V) - T["V"][i]) / T["V"][i])
            for k, at in enumerate(TRUTH_AT):
                x = ca.x + at * dl
                assert float(x) == T["xs"][i, k]
                lo, hi = ca.x - nl * s, ca.x + nr * s
                Cx = 0.0 if x <= lo else (1.0 if x >= hi else float(cdf_z(ca, s, lo, x) / Z))
                w["C"] = max(w["C"], abs(Cx - T["C"][i, k]))
            if len(modes) > 1:
                two.append(i)
                lo, hi = float(ca.x - nl * s), float(ca.x + nr * s)
                assert all(lo < float(c0.x + m) < hi for m in modes), i      # the grid covers every kept mode
                assert int(T["n_modes"][i]) == len(modes), i
    for grp, w in worst.items():
        print(f"llrb truth, {grp} sets: " + ", ".join(f"{k} {v:.2e}" for k, v in w.items()))
    print(f"llrb truth: sets with two kept modes: {two}")
    assert two, "no bimodal set"
    w = worst["ordinary"]                                         # no worse than bb_logsigma_rb's rule is recorded to do on its own cases
    assert w["lnZ"] <= LS_TRUTH["lnZ"] and w["E"] <= LS_TRUTH["E"] and w["V"] <= LS_TRUTH["V"] and w["C"] <= LS_TRUTH["C"], w
    w = worst["hard"]
    assert w["lnZ"] <= TRUTH_TOL and w["E"] <= TRUTH_TOL and w["V"] <= TRUTH_TOL and w["C"] <= TRUTH_CTOL, w


# ---- 4. invariance and robustness ----------------------------------------------------------------------------------------------
def check_rows_subset(lib, case="replicate_ragged", n=111):
    sp, mu, om = inputs(case)
    rows = rows_of(case)
    with engine(lib, case, mu, om) as e:
        full = ll(e, n, rows=rows)
        for sub in ([rows[1]], rows[2::3], rows[-1:]):
            part = ll(e, n, rows=sub)
            pick = [rows.index(x) for x in sub]
            assert same_bytes(part, {k: v[pick] for k, v in full.items()}), sub
    return full


def check_all_rows(lib, case=TINY, n=64):
    """rows = None is every row: the same bytes as the rows listed."""
    sp, mu, om = inputs(case)
    with engine(lib, case, mu, om) as e:
        a = ll(e, n)
        b = ll(e, n, rows=np.arange(sp.n_rep * sp.B))
    assert a["rb_mean"].shape == (sp.n_rep * sp.B, max(sp.n_time)) and same_bytes(a, b)


def check_launch_modes(lib, case="replicate_ragged"):
    import barbay_jl_amd as bb
    sp, mu, om = inputs(case)
    rows = rows_of(case)[3:9]
    out = []
    for mode in (1, 0):
        with bb.Engine(sp.kind, sp.counts, sp.n_neutral, sp.n_bc, env_idx=sp.env_idx, geno_idx=sp.geno_idx, seed=4, launch_mode=mode, _lib=lib) as e:
            e.set_params(mu, om)
            out.append(ll(e, 200, seed=2, rows=rows))
            out.append(ll(e, 200, seed=2, rows=rows))
    assert all(same_bytes(out[0], o) for o in out[1:])


def check_group_handle(lib, case):
    sp, mu, om = inputs(case)
    rows = rows_of(case)[:6]
    with engine(lib, case, mu, om, device_ids=[0, 0]) as e:
        a = ll(e, 111, rows=rows)
    with engine(lib, case, mu, om) as e:
        b = ll(e, 111, rows=rows)
    assert same_bytes(a, b)


GROUP_CASES = ("fitness", "genotype_regrouped", "replicate_ragged")


def check_internal_against_explicit_draws(lib, case, n=64):
    sp, mu, om = inputs(case)
    rows = rows_of(case)[:6]
    dr = rc.materialise(sp, mu, om, n, SEED)
    with engine(lib, case, mu, om) as e:
        a = ll(e, n, rows=rows)
        b = ll(e, n, rows=rows, draws=dr)
        c = ll(e, 5, rows=rows, draws=dr)
    assert same_bytes(b, c)
    err = errors(a, b)
    report(case + f"_n{n}", "own/explicit", err)
    assert_within(err, "explicit draws")


def check_buffer_reuse(lib):
    sp, mu, om = inputs("fitness")
    rows = rows_of("fitness")
    dr = rc.materialise(sp, mu, om, 7, 3)
    calls = [lambda e: ll(e, 111, rows=rows[:3]),
             lambda e: e.freq_bands((0.95, 0.5), mode="posterior", n_samples=200, n_ppc=1, seed=SEED),
             lambda e: ll(e, 500, rows=rows[3:5]),
             lambda e: e.logsigma_rb(block="pop", n_samples=111, seed=SEED),
             lambda e: ll(e, 2, rows=rows),
             lambda e: ll(e, 7, rows=rows[:2], draws=dr),
             lambda e: ll(e, 111, rows=rows[:3])]
    with engine(lib, "fitness", mu, om) as e:
        got = [pc._bits(f(e)) for f in calls]
    for i, f in enumerate(calls):
        with engine(lib, "fitness", mu, om) as e:
            assert got[i] == pc._bits(f(e)), i
    assert got[0] == got[6]


def check_handle_untouched(lib):
    sp = spec("fitness")
    rows = rows_of("fitness")[:3]
    with make_engine(sp, lib, seed=5) as a, make_engine(sp, lib, seed=5) as b:
        ll(b, 64, rows=rows)
        for x, y in zip(a.get_params(), b.get_params()):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
        a.run(5)
        ll(b, 32, seed=1, rows=rows)
        b.run(5)
        for x, y in zip(a.get_params(), b.get_params()):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64))


def check_nan_stays(lib, case="replicate_ragged", n=32):
    """(a) One mutant's logsigma_bc NaN: at n_sides >= 1 every entry of its replicate reads it through the tables A, B; no entry of
    another replicate changes a byte.  (b) One loglambda (r = 1, t = 2, b) NaN: every entry of (r = 1, t = 2) is NaN through Z, as
    are those of t = 1 and t = 3 (the steps' tables); the other time points of r = 1 and all of the other replicates keep their bytes."""
    sp, mu, om = inputs(case)
    off, B, nn = sp.offsets(), sp.B, sp.n_neutral
    rows = [r * B + b for r in range(sp.n_rep) for b in (0, nn + 5, B - 1)]
    with engine(lib, case, mu, om) as e:
        base = ll(e, n, rows=rows)
    mu2 = mu.copy()
    mu2[off["logsigma_bc"][0] + sp.n_bc * 1 + 2] = np.nan          # replicate kind: unit m + nb r; mutant 2 of replicate 1
    with engine(lib, case, mu2, om) as e:
        got = ll(e, n, rows=rows)
    keep = [0, 1, 2, 6, 7, 8]
    assert same_bytes({k: v[keep] for k, v in got.items()}, {k: v[keep] for k, v in base.items()})
    T1 = sp.n_time[1]
    assert np.all(np.isnan(got["rb_mean"][3:6, :T1])) and np.all(np.isnan(got["quantiles"][3:6, :T1]))
    assert same_bytes({k: got[k][3:6] for k in ("q_mean", "q_sd", "n_reads", "n_sides")}, {k: base[k][3:6] for k in ("q_mean", "q_sd", "n_reads", "n_sides")})
    mu3 = mu.copy()
    lo1 = off["loglambda"][0] + sp.n_time[0] * B
    mu3[lo1 + (nn + 7) * T1 + 2] = np.nan
    with engine(lib, case, mu3, om) as e:
        got = ll(e, n, rows=rows)
    assert same_bytes({k: v[keep] for k, v in got.items()}, {k: v[keep] for k, v in base.items()})
    for k in ("rb_mean", "rb_sd", "lambda_mean", "mode_mean"):
        assert np.all(np.isnan(got[k][3:6, 1:4])), k
        for t in [0] + list(range(4, T1)):
            assert np.array_equal(got[k][3:6, t].view(np.uint64), base[k][3:6, t].view(np.uint64)), (k, t)


def raw_ll(engine_, n_samples, probs=PROBS, seed=SEED, draws=None, rows=None, n_rows=None, null=(), want=UNITS + ("quantiles", "n_reads", "n_sides"),
           n_quantiles=None):
    """bb_loglambda_rb through ctypes with only the outputs in `want` non-NULL; `null` names arguments passed as NULL."""
    nr, nc = engine_.loglambda_rb_shape()
    p = np.ascontiguousarray(probs, dtype=np.float64)
    o = _capi.bb_loglambda_rb_opts()
    o.n_samples, o.n_quantiles, o.seed = n_samples, len(p) if n_quantiles is None else n_quantiles, seed
    o.probs = None if "probs" in null or not len(p) else _capi._ptr(p)
    if draws is not None:
        o.draws = _capi._ptr(draws)
    if rows is not None:
        rr = np.ascontiguousarray(rows, dtype=np.int64)
        o.rows, o.n_rows = rr.ctypes.data_as(C.POINTER(C.c_int64)), len(rr) if n_rows is None else n_rows
        nr = max(len(rr), 0)
    res, out = {}, _capi.bb_loglambda_rb_out()
    for k in want:
        if k in ("n_reads", "n_sides"):
            res[k] = np.full((nr, nc), -7, dtype=np.int64 if k == "n_reads" else np.int32)
            setattr(out, k, res[k].ctypes.data_as(C.POINTER(C.c_int64 if k == "n_reads" else C.c_int32)))
        else:
            res[k] = np.full((nr, nc, len(p)) if k == "quantiles" else (nr, nc), -7.0)
            setattr(out, k, _capi._ptr(res[k]))
    rc_ = engine_._lib.bb_loglambda_rb(None if "h" in null else engine_._h, None if "o" in null else C.byref(o),
                                       None if "out" in null else C.byref(out))
    return rc_, res


def check_errors(lib):
    """Every BB_ERR_INVALID and BB_ERR_UNSUPPORTED of the contract, with a message (BB_ERR_DEVICE for an allocation the device
    cannot make is not provoked, as in `_rb_cases.check_errors`)."""
    sp, mu, om = inputs(TINY)
    INVALID, UNSUPPORTED = -1, _capi.BB_ERR_UNSUPPORTED
    msg = lambda: lib.bb_last_error().decode()
    dr = rc.materialise(sp, mu, om, 3, 1)
    n_all = sp.n_rep * sp.B
    with engine(lib, TINY, mu, om) as e:
        for null in ("h", "o", "out"):
            assert raw_ll(e, 10, null=(null,))[0] == INVALID and msg(), null
        for nq in (-1, 9):
            assert raw_ll(e, 10, n_quantiles=nq)[0] == INVALID and "n_quantiles" in msg(), nq
        assert raw_ll(e, 10, null=("probs",), n_quantiles=3)[0] == INVALID and "probs" in msg()
        for bad in (0.0, 1.0, -0.1, 1.5, np.nan):
            assert raw_ll(e, 10, probs=(0.5, bad))[0] == INVALID and "prob" in msg(), bad
        for n in (1, 0, -3, MAXN + 1):
            assert raw_ll(e, n)[0] == UNSUPPORTED and "n_samples" in msg(), n
        for n in (0, MAXN + 1):
            assert raw_ll(e, n, draws=dr)[0] == UNSUPPORTED and "n_samples" in msg(), n
        for bad in ([-1], [n_all], [3, 3], [5, 2], [0, 1, n_all + 4]):
            assert raw_ll(e, 10, rows=bad)[0] == INVALID and "rows" in msg(), bad
        assert raw_ll(e, 10, rows=[1], n_rows=-2)[0] == INVALID and "n_rows" in msg()
        assert raw_ll(e, 1, draws=dr, rows=[2])[0] == 0 and raw_ll(e, 3, draws=dr, rows=[2])[0] == 0      # one explicit draw is served
        assert raw_ll(e, 16, want=(), rows=[2])[0] == 0                                                     # an all-NULL out
        assert raw_ll(e, 16, probs=(), rows=[2])[0] == 0                                                    # no quantiles
        assert raw_ll(e, 16, rows=[2], n_rows=0)[0] == 0                                                    # no rows: nothing to do
        full = ll(e, 16, rows=[2, 7])
        assert same_bytes(raw_ll(e, 16, rows=[2, 7])[1], full)
        for k in UNITS + ("quantiles", "n_reads", "n_sides"):                                               # every output NULL except one
            rc_, one = raw_ll(e, 16, rows=[2, 7], want=(k,))
            assert rc_ == 0 and same_bytes(one, {k: full[k]}), k
        try:
            e.loglambda_rb(n_samples=1)
        except _capi.BarBayHipError as ex:
            assert "error -4" in str(ex) and "n_samples" in str(ex)
        else:
            raise AssertionError("no error")
        try:
            e.loglambda_rb(draws=np.zeros((3, sp.D + 1)))
        except _capi.BarBayHipError as ex:
            assert "draws" in str(ex)
        else:
            raise AssertionError("no error")


# ---- 5. statistics (GPU) ---------------------------------------------------------------------------------------------------------
def check_statistics(lib, case="fitness", n_big=20000):
    """One entry with R = 2 (the count of a mutant of `fitness` set to 2 at t = 2) at the sample cap: rb_mean, rb_sd^2 and
    lambda_mean against an independent numpy sample of `n_big` joint draws (numpy's generator, not the library's keying) pushed
    through the restatement's per-draw rule, within 6 Monte-Carlo standard errors of the difference of the two means."""
    sp0 = spec(case)
    counts = [np.array(c) for c in sp0.counts]
    b = sp0.n_neutral + 6
    counts[0][2, b] = 2
    sp = ModelSpec(kind=sp0.kind, counts=counts, totals=[c.sum(axis=1) for c in counts], n_neutral=sp0.n_neutral, n_bc=sp0.n_bc)
    mu, om = rc.params(sp)
    with pc._handle(lib, sp, mu, om) as e:
        got = ll(e, MAXN, rows=[b], probs=())
    g = np.random.default_rng(77)
    dr = mu[None, :] + pc.softplus(om)[None, :] * g.standard_normal((n_big, sp.D))
    inp = cond_inputs(sp, rc.Rows(dr), n_big, [b])[(0, 2)]
    assert inp["R"] == 2.0
    E, V, L = _vector_moments(inp)
    for k, ref, lib_v in (("rb_mean", E, got["rb_mean"][0, 2]), ("lambda_mean", L, got["lambda_mean"][0, 2])):
        se = ref.std() * math.sqrt(1.0 / n_big + 1.0 / MAXN)
        print(f"llrb statistics {k}: library {lib_v:.6f}, sample {ref.mean():.6f}, se {se:.2e}")
        assert abs(lib_v - ref.mean()) <= 6.0 * se, k
    tot = V + (E - E.mean()) ** 2
    se = tot.std() * math.sqrt(1.0 / n_big + 1.0 / MAXN)
    print(f"llrb statistics rb_sd^2: library {got['rb_sd'][0, 2] ** 2:.6f}, sample {tot.mean():.6f}, se {se:.2e}")
    assert abs(got["rb_sd"][0, 2] ** 2 - tot.mean()) <= 6.0 * se


def _vector_moments(inp, half=12.0, nodes=4001):
    """(E_j, V_j, Lam_j) of many draws at once: a fixed fine trapezoid grid about x0 (not the rule: an independent quadrature, good
    to far below a Monte-Carlo standard error for the smooth unimodal entries it is used on)."""
    u = np.linspace(-half, half, nodes)[None, :]
    col = lambda k: np.asarray(inp[k])[:, None]
    em = np.expm1(u)
    y = col("f0") * em
    dl = np.log1p(y)
    x0 = col("x0")
    g = (-(inp["ib2"] / 2) * (u * (u + 2 * (x0 - inp["a"]))) + inp["R"] * u - np.exp(x0) * em - col("Bs") * dl - (col("As") / 2) * dl * dl
         - (col("ws") / 2) * u * u + u * col("wr") + col("ws") * u * dl)
    p = np.exp(g - g.max(axis=1, keepdims=True))
    z = p.sum(axis=1)
    E = (p * u).sum(axis=1) / z
    V = (p * u * u).sum(axis=1) / z - E * E
    L = (p * np.exp(x0 + u)).sum(axis=1) / z
    return x0[:, 0] + E, V, L
