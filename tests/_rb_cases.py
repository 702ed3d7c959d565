"""bb_fitness_rb (Rao-Blackwellised fitness marginals, barbay.jl_amd/csrc/bb_rb.h) restated in numpy from the formulas of
include/barbay_hip.h, and the cases the emulation and GPU tests share.  The keying is the header's: parameter draw j of the
caller's latent i is pairs(seed, i, j >> 1, 0xFFFFFFE0), an even index taking the cosine branch -- the draw of bb_ppc_bands.

Expected values: tests/golden/rb_<case>_n<samples>.npz, a 50-digit mpmath evaluation of the same formulas on this restatement's
float64 (s_j, m_j, sd_j), written by tests/golden/make_rb_golden.py (the quantile: the 50-digit root of the mixture CDF); mpmath
is not needed to read them.  Bounds, in `_score_cases`' sense: TOL = 1e-12 relative to max(|x|, 1) for q_mean, q_sd, rb_mean,
rb_sd; relative to the value itself for p_pos and p_neg (`params` and THRESHOLD keep |m_j - s0| / sd_j <= 20, `check_z_range`);
n_steps and the NaN pattern exact.  Quantiles: QTOL = the larger of 1e-12 max(|x|, 1) and 8 x the float64 restatement's own
measured error against the 50-digit root (Q_MEASURED, the margin `_accuracy_cases` gives the literal oracle).

Why the library stays inside: its (m_j, sd_j) differ from the restatement's by the few ulp between its exp / log / Box-Muller and
numpy's, amplified by the cancellation in gamma (a difference of loglambda draws near 5 and of log Z near 10 giving a step of
0.1 .. 1: some 50 ulp of the result); a tail at |z| = 20 moves by |z|^2 ulp per ulp of z.

Measured, largest error over a case's units against the golden, float64 restatement / host emulation / MI355X, in units of 1e-16
(relative as above; each test prints its own line):

case                                                      q_mean               q_sd            rb_mean              rb_sd              p_pos              p_neg          quantiles
fitness_chunk_n1000                    2.1/  4.5/  4.5    0.1/  0.2/  0.2    1.1/  4.4/  4.4    0.6/  0.8/  0.8    6.9/ 12.9/ 15.0   26.9/ 30.6/ 29.0    6.4/ 25.5/ 25.5 
fitness_chunk_n111                     4.2/  5.6/  5.6    0.1/  0.2/  0.2    3.3/  4.4/  4.4    0.6/  1.1/  1.1   11.3/ 45.1/ 48.3   26.0/ 26.0/ 29.2   15.5/ 25.5/ 25.5 
fitness_chunk_n2                       0.0/  1.1/  1.1    0.0/  2.2/  2.2    0.0/  2.2/  2.2    0.6/  0.8/  0.8   21.9/ 69.2/ 66.7   67.3/ 81.5/ 87.1    4.4/  4.4/  4.4 
fitness_n1000                          2.2/  2.8/  2.8    0.1/  0.1/  0.1    1.1/  2.2/  2.2    0.3/  0.6/  0.6    3.1/  4.6/  4.6   25.3/ 46.7/ 46.7    3.3/ 12.2/ 12.2 
fitness_n111                           3.0/  4.4/  4.4    0.1/  0.1/  0.1    2.2/  4.4/  4.4    0.3/  0.6/  0.6    3.9/  7.5/  7.5   27.1/ 50.5/ 48.5   12.2/ 14.4/ 14.4 
fitness_n2                             0.0/  1.1/  1.1    0.0/  0.6/  0.6    0.0/  1.1/  1.1    0.3/  0.3/  0.3   11.7/  9.3/ 10.5  104.4/ 87.0/ 87.0    2.2/  2.2/  2.2 
fitness_n2049                          1.6/  4.4/  4.4    0.1/  0.1/  0.1    1.1/  3.3/  3.3    0.3/  0.3/  0.3    4.8/  4.4/  6.3   25.2/ 40.9/ 42.4    4.4/ 12.2/ 12.2 
fitness_n8672                          1.4/  5.6/  5.6    0.0/  0.1/  0.1    0.6/  5.6/  5.6    0.0/  0.3/  0.3    1.1/  3.1/  3.8    5.4/  6.8/  6.8    2.0/  6.1/  6.1 
genotype_regrouped_n1000               1.5/  4.6/  4.6    0.3/  0.3/  0.4    1.1/  2.2/  2.2    0.1/  0.1/  0.1    2.8/  5.6/  5.6   61.5/ 73.8/ 79.9    2.2/  4.4/  4.4 
genotype_regrouped_n111                2.2/  6.9/  6.9    0.1/  0.4/  0.8    1.7/  3.3/  2.2    0.1/  0.1/  0.1    4.2/  7.2/  8.7   69.1/ 55.0/ 60.6    3.3/  6.7/  6.7 
genotype_regrouped_n2                  0.0/  1.2/  1.2    0.0/  2.2/  2.2    0.0/  0.6/  1.1    0.1/  0.3/  0.5    1.7/  3.6/  6.0  102.8/217.1/324.5    1.1/  1.1/  2.2 
multienv_env0_only_first_n1000         1.5/  5.1/  5.1    0.1/  0.1/  0.1    1.1/  3.3/  3.3    0.6/  0.6/  0.6    4.2/  7.2/  7.2    4.9/  9.3/  9.3   12.5/ 35.1/ 35.1 
multienv_env0_only_first_n111          2.9/  4.2/  4.2    0.1/  0.1/  0.1    1.7/  4.4/  4.4    0.6/  0.8/  0.6    4.6/  9.5/  8.8    6.0/ 10.0/ 10.0   41.9/ 23.8/ 23.8 
multienv_env0_only_first_n2            0.0/  0.3/  0.3    0.1/  0.1/  0.1    0.0/  2.2/  2.2    0.6/  0.6/  0.6    5.6/  6.3/  6.3   13.3/ 51.0/ 48.8    5.7/  5.7/  5.7 
multienv_n1000                         2.1/  4.7/  4.7    0.1/  0.1/  0.1    2.0/  4.4/  4.4    0.6/  1.1/  0.6    7.7/ 12.4/  7.7   48.9/266.8/251.8    6.4/ 28.9/ 28.9 
multienv_n111                          3.3/  6.5/  6.5    0.1/  0.3/  0.3    2.2/  5.6/  5.6    0.6/  0.6/  0.6   17.9/ 16.6/ 16.6   59.8/ 77.7/ 75.8   18.9/ 36.6/ 36.6 
multienv_n2                            0.0/  2.1/  2.1    0.0/  4.4/  4.4    0.0/  4.4/  4.4    0.6/  0.6/  0.6   12.9/ 22.1/ 24.0  128.0/217.3/217.3    4.4/  6.1/  6.1 
multienv_replicate_n1000               2.1/  4.4/  4.4    0.3/  0.3/  0.7    1.1/  5.6/  5.6    0.1/  0.1/  0.1  126.0/ 85.4/ 91.8  263.9/256.4/353.5    2.2/  5.6/  5.0 
multienv_replicate_n111                3.3/  6.0/  4.4    0.1/  0.6/  1.0    3.3/  4.4/  4.4    0.1/  0.2/  0.2   89.6/ 85.3/ 85.3  202.6/215.0/213.4    4.4/  6.7/  6.7 
multienv_replicate_n2                  0.0/  3.1/  3.1    0.1/  8.9/ 11.1    0.0/  1.1/  2.2    0.1/  0.4/  0.4  188.7/197.3/197.3  287.9/257.4/257.4    1.1/  2.2/  2.2 
replicate_ragged_n1000                 1.5/  4.0/  4.0    0.1/  0.3/  0.6    1.1/  4.4/  4.4    0.1/  0.1/  0.1   51.6/ 46.2/ 44.0   98.4/105.4/159.0    1.7/  4.9/  5.1 
replicate_ragged_n111                  3.3/  6.0/  6.0    0.3/  0.4/  0.8    2.2/  3.3/  3.3    0.1/  0.1/  0.1   59.2/ 78.0/ 83.4   96.7/283.5/227.1    3.3/  6.7/  6.7 
replicate_ragged_n2                    0.0/  1.1/  2.5    0.0/  0.6/  2.2    0.0/  1.1/  1.1    0.1/  0.4/  0.4   78.8/ 87.2/ 87.2  128.5/250.5/420.4    1.1/  2.2/  2.2 
(the largest entry of the first six columns, 420.4e-16, is 0.042 of the bound 1e-12; the largest quantile entry, 41.9e-16 -- the
 restatement's own: Q_MEASURED --, is 0.0042 of QTOL = 1e-12, 8 x 4.2e-15 = 3.4e-14 being the smaller of the two)
Four and eight quantiles (`check_many_quantiles`, multienv at n = 111, against the float64 restatement, no golden): quantiles
33.3 (emulation) / 33.3 (MI355X) with four, 391.7 / 391.7 with eight, which include the probabilities 0.001 and 0.999, where the
mixture's density is small and the root less well conditioned: 0.039 of QTOL.
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
from oracle import fixtures
from oracle.spec import ModelSpec

GOLD = os.path.join(os.path.dirname(__file__), "golden")
UNITS = ("q_mean", "q_sd", "rb_mean", "rb_sd", "p_pos", "p_neg")
SELF_RELATIVE = ("p_pos", "p_neg")
TOL = 1e-12
Q_MEASURED = 4.2e-15      # the float64 restatement's largest quantile error against the 50-digit root, relative to max(|x|, 1): see the table
QTOL = max(1e-12, 8.0 * Q_MEASURED)
SEED = 11
PSEED = 5
NS = (2, 111, 1000)
PROBS = (0.025, 0.5, 0.975)
THRESHOLD = 0.3
MAXN = _capi.BB_RB_MAX_SAMPLES
Z_HI = 20.0
Z_REACH = {"multienv_replicate_n1000": 12.0, "replicate_ragged_n1000": 12.0, "genotype_regrouped_n1000": 10.0}      # |z| these cases get to at least
HIER = ("genotype", "replicate", "multienv_replicate")
NEW_CASES = ("multienv_env0_only_first", "fitness_chunk")
# name -> (case, n_samples, units with a golden or None for all)
BIG = {
    "fitness_n2049": ("fitness", 2049, None),                    # more draws than the block has threads, no multiple of 64
    f"fitness_n{MAXN}": ("fitness", MAXN, (0, 3, 10, 27, 49)),  # the largest call: the first / some middle (3, 10: sharp ones) / the last mutant
}


@functools.lru_cache(maxsize=None)
def spec(case):
    if case in pc.CASES:
        return pc.spec(case)
    if case == "multienv_env0_only_first":                       # environment 0 at time point 0 only: its units have n_u = 0
        sp = fixtures.synthetic("multienv", B=30, T=5, n_env=3, n_neutral=6, seed=3)
        return ModelSpec(kind=sp.kind, counts=sp.counts, totals=sp.totals, n_neutral=sp.n_neutral, n_bc=sp.n_bc, env_idx=[0, 1, 2, 1, 2])
    if case == "multienv_env0_matrix_prior":                     # (identity only) the same with a Matrix-form s_bc prior
        sp, g = spec("multienv_env0_only_first"), np.random.default_rng(4)
        n = sp.n_bc * sp.n_env
        return ModelSpec(kind=sp.kind, counts=sp.counts, totals=sp.totals, n_neutral=sp.n_neutral, n_bc=sp.n_bc, env_idx=sp.env_idx,
                         priors=dict(s_bc_prior=(g.normal(0.0, 1.0, n), g.uniform(0.3, 3.0, n))))
    if case == "fitness_chunk":                                  # B = 300 crosses the 256-column chunk of the normalisers
        return fixtures.synthetic("fitness", B=300, T=3, n_neutral=20, seed=3)
    if case == "fitness_matrix_prior":                           # (identity only) a Matrix-form s_bc prior
        g = np.random.default_rng(2)
        return fixtures.synthetic("fitness", B=30, T=4, n_neutral=5, seed=3, s_bc_prior=(g.normal(0.0, 1.0, 25), g.uniform(0.5, 3.0, 25)))
    raise KeyError(case)


def all_cases():
    return sorted(pc.CASES) + list(NEW_CASES)


def golden_cases():
    out = {f"{c}_n{n}": (c, n, None) for c in all_cases() for n in NS}
    out.update(BIG)
    return out


def golden_path(name):
    return os.path.join(GOLD, f"rb_{name}.npz")


def n_env(sp):
    return sp.n_env if sp.kind in ("multienv", "multienv_replicate") else 1


def n_units(sp):
    return sp.n_rep * sp.n_bc * n_env(sp)


def env_of(sp, r, t):
    """Environment of the LATER time point of step t."""
    return sc._env(sp, r, t)


# ---- parameters -----------------------------------------------------------------------------------------------------------------
def params(sp, seed=PSEED):
    """(mu, omega): `_score_cases.params` (a posterior that roughly explains the data, posterior sd 0.03) with the loglambda means
    at ln(count + 1/2), so that the steps gamma_t are the data's, and every seventh mutant's logsigma_bc at -2.3: conditionals five
    times as sharp, the tails of p_pos / p_neg out to |z| near 15."""
    mu, om = sc.params(sp, seed)
    off = sp.offsets()
    lo = off["loglambda"][0]
    for cnt in sp.counts:                                         # flat: replicate slabs, (r, t, b) at slab + b T + t
        T, B = cnt.shape
        mu[lo:lo + T * B] = np.log(cnt.T.astype(np.float64) + 0.5).reshape(-1)
        lo += T * B
    ls = mu[slice(*off["logsigma_bc"])]
    E = n_env(sp)
    per = ls.reshape(-1, sp.n_bc, E) if sp.kind != "genotype" else ls.reshape(1, sp.n_bc, 1)
    per[:, 3::7, :] = -2.3
    return mu, om


@functools.lru_cache(maxsize=None)
def inputs(case):
    sp = spec(case)
    mu, om = params(sp)
    mu.setflags(write=False)
    om.setflags(write=False)
    return sp, mu, om


# ---- the restatement ----------------------------------------------------------------------------------------------------------
class Rows:
    """Explicit draws [n, D]: latent i's draws are column i."""

    def __init__(self, draws):
        self.x = np.ascontiguousarray(draws, dtype=np.float64)

    def __call__(self, i):
        return self.x[:, int(i)]


def conditionals(sp, D, n, mutants=None):
    """(s, m, sd) [n_units, n] and n_steps [n_units] from the draws D(i) -> [n] of the caller's latents: the header's formulas.
    `mutants`: only these mutants' units are filled."""
    off = sp.offsets()
    B, nb, nn, R = sp.B, sp.n_bc, sp.n_neutral, sp.n_rep
    E = n_env(sp)
    hier = sp.kind in HIER
    pm, ps = sp.prior_arrays()
    nu_ = n_units(sp)
    s = np.empty((nu_, n))
    m = np.empty((nu_, n))
    sd = np.empty((nu_, n))
    nst = np.zeros(nu_, dtype=np.int32)
    lo_l, g0 = off["loglambda"][0], 0
    for r in range(R):
        T = sp.n_time[r]
        ll = lambda b, t: D(lo_l + b * T + t)
        logZ = []
        for t in range(T):                                        # chunks of 256 columns in index order, then the chunks in order
            Z = None
            for b0 in range(0, B, 256):
                part = np.zeros(n)
                for b in range(b0, min(b0 + 256, B)):
                    part = part + np.exp(ll(b, t))
                Z = part if Z is None else Z + part
            logZ.append(np.log(Z))
        sbar = [D(off["s_pop"][0] + g0 + t) for t in range(T - 1)]
        for mm in (range(nb) if mutants is None else mutants):
            b = nn + mm
            y = np.zeros((E, n))
            cnt = [0] * E
            for t in range(T - 1):
                e = env_of(sp, r, t)
                gam = (ll(b, t + 1) - ll(b, t)) - (logZ[t + 1] - logZ[t])
                y[e] = y[e] + (gam + sbar[t])
                cnt[e] += 1
            for e in range(E):
                em = e + E * mm
                u = em + E * nb * r
                if not hier:
                    i = off["s_bc"][0] + em
                    sj, a, ib2 = D(i), np.full(n, pm[i]), np.full(n, 1.0 / (ps[i] * ps[i]))
                    ls, tau = D(off["logsigma_bc"][0] + em), None
                else:
                    th = int(sp.geno_idx[mm]) if sp.kind == "genotype" else em
                    uu = mm if sp.kind == "genotype" else u
                    a = D(off["theta"][0] + th)
                    tau = np.exp(D(off["logtau"][0] + uu))
                    sj = a + tau * D(off["theta_tilde"][0] + uu)
                    ib2 = 1.0 / (tau * tau)
                    ls = D(off["logsigma_bc"][0] + uu)
                if cnt[e] == 0:
                    m[u], sd[u] = a, (tau if hier else 1.0 / np.sqrt(ib2))
                else:
                    w = np.exp(-2.0 * ls)
                    P = ib2 + cnt[e] * w
                    m[u], sd[u] = (a * ib2 + w * y[e]) / P, 1.0 / np.sqrt(P)
                s[u] = sj
                nst[u] = cnt[e]
        lo_l += T * B
        g0 += T - 1
    return s, m, sd, nst


def mixture_cdf(x, m, sd):
    from scipy.special import erfc
    return (0.5 * erfc(-((x - m) / sd * math.sqrt(0.5)))).sum() / m.shape[0]


def unit64(s, m, sd, threshold, probs):
    """The outputs of one unit from its float64 (s_j, m_j, sd_j), the header's formulas as they stand."""
    from scipy.special import erfc
    n = m.shape[0]
    qm, rm = s.sum() / n, m.sum() / n
    v = (m - threshold) / sd * math.sqrt(0.5)
    out = [qm, math.sqrt(((s - qm) ** 2).sum() / n), rm, math.sqrt((sd * sd).sum() / n + ((m - rm) ** 2).sum() / n),
           (0.5 * erfc(-v)).sum() / n, (0.5 * erfc(v)).sum() / n]
    qs = []
    lo0, hi0 = m.min() - 40.0 * sd.max(), m.max() + 40.0 * sd.max()
    for p in probs:
        if not (np.isfinite(lo0) and np.isfinite(hi0)):
            qs.append(np.nan)
            continue
        lo, hi = lo0, hi0
        for _ in range(64):
            x = lo + (hi - lo) / 2.0
            if mixture_cdf(x, m, sd) < p:
                lo = x
            else:
                hi = x
        qs.append(lo + (hi - lo) / 2.0)
    return out, qs


def restate(sp, mu, omega, n, seed, threshold=THRESHOLD, probs=PROBS, draws=None, units=None, unit=unit64, want_z=False):
    """bb_fitness_rb at (mu, omega) -- or at the explicit `draws` [n, D] -- for `units` (all): a dict as Engine.fitness_rb returns,
    the units' entries only.  `unit`: the evaluation of one unit (the golden generator passes its 50-digit one)."""
    with np.errstate(all="ignore"):
        D = Rows(draws) if draws is not None else sc.Draws(seed, mu, pc.softplus(omega), n)
        s, m, sd, nst = conditionals(sp, D, n)
        units = np.arange(n_units(sp)) if units is None else np.asarray(units)
        out = {k: np.empty(len(units)) for k in UNITS}
        out["quantiles"] = np.empty((len(units), len(probs)))
        out["n_steps"] = nst[units]
        if want_z:
            out["zmax"] = np.array([np.abs((m[u] - threshold) / sd[u]).max() for u in units])
        for x, u in enumerate(units):
            vals, qs = unit(s[u], m[u], sd[u], threshold, probs)
            for k, v in zip(UNITS, vals):
                out[k][x] = float(v)
            out["quantiles"][x] = [float(q) for q in qs]
    return out


def materialise(sp, mu, omega, n, seed):
    """The draws [n, D] the library makes from (mu, omega) at `seed`, on the host (`_ppc_cases._param`)."""
    sig = pc.softplus(omega)
    j = np.arange(n, dtype=np.uint64)
    return np.stack([pc._param(seed, mu, sig, i, j) for i in range(sp.D)], axis=1)


@functools.lru_cache(maxsize=None)
def golden(name):
    with np.load(golden_path(name)) as f:
        g = {k: f[k] for k in f.files}
    for v in g.values():
        v.setflags(write=False)
    return g


# ---- comparison -----------------------------------------------------------------------------------------------------------------
def errors(got, ref):
    """Largest error per output under the rule of the module docstring; the NaN pattern and n_steps must be equal."""
    err = {}
    for k in UNITS + ("quantiles",):
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
    assert np.array_equal(got["n_steps"], ref["n_steps"])
    return err


def assert_within(err, who):
    for k in UNITS:
        assert err[k] <= TOL, (who, k, err[k])
    assert err["quantiles"] <= QTOL, (who, "quantiles", err["quantiles"])


def take(res, units):
    return res if units is None else {k: v[list(units)] for k, v in res.items()}


def report(name, label, err):
    print(f"rb case {name:36s} {label:12s} " + " ".join(f"{k} {err[k] / 1e-16:7.1f}" for k in UNITS + ("quantiles",)) + "  (1e-16)")


def same_bytes(a, b):
    return set(a) == set(b) and all(np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes() for k in a)


def rb(e, n, **kw):
    kw.setdefault("probs", PROBS)
    kw.setdefault("threshold", THRESHOLD)
    kw.setdefault("seed", SEED)
    return e.fitness_rb(n_samples=n, **kw)


# ---- 1. the identity against the log-joint -----------------------------------------------------------------------------------------
IDENTITY = all_cases() + ["fitness_matrix_prior", "multienv_env0_matrix_prior", "replicate_ragged_method"]


def check_identity(lib, name, device=False):
    """At 3 random points, each passed as one explicit draw: P (m - s) (times tau for the hierarchical kinds) from rb_mean, rb_sd
    and q_mean against the literal oracle's gradient entries of the s_bc / theta_tilde block (and, device, against
    Engine.logdensity_grad), at `_logp_cases`' tolerance for a gradient: 1e-9 of the largest entry -- here of the block alone."""
    from oracle import literal
    quirk = name == "replicate_ragged_method"
    sp = spec("replicate_ragged" if quirk else name)
    off = sp.offsets()
    hier = sp.kind in HIER
    blk = slice(*off["theta_tilde" if hier else "s_bc"])
    g = np.random.default_rng(8)
    kw = dict(ragged_method=True) if quirk else {}
    with make_engine(sp, lib, seed=1, use_priors=name.endswith("matrix_prior"), **kw) as e:
        assert e.fitness_rb_shape() == n_units(sp) == blk.stop - blk.start
        for scale in (0.3, 1.0, 0.3):                             # drawn as in _logp_cases.spec
            z = g.normal(0.0, scale, sp.D)
            got = e.fitness_rb(probs=(), draws=z)
            ref = restate(sp, None, None, 1, 0, probs=(), draws=z[None, :])
            P = 1.0 / got["rb_sd"] ** 2
            lhs = P * (got["rb_mean"] - got["q_mean"])
            if hier:
                lhs = lhs * np.exp(z[slice(*off["logtau"])])
            grad = literal.logjoint_and_grad(z, sp, **(dict(ragged_quirk=True) if quirk else {}))[1][blk]
            scale_g = np.abs(grad).max()
            err = np.abs(lhs - grad).max() / scale_g
            r64 = 1.0 / ref["rb_sd"] ** 2 * (ref["rb_mean"] - ref["q_mean"]) * (np.exp(z[slice(*off["logtau"])]) if hier else 1.0)
            print(f"rb identity {name:28s} sd {scale}: library {err:.2e}, restatement {np.abs(r64 - grad).max() / scale_g:.2e} of max |g| = {scale_g:.3g}")
            assert err <= 1e-9
            assert np.all(got["q_sd"] == 0.0) and (hier or np.array_equal(got["q_mean"], z[blk]))
            assert np.array_equal(got["n_steps"], ref["n_steps"])
            if device:
                gd = e.logdensity_grad(z)[1][blk]
                assert np.abs(lhs - gd).max() <= 1e-9 * np.abs(gd).max()
            if name.startswith("multienv_env0"):                  # n_u = 0: the prior (mean, std)
                u0 = np.arange(0, n_units(sp), n_env(sp))
                assert np.all(got["n_steps"][u0] == 0) and np.all(got["n_steps"][u0 + 1] == 2)
                pm, ps = (np.asarray(v, dtype=np.float64) * np.ones(n_units(sp)) for v in sp.priors["s_bc_prior"])
                assert np.array_equal(got["rb_mean"][u0], pm[u0])                                  # the mean exactly
                if name == "multienv_env0_only_first":            # the default (0, 2): the std exactly too
                    assert np.all(pm[u0] == 0.0) and np.all(got["rb_sd"][u0] == 2.0)
                else:                                             # Matrix form: the handle holds 1 / std^2, and 1 / sqrt of it is std to an ulp
                    assert np.all(np.abs(got["rb_sd"][u0] - ps[u0]) <= np.spacing(ps[u0])) and len(set(ps[u0])) == len(u0)


# ---- 2. golden values ----------------------------------------------------------------------------------------------------------
def check_golden(lib, name, label):
    case, n, units = golden_cases()[name]
    sp, mu, om = inputs(case)
    ref = golden(name)
    e0 = errors(restate(sp, mu, om, n, SEED, units=units), ref)
    report(name, "restatement", e0)
    with pc._handle(lib, sp, mu, om) as e:
        got = rb(e, n)
    assert got["quantiles"].shape == (n_units(sp), len(PROBS)) and np.all(np.diff(got["quantiles"], axis=1) > 0)
    err = errors(take(got, units), ref)
    report(name, label, err)
    assert_within(e0, "restatement")
    assert_within(err, label)
    return got


def check_z_range(name):
    """The parameters keep every conditional within 20 of its sds of the threshold; the hierarchical cases reach 10 .. 12 (CPU, the
    restatement)."""
    case, n, units = golden_cases()[name]
    sp, mu, om = inputs(case)
    z = restate(sp, mu, om, n, SEED, probs=(), units=units, want_z=True)["zmax"]
    assert z.max() <= Z_HI, z.max()
    assert z.max() >= Z_REACH.get(name, 0.0), z.max()


def check_many_quantiles(lib, case="multienv", n=111):
    """4 and 8 quantiles (two and three sweeps per bisection step, the last one partly filled) against the float64 restatement,
    itself within Q_MEASURED of the 50-digit root: QTOL; the first three columns are the goldens' probabilities and values."""
    sp, mu, om = inputs(case)
    p8 = PROBS + (0.001, 0.16, 0.84, 0.999, 0.3)
    with pc._handle(lib, sp, mu, om) as e:
        base = rb(e, n)
        for probs in (p8[:4], p8):
            got = rb(e, n, probs=probs)
            ref = restate(sp, mu, om, n, SEED, probs=probs)
            err = errors(got, ref)
            report(f"{case}_n{n}_q{len(probs)}", "vs restated", err)
            assert_within(err, f"{len(probs)} quantiles")
            assert same_bytes({k: v for k, v in got.items() if k != "quantiles"}, {k: v for k, v in base.items() if k != "quantiles"})
            assert np.array_equal(got["quantiles"][:, :3], base["quantiles"])
            order = np.argsort(probs)
            assert np.all(np.diff(got["quantiles"][:, order], axis=1) > 0)


# ---- 3. determinism ------------------------------------------------------------------------------------------------------------
def check_launch_modes(lib, case="replicate_ragged"):
    import barbay_jl_amd as bb
    sp, mu, om = inputs(case)
    out = []
    for mode in (1, 0):
        with bb.Engine(sp.kind, sp.counts, sp.n_neutral, sp.n_bc, env_idx=sp.env_idx, geno_idx=sp.geno_idx, seed=4, launch_mode=mode, _lib=lib) as e:
            e.set_params(mu, om)
            out.append(rb(e, 500, seed=2))
            out.append(rb(e, 500, seed=2))
    assert all(same_bytes(out[0], o) for o in out[1:])


def check_group_handle(lib, case):
    sp, mu, om = inputs(case)
    with pc._handle(lib, sp, mu, om, device_ids=[0, 0]) as e:
        a = rb(e, 111)
    with pc._handle(lib, sp, mu, om) as e:
        b = rb(e, 111)
    assert same_bytes(a, b)


def check_buffer_reuse(lib):
    """The call interleaved with the other post-fit calls at changing sizes on one handle (the buffer regrows and is reused
    stale): every result is byte for byte what a fresh handle gives."""
    sp, mu, om = inputs("fitness")
    om = np.minimum(om, -2.0)
    qs = (0.95, 0.675, 0.05)
    chain = np.random.default_rng(12).standard_normal((2, 5, 6))
    dr = materialise(sp, mu, om, 7, 3)
    calls = [lambda e: rb(e, 111),
             lambda e: e.ppc_bands(qs, n_samples=111, n_ppc=7, seed=SEED),
             lambda e: rb(e, 1000),
             lambda e: e.freq_bands(qs, mode="posterior", n_samples=200, n_ppc=1, seed=SEED),
             lambda e: rb(e, 2),
             lambda e: e.chain_summary(chain),
             lambda e: e.ppc_score(n_samples=111, seed=SEED),
             lambda e: rb(e, 7, draws=dr),
             lambda e: rb(e, 2049, probs=(0.5,)),
             lambda e: rb(e, 111)]
    with pc._handle(lib, sp, mu, om) as e:
        got = [pc._bits(f(e)) for f in calls]
    for i, f in enumerate(calls):
        with pc._handle(lib, sp, mu, om) as e:
            assert got[i] == pc._bits(f(e)), i
    assert got[0] == got[9]


def check_handle_untouched(lib):
    sp = spec("fitness")
    with make_engine(sp, lib, seed=5) as a, make_engine(sp, lib, seed=5) as b:
        rb(b, 111)
        for x, y in zip(a.get_params(), b.get_params()):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
        a.run(5)
        rb(b, 64, seed=1)
        b.run(5)
        for x, y in zip(a.get_params(), b.get_params()):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64))


def check_internal_against_explicit_draws(lib, case, n=111):
    """The library's own draws against the same draws made on the host and passed in: within the bounds of the goldens (numpy's
    Box-Muller step and the library's differ by ulps, so not the bytes)."""
    sp, mu, om = inputs(case)
    dr = materialise(sp, mu, om, n, SEED)
    with pc._handle(lib, sp, mu, om) as e:
        a = rb(e, n)
        b = rb(e, n, draws=dr)
        c = rb(e, 5, draws=dr)                                    # n_samples is the row count; the argument is ignored
    assert same_bytes(b, c)
    err = errors(a, b)
    report(case + f"_n{n}", "own/explicit", err)
    assert_within(err, "explicit draws")


# ---- 4. non-finite values and errors ---------------------------------------------------------------------------------------------
def check_nan_parameter(lib, case="multienv", n=111):
    """One mutant's logsigma_bc means NaN: its units' conditionals are NaN (the draws' own fitness and n_steps are not), every other
    unit keeps its bytes."""
    sp, mu, om = inputs(case)
    E, m = n_env(sp), 7
    mu2 = mu.copy()
    lo = sp.offsets()["logsigma_bc"][0]
    mu2[lo + E * m:lo + E * (m + 1)] = np.nan
    with pc._handle(lib, sp, mu, om) as e:
        base = rb(e, n)
    with pc._handle(lib, sp, mu2, om) as e:
        got = rb(e, n)
    bad = np.arange(E * m, E * (m + 1))
    rest = np.setdiff1d(np.arange(n_units(sp)), bad)
    assert same_bytes({k: v[rest] for k, v in got.items()}, {k: v[rest] for k, v in base.items()})
    for k in ("rb_mean", "rb_sd", "p_pos", "p_neg", "quantiles"):
        assert np.all(np.isnan(got[k][bad])), k
    keep = ("q_mean", "q_sd", "n_steps")
    assert same_bytes({k: got[k][bad] for k in keep}, {k: base[k][bad] for k in keep})


def raw_rb(engine, n_samples, probs=PROBS, threshold=THRESHOLD, seed=SEED, draws=None, null=(), want=UNITS + ("quantiles", "n_steps"),
           n_quantiles=None):
    """bb_fitness_rb through ctypes with only the outputs in `want` non-NULL; `null` names arguments passed as NULL (h, o, out, probs)."""
    nu = engine.fitness_rb_shape()
    p = np.ascontiguousarray(probs, dtype=np.float64)
    o = _capi.bb_rb_opts()
    o.n_samples, o.n_quantiles, o.threshold, o.seed = n_samples, len(p) if n_quantiles is None else n_quantiles, threshold, seed
    o.probs = None if "probs" in null or not len(p) else _capi._ptr(p)
    if draws is not None:
        o.draws = _capi._ptr(draws)
    res, out = {}, _capi.bb_rb_out()
    for k in want:
        if k == "n_steps":
            res[k] = np.full(nu, -7, dtype=np.int32)
            out.n_steps = res[k].ctypes.data_as(C.POINTER(C.c_int32))
        else:
            res[k] = np.full((nu, len(p)) if k == "quantiles" else nu, -7.0)
            setattr(out, k, _capi._ptr(res[k]))
    rc = engine._lib.bb_fitness_rb(None if "h" in null else engine._h, None if "o" in null else C.byref(o),
                                   None if "out" in null else C.byref(out))
    return rc, res


def check_errors(lib):
    """Every BB_ERR_INVALID and BB_ERR_UNSUPPORTED of the contract, with a message.  NOT exercised: BB_ERR_DEVICE for draws the
    device cannot allocate -- provoking it takes an allocation of the device's whole memory, which a test on a shared machine
    does not do; the path is DevBuf::grow's, the one every post-fit call's buffer goes through."""
    sp, mu, om = inputs("fitness")
    INVALID, UNSUPPORTED = -1, _capi.BB_ERR_UNSUPPORTED
    msg = lambda: lib.bb_last_error().decode()
    dr = materialise(sp, mu, om, 3, 1)
    with pc._handle(lib, sp, mu, om) as e:
        for null in ("h", "o", "out"):
            assert raw_rb(e, 10, null=(null,))[0] == INVALID and msg(), null
        for nq in (-1, 9):
            assert raw_rb(e, 10, n_quantiles=nq)[0] == INVALID and "n_quantiles" in msg(), nq
        assert raw_rb(e, 10, null=("probs",), n_quantiles=3)[0] == INVALID and "probs" in msg()
        for bad in (0.0, 1.0, -0.1, 1.5, np.nan):
            assert raw_rb(e, 10, probs=(0.5, bad))[0] == INVALID and "prob" in msg(), bad
        for bad in (np.inf, -np.inf, np.nan):
            assert raw_rb(e, 10, threshold=bad)[0] == INVALID and "threshold" in msg(), bad
        for n in (1, 0, -3, MAXN + 1):
            assert raw_rb(e, n)[0] == UNSUPPORTED and "n_samples" in msg(), n
        for n in (0, MAXN + 1):
            assert raw_rb(e, n, draws=dr)[0] == UNSUPPORTED and "n_samples" in msg(), n
        assert raw_rb(e, 1, draws=dr)[0] == 0 and raw_rb(e, 3, draws=dr)[0] == 0      # one explicit draw is served
        assert raw_rb(e, 64, want=())[0] == 0                                          # an all-NULL out
        assert raw_rb(e, 64, probs=())[0] == 0                                         # no quantiles
        full = rb(e, 64)
        assert same_bytes(raw_rb(e, 64)[1], full)
        for k in UNITS + ("quantiles", "n_steps"):                                     # every output NULL except one
            rc, one = raw_rb(e, 64, want=(k,))
            assert rc == 0 and same_bytes(one, {k: full[k]}), k
        try:
            e.fitness_rb(n_samples=1)
        except _capi.BarBayHipError as ex:
            assert "error -4" in str(ex) and "n_samples" in str(ex)
        else:
            raise AssertionError("no error")
        try:
            e.fitness_rb(draws=np.zeros((3, sp.D + 1)))
        except _capi.BarBayHipError as ex:
            assert "draws" in str(ex)
        else:
            raise AssertionError("no error")
