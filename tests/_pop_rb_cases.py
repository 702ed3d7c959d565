"""bb_popmean_rb (Rao-Blackwellised population-mean fitness marginals, barbay.jl_amd/csrc/bb_rb.h) restated in numpy from the formulas
of include/barbay_hip.h, and the cases the emulation and GPU tests share.  The draws, their keying, the normalisers and the mixture
of a group's conditionals are `_rb_cases`'; the new part is the sum over every barcode of a replicate by the chunk rule, and the
ragged method's pairing of the neutral members.

Expected values: tests/golden/pop_rb_<case>_n<samples>.npz, a 50-digit mpmath evaluation of `_rb_cases.unit64`'s formulas on this
restatement's float64 (sbar_j, m_j, sd_j), written by tests/golden/make_pop_rb_golden.py.  Bounds, in `_rb_cases`' sense (relative to
max(|x|, 1); to the value itself for p_pos, p_neg): the larger of 1e-12 and 8 x the float64 restatement's own measured error against
the goldens (MEASURED / Q_MEASURED below; the project's standing margin).  Thresholds: the conditional of a population mean is sharp
(every barcode of the replicate informs it), so the threshold is chosen per group, the multiple of STEP nearest the group's rb_mean
(stored in the golden file): the library is called once per distinct threshold, a group's p_pos / p_neg are taken from the call at
its threshold, and everything that does not depend on the threshold must come out of all those calls with the same bytes.
`check_z_range` checks |m_j - s0| / sd_j <= 20 on the CPU, as the generator does before it writes a file (the cases reach 12.4:
the sharpest group has sd 0.008, and half a step of the grid is 0.05).

Measured, largest error over a case's groups against the golden, float64 restatement / host emulation / MI355X, in units of 1e-16
(each test prints its own line; the device run is kept in profiles/popmean_rb/gpu_pop_rb_tests.log, the table in errors.txt there):

case                                                 q_mean               q_sd            rb_mean              rb_sd              p_pos              p_neg          quantiles
fitness_b256_n1000                  1.1/  0.6/  0.6    0.0/  0.0/  0.0    0.0/  0.6/  0.6    0.0/  0.1/  0.1    0.0/  2.3/  5.1    2.1/ 23.4/ 14.9    0.6/  0.6/  0.6
fitness_b256_n111                   1.1/  0.6/  0.6    0.0/  0.1/  0.1    0.6/  1.7/  1.7    0.0/  0.3/  0.3    2.3/ 11.7/ 13.3    1.7/ 26.6/ 19.9    0.6/  2.2/  2.2
fitness_b256_n2                     0.0/  0.6/  0.6    0.0/  0.3/  0.3    0.0/  1.1/  1.1    0.0/  0.9/  1.4    1.1/ 26.7/ 13.4    1.5/264.3/182.1    0.6/  2.2/  2.8
fitness_b257_n1000                  0.6/  1.1/  1.1    0.0/  0.0/  0.0    0.0/  0.6/  0.6    0.0/  0.1/  0.0    1.3/ 36.2/ 31.0    0.0/ 18.4/ 14.7    0.6/  1.1/  1.1
fitness_b257_n111                   0.6/  1.7/  1.7    0.0/  0.1/  0.1    0.6/  1.1/  1.1    0.0/  0.2/  0.2    1.5/ 19.9/ 10.7    3.5/  5.3/  3.5    1.1/  1.1/  1.1
fitness_b257_n2                     0.0/  0.0/  0.0    0.0/  0.0/  0.0    0.0/  0.0/  1.1    0.0/  0.3/  0.3   21.6/ 37.8/ 43.2    1.4/ 82.6/ 32.2    0.6/  1.7/  1.1
fitness_b600_n1000                  0.6/  1.1/  1.1    0.1/  0.1/  0.1    0.0/  1.1/  1.1    0.0/  0.1/  0.1    0.0/  1.5/  9.3    1.4/  5.8/ 11.6    0.6/  2.2/  1.1
fitness_b600_n111                   1.7/  1.1/  1.1    0.0/  0.1/  0.1    0.6/  0.6/  0.6    0.0/  0.1/  0.1    1.8/  7.7/  6.4    2.1/ 19.1/ 19.1    1.1/  1.1/  1.1
fitness_b600_n2                     0.0/  0.0/  0.0    0.0/  0.0/  0.0    0.0/  1.1/  0.0    0.0/  0.0/  0.1   13.4/139.1/253.0    1.9/114.2/ 40.6    0.6/  1.1/  0.6
fitness_n1000                       1.1/  1.1/  1.1    0.1/  0.1/  0.1    1.1/  3.3/  3.3    0.1/  0.1/  0.1    1.6/  3.6/  6.3    0.0/  5.5/  5.5    1.1/  2.2/  2.2
fitness_n111                        1.1/  2.2/  2.2    0.0/  0.1/  0.1    1.1/  3.3/  3.3    0.1/  0.3/  0.6    1.4/  6.1/  6.1    2.6/ 12.2/ 14.3    3.3/  2.2/  4.4
fitness_n2                          0.0/  0.6/  0.6    0.0/  0.3/  0.3    0.0/  2.2/  1.1    0.0/  0.8/  1.1    1.3/ 14.9/108.8    2.6/153.1/113.5    1.1/  3.3/  2.2
genotype_b600_n1000                 0.6/  1.7/  1.7    0.0/  0.0/  0.0    0.6/  1.7/  1.7    0.0/  0.1/  0.0    1.2/  4.7/  1.2    0.0/  2.2/  4.4    1.1/  1.1/  1.1
genotype_b600_n111                  0.0/  1.1/  1.1    0.0/  0.1/  0.1    1.1/  1.1/  2.2    0.0/  0.1/  0.1    1.4/  1.4/  4.1    1.9/  7.8/ 15.6    1.1/  1.1/  1.7
genotype_b600_n2                    0.0/  0.0/  0.0    0.0/  0.0/  0.0    0.0/  0.0/  0.6    0.0/  0.0/  0.1    0.0/101.4/185.1    0.0/ 11.1/ 21.0    1.1/  1.1/  1.1
genotype_regrouped_n1000            1.1/  3.3/  3.3    0.0/  0.1/  0.1    1.1/  2.2/  2.2    0.0/  0.2/  0.3    1.3/  4.1/  7.7    2.0/  2.2/  2.0    1.1/  1.1/  1.1
genotype_regrouped_n111             1.1/  3.3/  3.3    0.0/  0.1/  0.1    1.1/  2.2/  2.2    0.1/  0.2/  0.3    2.8/  7.5/  9.8    1.8/  3.7/  9.2    2.2/  6.7/  6.7
genotype_regrouped_n2               0.0/  0.0/  0.0    0.0/  0.6/  0.6    0.0/  2.2/  2.2    0.0/  0.3/  0.4    1.4/155.4/163.9    0.0/ 53.4/ 32.2    1.1/  3.3/  3.3
multienv_n1000                      1.1/  1.1/  1.1    0.1/  0.1/  0.1    1.1/  2.2/  1.1    0.1/  0.2/  0.1    0.0/  5.3/  8.9    3.0/  4.8/  4.8    2.2/  3.3/  3.3
multienv_n111                       1.1/  3.3/  3.3    0.1/  0.1/  0.1    1.1/  2.2/  2.2    0.1/  0.2/  0.1    1.9/  5.8/ 11.6    3.4/  4.3/  8.5    3.3/  1.1/  1.1
multienv_n2                         0.0/  0.6/  0.6    0.0/  0.6/  0.6    0.0/  2.2/  2.2    0.1/  0.9/  1.4    0.0/  8.5/ 18.8    1.7/ 15.9/ 34.9    1.1/  2.2/  4.4
multienv_replicate_n1000            1.1/  1.1/  1.1    0.1/  0.1/  0.1    2.1/  2.2/  2.2    0.1/  0.3/  0.1    1.7/  4.3/  5.2    2.5/  5.1/  6.5    2.0/  3.3/  3.3
multienv_replicate_n111             2.2/  2.2/  2.2    0.1/  0.1/  0.1    2.2/  6.3/  3.3    0.1/  0.4/  0.3    3.1/  6.9/ 12.5    3.7/  5.8/  5.6    3.3/  4.4/  4.1
multienv_replicate_n2               0.0/  0.0/  0.0    0.0/  0.0/  0.0    0.0/  2.2/  2.2    0.1/  1.0/  1.5    1.6/ 24.0/ 25.5    7.4/ 16.5/ 50.5    2.2/  2.2/  4.1
replicate_ragged_method_n1000       1.1/  2.2/  2.2    0.1/  0.1/  0.1    1.1/  4.4/  3.3    0.1/  0.3/  0.1    1.8/  5.2/  3.8    1.7/  4.4/  5.2    2.2/  5.6/  5.6
replicate_ragged_method_n111        1.1/  3.3/  3.3    0.0/  0.1/  0.1    3.3/  5.6/  5.6    0.1/  0.3/  0.4    3.4/ 12.0/ 12.0    2.2/  9.7/  9.7    4.3/  7.8/  7.8
replicate_ragged_method_n2          0.0/  0.0/  0.0    0.0/  0.0/  0.0    0.0/  2.2/  3.3    0.1/  0.6/  1.9    2.0/ 20.1/ 52.0    1.5/ 41.2/ 90.6    1.1/  3.3/  5.6
replicate_ragged_n1000              1.1/  2.2/  2.2    0.1/  0.1/  0.1    1.1/  3.3/  2.2    0.1/  0.3/  0.1    2.0/  4.4/  5.3    2.0/  6.7/  5.0    2.2/  4.4/  4.4
replicate_ragged_n111               1.1/  3.3/  3.3    0.0/  0.1/  0.1    2.2/  3.3/  3.3    0.1/  0.3/  0.4    4.6/ 13.6/ 12.9    3.3/ 11.6/ 11.6    6.3/  8.9/  8.9
replicate_ragged_n2                 0.0/  0.0/  0.0    0.0/  0.0/  0.0    0.0/  1.1/  2.2    0.1/  0.3/  1.0    1.2/ 25.6/ 65.8    1.9/ 38.9/ 75.9    1.1/  2.2/  4.4
replicate_ragged_n8672              0.6/  1.1/  1.1    0.0/  0.1/  0.1    1.1/  2.2/  2.2    0.0/  0.1/  0.1    1.7/  3.3/  3.4    2.2/  1.9/  2.2    1.1/  5.6/  5.6
(the largest entry of the first six columns, 264.3e-16, is 0.0264 of the bound 1e-12; the largest quantile entry, 8.9e-16,
 is 0.0009 of QTOL = 1e-12; the restatement's own largest are 2.2e-15 and 6.3e-16, 8 x which is below 1e-12 in both)
Chunk rule (`check_chunk_rule`, fitness_b600 at n = 111 with explicit draws, against the float64 restatement, no golden), emulation / MI355X:
q_mean 2.8/2.8 q_sd 0.1/0.1 rb_mean 1.1/0.0 rb_sd 0.1/0.1 p_pos 5.4/10.8 p_neg 8.5/12.7 quantiles 2.2/2.2.
Chunk rule (`check_chunk_rule`, genotype_b600 at n = 111 with explicit draws, against the float64 restatement, no golden), emulation / MI355X:
q_mean 1.1/1.1 q_sd 0.1/0.1 rb_mean 2.8/3.3 rb_sd 0.0/0.2 p_pos 1.4/1.2 p_neg 3.8/15.6 quantiles 1.1/1.1.
"""
import ctypes as C
import functools
import os

import numpy as np

import _ppc_cases as pc
import _rb_cases as rc
import _score_cases as sc
from conftest import make_engine
from barbay_jl_amd import _capi
from oracle.spec import ModelSpec

UNITS = rc.UNITS
CHUNK = _capi.BB_POPMEAN_RB_CHUNK
MEASURED = 2.2e-15        # the float64 restatement's largest error of the six moments and tails against the goldens
Q_MEASURED = 6.3e-16      # ... and of the quantiles
SEED, PROBS, NS, MAXN, Z_HI = rc.SEED, rc.PROBS, rc.NS, rc.MAXN, rc.Z_HI
STEP = 0.1                                                        # a group's tails are taken at the multiple nearest its rb_mean (`nearest`)
SHAPES = tuple(pc.CASES) + ("replicate_ragged_method", "fitness_b256", "fitness_b257", "fitness_b600", "genotype_b600")
BIG = {f"replicate_ragged_n{MAXN}": ("replicate_ragged", MAXN, (0, 5, 12))}
IDENTITY = SHAPES + ("fitness_matrix_prior", "replicate_matrix_prior")


def quirk_of(case):
    return case == "replicate_ragged_method"


@functools.lru_cache(maxsize=None)
def spec(case):
    from oracle import fixtures
    if case in pc.CASES:
        return pc.spec(case)
    if case == "replicate_ragged_method":                         # the same data; the handle is made with BB_FLAG_RAGGED_METHOD
        return pc.spec("replicate_ragged")
    if case.startswith("fitness_b"):                              # a full chunk, a chunk boundary, two full chunks and a remainder
        return fixtures.synthetic("fitness", B=int(case[len("fitness_b"):]), T=3, n_neutral=20, seed=3)
    if case == "genotype_b600":                                   # scattered geno_idx: the caller's order differs from the internal one across chunks
        sp = fixtures.synthetic("genotype", B=600, T=3, n_geno=5, n_neutral=20, seed=3)
        gi = np.random.default_rng(6).integers(0, 5, sp.n_bc)
        first = {}
        gi = np.array([first.setdefault(int(g), len(first)) for g in gi])      # first-appearance numbering, as the host hands it over
        assert len(first) == 5 and np.count_nonzero(np.diff(gi)) > sp.n_bc // 2
        return ModelSpec(kind=sp.kind, counts=sp.counts, totals=sp.totals, n_neutral=sp.n_neutral, n_bc=sp.n_bc, geno_idx=gi)
    if case == "fitness_matrix_prior":                            # (identity only) a Matrix-form s_pop prior: one row per step
        g = np.random.default_rng(2)
        return fixtures.synthetic("fitness", B=30, T=4, n_neutral=5, seed=3, s_pop_prior=(g.normal(0.0, 1.0, 3), g.uniform(0.5, 3.0, 3)))
    if case == "replicate_matrix_prior":                          # (identity only) ... over ragged replicates
        sp, g = pc.spec("replicate_ragged"), np.random.default_rng(4)
        n = n_groups(sp)
        return ModelSpec(kind=sp.kind, counts=sp.counts, totals=sp.totals, n_neutral=sp.n_neutral, n_bc=sp.n_bc,
                         priors=dict(s_pop_prior=(g.normal(0.0, 1.0, n), g.uniform(0.3, 3.0, n))))
    raise KeyError(case)


def golden_cases():
    out = {f"{c}_n{n}": (c, n, None) for c in SHAPES for n in NS}
    out.update(BIG)
    return out


def golden_path(name):
    return os.path.join(rc.GOLD, f"pop_rb_{name}.npz")


def n_groups(sp):
    lo, hi = sp.offsets()["s_pop"]
    return hi - lo


def group_of(sp, r, k):
    return sum(T - 1 for T in sp.n_time[:r]) + k


@functools.lru_cache(maxsize=None)
def inputs(case):
    sp = spec(case)
    mu, om = rc.params(sp)
    mu.setflags(write=False)
    om.setflags(write=False)
    return sp, mu, om


def engine(lib, case, mu=None, om=None, **kw):
    """A handle of the case (flagged for the ragged method's case), at (mu, om) if given."""
    if quirk_of(case):
        kw["ragged_method"] = True
    if mu is None:
        return make_engine(spec(case), lib, **kw)
    return pc._handle(lib, spec(case), mu, om, **kw)


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def conditionals(sp, D, n, groups=None, quirk=False, chunk=CHUNK):
    """(sbar, m, sd) [n_groups, n] from the draws D(i) -> [n] of the caller's latents: the header's formulas, a group's members
    (neutrals, then mutants) summed in chunks of `chunk` consecutive member indices, the chunks in order.  Only `groups` are filled."""
    off = sp.offsets()
    B, nb, nn, R = sp.B, sp.n_bc, sp.n_neutral, sp.n_rep
    E = rc.n_env(sp)
    hier = sp.kind in rc.HIER
    pm, ps = sp.prior_arrays()
    G = n_groups(sp)
    want = set(range(G) if groups is None else (int(g) for g in groups))
    sb, m, sd = np.empty((G, n)), np.empty((G, n)), np.empty((G, n))
    lo_l, g0 = off["loglambda"][0], 0
    for r in range(R):
        T = sp.n_time[r]
        ks = [k for k in range(T - 1) if g0 + k in want]
        ll = lambda b, t: D(lo_l + b * T + t)
        logZ = {}
        for t in (range(T) if quirk else sorted({k + d for k in ks for d in (0, 1)})) if ks else ():
            Z = None                                              # chunks of 256 columns in index order, then the chunks in order
            for b0 in range(0, B, 256):
                part = np.zeros(n)
                for b in range(b0, min(b0 + 256, B)):
                    part = part + np.exp(ll(b, t))
                Z = part if Z is None else Z + part
            logZ[t] = np.log(Z)
        for k in ks:
            g = g0 + k
            e = rc.env_of(sp, r, k)
            wn = np.exp(-2.0 * D(off["logsigma_pop"][0] + g))
            SP, SN = np.zeros(n), np.zeros(n)
            for i0 in range(0, nn + nb, chunk):
                cp, cn = np.zeros(n), np.zeros(n)
                for i in range(i0, min(i0 + chunk, nn + nb)):
                    t, b = k, i
                    if i < nn and quirk:                          # element x of the replicate's time-fastest neutral vector
                        x = k * nn + i
                        t, b = x % (T - 1), x // (T - 1)
                    gam = (ll(b, t + 1) - ll(b, t)) - (logZ[t + 1] - logZ[t])
                    if i < nn:
                        cp = cp + wn
                        cn = cn + -(wn * gam)
                        continue
                    mm = i - nn
                    em = e + E * mm
                    u = em + E * nb * r
                    if not hier:
                        s, ls = D(off["s_bc"][0] + em), D(off["logsigma_bc"][0] + em)
                    else:
                        th = int(sp.geno_idx[mm]) if sp.kind == "genotype" else em
                        uu = mm if sp.kind == "genotype" else u
                        tau = np.exp(D(off["logtau"][0] + uu))
                        s = D(off["theta"][0] + th) + tau * D(off["theta_tilde"][0] + uu)
                        ls = D(off["logsigma_bc"][0] + uu)
                    w = np.exp(-2.0 * ls)
                    cp = cp + w
                    cn = cn + w * (s - gam)
                SP, SN = SP + cp, SN + cn
            i = off["s_pop"][0] + g
            a, ib2 = pm[i], 1.0 / (ps[i] * ps[i])
            P = ib2 + SP
            m[g], sd[g] = (a * ib2 + SN) / P, 1.0 / np.sqrt(P)
            sb[g] = D(i)
        lo_l += T * B
        g0 += T - 1
    return sb, m, sd


def nearest(x):
    """The multiple of STEP nearest to x (elementwise)."""
    return np.round(np.asarray(x) / STEP) * STEP


def restate(sp, mu, omega, n, seed, threshold=0.0, probs=PROBS, draws=None, groups=None, unit=rc.unit64, want_z=False, quirk=False, chunk=CHUNK):
    """bb_popmean_rb at (mu, omega) -- or at the explicit `draws` [n, D] -- for `groups` (all): a dict as Engine.popmean_rb returns,
    plus the thresholds used.  `threshold`: one for all groups, one per group, or None: per group the multiple of STEP nearest to the
    mean of its m_j."""
    with np.errstate(all="ignore"):
        D = rc.Rows(draws) if draws is not None else sc.Draws(seed, mu, pc.softplus(omega), n)
        groups = np.arange(n_groups(sp)) if groups is None else np.asarray(groups)
        sb, m, sd = conditionals(sp, D, n, groups=groups, quirk=quirk, chunk=chunk)
        out = {k: np.empty(len(groups)) for k in UNITS}
        out["quantiles"] = np.empty((len(groups), len(probs)))
        out["n_members"] = np.full(len(groups), sp.n_neutral + sp.n_bc, dtype=np.int32)
        s0 = np.broadcast_to(np.asarray(nearest(m[groups].mean(axis=1)) if threshold is None else threshold, dtype=np.float64), groups.shape)
        out["threshold"] = s0.copy()
        if want_z:
            out["zmax"] = np.array([np.abs((m[g] - s0[x]) / sd[g]).max() for x, g in enumerate(groups)])
        for x, g in enumerate(groups):
            vals, qs = unit(sb[g], m[g], sd[g], float(s0[x]), probs)
            for k, v in zip(UNITS, vals):
                out[k][x] = float(v)
            out["quantiles"][x] = [float(q) for q in qs]
    return out


@functools.lru_cache(maxsize=None)
def golden(name):
    with np.load(golden_path(name)) as f:
        g = {k: f[k] for k in f.files}
    for v in g.values():
        v.setflags(write=False)
    return g


# ---- comparison -----------------------------------------------------------------------------------------------------------------
def errors(got, ref):
    skip = ("threshold", "n_members")
    err = rc.errors({**{k: v for k, v in got.items() if k not in skip}, "n_steps": 0}, {**{k: v for k, v in ref.items() if k not in skip}, "n_steps": 0})
    assert np.array_equal(got["n_members"], ref["n_members"])
    return err


def tolerances():
    return max(1e-12, 8.0 * MEASURED), max(1e-12, 8.0 * Q_MEASURED)


def assert_within(err, who):
    tol, qtol = tolerances()
    for k in UNITS:
        assert err[k] <= tol, (who, k, err[k])
    assert err["quantiles"] <= qtol, (who, "quantiles", err["quantiles"])


def report(name, label, err):
    print(f"pop_rb case {name:34s} {label:12s} " + " ".join(f"{k} {err[k] / 1e-16:7.1f}" for k in UNITS + ("quantiles",)) + "  (1e-16)")


def prb(e, n, **kw):
    kw.setdefault("probs", PROBS)
    kw.setdefault("threshold", 0.0)
    kw.setdefault("seed", SEED)
    return e.popmean_rb(n_samples=n, **kw)


# ---- 1. the identity against the log-joint -----------------------------------------------------------------------------------------
def check_identity(lib, name, device=False):
    """At 3 random points, each passed as one explicit draw: P (m - sbar) from rb_sd, rb_mean, q_mean against the literal oracle's
    gradient over the s_pop block (and, device, against Engine.logdensity_grad): 1e-9 of the block's largest entry."""
    from oracle import literal
    quirk = quirk_of(name)
    sp = spec(name)
    blk = slice(*sp.offsets()["s_pop"])
    g = np.random.default_rng(8)
    with engine(lib, name, seed=1, use_priors=name.endswith("matrix_prior")) as e:
        assert e.popmean_rb_shape() == n_groups(sp) == blk.stop - blk.start
        for scale in (0.3, 1.0, 0.3):                             # drawn as in _logp_cases.spec
            z = g.normal(0.0, scale, sp.D)
            got = e.popmean_rb(probs=(), draws=z)
            ref = restate(sp, None, None, 1, 0, probs=(), draws=z[None, :], quirk=quirk)
            lhs = 1.0 / got["rb_sd"] ** 2 * (got["rb_mean"] - got["q_mean"])
            grad = literal.logjoint_and_grad(z, sp, **(dict(ragged_quirk=True) if quirk else {}))[1][blk]
            scale_g = np.abs(grad).max()
            err = np.abs(lhs - grad).max() / scale_g
            r64 = 1.0 / ref["rb_sd"] ** 2 * (ref["rb_mean"] - ref["q_mean"])
            print(f"pop_rb identity {name:26s} sd {scale}: library {err:.2e}, restatement {np.abs(r64 - grad).max() / scale_g:.2e} of max |g| = {scale_g:.3g}")
            assert err <= 1e-9
            assert np.all(got["q_sd"] == 0.0) and np.array_equal(got["q_mean"], z[blk])
            assert np.array_equal(got["n_members"], ref["n_members"])
            if device:
                gd = e.logdensity_grad(z)[1][blk]
                assert np.abs(lhs - gd).max() <= 1e-9 * np.abs(gd).max()


# ---- 2. golden values ----------------------------------------------------------------------------------------------------------
def at_thresholds(e, n, s0, **kw):
    """popmean_rb with group g's tails taken at s0[g]: one call per distinct threshold; whatever does not depend on the threshold has
    the same bytes in all of them."""
    out = None
    for t in sorted(set(s0.tolist())):
        got = prb(e, n, threshold=t, **kw)
        if out is None:
            out = {k: v.copy() for k, v in got.items()}
        free = [k for k in got if k not in rc.SELF_RELATIVE]
        assert rc.same_bytes({k: got[k] for k in free}, {k: out[k] for k in free}), t
        for k in rc.SELF_RELATIVE:
            out[k][s0 == t] = got[k][s0 == t]
    return out


def check_golden(lib, name, label):
    case, n, groups = golden_cases()[name]
    sp, mu, om = inputs(case)
    ref = golden(name)
    s0 = ref["threshold"]
    ref = {k: v for k, v in ref.items() if k != "threshold"}
    e0 = errors(restate(sp, mu, om, n, SEED, threshold=s0, groups=groups, quirk=quirk_of(case)), ref)
    report(name, "restatement", e0)
    full = np.full(n_groups(sp), s0[0])
    full[slice(None) if groups is None else list(groups)] = s0
    with engine(lib, case, mu, om) as e:
        got = at_thresholds(e, n, full)
    assert got["quantiles"].shape == (n_groups(sp), len(PROBS)) and np.all(np.diff(got["quantiles"], axis=1) > 0)
    err = errors(rc.take(got, groups), ref)
    report(name, label, err)
    assert_within(e0, "restatement")
    assert_within(err, label)


def check_z_range(name):
    """The thresholds keep every group's conditionals within 20 of their sds (CPU, the restatement)."""
    case, n, groups = golden_cases()[name]
    sp, mu, om = inputs(case)
    ref = golden(name)
    z = restate(sp, mu, om, n, SEED, threshold=ref["threshold"], probs=(), groups=groups, want_z=True, quirk=quirk_of(case))["zmax"]
    print(f"pop_rb z range {name}: {z.max():.2f}")
    assert z.max() <= Z_HI, z.max()


# ---- 3. the chunk rule ------------------------------------------------------------------------------------------------------------
def check_chunk_rule(lib, label, n=111):
    """B = 600 (two full chunks and a remainder) on explicit draws: the library against the restatement summed by the chunk rule,
    which another order of the sums does not reproduce; both for the caller's order (fitness) and the regrouped genotype model."""
    for case in ("fitness_b600", "genotype_b600"):
        sp, mu, om = inputs(case)
        dr = rc.materialise(sp, mu, om, n, SEED)
        ref = restate(sp, None, None, n, 0, threshold=None, draws=dr)         # each group's tails at the threshold nearest its rb_mean
        s0 = ref.pop("threshold")
        one = restate(sp, None, None, n, 0, threshold=s0, draws=dr, chunk=10 ** 9)  # all members in one run: another order of the sums
        one.pop("threshold")
        assert not rc.same_bytes(ref, one)
        with engine(lib, case, seed=4) as e:
            got = at_thresholds(e, n, s0, draws=dr)
            if case == "genotype_b600":
                perm = np.asarray(e.permutation())
                assert not np.array_equal(perm, np.arange(perm.shape[0]))     # the library keeps the mutants in another order
        err = errors(got, ref)
        report(case + " explicit", label, err)
        assert_within(err, label)


# ---- 4. determinism ------------------------------------------------------------------------------------------------------------
def check_launch_modes(lib, case="genotype_b600"):
    import barbay_jl_amd as bb
    sp, mu, om = inputs(case)
    out = []
    for mode in (1, 0):
        with bb.Engine(sp.kind, sp.counts, sp.n_neutral, sp.n_bc, env_idx=sp.env_idx, geno_idx=sp.geno_idx, seed=4, launch_mode=mode, _lib=lib) as e:
            e.set_params(mu, om)
            out.append(prb(e, 500, seed=2))
            out.append(prb(e, 500, seed=2))
    assert all(rc.same_bytes(out[0], o) for o in out[1:])


GROUP_CASES = pc.GROUP_CASES


def check_group_handle(lib, case):
    sp, mu, om = inputs(case)
    with pc._handle(lib, sp, mu, om, device_ids=[0, 0]) as e:
        a = prb(e, 111)
    with pc._handle(lib, sp, mu, om) as e:
        b = prb(e, 111)
    assert rc.same_bytes(a, b)


def check_buffer_reuse(lib):
    """The call interleaved with the other post-fit calls at changing sizes on one handle (the buffer regrows and is reused
    stale): every result is byte for byte what a fresh handle gives."""
    sp, mu, om = inputs("genotype_regrouped")
    om = np.minimum(om, -2.0)
    qs = (0.95, 0.675, 0.05)
    chain = np.random.default_rng(12).standard_normal((2, 5, 6))
    dr = rc.materialise(sp, mu, om, 7, 3)
    calls = [lambda e: prb(e, 111),
             lambda e: e.ppc_bands(qs, n_samples=111, n_ppc=7, seed=SEED),
             lambda e: prb(e, 1000),
             lambda e: rc.rb(e, 200),
             lambda e: e.freq_bands(qs, mode="posterior", n_samples=200, n_ppc=1, seed=SEED),
             lambda e: prb(e, 2),
             lambda e: e.theta_rb(n_samples=111, seed=SEED),
             lambda e: e.chain_summary(chain),
             lambda e: e.ppc_score(n_samples=111, seed=SEED),
             lambda e: prb(e, 7, draws=dr),
             lambda e: rc.rb(e, 2049, probs=(0.5,)),
             lambda e: prb(e, 2049, probs=(0.5,)),
             lambda e: prb(e, 111)]
    with pc._handle(lib, sp, mu, om) as e:
        got = [pc._bits(f(e)) for f in calls]
    for i, f in enumerate(calls):
        with pc._handle(lib, sp, mu, om) as e:
            assert got[i] == pc._bits(f(e)), i
    assert got[0] == got[-1]


def check_handle_untouched(lib):
    sp = spec("genotype_regrouped")
    with make_engine(sp, lib, seed=5) as a, make_engine(sp, lib, seed=5) as b:
        prb(b, 111)
        for x, y in zip(a.get_params(), b.get_params()):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
        a.run(5)
        prb(b, 64, seed=1)
        b.run(5)
        for x, y in zip(a.get_params(), b.get_params()):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64))


# ---- 5. own draws against the same draws passed in -----------------------------------------------------------------------------------
def check_internal_against_explicit_draws(lib, case, n=111):
    sp, mu, om = inputs(case)
    dr = rc.materialise(sp, mu, om, n, SEED)
    with engine(lib, case, mu, om) as e:
        s0 = nearest(prb(e, n)["rb_mean"])                  # each group's tails at the threshold nearest its rb_mean
        a = at_thresholds(e, n, s0)
        b = at_thresholds(e, n, s0, draws=dr)
        t0 = float(s0[0])
        assert rc.same_bytes(prb(e, n, threshold=t0, draws=dr), prb(e, 5, threshold=t0, draws=dr))      # n_samples is the row count; the argument is ignored
    err = errors(a, b)
    report(case + f"_n{n}", "own/explicit", err)
    assert_within(err, "explicit draws")


# ---- 6. non-finite values ---------------------------------------------------------------------------------------------------------
RB_KEYS = ("rb_mean", "rb_sd", "p_pos", "p_neg", "quantiles")


def check_nan_in_own_mean(lib, case="replicate_ragged", n=111):
    """A NaN mean of s_pop[g]: q_mean and q_sd of g are NaN; g's conditionals, which do not read sbar_g, and every other group keep
    their bytes."""
    sp, mu, om = inputs(case)
    g = 5
    mu2 = mu.copy()
    mu2[sp.offsets()["s_pop"][0] + g] = np.nan
    with pc._handle(lib, sp, mu, om) as e:
        base = prb(e, n)
    with pc._handle(lib, sp, mu2, om) as e:
        got = prb(e, n)
    assert np.isnan(got["q_mean"][g]) and np.isnan(got["q_sd"][g])
    rest = np.setdiff1d(np.arange(n_groups(sp)), [g])
    assert rc.same_bytes({k: v[rest] for k, v in got.items()}, {k: v[rest] for k, v in base.items()})
    keep = RB_KEYS + ("n_members",)
    assert rc.same_bytes({k: got[k][[g]] for k in keep}, {k: base[k][[g]] for k in keep})
    assert not np.any(np.isnan(got["rb_sd"]))


def check_nan_in_a_mutant(lib, case="multienv_replicate", n=111):
    """One mutant's logsigma_bc mean NaN, a unit of replicate 1 and environment 0: exactly the groups of replicate 1 whose step
    uses environment 0 have NaN conditionals (their own draws have not); no group of another replicate, or of another
    environment's steps, changes a bit."""
    sp, mu, om = inputs(case)
    E, m, r, env = rc.n_env(sp), 5, 1, 0
    u = env + E * m + E * sp.n_bc * r
    hit = [group_of(sp, r, k) for k in range(sp.n_time[r] - 1) if rc.env_of(sp, r, k) == env]
    rest = np.setdiff1d(np.arange(n_groups(sp)), hit)
    assert hit and len(rest) > sp.n_time[0] - 1                   # some steps of replicate 1 are spared, besides all of replicate 0
    mu2 = mu.copy()
    mu2[sp.offsets()["logsigma_bc"][0] + u] = np.nan
    with pc._handle(lib, sp, mu, om) as e:
        base = prb(e, n)
    with pc._handle(lib, sp, mu2, om) as e:
        got = prb(e, n)
    assert rc.same_bytes({k: v[rest] for k, v in got.items()}, {k: v[rest] for k, v in base.items()})
    for k in RB_KEYS:
        assert np.all(np.isnan(got[k][hit])), k
        assert not np.any(np.isnan(got[k][rest])), k
    keep = ("q_mean", "q_sd", "n_members")
    assert rc.same_bytes({k: got[k][hit] for k in keep}, {k: base[k][hit] for k in keep})


# ---- 7. errors ------------------------------------------------------------------------------------------------------------------
OUTS = UNITS + ("quantiles", "n_members")


def raw(engine, n_samples, probs=PROBS, threshold=0.0, seed=SEED, draws=None, null=(), want=OUTS, n_quantiles=None):
    """bb_popmean_rb through ctypes with only the outputs in `want` non-NULL; `null` names arguments passed as NULL."""
    ng = engine.popmean_rb_shape()
    p = np.ascontiguousarray(probs, dtype=np.float64)
    o = _capi.bb_rb_opts()
    o.n_samples, o.n_quantiles, o.threshold, o.seed = n_samples, len(p) if n_quantiles is None else n_quantiles, threshold, seed
    o.probs = None if "probs" in null or not len(p) else _capi._ptr(p)
    if draws is not None:
        o.draws = _capi._ptr(draws)
    res, out = {}, _capi.bb_popmean_rb_out()
    for k in want:
        if k == "n_members":
            res[k] = np.full(ng, -7, dtype=np.int32)
            setattr(out, k, res[k].ctypes.data_as(C.POINTER(C.c_int32)))
        else:
            res[k] = np.full((ng, len(p)) if k == "quantiles" else ng, -7.0)
            setattr(out, k, _capi._ptr(res[k]))
    rcode = engine._lib.bb_popmean_rb(None if "h" in null else engine._h, None if "o" in null else C.byref(o),
                                      None if "out" in null else C.byref(out))
    return rcode, res


def check_errors(lib):
    """Every BB_ERR_INVALID and BB_ERR_UNSUPPORTED of the contract, with a message: bb_fitness_rb's.  NOT exercised: BB_ERR_DEVICE
    for what the device cannot allocate (a test on a shared machine does not take the device's whole memory)."""
    sp, mu, om = inputs("fitness")
    INVALID, UNSUPPORTED = -1, _capi.BB_ERR_UNSUPPORTED
    msg = lambda: lib.bb_last_error().decode()
    dr = rc.materialise(sp, mu, om, 3, 1)
    with pc._handle(lib, sp, mu, om) as e:
        for null in ("h", "o", "out"):
            assert raw(e, 10, null=(null,))[0] == INVALID and msg(), null
        for nq in (-1, 9):
            assert raw(e, 10, n_quantiles=nq)[0] == INVALID and "n_quantiles" in msg(), nq
        assert raw(e, 10, null=("probs",), n_quantiles=3)[0] == INVALID and "probs" in msg()
        for bad in (0.0, 1.0, -0.1, 1.5, np.nan):
            assert raw(e, 10, probs=(0.5, bad))[0] == INVALID and "prob" in msg(), bad
        for bad in (np.inf, -np.inf, np.nan):
            assert raw(e, 10, threshold=bad)[0] == INVALID and "threshold" in msg(), bad
        for n in (1, 0, -3, MAXN + 1):
            assert raw(e, n)[0] == UNSUPPORTED and "n_samples" in msg(), n
        for n in (0, MAXN + 1):
            assert raw(e, n, draws=dr)[0] == UNSUPPORTED and "n_samples" in msg(), n
        assert raw(e, 1, draws=dr)[0] == 0 and raw(e, 3, draws=dr)[0] == 0      # one explicit draw is served
        assert raw(e, 64, want=())[0] == 0                                       # an all-NULL out
        assert raw(e, 64, probs=())[0] == 0                                      # no quantiles
        full = prb(e, 64)
        assert rc.same_bytes(raw(e, 64)[1], full)
        for k in OUTS:                                                           # every output NULL except one
            rcode, one = raw(e, 64, want=(k,))
            assert rcode == 0 and rc.same_bytes(one, {k: full[k]}), k
        try:
            e.popmean_rb(n_samples=1)
        except _capi.BarBayHipError as ex:
            assert "error -4" in str(ex) and "n_samples" in str(ex)
        else:
            raise AssertionError("no error")
        try:
            e.popmean_rb(draws=np.zeros((3, sp.D + 1)))
        except _capi.BarBayHipError as ex:
            assert "draws" in str(ex)
        else:
            raise AssertionError("no error")
