"""bb_theta_rb (Rao-Blackwellised hyper-fitness marginals, barbay.jl_amd/csrc/bb_rb.h) restated in numpy from the formulas of
include/barbay_hip.h, and the cases the emulation and GPU tests share.  The draws, their keying, the steps y_{u,j} of a member and
the mixture of a group's conditionals are `_rb_cases`' (`steps` here repeats the walk of `_rb_cases.conditionals`, which returns a
unit's finished (m, sd) and not its y); the new part is the sum over a group's members by the chunk rule.

Expected values: tests/golden/theta_rb_<case>_n<samples>.npz, a 50-digit mpmath evaluation of `_rb_cases.unit64`'s formulas on
this restatement's float64 (theta_j, m_j, sd_j), written by tests/golden/make_theta_rb_golden.py.  Bounds, in `_rb_cases`' sense
(relative to max(|x|, 1); to the value itself for p_pos, p_neg): the larger of 1e-12 and 8 x the float64 restatement's own measured
error against the goldens (MEASURED / Q_MEASURED below; the project's standing margin).  Thresholds: a hyper-fitness is sharp (sd
0.04 .. 0.2 here) and the groups' means spread over -4 .. 4, so no single threshold lies within 20 sd of every group's conditionals;
the parameters stay `_rb_cases.params`' and the threshold is chosen per group instead, the multiple of 0.25 nearest the group's rb_mean
(stored in the golden file): the library is called once per distinct threshold, a group's p_pos / p_neg are taken from the call at
its threshold, and everything that does not depend on the threshold must come out of all those calls with the same bytes.
`check_z_range` checks |m_j - s0| / sd_j <= 20 on the CPU (the cases get to 10 .. 15.4 at n = 1000; whole-number thresholds gave 28).

Measured, largest error over a case's groups against the golden, float64 restatement / host emulation / MI355X, in units of 1e-16
(each test prints its own line):

case                                                     q_mean               q_sd            rb_mean              rb_sd              p_pos              p_neg          quantiles
genotype_chunks_n1000             0.6/  1.7/  1.7    0.0/  0.0/  0.0    1.3/  4.0/  2.7    0.3/  0.1/  0.1    2.1/  6.2/  8.3    1.3/  4.0/  3.6    3.3/  3.3/  3.3
genotype_chunks_n111              0.6/  2.2/  2.2    0.0/  0.1/  0.1    2.7/  5.4/  5.4    0.1/  0.3/  0.3    3.7/ 17.9/ 28.4    3.9/  5.2/  5.2    3.3/  5.6/  5.6
genotype_chunks_n2                0.0/  0.0/  0.0    0.0/  0.0/  0.0    0.0/  0.3/  1.4    0.0/  0.3/  0.9    1.6/ 18.4/ 59.0   29.3/ 34.8/ 33.0    1.4/  1.4/  1.4
genotype_regrouped_n1000          0.6/  2.2/  2.2    0.1/  0.1/  0.1    1.8/  5.2/  5.2    0.1/  0.3/  0.4    1.6/  3.8/  8.8    1.5/  7.6/  8.9    2.1/  3.2/  3.4
genotype_regrouped_n111           1.7/  1.7/  1.7    0.1/  0.1/  0.1    3.6/  5.2/  8.6    0.1/  0.3/  0.6    1.8/  9.2/  9.7    3.6/  3.5/  9.1    3.8/  7.2/  6.7
genotype_regrouped_n2             0.0/  0.6/  0.6    0.0/  0.3/  0.3    0.0/  1.6/  1.6    0.0/  1.7/  3.6    2.0/  3.9/  3.9    2.8/408.4/409.7    2.2/  4.0/  5.0
genotype_regrouped_n8672          0.6/  1.7/  1.7    0.1/  0.0/  0.0    2.1/  1.7/  1.7    0.1/  0.1/  0.1    0.0/  3.8/  3.8    1.9/  5.7/  6.2    2.1/  2.3/  2.3
multienv_replicate_n1000          1.1/  2.2/  2.2    0.1/  0.1/  0.1    1.4/  5.6/  5.6    0.3/  0.6/  0.6    2.2/  9.1/ 11.4    3.1/ 11.0/  8.8    4.4/ 12.2/ 12.2
multienv_replicate_n111           1.1/  3.3/  3.3    0.1/  0.1/  0.1    2.8/  6.5/  6.5    0.3/  0.8/  0.8    3.5/ 13.2/ 15.4    3.4/ 30.4/ 16.0    8.9/ 21.6/ 21.6
multienv_replicate_n2             0.0/  1.1/  1.1    0.0/  0.6/  0.6    0.0/  2.2/  2.2    0.3/  0.3/  3.9    2.2/ 11.7/120.0    2.8/168.8/267.5    2.8/  2.8/  3.5
replicate_ragged_n1000            1.1/  2.8/  2.8    0.1/  0.1/  0.1    2.1/  3.0/  2.2    0.1/  0.3/  0.3    2.2/ 11.6/ 20.5    2.1/  4.1/ 10.2    2.2/  7.8/  7.8
replicate_ragged_n111             1.1/  3.3/  3.3    0.1/  0.1/  0.1    2.5/  6.2/  6.2    0.1/  0.4/  0.4    3.8/  7.3/ 23.2    4.3/  8.1/ 24.6    3.9/  6.7/  6.7
replicate_ragged_n2               0.0/  1.1/  1.1    0.0/  0.6/  0.6    0.0/  0.6/  2.1    0.1/  0.1/  3.7    9.1/ 16.2/248.3    4.4/  6.6/515.7    2.1/  2.1/  4.1
(the largest entry of the first six columns, 515.7e-16, is 0.052 of the bound 1e-12; the largest quantile entry, 21.6e-16,
 is 0.0022 of QTOL = 1e-12; the restatement's own largest are 2.9e-15 and 8.9e-16, 8 x which is below 1e-12 in both)
Chunk rule (`check_chunk_rule`, genotype_chunks at n = 111 with explicit draws, against the float64 restatement, no golden), emulation / MI355X:
q_mean 2.2/2.2 q_sd 0.1/0.1 rb_mean 2.7/2.7 rb_sd 0.2/0.2 p_pos 7.3/1.1 p_neg 10.7/25.4 quantiles 8.9/8.9.
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
CHUNK = _capi.BB_THETA_RB_CHUNK
MEASURED = 2.9e-15        # the float64 restatement's largest error of the six moments and tails against the goldens
Q_MEASURED = 8.9e-16      # ... and of the quantiles
TOL = max(1e-12, 8.0 * MEASURED)
QTOL = max(1e-12, 8.0 * Q_MEASURED)
SEED, PROBS, NS, MAXN, Z_HI = rc.SEED, rc.PROBS, rc.NS, rc.MAXN, rc.Z_HI
THRESHOLDS = tuple(0.25 * x for x in range(-24, 25))              # a group's tails are taken at the one nearest its rb_mean (`nearest`)
CASES = ("genotype_chunks", "genotype_regrouped", "multienv_replicate", "replicate_ragged")
CHUNK_SIZES = (1, 64, 65)                                         # genotype_chunks: members of genotypes 0, 1, 2; genotype 3 has the rest
BIG = {f"genotype_regrouped_n{MAXN}": ("genotype_regrouped", MAXN, (0, 3, 6))}
IDENTITY = list(CASES) + ["genotype_matrix_prior", "replicate_ragged_method"]


@functools.lru_cache(maxsize=None)
def spec(case):
    if case in pc.CASES:
        return pc.spec(case)
    if case == "genotype_chunks":                                 # one member, a full chunk, a chunk boundary, several chunks
        from oracle import fixtures
        sp = fixtures.synthetic("genotype", B=290, T=3, n_geno=4, n_neutral=10, seed=3)   # 280 mutants: 150 = 2 x 64 + 22 are left for genotype 3
        nb = sp.n_bc
        gi = np.full(nb, 3, dtype=np.int64)
        where = np.random.default_rng(6).permutation(nb)          # scattered: no genotype's mutants are consecutive
        lo = 0
        for g, k in enumerate(CHUNK_SIZES):
            gi[where[lo:lo + k]] = g
            lo += k
        first = {}
        gi = np.array([first.setdefault(int(g), len(first)) for g in gi])      # first-appearance numbering, as the host hands it over
        assert sorted(np.bincount(gi)) == sorted(CHUNK_SIZES + (nb - lo,)) and nb - lo >= 2 * CHUNK + 1 and (nb - lo) % CHUNK
        return ModelSpec(kind=sp.kind, counts=sp.counts, totals=sp.totals, n_neutral=sp.n_neutral, n_bc=nb, geno_idx=gi)
    if case == "genotype_matrix_prior":                           # (identity only) a Matrix-form s_bc prior: one row per genotype
        sp, g = spec("genotype_regrouped"), np.random.default_rng(4)
        return ModelSpec(kind=sp.kind, counts=sp.counts, totals=sp.totals, n_neutral=sp.n_neutral, n_bc=sp.n_bc, geno_idx=sp.geno_idx,
                         priors=dict(s_bc_prior=(g.normal(0.0, 1.0, sp.n_geno), g.uniform(0.3, 3.0, sp.n_geno))))
    if case == "multienv_replicate_ragged_env":                   # the second replicate never returns to environment 0: n_u = 0 there
        sp = spec("multienv_replicate")
        env = [np.asarray(sp.env_idx[0]), np.r_[0, np.ones(sp.n_time[1] - 1, dtype=np.int64)]]
        assert set(env[0][1:]) == {0, 1}
        return ModelSpec(kind=sp.kind, counts=sp.counts, totals=sp.totals, n_neutral=sp.n_neutral, n_bc=sp.n_bc, env_idx=env)
    raise KeyError(case)


def golden_cases():
    out = {f"{c}_n{n}": (c, n, None) for c in CASES for n in NS}
    out.update(BIG)
    return out


def golden_path(name):
    return os.path.join(rc.GOLD, f"theta_rb_{name}.npz")


def n_groups(sp):
    return slice(*sp.offsets()["theta"]).stop - sp.offsets()["theta"][0]


def members(sp, g):
    """The units of group g's members, in member order."""
    if sp.kind == "genotype":
        return [int(m) for m in np.flatnonzero(sp.geno_idx == g)]
    E = rc.n_env(sp)
    return [g + E * sp.n_bc * r for r in range(sp.n_rep)]


@functools.lru_cache(maxsize=None)
def inputs(case):
    sp = spec(case)
    mu, om = rc.params(sp)
    mu.setflags(write=False)
    om.setflags(write=False)
    return sp, mu, om


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def steps(sp, D, n):
    """y [n_units, n] and n_u [n_units] of every fitness unit from the draws D(i) -> [n]: bb_fitness_rb's, as
    `_rb_cases.conditionals` forms them."""
    off = sp.offsets()
    B, nb, nn, R = sp.B, sp.n_bc, sp.n_neutral, sp.n_rep
    E = rc.n_env(sp)
    y = np.zeros((rc.n_units(sp), n))
    nst = np.zeros(rc.n_units(sp), dtype=np.int32)
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
        for mm in range(nb):
            for t in range(T - 1):
                u = rc.env_of(sp, r, t) + E * mm + E * nb * r
                y[u] = y[u] + (((ll(nn + mm, t + 1) - ll(nn + mm, t)) - (logZ[t + 1] - logZ[t])) + sbar[t])
                nst[u] += 1
        lo_l += T * B
        g0 += T - 1
    return y, nst


def conditionals(sp, D, n, groups=None, chunk=CHUNK):
    """(theta, m, sd) [n_groups, n], n_members and n_steps [n_groups]: the header's formulas, a group's members summed in chunks
    of `chunk` consecutive members, the chunks in order."""
    off = sp.offsets()
    y, nst = steps(sp, D, n)
    G = n_groups(sp)
    pm, ps = sp.prior_arrays()
    th, m, sd = np.empty((G, n)), np.empty((G, n)), np.empty((G, n))
    nmem, nsteps = np.zeros(G, dtype=np.int32), np.zeros(G, dtype=np.int32)
    for g in (range(G) if groups is None else groups):
        us = members(sp, g)
        SP, SN = np.zeros(n), np.zeros(n)
        for c0 in range(0, len(us), chunk):
            cp, cn = np.zeros(n), np.zeros(n)
            for u in us[c0:c0 + chunk]:
                if nst[u] == 0:
                    continue
                w = np.exp(-2.0 * D(off["logsigma_bc"][0] + u))
                tau, tt = np.exp(D(off["logtau"][0] + u)), D(off["theta_tilde"][0] + u)
                cp = cp + float(nst[u]) * w
                cn = cn + w * (y[u] - float(nst[u]) * (tau * tt))
            SP, SN = SP + cp, SN + cn
        i = off["theta"][0] + g
        a, ib2 = pm[i], 1.0 / (ps[i] * ps[i])
        nmem[g], nsteps[g] = len(us), int(nst[us].sum()) if us else 0
        if nsteps[g] == 0:
            m[g], sd[g] = a, 1.0 / np.sqrt(ib2)
        else:
            P = ib2 + SP
            m[g], sd[g] = (a * ib2 + SN) / P, 1.0 / np.sqrt(P)
        th[g] = D(i)
    return th, m, sd, nmem, nsteps


def nearest(x):
    """The threshold of THRESHOLDS nearest to x (elementwise)."""
    t = np.asarray(THRESHOLDS)
    return t[np.abs(np.asarray(x)[..., None] - t).argmin(axis=-1)]


def restate(sp, mu, omega, n, seed, threshold=0.0, probs=PROBS, draws=None, groups=None, unit=rc.unit64, want_z=False, chunk=CHUNK):
    """bb_theta_rb at (mu, omega) -- or at the explicit `draws` [n, D] -- for `groups` (all): a dict as Engine.theta_rb returns, plus
    the thresholds used.  `threshold`: one for all groups, one per group, or None: per group the one of THRESHOLDS nearest to the mean
    of its m_j."""
    with np.errstate(all="ignore"):
        D = rc.Rows(draws) if draws is not None else sc.Draws(seed, mu, pc.softplus(omega), n)
        groups = np.arange(n_groups(sp)) if groups is None else np.asarray(groups)
        th, m, sd, nmem, nsteps = conditionals(sp, D, n, groups=groups, chunk=chunk)
        out = {k: np.empty(len(groups)) for k in UNITS}
        out["quantiles"] = np.empty((len(groups), len(probs)))
        out["n_steps"], out["n_members"] = nsteps[groups], nmem[groups]
        s0 = np.broadcast_to(np.asarray(nearest(m[groups].mean(axis=1)) if threshold is None else threshold, dtype=np.float64), groups.shape)
        out["threshold"] = s0.copy()
        if want_z:
            out["zmax"] = np.array([np.abs((m[g] - s0[x]) / sd[g]).max() for x, g in enumerate(groups)])
        for x, g in enumerate(groups):
            vals, qs = unit(th[g], m[g], sd[g], float(s0[x]), probs)
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
    err = rc.errors({k: v for k, v in got.items() if k != "threshold"}, ref)
    assert np.array_equal(got["n_members"], ref["n_members"])
    return err


def assert_within(err, who):
    for k in UNITS:
        assert err[k] <= TOL, (who, k, err[k])
    assert err["quantiles"] <= QTOL, (who, "quantiles", err["quantiles"])


def report(name, label, err):
    print(f"theta_rb case {name:30s} {label:12s} " + " ".join(f"{k} {err[k] / 1e-16:7.1f}" for k in UNITS + ("quantiles",)) + "  (1e-16)")


def trb(e, n, **kw):
    kw.setdefault("probs", PROBS)
    kw.setdefault("threshold", 0.0)
    kw.setdefault("seed", SEED)
    return e.theta_rb(n_samples=n, **kw)


# ---- 1. the identity against the log-joint -----------------------------------------------------------------------------------------
def check_identity(lib, name, device=False):
    """At 3 random points, each passed as one explicit draw: P (m - theta) from rb_sd, rb_mean, q_mean against the literal oracle's
    gradient over the theta block (and, device, against Engine.logdensity_grad): 1e-9 of the block's largest entry."""
    from oracle import literal
    quirk = name == "replicate_ragged_method"
    sp = spec("replicate_ragged" if quirk else name)
    blk = slice(*sp.offsets()["theta"])
    g = np.random.default_rng(8)
    kw = dict(ragged_method=True) if quirk else {}
    with make_engine(sp, lib, seed=1, use_priors=name.endswith("matrix_prior"), **kw) as e:
        assert e.theta_rb_shape() == n_groups(sp) == blk.stop - blk.start
        for scale in (0.3, 1.0, 0.3):                             # drawn as in _logp_cases.spec
            z = g.normal(0.0, scale, sp.D)
            got = e.theta_rb(probs=(), draws=z)
            ref = restate(sp, None, None, 1, 0, probs=(), draws=z[None, :])
            lhs = 1.0 / got["rb_sd"] ** 2 * (got["rb_mean"] - got["q_mean"])
            grad = literal.logjoint_and_grad(z, sp, **(dict(ragged_quirk=True) if quirk else {}))[1][blk]
            scale_g = np.abs(grad).max()
            err = np.abs(lhs - grad).max() / scale_g
            r64 = 1.0 / ref["rb_sd"] ** 2 * (ref["rb_mean"] - ref["q_mean"])
            print(f"theta_rb identity {name:26s} sd {scale}: library {err:.2e}, restatement {np.abs(r64 - grad).max() / scale_g:.2e} of max |g| = {scale_g:.3g}")
            assert err <= 1e-9
            assert np.all(got["q_sd"] == 0.0) and np.array_equal(got["q_mean"], z[blk])
            assert np.array_equal(got["n_members"], ref["n_members"]) and np.array_equal(got["n_steps"], ref["n_steps"])
            if device:
                gd = e.logdensity_grad(z)[1][blk]
                assert np.abs(lhs - gd).max() <= 1e-9 * np.abs(gd).max()


# ---- 2. golden values ----------------------------------------------------------------------------------------------------------
def at_thresholds(e, n, s0, **kw):
    """theta_rb with group g's tails taken at s0[g]: one call per distinct threshold; whatever does not depend on the threshold has
    the same bytes in all of them."""
    out = None
    for t in sorted(set(s0.tolist())):
        got = trb(e, n, threshold=t, **kw)
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
    e0 = errors(restate(sp, mu, om, n, SEED, threshold=s0, groups=groups), ref)
    report(name, "restatement", e0)
    full = np.full(n_groups(sp), s0[0])
    full[slice(None) if groups is None else list(groups)] = s0
    with pc._handle(lib, sp, mu, om) as e:
        got = at_thresholds(e, n, full)
    assert got["quantiles"].shape == (n_groups(sp), len(PROBS)) and np.all(np.diff(got["quantiles"], axis=1) > 0)
    err = errors(rc.take(got, groups), ref)
    report(name, label, err)
    assert_within(e0, "restatement")
    assert_within(err, label)


def check_z_range(name):
    """The thresholds keep every group's conditionals within 20 of their sds (CPU, the restatement), and at n >= 1000
    the sharpest get beyond 8."""
    case, n, groups = golden_cases()[name]
    sp, mu, om = inputs(case)
    ref = golden(name)
    z = restate(sp, mu, om, n, SEED, threshold=ref["threshold"], probs=(), groups=groups, want_z=True)["zmax"]
    print(f"theta_rb z range {name}: {z.max():.2f}")
    assert z.max() <= Z_HI, z.max()
    assert n < 1000 or z.max() >= 8.0, z.max()


# ---- 3. the chunk rule ------------------------------------------------------------------------------------------------------------
def relabelled(sp, draws):
    """`genotype_chunks` with the caller's mutants relabelled, and the draws moved with them: pairs of neighbouring mutants of
    different genotypes change places, so the library's regrouping permutation differs while every genotype's members keep
    their relative order.  The normalisers add the columns in the caller's order, so a swapped pair must hand them equal
    addends for the bytes to stay: the pair's loglambda draws are made equal, in a copy of `draws` that is returned as well.
    Returns (spec, draws of the original labelling, draws of the new one, new mutant of each old one)."""
    nb, nn, T = sp.n_bc, sp.n_neutral, sp.n_time[0]
    off = sp.offsets()
    new_of = np.arange(nb)
    draws = draws.copy()
    ll = lambda m: slice(off["loglambda"][0] + (nn + m) * T, off["loglambda"][0] + (nn + m + 1) * T)
    m, swaps = 0, 0
    while m + 1 < nb:
        if sp.geno_idx[m] != sp.geno_idx[m + 1] and m % 3 == 0:
            new_of[m], new_of[m + 1] = m + 1, m
            draws[:, ll(m + 1)] = draws[:, ll(m)]
            swaps += 1
            m += 2
        else:
            m += 1
    assert swaps >= 10
    old_of = np.argsort(new_of)
    cnt = sp.counts[0].copy()
    cnt[:, nn:] = cnt[:, nn + old_of]
    gi = sp.geno_idx[old_of]                                      # (a genotype keeps its number)
    sp2 = ModelSpec(kind=sp.kind, counts=[cnt], totals=sp.totals, n_neutral=nn, n_bc=nb, geno_idx=gi)
    d2 = draws.copy()
    for name in ("theta_tilde", "logtau", "logsigma_bc"):
        lo = off[name][0]
        d2[:, lo:lo + nb] = draws[:, lo + old_of]
    for mm in range(nb):
        d2[:, ll(mm)] = draws[:, ll(old_of[mm])]
    return sp2, draws, d2, new_of


def check_chunk_rule(lib, label, n=111):
    """(a) The library against the restatement summed by the chunk rule, on explicit draws as they are.  (b) The same draws with
    the swapped pairs' loglambda rows equalised (`relabelled`), in the original and in the relabelled labelling: equal bytes."""
    sp, mu, om = inputs("genotype_chunks")
    assert sorted(np.bincount(sp.geno_idx))[:3] == list(CHUNK_SIZES)
    dr = rc.materialise(sp, mu, om, n, SEED)
    ref = restate(sp, None, None, n, 0, draws=dr)
    one = restate(sp, None, None, n, 0, draws=dr, chunk=10 ** 9)  # a group's members in one run: another order of the sums
    assert not rc.same_bytes(ref, one)
    sp2, dr1, dr2, new_of = relabelled(sp, dr)
    with make_engine(sp, lib, seed=4) as e:
        got = trb(e, n, draws=dr)
        got1 = trb(e, n, draws=dr1)
        perm = np.asarray(e.permutation())
    err = errors(got, ref)
    report("genotype_chunks explicit", label, err)
    assert_within(err, label)
    with make_engine(sp2, lib, seed=4) as e:
        got2 = trb(e, n, draws=dr2)
        perm2 = np.asarray(e.permutation())
    assert not np.array_equal(perm, perm2)                        # the library regroups the two labellings differently
    assert rc.same_bytes(got1, got2) and not rc.same_bytes(got, got1)
    return got


# ---- 4. determinism ------------------------------------------------------------------------------------------------------------
def check_launch_modes(lib, case="genotype_chunks"):
    import barbay_jl_amd as bb
    sp, mu, om = inputs(case)
    out = []
    for mode in (1, 0):
        with bb.Engine(sp.kind, sp.counts, sp.n_neutral, sp.n_bc, env_idx=sp.env_idx, geno_idx=sp.geno_idx, seed=4, launch_mode=mode, _lib=lib) as e:
            e.set_params(mu, om)
            out.append(trb(e, 500, seed=2))
            out.append(trb(e, 500, seed=2))
    assert all(rc.same_bytes(out[0], o) for o in out[1:])


GROUP_CASES = tuple(c for c in pc.GROUP_CASES if pc.CASES[c][0] in rc.HIER)


def check_group_handle(lib, case):
    sp, mu, om = inputs(case)
    with pc._handle(lib, sp, mu, om, device_ids=[0, 0]) as e:
        a = trb(e, 111)
    with pc._handle(lib, sp, mu, om) as e:
        b = trb(e, 111)
    assert rc.same_bytes(a, b)


def check_buffer_reuse(lib):
    """The call interleaved with the other post-fit calls at changing sizes on one handle (the buffer regrows and is reused
    stale): every result is byte for byte what a fresh handle gives."""
    sp, mu, om = inputs("genotype_regrouped")
    om = np.minimum(om, -2.0)
    qs = (0.95, 0.675, 0.05)
    chain = np.random.default_rng(12).standard_normal((2, 5, 6))
    dr = rc.materialise(sp, mu, om, 7, 3)
    calls = [lambda e: trb(e, 111),
             lambda e: e.ppc_bands(qs, n_samples=111, n_ppc=7, seed=SEED),
             lambda e: trb(e, 1000),
             lambda e: rc.rb(e, 200),
             lambda e: e.freq_bands(qs, mode="posterior", n_samples=200, n_ppc=1, seed=SEED),
             lambda e: trb(e, 2),
             lambda e: e.chain_summary(chain),
             lambda e: e.ppc_score(n_samples=111, seed=SEED),
             lambda e: trb(e, 7, draws=dr),
             lambda e: rc.rb(e, 2049, probs=(0.5,)),
             lambda e: trb(e, 2049, probs=(0.5,)),
             lambda e: trb(e, 111)]
    with pc._handle(lib, sp, mu, om) as e:
        got = [pc._bits(f(e)) for f in calls]
    for i, f in enumerate(calls):
        with pc._handle(lib, sp, mu, om) as e:
            assert got[i] == pc._bits(f(e)), i
    assert got[0] == got[-1]


def check_handle_untouched(lib):
    sp = spec("genotype_regrouped")
    with make_engine(sp, lib, seed=5) as a, make_engine(sp, lib, seed=5) as b:
        trb(b, 111)
        for x, y in zip(a.get_params(), b.get_params()):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
        a.run(5)
        trb(b, 64, seed=1)
        b.run(5)
        for x, y in zip(a.get_params(), b.get_params()):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64))


# ---- 5. own draws against the same draws passed in -----------------------------------------------------------------------------------
def check_internal_against_explicit_draws(lib, case, n=111):
    sp, mu, om = inputs(case)
    dr = rc.materialise(sp, mu, om, n, SEED)
    with pc._handle(lib, sp, mu, om) as e:
        a = trb(e, n)
        b = trb(e, n, draws=dr)
        c = trb(e, 5, draws=dr)                             # n_samples is the row count; the argument is ignored
    assert rc.same_bytes(b, c)
    err = errors(a, b)
    report(case + f"_n{n}", "own/explicit", err)
    assert_within(err, "explicit draws")


# ---- 6. non-finite values ---------------------------------------------------------------------------------------------------------
def check_nan_parameter(lib, case="genotype_regrouped", n=111):
    """One member's logsigma_bc mean NaN: exactly its group's conditionals are NaN (theta's own draws, n_members and n_steps are
    not), every other group keeps its bytes."""
    sp, mu, om = inputs(case)
    u = 7
    g = int(sp.geno_idx[u])
    mu2 = mu.copy()
    mu2[sp.offsets()["logsigma_bc"][0] + u] = np.nan
    with pc._handle(lib, sp, mu, om) as e:
        base = trb(e, n)
    with pc._handle(lib, sp, mu2, om) as e:
        got = trb(e, n)
    rest = np.setdiff1d(np.arange(n_groups(sp)), [g])
    assert rc.same_bytes({k: v[rest] for k, v in got.items()}, {k: v[rest] for k, v in base.items()})
    for k in ("rb_mean", "rb_sd", "p_pos", "p_neg", "quantiles"):
        assert np.all(np.isnan(got[k][g])), k
        assert not np.any(np.isnan(got[k][rest])), k
    keep = ("q_mean", "q_sd", "n_members", "n_steps")
    assert rc.same_bytes({k: got[k][[g]] for k in keep}, {k: base[k][[g]] for k in keep})


def check_nan_in_a_member_without_steps(lib, n=111):
    """The same NaN in a member with n_u = 0 (a replicate that never returns to the group's environment) changes nothing."""
    sp = spec("multienv_replicate_ragged_env")
    mu, om = rc.params(sp)
    E, m = rc.n_env(sp), 5
    u = 0 + E * m + E * sp.n_bc * 1                               # environment 0, mutant 5, the second replicate
    _, nst = steps(sp, rc.Rows(mu[None, :]), 1)
    assert nst[u] == 0 and nst[u + 1] > 0 and nst[0 + E * m] > 0
    mu2 = mu.copy()
    mu2[sp.offsets()["logsigma_bc"][0] + u] = np.nan
    with pc._handle(lib, sp, mu, om) as e:
        base = trb(e, n)
    with pc._handle(lib, sp, mu2, om) as e:
        got = trb(e, n)
    assert rc.same_bytes(got, base) and not np.any(np.isnan(got["rb_sd"]))
    ref = restate(sp, mu2, om, n, SEED)
    assert np.array_equal(got["n_steps"], ref["n_steps"]) and got["n_steps"][E * m] == nst[E * m] and got["n_members"][E * m] == 2
    err = errors(got, ref)
    report("multienv_replicate_ragged_env", "vs restated", err)
    assert_within(err, "n_u = 0 member")


# ---- 7. errors ------------------------------------------------------------------------------------------------------------------
OUTS = UNITS + ("quantiles", "n_members", "n_steps")


def raw(engine, n_samples, probs=PROBS, threshold=0.0, seed=SEED, draws=None, null=(), want=OUTS, n_quantiles=None):
    """bb_theta_rb through ctypes with only the outputs in `want` non-NULL; `null` names arguments passed as NULL."""
    ng = engine.theta_rb_shape()
    p = np.ascontiguousarray(probs, dtype=np.float64)
    o = _capi.bb_rb_opts()
    o.n_samples, o.n_quantiles, o.threshold, o.seed = n_samples, len(p) if n_quantiles is None else n_quantiles, threshold, seed
    o.probs = None if "probs" in null or not len(p) else _capi._ptr(p)
    if draws is not None:
        o.draws = _capi._ptr(draws)
    res, out = {}, _capi.bb_theta_rb_out()
    for k in want:
        if k in ("n_steps", "n_members"):
            res[k] = np.full(ng, -7, dtype=np.int32)
            setattr(out, k, res[k].ctypes.data_as(C.POINTER(C.c_int32)))
        else:
            res[k] = np.full((ng, len(p)) if k == "quantiles" else ng, -7.0)
            setattr(out, k, _capi._ptr(res[k]))
    rcode = engine._lib.bb_theta_rb(None if "h" in null else engine._h, None if "o" in null else C.byref(o),
                                    None if "out" in null else C.byref(out))
    return rcode, res


def check_errors(lib):
    """Every BB_ERR_INVALID and BB_ERR_UNSUPPORTED of the contract, with a message.  NOT exercised: BB_ERR_DEVICE for what the
    device cannot allocate (a test on a shared machine does not take the device's whole memory)."""
    sp, mu, om = inputs("genotype_regrouped")
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
        full = trb(e, 64)
        assert rc.same_bytes(raw(e, 64)[1], full)
        for k in OUTS:                                                           # every output NULL except one
            rcode, one = raw(e, 64, want=(k,))
            assert rcode == 0 and rc.same_bytes(one, {k: full[k]}), k
        try:
            e.theta_rb(n_samples=1)
        except _capi.BarBayHipError as ex:
            assert "error -4" in str(ex) and "n_samples" in str(ex)
        else:
            raise AssertionError("no error")
        try:
            e.theta_rb(draws=np.zeros((3, sp.D + 1)))
        except _capi.BarBayHipError as ex:
            assert "draws" in str(ex)
        else:
            raise AssertionError("no error")
    for case, kind in (("fitness", "BB_MODEL_FITNESS"), ("multienv", "BB_MODEL_MULTIENV")):      # the kinds without a theta
        sp, mu, om = rc.inputs(case)
        with pc._handle(lib, sp, mu, om) as e:
            assert e.theta_rb_shape() == 0
            assert raw(e, 64)[0] == UNSUPPORTED and kind in msg()
            try:
                e.theta_rb()
            except _capi.BarBayHipError as ex:
                assert "error -4" in str(ex) and kind in str(ex)
            else:
                raise AssertionError("no error")
