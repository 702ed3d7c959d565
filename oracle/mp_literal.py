"""50-digit transcription of the five log-joints (mpmath).  TEST INFRASTRUCTURE ONLY.

The same statement-order transcription as ``oracle/literal.py`` -- priors, ``Poisson`` on the totals, one ``Multinomial``
per time point, the two diagonal ``MvNormal`` on the log frequency ratios -- with every residual written directly
(no moment expansion, no fused Poisson identity), in ``mpmath`` arithmetic at 50 significant digits.  It exists so that
the fp64 oracle and the engine can both be measured against something that is not fp64 itself.

Every log-joint is formed as a flat list of *elementary addends*; nothing is added up before the end:

* Poisson      ``n log(sum lam)``, ``-sum lam``, ``-lgamma(n + 1)``
* Multinomial  ``lgamma(n + 1)``, each ``-lgamma(x_i + 1)``, each ``x_i log p_i``
* Normal       per entry the log-normaliser ``-(log 2 pi + log v) / 2`` and the quadratic ``-(x - m)^2 / (2 v)``

``logjoint`` returns the sum and the *scale*, the sum of the addends' absolute values: an fp64 evaluation of the same
statements cannot be expected to do better than a few ``2^-53 * scale``, however small ``|logp|`` itself comes out.
``grad`` differences every addend separately (central, ``h = 1e-18``; truncation ~ ``h^2 f''' / 6 ~ 1e-30``) and returns
per entry the derivative ``g_i`` and ``G_i = sum_addends |d addend / d z_i|``, the scale an "ulp of entry i" refers to.

What this pins is arithmetic: it is this repository's reading of the model statements, evaluated exactly.  It says nothing
about parity with Turing (PARITY UNPINNED, see oracle/__init__.py) -- a transcription mistake shared with literal.py
would pass unnoticed here, which is why tests/test_emu_accuracy.py checks the two against each other only as a guard on
THIS file.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import mpmath
import numpy as np

from .spec import ModelSpec

DPS = 50
H = "1e-18"

ctx = mpmath.mp.clone()
ctx.dps = DPS
mpf = ctx.mpf
LOG2PI = ctx.log(2 * ctx.pi)
HALF = mpf("0.5")

# ---- memoised elementary functions: differencing moves one latent at a time, so almost every argument repeats ---------------------
class _Memo:
    """base: filled while the unperturbed point is evaluated; scratch: what one perturbed evaluation adds, dropped after it."""

    def __init__(self):
        self.base, self.scratch, self.frozen = {}, {}, False

    def get(self, key, fn):
        v = self.base.get(key)
        if v is None:
            v = self.scratch.get(key)
            if v is None:
                v = fn(key)
                (self.scratch if self.frozen else self.base)[key] = v
        return v


_memo = {"exp": _Memo(), "log": _Memo(), "lgamma": _Memo(), "normal": _Memo()}


def clear_cache():
    for m in _memo.values():
        m.base.clear(), m.scratch.clear()
        m.frozen = False


def _freeze(on: bool):
    for m in _memo.values():
        m.scratch.clear()
        m.frozen = on


def _exp(x):
    return _memo["exp"].get(x, ctx.exp)


def _log(x):
    return _memo["log"].get(x, ctx.log)


def _lgamma(x: int):
    return _memo["lgamma"].get(x, lambda n: ctx.loggamma(mpf(n)))


def _normal_pair(key):
    xi, mi, vi = key
    return (-HALF * (LOG2PI + _log(vi)), -HALF * (xi - mi) ** 2 / vi)


def _xlogy(x: int, y):
    return mpf(0) if x == 0 else x * _log(y)


# ---- distribution pieces (each returns its addends) -------------------------------------------------------------------------------
def mvnormal_diag_terms(x: Sequence, mean: Sequence, var: Sequence) -> List:
    assert len(x) == len(mean) == len(var)
    out = []
    for key in zip(x, mean, var):
        out.extend(_memo["normal"].get(key, _normal_pair))
    return out


def poisson_terms(x: int, lam) -> List:
    return [_xlogy(x, lam), -lam, -_lgamma(x + 1)]


def multinomial_terms(x: Sequence[int], n: int, p: Sequence) -> List:
    assert sum(x) == n
    return [_lgamma(n + 1)] + [-_lgamma(xi + 1) for xi in x] + [_xlogy(xi, pi) for xi, pi in zip(x, p)]


def _prior_terms(z: Sequence, mean, std) -> List:
    n = len(z)
    m = [mpf(float(v)) for v in np.broadcast_to(np.asarray(mean, dtype=np.float64), (n,))]
    s = [mpf(float(v)) for v in np.broadcast_to(np.asarray(std, dtype=np.float64), (n,))]
    return mvnormal_diag_terms(z, m, [v ** 2 for v in s])


def _rep(v: Sequence, n: int) -> List:
    """Julia repeat(v, n) / torch .repeat(n): the whole vector n times."""
    return list(v) * n


def _rep_in(v: Sequence, n: int) -> List:
    """Julia repeat(v, inner=n) / torch .repeat_interleave(n): every entry n times."""
    return [x for x in v for _ in range(n)]


def _matrix(v: Sequence, T: int, B: int) -> List[List]:
    """Julia reshape(v, T, B) (column-major) as rows[t][b]."""
    return [[v[t + T * b] for b in range(B)] for t in range(T)]


def _vec(rows: List[List], cols: range) -> List:
    """Julia vec(A[:, cols]) of rows[t][b]: time fastest."""
    return [rows[t][b] for b in cols for t in range(len(rows))]


def _frequencies(logL: Sequence, T: int, B: int):
    Lam = _matrix([_exp(v) for v in logL], T, B)
    tot = [sum(row[1:], row[0]) for row in Lam]
    F = [[lam / tot[t] for lam in Lam[t]] for t in range(T)]
    logG = [[_log(F[t + 1][b] / F[t][b]) for b in range(B)] for t in range(T - 1)]
    return tot, F, logG


def _obs_terms(tot, F, R: np.ndarray, n_t: np.ndarray) -> List:
    out = []
    for t in range(len(tot)):
        out += poisson_terms(int(n_t[t]), tot[t])
    for t in range(len(tot)):
        out += multinomial_terms([int(v) for v in R[t]], int(n_t[t]), F[t])
    return out


def _sl(z, off, name):
    lo, hi = off[name]
    return z[lo:hi]


# ---- models (statement order of oracle/literal.py) --------------------------------------------------------------------------------
def terms_fitness(z, sp: ModelSpec) -> List:
    off, pr = sp.offsets(), sp.priors
    T, B, nn, nb = sp.n_time[0], sp.B, sp.n_neutral, sp.n_bc
    s_t, lsig_t = _sl(z, off, "s_pop"), _sl(z, off, "logsigma_pop")
    s_m, lsig_m, logL = _sl(z, off, "s_bc"), _sl(z, off, "logsigma_bc"), _sl(z, off, "loglambda")
    a = _prior_terms(s_t, *pr["s_pop_prior"])
    a += _prior_terms(lsig_t, *pr["logsigma_pop_prior"])
    a += _prior_terms(s_m, *pr["s_bc_prior"])
    a += _prior_terms(lsig_m, *pr["logsigma_bc_prior"])
    a += _prior_terms(logL, *pr["loglambda_prior"])
    tot, F, logG = _frequencies(logL, T, B)
    a += _obs_terms(tot, F, sp.counts[0], sp.totals[0])
    a += mvnormal_diag_terms(_vec(logG, range(nn)), _rep([-v for v in s_t], nn), _rep([_exp(v) ** 2 for v in lsig_t], nn))
    a += mvnormal_diag_terms(_vec(logG, range(nn, nn + nb)),
                             [p - q for p, q in zip(_rep_in(s_m, T - 1), _rep(s_t, nb))],
                             _rep_in([_exp(v) ** 2 for v in lsig_m], T - 1))
    return a


def terms_multienv(z, sp: ModelSpec) -> List:
    off, pr = sp.offsets(), sp.priors
    T, B, nn, nb, E = sp.n_time[0], sp.B, sp.n_neutral, sp.n_bc, sp.n_env
    env = [int(v) for v in sp.env_idx]
    s_t, lsig_t = _sl(z, off, "s_pop"), _sl(z, off, "logsigma_pop")
    s_m, lsig_m, logL = _sl(z, off, "s_bc"), _sl(z, off, "logsigma_bc"), _sl(z, off, "loglambda")
    a = _prior_terms(s_t, *pr["s_pop_prior"])
    a += _prior_terms(lsig_t, *pr["logsigma_pop_prior"])
    a += _prior_terms(s_m, *pr["s_bc_prior"])
    a += _prior_terms(lsig_m, *pr["logsigma_bc_prior"])
    a += _prior_terms(logL, *pr["loglambda_prior"])
    tot, F, logG = _frequencies(logL, T, B)
    a += _obs_terms(tot, F, sp.counts[0], sp.totals[0])
    s_m2 = _matrix(s_m, E, nb)                                  # n_env x n_bc
    lsig_m2 = _matrix(lsig_m, E, nb)
    a += mvnormal_diag_terms(_vec(logG, range(nn)), _rep([-v for v in s_t], nn), _rep([_exp(v) ** 2 for v in lsig_t], nn))
    sel = [s_m2[e] for e in env[1:]]                            # s_m2[env_idx[2:end], :]
    sel_sig = [[_exp(v) ** 2 for v in lsig_m2[e]] for e in env[1:]]
    a += mvnormal_diag_terms(_vec(logG, range(nn, nn + nb)),
                             [p - q for p, q in zip(_vec(sel, range(nb)), _rep(s_t, nb))],
                             _vec(sel_sig, range(nb)))
    return a


def terms_genotype(z, sp: ModelSpec) -> List:
    off, pr = sp.offsets(), sp.priors
    T, B, nn, nb = sp.n_time[0], sp.B, sp.n_neutral, sp.n_bc
    gi = [int(v) for v in sp.geno_idx]
    s_t, lsig_t = _sl(z, off, "s_pop"), _sl(z, off, "logsigma_pop")
    theta, theta_t, ltau = _sl(z, off, "theta"), _sl(z, off, "theta_tilde"), _sl(z, off, "logtau")
    lsig_m, logL = _sl(z, off, "logsigma_bc"), _sl(z, off, "loglambda")
    a = _prior_terms(s_t, *pr["s_pop_prior"])
    a += _prior_terms(lsig_t, *pr["logsigma_pop_prior"])
    a += _prior_terms(theta, *pr["s_bc_prior"])
    a += _prior_terms(theta_t, 0.0, 1.0)
    a += _prior_terms(ltau, *pr["logtau_prior"])
    s_m = [theta[gi[b]] + _exp(ltau[b]) * theta_t[b] for b in range(nb)]
    a += _prior_terms(lsig_m, *pr["logsigma_bc_prior"])
    a += _prior_terms(logL, *pr["loglambda_prior"])
    tot, F, logG = _frequencies(logL, T, B)
    a += _obs_terms(tot, F, sp.counts[0], sp.totals[0])
    a += mvnormal_diag_terms(_vec(logG, range(nn)), _rep([-v for v in s_t], nn), _rep([_exp(v) ** 2 for v in lsig_t], nn))
    a += mvnormal_diag_terms(_vec(logG, range(nn, nn + nb)),
                             [p - q for p, q in zip(_rep_in(s_m, T - 1), _rep(s_t, nb))],
                             _rep_in([_exp(v) ** 2 for v in lsig_m], T - 1))
    return a


def terms_replicate(z, sp: ModelSpec, ragged_quirk: bool = False) -> List:
    """ragged_quirk: the neutral term's pairing as the ragged method writes it (literal.logjoint_replicate)."""
    off, pr = sp.offsets(), sp.priors
    B, nn, nb, Rn, Ts = sp.B, sp.n_neutral, sp.n_bc, sp.n_rep, sp.n_time
    s_t, lsig_t = _sl(z, off, "s_pop"), _sl(z, off, "logsigma_pop")
    theta, theta_t, ltau = _sl(z, off, "theta"), _sl(z, off, "theta_tilde"), _sl(z, off, "logtau")
    lsig_m, logL = _sl(z, off, "logsigma_bc"), _sl(z, off, "loglambda")
    a = _prior_terms(s_t, *pr["s_pop_prior"])
    a += _prior_terms(lsig_t, *pr["logsigma_pop_prior"])
    a += _prior_terms(theta, *pr["s_bc_prior"])
    a += _prior_terms(theta_t, 0.0, 1.0)
    a += _prior_terms(ltau, *pr["logtau_prior"])
    s_m = [p + _exp(q) * r for p, q, r in zip(_rep(theta, Rn), ltau, theta_t)]
    a += _prior_terms(lsig_m, *pr["logsigma_bc_prior"])
    a += _prior_terms(logL, *pr["loglambda_prior"])
    ro, to = 0, 0
    for r in range(Rn):
        T = Ts[r]
        tot, F, logG = _frequencies(logL[ro:ro + T * B], T, B)
        a += _obs_terms(tot, F, sp.counts[r], sp.totals[r])
        st_r, sg_r = s_t[to:to + T - 1], lsig_t[to:to + T - 1]
        s_mr, lsig_mr = s_m[nb * r:nb * (r + 1)], lsig_m[nb * r:nb * (r + 1)]        # column r of reshape(., n_bc, n_rep)
        if ragged_quirk:
            mean_n, var_n = [-v for v in _rep_in(st_r, nn)], _rep_in([_exp(v) ** 2 for v in sg_r], nn)
        else:
            mean_n, var_n = _rep([-v for v in st_r], nn), _rep([_exp(v) ** 2 for v in sg_r], nn)
        a += mvnormal_diag_terms(_vec(logG, range(nn)), mean_n, var_n)
        a += mvnormal_diag_terms(_vec(logG, range(nn, nn + nb)),
                                 [p - q for p, q in zip(_rep_in(s_mr, T - 1), _rep(st_r, nb))],
                                 _rep_in([_exp(v) ** 2 for v in lsig_mr], T - 1))
        ro += T * B
        to += T - 1
    return a


def terms_multienv_replicate(z, sp: ModelSpec) -> List:
    off, pr = sp.offsets(), sp.priors
    B, nn, nb, Rn, E, Ts = sp.B, sp.n_neutral, sp.n_bc, sp.n_rep, sp.n_env, sp.n_time
    s_t, lsig_t = _sl(z, off, "s_pop"), _sl(z, off, "logsigma_pop")
    theta, theta_t, ltau = _sl(z, off, "theta"), _sl(z, off, "theta_tilde"), _sl(z, off, "logtau")
    lsig_m, logL = _sl(z, off, "logsigma_bc"), _sl(z, off, "loglambda")
    a = _prior_terms(s_t, *pr["s_pop_prior"])
    a += _prior_terms(lsig_t, *pr["logsigma_pop_prior"])
    a += _prior_terms(theta, *pr["s_bc_prior"])
    a += _prior_terms(theta_t, 0.0, 1.0)
    a += _prior_terms(ltau, *pr["logtau_prior"])
    s_m = [p + _exp(q) * r for p, q, r in zip(_rep(theta, Rn), ltau, theta_t)]
    a += _prior_terms(lsig_m, *pr["logsigma_bc_prior"])
    a += _prior_terms(logL, *pr["loglambda_prior"])
    ro, to = 0, 0
    for r in range(Rn):
        T = Ts[r]
        env = [int(v) for v in sp.env_idx[r]]
        tot, F, logG = _frequencies(logL[ro:ro + T * B], T, B)
        a += _obs_terms(tot, F, sp.counts[r], sp.totals[r])
        st_r, sg_r = s_t[to:to + T - 1], lsig_t[to:to + T - 1]
        s_m2 = _matrix(s_m[E * nb * r:E * nb * (r + 1)], E, nb)                    # [:, :, r] of reshape(., n_env, n_bc, n_rep)
        lsig_m2 = _matrix(lsig_m[E * nb * r:E * nb * (r + 1)], E, nb)
        a += mvnormal_diag_terms(_vec(logG, range(nn)), _rep([-v for v in st_r], nn), _rep([_exp(v) ** 2 for v in sg_r], nn))
        sel = [s_m2[e] for e in env[1:]]
        sel_sig = [[_exp(v) ** 2 for v in lsig_m2[e]] for e in env[1:]]
        a += mvnormal_diag_terms(_vec(logG, range(nn, nn + nb)),
                                 [p - q for p, q in zip(_vec(sel, range(nb)), _rep(st_r, nb))],
                                 _vec(sel_sig, range(nb)))
        ro += T * B
        to += T - 1
    return a


_TERMS = {
    "fitness": terms_fitness,
    "multienv": terms_multienv,
    "genotype": terms_genotype,
    "replicate": terms_replicate,
    "multienv_replicate": terms_multienv_replicate,
}


def as_mp(z) -> List:
    """fp64 values are taken exactly; mpf values pass through."""
    return [v if isinstance(v, ctx.mpf) else mpf(float(v)) for v in z]


def addends(z, sp: ModelSpec, **kw) -> List:
    return _TERMS[sp.kind](as_mp(z), sp, **kw)


def logjoint(z, sp: ModelSpec, **kw) -> Tuple:
    """(log-joint, scale = sum |addend|), both mpf."""
    a = addends(z, sp, **kw)
    return ctx.fsum(a), ctx.fsum(a, absolute=True)


def grad(z, sp: ModelSpec, **kw) -> Tuple[List, List]:
    """(g, G): g[i] = d logjoint / d z_i by central differences, G[i] = sum over the addends of |d addend / d z_i|."""
    z = as_mp(z)
    h = mpf(H)
    g, G = [], []
    _freeze(False)
    _TERMS[sp.kind](z, sp, **kw)             # fills the memo with everything a perturbed evaluation leaves unchanged
    for i in range(len(z)):
        _freeze(True)
        zi = z[i]
        z[i] = zi + h
        up = _TERMS[sp.kind](z, sp, **kw)
        z[i] = zi - h
        dn = _TERMS[sp.kind](z, sp, **kw)
        z[i] = zi
        d = [(p - q) / (2 * h) for p, q in zip(up, dn) if p is not q]
        g.append(ctx.fsum(d))
        G.append(ctx.fsum(d, absolute=True))
    _freeze(False)
    return g, G


def softplus(x):
    return ctx.log(1 + ctx.exp(x))


def sigmoid(x):
    return 1 / (1 + ctx.exp(-x))
