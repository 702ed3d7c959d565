"""bb_logtau_rb (Rao-Blackwellised logtau marginals, barbay.jl_amd/csrc/bb_ltrb.h) restated from the rule of include/barbay_hip.h,
and the cases the emulation and GPU tests share.  The draws, their keying, ln Z and the unit walk are `_rb_cases`' / `_logsigma_rb_cases`'.

The per-draw rule (`Cond`) is written once for two arithmetics: float64 (numpy; what the engine is compared with) and mpmath at any
precision (what tests/golden/make_logtau_rb_golden.py evaluates at 50 digits).  Both run the same statements; only the number type
and the elementary functions differ.

Expected values: tests/golden/logtau_rb_<mode>_<case>_n<samples>.npz, the 50-digit evaluation of the SAME rule on this restatement's
float64 per-draw inputs (l_j, n, w_j, tt_j, Y_j, a, 1/b^2).  Moments at every n_samples for the entries `golden_cases` names; the
50-digit bisection at n_samples = 2 (one entry), the quantiles elsewhere against the float64 restatement (one entry; at the cap its
median alone).
Bounds: the larger of 1e-12 and 8 x the float64 restatement's own measured error against the goldens (MEASURED / Q_MEASURED),
relative to max(|x|, 1).  n_terms, n_two_modes and the NaN pattern are exact.  Measured, the largest error over all cases and
outputs against the goldens: restatement 4.6e-15 (quantiles 1.6e-15), MI355X 8.9e-14 (tau_mean of an entry with
two-mode draws: e^{l*} times a ratio of sums whose terms reach e^{u} ~ 30 at the far mode); the bound is 1e-12.  Each test prints its
own line; the device run is kept in profiles/logtau_rb/gpu_logtau_rb_tests.log, the table in errors.txt there.  The emulation works
every entry of a call, so it runs the cases of at most 8 300 entry-draws -- every shape at n_samples = 2, the genotype shapes at
111, the eight-entry handles TINY and MTINY at 111, 1000 and 1030 (more draws than threads) --; the device runs all, the cap included.

Inputs: `params` -- `_rb_cases.params` with theta_tilde means of a few hundredths and every theta 0.6 below the units' mean, so that
|Y| is 2 .. 3 and a good part of the FULL conditionals has two modes (`check_bimodal_inputs`).

The rule against the truth: tests/golden/logtau_rb_truth.npz, `mpmath.quad` of the density itself at 40 digits, split at the modes
(found there by a scan of h' for sign changes, not by the rule); what the sets give is in `check_truth`'s docstring."""
import math

import numpy as np

FULL, COLLAPSED = 0, 1
ITER, TAIL, REACH, REACH_MAX, REFINE_MAX, NODES_MAX, MODE_ITER, SEG_ITER = 40, -40.0, 8, 4096, 64, 8192, 100, 60
STOP = 2.0 ** -40
SLACK = 2.0 ** -20         # taken off a quotient before ceil: a quotient that is a whole number but for rounding does not tip over


class F64:
    """float64: numpy's elementary functions on Python floats (scalars) and on arrays of nodes."""
    name = "float64"

    @staticmethod
    def num(x):
        return float(x)

    exp = staticmethod(lambda x: np.exp(x))
    expm1 = staticmethod(lambda x: np.expm1(x))
    log = staticmethod(lambda x: np.log(x))
    log1p = staticmethod(lambda x: np.log1p(x))
    sqrt = staticmethod(lambda x: np.sqrt(x))

    @staticmethod
    def ceil(x):
        return math.ceil(x) if math.isfinite(x) else float("nan")

    @staticmethod
    def finite(x):
        return bool(np.isfinite(x))

    @staticmethod
    def nodes(k0, k1, nleft, s):
        return (np.arange(k0, k1 + 1, dtype=np.float64) - float(nleft)) * s

    @staticmethod
    def total(x):
        return float(np.cumsum(x)[-1])                            # ascending k

    @staticmethod
    def inner_sum(first, p, ulo, sx, N):
        """first + sum of p(ulo + i sx), i = 1 .. N - 1, ascending i."""
        if N <= 1:
            return first
        return float(np.cumsum(np.concatenate([[first], p(ulo + np.arange(1, N, dtype=np.float64) * sx)]))[-1])


class MP:
    """mpmath at the precision in force."""
    name = "mpmath"

    def __init__(self):
        import mpmath
        self.mp = mpmath.mp
        self.exp, self.expm1, self.log, self.log1p, self.sqrt = self.mp.exp, self.mp.expm1, self.mp.log, self.mp.log1p, self.mp.sqrt

    def num(self, x):
        return self.mp.mpf(x)

    def ceil(self, x):
        return int(self.mp.ceil(x))

    def finite(self, x):
        return bool(self.mp.isfinite(x))

    def nodes(self, k0, k1, nleft, s):
        return [(k - nleft) * s for k in range(k0, k1 + 1)]

    def total(self, x):
        return self.mp.fsum(x)

    def inner_sum(self, first, p, ulo, sx, N):
        acc = first
        for i in range(1, N):
            acc += p(ulo + i * sx)
        return acc


class Cond:
    """One draw's conditional: the header's rule, statement by statement.  FULL reads (n, w, tt, Y); COLLAPSED (n, w, Y)."""

    def __init__(self, be, mode, n, w, tt, Y, a, ib2):
        with np.errstate(all="ignore"):
            self._init(be, mode, n, w, tt, Y, a, ib2)

    def _init(self, be, mode, n, w, tt, Y, a, ib2):
        N = be.num
        self.be, self.mode, self.n = be, mode, int(n)
        self.a, self.ib2 = N(a), N(ib2)
        self.prior = self.n == 0                                 # no term: w, tt, Y are not read
        nf = N(self.n)
        if self.prior:
            self.nw = self.A = self.B = self.v = self.q = N(0)
        else:
            w, tt, Y = N(w), N(tt), N(Y)
            self.nw = nf * w
            if mode == FULL:
                self.A, self.B = N(0.5) * self.nw * (tt * tt), (w * tt) * Y
            else:
                self.v, self.q = 1 / self.nw, (Y / nf) * (Y / nf)
                self.c, self.k = self.q - self.v, self.q + self.v
        modes = self._modes()
        # the global mode, the kept ones
        if len(modes) == 2:
            self._anchor(modes[0])
            d = self.lnp(modes[1] - modes[0])
            glob = modes[1] if d > 0 else modes[0]
            kept = modes if abs(d) <= -TAIL else [glob]
        else:
            glob, kept = modes[0], modes
        self._anchor(glob)
        self.kept, self.two = kept, len(kept) == 2
        dls = [1 / be.sqrt(-self.d2(l)) for l in kept]
        dmin = dls[0] if len(dls) == 1 or not dls[1] < dls[0] else dls[1]
        self.dl = dmin
        m = be.ceil(2 * dmin - SLACK) if be.finite(dmin) else 1
        m = min(max(m, 1), REFINE_MAX)
        s = dmin / (4 * m)
        ends = []
        for sign, l, d in ((-1, kept[0], dls[0]), (1, kept[-1], dls[-1])):
            r = 1
            while r < REACH_MAX and self.lnp((l + sign * (REACH * r) * d) - self.lm) > TAIL:
                r *= 2
            ends.append(l + sign * (REACH * r) * d)
        nl, nr = (self.lm - ends[0]) / s, (ends[1] - self.lm) / s
        nl = be.ceil(nl - SLACK) if be.finite(nl) and 1 <= nl <= 1e9 else 1
        nr = be.ceil(nr - SLACK) if be.finite(nr) and 1 <= nr <= 1e9 else 1
        f = (nl + nr + NODES_MAX - 1) // NODES_MAX
        self.s, self.nleft, self.nright = s * f, (nl + f - 1) // f, (nr + f - 1) // f
        self.lo, self.hi = self.lm - self.nleft * self.s, self.lm + self.nright * self.s

    # ---- h' and h'' ---------------------------------------------------------------------------------------------------------------
    def d1(self, l):
        be = self.be
        g = -(l - self.a) * self.ib2
        if self.prior:
            return g
        if self.mode == FULL:
            x = be.exp(l)
            return g + x * (self.B - 2 * self.A * x)
        s = be.exp(2 * l)
        V = s + self.v
        return g + (s / V) * ((self.q - V) / V)

    def d2(self, l):
        be = self.be
        if self.prior:
            return -self.ib2
        if self.mode == FULL:
            x = be.exp(l)
            return -self.ib2 + x * (self.B - 4 * self.A * x)
        return -self.ib2 + self._G(be.exp(2 * l))

    def _G(self, s):
        V = s + self.v
        return 2 * (s / V) * ((self.c * self.v - s * self.k) / V) / V

    # ---- the modes ----------------------------------------------------------------------------------------------------------------
    def _solve(self, lo, hi, x):
        for _ in range(MODE_ITER):
            g = self.d1(x)
            if g == 0 or g != g:                                  # (a NaN h': the mode is NaN)
                return x + g
            if g > 0:
                lo = x
            else:
                hi = x
            c = self.d2(x)
            xn = x - g / c
            if not (c < 0 and xn >= lo and xn <= hi):
                xn = lo + (hi - lo) / 2
            step = xn - x
            x = xn
            if abs(step) <= STOP * (1 + abs(x)):
                break
        g, c = self.d1(x), self.d2(x)                             # one more Newton step where it stays inside: the iteration's last
        xn = x - g / c                                            # step bounds the error by 2^-40 only, this one squares it
        return xn if c < 0 and xn >= lo and xn <= hi else x

    def _modes(self):
        be, a, ib2 = self.be, self.a, self.ib2
        l1 = l2 = None
        if self.prior:
            return [a]
        if self.mode == FULL:
            A, B = self.A, self.B
            if B > 0:
                t = be.log(B / (2 * A))
                L, U = (t, a) if t < a else (a, t)
                disc = B * B - 16 * A * ib2
                if disc > 0:
                    r = be.sqrt(disc)
                    l1, l2 = be.log(2 * ib2 / (B + r)), be.log((B + r) / (8 * A))
            else:
                ea = be.exp(a)
                L, U = a - ea * (2 * A * ea - B) / ib2, a
        else:
            c, k, v = self.c, self.k, self.v
            L = a - 1 / ib2
            U = a
            if c > 0:
                t = be.log(c) / 2
                U = t if t > a else a
                sp = v * c / ((c + k) + be.sqrt(c * c + c * k + k * k))
                if self._G(sp) > ib2:
                    lo, hi = ib2 * v * v / (2 * c), sp
                    for _ in range(SEG_ITER):
                        mid = be.sqrt(lo * hi)
                        if self._G(mid) < ib2:
                            lo = mid
                        else:
                            hi = mid
                    l1 = be.log(be.sqrt(lo * hi)) / 2
                    lo, hi = sp, c * v / k
                    for _ in range(SEG_ITER):
                        mid = be.sqrt(lo * hi)
                        if self._G(mid) > ib2:
                            lo = mid
                        else:
                            hi = mid
                    l2 = be.log(be.sqrt(lo * hi)) / 2
        out = []
        if l1 is not None:
            if self.d1(l1) < 0:
                out.append(self._solve(L, l1, L))
            if self.d1(l2) > 0:
                out.append(self._solve(l2, U, U))
        if not out:
            out.append(self._solve(L, U, U))
        return out

    # ---- the density about the anchor ---------------------------------------------------------------------------------------------
    def _anchor(self, lm):
        be = self.be
        self.lm = lm
        self.c1 = self.ib2 * (lm - self.a)
        if self.prior:
            self.nws = self.be.num(0)
            return
        s = be.exp(2 * lm)
        self.nws = self.nw * s                                    # n w e^{2 l*}
        if self.mode == FULL:
            x = be.exp(lm)
            self.A2 = self.A * (x * x)
            self.D1 = self.B * x - 2 * self.A2
        else:
            V = s + self.v
            self.rho, self.kap = s / V, self.q / (2 * V)

    def lnp(self, u, parts=False):
        """ln p(u) = h(l* + u) - h(l*); with `parts` also e^{2u} (for the pooling factor) and e^u."""
        be = self.be
        g = -(u * self.c1) - self.ib2 * (u * u) / 2
        if self.prior:
            return (g, None, be.exp(u)) if parts else g
        if self.mode == FULL:
            e1 = be.expm1(u)
            g = g + e1 * (self.D1 - self.A2 * e1)
            return (g, (e1 + 1) * (e1 + 1), be.exp(u)) if parts else g
        E2 = be.expm1(2 * u)
        y = self.rho * E2
        g = g - be.log1p(y) / 2 + self.kap * (y / (1 + y))
        return (g, E2 + 1, be.exp(u)) if parts else g

    def _terms(self, u):
        """(p, e^{2u}, e^u) at the nodes u (an array, or a list of numbers)."""
        be = self.be
        if isinstance(u, list):
            rows = [self.lnp(x, True) for x in u]
            return [be.exp(r[0]) for r in rows], [r[1] for r in rows], [r[2] for r in rows]
        g, e2, eu = self.lnp(u, True)
        return be.exp(g), e2, eu

    def moments(self):
        """(Z, E, V, T, P): the normaliser, mean, variance, E[e^l] and E[1 / (1 + n w e^{2l})]."""
        with np.errstate(all="ignore"):
            be, nodes = self.be, self.nleft + self.nright
            u = be.nodes(0, nodes, self.nleft, self.s)
            p, e2, eu = self._terms(u)
            if isinstance(u, list):
                p[0], p[-1] = p[0] / 2, p[-1] / 2
                pool = [be.num(1) if self.prior else 1 / (1 + self.nws * x) for x in e2]
                z, m1, m2 = be.total(p), be.total([a * b for a, b in zip(p, u)]), be.total([a * b * b for a, b in zip(p, u)])
                st, spl = be.total([a * b for a, b in zip(p, eu)]), be.total([a * b for a, b in zip(p, pool)])
            else:
                p = p.copy()
                p[0], p[-1] = p[0] * 0.5, p[-1] * 0.5
                pool = np.ones_like(p) if self.prior else 1.0 / (1.0 + self.nws * e2)
                z, m1, m2, st, spl = be.total(p), be.total(p * u), be.total(p * (u * u)), be.total(p * eu), be.total(p * pool)
            r1 = m1 / z
            self.Z = self.s * z
            return self.Z, self.lm + r1, m2 / z - r1 * r1, be.exp(self.lm) * (st / z), spl / z

    def cdf(self, x):
        with np.errstate(all="ignore"):
            be = self.be
            if x <= self.lo:
                return be.num(0)
            if x >= self.hi:
                return be.num(1)
            r = x - self.lo
            ulo = -(self.nleft * self.s)
            N = max(1, be.ceil(r / self.s))
            sx = r / N
            ux = x - self.lm
            p0, p1 = be.exp(self.lnp(ulo)), be.exp(self.lnp(ux))
            acc = be.inner_sum(p0 / 2, lambda u: be.exp(self.lnp(u)), ulo, sx, N) + p1 / 2
            v = (sx * acc - sx * sx / 12 * (self.d1(x) * p1 - self.d1(self.lo) * p0)) / self.Z
            return min(max(v, be.num(0)), be.num(1)) if v == v else v


# ==== the cases ======================================================================================================================
import ctypes as C  # noqa: E402
import functools  # noqa: E402
import os  # noqa: E402

import _logsigma_rb_cases as lc  # noqa: E402
import _ppc_cases as pc  # noqa: E402
import _rb_cases as rc  # noqa: E402
from barbay_jl_amd import _capi  # noqa: E402
from oracle.spec import ModelSpec  # noqa: E402

UNITS = _capi.LT_UNITS
MODES = ("full", "collapsed")
MODE_ID = _capi.BB_LOGTAU_MODES
MAXN = _capi.BB_LOGTAU_RB_MAX_SAMPLES
MEASURED = 4.6e-15        # the float64 restatement's largest error of the seven moments against the goldens (make_logtau_rb_golden.py --measure)
Q_MEASURED = 1.6e-15      # ... and of the quantiles (n_samples = 2)
SEED, PROBS, NS = rc.SEED, rc.PROBS, rc.NS
TRUTH_AT = (-2.3, -0.7, 0.11, 1.9, 4.4)                           # the CDF's points: E + these x sd of the true conditional
TRUTH_TOL, TRUTH_CTOL = lc.TRUTH_TOL, lc.TRUTH_CTOL
SHAPES = ("genotype_regrouped", "replicate_ragged", "replicate_ragged_method", "multienv_replicate", "genotype_matrix_prior")
PRIOR_ONLY = "multienv_replicate_env0_first"
TINY = "replicate_tiny"
MTINY = "multienv_replicate_tiny"
OVER = 1030                                                       # more draws than the block has threads, no multiple of 64


def quirk_of(case):
    return case == "replicate_ragged_method"


@functools.lru_cache(maxsize=None)
def spec(case):
    if case in SHAPES:
        return lc.spec(case)
    if case == PRIOR_ONLY:                                        # environment 0 at time point 0 only: its units have n = 0
        sp = pc.spec("multienv_replicate")
        return ModelSpec(kind=sp.kind, counts=sp.counts, totals=sp.totals, n_neutral=sp.n_neutral, n_bc=sp.n_bc,
                         env_idx=[[0] + [1] * (T - 1) for T in sp.n_time])
    if case == TINY:                                              # the large n_samples: a handful of entries
        from oracle import fixtures
        return fixtures.synthetic("replicate", B=7, T=[4, 3], n_rep=2, n_neutral=3, seed=3)
    if case == MTINY:                                             # ... with two environments: eight entries again
        from oracle import fixtures
        return fixtures.synthetic("multienv_replicate", B=5, T=[5, 4], n_rep=2, n_env=2, n_neutral=3, seed=3)
    raise KeyError(case)


def n_entries(sp):
    lo, hi = sp.offsets()["logtau"]
    return hi - lo


def params(sp):
    mu, om = rc.params(sp)
    off = sp.offsets()
    g = np.random.default_rng(12)
    ne = n_entries(sp)
    mu[slice(*off["theta_tilde"])] = g.uniform(0.015, 0.09, ne) * np.where(g.random(ne) < 0.8, 1.0, -1.0)
    mu[slice(*off["theta"])] -= 0.6
    mu[slice(*off["logtau"])] = g.normal(-2.0, 0.7, ne)
    return mu, om


@functools.lru_cache(maxsize=None)
def inputs(case):
    sp = spec(case)
    mu, om = params(sp)
    mu.setflags(write=False)
    om.setflags(write=False)
    return sp, mu, om


def engine(lib, case, mu=None, om=None, **kw):
    if quirk_of(case):
        kw["ragged_method"] = True
    if lc.uses_priors(case):
        kw["use_priors"] = True
    if mu is None:
        return lc.make_engine(spec(case), lib, **kw)
    return pc._handle(lib, spec(case), mu, om, **kw)


def golden_cases():
    """name -> (mode, case, n_samples, entries with a golden)."""
    out = {}
    for mode in MODES:
        for c in SHAPES:
            ne = n_entries(spec(c))
            few = tuple(sorted({0, 3, ne // 2, ne - 1}))
            for n in NS:
                more = tuple(sorted(set(few) | {1, ne // 3}))
                out[f"{mode}_{c}_n{n}"] = (mode, c, n, tuple(range(ne)) if n == 2 else more if n == 111 else few)
        for c in (TINY, MTINY):                                   # small handles, every size in the emulation too: the strided draw loop
            ne = n_entries(spec(c))
            for n in (111, 1000, OVER):
                out[f"{mode}_{c}_n{n}"] = (mode, c, n, tuple(range(ne)) if n == 111 else (1, ne - 3))
        out[f"{mode}_{TINY}_n{MAXN}"] = (mode, TINY, MAXN, (1,))  # the cap: device only
    return out


def emu_cases():
    """The golden cases the host emulation works (it works every entry of a call): those of at most 8 300 entry-draws."""
    return sorted(k for k, v in golden_cases().items() if v[2] * n_entries(spec(v[1])) <= 8300)


def golden_path(name):
    return os.path.join(rc.GOLD, f"logtau_rb_{name}.npz")


# ---- the restatement: per-draw inputs ------------------------------------------------------------------------------------------
def cond_inputs(sp, D, n, entries=None):
    """{entry: (l [n], n_terms, w [n], tt [n], Y [n], a, ib2)} from the draws D(i) -> [n] of the caller's latents."""
    off = sp.offsets()
    B, nb, nn, R = sp.B, sp.n_bc, sp.n_neutral, sp.n_rep
    E = rc.n_env(sp)
    pm, ps = sp.prior_arrays()
    want = set(range(n_entries(sp)) if entries is None else (int(x) for x in entries))
    out = {}
    lo_l, g0 = off["loglambda"][0], 0
    for r in range(R):
        T = sp.n_time[r]
        ll = lambda b, t, lo_l=lo_l, T=T: D(lo_l + b * T + t)
        rows = sorted({(x - E * nb * r) // E for x in want if E * nb * r <= x < E * nb * (r + 1)})
        logZ = lc._logz(sp, ll, range(T) if rows else (), n)
        sbar = [D(off["s_pop"][0] + g0 + t) for t in range(T - 1)]
        for mm in rows:
            b = nn + mm
            for e in range(E):
                em = e + E * mm
                u = em + E * nb * r
                if u not in want:
                    continue
                th = int(sp.geno_idx[mm]) if sp.kind == "genotype" else em
                y, cnt = np.zeros(n), 0
                for t in range(T - 1):
                    if rc.env_of(sp, r, t) != e:
                        continue
                    y = y + (((ll(b, t + 1) - ll(b, t)) - (logZ[t + 1] - logZ[t])) + sbar[t])
                    cnt += 1
                i = off["logtau"][0] + u
                w = np.exp(-2.0 * D(off["logsigma_bc"][0] + u))
                Y = y - cnt * D(off["theta"][0] + th)
                out[u] = (D(i), cnt, w, D(off["theta_tilde"][0] + u), Y, pm[i], 1.0 / (ps[i] * ps[i]))
        lo_l += T * B
        g0 += T - 1
    return out


def conds(be, mode, nt, w, tt, Y, a, ib2):
    return [Cond(be, mode, nt, w[j], tt[j], Y[j], a, ib2) for j in range(w.shape[0])]


def entry(be, mode, l, nt, w, tt, Y, a, ib2, probs, want_q=True):
    """The outputs of one entry from its float64 per-draw inputs: the header's rule, in the arithmetic `be`."""
    ns = l.shape[0]
    f64 = be is F64
    tot = lc.reduce_sum if f64 else be.total
    num = float if f64 else be.num
    cs = conds(be, mode, nt, w, tt, Y, a, ib2)
    mom = [c.moments() for c in cs]
    with np.errstate(all="ignore"):
        lj = [num(float(x)) for x in l]
        qm, rm = tot(lj) / ns, tot([m[1] for m in mom]) / ns
        vals = [qm, be.sqrt(tot([(x - qm) ** 2 for x in lj]) / ns), rm,
                be.sqrt(tot([m[2] for m in mom]) / ns + tot([(m[1] - rm) ** 2 for m in mom]) / ns),
                tot([m[3] for m in mom]) / ns, tot([m[4] for m in mom]) / ns, tot([c.lm for c in cs]) / ns]
    two = sum(c.two for c in cs)
    qs = []
    ok = all(be.finite(c.lm) and be.finite(c.s) and be.finite(c.Z) for c in cs)
    for p in (probs if want_q else ()):
        if not ok:
            qs.append(np.nan)
            continue
        lo, hi = min(c.lo for c in cs), max(c.hi for c in cs)
        for _ in range(ITER):
            x = lo + (hi - lo) / 2
            if tot([c.cdf(x) for c in cs]) / ns < num(float(p)):
                lo = x
            else:
                hi = x
        qs.append(lo + (hi - lo) / 2)
    return vals, qs, two


def restate(sp, mode, mu, omega, n, seed, probs=PROBS, draws=None, entries=None, be=F64, want_q=True):
    """bb_logtau_rb at (mu, omega) -- or at the explicit `draws` [n, D] -- for `entries` (all): a dict as Engine.logtau_rb returns,
    the entries' rows only."""
    with np.errstate(all="ignore"):
        D = lc.draws_of(sp, mu, omega, n, seed, draws)
        entries = np.arange(n_entries(sp)) if entries is None else np.asarray(entries)
        ci = cond_inputs(sp, D, n, entries=entries)
        out = {k: np.empty(len(entries)) for k in UNITS}
        out["quantiles"] = np.full((len(entries), len(probs)), np.nan)
        out["n_terms"] = np.array([ci[int(u)][1] for u in entries], dtype=np.int32)
        out["n_two_modes"] = np.zeros(len(entries), dtype=np.int32)
        for x, u in enumerate(entries):
            l, nt, w, tt, Y, a, ib2 = ci[int(u)]
            vals, qs, two = entry(be, MODE_ID[mode], l, nt, w, tt, Y, a, ib2, probs, want_q)
            for k, v in zip(UNITS, vals):
                out[k][x] = float(v)
            out["n_two_modes"][x] = two
            if want_q and len(probs):
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
def errors(got, ref, keys=UNITS + ("quantiles",)):
    """Largest error per output relative to max(|x|, 1); the NaN pattern, n_terms and n_two_modes must be equal."""
    err = {}
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        assert a.shape == b.shape, (k, a.shape, b.shape)
        assert np.array_equal(np.isnan(a), np.isnan(b)), k
        ok = ~np.isnan(b)
        err[k] = float(np.max(np.abs(a[ok] - b[ok]) / np.maximum(np.abs(b[ok]), 1.0))) if ok.any() else 0.0
    for k in ("n_terms", "n_two_modes"):
        if k in ref:
            assert np.array_equal(got[k], ref[k]), (k, got[k], ref[k])
    return err


def tolerances():
    return max(1e-12, 8.0 * MEASURED), max(1e-12, 8.0 * Q_MEASURED)


def assert_within(err, who):
    tol, qtol = tolerances()
    for k, v in err.items():
        assert v <= (qtol if k == "quantiles" else tol), (who, k, v)


def report(name, label, err):
    print(f"logtau_rb case {name:44s} {label:12s} " + " ".join(f"{k} {err[k] / 1e-16:7.1f}" for k in err) + "  (1e-16)")


def take(res, entries):
    return {k: v[list(entries)] for k, v in res.items()}


def ltrb(e, mode, n, **kw):
    kw.setdefault("probs", PROBS)
    kw.setdefault("seed", SEED)
    return e.logtau_rb(mode=mode, n_samples=n, **kw)


def both(e, n, **kw):
    out = {}
    for mode in MODES:
        out.update({f"{mode}_{k}": v for k, v in ltrb(e, mode, n, **kw).items()})
    return out


same_bytes = rc.same_bytes


# ---- 1. the rule against the truth ---------------------------------------------------------------------------------------------
def check_truth():
    """The float64 restatement's ln Z, E, V, E[e^l], the pooling expectation and C against `mpmath.quad` of the density itself
    (stored by the golden maker, split at the modes it finds by a scan), and the number of kept modes against the truth's: on the
    cases' own per-draw inputs, seven sets chosen from a sweep over parameters of use (six of them bimodal) and sets with n = 0, tt = 0, Y = 0, w from 1e-6
    to 1e8, b from 0.2 to 3.  Bounds: 4e-12 for the moments (ln Z absolute, E in units of the smallest kept delta, V, E[e^l] and the
    pooling expectation relative), 3e-5 absolute for C.  Measured on the 58 sets (11 of them bimodal; 97 .. 577 nodes a draw):
      ln Z 3.2e-15   E 8.9e-14 delta   V 2.2e-15   E[e^l] 1.6e-14   pooling 5.8e-15   C 3.2e-06"""
    t = golden("truth")
    worst = {"lnZ": 0.0, "E": 0.0, "V": 0.0, "T": 0.0, "P": 0.0, "C": 0.0}
    nodes = []
    for i in range(t["n"].shape[0]):
        c = Cond(F64, int(t["mode"][i]), int(t["n"][i]), float(t["w"][i]), float(t["tt"][i]), float(t["Y"][i]), float(t["a"][i]), float(t["ib2"][i]))
        Z, E, V, T, P = c.moments()
        assert len(c.kept) == int(t["n_modes"][i]), (i, c.kept, t["n_modes"][i])
        assert abs(c.lm - t["glob"][i]) <= 1e-10 * max(1.0, abs(t["glob"][i])), i
        nodes.append(c.nleft + c.nright + 1)
        e = {"lnZ": abs(np.log(Z) - t["lnZ"][i]), "E": abs(E - t["E"][i]) / c.dl, "V": abs(V / t["V"][i] - 1.0), "T": abs(T / t["T"][i] - 1.0),
             "P": abs(P / t["P"][i] - 1.0), "C": max(abs(c.cdf(float(t["x"][i, k])) - t["C"][i, k]) for k in range(len(TRUTH_AT)))}
        for k in worst:
            worst[k] = max(worst[k], float(e[k]))
    print(f"logtau_rb rule against mpmath.quad, {t['n'].shape[0]} sets, {int((t['n_modes'] == 2).sum())} bimodal, nodes {min(nodes)}..{max(nodes)}:",
          " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= (TRUTH_CTOL if k == "C" else TRUTH_TOL), (k, v)


def check_collapsed_identity():
    """exp(h_c(l)) = the integral over tt of exp(h(l; tt)) N(tt; 0, 1) up to a factor free of l: on the truth file's COLLAPSED sets
    the restatement's ln p about the mode against the logarithm of the ratio of two 30-digit quadratures over tt, at five l."""
    import mpmath as mp
    mp.mp.dps = 30
    t = golden("truth")
    worst = 0.0
    for i in range(t["n"].shape[0]):
        if int(t["mode"][i]) != COLLAPSED or int(t["n"][i]) == 0:
            continue
        n, w, Y, a, ib2 = int(t["n"][i]), mp.mpf(float(t["w"][i])), mp.mpf(float(t["Y"][i])), float(t["a"][i]), float(t["ib2"][i])
        c = Cond(F64, COLLAPSED, n, float(w), 0.0, float(Y), a, ib2)

        def marg(l):                                               # ln of the integral, the prior of l left out; the integrand's
            x = mp.exp(l)                                          # own peak taken out so that the quadrature sees O(1) numbers
            A, B = n * w * x * x / 2, w * x * Y
            pk = B / (2 * A + 1)
            sd = 1 / mp.sqrt(2 * A + 1)
            f = lambda tt: mp.exp(-A * tt * tt + B * tt - tt * tt / 2 - (B * pk / 2))
            return mp.log(mp.quad(f, [pk - 40 * sd, pk - 5 * sd, pk, pk + 5 * sd, pk + 40 * sd])) + B * pk / 2
        m0 = marg(mp.mpf(float(c.lm)))
        for u in (-1.3, -0.4, 0.2, 0.9, 2.1):
            want = float(marg(mp.mpf(float(c.lm)) + mp.mpf(u)) - m0 - (mp.mpf(u) * float(c.c1) + mp.mpf(ib2) * mp.mpf(u) ** 2 / 2))
            got = float(c.lnp(u))
            worst = max(worst, abs(got - want) / max(1.0, abs(want)))
    print(f"logtau_rb collapsed identity: ln p against the quadrature over theta_tilde, largest error {worst:.2e}")
    assert worst <= 1e-12


def check_bimodal_inputs():
    """The condition on the inputs: a golden case has an entry with 0.1 n_samples < n_two_modes < 0.9 n_samples (restatement only)."""
    hits = []
    for name, (mode, case, n, ents) in golden_cases().items():
        if n != 111 or mode != "full":
            continue
        sp, mu, om = inputs(case)
        r = restate(sp, mode, mu, om, n, SEED, entries=ents, want_q=False)
        hits += [(name, int(u), int(k)) for u, k in zip(ents, r["n_two_modes"]) if 0.1 * n < k < 0.9 * n]
    print("logtau_rb entries with a mixed number of two-mode draws:", hits)
    assert hits


# ---- 2. golden values ----------------------------------------------------------------------------------------------------------
def check_golden(lib, name, label):
    mode, case, n, ents = golden_cases()[name]
    sp, mu, om = inputs(case)
    ref = golden(name)
    ents = list(ents)
    r64 = restate(sp, mode, mu, om, n, SEED, entries=ents, want_q=False)
    mom = {k: ref[k] for k in UNITS + ("n_terms", "n_two_modes")}
    e0 = errors(r64, mom, UNITS)
    with engine(lib, case, mu, om) as e:
        got = ltrb(e, mode, n)
    assert got["quantiles"].shape == (n_entries(sp), len(PROBS)) and np.all(np.diff(got["quantiles"], axis=1) > 0)
    err = errors(take(got, ents), mom, UNITS)
    if "quantiles" in ref:                                        # 50-digit bisection (n = 2)
        qe = [int(x) for x in ref["q_entries"]]
        rq = restate(sp, mode, mu, om, n, SEED, entries=qe)
        e0["quantiles"] = errors({"quantiles": rq["quantiles"]}, {"quantiles": ref["quantiles"]}, ("quantiles",))["quantiles"]
        err["quantiles"] = errors({"quantiles": got["quantiles"][qe]}, {"quantiles": ref["quantiles"]}, ("quantiles",))["quantiles"]
    elif n == MAXN:                                               # the cap: the median alone (a bisection is its quantile's own), 40 mixture
        qe = [u for u, nt in zip(ents, ref["n_terms"]) if nt > 0][:1]      # CDFs of 5781 draws in the restatement, not 120
        rq = restate(sp, mode, mu, om, n, SEED, entries=qe, probs=PROBS[1:2])
        err["quantiles"] = errors({"quantiles": got["quantiles"][qe][:, 1:2]}, {"quantiles": rq["quantiles"]}, ("quantiles",))["quantiles"]
    else:                                                         # the float64 restatement, one entry with terms
        qe = [u for u, nt in zip(ents, ref["n_terms"]) if nt > 0][:1]
        rq = restate(sp, mode, mu, om, n, SEED, entries=qe)
        err["quantiles"] = errors({"quantiles": got["quantiles"][qe]}, {"quantiles": rq["quantiles"]}, ("quantiles",))["quantiles"]
    report(name, "restatement", e0)
    report(name, label, err)
    assert_within(e0, "restatement")
    assert_within(err, label)


# ---- 3. the identity against the log-joint -----------------------------------------------------------------------------------------
IDENTITY = SHAPES + (PRIOR_ONLY,)


def check_identity(lib, name, device=False):
    """A point z passed as one explicit draw (FULL); z' = z with every logtau entry at its mode_mean, the global mode: the gradient of
    the log-joint at z' vanishes there to within 2^-30 (-h''(l*)) (1 + |l*|), -h'' from the restatement's own inputs; with one
    draw the outputs are the conditional itself."""
    from oracle import literal
    quirk = quirk_of(name)
    sp = spec(name)
    sl = slice(*sp.offsets()["logtau"])
    g = np.random.default_rng(8)
    with engine(lib, name, seed=1) as e:
        assert e.logtau_rb_shape() == sl.stop - sl.start == n_entries(sp)
        for scale in (0.3, 1.0):
            z = g.normal(0.0, scale, sp.D)
            z[sl] = g.normal(-2.0, 1.0, sl.stop - sl.start)
            got = e.logtau_rb(mode="full", probs=(), draws=z)
            ref = restate(sp, "full", None, None, 1, 0, probs=(), draws=z[None, :])
            assert np.array_equal(got["n_terms"], ref["n_terms"]) and np.array_equal(got["n_two_modes"], ref["n_two_modes"])
            assert np.all(got["q_sd"] == 0.0) and np.array_equal(got["q_mean"], z[sl])
            assert_within(errors(got, ref, UNITS), "one draw")
            z2 = z.copy()
            z2[sl] = got["mode_mean"]
            ci = cond_inputs(sp, rc.Rows(z[None, :]), 1)
            curv = np.array([-Cond(F64, FULL, ci[u][1], ci[u][2][0], ci[u][3][0], ci[u][4][0], ci[u][5], ci[u][6]).d2(got["mode_mean"][u])
                             for u in range(n_entries(sp))])
            bound = 2.0 ** -30 * curv * (1.0 + np.abs(got["mode_mean"]))
            grad = literal.logjoint_and_grad(z2, sp, **(dict(ragged_quirk=True) if quirk else {}))[1]
            worst = np.max(np.abs(grad[sl]) / bound)
            print(f"logtau_rb identity {name:30s} sd {scale}: |dlogp/dlogtau| at the modes at most {worst:.2e} of the bound; two-mode entries {int(got['n_two_modes'].sum())}")
            assert np.all(np.abs(grad[sl]) <= bound), worst
            if device:
                gd = e.logdensity_grad(z2)[1]
                assert np.all(np.abs(gd[sl]) <= bound)


# ---- 4. prior-only entries -----------------------------------------------------------------------------------------------------
def check_prior_only(lib, n=9):
    """PRIOR_ONLY: the units of environment 0 have n = 0; their conditional is the prior N(a, b) in both modes, pool_mean is 1
    exactly -- and a NaN logsigma of such a unit reaches nothing."""
    from scipy.special import ndtri
    sp, mu, om = inputs(PRIOR_ONLY)
    E = rc.n_env(sp)
    u0 = np.arange(0, n_entries(sp), E)
    pm, ps = sp.prior_arrays()
    sl = slice(*sp.offsets()["logtau"])
    a, b = pm[sl][u0], ps[sl][u0]
    mu2 = mu.copy()
    mu2[sp.offsets()["logsigma_bc"][0] + u0[2]] = np.nan
    probs = (0.001, 0.025, 0.5, 0.975, 0.999)
    for mode in MODES:
        with engine(lib, PRIOR_ONLY, mu, om) as e:
            got = ltrb(e, mode, n, probs=probs)
        with engine(lib, PRIOR_ONLY, mu2, om) as e:
            got2 = ltrb(e, mode, n, probs=probs)
        assert same_bytes(got, got2)
        assert np.all(got["n_terms"][u0] == 0) and np.all(got["n_terms"][u0 + 1] > 0) and np.all(got["n_two_modes"][u0] == 0)
        assert np.all(got["pool_mean"][u0] == 1.0) and np.all(got["pool_mean"][u0 + 1] < 1.0)
        assert np.array_equal(got["rb_mean"][u0], a) and np.array_equal(got["mode_mean"][u0], a)
        assert np.all(np.abs(got["rb_sd"][u0] / b - 1.0) <= 1e-12)
        assert np.all(np.abs(got["tau_mean"][u0] / np.exp(a + b * b / 2.0) - 1.0) <= 1e-12)
        for i, p in enumerate(probs):
            zq = ndtri(p)
            phi = np.exp(-0.5 * zq * zq) / np.sqrt(2.0 * np.pi)
            d = np.abs(got["quantiles"][u0, i] - (a + b * zq))
            assert np.all(d <= 3e-5 * b / phi), (mode, p, d.max())


# ---- 5. family checks ------------------------------------------------------------------------------------------------------------
def check_launch_modes(lib, case="genotype_regrouped"):
    import barbay_jl_amd as bb
    sp, mu, om = inputs(case)
    out = []
    for lm in (1, 0):
        with bb.Engine(sp.kind, sp.counts, sp.n_neutral, sp.n_bc, env_idx=sp.env_idx, geno_idx=sp.geno_idx, seed=4, launch_mode=lm, _lib=lib) as e:
            e.set_params(mu, om)
            out.append(both(e, 9, seed=2))
            out.append(both(e, 9, seed=2))
    assert all(same_bytes(out[0], o) for o in out[1:])


GROUP_CASES = ("genotype_regrouped", "replicate_ragged")


def check_group_handle(lib, case):
    sp, mu, om = inputs(case)
    with pc._handle(lib, sp, mu, om, device_ids=[0, 0]) as e:
        a = both(e, 17)
    with pc._handle(lib, sp, mu, om) as e:
        b = both(e, 17)
    assert same_bytes(a, b)


def check_buffer_reuse(lib):
    """The call interleaved with the other post-fit calls at changing sizes and across its two modes on one handle: every result is
    byte for byte what a fresh handle gives."""
    sp, mu, om = inputs(TINY)
    dr = rc.materialise(sp, mu, om, 7, 3)
    calls = [lambda e: ltrb(e, "full", 111),
             lambda e: e.ppc_bands((0.95, 0.675, 0.05), n_samples=111, n_ppc=7, seed=SEED),
             lambda e: ltrb(e, "collapsed", 300),
             lambda e: rc.rb(e, 200),
             lambda e: ltrb(e, "full", 2),
             lambda e: lc.lrb(e, "bc", 111),
             lambda e: ltrb(e, "collapsed", 7, draws=dr),
             lambda e: ltrb(e, "full", 1030, probs=(0.5,)),
             lambda e: ltrb(e, "collapsed", 2),
             lambda e: ltrb(e, "full", 111)]
    with pc._handle(lib, sp, mu, om) as e:
        got = [pc._bits(f(e)) for f in calls]
    for i, f in enumerate(calls):
        with pc._handle(lib, sp, mu, om) as e:
            assert got[i] == pc._bits(f(e)), i
    assert got[0] == got[-1]


def check_handle_untouched(lib):
    sp = spec("genotype_regrouped")
    with lc.make_engine(sp, lib, seed=5) as a, lc.make_engine(sp, lib, seed=5) as b:
        both(b, 16)
        for x, y in zip(a.get_params(), b.get_params()):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
        a.run(5)
        both(b, 8, seed=1)
        b.run(5)
        for x, y in zip(a.get_params(), b.get_params()):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64))


def check_internal_against_explicit_draws(lib, case, n=9):
    sp, mu, om = inputs(case)
    dr = rc.materialise(sp, mu, om, n, SEED)
    with engine(lib, case, mu, om) as e:
        for mode in MODES:
            a, b = ltrb(e, mode, n), ltrb(e, mode, n, draws=dr)
            assert same_bytes(b, ltrb(e, mode, 5, draws=dr))      # n_samples is the row count; the argument is ignored
            err = errors(a, b)
            report(f"{mode}_{case}_n{n}", "own/explicit", err)
            assert_within(err, "explicit draws")


def check_nan_stays(lib, case="multienv_replicate", n=9):
    """A NaN mean of one unit's theta_tilde: exactly that entry's FULL conditionals are NaN (its own draws are not), and COLLAPSED,
    which does not read theta_tilde, does not change a bit; a NaN mean of one unit's logsigma_bc: that entry in both modes.  No
    other entry changes a bit."""
    sp, mu, om = inputs(case)
    E, off = rc.n_env(sp), sp.offsets()
    u = 0 + E * 5 + E * sp.n_bc * 1
    v = 1 + E * 2
    mu2 = mu.copy()
    mu2[off["theta_tilde"][0] + u] = np.nan
    mu2[off["logsigma_bc"][0] + v] = np.nan
    with pc._handle(lib, sp, mu, om) as e:
        base = {m: ltrb(e, m, n) for m in MODES}
    with pc._handle(lib, sp, mu2, om) as e:
        got = {m: ltrb(e, m, n) for m in MODES}
    cond = ("rb_mean", "rb_sd", "tau_mean", "pool_mean", "mode_mean", "quantiles")
    keep = ("q_mean", "q_sd", "n_terms")
    for m, bad in (("full", [u, v]), ("collapsed", [v])):
        rest = np.setdiff1d(np.arange(n_entries(sp)), bad)
        assert same_bytes({k: x[rest] for k, x in got[m].items()}, {k: x[rest] for k, x in base[m].items()}), m
        for k in cond:
            assert np.all(np.isnan(got[m][k][bad])), (m, k)
        assert same_bytes({k: got[m][k][bad] for k in keep}, {k: base[m][k][bad] for k in keep})


def check_more_quantiles(lib, label, case=TINY, n=33):
    """Four and eight quantiles, 0.001 and 0.999 among them, against the restatement."""
    sp, mu, om = inputs(case)
    for probs in ((0.001, 0.25, 0.75, 0.999), (0.001, 0.025, 0.16, 0.5, 0.84, 0.975, 0.99, 0.999)):
        for mode in MODES:
            ents = [1, n_entries(sp) - 1]
            ref = restate(sp, mode, mu, om, n, SEED, probs=probs, entries=ents)
            with engine(lib, case, mu, om) as e:
                got = ltrb(e, mode, n, probs=probs)
            err = errors(take(got, ents), ref)
            report(f"{mode}_{case}_n{n}_q{len(probs)}", label, err)
            assert_within(err, label)


# ---- 6. errors ------------------------------------------------------------------------------------------------------------------
OUTS = UNITS + ("quantiles", "n_terms", "n_two_modes")


def raw(engine_, n_samples, mode=0, probs=PROBS, seed=SEED, draws=None, null=(), want=OUTS, n_quantiles=None):
    """bb_logtau_rb through ctypes with only the outputs in `want` non-NULL; `null` names arguments passed as NULL."""
    ne = engine_.logtau_rb_shape()
    p = np.ascontiguousarray(probs, dtype=np.float64)
    o = _capi.bb_logtau_rb_opts()
    o.mode, o.n_samples, o.n_quantiles, o.seed = mode, n_samples, len(p) if n_quantiles is None else n_quantiles, seed
    o.probs = None if "probs" in null or not len(p) else _capi._ptr(p)
    if draws is not None:
        o.draws = _capi._ptr(draws)
    res, out = {}, _capi.bb_logtau_rb_out()
    for k in want:
        if k in ("n_terms", "n_two_modes"):
            res[k] = np.full(ne, -7, dtype=np.int32)
            setattr(out, k, res[k].ctypes.data_as(C.POINTER(C.c_int32)))
        else:
            res[k] = np.full((ne, len(p)) if k == "quantiles" else ne, -7.0)
            setattr(out, k, _capi._ptr(res[k]))
    rcode = engine_._lib.bb_logtau_rb(None if "h" in null else engine_._h, None if "o" in null else C.byref(o),
                                      None if "out" in null else C.byref(out))
    return rcode, res


def check_errors(lib):
    """Every BB_ERR_INVALID and BB_ERR_UNSUPPORTED of the contract, with a message.  NOT exercised: BB_ERR_DEVICE for what the device
    cannot allocate (a test on a shared machine does not take the device's whole memory)."""
    sp, mu, om = inputs(TINY)
    INVALID, UNSUPPORTED = -1, _capi.BB_ERR_UNSUPPORTED
    msg = lambda: lib.bb_last_error().decode()
    dr = rc.materialise(sp, mu, om, 3, 1)
    with pc._handle(lib, sp, mu, om) as e:
        for null in ("h", "o", "out"):
            assert raw(e, 10, null=(null,))[0] == INVALID and msg(), null
        for md in (-1, 2, 7):
            assert raw(e, 10, mode=md)[0] == INVALID and "mode" in msg(), md
        for nq in (-1, 9):
            assert raw(e, 10, n_quantiles=nq)[0] == INVALID and "n_quantiles" in msg(), nq
        assert raw(e, 10, null=("probs",), n_quantiles=3)[0] == INVALID and "probs" in msg()
        for bad in (0.0, 1.0, -0.1, 1.5, np.nan):
            assert raw(e, 10, probs=(0.5, bad))[0] == INVALID and "prob" in msg(), bad
        for n in (1, 0, -3, MAXN + 1):
            assert raw(e, n)[0] == UNSUPPORTED and "n_samples" in msg(), n
        for n in (0, MAXN + 1):
            assert raw(e, n, draws=dr)[0] == UNSUPPORTED and "n_samples" in msg(), n
        for md, name in enumerate(MODES):
            assert raw(e, 1, mode=md, draws=dr)[0] == 0 and raw(e, 3, mode=md, draws=dr)[0] == 0      # one explicit draw is served
            assert raw(e, 16, mode=md, want=())[0] == 0                                  # an all-NULL out
            assert raw(e, 16, mode=md, probs=())[0] == 0                                 # no quantiles
            full = ltrb(e, name, 16)
            assert same_bytes(raw(e, 16, mode=md)[1], full)
            for k in OUTS:                                                               # every output NULL except one
                rcode, one = raw(e, 16, mode=md, want=(k,))
                assert rcode == 0 and same_bytes(one, {k: full[k]}), k
        for call, word in ((lambda: e.logtau_rb(n_samples=1), "n_samples"), (lambda: e.logtau_rb(mode="tau"), "mode"),
                           (lambda: e.logtau_rb(draws=np.zeros((3, sp.D + 1))), "draws")):
            try:
                call()
            except _capi.BarBayHipError as ex:
                assert word in str(ex)
            else:
                raise AssertionError("no error")
    for case, kind in (("fitness", "BB_MODEL_FITNESS"), ("multienv", "BB_MODEL_MULTIENV")):      # the kinds without a logtau
        with lc.make_engine(pc.spec(case), lib) as e:
            assert e.logtau_rb_shape() == 0
            o, out = _capi.bb_logtau_rb_opts(), _capi.bb_logtau_rb_out()
            o.mode, o.n_samples = 0, 10
            assert lib.bb_logtau_rb(e._h, C.byref(o), C.byref(out)) == UNSUPPORTED and kind in msg(), case


# ---- 7. the rule on many draws at once -----------------------------------------------------------------------------------------
def moments_many(mode, nt, w, tt, Y, a, ib2, chunk=8192):
    """(E, V, T, P) [n] of `Cond(F64, ...)` for arrays of draws: the same statements on arrays (masks where `Cond` branches, the
    grids padded to the longest of a chunk), for the statistical check's 200 000 draws; `check_many` holds it to `Cond`."""
    n = w.shape[0]
    out = [np.empty(n) for _ in range(4)]
    for i0 in range(0, n, chunk):
        sl = slice(i0, min(i0 + chunk, n))
        for o, v in zip(out, _many(mode, nt, w[sl], tt[sl], Y[sl], a, ib2)):
            o[sl] = v
    return out


def _many(mode, nt, w, tt, Y, a, ib2):
    with np.errstate(all="ignore"):
        n = w.shape[0]
        prior = nt == 0
        nw = nt * w
        if mode == FULL:
            A, B = 0.5 * nw * (tt * tt), (w * tt) * Y
        else:
            v, q = 1.0 / nw, (Y / nt) * (Y / nt)
            c, k = q - v, q + v

        def G(s):
            V = s + v
            return 2.0 * (s / V) * ((c * v - s * k) / V) / V

        def d1(l):
            g = -(l - a) * ib2
            if prior:
                return g
            if mode == FULL:
                x = np.exp(l)
                return g + x * (B - 2.0 * A * x)
            s = np.exp(2.0 * l)
            V = s + v
            return g + (s / V) * ((q - V) / V)

        def d2(l):
            if prior:
                return np.full(n, -ib2)
            if mode == FULL:
                x = np.exp(l)
                return -ib2 + x * (B - 4.0 * A * x)
            return -ib2 + G(np.exp(2.0 * l))

        def solve(lo, hi, x):
            lo, hi, x = lo.copy(), hi.copy(), x.copy()
            act = np.ones(n, dtype=bool)
            for _ in range(MODE_ITER):
                g = d1(x)
                x = np.where(act & (g != g), g, x)
                act &= (g != 0.0) & (g == g)
                if not act.any():
                    break
                lo = np.where(act & (g > 0), x, lo)
                hi = np.where(act & ~(g > 0), x, hi)
                cv = d2(x)
                xn = x - g / cv
                xn = np.where((cv < 0) & (xn >= lo) & (xn <= hi), xn, lo + (hi - lo) / 2.0)
                step = xn - x
                x = np.where(act, xn, x)
                act &= ~(np.abs(step) <= STOP * (1.0 + np.abs(x)))
            g, cv = d1(x), d2(x)
            xn = x - g / cv
            return np.where((g != 0.0) & (cv < 0) & (xn >= lo) & (xn <= hi), xn, x)

        av = np.full(n, float(a))
        split = np.zeros(n, dtype=bool)
        l1 = l2 = av
        if prior:
            L = U = av
        elif mode == FULL:
            pos = B > 0
            t = np.log(B / (2.0 * A))
            ea = np.exp(a)
            L = np.where(pos, np.minimum(av, t), a - ea * (2.0 * A * ea - B) / ib2)
            U = np.where(pos, np.where(t < av, av, t), av)
            disc = B * B - 16.0 * A * ib2
            split = pos & (disc > 0)
            r = np.sqrt(np.where(split, disc, 1.0))
            l1, l2 = np.log(2.0 * ib2 / (B + r)), np.log((B + r) / (8.0 * A))
        else:
            L = np.full(n, a - 1.0 / ib2)
            t = np.log(c) / 2.0
            U = np.where((c > 0) & (t > av), t, av)
            sp = v * c / ((c + k) + np.sqrt(c * c + c * k + k * k))
            split = (c > 0) & (G(sp) > ib2)
            lo, hi = ib2 * v * v / (2.0 * c), sp.copy()
            for _ in range(SEG_ITER):
                mid = np.sqrt(lo * hi)
                left = G(mid) < ib2
                lo, hi = np.where(left, mid, lo), np.where(left, hi, mid)
            l1 = np.log(np.sqrt(lo * hi)) / 2.0
            lo, hi = sp.copy(), c * v / k
            for _ in range(SEG_ITER):
                mid = np.sqrt(lo * hi)
                left = G(mid) > ib2
                lo, hi = np.where(left, mid, lo), np.where(left, hi, mid)
            l2 = np.log(np.sqrt(lo * hi)) / 2.0
        if prior:
            m0, m1, has0, has1 = av, av, np.ones(n, dtype=bool), np.zeros(n, dtype=bool)
        else:
            has0 = split & (d1(np.where(split, l1, av)) < 0)
            has1 = split & (d1(np.where(split, l2, av)) > 0)
            one = ~(has0 | has1)
            ma = solve(L, np.where(split, l1, U), L)
            mb = solve(np.where(split, l2, L), U, U)
            mc = solve(L, U, U)
            m0 = np.where(one, mc, np.where(has0, ma, mb))
            m1 = np.where(has0 & has1, mb, m0)
        both_ = has0 & has1

        def anchor(lm):
            g1 = ib2 * (lm - a)
            s = np.exp(2.0 * lm)
            if prior:
                return lm, g1, np.zeros(n), None, None
            if mode == FULL:
                x = np.exp(lm)
                A2 = A * (x * x)
                return lm, g1, nw * s, A2, B * x - 2.0 * A2
            V = s + v
            return lm, g1, nw * s, s / V, q / (2.0 * V)

        def lnp(an, u, parts=False):
            lm, g1, nws, k0, k1 = an
            col = (lambda x: x[:, None]) if np.ndim(u) == 2 else (lambda x: x)
            g = -(u * col(g1)) - ib2 * (u * u) / 2.0
            if prior:
                return (g, np.ones_like(u)) if parts else g
            if mode == FULL:
                e1 = np.expm1(u)
                g = g + e1 * (col(k1) - col(k0) * e1)
                return (g, (e1 + 1.0) * (e1 + 1.0)) if parts else g
            E2 = np.expm1(2.0 * u)
            y = col(k0) * E2
            g = g - np.log1p(y) / 2.0 + col(k1) * (y / (1.0 + y))
            return (g, E2 + 1.0) if parts else g

        d = np.where(both_, lnp(anchor(m0), m1 - m0), 0.0)
        glob = np.where(both_ & (d > 0), m1, m0)
        kept2 = both_ & (np.abs(d) <= -TAIL)
        left, right = np.where(kept2, m0, glob), np.where(kept2, m1, glob)
        an = anchor(glob)
        dl0 = 1.0 / np.sqrt(-d2(left))
        dl1 = np.where(kept2, 1.0 / np.sqrt(-d2(right)), dl0)
        dmin = np.where(~kept2 | ~(dl1 < dl0), dl0, dl1)
        m = np.clip(np.where(np.isfinite(dmin), np.ceil(2.0 * dmin - SLACK), 1.0), 1.0, float(REFINE_MAX))
        s = dmin / (4.0 * m)
        ends = []
        for sign, lmode, dd in ((-1.0, left, dl0), (1.0, right, dl1)):
            r = np.ones(n)
            while True:
                more = (r < REACH_MAX) & (lnp(an, (lmode + sign * (REACH * r) * dd) - glob) > TAIL)
                if not more.any():
                    break
                r = np.where(more, 2.0 * r, r)
            ends.append(lmode + sign * (REACH * r) * dd)
        cnt = lambda x: np.where((x >= 1.0) & (x <= 1e9), np.ceil(x - SLACK), 1.0).astype(np.int64)
        nl, nr = cnt((glob - ends[0]) / s), cnt((ends[1] - glob) / s)
        f = (nl + nr + NODES_MAX - 1) // NODES_MAX
        s, nleft, nright = s * f, (nl + f - 1) // f, (nr + f - 1) // f
        nodes = nleft + nright
        kk = np.arange(int(nodes.max()) + 1)[None, :]
        u = (kk - nleft[:, None]) * s[:, None]
        g, e2 = lnp(an, u, True)
        wgt = np.where(kk <= nodes[:, None], np.where((kk == 0) | (kk == nodes[:, None]), 0.5, 1.0), 0.0)
        p = np.where(wgt > 0, np.exp(g) * wgt, 0.0)
        u = np.where(wgt > 0, u, 0.0)
        pool = 1.0 if prior else 1.0 / (1.0 + an[2][:, None] * np.where(wgt > 0, e2, 0.0))
        z = p.sum(axis=1)
        r1 = (p * u).sum(axis=1) / z
        return glob + r1, (p * (u * u)).sum(axis=1) / z - r1 * r1, np.exp(glob) * ((p * np.exp(u)).sum(axis=1) / z), (p * pool).sum(axis=1) / z


def check_many(n=300):
    """`moments_many` against `Cond` on the TINY case's draws, both modes, and on the truth file's sets."""
    sp, mu, om = inputs(TINY)
    ci = cond_inputs(sp, lc.draws_of(sp, mu, om, n, SEED), n)
    worst = 0.0
    for mode in (FULL, COLLAPSED):
        for u, (l, nt, w, tt, Y, a, ib2) in ci.items():
            ref = np.array([c.moments()[1:] for c in conds(F64, mode, nt, w, tt, Y, a, ib2)]).T
            got = moments_many(mode, nt, w, tt, Y, a, ib2)
            worst = max(worst, max(float(np.max(np.abs(g - r) / np.maximum(np.abs(r), 1.0))) for g, r in zip(got, ref)))
    t = golden("truth")
    for i in range(t["n"].shape[0]):
        args = (int(t["mode"][i]), int(t["n"][i]), np.array([t["w"][i]]), np.array([t["tt"][i]]), np.array([t["Y"][i]]), float(t["a"][i]), float(t["ib2"][i]))
        ref = Cond(F64, args[0], args[1], args[2][0], args[3][0], args[4][0], args[5], args[6]).moments()[1:]
        got = moments_many(*args)
        worst = max(worst, max(abs(float(g[0]) - float(r)) / max(abs(float(r)), 1.0) for g, r in zip(got, ref)))
    print(f"logtau_rb: the vectorised restatement against the per-draw one, largest difference {worst:.2e}")
    assert worst <= 1e-11
