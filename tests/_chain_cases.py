"""bb_chain_summary (chain diagnostics, barbay.jl_amd/csrc/bb_chain.h) restated in plain numpy from the formulas of
include/barbay_hip.h -- direct lag sums, no FFT -- and the cases the emulation and GPU tests share.

The restatement runs twice, in float64 and in np.longdouble.  The library is compared against the longdouble one; per statistic
and case the allowed relative error (the largest over the case's columns) is 8 x the largest error of the float64 restatement
against the longdouble one on the same input, floored at 4 ulp of a double: a bound taken from the reference's own error and the
number format, the factor 8 covering a different but fixed summation order.  n_lags must be equal, quantiles equal within
`_ppc_cases.assert_bands_close`'s tolerance.

Measured, largest relative error over a case's columns against the longdouble restatement (x86-64, 80-bit long double), float64
restatement / host emulation / MI355X, all in units of 1e-16:

case                              mean                sd              mcse               ess              rhat
offset_1e6                 0.9/0.9/0.9      31.7/1.3/1.3 1.5e+09/1.2e+05/1.2e+05 2.9e+09/2.4e+05/2.4e+05 1.7e+08/7.8e+03/7.8e+03
w100_n8                1.4/  0.9/  0.9   0.6/  1.6/  1.6   5.2/  2.8/  3.2   9.4/  4.7/  8.8   1.1/  1.0/  1.0
w1_n300_trend          0.6/  1.0/  1.0   0.9/  2.0/  2.0   3.5/  4.0/  4.0   5.5/  5.5/  5.5   2.4/  1.2/  1.3
w1_n300_trend_lag20    0.6/  1.0/  1.0   0.9/  2.0/  2.0   0.9/  2.9/  2.9   4.6/  3.4/  3.4   2.4/  1.2/  1.3
w1_n4                  1.2/  1.1/  1.1   1.1/  1.1/  1.1   0.3/  0.3/  0.3  13.4/ 11.0/ 11.0   2.9/  0.7/  0.7
w2_n200_arneg          1.0/  1.0/  1.0   1.5/  1.5/  1.5   8.2/  8.5/  8.2  15.1/ 16.6/ 15.1   0.5/  0.5/  0.8
w2_n5                  1.9/  1.6/  1.6   1.2/  0.9/  0.9   6.7/  4.7/  4.7  25.1/ 68.9/ 68.9   0.9/  0.9/  0.9
w300_n6                1.0/  1.0/  1.0   1.5/  1.1/  1.1   5.7/ 11.1/ 11.1   9.4/ 21.5/ 21.5   0.1/  1.1/  1.1
w3_n400_ar95           1.1/  1.1/  1.1   0.8/  0.8/  0.8  14.9/ 16.0/ 16.0  30.7/ 32.1/ 32.1   0.5/  0.5/  0.5
w4_n200_means          1.9/  0.8/  0.8   1.0/  2.2/  2.2  10.6/ 10.6/  8.7  20.1/ 20.1/ 20.1   0.9/  1.4/  1.4
w4_n4096               4.3/  0.8/  0.8   0.8/  1.3/  1.3   2.2/  3.4/  2.2   4.0/  4.0/  2.2   0.3/  0.3/  0.3
w4_n64_iid             4.3/  1.0/  1.0   1.0/  1.5/  1.5   7.2/  4.2/  4.2  12.1/  5.8/  4.3   0.9/  0.9/  0.9
(offset_1e6: both restatements centre 1e6 + 1e-3 noise about chain means that carry the rounding of 1e6-sized sums -- 1e-10 in
 float64, 1e-13 in longdouble, against noise of 1e-3 -- while the library works on the column shifted by its pooled mean: that
 row's figures measure the restatements, the longdouble one included.  So `check_offset_binds` restates such columns on x - 1e6,
 exact in float64 and the same function of the column for all but the mean, under the same rule; there: sd 1.3/1.3/1.3,
 mcse 4.5/4.5/5.8, ess 5.4/5.4/7.8, rhat 1.1/1.1/1.1, and for the offset column of `special_columns` 0.1/0.1/0.1, 0.3/1.2/1.2,
 0.3/2.6/2.6, 0.7/0.7/0.7 against 8.9 allowed)
(the largest share of its allowance any entry uses: 0.34)
"""
import ctypes as C
import functools

import numpy as np

import _ppc_cases as pc
from conftest import make_engine
from barbay_jl_amd import _capi

STATS = ("mean", "sd", "mcse", "ess", "rhat")
PROBS = (0.025, 0.25, 0.5, 0.75, 0.975)
ULP = float(np.finfo(np.float64).eps)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def ar1(g, W, N, D, phi, loc=0.0):
    x = np.empty((W, N, D))
    x[:, 0] = g.standard_normal((W, D)) / np.sqrt(1.0 - phi * phi)
    for n in range(1, N):
        x[:, n] = phi * x[:, n - 1] + g.standard_normal((W, D))
    return x + loc


def _trend(g, W, N, D):
    return 0.01 * np.arange(N)[None, :, None] + g.standard_normal((W, N, D))


def _shifted(g, W, N, D):
    return g.standard_normal((W, N, D)) + 0.7 * np.arange(W)[:, None, None]


# name -> (builder(generator) -> chain[W, N, D], seed, keyword arguments of the call)
CASES = {
    "w1_n4": (lambda g: g.standard_normal((1, 4, 6)) + 2.0, 1, {}),                  # no between-chain term, smallest halves
    "w2_n5": (lambda g: g.standard_normal((2, 5, 6)) + 2.0, 2, {}),                  # odd N: the split drops the middle draw
    "w4_n64_iid": (lambda g: g.standard_normal((4, 64, 6)), 3, {}),
    "w3_n400_ar95": (lambda g: ar1(g, 3, 400, 4, 0.95), 4, {}),                      # truncation beyond the first lag batch
    "w2_n200_arneg": (lambda g: ar1(g, 2, 200, 5, -0.5, 1.0), 5, {}),                # ESS above WN: the log10 cap
    "w1_n300_trend": (lambda g: _trend(g, 1, 300, 4), 6, {}),
    "w1_n300_trend_lag20": (lambda g: _trend(g, 1, 300, 4), 6, {"max_lag": 20}),     # the lag bound ends the sum
    "w4_n200_means": (lambda g: _shifted(g, 4, 200, 5), 7, {}),                      # R-hat well above 1
    "w4_n4096": (lambda g: ar1(g, 4, 4096, 3, 0.5), 8, {}),                          # K = 16 384, the largest column
    "w100_n8": (lambda g: g.standard_normal((100, 8, 3)) - 1.0, 9, {}),              # several chains per wave: 2 / 4 lanes a segment
    "w300_n6": (lambda g: g.standard_normal((300, 6, 3)) + 1.0, 10, {}),             # a lane takes whole segments, 600 halves on 512 lanes
    "offset_1e6": (lambda g: 1e6 + 1e-3 * ar1(g, 2, 100, 4, 0.3), 11, {}),
}


@functools.lru_cache(maxsize=None)
def chain_of(name):
    build, seed, _ = CASES[name]
    x = np.ascontiguousarray(build(np.random.default_rng(seed)))
    x.setflags(write=False)
    return x


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def _var_plus(seg, dt):
    """Wbar and var+ of segments seg[S, L] (header: s2_c = a_c(0) L / (L - 1), the chain means' variance taken with S - 1)."""
    S, L = seg.shape
    m = seg.sum(axis=1) / dt(L)
    y = seg - m[:, None]
    s2 = (y * y).sum(axis=1) / dt(L) * dt(L) / dt(L - 1)
    wbar = s2.sum() / dt(S)
    b = ((m - m.sum() / dt(S)) ** 2).sum() / dt(S - 1) if S > 1 else dt(0)
    return wbar, dt(L - 1) / dt(L) * wbar + b, y


def restate(chain, probs=PROBS, max_lag=0, dtype=np.float64):
    """The header's per-column definitions.  Returns a dict: the five statistics [D] in `dtype`, n_lags [D], quantiles [D, n_q]."""
    dt = dtype
    x = np.asarray(chain, dtype=np.float64)
    if x.ndim == 2:
        x = x[None]
    W, N, D = x.shape
    K = W * N
    lim = N - 1 if max_lag == 0 else min(max_lag, N - 1)
    out = {k: np.full(D, np.nan, dtype=dt) for k in STATS}
    out["n_lags"] = np.zeros(D, dtype=np.int32)
    out["quantiles"] = np.empty((D, len(probs)))
    for j in range(D):
        raw = x[:, :, j]
        srt = np.sort(raw.reshape(-1))                      # NaN last, as the select orders it
        for i, p in enumerate(probs):
            out["quantiles"][j, i] = pc.quantile7(srt, float(p))
        if not np.isfinite(raw).all():
            continue
        if (raw == raw[0, 0]).all():
            out["mean"][j], out["sd"][j] = dt(raw[0, 0]), dt(0)
            continue
        col = raw.astype(dt)
        pooled = col.reshape(-1)
        mean = pooled.sum() / dt(K)
        sd = np.sqrt(((pooled - mean) ** 2).sum() / dt(K - 1))
        wbar, vp, y = _var_plus(col, dt)
        tot, prev, k = dt(0), dt(0), 0
        rho = lambda t: dt(1) - (wbar - ((y[:, :N - t] * y[:, t:]).sum(axis=1) / dt(N)).sum() / dt(W)) / vp
        while 2 * k + 1 <= lim:
            pk = rho(2 * k) + rho(2 * k + 1)
            if not pk > 0:
                break
            if k > 0:
                pk = min(pk, prev)
            tot, prev, k = tot + pk, pk, k + 1
        tau = dt(-1) + dt(2) * tot
        ess = min(dt(K) / tau, dt(K) * np.log10(dt(K)))
        h = N // 2
        halves = np.concatenate([col[:, :h], col[:, N - h:]], axis=0)
        wb2, vp2, _ = _var_plus(halves, dt)
        with np.errstate(invalid="ignore"):                 # tau < 0 (a few draws): ess < 0, mcse NaN
            out["mean"][j], out["sd"][j], out["ess"][j], out["mcse"][j] = mean, sd, ess, sd / np.sqrt(ess)
        out["rhat"][j] = np.sqrt(vp2 / wb2)
        out["n_lags"][j] = 2 * k
    return out


@functools.lru_cache(maxsize=None)
def references(name):
    """(float64 restatement, longdouble restatement, tolerance per statistic) of a case, computed once."""
    kw = CASES[name][2]
    r64 = restate(chain_of(name), dtype=np.float64, **kw)
    rld = restate(chain_of(name), dtype=np.longdouble, **kw)
    assert np.array_equal(r64["n_lags"], rld["n_lags"]), "the truncation is within rounding of 0: change the case's seed"
    tol = {k: max(8.0 * rel_err(r64[k], rld[k]), 4.0 * ULP) for k in STATS}
    return r64, rld, tol


def rel_err(a, ref):
    """Largest relative error over the columns, in longdouble; NaNs must coincide."""
    a, ref = np.asarray(a, dtype=np.longdouble), np.asarray(ref, dtype=np.longdouble)
    assert np.array_equal(np.isnan(a), np.isnan(ref)), (a, ref)
    ok = ~np.isnan(ref)
    if not ok.any():
        return 0.0
    d = np.abs(a[ok] - ref[ok])
    den = np.abs(ref[ok])
    return float(np.max(np.where(d == 0, 0, d / np.where(den == 0, 1, den))))


def check_case(engine, name, label="library"):
    """One case against the longdouble restatement; returns the library's result."""
    r64, rld, tol = references(name)
    got = engine.chain_summary(chain_of(name), PROBS, **CASES[name][2])
    for k in STATS:
        err = rel_err(got[k], rld[k])
        print(f"chain case {name:20s} {k:5s} float64 restatement {rel_err(r64[k], rld[k]) / 1e-16:8.2f}e-16  {label} {err / 1e-16:8.2f}e-16  "
              f"allowed {tol[k] / 1e-16:8.2f}e-16")
    for k in STATS:
        assert rel_err(got[k], rld[k]) <= tol[k], (name, k, rel_err(got[k], rld[k]), tol[k])
    assert np.array_equal(got["n_lags"], rld["n_lags"]), (name, got["n_lags"], rld["n_lags"])
    assert_quantiles_close(got["quantiles"], rld["quantiles"])
    if name == "offset_1e6":
        check_offset_binds(got, chain_of(name), label)
    return got


def assert_quantiles_close(a, b):
    """`_ppc_cases.assert_bands_close` (its tolerance) on the entries that are not infinite; infinities must be equal."""
    inf = np.isinf(b)
    assert np.array_equal(np.isinf(a), inf) and np.array_equal(a[inf], b[inf])
    pc.assert_bands_close(np.where(inf, 0.0, a), np.where(inf, 0.0, b))


def same_bits(a, b):
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)) for k in a)


def column(res, j):
    return {k: np.asarray(v[j]) for k, v in res.items()}


def column_slice(res, j):
    return {k: np.asarray(v[j:j + 1]) for k, v in res.items()}


def check_offset_binds(got, x, label="library"):
    """Columns 1e6 + 1e-3 noise, `got` the library's result on x: the case's own bound is loose for sd, mcse, ess and rhat, since
    both restatements centre about chain means that carry the rounding of 1e6-sized sums (1e-10 in float64, 1e-13 in longdouble,
    against noise of 1e-3).  x - 1e6 is exact in float64 (1e6 is a double and x lies within a factor 2 of it), and every statistic
    but the mean is the same function of x - 1e6 as of x: restated on the shifted columns both restatements are good to their own
    precision, and the same rule -- 8 x the float64 restatement's error, floored at 4 ulp -- binds."""
    sh = x - 1e6
    assert np.array_equal(sh.astype(np.longdouble) + np.longdouble(1e6), x.astype(np.longdouble))
    ld0, r0 = restate(sh, dtype=np.longdouble), restate(sh, dtype=np.float64)
    for k in STATS[1:]:
        ref, tol, err = rel_err(r0[k], ld0[k]), max(8.0 * rel_err(r0[k], ld0[k]), 4.0 * ULP), rel_err(got[k], ld0[k])
        print(f"chain 1e6 + 1e-3 noise restated on x - 1e6: {k:5s} float64 restatement {ref / 1e-16:8.2f}e-16  {label} {err / 1e-16:8.2f}e-16  "
              f"allowed {tol / 1e-16:8.2f}e-16")
        assert err <= tol, (k, err, tol)
    assert np.array_equal(got["n_lags"], ld0["n_lags"])


# ---- the C entry itself: null outputs, null arguments ----------------------------------------------------------------------------
def raw_summary(engine, chain, probs=(), max_lag=0, slab_cols=0, want=STATS + ("quantiles", "n_lags"), n_quantiles=None, n_cols=None,
                null=()):
    """bb_chain_summary through ctypes with only the outputs in `want` non-NULL; returns (status, dict of the wanted outputs).
    `null` names arguments passed as NULL (h, o, chain, out, probs); n_quantiles / n_cols override what the arrays say."""
    x = np.ascontiguousarray(chain, dtype=np.float64)
    W, N, D = x.shape
    p = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
    o = _capi.bb_chain_opts()
    o.n_chains, o.n_draws, o.max_lag, o.slab_cols = W, N, max_lag, slab_cols
    o.n_quantiles = len(p) if n_quantiles is None else n_quantiles
    o.probs = None if "probs" in null or not len(p) else _capi._ptr(p)
    res, out = {}, _capi.bb_chain_out()
    for k in want:
        if k == "quantiles":
            res[k] = np.full((D, len(p)), -7.0)
            out.quantiles = _capi._ptr(res[k])
        elif k == "n_lags":
            res[k] = np.full(D, -7, dtype=np.int32)
            out.n_lags = res[k].ctypes.data_as(C.POINTER(C.c_int32))
        else:
            res[k] = np.full(D, -7.0)
            setattr(out, k, _capi._ptr(res[k]))
    rc = engine._lib.bb_chain_summary(None if "h" in null else engine._h, None if "o" in null else C.byref(o),
                                      D if n_cols is None else n_cols, None if "chain" in null else _capi._ptr(x),
                                      None if "out" in null else C.byref(out))
    return rc, res


# ---- checks the emulation and GPU tests share ------------------------------------------------------------------------------------
def special_columns():
    """Ordinary columns at the even positions; 1: 1e6 + 1e-3 noise, 3: constant, 5: one NaN, 7: one +Inf."""
    g = np.random.default_rng(21)
    x = ar1(g, 2, 100, 9, 0.4)
    x[:, :, 1] = 1e6 + 1e-3 * x[:, :, 1]
    x[:, :, 3] = 0.1
    x[1, 17, 5] = np.nan
    x[0, 63, 7] = np.inf
    return x


def check_special_columns(e):
    x = special_columns()
    got = e.chain_summary(x, PROBS)
    plain = e.chain_summary(np.ascontiguousarray(x[:, :, 0::2]), PROBS)
    for i, j in enumerate(range(0, 9, 2)):                               # the neighbours are unaffected, bitwise
        assert same_bits(column(got, j), column(plain, i)), j
    ld = restate(x, dtype=np.longdouble)
    r64 = restate(x, dtype=np.float64)
    for k in STATS:                                                   # 1e6 + 1e-3 noise keeps its digits
        tol = max(8.0 * rel_err(r64[k][1:2], ld[k][1:2]), 4.0 * ULP)
        assert rel_err(got[k][1:2], ld[k][1:2]) <= tol, (k, rel_err(got[k][1:2], ld[k][1:2]), tol)
    assert got["n_lags"][1] == ld["n_lags"][1]
    check_offset_binds(column_slice(got, 1), x[:, :, 1:2])
    assert got["mean"][3] == 0.1 and got["sd"][3] == 0.0 and got["n_lags"][3] == 0
    assert all(np.isnan(got[k][3]) for k in ("mcse", "ess", "rhat"))
    assert np.all(got["quantiles"][3] == 0.1)
    for j in (5, 7):
        assert all(np.isnan(got[k][j]) for k in STATS) and got["n_lags"][j] == 0
    assert_quantiles_close(got["quantiles"], ld["quantiles"])
    tail = e.chain_summary(x, (0.5, 0.999, 1.0))["quantiles"]                        # the last order statistics: the NaN, the +Inf
    assert_quantiles_close(tail, restate(x, probs=(0.5, 0.999, 1.0))["quantiles"])
    assert np.isfinite(tail[:, 0]).all() and np.isnan(tail[5, 1:]).all() and np.all(tail[7, 1:] == np.inf)


def check_placement(e):
    """A column's results do not depend on n_cols, its position, the slab size or its neighbours."""
    g = np.random.default_rng(31)
    W, N = 2, 50
    v = ar1(g, W, N, 1, 0.6)[:, :, 0]
    alone = column(e.chain_summary(v[:, :, None], PROBS), 0)
    for D in (1, 17, 130):
        base = g.standard_normal((W, N, D))
        whole = None
        for pos in sorted({0, D - 1, min(15, D - 1), min(16, D - 1), min(49, D - 1), min(50, D - 1)}):
            x = base.copy()
            x[:, :, pos] = v
            for slab in ((0, 1, 16, 50) if D == 130 else (0, 16)):
                got = e.chain_summary(x, PROBS, slab_cols=slab)
                assert same_bits(column(got, pos), alone), (D, pos, slab)
                if pos == 0:
                    whole = whole or got
                    assert same_bits(got, whole), (D, slab)


def check_null_outputs(e):
    x = chain_of("w4_n64_iid")
    full = e.chain_summary(x, (0.0, 1.0, 0.5))
    srt = np.sort(x.reshape(-1, x.shape[2]), axis=0)
    assert np.array_equal(full["quantiles"][:, 0], srt[0]) and np.array_equal(full["quantiles"][:, 1], srt[-1])
    assert np.array_equal(full["quantiles"][:, 2], srt[127] + 0.5 * (srt[128] - srt[127]))
    rc, res = raw_summary(e, x, probs=(), want=STATS + ("n_lags",))           # n_quantiles = 0, quantiles = NULL
    assert rc == 0 and all(np.array_equal(res[k], full[k]) for k in res)
    for k in STATS + ("quantiles", "n_lags"):                                     # every output NULL except one
        rc, res = raw_summary(e, x, probs=(0.0, 1.0, 0.5), want=(k,))
        assert rc == 0 and np.array_equal(res[k], full[k]), k
    rc, _ = raw_summary(e, x, probs=(0.5,), want=())
    assert rc == 0


def check_errors(e):
    x = np.zeros((2, 8, 3)) + np.arange(8)[None, :, None]
    inv, uns = -1, _capi.BB_ERR_UNSUPPORTED
    for null in ("h", "o", "chain", "out"):
        assert raw_summary(e, x, null=(null,))[0] == inv, null
    assert raw_summary(e, x, n_cols=0)[0] == inv and raw_summary(e, x, n_cols=-3)[0] == inv
    assert raw_summary(e, np.zeros((2, 3, 3)))[0] == inv                         # N < 4
    assert raw_summary(e, np.zeros((0, 8, 3)), n_cols=3)[0] == inv               # W < 1
    for p in ((1.5,), (-0.1,), (float("nan"),), (0.5, 2.0)):
        assert raw_summary(e, x, probs=p)[0] == inv, p
    assert raw_summary(e, x, probs=(0.5,) * 9)[0] == inv
    assert raw_summary(e, x, n_quantiles=-1)[0] == inv
    assert raw_summary(e, x, probs=(0.5,), null=("probs",))[0] == inv
    assert raw_summary(e, x, max_lag=-1)[0] == inv and raw_summary(e, x, slab_cols=-1)[0] == inv
    big = np.random.default_rng(0).standard_normal((1, 16385, 1))
    assert raw_summary(e, big)[0] == uns                                          # W N = 16 385
    assert raw_summary(e, big[:, :16384])[0] == 0                                 # 16 384 is accepted
    assert raw_summary(e, x, probs=(0.0, 1.0, 0.5) * 2 + (0.1, 0.9))[0] == 0      # 8 quantiles
    for bad in (np.zeros((2, 3, 3)), np.zeros(7)):
        try:
            e.chain_summary(bad)
        except _capi.BarBayHipError:
            continue
        raise AssertionError("no error")


def check_handle_untouched(lib):
    sp = pc.spec("fitness")
    with make_engine(sp, lib, seed=5) as a, make_engine(sp, lib, seed=5) as b:
        b.chain_summary(chain_of("w4_n64_iid"))
        for x, y in zip(a.get_params(), b.get_params()):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
        a.run(5)
        b.chain_summary(chain_of("w2_n5"), slab_cols=2)
        b.run(5)
        for x, y in zip(a.get_params(), b.get_params()):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
