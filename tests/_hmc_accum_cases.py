"""Cases of the HMC session's streaming moments and metric, bb_hmc_accum_* / bb_hmc_set_metric / bb_hmc_get_metric
(barbay.jl_amd/csrc/bb_hmc_accum.h), shared by the emulation tests (CPU) and the GPU tests: each takes the loaded C-ABI library.  Shapes,
points and step sizes are those of `_logp_cases` / `_hmc_cases`.

The reference is always the chain itself, collected by `hmc_get` after each `hmc_step` (both pinned by `_hmc_cases`), never an
accumulator output: the rows against a numpy Welford restatement with the operations rounded one by one, the statistics against a
two-pass np.longdouble evaluation of the formulas of include/barbay_hip.h on that chain."""
import ctypes

import numpy as np
import pytest

import _hmc_cases as hc
import _logp_cases as lc
import barbay_jl_amd as bb
from barbay_jl_amd import _capi
from conftest import make_engine

NAMES = lc.NAMES
same = lc.same
SEED = hc.SEED
W3 = 3
LD = np.longdouble
QUANT = ("mean", "sd", "within", "between", "rhat")

# The three kinds of shape the kernels can go wrong at, all among the six (checked by check_kinds with a handle of each):
ODD_D = ("genotype",)                       # the pad entry (D = 6459)
REGROUPED = ("genotype",)                   # a non-empty permutation
SEVERAL_CHUNKS = ("fitness_multi_tile",)    # D > BB_HMC_CHUNK

# e_ref per shape as measured (the largest relative deviation over the latents between the fp64 numpy evaluation of the header's formulas
# and the np.longdouble one, on the 6-draw chain of case_statistics; mean, sd, within, between, rhat).  The bound of case_statistics is
# 8 * e_ref, measured afresh in the test (these are a record, not an input; the same figures in the emulation and on the MI355X where the
# chains agree: the evaluations run on the host):
E_REF_MEASURED = {          # (in brackets: `within` and `rhat` of a TWO-PASS fp64 evaluation, which the one-pass update cannot reach: see bounds)
    "fitness_T2":         (8.47e-15, 2.42e-16, 7.20e-14, 4.31e-16, 3.60e-14),     # (3.24e-16, 6.03e-16)
    "fitness_multi_tile": (2.70e-13, 7.39e-16, 9.48e-13, 1.75e-15, 4.74e-13),     # (3.86e-16, 3.19e-15)
    "multienv":           (4.87e-13, 1.36e-15, 1.26e-12, 2.45e-15, 6.31e-13),     # (4.71e-16, 1.68e-15)
    "replicate_ragged":   (1.19e-12, 1.15e-15, 1.37e-11, 2.26e-15, 6.87e-12),     # (3.90e-16, 1.37e-15)
    "multienv_replicate": (4.77e-12, 2.72e-15, 1.33e-11, 5.21e-15, 6.65e-12),     # (4.19e-16, 6.38e-15)
    "genotype":           (5.15e-13, 2.96e-15, 1.84e-11, 5.78e-15, 9.18e-12),     # (3.96e-16, 9.55e-15)
}                           # (the device's own deviation equals e_ref in all 30 figures: its rows are the restatement's, bit for bit)


def check_kinds(lib):
    odd = regrouped = chunks = 0
    for name in NAMES:
        sp, _, _ = lc.spec(name)
        with make_engine(sp, lib, seed=SEED) as e:
            perm = e.permutation()
        odd += sp.D % 2 == 1
        regrouped += not np.array_equal(perm, np.arange(sp.D))
        chunks += sp.D > _capi.BB_HMC_CHUNK
        assert (name in ODD_D) <= (sp.D % 2 == 1) and (name in SEVERAL_CHUNKS) <= (sp.D > _capi.BB_HMC_CHUNK)
        assert (name in REGROUPED) <= (not np.array_equal(perm, np.arange(sp.D)))
    assert odd and regrouped and chunks, (odd, regrouped, chunks)


def log_us(n, W=W3, seed=41):
    """log(u) of n transitions: -inf on the first two (every walker moves: no latent is constant), then random."""
    lu = np.log(np.random.default_rng(seed).random((n, W)))
    lu[:2] = -np.inf
    return lu


def run(e, name, n, segments, S=2, Z=None, lu=None, between=None, minv=None):
    """A session at Z (default: the shape's three points), accumulators of S segments, n transitions; after transition t the walkers are
    added to segments[t] ([W], or None: no add).  Returns the chain [n, W, D] as hmc_get gave it and the step outputs; the session and its
    accumulators stay open (the caller ends it)."""
    sp, Z3, _ = lc.spec(name)
    Z = Z3 if Z is None else Z
    W = Z.shape[0]
    eps = np.resize(hc.EPS3, W) * hc.EPS_SCALE[name]
    lu = log_us(n, W) if lu is None else lu
    e.hmc_begin(Z, seed=SEED, inv_mass=hc.inv_mass(sp.D) if minv is None else minv)
    e.hmc_accum_begin(S)
    chain, outs = [], []
    for t in range(n):
        outs.append(e.hmc_step(t + 1, eps, np.resize(hc.L3, W), lu[t]))
        chain.append(e.hmc_get(grad=True))
        if segments[t] is not None:
            e.hmc_accum_add(segments[t])
        if between is not None:
            between(t)
    return np.stack([c[0] for c in chain]), outs, chain


def welford(xs):
    """The device's update on the rows xs [n, D], every operation rounded on its own, 1 / n as the host forms it."""
    mean, m2 = np.zeros(xs.shape[1]), np.zeros(xs.shape[1])
    for n, x in enumerate(xs, start=1):
        inv_n = 1.0 / float(n)
        d = x - mean
        mean = mean + d * inv_n
        m2 = m2 + d * (x - mean)
    return mean, m2, len(xs)


def check_rows(e, chain, segments, S, walkers=None):
    """hmc_accum_get(w, s) of every (w, s) against the restatement on the rows of `chain` that went there."""
    n, W, D = chain.shape
    for w in (range(W) if walkers is None else walkers):
        for s in range(S):
            ts = [t for t in range(n) if segments[t] is not None and np.broadcast_to(segments[t], (W,))[w] == s]
            mean, m2, cnt = e.hmc_accum_get(w, s)
            rm, rq, rn = welford(chain[ts, w]) if ts else (np.zeros(D), np.zeros(D), 0)
            assert cnt == rn, (w, s, cnt, rn)
            assert same(mean, rm) and same(m2, rq), (w, s)


# segment vectors of the six transitions of case_accumulators: -1 and both segments of S = 2, every (w, s) gets at least one state
SEG6 = [np.array(v, dtype=np.int32) for v in ([0, 1, -1], [0, 0, 1], [1, -1, 0], [-1, 1, 0], [1, 0, 1], [0, 1, -1])]


def case_accumulators(lib, name):
    sp, _, _ = lc.spec(name)
    with make_engine(sp, lib, seed=SEED) as e:
        chain, outs, _ = run(e, name, 6, SEG6)
        assert all(o["accepted"].all() for o in outs[:2])
        assert (np.abs(chain[1] - chain[0]) > 0).all()                        # every latent of every walker moved
        check_rows(e, chain, SEG6, 2)
        e.hmc_end()


def formulas(chains, T, streamed=False):
    """The header's formulas in T on the live chains `chains` (a list of [n_c, D]): m_c and M2_c two-pass, or `streamed` by the header's
    update as `welford` restates it; then the four rows, sd and rhat.  Returns mean, sd, within, between, rhat."""
    xs = [c.astype(T) for c in chains]
    C, K = len(xs), sum(len(c) for c in xs)
    if streamed:
        ms, M2 = zip(*[welford(c)[:2] for c in xs])
    else:
        ms = [c.sum(axis=0) / T(len(c)) for c in xs]
        M2 = [((c - m) ** 2).sum(axis=0) for c, m in zip(xs, ms)]
    mean = sum(T(len(c)) * m for c, m in zip(xs, ms)) / T(K)
    pooled = sum(M2) + sum(T(len(c)) * (m - mean) ** 2 for c, m in zip(xs, ms))
    within = sum(q / T(len(c) - 1) for c, q in zip(xs, M2)) / T(C)
    mbar = sum(ms) / T(C)
    between = sum((m - mbar) ** 2 for m in ms) / T(C - 1) if C > 1 else np.zeros_like(mean)
    nbar = T(K) / T(C)
    sd = np.sqrt(pooled / T(K - 1))
    rhat = np.sqrt(((nbar - T(1)) / nbar * within + between) / within)
    return dict(mean=mean, sd=sd, within=within, between=between, rhat=rhat)


def bounds(live):
    """The longdouble two-pass reference of the live chains and, per quantity, 8 x e_ref.  e_ref is the deviation from that reference of
    the header's formulas evaluated in fp64 numpy -- the accumulators by the header's streaming update, which is what the header defines
    them by.  The update loses |mean| / sd digits of M2 more than a two-pass sum (its d (x - mean) carries the rounding of the running
    mean, which a two-pass sum cancels to first order), and the chains here move by ~1e-3 of |z| per transition: against a two-pass fp64
    evaluation (`two_pass`, printed by case_statistics and recorded in E_REF_MEASURED) `within` and `rhat` deviate by 1e2 .. 5e4 times
    that evaluation's own error (`within` 7e-14 .. 2e-11 against 3e-16 .. 5e-16), so 8 x the two-pass figure would fail for these two
    quantities on every shape, while mean, sd and between would hold.  That is the price of the prescribed one-pass arithmetic at
    |mean| / sd ~ 1e3 .. 1e5, not of the device: the device's rows equal the fp64 restatement's bit for bit."""
    ref = formulas(live, LD)
    e_ref = {k: rel_dev(formulas(live, np.float64, streamed=True)[k], ref[k]) for k in QUANT}
    two_pass = {k: rel_dev(formulas(live, np.float64)[k], ref[k]) for k in QUANT}
    return ref, e_ref, two_pass


def rel_dev(a, ref):
    """The largest relative deviation over the latents."""
    ref = np.asarray(ref, dtype=LD)
    return float(np.max(np.abs(np.asarray(a, dtype=LD) - ref) / np.abs(ref)))


def halves(n, W=W3):
    return [np.full(W, 0 if t < n // 2 else 1, dtype=np.int32) for t in range(n)]


def derived_ok(st):
    """mcse and ess as the stated functions of the returned rows (the host forms them with the same IEEE operations: a few ulp at most
    separate numpy's log10 and sqrt from libm's)."""
    K = st["n_total"]
    C = st["_C"]
    mcse = np.sqrt(st["between"] / C)
    ess = np.minimum(st["sd"] * st["sd"] / (mcse * mcse), K * np.log10(K))
    assert np.allclose(st["mcse"], mcse, rtol=4e-16, atol=0.0) and np.allclose(st["ess"], ess, rtol=8e-16, atol=0.0)


def case_statistics(lib, name):
    """S = 2, equal halves of 6 draws per walker: the five rows against the longdouble evaluation, bound 8 x the fp64 numpy evaluation's own
    deviation from it; then 8 draws per walker against Engine.chain_summary on the host chain within the same bound."""
    sp, _, _ = lc.spec(name)
    e_ref = {}
    with make_engine(sp, lib, seed=SEED) as e:
        for n in (6, 8):
            chain, _, _ = run(e, name, n, halves(n))
            st = e.hmc_accum_stats()
            e.hmc_end()
            assert st["n_total"] == n * W3
            live = [chain[:n // 2, w] for w in range(W3)] + [chain[n // 2:, w] for w in range(W3)]
            live = [live[i] for i in (0, 3, 1, 4, 2, 5)]                     # (w ascending, then s: the order plays no part in the formulas)
            ref, e_n, two_pass = bounds(live)
            bound = {k: 8.0 * e_n[k] for k in QUANT}
            if n == 6:
                e_ref = e_n
                print(name, "e_ref", {k: "%.3g" % v for k, v in e_ref.items()}, "two-pass fp64", {k: "%.3g" % v for k, v in two_pass.items()})
                for k in QUANT:
                    d = rel_dev(st[k], ref[k])
                    print(name, k, "dev", d, "bound", bound[k])
                    assert d <= bound[k], (k, d, bound[k])
                st["_C"] = 2 * W3
                derived_ok(st)
            else:
                cs = e.chain_summary(np.ascontiguousarray(chain.transpose(1, 0, 2)), ())
                for k in ("mean", "sd", "rhat"):
                    d = rel_dev(st[k], cs[k])
                    print(name, "chain_summary", k, "dev", d, "bound", bound[k])
                    assert d <= bound[k], (k, d, bound[k])
    return e_ref


def case_independence(lib, name):
    """Walker 1's rows from the W = 3 run of case_accumulators equal those of a run in which the other walkers go to other segments (of
    more segments) or are not added, those of a W = 2 session in which walker 0 is never added, and those of a two-kernel handle.  A
    walker's momenta come from the stream of its session index (BB_HMC_STREAM0 + w, `_hmc_cases.case_independence`), so the W = 1 session
    at the same start is compared for the walker it can hold, walker 0."""
    sp, Z, _ = lc.spec(name)
    lu = log_us(6)

    def rows_equal(e, w, ref):
        for s in range(2):
            got = e.hmc_accum_get(w, s)
            assert same(got[0], ref[s][0]) and same(got[1], ref[s][1]) and got[2] == ref[s][2], (w, s)

    with make_engine(sp, lib, seed=SEED) as e:
        chain, _, _ = run(e, name, 6, SEG6)
        base = [[e.hmc_accum_get(w, s) for s in range(2)] for w in range(2)]
        e.hmc_end()
        other = [np.array([(t + 1) % 3, SEG6[t][1], -1 if t % 2 else 2], dtype=np.int32) for t in range(6)]
        chain2, _, _ = run(e, name, 6, other, S=3)
        assert same(chain2, chain)
        rows_equal(e, 1, base[1])
        e.hmc_end()
        chain2, _, _ = run(e, name, 6, [np.array([-1, SEG6[t][1]], dtype=np.int32) for t in range(6)], Z=Z[:2], lu=lu[:, :2])
        assert same(chain2[:, 1], chain[:, 1])
        rows_equal(e, 1, base[1])
        assert e.hmc_accum_get(0, 0)[2] == 0 and not e.hmc_accum_get(0, 0)[0].any()
        e.hmc_end()
        chain1, _, _ = run(e, name, 6, [SEG6[t][:1] for t in range(6)], Z=Z[:1], lu=lu[:, :1])
        assert same(chain1[:, 0], chain[:, 0])
        rows_equal(e, 0, base[0])
        e.hmc_end()
    with make_engine(sp, lib, seed=SEED, launch_mode=1) as e:                 # two-kernel handle against the default mode
        run(e, name, 6, SEG6)
        rows_equal(e, 1, base[1])
        e.hmc_end()


def case_nothing_disturbed(lib, name):
    sp, Z, _ = lc.spec(name)

    def flat(outs, chain):
        return [o[k] for o in outs for k in hc.FIELDS] + [x for c in chain for x in c]

    with make_engine(sp, lib, seed=SEED) as e:
        mu0, om0 = e.get_params()

        def meddle(t):
            if t == 2:
                e.hmc_accum_get(2, 1)
            if t == 4:                                                        # (every (w, s) of SEG6 holds two states by now)
                e.hmc_accum_stats()
                e.hmc_accum_reset()

        _, outs, chain = run(e, name, 6, SEG6, between=meddle)
        e.hmc_end()
        with_acc = flat(outs, chain)
        mu1, om1 = e.get_params()
        assert same(mu0, mu1) and same(om0, om1)
        e.run(5)
        after = e.get_params() + e.opt_state()
    with make_engine(sp, lib, seed=SEED) as e:
        e.hmc_begin(Z, seed=SEED, inv_mass=hc.inv_mass(sp.D))
        eps, lu = hc.EPS3 * hc.EPS_SCALE[name], log_us(6)
        outs, chain = [], []
        for t in range(6):
            outs.append(e.hmc_step(t + 1, eps, hc.L3, lu[t]))
            chain.append(e.hmc_get(grad=True))
        e.hmc_end()
        assert all(same(a, b) for a, b in zip(with_acc, flat(outs, chain)))
        e.run(5)
        plain = e.get_params() + e.opt_state()
    assert all(same(a, b) if a.dtype == np.float64 else np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(after, plain))


def case_metric(lib, name):
    sp, Z, _ = lc.spec(name)
    D = sp.D
    eps, lu = hc.EPS3 * hc.EPS_SCALE[name], log_us(3)
    v = np.random.default_rng(13).uniform(0.2, 5.0, D)
    with make_engine(sp, lib, seed=SEED) as e:
        e.hmc_begin(Z, seed=SEED, inv_mass=hc.inv_mass(D))
        assert same(e.hmc_get_metric(), hc.inv_mass(D))
        e.hmc_set_metric(None)
        assert same(e.hmc_get_metric(), np.ones(D))
        e.hmc_set_metric(hc.inv_mass(D))
        e.hmc_accum_begin(1)
        for t in range(2):
            e.hmc_step(t + 1, eps, hc.L3, lu[t])
            e.hmc_accum_add(0)
        mid = e.hmc_get(grad=True)
        rows = e.hmc_accum_get(1, 0)
        e.hmc_set_metric(v)
        assert same(e.hmc_get_metric(), v)
        assert all(same(a, b) for a, b in zip(mid, e.hmc_get(grad=True)))     # z, logp, g untouched
        got = e.hmc_accum_get(1, 0)
        assert same(got[0], rows[0]) and same(got[1], rows[1]) and got[2] == rows[2] == 2
        a = (e.hmc_step(3, eps, hc.L3, lu[2]), e.hmc_get(grad=True))
        e.hmc_end()
        with e.hmc_begin(mid[0], seed=SEED, inv_mass=v):
            b = (e.hmc_step(3, eps, hc.L3, lu[2]), e.hmc_get(grad=True))
        for w in range(W3):
            assert hc.same_walker(a, w, b, w), w


def case_full_width(lib, name="fitness_T2"):
    """W = BB_HMC_MAX_WALKERS, S = BB_HMC_MAX_SEGMENTS, two adds per (w, s): 16 transitions, walker w going to segment (t // 2 + w) % 8."""
    sp, _, _ = lc.spec(name)
    W, S = _capi.BB_HMC_MAX_WALKERS, _capi.BB_HMC_MAX_SEGMENTS
    Z = np.random.default_rng(33).normal(0.0, 0.4, (W, sp.D))
    n = 2 * S
    segs = [((t // 2 + np.arange(W)) % S).astype(np.int32) for t in range(n)]
    with make_engine(sp, lib, seed=SEED) as e:
        chain, _, _ = run(e, name, n, segs, S=S, Z=Z, lu=log_us(n, W))
        check_rows(e, chain, segs, S, walkers=(0, W - 1))
        st = e.hmc_accum_stats()
        e.hmc_end()
    assert st["n_total"] == n * W
    assert all(np.isfinite(st[k]).all() for k in _capi.HMC_ACCUM_FIELDS)


def case_errors(lib):
    sp, Z, _ = lc.spec("fitness_T2")
    D = sp.D
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    P = lambda a, t=dp: a.ctypes.data_as(t)
    err = lambda: lib.bb_last_error().decode()
    buf, n64 = np.zeros(D), ctypes.c_int64(0)

    def aopts(S=2, reserved=0):
        o = _capi.bb_hmc_accum_opts()
        o.n_segments, o.reserved0 = S, reserved
        return o

    seg = lambda *v: P(np.array(v, dtype=np.int32), ip)
    out = _capi.bb_hmc_accum_out()
    with make_engine(sp, lib, seed=SEED) as e:
        h = e._h
        calls = {"begin": lambda: lib.bb_hmc_accum_begin(h, ctypes.byref(aopts())), "add": lambda: lib.bb_hmc_accum_add(h, seg(0, 0, 0)),
                 "reset": lambda: lib.bb_hmc_accum_reset(h), "get": lambda: lib.bb_hmc_accum_get(h, 0, 0, P(buf), None, None),
                 "stats": lambda: lib.bb_hmc_accum_stats(h, ctypes.byref(out)), "set_metric": lambda: lib.bb_hmc_set_metric(h, None),
                 "get_metric": lambda: lib.bb_hmc_get_metric(h, P(buf))}
        for k, f in calls.items():                                            # no session
            assert f() == -1 and "session" in err(), k
        e.hmc_begin(Z, seed=SEED)
        for k in ("add", "reset", "get", "stats"):                            # no accumulators
            assert calls[k]() == -1 and "accumulators" in err(), k
        # null arguments
        assert lib.bb_hmc_accum_begin(None, ctypes.byref(aopts())) == -1 and lib.bb_hmc_accum_begin(h, None) == -1
        assert lib.bb_hmc_accum_add(None, seg(0, 0, 0)) == -1 and lib.bb_hmc_accum_reset(None) == -1
        assert lib.bb_hmc_accum_get(None, 0, 0, None, None, None) == -1 and lib.bb_hmc_accum_stats(None, ctypes.byref(out)) == -1
        assert lib.bb_hmc_set_metric(None, None) == -1 and lib.bb_hmc_get_metric(None, P(buf)) == -1 and lib.bb_hmc_get_metric(h, None) == -1
        # begin
        for S in (0, 9, -1):
            assert lib.bb_hmc_accum_begin(h, ctypes.byref(aopts(S))) == -1 and "n_segments" in err(), S
        assert lib.bb_hmc_accum_begin(h, ctypes.byref(aopts(2, reserved=1))) == -1 and "reserved0" in err()
        assert calls["add"]() == -1                                           # a refused begin leaves no accumulators
        assert calls["begin"]() == 0 and calls["begin"]() == 0                # a second call replaces
        assert lib.bb_hmc_accum_add(h, None) == -1 and lib.bb_hmc_accum_stats(h, None) == -1
        for bad in (2, -2):
            assert lib.bb_hmc_accum_add(h, seg(0, bad, 0)) == -1 and "walker 1" in err(), bad
        for w, s in ((3, 0), (-1, 0)):
            assert lib.bb_hmc_accum_get(h, w, s, None, None, None) == -1 and "walker" in err()
        for w, s in ((0, 2), (0, -1)):
            assert lib.bb_hmc_accum_get(h, w, s, None, None, None) == -1 and "segment" in err()
        assert lib.bb_hmc_accum_get(h, 2, 1, None, None, ctypes.byref(n64)) == 0 and n64.value == 0      # every output may be NULL
        assert calls["stats"]() == -1                                         # nothing added
        for bad in (0.0, -1.0, np.inf, np.nan):
            im = np.ones(D)
            im[7] = bad
            assert lib.bb_hmc_set_metric(h, P(im)) == -1 and "inv_mass[7]" in err(), bad
        assert same(e.hmc_get_metric(), np.ones(D))                           # a refused metric changes nothing
        # a chain with one state; C = 1; probes only
        e.hmc_accum_add([0, -1, -1])
        assert calls["stats"]() == -1 and "walker 0" in err() and "segment 0" in err()
        e.hmc_step(1, hc.EPS3, hc.L3, -np.inf)
        e.hmc_accum_add([0, -1, -1])
        st = e.hmc_accum_stats()                                              # C = 1: a sd, no rhat, mcse, ess
        assert st["n_total"] == 2 and np.isfinite(st["mean"]).all() and (st["sd"] > 0).all() and (st["between"] == 0).all()
        assert all(np.isnan(st[k]).all() for k in ("rhat", "mcse", "ess"))
        assert lib.bb_hmc_accum_stats(h, ctypes.byref(_capi.bb_hmc_accum_out())) == 0                     # every output may be NULL
        e.hmc_accum_reset()
        assert e.hmc_accum_get(0, 0)[2] == 0 and not e.hmc_accum_get(0, 0)[0].any() and not e.hmc_accum_get(0, 0)[1].any()
        # a walker set that never moved (only probes), every walker at the same point: constant columns
        e.hmc_begin(np.repeat(Z[:1], 3, axis=0), seed=SEED)
        assert calls["add"]() == -1 and "accumulators" in err()               # bb_hmc_begin dropped them
        e.hmc_accum_begin(2)
        for t in range(4):
            e.hmc_step(t + 1, hc.EPS3, 1, np.inf)
            e.hmc_accum_add(t // 2)
        st = e.hmc_accum_stats()
        assert same(st["mean"], Z[0]) and not st["sd"].any() and all(np.isnan(st[k]).all() for k in ("rhat", "mcse", "ess"))
        # a non-finite accumulator: NaN for that latent, no other disturbed
        zz = np.array(Z)
        zz[1, 5] = 1e308
        e.hmc_begin(zz, seed=SEED)
        e.hmc_accum_begin(1)
        e.hmc_accum_add(0)
        e.hmc_step(1, hc.EPS3, 1, np.inf)
        e.hmc_accum_add(0)
        bad = e.hmc_accum_stats()
        e.hmc_begin(Z, seed=SEED)
        e.hmc_accum_begin(1)
        e.hmc_accum_add(0)
        e.hmc_step(1, hc.EPS3, 1, np.inf)
        e.hmc_accum_add(0)
        good = e.hmc_accum_stats()
        keep = np.arange(D) != 5
        for k in ("mean", "sd", "mcse", "ess", "rhat"):
            assert np.isnan(bad[k][5]) and same(bad[k][keep], good[k][keep]), k
        # an add after bb_hmc_end
        e.hmc_end()
        assert calls["add"]() == -1 and "session" in err()
    with make_engine(sp, lib, seed=SEED, world_size=2, rank=0) as e:          # BB_ERR_UNSUPPORTED, as for bb_hmc_*
        h = e._h
        assert lib.bb_hmc_accum_begin(h, ctypes.byref(aopts())) == -4 and "sharded" in err()
        assert lib.bb_hmc_accum_add(h, seg(0, 0, 0)) == -4 and lib.bb_hmc_accum_reset(h) == -4 and lib.bb_hmc_set_metric(h, None) == -4
        assert lib.bb_hmc_accum_stats(h, ctypes.byref(out)) == -4 and lib.bb_hmc_get_metric(h, P(buf)) == -4
        assert lib.bb_hmc_accum_get(h, 0, 0, None, None, None) == -4


# ---- end to end: mcmc_sample(sampler="hmc") with the adapted metric and the streamed summary ----------------------------------------
E2E_KW = dict(n_walkers=4, n_adapt=60, n_steps=40, advi_steps=200, outputname=None, verbose=False, seed=3)


def case_end_to_end(lib):
    df = lc.load("data001_single")
    kw = dict(data=df, model=bb.model.fitness_normal, engine_kwargs={"_lib": lib}, sampler="hmc", **E2E_KW)
    out = bb.mcmc.mcmc_sample(hmc_kwargs=dict(adapt_metric=True, segments=2), **kw)
    D = out["chain"].shape[2]
    assert out["chain"].shape == (4, 40, D)
    for k in ("stream_mean", "stream_sd", "stream_mcse", "stream_ess", "stream_rhat", "inv_mass"):
        assert out[k].shape == (D,), k
    assert out["stream_n"] == 160
    assert np.isfinite(out["inv_mass"]).all() and (out["inv_mass"] > 0).all()
    live = [out["chain"][w, lo:lo + 20] for w in range(4) for lo in (0, 20)]
    ref, e_ref, _ = bounds(live)
    for k in ("mean", "sd"):
        d, bound = rel_dev(out["stream_" + k], ref[k]), 8.0 * e_ref[k]
        print("end to end", k, "dev", d, "bound", bound)
        assert d <= bound, (k, d, bound)
    tab = bb.mcmc.summarize({k: v for k, v in out.items() if k != "chain"})
    assert list(tab.columns) == ["parameters", "mean", "std", "mcse", "ess", "rhat"] and len(tab) == D
    assert same(tab["mean"].to_numpy(), out["stream_mean"]) and same(tab["std"].to_numpy(), out["stream_sd"])
    # without the chain: the same stream, no download
    lean = bb.mcmc.mcmc_sample(hmc_kwargs=dict(adapt_metric=True, segments=2, keep_chain=False), **kw)
    assert lean["chain"].shape == (4, 0, D) and same(lean["stream_mean"], out["stream_mean"]) and same(lean["stream_sd"], out["stream_sd"])
    with pytest.raises(bb.BarBayError, match="keep_chain"):
        bb.mcmc.mcmc_sample(hmc_kwargs=dict(segments=2, keep_chain=False), summary=True, **kw)
    with pytest.raises(bb.BarBayError, match="BB_HMC_MAX_WALKERS"):
        bb.mcmc.mcmc_sample(hmc_kwargs=dict(segments=2), **{**kw, "n_walkers": _capi.BB_HMC_MAX_WALKERS + 1})
