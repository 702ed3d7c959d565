"""The iterate trace (bb_trace_*, barbay.jl_amd/csrc/bb_trace.h; the contract: include/barbay_hip.h) and the stopping rule on top of it
(barbay.jl_amd/vi.py, Convergence): the cases the emulation tests (CPU, `-m "not gpu"`) and the GPU tests (`-m gpu`) share.  Each case takes
the loaded C-ABI library.  Nothing here restates a statistic: bb_trace_summary is held, byte for byte, to bb_chain_summary on the arrays
bb_trace_get returns (tests/_chain_cases.py holds that one to the header's formulas), the snapshots to an untraced twin's parameters, and the
verdict to a numpy recount of the same call's per-column outputs."""
import functools
import math
import os

import numpy as np
import pandas as pd
import pytest

import _ppc_cases as pc
import _run_cases as rc
from conftest import make_engine
from oracle import fixtures

SEED = 11
GOLD = os.path.join(os.path.dirname(__file__), "golden")
COLS = ("mean", "sd", "mcse", "ess", "rhat", "n_lags")

# the shapes: three of _ppc_cases.CASES and a genotype shape with n_geno + n_bc odd and T even, whose loglambda the handle lays out first
SHAPES = ("fitness", "genotype_regrouped", "genotype_odd", "replicate_ragged")
# the launch paths these shapes reach: launch_mode 0 (the library's choice: a resident launch where one fits) and 1 (the two-kernel step);
# "ms": S = 2 samples per step and ELBO recording every 3 steps (the MS instances); "lean": neither (the lean instances)
MODES = (0, 1)
SETTINGS = {"ms": dict(samples_per_step=2, elbo_every=3), "lean": dict(samples_per_step=1, elbo_every=0)}
PLAN = (1, 6, 5, 11, 9)          # 32 steps; every = 3: 10 snapshots, a ring of 8 wraps; calls start off and on the boundaries


@functools.lru_cache(maxsize=None)
def spec(name):
    if name == "genotype_odd":
        return fixtures.synthetic("genotype", seed=3, B=70, T=6, n_geno=7, n_neutral=10)
    return pc.spec(name)


def engine(lib, shape, mode, setting="ms", **kw):
    return make_engine(spec(shape), lib, **{**dict(seed=SEED, window=5, launch_mode=mode), **SETTINGS[setting], **kw})


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def same(a, b):
    return all(bits(x) == bits(y) for x, y in zip(a, b))


def cut(t, n, every):
    """The pieces of a run of n steps that starts at trace step t."""
    out = []
    while n > 0:
        p = min(n, every - t % every)
        out.append(p)
        t += p
        n -= p
    return out


def check_order(e, shape):
    """The shapes are what they are for: the handle's order differs from the caller's; genotype_odd has loglambda first."""
    perm = e.permutation()
    if shape == "genotype_regrouped":
        assert not np.array_equal(perm, np.arange(e.D))
    if shape == "genotype_odd":
        sp = spec(shape)
        lo, hi = next((lo, hi) for nm, lo, hi in e.layout() if nm == "loglambda")
        assert (sp.n_geno + sp.n_bc) % 2 == 1 and lo <= perm[2 * (sp.n_time[0] - 1)] < hi, perm[:16]


# ---------------------------------------------------------------------------------------------------------------------------
# 1. snapshots are the parameters
# ---------------------------------------------------------------------------------------------------------------------------
def case_snapshots(lib, shape, mode, setting):
    """every = 3, capacity = 8, the plan [1, 6, 5, 11, 9]: an untraced twin is stepped with run() calls cut at the boundaries, get_params
    in between.  The live snapshots, the final parameters, steps_done and the ELBO trace are equal bit for bit; trace_count is right after
    every call; dead snapshots are refused with the live range in the message."""
    import barbay_jl_amd as bb
    every, cap = 3, 8
    with engine(lib, shape, mode, setting) as e, engine(lib, shape, mode, setting) as t:
        check_order(e, shape)
        assert same(e.get_params(), t.get_params())
        e.trace_begin(every, cap)
        assert e.trace_count() == (0, 0)
        want, tt = [], 0
        for n in PLAN:
            e.run(n)
            for p in cut(tt, n, every):
                t.run(p)
                tt += p
                if tt % every == 0:
                    want.append(t.get_params())
            taken, live = e.trace_count()
            assert (taken, live) == (len(want), max(0, len(want) - cap)), (n, taken, live)
            assert e.stats()["steps_done"] == t.stats()["steps_done"] == tt
            mu, om = e.trace_get(live, taken - live)
            for k in range(live, taken):
                assert same((mu[k - live], om[k - live]), want[k]), (shape, mode, setting, n, k)
        assert (taken, live) == (10, 2) and tt == 32
        assert same(e.get_params(), t.get_params())
        if SETTINGS[setting]["elbo_every"]:
            tr = e.elbo_trace(0, math.ceil(tt / 3))
            assert np.isfinite(tr).all() and bits(tr) == bits(t.elbo_trace(0, math.ceil(tt / 3)))
        one = e.trace_get(5, 1)          # a single live snapshot, past the wrap (slot 5 holds it, slots 0 and 1 hold 8 and 9)
        assert same((one[0][0], one[1][0]), want[5])
        for first, n in ((0, 1), (1, 3), (9, 2), (10, 1)):
            with pytest.raises(bb.BarBayHipError, match=r"error -1: .*the ring holds 2 \.\. 9 "):
                e.trace_get(first, n)
        print(f"snapshots {shape} mode {mode} {setting}: {e.kernel_name()}: 10 snapshots, 8 live, bit-equal to the twin's parameters")
        e.trace_end()
        e.run(2)          # untraced again
        t.run(2)
        assert same(e.get_params(), t.get_params())


# ---------------------------------------------------------------------------------------------------------------------------
# 2. / 3. the summary equals bb_chain_summary; the verdict is what the per-column outputs imply
# ---------------------------------------------------------------------------------------------------------------------------
def softplus(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def recount(e, s, rhat_max):
    """The verdict frame recomputed from the per-column outputs `s` of the same call.  Counts, max_rhat and min_ess exactly;
    max_mcse_rel to 1e-12 relative: a softplus, a sigmoid and two divisions, each good to a few ulp (tests/_math_cases.py)."""
    D, lay, bl = e.D, e.layout(), s["blocks"]
    nb = len(lay)
    assert len(bl) == 2 * nb
    with np.errstate(all="ignore"):
        for v in range(2 * nb):
            row = bl.iloc[v]
            name, lo, hi = lay[v % nb]
            part = v // nb
            idx = part * D + np.arange(lo, hi)
            assert (row["name"], row["part"], row["n_cols"]) == (name, "omega" if part else "mu", hi - lo), (v, row)
            assert row["n_nonfinite"] == np.isnan(s["mean"][idx]).sum(), (v, row)
            assert row["n_const"] == (s["sd"][idx] == 0).sum(), (v, row)
            rh, es = s["rhat"][idx], s["ess"][idx]
            assert row["n_above"] == (rh[np.isfinite(rh)] > rhat_max).sum(), (v, row)
            om = s["mean"][D + np.arange(lo, hi)]
            rel = s["mcse"][idx] * (sigmoid(om) if part else 1.0) / softplus(om)
            for got, x, red, tol in ((row["max_rhat"], rh, np.max, 0.0), (row["min_ess"], es, np.min, 0.0), (row["max_mcse_rel"], rel, np.max, 1e-12)):
                x = x[np.isfinite(x)]
                if x.size == 0:
                    assert np.isnan(got), (v, row)
                else:
                    assert abs(got - red(x)) <= tol * abs(red(x)), (v, row, red(x))


# (first, W, N) on a ring of 64 after 80 snapshots (16 .. 79 live, snapshot 64 in slot 0): the last straddles the wrap
WINDOWS = ((70, 1, 4), (20, 4, 5), (30, 2, 16), (56, 2, 8))


def reference(e, first, W, N, max_lag, slab_cols):
    mu, om = e.trace_get(first, W * N)
    chain = np.concatenate([mu, om], axis=1).reshape(W, N, 2 * e.D)
    return e.chain_summary(chain, probs=(), max_lag=max_lag, slab_cols=slab_cols)


def case_summary(lib, shape, mode):
    """capacity = 64, every = 1, 80 steps.  Every per-column output of trace_summary matches Engine.chain_summary on the trace_get arrays
    byte for byte -- slab_cols 0 and 32 (several slabs, the last partly filled: 2 D is no multiple of 32), max_lag 0 and 3 -- any subset of
    NULL outputs gives the same bytes for the rest, and the verdict is the recount of the columns, rhat_max 1.0 and 1e9 included."""
    with engine(lib, shape, mode) as e:
        assert (2 * e.D) % 32 != 0 and 2 * e.D > 64
        e.trace_begin(1, 64)
        e.run(50)
        e.run(30)
        assert e.trace_count() == (80, 16)
        ring = e.trace_get(16, 64)
        params = e.get_params()
        for first, W, N in WINDOWS:
            for slab in (0, 32):
                for lag in (0, 3):
                    s = e.trace_summary(first, W, N, max_lag=lag, slab_cols=slab, columns=True)
                    ref = reference(e, first, W, N, lag, slab)
                    for k in COLS:
                        assert bits(s[k]) == bits(ref[k]), (shape, mode, first, W, N, slab, lag, k)
                    recount(e, s, 1.1)
            assert np.isfinite(s["rhat"]).any()
            for only in (("sd", "rhat"), ("n_lags",), ("mean",), ()):
                part = e.trace_summary(first, W, N, max_lag=3, slab_cols=32, columns=True, only=only)
                assert set(part) == set(only) | {"blocks"}
                assert all(bits(part[k]) == bits(s[k]) for k in only) and part["blocks"].equals(s["blocks"]), only
            none = e.trace_summary(first, W, N, max_lag=3, slab_cols=32, columns=True, blocks=False)
            assert "blocks" not in none and all(bits(none[k]) == bits(s[k]) for k in COLS)
            for rmax in (1.0, 1e9):
                t = e.trace_summary(first, W, N, max_lag=3, slab_cols=32, columns=True, rhat_max=rmax)
                recount(e, t, rmax)
                assert rmax == 1.0 or (t["blocks"]["n_above"] == 0).all()
        assert same(e.trace_get(16, 64), ring) and same(e.get_params(), params) and e.trace_count() == (80, 16)
        print(f"summary {shape} mode {mode}: {e.kernel_name()}: {len(WINDOWS)} windows x 2 slab widths x 2 lag bounds bit-equal to chain_summary")


def case_verdict_frozen(lib):
    """eta = 0: the parameters do not move, every column is constant."""
    with engine(lib, "fitness", 1, eta=0.0) as e:
        e.trace_begin(1, 8)
        e.run(8)
        s = e.trace_summary(0, 2, 4, columns=True)
        recount(e, s, 1.1)
        b = s["blocks"]
        assert (b["n_const"] == b["n_cols"]).all() and (b["n_above"] == 0).all() and (b["n_nonfinite"] == 0).all()
        assert b[["max_rhat", "min_ess", "max_mcse_rel"]].isna().all().all()


def case_verdict_nonfinite(lib, mode):
    """A NaN planted in one logsigma_bc mean through set_params before the trace's steps: bb_run reports BB_ERR_NONFINITE, the steps are
    taken and the snapshots recorded.  The block's n_nonfinite counts exactly the columns chain_summary reports as NaN; a block whose
    columns keep their bytes against a clean twin keeps its verdict's."""
    import barbay_jl_amd as bb
    with engine(lib, "fitness", mode) as e, engine(lib, "fitness", mode) as clean:
        D, lay = e.D, e.layout()
        lo, hi = next((lo, hi) for nm, lo, hi in lay if nm == "logsigma_bc")
        for x in (e, clean):
            x.trace_begin(1, 16)
        mu, om = e.get_params()
        mu[lo + 3] = np.nan
        e.set_params(mu, om)
        assert e.trace_count() == (0, 0)
        with pytest.raises(bb.BarBayNonFinite):
            e.run(8)
        clean.run(8)
        assert e.trace_count() == clean.trace_count() == (8, 0) and e.stats()["steps_done"] == 8
        s, c = (x.trace_summary(0, 2, 4, columns=True) for x in (e, clean))
        ref = reference(e, 0, 2, 4, 0, 0)
        assert all(bits(s[k]) == bits(ref[k]) for k in COLS)
        recount(e, s, 1.1)
        recount(clean, c, 1.1)
        nb = len(lay)
        v = next(i for i, (nm, _, _) in enumerate(lay) if nm == "logsigma_bc")
        n_nan = int(np.isnan(ref["mean"][lo:hi]).sum())
        assert n_nan >= 1 and s["blocks"].iloc[v]["n_nonfinite"] == n_nan and (c["blocks"]["n_nonfinite"] == 0).all()
        kept = 0
        for w in range(2 * nb):
            _, blo, bhi = lay[w % nb]
            idx = np.concatenate([(w // nb) * D + np.arange(blo, bhi), D + np.arange(blo, bhi)])          # its columns and the omega means it divides by
            if all(bits(s[k][idx]) == bits(c[k][idx]) for k in COLS):
                assert s["blocks"].iloc[w].equals(c["blocks"].iloc[w]), w
                kept += 1
        print(f"non-finite mode {mode}: {e.kernel_name()}: {n_nan} NaN columns in logsigma_bc, {kept} of {2 * nb} verdicts keep their columns' bytes")


# ---------------------------------------------------------------------------------------------------------------------------
# 4. handle untouched, buffers shared
# ---------------------------------------------------------------------------------------------------------------------------
def _tbits(res):
    vals = list(res.values()) if isinstance(res, dict) else list(res)
    out = []
    for v in vals:
        if isinstance(v, pd.DataFrame):
            out += [str(list(v["name"])), str(list(v["part"]))] + [bits(v[k].to_numpy()) for k in v.columns[2:]]
        elif v is not None:
            out.append(bits(v))
    return out


def case_buffer_reuse(lib):
    """trace_summary interleaved with the other post-fit calls at changing sizes on one handle (the chain buffer regrows and is reused
    stale, as _rb_cases.check_buffer_reuse): every result is byte for byte what a fresh handle gives."""
    qs = (0.95, 0.675, 0.05)
    chain = np.random.default_rng(12).standard_normal((2, 40, 3001))

    def fresh():
        e = engine(lib, "fitness", 1)
        e.trace_begin(1, 16)
        e.run(12)
        return e

    calls = [lambda e: e.trace_summary(0, 2, 4, columns=True),
             lambda e: e.ppc_bands(qs, n_samples=111, n_ppc=7, seed=SEED),
             lambda e: e.trace_summary(2, 2, 5, slab_cols=32, columns=True),
             lambda e: e.fitness_rb(n_samples=111, seed=SEED),
             lambda e: e.chain_summary(chain),
             lambda e: e.trace_summary(0, 1, 12, max_lag=3, columns=True),
             lambda e: e.chain_summary(chain[:, :5, :6]),
             lambda e: e.trace_summary(0, 2, 4, columns=True)]
    with fresh() as e:
        got = [_tbits(f(e)) for f in calls]
    for i, f in enumerate(calls):
        with fresh() as e:
            assert got[i] == _tbits(f(e)), i
    assert got[0] == got[7]


def case_handle_untouched(lib, mode):
    """run(5); trace_summary; run(5) leaves the parameters, the ring, steps_done and the ELBO trace of a twin without the summary;
    set_params and init_meanfield under a trace discard the snapshots and keep the trace on."""
    with engine(lib, "fitness", mode) as a, engine(lib, "fitness", mode) as b:
        for x in (a, b):
            x.trace_begin(1, 8)
            x.run(5)
        s1 = b.trace_summary(1, 1, 4, columns=True)
        assert same(a.get_params(), b.get_params())
        s2 = b.trace_summary(1, 1, 4, columns=True)
        assert _tbits(s1) == _tbits(s2)
        for x in (a, b):
            x.run(5)
        assert same(a.get_params(), b.get_params()) and same(a.trace_get(2, 8), b.trace_get(2, 8))
        assert a.stats()["steps_done"] == b.stats()["steps_done"] == 10 and bits(a.elbo_trace(0, 4)) == bits(b.elbo_trace(0, 4))
        mu, om = b.get_params()
        b.set_params(mu, om)
        assert b.trace_count() == (0, 0)
        b.run(3)
        assert b.trace_count() == (3, 0) and same([r[2] for r in b.trace_get(0, 3)], b.get_params())
        b.init_meanfield()
        assert b.trace_count() == (0, 0)
        b.run(1)
        assert b.trace_count() == (1, 0)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. errors
# ---------------------------------------------------------------------------------------------------------------------------
def case_errors(lib):
    import barbay_jl_amd as bb
    err = bb.BarBayHipError
    sp = spec("fitness")
    with engine(lib, "fitness", 1) as e:
        e.trace_end()          # without a trace: BB_OK
        for call in (lambda: e.trace_count(), lambda: e.trace_get(0, 1), lambda: e.trace_summary(0, 1, 4)):
            with pytest.raises(err, match="error -1: .*no iterate trace is on"):
                call()
        for every, cap in ((0, 8), (-1, 8), (1, 7), (1, 16385)):
            with pytest.raises(err, match="error -1: .*(every must be|capacity = )"):
                e.trace_begin(every, cap)
        e.trace_begin(2, 8)
        with pytest.raises(err, match="error -1: .*on already"):
            e.trace_begin(2, 8)
        for name, call in (("bb_run_profiled", lambda: e.run_profiled(2)), ("bb_step_moments", lambda: e.step_moments()),
                           ("bb_step_apply", lambda: e.step_apply(np.zeros(int(e.stats()["n_moments"]))))):
            with pytest.raises(err, match=f"error -4: {name} is not available while an iterate trace is on"):
                call()
        assert e.stats()["steps_done"] == 0
        e.run(20)
        assert e.trace_count() == (10, 2)
        ok = dict(first=2, n_chains=2, n_draws=4)
        e.trace_summary(**ok)
        for bad in (dict(n_chains=0), dict(n_draws=3), dict(max_lag=-1), dict(slab_cols=-1), dict(rhat_max=0.5), dict(rhat_max=np.nan),
                    dict(rhat_max=np.inf)):
            with pytest.raises(err, match="error -1: .*(must be)"):
                e.trace_summary(**{**ok, **bad})
        with pytest.raises(err, match="error -4: .*must be <= 16384"):
            e.trace_summary(2, 5, 4000)
        for first, W, N in ((1, 2, 4), (3, 2, 4), (0, 1, 4), (7, 1, 4), (-1, 1, 4)):
            with pytest.raises(err, match=r"error -1: bb_trace_summary: .*the ring holds 2 \.\. 9 "):
                e.trace_summary(first, W, N)
        e.trace_end()
        e.trace_end()
        e.run_profiled(1)          # available again
    with make_engine(sp, lib, seed=SEED, rank=0, world_size=2, launch_mode=1) as e:
        with pytest.raises(err, match="error -4: .*sharded handle"):
            e.trace_begin(1, 8)
    with make_engine(sp, lib, seed=SEED, device_ids=[0, 0], launch_mode=1) as e:
        with pytest.raises(err, match="error -4: .*multi-device handle"):
            e.trace_begin(1, 8)
        e.trace_end()


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the stopping rule, end to end (host logic: it runs on the emulation too)
# ---------------------------------------------------------------------------------------------------------------------------
def load(name):
    return pd.read_csv(os.path.join(GOLD, name + ".csv"))


# Chosen on the CPU, with the emulation, so that the run stops by itself at no more than half of max_iters.  The iterates of the default
# optimiser (eta 0.1, a window of 100 gradients) are a slow random walk about the optimum: over any window a fit of 10 000 steps affords,
# most columns sit far above 1.1 -- 2 to 6 -- whatever the thinning.  eta = 5 with a window of 10 gradients mixes within a few hundred
# steps; 4 segments of 100 snapshots 25 steps apart then give split-R-hat at most 1.06 .. 1.09 over all columns for the seeds 1, 2, 3, 4, 11,
# and the first window that exists (10 000 steps) is already within the rule (data002, seed 2: the second, 12 500).
MAX_ITERS = 25000
OPT = dict(eta=5.0, tau=40.0, n=10)
CONV = dict(every=25, window=400, n_chains=4, check_every=2500, rhat_max=1.1, max_share=0.0)


def fit(lib, conv, data="data001_single", model="fitness_normal", max_iters=MAX_ITERS, **kw):
    import barbay_jl_amd as bb
    return bb.vi.advi(data=load(data), model=getattr(bb.model, model), advi=bb.vi.ADVI(1, max_iters), opt=bb.vi.TruncatedADAGrad(**OPT),
                      seed=SEED, verbose=False, convergence=conv, engine_kwargs=dict(_lib=lib, launch_mode=1), **kw)


def twin_engine(lib, data="data001_single", model="fitness_normal", **cols):
    """The engine vi.vi makes for the fit above."""
    import barbay_jl_amd as bb
    a = bb.utils.data_to_arrays(load(data), **cols)
    bm = getattr(bb.model, model)(a.bc_count, a.bc_total, a.n_neutral, a.n_bc)
    return bb.vi.make_engine(bm, bb.vi.ADVI(1, MAX_ITERS), bb.vi.TruncatedADAGrad(**OPT), SEED, 0, _lib=lib, launch_mode=1)


def traced_twin(lib, steps, **kw):
    """A twin engine stepped by the calls of the monitored run: the trace's cuts and run(check_every) up to `steps`."""
    e = twin_engine(lib, **kw)
    e.trace_begin(CONV["every"], CONV["window"])
    for _ in range(steps // CONV["check_every"]):
        e.run(CONV["check_every"])
    assert e.stats()["steps_done"] == steps
    return e


def averaged(e):
    """The averaged iterate of the last full window, as run_monitored forms it."""
    taken, _ = e.trace_count()
    first = taken - CONV["window"]
    W = CONV["n_chains"]
    return first, e.trace_summary(first, W, CONV["window"] // W, columns=True, only=("mean",), blocks=False)["mean"]


def case_stopping_rule(lib):
    """data001_single, fitness_normal, the settings above: the run stops by itself -- in the emulation at step 10 000 of 25 000, the first
    window that exists (max split-R-hat 1.062).  The frame is plain advi's in columns and rows; the averaged fit reports the window mean of
    (mu, omega); average=False the last iterate, Engine.posterior() of a twin stepped by the same calls."""
    import barbay_jl_amd as bb
    df = fit(lib, bb.vi.Convergence(**CONV))
    c = df.attrs["convergence"]
    print(f"stopping rule: converged {c['converged']} at step {c['steps']} of {MAX_ITERS}, window from step {c['window_first_step']}, "
          f"max rhat {c['blocks']['max_rhat'].max():.4f}, max mcse_rel {c['blocks']['max_mcse_rel'].max():.3g}")
    assert c["converged"] is True and CONV["every"] * CONV["window"] <= c["steps"] < MAX_ITERS and c["steps"] % CONV["check_every"] == 0
    assert c["window_first_step"] == c["steps"] - CONV["every"] * (CONV["window"] - 1)
    b = c["blocks"]
    assert bb.vi.blocks_within_rule(b, 0.0) and (b["n_nonfinite"] == 0).all() and (b["n_above"] == 0).all() and b["max_rhat"].max() <= 1.1
    plain = fit(lib, None, max_iters=50)
    assert "convergence" not in plain.attrs
    assert list(df.columns) == list(plain.columns) and len(df) == len(plain) and list(df["varname"]) == list(plain["varname"])
    with traced_twin(lib, c["steps"]) as t:
        D = t.D
        last = t.posterior()
        first, mean = averaged(t)
        assert (first + 1) * CONV["every"] == c["window_first_step"]
        t.trace_end()
        t.set_params(mean[:D], mean[D:])
        avg = t.posterior()
    assert len(df) == D and same((df["mean"].to_numpy(), df["std"].to_numpy()), avg)
    assert not same((df["mean"].to_numpy(),), (last[0],))
    df2 = fit(lib, bb.vi.Convergence(**{**CONV, "average": False}))
    c2 = df2.attrs["convergence"]
    assert c2["converged"] and c2["steps"] == c["steps"] and c2["blocks"].equals(b)
    assert same((df2["mean"].to_numpy(), df2["std"].to_numpy()), last)


def case_never_converges(lib):
    """rhat_max = 1.0 runs to max_iters, reports converged False, and is still averaged."""
    import barbay_jl_amd as bb
    n = 12500
    df = fit(lib, bb.vi.Convergence(**{**CONV, "rhat_max": 1.0}), max_iters=n)
    c = df.attrs["convergence"]
    assert c["converged"] is False and c["steps"] == n and c["window_first_step"] == n - CONV["every"] * (CONV["window"] - 1)
    assert c["blocks"]["n_above"].sum() > 0 and not bb.vi.blocks_within_rule(c["blocks"], 0.0)
    with traced_twin(lib, n) as t:
        _, mean = averaged(t)
        t.trace_end()
        t.set_params(mean[:t.D], mean[t.D:])
        assert same((df["mean"].to_numpy(), df["std"].to_numpy()), t.posterior())
    # fewer steps than one window: nothing is summarised, the last iterate is reported
    df = fit(lib, bb.vi.Convergence(**CONV), max_iters=300)
    c = df.attrs["convergence"]
    assert c == dict(converged=False, steps=300, window_first_step=None, blocks=None)
    with traced_twin(lib, 0) as t:
        t.run(300)
        assert same((df["mean"].to_numpy(), df["std"].to_numpy()), t.posterior())


def case_convergence_none(lib):
    """convergence=None: the fixed number of steps and the last iterate, as before -- the frame's mean and std are the bytes of
    Engine.posterior() after one run(max_iters) on an engine that never heard of a trace."""
    df = fit(lib, None, max_iters=500)
    assert "convergence" not in df.attrs
    with twin_engine(lib) as t:
        t.run(500)
        assert same((df["mean"].to_numpy(), df["std"].to_numpy()), t.posterior())


def case_hierarchical(lib):
    """data002_hier-rep, replicate_fitness_normal: the derived bc_fitness rows (reported as median and std of n = 10 000 draws of
    theta + exp(logtau) theta_tilde) are sampled from the averaged q.  Their medians lie within 6 Monte-Carlo standard errors of a direct
    hier_fitness at the averaged parameters under another seed -- the standard error of the difference of two independent sample medians
    of n draws, sqrt(2) sqrt(pi / 2) sd / sqrt(n) -- and at the same seed they are its bytes; at the last iterate they are not.
    In the emulation the run stops at step 10 000."""
    import barbay_jl_amd as bb
    kw = dict(data="data002_hier-rep", model="replicate_fitness_normal", rep_col="rep")
    df = fit(lib, bb.vi.Convergence(**CONV), **kw)
    c = df.attrs["convergence"]
    print(f"hierarchical: converged {c['converged']} at step {c['steps']} of {MAX_ITERS}, max rhat {c['blocks']['max_rhat'].max():.4f}")
    assert c["converged"] is True and c["steps"] < MAX_ITERS
    n = 10_000
    with traced_twin(lib, c["steps"], **kw) as t:
        D = t.D
        rows = df.iloc[D:]
        assert len(rows) == t.hier_units() > 0 and (rows["vartype"] == "bc_fitness").all()
        last = t.hier_fitness(n, seed=SEED)
        _, mean = averaged(t)
        t.trace_end()
        t.set_params(mean[:D], mean[D:])
        assert same((df["mean"].to_numpy()[:D], df["std"].to_numpy()[:D]), t.posterior())
        med, sd = t.hier_fitness(n, seed=SEED)
        med2, sd2 = t.hier_fitness(n, seed=SEED + 1)
    got = rows["mean"].to_numpy()
    assert same((got, rows["std"].to_numpy()), (med, sd)) and not same((got,), (last[0],))
    se = np.sqrt(2.0) * np.sqrt(np.pi / 2.0) * sd2 / np.sqrt(n)
    z = np.abs(got - med2) / se
    print(f"hierarchical: {len(rows)} derived rows, worst |median - direct| = {z.max():.2f} standard errors")
    assert (z <= 6.0).all(), z.max()


# ---------------------------------------------------------------------------------------------------------------------------
# 7. GPU only
# ---------------------------------------------------------------------------------------------------------------------------
def case_traced_against_uncut(lib, mode, row):
    """One bb_run(40) under a trace (every = 7: pieces of 7, 7, 7, 7, 7, 5) against the same call untraced.  A cut run is not promised
    to equal an uncut one bit for bit -- a resident launch and a graph replay add in their own orders -- so the parameters are held to
    the plan-against-plan tolerance of the settings row of _run_cases.ROWS used."""
    r = rc.ROWS[row]
    kw = dict(samples_per_step=r["S"], optimizer=r["opt"], elbo_every=r["ev"], **r["kw"])
    with engine(lib, "fitness", mode, **kw) as e, engine(lib, "fitness", mode, **kw) as u:
        e.trace_begin(7, 8)
        e.run(40)
        u.run(40)
        assert e.trace_count() == (5, 0) and e.stats()["steps_done"] == u.stats()["steps_done"] == 40
        (m1, o1), (m2, o2) = e.get_params(), u.get_params()
        d = max(np.abs(m1 - m2).max(), np.abs(o1 - o2).max())
        print(f"traced against uncut, mode {mode} row {row}: {e.kernel_name()}: {d:.3e}")
        assert d < r["plans"], d


def case_tool_small(tmp_path):
    """tools/trace_cost.py --small: 2 000 barcodes, 200 steps, every = 10, both shapes."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(root, "tools", "trace_cost.py"), "--small", "--out", str(tmp_path)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    res = json.load(open(os.path.join(str(tmp_path), "trace_cost.json")))
    assert [s["shape"] for s in res["shapes"]] == ["bench", "genotype"]
    for s in res["shapes"]:
        assert s["steps_per_s_untraced"] > 0 and s["steps_per_s_traced"]["10"] > 0 and s["summary_s_min"] > 0
        assert len(s["verdict"]) in (10, 14) and all(v["n_nonfinite"] == 0 for v in s["verdict"])
