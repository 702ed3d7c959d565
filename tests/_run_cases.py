"""bb_run's bookkeeping around the step, shared by the emulation tests (CPU, `-m "not gpu"`) and the GPU tests (`-m gpu`): which step a
launch believes it is at and what follows from that number -- the window slot, the re-add counter, the ELBO recording period and its
ring, the 4096-step launch cut, hipGraph replay, and the non-finite status.  Each case takes the loaded C-ABI library (`lib`) and one
row of PATHS, and compares the engine with the literal oracle."""
import functools
import math

import numpy as np
import pytest

import _cases as c
from conftest import make_engine
from oracle import advi, literal

# The launch paths: shape (a row of _cases.SYNTH), engine settings, BB_TUNE_* environment, bb_stats.resident_kernel, kernel_name() prefix.
# k_persist has no instance with several samples per step or ELBO recording: the library takes k_res's MS instances there (kernel 2).
PATHS = {
    "two_kernel": dict(shape="fitness_T6", kw=dict(launch_mode=1, steps_per_graph=-1), env={}, kernel=0, prefix="k_sample"),
    "k_persist": dict(shape="fitness_multi_tile", kw=dict(launch_mode=2), env={}, kernel=1, prefix="k_persist<"),
    "k_res": dict(shape="fitness_T6", kw=dict(launch_mode=2), env={}, kernel=2, prefix="k_res<"),
    "k_res_genotype": dict(shape="genotype_runs", kw=dict(launch_mode=2), env={}, kernel=2, prefix="k_res<2,"),
    "k_stream": dict(shape="replicate_R3_T6", kw=dict(launch_mode=2), env=dict(BB_TUNE_NB="100", BB_TUNE_NTHR="512", BB_TUNE_STREAM="1"),
                     kernel=3, prefix="k_stream<"),
}
# the frozen run's paths (fitness_T4): k_stream's geometry is test_streaming_resident_launch's for this shape
FROZEN_PATHS = {
    "two_kernel": dict(kw=dict(launch_mode=1, steps_per_graph=-1), env={}, kernel=0, prefix="k_sample"),
    "k_res": dict(kw=dict(launch_mode=2), env={}, kernel=2, prefix="k_res<"),
    "k_stream": dict(kw=dict(launch_mode=2), env=dict(BB_TUNE_NB="333", BB_TUNE_NTHR="1024", BB_TUNE_STREAM="1"), kernel=3, prefix="k_stream<"),
}

# A: the settings rows.  tol: each plan against the oracle; plans: plan against plan; trace: relative, the project's own trace tolerances
ROWS = {
    1: dict(S=1, ev=3, opt="TruncatedADAGrad", kw=dict(resum_every=1), tol=1e-10, plans=1e-11, trace=1e-10),
    2: dict(S=2, ev=2, opt="DecayedADAGrad", kw={}, tol=1e-10, plans=1e-11, trace=1e-10),
    3: dict(S=1, ev=0, opt="TruncatedADAGrad", kw=dict(resum_every=3), tol=1e-6, plans=1e-6, trace=None),      # the lean instances, the rs counter
    4: dict(S=2, ev=3, opt="TruncatedADAGrad", kw=dict(resum_every=0), tol=1e-6, plans=1e-6, trace=1e-6),
}
NSTEPS, WINDOW, SEED = 23, 5, 11
PLANS = ([23], [1, 6, 5, 11])          # the second: launches start at steps 1, 7, 12 -- odd, off phase for W = 5 and periods 3 and 2


@functools.lru_cache(maxsize=None)
def _sp(name):
    return c.synth(name, seed=2)


def set_env(monkeypatch, path):
    for k, v in path["env"].items():
        monkeypatch.setenv(k, v)


def check_instance(e, path, ms=False):
    """The kernel instance the handle runs: bb_stats.resident_kernel and kernel_name()."""
    k, nm = e.stats()["resident_kernel"], e.kernel_name()
    nm = nm[4:] if nm.startswith("emu:") else nm          # (the emulation names the instance whose block programs it steps)
    want, prefix = path["kernel"], path["prefix"]
    if want == 1 and ms:
        want, prefix = 2, "k_res<"
    assert k == want and nm.startswith(prefix), (k, nm)
    if ms and want >= 2:
        assert nm.endswith(",true>"), nm          # the MS instances
    return nm


# ---------------------------------------------------------------------------------------------------------------------------
# A. split launches against the oracle loop
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_loop(name, S, optname, mu0_b, om0_b, perm_b):
    """advi.run_advi on literal.elbo_and_grad over the 23 steps from the handle's initial parameters (as _cases._trajectory; the draws
    in the caller's order).  Cached on what determines it: both plans, every path of a shape and the settings rows that differ only in
    the engine's own schedules (elbo_every, resum_every) share one loop."""
    sp = _sp(name)
    mu0, om0, perm = np.frombuffer(mu0_b), np.frombuffer(om0_b), np.frombuffer(perm_b, dtype=np.int64)

    class _E:          # what caller_normals asks of an engine
        @staticmethod
        def permutation():
            return perm
    opt = advi.TruncatedADAGrad(n=WINDOW) if optname == "TruncatedADAGrad" else advi.DecayedADAGrad()
    f = lambda m, o, eps: literal.elbo_and_grad(m, o, eps, sp)
    eps_fn = lambda i: np.stack([c.caller_normals(_E, SEED, i, s, sp.D) for s in range(S)])
    m, o, tr = advi.run_advi(sp, f, mu0, om0, NSTEPS, S, opt, SEED, eps_fn=eps_fn)
    for a in (m, o, tr):
        a.setflags(write=False)
    return m, o, tr


def _check_trace(e, r, tr, done):
    """The recorded ELBOs after `done` steps: the oracle's at the recording steps taken so far, NaN for those not yet taken."""
    ev = r["ev"]
    n = math.ceil(NSTEPS / ev)
    got = e.elbo_trace(0, n)
    want = tr[::ev]
    have = np.arange(n) * ev < done
    assert np.isnan(got[~have]).all(), (done, got)
    assert np.abs(got[have] - want[have]).max() <= r["trace"] * np.abs(want).max(), (done, got, want)
    if ev == 3:
        assert np.isnan(e.elbo_trace(1, 3)).all()          # first step off phase
    edge = e.elbo_trace(-ev, 2)          # [before the run, step 0]
    assert np.isnan(edge[0]) and abs(edge[1] - tr[0]) <= r["trace"] * np.abs(want).max(), edge


def case_split_launches(lib, pname, row):
    path, r = PATHS[pname], ROWS[row]
    name = path["shape"]
    sp = _sp(name)
    ms = r["S"] > 1 or r["ev"] > 0
    outs = []
    for plan in PLANS:
        with make_engine(sp, lib, seed=SEED, samples_per_step=r["S"], optimizer=r["opt"], window=WINDOW, elbo_every=r["ev"],
                         **r["kw"], **path["kw"]) as e:
            nm = check_instance(e, path, ms)
            mu0, om0 = e.get_params()
            m2, o2, tr = _oracle_loop(name, r["S"], r["opt"], mu0.tobytes(), om0.tobytes(), e.permutation().tobytes())
            done = 0
            for n in plan:
                e.run(n)
                done += n
                assert e.stats()["steps_done"] == done
                if r["ev"] > 0:
                    _check_trace(e, r, tr, done)
            mu, om = e.get_params()
        a, b = np.abs(mu - m2).max(), np.abs(om - o2).max()
        print(f"{pname} row {row} plan {plan}: {nm}: against the oracle loop |dmu| {a:.3e} |domega| {b:.3e}")
        assert a < r["tol"] and b < r["tol"], (plan, a, b)
        outs.append((mu, om))
    d = max(np.abs(outs[0][0] - outs[1][0]).max(), np.abs(outs[0][1] - outs[1][1]).max())
    print(f"{pname} row {row}: {nm}: plan against plan {d:.3e}")
    assert d < r["plans"], d


# ---------------------------------------------------------------------------------------------------------------------------
# B. the ELBO ring's wrap and the 4096-step launch cut on a frozen run
# ---------------------------------------------------------------------------------------------------------------------------
RING = 4096          # BB_ELBO_RING
FROZEN_STEPS = 4200
# Every live entry (steps 104..4199: both ends, the launch cut and the ring's wrap at 4095 | 4096, every window slot at every ring slot)
# is checked against the oracle.  The 4096 literal evaluations are made once: every path and both handles of a shape share them
# (_frozen_elbo).


@functools.lru_cache(maxsize=None)
def _frozen_elbo(name, step, mu0_b, om0_b):
    """The ELBO estimate of one step at the frozen parameters: each recorded value depends on (mu0, omega0) and its step's draws only."""
    sp = _sp(name)
    mu0, om0 = np.frombuffer(mu0_b), np.frombuffer(om0_b)

    class _E:          # (no genotype shape here: the caller's order is the handle's)
        @staticmethod
        def permutation():
            return np.arange(sp.D)
    return literal.elbo_and_grad(mu0, om0, c.caller_normals(_E, SEED, step, 0, sp.D)[None], sp)[0]


def _frozen_engine(lib, sp, path):
    return make_engine(sp, lib, seed=SEED, eta=0.0, elbo_every=1, samples_per_step=1, window=4, resum_every=1, **path["kw"])


def case_frozen_ring(lib, pname):
    """eta = 0: the update is d * (0 * ...) = 0, the parameters do not move, and every recorded ELBO can be checked against the literal
    oracle on its own, however long the run.  4200 steps wrap the 4096-entry ring and cross the 4096-step cut of a resident launch."""
    path, name = FROZEN_PATHS[pname], "fitness_T4"
    sp = _sp(name)
    resident = path["kernel"] > 0

    def spot(tr, first, steps):
        mu0_b, om0_b = mu0.tobytes(), om0.tobytes()
        steps = np.asarray(steps)
        want = np.array([_frozen_elbo(name, int(st), mu0_b, om0_b) for st in steps])
        got = tr[steps - first]
        bad = np.nonzero(~(np.abs(got - want) <= 1e-10 * np.abs(want)))[0]
        assert bad.size == 0, (bad.size, [(int(steps[k]), got[k], want[k]) for k in bad[:4]])
        return (np.abs(got - want) / np.abs(want)).max()

    def frozen(e):
        m, o = e.get_params()
        assert np.array_equal(m, mu0) and np.array_equal(o, om0)

    with _frozen_engine(lib, sp, path) as e:
        nm = check_instance(e, path, ms=True)
        assert (e.permutation() == np.arange(sp.D)).all()
        mu0, om0 = e.get_params()
        e.run(FROZEN_STEPS)
        frozen(e)
        st = e.stats()
        assert st["steps_done"] == FROZEN_STEPS
        if resident:
            assert st["launches_last_run"] == 2, st
        tr = e.elbo_trace(0, FROZEN_STEPS)
        lo = FROZEN_STEPS - RING          # 104: the oldest entry the ring still holds
        assert np.isnan(tr[:lo]).all() and np.isfinite(tr[lo:]).all(), (np.isnan(tr).sum(), np.nonzero(np.isnan(tr[lo:]))[0][:8])
        worst = spot(tr, 0, range(lo, FROZEN_STEPS))
        e.run(4000)          # 8200 steps in all
        frozen(e)
        assert e.stats()["steps_done"] == 8200
        tail = e.elbo_trace(4103, 8200 - 4103)
        assert np.isnan(tail[0]) and np.isfinite(tail[1:]).all()
        spot(tail, 4103, (4104, 8199))
    print(f"frozen {pname}: {nm}: ring wrapped twice, launch cut crossed; {RING} live entries against the oracle, worst {worst:.2e} relative")
    # the same 4200 steps in three calls: the second starts on the last step of the first launch's 4096, the third straddles nothing
    with _frozen_engine(lib, sp, path) as e:
        m, o = e.get_params()
        assert np.array_equal(m, mu0) and np.array_equal(o, om0)
        for n in (4095, 2, 103):
            e.run(n)
        frozen(e)
        assert e.stats()["steps_done"] == FROZEN_STEPS
        tr = e.elbo_trace(0, FROZEN_STEPS)
        assert np.isnan(tr[:lo]).all() and np.isfinite(tr[lo:]).all()
        worst = spot(tr, 0, range(lo, FROZEN_STEPS))
    print(f"frozen {pname}: {nm}: run(4095), run(2), run(103): {RING} live entries against the oracle, worst {worst:.2e} relative")


# ---------------------------------------------------------------------------------------------------------------------------
# C. hipGraph replay against the oracle loop (GPU only: the emulation has no graphs)
# ---------------------------------------------------------------------------------------------------------------------------
def case_graph_replay(lib, name, g, S, optname):
    """run(3), run(20) with graphs of g steps (4 or 6: neither divides the window of 5, so every replay starts at another slot): the
    second call starts on the odd step 3, takes one step eagerly, floor(19 / g) graphs, and the rest eagerly."""
    sp = _sp(name)
    kw = dict(seed=SEED, samples_per_step=S, optimizer=optname, launch_mode=1, elbo_every=0, window=WINDOW, resum_every=1)
    outs = []
    for spg in (g, -1):
        with make_engine(sp, lib, steps_per_graph=spg, **kw) as e:
            assert e.stats()["resident_kernel"] == 0 and e.kernel_name().startswith("k_sample<"), e.kernel_name()
            mu0, om0 = e.get_params()
            e.run(3)
            assert e.graph_launches() == 0          # fewer steps than one graph
            e.run(20)
            n = e.graph_launches()
            print(f"graph {name} g={g} S={S} {optname}: steps_per_graph {spg}: {n} graph launches in run(20)")
            assert n == (19 // g if spg > 0 else 0), n
            assert e.stats()["steps_done"] == 23
            outs.append(e.get_params())
            perm = e.permutation()
    m2, o2, _ = _oracle_loop(name, S, optname, mu0.tobytes(), om0.tobytes(), perm.tobytes())
    a, b = np.abs(outs[0][0] - m2).max(), np.abs(outs[0][1] - o2).max()
    d = max(np.abs(outs[0][0] - outs[1][0]).max(), np.abs(outs[0][1] - outs[1][1]).max())
    print(f"graph {name} g={g} S={S} {optname}: against the oracle loop {a:.3e} {b:.3e}, against eager {d:.3e}")
    assert a < 1e-10 and b < 1e-10, (a, b)
    assert d < 1e-11, d


# ---------------------------------------------------------------------------------------------------------------------------
# D. bb_run_profiled: bb_run's two-kernel step with events between the two launches
# ---------------------------------------------------------------------------------------------------------------------------
def case_run_profiled(lib, row, gpu):
    """run_profiled(7) launches the kernels run(7) launches, with the same arguments in the same order: parameters, step count and ELBO
    trace are equal bit for bit (as test_graph_equals_eager holds graph replay to eager).  On the GPU it leaves the two launches' mean
    times in bb_stats.  A multi-device handle is refused, and on the GPU a handle that reduces (world_size = 2) too; the emulation has no
    clock, runs bb_run in its place and so has nothing to refuse there."""
    import barbay_jl_amd as bb
    path, r = PATHS["two_kernel"], ROWS[row]
    sp = _sp(path["shape"])
    kw = dict(seed=SEED, samples_per_step=r["S"], optimizer=r["opt"], window=WINDOW, elbo_every=r["ev"], **r["kw"], **path["kw"])
    n = math.ceil(7 / r["ev"])
    outs = []
    for profiled in (False, True):
        with make_engine(sp, lib, **kw) as e:
            check_instance(e, path)
            outs.append([e.get_params()])
            (e.run_profiled if profiled else e.run)(7)
            st = e.stats()
            outs[-1] += [e.get_params(), st["steps_done"], e.elbo_trace(0, n)]
    (p0, p1, done, tr), (q0, q1, qdone, qtr) = outs
    assert np.array_equal(p0[0], q0[0]) and np.array_equal(p0[1], q0[1])          # the same initial state
    assert not np.array_equal(p0[0], p1[0])          # ... which the seven steps moved
    assert np.array_equal(p1[0], q1[0]) and np.array_equal(p1[1], q1[1])
    assert done == qdone == 7
    assert np.isfinite(tr).all() and np.array_equal(tr, qtr), (tr, qtr)
    print(f"run_profiled row {row}: avg_sample_ms {st['avg_sample_ms']:.4f} avg_update_ms {st['avg_update_ms']:.4f}")
    if gpu:
        assert st["avg_sample_ms"] > 0 and st["avg_update_ms"] > 0, st
        with make_engine(sp, lib, rank=0, world_size=2, **kw) as e:
            with pytest.raises(bb.BarBayHipError, match="single-GPU two-kernel step only"):
                e.run_profiled(7)
    with make_engine(sp, lib, device_ids=[0, 0], **kw) as e:
        with pytest.raises(bb.BarBayHipError, match="not available on a multi-device handle"):
            e.run_profiled(7)


# ---------------------------------------------------------------------------------------------------------------------------
# E. the non-finite status
# ---------------------------------------------------------------------------------------------------------------------------
def case_nonfinite(lib, pname):
    """A NaN / Inf planted in any block of the parameters makes bb_run return BB_ERR_NONFINITE -- after taking its steps, with the state
    still readable -- and the flag belongs to the run that set it: the next run from finite parameters succeeds."""
    import barbay_jl_amd as bb
    path = PATHS[pname]
    sp = _sp(path["shape"])
    with make_engine(sp, lib, seed=SEED, window=WINDOW, **path["kw"]) as e:
        nm = check_instance(e, path)
        mu0, om0 = e.get_params()
        lay = e.layout()
        plants = []
        for k, (blk, lo, hi) in enumerate(lay):
            for i in sorted({lo, hi - 1}):          # the last index: the last tile, the single-latent lanes
                plants.append((blk, "mu", i, np.nan))
            if k == 0:
                plants += [(blk, "mu", lo, np.inf), (blk, "omega", lo, np.nan)]
        for blk, which, i, v in plants:
            mu, om = mu0.copy(), om0.copy()
            (mu if which == "mu" else om)[i] = v
            e.set_params(mu, om)
            before = e.stats()["steps_done"]
            with pytest.raises(bb.BarBayNonFinite):
                e.run(2)
                pytest.fail(f"{pname} ({nm}): {which}[{i}] = {v} in block {blk}: bb_run returned success")
            assert e.stats()["steps_done"] == before + 2, (blk, which, i)
            m, o = e.get_params()
            assert not (np.isfinite(m).all() and np.isfinite(o).all()), (blk, which, i)
            e.set_params(mu0, om0)
            e.run(2)          # must not raise: nothing of the last run's flag is left
            m, o = e.get_params()
            assert np.isfinite(m).all() and np.isfinite(o).all(), (blk, which, i)
    print(f"non-finite {pname}: {nm}: {len(plants)} plants over {len(lay)} blocks")
