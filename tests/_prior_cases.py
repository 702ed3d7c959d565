"""Matrix-form (per-element) priors and non-default optimiser constants on every launch path, shared by the emulation tests (CPU,
tests/test_emu_priors.py) and the GPU tests (tests/test_gpu_priors.py).  The prior is read by code that exists in several copies --
bb_prior_of (the two-kernel step, k_persist, bb_logp.h), br_pair_prior (k_res: Vector form from the tile's segment in LDS, Matrix form
through mean_e[], the pair's second element under the any-parity mask), the loglambda term folded into the gradient in the exchange's
shadow, k_stream's three call sites, the host-built segment tables, bb_create's regrouping of a scattered genotype model and its
loglambda-first reorder -- and the optimiser constants reach every kernel through a per-handle device table (DevState.optc).  Each
case takes the loaded C-ABI library and compares the engine with the literal oracle under priors that differ element by element by
orders of magnitude, and under constants that are nobody's default."""
import dataclasses
import functools

import numpy as np

import _cases as c
import _run_cases as r
from conftest import make_engine
from oracle import advi, literal, naive

# the constants of every trajectory here, on both sides (the defaults are 0.1, 40 and 0.1, 1.0, 0.9)
TRUNC = dict(optimizer="TruncatedADAGrad", eta=0.037, tau=3.5)
DECAY = dict(optimizer="DecayedADAGrad", eta=0.021, pre=0.8, post=0.65)
NSTEPS, WINDOW, SEED = 12, 4, 11
FORMS = ("stress", "naive", "vector")
SHAPE_SEED = {}          # shape -> seed of its counts and priors where it is not 2 (test_sensitivity says when to change one)
TOL, MODES_TOL, TRACE_RTOL = 1e-10, 1e-11, 1e-10          # the project's figures for exact-window trajectories


def _loglambda_counts(sp):
    """The counts in the loglambda block's own order: t fastest per barcode, replicate-major."""
    return np.concatenate([np.ascontiguousarray(cn.T).reshape(-1) for cn in sp.counts]).astype(np.float64)


def naive_means(sp):
    """`naive_prior` (src/stats.jl:1175-1359; oracle/naive.py is its loop-for-loop form) on the spec's raw counts, as arrays.  With a
    single neutral barcode the reference's corrected std over the neutrals is NaN -- a prior nobody can pass -- and the logsigma_pop
    means are then 0."""
    s_pop, ls_pop = [], []
    for R in sp.counts:
        R = R + 1.0
        f = R / R.sum(axis=1, keepdims=True)
        x = np.log(f[1:, :sp.n_neutral] / f[:-1, :sp.n_neutral])          # [T - 1, n_neutral]
        s_pop.append(-x.mean(axis=1))
        ls_pop.append(-x.std(axis=1, ddof=1) if sp.n_neutral > 1 else np.zeros(x.shape[0]))
    return np.concatenate(s_pop), np.concatenate(ls_pop), np.log(_loglambda_counts(sp) + 1.0)


def with_priors(sp, seed, form):
    """`sp` with priors of one of three forms, built from sp.blocks():
    stress -- every block but theta_tilde and logtau per element: mean N(0, 1) (loglambda: log(count + 1)), std log-uniform over
              [0.02, 5] ([0.05, 5] for loglambda), logtau_prior = (-1.3, 0.6): an element read from the wrong place shows by orders
              of magnitude, not in the last digits;
    naive  -- the documented usage (docs/src/examples.md:122-160): naive_prior's means in Matrix form for s_pop (std 0.05),
              logsigma_pop (std 1) and loglambda (std 3), Vector form for the rest -- a Vector / Matrix mix inside one handle;
    vector -- non-default Vector form for every block, logtau included: mean_e == nullptr, the constants of a tile's segment."""
    g = np.random.default_rng(seed)
    pri = {}
    if form == "stress":
        for name, n, pname in sp.blocks():
            if name in ("theta_tilde", "logtau"):
                continue
            lo = 0.05 if name == "loglambda" else 0.02
            mean = np.log(_loglambda_counts(sp) + 1.0) if name == "loglambda" else g.normal(0.0, 1.0, n)
            pri[pname] = (mean, np.exp(g.uniform(np.log(lo), np.log(5.0), n)))
        pri["logtau_prior"] = (-1.3, 0.6)
    elif form == "naive":
        s_pop, ls_pop, ll = naive_means(sp)
        pri = {"s_pop_prior": (s_pop, np.full(s_pop.shape, 0.05)), "logsigma_pop_prior": (ls_pop, np.ones(ls_pop.shape)),
               "loglambda_prior": (ll, np.full(ll.shape, 3.0)), "s_bc_prior": (0.0, 1.0), "logsigma_bc_prior": (float(ls_pop.mean()), 1.0)}
    elif form == "vector":
        pri = {"s_pop_prior": (0.3, 1.5), "logsigma_pop_prior": (-0.7, 0.8), "s_bc_prior": (0.2, 1.3), "logsigma_bc_prior": (-0.4, 0.6),
               "loglambda_prior": (4.0, 2.5), "logtau_prior": (-1.3, 0.6)}
    else:
        raise KeyError(form)
    return dataclasses.replace(sp, priors=pri)


@functools.lru_cache(maxsize=None)
def _sp(name, form=None):
    seed = SHAPE_SEED.get(name, 2)
    sp = c.synth(name, seed=seed)
    return sp if form is None else with_priors(sp, seed, form)


def _perm_engine(perm):
    class _E:          # what caller_normals asks of an engine
        @staticmethod
        def permutation():
            return perm
    return _E


def oracle_loop(sp, mu0, om0, perm, nsteps, S, opt, seed=SEED):
    """advi.run_advi on literal.elbo_and_grad from the handle's initial parameters, the handle's draws in the caller's order, the
    oracle's optimiser with the constants the handle was given."""
    opt = dict(opt)
    o = c.oracle_optimizer(opt.pop("optimizer"), window=WINDOW, **opt)
    f = lambda m, om, eps: literal.elbo_and_grad(m, om, eps, sp)
    eps_fn = lambda i: np.stack([c.caller_normals(_perm_engine(perm), seed, i, s, sp.D) for s in range(S)])
    return advi.run_advi(sp, f, mu0, om0, nsteps, S, o, seed, eps_fn=eps_fn)


@functools.lru_cache(maxsize=None)
def _oracle_cached(name, form, S, optname, mu0_b, om0_b, perm_b):
    """Cached on what determines it: the two launch modes, the graph and the eager run, and every path of a shape share one loop."""
    out = oracle_loop(_sp(name, form), np.frombuffer(mu0_b), np.frombuffer(om0_b), np.frombuffer(perm_b, dtype=np.int64), NSTEPS, S,
                      TRUNC if optname == "TruncatedADAGrad" else DECAY)
    for a in out:
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# A. trajectory against the literal oracle's loop, per launch path
# ---------------------------------------------------------------------------------------------------------------------------
def _row(shape, kernel, prefix, nb=0, nthr=0, ms=False, ap=None, graph=False, **env):
    """shape: a row of _cases.SYNTH; kernel / prefix: bb_stats.resident_kernel and what kernel_name() starts with; nb, nthr:
    BB_TUNE_NB / BB_TUNE_NTHR (0: the library's own geometry); ms: samples_per_step = 2, elbo_every = 1, DecayedADAGrad (the MS
    instances); ap: k_res's any-parity argument; graph: hipGraph replay of 4 steps (GPU only); env: further BB_TUNE_* settings."""
    e = {f"BB_TUNE_{k}": str(v) for k, v in env.items()}
    if nb:
        e.update(BB_TUNE_NB=str(nb), BB_TUNE_NTHR=str(nthr))
    kw = dict(launch_mode=1, steps_per_graph=4 if graph else -1) if kernel == 0 else dict(launch_mode=2)
    return dict(shape=shape, kernel=kernel, prefix=prefix, kw=kw, env=e, ms=ms, ap=ap, graph=graph)


A_ROWS = {}
for _s in ("fitness_multi_tile", "genotype", "replicate_ragged"):
    A_ROWS[f"two_kernel-{_s}"] = _row(_s, 0, "k_sample")
    A_ROWS[f"two_kernel_graph-{_s}"] = _row(_s, 0, "k_sample", graph=True)
for _s in ("fitness_multi_tile", "multienv", "replicate_ragged", "multienv_replicate_3d"):
    A_ROWS[f"k_persist-{_s}"] = _row(_s, 1, "k_persist<")
A_ROWS["k_persist-replicate_ragged-P2"] = _row("replicate_ragged", 1, "k_persist<3,2,512", nb=60, nthr=512)          # two pairs per thread
for _s in ("fitness_T6", "multienv_T8", "genotype_runs", "replicate_R3", "multienv_replicate_T6"):
    A_ROWS[f"k_res-{_s}"] = _row(_s, 2, "k_res<", ap=False)
A_ROWS["k_res-replicate_R3_T6-P2"] = _row("replicate_R3_T6", 2, "k_res<3,2,", ap=False)
A_ROWS["k_res_ap-genotype_T5"] = _row("genotype_T5", 2, "k_res<2,", ap=True)
for _s in ("multienv", "replicate_odd"):
    A_ROWS[f"k_res_ap-{_s}"] = _row(_s, 2, "k_res<", ap=True, AP=1)
# genotype_odd: loglambda would start at an odd flat index, so bb_create lays it out in FRONT of theta (loglambda_first) and the plain
# instance runs, also where the any-parity ones are asked for: the prior arrays keep the caller's order, the block that moves is the
# one whose prior is largest
A_ROWS["k_res_ap-genotype_odd"] = _row("genotype_odd", 2, "k_res<2,", ap=False, AP=1)
A_ROWS["k_res_ap-genotype_odd-24x128"] = _row("genotype_odd", 2, "k_res<2,", nb=24, nthr=128, ap=False, AP=1)
for _s in ("fitness_T6", "genotype_runs", "replicate_R3"):
    A_ROWS[f"k_res_ms-{_s}"] = _row(_s, 2, "k_res<", ms=True, ap=False)
A_ROWS["k_res_ms-multienv"] = _row("multienv", 2, "k_res<1,", ms=True, ap=True)          # AP + MS
for _s, _nb, _nthr in (("fitness_T6", 350, 1024), ("multienv_T8", 150, 512), ("genotype_T8", 250, 512), ("replicate_R3_T6", 100, 512),
                       ("multienv_replicate_T6", 75, 512)):
    A_ROWS[f"k_stream-{_s}"] = _row(_s, 3, "k_stream<", nb=_nb, nthr=_nthr, STREAM=1)
    # (the library has no 512-thread MS instance of the multienv kinds, and says so where one is asked for: their MS rows take the 1024
    #  threads of test_streaming_resident_launch_several_samples_and_elbo_trace)
    A_ROWS[f"k_stream_ms-{_s}"] = _row(_s, 3, "k_stream<", nb=_nb, nthr=1024 if _s.startswith("multienv") else _nthr, ms=True, STREAM=1)
EMU_ROWS = [k for k, v in A_ROWS.items() if not v["graph"]]          # (the emulation has no graphs)


def check_row_instance(e, row, xg=False):
    """The instance the handle runs, by the library's own word: _run_cases.check_instance's checks, and of a k_res instance
    "k_res<KIND,P,NT,XG,TT,AP,MS>" the cross-GPU, any-parity and several-samples arguments."""
    nm = r.check_instance(e, row, row["ms"])
    if nm.startswith("k_res<"):
        a = nm[6:-1].split(",")
        assert len(a) == 7 and a[3] == ("true" if xg else "false") and a[6] == ("true" if row["ms"] else "false"), nm
        if row["ap"] is not None:
            assert a[5] == ("true" if row["ap"] else "false"), nm
    if nm.startswith("k_stream<") and not row["ms"]:
        assert not nm.endswith(",true>"), nm
    return nm


def _settings(row):
    opt = DECAY if row["ms"] else TRUNC
    return opt, dict(seed=SEED, samples_per_step=2 if row["ms"] else 1, elbo_every=1 if row["ms"] else 0, window=WINDOW, resum_every=1, **opt)


def case_path(lib, rname, form):
    """One launch path under one form of priors: 12 steps, exact window, against the oracle's loop (1e-10), the recorded ELBOs where
    the row records them (1e-10 relative: their constant holds the sum of the log stds), and a resident row against the two-kernel
    step on the same handle settings (1e-11).  Set the row's environment first (_run_cases.set_env)."""
    row = A_ROWS[rname]
    sp = _sp(row["shape"], form)
    opt, kw = _settings(row)
    S = kw["samples_per_step"]
    outs = []
    for rw in ([row] if row["kernel"] == 0 else [row, dict(row, kernel=0, prefix="k_sample", kw=dict(launch_mode=1, steps_per_graph=-1))]):
        with make_engine(sp, lib, use_priors=True, **kw, **rw["kw"]) as e:
            nm = r.check_instance(e, rw) if rw is not row else check_row_instance(e, row)
            mu0, om0 = e.get_params()
            m2, o2, tr = _oracle_cached(row["shape"], form, S, opt["optimizer"], mu0.tobytes(), om0.tobytes(), e.permutation().tobytes())
            e.run(NSTEPS)
            assert e.stats()["steps_done"] == NSTEPS
            if row["graph"]:
                assert e.graph_launches() == NSTEPS // 4, e.graph_launches()
            mu, om = e.get_params()
            a, b = np.abs(mu - m2).max(), np.abs(om - o2).max()
            msg = f"{rname} [{form}]: {nm}: against the oracle loop |dmu| {a:.3e} |domega| {b:.3e}"
            if kw["elbo_every"]:
                t = np.abs(e.elbo_trace(0, NSTEPS) - tr).max() / np.abs(tr).max()
                msg += f" trace {t:.3e} relative"
            print(msg)
            assert a < TOL and b < TOL, (rname, form, nm, a, b)
            if kw["elbo_every"]:
                assert t <= TRACE_RTOL, (rname, form, nm, t)
            outs.append((mu, om))
    if len(outs) == 2:
        d = max(np.abs(outs[0][0] - outs[1][0]).max(), np.abs(outs[0][1] - outs[1][1]).max())
        print(f"{rname} [{form}]: launch_mode 2 against 1 {d:.3e}")
        assert d < MODES_TOL, (rname, form, d)


# ---------------------------------------------------------------------------------------------------------------------------
# B. the point services under the same priors
# ---------------------------------------------------------------------------------------------------------------------------
B_SHAPES = ("fitness_T6", "multienv_T8", "genotype_odd", "replicate_R3", "multienv_replicate_T6")          # one per kind


@functools.lru_cache(maxsize=None)
def _points(name):
    """Three points -- near the initial parameters, N(0, 1), near the prior means -- and the oracle's log-joint and gradient there."""
    sp = _sp(name, "stress")
    g = np.random.default_rng(8)
    Z = np.stack([g.normal(0.0, 0.3, sp.D), g.normal(0.0, 1.0, sp.D), sp.prior_arrays()[0] + g.normal(0.0, 0.5, sp.D)])
    return Z, [literal.logjoint_and_grad(z, sp) for z in Z]


def case_point_services(lib, name, mode):
    """bb_elbo_grad, bb_logdensity_grad and bb_logdensity_grad_batch under stress priors on a handle created in launch_mode `mode`:
    against the literal oracle at the project's tolerances.  A batch's rows are bit-equal to the same point as a batch of its own (the
    property bb_logdensity_grad_batch documents; bb_logdensity_grad is another kernel and is held to the oracle's tolerances), and the
    handle's parameters are untouched, bitwise."""
    sp = _sp(name, "stress")
    Z, ref = _points(name)
    with make_engine(sp, lib, use_priors=True, seed=SEED, launch_mode=mode, **TRUNC) as e:
        mu0, om0 = e.get_params()
        eps = np.stack([c.rng.normals(5, 1, s_, sp.D) for s_ in range(2)])
        c.check_grad(e, sp, mu0 * 0.3 + 2, om0 * 0.5 - 1, eps)
        lpb, grb = e.logdensity_grad_batch(Z)
        for w in range(3):
            lp2, gr2 = ref[w]
            lp, gr = e.logdensity_grad(Z[w])
            lp1, gr1 = e.logdensity_grad_batch(Z[w])
            assert np.array_equal(lp1[0:1].view(np.uint64), lpb[w:w + 1].view(np.uint64)) and np.array_equal(gr1[0].view(np.uint64), grb[w].view(np.uint64)), w
            for what, l_, g_ in (("single", lp, gr), ("batch", lpb[w], grb[w])):
                el, eg = abs(l_ - lp2) / abs(lp2), np.abs(g_ - gr2).max() / np.abs(gr2).max()
                print(f"point services {name} launch_mode {mode} point {w} {what}: logp rel {el:.3e} grad rel {eg:.3e} worst block {c.block_rel(g_, gr2, sp)}")
                assert el <= 1e-11, (name, mode, w, what, l_, lp2)
                assert eg <= 1e-9, (name, mode, w, what, eg)
        mu1, om1 = e.get_params()
        assert np.array_equal(mu0.view(np.uint64), mu1.view(np.uint64)) and np.array_equal(om0.view(np.uint64), om1.view(np.uint64))


# ---------------------------------------------------------------------------------------------------------------------------
# C. the genotype model as the reference hands it over
# ---------------------------------------------------------------------------------------------------------------------------
def stress(sp):
    return with_priors(sp, 2, "stress")


def case_genotype_regrouped(lib, name, expect_kernel=2):
    """_cases.case_genotype_regrouped with stress priors handed over in the caller's order: bb_create's regrouping permutes the
    logsigma_bc and loglambda priors with the barcodes (and, genotype_odd, moves the loglambda block in front of theta)."""
    c.case_genotype_regrouped(lib, name, priors=stress, expect_kernel=expect_kernel)


def case_genotype_permuted(lib, name="genotype_runs"):
    """An arbitrary permutation of the mutants (a genotype's mutants change their relative order too), stress priors in the caller's
    order: against the oracle on the permuted problem, both launch modes."""
    sp = c.synth(name, seed=6)
    p = np.random.default_rng(5).permutation(sp.n_bc)
    cols = np.concatenate([np.arange(sp.n_neutral), sp.n_neutral + p])
    sp2 = stress(dataclasses.replace(sp, counts=[cn[:, cols] for cn in sp.counts], geno_idx=np.asarray(sp.geno_idx)[p]))
    for mode in (1, 2):
        e, a, b, _ = c._trajectory(lib, sp2, 9, 1, "TruncatedADAGrad", seed=13, use_priors=True, window=WINDOW, resum_every=1, launch_mode=mode,
                                   eta=TRUNC["eta"], tau=TRUNC["tau"])
        k, nm = e.stats()["resident_kernel"], e.kernel_name()
        assert not (e.permutation() == np.arange(sp.D)).all()
        e.close()
        print(f"permuted {name} launch_mode {mode}: {nm}: against the oracle loop |dmu| {a:.3e} |domega| {b:.3e}")
        assert k == (2 if mode == 2 else 0), (k, nm)
        assert a < TOL and b < TOL, (mode, a, b)


# ---------------------------------------------------------------------------------------------------------------------------
# D. shards
# ---------------------------------------------------------------------------------------------------------------------------
def case_sharded_split_phase(lib, name, W=3, S=2, nsteps=5):
    """_cases.case_sharded_split_phase's stepping (bb_step_moments / bb_step_apply, the sum on the caller's side) with stress priors
    and the non-default constants, the gathered parameters against the ORACLE's loop."""
    from barbay_jl_amd.sharding import gather_params
    sp = _sp(name, "stress")
    kw = dict(seed=5, samples_per_step=S, window=WINDOW, resum_every=1, **TRUNC)
    es = [make_engine(sp, lib, use_priors=True, rank=rk, world_size=W, **kw) for rk in range(W)]
    try:
        mu0, om0 = es[0].get_params()
        perm = es[0].permutation()
        lay = {n: (lo, hi) for n, lo, hi in es[0].layout()}
        full0 = [np.stack([e.get_params()[i] for e in es]) for i in (0, 1)]
        assert all((f == f[0]).all() for f in full0)          # every shard starts from the whole initial vector
        for _ in range(nsteps * S):
            tot = sum(e.step_moments() for e in es)
            for e in es:
                e.step_apply(tot)
        own = [e.owned() for e in es]
        st = [e.stats() for e in es]
        mu, om = (gather_params([e.get_params()[i] for e in es], st, sp.kind, lay, sp.n_neutral, sp.n_bc, sp.n_time, sp.n_rep, sp.n_env,
                                owned=own) for i in (0, 1))
    finally:
        for e in es:
            e.close()
    m2, o2, _ = oracle_loop(sp, mu0, om0, perm, nsteps, S, TRUNC, seed=5)
    a, b = np.abs(mu - m2).max(), np.abs(om - o2).max()
    print(f"split-phase {name} W={W} S={S}: against the oracle loop |dmu| {a:.3e} |domega| {b:.3e}")
    assert a < TOL and b < TOL, (a, b)


def case_multi_device(lib, name, ms):
    """One handle, two shards on device 0 (bb_advi_opts.n_devices), stress priors: the cross-GPU instances k_res<.., XG = true, ..>
    read a shard's cut of the prior arrays.  run(5), run(7) against the oracle's loop, the recorded ELBOs where recorded.  Set
    BB_TUNE_NB / BB_TUNE_NTHR first (>= 8 tiles per shard); on a GPU in a process of its own (co-resident launches need a hardware
    queue per shard)."""
    row = dict(kernel=2, prefix="k_res<", ms=ms, ap=None)
    sp = _sp(name, "stress")
    opt, kw = _settings(row)
    with make_engine(sp, lib, use_priors=True, device_ids=[0, 0], **kw) as e:
        nm = check_row_instance(e, row, xg=True)
        mu0, om0 = e.get_params()
        m2, o2, tr = _oracle_cached(name, "stress", kw["samples_per_step"], opt["optimizer"], mu0.tobytes(), om0.tobytes(), e.permutation().tobytes())
        e.run(5)
        e.run(NSTEPS - 5)
        st = e.stats()
        assert st["steps_done"] == NSTEPS and st["resident_kernel"] == 2 and (st["shard_lo"], st["shard_hi"]) == (0, sp.B), st
        mu, om = e.get_params()
        a, b = np.abs(mu - m2).max(), np.abs(om - o2).max()
        msg = f"multi-device {name} ms={ms}: {nm}: against the oracle loop |dmu| {a:.3e} |domega| {b:.3e}"
        if ms:
            t = np.abs(e.elbo_trace(0, NSTEPS) - tr).max() / np.abs(tr).max()
            msg += f" trace {t:.3e} relative"
        print(msg)
        assert a < TOL and b < TOL, (nm, a, b)
        if ms:
            assert t <= TRACE_RTOL, (nm, t)


# ---------------------------------------------------------------------------------------------------------------------------
# E. the BASELINE instances (GPU only: compile-time-T instances at the full-size tile geometry)
# ---------------------------------------------------------------------------------------------------------------------------
def case_baseline_instance(lib, monkeypatch, cfg):
    """A row of _cases.BASELINE_INSTANCES again with naive-form priors (seed of the row's counts irrelevant: the form draws nothing)
    and the non-default TruncatedADAGrad constants."""
    c.case_baseline_instance(lib, monkeypatch, cfg, priors=lambda sp: with_priors(sp, 2, "naive"), eta=TRUNC["eta"], tau=TRUNC["tau"])


# ---------------------------------------------------------------------------------------------------------------------------
# F. constants belong to the handle
# ---------------------------------------------------------------------------------------------------------------------------
def case_constants_per_handle(lib, pname):
    """Two TruncatedADAGrad handles of one shape alive at once, one with (0.037, 3.5), one with the defaults, their run(5), run(7)
    interleaved, and a DecayedADAGrad handle with (0.021, 0.8, 0.65) that is run, re-initialised and run again: each against its own
    oracle loop.  pname: a row of _run_cases.PATHS (set its environment first)."""
    path = r.PATHS[pname]
    sp = _sp(path["shape"])
    kw = dict(seed=SEED, window=WINDOW, resum_every=1, **path["kw"])
    opts = [TRUNC, dict(optimizer="TruncatedADAGrad", eta=0.1, tau=40.0), DECAY]
    es = [make_engine(sp, lib, **kw, **(o if i != 1 else {})) for i, o in enumerate(opts)]          # (the second: the library's own defaults)
    try:
        nm = [r.check_instance(e, path) for e in es]
        mu0, om0 = es[0].get_params()
        perm = es[0].permutation()
        for e in es[1:]:
            m, o = e.get_params()
            assert np.array_equal(m, mu0) and np.array_equal(o, om0)
        es[0].run(5)
        es[2].run(3)
        es[1].run(5)
        es[0].run(7)
        es[2].init_meanfield()
        m, o = es[2].get_params()
        assert np.array_equal(m, mu0) and np.array_equal(o, om0)
        es[2].run(5)
        es[1].run(7)
        es[2].run(7)
        for e, o, n in zip(es, opts, nm):
            assert e.stats()["steps_done"] == NSTEPS
            m2, o2, _ = oracle_loop(sp, mu0, om0, perm, NSTEPS, 1, o)
            mu, om = e.get_params()
            a, b = np.abs(mu - m2).max(), np.abs(om - o2).max()
            print(f"constants {pname}: {n}: {o}: against its own oracle loop |dmu| {a:.3e} |domega| {b:.3e}")
            assert a < TOL and b < TOL, (pname, o, a, b)
    finally:
        for e in es:
            e.close()


# ---------------------------------------------------------------------------------------------------------------------------
# the tests must be able to fail
# ---------------------------------------------------------------------------------------------------------------------------
SENSITIVITY = 1e-7          # 1000 x TOL


def sensitivity(name):
    """{block: max over the block's mu of |trajectory with the block's (mean, std) rolled by one element - trajectory|} over the
    oracle's own 12 steps under stress priors: what a kernel that read a neighbour's prior would be off by."""
    sp = _sp(name, "stress")
    mu0, om0 = advi.meanfield_init(SEED, sp.D)
    perm = np.arange(sp.D)
    base = oracle_loop(sp, mu0, om0, perm, NSTEPS, 1, TRUNC)[0]
    out = {}
    for blk, n, pname in sp.blocks():
        mean, std = sp.priors.get(pname, (0.0, 1.0))
        if np.ndim(mean) == 0:          # (theta_tilde, logtau: no Matrix form)
            continue
        sp2 = dataclasses.replace(sp, priors={**sp.priors, pname: (np.roll(mean, 1), np.roll(std, 1))})
        lo, hi = sp.offsets()[blk]
        out[blk] = float(np.abs(oracle_loop(sp2, mu0, om0, perm, NSTEPS, 1, TRUNC)[0][lo:hi] - base[lo:hi]).max())
    return out
