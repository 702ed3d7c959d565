"""Accuracy at posterior-like points against the committed 50-digit truth (tests/golden/accuracy_<case>.npz, written by
tests/golden/make_accuracy_golden.py from oracle/mp_literal.py), shared by the emulation tests (CPU) and the GPU tests.

Units.  logp: |error| / (u * scale), u = 2^-53, scale = the sum of the absolute values of the log-joint's elementary addends.
Gradient entry i: |error| / (u * G_i), G_i = the sum over the addends of |d addend / d z_i|, maximised PER BLOCK of the layout --
a block whose entries are a millionth of the largest loglambda entry is judged on its own.

Bounds.  The yardstick is the fp64 literal oracle's own error against the same truth in the same units, per case, point and
block (stored in the npz, never taken from the engine's output).  The engine may exceed it by FACTOR = 8: its elementary
functions (bb_math.h) are specified at 1 - 2 ulp against libm's <= 1, its sums run tile by tile in another order, and the fused
Poisson identity adds about one rounding per term.  FLOOR = 4 units keeps a block where the oracle happens to be exact from
making the bound zero (the stored truth is itself rounded to fp64: up to half a unit).

MEASURED with the committed code (profiles/accuracy/units.json, sections "emulation" and "device" = MI355X; 1312 rows each, the sixteen cases
that came with that fix: the even-T cases added since are asserted by the same tests, not tabulated).  No row over
its bound in either; the worst gradient block is at 5.2 times the oracle in both (fitness_zero logsigma-6 s_pop, 22.4 units against 4.3).
logp: at most 1.89 units in the emulation (multienv_d200 logsigma-6, the oracle's own 1.89 there) and 1.91 on the device (fitness_tiny
logsigma-6).  At depth 20 000 the posterior-like points reach 1.26 units (emulation) and 1.23 (device) against the oracle's 0.05
(genotype_d20000 logsigma-2), which is 1.3e-11 of |logp| -- the old relative bound measures the conditioning of the point there, not a
loss in the engine.  Before bb_block.h formed c_t from log(S[t+1] / S[t]) and its moments about a per-step pivot these
tests failed on the population-level blocks, in the emulation and on the device alike (58 and 60 rows over): s_pop 80 .. 350 units against
the oracle's 4 .. 21, logsigma_pop up to 759 against 15, loglambda up to 514 against 23 -- ~1e-13 of the gradient's largest entry, which is
why the max-norm assertions never saw them.

The resident launches (k_res, k_stream; k_persist shares bb_block.h) form their moments and c_t in code of their own, and none of the entry
points above runs them.  Their gradient is read back through ONE optimiser step made linear in it (resident_grad below) and judged in the
same units and bounds, per config of RESIDENT (one tile, several tiles, two samples per step, the streaming launch, launch mode 1 as the
probe's control), at the four points and -- where the handle keeps the caller's latent order -- the ELBO point with its omega gradient.
MEASURED (units.json, "resident_emulation" and "resident_device", "commit": 3508 and 3342 rows, summed up per kernel and model kind): no
asserted row over its bound.
Worst against the oracle, emulation and device alike: genotype_d20000 logsigma-4 s_pop, 119.8 units against 19.4 (6.2x; k_res<2>, several
tiles).  k_stream's omega rows at the ELBO point are printed, not asserted (its default build recovers eps from the kept z): up to 5355
units against 25.9 in the emulation (replicate_T44_d200 loglambda), 4108 against 30.7 on the device (replicate_T66_d200 loglambda).
The parent of the commit that brought these tests ("parent" in the same sections) had 169 rows over in the emulation and
143 on the device, all in k_res / k_stream and none in launch mode 1 or k_persist: s_pop 54 .. 448 units against the oracle's 4 .. 49,
logsigma_pop up to 759 against 15, theta / theta_tilde / logtau of k_res<3> and k_res<4> 133 .. 1781 against 16 .. 184, logsigma_bc up to 1677
against 173, loglambda up to 648 against 81.  On the device the streaming launch has no T = 4 instance for the replicate kinds and no MS
instance at T = 4 beyond the fitness kind (DEVICE_STREAM): replicate_T66_d200 is the device's kind-3 streaming case, replicate_T44_d200 the
emulation's second.
"""
import importlib.util
import json
import os

import numpy as np

import _cases
from conftest import make_engine
from oracle import advi, literal, port, rng
from oracle.spec import ModelSpec

GOLD = os.path.join(os.path.dirname(__file__), "golden")
U = 2.0 ** -53
FACTOR, FLOOR = 8.0, 4.0
SEVERAL_TILES = dict(BB_TUNE_NB="16", BB_TUNE_NTHR="128")
GEOMETRIES = {"tiles16": SEVERAL_TILES, "default": {}}

_spec = importlib.util.spec_from_file_location("make_accuracy_golden", os.path.join(GOLD, "make_accuracy_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)
CASES = list(gen.CASES)

_cache = {}


def load(case):
    """(ModelSpec, npz contents) of a committed case; read once, never written to."""
    if case not in _cache:
        d = dict(np.load(os.path.join(GOLD, f"accuracy_{case}.npz")))
        R = int(d["n_rep"])
        kind = str(d["kind"])
        counts = [d[f"counts{r}"] for r in range(R)]
        kw = {}
        if kind == "multienv":
            kw["env_idx"] = d["env0"]
        if kind == "multienv_replicate":
            kw["env_idx"] = [d[f"env{r}"] for r in range(R)]
        if kind == "genotype":
            kw["geno_idx"] = d["geno_idx"]
        sp = ModelSpec(kind=kind, counts=counts, totals=[c.sum(axis=1) for c in counts], n_neutral=int(d["n_neutral"]),
                       n_bc=int(d["n_bc"]), **kw)
        d["mu"] = d["Z"][1].copy()                                          # the ELBO point's mean and draw are not stored
        d["eps"] = rng.normals(int(d["seed"]), 0, 0, sp.D)
        for v in d.values():
            v.setflags(write=False)
        _cache[case] = (sp, d)
    return _cache[case]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def logp_units(val, truth, scale):
    return float(abs(val - truth) / (U * scale))


def err_units(err, G, off):
    """block -> max_i |err_i| / (u G_i)."""
    e = np.abs(np.asarray(err, dtype=np.float64)) / (U * np.maximum(G.astype(np.float64), 1e-300))
    return {name: float(e[lo:hi].max()) for name, (lo, hi) in off.items()}


def grad_units(val, truth, G, off):
    return err_units(np.asarray(val) - truth, G, off)


def bound(oracle_units):
    return max(FLOOR, FACTOR * oracle_units)


def measure(lib, case):
    """Rows (point, quantity, block, oracle units, engine units, entry point of the engine's worst, global max-norm figure) of one
    case under the geometry the environment sets, and the bit-equality the header promises for the batch service."""
    sp, d = load(case)
    off = sp.offsets()
    kw = dict(ragged_method=True) if bool(d["ragged"]) else {}
    Z, P = d["Z"], len(d["points"])
    om1 = np.full(sp.D, -1.0)
    om6 = np.full(sp.D, float(d["omega"]))
    rows = []

    def add(point, truth_lp, scale, truth_g, G, lit_dlp, lit_dg, got, quantity="grad"):
        """got: [(entry point, logp or None, grad)]; lit_dlp, lit_dg: the literal oracle's stored errors"""
        o_lp = float(abs(lit_dlp) / (U * scale)) if truth_lp is not None else None
        o_g = err_units(lit_dg, G, off)
        if truth_lp is not None:
            worst = max(((logp_units(lp, truth_lp, scale), name) for name, lp, _ in got if lp is not None))
            rows.append(dict(point=point, quantity="logp", block="", oracle=o_lp, engine=worst[0], entry=worst[1],
                             rel=float(max(abs(lp - truth_lp) for _, lp, _ in got if lp is not None) / abs(truth_lp))))
        for blk in off:
            worst = max((grad_units(g, truth_g, G, off)[blk], name) for name, _, g in got)
            rows.append(dict(point=point, quantity=quantity, block=blk, oracle=o_g[blk], engine=worst[0], entry=worst[1],
                             rel=float(max(np.abs(g - truth_g).max() for _, _, g in got) / np.abs(truth_g).max())))

    batches = []
    for mode in (1, 2):
        with make_engine(sp, lib, seed=1, launch_mode=mode, **kw) as e:
            assert [(n, lo, hi) for n, (lo, hi) in off.items()] == e.layout()
            lpB, grB = e.logdensity_grad_batch(Z)
            batches.append((lpB, grB))
            if mode == 2:
                continue
            lpR, grR = e.logdensity_grad_batch(Z[::-1])                      # a point's result does not depend on its slot
            assert same(lpR[::-1], lpB) and same(grR[::-1], grB)
            for k in range(P):
                lp1, gr1 = e.logdensity_grad(Z[k])
                el0, g0, _ = e.elbo_grad(Z[k], om1, np.zeros((1, sp.D)))
                got = [("batch", lpB[k], grB[k]), ("single", lp1, gr1), ("elbo_eps0", el0 - gen.entropy(om1), g0)]
                add(str(d["points"][k]), float(d["logp"][k]), float(d["scale"][k]), d["grad"][k], d["G"][k], float(d["lit_dlogp"][k]),
                    d["lit_dgrad"][k], got)
            el, gm, go = e.elbo_grad(d["mu"], om6, d["eps"][None, :])
            add("elbo_eps", float(d["e_logp"]), float(d["e_scale"]), d["e_grad"], d["e_G"], float(d["e_lit_dlogp"]), d["e_lit_dgmu"],
                [("elbo_eps", el - gen.entropy(om6), gm)])
            add("elbo_eps", None, None, d["e_gom"], d["e_Gom"], None, d["e_lit_dgom"], [("elbo_eps", None, go)], quantity="grad_omega")
    assert same(batches[0][0], batches[1][0]) and same(batches[0][1], batches[1][1])          # launch modes 1 and 2: the same bits
    return rows


def failures(case, rows):
    return [f"{case} {r['point']} {r['quantity']} {r['block']}: engine {r['engine']:.1f} units ({r['entry']}) > bound "
            f"{bound(r['oracle']):.1f} (oracle {r['oracle']:.2f})" for r in rows if not r["engine"] <= bound(r["oracle"])]


def case_accuracy(lib, case):
    rows = measure(lib, case)
    for r in rows:
        print(f"{case:28s} {r['point']:11s} {r['quantity']:10s} {r['block']:13s} oracle {r['oracle']:9.2f}  engine {r['engine']:9.2f}  "
              f"bound {bound(r['oracle']):9.2f}  ({r['entry']}; max-norm figure {r['rel']:.2e})")
    bad = failures(case, rows)
    assert not bad, "\n".join(bad)


def case_transcription(case):
    """mp_literal against the fp64 literal oracle at the control point (index 3): <= 1e-13 of the scale -- a guard on the transcription,
    three orders above fp64 rounding (the stored figures: logp ~ 1e-16 of the scale, gradient below 1e-15 of G)."""
    sp, d = load(case)
    k = list(d["points"]).index("control")
    assert abs(float(d["lit_dlogp"][k])) <= 1e-13 * float(d["scale"][k])
    assert (np.abs(d["lit_dgrad"][k].astype(np.float64)) <= 1e-13 * d["G"][k].astype(np.float64)).all()


def case_mp_literal_runs(case):
    """mp_literal itself, run now: its log-joint at the stored control point is the stored truth (to the fp64 rounding of that value) and
    the literal oracle, run now, is within 1e-13 of the scale of it -- so an edit to either transcription of this model kind shows here
    and not only when someone regenerates the fixtures."""
    from oracle import mp_literal
    sp, d = load(case)
    k = list(d["points"]).index("control")
    kw = dict(ragged_quirk=True) if bool(d["ragged"]) else {}
    mp_literal.clear_cache()
    lp, sc = mp_literal.logjoint(d["Z"][k], sp, **kw)
    mp_literal.clear_cache()
    assert float(lp) == float(d["logp"][k]) and float(sc) == float(d["scale"][k])
    assert abs(float(literal.logjoint(np.array(d["Z"][k]), sp, **kw)) - float(lp)) <= 1e-13 * float(sc)


# ---- the gradient inside the resident launches (k_res, k_stream, k_persist), read back through one optimiser step ----------------------
# TruncatedADAGrad moves a latent by eta g / (tau + sqrt(sum of the window's g^2)).  With tau = 2^100 the denominator is tau exactly for
# any |g| < 2^46 (half an ulp of 2^100 is 2^47), with eta = 2^140 the step is mu <- mu + 2^40 g: a power of two times the gradient the
# kernel formed, rounded once into mu.  omega = -60 puts the draw on z = mu to the last bit (softplus(-60) = 9e-27; a zero entry lands
# 1e-25 away), so g is the log-joint's gradient at Z[k].  Read back as (mu_new - mu) / 2^40 in long double the probe's own rounding is at
# most u (|mu| 2^-40 + |g|) (one rounding of mu_new), below one of the suite's units.
PROBE_ETA, PROBE_TAU, PROBE_GAIN, PROBE_OMEGA = 2.0 ** 140, 2.0 ** 100, 2.0 ** 40, -60.0
STREAM = dict(BB_TUNE_STREAM="1", BB_TUNE_NB="350", BB_TUNE_NTHR="1024")
RESIDENT = {            # config -> (samples per step, BB_TUNE_* environment, launch mode)
    "default": ((1,), {}, 2),
    "tiles16": ((1,), SEVERAL_TILES, 2),              # several tiles: the exchange carries the moments
    "S2": ((2,), {}, 2),                              # the MS instances: both samples sit at z = mu, their mean is the gradient
    "stream": ((1, 2), STREAM, 2),                    # only where every replicate has the same even T
    "mode1": ((1,), {}, 1),                           # the probe's control: the two-kernel step, measured by case_accuracy already
}
KIND_NO = {"fitness": 0, "multienv": 1, "genotype": 2, "replicate": 3, "multienv_replicate": 4}


# k_stream instances of the device library with T <= 6, (kind, T) -> samples per step it serves (bb_inst_stream.hip, bb_inst_stream_ms.hip:
# the MS form exists for T = 4 in the fitness kind only, the replicate kinds start at T = 6).  The emulation instantiates the template for
# whatever shape comes.
DEVICE_STREAM = {(0, 4): (1, 2), (1, 4): (1,), (2, 4): (1,), (0, 6): (1, 2), (1, 6): (1, 2), (2, 6): (1, 2), (3, 6): (1, 2), (4, 6): (1, 2)}


def resident_samples(case, config, device):
    """Samples per step a (case, config) runs with; () where the config does not apply to the case."""
    sp, d = load(case)
    Ss = RESIDENT[config][0]
    if config == "stream":           # every replicate the same even T
        T = {c.shape[0] for c in sp.counts}
        if len(T) != 1 or min(T) % 2:
            return ()
        return DEVICE_STREAM.get((KIND_NO[sp.kind], min(T)), ()) if device else Ss
    if config == "S2" and bool(d["ragged"]):          # (bb_create refuses launch mode 2 with several samples under the ragged method)
        return ()
    return Ss


def resident_cases(device=False):
    """(case, config) pairs of the resident accuracy tests; fitness_tiny is the regeneration fixture, too small for several tiles."""
    return [(c, g) for c in CASES if c != "fitness_tiny" for g in RESIDENT if resident_samples(c, g, device)]


def resident_kernel(case, config, S):
    """The kernel_name() prefix ('emu:' stripped) a (case, config, S) launch is meant to reach.  The resident launch of the second
    generation takes 2 <= T <= 16 without the ragged method; with one sample per step its plain instances need even T (odd T and the
    ragged method keep k_persist), the MS instances (S > 1) take any parity."""
    sp, d = load(case)
    K = KIND_NO[sp.kind]
    if RESIDENT[config][2] == 1:
        return "k_sample"                                  # ("k_sample + k_update", on the device with the kind: "k_sample<0> + k_update<0>")
    if config == "stream":
        return f"k_stream<{K},"
    odd = any(c.shape[0] % 2 for c in sp.counts)
    if bool(d["ragged"]) or (odd and S == 1):
        return f"k_persist<{K},"
    return f"k_res<{K},"


def _probe_step(lib, case, mu, omega, S, env, mode, seed):
    """One step of a handle whose optimiser is linear in the gradient: (mu_new, omega_new, kernel name, bb_get_permutation)."""
    sp, d = load(case)
    kw = dict(ragged_method=True) if bool(d["ragged"]) else {}
    old = {k: os.environ.get(k) for k in ("BB_TUNE_NB", "BB_TUNE_NTHR", "BB_TUNE_STREAM")}
    try:
        for k in old:                                       # (the switches are read when the handle is created)
            os.environ.pop(k, None)
        os.environ.update(env)
        with make_engine(sp, lib, seed=seed, samples_per_step=S, eta=PROBE_ETA, tau=PROBE_TAU, window=4, resum_every=1,
                         launch_mode=mode, **kw) as e:
            e.set_params(mu, omega)
            e.run(1)
            m1, o1 = e.get_params()
            return m1, o1, e.kernel_name(), e.permutation()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _probe_read(new, old):
    return (new.astype(np.longdouble) - old.astype(np.longdouble)) / np.longdouble(PROBE_GAIN)


def resident_grad(lib, case, k, S, env, mode=2):
    """(g, kernel name): the gradient of the log-joint at Z[k] as the launch's own G pass formed it."""
    _, d = load(case)
    mu = d["Z"][k]
    m1, _, kn, _ = _probe_step(lib, case, mu, np.full(mu.shape[0], PROBE_OMEGA), S, env, mode, seed=1)
    return _probe_read(m1, mu), kn


def resident_elbo_grads(lib, case, env, mode=2):
    """(g_mu, g_omega, kernel name) at the ELBO point (mu, omega = -6, the handle's own first draw with seed = d["seed"]), or None where
    the handle's internal latent order is not the caller's: the stored truth was taken at the caller-order draw."""
    sp, d = load(case)
    om = np.full(sp.D, float(d["omega"]))
    m1, o1, kn, perm = _probe_step(lib, case, d["mu"], om, 1, env, mode, seed=int(d["seed"]))
    if not np.array_equal(perm, np.arange(sp.D)):
        return None
    return _probe_read(m1, d["mu"]), _probe_read(o1, om), kn


def resident_measure(lib, case, config, device=False):
    """Rows (point, quantity, block, S, oracle units, engine units, kernel, asserted) of one case under one config."""
    sp, d = load(case)
    off = sp.offsets()
    _, env, mode = RESIDENT[config]
    Ss = resident_samples(case, config, device)
    rows = []

    def add(point, quantity, S, g, truth, G, lit_d, kn, asserted=True):
        o, e = err_units(lit_d, G, off), err_units(g - truth.astype(np.longdouble), G, off)
        for blk in off:
            rows.append(dict(point=point, quantity=quantity, block=blk, S=S, oracle=o[blk], engine=e[blk], kernel=kn, asserted=asserted))

    for S in Ss:
        want = resident_kernel(case, config, S)
        for k, point in enumerate(d["points"]):
            g, kn = resident_grad(lib, case, k, S, env, mode)
            assert kn.replace("emu:", "").startswith(want), (case, config, S, kn, want)
            add(str(point), "grad", S, g, d["grad"][k], d["G"][k], d["lit_dgrad"][k], kn)
    if 1 in Ss:
        got = resident_elbo_grads(lib, case, env, mode)
        if got is None:
            print(f"{case} {config}: the ELBO point is left out (the handle regrouped the latents)")
        else:
            gm, go, kn = got
            assert kn.replace("emu:", "").startswith(resident_kernel(case, config, 1)), (case, config, kn)
            add("elbo_eps", "grad", 1, gm, d["e_grad"], d["e_G"], d["e_lit_dgmu"], kn)
            # (k_stream's default build recovers eps from the kept z, BS_ZKEEP: its omega rows are printed, that tolerance is documented apart)
            add("elbo_eps", "grad_omega", 1, go, d["e_gom"], d["e_Gom"], d["e_lit_dgom"], kn, asserted=config != "stream")
    return rows


def resident_failures(case, config, rows):
    return [f"{case} {config} S={r['S']} {r['point']} {r['quantity']} {r['block']}: {r['kernel']} {r['engine']:.1f} units > bound "
            f"{bound(r['oracle']):.1f} (oracle {r['oracle']:.2f})" for r in rows if r["asserted"] and not r["engine"] <= bound(r["oracle"])]


def case_resident_accuracy(lib, case, config, device=False):
    rows = resident_measure(lib, case, config, device)
    for r in rows:
        print(f"{case:28s} {config:8s} S={r['S']} {r['point']:11s} {r['quantity']:10s} {r['block']:13s} oracle {r['oracle']:9.2f}  engine "
              f"{r['engine']:9.2f}  bound {bound(r['oracle']):9.2f}  {r['kernel']}" + ("" if r["asserted"] else "  (printed only)"))
    bad = resident_failures(case, config, rows)
    assert not bad, "\n".join(bad)
    return rows


def case_probe_selfcheck(lib, case):
    """The probe against bb_elbo_grad at the same point and the handle's own draw, launch mode 1 (the same block programs): entry by
    entry within the probe's rounding, u (3 |g_i| + |mu_i| 2^-40) -- so a change to bb_opt_apply cannot turn the probe into something else."""
    sp, d = load(case)
    om = np.full(sp.D, PROBE_OMEGA)
    for k in range(len(d["points"])):
        g, kn = resident_grad(lib, case, k, 1, {}, mode=1)
        assert kn.replace("emu:", "").startswith("k_sample"), kn
        with make_engine(sp, lib, seed=1, launch_mode=1) as e:
            _, gm, _ = e.elbo_grad(d["Z"][k], om, _cases.caller_normals(e, 1, 0, 0, sp.D)[None, :])
        allow = U * (3.0 * np.abs(gm) + np.abs(d["Z"][k]) / PROBE_GAIN)
        worst = float(np.max(np.abs((g - gm.astype(np.longdouble)).astype(np.float64)) / np.maximum(allow, 1e-300)))
        print(f"{case} {d['points'][k]}: probe against bb_elbo_grad, worst entry at {worst:.3f} of its allowance")
        assert worst <= 1.0, (case, k, worst)


# ---- optimiser trajectories from a posterior-like start ------------------------------------------------------------------------------
TRAJ_STEPS, TRAJ_WINDOW, TRAJ_OMEGA, TRAJ_SEED = 12, 5, -5.0, 17
TRAJ = {                # name -> (shape of _cases.SYNTH, BB_TUNE_* environment, kernel_name() prefix in launch mode 2)
    "fitness_T6": ("fitness_T6", {}, "k_res<"),
    "genotype_runs": ("genotype_runs", {}, "k_res<"),
    "replicate_R3": ("replicate_R3", {}, "k_res<"),
    "replicate_ragged": ("replicate_ragged", {}, {1: "k_persist<", 2: "k_res<"}),      # (several samples per step: the library takes k_res's MS instance)
    "fitness_T6_stream": ("fitness_T6", dict(BB_TUNE_NB="350", BB_TUNE_NTHR="1024", BB_TUNE_STREAM="1"), "k_stream<"),
}
YARDSTICKS = os.path.join(GOLD, "accuracy_trajectories.json")


def traj_start(name):
    sp = _cases.synth(TRAJ[name][0], seed=2)
    mu = gen.posterior_like(sp, 77)[1]                     # logsigma = -4
    return sp, mu, np.full(sp.D, TRAJ_OMEGA)


def traj_run(lib, name, S, mode):
    """12 exact-window steps of the engine from the posterior-like start; (mu, omega, kernel name, the draws in the caller's order)."""
    sp, mu0, om0 = traj_start(name)
    with make_engine(sp, lib, seed=TRAJ_SEED, samples_per_step=S, window=TRAJ_WINDOW, resum_every=1, launch_mode=mode) as e:
        e.set_params(mu0, om0)
        e.run(TRAJ_STEPS)
        mu, om = e.get_params()
        eps = [np.stack([_cases.caller_normals(e, TRAJ_SEED, i, s, sp.D) for s in range(S)]) for i in range(TRAJ_STEPS)]
        return mu, om, e.kernel_name(), eps


def traj_oracle(name, S, eps, which="literal"):
    sp, mu0, om0 = traj_start(name)
    if which == "literal":
        f = lambda m, o, ee: literal.elbo_and_grad(m, o, ee, sp)
    else:
        p = port.Port(sp)
        f = lambda m, o, ee: p.elbo_grad(m, o, ee)
    m, o, _ = advi.run_advi(sp, f, mu0, om0, TRAJ_STEPS, S, advi.TruncatedADAGrad(n=TRAJ_WINDOW), TRAJ_SEED, eps_fn=lambda i: eps[i])
    return m, o


def traj_yardstick(name, S):
    with open(YARDSTICKS) as f:
        y = json.load(f)[f"{name}_S{S}"]
    return max(y["dmu"], y["domega"])


def case_trajectory(lib, name, S):
    """Launch modes 1 and 2 against the literal oracle's loop: within 8x of what two CPU loops of different algebra (the literal
    oracle and the C port) differ by from the same start -- the committed yardstick -- and not below the suite's 1e-10; the two modes
    within 1e-11 of each other."""
    tol = max(1e-10, FACTOR * traj_yardstick(name, S))
    outs = []
    for mode in (1, 2):
        mu, om, kn, eps = traj_run(lib, name, S, mode)
        if mode == 2:
            want = TRAJ[name][2]
            assert kn.replace("emu:", "").startswith(want[S] if isinstance(want, dict) else want), kn
        outs.append((mu, om))
    m2, o2 = traj_oracle(name, S, eps)
    for mode, (mu, om) in zip((1, 2), outs):
        a, b = np.abs(mu - m2).max(), np.abs(om - o2).max()
        print(f"{name} S={S} mode {mode}: max|dmu| {a:.3e} max|domega| {b:.3e} (tolerance {tol:.3e})")
        assert a <= tol and b <= tol, (mode, a, b, tol)
    assert np.abs(outs[0][0] - outs[1][0]).max() < 1e-11 and np.abs(outs[0][1] - outs[1][1]).max() < 1e-11
