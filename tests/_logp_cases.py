"""Cases of bb_logdensity_grad_batch (barbay.jl_amd/csrc/bb_logp.h) shared by the emulation tests (CPU) and the GPU tests: each
takes the loaded C-ABI library.  Shapes come from `_cases.SYNTH`, the smallest that reach each branch."""
import ctypes
import os

import numpy as np
import pandas as pd

import _cases
import barbay_jl_amd as bb
from barbay_jl_amd import _capi
from conftest import make_engine
from oracle import literal

# one tile with T = 2; odd T over several tiles (the tile-order sum); multienv with T = 7; ragged replicates; both hierarchies;
# scattered genotypes (the caller-order <-> internal-order permutation)
NAMES = ["fitness_T2", "fitness_multi_tile", "multienv", "replicate_ragged", "multienv_replicate", "genotype"]
MAXB = _capi.BB_LOGP_MAX_BATCH
GOLD = os.path.join(os.path.dirname(__file__), "golden")

_cache = {}


def spec(name):
    if name not in _cache:
        sp = _cases.synth(name, seed=6)
        g = np.random.default_rng(8)
        Z = np.stack([g.normal(0.0, s, sp.D) for s in (0.3, 1.0, 0.3)])      # drawn as in _cases.case_logdensity
        Z.setflags(write=False)
        ref = [literal.logjoint_and_grad(z, sp) for z in Z]
        _cache[name] = (sp, Z, ref)
    return _cache[name]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def case_oracle(lib, name):
    """W = 3 points against the literal oracle and against the single-point service, point by point, at the tolerances the
    project holds bb_logdensity_grad to."""
    sp, Z, ref = spec(name)
    with make_engine(sp, lib, seed=1) as e:
        lp, gr = e.logdensity_grad_batch(Z)
        assert lp.shape == (3,) and gr.shape == (3, sp.D)
        for w in range(3):
            lp2, gr2 = ref[w]
            print(name, w, "logp rel", abs(lp[w] - lp2) / abs(lp2), "grad rel", np.abs(gr[w] - gr2).max() / np.abs(gr2).max(),
                  "worst block", _cases.block_rel(gr[w], gr2, sp))
            assert abs(lp[w] - lp2) <= 1e-11 * abs(lp2), (lp[w], lp2)
            assert np.abs(gr[w] - gr2).max() <= 1e-9 * np.abs(gr2).max()
            lp1, gr1 = e.logdensity_grad(Z[w])
            assert abs(lp[w] - lp1) <= 1e-11 * abs(lp2), (lp[w], lp1)
            assert np.abs(gr[w] - gr1).max() <= 1e-9 * np.abs(gr2).max()
        lp1, gr1 = e.logdensity_grad_batch(Z[1])                              # [D] is a batch of one
        assert lp1.shape == (1,) and gr1.shape == (1, sp.D) and same(lp1[0], lp[1]) and same(gr1[0], gr[1])


def case_independence(lib, name):
    """A point's result is a function of the point alone, bit for bit: slot, batch size, batch order, a non-finite neighbour,
    the handle's launch mode."""
    sp, Z, _ = spec(name)
    g = np.random.default_rng(21)
    others = g.normal(0.0, 0.5, (4, sp.D))
    with make_engine(sp, lib, seed=1) as e:
        lp1, gr1 = e.logdensity_grad_batch(Z[0])
        assert np.isfinite(lp1[0]) and np.isfinite(gr1).all()
        for slot in (0, 2, 4):                                                # first, middle and last slot of W = 5
            batch = np.insert(others, slot, Z[0], axis=0)
            lp, gr = e.logdensity_grad_batch(batch)
            assert same(lp[slot], lp1[0]) and same(gr[slot], gr1[0]), slot
        batch = np.concatenate([Z, others])
        lp, gr = e.logdensity_grad_batch(batch)
        lpr, grr = e.logdensity_grad_batch(batch[::-1])
        assert same(lpr[::-1], lp) and same(grr[::-1], gr)                    # reversing the batch reverses the results
        bad = batch.copy()
        bad[3, sp.D // 2] = 1e308                                             # one point whose log-joint is not finite
        lpb, grb = e.logdensity_grad_batch(bad)
        assert not np.isfinite(lpb[3])
        keep = [w for w in range(len(batch)) if w != 3]
        assert same(lpb[keep], lp[keep]) and same(grb[keep], gr[keep])
    with make_engine(sp, lib, seed=1, launch_mode=1) as e:                    # two-kernel handle against the default mode
        lpm, grm = e.logdensity_grad_batch(batch)
        assert same(lpm, lp) and same(grm, gr)


def case_full_batch(lib, name="fitness_multi_tile"):
    """One call with W = BB_LOGP_MAX_BATCH points: every slot equals its point's result at W = 1 or 3."""
    sp, Z, _ = spec(name)
    g = np.random.default_rng(33)
    batch = g.normal(0.0, 0.4, (MAXB, sp.D))
    batch[[0, MAXB // 2, MAXB - 1]] = Z
    with make_engine(sp, lib, seed=1) as e:
        lp, gr = e.logdensity_grad_batch(batch)
        assert np.isfinite(lp).all() and np.isfinite(gr).all()
        lp3, gr3 = e.logdensity_grad_batch(Z)
        assert same(lp[[0, MAXB // 2, MAXB - 1]], lp3) and same(gr[[0, MAXB // 2, MAXB - 1]], gr3)
        lp1, gr1 = e.logdensity_grad_batch(batch[17])
        assert same(lp[17], lp1[0]) and same(gr[17], gr1[0])


def case_state_untouched(lib, name):
    """mu and omega are bitwise what they were; run(5) after a batch call equals run(5) on a fresh handle."""
    sp, Z, _ = spec(name)
    with make_engine(sp, lib, seed=1) as e:
        mu0, om0 = e.get_params()
        e.logdensity_grad_batch(Z)
        mu1, om1 = e.get_params()
        assert same(mu0, mu1) and same(om0, om1)
        e.run(5)
        mu_a, om_a = e.get_params()
    with make_engine(sp, lib, seed=1) as e:
        e.run(5)
        mu_b, om_b = e.get_params()
    assert same(mu_a, mu_b) and same(om_a, om_b)


def case_errors(lib):
    sp, Z, _ = spec("fitness_T2")
    dp = ctypes.POINTER(ctypes.c_double)
    with make_engine(sp, lib, seed=1) as e:
        z = np.zeros((MAXB + 1, sp.D))
        lp = np.zeros(MAXB + 1)
        gr = np.zeros((MAXB + 1, sp.D))
        call = lambda W, zz=z: lib.bb_logdensity_grad_batch(e._h, W, zz.ctypes.data_as(dp) if zz is not None else None,
                                                            lp.ctypes.data_as(dp), gr.ctypes.data_as(dp))
        assert call(0) == -1 and call(MAXB + 1) == -1 and call(-3) == -1      # BB_ERR_INVALID
        assert call(2, None) == -1
        assert lib.bb_logdensity_grad_batch(None, 1, z.ctypes.data_as(dp), lp.ctypes.data_as(dp), gr.ctypes.data_as(dp)) == -1
        assert call(MAXB) == 0
        assert lib.bb_logdensity_grad_batch(e._h, 2, z.ctypes.data_as(dp), None, None) == 0      # both outputs may be NULL
    with make_engine(sp, lib, seed=1, world_size=2, rank=0) as e:
        with __import__("pytest").raises(_capi.BarBayHipError, match="error -4"):      # BB_ERR_UNSUPPORTED
            e.logdensity_grad_batch(Z)


# ---- end to end: mcmc_sample on the reference's single-condition fixture -------------------------------------------------------
MCMC_KW = dict(n_walkers=3, n_steps=20, n_adapt=10, advi_steps=200, outputname=None, verbose=False, seed=3)


def load(name):
    return pd.read_csv(os.path.join(GOLD, name + ".csv"))


def case_mcmc_batched(lib):
    """ensemble="batched": shapes, finite log-densities, and walker 1 equal to a single `nuts` run on the batch service at
    W = 1 with the same generator and start."""
    df = load("data001_single")
    out = bb.mcmc.mcmc_sample(data=df, model=bb.model.fitness_normal, ensemble="batched", engine_kwargs={"_lib": lib}, **MCMC_KW)
    arr = bb.utils.data_to_arrays(df)
    D = 2 * (arr.bc_count.shape[0] - 1) + 2 * arr.n_bc + arr.bc_count.size
    assert out["chain"].shape == (3, 20, D) and out["logp"].shape == (3, 20) and out["step_size"].shape == (3,)
    assert np.isfinite(out["logp"]).all() and len(out["var_names"]) == D
    model = bb.model.fitness_normal(arr.bc_count, arr.bc_total, arr.n_neutral, arr.n_bc)
    with bb.vi.make_engine(model, bb.vi.ADVI(1, 200), bb.vi.TruncatedADAGrad(), 3, 0, _lib=lib) as e:
        e.run(200)
        mean, sigma = e.posterior()
        minv = sigma ** 2
        r = np.random.default_rng([3, 1])
        z0 = mean + np.sqrt(minv) * r.standard_normal(D) * 0.1

        def f(z):
            lp, g = e.logdensity_grad_batch(z)
            return float(lp[0]), g[0]
        c, lp, info = bb.mcmc.nuts(f, z0, 20, 10, minv=minv, rng=r)
    assert same(c, out["chain"][1]) and same(lp, out["logp"][1]) and same(info["step_size"], out["step_size"][1])
    return out
