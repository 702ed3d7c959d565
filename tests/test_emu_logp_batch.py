"""bb_logdensity_grad_batch (barbay.jl_amd/csrc/bb_logp.h) in the host emulation of the block programs, the ensemble NUTS driver
on a known Gaussian (no engine), and mcmc_sample(ensemble=...) end to end on the emulation (tests/_logp_cases.py)."""
import hashlib

import numpy as np
import pytest

import _logp_cases as lc
import barbay_jl_amd as bb


@pytest.mark.parametrize("name", lc.NAMES)
def test_batch_matches_oracle_and_single_call(emu_lib, name):
    lc.case_oracle(emu_lib, name)


@pytest.mark.parametrize("name", lc.NAMES)
def test_batch_points_are_independent_bitwise(emu_lib, name):
    lc.case_independence(emu_lib, name)


@pytest.mark.parametrize("name", lc.NAMES)
def test_batch_leaves_state_untouched(emu_lib, name):
    lc.case_state_untouched(emu_lib, name)


def test_batch_errors(emu_lib):
    lc.case_errors(emu_lib)


# ---- the ensemble driver, no engine ----------------------------------------------------------------------------------------------
VAR = np.array([1.0, 4.0, 0.25] * 3)


def _f(z):
    return -0.5 * float(np.sum(z * z / VAR)), -z / VAR


def _fbatch(Z):
    return np.array([_f(z)[0] for z in Z]), np.stack([_f(z)[1] for z in Z])


def _starts(seed, W):
    return [np.random.default_rng([seed, 100 + w]).standard_normal(VAR.shape[0]) for w in range(W)]


def test_ensemble_equals_single_chains_bitwise():
    seed, W = 5, 4
    z0s = _starts(seed, W)
    sizes = []

    def counting(Z):
        sizes.append(len(Z))
        return _fbatch(Z)
    res = bb.mcmc.nuts_ensemble(counting, z0s, 30, 20, rngs=[np.random.default_rng([seed, w]) for w in range(W)])
    assert len(res) == W and sizes[0] == W and sizes[-1] < W          # walkers drop out as they finish: the batch shrinks
    assert all(a >= b for a, b in zip(sizes, sizes[1:]))
    for w in range(W):
        c, lp, info = bb.mcmc.nuts(_f, z0s[w], 30, 20, rng=np.random.default_rng([seed, w]))
        assert c.shape == (30, VAR.shape[0])
        assert lc.same(res[w][0], c) and lc.same(res[w][1], lp) and lc.same(res[w][2]["step_size"], info["step_size"])
        assert res[w][2] == info


def test_ensemble_early_finisher_does_not_disturb_the_others():
    seed, W = 5, 4
    z0s = _starts(seed, W)
    rngs = lambda: [np.random.default_rng([seed, w]) for w in range(W)]
    full = bb.mcmc.nuts_ensemble(_fbatch, z0s, 30, 20, rngs=rngs())

    def short_second(fbatch, z0s, n_steps, n_adapt, **kw):            # walker 1 asks for 4 draws only
        return bb.mcmc.nuts_ensemble(fbatch, z0s, [n_steps, 4, n_steps, n_steps], n_adapt, **kw)
    part = short_second(_fbatch, z0s, 30, 20, rngs=rngs())
    assert part[1][0].shape == (4, VAR.shape[0]) and lc.same(part[1][0], full[1][0][:4])
    for w in (0, 2, 3):
        assert lc.same(part[w][0], full[w][0]) and lc.same(part[w][1], full[w][1]) and part[w][2] == full[w][2]


def test_ensemble_argument_errors():
    with pytest.raises(bb.BarBayError, match="one random generator per walker"):
        bb.mcmc.nuts_ensemble(_fbatch, _starts(1, 2), 3, 2, rngs=[np.random.default_rng(0)])
    with pytest.raises(bb.BarBayError, match="ensemble must be"):
        bb.mcmc.mcmc_sample(data=lc.load("data001_single"), n_walkers=1, n_steps=2, outputname=None,
                            model=bb.model.fitness_normal, ensemble="threads")


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def test_mcmc_batched_emulated(emu_lib):
    lc.case_mcmc_batched(emu_lib)


# sha256 over chain, logp and step_size (float64, C order) of mcmc_sample(**MCMC_KW) on the emulation, recorded from the commit
# before `ensemble` existed ("8db3d6c5..."), and recorded again when bb_logdensity_grad's arithmetic changed on purpose: c_t from the log of
# the totals' ratio and the moments about a per-step pivot move the last bits of every gradient, hence of the chain
SERIAL_SHA256 = "949fb6111d28a48425e187501c3b477006257ee30ececd772d09b76743750a45"


def test_mcmc_serial_is_what_it_was(emu_lib):
    out = bb.mcmc.mcmc_sample(data=lc.load("data001_single"), model=bb.model.fitness_normal, ensemble="serial",
                              engine_kwargs={"_lib": emu_lib}, **lc.MCMC_KW)
    h = hashlib.sha256()
    for k in ("chain", "logp", "step_size"):
        h.update(np.ascontiguousarray(out[k], dtype=np.float64).tobytes())
    assert out["chain"].shape[:2] == (3, 20) and h.hexdigest() == SERIAL_SHA256
