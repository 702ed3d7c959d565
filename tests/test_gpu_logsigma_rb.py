"""bb_logsigma_rb (Rao-Blackwellised noise-scale marginals, barbay.jl_amd/csrc/bb_lsrb.h) on the device: the emulation's cases and
the goldens the emulation is too slow for, the identity also against the device's own gradient, a statistical check against
independent numpy draws, and the user entry point end to end."""
import os

import numpy as np
import pandas as pd
import pytest

import _ppc_cases as pc
import _logsigma_rb_cases as lc

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("name", sorted(lc.golden_cases()))
def test_marginals_match_golden(hip_lib, name):
    lc.check_golden(hip_lib, name, "device")


@pytest.mark.parametrize("name", lc.IDENTITY)
def test_gradient_of_the_log_joint_vanishes_at_the_modes(hip_lib, name):
    lc.check_identity(hip_lib, name, device=True)


def test_prior_only_entries(hip_lib):
    lc.check_prior_only(hip_lib)


def test_independent_of_launch_mode_and_repeatable(hip_lib):
    lc.check_launch_modes(hip_lib)


@pytest.mark.parametrize("name", lc.GROUP_CASES)
def test_group_handle_equals_single_device(hip_lib, name):
    lc.check_group_handle(hip_lib, name)


def test_buffer_reuse_across_calls_sizes_and_blocks(hip_lib):
    lc.check_buffer_reuse(hip_lib)


def test_handle_untouched(hip_lib):
    lc.check_handle_untouched(hip_lib)


@pytest.mark.parametrize("name", ["genotype_matrix_prior", "multienv_replicate", "replicate_ragged_method"])
def test_own_draws_equal_the_same_draws_passed_in(hip_lib, name):
    lc.check_internal_against_explicit_draws(hip_lib, name)


def test_nan_stays_in_its_entries(hip_lib):
    lc.check_nan_stays(hip_lib)


def test_four_and_eight_quantiles(hip_lib):
    lc.check_more_quantiles(hip_lib, "device")


def test_logsigma_rb_errors(hip_lib):
    lc.check_errors(hip_lib)


@pytest.mark.parametrize("block,entry", [("bc", 3), ("pop", 1)])
def test_marginal_against_a_large_numpy_sample(hip_lib, block, entry):
    """One entry's rb_mean, rb_sd^2 and sigma_mean at n_samples = BB_LOGSIGMA_RB_MAX_SAMPLES against 200 000 independent numpy draws
    of the posterior pushed through the numpy restatement, each within 6 Monte-Carlo standard errors of the two estimates together."""
    sp, mu, om = lc.inputs(lc.TINY)
    n, N = 200_000, lc.MAXN
    with pc._handle(hip_lib, sp, mu, om) as e:
        mean, sigma = e.posterior()
        got = lc.lrb(e, block, N, seed=17, probs=())

    def draw(i):                                                    # latent i's draws: its own stream, the same whenever it is asked for
        return np.random.default_rng([0, int(i)]).normal(mean[i], sigma[i], n)

    l, SS, nt, a, ib2 = lc.cond_inputs(sp, draw, n, block, entries=[entry])[entry]
    _, E, V, S = lc.Cond(SS, nt, a, ib2).moments()
    v = V + (E - E.mean()) ** 2                                     # per-draw terms of rb_sd^2 (the centring's own error is of second order)
    for name, dev, x in (("rb_mean", got["rb_mean"][entry], E), ("rb_sd^2", got["rb_sd"][entry] ** 2, v), ("sigma_mean", got["sigma_mean"][entry], S)):
        se = np.sqrt(x.var() / n + x.var() / N)
        print(block, name, dev, "numpy", x.mean(), "se", se)
        assert abs(dev - x.mean()) < 6 * se, name


def _check_frame(out, blk, probs=("q2.5", "q50", "q97.5")):
    labels = [c for c in blk.columns if c not in ("mean", "std")]
    tail = ["n_terms", "q_mean", "q_sd", "rb_mean", "rb_sd", "sd_ratio", "mode_mean", "sigma_mean"] + list(probs) + ["sigma_" + p for p in probs]
    assert list(out.columns) == labels + tail and len(out) == len(blk) > 0
    for c in labels:                                                # the rows and labels of the frame's own rows, in their order
        assert list(out[c]) == list(blk[c]), c
    assert np.isfinite(out[tail].to_numpy(dtype=np.float64)).all()
    assert (out["rb_sd"] > 0).all() and (out["q_sd"] > 0).all() and (out["n_terms"] > 0).all()
    for p in probs:
        assert np.array_equal(out["sigma_" + p].to_numpy(), np.exp(out[p].to_numpy()))
    q = out[list(probs)].to_numpy()
    assert (np.diff(q, axis=1) > 0).all() and (out["sigma_mean"] > 0).all()
    print("sd_ratio: median", out["sd_ratio"].median(), "min", out["sd_ratio"].min(), "max", out["sd_ratio"].max())


def test_noise_marginals_end_to_end():
    """`stats.noise_marginals` on a short fit of the single-dataset example, both blocks: one row per bc_std / pop_std row of the fit
    frame, labelled as the frame labels them, in their order; sigma_q* = exp of the quantiles; a wrong block is refused."""
    import barbay_jl_amd as bb
    data = pd.read_csv(os.path.join(GOLD, "data001_single.csv"))
    model = bb.model.fitness_normal
    df = bb.vi.advi(data=data, model=model, advi=bb.vi.ADVI(1, 200), verbose=False, seed=1)
    for block, vartype in (("bc", "bc_std"), ("pop", "pop_std")):
        out = bb.stats.noise_marginals(data, df, model=model, block=block, n_samples=64, seed=3)
        blk = df[df["vartype"] == vartype].reset_index(drop=True)
        _check_frame(out, blk)
    assert len(out) == data["time"].nunique() - 1
    with pytest.raises(bb.BarBayError):
        bb.stats.noise_marginals(data, df, model=model, block="tau")
