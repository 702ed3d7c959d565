"""bb_logtau_rb (Rao-Blackwellised logtau marginals, barbay.jl_amd/csrc/bb_ltrb.h) on the device: the emulation's cases and the golden
at the largest sample count, the identity also against the device's own gradient, a statistical check against independent numpy
draws, and the user entry point end to end."""
import os

import numpy as np
import pandas as pd
import pytest

import _ppc_cases as pc
import _logtau_rb_cases as tc

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("name", sorted(tc.golden_cases()))
def test_marginals_match_golden(hip_lib, name):
    tc.check_golden(hip_lib, name, "device")


@pytest.mark.parametrize("name", tc.IDENTITY)
def test_gradient_of_the_log_joint_vanishes_at_the_modes(hip_lib, name):
    tc.check_identity(hip_lib, name, device=True)


def test_prior_only_entries(hip_lib):
    tc.check_prior_only(hip_lib)


def test_independent_of_launch_mode_and_repeatable(hip_lib):
    tc.check_launch_modes(hip_lib)


@pytest.mark.parametrize("name", tc.GROUP_CASES)
def test_group_handle_equals_single_device(hip_lib, name):
    tc.check_group_handle(hip_lib, name)


def test_buffer_reuse_across_calls_sizes_and_modes(hip_lib):
    tc.check_buffer_reuse(hip_lib)


def test_handle_untouched(hip_lib):
    tc.check_handle_untouched(hip_lib)


@pytest.mark.parametrize("name", ["genotype_matrix_prior", "multienv_replicate", "replicate_ragged_method"])
def test_own_draws_equal_the_same_draws_passed_in(hip_lib, name):
    tc.check_internal_against_explicit_draws(hip_lib, name)


def test_nan_stays_in_its_entries(hip_lib):
    tc.check_nan_stays(hip_lib)


def test_four_and_eight_quantiles(hip_lib):
    tc.check_more_quantiles(hip_lib, "device")


def test_logtau_rb_errors(hip_lib):
    tc.check_errors(hip_lib)


@pytest.mark.parametrize("mode", tc.MODES)
def test_marginal_against_a_large_numpy_sample(hip_lib, mode, entry=1):
    """One entry's rb_mean, rb_sd^2, tau_mean and pool_mean at n_samples = BB_LOGTAU_RB_MAX_SAMPLES against 200 000 independent numpy
    draws of the posterior pushed through the numpy restatement, each within 6 Monte-Carlo standard errors of the two estimates
    together.  (The restatement works one draw at a time: 200 000 of them are 4000 draws' worth of work forty times over, so the
    independent sample is pushed through in its vectorised form below -- the same statements on arrays.)"""
    sp, mu, om = tc.inputs(tc.TINY)
    n, N = 200_000, tc.MAXN
    with pc._handle(hip_lib, sp, mu, om) as e:
        mean, sigma = e.posterior()
        got = tc.ltrb(e, mode, N, seed=17, probs=())

    def draw(i):                                                    # latent i's draws: its own stream, the same whenever it is asked for
        return np.random.default_rng([0, int(i)]).normal(mean[i], sigma[i], n)

    l, nt, w, tt, Y, a, ib2 = tc.cond_inputs(sp, draw, n, entries=[entry])[entry]
    E, V, T, P = tc.moments_many(tc.MODE_ID[mode], nt, w, tt, Y, a, ib2)
    v = V + (E - E.mean()) ** 2                                     # per-draw terms of rb_sd^2 (the centring's own error is of second order)
    for name, dev, x in (("rb_mean", got["rb_mean"][entry], E), ("rb_sd^2", got["rb_sd"][entry] ** 2, v), ("tau_mean", got["tau_mean"][entry], T),
                         ("pool_mean", got["pool_mean"][entry], P)):
        se = np.sqrt(x.var() / n + x.var() / N)
        print(mode, name, dev, "numpy", x.mean(), "se", se)
        assert abs(dev - x.mean()) < 6 * se, name


def test_deviation_marginals_end_to_end():
    """`stats.deviation_marginals` on a short fit of the hierarchical-replicate example, both modes: one row per bc_deviations row of
    the fit frame, labelled as the frame labels them, in their order; tau_q* = exp of the quantiles; a model without a logtau is
    refused."""
    import barbay_jl_amd as bb
    data = pd.read_csv(os.path.join(GOLD, "data002_hier-rep.csv"))
    model = bb.model.replicate_fitness_normal
    df = bb.vi.advi(data=data, model=model, advi=bb.vi.ADVI(1, 200), verbose=False, seed=1, rep_col="rep")
    blk = df[df["vartype"] == "bc_deviations"].reset_index(drop=True)
    labels = [c for c in blk.columns if c not in ("mean", "std")]
    probs = ("q2.5", "q50", "q97.5")
    tail = ["n_terms", "q_mean", "q_sd", "rb_mean", "rb_sd", "sd_ratio", "mode_mean", "tau_mean", "pool_mean", "n_two_modes"] + list(probs) + ["tau_" + p for p in probs]
    for mode in tc.MODES:
        out = bb.stats.deviation_marginals(data, df, model=model, mode=mode, n_samples=64, seed=3, rep_col="rep")
        assert list(out.columns) == labels + tail and len(out) == len(blk) > 0
        for c in labels:
            assert [x for x in out[c]] == [x for x in blk[c]] or (out[c].isna().all() and blk[c].isna().all()), c
        assert np.isfinite(out[tail].to_numpy(dtype=np.float64)).all()
        assert (out["rb_sd"] > 0).all() and (out["q_sd"] > 0).all() and (out["n_terms"] > 0).all()
        assert ((out["pool_mean"] >= 0) & (out["pool_mean"] <= 1)).all() and (out["tau_mean"] > 0).all()
        assert ((out["n_two_modes"] >= 0) & (out["n_two_modes"] <= 64)).all()
        for p in probs:
            assert np.array_equal(out["tau_" + p].to_numpy(), np.exp(out[p].to_numpy()))
        assert (np.diff(out[list(probs)].to_numpy(), axis=1) > 0).all()
        print(mode, "sd_ratio: median", out["sd_ratio"].median(), "pool_mean: median", out["pool_mean"].median(), "two-mode draws", int(out["n_two_modes"].sum()))
    with pytest.raises(bb.BarBayError):
        bb.stats.deviation_marginals(data, df, model=model, mode="tau", rep_col="rep")
    single = pd.read_csv(os.path.join(GOLD, "data001_single.csv"))
    flat = bb.model.fitness_normal
    df1 = bb.vi.advi(data=single, model=flat, advi=bb.vi.ADVI(1, 20), verbose=False, seed=1)
    with pytest.raises(bb.BarBayError):
        bb.stats.deviation_marginals(single, df1, model=flat)
