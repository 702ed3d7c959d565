"""bb_popmean_rb (Rao-Blackwellised population-mean fitness marginals, barbay.jl_amd/csrc/bb_rb.h) on the device: the emulation's
cases, the identity also against the device's own gradient, a statistical check against independent numpy draws, and the user entry
point end to end."""
import os

import numpy as np
import pandas as pd
import pytest

import _ppc_cases as pc
import _pop_rb_cases as qc

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("name", qc.IDENTITY)
def test_conditional_matches_the_gradient_of_the_log_joint(hip_lib, name):
    qc.check_identity(hip_lib, name, device=True)


@pytest.mark.parametrize("name", sorted(qc.golden_cases()))
def test_marginals_match_golden(hip_lib, name):
    qc.check_golden(hip_lib, name, "device")


def test_members_are_summed_by_the_chunk_rule(hip_lib):
    qc.check_chunk_rule(hip_lib, "device")


def test_independent_of_launch_mode_and_repeatable(hip_lib):
    qc.check_launch_modes(hip_lib)


@pytest.mark.parametrize("name", qc.GROUP_CASES)
def test_group_handle_equals_single_device(hip_lib, name):
    qc.check_group_handle(hip_lib, name)


def test_buffer_reuse_across_calls_and_sizes(hip_lib):
    qc.check_buffer_reuse(hip_lib)


def test_handle_untouched(hip_lib):
    qc.check_handle_untouched(hip_lib)


@pytest.mark.parametrize("name", ["genotype_regrouped", "multienv_replicate", "replicate_ragged_method"])
def test_own_draws_equal_the_same_draws_passed_in(hip_lib, name):
    qc.check_internal_against_explicit_draws(hip_lib, name)


def test_nan_in_its_own_mean_leaves_the_conditional_alone(hip_lib):
    qc.check_nan_in_own_mean(hip_lib)


def test_nan_in_a_mutant_stays_in_its_replicate_and_environment(hip_lib):
    qc.check_nan_in_a_mutant(hip_lib)


def test_popmean_rb_errors(hip_lib):
    qc.check_errors(hip_lib)


def test_marginal_against_a_large_numpy_sample(hip_lib):
    """One group's rb_mean, rb_sd^2 and p_pos (threshold at its rb_mean + rb_sd) at n_samples = BB_RB_MAX_SAMPLES against 400 000
    independent numpy draws of the posterior pushed through the numpy restatement, each within 6 Monte-Carlo standard errors of the
    two estimates together."""
    from scipy.special import erfc
    sp, mu, om = qc.inputs("multienv_replicate")
    g, n, N = 6, 400_000, qc.MAXN                                   # the third step of the second replicate
    with pc._handle(hip_lib, sp, mu, om) as e:
        mean, sigma = e.posterior()
        first = qc.prb(e, N, seed=17, probs=())
        s0 = float(first["rb_mean"][g] + first["rb_sd"][g])
        got = qc.prb(e, N, seed=17, probs=(), threshold=s0)
    assert got["rb_mean"][g] == first["rb_mean"][g] and got["rb_sd"][g] == first["rb_sd"][g]

    def draw(i):                                                    # latent i's draws: its own stream, the same whenever it is asked for
        return np.random.default_rng([0, int(i)]).normal(mean[i], sigma[i], n)

    _, m, sd = qc.conditionals(sp, draw, n, groups=[g])
    m, sd = m[g], sd[g]
    p = 0.5 * erfc(-(m - s0) / (sd * np.sqrt(2.0)))
    v = sd * sd + (m - m.mean()) ** 2                               # per-draw terms of rb_sd^2 (the centring's own error is of second order)
    for name, dev, x in (("rb_mean", got["rb_mean"][g], m), ("rb_sd^2", got["rb_sd"][g] ** 2, v), ("p_pos", got["p_pos"][g], p)):
        se = np.sqrt(x.var() / n + x.var() / N)
        print(name, dev, "numpy", x.mean(), "se", se)
        assert abs(dev - x.mean()) < 6 * se, name


def _check_frame(out, blk, n_members, n, probs=("q2.5", "q50", "q97.5")):
    labels = [c for c in blk.columns if c not in ("mean", "std")]
    tail = ["n_members", "q_mean", "q_sd", "rb_mean", "rb_sd", "sd_ratio", "p_pos", "p_neg"] + list(probs)
    assert list(out.columns) == labels + tail and len(out) == len(blk) > 0
    for c in labels:                                                # the rows and labels of the frame's pop_mean_fitness rows, in their order
        assert list(out[c]) == list(blk[c]), c
    assert np.isfinite(out[tail].to_numpy(dtype=np.float64)).all()
    assert (out["rb_sd"] > 0).all() and (out["q_sd"] > 0).all() and (out["n_members"] == n_members).all()
    assert (np.abs(out["q_mean"] - blk["mean"]) <= 6 * blk["std"] / np.sqrt(n)).all()
    assert np.abs(out["p_pos"] + out["p_neg"] - 1.0).max() <= 1e-12
    q = out[list(probs)].to_numpy()
    assert (np.diff(q, axis=1) > 0).all()
    print("sd_ratio: median", out["sd_ratio"].median(), "min", out["sd_ratio"].min(), "max", out["sd_ratio"].max())


def test_popmean_marginals_end_to_end_single():
    """`stats.popmean_marginals` on a short fit of the single-dataset example: one row per pop_mean_fitness row of the fit frame,
    labelled as the frame labels them, in their order; a chain in place of q's draws; a chain of the wrong width is refused."""
    import barbay_jl_amd as bb
    data = pd.read_csv(os.path.join(GOLD, "data001_single.csv"))
    model = bb.model.fitness_normal
    df = bb.vi.advi(data=data, model=model, advi=bb.vi.ADVI(1, 200), verbose=False, seed=1)
    out = bb.stats.popmean_marginals(data, df, model=model, n_samples=500, seed=3)
    blk = df[df["vartype"] == "pop_mean_fitness"].reset_index(drop=True)
    assert len(blk) == data["time"].nunique() - 1
    _check_frame(out, blk, data["barcode"].nunique(), 500)
    D = int((df["vartype"] == "log_poisson").to_numpy().nonzero()[0][-1]) + 1       # (the frame's later rows, if any, are derived, not latents)
    g = np.random.default_rng(1)
    chain = df["mean"].to_numpy()[:D] + 0.01 * g.standard_normal((2, 20, D))
    oc = bb.stats.popmean_marginals(data, df, model=model, chain=chain, probs=(0.5,))
    assert list(oc.columns)[-1] == "q50" and len(oc) == len(out) and np.isfinite(oc["rb_sd"]).all() and (oc["q_sd"] < 0.05).all()
    with pytest.raises(bb.BarBayError):
        bb.stats.popmean_marginals(data, df, model=model, chain=chain[..., :-1])


def test_popmean_marginals_end_to_end_replicates():
    """The same on the hierarchical-replicate data: the rows run replicate by replicate, as the frame's do."""
    import barbay_jl_amd as bb
    data = pd.read_csv(os.path.join(GOLD, "data002_hier-rep.csv"))
    model = bb.model.replicate_fitness_normal
    df = bb.vi.advi(data=data, model=model, advi=bb.vi.ADVI(1, 200), verbose=False, seed=1, rep_col="rep")
    out = bb.stats.popmean_marginals(data, df, model=model, n_samples=500, seed=3, rep_col="rep")
    blk = df[df["vartype"] == "pop_mean_fitness"].reset_index(drop=True)
    _check_frame(out, blk, data["barcode"].nunique(), 500)
    assert out["rep"].nunique() == data["rep"].nunique()
    with pytest.raises(bb.BarBayError):
        bb.stats.popmean_marginals(data, df.iloc[3:], model=model, rep_col="rep")
