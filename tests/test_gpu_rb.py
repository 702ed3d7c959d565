"""bb_fitness_rb (Rao-Blackwellised fitness marginals, barbay.jl_amd/csrc/bb_rb.h) on the device: the emulation's cases, the
identity also against the device's own gradient, a statistical check against independent numpy draws, and the user entry point
end to end."""
import os

import numpy as np
import pandas as pd
import pytest

import _ppc_cases as pc
import _rb_cases as rc

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("name", rc.IDENTITY)
def test_conditional_matches_the_gradient_of_the_log_joint(hip_lib, name):
    rc.check_identity(hip_lib, name, device=True)


@pytest.mark.parametrize("name", sorted(rc.golden_cases()))
def test_marginals_match_golden(hip_lib, name):
    rc.check_golden(hip_lib, name, "device")


def test_four_and_eight_quantiles_match_the_restatement(hip_lib):
    rc.check_many_quantiles(hip_lib)


def test_independent_of_launch_mode_and_repeatable(hip_lib):
    rc.check_launch_modes(hip_lib)


@pytest.mark.parametrize("name", pc.GROUP_CASES)
def test_group_handle_equals_single_device(hip_lib, name):
    rc.check_group_handle(hip_lib, name)


def test_buffer_reuse_across_calls_and_sizes(hip_lib):
    rc.check_buffer_reuse(hip_lib)


def test_handle_untouched(hip_lib):
    rc.check_handle_untouched(hip_lib)


@pytest.mark.parametrize("name", ["fitness", "genotype_regrouped", "multienv_replicate"])
def test_own_draws_equal_the_same_draws_passed_in(hip_lib, name):
    rc.check_internal_against_explicit_draws(hip_lib, name)


def test_nan_parameter_stays_in_its_units(hip_lib):
    rc.check_nan_parameter(hip_lib)


def test_rb_errors(hip_lib):
    rc.check_errors(hip_lib)


def test_marginal_against_a_large_numpy_sample(hip_lib):
    """One mutant's rb_mean, rb_sd^2 and p_pos (threshold at its rb_mean + rb_sd) at n_samples = BB_RB_MAX_SAMPLES against 400 000
    independent numpy draws of the posterior pushed through the numpy restatement, each within 6 Monte-Carlo standard errors of the
    two estimates together."""
    from scipy.special import erfc
    sp, mu, om = rc.inputs("fitness")
    u, n, N = 22, 400_000, rc.MAXN
    with pc._handle(hip_lib, sp, mu, om) as e:
        mean, sigma = e.posterior()
        first = rc.rb(e, N, seed=17, probs=())
        s0 = float(first["rb_mean"][u] + first["rb_sd"][u])
        got = rc.rb(e, N, seed=17, probs=(), threshold=s0)
    assert got["rb_mean"][u] == first["rb_mean"][u] and got["rb_sd"][u] == first["rb_sd"][u]
    g = np.random.default_rng(0)
    T = sp.n_time[0]
    lo = sp.offsets()["loglambda"][0] + (sp.n_neutral + u) * T
    cache = {}

    def draw(i):                                                    # every latent drawn once, independently; the mutant's own loglambda
        if i in cache:                                              # row is read twice (the normalisers, then its steps) and kept
            return cache[i]
        x = g.normal(mean[i], sigma[i], n)
        if lo <= i < lo + T:
            cache[i] = x
        return x

    _, m, sd, _ = rc.conditionals(sp, draw, n, mutants=[u])
    m, sd = m[u], sd[u]
    p = 0.5 * erfc(-(m - s0) / (sd * np.sqrt(2.0)))
    v = sd * sd + (m - m.mean()) ** 2                               # per-draw terms of rb_sd^2 (the centring's own error is of second order)
    for name, dev, x in (("rb_mean", got["rb_mean"][u], m), ("rb_sd^2", got["rb_sd"][u] ** 2, v), ("p_pos", got["p_pos"][u], p)):
        se = np.sqrt(x.var() / n + x.var() / N)
        print(name, dev, "numpy", x.mean(), "se", se)
        assert abs(dev - x.mean()) < 6 * se, name
    assert 0.05 < got["p_pos"][u] < 0.5


def _fit(data):
    import barbay_jl_amd as bb
    return bb.vi.advi(data=data, model=bb.model.fitness_normal, advi=bb.vi.ADVI(1, 3000), verbose=False, seed=1)


def test_fitness_marginals_end_to_end_and_a_starved_mutant_is_no_sharper():
    """The frame of `stats.fitness_marginals` on a fit; a mutant whose counts were cut to at most 3 reads at every time point before
    the fit has an rb_sd of at least the median mutant's (a sign-only property: nobody has measured the size of sd_ratio)."""
    import barbay_jl_amd as bb
    data = pd.read_csv(os.path.join(GOLD, "data001_single.csv"))
    starved = sorted(data.loc[~data["neutral"], "barcode"].unique())[4]
    sel = data["barcode"] == starved
    data.loc[sel, "count"] = np.minimum(data.loc[sel, "count"], 3)
    df = _fit(data)
    out = bb.stats.fitness_marginals(data, df, model=bb.model.fitness_normal, n_samples=500, seed=3)
    assert list(out.columns) == ["id", "rep", "env", "n_steps", "q_mean", "q_sd", "rb_mean", "rb_sd", "sd_ratio", "p_pos", "p_neg",
                                 "q2.5", "q50", "q97.5"]
    mutants = data.loc[~data["neutral"], "barcode"]
    assert len(out) == mutants.nunique() and set(out["id"]) == set(mutants)
    assert (out["n_steps"] == data["time"].nunique() - 1).all() and (out["rep"] == "R1").all() and out["env"].isna().all()
    assert np.isfinite(out.drop(columns=["id", "rep", "env"]).to_numpy(dtype=np.float64)).all()
    assert (out["rb_sd"] > 0).all() and (out["q_sd"] > 0).all()
    assert np.abs(out["p_pos"] + out["p_neg"] - 1.0).max() <= 1e-12
    assert (out["q2.5"] < out["q50"]).all() and (out["q50"] < out["q97.5"]).all()
    with pytest.raises(bb.BarBayError):
        bb.stats.fitness_marginals(data, df.iloc[3:], model=bb.model.fitness_normal)
    print("sd_ratio: median", out["sd_ratio"].median(), "min", out["sd_ratio"].min(), "max", out["sd_ratio"].max())
    assert out.loc[out["id"] == starved, "rb_sd"].iloc[0] >= out["rb_sd"].median()
    # an explicit chain in place of q's draws: here 40 draws around the fit, as mcmc_sample returns them ([walkers, steps, D])
    D = len(out) * 2 + 2 * (data["time"].nunique() - 1) + data["barcode"].nunique() * data["time"].nunique()
    g = np.random.default_rng(1)
    chain = df["mean"].to_numpy()[:D] + 0.01 * g.standard_normal((2, 20, D))
    oc = bb.stats.fitness_marginals(data, df, model=bb.model.fitness_normal, chain=chain, probs=(0.5,))
    assert list(oc.columns)[-1] == "q50" and len(oc) == len(out) and np.isfinite(oc["rb_sd"]).all() and (oc["q_sd"] < 0.05).all()
    with pytest.raises(bb.BarBayError):
        bb.stats.fitness_marginals(data, df, model=bb.model.fitness_normal, chain=chain[..., :-1])


def _labels_case(kind):
    import barbay_jl_amd as bb
    if kind == "multienv":
        data = pd.read_csv(os.path.join(GOLD, "data003_multienv.csv"))
        return data, bb.model.multienv_fitness_normal, dict(env_col="env"), "bc_fitness"
    from test_host_surface import _tidy_rep_env
    return _tidy_rep_env(ragged=True), bb.model.multienv_replicate_fitness_normal, dict(rep_col="rep", env_col="env"), "bc_noncenter"


@pytest.mark.parametrize("kind", ["multienv", "multienv_replicate_ragged"])
def test_fitness_marginals_labels_units_as_the_fit_frame_does(kind):
    """Environments and replicates: the rows of `stats.fitness_marginals` carry, row by row, the (id, rep, env) labels the fit's
    own frame gives the block the units are numbered by (s_bc, or theta_tilde for the hierarchical kinds); n_steps is the number
    of the replicate's later time points in the row's environment, counted from the data; for the s_bc block q_mean is the mean
    of draws of that very row of the fit (within 6 of its standard errors)."""
    import barbay_jl_amd as bb
    data, model, cols, vartype = _labels_case(kind)
    df = bb.vi.advi(data=data, model=model, advi=bb.vi.ADVI(1, 50), verbose=False, seed=1, **cols)
    n = 500
    out = bb.stats.fitness_marginals(data, df, model=model, n_samples=n, seed=3, probs=(0.5,), **cols)
    blk = df[df["vartype"] == vartype].reset_index(drop=True)
    assert len(out) == len(blk) and list(out["id"]) == list(blk["id"]) and list(out["env"]) == list(blk["env"])
    rep = list(blk["rep"]) if "rep" in blk.columns else ["R1"] * len(blk)
    assert list(out["rep"]) == rep
    assert not out.duplicated(subset=["id", "rep", "env"]).any()
    d = data.assign(rep=data["rep"] if "rep" in data.columns else "R1")
    later = {}                                                      # (rep, env) -> later time points in that environment
    for r, dr in d.groupby("rep"):
        envs = dr.drop_duplicates("time").sort_values("time")["env"].tolist()
        for e in set(d["env"]):
            later[(r, e)] = envs[1:].count(e)
    assert list(out["n_steps"]) == [later[(r, e)] for r, e in zip(out["rep"], out["env"])]
    assert np.isfinite(out[["rb_mean", "rb_sd", "q50"]].to_numpy()).all()
    if kind == "multienv_replicate_ragged":                         # its second replicate never returns to environment "a": the prior
        assert later[("R2", "a")] == 0 and later[("R1", "a")] == 1
    if vartype == "bc_fitness":
        assert (np.abs(out["q_mean"] - blk["mean"]) <= 6 * blk["std"] / np.sqrt(n)).all()
        assert (np.abs(out["q_sd"] / blk["std"] - 1.0) < 0.25).all()
