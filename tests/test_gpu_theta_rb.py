"""bb_theta_rb (Rao-Blackwellised hyper-fitness marginals, barbay.jl_amd/csrc/bb_rb.h) on the device: the emulation's cases, the
identity also against the device's own gradient, a statistical check against independent numpy draws, and the user entry point
end to end."""
import os

import numpy as np
import pandas as pd
import pytest

import _ppc_cases as pc
import _theta_rb_cases as tc

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("name", tc.IDENTITY)
def test_conditional_matches_the_gradient_of_the_log_joint(hip_lib, name):
    tc.check_identity(hip_lib, name, device=True)


@pytest.mark.parametrize("name", sorted(tc.golden_cases()))
def test_marginals_match_golden(hip_lib, name):
    tc.check_golden(hip_lib, name, "device")


def test_members_are_summed_by_the_chunk_rule_whatever_the_internal_order(hip_lib):
    tc.check_chunk_rule(hip_lib, "device")


def test_independent_of_launch_mode_and_repeatable(hip_lib):
    tc.check_launch_modes(hip_lib)


@pytest.mark.parametrize("name", tc.GROUP_CASES)
def test_group_handle_equals_single_device(hip_lib, name):
    tc.check_group_handle(hip_lib, name)


def test_buffer_reuse_across_calls_and_sizes(hip_lib):
    tc.check_buffer_reuse(hip_lib)


def test_handle_untouched(hip_lib):
    tc.check_handle_untouched(hip_lib)


@pytest.mark.parametrize("name", ["genotype_regrouped", "multienv_replicate"])
def test_own_draws_equal_the_same_draws_passed_in(hip_lib, name):
    tc.check_internal_against_explicit_draws(hip_lib, name)


def test_nan_parameter_stays_in_its_group(hip_lib):
    tc.check_nan_parameter(hip_lib)


def test_nan_in_a_member_without_steps_changes_nothing(hip_lib):
    tc.check_nan_in_a_member_without_steps(hip_lib)


def test_theta_rb_errors(hip_lib):
    tc.check_errors(hip_lib)


def test_marginal_against_a_large_numpy_sample(hip_lib):
    """One genotype's rb_mean, rb_sd^2 and p_pos (threshold at its rb_mean + rb_sd) at n_samples = BB_RB_MAX_SAMPLES against 400 000
    independent numpy draws of the posterior pushed through the numpy restatement, each within 6 Monte-Carlo standard errors of the
    two estimates together."""
    from scipy.special import erfc
    sp, mu, om = tc.inputs("genotype_regrouped")
    g, n, N = 2, 400_000, tc.MAXN
    with pc._handle(hip_lib, sp, mu, om) as e:
        mean, sigma = e.posterior()
        first = tc.trb(e, N, seed=17, probs=())
        s0 = float(first["rb_mean"][g] + first["rb_sd"][g])
        got = tc.trb(e, N, seed=17, probs=(), threshold=s0)
    assert got["rb_mean"][g] == first["rb_mean"][g] and got["rb_sd"][g] == first["rb_sd"][g]
    gen = np.random.default_rng(0)
    T = sp.n_time[0]
    lo = sp.offsets()["loglambda"][0]
    rows = {lo + (sp.n_neutral + m) * T + t for m in tc.members(sp, g) for t in range(T)}
    cache = {}

    def draw(i):                                                    # every latent drawn once, independently; the members' own loglambda
        if i in cache:                                              # rows are read twice (the normalisers, then their steps) and kept
            return cache[i]
        x = gen.normal(mean[i], sigma[i], n)
        if i in rows:
            cache[i] = x
        return x

    _, m, sd, _, _ = tc.conditionals(sp, draw, n, groups=[g])
    m, sd = m[g], sd[g]
    p = 0.5 * erfc(-(m - s0) / (sd * np.sqrt(2.0)))
    v = sd * sd + (m - m.mean()) ** 2                               # per-draw terms of rb_sd^2 (the centring's own error is of second order)
    for name, dev, x in (("rb_mean", got["rb_mean"][g], m), ("rb_sd^2", got["rb_sd"][g] ** 2, v), ("p_pos", got["p_pos"][g], p)):
        se = np.sqrt(x.var() / n + x.var() / N)
        print(name, dev, "numpy", x.mean(), "se", se)
        assert abs(dev - x.mean()) < 6 * se, name


COLUMNS = ["genotype", "id", "env", "n_members", "n_steps", "q_mean", "q_sd", "rb_mean", "rb_sd", "sd_ratio", "p_pos", "p_neg"]


def _check_frame(out, blk, probs=("q2.5", "q50", "q97.5")):
    assert list(out.columns) == COLUMNS + list(probs) and len(out) == len(blk)
    assert np.isfinite(out.drop(columns=["genotype", "id", "env"]).to_numpy(dtype=np.float64)).all()
    assert (out["rb_sd"] > 0).all() and (out["q_sd"] > 0).all() and (out["n_members"] > 0).all() and (out["n_steps"] > 0).all()
    assert np.abs(out["p_pos"] + out["p_neg"] - 1.0).max() <= 1e-12
    q = out[list(probs)].to_numpy()
    assert (np.diff(q, axis=1) > 0).all()
    print("sd_ratio: median", out["sd_ratio"].median(), "min", out["sd_ratio"].min(), "max", out["sd_ratio"].max(),
          "quartiles", out["sd_ratio"].quantile([0.25, 0.75]).tolist())


def test_hyperfitness_marginals_end_to_end_genotypes():
    """`stats.hyperfitness_marginals` on a short fit of the genotype data: one row per genotype, labelled as the fit frame labels
    its bc_hyperfitness rows, in their order; a chain in place of q's draws; a model without a theta is refused."""
    import barbay_jl_amd as bb
    data = pd.read_csv(os.path.join(GOLD, "data004_multigen.csv"))
    model = bb.model.genotype_fitness_normal
    df = bb.vi.advi(data=data, model=model, advi=bb.vi.ADVI(1, 200), verbose=False, seed=1, genotype_col="genotype")
    out = bb.stats.hyperfitness_marginals(data, df, model=model, n_samples=500, seed=3, genotype_col="genotype")
    blk = df[df["vartype"] == "bc_hyperfitness"].reset_index(drop=True)
    _check_frame(out, blk)
    assert list(out["genotype"]) == list(blk["id"]) and out["id"].isna().all() and out["env"].isna().all()
    per = data.loc[~data["neutral"]].groupby("genotype")["barcode"].nunique()
    assert list(out["n_members"]) == [per[g] for g in out["genotype"]]
    assert list(out["n_steps"]) == [per[g] * (data["time"].nunique() - 1) for g in out["genotype"]]
    assert (np.abs(out["q_mean"] - blk["mean"]) <= 6 * blk["std"] / np.sqrt(500)).all()
    flat = bb.vi.advi(data=data, model=bb.model.fitness_normal, advi=bb.vi.ADVI(1, 20), verbose=False, seed=1)
    with pytest.raises(bb.BarBayError, match="hyper-fitness"):        # a fit of a model without a theta, handed over whole
        bb.stats.hyperfitness_marginals(data, flat, model=bb.model.fitness_normal)
    D = int((df["vartype"] == "log_poisson").to_numpy().nonzero()[0][-1]) + 1       # (the frame's later rows are derived, not latents)
    g = np.random.default_rng(1)
    chain = df["mean"].to_numpy()[:D] + 0.01 * g.standard_normal((2, 20, D))
    oc = bb.stats.hyperfitness_marginals(data, df, model=model, chain=chain, probs=(0.5,), genotype_col="genotype")
    assert list(oc.columns)[-1] == "q50" and len(oc) == len(out) and np.isfinite(oc["rb_sd"]).all() and (oc["q_sd"] < 0.05).all()
    with pytest.raises(bb.BarBayError):
        bb.stats.hyperfitness_marginals(data, df, model=model, chain=chain[..., :-1], genotype_col="genotype")


def test_hyperfitness_marginals_keeps_the_order_of_scattered_genotypes():
    """`data004_multigen.csv` has one genotype, so its rows cannot be out of order.  The same counts with its ten mutants dealt to
    three genotypes, scattered and named so that neither the sorted nor the grouped order is the order of first appearance: the
    rows follow the fit frame's bc_hyperfitness rows, and n_members counts each genotype's mutants."""
    import barbay_jl_amd as bb
    data = pd.read_csv(os.path.join(GOLD, "data004_multigen.csv"))
    mutants = list(dict.fromkeys(data.loc[~data["neutral"], "barcode"]))
    deal = dict(zip(mutants, ["gz", "ga", "gz", "gm", "ga", "gm", "gm", "gz", "ga", "gm"]))
    assert len(mutants) == len(deal) == 10
    data.loc[~data["neutral"], "genotype"] = data.loc[~data["neutral"], "barcode"].map(deal)
    model = bb.model.genotype_fitness_normal
    df = bb.vi.advi(data=data, model=model, advi=bb.vi.ADVI(1, 50), verbose=False, seed=1, genotype_col="genotype")
    out = bb.stats.hyperfitness_marginals(data, df, model=model, n_samples=200, seed=3, probs=(0.5,), genotype_col="genotype")
    blk = df[df["vartype"] == "bc_hyperfitness"].reset_index(drop=True)
    assert list(out["genotype"]) == list(blk["id"]) and sorted(out["genotype"]) == ["ga", "gm", "gz"]
    assert list(out["genotype"]) != sorted(out["genotype"])
    count = pd.Series(list(deal.values())).value_counts()
    assert list(out["n_members"]) == [count[g] for g in out["genotype"]] and sorted(out["n_members"]) == [3, 3, 4]
    assert (np.abs(out["q_mean"] - blk["mean"]) <= 6 * blk["std"] / np.sqrt(200)).all()
    assert np.isfinite(out[["rb_mean", "rb_sd", "q50"]].to_numpy()).all()


def test_hyperfitness_marginals_end_to_end_replicates():
    """The same on the hierarchical-replicate data: one row per mutant, labelled as the fit frame's bc_hyperfitness rows."""
    import barbay_jl_amd as bb
    data = pd.read_csv(os.path.join(GOLD, "data002_hier-rep.csv"))
    model = bb.model.replicate_fitness_normal
    df = bb.vi.advi(data=data, model=model, advi=bb.vi.ADVI(1, 200), verbose=False, seed=1, rep_col="rep")
    out = bb.stats.hyperfitness_marginals(data, df, model=model, n_samples=500, seed=3, rep_col="rep")
    blk = df[df["vartype"] == "bc_hyperfitness"].reset_index(drop=True)
    _check_frame(out, blk)
    assert list(out["id"]) == list(blk["id"]) and out["genotype"].isna().all() and out["env"].isna().all()
    assert (out["n_members"] == data["rep"].nunique()).all()
    with pytest.raises(bb.BarBayError):
        bb.stats.hyperfitness_marginals(data, df.iloc[3:], model=model, rep_col="rep")
