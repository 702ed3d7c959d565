"""bb_contrast_rb (Rao-Blackwellised fitness contrasts, barbay.jl_amd/csrc/bb_contrast.h) on the device: the emulation's cases,
a statistical check against independent numpy draws, and the user entry point `stats.fitness_contrasts` end to end."""
import os

import numpy as np
import pandas as pd
import pytest

import _contrast_cases as cc
import _ppc_cases as pc
import _rb_cases as rc

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("space,name", cc.single_term_cases())
def test_one_term_contrasts_match_the_marginals_goldens(hip_lib, space, name):
    cc.check_single_term(hip_lib, space, name, "device")


@pytest.mark.parametrize("space,case", cc.SPACE_CASES)
def test_contrast_composes_the_conditionals_of_its_terms(hip_lib, space, case):
    cc.check_composition(hip_lib, space, case)


@pytest.mark.parametrize("name", sorted(cc.golden_cases()))
def test_contrasts_match_golden(hip_lib, name):
    cc.check_golden(hip_lib, name, "device")


def test_difference_is_sharper_and_sum_wider_than_the_marginals_say(hip_lib):
    cc.check_point(hip_lib)


@pytest.mark.parametrize("space,case", [("fitness", "multienv"), ("fitness", "fitness_chunk"), ("theta", "genotype_chunks"), ("theta", "multienv_replicate")])
def test_independent_of_the_other_contrasts(hip_lib, space, case):
    cc.check_independent_of_the_other_contrasts(hip_lib, space, case)


def test_independent_of_launch_mode_and_repeatable(hip_lib):
    cc.check_launch_modes(hip_lib)


@pytest.mark.parametrize("space,case", [("fitness", "fitness"), ("fitness", "replicate_ragged"), ("theta", "genotype_regrouped")])
def test_group_handle_equals_single_device(hip_lib, space, case):
    cc.check_group_handle(hip_lib, space, case)


def test_buffer_reuse_across_calls_and_sizes(hip_lib):
    cc.check_buffer_reuse(hip_lib)


def test_handle_untouched(hip_lib):
    cc.check_handle_untouched(hip_lib)


@pytest.mark.parametrize("space,case", [("fitness", "fitness"), ("fitness", "genotype_regrouped"), ("theta", "multienv_replicate")])
def test_own_draws_equal_the_same_draws_passed_in(hip_lib, space, case):
    cc.check_internal_against_explicit_draws(hip_lib, space, case)


def test_nan_parameter_stays_in_its_contrasts(hip_lib):
    cc.check_nan_parameter(hip_lib)


def test_contrast_errors(hip_lib):
    cc.check_errors(hip_lib)


def test_contrast_against_a_large_numpy_sample(hip_lib):
    """The within-replicate pair s_10 - s_3 (posterior sd of the population mean 0.3: `_contrast_cases.point_inputs`) at n_samples =
    BB_RB_MAX_SAMPLES: rb_mean, rb_sd^2 and p_pos (threshold at rb_mean + rb_sd) against 400 000 independent numpy draws of the
    posterior pushed through the numpy restatement, each within 6 Monte-Carlo standard errors of the two estimates together."""
    from scipy.special import erfc
    sp, mu, om = cc.point_inputs()
    a, b, n, N = 10, 3, 400_000, cc.MAXN
    terms = [[(a, 1.0), (b, -1.0)]]
    with pc._handle(hip_lib, sp, mu, om) as e:
        mean, sigma = e.posterior()
        first = cc.crb(e, terms, "fitness", N, seed=17, probs=())
        s0 = float(first["rb_mean"][0] + first["rb_sd"][0])
        got = cc.crb(e, terms, "fitness", N, seed=17, probs=(), threshold=s0)
    assert got["rb_mean"][0] == first["rb_mean"][0] and got["rb_sd"][0] == first["rb_sd"][0]
    g = np.random.default_rng(0)
    T = sp.n_time[0]
    rows = [sp.offsets()["loglambda"][0] + (sp.n_neutral + m) * T for m in (a, b)]
    keep = sp.offsets()["s_pop"]
    cache = {}

    def draw(i):                                                    # every latent drawn once, independently; the two mutants' loglambda rows
        if i in cache:                                              # are read twice (the normalisers, then their steps) and kept, as is sbar
            return cache[i]
        x = g.normal(mean[i], sigma[i], n)
        if any(lo <= i < lo + T for lo in rows) or keep[0] <= i < keep[1]:
            cache[i] = x
        return x

    el = rc.conditionals(sp, draw, n, mutants=[a, b])
    _, m, sd, _ = cc.compose(el, terms[0])
    p = 0.5 * erfc(-(m - s0) / (sd * np.sqrt(2.0)))
    v = sd * sd + (m - m.mean()) ** 2                               # per-draw terms of rb_sd^2 (the centring's own error is of second order)
    for name, dev, x in (("rb_mean", got["rb_mean"][0], m), ("rb_sd^2", got["rb_sd"][0] ** 2, v), ("p_pos", got["p_pos"][0], p)):
        se = np.sqrt(x.var() / n + x.var() / N)
        print(name, dev, "numpy", x.mean(), "se", se)
        assert abs(dev - x.mean()) < 6 * se, name
    assert 0.05 < got["p_pos"][0] < 0.5


QCOLS = ["q2.5", "q50", "q97.5"]
COLUMNS = ["contrast", "terms", "n_terms", "min_steps", "q_mean", "q_sd", "rb_mean", "rb_sd", "sd_ratio", "indep_sd", "common_mode", "p_pos", "p_neg"] + QCOLS


def test_fitness_contrasts_between_environments_end_to_end():
    """`stats.fitness_contrasts(between="env")` on a multi-environment fit: one line per (mutant, pair of environments), later label
    minus earlier; the draws' own contrast is the difference of the two `fitness_marginals` rows at equal seed."""
    import barbay_jl_amd as bb
    data = pd.read_csv(os.path.join(GOLD, "data003_multienv.csv"))
    model, cols = bb.model.multienv_fitness_normal, dict(env_col="env")
    df = bb.vi.advi(data=data, model=model, advi=bb.vi.ADVI(1, 50), verbose=False, seed=1, **cols)
    n = 500
    out = bb.stats.fitness_contrasts(data, df, model=model, between="env", n_samples=n, seed=3, **cols)
    fm = bb.stats.fitness_marginals(data, df, model=model, n_samples=n, seed=3, **cols)
    assert list(out.columns) == COLUMNS
    envs = list(dict.fromkeys(fm["env"]))
    ids = list(dict.fromkeys(fm["id"]))
    E = len(envs)
    assert E >= 2 and len(out) == len(ids) * E * (E - 1) // 2 and list(out["contrast"]) == list(range(len(out)))
    assert (out["n_terms"] == 2).all() and not out["terms"].duplicated().any()
    at = {(i, r, e): k for k, (i, r, e) in enumerate(zip(fm["id"], fm["rep"], fm["env"]))}
    x = 0
    for i in ids:
        for a in range(E):
            for b in range(a + 1, E):
                assert out["terms"][x] == f"+1 ({i}, R1, {envs[b]}) -1 ({i}, R1, {envs[a]})", out["terms"][x]
                ka, kb = at[(i, "R1", envs[a])], at[(i, "R1", envs[b])]
                want = fm["q_mean"][kb] - fm["q_mean"][ka]
                assert abs(out["q_mean"][x] - want) <= rc.TOL * max(abs(want), 1.0)
                assert out["min_steps"][x] == min(fm["n_steps"][ka], fm["n_steps"][kb])
                ind = np.sqrt(fm["rb_sd"][ka] ** 2 + fm["rb_sd"][kb] ** 2)
                assert abs(out["indep_sd"][x] - ind) <= rc.TOL * max(ind, 1.0)
                x += 1
    live = out[out["min_steps"] > 0]
    assert len(live) and np.isfinite(live.drop(columns=["terms"]).to_numpy(dtype=np.float64)).all()
    assert np.abs(out["p_pos"] + out["p_neg"] - 1.0).max() <= 1e-12
    assert (out["q2.5"] < out["q50"]).all() and (out["q50"] < out["q97.5"]).all()
    assert np.allclose(out["sd_ratio"], out["rb_sd"] / out["q_sd"]) and np.allclose(out["common_mode"], out["rb_sd"] / out["indep_sd"])
    print("between env: common_mode median", out["common_mode"].median(), "min", out["common_mode"].min(), "max", out["common_mode"].max())
    with pytest.raises(bb.BarBayError):
        bb.stats.fitness_contrasts(data, df, model=model, between="rep", **cols)                        # one replicate
    with pytest.raises(bb.BarBayError):
        bb.stats.fitness_contrasts(data, df, model=model, between="env", level="hyper", **cols)         # no theta


def test_fitness_contrasts_against_a_reference_and_explicit_lists_agree():
    """`between="id"` with a reference and the same pairs named in `contrasts=` give the same frame; the errors of the entry point."""
    import barbay_jl_amd as bb
    data = pd.read_csv(os.path.join(GOLD, "data001_single.csv"))
    model = bb.model.fitness_normal
    df = bb.vi.advi(data=data, model=model, advi=bb.vi.ADVI(1, 50), verbose=False, seed=1)
    mutants = list(dict.fromkeys(bb.stats.fitness_marginals(data, df, model=model, n_samples=2, probs=())["id"]))
    ref = mutants[2]
    kw = dict(model=model, n_samples=300, seed=3)
    a = bb.stats.fitness_contrasts(data, df, between="id", reference=ref, **kw)
    b = bb.stats.fitness_contrasts(data, df, contrasts=[{(m, "R1", None): 1.0, (ref, "R1", None): -1.0} for m in mutants if m != ref], **kw)
    assert list(a.columns) == COLUMNS and len(a) == len(mutants) - 1
    pd.testing.assert_frame_equal(a, b, check_exact=True)
    assert np.isfinite(a.drop(columns=["terms"]).to_numpy(dtype=np.float64)).all()
    print("between id: common_mode median", a["common_mode"].median(), "min", a["common_mode"].min(), "max", a["common_mode"].max())
    for bad in (dict(contrasts=[{("no such barcode", "R1", None): 1.0}]),                               # an unknown label
                dict(contrasts=[{(ref, "R1", None): 1.0}], between="id", reference=ref),                # both
                dict(),                                                                                  # neither
                dict(between="env"),                                                                     # a model without environments
                dict(between="id"),                                                                      # no reference
                dict(between="id", reference="no such barcode"),
                dict(between="id", reference=ref, level="hyper")):                                       # fitness_normal has no theta
        with pytest.raises(bb.BarBayError):
            bb.stats.fitness_contrasts(data, df, **kw, **bad)
