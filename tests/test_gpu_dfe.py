"""bb_dfe_rb (posterior of the fitness distribution of sets of units, barbay.jl_amd/csrc/bb_dfe.h) on the device: the emulation's
cases, a statistical check against independent numpy draws, and the user entry point `stats.fitness_distribution` end to end."""
import os

import numpy as np
import pandas as pd
import pytest

import _contrast_cases as cc
import _dfe_cases as dc
import _ppc_cases as pc
import _rb_cases as rc

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("name", sorted(dc.golden_cases()))
def test_dfe_matches_golden(hip_lib, name):
    dc.check_golden(hip_lib, name, "device")


@pytest.mark.parametrize("name", sorted(rc.golden_cases()))
def test_one_unit_sets_match_the_marginals_tails(hip_lib, name):
    dc.check_tie(hip_lib, name, "device")


@pytest.mark.parametrize("case", dc.CASES)
def test_dfe_composes_the_tails_of_its_units(hip_lib, case):
    dc.check_composition(hip_lib, case)


def test_fraction_moves_between_draws_more_than_within(hip_lib):
    dc.check_point(hip_lib)


@pytest.mark.parametrize("case", ["fitness_chunk", "multienv_replicate", "multienv_env0_only_first"])
def test_independent_of_the_rest_of_the_call(hip_lib, case):
    dc.check_independent_of_the_rest_of_the_call(hip_lib, case)


def test_grids_of_1_5_and_64_points(hip_lib):
    dc.check_grid_sizes_against_restatement(hip_lib)


def test_independent_of_launch_mode_and_repeatable(hip_lib):
    dc.check_launch_modes(hip_lib)


@pytest.mark.parametrize("case", ["fitness", "replicate_ragged", "genotype_regrouped"])
def test_group_handle_equals_single_device(hip_lib, case):
    dc.check_group_handle(hip_lib, case)


def test_buffer_reuse_across_calls_and_sizes(hip_lib):
    dc.check_buffer_reuse(hip_lib)


def test_handle_untouched(hip_lib):
    dc.check_handle_untouched(hip_lib)


@pytest.mark.parametrize("case", ["fitness", "genotype_regrouped", "multienv_replicate"])
def test_own_draws_equal_the_same_draws_passed_in(hip_lib, case):
    dc.check_internal_against_explicit_draws(hip_lib, case)


def test_nan_parameter_stays_in_its_sets(hip_lib):
    dc.check_nan_parameter(hip_lib)


def test_dfe_errors(hip_lib):
    dc.check_errors(hip_lib)


def test_dfe_against_a_large_numpy_sample(hip_lib):
    """A set of six mutants of one replicate (posterior sd of the population mean 0.3: `_contrast_cases.point_inputs`) at n_samples =
    BB_DFE_MAX_SAMPLES, at the multiple of 1 / 1024 nearest the median of their rb_mean: below_mean, between_sd^2 and within_sd^2
    against 400 000 independent numpy draws of the posterior pushed through the numpy restatement, each within 6 Monte-Carlo
    standard errors of the two estimates together."""
    from scipy.special import erfc
    sp, mu, om = cc.point_inputs()
    units, n, N = [10, 3, 17, 5, 24, 31], 400_000, dc.MAXN
    with pc._handle(hip_lib, sp, mu, om) as e:
        mean, sigma = e.posterior()
        x0 = cc.nearest(float(np.median(rc.rb(e, 1000, probs=())["rb_mean"][units])))
        got = dc.dfe(e, [units], [x0], N, seed=17, probs=())
    g = np.random.default_rng(0)
    T = sp.n_time[0]
    rows = [sp.offsets()["loglambda"][0] + (sp.n_neutral + m) * T for m in units]
    keep = sp.offsets()["s_pop"]
    cache = {}

    def draw(i):                                                    # every latent drawn once, independently; the set's loglambda rows
        if i in cache:                                              # are read twice (the normalisers, then their steps) and kept, as is sbar
            return cache[i]
        x = g.normal(mean[i], sigma[i], n)
        if any(lo <= i < lo + T for lo in rows) or keep[0] <= i < keep[1]:
            cache[i] = x
        return x

    _, m, sd, _ = rc.conditionals(sp, draw, n, mutants=units)
    v = (m[units] - x0) / sd[units] * dc.RSQRT2
    pl, pu = 0.5 * erfc(v), 0.5 * erfc(-v)
    L, V = pl.sum(axis=0) / len(units), (pl * pu).sum(axis=0) / len(units) ** 2
    B = (L - L.mean()) ** 2                                         # per-draw terms of between_sd^2 (the centring's own error is of second order)
    for name, dev, x in (("below_mean", got["below_mean"][0, 0], L), ("between_sd^2", got["between_sd"][0, 0] ** 2, B),
                         ("within_sd^2", got["within_sd"][0, 0] ** 2, V)):
        se = np.sqrt(x.var() / n + x.var() / N)
        print(name, dev, "numpy", x.mean(), "se", se)
        assert abs(dev - x.mean()) < 6 * se, name
    assert 0.2 < got["below_mean"][0, 0] < 0.8 and got["between_sd"][0, 0] > 0.0 and got["within_sd"][0, 0] > 0.0


QCOLS = [f"{side}_q{p}" for side in ("below", "above") for p in ("2.5", "50", "97.5")]
COLUMNS = ["rep", "env", "genotype", "group", "n_units", "x", "below_mean", "above_mean", "between_sd", "within_sd", "q_below_mean", "q_below_sd",
           "total_sd", "common_mode"] + QCOLS


def relations(out):
    """The relations of `_dfe_cases.check_relations` on the frame, set by set."""
    num = out.drop(columns=["rep", "env", "genotype", "group"]).to_numpy(dtype=np.float64)
    assert np.isfinite(num).all()
    assert np.abs(out["below_mean"] + out["above_mean"] - 1.0).max() <= 1e-12
    for _, s in out.groupby(["rep", "env", "genotype", "group"], dropna=False, sort=False):
        assert np.all(np.diff(s["x"]) > 0)
        assert np.all(np.diff(s["below_mean"]) >= 0) and np.all(np.diff(s["above_mean"]) <= 0)
    for side in ("below", "above"):
        assert (out[f"{side}_q2.5"] <= out[f"{side}_q50"]).all() and (out[f"{side}_q50"] <= out[f"{side}_q97.5"]).all()
    assert np.allclose(out["total_sd"], np.hypot(out["between_sd"], out["within_sd"]))
    assert np.allclose(out["common_mode"], out["between_sd"] / out["within_sd"])


def test_fitness_distribution_by_environment_end_to_end():
    """`stats.fitness_distribution(by="env")` on a multi-environment fit: one line per (environment, grid point) on the default
    grid.  At equal seed the draws are `fitness_marginals`': below_mean is the mean over the set's units of its p_neg at threshold
    x (the same tails, averaged the other way round); and with explicit draws (`chain=`) q_below_mean is their own ECDF.
    `fitness_marginals` returns moments of its draws, not the draws, so the ECDF of q's INTERNAL draws cannot be formed from it:
    the C_j of internal draws are held to their values by the goldens (q_below_mean, q_below_sd of `test_dfe_matches_golden`) and
    by `test_own_draws_equal_the_same_draws_passed_in`, through `Engine.dfe_rb`, not through `stats`."""
    import barbay_jl_amd as bb
    data = pd.read_csv(os.path.join(GOLD, "data003_multienv.csv"))
    model, cols = bb.model.multienv_fitness_normal, dict(env_col="env")
    df = bb.vi.advi(data=data, model=model, advi=bb.vi.ADVI(1, 50), verbose=False, seed=1, **cols)
    n = 300
    out = bb.stats.fitness_distribution(data, df, model=model, by="env", n_samples=n, seed=3, **cols)
    assert list(out.columns) == COLUMNS
    fm = bb.stats.fitness_marginals(data, df, model=model, n_samples=n, seed=3, probs=(), **cols)
    envs = list(dict.fromkeys(fm["env"]))
    fit = df[df["vartype"] == "bc_fitness"]
    grid = np.linspace((fit["mean"] - 3 * fit["std"]).min(), (fit["mean"] + 3 * fit["std"]).max(), 32)
    assert len(envs) >= 2 and len(out) == len(envs) * 32
    assert list(out["env"]) == [x for x in envs for _ in range(32)] and out["rep"].isna().all() and out["genotype"].isna().all() and out["group"].isna().all()
    assert np.array_equal(out["x"].to_numpy().reshape(len(envs), 32), np.tile(grid, (len(envs), 1)))
    assert (out["n_units"] == len(fm) // len(envs)).all()
    relations(out)
    for gi in (5, 16, 27):                                           # three thresholds: the marginals' own tails, averaged over the set
        at = bb.stats.fitness_marginals(data, df, model=model, n_samples=n, seed=3, probs=(), threshold=float(grid[gi]), **cols)
        for x, env in enumerate(envs):
            want = at["p_neg"][at["env"] == env].mean()
            assert abs(out["below_mean"][x * 32 + gi] - want) <= rc.TOL * want, (env, gi)
    z = np.random.default_rng(5).normal(df["mean"].to_numpy(), df["std"].to_numpy(), (n, len(df)))
    own = bb.stats.fitness_distribution(data, df, model=model, by="env", chain=z, **cols)
    s = z[:, np.flatnonzero((df["vartype"] == "bc_fitness").to_numpy())]      # [draws, units]: unit e + E m
    E = len(envs)
    for x in range(E):
        ecdf = np.array([(s[:, x::E] <= t).mean() for t in grid])
        assert np.abs(own["q_below_mean"].to_numpy()[x * 32:(x + 1) * 32] - ecdf).max() <= 1e-12
    print("by env: common_mode median", out["common_mode"].median(), "min", out["common_mode"].min(), "max", out["common_mode"].max())
    with pytest.raises(bb.BarBayError):
        bb.stats.fitness_distribution(data, df, model=model, by="genotype", **cols)                      # no genotypes
    with pytest.raises(bb.BarBayError):
        bb.stats.fitness_distribution(data, df, model=model, by="environment", **cols)                   # no such split


def test_fitness_distribution_of_user_classes_end_to_end():
    """`groups=` splits the library into user classes (mutants it does not name are left out), on a caller's grid; the errors of
    the entry point."""
    import barbay_jl_amd as bb
    data = pd.read_csv(os.path.join(GOLD, "data001_single.csv"))
    model = bb.model.fitness_normal
    df = bb.vi.advi(data=data, model=model, advi=bb.vi.ADVI(1, 50), verbose=False, seed=1)
    fm = bb.stats.fitness_marginals(data, df, model=model, n_samples=2, probs=())
    mutants = list(dict.fromkeys(fm["id"]))
    groups = {m: ("even" if i % 2 == 0 else "odd") for i, m in enumerate(mutants) if i % 5 != 4}
    grid = [-0.5, 0.0, 0.125, 1.0]
    kw = dict(model=model, n_samples=300, seed=3)
    out = bb.stats.fitness_distribution(data, df, by="all", groups=groups, grid=grid, **kw)
    assert list(out.columns) == COLUMNS and len(out) == 2 * len(grid)
    assert list(out["group"]) == ["even"] * 4 + ["odd"] * 4 and out["rep"].isna().all() and out["env"].isna().all()
    want = [sum(1 for v in groups.values() if v == k) for k in ("even", "odd")]
    assert list(out["n_units"]) == [want[0]] * 4 + [want[1]] * 4 and list(out["x"]) == grid * 2
    relations(out)
    per_rep = bb.stats.fitness_distribution(data, df, groups=groups, grid=grid, **kw)                    # by="rep_env": one replicate, no environments
    assert list(per_rep["rep"]) == ["R1"] * 8 and per_rep["env"].isna().all()
    pd.testing.assert_frame_equal(per_rep.drop(columns=["rep"]), out.drop(columns=["rep"]), check_exact=True)
    whole = bb.stats.fitness_distribution(data, df, by="all", **kw)
    assert len(whole) == 32 and (whole["n_units"] == len(mutants)).all() and whole["group"].isna().all()
    relations(whole)
    print("by class: common_mode", out["common_mode"].to_numpy())
    for bad in (dict(by="env"),                                                                          # a model without environments
                dict(by="genotype"),                                                                     # no genotype_col
                dict(by="class"),
                dict(groups={"no such barcode": "a"}),
                dict(groups={}),
                dict(grid=[0.5, 0.25]),
                dict(grid=[]),
                dict(grid=list(np.arange(65.0))),
                dict(grid=[0.0, np.nan])):
        with pytest.raises(bb.BarBayError):
            bb.stats.fitness_distribution(data, df, **kw, **bad)
