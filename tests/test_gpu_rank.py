"""bb_fitness_rank (posterior ranks and top-k membership of the units of sets, barbay.jl_amd/csrc/bb_rank.h) on the device: the
emulation's cases, a statistical check against independent numpy draws, and the user entry point `stats.fitness_ranking` end to end."""
import os

import numpy as np
import pandas as pd
import pytest

import _contrast_cases as cc
import _ppc_cases as pc
import _rank_cases as kc
import _rb_cases as rc

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_sorter_matches_numpy_on_planted_columns(hip_lib):
    kc.check_sorter(hip_lib)


def test_sorter_at_the_full_run_and_beyond(hip_lib):
    kc.check_sorter_large(hip_lib)


@pytest.mark.parametrize("n", kc.NS)
@pytest.mark.parametrize("case", kc.CASES)
def test_conditional_ranks_match_the_restatement(hip_lib, case, n):
    kc.check_conditional(hip_lib, case, n, "device")


def test_rank_sd_grows_with_the_shared_uncertainty(hip_lib):
    kc.check_point(hip_lib)


@pytest.mark.parametrize("case", ["fitness_chunk", "multienv_replicate"])
def test_independent_of_the_rest_of_the_call(hip_lib, case):
    kc.check_independent_of_the_rest_of_the_call(hip_lib, case)


def test_independent_of_launch_mode_and_repeatable(hip_lib):
    kc.check_launch_modes(hip_lib)


@pytest.mark.parametrize("case", ["fitness", "replicate_ragged", "genotype_regrouped"])
def test_group_handle_equals_single_device(hip_lib, case):
    kc.check_group_handle(hip_lib, case)


def test_buffer_reuse_across_calls_and_sizes(hip_lib):
    kc.check_buffer_reuse(hip_lib)


def test_handle_untouched(hip_lib):
    kc.check_handle_untouched(hip_lib)


@pytest.mark.parametrize("case", ["fitness", "genotype_regrouped", "multienv_replicate"])
def test_own_draws_equal_the_same_draws_passed_in(hip_lib, case):
    kc.check_internal_against_explicit_draws(hip_lib, case)


def test_nan_parameter_ranks_last_and_stays_in_its_sets(hip_lib):
    kc.check_nan_parameter(hip_lib)


def test_rank_errors(hip_lib):
    kc.check_errors(hip_lib)


def test_ranks_against_a_large_numpy_sample(hip_lib):
    """A set of six mutants of one replicate (posterior sd of the population mean 0.3: `_contrast_cases.point_inputs`) at n_samples =
    BB_RANK_MAX_SAMPLES: p_top[k = 2] and rank_mean of every unit against 400 000 independent numpy draws of the posterior pushed
    through the numpy restatement (the conditionals, then an independent normal per unit and draw), each within 6 Monte-Carlo
    standard errors of the two estimates together."""
    sp, mu, om = cc.point_inputs()
    units, n, N = [10, 3, 17, 5, 24, 31], 400_000, kc.MAXN
    with pc._handle(hip_lib, sp, mu, om) as e:
        mean, sigma = e.posterior()
        got = kc.rank(e, [units], N, seed=17, top=(2,), probs=())
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
    v = m[units] + sd[units] * g.standard_normal((len(units), n))
    r = kc.order_ranks(v)
    assert np.array_equal(got["n_units"], [len(units)])
    for x, u in enumerate(units):
        for name, dev, per_draw in (("p_top2", got["p_top"][x, 0], (r[x] < 2).astype(np.float64)), ("rank_mean", got["rank_mean"][x], r[x].astype(np.float64))):
            se = np.sqrt(per_draw.var() / n + per_draw.var() / N)
            print(f"unit {u:2d} {name:9s} device {dev:.4f} numpy {per_draw.mean():.4f} se {se:.4f}")
            assert abs(dev - per_draw.mean()) <= 6 * se, (u, name)               # (a unit that is never, or always, among the two fittest: 0 <= 0)
    assert 0.0 < np.median(got["p_top"][:, 0]) < 1.0 and abs(got["p_top"][:, 0].sum() - 2.0) < 1e-12


def frame_checks(out, top=(1, 10), probs=("2.5", "50", "97.5"), by=("rep", "env")):
    columns = ["id", "rep", "env", "genotype", "group", "n_units", "rank", "rank_mean", "rank_sd"] + [f"rank_q{p}" for p in probs] + [f"p_top{k}" for k in top]
    assert list(out.columns) == columns
    for _, s in out.groupby([c for c in by], dropna=False, sort=False):
        n = len(s)
        assert (s["n_units"] == n).all()
        assert sorted(s["rank"]) == list(range(1, n + 1))                                   # a permutation per set, 1-based
        assert np.array_equal(s["rank"].to_numpy()[np.argsort(s["rank_mean"].to_numpy(), kind="stable")], np.arange(1, n + 1))
        assert s["rank_mean"].min() >= 1.0 and s["rank_mean"].max() <= n
        assert abs(s["rank_mean"].sum() - n * (n + 1) / 2) <= 1e-9 * n * n                  # every draw's ranks are 1 .. n
        for k in top:
            assert abs(s[f"p_top{k}"].sum() - min(k, n)) <= 1e-9 * n
        assert (s[f"rank_q{probs[0]}"] <= s[f"rank_q{probs[-1]}"]).all() and s[f"rank_q{probs[0]}"].min() >= 1.0


def test_fitness_ranking_by_environment_end_to_end():
    """`stats.fitness_ranking(by="env")` on a multi-environment fit: one line per (environment, unit), the columns and their order,
    the 1-based convention, `rank` a permutation per set; with `chain=` and source="draws" the ranks are numpy's on the chain."""
    import barbay_jl_amd as bb
    data = pd.read_csv(os.path.join(GOLD, "data003_multienv.csv"))
    model, cols = bb.model.multienv_fitness_normal, dict(env_col="env")
    df = bb.vi.advi(data=data, model=model, advi=bb.vi.ADVI(1, 50), verbose=False, seed=1, **cols)
    n = 300
    out = bb.stats.fitness_ranking(data, df, model=model, by="env", n_samples=n, seed=3, **cols)
    fm = bb.stats.fitness_marginals(data, df, model=model, n_samples=2, seed=3, probs=(), **cols)
    envs = list(dict.fromkeys(fm["env"]))
    E = len(envs)
    assert E >= 2 and len(out) == len(fm)
    assert list(out["env"]) == [x for x in envs for _ in range(len(fm) // E)] and out["genotype"].isna().all() and out["group"].isna().all()
    for x, env in enumerate(envs):
        assert list(out["id"][out["env"] == env]) == list(fm["id"][fm["env"] == env])
    frame_checks(out, by=("env",))
    own = bb.stats.fitness_ranking(data, df, model=model, by="env", n_samples=n, seed=3, source="draws", **cols)
    frame_checks(own, by=("env",))
    print("by env: mean rank_sd conditional", out["rank_sd"].mean(), "draws", own["rank_sd"].mean())
    z = np.random.default_rng(5).normal(df["mean"].to_numpy(), df["std"].to_numpy(), (n, len(df)))
    z[:, np.flatnonzero((df["vartype"] == "bc_fitness").to_numpy())[:6]] = 0.125         # ties: the caller's order decides
    ch = bb.stats.fitness_ranking(data, df, model=model, by="env", chain=z, source="draws", top=(1, 3, 5), probs=(0.5,), **cols)
    frame_checks(ch, top=(1, 3, 5), probs=("50",), by=("env",))
    s = z[:, np.flatnonzero((df["vartype"] == "bc_fitness").to_numpy())]                 # [draws, units]: unit e + E m
    for x, env in enumerate(envs):
        r = kc.order_ranks(s[:, x::E].T)
        ref = kc.summaries(r, (1, 3, 5), (0.5,))
        got = ch[ch["env"] == env]
        assert np.array_equal(got["rank_mean"].to_numpy(), ref["rank_mean"] + 1.0)
        assert np.array_equal(got[["p_top1", "p_top3", "p_top5"]].to_numpy(), ref["p_top"])
        assert np.abs(got["rank_q50"].to_numpy() - (ref["quantiles"][:, 0] + 1.0)).max() <= 1e-12 * len(got)
        assert np.abs(got["rank_sd"].to_numpy() - ref["rank_sd"]).max() <= 1e-12 * len(got)
    with pytest.raises(bb.BarBayError):
        bb.stats.fitness_ranking(data, df, model=model, by="genotype", **cols)                           # no genotypes
    with pytest.raises(bb.BarBayError):
        bb.stats.fitness_ranking(data, df, model=model, by="environment", **cols)                        # no such split


def test_fitness_ranking_of_user_classes_end_to_end():
    """`groups=` splits the library into user classes (mutants it does not name are left out); the errors of the entry point."""
    import barbay_jl_amd as bb
    data = pd.read_csv(os.path.join(GOLD, "data001_single.csv"))
    model = bb.model.fitness_normal
    df = bb.vi.advi(data=data, model=model, advi=bb.vi.ADVI(1, 50), verbose=False, seed=1)
    fm = bb.stats.fitness_marginals(data, df, model=model, n_samples=2, probs=())
    mutants = list(dict.fromkeys(fm["id"]))
    groups = {m: ("even" if i % 2 == 0 else "odd") for i, m in enumerate(mutants) if i % 5 != 4}
    kw = dict(model=model, n_samples=300, seed=3)
    out = bb.stats.fitness_ranking(data, df, by="all", groups=groups, **kw)
    want = {k: [m for m in mutants if groups.get(m) == k] for k in ("even", "odd")}
    assert list(out["group"]) == ["even"] * len(want["even"]) + ["odd"] * len(want["odd"])
    assert list(out["id"]) == want["even"] + want["odd"] and (out["rep"] == "R1").all() and out["env"].isna().all() and out["genotype"].isna().all()
    frame_checks(out, by=("group",))
    per_rep = bb.stats.fitness_ranking(data, df, groups=groups, **kw)                                    # by="rep_env": one replicate, no environments
    pd.testing.assert_frame_equal(per_rep, out, check_exact=True)
    whole = bb.stats.fitness_ranking(data, df, by="all", top=(len(mutants), 10 * len(mutants)), probs=(), **kw)
    assert len(whole) == len(mutants) and (whole["n_units"] == len(mutants)).all() and whole["group"].isna().all()
    assert (whole[f"p_top{len(mutants)}"] == 1.0).all() and (whole[f"p_top{10 * len(mutants)}"] == 1.0).all()      # k = n and k > n
    assert sorted(whole["rank"]) == list(range(1, len(mutants) + 1))
    best = whole.sort_values("rank").iloc[0]
    print("fittest:", best["id"], "rank_mean", best["rank_mean"], "rank_sd", best["rank_sd"])
    for bad in (dict(by="env"),                                                                          # a model without environments
                dict(by="genotype"),                                                                     # no genotype_col
                dict(by="class"),
                dict(groups={"no such barcode": "a"}),
                dict(groups={}),
                dict(top=(0,)),
                dict(top=(1.5,)),
                dict(top=(2, 2)),
                dict(top=tuple(range(1, 10))),
                dict(source="both")):
        with pytest.raises(bb.BarBayError):
            bb.stats.fitness_ranking(data, df, **kw, **bad)
