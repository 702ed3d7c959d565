"""bb_ppc_score (predictive log score and PIT per barcode, barbay.jl_amd/csrc/bb_score.h) on the device: the emulation's cases,
determinism across launch modes and calls, a statistical check against independent numpy draws, and the user entry point end to end."""
import os

import numpy as np
import pandas as pd
import pytest

import _ppc_cases as pc
import _score_cases as sc

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("name", sorted(sc.golden_cases()))
def test_scores_match_golden(hip_lib, name):
    sc.check_golden(hip_lib, name, "device")


def test_zero_counts_are_unscored(hip_lib):
    sc.check_zero_counts(hip_lib)


def test_nan_parameter_stays_in_its_rows(hip_lib):
    sc.check_nan_parameter(hip_lib)


def test_score_errors(hip_lib):
    sc.check_errors(hip_lib)


def test_buffer_reuse_across_calls_and_sizes(hip_lib):
    sc.check_buffer_reuse(hip_lib)


@pytest.mark.parametrize("name", pc.GROUP_CASES)
def test_group_handle_equals_single_device(hip_lib, name):
    sc.check_group_handle(hip_lib, name)


def test_handle_untouched(hip_lib):
    sc.check_handle_untouched(hip_lib)


def test_independent_of_launch_mode_and_repeatable(hip_lib):
    import barbay_jl_amd as bb
    sp, mu, om = sc.inputs("replicate_ragged")
    out = []
    for mode in (1, 0):
        with bb.Engine(sp.kind, sp.counts, sp.n_neutral, sp.n_bc, seed=4, launch_mode=mode, _lib=hip_lib) as e:
            e.set_params(mu, om)
            out.append(e.ppc_score(n_samples=500, seed=2))
            out.append(e.ppc_score(n_samples=500, seed=2))
    assert all(sc.same_bytes(out[0], o) for o in out[1:])


def test_pit_against_a_large_numpy_sample(hip_lib):
    """One mutant cell's pit at n_samples = 16384 against 400 000 independent numpy draws of the parameters, within 6 Monte-Carlo
    standard errors of the two estimates together."""
    from scipy.special import erfc
    sp, mu, om = sc.inputs("fitness")
    off = sp.offsets()
    m, t = 22, 2                                                    # (not a pushed mutant: a pit well inside (0, 1))
    row = sp.n_neutral + m
    with pc._handle(hip_lib, sp, mu, om) as e:
        mean, sigma = e.posterior()
        got = e.ppc_score(n_samples=16384, seed=17)
    y, pit = got["observed"][row, t], got["pit"][row, t]
    assert 0.02 < pit < 0.98
    g = np.random.default_rng(0)
    n = 400_000

    def draw(i):
        return g.normal(mean[i], sigma[i], n)

    z = (y - (draw(off["s_bc"][0] + m) - draw(off["s_pop"][0] + t))) / np.exp(draw(off["logsigma_bc"][0] + m))
    p = 0.5 * erfc(-z / np.sqrt(2.0))
    se = np.sqrt(p.var() / n + p.var() / 16384)
    print("pit", pit, "numpy", p.mean(), "se", se)
    assert abs(pit - p.mean()) < 6 * se


def _fit(data):
    import barbay_jl_amd as bb
    return bb.vi.advi(data=data, model=bb.model.fitness_normal, advi=bb.vi.ADVI(1, 3000), verbose=False, seed=1)


def test_scores_end_to_end_and_planted_misfit_ranks_first():
    """The frame of `stats.logfreq_ratio_ppc_scores`; a barcode whose counts are changed after the fit (up and down by 30x at
    alternate time points) has the lowest row_lpd and the smallest min(pit, pit_upper)."""
    import barbay_jl_amd as bb
    data = pd.read_csv(os.path.join(GOLD, "data001_single.csv"))
    df = _fit(data)
    out = bb.stats.logfreq_ratio_ppc_scores(data, df, model=bb.model.fitness_normal, n_samples=500, seed=3)
    assert list(out.columns) == ["id", "neutral", "rep", "env", "time", "observed", "pred_mean", "pred_sd", "lpd", "p_waic", "pit",
                                 "pit_upper", "row_lpd", "n_scored"]
    assert len(out) == data["barcode"].nunique() * (data["time"].nunique() - 1)
    assert set(out["id"]) == set(data["barcode"]) and out["neutral"].sum() == data.loc[data["neutral"], "barcode"].nunique() * (data["time"].nunique() - 1)
    sc_ = out.dropna(subset=["observed"])
    assert np.isfinite(sc_[["pred_mean", "pred_sd", "lpd", "p_waic", "pit", "pit_upper"]].to_numpy()).all()
    assert np.allclose(sc_["pit"] + sc_["pit_upper"], 1.0, atol=1e-12) and (sc_["pred_sd"] > 0).all()
    h = bb.stats.pit_histogram(out, bins=10)
    assert h["neutral"].sum() + h["mutant"].sum() == len(sc_)
    with pytest.raises(bb.BarBayError):
        bb.stats.logfreq_ratio_ppc_scores(data, df.iloc[3:], model=bb.model.fitness_normal)

    bad = sorted(data.loc[~data["neutral"], "barcode"].unique())[4]
    d2 = data.copy()
    sel = d2["barcode"] == bad
    fac = np.where(d2.loc[sel, "time"].to_numpy() % 2 == 0, 30.0, 1.0 / 30.0)
    d2.loc[sel, "count"] = np.maximum(1, np.round(d2.loc[sel, "count"].to_numpy() * fac)).astype(np.int64)
    out2 = bb.stats.logfreq_ratio_ppc_scores(d2, df, model=bb.model.fitness_normal, n_samples=1000)
    mut = out2[~out2["neutral"]]
    per = mut.groupby("id")["row_lpd"].first().sort_values()
    assert per.index[0] == bad and per.iloc[0] < per.iloc[1], per.head()
    tail = np.minimum(mut["pit"], mut["pit_upper"]).groupby(mut["id"]).min().sort_values()
    assert tail.index[0] == bad, tail.head()
