"""bb_ppc_loo (PSIS leave-one-out scores per cell and per barcode, barbay.jl_amd/csrc/bb_loo.h) on the device: the emulation's cases,
determinism across launch modes and calls, the closed form against an independent numpy sample, and the user entry points end to
end."""
import os

import numpy as np
import pandas as pd
import pytest

import _loo_cases as lc
import _ppc_cases as pc

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("name", sorted(lc.golden_cases()))
def test_loo_matches_golden(hip_lib, name):
    lc.check_golden(hip_lib, name, "device")


def test_lpd_shares_the_bytes_of_the_score(hip_lib):
    lc.check_shared_bytes(hip_lib)


def test_unsmoothed_sizes(hip_lib):
    lc.check_unsmoothed(hip_lib)


def test_zero_counts_empty_rows_and_one_step_rows(hip_lib):
    lc.check_zero_counts(hip_lib)


def test_nan_parameter_stays_in_its_rows(hip_lib):
    lc.check_nan_parameter(hip_lib)


def test_loo_errors_and_limits(hip_lib):
    lc.check_errors(hip_lib)


def test_buffer_reuse_across_calls_and_sizes(hip_lib):
    lc.check_buffer_reuse(hip_lib)


@pytest.mark.parametrize("name", pc.GROUP_CASES)
def test_group_handle_equals_single_device(hip_lib, name):
    lc.check_group_handle(hip_lib, name)


def test_handle_untouched(hip_lib):
    lc.check_handle_untouched(hip_lib)


def test_independent_of_launch_mode_and_repeatable(hip_lib):
    lc.check_repeatable(hip_lib, modes=(1, 0))


def test_closed_form(hip_lib):
    lc.check_closed_form(hip_lib)


def test_loo_end_to_end_and_compare():
    """The frame of `stats.logfreq_ratio_loo` on a fitted fixture; a fit compared with itself gives 0 +- 0; a barcode whose counts are
    changed after the fit has the lowest elpd_loo and drives the comparison; two fits over different rows raise."""
    import barbay_jl_amd as bb
    data = pd.read_csv(os.path.join(GOLD, "data001_single.csv"))
    df = bb.vi.advi(data=data, model=bb.model.fitness_normal, advi=bb.vi.ADVI(1, 3000), verbose=False, seed=1)
    out = bb.stats.logfreq_ratio_loo(data, df, model=bb.model.fitness_normal, n_samples=500, seed=3)
    assert list(out.columns) == ["id", "neutral", "rep", "elpd_loo", "p_loo", "khat", "n_eff", "khat_max_cell", "n_scored", "flag"]
    assert len(out) == data["barcode"].nunique() and set(out["id"]) == set(data["barcode"])
    sc_ = bb.stats.logfreq_ratio_ppc_scores(data, df, model=bb.model.fitness_normal, n_samples=500, seed=3)
    assert list(out["id"]) == list(sc_.groupby(["rep", "id"], sort=False)["id"].first())
    ok = out["n_scored"] > 0
    assert ok.all() and np.isfinite(out[["elpd_loo", "p_loo", "n_eff"]].to_numpy()).all() and (out["n_eff"] <= 500 * (1 + 1e-12)).all()
    assert (out["p_loo"] > -1e-9).all()                                        # leave-one-out never beats in-sample
    thr = min(1.0 - 1.0 / np.log10(500), 0.7)
    assert out.attrs["khat_threshold"] == thr and list(out["flag"]) == list(out["khat"] > thr)
    assert out.attrs["n_flagged"] == int(out["flag"].sum())
    assert np.isclose(out.attrs["elpd_loo"], out["elpd_loo"].sum(), rtol=1e-14)
    assert np.isclose(out.attrs["se"], np.sqrt(len(out) * out["elpd_loo"].var(ddof=1)), rtol=1e-12)
    same = bb.stats.loo_compare(out, out)
    assert same["elpd_diff"] == 0.0 and same["se_diff"] == 0.0 and same["n"] == len(out)

    bad = sorted(data.loc[~data["neutral"], "barcode"].unique())[4]
    d2 = data.copy()
    sel = d2["barcode"] == bad
    fac = np.where(d2.loc[sel, "time"].to_numpy() % 2 == 0, 30.0, 1.0 / 30.0)
    d2.loc[sel, "count"] = np.maximum(1, np.round(d2.loc[sel, "count"].to_numpy() * fac)).astype(np.int64)
    out2 = bb.stats.logfreq_ratio_loo(d2, df, model=bb.model.fitness_normal, n_samples=500, seed=3)
    mut = out2[~out2["neutral"]].sort_values("elpd_loo")
    assert mut["id"].iloc[0] == bad, mut.head()
    cmp_ = bb.stats.loo_compare(out, out2)
    assert cmp_["rows"]["id"].iloc[0] == bad and cmp_["se_diff"] > 0
    with pytest.raises(bb.BarBayError):
        bb.stats.loo_compare(out, out2.iloc[1:])
    with pytest.raises(RuntimeError, match="error -4"):
        bb.stats.logfreq_ratio_loo(data, df, model=bb.model.fitness_normal, n_samples=8193)
