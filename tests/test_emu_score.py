"""bb_ppc_score (predictive log score and PIT per barcode, barbay.jl_amd/csrc/bb_score.h) in the host emulation of the block
program, against the 50-digit goldens of tests/golden/make_score_golden.py and the numpy restatement (tests/_score_cases.py)."""
import numpy as np
import pandas as pd
import pytest

import _ppc_cases as pc
import _score_cases as sc


@pytest.mark.parametrize("name", sorted(sc.golden_cases()))
def test_parameters_reach_the_tails_and_not_beyond(name):
    sc.check_z_range(name)


@pytest.mark.parametrize("name", sorted(sc.golden_cases()))
def test_scores_match_golden(emu_lib, name):
    sc.check_golden(emu_lib, name, "emulation")


def test_zero_counts_are_unscored(emu_lib):
    sc.check_zero_counts(emu_lib)


def test_nan_parameter_stays_in_its_rows(emu_lib):
    sc.check_nan_parameter(emu_lib)


def test_score_errors(emu_lib):
    sc.check_errors(emu_lib)


def test_buffer_reuse_across_calls_and_sizes(emu_lib):
    sc.check_buffer_reuse(emu_lib)


@pytest.mark.parametrize("name", pc.GROUP_CASES)
def test_group_handle_equals_single_device(emu_lib, name):
    sc.check_group_handle(emu_lib, name)


def test_handle_untouched(emu_lib):
    sc.check_handle_untouched(emu_lib)


def test_shares_the_draws_of_the_bands(emu_lib):
    """At equal seed pred_mean is the mean of the very draws bb_ppc_bands samples from: with one predictive draw per sample and a
    tiny predictive sd the band's median column is the draws' own, so its q = 1 band brackets pred_mean tightly."""
    sp, mu, om = sc.inputs("fitness")
    mu = mu.copy()
    mu[slice(*sp.offsets()["logsigma_bc"])] = -40.0
    with pc._handle(emu_lib, sp, mu, om) as e:
        got = e.ppc_score(n_samples=111, seed=sc.SEED)
        bands, _ = e.ppc_bands([1.0], n_samples=111, n_ppc=1, seed=sc.SEED, outside=False)
    rows = sp.n_neutral + np.arange(sp.n_bc)                       # score rows of the mutants; their band rows: 1 + m
    pm, lo, hi = got["pred_mean"][rows], bands[1:, :, 0, 0], bands[1:, :, 0, 1]
    ok = ~np.isnan(pm)
    assert ok.any() and np.all(lo[ok] <= pm[ok]) and np.all(pm[ok] <= hi[ok]) and np.all(hi[ok] - lo[ok] < 0.5)


def test_pit_histogram():
    import barbay_jl_amd as bb
    df = pd.DataFrame({"pit": [0.0, 0.05, 0.95, 1.0, np.nan, 0.5, 0.31], "neutral": [True, True, False, False, True, False, True]})
    h = bb.stats.pit_histogram(df, bins=10)
    assert list(h.columns) == ["lower", "upper", "neutral", "mutant"] and len(h) == 10
    assert list(h["neutral"]) == [2, 0, 0, 1, 0, 0, 0, 0, 0, 0] and list(h["mutant"]) == [0, 0, 0, 0, 0, 1, 0, 0, 0, 2]
    assert bb.stats.pit_histogram(df, bins=2)["neutral"].sum() == 3
    with pytest.raises(bb.BarBayError):
        bb.stats.pit_histogram(df, bins=0)
