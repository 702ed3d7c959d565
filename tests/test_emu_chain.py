"""bb_chain_summary (chain diagnostics, barbay.jl_amd/csrc/bb_chain.h) in the host emulation of the block programs, against the
numpy restatement of the header's formulas (tests/_chain_cases.py)."""
import numpy as np
import pytest

import _chain_cases as cc
import _ppc_cases as pc
from barbay_jl_amd import _capi
from conftest import make_engine


@pytest.fixture(scope="module")
def eng(emu_lib):
    with make_engine(pc.spec("fitness"), emu_lib, seed=2) as e:
        yield e


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_chain_summary_matches_restatement(eng, name):
    cc.check_case(eng, name, "emulation")


def test_cases_show_what_they_are_for():
    """The restatement itself: the AR(0.95) case truncates beyond the library's first lag batch, the antithetic case meets the
    log10 cap, the lag bound ends the trend's sum, the shifted chains have a large R-hat."""
    ld = {n: cc.references(n)[1] for n in ("w3_n400_ar95", "w2_n200_arneg", "w1_n300_trend", "w1_n300_trend_lag20", "w4_n200_means")}
    assert ld["w3_n400_ar95"]["n_lags"].min() > _capi.BB_CHAIN_LAG_BATCH
    ess = ld["w2_n200_arneg"]["ess"]
    assert np.all(ess > 400) and np.sum(ess == 400 * np.log10(np.longdouble(400))) >= 2 and np.sum(ess < 1040) >= 1
    assert np.all(ld["w1_n300_trend_lag20"]["n_lags"] == 20) and np.all(ld["w1_n300_trend"]["n_lags"] > 20)
    assert ld["w4_n200_means"]["rhat"].min() > 1.2


def test_special_columns(eng):
    cc.check_special_columns(eng)


def test_placement_and_slabs_are_bit_identical(eng):
    cc.check_placement(eng)


def test_null_outputs_and_edge_probabilities(eng):
    cc.check_null_outputs(eng)


def test_errors(eng):
    cc.check_errors(eng)


def test_handle_untouched(emu_lib):
    cc.check_handle_untouched(emu_lib)


def test_one_chain_as_a_matrix(eng):
    x = cc.chain_of("w1_n300_trend")
    assert cc.same_bits(eng.chain_summary(x[0]), eng.chain_summary(x))
