"""bb_chain_summary (chain diagnostics, barbay.jl_amd/csrc/bb_chain.h) on the device: the emulation's cases and checks through
the product library, and the device against the emulation on the whole case list."""
import numpy as np
import pytest

import _chain_cases as cc
import _ppc_cases as pc
from conftest import make_engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(hip_lib):
    with make_engine(pc.spec("fitness"), hip_lib, seed=2) as e:
        yield e


@pytest.fixture(scope="module")
def emu_eng(emu_lib):
    with make_engine(pc.spec("fitness"), emu_lib, seed=2) as e:
        yield e


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_chain_summary_matches_restatement_and_emulation(eng, emu_eng, name):
    got = cc.check_case(eng, name, "MI355X")
    ref = emu_eng.chain_summary(cc.chain_of(name), cc.PROBS, **cc.CASES[name][2])
    tol = cc.references(name)[2]
    for k in cc.STATS:
        assert cc.rel_err(got[k], ref[k]) <= tol[k], (name, k, cc.rel_err(got[k], ref[k]), tol[k])
    assert np.array_equal(got["n_lags"], ref["n_lags"])
    assert np.array_equal(got["quantiles"].view(np.uint64), ref["quantiles"].view(np.uint64))


def test_special_columns(eng):
    cc.check_special_columns(eng)


def test_placement_and_slabs_are_bit_identical(eng):
    cc.check_placement(eng)


def test_null_outputs_and_edge_probabilities(eng):
    cc.check_null_outputs(eng)


def test_errors(eng):
    cc.check_errors(eng)


def test_handle_untouched(hip_lib):
    cc.check_handle_untouched(hip_lib)


def test_repeatable_and_grid_independent(eng):
    """More columns than one wave of workgroups: the same column everywhere gives the same bits, twice."""
    v = cc.ar1(np.random.default_rng(41), 4, 250, 1, 0.8)
    x = np.ascontiguousarray(np.repeat(v, 3000, axis=2))
    a = eng.chain_summary(x, cc.PROBS)
    b = eng.chain_summary(x, cc.PROBS, slab_cols=777)
    assert cc.same_bits(a, b)
    for k, val in a.items():
        assert np.all(val.view(np.uint8).reshape(3000, -1) == val.view(np.uint8).reshape(3000, -1)[0]), k
