"""The device-resident NUTS tree on the MI355X (barbay.jl_amd/csrc/bb_nuts.h): the cases of tests/_nuts_cases.py through the product
library, the full width of BB_HMC_MAX_WALKERS walkers, and mcmc.nuts_device end to end against the driver on a numpy stand-in."""
import pytest

import _nuts_cases as nc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", nc.NAMES)
def test_tree_against_host(hip_lib, name):
    nc.case_tree_against_host(hip_lib, name)


@pytest.mark.parametrize("name", nc.NAMES)
def test_walkers_are_independent_bitwise(hip_lib, name):
    nc.case_independence(hip_lib, name)


@pytest.mark.parametrize("name", nc.NAMES)
def test_nothing_else_moves(hip_lib, name):
    nc.case_state_untouched(hip_lib, name)


def test_full_width(hip_lib):
    nc.case_full_width(hip_lib)


def test_errors(hip_lib):
    nc.case_errors(hip_lib)


def test_end_to_end_against_stand_in(hip_lib):
    nc.case_end_to_end(hip_lib)


def test_sampler(hip_lib, monkeypatch):
    nc.case_sampler(hip_lib, monkeypatch)


@pytest.mark.parametrize("kind", list(nc.SAMPLER_KINDS))
def test_sampler_on_every_model_kind(hip_lib, kind):
    nc.case_sampler_kind(hip_lib, kind)
