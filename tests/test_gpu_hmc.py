"""The device-resident HMC session on the MI355X (barbay.jl_amd/csrc/bb_hmc.h): the cases of tests/_hmc_cases.py through the product
library, the full width of BB_HMC_MAX_WALKERS walkers, and mcmc_sample(sampler="hmc") against the default sampler end to end."""
import pytest

import _hmc_cases as hc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", hc.NAMES)
def test_transition_against_host(hip_lib, name):
    hc.case_transition_against_host(hip_lib, name)


@pytest.mark.parametrize("name", hc.NAMES)
def test_walkers_are_independent_bitwise(hip_lib, name):
    hc.case_independence(hip_lib, name)


@pytest.mark.parametrize("name", hc.NAMES)
def test_session_leaves_state_untouched(hip_lib, name):
    hc.case_state_untouched(hip_lib, name)


def test_full_width(hip_lib):
    hc.case_full_width(hip_lib)


def test_errors(hip_lib):
    hc.case_errors(hip_lib)


def test_sampler_agrees_with_nuts(hip_lib):
    hc.case_sampler_agrees_with_nuts(hip_lib)
