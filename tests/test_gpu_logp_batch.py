"""bb_logdensity_grad_batch on the MI355X (barbay.jl_amd/csrc/bb_logp.h): the cases of tests/_logp_cases.py through the product
library, the full batch of BB_LOGP_MAX_BATCH points, and mcmc_sample(ensemble="batched") end to end."""
import pytest

import _logp_cases as lc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", lc.NAMES)
def test_batch_matches_oracle_and_single_call(hip_lib, name):
    lc.case_oracle(hip_lib, name)


@pytest.mark.parametrize("name", lc.NAMES)
def test_batch_points_are_independent_bitwise(hip_lib, name):
    lc.case_independence(hip_lib, name)


def test_full_batch(hip_lib):
    lc.case_full_batch(hip_lib)


@pytest.mark.parametrize("name", lc.NAMES)
def test_batch_leaves_state_untouched(hip_lib, name):
    lc.case_state_untouched(hip_lib, name)


def test_batch_errors(hip_lib):
    lc.case_errors(hip_lib)


def test_mcmc_batched_gpu(hip_lib):
    lc.case_mcmc_batched(hip_lib)
