"""The HMC session's streaming moments and metric on the MI355X (barbay.jl_amd/csrc/bb_hmc_accum.h): the cases of
tests/_hmc_accum_cases.py through the product library."""
import pytest

import _hmc_accum_cases as ac

pytestmark = pytest.mark.gpu


def test_shapes_cover_the_three_kinds(hip_lib):
    ac.check_kinds(hip_lib)


@pytest.mark.parametrize("name", ac.NAMES)
def test_accumulators_bitwise(hip_lib, name):
    ac.case_accumulators(hip_lib, name)


@pytest.mark.parametrize("name", ac.NAMES)
def test_statistics(hip_lib, name):
    ac.case_statistics(hip_lib, name)


@pytest.mark.parametrize("name", ac.NAMES)
def test_rows_are_independent_bitwise(hip_lib, name):
    ac.case_independence(hip_lib, name)


@pytest.mark.parametrize("name", ac.NAMES)
def test_nothing_disturbed_bitwise(hip_lib, name):
    ac.case_nothing_disturbed(hip_lib, name)


@pytest.mark.parametrize("name", ac.NAMES)
def test_metric(hip_lib, name):
    ac.case_metric(hip_lib, name)


def test_full_width(hip_lib):
    ac.case_full_width(hip_lib)


def test_errors_and_degenerate_columns(hip_lib):
    ac.case_errors(hip_lib)


def test_end_to_end(hip_lib):
    ac.case_end_to_end(hip_lib)
