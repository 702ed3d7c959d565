"""bb_fitness_rb (Rao-Blackwellised fitness marginals, barbay.jl_amd/csrc/bb_rb.h) in the host emulation of the block program:
the identity against the literal oracle's gradient, the 50-digit goldens of tests/golden/make_rb_golden.py and the numpy
restatement (tests/_rb_cases.py), determinism, non-finite values and errors."""
import pytest

import _ppc_cases as pc
import _rb_cases as rc


@pytest.mark.parametrize("name", rc.IDENTITY)
def test_conditional_matches_the_gradient_of_the_log_joint(emu_lib, name):
    rc.check_identity(emu_lib, name)


@pytest.mark.parametrize("name", sorted(rc.golden_cases()))
def test_parameters_stay_within_the_tails(name):
    rc.check_z_range(name)


@pytest.mark.parametrize("name", sorted(rc.golden_cases()))
def test_marginals_match_golden(emu_lib, name):
    rc.check_golden(emu_lib, name, "emulation")


def test_four_and_eight_quantiles_match_the_restatement(emu_lib):
    rc.check_many_quantiles(emu_lib)


def test_independent_of_launch_mode_and_repeatable(emu_lib):
    rc.check_launch_modes(emu_lib)


@pytest.mark.parametrize("name", pc.GROUP_CASES)
def test_group_handle_equals_single_device(emu_lib, name):
    rc.check_group_handle(emu_lib, name)


def test_buffer_reuse_across_calls_and_sizes(emu_lib):
    rc.check_buffer_reuse(emu_lib)


def test_handle_untouched(emu_lib):
    rc.check_handle_untouched(emu_lib)


@pytest.mark.parametrize("name", ["fitness", "genotype_regrouped", "multienv_replicate"])
def test_own_draws_equal_the_same_draws_passed_in(emu_lib, name):
    rc.check_internal_against_explicit_draws(emu_lib, name)


def test_nan_parameter_stays_in_its_units(emu_lib):
    rc.check_nan_parameter(emu_lib)


def test_rb_errors(emu_lib):
    rc.check_errors(emu_lib)
