"""bb_theta_rb (Rao-Blackwellised hyper-fitness marginals, barbay.jl_amd/csrc/bb_rb.h) in the host emulation of the block
programs: the identity against the literal oracle's gradient, the 50-digit goldens of tests/golden/make_theta_rb_golden.py and the
numpy restatement (tests/_theta_rb_cases.py), the chunk rule, determinism, non-finite values and errors."""
import pytest

import _theta_rb_cases as tc


@pytest.mark.parametrize("name", tc.IDENTITY)
def test_conditional_matches_the_gradient_of_the_log_joint(emu_lib, name):
    tc.check_identity(emu_lib, name)


@pytest.mark.parametrize("name", sorted(tc.golden_cases()))
def test_thresholds_stay_within_the_tails(name):
    tc.check_z_range(name)


@pytest.mark.parametrize("name", sorted(tc.golden_cases()))
def test_marginals_match_golden(emu_lib, name):
    tc.check_golden(emu_lib, name, "emulation")


def test_members_are_summed_by_the_chunk_rule_whatever_the_internal_order(emu_lib):
    tc.check_chunk_rule(emu_lib, "emulation")


def test_independent_of_launch_mode_and_repeatable(emu_lib):
    tc.check_launch_modes(emu_lib)


@pytest.mark.parametrize("name", tc.GROUP_CASES)
def test_group_handle_equals_single_device(emu_lib, name):
    tc.check_group_handle(emu_lib, name)


def test_buffer_reuse_across_calls_and_sizes(emu_lib):
    tc.check_buffer_reuse(emu_lib)


def test_handle_untouched(emu_lib):
    tc.check_handle_untouched(emu_lib)


@pytest.mark.parametrize("name", ["genotype_regrouped", "multienv_replicate"])
def test_own_draws_equal_the_same_draws_passed_in(emu_lib, name):
    tc.check_internal_against_explicit_draws(emu_lib, name)


def test_nan_parameter_stays_in_its_group(emu_lib):
    tc.check_nan_parameter(emu_lib)


def test_nan_in_a_member_without_steps_changes_nothing(emu_lib):
    tc.check_nan_in_a_member_without_steps(emu_lib)


def test_theta_rb_errors(emu_lib):
    tc.check_errors(emu_lib)
