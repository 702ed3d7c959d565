"""bb_logtau_rb (Rao-Blackwellised logtau marginals, barbay.jl_amd/csrc/bb_ltrb.h) in the host emulation of the block programs: the
rule against `mpmath.quad` of the density, the collapsed conditional against the quadrature over theta_tilde, the condition on the
inputs (a good part of the draws has two modes), the 50-digit goldens of tests/golden/make_logtau_rb_golden.py and the numpy
restatement (tests/_logtau_rb_cases.py), the identity against the literal oracle's gradient, the prior-only entries, determinism,
non-finite values and errors."""
import pytest

import _logtau_rb_cases as tc


def test_rule_against_quadrature_of_the_density():
    tc.check_truth()


def test_collapsed_conditional_is_the_integral_over_theta_tilde():
    tc.check_collapsed_identity()


def test_inputs_have_entries_with_a_mixed_number_of_modes():
    tc.check_bimodal_inputs()


@pytest.mark.parametrize("name", tc.emu_cases())
def test_marginals_match_golden(emu_lib, name):
    tc.check_golden(emu_lib, name, "emulation")


@pytest.mark.parametrize("name", tc.IDENTITY)
def test_gradient_of_the_log_joint_vanishes_at_the_modes(emu_lib, name):
    tc.check_identity(emu_lib, name)


def test_prior_only_entries(emu_lib):
    tc.check_prior_only(emu_lib)


def test_independent_of_launch_mode_and_repeatable(emu_lib):
    tc.check_launch_modes(emu_lib)


@pytest.mark.parametrize("name", tc.GROUP_CASES)
def test_group_handle_equals_single_device(emu_lib, name):
    tc.check_group_handle(emu_lib, name)


def test_buffer_reuse_across_calls_sizes_and_modes(emu_lib):
    tc.check_buffer_reuse(emu_lib)


def test_handle_untouched(emu_lib):
    tc.check_handle_untouched(emu_lib)


@pytest.mark.parametrize("name", ["genotype_matrix_prior", "multienv_replicate", "replicate_ragged_method"])
def test_own_draws_equal_the_same_draws_passed_in(emu_lib, name):
    tc.check_internal_against_explicit_draws(emu_lib, name)


def test_nan_stays_in_its_entries(emu_lib):
    tc.check_nan_stays(emu_lib)


def test_four_and_eight_quantiles(emu_lib):
    tc.check_more_quantiles(emu_lib, "emulation")


def test_logtau_rb_errors(emu_lib):
    tc.check_errors(emu_lib)


def test_vectorised_restatement_equals_the_per_draw_one():
    tc.check_many()
