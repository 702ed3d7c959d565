"""bb_loglambda_rb (Rao-Blackwellised loglambda marginals, barbay.jl_amd/csrc/bb_llrb.h) in the host emulation of the block
programs: the 50-digit goldens of tests/golden/make_loglambda_rb_golden.py and the restatement (tests/_loglambda_rb_cases.py), the
rule against `mpmath.quad` of the density, the identity against the literal oracle's gradient, rows, determinism, non-finite values
and errors."""
import pytest

import _loglambda_rb_cases as lc


def test_rule_against_quadrature_of_the_density():
    lc.check_truth()


@pytest.mark.parametrize("name", lc.emu_cases())
def test_marginals_match_golden(emu_lib, name):
    lc.check_golden(emu_lib, name, "emulation")


def test_two_kept_modes_match_golden(emu_lib):
    lc.check_bimodal(emu_lib, "emulation")


@pytest.mark.parametrize("name", lc.IDENTITY)
def test_derivative_at_the_draw_is_the_gradient_of_the_log_joint(emu_lib, name):
    lc.check_identity(emu_lib, name)


def test_rows_subset_equals_the_rows_of_the_full_call(emu_lib):
    lc.check_rows_subset(emu_lib)


def test_no_rows_means_every_row(emu_lib):
    lc.check_all_rows(emu_lib)


def test_independent_of_launch_mode_and_repeatable(emu_lib):
    lc.check_launch_modes(emu_lib)


@pytest.mark.parametrize("name", lc.GROUP_CASES)
def test_group_handle_equals_single_device(emu_lib, name):
    lc.check_group_handle(emu_lib, name)


def test_buffer_reuse_across_calls_and_sizes(emu_lib):
    lc.check_buffer_reuse(emu_lib)


def test_handle_untouched(emu_lib):
    lc.check_handle_untouched(emu_lib)


@pytest.mark.parametrize("name", ["genotype_regrouped", "multienv_replicate", "replicate_ragged_method", "fitness_matrix_prior"])
def test_own_draws_equal_the_same_draws_passed_in(emu_lib, name):
    lc.check_internal_against_explicit_draws(emu_lib, name)


def test_nan_stays_in_the_entries_that_read_it(emu_lib):
    lc.check_nan_stays(emu_lib)


def test_loglambda_rb_errors(emu_lib):
    lc.check_errors(emu_lib)
