"""bb_logsigma_rb (Rao-Blackwellised noise-scale marginals, barbay.jl_amd/csrc/bb_lsrb.h) in the host emulation of the block
programs: the 50-digit goldens of tests/golden/make_logsigma_rb_golden.py and the numpy restatement (tests/_logsigma_rb_cases.py),
the rule against `mpmath.quad` of the density, the identity against the literal oracle's gradient, the prior-only entries,
determinism, non-finite values and errors."""
import pytest

import _logsigma_rb_cases as lc


def test_rule_against_quadrature_of_the_density():
    lc.check_truth()


@pytest.mark.parametrize("name", lc.emu_cases())
def test_marginals_match_golden(emu_lib, name):
    lc.check_golden(emu_lib, name, "emulation")


@pytest.mark.parametrize("name", lc.IDENTITY)
def test_gradient_of_the_log_joint_vanishes_at_the_modes(emu_lib, name):
    lc.check_identity(emu_lib, name)


def test_prior_only_entries(emu_lib):
    lc.check_prior_only(emu_lib)


def test_independent_of_launch_mode_and_repeatable(emu_lib):
    lc.check_launch_modes(emu_lib)


@pytest.mark.parametrize("name", lc.GROUP_CASES)
def test_group_handle_equals_single_device(emu_lib, name):
    lc.check_group_handle(emu_lib, name)


def test_buffer_reuse_across_calls_sizes_and_blocks(emu_lib):
    lc.check_buffer_reuse(emu_lib)


def test_handle_untouched(emu_lib):
    lc.check_handle_untouched(emu_lib)


@pytest.mark.parametrize("name", ["genotype_matrix_prior", "multienv_replicate", "replicate_ragged_method"])
def test_own_draws_equal_the_same_draws_passed_in(emu_lib, name):
    lc.check_internal_against_explicit_draws(emu_lib, name)


def test_nan_stays_in_its_entries(emu_lib):
    lc.check_nan_stays(emu_lib)


def test_four_and_eight_quantiles(emu_lib):
    lc.check_more_quantiles(emu_lib, "emulation")


def test_logsigma_rb_errors(emu_lib):
    lc.check_errors(emu_lib)
