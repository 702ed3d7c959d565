"""bb_popmean_rb (Rao-Blackwellised population-mean fitness marginals, barbay.jl_amd/csrc/bb_rb.h) in the host emulation of the
block programs: the identity against the literal oracle's gradient, the 50-digit goldens of tests/golden/make_pop_rb_golden.py and
the numpy restatement (tests/_pop_rb_cases.py), the chunk rule, determinism, non-finite values and errors."""
import pytest

import _pop_rb_cases as qc


@pytest.mark.parametrize("name", qc.IDENTITY)
def test_conditional_matches_the_gradient_of_the_log_joint(emu_lib, name):
    qc.check_identity(emu_lib, name)


@pytest.mark.parametrize("name", sorted(qc.golden_cases()))
def test_thresholds_stay_within_the_tails(name):
    qc.check_z_range(name)


@pytest.mark.parametrize("name", sorted(qc.golden_cases()))
def test_marginals_match_golden(emu_lib, name):
    qc.check_golden(emu_lib, name, "emulation")


def test_members_are_summed_by_the_chunk_rule(emu_lib):
    qc.check_chunk_rule(emu_lib, "emulation")


def test_independent_of_launch_mode_and_repeatable(emu_lib):
    qc.check_launch_modes(emu_lib)


@pytest.mark.parametrize("name", qc.GROUP_CASES)
def test_group_handle_equals_single_device(emu_lib, name):
    qc.check_group_handle(emu_lib, name)


def test_buffer_reuse_across_calls_and_sizes(emu_lib):
    qc.check_buffer_reuse(emu_lib)


def test_handle_untouched(emu_lib):
    qc.check_handle_untouched(emu_lib)


@pytest.mark.parametrize("name", ["genotype_regrouped", "multienv_replicate", "replicate_ragged_method"])
def test_own_draws_equal_the_same_draws_passed_in(emu_lib, name):
    qc.check_internal_against_explicit_draws(emu_lib, name)


def test_nan_in_its_own_mean_leaves_the_conditional_alone(emu_lib):
    qc.check_nan_in_own_mean(emu_lib)


def test_nan_in_a_mutant_stays_in_its_replicate_and_environment(emu_lib):
    qc.check_nan_in_a_mutant(emu_lib)


def test_popmean_rb_errors(emu_lib):
    qc.check_errors(emu_lib)
