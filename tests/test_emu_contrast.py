"""bb_contrast_rb (Rao-Blackwellised fitness contrasts, barbay.jl_amd/csrc/bb_contrast.h) in the host emulation of the block
program: one-term contrasts against the goldens of bb_fitness_rb and bb_theta_rb, composition at explicit draws, the 50-digit
goldens of tests/golden/make_contrast_golden.py and the numpy restatement (tests/_contrast_cases.py), the cancellation the call
exists for, determinism, non-finite values and errors."""
import pytest

import _contrast_cases as cc


@pytest.mark.parametrize("space,name", cc.single_term_cases())
def test_one_term_contrasts_match_the_marginals_goldens(emu_lib, space, name):
    cc.check_single_term(emu_lib, space, name, "emulation")


@pytest.mark.parametrize("space,case", cc.SPACE_CASES)
def test_contrast_composes_the_conditionals_of_its_terms(emu_lib, space, case):
    cc.check_composition(emu_lib, space, case)


@pytest.mark.parametrize("name", sorted(cc.golden_cases()))
def test_thresholds_stay_within_the_tails(name):
    cc.check_z_range(name)


@pytest.mark.parametrize("name", sorted(cc.golden_cases()))
def test_contrasts_match_golden(emu_lib, name):
    cc.check_golden(emu_lib, name, "emulation")


def test_restated_difference_is_sharper_and_sum_wider_than_the_marginals_say():
    cc.check_point_restated()


def test_difference_is_sharper_and_sum_wider_than_the_marginals_say(emu_lib):
    cc.check_point(emu_lib)


@pytest.mark.parametrize("space,case", [("fitness", "multienv"), ("fitness", "fitness_chunk"), ("theta", "genotype_chunks"), ("theta", "multienv_replicate")])
def test_independent_of_the_other_contrasts(emu_lib, space, case):
    cc.check_independent_of_the_other_contrasts(emu_lib, space, case)


def test_independent_of_launch_mode_and_repeatable(emu_lib):
    cc.check_launch_modes(emu_lib)


@pytest.mark.parametrize("space,case", [("fitness", "fitness"), ("fitness", "replicate_ragged"), ("theta", "genotype_regrouped")])
def test_group_handle_equals_single_device(emu_lib, space, case):
    cc.check_group_handle(emu_lib, space, case)


def test_buffer_reuse_across_calls_and_sizes(emu_lib):
    cc.check_buffer_reuse(emu_lib)


def test_handle_untouched(emu_lib):
    cc.check_handle_untouched(emu_lib)


@pytest.mark.parametrize("space,case", [("fitness", "fitness"), ("fitness", "genotype_regrouped"), ("theta", "multienv_replicate")])
def test_own_draws_equal_the_same_draws_passed_in(emu_lib, space, case):
    cc.check_internal_against_explicit_draws(emu_lib, space, case)


def test_nan_parameter_stays_in_its_contrasts(emu_lib):
    cc.check_nan_parameter(emu_lib)


def test_contrast_errors(emu_lib):
    cc.check_errors(emu_lib)
