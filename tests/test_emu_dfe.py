"""bb_dfe_rb (posterior of the fitness distribution of sets of units, barbay.jl_amd/csrc/bb_dfe.h) in the host emulation of the
block programs: the 50-digit goldens of tests/golden/make_dfe_golden.py and the numpy restatement (tests/_dfe_cases.py), the tie to
bb_fitness_rb, composition at explicit draws, the common mode the call exists for, determinism, non-finite values and errors."""
import pytest

import _dfe_cases as dc
import _rb_cases as rc


@pytest.mark.parametrize("name", sorted(dc.golden_cases()))
def test_small_sets_stay_within_the_tails(name):
    dc.check_z_range(name)


@pytest.mark.parametrize("name", sorted(dc.golden_cases()))
def test_dfe_matches_golden(emu_lib, name):
    dc.check_golden(emu_lib, name, "emulation")


@pytest.mark.parametrize("name", sorted(rc.golden_cases()))
def test_one_unit_sets_match_the_marginals_tails(emu_lib, name):
    dc.check_tie(emu_lib, name, "emulation")


@pytest.mark.parametrize("case", dc.CASES)
def test_dfe_composes_the_tails_of_its_units(emu_lib, case):
    dc.check_composition(emu_lib, case)


def test_restated_fraction_moves_between_draws_more_than_within():
    dc.check_point_restated()


def test_fraction_moves_between_draws_more_than_within(emu_lib):
    dc.check_point(emu_lib)


@pytest.mark.parametrize("case", ["fitness_chunk", "multienv_replicate", "multienv_env0_only_first"])
def test_independent_of_the_rest_of_the_call(emu_lib, case):
    dc.check_independent_of_the_rest_of_the_call(emu_lib, case)


def test_grids_of_1_5_and_64_points(emu_lib):
    dc.check_grid_sizes_against_restatement(emu_lib)


def test_independent_of_launch_mode_and_repeatable(emu_lib):
    dc.check_launch_modes(emu_lib)


@pytest.mark.parametrize("case", ["fitness", "replicate_ragged", "genotype_regrouped"])
def test_group_handle_equals_single_device(emu_lib, case):
    dc.check_group_handle(emu_lib, case)


def test_buffer_reuse_across_calls_and_sizes(emu_lib):
    dc.check_buffer_reuse(emu_lib)


def test_handle_untouched(emu_lib):
    dc.check_handle_untouched(emu_lib)


@pytest.mark.parametrize("case", ["fitness", "genotype_regrouped", "multienv_replicate"])
def test_own_draws_equal_the_same_draws_passed_in(emu_lib, case):
    dc.check_internal_against_explicit_draws(emu_lib, case)


def test_nan_parameter_stays_in_its_sets(emu_lib):
    dc.check_nan_parameter(emu_lib)


def test_dfe_errors(emu_lib):
    dc.check_errors(emu_lib)
