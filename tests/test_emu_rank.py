"""bb_fitness_rank (posterior ranks and top-k membership of the units of sets, barbay.jl_amd/csrc/bb_rank.h) in the host emulation
of the block programs: the sorter against numpy's stable lexsort on planted columns, the conditional source against the numpy
restatement (tests/_rank_cases.py), the coupling the call exists for, determinism, non-finite values and errors."""
import os
import re

import pytest

import _rank_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_binding_and_julia_wrapper_agree():
    from barbay_jl_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "barbay_hip.h")).read()
    jl = open(os.path.join(ROOT, "julia", "BarBayHIP.jl")).read()
    assert re.search(r"\bint bb_fitness_rank\(", hdr) and "bb_fitness_rank" in _capi.EXPORTS and ":bb_fitness_rank" in jl
    for name in ("BB_RANK_MAX_TOP", "BB_RANK_RUN", "BB_RANK_MAX_SAMPLES"):
        assert re.search(rf"#define {name}\s+{getattr(_capi, name)}\b", hdr), name
    for struct in ("bb_rank_opts", "bb_rank_out"):
        fields = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, flags=re.S).group(1)
        fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
        names = re.findall(r"[\s\*]([a-z_0-9]+)\s*[;,]", fields)
        assert names == [f[0] for f in getattr(_capi, struct)._fields_], struct


def test_numpy_order_on_a_column_by_hand():
    import numpy as np
    v = np.array([[0.0], [np.nan], [-0.0], [np.inf], [-np.inf], [1.0], [np.copysign(np.nan, -1.0)], [1.0]])
    assert list(kc.order_ranks(v)[:, 0]) == [3, 6, 4, 0, 5, 1, 7, 2]


@pytest.mark.parametrize("n", kc.NS)
@pytest.mark.parametrize("case", kc.CASES)
def test_restated_columns_have_gaps(case, n):
    kc.check_gaps(case, n)


def test_restated_rank_sd_grows_with_the_shared_uncertainty():
    kc.check_point_restated()


def test_sorter_matches_numpy_on_planted_columns(emu_lib):
    kc.check_sorter(emu_lib)


def test_sorter_at_the_full_run_and_beyond(emu_lib):
    kc.check_sorter_large(emu_lib)


@pytest.mark.parametrize("n", kc.NS)
@pytest.mark.parametrize("case", kc.CASES)
def test_conditional_ranks_match_the_restatement(emu_lib, case, n):
    kc.check_conditional(emu_lib, case, n, "emulation")


def test_rank_sd_grows_with_the_shared_uncertainty(emu_lib):
    kc.check_point(emu_lib)


@pytest.mark.parametrize("case", ["fitness_chunk", "multienv_replicate"])
def test_independent_of_the_rest_of_the_call(emu_lib, case):
    kc.check_independent_of_the_rest_of_the_call(emu_lib, case)


def test_independent_of_launch_mode_and_repeatable(emu_lib):
    kc.check_launch_modes(emu_lib)


@pytest.mark.parametrize("case", ["fitness", "replicate_ragged", "genotype_regrouped"])
def test_group_handle_equals_single_device(emu_lib, case):
    kc.check_group_handle(emu_lib, case)


def test_buffer_reuse_across_calls_and_sizes(emu_lib):
    kc.check_buffer_reuse(emu_lib)


def test_handle_untouched(emu_lib):
    kc.check_handle_untouched(emu_lib)


@pytest.mark.parametrize("case", ["fitness", "genotype_regrouped", "multienv_replicate"])
def test_own_draws_equal_the_same_draws_passed_in(emu_lib, case):
    kc.check_internal_against_explicit_draws(emu_lib, case)


def test_nan_parameter_ranks_last_and_stays_in_its_sets(emu_lib):
    kc.check_nan_parameter(emu_lib)


def test_rank_errors(emu_lib):
    kc.check_errors(emu_lib)
