"""The iterate trace (bb_trace_*, barbay.jl_amd/csrc/bb_trace.h) and the stopping rule of barbay.jl_amd/vi.py in the host emulation of the
block programs; the cases are tests/_trace_cases.py's, shared with the GPU tests."""
import pytest

import _trace_cases as tc


@pytest.mark.parametrize("setting", sorted(tc.SETTINGS))
@pytest.mark.parametrize("mode", tc.MODES)
@pytest.mark.parametrize("shape", tc.SHAPES)
def test_snapshots_are_the_parameters(emu_lib, shape, mode, setting):
    tc.case_snapshots(emu_lib, shape, mode, setting)


@pytest.mark.parametrize("mode", tc.MODES)
@pytest.mark.parametrize("shape", tc.SHAPES)
def test_summary_equals_chain_summary(emu_lib, shape, mode):
    tc.case_summary(emu_lib, shape, mode)


def test_verdict_of_a_frozen_run(emu_lib):
    tc.case_verdict_frozen(emu_lib)


@pytest.mark.parametrize("mode", tc.MODES)
def test_verdict_with_a_planted_nan(emu_lib, mode):
    tc.case_verdict_nonfinite(emu_lib, mode)


def test_buffers_shared_with_the_other_post_fit_calls(emu_lib):
    tc.case_buffer_reuse(emu_lib)


@pytest.mark.parametrize("mode", tc.MODES)
def test_handle_untouched(emu_lib, mode):
    tc.case_handle_untouched(emu_lib, mode)


def test_errors(emu_lib):
    tc.case_errors(emu_lib)


def test_stopping_rule_end_to_end(emu_lib):
    tc.case_stopping_rule(emu_lib)


def test_rhat_max_of_one_runs_to_max_iters(emu_lib):
    tc.case_never_converges(emu_lib)


def test_without_convergence_nothing_changes(emu_lib):
    tc.case_convergence_none(emu_lib)


def test_hierarchical_rows_come_from_the_averaged_q(emu_lib):
    tc.case_hierarchical(emu_lib)
