"""The iterate trace (bb_trace_*, barbay.jl_amd/csrc/bb_trace.h) and the stopping rule of barbay.jl_amd/vi.py on the GPU; the cases are
tests/_trace_cases.py's, shared with the emulation tests."""
import pytest

import _trace_cases as tc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("setting", sorted(tc.SETTINGS))
@pytest.mark.parametrize("mode", tc.MODES)
@pytest.mark.parametrize("shape", tc.SHAPES)
def test_snapshots_are_the_parameters(hip_lib, shape, mode, setting):
    tc.case_snapshots(hip_lib, shape, mode, setting)


@pytest.mark.parametrize("mode", tc.MODES)
@pytest.mark.parametrize("shape", tc.SHAPES)
def test_summary_equals_chain_summary(hip_lib, shape, mode):
    tc.case_summary(hip_lib, shape, mode)


def test_verdict_of_a_frozen_run(hip_lib):
    tc.case_verdict_frozen(hip_lib)


@pytest.mark.parametrize("mode", tc.MODES)
def test_verdict_with_a_planted_nan(hip_lib, mode):
    tc.case_verdict_nonfinite(hip_lib, mode)


def test_buffers_shared_with_the_other_post_fit_calls(hip_lib):
    tc.case_buffer_reuse(hip_lib)


@pytest.mark.parametrize("mode", tc.MODES)
def test_handle_untouched(hip_lib, mode):
    tc.case_handle_untouched(hip_lib, mode)


def test_errors(hip_lib):
    tc.case_errors(hip_lib)


def test_stopping_rule_end_to_end(hip_lib):
    tc.case_stopping_rule(hip_lib)


def test_rhat_max_of_one_runs_to_max_iters(hip_lib):
    tc.case_never_converges(hip_lib)


def test_without_convergence_nothing_changes(hip_lib):
    tc.case_convergence_none(hip_lib)


def test_hierarchical_rows_come_from_the_averaged_q(hip_lib):
    tc.case_hierarchical(hip_lib)


@pytest.mark.parametrize("row", (1, 4))
@pytest.mark.parametrize("mode", tc.MODES)
def test_traced_run_against_the_uncut_run(hip_lib, mode, row):
    tc.case_traced_against_uncut(hip_lib, mode, row)


def test_trace_cost_tool_small_mode(hip_lib, tmp_path):
    tc.case_tool_small(tmp_path)
