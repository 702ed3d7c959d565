"""bb_debug_math in the host emulation: the host build of barbay.jl_amd/csrc/bb_math.h and the Box-Muller step at the stored
arguments of tests/golden/math_<fn>.npz against their 50-digit values, and the entry point itself (tests/_math_cases.py)."""
import pytest

import _math_cases as mc


@pytest.mark.parametrize("fn", mc.FNS)
def test_function_within_its_bound(emu_lib, fn):
    mc.check(emu_lib, fn, "emulation")


def test_probe_errors_and_empty_call(emu_lib):
    mc.check_errors(emu_lib)


def test_group_handle_equals_single_handle(emu_lib):
    mc.check_group_handle(emu_lib)


def test_debug_buffer_reuse(emu_lib):
    mc.check_buffer_reuse(emu_lib)
