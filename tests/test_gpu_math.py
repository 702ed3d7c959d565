"""bb_debug_math on the device: the DEVICE build of barbay.jl_amd/csrc/bb_math.h -- hardware rcp / rsq seeds and the Newton steps
behind them, the v_fma_f64 Horner blocks on scalar coefficients, the __constant__ tables, the device ldexp / frexp / rint -- and
the Box-Muller step, at the stored arguments of tests/golden/math_<fn>.npz against their 50-digit values, under the bounds the
host build is held to (tests/_math_cases.py).  Each case is one launch of a few thousand elements."""
import pytest

import _math_cases as mc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fn", mc.FNS)
def test_function_within_its_bound(hip_lib, emu_lib, fn):
    mc.check(hip_lib, fn, "device", other=emu_lib)


def test_probe_errors_and_empty_call(hip_lib):
    mc.check_errors(hip_lib)


def test_group_handle_equals_single_handle(hip_lib):
    mc.check_group_handle(hip_lib)


def test_debug_buffer_reuse(hip_lib):
    mc.check_buffer_reuse(hip_lib)
