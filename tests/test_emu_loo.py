"""bb_ppc_loo (PSIS leave-one-out scores per cell and per barcode, barbay.jl_amd/csrc/bb_loo.h) in the host emulation of the block
program, against the 50-digit goldens of tests/golden/make_loo_golden.py and the numpy restatement (tests/_loo_cases.py); the
wiring of the call through the header, the binding and the Julia module; `stats.loo_compare`."""
import os
import re

import numpy as np
import pandas as pd
import pytest

import _loo_cases as lc
import _ppc_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wiring():
    """bb_ppc_loo and bb_loo_shape are declared in the header, listed and bound in the Python binding and called by the Julia
    module, struct for struct."""
    from barbay_jl_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "barbay_hip.h")).read()
    jl = open(os.path.join(ROOT, "julia", "BarBayHIP.jl")).read()
    for sym in ("bb_ppc_loo", "bb_loo_shape"):
        assert re.search(r"\bint " + sym + r"\(", hdr), sym
        assert sym in _capi.EXPORTS, sym
        assert ":" + sym in jl, sym
    assert "#define BB_LOO_MAX_SAMPLES 8192" in hdr and _capi.BB_LOO_MAX_SAMPLES == 8192
    fields = re.search(r"typedef struct bb_loo_out \{(.*?)\} bb_loo_out;", hdr, flags=re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = re.findall(r"\*\s*([a-z_]+)", fields)
    assert names == [f[0] for f in _capi.bb_loo_out._fields_]
    jl_fields = re.search(r"struct bb_loo_out\n(.*?)\nend", jl, flags=re.S).group(1)
    assert re.findall(r"([a-z_]+)::Ptr", jl_fields) == names
    assert hasattr(_capi.Engine, "ppc_loo") and hasattr(_capi.Engine, "loo_shape")


def test_wiring_in_the_library(emu_lib):
    assert hasattr(emu_lib, "bb_ppc_loo") and hasattr(emu_lib, "bb_loo_shape")


def test_parameters_reach_every_band_of_khat_and_the_raw_branch():
    lc.check_bands()


def test_tail_length():
    assert [lc.tail_len(n) for n in (2, 4, 5, 24, 25, 111, 1000, 1025, 8192)] == [0, 0, 1, 4, 5, 22, 95, 97, 272]


@pytest.mark.parametrize("name", sorted(lc.golden_cases()))
def test_loo_matches_golden(emu_lib, name):
    lc.check_golden(emu_lib, name, "emulation")


def test_lpd_shares_the_bytes_of_the_score(emu_lib):
    lc.check_shared_bytes(emu_lib)


def test_unsmoothed_sizes(emu_lib):
    lc.check_unsmoothed(emu_lib)


def test_zero_counts_empty_rows_and_one_step_rows(emu_lib):
    lc.check_zero_counts(emu_lib)


def test_nan_parameter_stays_in_its_rows(emu_lib):
    lc.check_nan_parameter(emu_lib)


def test_loo_errors_and_limits(emu_lib):
    lc.check_errors(emu_lib)


def test_buffer_reuse_across_calls_and_sizes(emu_lib):
    lc.check_buffer_reuse(emu_lib)


@pytest.mark.parametrize("name", pc.GROUP_CASES)
def test_group_handle_equals_single_device(emu_lib, name):
    lc.check_group_handle(emu_lib, name)


def test_handle_untouched(emu_lib):
    lc.check_handle_untouched(emu_lib)


def test_repeatable(emu_lib):
    lc.check_repeatable(emu_lib)


def test_closed_form(emu_lib):
    lc.check_closed_form(emu_lib)


def _frame(ids, elpd, khat=None):
    n = len(ids)
    return pd.DataFrame({"id": ids, "neutral": [False] * n, "rep": ["R1"] * n, "elpd_loo": elpd, "p_loo": np.zeros(n),
                         "khat": np.zeros(n) if khat is None else khat, "n_eff": np.ones(n), "khat_max_cell": np.zeros(n),
                         "n_scored": np.ones(n, dtype=int), "flag": [False] * n})


def test_loo_compare():
    import barbay_jl_amd as bb
    a = _frame(["x", "y", "z", "w"], [-1.0, -2.0, -3.0, -4.0])
    same = bb.stats.loo_compare(a, a)
    assert same["elpd_diff"] == 0.0 and same["se_diff"] == 0.0 and same["n"] == 4
    b = _frame(["x", "y", "z", "w"], [-1.5, -2.0, -1.0, -4.25])
    c = bb.stats.loo_compare(a, b)
    d = np.array([-0.5, 0.0, 2.0, -0.25])
    assert c["elpd_diff"] == d.sum() and np.isclose(c["se_diff"], np.sqrt(4 * d.var(ddof=1)), rtol=1e-15)
    assert list(c["rows"]["id"]) == ["z", "x", "w", "y"] and list(c["rows"]["elpd_diff"]) == [2.0, -0.5, -0.25, 0.0]
    with pytest.raises(bb.BarBayError):
        bb.stats.loo_compare(a, _frame(["x", "y", "z", "v"], [0.0] * 4))
    with pytest.raises(bb.BarBayError):
        bb.stats.loo_compare(a, b.iloc[:3])
    u = _frame(["x", "y", "z", "w"], [-1.0, np.nan, -3.0, -4.0])            # a barcode without a scored step: left out of both
    cu = bb.stats.loo_compare(u, b)
    assert cu["n"] == 3 and cu["elpd_diff"] == -0.5 + 2.0 - 0.25
