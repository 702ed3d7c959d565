"""bb_ppc_bands (posterior predictive bands, barbay.jl_amd/csrc/bb_ppc.h) in the host emulation of the block programs, against the
numpy restatement draw for draw (tests/_ppc_cases.py)."""
import numpy as np
import pytest

import _ppc_cases as pc
from conftest import make_engine


@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_ppc_bands_match_restatement(emu_lib, name):
    pc.case_ppc(emu_lib, name)


def test_buffer_reuse_across_calls_and_sizes(emu_lib):
    pc.case_buffer_reuse(emu_lib)


@pytest.mark.parametrize("name", pc.GROUP_CASES)
def test_group_handle_equals_single_device(emu_lib, name):
    pc.case_group_handle(emu_lib, name)


def test_ppc_rows_subset_and_outside_flag(emu_lib):
    sp = pc.spec("fitness")
    with make_engine(sp, emu_lib, seed=2) as e:
        b1, n1 = e.ppc_bands([0.9], n_samples=64, n_ppc=3, seed=5)
        b2, n2 = e.ppc_bands([0.9], n_samples=64, n_ppc=3, seed=5, outside=False)
        assert n2 is None and np.array_equal(b1, b2)
        mu, om = e.get_params()
        rows = [0, 1, 17, sp.n_bc]
        b3, n3 = pc.restate(sp, mu, om, [0.9], 64, 3, 5, rows=rows)
        pc.assert_bands_close(b1[rows], b3)
        assert np.array_equal(n1[rows], n3)


def test_ppc_edge_quantiles(emu_lib):
    """q = 1 is the column's range, q = 0 its median (both order statistics exact); K = 2 is the smallest column."""
    sp = pc.spec("fitness")
    with make_engine(sp, emu_lib, seed=2) as e:
        mu, om = e.get_params()
        for ns, npp in ((2, 1), (1, 2), (50, 1)):
            b, n = e.ppc_bands([1.0, 0.0], n_samples=ns, n_ppc=npp, seed=9)
            b2, n2 = pc.restate(sp, mu, om, [1.0, 0.0], ns, npp, 9)
            pc.assert_bands_close(b, b2)
            assert np.array_equal(n, n2)
            assert np.array_equal(b[:, :, 1, 0], b[:, :, 1, 1])


def test_ppc_errors(emu_lib):
    from barbay_jl_amd._capi import BarBayHipError
    sp = pc.spec("fitness")
    with make_engine(sp, emu_lib, seed=2) as e:
        for qs in ([1.5], [-0.5], [float("nan")], [], [0.5] * 9):
            with pytest.raises(BarBayHipError, match="error -1"):
                e.ppc_bands(qs, n_samples=10, n_ppc=2)
        for ns, npp in ((0, 5), (5, 0), (1, 1), (16385, 1), (4097, 4)):
            with pytest.raises(BarBayHipError, match="error -4"):
                e.ppc_bands([0.9], n_samples=ns, n_ppc=npp)
        e.ppc_bands([0.9], n_samples=16384, n_ppc=1)          # the largest column is accepted
