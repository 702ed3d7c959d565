"""bb_freq_bands (frequency-trajectory bands, barbay.jl_amd/csrc/bb_freq.h) in the host emulation of the block programs, against
the numpy restatement draw for draw (tests/_freq_cases.py)."""
import numpy as np
import pytest

import _freq_cases as fc
from conftest import make_engine


@pytest.mark.parametrize("mode", ["trajectory", "posterior"])
@pytest.mark.parametrize("name", fc.CASES)
def test_freq_bands_match_restatement(emu_lib, name, mode):
    fc.case_freq(emu_lib, name, mode)


def test_freq_extreme_posterior(emu_lib):
    fc.case_extreme(emu_lib)


def test_freq_rows_subset_and_outside_flag(emu_lib):
    sp = fc.spec("replicate_ragged")
    with make_engine(sp, emu_lib, seed=2) as e:
        b1, n1 = e.freq_bands([0.9], n_samples=64, n_ppc=3, seed=5)
        b2, n2 = e.freq_bands([0.9], n_samples=64, n_ppc=3, seed=5, outside=False)
        assert n2 is None and np.array_equal(b1.view(np.uint64), b2.view(np.uint64))
        mu, om = e.get_params()
        rows = [0, 5, 6, 17, sp.B, sp.B + 7, 3 * sp.B - 1]         # neutrals and mutants of every replicate
        b3, n3 = fc.restate(sp, mu, om, [0.9], "trajectory", 64, 3, 5, rows=rows)
        fc.assert_bands_close(b1[rows], b3)
        assert np.array_equal(n1[rows], n3)


def test_freq_edge_quantiles(emu_lib):
    """q = 1 is the column's range, q = 0 its median (both order statistics exact, coinciding ends); K = 2 is the smallest column."""
    sp = fc.spec("fitness")
    with make_engine(sp, emu_lib, seed=2) as e:
        mu, om = e.get_params()
        for ns, npp in ((2, 1), (1, 2), (50, 1)):
            b, n = e.freq_bands([1.0, 0.0], n_samples=ns, n_ppc=npp, seed=9)
            b2, n2 = fc.restate(sp, mu, om, [1.0, 0.0], "trajectory", ns, npp, 9)
            fc.assert_bands_close(b, b2)
            assert np.array_equal(n, n2)
            assert np.array_equal(b[:, :, 1, 0], b[:, :, 1, 1])
            assert np.all(b[:, :, 0, 0] <= b[:, :, 1, 0]) and np.all(b[:, :, 1, 0] <= b[:, :, 0, 1])
        b, _ = e.freq_bands([1.0, 0.0], mode="posterior", n_samples=50, n_ppc=1, seed=9, outside=False)
        b2, _ = fc.restate(sp, mu, om, [1.0, 0.0], "posterior", 50, 1, 9)
        fc.assert_bands_close(b, b2)


def test_freq_shares_parameter_draws_with_ppc(emu_lib):
    """At equal seed column 0 of a trajectory is the posterior-mode column 0, the same joint draws, each n_ppc times: the same
    minimum, bit for bit (the q = 1 upper end is a + 1 (b - a) of the two largest values, which differ only in posterior mode)."""
    sp = fc.spec("fitness")
    with make_engine(sp, emu_lib, seed=2) as e:
        a, _ = e.freq_bands([1.0], n_samples=40, n_ppc=3, seed=6, outside=False)
        b, _ = e.freq_bands([1.0], mode="posterior", n_samples=40, n_ppc=1, seed=6, outside=False)
        assert np.array_equal(a[:, 0, 0, 0].view(np.uint64), b[:, 0, 0, 0].view(np.uint64))
        assert np.all(np.abs(a[:, 0, 0, 1] - b[:, 0, 0, 1]) <= 4e-16 * b[:, 0, 0, 1])


def test_freq_errors(emu_lib):
    from barbay_jl_amd._capi import BarBayHipError
    sp = fc.spec("fitness")
    with make_engine(sp, emu_lib, seed=2) as e:
        for qs in ([1.5], [-0.5], [float("nan")], [], [0.5] * 9):
            with pytest.raises(BarBayHipError, match="error -1"):
                e.freq_bands(qs, n_samples=10, n_ppc=2)
        for ns, npp in ((0, 5), (5, 0), (1, 1), (16385, 1), (4097, 4)):
            with pytest.raises(BarBayHipError, match="error -4"):
                e.freq_bands([0.9], n_samples=ns, n_ppc=npp)
        with pytest.raises(BarBayHipError, match="error -1"):
            e.freq_bands([0.9], mode="posterior", n_samples=10, n_ppc=2)
        with pytest.raises(BarBayHipError, match="error -1"):
            e.freq_bands([0.9], mode=7, n_samples=10, n_ppc=2)
        e.freq_bands([0.9], n_samples=16384, n_ppc=1, outside=False)          # the largest column is accepted
