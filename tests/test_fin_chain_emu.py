"""k_res's one-wave consume + finish (br_consume_finish: the OS instances of the fitness / multienv / genotype kinds with a compile-time T)
against bbp_consume_tg + br_finish, through the host emulation of the same templates: the two forms do the same operations on the same
values in the same order, so two handles -- the second created with BB_TUNE_OPT_SPEC=0 -- agree BIT FOR BIT on the parameters, the
accumulators and the window sums' low-order parts.  The cases (tests/_fin_chain_cases.py) are those of tests/test_gpu_fin_chain.py: here
it is also checked that every shape reaches the instance it names before it is sent to a GPU."""
import numpy as np
import pytest

import _fin_chain_cases as fc
from conftest import make_engine


@pytest.mark.parametrize("cid", list(fc.CASES))
def test_one_wave_leg_equals_the_general_chain(emu_lib, monkeypatch, cid):
    a, b = fc.run_pair(make_engine, emu_lib, monkeypatch, cid, emu=True)
    assert np.all(np.isfinite(a[0])) and np.all(np.isfinite(a[1])) and np.any(a[4] != 0.0)
    for x, y, what in zip(a, b, ("mu", "omega", "acc_mu", "acc_omega", "lo")):
        assert x.tobytes() == y.tobytes(), (what, int((x != y).sum()), float(np.abs(x.astype(np.float64) - y.astype(np.float64)).max()))
