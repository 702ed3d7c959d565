"""GPU: k_res's one-wave consume + finish (br_consume_finish: wave 0 alone from the end of its poll to barrier 3, no workgroup barrier in
between, the LDS offsets and the F pass's tables compile-time arithmetic) against the generic instances' bbp_consume_tg + br_finish.  Two
handles in one process, the second created with BB_TUNE_OPT_SPEC=0 (the pattern of tests/test_gpu_opt_spec.py): seed 13, a window of 4
slots, run(4) then run(6) -- mu, omega and the three opt_state arrays must compare byte for byte.  The shapes
(tests/_fin_chain_cases.py) are the smallest at which the leg can go wrong: one tile, fewer groups than eight, non-leader tiles, T = 6,
time points without moments, tiles of whole genotypes, and 16 first-hop groups, which must keep the generic instance.

A wrong barrier count or poll mask would hang a tile rather than fail: every test runs under a watchdog of its own that ends the
process."""
import faulthandler

import numpy as np
import pytest

import _fin_chain_cases as fc
from conftest import make_engine

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def watchdog():
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.mark.parametrize("cid", list(fc.CASES))
def test_one_wave_leg_equals_the_general_chain(hip_lib, monkeypatch, cid):
    outs = fc.run_pair(make_engine, hip_lib, monkeypatch, cid, emu=False)
    if outs is None:          # (no resident launch for the shape: tests/_fin_chain_cases.py)
        return
    a, b = outs
    assert np.all(np.isfinite(a[0])) and np.all(np.isfinite(a[1])) and np.any(a[4] != 0.0)
    for x, y, what in zip(a, b, ("mu", "omega", "acc_mu", "acc_omega", "lo")):
        assert x.tobytes() == y.tobytes(), (what, int((x != y).sum()), float(np.abs(x.astype(np.float64) - y.astype(np.float64)).max()))
