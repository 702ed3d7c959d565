"""bb_run's step bookkeeping on the host emulation of the block programs (g++ -DBB_EMU, no GPU): split launches, the ELBO ring's wrap and
the non-finite status on every launch path the emulation runs.  The emulation recomputes the window slot, the re-add phase and the ring
slot from the step number at every step, so these runs verify the oracle side of tests/test_gpu_run_seams.py and the arithmetic the
kernels share with it -- not the counters the kernels carry by increments."""
import pytest

import _run_cases as r


@pytest.mark.parametrize("row", list(r.ROWS))
@pytest.mark.parametrize("path", list(r.PATHS))
def test_split_launches(emu_lib, monkeypatch, path, row):
    r.set_env(monkeypatch, r.PATHS[path])
    r.case_split_launches(emu_lib, path, row)


@pytest.mark.parametrize("path", list(r.FROZEN_PATHS))
def test_frozen_run_wraps_the_elbo_ring(emu_lib, monkeypatch, path):
    """eta = 0 freezes the parameters on the emulation too.  On fitness_T4, the GPU test's shape, which the emulation steps fast enough
    on every path (k_stream through emu_stream_phase); the 4096 oracle values are computed once for the three."""
    r.set_env(monkeypatch, r.FROZEN_PATHS[path])
    r.case_frozen_ring(emu_lib, path)


@pytest.mark.parametrize("row", [1, 2])
def test_run_profiled(emu_lib, row):
    r.case_run_profiled(emu_lib, row, gpu=False)


@pytest.mark.parametrize("path", list(r.PATHS))
def test_nonfinite_status(emu_lib, monkeypatch, path):
    r.set_env(monkeypatch, r.PATHS[path])
    r.case_nonfinite(emu_lib, path)


def test_no_graph_launches_in_the_emulation(emu_lib):
    """bb_debug_graph_launches: the emulation enqueues every step on its own, whatever steps_per_graph asks for."""
    from conftest import make_engine
    with make_engine(r._sp("fitness_T2"), emu_lib, seed=r.SEED, launch_mode=1, steps_per_graph=4) as e:
        e.run(9)
        assert e.graph_launches() == 0 and e.stats()["steps_done"] == 9
