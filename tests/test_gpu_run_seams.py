"""bb_run's step bookkeeping on the GPU (`-m gpu`, MI355X): the counters k_res and k_stream carry by increments from the step a launch
starts at (window slot, re-add phase, ELBO recording period and ring slot), the ring's wrap, the 4096-step cut between resident launches,
hipGraph replay, and the non-finite status of every launch path -- against the literal oracle (tests/_run_cases.py; the emulation runs
what it can of the same cases in tests/test_emu_run_seams.py)."""
import pytest

import _run_cases as r

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("row", list(r.ROWS))
@pytest.mark.parametrize("path", list(r.PATHS))
def test_split_launches(hip_lib, monkeypatch, path, row):
    r.set_env(monkeypatch, r.PATHS[path])
    r.case_split_launches(hip_lib, path, row)


@pytest.mark.parametrize("path", list(r.FROZEN_PATHS))
def test_frozen_run_wraps_the_elbo_ring(hip_lib, monkeypatch, path):
    r.set_env(monkeypatch, r.FROZEN_PATHS[path])
    r.case_frozen_ring(hip_lib, path)


@pytest.mark.parametrize("S,opt", [(1, "TruncatedADAGrad"), (2, "DecayedADAGrad")])
@pytest.mark.parametrize("g", [4, 6])
@pytest.mark.parametrize("name", ["fitness_multi_tile", "replicate_ragged"])
def test_graph_replay(hip_lib, name, g, S, opt):
    r.case_graph_replay(hip_lib, name, g, S, opt)


@pytest.mark.parametrize("row", [1, 2])
def test_run_profiled(hip_lib, row):
    r.case_run_profiled(hip_lib, row, gpu=True)


@pytest.mark.parametrize("path", list(r.PATHS))
def test_nonfinite_status(hip_lib, monkeypatch, path):
    r.set_env(monkeypatch, r.PATHS[path])
    r.case_nonfinite(hip_lib, path)
