"""The 50-digit reference (oracle/mp_literal.py), its committed fixtures, and the accuracy assertions of tests/_accuracy_cases.py on the
host emulation of the block programs.  The GPU run of the same cases is tests/test_gpu_accuracy.py."""
import numpy as np
import pytest

import _accuracy_cases as a


@pytest.mark.parametrize("case", a.CASES)
def test_mp_literal_agrees_with_the_literal_oracle_on_the_control_point(case):
    a.case_transcription(case)


@pytest.mark.parametrize("case", ["fitness_T5_d200", "multienv_d200", "genotype_d200", "replicate_d200", "replicate_ragged_d200",
                                  "multienv_replicate_d200", "multienv_replicate_T46_d200"])
def test_mp_literal_runs_every_model_kind(case):
    a.case_mp_literal_runs(case)


def test_fixture_regenerates_bit_equal():
    """The generator, run here with mpmath, reproduces the committed fitness_tiny case bit for bit -- every array, the data included."""
    fresh = a.gen.generate("fitness_tiny")
    d = dict(np.load(a.gen.path("fitness_tiny")))
    assert sorted(fresh) == sorted(d)
    for k, v in fresh.items():
        v = np.asarray(v)
        assert v.dtype == d[k].dtype and v.shape == d[k].shape, k
        assert v.tobytes() == d[k].tobytes(), k


def test_mp_literal_is_not_the_fused_form():
    """Scale and G are sums over elementary addends: at a posterior-like point of a deep data set |logp| is orders below the scale
    (that is what makes a bound relative to |logp| a statement about conditioning), and G_i >= |g_i| everywhere."""
    _, d = a.load("fitness_T4_d20000")
    assert (np.abs(d["logp"][:3]) < 1e-2 * d["scale"][:3]).all()
    for case in a.CASES:
        _, d = a.load(case)
        assert (np.abs(d["grad"]) <= d["G"].astype(np.float64) * (1 + 1e-6)).all()


@pytest.mark.parametrize("geometry", list(a.GEOMETRIES))
@pytest.mark.parametrize("case", a.CASES)
def test_accuracy_emulation(emu_lib, monkeypatch, case, geometry):
    for k, v in a.GEOMETRIES[geometry].items():
        monkeypatch.setenv(k, v)
    a.case_accuracy(emu_lib, case)


@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("name", list(a.TRAJ))
def test_trajectory_from_posterior_like_start_emulation(emu_lib, monkeypatch, name, S):
    for k, v in a.TRAJ[name][1].items():
        monkeypatch.setenv(k, v)
    a.case_trajectory(emu_lib, name, S)


@pytest.mark.parametrize("case,config", a.resident_cases())
def test_resident_accuracy_emulation(emu_lib, case, config):
    """The gradient the resident launches form (k_res, k_stream, k_persist), read back through one linear optimiser step."""
    a.case_resident_accuracy(emu_lib, case, config)


@pytest.mark.parametrize("case", ["fitness_T4_d200", "replicate_d200"])
def test_resident_probe_is_the_gradient_emulation(emu_lib, case):
    a.case_probe_selfcheck(emu_lib, case)
