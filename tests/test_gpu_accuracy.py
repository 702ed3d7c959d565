"""Accuracy on the device at posterior-like points, against the committed 50-digit truth: bb_logdensity_grad_batch (k_logp_moments,
k_logp_grad, k_logp_geno), bb_logdensity_grad and bb_elbo_grad in units of u * scale and, per block of the layout, u * G_i; bounds from
the fp64 literal oracle's own stored error (tests/_accuracy_cases.py).  Then the resident kernels stepping from such a point, and the
gradient they form inside one step (k_res, k_stream, k_persist) in the same units, read back through a linear optimiser step.
Reads only tests/golden/accuracy_*; run with `-m gpu` on an MI355X."""
import pytest

import _accuracy_cases as a

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("geometry", list(a.GEOMETRIES))
@pytest.mark.parametrize("case", a.CASES)
def test_accuracy(hip_lib, monkeypatch, case, geometry):
    for k, v in a.GEOMETRIES[geometry].items():
        monkeypatch.setenv(k, v)
    a.case_accuracy(hip_lib, case)


@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("name", list(a.TRAJ))
def test_trajectory_from_posterior_like_start(hip_lib, monkeypatch, name, S):
    for k, v in a.TRAJ[name][1].items():
        monkeypatch.setenv(k, v)
    a.case_trajectory(hip_lib, name, S)


@pytest.mark.parametrize("case,config", a.resident_cases(device=True))
def test_resident_accuracy(hip_lib, case, config):
    a.case_resident_accuracy(hip_lib, case, config, device=True)


@pytest.mark.parametrize("case", ["fitness_T4_d200", "replicate_d200"])
def test_resident_probe_is_the_gradient(hip_lib, case):
    a.case_probe_selfcheck(hip_lib, case)
