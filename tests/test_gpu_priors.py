"""Matrix-form priors and non-default optimiser constants on the GPU (`-m gpu`, MI355X): the compiled kernels of every launch path --
their LDS segment tables, the scalar-load table of optimiser constants, the any-parity instances' 8-byte accesses, k_stream's streamed
state, the compile-time-T instances of the BASELINE shapes -- against the literal oracle (tests/_prior_cases.py; the emulation runs
what it can of the same cases in tests/test_emu_priors.py).  Run with -s for the per-row figures and instance names."""
import pytest
import torch.multiprocessing as mp

import _cases as c
import _prior_cases as p
import _run_cases as r

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("form", p.FORMS)
@pytest.mark.parametrize("row", list(p.A_ROWS))
def test_launch_path(hip_lib, monkeypatch, row, form):
    r.set_env(monkeypatch, p.A_ROWS[row])
    p.case_path(hip_lib, row, form)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", p.B_SHAPES)
def test_point_services(hip_lib, name, mode):
    p.case_point_services(hip_lib, name, mode)


@pytest.mark.parametrize("name", ["genotype_runs", "genotype_odd"])
def test_genotype_regrouped(hip_lib, name):
    p.case_genotype_regrouped(hip_lib, name)


def test_genotype_regrouped_streamed(hip_lib, monkeypatch):
    r.set_env(monkeypatch, p.A_ROWS["k_stream-genotype_T8"])
    p.case_genotype_regrouped(hip_lib, "genotype_T8", expect_kernel=3)


def test_genotype_permuted(hip_lib):
    p.case_genotype_permuted(hip_lib)


@pytest.mark.parametrize("name", ["fitness_multi_tile", "multienv", "replicate_ragged", "multienv_replicate"])
def test_sharded_split_phase(hip_lib, name):
    p.case_sharded_split_phase(hip_lib, name)


def _multi_device_case(_, name, ms):
    p.case_multi_device(None, name, ms)


@pytest.mark.parametrize("ms", [False, True])
@pytest.mark.parametrize("name,nb", [("fitness_T6", 16), ("genotype_runs", 24)])
def test_multi_device_handle(hip_lib, monkeypatch, name, nb, ms):
    """In a process of its own, as test_gpu_parity.test_multi_device_handle: the two shards' launches are co-resident on device 0 only
    if each stream has a hardware queue to itself (the BB_TUNE_* settings travel in the environment)."""
    monkeypatch.setenv("BB_TUNE_NB", str(nb))
    monkeypatch.setenv("BB_TUNE_NTHR", "512")
    mp.spawn(_multi_device_case, args=(name, ms), nprocs=1)


@pytest.mark.parametrize("cfg", list(c.BASELINE_INSTANCES))
def test_baseline_kernel_instance_with_naive_priors(hip_lib, monkeypatch, cfg):
    p.case_baseline_instance(hip_lib, monkeypatch, cfg)


@pytest.mark.parametrize("path", ["two_kernel", "k_res", "k_stream"])
def test_constants_belong_to_the_handle(hip_lib, monkeypatch, path):
    r.set_env(monkeypatch, r.PATHS[path])
    p.case_constants_per_handle(hip_lib, path)
