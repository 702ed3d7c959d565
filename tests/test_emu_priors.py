"""Matrix-form priors and non-default optimiser constants on the host emulation of the block programs (g++ -DBB_EMU, no GPU): every
launch path the emulation steps, the point services, the regrouped genotype model, shards and per-handle constants against the
literal oracle (tests/_prior_cases.py).  The emulation steps the block programs the kernels share, the host-built segment tables and
bb_create's permutations; the compiled instances, their LDS tables and scalar loads are what tests/test_gpu_priors.py runs.  Instance
names are checked after stripping the emulation's "emu:"."""
import numpy as np
import pytest

import _prior_cases as p
import _run_cases as r


@pytest.mark.parametrize("form", p.FORMS)
@pytest.mark.parametrize("row", p.EMU_ROWS)
def test_launch_path(emu_lib, monkeypatch, row, form):
    r.set_env(monkeypatch, p.A_ROWS[row])
    p.case_path(emu_lib, row, form)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", p.B_SHAPES)
def test_point_services(emu_lib, name, mode):
    p.case_point_services(emu_lib, name, mode)


@pytest.mark.parametrize("name", ["genotype_runs", "genotype_odd"])
def test_genotype_regrouped(emu_lib, name):
    p.case_genotype_regrouped(emu_lib, name)


def test_genotype_regrouped_streamed(emu_lib, monkeypatch):
    r.set_env(monkeypatch, p.A_ROWS["k_stream-genotype_T8"])
    p.case_genotype_regrouped(emu_lib, "genotype_T8", expect_kernel=3)


def test_genotype_permuted(emu_lib):
    p.case_genotype_permuted(emu_lib)


@pytest.mark.parametrize("name", ["fitness_multi_tile", "multienv", "replicate_ragged", "multienv_replicate"])
def test_sharded_split_phase(emu_lib, name):
    p.case_sharded_split_phase(emu_lib, name)


@pytest.mark.parametrize("ms", [False, True])
@pytest.mark.parametrize("name,nb", [("fitness_T6", 16), ("genotype_runs", 24)])
def test_multi_device_handle(emu_lib, monkeypatch, name, nb, ms):
    monkeypatch.setenv("BB_TUNE_NB", str(nb))
    monkeypatch.setenv("BB_TUNE_NTHR", "512")
    p.case_multi_device(emu_lib, name, ms)


@pytest.mark.parametrize("path", ["two_kernel", "k_res", "k_stream"])
def test_constants_belong_to_the_handle(emu_lib, monkeypatch, path):
    r.set_env(monkeypatch, r.PATHS[path])
    p.case_constants_per_handle(emu_lib, path)


@pytest.mark.parametrize("name", sorted({v["shape"] for v in p.A_ROWS.values()}))
def test_sensitivity(name):
    """The launch-path tests can fail: on every shape they run, the oracle's own trajectory with one Matrix block's prior rolled by one
    element differs from the unrolled one by at least 1000 x their tolerance, in that block's mu.  A shape that falls under the bound
    gets another seed (_prior_cases.SHAPE_SEED), not another bound."""
    d = p.sensitivity(name)
    print(name, {k: f"{v:.2e}" for k, v in d.items()})
    assert set(d) >= {"s_pop", "logsigma_pop", "logsigma_bc", "loglambda"} and len(d) == 5, d
    assert min(d.values()) >= p.SENSITIVITY, d


def test_naive_means_are_naive_prior():
    """with_priors' naive form feeds what the loop-for-loop naive_prior returns."""
    from oracle import naive
    sp = p._sp("replicate_ragged")
    ref = naive.naive_prior(sp)
    got = p.naive_means(sp)
    for a, b in zip(got, (ref["s_pop_prior"], ref["logσ_pop_prior"], ref["logλ_prior"])):
        assert a.shape == b.shape and np.abs(a - b).max() < 1e-12
