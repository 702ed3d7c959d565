"""The resident kernels' instances with the optimiser compiled in (k_res / k_stream<.., OS = true>: TruncatedADAGrad with resum_every == 0,
bb_opt_apply<0, 0> of csrc/bb_block.h) against the generic instances, through the host emulation of the same templates: the two forms take
the same steps on the same numbers, so parameters, accumulators and the window sums' low-order parts must agree BIT FOR BIT, and
bb_stats.opt_compiled says which form ran.  BB_TUNE_OPT_SPEC=0 in the environment keeps the generic form.  The branch-free square root of
the specialised arm (bb_sqrt_nonneg, csrc/bb_math.h) against bb_sqrt from a host program built from the header."""
import os
import subprocess

import numpy as np
import pytest

import _cases as c
from conftest import make_engine
from oracle import fixtures

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The 15 x 5 fixtures of all four files, the BASELINE cuts of at most 2 000 barcodes (tile geometry of the full-size problem) and, for
# the genotype model and k_stream, small synthetic problems: (problem, environment, resident_kernel expected)
FIX = {n: (lambda n=n: fixtures.load(n)) for n in ("data001_single", "data002_hier-rep", "data003_multienv", "data004_multigen")}
CUT = {n: (lambda n=n: fixtures.synthetic(c.BASELINE_INSTANCES[n][0][0], **c.BASELINE_INSTANCES[n][0][1]))
       for n in ("C2_fitness", "C3_replicate", "C4_multienv", "multienv_replicate_even")}
CASES = ([(n, f, {}, None) for n, f in FIX.items()]
         + [(n, f, {"BB_TUNE_NB": str(c.BASELINE_INSTANCES[n][1]), "BB_TUNE_NTHR": str(c.BASELINE_INSTANCES[n][2])}, 2) for n, f in CUT.items()]
         + [("genotype_T8", lambda: c.synth("genotype_T8", seed=6), {}, 2),
            ("genotype_T5_any_parity", lambda: c.synth("genotype_T5", seed=6), {}, 2),
            ("stream_fitness", lambda: c.synth("fitness_neutral_heavy", seed=6), {"BB_TUNE_NB": "140", "BB_TUNE_NTHR": "128", "BB_TUNE_STREAM": "1"}, 3),
            ("stream_genotype", lambda: c.synth("genotype_runs", seed=6), {"BB_TUNE_NB": "110", "BB_TUNE_NTHR": "128", "BB_TUNE_STREAM": "1"}, 3),
            ("stream_replicate", lambda: c.synth("replicate_R3_T6", seed=6), {"BB_TUNE_NB": "50", "BB_TUNE_NTHR": "128", "BB_TUNE_STREAM": "1"}, 3)])


def _state(e):
    mu, om = e.get_params()
    return (mu, om) + e.opt_state()


def _same_bits(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("name,make,env,kernel", CASES, ids=[k[0] for k in CASES])
def test_specialised_equals_generic(emu_lib, monkeypatch, name, make, env, kernel):
    """12 steps with a window of 4 slots: from step 4 on a slot with non-zero contents leaves the window at every step (the
    subtraction of the compensated sum), in two runs so that the state leaves and re-enters the launch."""
    sp = make()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    outs = []
    for spec in (None, "0"):
        if spec is None:
            monkeypatch.delenv("BB_TUNE_OPT_SPEC", raising=False)
        else:
            monkeypatch.setenv("BB_TUNE_OPT_SPEC", spec)
        with make_engine(sp, emu_lib, seed=13, window=4, launch_mode=2) as e:
            st = e.stats()
            if kernel is not None:
                assert st["resident_kernel"] == kernel, st
            # (k_persist, where a fixture's odd T selects it, has the generic form only)
            assert st["opt_compiled"] == (1 if spec is None and st["resident_kernel"] >= 2 else 0), st
            e.run(5)
            e.run(7)
            assert e.stats()["steps_done"] == 12
            outs.append((st, _state(e)))
    assert outs[0][0]["resident_kernel"] == outs[1][0]["resident_kernel"]
    assert np.all(np.isfinite(outs[0][1][0])) and np.any(outs[0][1][4] != 0.0)          # (the low-order parts are in use)
    assert _same_bits(outs[0][1], outs[1][1]), [float(np.abs(x.astype(np.float64) - y.astype(np.float64)).max()) for x, y in zip(outs[0][1], outs[1][1])]


@pytest.mark.parametrize("name", ["data001_single", "data002_hier-rep", "data003_multienv", "data004_multigen"])
def test_fixtures_run_the_specialised_form_under_k_res(emu_lib, monkeypatch, name):
    """The fixtures have five time points: BB_TUNE_AP=1 puts them on k_res's any-parity form, so that every model kind's specialised
    G pass runs on them too."""
    monkeypatch.setenv("BB_TUNE_AP", "1")
    sp = fixtures.load(name)
    outs = []
    for spec in (None, "0"):
        if spec is None:
            monkeypatch.delenv("BB_TUNE_OPT_SPEC", raising=False)
        else:
            monkeypatch.setenv("BB_TUNE_OPT_SPEC", spec)
        with make_engine(sp, emu_lib, seed=13, window=4, launch_mode=2) as e:
            st = e.stats()
            assert st["resident_kernel"] == 2 and st["opt_compiled"] == (1 if spec is None else 0), st
            e.run(12)
            outs.append(_state(e))
    assert _same_bits(outs[0], outs[1])


@pytest.mark.parametrize("name", ["fitness_T6", "genotype_runs", "replicate_R3"])
@pytest.mark.parametrize("how", ["resum_every_1", "resum_every_3", "DecayedADAGrad", "two_samples", "elbo_trace"])
def test_other_configurations_keep_the_generic_form(emu_lib, name, how):
    """Whatever is not TruncatedADAGrad on the compensated sum alone, one sample per step without the ELBO trace, runs the generic
    instance -- and, where the window is exact, the literal oracle's trajectory as before."""
    sp = c.synth(name, seed=2)
    opt = "DecayedADAGrad" if how == "DecayedADAGrad" else "TruncatedADAGrad"
    kw = {"resum_every_1": dict(window=5, resum_every=1), "resum_every_3": dict(window=5, resum_every=3), "DecayedADAGrad": {},
          "two_samples": dict(window=5, resum_every=0), "elbo_trace": dict(window=5, resum_every=0, elbo_every=1)}[how]
    e, a, b, _ = c._trajectory(emu_lib, sp, 12, 2 if how == "two_samples" else 1, opt, launch_mode=2, **kw)
    st = e.stats()
    e.close()
    assert st["resident_kernel"] == 2 and st["opt_compiled"] == 0, st
    tol = 1e-10 if how in ("resum_every_1", "DecayedADAGrad") else 1e-6          # (running window: tests/_cases.py, case_trajectory_running)
    assert a < tol and b < tol, (a, b)


def test_two_kernel_step_reports_no_compiled_optimiser(emu_lib):
    with make_engine(c.synth("fitness_T6"), emu_lib, launch_mode=1) as e:
        assert e.stats()["resident_kernel"] == 0 and e.stats()["opt_compiled"] == 0


def test_branch_free_sqrt_has_the_bits_of_bb_sqrt(tmp_path):
    """bb_sqrt_nonneg against bb_sqrt on 0, the smallest subnormal, 2^-1022, both sides of 2^-900 (where bb_sqrt changes its path), 1,
    1e300, +inf and 10 000 log-uniform values of [2^-1074, 2^1000]: equal bits."""
    exe = str(tmp_path / "bb_sqrt_bits")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "barbay.jl_amd", "csrc"), os.path.join(ROOT, "tests", "bb_sqrt_bits.cpp"),
                    "-o", exe], check=True)
    edge = [0.0, 2.0 ** -1074, 2.0 ** -1022, np.nextafter(2.0 ** -900, 0.0), 2.0 ** -900, np.nextafter(2.0 ** -900, 1.0), 1.0, 1e300, np.inf]
    x = np.concatenate([edge, np.exp2(np.random.default_rng(7).uniform(-1074.0, 1000.0, 10_000))])
    assert x[1] > 0.0 and x[1] == 5e-324 and (x[len(edge):] > 0.0).all() and (x[len(edge):] < 2.0 ** -1022).sum() > 100
    x.tofile(str(tmp_path / "x.bin"))
    subprocess.run([exe, str(tmp_path / "x.bin"), str(tmp_path / "r.bin")], check=True)
    r = np.fromfile(str(tmp_path / "r.bin"), dtype=np.uint64).reshape(-1, 2)
    assert r.shape[0] == x.shape[0]
    bad = np.nonzero(r[:, 0] != r[:, 1])[0]
    assert bad.size == 0, [(float(x[i]), hex(int(r[i, 0])), hex(int(r[i, 1]))) for i in bad[:5]]
    # (and the reference is doing its job: exact where the root is exact, within an ulp elsewhere)
    ref = r[:, 0].view(np.float64)
    assert ref[0] == 0.0 and ref[6] == 1.0 and ref[4] == 2.0 ** -450 and ref[2] == 2.0 ** -511
    fin = np.isfinite(x) & (x > 0)
    assert np.abs(ref[fin] / np.sqrt(x[fin]) - 1.0).max() < 4e-16
