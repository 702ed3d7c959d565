"""`mcmc.summarize` and `mcmc_sample(summary=True)`: the chain diagnostics of `bb_chain_summary` at the user's entry points
(host emulation of the engine)."""
import os

import numpy as np
import pandas as pd
import pytest

import barbay_jl_amd as bb
import _chain_cases as cc
import _ppc_cases as pc
from conftest import make_engine

GOLD = os.path.join(os.path.dirname(__file__), "golden")
COLUMNS = ["parameters", "mean", "std", "mcse", "ess", "rhat", "q2.5", "q25", "q50", "q75", "q97.5"]


def sample(lib, **kw):
    data = pd.read_csv(os.path.join(GOLD, "data001_single.csv"))
    return bb.mcmc.mcmc_sample(data=data, model=bb.model.fitness_normal, verbose=False, seed=3, engine_kwargs={"_lib": lib}, **kw)


@pytest.fixture(scope="module")
def run(emu_lib):
    # 400 draws a walker: at 150 the largest R-hat of this unconverged run moved between 2.4 and 3.5 with the last bits of the gradient
    # (another seed, or a rounding-level change in bb_logdensity_grad), around the 3.0 asserted below; at 400 it is 1.4
    return sample(emu_lib, n_walkers=2, n_steps=400, outputname=None, advi_steps=1500, summary=True)


def test_default_output_keys_are_unchanged(emu_lib, tmp_path):
    out = sample(emu_lib, n_walkers=1, n_steps=4, outputname=None, advi_steps=50)
    assert list(out) == ["ids", "var_names", "chain", "logp", "step_size"]
    assert sample(emu_lib, n_walkers=1, n_steps=4, outputname=str(tmp_path / "c"), advi_steps=50) is None
    with np.load(str(tmp_path / "c.npz"), allow_pickle=True) as z:
        assert sorted(z.files) == sorted(out)


def test_summary_arrays_equal_chain_summary(run, emu_lib):
    assert list(run)[:5] == ["ids", "var_names", "chain", "logp", "step_size"]
    assert sorted(k for k in run if k.startswith("summary_")) == sorted(
        "summary_" + k for k in ("mean", "std", "mcse", "ess", "rhat", "quantiles", "probs", "n_lags"))
    with make_engine(pc.spec("fitness"), emu_lib, seed=2) as e:
        ref = e.chain_summary(run["chain"])
    for k, src in (("mean", "mean"), ("std", "sd"), ("mcse", "mcse"), ("ess", "ess"), ("rhat", "rhat"), ("quantiles", "quantiles"),
                   ("n_lags", "n_lags")):
        assert cc.same_bits({k: run["summary_" + k]}, {k: ref[src]}), k
    assert np.array_equal(run["summary_probs"], [0.025, 0.25, 0.5, 0.75, 0.975])
    D = run["chain"].shape[2]
    assert run["summary_quantiles"].shape == (D, 5) and run["summary_n_lags"].dtype == np.int32
    assert np.isfinite(run["summary_ess"]).all() and (run["summary_ess"] > 1).all() and (run["summary_ess"] <= 800 * np.log10(800)).all()
    assert (run["summary_rhat"] > 0.9).all() and (run["summary_rhat"] < 3.0).all()        # 400 draws a walker: not converged, but sane
    assert np.allclose(run["summary_mean"], run["chain"].reshape(-1, D).mean(0), rtol=1e-10, atol=1e-12)


def test_summarize_table(run, emu_lib, tmp_path):
    df = bb.mcmc.summarize(run)
    assert list(df.columns) == COLUMNS
    assert list(df["parameters"]) == [str(v) for v in run["var_names"]]
    assert np.array_equal(df["std"].to_numpy(), run["summary_std"]) and np.array_equal(df["q97.5"].to_numpy(), run["summary_quantiles"][:, 4])
    # an output without the arrays: through a handle of the caller's, and through summarize's own; from the .npz too
    bare = {k: v for k, v in run.items() if not k.startswith("summary_")}
    with make_engine(pc.spec("fitness"), emu_lib, seed=2) as e:
        d2 = bb.mcmc.summarize(bare, e)
    np.savez(str(tmp_path / "chain.npz"), **bare)
    d3 = bb.mcmc.summarize(str(tmp_path / "chain"), _lib=emu_lib)
    d4 = bb.mcmc.summarize(str(tmp_path / "chain.npz"), _lib=emu_lib, probs=(0.1, 0.9))
    assert df.equals(d2) and df.equals(d3)
    assert list(d4.columns) == COLUMNS[:6] + ["q10", "q90"] and d4[COLUMNS[:6]].equals(df[COLUMNS[:6]])


def test_summary_limits_fail_before_sampling(emu_lib, monkeypatch, tmp_path):
    """n_walkers * n_steps > BB_CHAIN_MAX_K, or n_steps < 4, with summary=True: refused from the arguments, before the data is
    read, a handle is made or a draw is taken (a chain sampled first would be lost with the exception), and nothing is written."""
    def no_work(*a, **k):
        raise AssertionError("work was started before the summary's limits were checked")
    for name in ("nuts", "nuts_ensemble"):
        monkeypatch.setattr(bb.mcmc, name, no_work)
    monkeypatch.setattr(bb.mcmc._vi, "make_engine", no_work)
    monkeypatch.setattr(bb.mcmc.utils, "data_to_arrays", no_work)
    for kw in (dict(n_walkers=4, n_steps=5000), dict(n_walkers=2, n_steps=8193), dict(n_walkers=2, n_steps=3),
               dict(n_walkers=64, n_steps=257, ensemble="batched")):
        with pytest.raises(bb.model.BarBayError, match="n_walkers \\* n_steps <= 16384"):
            sample(emu_lib, outputname=str(tmp_path / "big"), summary=True, **kw)
        assert not os.path.exists(str(tmp_path / "big.npz"))
    with pytest.raises(AssertionError, match="work was started"):                  # 4 x 4096 = 16 384 passes the check
        sample(emu_lib, outputname=None, summary=True, n_walkers=4, n_steps=4096)
    with pytest.raises(AssertionError, match="work was started"):                  # and summary=False has no such limit
        sample(emu_lib, outputname=None, n_walkers=4, n_steps=5000)


def test_summarize_recomputes_what_the_stored_arrays_do_not_answer(run, emu_lib):
    """An output that carries summary_* arrays: other probabilities or a lag bound are computed from the chain, not ignored."""
    df = bb.mcmc.summarize(run)
    with make_engine(pc.spec("fitness"), emu_lib, seed=2) as e:
        same = bb.mcmc.summarize(run, e, probs=(0.025, 0.25, 0.5, 0.75, 0.975))
        d2 = bb.mcmc.summarize(run, e, probs=(0.1, 0.9))
        d3 = bb.mcmc.summarize(run, e, max_lag=2)
        ref2 = e.chain_summary(run["chain"], (0.1, 0.9))
        ref3 = e.chain_summary(run["chain"], max_lag=2)
    d4 = bb.mcmc.summarize(run, _lib=emu_lib, probs=(0.1, 0.9))
    assert same.equals(df)
    assert list(d2.columns) == COLUMNS[:6] + ["q10", "q90"] and d2.equals(d4) and d2[COLUMNS[:6]].equals(df[COLUMNS[:6]])
    assert np.array_equal(d2[["q10", "q90"]].to_numpy(), ref2["quantiles"])
    assert list(d3.columns) == COLUMNS and np.array_equal(d3["ess"].to_numpy(), ref3["ess"])
    assert (ref3["n_lags"] <= 2).all() and (run["summary_n_lags"] > 2).any() and not d3["ess"].equals(df["ess"])
