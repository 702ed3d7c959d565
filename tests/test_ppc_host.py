"""Host ports of the reference's posterior-predictive helpers (src/stats.jl:55-1000; test/stats_tests.jl:16-130)."""
import numpy as np
import pandas as pd
import pytest

import barbay_jl_amd as bb
from barbay_jl_amd import stats


def test_matrix_quantile_range_against_numpy():
    x = np.random.default_rng(0).normal(size=(10, 5))
    qs = [0.95, 0.675, 0.05, 1.0, 0.0]
    r = stats.matrix_quantile_range(qs, x)
    assert r.shape == (5, len(qs), 2)
    for i, q in enumerate(qs):
        assert np.allclose(r[:, i, 0], np.quantile(x, (1 - q) / 2, axis=0), rtol=1e-14, atol=1e-15)
        assert np.allclose(r[:, i, 1], np.quantile(x, 1 - (1 - q) / 2, axis=0), rtol=1e-14, atol=1e-15)
    assert np.all(r[:, :, 1] >= r[:, :, 0])
    r1 = stats.matrix_quantile_range([0.9], x, dims=1)
    assert r1.shape == (10, 1, 2)
    assert np.allclose(r1[:, 0, 0], np.quantile(x, 0.05, axis=1), rtol=1e-14)


@pytest.mark.parametrize("kw", [dict(quantile=[1.5]), dict(quantile=[-0.5]), dict(quantile=[0.9], dims=3)])
def test_matrix_quantile_range_errors(kw):
    with pytest.raises(bb.BarBayError):
        stats.matrix_quantile_range(kw.pop("quantile"), np.zeros((4, 3)), **kw)


def _frame(n=100, std=None, seed=1):
    g = np.random.default_rng(seed)
    sd = np.abs(g.normal(size=n)) if std is None else np.full(n, std)
    return pd.DataFrame({"s⁽ᵐ⁾": g.normal(size=n), "σ⁽ᵐ⁾": sd, "f̲⁽ᵐ⁾[1]": np.abs(g.normal(size=n)),
                         "s̲ₜ₁": g.normal(size=n), "s̲ₜ₂": g.normal(size=n)})


def test_freq_bc_ppc_shapes_and_model():
    df = _frame()
    assert stats.freq_bc_ppc(df, 10).shape == (1000, 3)
    raw = stats.freq_bc_ppc(df, 10, flatten=False, rng=np.random.default_rng(3))
    assert raw.shape == (100, 3, 10)
    flat = stats.freq_bc_ppc(df, 10, rng=np.random.default_rng(3))
    assert np.array_equal(flat, raw.transpose(2, 0, 1).reshape(-1, 3))
    assert np.array_equal(raw[:, 0, :], np.repeat(df["f̲⁽ᵐ⁾[1]"].to_numpy()[:, None], 10, axis=1))
    assert stats.freq_bc_ppc(df, 5, model="normal").shape == (500, 3)
    with pytest.raises(bb.BarBayError, match="model must be"):
        stats.freq_bc_ppc(df, 5, model="poisson")


def test_logfreq_ratio_ppc_shapes_and_params():
    df = _frame()
    assert stats.logfreq_ratio_bc_ppc(df, 10).shape == (1000, 2)
    assert stats.logfreq_ratio_bc_ppc(df, 10, flatten=False).shape == (100, 2, 10)
    d2 = pd.DataFrame({"fit": df["s⁽ᵐ⁾"], "err": df["σ⁽ᵐ⁾"], "pop_a": df["s̲ₜ₁"], "pop_b": df["s̲ₜ₂"], "sd_a": 0.1, "sd_b": 0.2})
    p = {"bc_mean_fitness": "fit", "bc_std_fitness": "err", "population_mean_fitness": "pop_"}
    assert stats.logfreq_ratio_bc_ppc(d2, 4, param=p).shape == (400, 2)
    pp = {"population_mean_fitness": "pop_", "population_std_fitness": "sd_"}
    assert stats.logfreq_ratio_popmean_ppc(d2, 4, param=pp).shape == (400, 2)
    with pytest.raises(bb.BarBayError, match="does not match"):
        stats.logfreq_ratio_popmean_ppc(d2.drop(columns="sd_b"), 4, param=pp)
    dm = pd.DataFrame({"s̲ₜ[1]": df["s̲ₜ₁"], "s̲ₜ[2]": df["s̲ₜ₂"], "s̲⁽ᵐ⁾[1]": 0.1, "s̲⁽ᵐ⁾[2]": 0.5, "σ̲⁽ᵐ⁾[1]": 0.0, "σ̲⁽ᵐ⁾[2]": 0.0})
    assert stats.logfreq_ratio_multienv_ppc(dm, 6, ["a", "b", "a"]).shape == (600, 2)
    assert stats.logfreq_ratio_multienv_ppc(dm, 6, ["a", "b", "a"], flatten=False).shape == (100, 2, 6)
    with pytest.raises(bb.BarBayError, match="environments does not match"):
        stats.logfreq_ratio_multienv_ppc(dm, 6, ["a", "b", "a", "b"])
    with pytest.raises(bb.BarBayError, match="# of mutant-related"):
        stats.logfreq_ratio_multienv_ppc(dm, 6, ["a", "b", "c"])


def test_degenerate_spread_pins_means_and_order():
    """std = -inf: exp(std) = 0, every draw is its mean -- the flatten order and the env-of-the-later-time-point rule exactly."""
    n = 7
    g = np.random.default_rng(4)
    s, st1, st2, ls1, ls2 = g.normal(size=(5, n))
    df = pd.DataFrame({"s⁽ᵐ⁾": s, "σ⁽ᵐ⁾": -np.inf, "s̲ₜ₁": st1, "s̲ₜ₂": st2})
    out = stats.logfreq_ratio_bc_ppc(df, 3)
    want = np.tile(np.stack([s - st1, s - st2], axis=1), (3, 1))
    assert np.array_equal(out, want)
    dp = pd.DataFrame({"sₜ[1]": st1, "sₜ[2]": st2, "σₜ[1]": -np.inf, "σₜ[2]": -np.inf})
    assert np.array_equal(stats.logfreq_ratio_popmean_ppc(dp, 2), np.tile(np.stack([-st1, -st2], axis=1), (2, 1)))
    dm = pd.DataFrame({"s̲ₜ[1]": st1, "s̲ₜ[2]": st2, "s̲⁽ᵐ⁾[1]": ls1, "s̲⁽ᵐ⁾[2]": ls2, "σ̲⁽ᵐ⁾[1]": -np.inf, "σ̲⁽ᵐ⁾[2]": -np.inf})
    out = stats.logfreq_ratio_multienv_ppc(dm, 2, ["x", "y", "x"], flatten=False)
    assert np.array_equal(out[:, 0, 1], ls2 - st1) and np.array_equal(out[:, 1, 0], ls1 - st2)
    f = stats.freq_bc_ppc(pd.DataFrame({"s⁽ᵐ⁾": s, "σ⁽ᵐ⁾": 0.0, "f̲⁽ᵐ⁾[1]": 1.0, "s̲ₜ₁": st1, "s̲ₜ₂": st2}), 2, flatten=False)
    assert np.allclose(f[:, 2, 0], np.exp(s - st1) * np.exp(s - st2), rtol=1e-15)


def test_lexicographic_column_order_quirk():
    """11 time steps: the reference's `sort` compares the names character by character, and
    '0' < ']', so s̲ₜ[10], s̲ₜ[11] come first, before s̲ₜ[1] and s̲ₜ[2]; the port keeps that order."""
    n = 4
    cols = {f"s̲ₜ[{t}]": np.full(n, float(t)) for t in range(1, 12)}
    df = pd.DataFrame({"s⁽ᵐ⁾": 0.0, "σ⁽ᵐ⁾": -np.inf, **cols})
    out = stats.logfreq_ratio_bc_ppc(df, 1)
    assert list(-out[0]) == [10.0, 11.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0]
