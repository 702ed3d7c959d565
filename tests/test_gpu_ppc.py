"""bb_ppc_bands (posterior predictive bands, barbay.jl_amd/csrc/bb_ppc.h) on the device: the emulation cases, the full-size
C2 shape against the numpy restatement, determinism, a statistical check, and the user entry point end to end."""
import os

import numpy as np
import pandas as pd
import pytest

import _ppc_cases as pc
from oracle.spec import ModelSpec

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
QS = (0.95, 0.675, 0.05)


@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_ppc_bands_match_restatement(hip_lib, name):
    pc.case_ppc(hip_lib, name)


def test_buffer_reuse_across_calls_and_sizes(hip_lib):
    pc.case_buffer_reuse(hip_lib)


@pytest.fixture(scope="module")
def c2(hip_lib):
    import barbay_jl_amd as bb
    w = bb.synth.fitness_normal()
    sp = ModelSpec("fitness", w.counts, [c.sum(axis=1) for c in w.counts], w.n_neutral, w.n_bc)
    e = bb.Engine("fitness", w.counts, w.n_neutral, w.n_bc, seed=3, _lib=hip_lib)
    e.run(20)
    yield sp, e
    e.close()


def test_c2_full_size_against_restatement(c2):
    sp, e = c2
    mu, om = e.get_params()
    bands, nout = e.ppc_bands(QS, n_samples=1000, n_ppc=10, seed=7)
    assert bands.shape == (1 + sp.n_bc, 7, 3, 2) and not np.isnan(bands).any()
    rows = np.sort(np.random.default_rng(1).choice(bands.shape[0], 64, replace=False))
    rows[0] = 0                                                  # the population-mean row
    b2, n2 = pc.restate(sp, mu, om, QS, 1000, 10, 7, rows=rows)
    pc.assert_bands_close(bands[rows], b2)
    assert np.array_equal(nout[rows], n2)
    again, nout2 = e.ppc_bands(QS, n_samples=1000, n_ppc=10, seed=7)
    assert np.array_equal(bands.view(np.uint64), again.view(np.uint64)) and np.array_equal(nout, nout2)


def test_independent_of_launch_mode(hip_lib):
    import barbay_jl_amd as bb
    sp = pc.spec("fitness")
    out = []
    for mode in (1, 0):
        with bb.Engine(sp.kind, sp.counts, sp.n_neutral, sp.n_bc, seed=4, launch_mode=mode, _lib=hip_lib) as e:
            if mode == 1:
                mu, om = e.get_params()
            e.set_params(mu, om)
            out.append(e.ppc_bands(QS, n_samples=500, n_ppc=4, seed=2))
    assert np.array_equal(out[0][0].view(np.uint64), out[1][0].view(np.uint64)) and np.array_equal(out[0][1], out[1][1])


def test_bands_against_a_large_numpy_sample(c2):
    """One mutant row and step: the device's K = 10 000 quantiles against 400 000 independent draws, within 6 Monte-Carlo errors."""
    sp, e = c2
    mean, sigma = e.posterior()
    off = sp.offsets()
    m, t = 123, 3
    row = 1 + m
    bands, _ = e.ppc_bands(QS, n_samples=1000, n_ppc=10, seed=17, outside=False)
    g = np.random.default_rng(0)
    n = 400_000

    def draw(i):
        return g.normal(mean[i], sigma[i], n)

    x = g.normal(draw(off["s_bc"][0] + m) - draw(off["s_pop"][0] + t), np.exp(draw(off["logsigma_bc"][0] + m)))
    for i, q in enumerate(QS):
        for side, p in enumerate(((1 - q) / 2, 1 - (1 - q) / 2)):
            dq = np.quantile(x, min(p + 0.01, 1)) - np.quantile(x, max(p - 0.01, 0))
            dens_inv = dq / (min(p + 0.01, 1) - max(p - 0.01, 0))
            se = np.sqrt(p * (1 - p) / 10_000) * dens_inv
            assert abs(bands[row, t, i, side] - np.quantile(x, p)) < 6 * se, (q, side)


def _fit(data):
    import barbay_jl_amd as bb
    return bb.vi.advi(data=data, model=bb.model.fitness_normal, advi=bb.vi.ADVI(1, 3000), verbose=False, seed=1)


def test_logfreq_ratio_ppc_bands_end_to_end():
    import barbay_jl_amd as bb
    data = pd.read_csv(os.path.join(GOLD, "data001_single.csv"))
    df = _fit(data)
    out = bb.stats.logfreq_ratio_ppc_bands(data, df, model=bb.model.fitness_normal, n_samples=500, n_ppc=10, seed=3)
    n_bc = data.loc[~data["neutral"], "barcode"].nunique()
    T = data["time"].nunique()
    assert len(out) == (1 + n_bc) * (T - 1) * 3
    assert set(out["id"]) == {"neutral"} | set(data.loc[~data["neutral"], "barcode"])
    assert list(out.columns) == ["id", "rep", "env", "time", "quantile", "lower", "upper", "n_outside"]
    assert (out["lower"] <= out["upper"]).all() and np.isfinite(out[["lower", "upper"]].to_numpy()).all()
    w = out.pivot_table(index=["id", "time"], columns="quantile", values="upper")
    assert (w[0.95] >= w[0.675]).all() and (w[0.675] >= w[0.05]).all()
    with pytest.raises(bb.BarBayError):
        bb.stats.logfreq_ratio_ppc_bands(data, df.iloc[3:], model=bb.model.fitness_normal)


def test_planted_misfit_ranks_first():
    """A barcode whose counts are changed after the fit (up and down by 30x at alternate time points) has the most observed
    ratios outside its 95 % band."""
    import barbay_jl_amd as bb
    data = pd.read_csv(os.path.join(GOLD, "data001_single.csv"))
    df = _fit(data)
    bad = sorted(data.loc[~data["neutral"], "barcode"].unique())[4]
    d2 = data.copy()
    sel = d2["barcode"] == bad
    fac = np.where(d2.loc[sel, "time"].to_numpy() % 2 == 0, 30.0, 1.0 / 30.0)
    d2.loc[sel, "count"] = np.maximum(1, np.round(d2.loc[sel, "count"].to_numpy() * fac)).astype(np.int64)
    out = bb.stats.logfreq_ratio_ppc_bands(d2, df, model=bb.model.fitness_normal, quantiles=(0.95,), n_samples=1000, n_ppc=10)
    per = out[out["id"] != "neutral"].groupby("id")["n_outside"].first().sort_values(ascending=False)
    assert per.index[0] == bad and per.iloc[0] > per.iloc[1], per
