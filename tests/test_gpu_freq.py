"""bb_freq_bands (frequency-trajectory bands, barbay.jl_amd/csrc/bb_freq.h) on the device: the emulation cases, independence of the
launch mode, a statistical check, and the user entry point end to end."""
import os

import numpy as np
import pandas as pd
import pytest

import _freq_cases as fc
from conftest import make_engine

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
DRIFT = 0.42          # planted misfit: factor per time step (chosen in the host emulation, see test_planted_drift_ranks_first)


@pytest.mark.parametrize("mode", ["trajectory", "posterior"])
@pytest.mark.parametrize("name", fc.CASES)
def test_freq_bands_match_restatement(hip_lib, name, mode):
    fc.case_freq(hip_lib, name, mode)


def test_freq_extreme_posterior(hip_lib):
    fc.case_extreme(hip_lib)


def test_independent_of_launch_mode(hip_lib):
    import barbay_jl_amd as bb
    sp = fc.spec("fitness")
    out = []
    for lm in (1, 2):
        with bb.Engine(sp.kind, sp.counts, sp.n_neutral, sp.n_bc, seed=4, launch_mode=lm, _lib=hip_lib) as e:
            if lm == 1:
                mu, om = fc.tame(e)
            e.set_params(mu, om)
            out.append([e.freq_bands(fc.QS, mode="trajectory", n_samples=500, n_ppc=4, seed=2),
                        e.freq_bands(fc.QS, mode="posterior", n_samples=500, n_ppc=1, seed=2)])
    for a, b in zip(*out):
        assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and np.array_equal(a[1], b[1])


def test_bands_against_a_large_numpy_sample(hip_lib):
    """One mutant row and time point of a small handle: the device's K = 10 000 quantiles (n_ppc = 1, so the K trajectories are
    independent) against 400 000 independent numpy trajectories, within 6 Monte-Carlo errors."""
    sp = fc.spec("fitness")
    off = sp.offsets()
    m, t = 23, 3
    b = sp.n_neutral + m
    T, B = sp.n_time[0], sp.B
    with make_engine(sp, hip_lib, seed=4) as e:
        e.run(3)
        fc.tame(e)
        mean, sigma = e.posterior()
        bands, _ = e.freq_bands(fc.QS, mode="trajectory", n_samples=10_000, n_ppc=1, seed=17, outside=False)
    g = np.random.default_rng(0)
    n = 400_000

    def draw(i):
        return g.normal(mean[i], sigma[i], n)

    lo = off["loglambda"][0]
    z = np.zeros(n)
    for bb_ in range(B):
        lam = np.exp(draw(lo + bb_ * T))
        z += lam
        if bb_ == b:
            x = lam
    x = x / z
    s, sd = draw(off["s_bc"][0] + m), np.exp(draw(off["logsigma_bc"][0] + m))
    for tt in range(t):
        x = x * np.exp(g.normal(s - draw(off["s_pop"][0] + tt), sd))
    for i, q in enumerate(fc.QS):
        for side, p in enumerate(((1 - q) / 2, 1 - (1 - q) / 2)):
            dq = np.quantile(x, min(p + 0.01, 1)) - np.quantile(x, max(p - 0.01, 0))
            dens_inv = dq / (min(p + 0.01, 1) - max(p - 0.01, 0))
            se = np.sqrt(p * (1 - p) / 10_000) * dens_inv
            assert abs(bands[b, t, i, side] - np.quantile(x, p)) < 6 * se, (q, side)


@pytest.fixture(scope="module")
def fit():
    import barbay_jl_amd as bb
    data = pd.read_csv(os.path.join(GOLD, "data001_single.csv"))
    return data, bb.vi.advi(data=data, model=bb.model.fitness_normal, advi=bb.vi.ADVI(1, 3000), verbose=False, seed=1)


def test_freq_ppc_bands_end_to_end(fit):
    import barbay_jl_amd as bb
    data, df = fit
    out = bb.stats.freq_ppc_bands(data, df, model=bb.model.fitness_normal, n_samples=500, n_ppc=10, seed=3)
    n_all = data["barcode"].nunique()
    T = data["time"].nunique()
    assert list(out.columns) == ["id", "neutral", "rep", "env", "time", "quantile", "lower", "upper", "observed", "n_outside"]
    assert len(out) == n_all * T * 3
    assert not out.duplicated(["id", "time", "quantile"]).any()
    assert set(out["id"]) == set(data["barcode"]) and set(out["time"]) == set(range(T))
    assert set(out.loc[out["neutral"], "id"]) == set(data.loc[data["neutral"], "barcode"])
    assert (out["lower"] <= out["upper"]).all() and np.isfinite(out[["lower", "upper"]].to_numpy()).all() and (out["lower"] >= 0).all()
    times = np.sort(data["time"].unique())
    d = data.assign(t=np.searchsorted(times, data["time"].to_numpy()))
    d["freq"] = d["count"] / d.groupby("t")["count"].transform("sum")
    chk = out.merge(d[["barcode", "t", "freq"]], left_on=["id", "time"], right_on=["barcode", "t"])
    assert len(chk) == len(out) and np.array_equal(chk["observed"].to_numpy(), chk["freq"].to_numpy())
    post = bb.stats.freq_ppc_bands(data, df, model=bb.model.fitness_normal, mode="posterior", n_samples=500, seed=3)
    assert len(post) == len(out) and (post["upper"] <= 1).all()
    with pytest.raises(bb.BarBayError):
        bb.stats.freq_ppc_bands(data, df.iloc[3:], model=bb.model.fitness_normal)


def test_planted_drift_ranks_first(fit):
    """A barcode whose counts are changed after the fit to drift steadily away from its fitted trajectory -- count_t times DRIFT^t,
    the same direction at every time point -- has the most time points outside its 95 % trajectory band, although every one of
    its single-step ratios stays inside its bb_ppc_bands 95 % band.

    DRIFT = 0.42 per step, chosen on the CPU (the same fit and calls through the host emulation).  On this 15-barcode data set
    the bands are wide: at 1.5 (and at 1 / 1.5) per step the barcode stays inside BOTH kinds of band at every time point, so that
    factor shows nothing.  At 0.42 the four ratios lie 0.10, 0.34, 0.70 and 0.22 above their lower band ends, while the observed
    frequency is 0.86, 0.88 and 0.54 of the trajectory band's lower end at time points 2, 3 and 4: three outside, every other
    barcode one.  (0.44: two outside; 0.40: the first ratio is 0.05 from its band end.  Upwards, 2.0 gives two outside with the third
    ratio 0.09 from its upper end, and 2.2 puts that ratio outside.)"""
    import barbay_jl_amd as bb
    data, df = fit
    times = np.sort(data["time"].unique())
    bad = sorted(data.loc[~data["neutral"], "barcode"].unique())[4]
    d2 = data.copy()
    sel = (d2["barcode"] == bad).to_numpy()
    step = np.searchsorted(times, d2.loc[sel, "time"].to_numpy())
    d2.loc[sel, "count"] = np.maximum(1, np.round(d2.loc[sel, "count"].to_numpy() * DRIFT ** step)).astype(np.int64)
    kw = dict(model=bb.model.fitness_normal, quantiles=(0.95,), n_samples=1000, n_ppc=10)
    ratio = bb.stats.logfreq_ratio_ppc_bands(d2, df, **kw)
    assert ratio.loc[ratio["id"] == bad, "n_outside"].iloc[0] == 0
    out = bb.stats.freq_ppc_bands(d2, df, **kw)
    per = out[~out["neutral"]].groupby("id")["n_outside"].first().sort_values(ascending=False)
    assert per.index[0] == bad and per.iloc[0] > per.iloc[1], per
