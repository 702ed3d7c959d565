"""The HMC session's streaming moments and metric (barbay.jl_amd/csrc/bb_hmc_accum.h) in the host emulation of the block programs
(tests/_hmc_accum_cases.py), and the part of `mcmc.hmc_ensemble` that drives them -- Stan's windows, the metric update, the segments, the
chain that is not kept -- on the diagonal Gaussian of test_emu_hmc.py with a numpy stand-in for the session (no engine)."""
import numpy as np
import pytest

import _hmc_accum_cases as ac
import barbay_jl_amd as bb
from test_emu_hmc import VAR, FakeEngine, _starts


def test_shapes_cover_the_three_kinds(emu_lib):
    ac.check_kinds(emu_lib)


@pytest.mark.parametrize("name", ac.NAMES)
def test_accumulators_bitwise(emu_lib, name):
    ac.case_accumulators(emu_lib, name)


@pytest.mark.parametrize("name", ac.NAMES)
def test_statistics(emu_lib, name):
    ac.case_statistics(emu_lib, name)


@pytest.mark.parametrize("name", ac.NAMES)
def test_rows_are_independent_bitwise(emu_lib, name):
    ac.case_independence(emu_lib, name)


@pytest.mark.parametrize("name", ac.NAMES)
def test_nothing_disturbed_bitwise(emu_lib, name):
    ac.case_nothing_disturbed(emu_lib, name)


@pytest.mark.parametrize("name", ac.NAMES)
def test_metric(emu_lib, name):
    ac.case_metric(emu_lib, name)


def test_full_width(emu_lib):
    ac.case_full_width(emu_lib)


def test_errors_and_degenerate_columns(emu_lib):
    ac.case_errors(emu_lib)


def test_end_to_end_emulated(emu_lib):
    ac.case_end_to_end(emu_lib)


# ---- hmc_ensemble's own part, no engine ----------------------------------------------------------------------------------------------
class FakeAccumEngine(FakeEngine):
    """FakeEngine with the new methods: the added states are kept as they are (statistics by numpy over all of them); every call is
    logged by name, the state after every transition m > 0 is recorded in `trace[m]`."""

    def hmc_begin(self, z0, **kw):
        self.log, self.trace, self.adds, self.metrics, self.added = ["hmc_begin"], {}, [], [], []
        return super().hmc_begin(z0, **kw)

    def hmc_step(self, transition, *a):
        self.log.append("hmc_step")
        out = super().hmc_step(transition, *a)
        if transition > 0:
            self.trace[transition] = self.z.copy()
        return out

    def hmc_get(self, grad=False):
        self.log.append("hmc_get")
        return super().hmc_get(grad)

    def hmc_end(self):
        self.log.append("hmc_end")
        super().hmc_end()

    def hmc_accum_begin(self, n_segments=1):
        self.log.append("hmc_accum_begin")
        self.S, self.added = n_segments, []

    def hmc_accum_add(self, segment=0):
        self.log.append("hmc_accum_add")
        seg = np.broadcast_to(np.asarray(segment), (self.z.shape[0],)).copy()
        assert ((seg >= -1) & (seg < self.S)).all()
        self.adds.append((len(self.trace), seg))                               # (len(trace): the number of the last transition)
        self.added += [self.z[w].copy() for w in range(len(seg)) if seg[w] >= 0]

    def hmc_accum_reset(self):
        self.log.append("hmc_accum_reset")
        self.added = []

    def hmc_accum_stats(self):
        self.log.append("hmc_accum_stats")
        x = np.array(self.added)
        nan = np.full(x.shape[1], np.nan)
        return {"mean": x.mean(axis=0), "sd": x.std(axis=0, ddof=1), "mcse": nan, "ess": nan, "rhat": nan, "within": nan, "between": nan,
                "n_total": len(x)}

    def hmc_set_metric(self, inv_mass=None):
        self.log.append("hmc_set_metric")
        self.minv = np.ones(self.z.shape[1]) if inv_mass is None else np.array(inv_mass, dtype=np.float64)
        self.metrics.append((len(self.trace), self.minv.copy()))

    def hmc_get_metric(self):
        return self.minv.copy()


def _run(n_steps=30, n_adapt=20, W=4, seed=5, minv=VAR, **kw):
    e = FakeAccumEngine()
    res = bb.mcmc.hmc_ensemble(e, _starts(seed, W), n_steps, n_adapt, rngs=[np.random.default_rng([seed, w]) for w in range(W)],
                               minv=minv, seed=seed, **kw)
    assert e.ended == 1
    return e, res


def test_adapt_windows():
    w = bb.mcmc._adapt_windows
    assert [end for _, end in w(1000)] == [100, 150, 250, 450, 950] and w(1000)[0][0] == 75
    assert all(a[1] == b[0] for a, b in zip(w(1000), w(1000)[1:]))              # contiguous
    assert w(10) == [] and w(19) == [] and w(100) == [(15, 90)] and w(149) == [(22, 135)]
    assert w(150) == [(75, 100)] and w(160) == [(75, 110)] and w(300) == [(75, 100), (100, 150), (150, 250)]


def test_metric_is_the_regularised_variance_of_the_windows_states():
    W, n_adapt = 4, 300
    e, res = _run(8, n_adapt, W, adapt_metric=True)
    windows = bb.mcmc._adapt_windows(n_adapt)
    assert [m for m, _ in e.metrics] == [end for _, end in windows] and res[0][2]["metric_windows"] == windows
    for (start, end), (_, metric) in zip(windows, e.metrics):
        x = np.concatenate([e.trace[m] for m in range(start + 1, end + 1)])      # exactly the states of the window's transitions
        K = len(x)
        assert K == W * (end - start)
        want = x.var(axis=0, ddof=1) * K / (K + 5.0) + 1e-3 * 5.0 / (K + 5.0)
        assert np.allclose(metric, want, rtol=1e-13, atol=0.0)
    assert all(lc.tolist() == [0] * W for m, lc in e.adds)                      # every add of the warm-up: all walkers, segment 0
    assert [m for m, _ in e.adds] == [m for s, t in windows for m in range(s + 1, t + 1)]
    assert all(np.array_equal(r[2]["inv_mass"], e.metrics[-1][1]) for r in res)
    # the dual averaging restarts behind a window: mu = log(10 eps), h_bar = 0, counter 1
    moves = {c[0]: c for c in e.calls if c[0] > 0}
    for _, end in windows:
        for w in range(W):
            eps_end = moves[end + 1][1][w]                                      # (the step the window's last update left)
            out = moves[end + 1][4]
            alpha = 0.0 if out["divergent"][w] else min(1.0, float(np.exp(min(0.0, out["h1"][w] - out["h0"][w]))))
            h_bar = (0.65 - alpha) / 11.0
            assert moves[end + 2][1][w] == float(np.exp(np.log(10.0 * eps_end) - 1.0 / 0.05 * h_bar))
    with pytest.raises(bb.BarBayError, match="one n_adapt"):
        _run(8, [30, 40], 2, adapt_metric=True)


# From the unit metric, which is off by a factor 4 in two coordinates of three: 8 walkers, n_adapt = 300.  Seeds 0 .. 9 were scanned with
# the stand-in; every one passes (the last window holds 800 states: a variance estimate good to ~10 %).  Measured at ADAPT_SEED, final
# inv_mass / VAR per coordinate: see ADAPT_RATIOS (recorded, not an input).
ADAPT_SEED = 0
ADAPT_RATIOS = (0.956, 0.777, 1.123, 0.975, 0.889, 0.953, 1.094, 1.191, 0.870)     # (over seeds 0 .. 9: 0.777 .. 1.208)


def test_adapted_metric_finds_the_variances():
    _, res = _run(4, 300, 8, seed=ADAPT_SEED, minv=None, adapt_metric=True)
    ratio = res[0][2]["inv_mass"] / VAR
    print("inv_mass / VAR", np.round(ratio, 3))
    assert np.all(ratio > 0.5) and np.all(ratio < 2.0)


def test_defaults_make_no_new_call():
    e, _ = _run()
    assert set(e.log) == {"hmc_begin", "hmc_step", "hmc_get", "hmc_end"}
    plain = FakeEngine()
    ref = bb.mcmc.hmc_ensemble(plain, _starts(5, 4), 30, 20, rngs=[np.random.default_rng([5, w]) for w in range(4)], minv=VAR, seed=5)
    _, res = _run()
    for a, b in zip(ref, res):
        assert ac.same(a[0], b[0]) and ac.same(a[1], b[1]) and a[2] == b[2]


def test_segments_and_the_chain_that_is_not_kept():
    S, n_adapt, thin = 3, 20, 2
    n_st = [9, 6]
    e, res = _run(n_st, n_adapt, 2, segments=S, thin=thin)
    assert "hmc_accum_reset" not in e.log                                       # (nothing was added during the warm-up)
    want = {}
    for w in range(2):
        for k in range(n_st[w]):
            want.setdefault(n_adapt + (k + 1) * thin, np.full(2, -1))[w] = S * k // n_st[w]
    assert [m for m, _ in e.adds] == sorted(want) and all(np.array_equal(seg, want[m]) for m, seg in e.adds)
    x = np.concatenate([r[0] for r in res])
    assert res[0][2]["stream"]["n_total"] == 15 and res[0][2]["stream"] is res[1][2]["stream"]
    assert np.allclose(res[0][2]["stream"]["mean"], x.mean(axis=0), rtol=1e-13) and np.allclose(res[0][2]["stream"]["sd"], x.std(axis=0, ddof=1), rtol=1e-13)
    lean_e, lean = _run(n_st, n_adapt, 2, segments=S, thin=thin, keep_chain=False)
    assert "hmc_get" not in lean_e.log and [r[0].shape for r in lean] == [(0, VAR.shape[0])] * 2 and [r[1].shape for r in lean] == [(0,)] * 2
    assert ac.same(lean[0][2]["stream"]["mean"], res[0][2]["stream"]["mean"]) and lean[0][2]["step_size"] == res[0][2]["step_size"]
    # with the adapted metric the warm-up's moments are reset before the kept draws
    e2, res2 = _run(8, 100, 3, segments=2, adapt_metric=True)
    assert e2.log.count("hmc_accum_reset") == 2 and res2[0][2]["stream"]["n_total"] == 24
    with pytest.raises(bb.BarBayError, match="keep_chain"):
        _run(keep_chain=False)
    with pytest.raises(bb.BarBayError, match="segments"):
        _run(5, 20, 2, segments=3)
    with pytest.raises(bb.BarBayError, match="segments"):
        _run(segments=9)
