"""The device-resident HMC session (barbay.jl_amd/csrc/bb_hmc.h) in the host emulation of the block programs (tests/_hmc_cases.py), and
the pure-Python part of `mcmc.hmc_ensemble` on a known Gaussian with a numpy stand-in for the session (no engine)."""
import numpy as np
import pytest

import _hmc_cases as hc
import barbay_jl_amd as bb


@pytest.mark.parametrize("name", hc.NAMES)
def test_transition_against_host(emu_lib, name):
    hc.case_transition_against_host(emu_lib, name)


@pytest.mark.parametrize("name", hc.NAMES)
def test_walkers_are_independent_bitwise(emu_lib, name):
    hc.case_independence(emu_lib, name)


@pytest.mark.parametrize("name", hc.NAMES)
def test_session_leaves_state_untouched(emu_lib, name):
    hc.case_state_untouched(emu_lib, name)


def test_full_width(emu_lib):
    hc.case_full_width(emu_lib)


def test_errors(emu_lib):
    hc.case_errors(emu_lib)


def test_sampler_agrees_with_nuts_emulated(emu_lib):
    hc.case_sampler_agrees_with_nuts(emu_lib)


# ---- hmc_ensemble's own part, no engine: a numpy stand-in for the session on the diagonal Gaussian of test_emu_logp_batch.py --------
VAR = np.array([1.0, 4.0, 0.25] * 3)


class FakeSession:
    def __init__(self, logp):
        self.logp = logp


class FakeEngine:
    """hmc_begin / hmc_step / hmc_get / hmc_end with the arithmetic of include/barbay_hip.h in numpy; walker w's momenta of a transition
    come from default_rng([seed, transition, w]).  Every hmc_step call is recorded."""

    def hmc_begin(self, z0, *, seed=0, inv_mass=None):
        self.z = np.array(z0, dtype=np.float64)
        self.minv = np.ones(self.z.shape[1]) if inv_mass is None else np.asarray(inv_mass, dtype=np.float64)
        self.seed, self.calls, self.ended = seed, [], 0
        self.lp = np.array([self.f(z)[0] for z in self.z])
        return FakeSession(self.lp.copy())

    @staticmethod
    def f(z):
        return -0.5 * float(np.sum(z * z / VAR)), -z / VAR

    def hmc_step(self, transition, eps, n_leapfrog, log_u):
        W = self.z.shape[0]
        eps, L, lu = (np.broadcast_to(np.asarray(a), (W,)) for a in (eps, n_leapfrog, log_u))
        out = {k: np.zeros(W, dtype=np.int32 if k in ("accepted", "divergent") else np.float64) for k in hc.FIELDS}
        for w in range(W):
            r = np.random.default_rng([self.seed, transition, w]).standard_normal(self.z.shape[1]) / np.sqrt(self.minv)
            z, (lp, g) = self.z[w].copy(), self.f(self.z[w])
            k0 = 0.5 * np.sum(self.minv * r * r)
            for _ in range(int(L[w])):
                r = r + 0.5 * eps[w] * g
                z = z + eps[w] * self.minv * r
                lp, g = self.f(z)
                r = r + 0.5 * eps[w] * g
            k1 = 0.5 * np.sum(self.minv * r * r)
            h0, h1 = self.lp[w] - k0, lp - k1
            ok = bool(np.isfinite(h1) and lu[w] < h1 - h0)
            if ok:
                self.z[w], self.lp[w] = z, lp
            for k, v in zip(hc.FIELDS, (h0, h1, k0, k1, lp, self.lp[w], int(ok), int(not np.isfinite(h1)))):
                out[k][w] = v
        self.calls.append((transition, eps.copy(), L.copy(), lu.copy(), out))
        return out

    def hmc_get(self, grad=False):
        return self.z.copy(), self.lp.copy()

    def hmc_end(self):
        self.ended += 1


def _starts(seed, W):
    return [np.random.default_rng([seed, 100 + w]).standard_normal(VAR.shape[0]) for w in range(W)]


def _run(n_steps=30, n_adapt=20, W=4, seed=5, **kw):
    e = FakeEngine()
    res = bb.mcmc.hmc_ensemble(e, _starts(seed, W), n_steps, n_adapt, rngs=[np.random.default_rng([seed, w]) for w in range(W)],
                               minv=VAR, seed=seed, **kw)
    assert e.ended == 1
    return e, res


def test_ensemble_draws_and_dual_averaging():
    n_adapt, n_steps, W, seed = 20, 30, 4, 5
    e, res = _run(n_steps, n_adapt, W, seed, n_leapfrog=(3, 6), target_accept=0.65)
    probes = [c for c in e.calls if c[0] == 0]
    moves = [c for c in e.calls if c[0] > 0]
    assert [c[0] for c in moves] == list(range(1, n_adapt + n_steps + 1))
    assert all((c[2] == 1).all() and np.isposinf(c[3]).all() for c in probes)       # probes: one leapfrog, never accepted
    # walker w reads rngs[w] only, L first, then u, once per transition: a replay of its generator gives the recorded arguments
    for w in range(W):
        g = np.random.default_rng([seed, w])
        Ls = []
        for c in moves:
            assert c[2][w] == g.integers(3, 7) and c[3][w] == np.log(g.random())
            Ls.append(int(c[2][w]))
        assert min(Ls) == 3 and max(Ls) == 6                                        # the closed range, both ends
        assert sum(Ls) < res[w][2]["n_grad"] <= sum(Ls) + len(probes)               # (the probes a walker still needed are counted)
    # dual averaging with _walker's constants (gamma 0.05, t0 10, kappa 0.75, mu = log(10 eps_0)) on alpha = min(1, exp(h1 - h0))
    for w in range(W):
        eps0 = moves[0][1][w]
        mu, eps_bar, h_bar, eps = np.log(10.0 * eps0), 1.0, 0.0, eps0
        for m, c in enumerate(moves[:n_adapt], start=1):
            assert c[1][w] == eps
            out = c[4]
            alpha = 0.0 if out["divergent"][w] else min(1.0, float(np.exp(min(0.0, out["h1"][w] - out["h0"][w]))))
            h_bar = (1.0 - 1.0 / (m + 10.0)) * h_bar + (0.65 - alpha) / (m + 10.0)
            eps = float(np.exp(mu - np.sqrt(m) / 0.05 * h_bar))
            x = m ** -0.75
            eps_bar = float(np.exp(x * np.log(eps) + (1.0 - x) * np.log(eps_bar)))
        assert all(c[1][w] == eps_bar for c in moves[n_adapt:]) and res[w][2]["step_size"] == eps_bar
        post = moves[n_adapt:]
        assert res[w][2]["accept_rate"] == np.mean([c[4]["accepted"][w] for c in post]) and res[w][2]["divergences"] == 0
        assert res[w][0].shape == (n_steps, VAR.shape[0]) and np.isfinite(res[w][1]).all()


def test_ensemble_thin_keeps_every_other_draw():
    _, full = _run(30, 20, 2)
    _, thin = _run(15, 20, 2, thin=2)
    for w in range(2):
        assert hc.same(thin[w][0], full[w][0][1::2]) and hc.same(thin[w][1], full[w][1][1::2])


def test_ensemble_early_finisher_does_not_disturb_the_others():
    _, full = _run()
    _, part = _run([30, 4, 30, 30])
    assert part[1][0].shape == (4, VAR.shape[0]) and hc.same(part[1][0], full[1][0][:4])
    for w in (0, 2, 3):
        assert hc.same(part[w][0], full[w][0]) and hc.same(part[w][1], full[w][1]) and part[w][2] == full[w][2]


def test_ensemble_samples_the_gaussian():
    _, res = _run(600, 200, 4)
    x = np.concatenate([r[0] for r in res])
    assert np.all(np.abs(x.mean(axis=0)) < 0.35 * np.sqrt(VAR)) and np.all(np.abs(x.var(axis=0) / VAR - 1.0) < 0.35)
    assert all(0.4 < r[2]["accept_rate"] <= 1.0 for r in res)


def test_argument_errors():
    with pytest.raises(bb.BarBayError, match="one random generator per walker"):
        bb.mcmc.hmc_ensemble(FakeEngine(), _starts(1, 2), 3, 2, rngs=[np.random.default_rng(0)])
    with pytest.raises(bb.BarBayError, match="n_leapfrog"):
        bb.mcmc.hmc_ensemble(FakeEngine(), _starts(1, 1), 3, 2, rngs=[np.random.default_rng(0)], n_leapfrog=(5, 2))
    with pytest.raises(bb.BarBayError, match="sampler must be"):
        bb.mcmc.mcmc_sample(data=hc.lc.load("data001_single"), n_walkers=1, n_steps=2, outputname=None,
                            model=bb.model.fitness_normal, sampler="gibbs")
