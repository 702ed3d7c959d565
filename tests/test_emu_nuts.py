"""The device-resident NUTS tree (barbay.jl_amd/csrc/bb_nuts.h) in the host emulation of the block programs (tests/_nuts_cases.py), and
the pure-Python part of `mcmc.nuts_device` on a known Gaussian with a numpy stand-in for the session and the tree (no engine)."""
import numpy as np
import pytest

import _nuts_cases as nc
import barbay_jl_amd as bb


@pytest.mark.parametrize("name", nc.NAMES)
def test_tree_against_host(emu_lib, name):
    nc.case_tree_against_host(emu_lib, name)


@pytest.mark.parametrize("name", nc.NAMES)
def test_walkers_are_independent_bitwise(emu_lib, name):
    nc.case_independence(emu_lib, name)


@pytest.mark.parametrize("name", nc.NAMES)
def test_nothing_else_moves(emu_lib, name):
    nc.case_state_untouched(emu_lib, name)


def test_full_width(emu_lib):
    nc.case_full_width(emu_lib)


def test_errors(emu_lib):
    nc.case_errors(emu_lib)


def test_end_to_end_against_stand_in(emu_lib):
    nc.case_end_to_end(emu_lib)


def test_sampler(emu_lib, monkeypatch):
    nc.case_sampler(emu_lib, monkeypatch)


@pytest.mark.parametrize("kind", list(nc.SAMPLER_KINDS))
def test_sampler_on_every_model_kind(emu_lib, kind):
    nc.case_sampler_kind(emu_lib, kind)


def test_leaf_op_lists():
    nc.case_leaf_op_lists()
    for j in range(6):
        for i in range(2 ** j):
            assert bb.mcmc.nuts_leaf_op(i, j) == nc.leaf_op(i, j)


def test_header_binding_and_julia_wrapper_agree():
    import ctypes
    import os
    import re
    from barbay_jl_amd import _capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "barbay_hip.h")).read()
    jl = open(os.path.join(root, "julia", "BarBayHIP.jl")).read()
    for sym in ("bb_nuts_begin", "bb_nuts_start", "bb_nuts_leaf", "bb_nuts_take"):
        assert re.search(r"\bint " + sym + r"\(", hdr) and sym in _capi.EXPORTS and ":" + sym in jl, sym
    for name in ("BB_NUTS_MAX_DEPTH", "BB_NUTS_EDGE_OPP", "BB_NUTS_TAKE_LEAF", "BB_NUTS_TAKE_SUB", "BB_NUTS_TAKE_STATE"):
        v = getattr(_capi, name)
        assert re.search(rf"#define {name}\s+\(?{v}\)?\s", hdr), name
        assert re.search(rf"const {name} = (Int32\()?{v}\)?\s", jl), name
    # the structs, field for field: the header's order and types (LP64)
    assert ctypes.sizeof(_capi.bb_nuts_opts) == 8 and ctypes.sizeof(_capi.bb_nuts_leaf_opts) == 56 and ctypes.sizeof(_capi.bb_nuts_leaf_out) == 32
    for struct, fields in ((_capi.bb_nuts_opts, "max_depth reserved0"), (_capi.bb_nuts_leaf_opts, "dir first last store n_check check reserved0"),
                           (_capi.bb_nuts_leaf_out, "logp_leaf kinetic a b")):
        body = re.search(r"typedef struct " + struct.__name__ + r" \{(.*?)\} " + struct.__name__ + ";", hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = re.findall(r"\*?\b([a-z_0-9]+)\s*[,;]", body)
        assert names == fields.split() == [f[0] for f in struct._fields_], (struct.__name__, names)
        jbody = re.search(r"struct " + struct.__name__ + r"\n(.*?)\nend", jl, re.S).group(1)
        assert [ln.split("::")[0].strip() for ln in jbody.splitlines()] == fields.split(), struct.__name__


# ---- nuts_device's own part, no engine: a numpy stand-in for the session and the tree on the diagonal Gaussian of test_emu_hmc.py ----
VAR = np.array([1.0, 4.0, 0.25] * 3)
OPP, LEAF, SUB, STATE = nc.OPP, nc.LEAF, nc.SUB, nc.STATE


def f(z):
    return -0.5 * float(np.sum(z * z / VAR)), -z / VAR


def momentum(seed, transition, w, minv):
    return np.random.default_rng([seed, transition, w]).standard_normal(minv.shape[0]) / np.sqrt(minv)


def energy(lp, r, minv):
    h = lp - 0.5 * float(np.dot(r, minv * r))
    return h if np.isfinite(h) else -np.inf


class FakeSession:
    def __init__(self, logp):
        self.logp = logp


class FakeEngine:
    """The session's and the tree's calls with the arithmetic of include/barbay_hip.h in numpy; walker w's momenta of a transition come
    from default_rng([seed, transition, w]).  Every nuts_start is recorded with the state it found."""

    def hmc_begin(self, z0, *, seed=0, inv_mass=None):
        self.z = np.array(z0, dtype=np.float64)
        self.minv = np.ones(self.z.shape[1]) if inv_mass is None else np.asarray(inv_mass, dtype=np.float64)
        self.seed, self.starts, self.ended, self.gets = seed, [], 0, 0
        self.lp = np.array([f(z)[0] for z in self.z])
        self.g = np.array([f(z)[1] for z in self.z])
        return FakeSession(self.lp.copy())

    def hmc_step(self, transition, eps, n_leapfrog, log_u):                  # (the probes: one leapfrog, never accepted)
        W = self.z.shape[0]
        eps = np.broadcast_to(np.asarray(eps, dtype=np.float64), (W,))
        assert np.all(np.asarray(n_leapfrog) == 1) and np.all(np.isposinf(log_u)) and transition == 0
        out = {"h0": np.zeros(W), "h1": np.zeros(W)}
        for w in range(W):
            r = momentum(self.seed, transition, w, self.minv)
            out["h0"][w] = energy(self.lp[w], r, self.minv)
            r = r + 0.5 * eps[w] * self.g[w]
            z = self.z[w] + eps[w] * self.minv * r
            lp, g = f(z)
            r = r + 0.5 * eps[w] * g
            out["h1"][w] = lp - 0.5 * float(np.dot(r, self.minv * r))
        return out

    def nuts_begin(self, max_depth):
        self.depth = max_depth

    def nuts_start(self, transition, eps, live=1):
        W = self.z.shape[0]
        self.eps = np.array(np.broadcast_to(eps, (W,)), dtype=np.float64)
        self.live = np.broadcast_to(np.asarray(live), (W,)).astype(bool)
        r0 = [momentum(self.seed, transition, w, self.minv) for w in range(W)]
        self.edge = {v: [[self.z[w].copy(), r0[w].copy(), self.g[w].copy()] for w in range(W)] for v in (-1, 1)}
        self.trav, self.ck = [None] * W, [[None] * self.depth for _ in range(W)]
        self.sub, self.cand, self.lp_leaf = [None] * W, [None] * W, np.zeros(W)
        self.starts.append({"m": transition, "eps": self.eps.copy(), "live": self.live.copy(), "z": self.z.copy(), "lp": self.lp.copy(), "r0": r0})
        return np.array([0.5 * float(np.dot(r0[w], self.minv * r0[w])) if self.live[w] else 0.0 for w in range(W)])

    def nuts_leaf(self, dirs, first, last, store, checks):
        W = self.z.shape[0]
        out = {"logp_leaf": np.zeros(W), "kinetic": np.zeros(W), "a": np.zeros((W, self.depth + 1)), "b": np.zeros((W, self.depth + 1))}
        for w in range(W):
            v = int(dirs[w])
            if v == 0:
                continue
            assert self.live[w] and (first[w] or self.trav[w] is not None)
            z, r, g = self.edge[v][w] if first[w] else self.trav[w]
            e = v * self.eps[w]
            r = r + 0.5 * e * g
            z = z + e * self.minv * r
            lp, g = f(z)
            r = r + 0.5 * e * g
            self.trav[w], self.lp_leaf[w] = [z, r, g], lp
            out["logp_leaf"][w], out["kinetic"][w] = lp, 0.5 * float(np.dot(r, self.minv * r))
            for k, c in enumerate(checks[w]):
                assert c == OPP or (0 <= c < self.depth and c != store[w])
                zs, rs = self.edge[-v][w][:2] if c == OPP else self.ck[w][c]
                out["a"][w][k], out["b"][w][k] = float(np.dot(z - zs, self.minv * rs)), float(np.dot(z - zs, self.minv * r))
            if store[w] >= 0:
                self.ck[w][store[w]] = (z, r)
            if last[w]:
                self.edge[v][w] = [z, r, g]
        return out

    def nuts_take(self, flags):
        for w, fl in enumerate(flags):
            if fl & LEAF:
                self.sub[w] = (self.trav[w][0], self.trav[w][2], self.lp_leaf[w])
            if fl & SUB:
                self.cand[w] = self.sub[w]
            if fl & STATE:
                self.z[w], self.g[w], self.lp[w] = self.cand[w]

    def hmc_get(self, grad=False):
        self.gets += 1
        return self.z.copy(), self.lp.copy()

    def hmc_end(self):
        self.ended += 1


def _starts(seed, W):
    return [np.random.default_rng([seed, 100 + w]).standard_normal(VAR.shape[0]) for w in range(W)]


def _run(n_steps=30, n_adapt=20, W=4, seed=5, **kw):
    e = FakeEngine()
    rngs = [np.random.default_rng([seed, w]) for w in range(W)]
    res = bb.mcmc.nuts_device(e, _starts(seed, W), n_steps, n_adapt, rngs=rngs, minv=VAR, seed=seed, **kw)
    assert e.ended == 1
    return e, res, rngs


def tree(z, r, g, logu, v, j, eps, minv, log):
    """`_build_tree`'s structure restated, without its generator: which leaves are visited, which are valid, where it stops."""
    if j == 0:
        r = r + 0.5 * (v * eps) * g
        z = z + (v * eps) * minv * r
        lp, g = f(z)
        r = r + 0.5 * (v * eps) * g
        h1 = energy(lp, r, minv)
        s = bool(logu < 1000.0 + h1)
        log["leaves"].append(bool(logu <= h1))
        if not s:
            log["stop"] = "divergent"
        return z, r, g, z, r, g, s
    zm, rm, gm, zp, rp, gp, s = tree(z, r, g, logu, v, j - 1, eps, minv, log)
    if s:
        if v < 0:
            zm, rm, gm, _, _, _, s2 = tree(zm, rm, gm, logu, v, j - 1, eps, minv, log)
        else:
            _, _, _, zp, rp, gp, s2 = tree(zp, rp, gp, logu, v, j - 1, eps, minv, log)
        dz = zp - zm
        ok = float(np.dot(dz, minv * rm)) >= 0.0 and float(np.dot(dz, minv * rp)) >= 0.0
        if s2 and not ok:
            log["stop"] = "uturn"
        s = s2 and ok
    return zm, rm, gm, zp, rp, gp, s


def test_replay_against_the_recursion():
    """Every transition of a short run: the recursion, fed the same momenta, logu and directions, visits the same number of leaves to the
    same depth, stops for the same reason and finds the same valid leaves; and a replay of the walker's generator in the documented order
    reproduces logu, every direction and the chosen leaf, and ends in the state the walker's generator is in."""
    n_adapt, n_steps, W, seed, depth = 15, 25, 3, 5, 6
    trace = []
    e, res, rngs = _run(n_steps, n_adapt, W, seed, max_depth=depth, trace=trace)
    assert len(trace) == len(e.starts) == n_adapt + n_steps
    stops = set()
    for w in range(W):
        gen = np.random.default_rng([seed, w])
        chain = []
        for st, tr in zip(e.starts, trace):
            t = tr["walkers"][w]
            z, lp, r0, eps = st["z"][w], st["lp"][w], st["r0"][w], st["eps"][w]
            h0 = energy(lp, r0, VAR)
            logu = h0 + np.log(gen.random())
            assert logu == t["logu"]
            g = f(z)[1]
            zm, rm, gm, zp, rp, gp = z, r0, g, z, r0, g
            n, s, j, leaves, valid, chosen, stop = 1, True, 0, 0, [], None, None
            while s and j < depth:
                v = -1 if gen.random() < 0.5 else 1
                assert j < len(t["dirs"]) and v == t["dirs"][j]
                log = {"leaves": [], "stop": None}
                if v < 0:
                    zm, rm, gm, _, _, _, s1 = tree(zm, rm, gm, logu, v, j, eps, VAR, log)
                else:
                    _, _, _, zp, rp, gp, s1 = tree(zp, rp, gp, logu, v, j, eps, VAR, log)
                leaves += len(log["leaves"])
                c, sub = 0, None
                for i, ok in enumerate(log["leaves"]):                        # the reservoir, in the documented order of draws
                    if ok:
                        c += 1
                        valid.append((j, i))
                        if c == 1 or gen.random() < 1.0 / c:
                            sub = (j, i)
                if s1 and gen.random() < min(1.0, c / n) and c > 0:
                    chosen = sub
                n += c
                dz = zp - zm
                whole = float(np.dot(dz, VAR * rm)) >= 0.0 and float(np.dot(dz, VAR * rp)) >= 0.0
                stop = log["stop"] or (None if whole else "uturn")
                s = s1 and whole
                j += 1
            stop = stop or "depth"
            stops.add(stop)
            assert (j, leaves, stop, valid, chosen) == (t["depth"], t["leaves"], t["stop"], t["valid"], t["chosen"]), (w, st["m"])
            assert len(t["dirs"]) == j and t["divergent"] == (stop == "divergent")
            if st["m"] > n_adapt:
                chain.append(chosen)
        assert gen.bit_generator.state == rngs[w].bit_generator.state
        assert res[w][2]["mean_tree_depth"] == np.mean([tr["walkers"][w]["depth"] for tr in trace[n_adapt:]])
        assert res[w][0].shape == (n_steps, VAR.shape[0]) and np.isfinite(res[w][1]).all()
        assert any(c is not None for c in chain)
    assert "uturn" in stops


def _forced(eps):
    class Forced(FakeEngine):                                                 # the step size of every transition, whatever the probes found
        def nuts_start(self, transition, e, live=1):
            return super().nuts_start(transition, np.full(len(self.z), eps), live)
    return Forced()


def test_divergent_leaf_and_depth_limit_stop_the_tree():
    kw = dict(rngs=[np.random.default_rng([5, w]) for w in range(2)], minv=VAR, seed=5)
    trace = []
    res = bb.mcmc.nuts_device(_forced(1e-3), _starts(5, 2), 4, 0, max_depth=2, trace=trace, **kw)      # too short a step to turn: the depth limit
    assert all(t["walkers"][w]["stop"] == "depth" and t["walkers"][w]["depth"] == 2 and t["walkers"][w]["leaves"] == 3
               for t in trace for w in range(2))
    assert [r[2]["mean_tree_depth"] for r in res] == [2.0, 2.0] and [r[2]["divergences"] for r in res] == [0, 0]
    trace = []
    kw["rngs"] = [np.random.default_rng([5, w]) for w in range(2)]
    res = bb.mcmc.nuts_device(_forced(1e3), _starts(5, 2), 4, 0, trace=trace, **kw)                     # a step size the Gaussian diverges at
    assert all(t["walkers"][w]["stop"] == "divergent" and t["walkers"][w]["leaves"] == 1 and t["walkers"][w]["chosen"] is None
               for t in trace for w in range(2))
    assert [r[2]["divergences"] for r in res] == [4, 4] and all(nc.same(r[0], np.repeat(z[None], 4, axis=0)) for r, z in zip(res, _starts(5, 2)))


def test_early_finisher_does_not_disturb_the_others():
    _, full, _ = _run()
    _, part, _ = _run([30, 4, 30, 30])
    assert part[1][0].shape == (4, VAR.shape[0]) and nc.same(part[1][0], full[1][0][:4])
    for w in (0, 2, 3):
        assert nc.same(part[w][0], full[w][0]) and nc.same(part[w][1], full[w][1]) and part[w][2] == full[w][2]


def test_thin_keeps_every_other_draw():
    _, full, _ = _run(30, 20, 2)
    _, thin, _ = _run(15, 20, 2, thin=2)
    for w in range(2):
        assert nc.same(thin[w][0], full[w][0][1::2]) and nc.same(thin[w][1], full[w][1][1::2])


def test_samples_the_gaussian():
    _, res, _ = _run(600, 200, 4)
    x = np.concatenate([r[0] for r in res])
    print("mean / sd", np.abs(x.mean(axis=0)) / np.sqrt(VAR), "var ratio", x.var(axis=0) / VAR, [r[2] for r in res])
    assert np.all(np.abs(x.mean(axis=0)) < 0.35 * np.sqrt(VAR)) and np.all(np.abs(x.var(axis=0) / VAR - 1.0) < 0.35)
    assert all(0.4 < r[2]["accept_rate"] <= 1.0 and r[2]["divergences"] == 0 and 1.0 <= r[2]["mean_tree_depth"] <= 10.0 for r in res)


def test_keep_chain_false_downloads_nothing():
    class Acc(FakeEngine):
        def hmc_accum_begin(self, S):
            self.rows = []

        def hmc_accum_add(self, seg):
            self.rows += [self.z[w].copy() for w in range(len(self.z)) if np.broadcast_to(seg, (len(self.z),))[w] >= 0]

        def hmc_accum_reset(self):
            self.rows = []

        def hmc_accum_stats(self):
            return {"mean": np.mean(self.rows, axis=0), "n_total": len(self.rows)}
    e = Acc()
    res = bb.mcmc.nuts_device(e, _starts(5, 2), 8, 4, rngs=[np.random.default_rng([5, w]) for w in range(2)], minv=VAR, seed=5, segments=2,
                              keep_chain=False)
    assert e.gets == 0 and res[0][0].shape == (0, VAR.shape[0]) and res[0][2]["stream"]["n_total"] == 16


def test_adapt_metric_runs_the_windows():
    """`adapt_metric=True` from a unit metric on the Gaussian: Stan's windows of a 200-transition warm-up, the pooled variance of each
    regularised into the metric, the dual averaging restarted behind it; the chain still samples the Gaussian."""
    class Acc(FakeEngine):
        def hmc_accum_begin(self, S):
            self.rows, self.metrics, self.resets = [], [], 0

        def hmc_accum_add(self, seg):
            self.rows += [self.z[w].copy() for w in range(len(self.z)) if np.broadcast_to(seg, (len(self.z),))[w] >= 0]

        def hmc_accum_reset(self):
            self.rows, self.resets = [], self.resets + 1

        def hmc_accum_stats(self):
            x = np.array(self.rows)
            return {"mean": x.mean(axis=0), "sd": x.std(axis=0, ddof=1), "n_total": len(x)}

        def hmc_set_metric(self, inv_mass):
            self.metrics.append((len(self.starts), np.array(inv_mass)))
            self.minv = np.array(inv_mass, dtype=np.float64)
    e, W, seed = Acc(), 4, 5
    res = bb.mcmc.nuts_device(e, _starts(seed, W), 600, 200, rngs=[np.random.default_rng([seed, w]) for w in range(W)], seed=seed, adapt_metric=True)
    info = res[0][2]
    assert info["metric_windows"] == [(75, 100), (100, 150)] == bb.mcmc._adapt_windows(200)
    assert [m for m, _ in e.metrics] == [100, 150] and e.resets == 2 and nc.same(info["inv_mass"], e.metrics[-1][1])
    ratio = info["inv_mass"] / VAR
    print("inv_mass / VAR", ratio, [r[2]["step_size"] for r in res], [r[2]["accept_rate"] for r in res])
    # the second window holds K = 4 x 50 autocorrelated states: the variance of a latent is known to a factor of about 2
    assert np.all(ratio > 0.4) and np.all(ratio < 2.5)
    # the dual averaging restarts behind a window (mu = log(10 eps), h_bar = 0, counter 1): its first update gives
    # eps' = 10 eps exp(-20 (0.65 - alpha) / 11) with alpha in [0, 1], 3.07 .. 18.9 times eps; an update that continued the old averaging
    # could raise eps by exp(0.35 * 20 sqrt(m) / (m + 10)) at the most, 1.9 at m = 100
    for end in (100, 150):
        jump = e.starts[end + 1]["eps"] / e.starts[end]["eps"]               # (starts[k]: transition k + 1)
        assert np.all(jump > 3.0) and np.all(jump < 19.0), (end, jump)
    x = np.concatenate([r[0] for r in res])
    assert np.all(np.abs(x.mean(axis=0)) < 0.35 * np.sqrt(VAR)) and np.all(np.abs(x.var(axis=0) / VAR - 1.0) < 0.35)
    assert all(0.4 < r[2]["accept_rate"] <= 1.0 and r[2]["divergences"] == 0 for r in res)


def test_argument_errors():
    one = [np.random.default_rng(0)]
    with pytest.raises(bb.BarBayError, match="one random generator per walker"):
        bb.mcmc.nuts_device(FakeEngine(), _starts(1, 2), 3, 2, rngs=one)
    for bad in (0, 11):
        with pytest.raises(bb.BarBayError, match="max_depth"):
            bb.mcmc.nuts_device(FakeEngine(), _starts(1, 1), 3, 2, rngs=one, max_depth=bad)
    with pytest.raises(bb.BarBayError, match="thin"):
        bb.mcmc.nuts_device(FakeEngine(), _starts(1, 1), 3, 2, rngs=one, thin=0)
    with pytest.raises(bb.BarBayError, match="walkers in one session"):
        bb.mcmc.nuts_device(FakeEngine(), _starts(1, 65), 3, 2, rngs=one * 65)
    with pytest.raises(bb.BarBayError, match="keep_chain=False needs segments"):
        bb.mcmc.nuts_device(FakeEngine(), _starts(1, 1), 3, 2, rngs=one, keep_chain=False)
    with pytest.raises(bb.BarBayError, match="segments"):
        bb.mcmc.nuts_device(FakeEngine(), _starts(1, 1), 3, 2, rngs=one, segments=2)
    with pytest.raises(bb.BarBayError, match="adapt_metric"):
        bb.mcmc.nuts_device(FakeEngine(), _starts(1, 2), 3, [2, 3], rngs=one * 2, adapt_metric=True)
    # mcmc_sample refuses before anything is sampled (no engine is created: the data is not even looked at)
    kw = dict(data=None, n_walkers=1, n_steps=2, outputname=None, model=bb.model.fitness_normal)
    with pytest.raises(bb.BarBayError, match="sampler must be 'nuts'"):
        bb.mcmc.mcmc_sample(ensemble="device", sampler="hmc", **kw)
    with pytest.raises(bb.BarBayError, match="ensemble must be"):
        bb.mcmc.mcmc_sample(ensemble="resident", **kw)
    with pytest.raises(bb.BarBayError, match="nuts_kwargs"):
        bb.mcmc.mcmc_sample(ensemble="batched", nuts_kwargs={"max_depth": 3}, **kw)
    with pytest.raises(bb.BarBayError, match="nuts_kwargs"):
        bb.mcmc.mcmc_sample(sampler="hmc", nuts_kwargs={"max_depth": 3}, **kw)
    with pytest.raises(bb.BarBayError, match="one session"):
        bb.mcmc.mcmc_sample(ensemble="device", nuts_kwargs={"segments": 2}, **{**kw, "n_walkers": 65, "n_steps": 8})
    with pytest.raises(bb.BarBayError, match="needs the chain"):
        bb.mcmc.mcmc_sample(ensemble="device", nuts_kwargs={"segments": 2, "keep_chain": False}, summary=True, **{**kw, "n_steps": 8})
