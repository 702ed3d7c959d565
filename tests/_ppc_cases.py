"""bb_ppc_bands (posterior predictive bands, barbay.jl_amd/csrc/bb_ppc.h) restated in numpy, draw for draw, and the cases the
emulation and GPU tests share.  The keying is the header's: parameter draw j of the caller's latent i is
pairs(seed, i, j >> 1, 0xFFFFFFE0), predictive draw k' of (row, t) is pairs(seed, row | t << 32, k' >> 1, 0xFFFFFFE1), an even
index taking the cosine branch."""
import numpy as np

from conftest import make_engine
from oracle import fixtures, rng

STREAM_PARAM = 0xFFFFFFE0
STREAM_PRED = 0xFFFFFFE1

CASES = {
    "fitness": ("fitness", dict(B=60, T=5, n_neutral=10)),
    "multienv": ("multienv", dict(B=50, T=6, n_env=3, n_neutral=8)),
    "genotype_regrouped": ("genotype", dict(B=70, T=5, n_geno=7, n_neutral=10)),        # odd T; mutants regrouped inside the library
    "replicate_ragged": ("replicate", dict(B=40, T=[5, 7, 4], n_rep=3, n_neutral=6)),
    "multienv_replicate": ("multienv_replicate", dict(B=40, T=[5, 6], n_rep=2, n_env=2, n_neutral=6)),
}


def spec(name, seed=3):
    kind, kw = CASES[name]
    return fixtures.synthetic(kind, seed=seed, **kw)


def softplus(om):
    return np.maximum(om, 0.0) + np.log1p(np.exp(-np.abs(om)))


def _param(seed, mean, sigma, i, j):
    """Parameter draws of the caller's latents i (scalar) for the samples j (array)."""
    a, b = rng.pairs(seed, np.full(j.shape, i, dtype=np.uint64), j >> np.uint64(1), STREAM_PARAM)
    return mean[i] + sigma[i] * np.where(j & np.uint64(1), b, a)


def quantile7(xs, p):
    """StatsBase.quantile of sorted columns xs[..., K] (Statistics._quantile, alpha = beta = 1)."""
    K = xs.shape[-1]
    aleph = K * p + (1.0 - p)
    j = min(max(int(aleph), 1), K - 1)
    g = min(max(aleph - j, 0.0), 1.0)
    a, b = xs[..., j - 1], xs[..., j]
    return np.where(np.isfinite(a) & np.isfinite(b), a + g * (b - a), (1.0 - g) * a + g * b)


def restate(sp, mu, omega, quantiles, n_samples, n_ppc, seed, rows=None):
    """bands[len(rows), n_steps, n_q, 2] and n_outside[len(rows)] of bb_ppc_bands at the parameters (mu, omega), caller order."""
    mean, sigma = mu, softplus(omega)
    off = sp.offsets()
    R, nb, nn, E = sp.n_rep, sp.n_bc, sp.n_neutral, sp.n_env
    Ts = sp.n_time
    n_rows, n_steps = R * (1 + nb), max(Ts) - 1
    rows = np.arange(n_rows) if rows is None else np.asarray(rows)
    j = np.arange(n_samples, dtype=np.uint64)
    K = n_samples * n_ppc
    kp = np.arange(K, dtype=np.uint64)
    js = (kp // np.uint64(n_ppc)).astype(np.int64)
    tofs = np.concatenate([[0], np.cumsum([t - 1 for t in Ts])])
    hier = sp.kind in ("genotype", "replicate", "multienv_replicate")
    lo_s = off["theta"][0] if hier else off["s_bc"][0]
    lo_ls = off["logsigma_bc"][0]
    qs = np.asarray(quantiles, dtype=np.float64)
    qx = int(np.argmax(qs))
    bands = np.full((len(rows), n_steps, len(qs), 2), np.nan)
    nout = np.zeros(len(rows), dtype=np.int64)
    for x, row in enumerate(rows):
        row = int(row)
        popr = row < R
        r = row if popr else (row - R) // nb
        m = 0 if popr else (row - R) % nb
        for t in range(Ts[r] - 1):
            g = int(tofs[r]) + t
            sbar = _param(seed, mean, sigma, off["s_pop"][0] + g, j)
            sdbar = np.exp(_param(seed, mean, sigma, off["logsigma_pop"][0] + g, j))
            if popr:
                mu_j, sd_j = -sbar, sdbar
            else:
                if sp.kind in ("multienv", "multienv_replicate"):
                    e = int(sp.env_idx[t + 1]) if sp.kind == "multienv" else int(sp.env_idx[r][t + 1])
                else:
                    e = 0
                Ek = E if sp.kind in ("multienv", "multienv_replicate") else 1
                if sp.kind in ("fitness", "multienv"):
                    s = _param(seed, mean, sigma, lo_s + e + Ek * m, j)
                    ls = _param(seed, mean, sigma, lo_ls + e + Ek * m, j)
                else:
                    th = int(sp.geno_idx[m]) if sp.kind == "genotype" else e + Ek * m
                    u = m if sp.kind == "genotype" else e + Ek * m + Ek * nb * r
                    s = (_param(seed, mean, sigma, lo_s + th, j)
                         + np.exp(_param(seed, mean, sigma, off["logtau"][0] + u, j)) * _param(seed, mean, sigma, off["theta_tilde"][0] + u, j))
                    ls = _param(seed, mean, sigma, lo_ls + u, j)
                mu_j, sd_j = s - sbar, np.exp(ls)
            a, b = rng.pairs(seed, np.full(K, row | (t << 32), dtype=np.uint64), kp >> np.uint64(1), STREAM_PRED)
            col = np.sort(mu_j[js] + sd_j[js] * np.where(kp & np.uint64(1), b, a))
            for i, q in enumerate(qs):
                bands[x, t, i, 0] = quantile7(col, (1.0 - q) / 2.0)
                bands[x, t, i, 1] = quantile7(col, 1.0 - (1.0 - q) / 2.0)
        # observed ratios outside the widest band
        c = sp.counts[r].astype(np.float64)
        n = c.sum(axis=1)
        bcs = np.arange(nn) if popr else [nn + m]
        for bc in bcs:
            for t in range(Ts[r] - 1):
                if c[t, bc] > 0 and c[t + 1, bc] > 0:
                    v = np.log(c[t + 1, bc] / n[t + 1]) - np.log(c[t, bc] / n[t])
                    nout[x] += v < bands[x, t, qx, 0] or v > bands[x, t, qx, 1]
    return bands, nout


def assert_bands_close(a, b, rtol=1e-12):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(a)
    err = np.abs(a[ok] - b[ok]) / np.maximum(np.abs(b[ok]), 1.0)
    assert err.max() <= rtol, err.max()


def case_ppc(lib, name, Ks=((1000, 1), (111, 7))):
    """Every row of a small handle against the restatement, for K = 1000 and an odd K = 777."""
    sp = spec(name)
    qs = (0.95, 0.675, 0.05)
    with make_engine(sp, lib, seed=4) as e:
        e.run(3)
        mu, om = e.get_params()
        n_rows, n_steps = e.ppc_shape()
        assert (n_rows, n_steps) == (sp.n_rep * (1 + sp.n_bc), max(sp.n_time) - 1)
        for ns, npp in Ks:
            bands, nout = e.ppc_bands(qs, n_samples=ns, n_ppc=npp, seed=11)
            b2, n2 = restate(sp, mu, om, qs, ns, npp, 11)
            assert_bands_close(bands, b2)
            assert np.array_equal(nout, n2)
            ok = ~np.isnan(bands)
            assert np.all(bands[..., 0][ok[..., 0]] <= bands[..., 1][ok[..., 1]])
        # NaN exactly past each replicate's last step
        for r, T in enumerate(sp.n_time):
            rows = [r] + list(sp.n_rep + r * sp.n_bc + np.arange(sp.n_bc))
            assert np.all(np.isnan(bands[rows, T - 1:])) and not np.any(np.isnan(bands[rows, :T - 1]))


def _bits(res):
    """The raw bytes of a call's results: (bands, n_outside) or chain_summary's dict."""
    vals = list(res.values()) if isinstance(res, dict) else list(res)
    return [np.ascontiguousarray(v).tobytes() for v in vals]


def _handle(lib, sp, mu, om, **kw):
    e = make_engine(sp, lib, seed=4, **kw)
    e.set_params(mu, om)
    return e


def case_buffer_reuse(lib):
    """The calls' device buffers across calls and sizes on ONE handle: bands, frequency bands and a chain summary in turn, a call
    that regrows the bands' buffer, a small call on the large stale buffer, the first call again.  Every result, n_outside included,
    is byte for byte what the same call gives on a fresh handle."""
    sp = spec("fitness")
    qs = (0.95, 0.675, 0.05)
    with make_engine(sp, lib, seed=4) as e:
        e.run(3)
        mu, om = e.get_params()
    om = np.minimum(om, -2.0)                                  # (a fitted sigma: finite trajectories, as _freq_cases.tame)
    chain = np.random.default_rng(12).standard_normal((2, 5, 6))
    calls = [lambda e: e.ppc_bands(qs, n_samples=111, n_ppc=7, seed=11),
             lambda e: e.freq_bands(qs, mode="trajectory", n_samples=111, n_ppc=7, seed=11),
             lambda e: e.chain_summary(chain),
             lambda e: e.ppc_bands(qs, n_samples=1000, n_ppc=1, seed=11),
             lambda e: e.freq_bands(qs, mode="posterior", n_samples=2, n_ppc=1, seed=11),
             lambda e: e.ppc_bands(qs, n_samples=111, n_ppc=7, seed=11)]
    with _handle(lib, sp, mu, om) as e:
        got = [_bits(f(e)) for f in calls]
    for i, f in enumerate(calls):
        with _handle(lib, sp, mu, om) as e:
            assert got[i] == _bits(f(e)), i
    assert got[0] == got[5]


GROUP_CASES = ("fitness", "genotype_regrouped", "replicate_ragged")


def group_results(lib, name, **kw):
    """bb_ppc_bands, bb_freq_bands in both modes and (hierarchical kinds) bb_hier_fitness of a handle of the case at fixed parameters."""
    sp = spec(name)
    qs = (0.95, 0.675, 0.05)
    g = np.random.default_rng(5)
    mu, om = g.normal(0.0, 1.0, sp.D), g.normal(-3.0, 0.3, sp.D)
    with _handle(lib, sp, mu, om, **kw) as e:
        out = _bits(e.ppc_bands(qs, n_samples=111, n_ppc=7, seed=11))
        out += _bits(e.freq_bands(qs, mode="trajectory", n_samples=111, n_ppc=7, seed=11))
        out += _bits(e.freq_bands(qs, mode="posterior", n_samples=200, n_ppc=1, seed=11))
        if e.hier_units() > 0:
            out += _bits(e.hier_fitness(777, seed=21))
    return out


def case_group_handle(lib, name):
    """A multi-device handle (n_devices = 2, both shards on device 0, as `_cases.case_multi_device_handle`) against a single-device
    handle at the same parameters: the post-fit calls sample on shard 0 from the gathered posterior, byte for byte the same."""
    assert group_results(lib, name, device_ids=[0, 0]) == group_results(lib, name)
