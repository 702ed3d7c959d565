"""`BarBay.mcmc.mcmc_sample` on the device log-density (src/mcmc.jl:86-160).

The reference samples the Turing model with NUTS (`Turing.NUTS(0.65)`, `Turing.sample(model, sampler, ensemble,
n_steps, n_walkers)`) and saves the chain.  Here the sampler is a host-side NUTS (Hoffman & Gelman 2014, algorithm 6:
slice variant, dual-averaging step size, diagonal metric) whose every leapfrog asks the engine for
log p(data, z) and its gradient (`bb_logdensity_grad`: the same fused kernels as the ADVI step, draw pinned to z; with
`ensemble="batched"` the walkers run in lock-step on `bb_logdensity_grad_batch`, one call per round for all of them).
The metric and the start point come from a short ADVI run on the same handle (q's sigma^2 and mean): the
variational fit costs a few thousand device steps and spares NUTS its longest warm-up phase.

The reference's entry point is stale (it indexes the `data_to_arrays` result as a Dict and passes `rm_T0` / `verbose`
kwargs that function no longer has, src/mcmc.jl:120-129, 143-146); the argument list is kept, `rm_T0` is applied here.
Output: `<outputname>.npz` with `ids`, `var_names`, `chain` (n_walkers x n_steps x D), `logp` (the reference
writes `ids` and an MCMCChains object to `<outputname>.jld2`).  What MCMCChains' `summarystats` / `quantile` report for that
object -- mean, std, MCSE, ESS, R-hat and quantiles of every parameter -- comes from the device (`bb_chain_summary`):
`mcmc_sample(..., summary=True)` adds it to the output, `summarize` turns an output into the table.
"""
from __future__ import annotations

import logging
import os
from typing import Callable, Dict, Optional, Sequence

import numpy as np

from . import utils
from . import vi as _vi
from ._capi import (BB_CHAIN_MAX_K, BB_HMC_MAX_SEGMENTS, BB_HMC_MAX_WALKERS, BB_LOGP_MAX_BATCH, BB_NUTS_EDGE_OPP, BB_NUTS_MAX_DEPTH,
                    BB_NUTS_TAKE_LEAF, BB_NUTS_TAKE_STATE, BB_NUTS_TAKE_SUB, Engine)
from .model import BarBayError, BayesModel

log = logging.getLogger("barbay")


# The sampler asks for the log-density at one point at a time.  Its body is written as generators that YIELD the point and are
# resumed with (logp, grad): `nuts` answers each request at once, `nuts_ensemble` collects the requests of all its walkers and
# answers them with one batched evaluation per round.  Both run the same arithmetic in the same order.
def _leapfrog(z, r, g, eps, minv):
    r = r + 0.5 * eps * g
    z = z + eps * minv * r
    lp, g = yield z
    r = r + 0.5 * eps * g
    return z, r, lp, g


def _energy(lp, r, minv):
    h = lp - 0.5 * float(np.dot(r, minv * r))
    return h if np.isfinite(h) else -np.inf


def _find_step(z, lp, g, minv, rng):
    """Heuristic initial step size (Hoffman & Gelman, algorithm 4)."""
    eps = 1.0
    r = rng.standard_normal(z.shape[0]) / np.sqrt(minv)
    h0 = _energy(lp, r, minv)
    _, r1, lp1, _ = yield from _leapfrog(z, r, g, eps, minv)
    a = 1.0 if _energy(lp1, r1, minv) - h0 > np.log(0.5) else -1.0
    for _ in range(60):
        _, r1, lp1, _ = yield from _leapfrog(z, r, g, eps, minv)
        if a * (_energy(lp1, r1, minv) - h0) <= -a * np.log(2.0):
            break
        eps *= 2.0 ** a
    return eps


def _build_tree(z, r, g, logu, v, j, eps, h0, minv, rng):
    if j == 0:
        z1, r1, lp1, g1 = yield from _leapfrog(z, r, g, v * eps, minv)
        h1 = _energy(lp1, r1, minv)
        n1 = int(logu <= h1)
        s1 = logu < 1000.0 + h1
        alpha = min(1.0, float(np.exp(min(0.0, h1 - h0)))) if np.isfinite(h1) else 0.0
        return z1, r1, g1, z1, r1, g1, z1, lp1, g1, n1, s1, alpha, 1
    zm, rm, gm, zp, rp, gp, z1, lp1, g1, n1, s1, a1, na1 = yield from _build_tree(z, r, g, logu, v, j - 1, eps, h0, minv, rng)
    if s1:
        if v < 0:
            zm, rm, gm, _, _, _, z2, lp2, g2, n2, s2, a2, na2 = yield from _build_tree(zm, rm, gm, logu, v, j - 1, eps, h0, minv, rng)
        else:
            _, _, _, zp, rp, gp, z2, lp2, g2, n2, s2, a2, na2 = yield from _build_tree(zp, rp, gp, logu, v, j - 1, eps, h0, minv, rng)
        if n2 > 0 and rng.random() < n2 / max(n1 + n2, 1):
            z1, lp1, g1 = z2, lp2, g2
        dz = zp - zm
        s1 = s2 and float(np.dot(dz, minv * rm)) >= 0.0 and float(np.dot(dz, minv * rp)) >= 0.0
        n1 += n2
        a1 += a2
        na1 += na2
    return zm, rm, gm, zp, rp, gp, z1, lp1, g1, n1, s1, a1, na1


def _walker(z0, n_steps, n_adapt, target_accept, minv, rng, max_depth):
    """One NUTS chain as a generator: yields the point it needs the log-density at, is resumed with (logp, grad), and returns
    what `nuts` returns."""
    rng = rng or np.random.default_rng()
    z = np.array(z0, dtype=np.float64)
    D = z.shape[0]
    minv = np.ones(D) if minv is None else np.asarray(minv, dtype=np.float64)
    lp, g = yield z
    if not np.isfinite(lp):
        raise BarBayError("log density is not finite at the initial point")
    eps = yield from _find_step(z, lp, g, minv, rng)
    mu, eps_bar, h_bar, gamma, t0, kappa = np.log(10.0 * eps), 1.0, 0.0, 0.05, 10.0, 0.75
    chain = np.empty((n_steps, D))
    lps = np.empty(n_steps)
    depths, n_grad = [], 0
    for m in range(1, n_adapt + n_steps + 1):
        r0 = rng.standard_normal(D) / np.sqrt(minv)
        h0 = _energy(lp, r0, minv)
        logu = h0 + np.log(rng.random())
        zm = zp = z
        rm = rp = r0
        gm = gp = g
        j, n, s = 0, 1, True
        alpha = n_alpha = 0
        while s and j < max_depth:
            v = -1 if rng.random() < 0.5 else 1
            if v < 0:
                zm, rm, gm, _, _, _, z1, lp1, g1, n1, s1, alpha, n_alpha = yield from _build_tree(zm, rm, gm, logu, v, j, eps, h0, minv, rng)
            else:
                _, _, _, zp, rp, gp, z1, lp1, g1, n1, s1, alpha, n_alpha = yield from _build_tree(zp, rp, gp, logu, v, j, eps, h0, minv, rng)
            if s1 and rng.random() < min(1.0, n1 / n):
                z, lp, g = z1, lp1, g1
            n += n1
            dz = zp - zm
            s = s1 and float(np.dot(dz, minv * rm)) >= 0.0 and float(np.dot(dz, minv * rp)) >= 0.0
            j += 1
            n_grad += n_alpha
        if m <= n_adapt:
            h_bar = (1.0 - 1.0 / (m + t0)) * h_bar + (target_accept - alpha / max(n_alpha, 1)) / (m + t0)
            eps = float(np.exp(mu - np.sqrt(m) / gamma * h_bar))
            w = m ** -kappa
            eps_bar = float(np.exp(w * np.log(eps) + (1.0 - w) * np.log(eps_bar)))
            if m == n_adapt:
                eps = eps_bar
        else:
            chain[m - n_adapt - 1] = z
            lps[m - n_adapt - 1] = lp
            depths.append(j)
    return chain, lps, {"step_size": eps, "mean_tree_depth": float(np.mean(depths)) if depths else 0.0, "n_grad": n_grad}


def nuts(f: Callable, z0: np.ndarray, n_steps: int, n_adapt: int, *, target_accept: float = 0.65,
         minv: Optional[np.ndarray] = None, rng: Optional[np.random.Generator] = None, max_depth: int = 10):
    """One NUTS chain on `f(z) -> (logp, grad)`.  Returns (chain[n_steps, D], logp[n_steps], info); the n_adapt
    warm-up draws (step-size dual averaging towards `target_accept`) are not part of the returned chain, as with
    `Turing.NUTS` (`discard_adapt = true`)."""
    walker = _walker(z0, n_steps, n_adapt, target_accept, minv, rng, max_depth)
    try:
        z = next(walker)
        while True:
            z = walker.send(f(z))
    except StopIteration as done:
        return done.value


def nuts_ensemble(fbatch: Callable, z0s, n_steps, n_adapt, *, rngs: Sequence[np.random.Generator], target_accept: float = 0.65,
                  minv: Optional[np.ndarray] = None, max_depth: int = 10):
    """len(z0s) NUTS chains stepped in lock-step on `fbatch(Z[W, D]) -> (logp[W], grad[W, D])`: every round collects the point
    each unfinished walker waits for, evaluates them in ONE call and resumes the walkers.  Walkers drop out as they finish, so
    the batch shrinks.  Walker w draws from rngs[w] only and is resumed with row w's result only, so its chain is the one
    `nuts(f, z0s[w], ..., rng=rngs[w])` returns wherever f agrees with fbatch row by row.  `n_steps` / `n_adapt` may be sequences,
    one value per walker.  Returns a list of `nuts` results, one per walker."""
    W = len(z0s)
    if len(rngs) != W:
        raise BarBayError("nuts_ensemble needs one random generator per walker")
    per = lambda v, w: int(v[w]) if np.ndim(v) else int(v)
    walkers = [_walker(z0s[w], per(n_steps, w), per(n_adapt, w), target_accept, minv, rngs[w], max_depth) for w in range(W)]
    results = [None] * W
    pending = {w: next(walkers[w]) for w in range(W)}
    while pending:
        order = sorted(pending)
        lp, g = fbatch(np.stack([pending[w] for w in order]))
        for i, w in enumerate(order):
            try:
                pending[w] = walkers[w].send((float(lp[i]), np.array(g[i], dtype=np.float64)))
            except StopIteration as done:
                results[w] = done.value
                del pending[w]
    return results


def _adapt_windows(n_adapt: int):
    """Stan's metric windows of a warm-up of n_adapt transitions, as (start, end] pairs of transition numbers (1-based: the window holds
    the transitions start < m <= end).  Below 20 transitions none; below 150 one window between floor(0.15 n) and n - floor(0.1 n);
    otherwise an initial buffer of 75, a final buffer of 50, a first window of 25 and each next window twice as long, a window whose
    successor would not fit before the final buffer being extended to it (1000: windows ending at 100, 150, 250, 450, 950)."""
    n = int(n_adapt)
    if n < 20:
        return []
    if n < 150:
        return [(int(0.15 * n), n - int(0.1 * n))]
    start, size, last = 75, 25, n - 50
    out = []
    while start < last:
        end = start + size
        if end + 2 * size > last:
            end = last
        out.append((start, end))
        start, size = end, 2 * size
    return out


def hmc_ensemble(engine, z0s, n_steps, n_adapt, *, rngs: Sequence[np.random.Generator], target_accept: float = 0.65,
                 minv: Optional[np.ndarray] = None, n_leapfrog=(8, 24), thin: int = 1, seed: int = 0, adapt_metric: bool = False,
                 segments: int = 0, keep_chain: bool = True):
    """len(z0s) <= BB_HMC_MAX_WALKERS chains of Hamiltonian Monte Carlo (diagonal metric `minv`, a fixed number of leapfrogs per
    transition) whose position, momentum and gradient stay on the device (`Engine.hmc_begin / hmc_step / hmc_get / hmc_end`,
    csrc/bb_hmc.h): one call makes one transition of every walker, only scalars come back, and positions are downloaded when a draw
    is kept (every `thin`-th transition after the warm-up).  `engine` is an Engine, or anything with those four methods.

    Per transition walker w draws its number of leapfrogs uniformly from the closed range `n_leapfrog` and log(u) from rngs[w] -- and
    reads no other generator; the momenta are the engine's own normals (key `seed`, stream BB_HMC_STREAM0 + w, step = the transition's
    number).  The start step size follows `_find_step`'s doubling rule, run as probes (one leapfrog, never accepted, all on transition
    0); during the `n_adapt` warm-up transitions, which are discarded, the step size is adapted by dual averaging with `_walker`'s constants
    on alpha = min(1, exp(h1 - h0)), 0 for a divergent trajectory.  `n_steps` / `n_adapt` may be sequences, one value per walker: a
    walker that has finished is stepped on as a probe and disturbs no one.  The default range (8, 24) of `n_leapfrog` has been tuned by
    nobody.

    `adapt_metric`: the metric is adapted during the warm-up as Stan does (`n_adapt` must then be one value: the session has one metric).
    Inside each window of `_adapt_windows(n_adapt)` every walker's state is added, after each transition, to the device's running moments
    (`Engine.hmc_accum_add`, segment 0); at a window's end the pooled variance v of its K states (`hmc_accum_stats`' sd squared) becomes
    the metric, regularised as Stan regularises it, inv_mass = v K / (K + 5) + 1e-3 * 5 / (K + 5) (`hmc_set_metric`), the moments are reset
    and every walker's dual averaging restarts at mu = log(10 eps), h_bar = 0, eps_bar = 1, counter 1.  `info` gains `inv_mass` (the final
    metric) and `metric_windows`.
    `segments` = S > 0: after the warm-up the moments are reset and kept draw k of a walker with n kept draws (n >= 2 S) goes to its segment
    floor(S k / n); `info` gains `stream`, what `hmc_accum_stats` returns at the end (pooled mean, sd, split-R-hat for S = 2, and a
    batch-means mcse / ess over the W S segments: include/barbay_hip.h) -- the same dict in every walker's info.
    `keep_chain=False` (needs `segments`): `hmc_get` is never called and the chains come back with 0 rows: nothing of size D crosses the
    host link per draw.  With the three defaults the engine sees the calls it saw without them.

    Returns a list, per walker, of what `nuts` returns: (chain[n_steps, D], logp[n_steps], info), info holding `step_size`, `n_grad`
    (leapfrogs, probes included), `accept_rate` and `divergences` (both over the transitions after the warm-up) and `mean_leapfrog`."""
    W = len(z0s)
    if len(rngs) != W:
        raise BarBayError("hmc_ensemble needs one random generator per walker")
    lo_l, hi_l = (int(n_leapfrog), int(n_leapfrog)) if np.ndim(n_leapfrog) == 0 else (int(n_leapfrog[0]), int(n_leapfrog[1]))
    if not 1 <= lo_l <= hi_l or thin < 1:
        raise BarBayError(f"n_leapfrog must be a range 1 <= lo <= hi and thin >= 1, not {n_leapfrog!r}, {thin!r}")
    per = lambda v, w: int(v[w]) if np.ndim(v) else int(v)
    n_st = np.array([per(n_steps, w) for w in range(W)])
    n_ad = np.array([per(n_adapt, w) for w in range(W)])
    S = int(segments)
    if adapt_metric and not (n_ad == n_ad[0]).all():
        raise BarBayError("adapt_metric needs one n_adapt for all walkers: the session has one metric")
    if not 0 <= S <= BB_HMC_MAX_SEGMENTS or (S > 0 and (n_st < 2 * S).any()):
        raise BarBayError(f"segments must lie in 0 .. {BB_HMC_MAX_SEGMENTS} and every walker keep at least 2 draws per segment, not "
                          f"segments = {segments!r} with n_steps = {n_steps!r}")
    if not keep_chain and S == 0:
        raise BarBayError("keep_chain=False needs segments > 0: without the chain the streamed summary is all that is returned")
    windows = _adapt_windows(n_ad[0]) if adapt_metric else []
    Z0 = np.stack([np.asarray(z, dtype=np.float64) for z in z0s])
    D = Z0.shape[1]
    session = engine.hmc_begin(Z0, seed=seed, inv_mass=minv)
    try:
        if not np.isfinite(session.logp).all():
            raise BarBayError("log density is not finite at the initial point")
        if windows or S > 0:
            engine.hmc_accum_begin(max(S, 1))
        n_grad = np.zeros(W, dtype=np.int64)
        # the start step size: _find_step's rule on probes of one leapfrog, every probe with transition 0's momenta
        eps = np.ones(W)
        dh = lambda r: np.where(np.isfinite(r["h1"]), r["h1"] - r["h0"], -np.inf)
        d = dh(engine.hmc_step(0, eps, 1, np.inf))
        n_grad += 1
        a = np.where(d > np.log(0.5), 1.0, -1.0)
        done = np.zeros(W, dtype=bool)
        for _ in range(60):
            done |= a * d <= -a * np.log(2.0)
            if done.all():
                break
            eps = np.where(done, eps, eps * 2.0 ** a)
            d = np.where(done, d, dh(engine.hmc_step(0, eps, 1, np.inf)))
            n_grad += ~done
        mu, eps_bar, h_bar = np.log(10.0 * eps), np.ones(W), np.zeros(W)
        gamma, t0, kappa = 0.05, 10.0, 0.75
        chains = [np.empty((n_st[w] if keep_chain else 0, D)) for w in range(W)]
        lps = [np.empty(n_st[w] if keep_chain else 0) for w in range(W)]
        acc, div, leaps = np.zeros(W), np.zeros(W, dtype=np.int64), np.zeros(W)
        total = n_ad + n_st * thin
        da0 = 0                                                              # the transition the dual averaging last restarted behind
        metric, metric_windows = None, []
        win_end = {end: start for start, end in windows}
        in_window = lambda m: any(start < m <= end for start, end in windows)
        for m in range(1, int(total.max()) + 1):
            live = m <= total
            L, logu = np.ones(W, dtype=np.int32), np.full(W, np.inf)          # (a finished walker: a probe)
            for w in np.flatnonzero(live):
                L[w] = rngs[w].integers(lo_l, hi_l + 1)
                logu[w] = np.log(rngs[w].random())
            r = engine.hmc_step(m, eps, L, logu)
            n_grad += np.where(live, L, 0)
            alpha = np.where(r["divergent"] != 0, 0.0, np.minimum(1.0, np.exp(np.minimum(0.0, dh(r)))))
            keep = None
            seg = np.full(W, -1, dtype=np.int32)                              # where this transition's states go (segments > 0)
            md = m - da0                                                      # the dual averaging's own counter
            for w in np.flatnonzero(live):
                if m <= n_ad[w]:
                    h_bar[w] = (1.0 - 1.0 / (md + t0)) * h_bar[w] + (target_accept - alpha[w]) / (md + t0)
                    eps[w] = float(np.exp(mu[w] - np.sqrt(md) / gamma * h_bar[w]))
                    x = md ** -kappa
                    eps_bar[w] = float(np.exp(x * np.log(eps[w]) + (1.0 - x) * np.log(eps_bar[w])))
                    if m == n_ad[w]:
                        eps[w] = eps_bar[w]
                    continue
                acc[w] += r["accepted"][w]
                div[w] += r["divergent"][w]
                leaps[w] += L[w]
                if (m - n_ad[w]) % thin == 0:
                    k = (m - n_ad[w]) // thin - 1
                    if S > 0:
                        seg[w] = S * k // n_st[w]
                    if not keep_chain:
                        continue
                    if keep is None:
                        keep = engine.hmc_get()                               # (one download for all the walkers that keep this draw)
                    chains[w][k] = keep[0][w]
                    lps[w][k] = keep[1][w]
            if (seg >= 0).any():
                engine.hmc_accum_add(seg)
            if windows and in_window(m):
                engine.hmc_accum_add(0)
                if m in win_end:                                              # the window's variance becomes the metric
                    st = engine.hmc_accum_stats()
                    K = float(st["n_total"])
                    metric = st["sd"] ** 2 * (K / (K + 5.0)) + 1e-3 * (5.0 / (K + 5.0))
                    engine.hmc_set_metric(metric)
                    engine.hmc_accum_reset()
                    metric_windows.append((win_end[m], m))
                    if m < n_ad[0]:                                           # (a walker whose warm-up ends here keeps its eps_bar)
                        mu, eps_bar, h_bar, da0 = np.log(10.0 * eps), np.ones(W), np.zeros(W), m
            if windows and S > 0 and m == n_ad[0]:
                engine.hmc_accum_reset()
        stream = engine.hmc_accum_stats() if S > 0 else None
    finally:
        engine.hmc_end()
    post = np.maximum(n_st * thin, 1)
    extra = {}
    if adapt_metric:
        extra.update(inv_mass=np.array(metric if metric is not None else (np.ones(D) if minv is None else minv), dtype=np.float64),
                     metric_windows=metric_windows)
    if S > 0:
        extra.update(stream=stream)
    return [(chains[w], lps[w], {"step_size": float(eps[w]), "n_grad": int(n_grad[w]), "accept_rate": float(acc[w] / post[w]),
                                 "divergences": int(div[w]), "mean_leapfrog": float(leaps[w] / post[w]), **extra}) for w in range(W)]


def nuts_leaf_op(i: int, j: int):
    """(store, checks) of leaf i = 0 .. 2^j - 1 of a doubling of 2^j leaves, the ops `Engine.nuts_leaf` takes: with
    idx_max = popcount(i >> 1) and k = the number of trailing one-bits of i, an even leaf is stored in checkpoint slot idx_max and an odd
    leaf is checked against the slots idx_max down to idx_max - k + 1 -- the first leaves of the sub-subtrees of 2, 4, ..., 2^k leaves
    that end at i, innermost first: `_build_tree`'s U-turn tests -- and the last leaf, behind them, against the opposite edge
    (`_walker`'s test of the whole trajectory)."""
    idx_max = bin(i >> 1).count("1")
    if i & 1:
        k = (~i & (i + 1)).bit_length() - 1
        store, checks = -1, list(range(idx_max, idx_max - k, -1))
    else:
        store, checks = idx_max, []
    if i == (1 << j) - 1:
        checks.append(BB_NUTS_EDGE_OPP)
    return store, checks


def nuts_device(engine, z0s, n_steps, n_adapt, *, rngs: Sequence[np.random.Generator], target_accept: float = 0.65,
                minv: Optional[np.ndarray] = None, max_depth: int = 10, thin: int = 1, seed: int = 0, adapt_metric: bool = False,
                segments: int = 0, keep_chain: bool = True, trace: Optional[list] = None):
    """len(z0s) <= BB_HMC_MAX_WALKERS NUTS chains (Hoffman & Gelman's algorithm 6 as `_walker` states it: slice variable, position
    U-turn criterion, dual averaging with the same constants) whose every vector stays on the device: the session's state
    (`Engine.hmc_begin`), both ends of the trajectory, the U-turn checkpoints and the candidates (`Engine.nuts_begin / nuts_start /
    nuts_leaf / nuts_take`, csrc/bb_nuts.h).  The tree's decisions are made here, per walker, on the scalars a leaf brings back.  `engine`
    is an Engine, or anything with those methods and `hmc_step / hmc_get / hmc_end`.

    The walkers run in lock-step: every round issues one leaf for every walker whose tree still grows; a walker whose tree has ended idles
    until the deepest is done.  Against `_build_tree` two things differ.  (1) A doubling's 2^j leaves are built iteratively, leaf by leaf
    from the edge of side v; `nuts_leaf_op` says which checkpoint a leaf is stored in and which it is tested against, a test passing when
    v a >= 0 and v b >= 0; a leaf is divergent when not logu < 1000 + h1 (a non-finite h1 counting as -inf); the first failure of either
    kind ends the doubling and the transition, as the recursion does: the same leaves are visited and the same leaf stops the tree.
    (2) The candidate of a doubling is chosen by reservoir: the c-th valid leaf (logu <= h1) is taken at once for c = 1 and otherwise
    with probability 1 / c -- uniform over the valid leaves, as the recursion's n2 / (n1 + n2) merges are; a doubling that ends with
    s true hands its candidate to the transition with probability min(1, n1 / n); the last leaf's test against the opposite edge
    (`_walker`'s test of the whole trajectory) ends the transition without taking that away, as in `_walker`.
    Walker w reads rngs[w] only, per transition in this order: log(random()) for logu; per doubling random() < 0.5 for v = -1; per valid
    leaf with c >= 2 one random(), drawn before the leaf's U-turn tests are looked at; per completed doubling with s true one random().
    A walker that has finished or idles draws nothing.  The momenta are the engine's normals (key `seed`, stream BB_HMC_STREAM0 + w,
    step = the transition's number), those of `hmc_step`.  The start step size comes from `hmc_ensemble`'s probes (`hmc_step`, one
    leapfrog, never accepted, transition 0); alpha / n_alpha of the dual averaging is that of the last doubling's leaves.

    `thin`, `adapt_metric`, `segments`, `keep_chain` and a per-walker `n_steps` / `n_adapt`: as in `hmc_ensemble`.  `trace`: a list that
    receives one dict per transition, {"m", "walkers": {w: {"depth", "leaves", "stop", "valid", "chosen", "divergent", "logu", "dirs"}}}
    -- stop is "uturn", "divergent" or "depth"; valid and chosen hold (doubling, leaf) pairs, chosen the leaf whose position the
    transition ended on (None: it stayed).

    Returns a list, per walker, of (chain[n_steps, D], logp[n_steps], info), info holding `step_size`, `mean_tree_depth`, `n_grad`
    (leaves, probes included), `accept_rate` (the mean alpha / n_alpha after the warm-up), `divergences` (transitions after the warm-up
    with a divergent leaf) and `hmc_ensemble`'s `inv_mass` / `metric_windows` / `stream` extras."""
    W = len(z0s)
    if len(rngs) != W:
        raise BarBayError("nuts_device needs one random generator per walker")
    if not 1 <= W <= BB_HMC_MAX_WALKERS:
        raise BarBayError(f"nuts_device runs 1 .. {BB_HMC_MAX_WALKERS} walkers in one session, not {W}")
    if not 1 <= int(max_depth) <= BB_NUTS_MAX_DEPTH or thin < 1:
        raise BarBayError(f"max_depth must lie in 1 .. {BB_NUTS_MAX_DEPTH} and thin be >= 1, not {max_depth!r}, {thin!r}")
    max_depth = int(max_depth)
    per = lambda v, w: int(v[w]) if np.ndim(v) else int(v)
    n_st = np.array([per(n_steps, w) for w in range(W)])
    n_ad = np.array([per(n_adapt, w) for w in range(W)])
    S = int(segments)
    if adapt_metric and not (n_ad == n_ad[0]).all():
        raise BarBayError("adapt_metric needs one n_adapt for all walkers: the session has one metric")
    if not 0 <= S <= BB_HMC_MAX_SEGMENTS or (S > 0 and (n_st < 2 * S).any()):
        raise BarBayError(f"segments must lie in 0 .. {BB_HMC_MAX_SEGMENTS} and every walker keep at least 2 draws per segment, not "
                          f"segments = {segments!r} with n_steps = {n_steps!r}")
    if not keep_chain and S == 0:
        raise BarBayError("keep_chain=False needs segments > 0: without the chain the streamed summary is all that is returned")
    windows = _adapt_windows(n_ad[0]) if adapt_metric else []
    Z0 = np.stack([np.asarray(z, dtype=np.float64) for z in z0s])
    D = Z0.shape[1]
    session = engine.hmc_begin(Z0, seed=seed, inv_mass=minv)
    try:
        lp = np.array(session.logp, dtype=np.float64)
        if not np.isfinite(lp).all():
            raise BarBayError("log density is not finite at the initial point")
        engine.nuts_begin(max_depth)
        if windows or S > 0:
            engine.hmc_accum_begin(max(S, 1))
        n_grad = np.zeros(W, dtype=np.int64)
        # the start step size: _find_step's rule on probes of one leapfrog, every probe with transition 0's momenta (as hmc_ensemble)
        eps = np.ones(W)
        dh = lambda r: np.where(np.isfinite(r["h1"]), r["h1"] - r["h0"], -np.inf)
        d = dh(engine.hmc_step(0, eps, 1, np.inf))
        n_grad += 1
        a = np.where(d > np.log(0.5), 1.0, -1.0)
        done = np.zeros(W, dtype=bool)
        for _ in range(60):
            done |= a * d <= -a * np.log(2.0)
            if done.all():
                break
            eps = np.where(done, eps, eps * 2.0 ** a)
            d = np.where(done, d, dh(engine.hmc_step(0, eps, 1, np.inf)))
            n_grad += ~done
        mu, eps_bar, h_bar = np.log(10.0 * eps), np.ones(W), np.zeros(W)
        gamma, t0, kappa = 0.05, 10.0, 0.75
        chains = [np.empty((n_st[w] if keep_chain else 0, D)) for w in range(W)]
        lps = [np.empty(n_st[w] if keep_chain else 0) for w in range(W)]
        acc, div, depths = np.zeros(W), np.zeros(W, dtype=np.int64), np.zeros(W)
        total = n_ad + n_st * thin
        da0 = 0
        metric, metric_windows = None, []
        win_end = {end: start for start, end in windows}
        in_window = lambda m: any(start < m <= end for start, end in windows)
        for m in range(1, int(total.max()) + 1):
            live = m <= total
            k0 = engine.nuts_start(m, eps, live.astype(np.int32))
            # per walker: the transition's and the doubling's scalars
            h0, logu = lp - k0, np.zeros(W)
            build = live.copy()                                               # the tree still grows
            j, n, v, i = np.zeros(W, dtype=int), np.ones(W, dtype=int), np.zeros(W, dtype=int), np.zeros(W, dtype=int)
            c, alpha, n_alpha = np.zeros(W, dtype=int), np.zeros(W), np.zeros(W, dtype=int)
            lp_leaf, lp_sub, lp_cand = np.zeros(W), np.zeros(W), np.zeros(W)
            has_cand, diverged = np.zeros(W, dtype=bool), np.zeros(W, dtype=bool)
            rec = {w: {"depth": 0, "leaves": 0, "stop": None, "valid": [], "chosen": None, "divergent": False, "dirs": [], "_sub": None}
                   for w in np.flatnonzero(live)}
            for w in np.flatnonzero(live):
                logu[w] = h0[w] + np.log(rngs[w].random())
                rec[w]["logu"] = float(logu[w])
            while build.any():
                dirs, first, last, store = (np.zeros(W, dtype=np.int32) for _ in range(4))
                checks = [[] for _ in range(W)]
                store[:] = -1
                for w in np.flatnonzero(build):
                    if i[w] == 0:                                             # a doubling begins
                        v[w] = -1 if rngs[w].random() < 0.5 else 1
                        c[w], alpha[w], n_alpha[w] = 0, 0.0, 0
                        rec[w]["dirs"].append(int(v[w]))
                    dirs[w], first[w], last[w] = v[w], i[w] == 0, i[w] == (1 << j[w]) - 1
                    store[w], checks[w] = nuts_leaf_op(int(i[w]), int(j[w]))
                r = engine.nuts_leaf(dirs, first, last, store, checks)
                flags = np.zeros(W, dtype=np.int32)
                for w in np.flatnonzero(build):
                    h1 = r["logp_leaf"][w] - r["kinetic"][w]
                    fin = bool(np.isfinite(h1))
                    if not fin:
                        h1 = -np.inf
                    lp_leaf[w] = r["logp_leaf"][w]
                    rec[w]["leaves"] += 1
                    alpha[w] += min(1.0, float(np.exp(min(0.0, h1 - h0[w])))) if fin else 0.0
                    n_alpha[w] += 1
                    s = bool(logu[w] < 1000.0 + h1)
                    if not s:
                        diverged[w] = True
                        rec[w]["divergent"], rec[w]["stop"] = True, "divergent"
                    if logu[w] <= h1:                                         # a valid leaf: the reservoir
                        c[w] += 1
                        rec[w]["valid"].append((int(j[w]), int(i[w])))
                        if c[w] == 1 or rngs[w].random() < 1.0 / c[w]:
                            flags[w] |= BB_NUTS_TAKE_LEAF
                            lp_sub[w] = lp_leaf[w]
                            rec[w]["_sub"] = (int(j[w]), int(i[w]))
                    whole = True                                              # the test of the whole trajectory (the last leaf's)
                    if s:
                        for q, slot in enumerate(checks[w]):
                            if not (v[w] * r["a"][w][q] >= 0.0 and v[w] * r["b"][w][q] >= 0.0):
                                if slot == BB_NUTS_EDGE_OPP:
                                    whole = False
                                else:
                                    s = False
                                rec[w]["stop"] = "uturn"
                                break
                    ends = not s or last[w]
                    if s and last[w]:                                         # the doubling is complete: _walker's s1
                        if rngs[w].random() < min(1.0, c[w] / n[w]):
                            if c[w] > 0:
                                flags[w] |= BB_NUTS_TAKE_SUB
                                lp_cand[w], has_cand[w] = lp_sub[w], True
                                rec[w]["chosen"] = rec[w]["_sub"]
                        n[w] += c[w]
                    if ends:
                        n_grad[w] += n_alpha[w]
                        j[w] += 1
                        i[w] = 0
                        if not (s and whole) or j[w] >= max_depth:            # the transition is complete
                            build[w] = False
                            rec[w]["depth"] = int(j[w])
                            if rec[w]["stop"] is None:
                                rec[w]["stop"] = "depth"
                            if has_cand[w]:
                                flags[w] |= BB_NUTS_TAKE_STATE
                                lp[w] = lp_cand[w]
                    else:
                        i[w] += 1
                if flags.any():
                    engine.nuts_take(flags)
            if trace is not None:
                for x in rec.values():
                    del x["_sub"]
                trace.append({"m": m, "walkers": {int(w): x for w, x in rec.items()}})
            keep = None
            seg = np.full(W, -1, dtype=np.int32)
            md = m - da0
            for w in np.flatnonzero(live):
                if m <= n_ad[w]:
                    h_bar[w] = (1.0 - 1.0 / (md + t0)) * h_bar[w] + (target_accept - alpha[w] / max(n_alpha[w], 1)) / (md + t0)
                    eps[w] = float(np.exp(mu[w] - np.sqrt(md) / gamma * h_bar[w]))
                    x = md ** -kappa
                    eps_bar[w] = float(np.exp(x * np.log(eps[w]) + (1.0 - x) * np.log(eps_bar[w])))
                    if m == n_ad[w]:
                        eps[w] = eps_bar[w]
                    continue
                acc[w] += alpha[w] / max(n_alpha[w], 1)
                div[w] += diverged[w]
                depths[w] += j[w]
                if (m - n_ad[w]) % thin == 0:
                    k = (m - n_ad[w]) // thin - 1
                    if S > 0:
                        seg[w] = S * k // n_st[w]
                    if not keep_chain:
                        continue
                    if keep is None:
                        keep = engine.hmc_get()                               # (one download for all the walkers that keep this draw)
                    chains[w][k] = keep[0][w]
                    lps[w][k] = keep[1][w]
            if (seg >= 0).any():
                engine.hmc_accum_add(seg)
            if windows and in_window(m):
                engine.hmc_accum_add(0)
                if m in win_end:                                              # the window's variance becomes the metric
                    st = engine.hmc_accum_stats()
                    K = float(st["n_total"])
                    metric = st["sd"] ** 2 * (K / (K + 5.0)) + 1e-3 * (5.0 / (K + 5.0))
                    engine.hmc_set_metric(metric)
                    engine.hmc_accum_reset()
                    metric_windows.append((win_end[m], m))
                    if m < n_ad[0]:
                        mu, eps_bar, h_bar, da0 = np.log(10.0 * eps), np.ones(W), np.zeros(W), m
            if windows and S > 0 and m == n_ad[0]:
                engine.hmc_accum_reset()
        stream = engine.hmc_accum_stats() if S > 0 else None
    finally:
        engine.hmc_end()
    post = np.maximum(n_st * thin, 1)
    extra = {}
    if adapt_metric:
        extra.update(inv_mass=np.array(metric if metric is not None else (np.ones(D) if minv is None else minv), dtype=np.float64),
                     metric_windows=metric_windows)
    if S > 0:
        extra.update(stream=stream)
    return [(chains[w], lps[w], {"step_size": float(eps[w]), "mean_tree_depth": float(depths[w] / post[w]), "n_grad": int(n_grad[w]),
                                 "accept_rate": float(acc[w] / post[w]), "divergences": int(div[w]), **extra}) for w in range(W)]


SUMMARY_PROBS = (0.025, 0.25, 0.5, 0.75, 0.975)                  # MCMCChains.quantile's default q
_SUMMARY_KEYS = (("mean", "mean"), ("std", "sd"), ("mcse", "mcse"), ("ess", "ess"), ("rhat", "rhat"))


def _summary_arrays(engine, chain, probs, max_lag=0) -> Dict[str, np.ndarray]:
    """`Engine.chain_summary` under the `summary_*` keys of `mcmc_sample`'s output."""
    r = engine.chain_summary(chain, probs, max_lag=max_lag)
    out = {f"summary_{k}": r[src] for k, src in _SUMMARY_KEYS}
    out.update(summary_quantiles=r["quantiles"], summary_probs=np.asarray(probs, dtype=np.float64), summary_n_lags=r["n_lags"])
    return out


def _stream_engine(device: int = 0, _lib=None) -> Engine:
    """The smallest handle `bb_create` accepts (a fitness model of two barcodes, one neutral, three time points), for
    `summarize` without an engine of the caller's: `bb_chain_summary` takes its device and stream from a handle and reads nothing of
    the handle's model, so the counts below never reach a result."""
    return Engine("fitness", [np.array([[10, 12, 9], [11, 13, 8]], dtype=np.int64)], 2, 1, device=device, _lib=_lib)


def summarize(out_or_path, engine: Optional[Engine] = None, *, probs: Optional[Sequence[float]] = None, max_lag: int = 0,
              device: int = 0, _lib=None):
    """MCMCChains' `summarystats` + `quantile` of a chain as one table: one row per `var_names` entry, columns `parameters, mean,
    std, mcse, ess, rhat` and one `q<100 p>` per probability (`q2.5 ... q97.5`).  `out_or_path`: what `mcmc_sample` returned, or the
    `.npz` it wrote.  `probs` None: the output's own `summary_probs`, or SUMMARY_PROBS.  The `summary_*` arrays an output carries
    (`mcmc_sample(summary=True)`: `summary_probs`, no lag bound) are tabulated as they are where they answer the call -- `probs` None
    or equal to `summary_probs`, `max_lag` 0; otherwise the statistics are computed from `chain` on the device
    (`Engine.chain_summary`) through `engine`, or through a minimal handle of its own on `device`.  An output without a chain
    (`hmc_kwargs={"segments": S, "keep_chain": False}`) is tabulated from its `stream_*` arrays: no quantile columns, and its `ess` /
    `mcse` are the batch-means estimates of `Engine.hmc_accum_stats`."""
    import pandas as pd
    out = out_or_path
    if isinstance(out, (str, os.PathLike)):
        path = os.fspath(out)
        with np.load(path if os.path.isfile(path) else path + ".npz", allow_pickle=True) as z:
            out = {k: z[k] for k in z.files}
    if "stream_mean" in out and ("chain" not in out or np.shape(out["chain"])[1] == 0):      # the summary streamed on the device
        cols = {"parameters": [str(v) for v in out["var_names"]]}
        cols.update({k: np.asarray(out[f"stream_{src}"]) for k, src in _SUMMARY_KEYS})
        return pd.DataFrame(cols)
    stored = "summary_mean" in out and max_lag == 0 and (
        probs is None or np.array_equal(np.asarray(probs, dtype=np.float64), np.asarray(out["summary_probs"], dtype=np.float64)))
    probs = SUMMARY_PROBS if probs is None else probs
    if stored:
        s = out
    elif engine is not None:
        s = _summary_arrays(engine, out["chain"], probs, max_lag)
    else:
        with _stream_engine(device, _lib) as e:
            s = _summary_arrays(e, out["chain"], probs, max_lag)
    cols = {"parameters": [str(v) for v in out["var_names"]]}
    cols.update({k: np.asarray(s[f"summary_{k}"]) for k, _ in _SUMMARY_KEYS})
    for i, p in enumerate(np.asarray(s["summary_probs"], dtype=np.float64)):
        cols[f"q{100.0 * p:g}"] = np.asarray(s["summary_quantiles"])[:, i]
    return pd.DataFrame(cols)


def mcmc_sample(*, data, n_walkers: int, n_steps: int, outputname: Optional[str], model: Callable,
                model_kwargs: Optional[Dict] = None, id_col="barcode", time_col="time", count_col="count",
                neutral_col="neutral", rep_col: Optional[str] = None, env_col: Optional[str] = None,
                genotype_col: Optional[str] = None, rm_T0: bool = False, target_accept: float = 0.65,
                n_adapt: Optional[int] = None, advi_steps: int = 3000, verbose: bool = True, seed: int = 0, device: int = 0,
                engine_kwargs: Optional[Dict] = None, ensemble: str = "serial", summary: bool = False, sampler: str = "nuts",
                hmc_kwargs: Optional[Dict] = None, nuts_kwargs: Optional[Dict] = None):
    """src/mcmc.jl:86-160.  `sampler = Turing.NUTS(0.65)` becomes `target_accept`.  `ensemble` (the reference's
    `MCMCSerial()` / `MCMCThreads()` / `MCMCDistributed()`, all on one device here): "serial" runs the walkers one after another,
    all drawing from `default_rng(seed)`; "batched" steps them in lock-step, walker w drawing from `default_rng([seed, w])`, every
    round's log-densities in one `Engine.logdensity_grad_batch` call (chunks of BB_LOGP_MAX_BATCH walkers).
    `advi_steps` > 0 preconditions NUTS with a mean-field fit on the same handle (0: unit metric, prior-mean start).
    `summary` adds the chain diagnostics of every parameter (`Engine.chain_summary` on the same handle) to the output under
    `summary_mean, summary_std, summary_mcse, summary_ess, summary_rhat, summary_quantiles` (at `summary_probs`), `summary_n_lags`;
    `summarize` tabulates them.  It needs n_steps >= 4 and n_walkers * n_steps <= 16384 (BB_CHAIN_MAX_K: one pooled column in
    LDS), which is checked before anything is sampled.
    `sampler`: "nuts" (the default, the paths above) or "hmc": `hmc_ensemble` from the same ADVI start and metric, all walkers in
    lock-step with their state on the device (chunks of BB_HMC_MAX_WALKERS = 64 walkers; `ensemble` plays no part), walker w drawing from
    `default_rng([seed, w])`; `hmc_kwargs` go to `hmc_ensemble` (`n_leapfrog`, `thin`, `adapt_metric`, `segments`, `keep_chain`).  Its
    output has the same keys and `accept_rate`, `divergences`, `n_grad` per walker; with `adapt_metric` also `inv_mass` (the adapted
    metric), with `segments` the summary streamed on the device, `stream_mean, stream_sd, stream_mcse, stream_ess, stream_rhat` [D] and
    `stream_n` (`Engine.hmc_accum_stats`: `stream_ess` / `stream_mcse` are batch-means estimates over the walkers' segments, not the
    `summary_*` ones), which `summarize` tabulates when the output has no chain (`keep_chain=False`: `chain` has 0 draws and no position
    is ever downloaded).  Both need all walkers in one session, n_walkers <= BB_HMC_MAX_WALKERS; `summary=True` needs the chain.  Both
    are checked before anything is sampled.
    `ensemble="device"` (with `sampler="nuts"` only): `nuts_device`, the NUTS above with every vector of its tree on the device, from the
    same ADVI start and metric, in chunks of BB_HMC_MAX_WALKERS walkers with `hmc`'s generators and seed rule per chunk; `nuts_kwargs` go
    to `nuts_device` (`max_depth`, `thin`, `adapt_metric`, `segments`, `keep_chain`, with `hmc_kwargs`' conditions).  The output has
    `sampler="hmc"`'s keys and `mean_tree_depth`."""
    if sampler not in ("nuts", "hmc"):
        raise BarBayError(f"sampler must be 'nuts' or 'hmc', not {sampler!r}")
    if ensemble not in ("serial", "batched", "device"):
        raise BarBayError(f"ensemble must be 'serial', 'batched' or 'device', not {ensemble!r}")
    device_nuts = ensemble == "device"
    if device_nuts and sampler != "nuts":
        raise BarBayError(f"ensemble='device' is the device-resident NUTS: sampler must be 'nuts', not {sampler!r} (sampler='hmc' is "
                          f"device-resident whatever `ensemble`)")
    if nuts_kwargs and not device_nuts:
        raise BarBayError("nuts_kwargs go to nuts_device: they need sampler='nuts' with ensemble='device'")
    if summary and (n_walkers < 1 or n_steps < 4 or n_walkers * n_steps > BB_CHAIN_MAX_K):
        raise BarBayError(f"summary=True needs n_walkers >= 1, n_steps >= 4 and n_walkers * n_steps <= {BB_CHAIN_MAX_K}, not "
                          f"{n_walkers} x {n_steps}: sample with summary=False and summarize fewer draws")
    hk = (nuts_kwargs if device_nuts else hmc_kwargs) or {}
    resident = sampler == "hmc" or device_nuts
    if resident and (hk.get("segments", 0) or hk.get("adapt_metric", False)) and n_walkers > BB_HMC_MAX_WALKERS:
        raise BarBayError(f"segments / adapt_metric need all walkers in one session: n_walkers <= BB_HMC_MAX_WALKERS = "
                          f"{BB_HMC_MAX_WALKERS}, not {n_walkers}")
    if resident and summary and not hk.get("keep_chain", True):
        raise BarBayError("summary=True needs the chain: keep_chain=False returns the streamed summary (stream_*) alone")
    fname = None if outputname is None else f"{outputname}.npz"
    if fname is not None and os.path.isfile(fname):                                # :104-106
        raise BarBayError(f"{fname} was already processed")
    mname = getattr(model, "__name__", str(model))
    if "replicate" in mname and rep_col is None:                                   # :109-111
        raise BarBayError("Hierarchical models for experimental replicates require argument `:rep_col`")
    if "multienv" in mname and env_col is None:
        raise BarBayError("Models with multiple environments require argument `:env_col`")
    if verbose:
        log.info("Pre-processing data...")                                         # :115
    if rm_T0:                                                                      # documented kwarg of the reference
        data = data[data[time_col] != sorted(data[time_col].unique())[0]]
    arrays = utils.data_to_arrays(data, id_col=id_col, time_col=time_col, count_col=count_col, neutral_col=neutral_col,
                                  rep_col=rep_col, env_col=env_col, genotype_col=genotype_col)
    model_kwargs = dict(model_kwargs or {})
    if "multienv" in mname:
        model_kwargs = {"envs": arrays.envs, **model_kwargs}
    if "genotype" in mname:
        model_kwargs = {"genotypes": arrays.genotypes, **model_kwargs}
    bayes_model = model(arrays.bc_count, arrays.bc_total, arrays.n_neutral, arrays.n_bc, **model_kwargs)   # :138-144
    if not isinstance(bayes_model, BayesModel):
        raise BarBayError("model must be one of barbay model constructors (BarBay.model.*)")
    n_adapt = min(1000, n_steps // 2) if n_adapt is None else n_adapt              # Turing.NUTS default n_adapts
    if verbose:
        log.info("Sampling posterior...")                                          # :131-133
    rng = np.random.default_rng(seed)
    with _vi.make_engine(bayes_model, _vi.ADVI(1, max(advi_steps, 1)), _vi.TruncatedADAGrad(), seed, device,
                         **(engine_kwargs or {})) as e:
        ranges = [(lo, hi) for _, lo, hi in e.layout()]
        if advi_steps > 0:
            e.run(advi_steps)
            mean, sigma = e.posterior()
            minv = sigma ** 2
        else:
            mean, _ = e.posterior()
            mean, minv = np.zeros_like(mean), np.ones_like(mean)
        chains, lps, infos = [], [], []
        spread = 0.1 if advi_steps > 0 else 0.0
        batched = []
        lockstep = ensemble == "batched" or resident
        if lockstep:
            rngs = [np.random.default_rng([seed, w]) for w in range(n_walkers)]
            z0s = [mean + np.sqrt(minv) * r.standard_normal(mean.shape[0]) * spread for r in rngs]
            for lo in range(0, n_walkers, BB_LOGP_MAX_BATCH):                 # (= BB_HMC_MAX_WALKERS)
                hi = min(lo + BB_LOGP_MAX_BATCH, n_walkers)
                if resident:                                                  # (a walker's stream is its index in the chunk: a key per chunk)
                    batched += (nuts_device if device_nuts else hmc_ensemble)(
                        e, z0s[lo:hi], n_steps, n_adapt, rngs=rngs[lo:hi], target_accept=target_accept, minv=minv,
                        seed=(seed + 0x9E3779B97F4A7C15 * (lo // BB_LOGP_MAX_BATCH)) % 2 ** 64, **hk)
                else:
                    batched += nuts_ensemble(e.logdensity_grad_batch, z0s[lo:hi], n_steps, n_adapt, rngs=rngs[lo:hi],
                                             target_accept=target_accept, minv=minv)
        for w in range(n_walkers):
            if lockstep:
                c, lp, info = batched[w]
            else:
                z0 = mean + np.sqrt(minv) * rng.standard_normal(mean.shape[0]) * spread
                c, lp, info = nuts(e.logdensity_grad, z0, n_steps, n_adapt, target_accept=target_accept, minv=minv, rng=rng)
            chains.append(c)
            lps.append(lp)
            infos.append(info)
            if verbose and sampler == "hmc":
                log.info("walker %d: step size %.3g, acceptance %.2f, %d divergences, %d gradients", w + 1, info["step_size"],
                         info["accept_rate"], info["divergences"], info["n_grad"])
            elif verbose:
                log.info("walker %d: step size %.3g, mean tree depth %.2f, %d gradients", w + 1, info["step_size"],
                         info["mean_tree_depth"], info["n_grad"])
        summ = _summary_arrays(e, np.stack(chains), SUMMARY_PROBS) if summary else {}
    var_names = []
    for sym, (lo, hi) in zip(bayes_model.var_symbols(), ranges):
        var_names += [f"{sym}[{x}]" for x in range(1, hi - lo + 1)]
    out = {"ids": np.asarray(arrays.bc_ids, dtype=object), "var_names": np.asarray(var_names, dtype=object),
           "chain": np.stack(chains), "logp": np.stack(lps), "step_size": np.asarray([i["step_size"] for i in infos]), **summ}
    if resident:
        out.update({k: np.asarray([i[k] for i in infos]) for k in ("accept_rate", "divergences", "n_grad") + (("mean_tree_depth",) if device_nuts else ())})
        if "inv_mass" in infos[0]:
            out["inv_mass"] = infos[0]["inv_mass"]
        if "stream" in infos[0]:
            st = infos[0]["stream"]
            out.update({f"stream_{k}": st[k] for k in ("mean", "sd", "mcse", "ess", "rhat")}, stream_n=np.int64(st["n_total"]))
    if fname is None:
        return out
    if verbose:
        log.info("Saving %s chain...", fname)                                      # :155-157
    np.savez(fname, **out)
    return None
