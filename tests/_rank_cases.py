"""bb_fitness_rank (posterior ranks and top-k membership of the units of sets, barbay.jl_amd/csrc/bb_rank.h) restated in numpy, and
the cases the emulation and GPU tests share.

The order (include/barbay_hip.h): within a set position a ranks before b when v_a > v_b, or v_a is a number and v_b NaN, or neither
holds either way and a < b.  `order_ranks` is numpy's stable lexsort on (is NaN, -v): the primary key puts NaN last, -v descends
(-0.0 == +0.0 compare equal), stability gives ties to the caller's order.

The sorter is checked exactly: kind FITNESS, source "draws" and explicit draws, where s_{u,j} is the array entry itself
(`check_sorter`, `check_sorter_large`).  The conditional source is checked against `_rb_cases.conditionals` plus the host Philox
pair at stream 0xFFFFFFE3: the library's (m, sd, N) differ from numpy's by a few ulp (about 1e-15, `_rb_cases`), so a (set, draw)
column whose restated neighbours in value lie closer than GAP = 1e-10 is left out of the exact comparison of `ranks`; at most
1 % of a case's columns may be (`check_gaps`, on the restatement alone).  Over the kept columns `ranks` are exact.  rank_mean and
p_top are exact; rank_sd and quantiles within 1e-12 of max(|x|, 1) (sums of at most 8672 squares of integers below 2^31 in float64:
the restatement's own rounding is of order 1e-16 relative).

Measured (each test prints its own line):

`check_gaps` (restatement): smallest gap between restated neighbours over the case's (set, draw) columns, n = 2 / 111 / 1000;
no column was left out in any case
  fitness                   7.1e-04 / 8.5e-06 / 5.7e-07      genotype_regrouped        2.2e-05 / 1.2e-06 / 1.2e-07
  multienv                  5.1e-05 / 5.8e-08 / 5.8e-08      multienv_replicate        6.9e-06 / 5.3e-07 / 5.4e-09
  replicate_ragged          1.9e-06 / 2.5e-07 / 6.2e-08      multienv_env0_only_first  3.9e-04 / 1.9e-06 / 1.5e-07
  fitness_chunk             3.8e-06 / 4.4e-07 / 1.1e-08
`check_conditional`, emulation and MI355X alike (the printed lines are equal): `ranks` exact on every entry (208 entries for
fitness at n = 2 up to 564 000 for fitness_chunk at n = 1000), 0 columns left out, rank_mean and p_top exact, largest error of
rank_sd / quantiles relative to max(|x|, 1), n = 2 / 111 / 1000, in units of 1e-16
  fitness                   2.1 / 4.0 / 2.5      genotype_regrouped        1.5 / 4.0 / 4.0      multienv              2.1 / 5.6 / 4.6
  multienv_replicate        1.8 / 6.0 / 6.8      replicate_ragged          1.9 / 7.1 / 3.0      multienv_env0_only_first  2.1 / 5.2 / 4.8
  fitness_chunk             2.2 / 4.7 / 4.9
  (the largest, 7.1e-16, is 0.0007 of the bound 1e-12)
`check_sorter`: 11 planted columns, sets of 1 .. 280 units: ranks exact at runs of 64, 128 and 8192; rank_sd / quantiles 2.9e-16.
`check_sorter_large`: sets of 8191, 8192, 8193 and 20 000 units exact at runs of 8192 and 4096; 2.2e-16.  Creating the
20 000-mutant handle takes the emulation under three seconds, so both stay in the emulation's file too.
`check_point_restated` / `check_point` (replicate_ragged, posterior sd of s_pop 0.3, sets spanning the three replicates,
n = 1000): mean rank_sd conditional 7.052, draws 2.589 -- restatement, emulation and MI355X.
`test_ranks_against_a_large_numpy_sample` (MI355X): the largest deviation of p_top[k = 2] and rank_mean over the six units is
1.6 standard errors (unit 3, p_top2 0.0033 against 0.0025 +- 0.0005); unit 31 is never among the two fittest in either sample.
"""
import ctypes as C
import functools

import numpy as np

import _contrast_cases as cc
import _ppc_cases as pc
import _rb_cases as rc
import _score_cases as sc
from conftest import make_engine
from oracle import fixtures, rng
from barbay_jl_amd import _capi

STREAM_RANK = 0xFFFFFFE3
SEED, PROBS, NS = rc.SEED, rc.PROBS, rc.NS
MAXN = _capi.BB_RANK_MAX_SAMPLES
RUN = _capi.BB_RANK_RUN
GAP = 1e-10
TOL = 1e-12
BIGTOP = 2 ** 31 - 1
CASES = tuple(rc.all_cases())
SIZES = (1, 2, 3, 63, 64, 65, 127, 128, 129, 280)
VALUES = ("rank_mean", "rank_sd", "p_top", "quantiles")


# ---- the order and the summaries ------------------------------------------------------------------------------------------------
def order_ranks(v):
    """ranks [n, ns] (int32) of the values v [n, ns], column by column, by the header's order."""
    v = np.asarray(v, dtype=np.float64)
    nan = np.isnan(v)
    neg = np.where(nan, 0.0, -v)
    order = np.lexsort((neg, nan), axis=0)                       # stable: ties keep the caller's order
    ranks = np.empty(v.shape, dtype=np.int32)
    np.put_along_axis(ranks, order, np.arange(v.shape[0], dtype=np.int32)[:, None], axis=0)
    return ranks


def set_ranks(v, sets):
    """`order_ranks` per set of units of the values v [n_units, ns], concatenated by position."""
    return np.concatenate([order_ranks(v[np.asarray(s, dtype=np.int64)]) for s in sets], axis=0)


def summaries(ranks, top, probs):
    """rank_mean, rank_sd, p_top, quantiles from the rank table [n_idx, ns]: the header's formulas."""
    r = ranks.astype(np.float64)
    ns = r.shape[1]
    mean = r.sum(axis=1) / ns
    out = {"rank_mean": mean, "rank_sd": np.sqrt(((r - mean[:, None]) ** 2).sum(axis=1) / ns),
           "p_top": np.stack([(ranks < k).sum(axis=1) / ns for k in top], axis=1) if len(top) else np.empty((r.shape[0], 0))}
    srt = np.sort(r, axis=1)
    out["quantiles"] = np.stack([pc.quantile7(srt, p) for p in probs], axis=1) if len(probs) and ns >= 2 else np.empty((r.shape[0], 0))
    return out


def assert_summaries(got, ref, who):
    assert np.array_equal(got["rank_mean"], ref["rank_mean"]), who
    assert np.array_equal(got["p_top"], ref["p_top"]), who
    worst = 0.0
    for k in ("rank_sd", "quantiles"):
        assert got[k].shape == ref[k].shape, (who, k)
        err = np.abs(got[k] - ref[k]) / np.maximum(np.abs(ref[k]), 1.0)
        worst = max(worst, float(err.max(initial=0.0)))
        assert worst <= TOL, (who, k, worst)
    return worst


def assert_permutations(ranks, ptr):
    for c in range(len(ptr) - 1):
        col = np.sort(ranks[ptr[c]:ptr[c + 1]], axis=0)
        assert np.array_equal(col, np.broadcast_to(np.arange(ptr[c + 1] - ptr[c], dtype=np.int32)[:, None], col.shape)), c


def rank(e, sets, n, **kw):
    kw.setdefault("probs", PROBS)
    kw.setdefault("seed", SEED)
    kw.setdefault("want_ranks", True)
    return e.fitness_rank([list(s) for s in sets] if not isinstance(sets, tuple) else sets, n_samples=n, **kw)


def pieces(res, c):
    """The results of set c, as bytes."""
    a, b = int(res["set_ptr"][c]), int(res["set_ptr"][c + 1])
    return [np.ascontiguousarray(res[k][a:b]).tobytes() for k in VALUES + ("ranks",) if k in res] + [int(res["n_units"][c])]


def same_bytes(a, b):
    return rc.same_bytes(a, b)


# ---- 1. the sorter, exactly ------------------------------------------------------------------------------------------------------
def planted(n, seed=0):
    """Columns [P, n] of values that try the order: all equal; blocks of duplicates; +-0.0; +-Inf; NaN of both signs, several;
    subnormals; negative values; neighbours one ulp apart; ascending; descending; a shuffle of everything."""
    g = np.random.default_rng(seed)
    base = g.normal(0.0, 1.0, n)
    cols = [np.full(n, 0.25), np.repeat(g.normal(0.0, 1.0, (n + 6) // 7), 7)[:n]]
    z = np.where(np.arange(n) % 2 == 0, 0.0, -0.0)
    z[g.random(n) < 0.3] = 1e-300
    z[g.random(n) < 0.2] = -1e-300
    cols.append(z)
    x = base.copy()
    x[g.random(n) < 0.2] = np.inf
    x[g.random(n) < 0.2] = -np.inf
    cols.append(x)
    x = base.copy()
    x[g.random(n) < 0.25] = np.nan
    x[g.random(n) < 0.25] = np.copysign(np.nan, -1.0)
    x[g.random(n) < 0.1] = -np.inf
    cols.append(x)
    cols.append(g.integers(-3, 4, n) * 4.9406564584124654e-324)
    cols.append(-np.abs(base) - 1.0)
    x = np.full(n, 1.0)
    for i in range(1, n):
        x[i] = np.nextafter(x[i - 1], 2.0 if i % 3 else 0.0)
    cols.append(x)
    cols.append(np.arange(n, dtype=np.float64) / 16.0 - 3.0)
    cols.append(3.0 - np.arange(n, dtype=np.float64) / 16.0)
    mix = np.concatenate(cols)
    cols.append(g.permutation(mix)[:n])
    return np.stack(cols)


def planted_draws(sp, vals):
    """Explicit draws [P, D], zero except the s_bc block, which holds the planted columns: with source "draws" a FITNESS unit's
    value is that array entry itself."""
    lo, hi = sp.offsets()["s_bc"]
    assert hi - lo == vals.shape[1] and sp.kind == "fitness"
    dr = np.zeros((vals.shape[0], sp.D))
    dr[:, lo:hi] = vals
    return dr


def sorter_sets(nu, sizes=SIZES):
    """One set per size: consecutive units from a shifting start, every other one reversed (the caller's order is not the units')."""
    sets = []
    for i, k in enumerate(sizes):
        a = (17 * i) % (nu - k + 1)
        s = list(range(a, a + k))
        sets.append(s[::-1] if i % 2 else s)
    return sets


def check_sorter(lib):
    """The device `ranks` against numpy's stable lexsort, entry for entry, on the planted columns; sets of 1 .. 280 units of
    `fitness_chunk` at a run length of 64 (the 65 .. 280-unit sets take the multi-run path) and at the default run: bit-equal;
    rank_mean and p_top (k = 1, 64, 280, 2^31 - 1: below, at and above n) exact, rank_sd and quantiles within 1e-12."""
    sp = rc.spec("fitness_chunk")
    nu = rc.n_units(sp)
    assert nu == 280
    vals = planted(nu)
    dr = planted_draws(sp, vals)
    sets = sorter_sets(nu)
    top = (1, 64, 280, BIGTOP)
    want = set_ranks(vals.T, sets)
    ref = summaries(want, top, PROBS)
    with make_engine(sp, lib, seed=1) as e:
        short = rank(e, sets, 0, draws=dr, source="draws", top=top, _run=64)
        full = rank(e, sets, 0, draws=dr, source="draws", top=top)
        mid = rank(e, sets, 0, draws=dr, source="draws", top=top, _run=128)
    assert same_bytes(short, full) and same_bytes(mid, full)
    assert np.array_equal(full["ranks"], want)
    assert_permutations(full["ranks"], full["set_ptr"])
    assert np.array_equal(full["n_units"], [len(s) for s in sets])
    worst = assert_summaries(full, ref, "sorter")
    print(f"rank sorter: {vals.shape[0]} planted columns, sets {SIZES}: ranks exact at runs of 64, 128 and {RUN}; rank_sd / quantiles {worst:.1e}")


LARGE_B, LARGE_NEUTRAL = 20020, 20


@functools.lru_cache(maxsize=None)
def large_spec():
    return fixtures.synthetic("fitness", B=LARGE_B, T=3, n_neutral=LARGE_NEUTRAL, seed=5)


def check_sorter_large(lib):
    """One model of 20 000 mutants (T = 3, three draws) at the real BB_RANK_RUN: sets of 8191, 8192 and 8193 units (one run, a
    full run, two runs) and one of 20 000 (three runs), on planted columns with duplicates, NaN and infinities."""
    sp = large_spec()
    nu = rc.n_units(sp)
    assert nu == LARGE_B - LARGE_NEUTRAL == 20000
    g = np.random.default_rng(1)
    vals = np.stack([np.round(g.normal(0.0, 1.0, nu), 2), g.normal(0.0, 1.0, nu), planted(nu, 2)[-1]])
    dr = planted_draws(sp, vals)
    sets = [list(range(5, 5 + RUN - 1)), list(range(RUN, 0, -1)), list(range(100, 100 + RUN + 1)), list(range(nu))[::-1]]
    top = (1, RUN, BIGTOP)
    want = set_ranks(vals.T, sets)
    with make_engine(sp, lib, seed=1) as e:
        got = rank(e, sets, 0, draws=dr, source="draws", top=top)
        halved = rank(e, sets, 0, draws=dr, source="draws", top=top, _run=RUN // 2)
    assert np.array_equal(got["ranks"], want)
    assert same_bytes(got, halved)
    worst = assert_summaries(got, summaries(want, top, PROBS), "large sorter")
    print(f"rank sorter, large: sets {[len(s) for s in sets]} exact at runs of {RUN} and {RUN // 2}; rank_sd / quantiles {worst:.1e}")


# ---- 2. the conditional source against the restatement ----------------------------------------------------------------------------
def rank_normals(nu, n, seed=SEED):
    """N(u, j >> 1, 0xFFFFFFE3) [n_units, n]: an even j the cosine branch, an odd j the sine branch."""
    j = np.arange(n, dtype=np.uint64)
    out = np.empty((nu, n))
    for u in range(nu):
        a, b = rng.pairs(seed, np.full(j.shape, u, dtype=np.uint64), j >> np.uint64(1), STREAM_RANK)
        out[u] = np.where(j & np.uint64(1), b, a)
    return out


def redraw(el, seed=SEED):
    """v = m + sd N [n_units, n] from the elements (s, m, sd, n_steps)."""
    _, m, sd, _ = el
    with np.errstate(all="ignore"):
        return m + sd * rank_normals(m.shape[0], m.shape[1], seed)


@functools.lru_cache(maxsize=None)
def values_at(case, n):
    v = redraw(cc.elements_at("fitness", case, n))
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def case_sets(case):
    """The whole library, the by="rep_env" sets, a one-unit set and a three-unit set."""
    sp = rc.inputs(case)[0]
    E, nb, R, nu = rc.n_env(sp), sp.n_bc, sp.n_rep, rc.n_units(sp)
    sets = [list(range(nu))] + [[e + E * m + E * nb * r for m in range(nb)] for r in range(R) for e in range(E)]
    sets += [[nu // 2], [nu - 1, 0, nu // 3]]
    return tuple(tuple(s) for s in sets)


def kept_columns(v, sets):
    """Per set the draws whose sorted values have no two neighbours closer than GAP (NaN and infinities aside: they tie or
    differ exactly), and the smallest gap seen."""
    keep, smallest = [], np.inf
    for s in sets:
        x = np.sort(v[np.asarray(s, dtype=np.int64)], axis=0)
        with np.errstate(all="ignore"):
            d = np.diff(x, axis=0)
        d = np.where(np.isfinite(d), d, np.inf)
        gap = d.min(axis=0, initial=np.inf)
        smallest = min(smallest, float(gap.min(initial=np.inf)))
        keep.append(gap >= GAP)
    return keep, smallest


def check_gaps(case, n):
    """At most 1 % of the case's (set, draw) columns are left out of the exact comparison: on the restatement alone."""
    keep, smallest = kept_columns(values_at(case, n), case_sets(case))
    out, cols = sum(int((~k).sum()) for k in keep), sum(k.shape[0] for k in keep)
    print(f"rank gaps {case:28s} n {n:4d}: smallest {smallest:.2e}, {out} of {cols} columns left out")
    assert out <= 0.01 * cols, (case, n, out, cols)
    return out


def column_mask(keep, sets):
    """[n_idx, ns] True where the position's (set, draw) column is kept."""
    return np.concatenate([np.broadcast_to(k[None, :], (len(s), k.shape[0])) for k, s in zip(keep, sets)], axis=0)


def check_conditional(lib, case, n, label):
    sp, mu, om = rc.inputs(case)
    sets = case_sets(case)
    v = values_at(case, n)
    keep, _ = kept_columns(v, sets)
    want = set_ranks(v, sets)
    top = (1, 3, len(sets[1]), BIGTOP)
    with pc._handle(lib, sp, mu, om) as e:
        got = rank(e, sets, n, top=top)
    assert got["ranks"].shape == want.shape and got["ranks"].dtype == np.int32
    assert_permutations(got["ranks"], got["set_ptr"])
    mask = column_mask(keep, sets)
    assert np.array_equal(got["ranks"][mask], want[mask]), case
    left = int(sum((~k).sum() for k in keep))
    ref = summaries(want if left == 0 else got["ranks"], top, PROBS)
    worst = assert_summaries(got, ref, case)
    one = int(got["set_ptr"][len(sets) - 2])                      # the one-unit set: rank 0, sd 0, p_top 1, quantiles 0
    assert np.all(got["ranks"][one] == 0) and got["rank_mean"][one] == 0 and got["rank_sd"][one] == 0
    assert np.all(got["p_top"][one] == 1) and np.all(got["quantiles"][one] == 0)
    print(f"rank case {case:28s} n {n:4d} {label:10s}: ranks exact on {int(mask[:, :].sum())} entries, {left} columns left out, rank_sd / quantiles {worst:.1e}")
    return got


# ---- 3. what the call exists for ---------------------------------------------------------------------------------------------------
def point_inputs():
    """Case replicate_ragged (three replicates), `_rb_cases.params` with the s_pop block's posterior sd at 0.3, as
    `_contrast_cases.point_inputs` does for one replicate."""
    sp, mu, om = rc.inputs("replicate_ragged")
    om = om.copy()
    om[slice(*sp.offsets()["s_pop"])] = np.log(np.expm1(0.3))
    return sp, mu, om


def point_sets(sp):
    """The whole library and every environment's units across the replicates: sets that span the replicates."""
    E, nb, R, nu = rc.n_env(sp), sp.n_bc, sp.n_rep, rc.n_units(sp)
    return [list(range(nu))] + [[e + E * m + E * nb * r for r in range(R) for m in range(nb)] for e in range(E)]


def check_point_restated(n=1000):
    sp, mu, om = point_inputs()
    with np.errstate(all="ignore"):
        el = rc.conditionals(sp, sc.Draws(SEED, mu, pc.softplus(om), n), n)
    sets = point_sets(sp)
    cond = summaries(set_ranks(redraw(el), sets), (), ())["rank_sd"].mean()
    own = summaries(set_ranks(el[0], sets), (), ())["rank_sd"].mean()
    print(f"rank point, restatement: mean rank_sd conditional {cond:.3f}, draws {own:.3f}")
    assert cond > own, (cond, own)
    return cond, own


def check_point(lib, n=1000):
    """With the population means' posterior sd at 0.3 the units of a replicate move together with its sbar_t: over sets that span
    the replicates the mean rank_sd of the conditional redraw exceeds that of q's own draws, which have no such coupling."""
    sp, mu, om = point_inputs()
    sets = point_sets(sp)
    with pc._handle(lib, sp, mu, om) as e:
        cond = rank(e, sets, n, top=(), probs=(), want_ranks=False)["rank_sd"].mean()
        own = rank(e, sets, n, top=(), probs=(), want_ranks=False, source="draws")["rank_sd"].mean()
    print(f"rank point: mean rank_sd conditional {cond:.3f}, draws {own:.3f}")
    assert cond > own, (cond, own)
    return cond, own


# ---- 4. structure and determinism ------------------------------------------------------------------------------------------------
def check_independent_of_the_rest_of_the_call(lib, case, n=111):
    """A set's bytes do not change when other sets are added, removed or reordered, a unit also sits in another set, the CSR pair
    is given, the bound forces one set per slab or tiles of draws, or the run length changes."""
    sp, mu, om = rc.inputs(case)
    sets = [list(s) for s in case_sets(case)]
    perm = np.random.default_rng(3).permutation(len(sets))
    top = (1, 5)
    with pc._handle(lib, sp, mu, om) as e:
        base = rank(e, sets, n, top=top)
        again = rank(e, sets, n, top=top)
        shuffled = rank(e, [sets[i] for i in perm], n, top=top)
        more = rank(e, sets[::2] + sets, n, top=top)
        alone = [rank(e, [sets[i]], n, top=top) for i in (0, len(sets) - 1)]
        csr = rank(e, (np.cumsum([0] + [len(s) for s in sets]), [k for s in sets for k in s]), n, top=top)
        slabs = [rank(e, sets, n, top=top, _bound_kib=k) for k in (1, 8, 64, 1 << 20)]       # tiles of draws; sets one at a time; a few; all
        runs = rank(e, sets, n, top=top, _run=64, _bound_kib=4)
        both = [rank(e, sets, n, top=top, source="draws"), rank(e, sets, n, top=top, source="draws", _bound_kib=1, _run=64)]
    assert same_bytes(base, again) and same_bytes(base, csr) and same_bytes(base, runs) and same_bytes(both[0], both[1])
    assert not np.array_equal(base["ranks"], both[0]["ranks"])
    for s in slabs:
        assert same_bytes(base, s)
    for x, i in enumerate(perm):
        assert pieces(shuffled, x) == pieces(base, i), i
    half = len(sets[::2])
    for i in range(len(sets)):
        assert pieces(more, half + i) == pieces(base, i), i
        assert i % 2 or pieces(more, i // 2) == pieces(base, i), i
    assert pieces(alone[0], 0) == pieces(base, 0) and pieces(alone[1], 0) == pieces(base, len(sets) - 1)
    assert_permutations(base["ranks"], base["set_ptr"])


def check_launch_modes(lib, case="replicate_ragged"):
    import barbay_jl_amd as bb
    sp, mu, om = rc.inputs(case)
    sets = [list(s) for s in case_sets(case)]
    out = []
    for mode in (1, 0):
        with bb.Engine(sp.kind, sp.counts, sp.n_neutral, sp.n_bc, env_idx=sp.env_idx, geno_idx=sp.geno_idx, seed=4, launch_mode=mode, _lib=lib) as e:
            e.set_params(mu, om)
            out.append(rank(e, sets, 500, seed=2))
            out.append(rank(e, sets, 500, seed=2))
    assert all(same_bytes(out[0], o) for o in out[1:])


def check_group_handle(lib, case):
    sp, mu, om = rc.inputs(case)
    sets = [list(s) for s in case_sets(case)]
    with pc._handle(lib, sp, mu, om, device_ids=[0, 0]) as e:
        a = rank(e, sets, 111)
    with pc._handle(lib, sp, mu, om) as e:
        b = rank(e, sets, 111)
    assert same_bytes(a, b)


def check_buffer_reuse(lib):
    """The call among the other post-fit calls at growing and shrinking sizes on one handle: every result is byte for byte what
    a fresh handle gives."""
    sp, mu, om = rc.inputs("fitness")
    sets = [list(s) for s in case_sets("fitness")]
    dr = rc.materialise(sp, mu, om, 7, 3)
    calls = [lambda e: rank(e, sets, 111),
             lambda e: e.ppc_bands((0.95, 0.675, 0.05), n_samples=111, n_ppc=7, seed=SEED),
             lambda e: rank(e, sets[:2], 1000, top=(2,)),
             lambda e: rc.rb(e, 111),
             lambda e: rank(e, sets + sets, 2, source="draws"),
             lambda e: e.ppc_score(n_samples=111, seed=SEED),
             lambda e: rank(e, sets[2:], 7, draws=dr, _run=64),
             lambda e: e.dfe_rb(sets, (0.0, 0.25), n_samples=64, seed=SEED),
             lambda e: rank(e, sets[:1], 2049, probs=(0.5,), top=()),
             lambda e: rank(e, sets, 111)]
    with pc._handle(lib, sp, mu, om) as e:
        got = [pc._bits(f(e)) for f in calls]
    for i, f in enumerate(calls):
        with pc._handle(lib, sp, mu, om) as e:
            assert got[i] == pc._bits(f(e)), i
    assert got[0] == got[-1]


def check_handle_untouched(lib):
    sp = rc.spec("fitness")
    sets = [list(s) for s in case_sets("fitness")]
    with make_engine(sp, lib, seed=5) as a, make_engine(sp, lib, seed=5) as b:
        rank(b, sets, 111)
        for x, y in zip(a.get_params(), b.get_params()):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
        a.run(5)
        rank(b, sets, 64, seed=1, source="draws")
        b.run(5)
        for x, y in zip(a.get_params(), b.get_params()):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64))


def check_internal_against_explicit_draws(lib, case, n=111):
    """The library's own draws against the same draws made on the host and passed in (`seed` keys the redraw's normal with
    explicit draws too): `ranks` equal on every column the gap rule keeps, for both sources."""
    sp, mu, om = rc.inputs(case)
    sets = case_sets(case)
    dr = rc.materialise(sp, mu, om, n, SEED)
    with np.errstate(all="ignore"):
        el = rc.conditionals(sp, rc.Rows(dr), n)
    with pc._handle(lib, sp, mu, om) as e:
        for source, v in (("conditional", redraw(el)), ("draws", el[0])):
            a = rank(e, sets, n, source=source)
            b = rank(e, sets, n, source=source, draws=dr)
            c = rank(e, sets, 5, source=source, draws=dr)           # n_samples is the row count; the argument is ignored
            assert same_bytes(b, c)
            mask = column_mask(kept_columns(v, sets)[0], sets)
            assert mask.mean() >= 0.99 and np.array_equal(a["ranks"][mask], b["ranks"][mask]), (case, source)
            assert np.array_equal(b["ranks"][mask], set_ranks(v, sets)[mask]), (case, source)


def check_nan_parameter(lib, case="multienv", n=111):
    """One mutant's logsigma_bc means NaN: its units' conditionals are NaN, so they rank last in every set that names them -- in
    the caller's order among themselves -- and stay in their sets; the sets that name none of them keep their bytes."""
    sp, mu, om = rc.inputs(case)
    E, m = rc.n_env(sp), 4
    sets = [list(s) for s in case_sets(case)] + [[0, 1, 2], [E * 9 + 1]]
    mu2 = mu.copy()
    lo = sp.offsets()["logsigma_bc"][0]
    mu2[lo + E * m:lo + E * (m + 1)] = np.nan
    with pc._handle(lib, sp, mu, om) as e:
        base = rank(e, sets, n)
    with pc._handle(lib, sp, mu2, om) as e:
        got = rank(e, sets, n)
    assert_permutations(got["ranks"], got["set_ptr"])
    hit = 0
    for c, s in enumerate(sets):
        bad = [x for x, k in enumerate(s) if E * m <= k < E * (m + 1)]
        if not bad:
            assert pieces(got, c) == pieces(base, c), c
            continue
        hit += 1
        a = int(got["set_ptr"][c])
        for i, x in enumerate(bad):
            assert np.all(got["ranks"][a + x] == len(s) - len(bad) + i), (c, x)
    assert 0 < hit < len(sets)


# ---- 5. errors -----------------------------------------------------------------------------------------------------------------
OUTS = VALUES + ("ranks", "n_units")


def raw(engine, sets, n_samples=64, probs=PROBS, top=(1, 10), source=0, seed=SEED, draws=None, null=(), want=OUTS, n_quantiles=None, n_top=None,
        n_sets=None, ptr=None, nout=None, reserved0=0, reserved1=0):
    """bb_fitness_rank through ctypes with only the outputs in `want` non-NULL; `null` names arguments passed as NULL."""
    tp = np.ascontiguousarray(np.cumsum([0] + [len(s) for s in sets]) if ptr is None else ptr, dtype=np.int64)
    ti = np.ascontiguousarray([k for s in sets for k in s] + [0], dtype=np.int64)
    p = np.ascontiguousarray(probs, dtype=np.float64)
    t = np.ascontiguousarray(list(top) + [1], dtype=np.int64)
    nc = len(sets) if n_sets is None else n_sets
    o = _capi.bb_rank_opts()
    o.n_samples, o.n_quantiles, o.n_top, o.source = n_samples, len(p) if n_quantiles is None else n_quantiles, len(top) if n_top is None else n_top, source
    o.reserved0, o.reserved1, o.seed, o.n_sets = reserved0, reserved1, seed, nc
    i64 = C.POINTER(C.c_int64)
    o.probs = None if "probs" in null or not len(p) else _capi._ptr(p)
    o.top = None if "top" in null else t.ctypes.data_as(i64)
    o.set_ptr = None if "set_ptr" in null else tp.ctypes.data_as(i64)
    o.set_idx = None if "set_idx" in null else ti.ctypes.data_as(i64)
    if draws is not None:
        o.draws = _capi._ptr(draws)
    nix = (len(ti) - 1 if nc > 0 else 0) if nout is None else nout
    shapes = {"rank_mean": (nix,), "rank_sd": (nix,), "p_top": (nix, len(top)), "quantiles": (nix, len(p)), "ranks": (nix, max(n_samples, 1)), "n_units": (max(nc, 0),)}
    res, out = {}, _capi.bb_rank_out()
    for k in want:
        dt = np.int32 if k == "ranks" else np.int64 if k == "n_units" else np.float64
        res[k] = np.full(shapes[k], -7, dtype=dt)
        setattr(out, k, res[k].ctypes.data_as(C.POINTER({np.int32: C.c_int32, np.int64: C.c_int64, np.float64: C.c_double}[dt])))
    rcode = engine._lib.bb_fitness_rank(None if "h" in null else engine._h, None if "o" in null else C.byref(o), None if "out" in null else C.byref(out))
    return rcode, res


def check_errors(lib):
    """Every BB_ERR_INVALID and BB_ERR_UNSUPPORTED of the contract, the set errors with a message that names the set and the
    position; an all-NULL out, each output alone, n_sets == 0.  NOT exercised: BB_ERR_DEVICE, and the 2^31 indices as real arrays."""
    sp, mu, om = rc.inputs("fitness")
    INVALID, UNSUPPORTED = -1, _capi.BB_ERR_UNSUPPORTED
    msg = lambda: lib.bb_last_error().decode()
    sets = [list(s) for s in case_sets("fitness")]
    nu = rc.n_units(sp)
    dr = rc.materialise(sp, mu, om, 3, 1)
    with pc._handle(lib, sp, mu, om) as e:
        for null in ("h", "o", "out"):
            assert raw(e, sets, null=(null,))[0] == INVALID and msg(), null
        for null in ("set_ptr", "set_idx"):
            assert raw(e, sets, null=(null,))[0] == INVALID and "null" in msg(), null
        assert raw(e, sets, n_sets=-1)[0] == INVALID and "n_sets" in msg()
        for bad in (-1, 2, 7):
            assert raw(e, sets, source=bad)[0] == INVALID and "source" in msg(), bad
        for nt in (-1, 9):
            assert raw(e, sets, n_top=nt)[0] == INVALID and "n_top" in msg(), nt
        assert raw(e, sets, null=("top",))[0] == INVALID and "top" in msg() and "null" in msg()
        for bad in (0, -3, 1 << 31):
            assert raw(e, sets, top=(1, bad))[0] == INVALID and "top[1]" in msg(), bad
        assert raw(e, sets, top=(BIGTOP,))[0] == 0
        assert raw(e, sets, reserved0=-1)[0] == INVALID and "reserved0" in msg()
        assert raw(e, sets, reserved0=96)[0] == INVALID and "reserved0" in msg()
        assert raw(e, sets, reserved1=-1)[0] == INVALID and "reserved1" in msg()
        assert raw(e, sets, ptr=[1] + [2 * (i + 1) for i in range(len(sets))])[0] == INVALID and "set_ptr[0]" in msg()
        assert raw(e, sets[:3], ptr=[0, 2, 1, 3])[0] == INVALID and "set 1" in msg() and "decreases" in msg()
        assert raw(e, [sets[0], [], sets[1]])[0] == INVALID and "set 1" in msg() and "no units" in msg()
        for bad in (-1, nu, 1 << 40):
            assert raw(e, [sets[0], [3, bad]])[0] == INVALID and "set 1, position 1" in msg() and "outside" in msg(), bad
        assert raw(e, [sets[0], sets[1], [3, 5, 3]])[0] == INVALID and "set 2, position 2" in msg() and "twice" in msg()
        for nq in (-1, 9):
            assert raw(e, sets, n_quantiles=nq)[0] == INVALID and "n_quantiles" in msg(), nq
        assert raw(e, sets, null=("probs",), n_quantiles=3)[0] == INVALID and "probs" in msg()
        for bad in (0.0, 1.0, -0.1, 1.5, np.nan):
            assert raw(e, sets, probs=(0.5, bad))[0] == INVALID and "prob" in msg(), bad
        for n in (1, 0, -3, MAXN + 1):
            assert raw(e, sets, n_samples=n)[0] == UNSUPPORTED and "n_samples" in msg(), n
        for n in (0, MAXN + 1):
            assert raw(e, sets, n_samples=n, draws=dr)[0] == UNSUPPORTED and "n_samples" in msg(), n
        assert raw(e, sets, n_samples=1, draws=dr)[0] == UNSUPPORTED and "n_quantiles" in msg()      # quantiles over one draw
        assert raw(e, sets[:1], ptr=[0, 1 << 31], nout=1)[0] == UNSUPPORTED and "2^31" in msg()
        assert raw(e, sets, n_samples=1, draws=dr, probs=())[0] == 0 and raw(e, sets, n_samples=3, draws=dr)[0] == 0      # one explicit draw is served
        rcode, res = raw(e, sets, n_sets=0, nout=2)                                      # nothing computed, nothing written
        assert rcode == 0 and all(np.all(v == -7) for v in res.values())
        assert raw(e, sets, n_sets=0, null=("set_ptr", "set_idx"))[0] == 0
        assert raw(e, sets, want=())[0] == 0                                             # an all-NULL out
        assert raw(e, sets, probs=(), top=())[0] == 0                                    # no quantiles, no lists
        full = rank(e, sets, 64, top=(1, 10))
        del full["set_ptr"]
        assert same_bytes(raw(e, sets)[1], full)
        for k in OUTS:                                                                   # every output NULL except one
            rcode, one = raw(e, sets, want=(k,))
            assert rcode == 0 and same_bytes(one, {k: full[k]}), k
        for bad, what in ((dict(n_samples=1), "n_samples"), (dict(draws=np.zeros((3, sp.D + 1))), "draws"), (dict(source="both"), "source"),
                          (dict(top=(0,)), "top")):
            try:
                e.fitness_rank(sets, **bad)
            except _capi.BarBayHipError as ex:
                assert what in str(ex)
            else:
                raise AssertionError("no error")
        try:
            e.fitness_rank((np.array([0, 5]), np.arange(3)))
        except _capi.BarBayHipError as ex:
            assert "ptr" in str(ex)
        else:
            raise AssertionError("no error")
