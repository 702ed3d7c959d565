"""Cases of the device-resident NUTS tree bb_nuts_begin / bb_nuts_start / bb_nuts_leaf / bb_nuts_take (barbay.jl_amd/csrc/bb_nuts.h) shared
by the emulation tests (CPU) and the GPU tests: each takes the loaded C-ABI library.  Shapes and points are those of `_logp_cases`.

The reference of a tree is a numpy restatement of the arithmetic include/barbay_hip.h states, with two roundings where the device fuses;
its momenta come from `Engine.normals` (the engine is created with the session's seed) and every gradient from
`Engine.logdensity_grad_batch` -- never from the code under test.  The rule that turns a leaf's number into its ops is restated here too."""
import copy
import ctypes

import numpy as np
import pytest

import _hmc_cases as hc
import _logp_cases as lc
import barbay_jl_amd as bb
from barbay_jl_amd import _capi
from conftest import make_engine

NAMES = lc.NAMES
same = lc.same
SEED, TRANS, STREAM0 = hc.SEED, hc.TRANS, hc.STREAM0
EPS3, EPS_SCALE, inv_mass = hc.EPS3, hc.EPS_SCALE, hc.inv_mass
DEPTH = 3
DIRS = (1, -1, 1)                    # three doublings: 1 + 2 + 4 leaves
OPP = _capi.BB_NUTS_EDGE_OPP
LEAF, SUB, STATE = _capi.BB_NUTS_TAKE_LEAF, _capi.BB_NUTS_TAKE_SUB, _capi.BB_NUTS_TAKE_STATE
# how the end of doubling j is taken into the session's state: the three copies one call each, two and one, all in one call
TAKES = {0: (LEAF, SUB, STATE), 1: (LEAF | SUB, STATE)}
KINDS = ("z", "logp_leaf", "kinetic", "a", "b")

# e_ref per shape as measured in the emulation (the largest deviation, over the three walkers and the seven leaves, between the fp64
# restatement and the one that carries z and r in np.longdouble; z in units of max |z| of the walker, logp_leaf and kinetic of their own
# value, a and b of sum |z - z_c| |inv_mass r|).  The bound of case_tree_against_host is 8 * e_ref, e_ref measured afresh in the test
# (these are a record, not an input.  The restatements run on the host but take their gradients from the library under test's
# evaluation service, which need not agree with the emulation's to the last bit: on the MI355X the figures differ in places, multienv's kinetic e_ref
# being 1.68e-16 there; the test measures its own):
E_REF_MEASURED = {          # z, logp_leaf, kinetic, a, b
    "fitness_T2":         (2.16e-16, 0.0, 2.10e-16, 1.39e-15, 1.40e-15),
    "fitness_multi_tile": (2.12e-16, 0.0, 1.63e-16, 3.01e-15, 3.17e-15),
    "multienv":           (2.96e-16, 0.0, 1.34e-16, 3.69e-15, 3.81e-15),
    "replicate_ragged":   (3.12e-16, 0.0, 2.34e-16, 2.91e-14, 2.91e-14),
    "multienv_replicate": (2.17e-16, 0.0, 1.97e-16, 3.21e-14, 3.20e-14),
    "genotype":           (2.06e-16, 0.0, 1.74e-16, 4.26e-14, 4.24e-14),
}                           # (logp_leaf: 0 -- both restatements' leaves round to points with the same log-joint, so the bound asks for equality, which
#                              holds; a, b: the differences z - z_c cancel all but the last few digits of z at these step sizes, so the rounding of z itself,
#                              2^-53 |z|, is 10 to 200 units of 2^-53 sum |z - z_c| |inv_mass r|; the device's own deviation from the fp64 restatement
#                              is 1.4e-16 .. 4.0e-16 in these units for a and b, 2.2e-16 .. 3.9e-16 for kinetic, 2.6e-17 .. 1.2e-16 for z)


def leaf_op(i, j):
    """include/barbay_hip.h's caller (mcmc.nuts_device) restated: leaf i of a doubling of 2^j leaves -> (store, checks)."""
    idx_max = bin(i >> 1).count("1")
    k = 0
    while (i >> k) & 1:
        k += 1
    store = idx_max if i % 2 == 0 else -1
    checks = [idx_max - q for q in range(k)] if i % 2 else []
    if i == 2 ** j - 1:
        checks.append(OPP)
    return store, checks


def case_leaf_op_lists():
    assert [leaf_op(i, 2) for i in range(4)] == [(0, []), (-1, [0]), (1, []), (-1, [1, 0, OPP])]
    assert leaf_op(0, 0) == (0, [OPP]) and leaf_op(1, 1) == (-1, [0, OPP]) and leaf_op(7, 3) == (-1, [2, 1, 0, OPP])
    assert leaf_op(5, 3) == (-1, [1]) and leaf_op(3, 3) == (-1, [1, 0]) and leaf_op(6, 3) == (2, []) and leaf_op(4, 3) == (1, [])


def restate(e, z, lp, g, n, eps, minv, dirs, T=np.float64):
    """One walker's scripted tree as include/barbay_hip.h states it; z and r carried in T, gradients from the service at the fp64-rounded
    point.  Per leaf the scalars (and the scale of each a, b), per doubling the position of its last leaf."""
    mi = minv.astype(T)
    r0 = n.astype(T) * (1.0 / np.sqrt(minv)).astype(T)
    k0 = T(0.5) * np.sum(mi * r0 * r0)
    edge = {-1: (z.astype(T), r0, g), 1: (z.astype(T), r0, g)}
    ck, leaves, ends = {}, [], []
    for j, v in enumerate(dirs):
        zc, r, gc = edge[v]
        half, em = T(0.5 * (v * eps)), ((v * eps) * minv).astype(T)            # (the products rounded once, in fp64)
        for i in range(2 ** j):
            r = r + half * gc.astype(T)
            zc = zc + em * r
            lpb, gb = e.logdensity_grad_batch(np.asarray(zc, dtype=np.float64))
            lpl, gc = lpb[0], gb[0]
            r = r + half * gc.astype(T)
            m = mi * r
            store, checks = leaf_op(i, j)
            leaf = {"logp_leaf": T(lpl), "kinetic": T(0.5) * np.sum(m * r), "a": [], "b": [], "sa": [], "sb": []}
            for c in checks:
                zs, rs = edge[-v][:2] if c == OPP else ck[c]
                d, ms = zc - zs, mi * rs
                leaf["a"].append(np.sum(d * ms)), leaf["b"].append(np.sum(d * m))
                leaf["sa"].append(float(np.sum(np.abs(d) * np.abs(ms)))), leaf["sb"].append(float(np.sum(np.abs(d) * np.abs(m))))
            if store >= 0:
                ck[store] = (zc, r)
            leaves.append(leaf)
        edge[v] = (zc, r, gc)
        ends.append(zc)
    return {"kinetic0": k0, "leaves": leaves, "ends": ends}


def run_plans(e, Z, eps, plans, minv, delays=None, trans=TRANS, between=None, depth=DEPTH, mid=None):
    """A session at Z with the tree's rows; walker w walks the doublings of plans[w] (a tuple of directions; None: not live) from round
    delays[w] on, one leaf per round, and at each doubling's end takes its last leaf all the way into the session's state.  Per walker
    {"kinetic0", "leaves": [the leaf's outputs], "ends": [(z, logp, grad) of the state after each doubling]}.  `between` is called before
    the start, `mid(rnd)` before the leaves of every round."""
    W = len(Z)
    delays = [0] * W if delays is None else delays
    out = [{"leaves": [], "ends": []} for _ in range(W)]
    with e.hmc_begin(Z, seed=SEED, inv_mass=minv):
        e.nuts_begin(depth)
        if between is not None:
            between()
        k0 = e.nuts_start(trans, eps, [p is not None for p in plans])
        pos = [[0, 0] for _ in range(W)]
        left = lambda w: plans[w] is not None and pos[w][0] < len(plans[w])
        rnd = 0
        while any(left(w) for w in range(W)):
            if mid is not None:
                mid(rnd)
            act = [w for w in range(W) if left(w) and rnd >= delays[w]]
            dirs, first, last = (np.zeros(W, dtype=np.int32) for _ in range(3))
            store, checks = np.full(W, -1, dtype=np.int32), [[] for _ in range(W)]
            for w in act:
                j, i = pos[w]
                dirs[w], first[w], last[w] = plans[w][j], i == 0, i == 2 ** j - 1
                store[w], checks[w] = leaf_op(i, j)
            r = e.nuts_leaf(dirs, first, last, store, checks)
            seqs = {}
            for w in act:
                nc = len(checks[w])
                out[w]["leaves"].append({"logp_leaf": r["logp_leaf"][w], "kinetic": r["kinetic"][w], "a": r["a"][w][:nc].copy(), "b": r["b"][w][:nc].copy()})
                assert not r["a"][w][nc:].any() and not r["b"][w][nc:].any()
                if last[w]:
                    seqs[w] = TAKES.get(pos[w][0], (LEAF | SUB | STATE,))
                    pos[w] = [pos[w][0] + 1, 0]
                else:
                    pos[w][1] += 1
            for w in set(range(W)) - set(act):
                assert r["logp_leaf"][w] == 0.0 and r["kinetic"][w] == 0.0 and not r["a"][w].any()
            for k in range(3):
                flags = np.array([seqs[w][k] if w in seqs and k < len(seqs[w]) else 0 for w in range(W)], dtype=np.int32)
                if flags.any():
                    e.nuts_take(flags)
            if seqs:
                z, lp, g = e.hmc_get(grad=True)
                for w in seqs:
                    out[w]["ends"].append((z[w].copy(), lp[w], g[w].copy()))
            rnd += 1
        for w in range(W):
            out[w]["kinetic0"] = k0[w]
    return out


def same_walker(a, b):
    ok = same(a["kinetic0"], b["kinetic0"]) and len(a["leaves"]) == len(b["leaves"]) and len(a["ends"]) == len(b["ends"])
    ok = ok and all(same(x[k], y[k]) for x, y in zip(a["leaves"], b["leaves"]) for k in ("logp_leaf", "kinetic", "a", "b"))
    return ok and all(same(p, q) for x, y in zip(a["ends"], b["ends"]) for p, q in zip(x, y))


def case_tree_against_host(lib, name):
    sp, Z, _ = lc.spec(name)
    D = sp.D
    nchunk = -(-D // _capi.BB_HMC_CHUNK)
    assert D < 4096 or (2 + 8 + 8 + nchunk) + (2 + 128 + int(np.ceil(np.log2(D)))) < 4096       # kinetic0: _hmc_cases' argument
    minv = inv_mass(D)
    eps = EPS3 * EPS_SCALE[name]
    with make_engine(sp, lib, seed=SEED) as e:
        lp0, g0 = e.logdensity_grad_batch(Z)
        nrm = [e.normals(TRANS, STREAM0 + w, 0, D) for w in range(3)]
        r64 = [restate(e, Z[w], lp0[w], g0[w], nrm[w], eps[w], minv, DIRS) for w in range(3)]
        rld = [restate(e, Z[w], lp0[w], g0[w], nrm[w], eps[w], minv, DIRS, np.longdouble) for w in range(3)]
        ld = np.longdouble

        def deviations(get, ref):
            """{kind: largest deviation of get(w)'s figures from ref[w]'s, in the kind's units}"""
            d = {k: 0.0 for k in KINDS}
            for w in range(3):
                x = get(w)
                zs = float(np.abs(r64[w]["ends"][-1]).max())
                for za, zb in zip(x["ends"], ref[w]["ends"]):
                    d["z"] = max(d["z"], float(np.abs(np.asarray(za, dtype=ld) - zb).max()) / zs)
                for la, lb, l64 in zip(x["leaves"], ref[w]["leaves"], r64[w]["leaves"]):
                    for k in ("logp_leaf", "kinetic"):
                        d[k] = max(d[k], float(abs(ld(la[k]) - lb[k])) / abs(float(l64[k])))
                    for k, sk in (("a", "sa"), ("b", "sb")):
                        for q in range(len(l64[k])):
                            d[k] = max(d[k], float(abs(ld(la[k][q]) - lb[k][q])) / l64[sk][q])
            return d
        e_ref = deviations(lambda w: r64[w], rld)
        print(name, "e_ref", {k: "%.3g" % v for k, v in e_ref.items()})

        dev = run_plans(e, Z, eps, [DIRS] * 3, minv)
        got = [{"ends": [x[0] for x in dev[w]["ends"]], "leaves": dev[w]["leaves"]} for w in range(3)]
        d = deviations(lambda w: got[w], r64)
        print(name, "dev  ", {k: "%.3g" % v for k, v in d.items()})
        for w in range(3):
            assert len(dev[w]["leaves"]) == 7 and len(dev[w]["ends"]) == 3
            assert [len(x["a"]) for x in dev[w]["leaves"]] == [1, 0, 2, 0, 1, 0, 3]
            rel = abs(dev[w]["kinetic0"] - r64[w]["kinetic0"]) / r64[w]["kinetic0"]
            print(name, w, "kinetic0 rel", rel)
            assert rel <= 4096 * 2.0 ** -53
        for k in KINDS:
            assert d[k] <= 8 * e_ref[k], (k, d[k], e_ref[k])
        # the same transition number: bb_hmc_step's kinetic0, bit for bit
        with e.hmc_begin(Z, seed=SEED, inv_mass=minv):
            assert same(e.hmc_step(TRANS, eps, 1, np.inf)["kinetic0"], [dev[w]["kinetic0"] for w in range(3)])
        # the state after a full take chain is a point with ITS log-density and gradient
        for k in range(3):
            zk = np.stack([dev[w]["ends"][k][0] for w in range(3)])
            lpc, gc = e.logdensity_grad_batch(zk)
            assert same(lpc, [dev[w]["ends"][k][1] for w in range(3)]) and same(gc, np.stack([dev[w]["ends"][k][2] for w in range(3)])), k
            assert same(lpc, [dev[w]["leaves"][(0, 2, 6)[k]]["logp_leaf"] for w in range(3)])
    return e_ref


def case_independence(lib, name):
    """The walker under test is (Z[0], eps 1e-3, the plan DIRS).  Its stream is BB_HMC_STREAM0 + its session index w, so w is held fixed
    in every comparison: the run it is compared with has w + 1 walkers, the slots below w padded with a dummy (Z[1], one leaf)."""
    sp, Z, _ = lc.spec(name)
    minv = inv_mass(sp.D)
    x_eps = 1e-3 * EPS_SCALE[name]
    g = np.random.default_rng(21)
    others = g.normal(0.0, 0.5, (4, sp.D))
    o_eps = np.array([3e-4, 2e-3, 7e-4, 1.5e-3]) * EPS_SCALE[name]
    o_plans, o_delays = [(-1, 1, -1), None, (1, 1), (-1, -1, -1)], [0, 0, 2, 1]      # other directions, idle, later: other check lists

    def padded(e, w):
        Zs = np.concatenate([np.repeat(Z[1][None], w, axis=0), Z[:1]])
        return run_plans(e, Zs, np.r_[np.full(w, 1e-4), x_eps], [(1,)] * w + [DIRS], minv)[w]

    with make_engine(sp, lib, seed=SEED) as e:
        alone = padded(e, 0)
        assert all(np.isfinite(x["logp_leaf"]) and np.isfinite(x["kinetic"]) for x in alone["leaves"])
        for slot in (0, 2, 4):                                                # first, middle and last slot of W = 5
            ins = lambda a, v: np.insert(a, slot, v, axis=0)
            plans, delays = list(o_plans), list(o_delays)
            plans.insert(slot, DIRS), delays.insert(slot, 0)
            run = run_plans(e, ins(others, Z[0]), ins(o_eps, x_eps), plans, minv, delays)
            assert same_walker(run[slot], padded(e, slot)), slot
        # a neighbour that diverges: reported in its own outputs, no error
        run = run_plans(e, Z[:2], [x_eps, 1e6], [DIRS, DIRS], minv)
        assert same_walker(run[0], alone)
        assert not np.isfinite(run[1]["leaves"][0]["logp_leaf"] - run[1]["leaves"][0]["kinetic"])
        # an interleaved batch call between begin and start
        run = run_plans(e, Z[:1], [x_eps], [DIRS], minv, between=lambda: e.logdensity_grad_batch(others))
        assert same_walker(run[0], alone)
        # ... and between two leaves of one doubling: rounds 3 .. 6 are the j = 2 doubling, the calls fall before its second, third and fourth leaf
        run = run_plans(e, Z[:1], [x_eps], [DIRS], minv, mid=lambda rnd: e.logdensity_grad_batch(others) if rnd in (4, 5, 6) else None)
        assert same_walker(run[0], alone)
    with make_engine(sp, lib, seed=SEED, launch_mode=1) as e:                 # two-kernel handle against the default mode
        assert same_walker(padded(e, 0), alone)


def case_full_width(lib, name="fitness_multi_tile"):
    """W = BB_HMC_MAX_WALKERS, two doublings in drawn directions: slots 0, 31 and 63 equal the runs that hold the same point at the same
    session index among dummies."""
    sp, Z, _ = lc.spec(name)
    W = _capi.BB_HMC_MAX_WALKERS
    minv = inv_mass(sp.D)
    g = np.random.default_rng(33)
    batch = g.normal(0.0, 0.4, (W, sp.D))
    eps = g.uniform(2e-4, 2e-3, W) * EPS_SCALE[name]
    plans = [tuple(int(v) for v in g.choice([-1, 1], 2)) for _ in range(W)]
    with make_engine(sp, lib, seed=SEED) as e:
        full = run_plans(e, batch, eps, plans, minv, depth=2)
        assert all(np.isfinite(x["kinetic"]) for r in full for x in r["leaves"])
        for w in (0, 31, 63):
            Zs = np.concatenate([np.repeat(Z[1][None], w, axis=0), batch[w:w + 1]])
            ref = run_plans(e, Zs, np.r_[np.full(w, 1e-4), eps[w]], [(1,)] * w + [plans[w]], minv, depth=2)
            assert same_walker(full[w], ref[w]), w


def case_state_untouched(lib, name):
    sp, Z, _ = lc.spec(name)
    minv = inv_mass(sp.D)
    eps = EPS3 * EPS_SCALE[name]
    with make_engine(sp, lib, seed=SEED) as e:
        mu0, om0 = e.get_params()
        before = e.logdensity_grad_batch(Z)
        with e.hmc_begin(Z, seed=SEED, inv_mass=minv):
            plain = e.hmc_step(3, eps, hc.L3, -0.5), e.hmc_get(grad=True)
        with e.hmc_begin(Z, seed=SEED, inv_mass=minv):
            e.nuts_begin(DEPTH)
            again = e.hmc_step(3, eps, hc.L3, -0.5), e.hmc_get(grad=True)     # a step after bb_nuts_begin: the step without it
            assert all(same(plain[0][k], again[0][k]) for k in hc.FIELDS) and all(same(x, y) for x, y in zip(plain[1], again[1]))
            k0 = e.nuts_start(4, eps)
            e.nuts_leaf(1, 1, 1, 0, [[OPP]] * 3)
            during = e.logdensity_grad_batch(Z)
            e.nuts_take(LEAF | SUB | STATE)
            probe = e.hmc_step(4, eps, 1, np.inf)                             # between two transitions: legal; the same momenta
            assert same(probe["kinetic0"], k0)
            e.nuts_start(5, eps)
            e.nuts_leaf(-1, 1, 1, 0, [[OPP]] * 3)
        after = e.logdensity_grad_batch(Z)
        for r in (during, after):
            assert same(r[0], before[0]) and same(r[1], before[1])
        mu1, om1 = e.get_params()
        assert same(mu0, mu1) and same(om0, om1)
        e.run(5)
        mu_a, om_a = e.get_params()
    with make_engine(sp, lib, seed=SEED) as e:
        e.run(5)
        mu_b, om_b = e.get_params()
    assert same(mu_a, mu_b) and same(om_a, om_b)


def case_errors(lib):
    sp, Z, _ = lc.spec("fitness_T2")
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    P = lambda a, t=dp: a.ctypes.data_as(t)
    err = lambda: lib.bb_last_error().decode()
    W, CS = 2, _capi.BB_NUTS_MAX_DEPTH + 1
    z = np.ascontiguousarray(Z[:W])
    eps, live, flags = np.full(W, 1e-3), np.ones(W, dtype=np.int32), np.zeros(W, dtype=np.int32)

    def nopts(depth=DEPTH, reserved=0):
        o = _capi.bb_nuts_opts()
        o.max_depth, o.reserved0 = depth, reserved
        return o

    def lopts(dir=(1, 1), first=(1, 1), last=(1, 1), store=(-1, -1), n_check=(0, 0), check=(), reserved=0):
        keep = [np.asarray(a, dtype=np.int32) for a in (dir, first, last, store, n_check)] + [np.zeros((W, CS), dtype=np.int32)]
        for w, j, c in check:
            keep[5][w, j] = c
        o = _capi.bb_nuts_leaf_opts()
        o.dir, o.first, o.last, o.store, o.n_check, o.check = (P(a, ip) for a in keep)
        o.reserved0 = reserved
        return o, keep

    def hopts():
        o = _capi.bb_hmc_opts()
        o.n_walkers, o.reserved0, o.seed = W, 0, SEED
        return o

    with make_engine(sp, lib, seed=SEED) as e:
        h = e._h
        begin = lambda o: lib.bb_nuts_begin(h, ctypes.byref(o) if o is not None else None)
        start = lambda ee=eps, lv=live: lib.bb_nuts_start(h, 1, P(ee), P(lv, ip), None)
        leaf = lambda ok: lib.bb_nuts_leaf(h, ctypes.byref(ok[0]), None)
        take = lambda f: lib.bb_nuts_take(h, P(np.asarray(f, dtype=np.int32), ip))
        good = lopts()
        # no session
        assert begin(nopts()) == -1 and "session" in err()
        assert start() == -1 and "session" in err() and leaf(good) == -1 and take(flags) == -1
        assert lib.bb_hmc_begin(h, ctypes.byref(hopts()), P(z), None) == 0
        # no bb_nuts_begin
        assert start() == -1 and "bb_nuts_begin" in err()
        assert leaf(good) == -1 and "bb_nuts_begin" in err() and take(flags) == -1 and "bb_nuts_begin" in err()
        # begin
        assert lib.bb_nuts_begin(None, ctypes.byref(nopts())) == -1 and begin(None) == -1
        assert begin(nopts(0)) == -1 and begin(nopts(_capi.BB_NUTS_MAX_DEPTH + 1)) == -1 and "max_depth" in err()
        assert begin(nopts(reserved=1)) == -1 and "reserved0" in err()
        assert start() == -1                                                  # a refused begin leaves no rows
        assert begin(nopts(_capi.BB_NUTS_MAX_DEPTH)) == 0 and begin(nopts()) == 0
        # a leaf or a take before a start
        assert leaf(good) == -1 and "bb_nuts_start" in err()
        assert take([LEAF, 0]) == -1 and "bb_nuts_start" in err()
        # start
        assert lib.bb_nuts_start(h, 1, None, P(live, ip), None) == -1 and lib.bb_nuts_start(h, 1, P(eps), None, None) == -1
        for bad in (0.0, -1e-3, np.inf, np.nan):
            assert start(np.array([1e-3, bad])) == -1 and "walker 1" in err(), bad
        assert start(np.array([1e-3, np.nan]), np.array([1, 0], dtype=np.int32)) == 0      # (the eps of a walker that is not live is not read)
        assert leaf(lopts(dir=(1, 1))) == -1 and "walker 1" in err()          # ... and that walker has no leaf
        assert leaf(lopts(dir=(1, 0))) == 0
        assert start() == 0
        # leaf
        assert lib.bb_nuts_leaf(h, None, None) == -1 and lib.bb_nuts_leaf(None, ctypes.byref(good[0]), None) == -1
        assert leaf(lopts(reserved=2)) == -1 and "reserved0" in err()
        assert leaf(lopts(dir=(1, 2))) == -1 and "walker 1" in err()
        assert leaf(lopts(first=(0, 1))) == -1 and "walker 0" in err() and "first" in err()
        for bad in (-2, DEPTH, 99):
            assert leaf(lopts(store=(-1, bad))) == -1 and "walker 1" in err() and "store" in err(), bad
        for bad in (-1, DEPTH + 2):
            assert leaf(lopts(n_check=(bad, 0))) == -1 and "walker 0" in err() and "n_check" in err(), bad
        for bad in (-1, -3, DEPTH, 1000):
            assert leaf(lopts(n_check=(0, 2), check=[(1, 1, bad)])) == -1 and "walker 1" in err() and "check[1]" in err(), bad
        assert leaf(lopts(store=(1, -1), n_check=(2, 0), check=[(0, 0, 0), (0, 1, 1)])) == -1 and "walker 0" in err() and "both" in err()
        assert take([SUB, 0]) == -1 and "walker 0" in err()                   # nothing to take yet
        assert take([0, STATE]) == -1 and "walker 1" in err()
        assert take([LEAF, 0]) == -1 and "walker 0" in err()
        assert take([8, 0]) == -1 and lib.bb_nuts_take(h, None) == -1
        assert leaf(lopts(store=(0, 1), n_check=(1, DEPTH + 1), check=[(0, 0, OPP), (1, 0, OPP), (1, 1, 0), (1, 2, 2), (1, 3, OPP)])) == 0
        assert lib.bb_nuts_leaf(h, ctypes.byref(good[0]), ctypes.byref(_capi.bb_nuts_leaf_out())) == 0      # every output may be NULL
        assert take([LEAF | SUB | STATE, LEAF]) == 0 and take([0, SUB | STATE]) == 0 and take(flags) == 0
        # a bb_hmc_step redraws the travelling rows: a start comes before the next leaf
        e._hmc_W = W
        e.hmc_step(2, eps, 1, np.inf)
        assert leaf(good) == -1 and "bb_nuts_start" in err()
        assert start() == 0 and leaf(good) == 0
        # bb_hmc_end and bb_hmc_begin drop the rows
        assert lib.bb_hmc_end(h) == 0
        assert start() == -1 and "session" in err()
        assert lib.bb_hmc_begin(h, ctypes.byref(hopts()), P(z), None) == 0
        assert start() == -1 and "bb_nuts_begin" in err()
        assert begin(nopts()) == 0 and start() == 0 and leaf(good) == 0
        assert lib.bb_hmc_end(h) == 0
    with make_engine(sp, lib, seed=SEED, world_size=2, rank=0) as e:
        assert lib.bb_nuts_begin(e._h, ctypes.byref(nopts())) == -4 and "sharded" in err()        # BB_ERR_UNSUPPORTED
        assert lib.bb_nuts_start(e._h, 1, P(eps), P(live, ip), None) == -4 and lib.bb_nuts_leaf(e._h, ctypes.byref(good[0]), None) == -4
        assert lib.bb_nuts_take(e._h, P(flags, ip)) == -4
        with pytest.raises(_capi.BarBayHipError, match="error -4"):
            e.nuts_begin(DEPTH)
    with make_engine(sp, lib, seed=SEED, device_ids=[0, 0], launch_mode=1) as e:                  # n_devices > 1
        assert lib.bb_nuts_begin(e._h, ctypes.byref(nopts())) == -4 and "multi-device handle" in err()
        assert lib.bb_nuts_start(e._h, 1, P(eps), P(live, ip), None) == -4 and "multi-device handle" in err()
        assert lib.bb_nuts_leaf(e._h, ctypes.byref(good[0]), None) == -4 and "multi-device handle" in err()
        assert lib.bb_nuts_take(e._h, P(flags, ip)) == -4 and "multi-device handle" in err()
        with pytest.raises(_capi.BarBayHipError, match="error -4: .*multi-device handle"):
            e.nuts_begin(DEPTH)


# ---- end to end: nuts_device through the library against the driver on a numpy stand-in, transition by transition --------------------
E2E = dict(W=4, max_depth=5, n_adapt=10, n_steps=10, advi_steps=200, seed=3)
MARGIN = 1e-9


class StandIn:
    """`Engine`'s session and tree calls in numpy for ONE transition from a given state: the header's arithmetic with z and r carried
    in T, momenta from `Engine.normals`, gradients from `Engine.logdensity_grad_batch`.  The step size and the transition's number are
    the recorded ones, whatever the driver's probes arrive at.  Records how close every decision came to its threshold."""

    def __init__(self, e, z, lp, g, eps, m, minv, logu_of, T=np.float64):
        self.e, self.T, self.m, self.eps, self.minv = e, T, m, np.asarray(eps), minv
        self.z, self.lp, self.g = np.array(z, dtype=T), np.array(lp), np.array(g)
        self.margin, self.logu_of = np.inf, logu_of

    def hmc_begin(self, z0, *, seed=0, inv_mass=None):
        return hc_session(self.lp.copy())

    def hmc_step(self, transition, eps, n_leapfrog, log_u):                  # (a probe: the first one settles the search)
        W = len(self.z)
        return {"h0": np.zeros(W), "h1": np.full(W, np.log(0.5))}

    def nuts_begin(self, max_depth):
        self.depth = max_depth

    def nuts_start(self, transition, eps, live=1):
        T, W, D = self.T, len(self.z), self.z.shape[1]
        mi = self.minv.astype(T)
        isd = (1.0 / np.sqrt(self.minv)).astype(T)
        self.r0 = np.stack([self.e.normals(self.m, STREAM0 + w, 0, D).astype(T) * isd for w in range(W)])
        self.edge = {v: [self.z.copy(), self.r0.copy(), self.g.copy()] for v in (-1, 1)}
        self.trav = [self.z.copy(), self.r0.copy(), self.g.copy()]
        self.ck = [[None] * self.depth for _ in range(W)]
        self.sub, self.cand, self.lp_leaf, self.lp_sub, self.lp_cand = [None] * W, [None] * W, np.zeros(W), np.zeros(W), np.zeros(W)
        self.k0 = np.array([float(T(0.5) * np.sum(mi * r * r)) for r in self.r0])
        return self.k0.copy()

    def nuts_leaf(self, dirs, first, last, store, checks):
        with np.errstate(over="ignore", invalid="ignore"):                    # (a warm-up step size may diverge: that is a leaf's h1 = -inf)
            return self._leaf(dirs, first, last, store, checks)

    def _leaf(self, dirs, first, last, store, checks):
        T, W = self.T, len(self.z)
        mi = self.minv.astype(T)
        act = [w for w in range(W) if dirs[w]]
        for w in act:
            v = int(dirs[w])
            if first[w]:
                for q in range(3):
                    self.trav[q][w] = self.edge[v][q][w]
            e = v * float(self.eps[w])
            self.trav[1][w] = self.trav[1][w] + T(0.5 * e) * self.trav[2][w].astype(T)
            self.trav[0][w] = self.trav[0][w] + (e * self.minv).astype(T) * self.trav[1][w]
        lpb, gb = self.e.logdensity_grad_batch(np.asarray(self.trav[0][act], dtype=np.float64))
        out = {"logp_leaf": np.zeros(W), "kinetic": np.zeros(W), "a": np.zeros((W, self.depth + 1)), "b": np.zeros((W, self.depth + 1))}
        for q, w in enumerate(act):
            v = int(dirs[w])
            self.trav[2][w] = gb[q]
            self.trav[1][w] = self.trav[1][w] + T(0.5 * v * float(self.eps[w])) * gb[q].astype(T)
            z, r = self.trav[0][w], self.trav[1][w]
            m = mi * r
            kin = T(0.5) * np.sum(m * r)
            out["logp_leaf"][w], out["kinetic"][w], self.lp_leaf[w] = lpb[q], float(kin), lpb[q]
            h1 = float(lpb[q]) - float(kin)
            logu = self.logu_of(w)
            if np.isfinite(h1):                                               # the slice and the divergence test
                self.margin = min(self.margin, abs(logu - h1) / max(abs(h1), 1.0), abs(logu - 1000.0 - h1) / max(abs(h1), 1000.0))
            for k, c in enumerate(checks[w]):
                zs, rs = (self.edge[-v][0][w], self.edge[-v][1][w]) if c == OPP else self.ck[w][c]
                d, ms = z - zs, mi * rs
                a, b = np.sum(d * ms), np.sum(d * m)
                out["a"][w][k], out["b"][w][k] = float(a), float(b)
                if np.isfinite(h1):
                    self.margin = min(self.margin, float(abs(a) / np.sum(np.abs(d) * np.abs(ms))), float(abs(b) / np.sum(np.abs(d) * np.abs(m))))
            if store[w] >= 0:
                self.ck[w][store[w]] = (z.copy(), r.copy())
            if last[w]:
                for q3 in range(3):
                    self.edge[v][q3][w] = self.trav[q3][w]
        return out

    def nuts_take(self, flags):
        for w, f in enumerate(np.broadcast_to(flags, (len(self.z),))):
            if f & LEAF:
                self.sub[w], self.lp_sub[w] = (self.trav[0][w].copy(), self.trav[2][w].copy()), self.lp_leaf[w]
            if f & SUB:
                self.cand[w], self.lp_cand[w] = self.sub[w], self.lp_sub[w]
            if f & STATE:
                self.z[w], self.g[w], self.lp[w] = self.cand[w][0], self.cand[w][1], self.lp_cand[w]

    def hmc_get(self, grad=False):
        return np.asarray(self.z, dtype=np.float64), self.lp.copy()

    def hmc_end(self):
        pass


class hc_session:
    def __init__(self, logp):
        self.logp = logp


class Recorder:
    """Passes every call through to the engine; at each bb_nuts_start it downloads the state the transition starts from and copies the
    walkers' generators as they stand."""

    def __init__(self, e, rngs):
        self.e, self.rngs, self.starts = e, rngs, []

    def __getattr__(self, k):
        return getattr(self.e, k)

    def nuts_start(self, transition, eps, live=1):
        z, lp, g = self.e.hmc_get(grad=True)
        self.starts.append({"m": transition, "eps": np.array(eps), "z": z, "lp": lp, "g": g, "rngs": copy.deepcopy(self.rngs)})
        return self.e.nuts_start(transition, eps, live)


def case_end_to_end(lib):
    """data001_single (D = 103), W = 4, depth 5, 10 warm-up + 10 kept transitions through the library.  Every transition is run again
    from the device's downloaded state by the same driver on `StandIn`, in fp64 and with z, r in np.longdouble: depth, number of leaves,
    chosen leaf and divergence flag agree, the new z agrees within 8 x (the deviation between the two stand-ins in that transition), and
    no decision of the stand-in lies within 1e-9 (relative) of its threshold."""
    df = lc.load("data001_single")
    arr = bb.utils.data_to_arrays(df)
    model = bb.model.fitness_normal(arr.bc_count, arr.bc_total, arr.n_neutral, arr.n_bc)
    W, seed, depth = E2E["W"], E2E["seed"], E2E["max_depth"]
    with bb.vi.make_engine(model, bb.vi.ADVI(1, E2E["advi_steps"]), bb.vi.TruncatedADAGrad(), seed, 0, _lib=lib) as e:
        e.run(E2E["advi_steps"])
        mean, sigma = e.posterior()
        minv = sigma ** 2
        D = mean.shape[0]
        assert D == 103
        rngs = [np.random.default_rng([seed, w]) for w in range(W)]
        z0s = [mean + np.sqrt(minv) * r.standard_normal(D) * 0.1 for r in rngs]
        rec, trace = Recorder(e, rngs), []
        res = bb.mcmc.nuts_device(rec, z0s, E2E["n_steps"], E2E["n_adapt"], rngs=rngs, minv=minv, max_depth=depth, seed=seed, trace=trace)
        total = E2E["n_steps"] + E2E["n_adapt"]
        assert len(trace) == len(rec.starts) == total and all(r[0].shape == (E2E["n_steps"], D) and np.isfinite(r[1]).all() for r in res)
        nxt = [s["z"] for s in rec.starts[1:]] + [np.stack([r[0][-1] for r in res])]
        worst, margin = 0.0, np.inf
        for t, st in enumerate(rec.starts):
            runs = []
            for T in (np.float64, np.longdouble):
                tr = []
                logu = {}
                s = StandIn(e, st["z"], st["lp"], st["g"], st["eps"], st["m"], minv, lambda w: trace[t]["walkers"][w]["logu"], T)
                bb.mcmc.nuts_device(s, list(st["z"]), 1, 0, rngs=copy.deepcopy(st["rngs"]), minv=minv, max_depth=depth, seed=seed, trace=tr)
                runs.append((s, tr[0]["walkers"]))
            (s64, w64), (sld, wld) = runs
            margin = min(margin, s64.margin)
            for w in range(W):
                a, b = trace[t]["walkers"][w], w64[w]
                for k in ("depth", "leaves", "chosen", "divergent", "stop", "valid", "dirs"):
                    assert a[k] == b[k] == wld[w][k], (t, w, k, a[k], b[k], wld[w][k])
                assert a["logu"] == b["logu"] or abs(a["logu"] - b["logu"]) <= 1e-9 * abs(a["logu"])
                scale = float(np.abs(s64.z[w]).max())
                e_ref = float(np.abs(s64.z[w].astype(np.longdouble) - sld.z[w]).max()) / scale
                dev = float(np.abs(nxt[t][w] - s64.z[w]).max()) / scale
                worst = max(worst, dev / e_ref if e_ref > 0 else (0.0 if dev == 0 else np.inf))
                assert dev <= 8 * e_ref, (t, w, dev, e_ref)
        print("end to end: worst deviation / e_ref", worst, "smallest decision margin", margin, "depths",
              [[x["walkers"][w]["depth"] for x in trace] for w in range(W)])
        assert margin > MARGIN
        assert all(0 < r[2]["mean_tree_depth"] <= depth and r[2]["n_grad"] > total and 0.0 <= r[2]["accept_rate"] <= 1.0 for r in res)


def case_sampler(lib, monkeypatch):
    """mcmc_sample(sampler="nuts", ensemble="device"): the output's keys; segments=2, keep_chain=False returns stream_* and downloads no
    position."""
    df = lc.load("data001_single")
    kw = dict(data=df, model=bb.model.fitness_normal, engine_kwargs={"_lib": lib}, sampler="nuts", ensemble="device", n_walkers=3, n_steps=8,
              n_adapt=6, advi_steps=200, outputname=None, verbose=False, seed=3)
    out = bb.mcmc.mcmc_sample(nuts_kwargs=dict(max_depth=4), **kw)
    assert out["chain"].shape == (3, 8, 103) and np.isfinite(out["logp"]).all()
    for k in ("accept_rate", "divergences", "n_grad", "mean_tree_depth", "step_size"):
        assert out[k].shape == (3,), k
    assert (out["mean_tree_depth"] <= 4).all() and (out["mean_tree_depth"] > 0).all()
    gets = []
    orig = _capi.Engine.hmc_get
    monkeypatch.setattr(_capi.Engine, "hmc_get", lambda self, grad=False: gets.append(1) or orig(self, grad))
    lean = bb.mcmc.mcmc_sample(nuts_kwargs=dict(max_depth=4, segments=2, keep_chain=False), **kw)
    assert not gets and lean["chain"].shape == (3, 0, 103) and lean["stream_mean"].shape == (103,) and int(lean["stream_n"]) == 24
    assert np.isfinite(lean["stream_mean"]).all() and np.isfinite(lean["stream_sd"]).all()


# ---- mcmc_sample(sampler="nuts", ensemble="device") on every model kind ----------------------------------------------------------------
def _envs(df):
    """data002_hier-rep with an environment per time point (the first two in A, then alternating): a multienv_replicate data set."""
    t = np.sort(df["time"].unique())
    env = {v: ("A" if k < 2 or k % 2 == 0 else "B") for k, v in enumerate(t)}
    return df.assign(env=df["time"].map(env))


SAMPLER_KINDS = {      # model constructor, data set, its columns, D
    "fitness": ("fitness_normal", "data001_single", {}, None),
    "replicate": ("replicate_fitness_normal", "data002_hier-rep", dict(rep_col="rep"), None),
    "multienv": ("multienv_fitness_normal", "data003_multienv", dict(env_col="env"), None),
    "genotype": ("genotype_fitness_normal", "data004_multigen", dict(genotype_col="genotype"), None),
    "multienv_replicate": ("multienv_replicate_fitness_normal", "data002_hier-rep", dict(rep_col="rep", env_col="env"), _envs),
}


def case_sampler_kind(lib, kind):
    """A chain and its diagnostics for the model kind: 2 walkers, 6 warm-up + 4 kept transitions, depth <= 3."""
    model, data, cols, prep = SAMPLER_KINDS[kind]
    df = lc.load(data)
    if prep is not None:
        df = prep(df)
    out = bb.mcmc.mcmc_sample(data=df, model=getattr(bb.model, model), n_walkers=2, n_steps=4, n_adapt=6, advi_steps=100, outputname=None,
                              verbose=False, seed=3, engine_kwargs={"_lib": lib}, sampler="nuts", ensemble="device",
                              nuts_kwargs=dict(max_depth=3), **cols)
    D = len(out["var_names"])
    assert out["chain"].shape == (2, 4, D) and D > 100 and np.isfinite(out["chain"]).all() and np.isfinite(out["logp"]).all()
    for k in ("accept_rate", "divergences", "n_grad", "mean_tree_depth", "step_size"):
        assert out[k].shape == (2,) and np.isfinite(out[k]).all(), k
    assert (out["mean_tree_depth"] >= 1).all() and (out["mean_tree_depth"] <= 3).all() and (out["n_grad"] >= 10).all()
    assert (out["step_size"] > 0).all() and (out["accept_rate"] >= 0).all() and (out["accept_rate"] <= 1).all()
    print(kind, "D", D, "depth", out["mean_tree_depth"], "step", out["step_size"], "divergences", out["divergences"])
