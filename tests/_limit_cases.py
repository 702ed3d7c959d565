"""The edges of the shape range, shared by the emulation tests (CPU, tests/test_emu_limits.py) and the GPU tests
(tests/test_gpu_limits.py).

A. STEP: every step path at the top of the resident range -- 2 <= T_r <= 16, sum T_r <= 64, up to 16 replicates (br_eligible) -- where
   k_res works a barcode on LPB = ceil(T / 2) = 5 .. 8 lanes, and one past it; against the literal oracle's ADVI loop.
B. BOUNDARY: the largest uniform T bb_create accepts per (kind, R, E), and the refusal one past it.
C. HIER: bb_hier_fitness on every unit, at the ends of n_samples.

All problems come from oracle.fixtures.synthetic; geometries are forced through BB_TUNE_NB / BB_TUNE_NTHR / BB_TUNE_AP, which
bb_create reads."""
import re
import time

import numpy as np

import _cases
import _freq_cases
import _ppc_cases
import barbay_jl_amd as bb
from conftest import make_engine
from oracle import fixtures, rng

UNSUPPORTED = -4
TOL = 1e-10          # the project's bound on a trajectory against the oracle loop (_cases.case_trajectory_exact)
TOL_MODES = 1e-11    # launch_mode 2 against launch_mode 1 (_cases.case_persistent_equals_two_kernel)
TOL_TRACE = 1e-10    # the ELBO trace, relative (test_streaming_resident_launch_several_samples_and_elbo_trace)

TWO_KERNEL = {"emu": "emu:k_sample + k_update", "hip": "k_sample<{k}> + k_update<{k}>"}


# ------------------------------------------------------------------------------------------------
# A. the step kernels
# ------------------------------------------------------------------------------------------------
def _res(kind, P, nthr, ap=False):
    """The two spellings of a k_res instance with a run-time T, by sample count: S = 1 the plain form, S = 2 with the trace the MS
    form.  The emulation prints the launch's thread count and '*' for the run-time T; the product names the instance -- compiled for
    256, 512 or 1024 threads, T = 0."""
    inst = 256 if nthr <= 256 else (512 if nthr <= 512 else 1024)
    a = "true" if ap else "false"
    return {S: {"emu": f"emu:k_res<{kind},{P},{nthr},false,*,{a},{ms}>", "hip": f"k_res<{kind},{P},{inst},false,0,{a},{ms}>", "impl": {"emu": 2, "hip": 2}}
            for S, ms in ((1, "false"), (2, "true"))}


def _persist_then_two_kernel(kind, P, nthr, fits_lds=True):
    """No k_res plan: k_persist for one sample per step; several samples / the ELBO trace have only the two-kernel step (launch_mode
    0: launch_mode 2 is refused there, 'no owner-computes instance').  fits_lds = False: the tile with k_persist's lambda table does
    not fit the 160 KiB of a compute unit, so the product runs the two-kernel step for one sample too (launch_mode 0) -- the
    emulation, which has no compute unit to fit, still steps k_persist there (PERSIST_LDS_CAP, bb_backend.h)."""
    inst = 512 if nthr <= 512 else 1024
    two = {"emu": TWO_KERNEL["emu"], "hip": TWO_KERNEL["hip"].format(k=kind), "impl": {"emu": 0, "hip": 0}, "mode": 0}
    one = {"emu": f"emu:k_persist<{kind},{P},{nthr}>", "hip": f"k_persist<{kind},{P},{inst}>", "impl": {"emu": 1, "hip": 1}}
    if not fits_lds:
        one.update(hip=two["hip"], impl={"emu": 1, "hip": 0}, mode=0)
    return {1: one, 2: two}


def _geom(nb=None, nthr=None, ap=False):
    env = {}
    if nb:
        env["BB_TUNE_NB"] = str(nb)
    if nthr:
        env["BB_TUNE_NTHR"] = str(nthr)
    if ap:
        env["BB_TUNE_AP"] = "1"
    return env


def _case(kind, kw, env, names):
    return dict(kind=kind, kw=kw, env=env, names=names)


STEP = {}
# 1. plain k_res, LPB 5 .. 8: the default geometry (three tiles of 32 barcodes, one pair slot) and tiles of 16 barcodes on 128
#    threads (five tiles; two pair slots from T = 14)
for _T, _nthr, _P in ((10, 256, 1), (12, 256, 1), (14, 512, 2), (16, 512, 2)):
    _kw = dict(B=70, T=_T, n_neutral=9)
    STEP[f"fitness_T{_T}"] = _case("fitness", _kw, {}, _res(0, 1, _nthr))
    STEP[f"fitness_T{_T}_tiles"] = _case("fitness", _kw, _geom(16, 128), _res(0, _P, 128))
# 2. the any-parity instances, odd T: a barcode's last lane owns a single latent
for _T, _nthr, _P in ((9, 256, 1), (11, 256, 1), (13, 512, 2), (15, 512, 2)):
    _kw = dict(B=70, T=_T, n_neutral=9)
    STEP[f"fitness_T{_T}_ap"] = _case("fitness", _kw, _geom(ap=True), _res(0, 1, _nthr, ap=True))
    STEP[f"fitness_T{_T}_ap_tiles"] = _case("fitness", _kw, _geom(16, 128, ap=True), _res(0, _P, 128, ap=True))
STEP["genotype_T13"] = _case("genotype", dict(B=80, T=13, n_geno=9, n_neutral=10, geno_runs=True), {}, _res(2, 1, 512, ap=True))
# 3. the other kinds at T = 16: every time point an environment of its own; genotypes of many mutants and of about one
STEP["multienv_T16_E16"] = _case("multienv", dict(B=40, T=16, n_env=16, n_neutral=5), _geom(8, 256), _res(1, 1, 256))
#    ... and a short last tile under two pair slots: 40 barcodes in tiles of 32, four environments -- 8 barcodes in the second tile
STEP["multienv_T16_short_tile"] = _case("multienv", dict(B=40, T=16, n_env=4, n_neutral=5), _geom(32, 256), _res(1, 2, 256))
STEP["genotype_T16"] = _case("genotype", dict(B=80, T=16, n_geno=9, n_neutral=10, geno_runs=True), _geom(24, 256), _res(2, 2, 256))
STEP["genotype_T14_singletons"] = _case("genotype", dict(B=80, T=14, n_geno=70, n_neutral=10, geno_runs=True), {}, _res(2, 1, 512))
# 4. the hierarchical kinds at sum T = 64 and at 16 replicates; 1024 threads, so that the moment row K + 2 nt1 fits (first_hop_groups).
#    36 mutants: loglambda starts at an even flat index, the plain instances; 35 with BB_TUNE_AP: the any-parity ones (without
#    BB_TUNE_AP the plan is k_persist for one sample per step and an AP k_res only for several).
#    FINDING: within br_eligible, yet no k_res plan at the default tile of 32 barcodes -- the resident tile's LDS (br_layout) passes
#    160 KiB: 16 x T4 needs 194 560 B at 16 or 32 barcodes and 169 984 B at 8, the ragged shape 182 176 B at 32.  Such handles
#    run k_persist (one sample per step; on the device not even that: its tile does not fit LDS either) or the two-kernel step; k_res
#    takes them at tiles of 6 and of 16 barcodes, forced here -- 16 x T4 on 512 threads with three pair slots (the moment row's 402
#    entries fit; the product has no replicate instance of two slots on 1024 threads).
#    (Five replicates put 16 n_bc latents in front of loglambda, even whatever n_bc: the ragged shape's any-parity form has odd T_r.)
for _nm, _T, _Tap, _R, _nb, _nthr, _P in (("4xT16", 16, 16, 4, None, 1024, 1), ("16xT4", 4, 4, 16, 6, 512, 3),
                                          ("ragged_64", [16, 2, 12, 10, 14], [16, 3, 15, 14, 16], 5, 16, 1024, 1)):
    STEP[f"replicate_{_nm}"] = _case("replicate", dict(B=40, T=_T, n_rep=_R, n_neutral=4), _geom(_nb, _nthr), _res(3, _P, _nthr))
    STEP[f"replicate_{_nm}_ap"] = _case("replicate", dict(B=40, T=_Tap, n_rep=_R, n_neutral=5), _geom(_nb, _nthr, ap=True), _res(3, _P, _nthr, ap=True))
STEP["multienv_replicate_8xT8"] = _case("multienv_replicate", dict(B=30, T=8, n_rep=8, n_env=4, n_neutral=4), _geom(nthr=1024), _res(4, 1, 1024))
STEP["multienv_replicate_4xT16"] = _case("multienv_replicate", dict(B=30, T=16, n_rep=4, n_env=3, n_neutral=4), _geom(nthr=1024), _res(4, 1, 1024))
# ... and at their default geometry, on the path they do get (the finding above)
STEP["replicate_16xT4_default"] = _case("replicate", dict(B=40, T=4, n_rep=16, n_neutral=4), _geom(nthr=1024), _persist_then_two_kernel(3, 1, 1024, fits_lds=False))
STEP["replicate_ragged_64_default"] = _case("replicate", dict(B=40, T=[16, 2, 12, 10, 14], n_rep=5, n_neutral=4), _geom(nthr=1024), _persist_then_two_kernel(3, 2, 1024, fits_lds=False))
# 5. one past the edge: T = 17 and 18, sum T = 66
STEP["fitness_T17"] = _case("fitness", dict(B=70, T=17, n_neutral=9), {}, _persist_then_two_kernel(0, 1, 512))
STEP["fitness_T18"] = _case("fitness", dict(B=70, T=18, n_neutral=9), {}, _persist_then_two_kernel(0, 1, 512))
STEP["replicate_ragged_66"] = _case("replicate", dict(B=40, T=[16, 16, 16, 16, 2], n_rep=5, n_neutral=5), _geom(nthr=1024), _persist_then_two_kernel(3, 1, 1024, fits_lds=False))
K_RES = [n for n, c in STEP.items() if c["names"][1]["impl"]["hip"] == 2]
RESIDENT = [n for n, c in STEP.items() if c["names"][1]["impl"]["hip"] != 0]          # one sample per step is a resident launch: k_res or k_persist


def step_spec(name):
    c = STEP[name]
    return fixtures.synthetic(c["kind"], seed=2, **c["kw"])


def setenv(monkeypatch, name):
    for k in ("BB_TUNE_NB", "BB_TUNE_NTHR", "BB_TUNE_AP"):
        monkeypatch.delenv(k, raising=False)
    for k, v in STEP[name]["env"].items():
        monkeypatch.setenv(k, v)


def measure_step(lib, name, S):
    """One trajectory of a STEP case against the literal oracle's loop (the geometry is the caller's to force: setenv).  S = 1:
    TruncatedADAGrad, 12 steps; S = 2: DecayedADAGrad with the ELBO of every step, 8 steps.  Exact window in both.  Returns what the
    launch was and how far it is from the oracle."""
    sp = step_spec(name)
    mode = STEP[name]["names"][S].get("mode", 2)
    t0 = time.perf_counter()
    if S == 1:
        e, a, b, _ = _cases._trajectory(lib, sp, 12, 1, "TruncatedADAGrad", window=5, resum_every=1, launch_mode=mode)
        tr_err = 0.0
    else:
        e, a, b, tr = _cases._trajectory(lib, sp, 8, 2, "DecayedADAGrad", window=5, resum_every=1, elbo_every=1, launch_mode=mode)
        tr_err = float(np.abs(e.elbo_trace(0, 8) - tr).max() / np.abs(tr).max())
    st, nm = e.stats(), e.kernel_name()
    e.close()
    return dict(case=name, S=S, launch_mode=mode, kernel=nm, impl=st["resident_kernel"], n_blocks=st["n_blocks"], threads=st["block_threads"],
                dmu=float(a), domega=float(b), trace=tr_err, seconds=time.perf_counter() - t0)


def case_step(lib, monkeypatch, name, S, spelling):
    """spelling: 'emu' or 'hip' -- which column of the table of names the library's word is held to."""
    setenv(monkeypatch, name)
    want = STEP[name]["names"][S]
    r = measure_step(lib, name, S)
    print(r)
    assert r["kernel"] == want[spelling], (r["kernel"], want[spelling])
    assert r["impl"] == want["impl"][spelling], r
    assert r["dmu"] < TOL and r["domega"] < TOL, r
    assert r["trace"] <= TOL_TRACE, r


def case_step_modes(lib, monkeypatch, name, spelling):
    """The resident launch of a RESIDENT case against the two-kernel step on the same problem: 7 + 10 steps, as
    _cases.case_persistent_equals_two_kernel."""
    setenv(monkeypatch, name)
    sp = step_spec(name)
    outs = []
    for mode in (1, 2):
        with make_engine(sp, lib, seed=13, window=6, resum_every=1, launch_mode=mode) as e:
            e.run(7)
            e.run(10)
            outs.append(e.get_params())
            assert e.stats()["steps_done"] == 17
            assert e.stats()["resident_kernel"] == (0 if mode == 1 else STEP[name]["names"][1]["impl"][spelling]), e.stats()
    a, b = np.abs(outs[0][0] - outs[1][0]).max(), np.abs(outs[0][1] - outs[1][1]).max()
    print(f"{name}: launch_mode 2 against 1: |dmu| {a:.3e} |domega| {b:.3e}")
    assert a < TOL_MODES and b < TOL_MODES, (a, b)


# ------------------------------------------------------------------------------------------------
# B. the create boundary
# ------------------------------------------------------------------------------------------------
# (kind, n_rep, n_env) -> the largest uniform T bb_create accepts, on 10 barcodes of which 3 neutral.  The two-kernel step's tile of 8
# barcodes (pick_geometry halves the tile down to 8) must fit 160 KiB of LDS with bb_lds_layout's tables, whose `red` part grows as
# 16 K + 8 BB_NQ Ttot.  The host code decides it: the same in the emulation and on the device.
BOUNDARY = {
    ("fitness", 1, 1): 96,
    ("genotype", 1, 1): 96,
    ("multienv", 1, 4): 95,
    ("replicate", 2, 1): 47,
    ("replicate", 4, 1): 22,
    ("replicate", 8, 1): 9,
    ("replicate", 16, 1): 5,
    ("multienv_replicate", 16, 2): 4,
    ("multienv_replicate", 16, 6): 4,
    ("multienv_replicate", 4, 4): 20,
}


def boundary_spec(kind, R, E, T):
    kw = dict(B=10, T=T, n_neutral=3)
    if kind in ("replicate", "multienv_replicate"):
        kw["n_rep"] = R
    if kind in ("multienv", "multienv_replicate"):
        kw["n_env"] = E
    if kind == "genotype":
        kw["n_geno"] = 3
    return fixtures.synthetic(kind, seed=7, **kw)


def try_create(lib, sp, **kw):
    """(0, '') where bb_create accepts the problem, else (code, message)."""
    try:
        make_engine(sp, lib, **kw).close()
    except bb.BarBayHipError as e:
        m = re.match(r"barbay_hip error (-?\d+): (.*)$", str(e), re.S)
        return int(m.group(1)), m.group(2)
    return 0, ""


def largest_T(lib, kind, R, E):
    """The largest uniform T in 2 .. 255 that bb_create accepts, by bisection (acceptance is monotone in T: the layout only grows)."""
    lo, hi = 2, 256
    assert try_create(lib, boundary_spec(kind, R, E, lo))[0] == 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if try_create(lib, boundary_spec(kind, R, E, mid))[0] == 0:
            lo = mid
        else:
            hi = mid
    return lo


def edge_rows(sp):
    """The first and the last row of the first and the last replicate: of bb_ppc_bands (a replicate's population-mean row, its last
    mutant's row) and of bb_freq_bands (its first and last data column)."""
    R, nb, B = sp.n_rep, sp.n_bc, sp.B
    reps = sorted({0, R - 1})
    return ([x for r in reps for x in (r, R + r * nb + nb - 1)], [x for r in reps for x in (r * B, r * B + B - 1)])


def case_boundary_accepted(lib, key):
    """The last accepted shape is a working handle: created at launch_mode 0 and 1, five steps of two samples with the ELBO trace
    against the oracle loop on both, the predictive bands against their restatements."""
    kind, R, E = key
    sp = boundary_spec(kind, R, E, BOUNDARY[key])
    for mode in (0, 1):
        e, a, b, tr = _cases._trajectory(lib, sp, 5, 2, "DecayedADAGrad", window=5, resum_every=1, elbo_every=1, launch_mode=mode)
        with e:
            err = float(np.abs(e.elbo_trace(0, 5) - tr).max() / np.abs(tr).max())
            print(f"{key} T = {BOUNDARY[key]} launch_mode {mode}: {e.kernel_name()}: |dmu| {a:.3e} |domega| {b:.3e} trace {err:.3e}")
            assert a < TOL and b < TOL, (a, b)
            assert err <= TOL_TRACE, err
            if mode == 1:
                continue
            mu, om = _freq_cases.tame(e)
            prow, frow = edge_rows(sp)
            qs = _freq_cases.QS
            bands, nout = e.ppc_bands(qs, n_samples=33, n_ppc=3, seed=11)
            b2, n2 = _ppc_cases.restate(sp, mu, om, qs, 33, 3, 11, rows=prow)
            _ppc_cases.assert_bands_close(bands[prow], b2)
            assert np.array_equal(nout[prow], n2)
            bands, nout = e.freq_bands(qs, mode="trajectory", n_samples=33, n_ppc=2, seed=11)
            b2, n2 = _freq_cases.restate(sp, mu, om, qs, "trajectory", 33, 2, 11, rows=frow)
            _freq_cases.assert_bands_close(bands[frow], b2)
            assert np.array_equal(nout[frow], n2)


def case_boundary_refused(lib, key):
    """One more time point: refused, in bb_create, as a shape this build cannot hold."""
    kind, R, E = key
    sp = boundary_spec(kind, R, E, BOUNDARY[key] + 1)
    for mode in (0, 1):
        code, msg = try_create(lib, sp, launch_mode=mode)
        print(f"{key} T = {BOUNDARY[key] + 1} launch_mode {mode}: {code}: {msg}")
        assert code == UNSUPPORTED, (code, msg)
        assert re.search(r"^a tile of 8 barcodes needs \d+ bytes of LDS / \d+ threads \(n_time or n_rep too large for this build\)$", msg), msg
        need = int(re.search(r"needs (\d+) bytes", msg).group(1))
        assert need > 160 * 1024, msg


# ------------------------------------------------------------------------------------------------
# C. bb_hier_fitness
# ------------------------------------------------------------------------------------------------
HIER = {
    "grid_stride": ("replicate", dict(B=1100, T=[2, 3], n_rep=2, n_neutral=10)),              # 2180 units: more than the 2048 blocks of a launch
    "wrap_16": ("replicate", dict(B=40, T=4, n_rep=16, n_neutral=5)),                          # theta wraps 15 times
    "env_theta": ("multienv_replicate", dict(B=60, T=[3, 4], n_rep=2, n_env=2, n_neutral=5)),   # theta per (mutant, environment)
    "genotype_regrouped": ("genotype", dict(B=90, T=3, n_geno=7, n_neutral=10)),                # a non-identity permutation
}
HIER_N = {"grid_stride": (2, 777), "wrap_16": (2, 1000), "env_theta": (2, 3, 4, 5, 255, 256, 257, 1024, 1025, 2048, 16384),
          "genotype_regrouped": (2, 3, 4, 5, 255, 256, 257, 1024, 1025, 2048, 16384)}
HIER_BAD_N = (1, 0, -1, 16385)


def hier_spec(name):
    kind, kw = HIER[name]
    return fixtures.synthetic(kind, seed=3, **kw)


class HierHandle:
    """A handle of a HIER case three steps into a run, and its posterior as oracle/rng.hier_fitness takes it: every array in the
    handle's INTERNAL unit order (the oracle keys a unit's draws by its position), theta's index per unit."""

    def __init__(self, lib, name):
        self.sp = sp = hier_spec(name)
        self.e = e = make_engine(sp, lib, seed=4)
        e.run(3)
        self.refresh()

    def refresh(self):
        sp, e = self.sp, self.e
        mean, sigma = e.posterior()
        off = sp.offsets()
        (lo_th, hi_th), (lo_tt, hi_tt), (lo_lt, _) = off["theta"], off["theta_tilde"], off["logtau"]
        self.n_units = n = hi_tt - lo_tt
        idx = np.asarray(sp.geno_idx) if sp.kind == "genotype" else np.arange(n) % (hi_th - lo_th)
        cidx = e.permutation()
        self.pu = pu = cidx[(cidx >= lo_tt) & (cidx < hi_tt)] - lo_tt          # pu[u'] = the caller's unit of internal unit u'
        assert np.array_equal(np.sort(pu), np.arange(n))
        self.idx = idx[pu]
        self.theta = (mean[lo_th:hi_th], sigma[lo_th:hi_th])
        self.lt = (mean[lo_lt:lo_lt + n][pu], sigma[lo_lt:lo_lt + n][pu])
        self.tt = (mean[lo_tt:hi_tt][pu], sigma[lo_tt:hi_tt][pu])

    def oracle(self, n, seed):
        return rng.hier_fitness(seed, n, self.idx, *self.theta, *self.lt, *self.tt)

    def close(self):
        self.e.close()


def case_hier_all_units(hh, n, seed=21):
    """Every unit, in the handle's internal order, against the oracle on the same Philox draws."""
    med, sd = hh.e.hier_fitness(n, seed=seed)
    med2, sd2 = hh.oracle(n, seed)
    assert med.shape == sd.shape == (hh.n_units,)
    a, b = np.abs(med[hh.pu] - med2).max(), np.abs(sd[hh.pu] - sd2).max()
    print(f"bb_hier_fitness, {hh.n_units} units, n = {n}: |dmedian| {a:.3e} |dstd| {b:.3e}")
    assert a < 1e-10 and b < 1e-10, (a, b)


def case_hier_bad_n(hh):
    for n in HIER_BAD_N:
        with np.testing.assert_raises_regex(bb.BarBayHipError, r"error -4: n_samples must be in 2\.\.16384"):
            hh.e.hier_fitness(n, seed=1)
    hh.e.hier_fitness(2, seed=1)          # the handle still answers


def case_hier_degenerate(hh, ns=(2, 3, 777, 1024)):
    """omega = -800 everywhere: sigma = softplus(omega) underflows to 0, every draw of a unit is the same number -- every key of the
    sort equal, every deviation from the mean 0.  Every std is exactly 0 (the mean is formed about the first draw: summed plainly,
    n = 3 equal draws already left 383 of grid_stride's 2180 units with a std of 1e-15, n = 16384 all but 13 with up to 4e-13).
    Every median is, to the bit, m_th + exp(m_lt) m_tt as numpy evaluates it WITH THE LIBRARY'S exp (bb_exp through bb_debug_math;
    tests/_math_cases.py holds it to 4e-16 of the 50-digit value, not to the last bit of another libm: with np.exp 83 of those 2180
    medians differ, by an ulp, in the emulation, exactly the units on which the two exp differ); with np.exp itself the medians
    agree within that bound on exp, 4e-16 |exp(m_lt) m_tt|, and the two roundings of the expression."""
    e = hh.e
    mu, om = e.get_params()
    try:
        e.set_params(mu, np.full(e.D, -800.0))
        hh.refresh()
        assert not hh.theta[1].any() and not hh.lt[1].any() and not hh.tt[1].any()
        m_th, m_lt, m_tt = hh.theta[0][hh.idx], hh.lt[0], hh.tt[0]
        want = m_th + e.debug_math("exp", m_lt)[0] * m_tt
        want_np = m_th + np.exp(m_lt) * m_tt
        bound_np = 4e-16 * np.abs(np.exp(m_lt) * m_tt) + 2.0 ** -52 * (np.abs(np.exp(m_lt) * m_tt) + np.abs(want_np))
        for n in ns:
            med, sd = e.hier_fitness(n, seed=21)
            print(f"degenerate posterior, n = {n}: std != 0 on {int((sd != 0).sum())} units (max {np.abs(sd).max():.3e}); medians != the "
                  f"expression with bb_exp on {int((med[hh.pu] != want).sum())}, with np.exp on {int((med[hh.pu] != want_np).sum())} "
                  f"(max {np.abs(med[hh.pu] - want_np).max():.3e})")
            assert np.array_equal(sd, np.zeros(hh.n_units))
            assert np.array_equal(med[hh.pu], want)
            assert np.all(np.abs(med[hh.pu] - want_np) <= bound_np)
    finally:
        e.set_params(mu, om)
        hh.refresh()
