"""The requests bb_create refuses, shared by the emulation tests (CPU, tests/test_emu_create.py) and the GPU tests
(tests/test_gpu_create.py): one row per bb_fail site on the creation path (csrc/bb_create.h, group_create's argument checks included),
each on the smallest shape that reaches the check -- 2 neutral + 3 mutant barcodes, 3 time points -- with the code and a regular
expression for bb_last_error.  A row goes through bb.Engine where Engine can express the request ("engine": a change to its
keywords), else through the _capi structures ("md" / "opts": a change to the marshalled bb_model_desc / bb_advi_opts).  After every refusal
one valid handle is created and closed on the same library: a refusal leaves nothing behind that breaks the next create.  The
expectations were recorded from the library BEFORE creation moved into bb_create.h; which of two faults is reported is part of them
(the TWO_FAULTS rows)."""
import ctypes as C
import re

import numpy as np

import barbay_jl_amd as bb
from barbay_jl_amd import _capi

INVALID, DEVICE, UNSUPPORTED = -1, -2, -4
NN, NB, T = 2, 3, 3


def _counts(t=T, rep=0):
    """t x (NN + NB) counts, every one different and > 0."""
    return (np.arange(t * (NN + NB), dtype=np.int64).reshape(t, NN + NB) * 7 + 11 * rep) % 53 + 20


def base(kind="fitness"):
    """Engine's keywords of the valid request of a model kind (genotype: the mutants scattered, so bb_create regroups them)."""
    kw = dict(kind=kind, counts=[_counts()], n_neutral=NN, n_bc=NB, window=3)
    if kind in ("replicate", "multienv_replicate"):
        kw["counts"] = [_counts(), _counts(rep=1)]
    if kind in ("multienv", "multienv_replicate"):
        kw["env_idx"] = np.array([0, 1, 0] * len(kw["counts"]), dtype=np.int32)
    if kind == "genotype":
        kw["geno_idx"] = np.array([1, 0, 1], dtype=np.int32)
    return kw


def marshal(kw):
    """bb_model_desc and bb_advi_opts of Engine's keywords `kw` (defaults otherwise), and the arrays they point into."""
    counts = [np.asarray(c, dtype=np.int64) for c in kw["counts"]]
    keep = [np.asarray([c.shape[0] for c in counts], dtype=np.int32),
            np.concatenate([np.ascontiguousarray(c.T).reshape(-1) for c in counts]),
            np.concatenate([c.sum(axis=1) for c in counts])]
    md = _capi.bb_model_desc()
    md.kind, md.n_rep, md.n_neutral, md.n_bc = _capi.BB_MODEL[kw["kind"]], len(counts), kw["n_neutral"], kw["n_bc"]
    md.n_time = keep[0].ctypes.data_as(C.POINTER(C.c_int32))
    md.counts = keep[1].ctypes.data_as(C.POINTER(C.c_int64))
    md.totals = keep[2].ctypes.data_as(C.POINTER(C.c_int64))
    for name in ("env", "geno"):
        if kw.get(name + "_idx") is not None:
            a = np.ascontiguousarray(kw[name + "_idx"], dtype=np.int32)
            keep.append(a)
            setattr(md, "n_" + name, int(a.max()) + 1)
            setattr(md, name + "_idx", a.ctypes.data_as(C.POINTER(C.c_int32)))
    return md, keep


def _set(**changes):
    return lambda x: [setattr(x, k, v) for k, v in changes.items()]


def _kw(**changes):
    return lambda kw: kw.update(changes)


def _count(rep, t, b, v, stale_totals=False):
    """count [rep][t, b] = v; the totals follow (Engine sums the counts itself) unless stale_totals."""
    def f(kw):
        kw["counts"] = [c.copy() for c in kw["counts"]]
        if stale_totals:
            kw["totals"] = [c.sum(axis=1) for c in kw["counts"]]
        kw["counts"][rep][t, b] = v
    return f


def _at(a, i, v):
    a = np.array(a, dtype=np.float64)
    a[i] = v
    return a


def _prior(name, mean, std):
    return lambda kw: kw.update(priors={name: (mean, std)})


def row(kind, code, match, engine=None, md=None, opts=None, gpu_only=False, emu_only=False):
    return dict(kind=kind, code=code, match=match, engine=engine, md=md, opts=opts, gpu_only=gpu_only, emu_only=emu_only)


NL = T * (NN + NB)          # loglambda latents of the one-replicate shapes
ROWS = {
    "unknown_kind": row("fitness", INVALID, r"^unknown model kind 5$", md=_set(kind=5)),
    "negative_kind": row("fitness", INVALID, r"^unknown model kind -1$", md=_set(kind=-1)),
    "n_rep_zero": row("replicate", INVALID, r"^n_rep must be in 1\.\.16$", md=_set(n_rep=0)),
    "n_rep_17": row("replicate", INVALID, r"^n_rep must be in 1\.\.16$", engine=_kw(counts=[_counts()] * 17)),
    "n_rep_2_on_fitness": row("fitness", INVALID, r"^only the replicate models take n_rep > 1$", engine=_kw(counts=[_counts()] * 2)),
    "n_rep_2_on_genotype": row("genotype", INVALID, r"^only the replicate models take n_rep > 1$", engine=_kw(counts=[_counts()] * 2)),
    "no_neutral": row("fitness", INVALID, r"^need at least one neutral and one mutant barcode$", engine=_kw(n_neutral=0, n_bc=NN + NB)),
    "no_mutant": row("fitness", INVALID, r"^need at least one neutral and one mutant barcode$", engine=_kw(n_neutral=NN + NB, n_bc=0)),
    "n_time_missing": row("fitness", INVALID, r"^n_time/counts/totals missing$", md=_set(n_time=None)),
    "counts_missing": row("fitness", INVALID, r"^n_time/counts/totals missing$", md=_set(counts=None)),
    "totals_missing": row("genotype", INVALID, r"^n_time/counts/totals missing$", md=_set(totals=None)),
    "samples_per_step_0": row("fitness", INVALID, r"^samples_per_step must be >= 1$", engine=_kw(samples_per_step=0)),
    "unknown_optimizer": row("fitness", INVALID, r"^unknown optimizer 2$", opts=_set(optimizer=2)),
    "window_0": row("fitness", INVALID, r"^window must be >= 1$", engine=_kw(window=0)),
    "eta_nan": row("fitness", INVALID, r"^eta must be finite$", engine=_kw(eta=np.nan)),
    "tau_inf": row("fitness", INVALID, r"^tau must be finite$", engine=_kw(tau=np.inf)),
    "pre_inf": row("fitness", INVALID, r"^pre must be finite$", engine=_kw(optimizer="DecayedADAGrad", pre=-np.inf)),
    "post_nan": row("fitness", INVALID, r"^post must be finite$", engine=_kw(optimizer="DecayedADAGrad", post=np.nan)),
    "rank_is_world_size": row("fitness", INVALID, r"^bad rank/world_size 2/2$", engine=_kw(rank=2, world_size=2)),
    "negative_rank": row("fitness", INVALID, r"^bad rank/world_size -1/2$", engine=_kw(rank=-1, world_size=2)),
    "world_size_0": row("fitness", INVALID, r"^bad rank/world_size 0/0$", engine=_kw(world_size=0)),
    "n_devices_17": row("fitness", UNSUPPORTED, r"^at most 16 devices per handle$", engine=_kw(n_devices=17)),
    "n_devices_on_a_rank": row("fitness", INVALID, r"^n_devices > 1 needs rank 0 / world_size 1", engine=_kw(n_devices=2, rank=1, world_size=2)),
    "n_time_1": row("fitness", INVALID, r"^n_time\[0\] = 1 outside 2\.\.255$", engine=_kw(counts=[_counts(1)])),
    "n_time_256_second_replicate": row("replicate", INVALID, r"^n_time\[1\] = 256 outside 2\.\.255$", engine=_kw(counts=[_counts(), _counts(256)])),
    "env_idx_missing": row("multienv", INVALID, r"^multienv models need n_env >= 1 and env_idx$", engine=_kw(env_idx=None)),
    "n_env_0": row("multienv_replicate", INVALID, r"^multienv models need n_env >= 1 and env_idx$", md=_set(n_env=0)),
    "env_idx_negative": row("multienv", INVALID, r"^env_idx\[1\] out of range$", engine=_kw(env_idx=[0, -1, 1])),
    "env_idx_too_large": row("multienv_replicate", INVALID, r"^env_idx\[5\] out of range$", engine=_kw(env_idx=[0, 0, 0, 0, 0, 1]), md=_set(n_env=1)),
    "geno_idx_missing": row("genotype", INVALID, r"^genotype model needs n_geno >= 1 and geno_idx$", engine=_kw(geno_idx=None)),
    "n_geno_0": row("genotype", INVALID, r"^genotype model needs n_geno >= 1 and geno_idx$", md=_set(n_geno=0)),
    "geno_idx_negative": row("genotype", INVALID, r"^geno_idx\[2\] out of range$", engine=_kw(geno_idx=[0, 1, -1])),
    "geno_idx_too_large": row("genotype", INVALID, r"^geno_idx\[0\] out of range$", md=_set(n_geno=1)),
    "negative_count": row("fitness", INVALID, r"^count out of range at rep 0 t 1 barcode 4$", engine=_count(0, 1, 4, -1)),
    "count_2_to_32": row("replicate", INVALID, r"^count out of range at rep 1 t 2 barcode 0$", engine=_count(1, 2, 0, 2 ** 32)),
    "totals_mismatch": row("replicate", INVALID, r"^totals\[rep 1, t 2\] = (\d+) but the counts sum to (\d+) ", engine=_count(1, 2, 3, 5, stale_totals=True)),
    "totals_mismatch_regrouped": row("genotype", INVALID, r"^totals\[rep 0, t 0\] = (\d+) but the counts sum to (\d+) ", engine=_count(0, 0, 4, 5, stale_totals=True)),
    # the prior refusals _cases.case_errors does not make: a std of zero in Vector form, logtau_prior's Matrix form on a replicate model,
    # a Matrix loglambda prior one short, and a regrouped model's element named where the caller put it when it is NOT the last one
    "prior_std_zero": row("fitness", INVALID, r"^logsigma_bc_prior: std must be > 0 and finite$", engine=_prior("logsigma_bc_prior", 0.0, 0.0)),
    "logtau_mean_inf": row("replicate", INVALID, r"^logtau_prior: mean must be finite$", engine=_prior("logtau_prior", np.inf, 1.0)),
    "logtau_matrix_on_replicate": row("replicate", INVALID, r"^logtau_prior accepts only the Vector form \[mean, std\]$",
                                      engine=_prior("logtau_prior", np.full(2 * NB, -2.0), np.ones(2 * NB))),
    "loglambda_matrix_short": row("fitness", INVALID, rf"^loglambda_prior: Matrix form needs {NL} rows, got {NL - 1}$",
                                  engine=_prior("loglambda_prior", np.zeros(NL - 1), np.ones(NL - 1))),
    "regrouped_logsigma_bc_std": row("genotype", INVALID, r"^logsigma_bc_prior: std\[0\] must be > 0 and finite$",
                                     engine=_prior("logsigma_bc_prior", np.zeros(NB), _at(np.ones(NB), 0, -1.0))),
    "regrouped_loglambda_mean": row("genotype", INVALID, rf"^loglambda_prior: mean\[{NN * T + 1}\] must be finite$",
                                    engine=_prior("loglambda_prior", _at(np.full(NL, 3.0), NN * T + 1, np.nan), np.full(NL, 3.0))),
    "regrouped_theta_std": row("genotype", INVALID, r"^s_bc_prior: std\[1\] must be > 0 and finite$",
                               engine=_prior("s_bc_prior", np.zeros(2), _at(np.ones(2), 1, np.inf))),
    # the launch geometry: the ragged replicate method keeps 2 (T - 1)^2 more moments per replicate than a tile's LDS holds
    "tile_too_large": row("replicate", UNSUPPORTED, r"^a tile of \d+ barcodes needs \d+ bytes of LDS / \d+ threads \(n_time or n_rep too large for this build\)$",
                          engine=_kw(counts=[_counts(255), _counts(255, rep=1)], ragged_method=True)),
    "totals_mismatch_in_a_shard": row("fitness", INVALID, r"^totals\[rep 0, t 2\] = ", engine=lambda kw: (_count(0, 2, 1, 5, stale_totals=True)(kw), kw.update(n_devices=2))),
    # (a multi-device handle on one device: the emulation's; on a GPU its transport probe would launch)
    "group_cannot_run_resident": row("genotype", UNSUPPORTED, r"^launch_mode = 2: the shards cannot run resident launches with peer-mapped inboxes: launch_mode = 2 ",
                                     engine=_kw(device_ids=[0, 0], launch_mode=2), emu_only=True),
    "no_such_device": row("fitness", DEVICE, r"^device 99: no such HIP device \(\d+ visible\)$", engine=_kw(device=99), gpu_only=True),
}
# two faults in one request: the one reported is the one the checks meet first
TWO_FAULTS = {
    "optimizer_and_n_time": row("fitness", INVALID, r"^unknown optimizer 7$", opts=_set(optimizer=7), engine=_kw(counts=[_counts(1)])),
    "n_time_and_count": row("fitness", INVALID, r"^n_time\[0\] = 256 outside", engine=lambda kw: (_kw(counts=[_counts(256)])(kw), _count(0, 0, 0, -3)(kw))),
    "count_and_prior": row("fitness", INVALID, r"^count out of range at rep 0 t 0 barcode 0$", engine=lambda kw: (_count(0, 0, 0, -3)(kw), _prior("s_pop_prior", 0.0, -1.0)(kw))),
    "kind_and_window": row("fitness", INVALID, r"^unknown model kind 9$", md=_set(kind=9), engine=_kw(window=0)),
    "n_devices_and_env_idx": row("multienv", UNSUPPORTED, r"^at most 16 devices per handle$", engine=_kw(n_devices=17, env_idx=[0, -1, 1])),
}
ROWS.update(TWO_FAULTS)


def rows_for(gpu):
    return [k for k, v in ROWS.items() if not (v["emu_only"] if gpu else v["gpu_only"])]


def create(lib, kw, md_change=None, opts_change=None):
    """bb_create of Engine's keywords `kw`: through bb.Engine, or -- with a change to the structures -- through the C ABI itself.
    Returns (code, message); a handle that was created is closed."""
    if md_change is None and opts_change is None:
        try:
            bb.Engine(kw.pop("kind"), kw.pop("counts"), kw.pop("n_neutral"), kw.pop("n_bc"), _lib=lib, **kw).close()
        except bb.BarBayHipError as e:
            m = re.match(r"barbay_hip error (-?\d+): (.*)$", str(e), re.S)
            return int(m.group(1)), m.group(2)
        return 0, ""
    extra = set(kw) - {"kind", "counts", "n_neutral", "n_bc", "env_idx", "geno_idx", "window"}
    assert not extra, extra          # (a raw row's Engine change may only touch what marshal carries over)
    md, keep = marshal(kw)
    o = _capi.bb_advi_opts()
    lib.bb_default_opts(C.byref(o))
    o.window = kw["window"]
    for change, x in ((md_change, md), (opts_change, o)):
        if change:
            change(x)
    h = C.c_void_p()
    rc = lib.bb_create(C.byref(md), C.byref(o), C.byref(h))
    msg = lib.bb_last_error().decode()
    if rc == 0:
        lib.bb_destroy(h)
    else:
        assert not h.value, "a refused bb_create left a handle behind"
    return rc, msg


def case_refusal(lib, name):
    r = ROWS[name]
    kw = base(r["kind"])
    if r["engine"]:
        r["engine"](kw)
    code, msg = create(lib, kw, r["md"], r["opts"])
    print(f"{name}: {code}: {msg}")
    assert code == r["code"], (name, code, msg)
    assert re.search(r["match"], msg), (name, msg)
    assert create(lib, base(r["kind"])) == (0, ""), name          # the next create on this library


def case_null_arguments(lib):
    md, keep = marshal(base())
    o = _capi.bb_advi_opts()
    lib.bb_default_opts(C.byref(o))
    h = C.c_void_p()
    for args in ((None, C.byref(o), C.byref(h)), (C.byref(md), None, C.byref(h)), (C.byref(md), C.byref(o), None)):
        assert lib.bb_create(*args) == INVALID and lib.bb_last_error() == b"null argument"
    assert create(lib, base()) == (0, "")


def case_valid(lib, kind):
    """The base request of every kind is one the library accepts (else a row's refusal could be the base's)."""
    assert create(lib, base(kind)) == (0, "")
