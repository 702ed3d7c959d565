"""The launch plan of a handle (csrc/bb_plan.h): one row per branch of the planner, each a model request on a small shape, Engine
options, the environment switches (set before the create: read_tuning runs in bb_create) and, for the cross-GPU rows, how the leg
is switched on.  No row runs a step.  What a row expects is what bb_get_stats and bb_kernel_name report -- (resident_kernel,
persistent_pairs, n_blocks, block_threads, lds_bytes, name) -- or, for a refusal (launch_mode = 2, bb_p2p_enable),
BB_ERR_UNSUPPORTED and a regular expression for bb_last_error; a cross-GPU row also expects the plan before the attempt, after it
and after the leg is switched off again (a refused attempt leaves the handle planning exactly as before: the rollback).  The
expectations are recorded results, one column per backend under tests/golden/ (make_plan_columns.py records them): plan_emu.json
from the emulation library, run by tests/test_emu_plan.py, plan_gpu.json from the product library on an MI355X (kernel names, the
instances that exist, the LDS cap and whether a grid fits resident differ there), run by tests/test_gpu_plan.py -- both from the
libraries BEFORE the planner moved into bb_plan.h.  A row's name says which branch its shape was chosen for; where a name says which
implementation results, that is the emulation's.  The groups of the first hop (ng), the leader tiles' size (NBL) and the window
fetch (pf) do not show in the stats: a row that differs from its neighbour only in them records the same plan, and pins only that
the branch is walked without changing what is visible."""
import re

import numpy as np

import barbay_jl_amd as bb

UNSUPPORTED = -4


def counts(t, b, rep=0):
    """t x b counts, all > 0."""
    return (np.arange(t * b, dtype=np.int64).reshape(t, b) * 7 + 11 * rep) % 53 + 20


def row(kind, nn, nb, T, env=None, geno=None, p2p=None, emu_only=False, gpu_only=False, **opts):
    """T: time points per replicate (a list: one entry per replicate).  geno: "runs" (sorted), "scattered", or an explicit geno_idx.
    p2p: "self" (BB_P2P_SELF on a whole-problem handle), an int (that many ranks in this process: the emulation) -- the leg is then
    switched on after the create and the row also records the plan before the attempt."""
    return dict(kind=kind, nn=nn, nb=nb, T=T if isinstance(T, list) else [T], env=env or {}, geno=geno, p2p=p2p, emu_only=emu_only,
                gpu_only=gpu_only, opts=opts)


def _nb_nthr(nb, nthr, **more):
    return dict({"BB_TUNE_NB": str(nb), "BB_TUNE_NTHR": str(nthr)}, **{k: str(v) for k, v in more.items()})


ROWS = {
    # every kind, default switches
    "kind_fitness": row("fitness", 3, 20, 4),
    "kind_multienv": row("multienv", 3, 20, 4),
    "kind_genotype": row("genotype", 3, 20, 4, geno="runs"),
    "kind_replicate": row("replicate", 3, 20, [4, 4]),
    "kind_multienv_replicate": row("multienv_replicate", 3, 20, [4, 4]),
    # k_persist (BB_NO_RES): P = 1 .. 4 pairs per thread at the thread counts that allow them, then refused
    "persist_P1_128": row("fitness", 3, 37, 4, env=_nb_nthr(40, 128, BB_NO_RES=1), launch_mode=2),
    "persist_P2_128": row("fitness", 3, 77, 4, env=_nb_nthr(80, 128, BB_NO_RES=1), launch_mode=2),
    "persist_P3_128": row("fitness", 3, 117, 4, env=_nb_nthr(120, 128, BB_NO_RES=1), launch_mode=2),
    "persist_P4_128": row("fitness", 3, 157, 4, env=_nb_nthr(160, 128, BB_NO_RES=1), launch_mode=2),
    "persist_P5_128_refused": row("fitness", 3, 197, 4, env=_nb_nthr(200, 128, BB_NO_RES=1), launch_mode=2),
    "persist_P1_512": row("fitness", 3, 157, 4, env=_nb_nthr(160, 512, BB_NO_RES=1), launch_mode=2),
    "persist_P3_512": row("fitness", 3, 477, 4, env=_nb_nthr(480, 512, BB_NO_RES=1), launch_mode=2),
    "persist_P1_1024": row("fitness", 3, 157, 4, env=_nb_nthr(160, 1024, BB_NO_RES=1), launch_mode=2),
    "persist_P2_1024_over_the_lds_cap_on_the_device": row("fitness", 3, 477, 4, env=_nb_nthr(480, 1024, BB_NO_RES=1), launch_mode=2),
    "persist_P3_1024_is_4_refused": row("fitness", 3, 797, 4, env=_nb_nthr(800, 1024, BB_NO_RES=1), launch_mode=2),
    "persist_P3_1024_mode0": row("fitness", 3, 797, 4, env=_nb_nthr(800, 1024, BB_NO_RES=1)),
    # k_res: P = 1 .. Pmax, then k_stream for T = 8, 6, 4
    "res_P1_128": row("fitness", 3, 37, 4, env=_nb_nthr(40, 128)),
    "res_P2_128": row("fitness", 3, 77, 4, env=_nb_nthr(80, 128)),
    "res_P4_128": row("fitness", 3, 157, 4, env=_nb_nthr(160, 128)),
    "res_P3_512": row("fitness", 3, 477, 4, env=_nb_nthr(480, 512)),
    "res_P1_1024": row("fitness", 3, 317, 4, env=_nb_nthr(320, 1024)),
    "res_lds_too_large_k_persist": row("fitness", 3, 477, 4, env=_nb_nthr(480, 1024)),
    "stream_T8": row("fitness", 3, 157, 8, env=_nb_nthr(160, 128)),
    "stream_T6": row("fitness", 3, 197, 6, env=_nb_nthr(200, 128)),
    "stream_T4": row("fitness", 3, 297, 4, env=_nb_nthr(300, 128)),
    "stream_T8_1024": row("fitness", 3, 837, 8, env=_nb_nthr(105, 1024, BB_TUNE_RES_NB=420)),
    "replicate_T6_res_nb_512": row("replicate", 3, 317, [6, 6], env=_nb_nthr(40, 512, BB_TUNE_RES_NB=160)),
    # ... refused: T not in {4, 6, 8}, odd parity, BB_NO_STREAM, more than 64 streamed pairs per thread
    "stream_T10_refused": row("fitness", 3, 157, 10, env=_nb_nthr(160, 128), launch_mode=2),
    "stream_T10_mode0": row("fitness", 3, 157, 10, env=_nb_nthr(160, 128)),
    "stream_odd_T_refused": row("fitness", 3, 197, 7, env=_nb_nthr(200, 128, BB_TUNE_AP=1), launch_mode=2),
    "stream_no_stream_refused": row("fitness", 3, 157, 8, env=_nb_nthr(160, 128, BB_NO_STREAM=1), launch_mode=2),
    "stream_Ps_65_refused": row("fitness", 3, 2197, 8, env=_nb_nthr(200, 128, BB_TUNE_RES_NB=2200), launch_mode=2),
    "stream_forced_small": row("fitness", 3, 37, 8, env=_nb_nthr(16, 128, BB_TUNE_STREAM=1)),
    "stream_forced_several_samples": row("fitness", 3, 37, 8, env=_nb_nthr(16, 128, BB_TUNE_STREAM=1), samples_per_step=2),
    "stream_forced_T5_stays_k_res": row("fitness", 3, 37, 5, env=_nb_nthr(16, 128, BB_TUNE_STREAM=1, BB_TUNE_AP=1)),
    # any-parity shapes (odd T; the genotype model's odd loglambda offset): refused first and taken as the second chance after
    # k_persist refuses; taken first with BB_TUNE_AP, several samples, the ELBO trace, the genotype model
    "ap_odd_T_k_persist_first": row("fitness", 3, 37, 5, env=_nb_nthr(16, 128)),
    "ap_odd_T_k_persist_first_512": row("fitness", 3, 97, 5, env=_nb_nthr(100, 512)),
    "ap_odd_T_k_persist_first_1024": row("fitness", 3, 277, 5, env=_nb_nthr(280, 1024)),
    "ap_odd_T_both_refuse_two_kernels": row("fitness", 3, 197, 5, env=_nb_nthr(200, 128)),
    "ap_odd_T_second_chance_on_the_leg": row("fitness", 3, 637, 5, env=_nb_nthr(80, 128), p2p="self"),
    "ap_odd_T_BB_TUNE_AP": row("fitness", 3, 37, 5, env=_nb_nthr(16, 128, BB_TUNE_AP=1)),
    "ap_odd_T_several_samples": row("fitness", 3, 37, 5, env=_nb_nthr(16, 128), samples_per_step=2),
    "ap_odd_T_elbo_trace": row("fitness", 3, 37, 5, env=_nb_nthr(16, 128), elbo_every=1),
    "ap_genotype_odd_offset": row("genotype", 3, 38, 4, geno="runs", env=_nb_nthr(16, 128, BB_NO_REORDER=1)),
    "ap_replicate_ragged_T": row("replicate", 3, 37, [5, 4], env=_nb_nthr(16, 128)),
    # genotype model: sorted, scattered (regrouped), a genotype larger than a tile, the grow loop, the uniform-map fallback
    "geno_sorted": row("genotype", 3, 45, 4, geno="runs", env=_nb_nthr(16, 128)),
    "geno_scattered": row("genotype", 3, 45, 4, geno="scattered", env=_nb_nthr(16, 128)),
    "geno_scattered_no_regroup_refused": row("genotype", 3, 45, 4, geno="scattered", env=_nb_nthr(16, 128, BB_NO_REGROUP=1), launch_mode=2),
    "geno_larger_than_a_tile_refused": row("genotype", 3, 45, 4, geno=[0] * 30 + [1] * 15, env=_nb_nthr(8, 128), launch_mode=2),
    "geno_larger_than_a_tile_mode0": row("genotype", 3, 45, 4, geno=[0] * 30 + [1] * 15, env=_nb_nthr(8, 128)),
    "geno_grow": row("genotype", 3, 45, 4, geno=[i // 5 for i in range(45)], env=_nb_nthr(8, 128)),
    "geno_grow_leaders": row("genotype", 3, 160, 4, geno=[i // 5 for i in range(160)], env=_nb_nthr(8, 128, BB_TUNE_LEAD=50)),
    "geno_leaders_fall_back_to_uniform": row("genotype", 3, 160, 4, geno=[i // 8 for i in range(160)], env=_nb_nthr(8, 128, BB_TUNE_LEAD=50)),
    "geno_several_samples": row("genotype", 3, 45, 4, geno="runs", env=_nb_nthr(16, 128), samples_per_step=2),
    # leader tiles: BB_TUNE_LEAD at 100 and at the default 65, enough tiles (nblk0 >= 2 ng) and too few; the "stay uniform" fallback
    "lead_100": row("fitness", 3, 253, 4, env=_nb_nthr(16, 128, BB_TUNE_LEAD=100)),
    "lead_65_set": row("fitness", 3, 253, 4, env=_nb_nthr(16, 128, BB_TUNE_LEAD=65)),
    "lead_default_nb_fixed": row("fitness", 3, 253, 4, env=_nb_nthr(16, 128)),
    "lead_50_too_few_tiles": row("fitness", 3, 237, 4, env=_nb_nthr(16, 128, BB_TUNE_LEAD=50)),
    "lead_50_enough_tiles": row("fitness", 3, 253, 4, env=_nb_nthr(16, 128, BB_TUNE_LEAD=50)),
    "lead_out_of_range_is_100": row("fitness", 3, 253, 4, env=_nb_nthr(16, 128, BB_TUNE_LEAD=5)),
    "lead_stays_uniform": row("fitness", 3, 253, 4, env=_nb_nthr(16, 128, BB_TUNE_LEAD=99)),
    "lead_stays_uniform_over_the_grid": row("fitness", 3, 253, 4, env=_nb_nthr(8, 256, BB_TUNE_NG=16, BB_TUNE_LEAD=10)),
    "lead_stays_uniform_another_pair_slot": row("fitness", 3, 1053, 4, env={"BB_TUNE_NTHR": "128"}),
    "lead_default_free_tile_size": row("fitness", 3, 637, 4, env={"BB_TUNE_NTHR": "128"}),
    "lead_default_free_tile_size_nb_0": row("fitness", 3, 637, 4, env=_nb_nthr(0, 128)),
    "res_nb": row("fitness", 3, 253, 4, env=_nb_nthr(32, 128, BB_TUNE_RES_NB=16)),
    "res_nb_lead_50_over_the_buffers_k_persist": row("fitness", 3, 253, 4, env=_nb_nthr(32, 128, BB_TUNE_RES_NB=16, BB_TUNE_LEAD=50)),
    "res_nb_over_the_buffers_k_persist": row("fitness", 3, 253, 4, env=_nb_nthr(64, 128, BB_TUNE_RES_NB=8), launch_mode=2),
    # groups of the exchange's first hop: 8, then 16 and 32 where the shape allows and where it does not (ng itself is not in the stats)
    "groups_many_tiles_256_threads": row("fitness", 3, 637, 4, env=_nb_nthr(8, 256)),
    "groups_many_tiles_128_threads": row("fitness", 3, 637, 4, env=_nb_nthr(8, 128)),
    "groups_8_asked": row("fitness", 3, 637, 4, env=_nb_nthr(8, 128, BB_TUNE_NG=8)),
    "groups_16_asked": row("fitness", 3, 253, 4, env=_nb_nthr(8, 256, BB_TUNE_NG=16, BB_TUNE_LEAD=50)),
    "groups_16_asked_too_few_threads": row("fitness", 3, 253, 4, env=_nb_nthr(8, 64, BB_TUNE_NG=16, BB_TUNE_LEAD=50)),
    "groups_32_asked": row("fitness", 3, 637, 4, env=_nb_nthr(8, 256, BB_TUNE_NG=32, BB_TUNE_LEAD=50)),
    "groups_32_asked_too_few_tiles": row("fitness", 3, 253, 4, env=_nb_nthr(8, 256, BB_TUNE_NG=32, BB_TUNE_LEAD=50)),
    "groups_32_asked_too_few_threads": row("fitness", 3, 637, 4, env=_nb_nthr(8, 128, BB_TUNE_NG=32, BB_TUNE_LEAD=50)),
    "groups_24_asked_ignored": row("fitness", 3, 637, 4, env=_nb_nthr(8, 256, BB_TUNE_NG=24)),
    # the moment row longer than the workgroup (K + 2 nt1 > nthr)
    "row_longer_than_the_workgroup_refused": row("multienv_replicate", 3, 20, [12, 12], env=_nb_nthr(16, 64), launch_mode=2),
    "row_longer_than_the_workgroup_k_persist": row("multienv_replicate", 3, 20, [12, 12], env=_nb_nthr(8, 64)),
    # the switches that take a whole implementation out, and the launch modes
    "no_res": row("fitness", 3, 37, 4, env=_nb_nthr(16, 128, BB_NO_RES=1)),
    "no_persist_mode0": row("fitness", 3, 37, 4, env=_nb_nthr(16, 128, BB_NO_PERSIST=1)),
    "no_persist_mode2": row("fitness", 3, 37, 4, env=_nb_nthr(16, 128, BB_NO_PERSIST=1), launch_mode=2),
    "no_res_no_persist": row("fitness", 3, 37, 4, env=_nb_nthr(16, 128, BB_NO_RES=1, BB_NO_PERSIST=1)),
    "force_allreduce": row("fitness", 3, 37, 4, env=_nb_nthr(16, 128, BB_FORCE_ALLREDUCE=1)),
    "force_allreduce_refused": row("fitness", 3, 37, 4, env=_nb_nthr(16, 128, BB_FORCE_ALLREDUCE=1), launch_mode=2),
    "no_host_tables": row("fitness", 3, 37, 4, env=_nb_nthr(16, 128, BB_NO_HOST_TABLES=1)),
    "decayed_adagrad": row("fitness", 3, 37, 4, env=_nb_nthr(16, 128), optimizer="DecayedADAGrad"),
    "mode0": row("fitness", 3, 37, 4, env=_nb_nthr(16, 128), launch_mode=0),
    "mode1": row("fitness", 3, 37, 4, env=_nb_nthr(16, 128), launch_mode=1),
    "mode2": row("fitness", 3, 37, 4, env=_nb_nthr(16, 128), launch_mode=2),
    # the reasons launch_mode = 2 gives that no row above meets
    "why_sharded_run": row("fitness", 3, 37, 4, env=_nb_nthr(16, 128), launch_mode=2, rank=0, world_size=2),
    "sharded_run_mode0": row("fitness", 3, 37, 4, env=_nb_nthr(16, 128), rank=1, world_size=2),
    "why_samples_per_step": row("fitness", 3, 197, 10, env=_nb_nthr(200, 128), launch_mode=2, samples_per_step=2),
    "why_elbo_recording": row("fitness", 3, 197, 10, env=_nb_nthr(200, 128), launch_mode=2, elbo_every=2),
    "why_genotype_no_tile_map": row("genotype", 3, 197, 10, geno="runs", env=_nb_nthr(200, 128), launch_mode=2),
    # the cross-GPU leg: on; fewer than 8 tiles refused and the handle as before the attempt; more than one pair per thread refused
    "p2p_self": row("fitness", 3, 253, 4, env=_nb_nthr(16, 128), p2p="self"),
    "p2p_self_genotype": row("genotype", 3, 253, 4, geno="runs", env=_nb_nthr(16, 128), p2p="self"),
    "p2p_self_too_few_tiles": row("fitness", 3, 37, 4, env=_nb_nthr(16, 128), p2p="self"),
    "p2p_self_genotype_coarse_genotypes": row("genotype", 3, 125, 4, geno=[i // 12 for i in range(125)], env=_nb_nthr(16, 128, BB_TUNE_LEAD=100), p2p="self"),
    "p2p_self_genotype_too_few_tiles_of_its_own": row("genotype", 3, 125, 4, geno="runs", env=_nb_nthr(16, 128, BB_TUNE_RES_NB=32), p2p="self"),
    "p2p_self_two_pairs_refused": row("fitness", 3, 1597, 5, env=_nb_nthr(200, 128, BB_NO_RES=1), p2p="self"),
    "p2p_self_k_persist": row("fitness", 3, 253, 4, env=_nb_nthr(16, 128, BB_NO_RES=1), p2p="self"),
    "p2p_self_no_stream_on_the_leg": row("fitness", 3, 1597, 8, env=_nb_nthr(200, 128), p2p="self"),
    "p2p_two_ranks": row("fitness", 3, 509, 4, env=_nb_nthr(16, 128), p2p=2, emu_only=True),
    "p2p_two_ranks_too_few_tiles": row("fitness", 3, 125, 4, env=_nb_nthr(16, 128), p2p=2, emu_only=True),
    "p2p_three_ranks_genotype_several_samples": row("genotype", 3, 765, 4, geno="runs", env=_nb_nthr(24, 128), p2p=3, emu_only=True, samples_per_step=2),
    "group_two_shards": row("fitness", 3, 509, 4, env=_nb_nthr(16, 256), emu_only=True, device_ids=[0, 0]),
    "group_two_shards_mode2_refused": row("fitness", 3, 125, 4, env=_nb_nthr(16, 256), emu_only=True, device_ids=[0, 0], launch_mode=2),
}


def rows_for(gpu):
    return [k for k, v in ROWS.items() if not (v["emu_only"] if gpu else v["gpu_only"])]


def _geno_idx(r):
    g = r["geno"]
    if g == "runs":
        return np.arange(r["nb"], dtype=np.int32) // 3
    if g == "scattered":
        return (np.arange(r["nb"], dtype=np.int32) * 7) % ((r["nb"] + 2) // 3)
    return np.asarray(g, dtype=np.int32)


def _engine(lib, r, **more):
    B = r["nn"] + r["nb"]
    kw = dict(window=3, seed=3, _lib=lib)
    if r["kind"] in ("multienv", "multienv_replicate"):
        kw["env_idx"] = np.concatenate([np.arange(t, dtype=np.int32) % 2 for t in r["T"]])
    if r["kind"] == "genotype":
        kw["geno_idx"] = _geno_idx(r)
    kw.update(r["opts"])
    kw.update(more)
    return bb.Engine(r["kind"], [counts(t, B, rep=i) for i, t in enumerate(r["T"])], r["nn"], r["nb"], **kw)


def _plan(e):
    s = e.stats()
    return [int(s[k]) for k in ("resident_kernel", "persistent_pairs", "n_blocks", "block_threads", "lds_bytes")] + [e.kernel_name()]


def observe(lib, name, setenv):
    """What the library does with row `name`: {"plan": [...]} or {"refused": [code, message]}; a cross-GPU row: the plans of every rank
    before the attempt ("before"), what bb_p2p_enable(1) answered ("enable": True, or [code, message]) and the plans after it."""
    r = ROWS[name]
    for k, v in r["env"].items():
        setenv(k, v)
    if r["p2p"] == "self":
        setenv("BB_P2P_SELF", "1")
    world = r["p2p"] if isinstance(r["p2p"], int) else 1
    es = []
    try:
        try:
            for rank in range(world):
                es.append(_engine(lib, r, **(dict(rank=rank, world_size=world) if world > 1 else {})))
        except bb.BarBayHipError as e:
            m = re.match(r"barbay_hip error (-?\d+): (.*)$", str(e), re.S)
            return {"refused": [int(m.group(1)), m.group(2)]}
        if not r["p2p"]:
            return {"plan": _plan(es[0])}
        out = {"before": [_plan(e) for e in es]}
        handles = [e.p2p_export() for e in es]
        for e in es:
            e.p2p_import(handles)
        out["enable"] = []
        for e in es:
            ok = e.p2p_enable(True)
            out["enable"].append(True if ok else [UNSUPPORTED, lib.bb_last_error().decode()])
        out["after"] = [_plan(e) for e in es]
        for e in es:
            assert e.p2p_enable(False)
        out["off"] = [_plan(e) for e in es]
        return out
    finally:
        for e in es:
            e.close()


def export_requests(path):
    """The table's requests as lines of numbers and words for tests/plan_walk.cpp (the stand-alone walk under a sanitizer):
    name kind nn nb | n_rep T.. | n g.. (geno_idx) | n e.. (env_idx) | n K=V.. (switches) | samples elbo_every launch_mode optimizer | ranks
    (0: no cross-GPU attempt, -1: BB_P2P_SELF) n_devices."""
    with open(path, "w") as f:
        for name in rows_for(gpu=False):
            r, o = ROWS[name], ROWS[name]["opts"]
            extra = set(o) - {"samples_per_step", "elbo_every", "launch_mode", "optimizer", "device_ids", "rank", "world_size"}
            assert not extra, extra
            geno = list(_geno_idx(r)) if r["kind"] == "genotype" else []
            env_idx = [t % 2 for T in r["T"] for t in range(T)] if r["kind"] in ("multienv", "multienv_replicate") else []
            sw = [f"{k}={v}" for k, v in r["env"].items()]
            ranks = -1 if r["p2p"] == "self" else (r["p2p"] or 0)
            words = [name, bb._capi.BB_MODEL[r["kind"]], r["nn"], r["nb"], len(r["T"]), *r["T"], len(geno), *geno, len(env_idx), *env_idx, len(sw), *sw,
                     o.get("samples_per_step", 1), o.get("elbo_every", 0), o.get("launch_mode", 0), int(o.get("optimizer") == "DecayedADAGrad"),
                     o.get("rank", 0), o.get("world_size", 1), ranks, len(o.get("device_ids", [0]))]
            f.write(" ".join(str(w) for w in words) + "\n")


def _check_refusal(name, got, want):
    assert got[0] == want[0] == UNSUPPORTED, (name, got)
    assert re.search(want[1], got[1]), (name, got[1], want[1])


def case_plan(lib, name, setenv, expect):
    got = observe(lib, name, setenv)
    print(f"{name}: {got}")
    want = expect[name]
    assert set(got) == set(want), (name, got, want)
    if "refused" in want:
        return _check_refusal(name, got["refused"], want["refused"])
    if "plan" in want:
        assert got["plan"] == want["plan"], (name, got, want)
        return
    assert got["before"] == want["before"] and got["after"] == want["after"] and got["off"] == want["off"], (name, got, want)
    for g, w in zip(got["enable"], want["enable"]):
        if w is True:
            assert g is True, (name, got)
        else:
            _check_refusal(name, g, w)
    # the rollback: a refused bb_p2p_enable leaves the handle planning exactly as before the attempt; switching the leg off again too
    for i, w in enumerate(want["enable"]):
        if w is not True:
            assert got["after"][i] == got["before"][i], (name, got)
        assert got["off"][i] == got["before"][i], (name, got)
