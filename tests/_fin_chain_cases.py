"""Shapes for the one-wave consume + finish of k_res (br_consume_finish, csrc/bb_resident.h): the one-GPU instances with the optimiser
compiled in, fitness / multienv / genotype kinds, compile-time T.  The smallest problems at which that leg can go wrong, all with
BB_TUNE_NTHR=1024 on synthetic fixtures; shared by tests/test_fin_chain_emu.py (host emulation) and tests/test_gpu_fin_chain.py.

Every case: fixtures.synthetic's arguments, BB_TUNE_NB, further environment, and what the plan must make of it -- resident_kernel, tiles,
the product's kernel name, the emulation's, and bb_stats.opt_compiled of the handle created WITHOUT BB_TUNE_OPT_SPEC=0 (1: the instance
that runs the one-wave leg; the handle created with BB_TUNE_OPT_SPEC=0 always reports 0 and runs bbp_consume_tg + br_finish).

one_tile_B330: 330 barcodes of 8 time points are 1320 loglambda lanes, more than one 1024-thread tile holds at one pair per thread, and
two pair slots do not fit LDS beside the window slot: no k_res launch.  The emulation's plan takes k_persist, which has no such leg (the
two handles then run the same code); the product refuses launch_mode = 2 for the shape (k_persist's tile does not fit the device's LDS
either: product name None).  The case only pins that down; one_tile_B200 is the one-tile shape that does reach the instance (NG = 1: a
leader with itself as only member)."""
import pytest

from oracle import fixtures

FIT8 = dict(B=330, T=8, n_neutral=20, seed=3)
K0T8 = ("k_res<0,1,1024,false,8,false,false>", "emu:k_res<0,1,1024,false,*,false,false>")
K0T6 = ("k_res<0,1,1024,false,6,false,false>", "emu:k_res<0,1,1024,false,*,false,false>")
K1T6 = ("k_res<1,1,1024,false,6,false,false>", "emu:k_res<1,1,1024,false,*,false,false>")
K2T8 = ("k_res<2,1,1024,false,8,false,false>", "emu:k_res<2,1,1024,false,*,false,false>")

# id: (kind, synthetic's arguments, BB_TUNE_NB, environment, resident_kernel, tiles, (product name, emulation name), opt_compiled)
CASES = {
    "one_tile_B330": ("fitness", FIT8, 330, {}, 1, 1, (None, "emu:k_persist<0,2,1024>"), 0),
    "one_tile_B200": ("fitness", dict(B=200, T=8, n_neutral=20, seed=3), 200, {}, 2, 1, K0T8, 1),
    "three_tiles_all_leaders": ("fitness", FIT8, 110, {}, 2, 3, K0T8, 1),                       # NG = 3 < 8: the poll's per-entry selects
    "eleven_tiles": ("fitness", FIT8, 30, {}, 2, 11, K0T8, 1),                                  # NG = 8, groups of one and two, non-leader tiles
    "fitness_T6": ("fitness", dict(B=330, T=6, n_neutral=20, seed=3), 30, {}, 2, 11, K0T6, 1),
    # (the last time point's F lane has no moments; c_t of an environment's first time point)
    "multienv_T6_E4": ("multienv", dict(B=330, T=6, n_env=4, n_neutral=20, seed=3), 30, {}, 2, 11, K1T6, 1),
    # (tiles of whole genotypes: 36 barcodes at most give 11 of them)
    "genotype_T8": ("genotype", dict(B=330, T=8, n_geno=30, n_neutral=20, seed=3, geno_runs=True), 36, {}, 2, 11, K2T8, 1),
    # 16 first-hop groups: two thread groups poll, their sums cross LDS -- not the one-wave leg's shape, the plan keeps the generic instance
    "sixteen_groups_generic": ("fitness", FIT8, 30, {"BB_TUNE_NG": "16"}, 2, 11, K0T8, 0),
}


def run_pair(make_engine, lib, monkeypatch, cid, emu):
    """The case on two handles in one process, the second with BB_TUNE_OPT_SPEC=0; run(4) then run(6) with a window of 4 slots.
    Returns the two states (mu, omega, the three opt_state arrays) after the plan's asserts; None where the product refuses the shape."""
    kind, skw, nb, env, rk, tiles, names, oc = CASES[cid]
    sp = fixtures.synthetic(kind, **skw)
    monkeypatch.setenv("BB_TUNE_NTHR", "1024")
    monkeypatch.setenv("BB_TUNE_NB", str(nb))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if not emu and names[0] is None:
        with pytest.raises(Exception, match="not possible"):
            make_engine(sp, lib, seed=13, window=4, launch_mode=2)
        return None
    outs = []
    for spec in (None, "0"):
        if spec is None:
            monkeypatch.delenv("BB_TUNE_OPT_SPEC", raising=False)
        else:
            monkeypatch.setenv("BB_TUNE_OPT_SPEC", spec)
        with make_engine(sp, lib, seed=13, window=4, launch_mode=2) as e:
            st = e.stats()
            name = e.kernel_name()
            assert name == names[1] if emu else name.startswith(names[0]), name
            assert st["resident_kernel"] == rk and st["n_blocks"] == tiles and st["block_threads"] == 1024, st
            assert st["opt_compiled"] == (oc if spec is None else 0), st
            e.run(4)
            e.run(6)
            assert e.stats()["steps_done"] == 10
            mu, om = e.get_params()
            outs.append((mu, om) + e.opt_state())
    return outs
