"""ctypes binding of include/barbay_hip.h and the `Engine` wrapper the host layer drives.

The product path loads ``lib/libbarbay_hip.so`` (built by ``__graft_entry__.build()`` with hipcc
for gfx950) and raises if it is missing or fails to load -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libbarbay_hip.so")

BB_MODEL = {"fitness": 0, "multienv": 1, "genotype": 2, "replicate": 3, "multienv_replicate": 4}
BB_OPT_TRUNCATED_ADAGRAD = 0
BB_OPT_DECAYED_ADAGRAD = 1
BB_COMM_ID_BYTES = 128
BB_P2P_HANDLE_BYTES = 64
BB_LOGP_MAX_BATCH = 64
BB_HMC_MAX_WALKERS = BB_LOGP_MAX_BATCH
BB_HMC_MAX_LEAPFROG = 1024
BB_HMC_STREAM0 = 0xFFFFFF00
BB_HMC_CHUNK = 2048
BB_HMC_MAX_SEGMENTS = 8
BB_NUTS_MAX_DEPTH = 10
BB_NUTS_EDGE_OPP = -2
BB_NUTS_TAKE_LEAF, BB_NUTS_TAKE_SUB, BB_NUTS_TAKE_STATE = 1, 2, 4
BB_CHAIN_MAX_K = 16384
BB_CHAIN_MAX_Q = 8
BB_CHAIN_LAG_BATCH = 32
BB_TRACE_MAX_SNAPSHOTS = 16384
BB_SCORE_MAX_SAMPLES = 16384
BB_RB_MAX_SAMPLES = 8672
BB_RB_MAX_Q = 8
BB_THETA_RB_CHUNK = 64
BB_POPMEAN_RB_CHUNK = 256
BB_DFE_CHUNK = 128
BB_DFE_MAX_GRID = 64
BB_DFE_MAX_SAMPLES = 8672
BB_RANK_SOURCES = {"conditional": 0, "draws": 1}
BB_RANK_MAX_TOP = 8
BB_RANK_RUN = 8192
BB_RANK_MAX_SAMPLES = 8672
BB_LOGSIGMA_RB_MAX_SAMPLES = 5781
BB_LOGSIGMA_BLOCKS = {"bc": 0, "pop": 1}
BB_LOGTAU_RB_MAX_SAMPLES = 5781
BB_LOGTAU_MODES = {"full": 0, "collapsed": 1}
BB_LOGLAMBDA_RB_MAX_SAMPLES = 5781
BB_MATH_FN = {"exp": 0, "log": 1, "rcp": 2, "div": 3, "sqrt": 4, "softplus_sigmoid": 5, "sincospi": 6, "exp_nonpos": 7, "log_1to2": 8,
              "box_muller": 9}
BB_ERR_UNSUPPORTED = -4
BB_ERR_NONFINITE = -5

EXPORTS = [
    "bb_version", "bb_last_error", "bb_default_opts", "bb_create", "bb_destroy", "bb_num_latents",
    "bb_get_layout", "bb_init_meanfield", "bb_set_params", "bb_get_params", "bb_get_permutation", "bb_get_owned", "bb_run", "bb_run_profiled",
    "bb_get_posterior", "bb_elbo_grad", "bb_logdensity_grad", "bb_logdensity_grad_batch", "bb_hmc_begin", "bb_hmc_step", "bb_hmc_get", "bb_hmc_end",
    "bb_hmc_accum_begin", "bb_hmc_accum_add", "bb_hmc_accum_reset", "bb_hmc_accum_get", "bb_hmc_accum_stats", "bb_hmc_set_metric", "bb_hmc_get_metric",
    "bb_nuts_begin", "bb_nuts_start", "bb_nuts_leaf", "bb_nuts_take",
    "bb_get_elbo_trace", "bb_debug_normals", "bb_debug_math", "bb_debug_stamps", "bb_debug_opt_state", "bb_debug_graph_launches", "bb_get_stats", "bb_kernel_name",
    "bb_comm_make_id", "bb_comm_init", "bb_step_moments", "bb_step_apply", "bb_hier_units", "bb_hier_fitness", "bb_p2p_export", "bb_p2p_import", "bb_p2p_selftest", "bb_p2p_enable",
    "bb_ppc_shape", "bb_ppc_bands", "bb_freq_shape", "bb_freq_bands", "bb_score_shape", "bb_ppc_score", "bb_loo_shape", "bb_ppc_loo", "bb_chain_summary",
    "bb_fitness_rb_shape", "bb_fitness_rb", "bb_theta_rb_shape", "bb_theta_rb", "bb_contrast_rb", "bb_dfe_rb", "bb_fitness_rank", "bb_popmean_rb_shape", "bb_popmean_rb",
    "bb_logsigma_rb_shape", "bb_logsigma_rb", "bb_logtau_rb_shape", "bb_logtau_rb",
    "bb_loglambda_rb_shape", "bb_loglambda_rb",
    "bb_trace_begin", "bb_trace_end", "bb_trace_count", "bb_trace_get", "bb_trace_summary",
]

_dp = C.POINTER(C.c_double)


class bb_prior(C.Structure):
    _fields_ = [("mean", _dp), ("std", _dp), ("n", C.c_int64)]


class bb_model_desc(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("n_rep", C.c_int32), ("n_neutral", C.c_int64), ("n_bc", C.c_int64),
        ("n_time", C.POINTER(C.c_int32)), ("counts", C.POINTER(C.c_int64)), ("totals", C.POINTER(C.c_int64)),
        ("n_env", C.c_int32), ("env_idx", C.POINTER(C.c_int32)),
        ("n_geno", C.c_int32), ("geno_idx", C.POINTER(C.c_int32)),
        ("s_pop_prior", bb_prior), ("logsigma_pop_prior", bb_prior), ("s_bc_prior", bb_prior),
        ("logsigma_bc_prior", bb_prior), ("loglambda_prior", bb_prior), ("logtau_prior", bb_prior),
        ("flags", C.c_int32),
    ]


class bb_advi_opts(C.Structure):
    _fields_ = [
        ("samples_per_step", C.c_int32), ("optimizer", C.c_int32), ("eta", C.c_double), ("tau", C.c_double),
        ("window", C.c_int32), ("resum_every", C.c_int32), ("pre", C.c_double), ("post", C.c_double),
        ("seed", C.c_uint64), ("device", C.c_int32), ("rank", C.c_int32), ("world_size", C.c_int32),
        ("steps_per_graph", C.c_int32), ("elbo_every", C.c_int32), ("launch_mode", C.c_int32),
        ("n_devices", C.c_int32), ("device_ids", C.POINTER(C.c_int32)),
    ]


class bb_hmc_opts(C.Structure):
    _fields_ = [("n_walkers", C.c_int32), ("reserved0", C.c_int32), ("seed", C.c_uint64), ("inv_mass", _dp)]


class bb_hmc_step_opts(C.Structure):
    _fields_ = [("transition", C.c_uint32), ("reserved0", C.c_int32), ("eps", _dp), ("n_leapfrog", C.POINTER(C.c_int32)), ("log_u", _dp)]


class bb_hmc_step_out(C.Structure):
    _fields_ = [("h0", _dp), ("h1", _dp), ("kinetic0", _dp), ("kinetic1", _dp), ("logp_prop", _dp), ("logp", _dp),
                ("accepted", C.POINTER(C.c_int32)), ("divergent", C.POINTER(C.c_int32))]


HMC_STEP_FIELDS = ("h0", "h1", "kinetic0", "kinetic1", "logp_prop", "logp", "accepted", "divergent")


class bb_hmc_accum_opts(C.Structure):
    _fields_ = [("n_segments", C.c_int32), ("reserved0", C.c_int32)]


class bb_hmc_accum_out(C.Structure):
    _fields_ = [("mean", _dp), ("sd", _dp), ("mcse", _dp), ("ess", _dp), ("rhat", _dp), ("within", _dp), ("between", _dp),
                ("n_total", C.POINTER(C.c_int64))]


HMC_ACCUM_FIELDS = ("mean", "sd", "mcse", "ess", "rhat", "within", "between")


class bb_nuts_opts(C.Structure):
    _fields_ = [("max_depth", C.c_int32), ("reserved0", C.c_int32)]


class bb_nuts_leaf_opts(C.Structure):
    _fields_ = [("dir", C.POINTER(C.c_int32)), ("first", C.POINTER(C.c_int32)), ("last", C.POINTER(C.c_int32)), ("store", C.POINTER(C.c_int32)),
                ("n_check", C.POINTER(C.c_int32)), ("check", C.POINTER(C.c_int32)), ("reserved0", C.c_int32)]


class bb_nuts_leaf_out(C.Structure):
    _fields_ = [("logp_leaf", _dp), ("kinetic", _dp), ("a", _dp), ("b", _dp)]


class bb_block_range(C.Structure):
    _fields_ = [("name", C.c_char * 24), ("lo", C.c_int64), ("hi", C.c_int64)]


class bb_stats(C.Structure):
    _fields_ = [
        ("n_latents", C.c_int64), ("n_moments", C.c_int64), ("steps_done", C.c_int64),
        ("shard_lo", C.c_int64), ("shard_hi", C.c_int64), ("bytes_per_step", C.c_int64),
        ("bytes_sample", C.c_int64), ("bytes_update", C.c_int64), ("last_run_ms", C.c_double),
        ("avg_sample_ms", C.c_double), ("avg_update_ms", C.c_double),
        ("n_blocks", C.c_int32), ("block_threads", C.c_int32), ("lds_bytes", C.c_int32),
        ("persistent_pairs", C.c_int32), ("launches_last_run", C.c_int32), ("resident_kernel", C.c_int32),
        ("geno_lo", C.c_int32), ("geno_hi", C.c_int32),
        ("device_bytes", C.c_int64), ("window_row", C.c_int64),
        ("rows_same_xcd", C.c_int32), ("reserved0", C.c_int32),
        ("opt_compiled", C.c_int32), ("reserved1", C.c_int32),
    ]


class bb_ppc_opts(C.Structure):
    _fields_ = [
        ("n_samples", C.c_int32), ("n_ppc", C.c_int32), ("n_quantiles", C.c_int32), ("reserved0", C.c_int32),
        ("quantiles", _dp), ("seed", C.c_uint64),
    ]


BB_FREQ_MODE = {"trajectory": 0, "posterior": 1}


class bb_freq_opts(C.Structure):
    _fields_ = [
        ("mode", C.c_int32), ("n_samples", C.c_int32), ("n_ppc", C.c_int32), ("n_quantiles", C.c_int32),
        ("quantiles", _dp), ("seed", C.c_uint64),
    ]


class bb_score_opts(C.Structure):
    _fields_ = [("n_samples", C.c_int32), ("reserved0", C.c_int32), ("seed", C.c_uint64)]


SCORE_CELLS = ("observed", "pred_mean", "pred_sd", "lpd", "p_waic", "pit", "pit_upper")
SCORE_ROWS = ("row_lpd", "row_p_waic")


class bb_score_out(C.Structure):
    _fields_ = [(k, _dp) for k in SCORE_CELLS + SCORE_ROWS] + [("n_scored", C.POINTER(C.c_int32))]


class bb_loo_opts(C.Structure):
    _fields_ = [("n_samples", C.c_int32), ("reserved0", C.c_int32), ("seed", C.c_uint64)]


BB_LOO_MAX_SAMPLES = 8192
LOO_CELLS = ("elpd_loo", "p_loo", "khat", "n_eff", "lpd")
LOO_ROWS = ("row_elpd_loo", "row_p_loo", "row_khat", "row_n_eff", "row_elpd_cells", "row_khat_max")


class bb_loo_out(C.Structure):
    _fields_ = [(k, _dp) for k in LOO_CELLS + LOO_ROWS] + [("n_scored", C.POINTER(C.c_int32))]


RB_UNITS = ("q_mean", "q_sd", "rb_mean", "rb_sd", "p_pos", "p_neg")


class bb_rb_opts(C.Structure):
    _fields_ = [("n_samples", C.c_int32), ("n_quantiles", C.c_int32), ("probs", _dp), ("threshold", C.c_double), ("seed", C.c_uint64),
                ("draws", _dp)]


class bb_rb_out(C.Structure):
    _fields_ = [(k, _dp) for k in RB_UNITS] + [("quantiles", _dp), ("n_steps", C.POINTER(C.c_int32))]


class bb_theta_rb_out(C.Structure):
    _fields_ = [(k, _dp) for k in RB_UNITS] + [("quantiles", _dp), ("n_members", C.POINTER(C.c_int32)), ("n_steps", C.POINTER(C.c_int32))]


BB_CONTRAST_SPACES = {"fitness": 0, "theta": 1}


class bb_contrast_opts(C.Structure):
    _fields_ = [("space", C.c_int32), ("n_samples", C.c_int32), ("n_quantiles", C.c_int32), ("reserved0", C.c_int32), ("probs", _dp),
                ("threshold", C.c_double), ("seed", C.c_uint64), ("draws", _dp), ("n_contrasts", C.c_int64),
                ("term_ptr", C.POINTER(C.c_int64)), ("term_idx", C.POINTER(C.c_int64)), ("term_w", _dp)]


class bb_contrast_out(C.Structure):
    _fields_ = [(k, _dp) for k in RB_UNITS] + [("quantiles", _dp), ("min_steps", C.POINTER(C.c_int32))]


DFE_CELLS = ("below_mean", "above_mean", "between_sd", "within_sd", "q_below_mean", "q_below_sd")
DFE_BANDS = ("below_bands", "above_bands")


class bb_dfe_opts(C.Structure):
    _fields_ = [("n_samples", C.c_int32), ("n_quantiles", C.c_int32), ("n_grid", C.c_int32), ("reserved0", C.c_int32), ("probs", _dp),
                ("grid", _dp), ("seed", C.c_uint64), ("draws", _dp), ("n_sets", C.c_int64),
                ("set_ptr", C.POINTER(C.c_int64)), ("set_idx", C.POINTER(C.c_int64))]


class bb_dfe_out(C.Structure):
    _fields_ = [(k, _dp) for k in DFE_CELLS + DFE_BANDS] + [("n_units", C.POINTER(C.c_int64))]


class bb_rank_opts(C.Structure):
    _fields_ = [("n_samples", C.c_int32), ("n_quantiles", C.c_int32), ("n_top", C.c_int32), ("source", C.c_int32), ("reserved0", C.c_int32),
                ("reserved1", C.c_int32), ("probs", _dp), ("top", C.POINTER(C.c_int64)), ("seed", C.c_uint64), ("draws", _dp), ("n_sets", C.c_int64),
                ("set_ptr", C.POINTER(C.c_int64)), ("set_idx", C.POINTER(C.c_int64))]


class bb_rank_out(C.Structure):
    _fields_ = [("rank_mean", _dp), ("rank_sd", _dp), ("p_top", _dp), ("quantiles", _dp), ("ranks", C.POINTER(C.c_int32)),
                ("n_units", C.POINTER(C.c_int64))]


class bb_popmean_rb_out(C.Structure):
    _fields_ = [(k, _dp) for k in RB_UNITS] + [("quantiles", _dp), ("n_members", C.POINTER(C.c_int32))]


LS_UNITS = ("q_mean", "q_sd", "rb_mean", "rb_sd", "sigma_mean", "mode_mean")


class bb_logsigma_rb_opts(C.Structure):
    _fields_ = [("block", C.c_int32), ("n_samples", C.c_int32), ("n_quantiles", C.c_int32), ("reserved0", C.c_int32), ("probs", _dp),
                ("seed", C.c_uint64), ("draws", _dp)]


class bb_logsigma_rb_out(C.Structure):
    _fields_ = [(k, _dp) for k in LS_UNITS] + [("quantiles", _dp), ("n_terms", C.POINTER(C.c_int32))]


LT_UNITS = ("q_mean", "q_sd", "rb_mean", "rb_sd", "tau_mean", "pool_mean", "mode_mean")


class bb_logtau_rb_opts(C.Structure):
    _fields_ = [("mode", C.c_int32), ("n_samples", C.c_int32), ("n_quantiles", C.c_int32), ("reserved0", C.c_int32), ("probs", _dp),
                ("seed", C.c_uint64), ("draws", _dp)]


class bb_logtau_rb_out(C.Structure):
    _fields_ = [(k, _dp) for k in LT_UNITS] + [("quantiles", _dp), ("n_terms", C.POINTER(C.c_int32)), ("n_two_modes", C.POINTER(C.c_int32))]


LL_UNITS = ("q_mean", "q_sd", "rb_mean", "rb_sd", "lambda_mean", "mode_mean")


class bb_loglambda_rb_opts(C.Structure):
    _fields_ = [("n_samples", C.c_int32), ("n_quantiles", C.c_int32), ("probs", _dp), ("seed", C.c_uint64), ("draws", _dp),
                ("rows", C.POINTER(C.c_int64)), ("n_rows", C.c_int64)]


class bb_loglambda_rb_out(C.Structure):
    _fields_ = [(k, _dp) for k in LL_UNITS] + [("quantiles", _dp), ("n_reads", C.POINTER(C.c_int64)), ("n_sides", C.POINTER(C.c_int32))]


class bb_chain_opts(C.Structure):
    _fields_ = [
        ("n_chains", C.c_int32), ("n_draws", C.c_int32), ("n_quantiles", C.c_int32), ("max_lag", C.c_int32),
        ("probs", _dp), ("slab_cols", C.c_int64),
    ]


class bb_chain_out(C.Structure):
    _fields_ = [
        ("mean", _dp), ("sd", _dp), ("mcse", _dp), ("ess", _dp), ("rhat", _dp), ("quantiles", _dp),
        ("n_lags", C.POINTER(C.c_int32)),
    ]


class bb_trace_opts(C.Structure):
    _fields_ = [("every", C.c_int32), ("capacity", C.c_int32)]


class bb_trace_sum_opts(C.Structure):
    _fields_ = [
        ("first", C.c_int64), ("n_chains", C.c_int32), ("n_draws", C.c_int32), ("max_lag", C.c_int32), ("reserved0", C.c_int32),
        ("slab_cols", C.c_int64), ("rhat_max", C.c_double),
    ]


TRACE_COLS = ("mean", "sd", "mcse", "ess", "rhat")
TRACE_BLOCK_COUNTS = ("n_cols", "n_nonfinite", "n_const", "n_above")
TRACE_BLOCK_VALUES = ("max_rhat", "min_ess", "max_mcse_rel")


class bb_trace_block(C.Structure):
    _fields_ = ([("name", C.c_char * 24), ("part", C.c_int32), ("reserved0", C.c_int32)] + [(k, C.c_int64) for k in TRACE_BLOCK_COUNTS]
                + [(k, C.c_double) for k in TRACE_BLOCK_VALUES])


class bb_trace_sum_out(C.Structure):
    _fields_ = [(k, _dp) for k in TRACE_COLS] + [("n_lags", C.POINTER(C.c_int32)), ("blocks", C.POINTER(bb_trace_block))]


class BarBayHipError(RuntimeError):
    """Raised for any non-zero status of the C ABI (the reference throws ErrorException)."""


class BarBayNonFinite(BarBayHipError):
    """bb_run took its steps but the variational parameters went NaN / Inf (BB_ERR_NONFINITE); the state can still be read."""


def _declare(lib: C.CDLL) -> C.CDLL:
    vp = C.c_void_p
    lib.bb_version.restype = C.c_char_p
    lib.bb_last_error.restype = C.c_char_p
    lib.bb_default_opts.argtypes = [C.POINTER(bb_advi_opts)]
    lib.bb_default_opts.restype = None
    lib.bb_create.argtypes = [C.POINTER(bb_model_desc), C.POINTER(bb_advi_opts), C.POINTER(vp)]
    lib.bb_destroy.argtypes = [vp]
    lib.bb_destroy.restype = None
    lib.bb_num_latents.argtypes = [vp]
    lib.bb_num_latents.restype = C.c_int64
    lib.bb_get_layout.argtypes = [vp, C.POINTER(bb_block_range), C.POINTER(C.c_int32)]
    lib.bb_init_meanfield.argtypes = [vp]
    lib.bb_set_params.argtypes = [vp, _dp, _dp]
    lib.bb_get_params.argtypes = [vp, _dp, _dp]
    if hasattr(lib, "bb_get_permutation"):      # (A/B builds of older sources, tools/xp.py)
        lib.bb_get_permutation.argtypes = [vp, C.POINTER(C.c_int64)]
    if hasattr(lib, "bb_get_owned"):
        lib.bb_get_owned.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.bb_run.argtypes = [vp, C.c_int64]
    lib.bb_run_profiled.argtypes = [vp, C.c_int64]
    lib.bb_get_posterior.argtypes = [vp, _dp, _dp]
    lib.bb_elbo_grad.argtypes = [vp, _dp, _dp, _dp, C.c_int32, _dp, _dp, _dp]
    lib.bb_logdensity_grad.argtypes = [vp, _dp, _dp, _dp]
    lib.bb_logdensity_grad_batch.argtypes = [vp, C.c_int32, _dp, _dp, _dp]
    if hasattr(lib, "bb_hmc_begin"):            # (A/B builds of older sources, tools/xp.py)
        lib.bb_hmc_begin.argtypes = [vp, C.POINTER(bb_hmc_opts), _dp, _dp]
        lib.bb_hmc_step.argtypes = [vp, C.POINTER(bb_hmc_step_opts), C.POINTER(bb_hmc_step_out)]
        lib.bb_hmc_get.argtypes = [vp, _dp, _dp, _dp]
        lib.bb_hmc_end.argtypes = [vp]
    if hasattr(lib, "bb_hmc_accum_begin"):
        lib.bb_hmc_accum_begin.argtypes = [vp, C.POINTER(bb_hmc_accum_opts)]
        lib.bb_hmc_accum_add.argtypes = [vp, C.POINTER(C.c_int32)]
        lib.bb_hmc_accum_reset.argtypes = [vp]
        lib.bb_hmc_accum_get.argtypes = [vp, C.c_int32, C.c_int32, _dp, _dp, C.POINTER(C.c_int64)]
        lib.bb_hmc_accum_stats.argtypes = [vp, C.POINTER(bb_hmc_accum_out)]
        lib.bb_hmc_set_metric.argtypes = [vp, _dp]
        lib.bb_hmc_get_metric.argtypes = [vp, _dp]
    if hasattr(lib, "bb_nuts_begin"):
        lib.bb_nuts_begin.argtypes = [vp, C.POINTER(bb_nuts_opts)]
        lib.bb_nuts_start.argtypes = [vp, C.c_uint32, _dp, C.POINTER(C.c_int32), _dp]
        lib.bb_nuts_leaf.argtypes = [vp, C.POINTER(bb_nuts_leaf_opts), C.POINTER(bb_nuts_leaf_out)]
        lib.bb_nuts_take.argtypes = [vp, C.POINTER(C.c_int32)]
    lib.bb_get_elbo_trace.argtypes = [vp, C.c_int64, C.c_int64, _dp]
    lib.bb_debug_normals.argtypes = [vp, C.c_int64, C.c_uint32, C.c_int64, C.c_int64, _dp]
    if hasattr(lib, "bb_debug_math"):           # (A/B builds of older sources, tools/xp.py)
        lib.bb_debug_math.argtypes = [vp, C.c_int32, C.c_int64, _dp, _dp, _dp, _dp]
    lib.bb_get_stats.argtypes = [vp, C.POINTER(bb_stats)]
    if hasattr(lib, "bb_kernel_name"):          # (A/B builds of older sources, tools/xp.py)
        lib.bb_kernel_name.argtypes = [vp, C.c_char_p, C.c_int64]
    lib.bb_debug_stamps.argtypes = [vp, C.POINTER(C.c_uint64), C.c_int64]
    if hasattr(lib, "bb_debug_opt_state"):      # (A/B builds of older sources, tools/xp.py)
        lib.bb_debug_opt_state.argtypes = [vp, _dp, _dp, C.POINTER(C.c_float)]
    lib.bb_debug_graph_launches.argtypes = [vp]
    lib.bb_comm_make_id.argtypes = [C.c_void_p]
    lib.bb_comm_init.argtypes = [vp, C.c_void_p]
    lib.bb_step_moments.argtypes = [vp, _dp]
    lib.bb_step_apply.argtypes = [vp, _dp]
    lib.bb_p2p_export.argtypes = [vp, C.c_void_p]
    lib.bb_p2p_import.argtypes = [vp, C.c_void_p]
    lib.bb_p2p_selftest.argtypes = [vp, C.POINTER(C.c_int32)]
    lib.bb_p2p_enable.argtypes = [vp, C.c_int32]
    lib.bb_hier_units.argtypes = [vp]
    lib.bb_hier_units.restype = C.c_int64
    lib.bb_hier_fitness.argtypes = [vp, C.c_int32, C.c_uint64, _dp, _dp]
    if hasattr(lib, "bb_ppc_bands"):            # (A/B builds of older sources, tools/xp.py)
        lib.bb_ppc_shape.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
        lib.bb_ppc_bands.argtypes = [vp, C.POINTER(bb_ppc_opts), _dp, C.POINTER(C.c_int64)]
    if hasattr(lib, "bb_freq_bands"):
        lib.bb_freq_shape.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
        lib.bb_freq_bands.argtypes = [vp, C.POINTER(bb_freq_opts), _dp, C.POINTER(C.c_int64)]
    if hasattr(lib, "bb_ppc_score"):
        lib.bb_score_shape.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
        lib.bb_ppc_score.argtypes = [vp, C.POINTER(bb_score_opts), C.POINTER(bb_score_out)]
    if hasattr(lib, "bb_ppc_loo"):
        lib.bb_loo_shape.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
        lib.bb_ppc_loo.argtypes = [vp, C.POINTER(bb_loo_opts), C.POINTER(bb_loo_out)]
    if hasattr(lib, "bb_fitness_rb"):
        lib.bb_fitness_rb_shape.argtypes = [vp, C.POINTER(C.c_int64)]
        lib.bb_fitness_rb.argtypes = [vp, C.POINTER(bb_rb_opts), C.POINTER(bb_rb_out)]
    if hasattr(lib, "bb_theta_rb"):
        lib.bb_theta_rb_shape.argtypes = [vp, C.POINTER(C.c_int64)]
        lib.bb_theta_rb.argtypes = [vp, C.POINTER(bb_rb_opts), C.POINTER(bb_theta_rb_out)]
    if hasattr(lib, "bb_contrast_rb"):
        lib.bb_contrast_rb.argtypes = [vp, C.POINTER(bb_contrast_opts), C.POINTER(bb_contrast_out)]
    if hasattr(lib, "bb_dfe_rb"):
        lib.bb_dfe_rb.argtypes = [vp, C.POINTER(bb_dfe_opts), C.POINTER(bb_dfe_out)]
    if hasattr(lib, "bb_fitness_rank"):
        lib.bb_fitness_rank.argtypes = [vp, C.POINTER(bb_rank_opts), C.POINTER(bb_rank_out)]
    if hasattr(lib, "bb_popmean_rb"):
        lib.bb_popmean_rb_shape.argtypes = [vp, C.POINTER(C.c_int64)]
        lib.bb_popmean_rb.argtypes = [vp, C.POINTER(bb_rb_opts), C.POINTER(bb_popmean_rb_out)]
    if hasattr(lib, "bb_logsigma_rb"):
        lib.bb_logsigma_rb_shape.argtypes = [vp, C.c_int32, C.POINTER(C.c_int64)]
        lib.bb_logsigma_rb.argtypes = [vp, C.POINTER(bb_logsigma_rb_opts), C.POINTER(bb_logsigma_rb_out)]
    if hasattr(lib, "bb_logtau_rb"):
        lib.bb_logtau_rb_shape.argtypes = [vp, C.POINTER(C.c_int64)]
        lib.bb_logtau_rb.argtypes = [vp, C.POINTER(bb_logtau_rb_opts), C.POINTER(bb_logtau_rb_out)]
    if hasattr(lib, "bb_loglambda_rb"):
        lib.bb_loglambda_rb_shape.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
        lib.bb_loglambda_rb.argtypes = [vp, C.POINTER(bb_loglambda_rb_opts), C.POINTER(bb_loglambda_rb_out)]
    if hasattr(lib, "bb_chain_summary"):
        lib.bb_chain_summary.argtypes = [vp, C.POINTER(bb_chain_opts), C.c_int64, _dp, C.POINTER(bb_chain_out)]
    if hasattr(lib, "bb_trace_begin"):
        lib.bb_trace_begin.argtypes = [vp, C.POINTER(bb_trace_opts)]
        lib.bb_trace_end.argtypes = [vp]
        lib.bb_trace_count.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        lib.bb_trace_get.argtypes = [vp, C.c_int64, C.c_int64, _dp, _dp]
        lib.bb_trace_summary.argtypes = [vp, C.POINTER(bb_trace_sum_opts), C.POINTER(bb_trace_sum_out)]
    return lib


_LIB: Optional[C.CDLL] = None


def load_library(path: Optional[str] = None) -> C.CDLL:
    """Load the HIP engine.  No fallback: a missing/unloadable library is an error."""
    global _LIB
    if path is None and _LIB is not None:
        return _LIB
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise BarBayHipError(
            f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    try:
        import torch  # noqa: F401  (loads its libamdhip64.so.7 first so both share one HIP runtime)
    except Exception:
        pass
    lib = _declare(C.CDLL(p))
    if path is None:
        _LIB = lib
    return lib


def _f64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64)


def _ptr(a: np.ndarray, ty=_dp):
    return a.ctypes.data_as(ty)


class HmcSession:
    """What `Engine.hmc_begin` returns: `logp` [W] at the start points; ends the session when used as a context manager."""

    def __init__(self, engine: "Engine", logp: np.ndarray):
        self.engine, self.logp = engine, logp

    def __enter__(self):
        return self

    def __exit__(self, *a):
        if getattr(self.engine, "_h", None) is not None and self.engine._h.value:
            self.engine.hmc_end()


class Engine:
    """One model instance on one GPU (`bb_handle`).

    counts: list (one per replicate) of T_r x B int64 arrays, neutrals first.
    priors: name -> (mean, std), floats (Vector form) or 1-D arrays (Matrix form); names
    s_pop_prior, logsigma_pop_prior, s_bc_prior, logsigma_bc_prior, loglambda_prior, logtau_prior.
    """

    def __init__(self, kind: str, counts: Sequence[np.ndarray], n_neutral: int, n_bc: int, *,
                 totals: Optional[Sequence[np.ndarray]] = None, env_idx=None, geno_idx=None,
                 priors: Optional[Dict[str, Tuple[object, object]]] = None,
                 samples_per_step: int = 1, optimizer: str = "TruncatedADAGrad", eta: float = 0.1,
                 tau: float = 40.0, window: int = 100, resum_every: int = 0, pre: float = 1.0,
                 post: float = 0.9, seed: int = 0, device: int = 0, rank: int = 0, world_size: int = 1,
                 steps_per_graph: int = 0, elbo_every: int = 0, launch_mode: int = 0, ragged_method: bool = False,
                 n_devices: int = 1, device_ids: Optional[Sequence[int]] = None, _lib: Optional[C.CDLL] = None):
        self._lib = _lib if _lib is not None else load_library()
        self._h = C.c_void_p()
        self.kind = kind
        counts = [np.asarray(c, dtype=np.int64) for c in counts]
        if totals is None:
            totals = [c.sum(axis=1) for c in counts]
        totals = [np.asarray(t, dtype=np.int64) for t in totals]
        keep: List[np.ndarray] = []   # arrays the descriptor points into, alive for the bb_create call

        def hold(a):
            keep.append(a)
            return a

        md = bb_model_desc()
        md.kind = BB_MODEL[kind]
        md.n_rep = len(counts)
        md.n_neutral = int(n_neutral)
        md.flags = 1 if ragged_method else 0      # BB_FLAG_RAGGED_METHOD
        md.n_bc = int(n_bc)
        nt = hold(np.asarray([c.shape[0] for c in counts], dtype=np.int32))
        md.n_time = _ptr(nt, C.POINTER(C.c_int32))
        # Julia column-major T x B (t fastest) == C-order of the transpose
        cflat = hold(np.concatenate([np.ascontiguousarray(c.T).reshape(-1) for c in counts]).astype(np.int64))
        tflat = hold(np.concatenate(totals).astype(np.int64))
        md.counts = _ptr(cflat, C.POINTER(C.c_int64))
        md.totals = _ptr(tflat, C.POINTER(C.c_int64))
        if env_idx is not None:
            if isinstance(env_idx, (list, tuple)) and len(env_idx) and np.ndim(env_idx[0]) == 1:
                env_idx = np.concatenate([np.asarray(x) for x in env_idx])     # one list per replicate -> replicate-major
            e = hold(np.ascontiguousarray(env_idx, dtype=np.int32))
            md.n_env = int(e.max()) + 1
            md.env_idx = _ptr(e, C.POINTER(C.c_int32))
        if geno_idx is not None:
            g = hold(np.ascontiguousarray(geno_idx, dtype=np.int32))
            md.n_geno = int(g.max()) + 1
            md.geno_idx = _ptr(g, C.POINTER(C.c_int32))
        for name, (mean, std) in (priors or {}).items():
            m = hold(np.atleast_1d(_f64(mean)))
            s = hold(np.atleast_1d(_f64(std)))
            if m.shape != s.shape or m.ndim != 1:
                raise BarBayHipError(f"{name}: mean/std must be scalars or equal-length vectors")
            p = getattr(md, name)
            p.mean, p.std, p.n = _ptr(m), _ptr(s), m.shape[0]
        o = bb_advi_opts()
        self._lib.bb_default_opts(C.byref(o))
        o.samples_per_step = samples_per_step
        o.optimizer = {"TruncatedADAGrad": 0, "DecayedADAGrad": 1}[optimizer]
        o.eta, o.tau, o.window, o.resum_every, o.pre, o.post = eta, tau, window, resum_every, pre, post
        o.seed, o.device, o.rank, o.world_size = seed, device, rank, world_size
        o.steps_per_graph, o.elbo_every, o.launch_mode = steps_per_graph, elbo_every, launch_mode
        if device_ids is not None:
            n_devices = len(device_ids)
            ids = hold(np.ascontiguousarray(device_ids, dtype=np.int32))
            o.device_ids = _ptr(ids, C.POINTER(C.c_int32))
        o.n_devices = int(n_devices)
        self._check(self._lib.bb_create(C.byref(md), C.byref(o), C.byref(self._h)))
        self.D = int(self._lib.bb_num_latents(self._h))
        self.samples_per_step = samples_per_step
        self.world_size, self.rank = world_size, rank

    # -- plumbing -------------------------------------------------------------------------------
    def _check(self, rc: int):
        if rc == BB_ERR_NONFINITE:
            raise BarBayNonFinite(f"barbay_hip error {rc}: {self._lib.bb_last_error().decode()}")
        if rc != 0:
            raise BarBayHipError(f"barbay_hip error {rc}: {self._lib.bb_last_error().decode()}")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.bb_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- API ------------------------------------------------------------------------------------
    def layout(self) -> List[Tuple[str, int, int]]:
        blocks = (bb_block_range * 8)()
        n = C.c_int32()
        self._check(self._lib.bb_get_layout(self._h, blocks, C.byref(n)))
        return [(blocks[i].name.decode(), int(blocks[i].lo), int(blocks[i].hi)) for i in range(n.value)]

    def init_meanfield(self):
        self._check(self._lib.bb_init_meanfield(self._h))

    def set_params(self, mu, omega):
        mu, omega = _f64(mu), _f64(omega)
        assert mu.shape == (self.D,) and omega.shape == (self.D,)
        self._check(self._lib.bb_set_params(self._h, _ptr(mu), _ptr(omega)))

    def get_params(self) -> Tuple[np.ndarray, np.ndarray]:
        mu, om = np.empty(self.D), np.empty(self.D)
        self._check(self._lib.bb_get_params(self._h, _ptr(mu), _ptr(om)))
        return mu, om

    def permutation(self) -> np.ndarray:
        """caller_index[i] of the handle's internal latent i (identity unless the genotype model's mutants were regrouped)."""
        out = np.empty(self.D, dtype=np.int64)
        self._check(self._lib.bb_get_permutation(self._h, out.ctypes.data_as(C.POINTER(C.c_int64))))
        return out

    def owned(self) -> np.ndarray:
        """The caller's flat indices of the latents this handle owns on a sharded run (`bb_get_owned`): its barcodes' latents and,
        genotype model, theta of its own genotypes -- not the replicated global blocks."""
        out = np.empty(self.D, dtype=np.int64)
        n = C.c_int64(0)
        self._check(self._lib.bb_get_owned(self._h, out.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(n)))
        return out[:n.value].copy()

    def run(self, n_steps: int):
        self._check(self._lib.bb_run(self._h, int(n_steps)))

    def run_profiled(self, n_steps: int):
        self._check(self._lib.bb_run_profiled(self._h, int(n_steps)))

    def posterior(self) -> Tuple[np.ndarray, np.ndarray]:
        m, s = np.empty(self.D), np.empty(self.D)
        self._check(self._lib.bb_get_posterior(self._h, _ptr(m), _ptr(s)))
        return m, s

    def elbo_grad(self, mu, omega, eps=None, n_samples: Optional[int] = None):
        mu, omega = _f64(mu), _f64(omega)
        if eps is not None:
            eps = np.atleast_2d(_f64(eps))
            assert eps.shape[1] == self.D
            n_samples = eps.shape[0]
        n_samples = n_samples or 1
        gm, go = np.empty(self.D), np.empty(self.D)
        elbo = C.c_double()
        self._check(self._lib.bb_elbo_grad(self._h, _ptr(mu), _ptr(omega), _ptr(eps) if eps is not None else None,
                                           n_samples, C.byref(elbo), _ptr(gm), _ptr(go)))
        return elbo.value, gm, go

    def elbo_trace(self, first_step: int, n: int) -> np.ndarray:
        out = np.empty(n)
        self._check(self._lib.bb_get_elbo_trace(self._h, first_step, n, _ptr(out)))
        return out

    def normals(self, step: int, stream: int, lo: int, hi: int) -> np.ndarray:
        out = np.empty(hi - lo)
        self._check(self._lib.bb_debug_normals(self._h, step, stream, lo, hi, _ptr(out)))
        return out

    def debug_math(self, fn, x, y=None) -> Tuple[np.ndarray, Optional[np.ndarray]]:
        """One function of the kernels' fp64 math header, or the Box-Muller step, on the device at the arguments x (and y), for
        accuracy checks (`bb_debug_math`): fn is a name of BB_MATH_FN or its number.  Returns (out0, out1), out1 None for the
        functions of one result.  box_muller takes the two 64-bit words as uint64 arrays."""
        code = BB_MATH_FN[fn] if isinstance(fn, str) else int(fn)
        words = code == BB_MATH_FN["box_muller"]
        x = np.ascontiguousarray(x, dtype=np.uint64).view(np.float64) if words else _f64(x)
        if y is not None:
            y = np.ascontiguousarray(y, dtype=np.uint64).view(np.float64) if words else _f64(y)
            assert y.shape == x.shape
        assert x.ndim == 1
        out0 = np.empty(x.shape[0])
        out1 = np.empty(x.shape[0]) if code in (BB_MATH_FN["softplus_sigmoid"], BB_MATH_FN["sincospi"], BB_MATH_FN["box_muller"]) else None
        self._check(self._lib.bb_debug_math(self._h, code, x.shape[0], _ptr(x), _ptr(y) if y is not None else None, _ptr(out0),
                                            _ptr(out1) if out1 is not None else None))
        return out0, out1

    def stamps(self, per_wave: bool = False) -> np.ndarray:
        """Diagnostic build only: [tiles][32] block stamps, or with per_wave [tiles][4 events][16 waves]."""
        nb = int(self.stats()["n_blocks"])
        rows = np.zeros(1, dtype=np.uint64)
        self._check(self._lib.bb_debug_stamps(self._h, rows.ctypes.data_as(C.POINTER(C.c_uint64)), -1))
        rows = int(rows[0])
        raw = np.zeros(rows * 96, dtype=np.uint64)
        self._check(self._lib.bb_debug_stamps(self._h, raw.ctypes.data_as(C.POINTER(C.c_uint64)), raw.size))
        if not per_wave:
            return raw[:nb * 32].reshape(nb, 32).copy()
        return raw[rows * 32:rows * 32 + nb * 64].reshape(nb, 4, 16).copy()

    def graph_launches(self) -> int:
        """hipGraphLaunch calls of the last `run` (`bb_debug_graph_launches`); 0 on a resident launch, an eager run and the emulation."""
        return int(self._lib.bb_debug_graph_launches(self._h))

    def stats(self) -> Dict[str, float]:
        s = bb_stats()
        self._check(self._lib.bb_get_stats(self._h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in bb_stats._fields_}

    def kernel_name(self) -> str:
        """The kernel `run` launches, as text: the template instance, e.g. 'k_res<0,1,1024,false,8,false,false>' (`bb_kernel_name`)."""
        buf = C.create_string_buffer(128)
        self._check(self._lib.bb_kernel_name(self._h, buf, 128))
        return buf.value.decode()

    def opt_state(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Test hook (`bb_debug_opt_state`): the optimiser's accumulators of mu and omega [D] and the low-order parts of the compensated
        window sums [D, 2] (float32), in the handle's internal latent order."""
        am, ao, lo = np.empty(self.D), np.empty(self.D), np.empty((self.D, 2), dtype=np.float32)
        self._check(self._lib.bb_debug_opt_state(self._h, _ptr(am), _ptr(ao), lo.ctypes.data_as(C.POINTER(C.c_float))))
        return am, ao, lo

    def logdensity_grad(self, z) -> Tuple[float, np.ndarray]:
        """log p(data, z) and its gradient at a point of the flat latent vector (`bb_logdensity_grad`)."""
        z = np.ascontiguousarray(z, dtype=np.float64)
        assert z.shape == (self.D,)
        lp = C.c_double(0.0)
        g = np.empty(self.D)
        self._check(self._lib.bb_logdensity_grad(self._h, _ptr(z), C.byref(lp), _ptr(g)))
        return lp.value, g

    def logdensity_grad_batch(self, Z) -> Tuple[np.ndarray, np.ndarray]:
        """log p(data, z_w) and its gradient at W <= BB_LOGP_MAX_BATCH points in one call (`bb_logdensity_grad_batch`): Z is
        [W, D], or [D] for one point; returns (logp[W], grad[W, D]).  Each row's result is a function of that row alone."""
        Z = np.ascontiguousarray(Z, dtype=np.float64)
        if Z.ndim == 1:
            Z = Z[None, :]
        assert Z.ndim == 2 and Z.shape[1] == self.D
        W = Z.shape[0]
        lp = np.empty(W)
        g = np.empty((W, self.D))
        self._check(self._lib.bb_logdensity_grad_batch(self._h, W, _ptr(Z), _ptr(lp), _ptr(g)))
        return lp, g

    def hmc_begin(self, z0, *, seed: int = 0, inv_mass=None) -> "HmcSession":
        """Opens the device-resident HMC session (`bb_hmc_begin`): z0 is [W, D] (or [D]), W <= BB_HMC_MAX_WALKERS walkers whose position,
        momentum and gradient stay on the device until `hmc_end`; `inv_mass` [D] is the diagonal metric (None: ones), `seed` the key of the
        momentum draws.  Returns the session, whose `logp` holds log p at z0 (a non-finite value is reported, not raised); it is a context
        manager that ends the session on exit.  A second `hmc_begin` replaces the session."""
        z0 = np.ascontiguousarray(z0, dtype=np.float64)
        if z0.ndim == 1:
            z0 = z0[None, :]
        assert z0.ndim == 2 and z0.shape[1] == self.D
        o = bb_hmc_opts()
        o.n_walkers, o.reserved0, o.seed = z0.shape[0], 0, int(seed)
        if inv_mass is not None:
            inv_mass = _f64(inv_mass)
            assert inv_mass.shape == (self.D,)
            o.inv_mass = _ptr(inv_mass)
        lp = np.empty(z0.shape[0])
        self._check(self._lib.bb_hmc_begin(self._h, C.byref(o), _ptr(z0), _ptr(lp)))
        self._hmc_W = z0.shape[0]
        return HmcSession(self, lp)

    def hmc_step(self, transition: int, eps, n_leapfrog, log_u) -> Dict[str, np.ndarray]:
        """One HMC transition of every walker of the session (`bb_hmc_step`): `eps`, `n_leapfrog`, `log_u` are [W] (scalars are
        broadcast); walker w's momenta are the engine's normals (i, step=transition, stream=BB_HMC_STREAM0 + w).  Returns h0, h1,
        kinetic0, kinetic1, logp_prop, logp (of the state held after the call), accepted, divergent, each [W]."""
        W = self._hmc_W
        eps = _f64(np.broadcast_to(np.asarray(eps, dtype=np.float64), (W,)))
        nl = np.ascontiguousarray(np.broadcast_to(np.asarray(n_leapfrog), (W,)), dtype=np.int32)
        lu = _f64(np.broadcast_to(np.asarray(log_u, dtype=np.float64), (W,)))
        ip = C.POINTER(C.c_int32)
        o = bb_hmc_step_opts()
        o.transition, o.reserved0, o.eps, o.n_leapfrog, o.log_u = int(transition), 0, _ptr(eps), _ptr(nl, ip), _ptr(lu)
        res = {k: np.empty(W, dtype=np.int32 if k in ("accepted", "divergent") else np.float64) for k in HMC_STEP_FIELDS}
        out = bb_hmc_step_out()
        for k in HMC_STEP_FIELDS:
            setattr(out, k, _ptr(res[k], ip if res[k].dtype == np.int32 else _dp))
        self._check(self._lib.bb_hmc_step(self._h, C.byref(o), C.byref(out)))
        return res

    def hmc_get(self, grad: bool = False):
        """The walkers' current positions [W, D] and log-densities [W] (`bb_hmc_get`); with `grad`, the gradients [W, D] too."""
        W = self._hmc_W
        z, lp = np.empty((W, self.D)), np.empty(W)
        g = np.empty((W, self.D)) if grad else None
        self._check(self._lib.bb_hmc_get(self._h, _ptr(z), _ptr(lp), _ptr(g) if grad else None))
        return (z, lp, g) if grad else (z, lp)

    def hmc_end(self):
        self._check(self._lib.bb_hmc_end(self._h))

    def hmc_accum_begin(self, n_segments: int = 1):
        """Running moments of the session's state on the device (`bb_hmc_accum_begin`): per walker and segment < `n_segments`
        (<= BB_HMC_MAX_SEGMENTS) a mean and an m2 row, zeroed.  A second call replaces them; `hmc_begin` and `hmc_end` drop them."""
        o = bb_hmc_accum_opts()
        o.n_segments, o.reserved0 = int(n_segments), 0
        self._check(self._lib.bb_hmc_accum_begin(self._h, C.byref(o)))

    def hmc_accum_add(self, segment=0):
        """One Welford step of every walker's current state into its `segment` [W] (a scalar broadcasts; -1: the walker is not added)."""
        seg = np.ascontiguousarray(np.broadcast_to(np.asarray(segment), (self._hmc_W,)), dtype=np.int32)
        self._check(self._lib.bb_hmc_accum_add(self._h, _ptr(seg, C.POINTER(C.c_int32))))

    def hmc_accum_reset(self):
        self._check(self._lib.bb_hmc_accum_reset(self._h))

    def hmc_accum_get(self, w: int, s: int):
        """(mean [D], m2 [D], n) of walker `w`'s segment `s` (`bb_hmc_accum_get`)."""
        mean, m2, n = np.empty(self.D), np.empty(self.D), C.c_int64(0)
        self._check(self._lib.bb_hmc_accum_get(self._h, int(w), int(s), _ptr(mean), _ptr(m2), C.byref(n)))
        return mean, m2, int(n.value)

    def hmc_accum_stats(self) -> Dict[str, np.ndarray]:
        """Pooled statistics of everything added (`bb_hmc_accum_stats`): mean, sd, mcse, ess, rhat, within, between, each [D], and n_total.
        `ess` is a batch-means estimate over the live (walker, segment) chains, not Geyer's (include/barbay_hip.h)."""
        res = {k: np.empty(self.D) for k in HMC_ACCUM_FIELDS}
        n = C.c_int64(0)
        out = bb_hmc_accum_out()
        for k in HMC_ACCUM_FIELDS:
            setattr(out, k, _ptr(res[k]))
        out.n_total = C.pointer(n)
        self._check(self._lib.bb_hmc_accum_stats(self._h, C.byref(out)))
        res["n_total"] = int(n.value)
        return res

    def hmc_set_metric(self, inv_mass=None):
        """Replaces the session's diagonal metric (`bb_hmc_set_metric`; None: ones); positions, gradients and accumulators stay."""
        if inv_mass is not None:
            inv_mass = _f64(inv_mass)
            assert inv_mass.shape == (self.D,)
        self._check(self._lib.bb_hmc_set_metric(self._h, _ptr(inv_mass) if inv_mass is not None else None))

    def hmc_get_metric(self) -> np.ndarray:
        im = np.empty(self.D)
        self._check(self._lib.bb_hmc_get_metric(self._h, _ptr(im)))
        return im

    def nuts_begin(self, max_depth: int = BB_NUTS_MAX_DEPTH):
        """The rows of a No-U-Turn tree beside the open session (`bb_nuts_begin`): per walker both edges of the trajectory, the subtree's and
        the transition's candidate and `max_depth` (<= BB_NUTS_MAX_DEPTH) U-turn checkpoints.  `hmc_begin` and `hmc_end` drop them."""
        o = bb_nuts_opts()
        o.max_depth, o.reserved0 = int(max_depth), 0
        self._check(self._lib.bb_nuts_begin(self._h, C.byref(o)))
        self._nuts_depth = int(max_depth)

    def nuts_start(self, transition: int, eps, live=1) -> np.ndarray:
        """A NUTS transition begins for the walkers with `live` [W] != 0 (`bb_nuts_start`): `hmc_step`'s momenta of `transition`, the state to
        both edges.  Returns kinetic0 [W] (0 for a walker that is not live)."""
        W = self._hmc_W
        eps = _f64(np.broadcast_to(np.asarray(eps, dtype=np.float64), (W,)))
        lv = np.ascontiguousarray(np.broadcast_to(np.asarray(live), (W,)), dtype=np.int32)
        k0 = np.empty(W)
        self._check(self._lib.bb_nuts_start(self._h, int(transition), _ptr(eps), _ptr(lv, C.POINTER(C.c_int32)), _ptr(k0)))
        return k0

    def nuts_leaf(self, dir, first, last, store, checks) -> Dict[str, np.ndarray]:
        """One leaf of every walker with `dir` [W] != 0 (`bb_nuts_leaf`): `first` / `last` [W] flag the ends of its doubling, `store` [W] is -1
        or the checkpoint slot that takes the leaf, `checks` a list per walker of the stored points to test against (slots, or
        BB_NUTS_EDGE_OPP).  Returns logp_leaf, kinetic [W] and a, b [W, max_depth + 1] (0 beyond a walker's checks)."""
        W, ip = self._hmc_W, C.POINTER(C.c_int32)
        i32 = lambda v: np.ascontiguousarray(np.broadcast_to(np.asarray(v), (W,)), dtype=np.int32)
        d, f, l, st = i32(dir), i32(first), i32(last), i32(store)
        nc = np.array([len(c) for c in checks], dtype=np.int32)
        ck = np.zeros((W, BB_NUTS_MAX_DEPTH + 1), dtype=np.int32)
        for w, c in enumerate(checks):
            ck[w, :min(len(c), BB_NUTS_MAX_DEPTH + 1)] = list(c)[:BB_NUTS_MAX_DEPTH + 1]
        o = bb_nuts_leaf_opts()
        o.dir, o.first, o.last, o.store, o.n_check, o.check, o.reserved0 = _ptr(d, ip), _ptr(f, ip), _ptr(l, ip), _ptr(st, ip), _ptr(nc, ip), _ptr(ck, ip), 0
        n = self._nuts_depth + 1
        res = {"logp_leaf": np.empty(W), "kinetic": np.empty(W), "a": np.empty((W, n)), "b": np.empty((W, n))}
        out = bb_nuts_leaf_out()
        for k, v in res.items():
            setattr(out, k, _ptr(v))
        self._check(self._lib.bb_nuts_leaf(self._h, C.byref(o), C.byref(out)))
        return res

    def nuts_take(self, flags):
        """The copies `flags` [W] ask for (`bb_nuts_take`; BB_NUTS_TAKE_LEAF: leaf -> subtree candidate, BB_NUTS_TAKE_SUB: subtree candidate ->
        transition candidate, BB_NUTS_TAKE_STATE: transition candidate -> the session's state), applied in that order."""
        fl = np.ascontiguousarray(np.broadcast_to(np.asarray(flags), (self._hmc_W,)), dtype=np.int32)
        self._check(self._lib.bb_nuts_take(self._h, _ptr(fl, C.POINTER(C.c_int32))))

    def hier_units(self) -> int:
        """Length of the theta_tilde block (0 for the non-hierarchical models)."""
        return int(self._lib.bb_hier_units(self._h))

    def hier_fitness(self, n_samples: int = 10_000, seed: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """Device-side `process_hierarchical_samples!`: (median, std) of theta + exp(logtau) * theta_tilde per unit."""
        n = int(self._lib.bb_hier_units(self._h))
        med, sd = np.empty(n), np.empty(n)
        self._check(self._lib.bb_hier_fitness(self._h, n_samples, seed, _ptr(med), _ptr(sd)))
        return med, sd

    def ppc_shape(self) -> Tuple[int, int]:
        """(n_rows, n_steps) of `ppc_bands`: n_rep population-mean rows, then n_rep * n_bc mutant rows (replicate-major)."""
        n, t = C.c_int64(0), C.c_int32(0)
        self._check(self._lib.bb_ppc_shape(self._h, C.byref(n), C.byref(t)))
        return int(n.value), int(t.value)

    def ppc_bands(self, quantiles: Sequence[float], n_samples: int = 1000, n_ppc: int = 10, seed: int = 0,
                  outside: bool = True) -> Tuple[np.ndarray, Optional[np.ndarray]]:
        """Posterior predictive bands of the log-frequency ratios for every row (`bb_ppc_bands`): bands[n_rows, n_steps, n_q, 2]
        (lower, upper; NaN past a shorter replicate's last step) and, with `outside`, the per-row count of observed ratios outside
        the band of the largest q."""
        q = _f64(np.atleast_1d(quantiles))
        n_rows, n_steps = self.ppc_shape()
        o = bb_ppc_opts()
        o.n_samples, o.n_ppc, o.n_quantiles, o.seed = int(n_samples), int(n_ppc), int(q.shape[0]), int(seed)
        o.quantiles = _ptr(q)
        bands = np.empty((n_rows, n_steps, q.shape[0], 2))
        nout = np.zeros(n_rows, dtype=np.int64) if outside else None
        self._check(self._lib.bb_ppc_bands(self._h, C.byref(o), _ptr(bands),
                                           nout.ctypes.data_as(C.POINTER(C.c_int64)) if outside else None))
        return bands, nout

    def freq_shape(self) -> Tuple[int, int]:
        """(n_rows, n_cols) of `freq_bands`: n_rep * (n_neutral + n_bc) rows (replicate-major, data columns: neutrals first) and
        max_r T_r time points."""
        n, t = C.c_int64(0), C.c_int32(0)
        self._check(self._lib.bb_freq_shape(self._h, C.byref(n), C.byref(t)))
        return int(n.value), int(t.value)

    def freq_bands(self, quantiles: Sequence[float], mode="trajectory", n_samples: int = 1000, n_ppc: int = 10, seed: int = 0,
                   outside: bool = True) -> Tuple[np.ndarray, Optional[np.ndarray]]:
        """Bands of the frequency of every barcode at every time point (`bb_freq_bands`): bands[n_rows, n_cols, n_q, 2] (lower, upper;
        NaN past a shorter replicate's last time point) and, with `outside`, the per-row count of observed frequencies outside the
        band of the largest q.  mode "trajectory": the predictive trajectories f_{t+1} = f_t exp(N(s - sbar_t, sigma)) from the draws'
        initial frequencies; "posterior" (n_ppc = 1): the posterior of the model's own frequencies exp(loglambda) / sum."""
        q = _f64(np.atleast_1d(quantiles))
        n_rows, n_cols = self.freq_shape()
        o = bb_freq_opts()
        o.mode = BB_FREQ_MODE[mode] if isinstance(mode, str) else int(mode)
        o.n_samples, o.n_ppc, o.n_quantiles, o.seed = int(n_samples), int(n_ppc), int(q.shape[0]), int(seed)
        o.quantiles = _ptr(q)
        bands = np.empty((n_rows, n_cols, q.shape[0], 2))
        nout = np.zeros(n_rows, dtype=np.int64) if outside else None
        self._check(self._lib.bb_freq_bands(self._h, C.byref(o), _ptr(bands),
                                            nout.ctypes.data_as(C.POINTER(C.c_int64)) if outside else None))
        return bands, nout

    def score_shape(self) -> Tuple[int, int]:
        """(n_rows, n_steps) of `ppc_score`: the rows of `freq_bands` (n_rep * (n_neutral + n_bc), replicate-major, data columns:
        neutrals first) and max_r T_r - 1 steps."""
        n, t = C.c_int64(0), C.c_int32(0)
        self._check(self._lib.bb_score_shape(self._h, C.byref(n), C.byref(t)))
        return int(n.value), int(t.value)

    def ppc_score(self, n_samples: int = 1000, seed: int = 0) -> Dict[str, np.ndarray]:
        """Predictive log score and PIT of every observed log-frequency ratio (`bb_ppc_score`), the predictive density and CDF
        averaged over the posterior draws in closed form.  Returns observed, pred_mean, pred_sd, lpd, p_waic, pit, pit_upper, each
        [n_rows, n_steps] (NaN: no such step, or a zero count), and row_lpd, row_p_waic, n_scored (int32), each [n_rows]."""
        n_rows, n_steps = self.score_shape()
        o = bb_score_opts()
        o.n_samples, o.seed = int(n_samples), int(seed)
        res = {k: np.empty((n_rows, n_steps)) for k in SCORE_CELLS}
        res.update({k: np.empty(n_rows) for k in SCORE_ROWS})
        res["n_scored"] = np.empty(n_rows, dtype=np.int32)
        out = bb_score_out()
        for k in SCORE_CELLS + SCORE_ROWS:
            setattr(out, k, _ptr(res[k]))
        out.n_scored = res["n_scored"].ctypes.data_as(C.POINTER(C.c_int32))
        self._check(self._lib.bb_ppc_score(self._h, C.byref(o), C.byref(out)))
        return res

    def loo_shape(self) -> Tuple[int, int]:
        """(n_rows, n_steps) of `ppc_loo`: those of `ppc_score`."""
        n, t = C.c_int64(0), C.c_int32(0)
        self._check(self._lib.bb_loo_shape(self._h, C.byref(n), C.byref(t)))
        return int(n.value), int(t.value)

    def ppc_loo(self, n_samples: int = 1000, seed: int = 0) -> Dict[str, np.ndarray]:
        """Pareto-smoothed importance-sampling leave-one-out scores of every observed log-frequency ratio (`bb_ppc_loo`), on the
        draws and log densities of `ppc_score`.  Returns elpd_loo, p_loo, khat, n_eff, lpd, each [n_rows, n_steps] (NaN: no such
        step, or a zero count; khat = +Inf: too few draws, or too light a tail, to smooth), the barcode's whole trajectory left
        out: row_elpd_loo, row_p_loo, row_khat, row_n_eff, and row_elpd_cells, row_khat_max, n_scored (int32), each [n_rows].
        n_samples <= 8192."""
        n_rows, n_steps = self.loo_shape()
        o = bb_loo_opts()
        o.n_samples, o.seed = int(n_samples), int(seed)
        res = {k: np.empty((n_rows, n_steps)) for k in LOO_CELLS}
        res.update({k: np.empty(n_rows) for k in LOO_ROWS})
        res["n_scored"] = np.empty(n_rows, dtype=np.int32)
        out = bb_loo_out()
        for k in LOO_CELLS + LOO_ROWS:
            setattr(out, k, _ptr(res[k]))
        out.n_scored = res["n_scored"].ctypes.data_as(C.POINTER(C.c_int32))
        self._check(self._lib.bb_ppc_loo(self._h, C.byref(o), C.byref(out)))
        return res

    def fitness_rb_shape(self) -> int:
        """Fitness units of `fitness_rb`: u = e + E m + E n_bc r (replicate, mutant in the caller's order, environment) -- the order
        of the s_bc block (fitness, multienv) or the theta_tilde block (hierarchical kinds)."""
        n = C.c_int64(0)
        self._check(self._lib.bb_fitness_rb_shape(self._h, C.byref(n)))
        return int(n.value)

    def fitness_rb(self, n_samples: int = 1000, probs: Sequence[float] = (0.025, 0.5, 0.975), threshold: float = 0.0, seed: int = 0,
                   draws=None) -> Dict[str, np.ndarray]:
        """Rao-Blackwellised marginal of every fitness unit (`bb_fitness_rb`): the unit's exact Gaussian full conditional averaged
        over `n_samples` joint draws of everything else -- the posterior's own draws (those of `ppc_bands` at equal seed), or the
        rows of `draws` [n, D] in the caller's order (an MCMC chain; `n_samples` is then its row count).  Returns n_steps (int32),
        q_mean, q_sd (the draws' own fitness), rb_mean, rb_sd, p_pos, p_neg (the RB probability of a fitness above / below
        `threshold`), each [n_units], and quantiles [n_units, len(probs)] of the RB mixture at the probabilities `probs`."""
        n_units = self.fitness_rb_shape()
        o, p, _x = self._rb_opts(n_samples, probs, threshold, seed, draws)
        res = {k: np.empty(n_units) for k in RB_UNITS}
        res["quantiles"] = np.empty((n_units, p.shape[0]))
        res["n_steps"] = np.empty(n_units, dtype=np.int32)
        out = bb_rb_out()
        for k in RB_UNITS:
            setattr(out, k, _ptr(res[k]))
        out.quantiles = _ptr(res["quantiles"]) if p.shape[0] else None
        out.n_steps = res["n_steps"].ctypes.data_as(C.POINTER(C.c_int32))
        self._check(self._lib.bb_fitness_rb(self._h, C.byref(o), C.byref(out)))
        return res

    def _rb_opts(self, n_samples, probs, threshold, seed, draws, opts=bb_rb_opts):
        """(bb_rb_opts, probs, draws): the arrays the options point into must outlive the call."""
        p = _f64(np.atleast_1d(probs)).reshape(-1)
        o = opts()
        o.n_samples, o.n_quantiles, o.seed = int(n_samples), int(p.shape[0]), int(seed)
        if threshold is not None:                     # (bb_dfe_opts has none)
            o.threshold = float(threshold)
        o.probs = _ptr(p) if p.shape[0] else None
        x = None
        if draws is not None:
            x = np.ascontiguousarray(draws, dtype=np.float64)
            if x.ndim == 1:
                x = x[None, :]
            if x.ndim != 2 or x.shape[1] != self.D:
                raise BarBayHipError(f"draws must be [n_samples, {self.D}]")
            o.n_samples = x.shape[0]
            o.draws = _ptr(x)
        return o, p, x

    def theta_rb_shape(self) -> int:
        """Groups of `theta_rb`: the length of the theta block (genotypes; e + E m for the replicate kinds); 0 for the
        non-hierarchical kinds."""
        n = C.c_int64(0)
        self._check(self._lib.bb_theta_rb_shape(self._h, C.byref(n)))
        return int(n.value)

    def theta_rb(self, n_samples: int = 1000, probs: Sequence[float] = (0.025, 0.5, 0.975), threshold: float = 0.0, seed: int = 0,
                 draws=None) -> Dict[str, np.ndarray]:
        """Rao-Blackwellised marginal of every hyper-fitness theta_g of a hierarchical model (`bb_theta_rb`): its exact Gaussian
        full conditional -- the prior and the log-frequency-ratio terms of the group's members, a genotype's mutants or a mutant's
        replicates -- averaged over the draws of `fitness_rb` (same arguments).  Returns what `fitness_rb` returns, per group
        (n_steps: the members' steps together), plus n_members (int32)."""
        n_groups = self.theta_rb_shape()
        o, p, _x = self._rb_opts(n_samples, probs, threshold, seed, draws)
        res = {k: np.empty(n_groups) for k in RB_UNITS}
        res["quantiles"] = np.empty((n_groups, p.shape[0]))
        res["n_steps"] = np.empty(n_groups, dtype=np.int32)
        res["n_members"] = np.empty(n_groups, dtype=np.int32)
        out = bb_theta_rb_out()
        for k in RB_UNITS:
            setattr(out, k, _ptr(res[k]))
        out.quantiles = _ptr(res["quantiles"]) if p.shape[0] else None
        out.n_steps = res["n_steps"].ctypes.data_as(C.POINTER(C.c_int32))
        out.n_members = res["n_members"].ctypes.data_as(C.POINTER(C.c_int32))
        self._check(self._lib.bb_theta_rb(self._h, C.byref(o), C.byref(out)))
        return res

    def contrast_rb(self, terms, space: str = "fitness", n_samples: int = 1000, probs: Sequence[float] = (0.025, 0.5, 0.975),
                    threshold: float = 0.0, seed: int = 0, draws=None) -> Dict[str, np.ndarray]:
        """Rao-Blackwellised marginal of linear contrasts sum_k w_k x_k of distinct fitness units (`space="fitness"`, the units of
        `fitness_rb`) or distinct hyper-fitnesses (`space="theta"`, the groups of `theta_rb`) (`bb_contrast_rb`): the contrast's exact
        Gaussian conditional N(sum w m, sqrt(sum w^2 sd^2)) averaged over the draws of `fitness_rb` (same arguments), so that what
        the terms share -- the population mean fitness above all -- cancels or adds up draw by draw.  `terms`: a sequence of
        contrasts, each a sequence of (index, weight), or a CSR triple (ptr, idx, w).  Returns what `fitness_rb` returns, per
        contrast, with min_steps (int32, the smallest n_steps over the contrast's terms) in place of n_steps."""
        if space not in BB_CONTRAST_SPACES:
            raise BarBayHipError(f"space must be one of {sorted(BB_CONTRAST_SPACES)}")
        if isinstance(terms, tuple) and len(terms) == 3 and np.ndim(terms[0]) == 1 and len(terms[0]) > 0:
            ptr, idx, w = terms                       # (a contrast is a sequence of pairs: two-dimensional, or empty)
        else:
            terms = [list(c) for c in terms]
            ptr = np.cumsum([0] + [len(c) for c in terms])
            idx = [k for c in terms for k, _ in c]
            w = [x for c in terms for _, x in c]
        ptr = np.ascontiguousarray(ptr, dtype=np.int64).reshape(-1)
        idx = np.ascontiguousarray(idx, dtype=np.int64).reshape(-1)
        w = _f64(np.asarray(w, dtype=np.float64)).reshape(-1)
        if ptr.shape[0] < 1 or idx.shape[0] != w.shape[0] or (ptr.shape[0] > 1 and ptr[-1] != idx.shape[0]):
            raise BarBayHipError("terms: ptr must have n_contrasts + 1 entries ending at the number of terms, idx and w that many entries")
        n = ptr.shape[0] - 1
        o, p, _x = self._rb_opts(n_samples, probs, threshold, seed, draws, opts=bb_contrast_opts)
        o.space, o.n_contrasts = BB_CONTRAST_SPACES[space], n
        i64 = C.POINTER(C.c_int64)
        o.term_ptr, o.term_idx, o.term_w = ptr.ctypes.data_as(i64), idx.ctypes.data_as(i64), _ptr(w)
        res = {k: np.empty(n) for k in RB_UNITS}
        res["quantiles"] = np.empty((n, p.shape[0]))
        res["min_steps"] = np.empty(n, dtype=np.int32)
        out = bb_contrast_out()
        for k in RB_UNITS:
            setattr(out, k, _ptr(res[k]))
        out.quantiles = _ptr(res["quantiles"]) if p.shape[0] else None
        out.min_steps = res["min_steps"].ctypes.data_as(C.POINTER(C.c_int32))
        self._check(self._lib.bb_contrast_rb(self._h, C.byref(o), C.byref(out)))
        return res

    def dfe_rb(self, sets, grid, *, probs: Sequence[float] = (0.025, 0.5, 0.975), n_samples: int = 1000, seed: int = 0, draws=None,
               _slab_tables: int = 0) -> Dict[str, np.ndarray]:
        """Posterior of the distribution of fitness effects of sets of fitness units (`bb_dfe_rb`): per set and threshold x of
        `grid` (finite, strictly ascending, at most BB_DFE_MAX_GRID) the fraction of the set's units at or below (above) x, averaged
        over the draws of `fitness_rb` (same `n_samples`, `seed`, `draws`) with each unit's exact Gaussian conditional in place of its
        draw, so that what the units share -- the population mean fitness above all -- moves the whole curve draw by draw.  `sets`:
        a list of index sequences (the units of `fitness_rb`, each at most once per set), or a CSR pair as a tuple (ptr, idx).  Returns
        below_mean, above_mean, between_sd (sd over the draws of the conditional fraction below x), within_sd (sqrt of the mean
        conditional, Poisson-binomial, variance; the total variance of the fraction is between_sd^2 + within_sd^2), q_below_mean,
        q_below_sd (the draws' own ECDF at x), each [n_sets, n_grid]; below_bands, above_bands [n_sets, n_grid, len(probs)], the
        `probs` quantiles over the draws of the two conditional fractions; n_units [n_sets] (int64).  `_slab_tables`: tests only."""
        if isinstance(sets, tuple) and len(sets) == 2:
            ptr, idx = sets                           # (a tuple is the CSR pair; a list of two index lists is two sets)
        else:
            sets = [np.asarray(c, dtype=np.int64).reshape(-1) for c in sets]
            ptr = np.cumsum([0] + [len(c) for c in sets])
            idx = np.concatenate(sets) if sets else np.zeros(0, dtype=np.int64)
        ptr = np.ascontiguousarray(ptr, dtype=np.int64).reshape(-1)
        idx = np.ascontiguousarray(idx, dtype=np.int64).reshape(-1)
        if ptr.shape[0] < 1 or (ptr.shape[0] > 1 and ptr[-1] != idx.shape[0]):
            raise BarBayHipError("sets: ptr must have n_sets + 1 entries ending at the number of indices")
        n = ptr.shape[0] - 1
        x = _f64(np.atleast_1d(grid)).reshape(-1)
        o, p, _x = self._rb_opts(n_samples, probs, None, seed, draws, opts=bb_dfe_opts)
        o.n_grid, o.grid, o.n_sets, o.reserved0 = x.shape[0], _ptr(x) if x.shape[0] else None, n, int(_slab_tables)
        i64 = C.POINTER(C.c_int64)
        idx_ = idx if idx.shape[0] else np.zeros(1, dtype=np.int64)
        o.set_ptr, o.set_idx = ptr.ctypes.data_as(i64), idx_.ctypes.data_as(i64)
        res = {k: np.empty((n, x.shape[0])) for k in DFE_CELLS}
        res.update({k: np.empty((n, x.shape[0], p.shape[0])) for k in DFE_BANDS})
        res["n_units"] = np.empty(n, dtype=np.int64)
        out = bb_dfe_out()
        for k in DFE_CELLS:
            setattr(out, k, _ptr(res[k]))
        for k in DFE_BANDS:
            setattr(out, k, _ptr(res[k]) if p.shape[0] else None)
        out.n_units = res["n_units"].ctypes.data_as(i64)
        self._check(self._lib.bb_dfe_rb(self._h, C.byref(o), C.byref(out)))
        return res

    def fitness_rank(self, sets, *, top: Sequence[int] = (1, 10), probs: Sequence[float] = (0.025, 0.5, 0.975), source: str = "conditional",
                     n_samples: int = 1000, seed: int = 0, draws=None, want_ranks: bool = False, _run: int = 0,
                     _bound_kib: int = 0) -> Dict[str, np.ndarray]:
        """Posterior ranks of the fitness units of sets and their top-k membership (`bb_fitness_rank`): per joint draw of
        `fitness_rb` (same `n_samples`, `seed`, `draws`) every unit is redrawn from its exact Gaussian conditional
        (`source="conditional"`: one blocked Gibbs update of the fitness block, so that what the units share moves them together) or
        taken as the draw's own fitness (`source="draws"`), and ranked within each set: larger is fitter, rank 0 the fittest, a NaN
        after every number, ties by the caller's order.  `sets` as for `dfe_rb`.  Results are indexed by position in the
        concatenated sets: rank_mean, rank_sd [n_idx]; p_top [n_idx, len(top)], the fraction of the draws with rank < top[i];
        quantiles [n_idx, len(probs)] over the draws of the rank; n_units [n_sets] (int64); set_ptr [n_sets + 1] (int64); with
        `want_ranks` ranks [n_idx, n_samples] (int32).  `_run`, `_bound_kib`: tests only."""
        if source not in BB_RANK_SOURCES:
            raise BarBayHipError(f"source must be one of {sorted(BB_RANK_SOURCES)}")
        if isinstance(sets, tuple) and len(sets) == 2:
            ptr, idx = sets                           # (a tuple is the CSR pair; a list of two index lists is two sets)
        else:
            sets = [np.asarray(c, dtype=np.int64).reshape(-1) for c in sets]
            ptr = np.cumsum([0] + [len(c) for c in sets])
            idx = np.concatenate(sets) if sets else np.zeros(0, dtype=np.int64)
        ptr = np.ascontiguousarray(ptr, dtype=np.int64).reshape(-1)
        idx = np.ascontiguousarray(idx, dtype=np.int64).reshape(-1)
        if ptr.shape[0] < 1 or (ptr.shape[0] > 1 and ptr[-1] != idx.shape[0]):
            raise BarBayHipError("sets: ptr must have n_sets + 1 entries ending at the number of indices")
        n, nix = ptr.shape[0] - 1, idx.shape[0]
        t = np.ascontiguousarray(np.atleast_1d(top), dtype=np.int64).reshape(-1)
        o, p, _x = self._rb_opts(n_samples, probs, None, seed, draws, opts=bb_rank_opts)
        i64 = C.POINTER(C.c_int64)
        o.n_top, o.top, o.source = t.shape[0], t.ctypes.data_as(i64) if t.shape[0] else None, BB_RANK_SOURCES[source]
        o.reserved0, o.reserved1, o.n_sets = int(_run), int(_bound_kib), n
        idx_ = idx if nix else np.zeros(1, dtype=np.int64)
        o.set_ptr, o.set_idx = ptr.ctypes.data_as(i64), idx_.ctypes.data_as(i64)
        res = {"rank_mean": np.empty(nix), "rank_sd": np.empty(nix), "p_top": np.empty((nix, t.shape[0])), "quantiles": np.empty((nix, p.shape[0])),
               "n_units": np.empty(n, dtype=np.int64), "set_ptr": ptr.copy()}
        out = bb_rank_out()
        out.rank_mean, out.rank_sd = _ptr(res["rank_mean"]), _ptr(res["rank_sd"])
        out.p_top = _ptr(res["p_top"]) if t.shape[0] and nix else None
        out.quantiles = _ptr(res["quantiles"]) if p.shape[0] and nix else None
        out.n_units = res["n_units"].ctypes.data_as(i64)
        if want_ranks:
            res["ranks"] = np.empty((nix, int(o.n_samples)), dtype=np.int32)
            out.ranks = res["ranks"].ctypes.data_as(C.POINTER(C.c_int32))
        self._check(self._lib.bb_fitness_rank(self._h, C.byref(o), C.byref(out)))
        return res

    def popmean_rb_shape(self) -> int:
        """Groups of `popmean_rb`: the length of the s_pop block, g = (replicate, step), replicate-major."""
        n = C.c_int64(0)
        self._check(self._lib.bb_popmean_rb_shape(self._h, C.byref(n)))
        return int(n.value)

    def popmean_rb(self, n_samples: int = 1000, probs: Sequence[float] = (0.025, 0.5, 0.975), threshold: float = 0.0, seed: int = 0,
                   draws=None) -> Dict[str, np.ndarray]:
        """Rao-Blackwellised marginal of every population mean fitness sbar_g (`bb_popmean_rb`): its exact Gaussian full
        conditional -- the prior and the log-frequency-ratio terms of every barcode of the replicate at the step, neutrals and
        mutants -- averaged over the draws of `fitness_rb` (same arguments).  Returns q_mean, q_sd, rb_mean, rb_sd, p_pos, p_neg
        [n_groups], quantiles [n_groups, len(probs)] and n_members (int32: neutrals + mutants)."""
        n_groups = self.popmean_rb_shape()
        o, p, _x = self._rb_opts(n_samples, probs, threshold, seed, draws)
        res = {k: np.empty(n_groups) for k in RB_UNITS}
        res["quantiles"] = np.empty((n_groups, p.shape[0]))
        res["n_members"] = np.empty(n_groups, dtype=np.int32)
        out = bb_popmean_rb_out()
        for k in RB_UNITS:
            setattr(out, k, _ptr(res[k]))
        out.quantiles = _ptr(res["quantiles"]) if p.shape[0] else None
        out.n_members = res["n_members"].ctypes.data_as(C.POINTER(C.c_int32))
        self._check(self._lib.bb_popmean_rb(self._h, C.byref(o), C.byref(out)))
        return res

    @staticmethod
    def _logsigma_block(block) -> int:
        if block not in BB_LOGSIGMA_BLOCKS:
            raise BarBayHipError(f"block must be one of {sorted(BB_LOGSIGMA_BLOCKS)}, got {block!r}")
        return BB_LOGSIGMA_BLOCKS[block]

    def logsigma_rb_shape(self, block: str = "bc") -> int:
        """Entries of `logsigma_rb`: the length of the logsigma_bc ("bc") or logsigma_pop ("pop") block."""
        n = C.c_int64(0)
        self._check(self._lib.bb_logsigma_rb_shape(self._h, self._logsigma_block(block), C.byref(n)))
        return int(n.value)

    def logsigma_rb(self, block: str = "bc", n_samples: int = 1000, probs: Sequence[float] = (0.025, 0.5, 0.975), seed: int = 0,
                    draws=None) -> Dict[str, np.ndarray]:
        """Rao-Blackwellised marginal of every noise scale of a block (`bb_logsigma_rb`): "bc" the logsigma_bc entries (the units of
        `fitness_rb`), "pop" the logsigma_pop entries (the groups of `popmean_rb`).  The full conditional of a log-scale is
        one-dimensional and log-concave; it is integrated numerically per draw and averaged over the draws of `fitness_rb` (same
        arguments).  Returns q_mean, q_sd, rb_mean, rb_sd, sigma_mean (the RB mean of sigma itself), mode_mean [n_entries],
        quantiles [n_entries, len(probs)] (of logsigma; their exp are sigma's) and n_terms (int32)."""
        blk = self._logsigma_block(block)
        n_entries = self.logsigma_rb_shape(block)
        ro, p, _x = self._rb_opts(n_samples, probs, 0.0, seed, draws)
        o = bb_logsigma_rb_opts()
        o.block, o.n_samples, o.n_quantiles, o.probs, o.seed, o.draws = blk, ro.n_samples, ro.n_quantiles, ro.probs, ro.seed, ro.draws
        res = {k: np.empty(n_entries) for k in LS_UNITS}
        res["quantiles"] = np.empty((n_entries, p.shape[0]))
        res["n_terms"] = np.empty(n_entries, dtype=np.int32)
        out = bb_logsigma_rb_out()
        for k in LS_UNITS:
            setattr(out, k, _ptr(res[k]))
        out.quantiles = _ptr(res["quantiles"]) if p.shape[0] else None
        out.n_terms = res["n_terms"].ctypes.data_as(C.POINTER(C.c_int32))
        self._check(self._lib.bb_logsigma_rb(self._h, C.byref(o), C.byref(out)))
        return res

    def logtau_rb_shape(self) -> int:
        """Entries of `logtau_rb`: the length of the logtau block (0 for the kinds that have none)."""
        n = C.c_int64(0)
        self._check(self._lib.bb_logtau_rb_shape(self._h, C.byref(n)))
        return int(n.value)

    def logtau_rb(self, mode: str = "collapsed", n_samples: int = 1000, probs: Sequence[float] = (0.025, 0.5, 0.975), seed: int = 0,
                  draws=None) -> Dict[str, np.ndarray]:
        """Rao-Blackwellised marginal of every logtau of a hierarchical model (`bb_logtau_rb`; the entries are the units of
        `fitness_rb`).  `mode="full"`: the full conditional given everything else, theta_tilde included; `mode="collapsed"`: with
        theta_tilde integrated out against its prior -- the hierarchical-variance posterior.  Neither is log-concave and either can
        have two modes; it is integrated numerically per draw on one grid over all of them and averaged over the draws of
        `fitness_rb` (same arguments).  Returns q_mean, q_sd, rb_mean, rb_sd, tau_mean (the RB mean of tau itself), pool_mean (of
        1 / (1 + n w tau^2): 1 pooled onto the group, 0 on its own), mode_mean [n_entries], quantiles [n_entries, len(probs)] (of
        logtau; their exp are tau's), n_terms and n_two_modes (int32: the draws whose conditional kept two modes)."""
        if mode not in BB_LOGTAU_MODES:
            raise BarBayHipError(f"mode must be one of {sorted(BB_LOGTAU_MODES)}, got {mode!r}")
        ro, p, _x = self._rb_opts(n_samples, probs, 0.0, seed, draws)
        o = bb_logtau_rb_opts()
        o.mode, o.n_samples, o.n_quantiles, o.probs, o.seed, o.draws = BB_LOGTAU_MODES[mode], ro.n_samples, ro.n_quantiles, ro.probs, ro.seed, ro.draws
        n_entries = self.logtau_rb_shape()
        res = {k: np.empty(n_entries) for k in LT_UNITS}
        res["quantiles"] = np.empty((n_entries, p.shape[0]))
        res["n_terms"] = np.empty(n_entries, dtype=np.int32)
        res["n_two_modes"] = np.empty(n_entries, dtype=np.int32)
        out = bb_logtau_rb_out()
        for k in LT_UNITS:
            setattr(out, k, _ptr(res[k]))
        out.quantiles = _ptr(res["quantiles"]) if p.shape[0] else None
        out.n_terms = res["n_terms"].ctypes.data_as(C.POINTER(C.c_int32))
        out.n_two_modes = res["n_two_modes"].ctypes.data_as(C.POINTER(C.c_int32))
        self._check(self._lib.bb_logtau_rb(self._h, C.byref(o), C.byref(out)))
        return res

    def loglambda_rb_shape(self) -> Tuple[int, int]:
        """(n_rows, n_cols) of `loglambda_rb`: the rows and time points of `freq_bands`."""
        n, c = C.c_int64(0), C.c_int32(0)
        self._check(self._lib.bb_loglambda_rb_shape(self._h, C.byref(n), C.byref(c)))
        return int(n.value), int(c.value)

    def loglambda_rb(self, n_samples: int = 1000, probs: Sequence[float] = (0.025, 0.5, 0.975), seed: int = 0, draws=None,
                     rows=None) -> Dict[str, np.ndarray]:
        """Rao-Blackwellised marginal of the log-rates loglambda (`bb_loglambda_rb`), per (row, time point) of `freq_bands`: the
        full conditional of a log-rate -- its prior, its Poisson term and the ratio terms of the steps its time point bounds, those
        of every other barcode through the row normaliser -- is one-dimensional, skewed for low counts and not necessarily
        log-concave; it is integrated numerically per draw on one grid over all its modes and averaged over the draws of
        `fitness_rb` (same arguments).  `rows`: the rows wanted, strictly ascending (all).  Returns q_mean, q_sd, rb_mean, rb_sd,
        lambda_mean (the RB mean of lambda itself), mode_mean [n_rows, n_cols], quantiles [n_rows, n_cols, len(probs)], n_reads
        (int64, the observed count) and n_sides (int32: the steps bounding the time point); cells past a shorter replicate's last
        time point are NaN / 0."""
        ro, p, _x = self._rb_opts(n_samples, probs, 0.0, seed, draws)
        o = bb_loglambda_rb_opts()
        o.n_samples, o.n_quantiles, o.probs, o.seed, o.draws = ro.n_samples, ro.n_quantiles, ro.probs, ro.seed, ro.draws
        n_rows, n_cols = self.loglambda_rb_shape()
        rr = None
        if rows is not None:
            rr = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
            o.rows, o.n_rows = rr.ctypes.data_as(C.POINTER(C.c_int64)), rr.shape[0]
            if rr.shape[0] == 0:                      # (an empty array has no address to give)
                o.rows = (C.c_int64 * 1)()
            n_rows = rr.shape[0]
        res = {k: np.empty((n_rows, n_cols)) for k in LL_UNITS}
        res["quantiles"] = np.empty((n_rows, n_cols, p.shape[0]))
        res["n_reads"] = np.empty((n_rows, n_cols), dtype=np.int64)
        res["n_sides"] = np.empty((n_rows, n_cols), dtype=np.int32)
        out = bb_loglambda_rb_out()
        for k in LL_UNITS:
            setattr(out, k, _ptr(res[k]))
        out.quantiles = _ptr(res["quantiles"]) if p.shape[0] else None
        out.n_reads = res["n_reads"].ctypes.data_as(C.POINTER(C.c_int64))
        out.n_sides = res["n_sides"].ctypes.data_as(C.POINTER(C.c_int32))
        self._check(self._lib.bb_loglambda_rb(self._h, C.byref(o), C.byref(out)))
        return res

    def chain_summary(self, chain, probs: Sequence[float] = (0.025, 0.25, 0.5, 0.75, 0.975), max_lag: int = 0,
                      slab_cols: int = 0) -> Dict[str, np.ndarray]:
        """Chain diagnostics of every column of a host chain (`bb_chain_summary`): `chain` is [W, N, D], or [N, D] for one chain;
        D need not be the model's latent count.  Returns mean, sd, mcse, ess (Geyer's initial monotone sequence), rhat (split-R-hat),
        each [D]; quantiles [D, len(probs)] (StatsBase.quantile of the pooled draws at the probabilities `probs`); n_lags [D] (int32,
        the lags that entered the ESS sum).  `max_lag` > 0 bounds that sum; `slab_cols` > 0 sets the columns uploaded per slab."""
        x = np.ascontiguousarray(chain, dtype=np.float64)
        if x.ndim == 2:
            x = x[None, :, :]
        if x.ndim != 3:
            raise BarBayHipError("chain must be [n_chains, n_draws, n_cols] or [n_draws, n_cols]")
        W, N, D = x.shape
        p = _f64(np.atleast_1d(probs)).reshape(-1)
        o = bb_chain_opts()
        o.n_chains, o.n_draws, o.n_quantiles, o.max_lag, o.slab_cols = W, N, int(p.shape[0]), int(max_lag), int(slab_cols)
        o.probs = _ptr(p) if p.shape[0] else None
        res = {k: np.empty(D) for k in ("mean", "sd", "mcse", "ess", "rhat")}
        res["quantiles"] = np.empty((D, p.shape[0]))
        res["n_lags"] = np.empty(D, dtype=np.int32)
        out = bb_chain_out()
        for k in ("mean", "sd", "mcse", "ess", "rhat"):
            setattr(out, k, _ptr(res[k]))
        out.quantiles = _ptr(res["quantiles"]) if p.shape[0] else None
        out.n_lags = res["n_lags"].ctypes.data_as(C.POINTER(C.c_int32))
        self._check(self._lib.bb_chain_summary(self._h, C.byref(o), D, _ptr(x), C.byref(out)))
        return res

    # ---- the iterate trace (include/barbay_hip.h, bb_trace_*) ----
    def trace_begin(self, every: int, capacity: int):
        """Keep (mu, omega) after every `every` steps of `run` in a device ring of `capacity` snapshots (`bb_trace_begin`)."""
        o = bb_trace_opts()
        o.every, o.capacity = int(every), int(capacity)
        self._check(self._lib.bb_trace_begin(self._h, C.byref(o)))

    def trace_end(self):
        self._check(self._lib.bb_trace_end(self._h))

    def trace_count(self) -> Tuple[int, int]:
        """(taken, first_live): snapshots recorded since `trace_begin` or the last reset, and the oldest one the ring still holds."""
        taken, live = C.c_int64(0), C.c_int64(0)
        self._check(self._lib.bb_trace_count(self._h, C.byref(taken), C.byref(live)))
        return int(taken.value), int(live.value)

    def trace_get(self, first: int, n: int) -> Tuple[np.ndarray, np.ndarray]:
        """Snapshots first .. first + n - 1 as (mu[n, D], omega[n, D]) in the caller's latent order (`bb_trace_get`)."""
        mu, om = np.empty((int(n), self.D)), np.empty((int(n), self.D))
        self._check(self._lib.bb_trace_get(self._h, int(first), int(n), _ptr(mu), _ptr(om)))
        return mu, om

    def trace_summary(self, first: int, n_chains: int, n_draws: int, max_lag: int = 0, rhat_max: float = 1.1, columns: bool = False,
                      slab_cols: int = 0, blocks: bool = True, only: Optional[Sequence[str]] = None) -> Dict[str, object]:
        """Split-R-hat, ESS and MCSE of the window of n_chains * n_draws snapshots from `first`, computed on the ring where it lies
        (`bb_trace_summary`).  Returns {"blocks": DataFrame}: one row per (layout block, part) -- name, part ("mu" / "omega"), n_cols,
        n_nonfinite, n_const, n_above, max_rhat, min_ess, max_mcse_rel.  With `columns` also mean, sd, mcse, ess, rhat and n_lags
        (int32), each [2 D]: mu of the caller's latent i at i, its omega at D + i; `only` names the ones wanted (the others are not
        downloaded).  `blocks=False` leaves the verdict out."""
        o = bb_trace_sum_opts()
        o.first, o.n_chains, o.n_draws, o.max_lag, o.slab_cols, o.rhat_max = int(first), int(n_chains), int(n_draws), int(max_lag), int(slab_cols), float(rhat_max)
        out = bb_trace_sum_out()
        res: Dict[str, object] = {}
        if columns:
            for k in TRACE_COLS + ("n_lags",):
                if only is not None and k not in only:
                    continue
                if k == "n_lags":
                    res[k] = np.empty(2 * self.D, dtype=np.int32)
                    out.n_lags = res[k].ctypes.data_as(C.POINTER(C.c_int32))
                else:
                    res[k] = np.empty(2 * self.D)
                    setattr(out, k, _ptr(res[k]))
        nb = len(self.layout())
        vb = (bb_trace_block * (2 * nb))()
        if blocks:
            out.blocks = vb
        self._check(self._lib.bb_trace_summary(self._h, C.byref(o), C.byref(out)))
        if blocks:
            import pandas as pd
            rows = {"name": [vb[i].name.decode() for i in range(2 * nb)], "part": ["omega" if vb[i].part else "mu" for i in range(2 * nb)]}
            for k in TRACE_BLOCK_COUNTS + TRACE_BLOCK_VALUES:
                rows[k] = [getattr(vb[i], k) for i in range(2 * nb)]
            res["blocks"] = pd.DataFrame(rows)
        return res

    # ---- cross-GPU leg of the resident launch (include/barbay_hip.h, bb_p2p_*) ----
    def p2p_export(self) -> bytes:
        buf = C.create_string_buffer(BB_P2P_HANDLE_BYTES)
        self._check(self._lib.bb_p2p_export(self._h, buf))
        return buf.raw

    def p2p_import(self, handles: Sequence[bytes]):
        blob = b"".join(handles)
        assert len(blob) == BB_P2P_HANDLE_BYTES * len(handles)
        buf = C.create_string_buffer(blob, len(blob))
        self._check(self._lib.bb_p2p_import(self._h, buf))

    def p2p_selftest(self) -> bool:
        ok = C.c_int32(0)
        self._check(self._lib.bb_p2p_selftest(self._h, C.byref(ok)))
        return bool(ok.value)

    def p2p_enable(self, on: bool) -> bool:
        """True if the resident launch is now (on) / no longer (off) in use; False if this shard cannot use it."""
        rc = self._lib.bb_p2p_enable(self._h, 1 if on else 0)
        if rc == BB_ERR_UNSUPPORTED:
            return False
        self._check(rc)
        return True

    def make_comm_id(self) -> bytes:
        buf = C.create_string_buffer(BB_COMM_ID_BYTES)
        self._check(self._lib.bb_comm_make_id(buf))
        return buf.raw

    def comm_init(self, comm_id: bytes):
        assert len(comm_id) == BB_COMM_ID_BYTES
        buf = C.create_string_buffer(comm_id, BB_COMM_ID_BYTES)
        self._check(self._lib.bb_comm_init(self._h, buf))

    def step_moments(self) -> np.ndarray:
        k = int(self.stats()["n_moments"])
        out = np.empty(k)
        self._check(self._lib.bb_step_moments(self._h, _ptr(out)))
        return out

    def step_apply(self, total: np.ndarray):
        total = _f64(total)
        self._check(self._lib.bb_step_apply(self._h, _ptr(total)))
