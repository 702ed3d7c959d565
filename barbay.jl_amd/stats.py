"""Host-side mirror of the two `BarBay.stats` functions that feed the hot path's priors:

    naive_fitness    src/stats.jl:1040-1106
    naive_prior      src/stats.jl:1175-1359

Both are one-shot array passes over the tidy frame; their outputs (`s_pop_prior`, `logσ_pop_prior`, `logλ_prior`
means) are what `docs/src/examples.md:122-140` stacks with a chosen std into the matrix-form priors that
`bb_model_desc` takes per element.

The posterior-predictive checks of the reference's guide ("Validating the inference", docs/src/index.md:398-580) come in two forms:

    matrix_quantile_range, freq_bc_ppc, logfreq_ratio_bc_ppc,    host numpy ports of src/stats.jl:55-1000, on a DataFrame of
    logfreq_ratio_popmean_ppc, logfreq_ratio_multienv_ppc         posterior samples (numpy's Generator: Julia's stream is not matched)
    logfreq_ratio_ppc_bands                                       the same bands for every barcode and time step in one device call
                                                                  (`bb_ppc_bands`), from the ADVI frame itself
    freq_ppc_bands                                                the bands of the frequency trajectories (freq_bc_ppc) of every barcode,
                                                                  neutrals included, in one device call (`bb_freq_bands`)
    logfreq_ratio_ppc_scores, pit_histogram                       the log predictive density and PIT of every observed ratio, the
                                                                  draws averaged in closed form (`bb_ppc_score`), and the calibration
                                                                  histogram of the PITs (no reference counterpart)
    logfreq_ratio_loo, loo_compare                                Pareto-smoothed leave-one-out scores per barcode with the khat
                                                                  diagnostic (`bb_ppc_loo`), and the paired comparison of two fits
                                                                  (no reference counterpart)
    fitness_marginals                                             the Rao-Blackwellised marginal of every mutant's fitness beside the
                                                                  mean-field one (`bb_fitness_rb`): how far the fit's +- can be trusted
                                                                  (no reference counterpart)
    hyperfitness_marginals                                        the same for the hyper-fitness theta of the hierarchical models -- a
                                                                  genotype's fitness, a mutant's across its replicates -- whose
                                                                  conditional sums over the group's members (`bb_theta_rb`)
    fitness_contrasts                                             differences and other linear contrasts of fitnesses or hyper-fitnesses
                                                                  from the joint draws (`bb_contrast_rb`): what the terms share cancels
    popmean_marginals                                             the same for the population mean fitness of every time step, whose
                                                                  conditional sums over every barcode of the replicate (`bb_popmean_rb`)
    noise_marginals                                               the same for the noise scales logsigma of the mutants and of the time
                                                                  steps, whose conditional is integrated numerically (`bb_logsigma_rb`)
    deviation_marginals                                           the same for logtau, the deviation scale of the hierarchical models,
                                                                  whose conditional can have two modes (`bb_logtau_rb`)
"""
from __future__ import annotations

import math
from contextlib import contextmanager
from typing import Dict, List, Optional, Sequence

import numpy as np
import pandas as pd

from . import utils
from .model import BarBayError
from .utils import _neutral_mask


def naive_fitness(data: pd.DataFrame, *, id_col="barcode", time_col="time", count_col="count", neutral_col="neutral",
                  pseudocount: int = 1) -> pd.DataFrame:
    """Mean over time of log(f_{t+1}/f_t) of a mutant minus the neutrals' mean of the same (src/stats.jl:1040-1106).
    Frequencies use per-time totals of the pseudocounted counts (:1053-1060); the first time point of every barcode
    has no ratio (:1075-1080); rows come back in the frame's barcode order (groupby, first appearance)."""
    d = data[[id_col, time_col, count_col, neutral_col]]
    cnt = d[count_col].to_numpy(dtype=np.float64) + pseudocount
    tr = utils._time_rank(d, time_col)
    freq = cnt / np.bincount(tr, weights=cnt)[tr]
    codes, ids = pd.factorize(d[id_col], sort=False)
    order = np.lexsort((np.arange(len(d)), codes))                # rows of a barcode in frame order (the reference does not sort here)
    c, t, lf = codes[order], tr[order], np.log(freq[order])
    same = c[1:] == c[:-1]
    logf, t2, c2 = (lf[1:] - lf[:-1])[same], t[1:][same], c[1:][same]
    first = np.zeros(len(ids), dtype=np.int64)
    first[codes[::-1]] = np.arange(len(d))[::-1]
    neu = _neutral_mask(d, neutral_col)[first]                    # first(d[:, neutral_col]) per barcode (:1082)
    n2 = neu[c2]
    nt = int(tr.max()) + 1
    st = np.bincount(t2[n2], weights=logf[n2], minlength=nt) / np.maximum(np.bincount(t2[n2], minlength=nt), 1)
    norm = logf - st[t2]
    keep = ~n2
    fit = np.bincount(c2[keep], weights=norm[keep], minlength=len(ids)) / np.maximum(np.bincount(c2[keep], minlength=len(ids)), 1)
    mut = ~neu
    return pd.DataFrame({id_col: np.asarray(ids)[mut], "fitness": fit[mut]})


def _finite_mean_std(x: np.ndarray):
    """Row-wise mean and corrected std over the finite entries (`x[.!isinf.(x)]`, src/stats.jl:1264-1266, :1300-1302)."""
    ok = ~np.isinf(x)
    n = ok.sum(axis=1)
    xs = np.where(ok, x, 0.0)
    mean = xs.sum(axis=1) / n
    var = (np.where(ok, x - mean[:, None], 0.0) ** 2).sum(axis=1) / (n - 1)
    return mean, np.sqrt(var)


def naive_prior(data: pd.DataFrame, *, id_col="barcode", time_col="time", count_col="count", neutral_col="neutral",
                rep_col: Optional[str] = None, pseudocount: int = 1) -> Dict[str, np.ndarray]:
    """Empirical prior means from the neutral lineages (src/stats.jl:1175-1359):
        s_pop_prior    = -mean_b log(f_{t+1,b}/f_{t,b})   per time step (and replicate, replicate-major)
        logσ_pop_prior = -std_b  log(f_{t+1,b}/f_{t,b})   (sic: minus the std, :1338)
        logλ_prior     = log(counts + pseudocount), time-fastest per barcode (and replicate-major)  (:1347-1352)
    Unlike the reference (:1187) the caller's frame is left untouched."""
    d = data.copy()
    d[count_col] = d[count_col] + pseudocount
    arr = utils.data_to_arrays(d, id_col=id_col, time_col=time_col, count_col=count_col, neutral_col=neutral_col, rep_col=rep_col)
    if isinstance(arr.bc_count, list):                                             # uneven replicates (:1237-1258)
        mats, tots = arr.bc_count, arr.bc_total
    elif arr.bc_count.ndim == 3:                                                   # T x B x R (:1211-1236)
        mats = [arr.bc_count[:, :, r] for r in range(arr.bc_count.shape[2])]
        tots = [arr.bc_total[:, r] for r in range(arr.bc_count.shape[2])]
    else:
        mats, tots = [arr.bc_count], [arr.bc_total]
    s_pop, ls_pop, loglam = [], [], []
    for R, n in zip(mats, tots):
        f = R[:, :arr.n_neutral] / n[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            lr = np.log(f[1:] / f[:-1])
        m, sd = _finite_mean_std(lr)
        s_pop.append(-m)
        ls_pop.append(-sd)
        with np.errstate(divide="ignore"):
            loglam.append(np.log(R.astype(np.float64)).T.reshape(-1))              # column-major `[:]`
    return {"s_pop_prior": np.concatenate(s_pop), "logσ_pop_prior": np.concatenate(ls_pop),
            "logλ_prior": np.concatenate(loglam)}


# ---- posterior predictive checks (src/stats.jl:55-1000) ------------------------------------------------------------------------
def _quantile7(xs: np.ndarray, p: float) -> np.ndarray:
    """StatsBase.quantile of the sorted last axis (Statistics._quantile, alpha = beta = 1: numpy's method="linear")."""
    n = xs.shape[-1]
    if n == 1:
        return xs[..., 0].copy()
    aleph = n * p + (1.0 - p)
    j = min(max(int(aleph), 1), n - 1)
    g = min(max(aleph - j, 0.0), 1.0)
    a, b = xs[..., j - 1], xs[..., j]
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(a) & np.isfinite(b), a + g * (b - a), (1.0 - g) * a + g * b)


def matrix_quantile_range(quantile: Sequence[float], matrix, *, dims: int = 2) -> np.ndarray:
    """src/stats.jl:55-92: for every q the (1 - q) / 2 and 1 - (1 - q) / 2 quantiles of each slice along `dims` (2: every column,
    1: every row), shape [size(matrix, dims), len(quantile), 2]."""
    q = [float(x) for x in quantile]
    if any(not (0.0 <= x <= 1) for x in q):
        raise BarBayError("All quantiles must be between zero and one")
    if dims not in (1, 2):
        raise BarBayError("Dimensions should match a Matrix dimensiosn, i.e., 1 or 2")
    m = np.asarray(matrix, dtype=np.float64)
    xs = np.sort(m.T if dims == 2 else m, axis=-1)
    out = np.empty((xs.shape[0], len(q), 2))
    for i, x in enumerate(q):
        out[:, i, 0] = _quantile7(xs, (1.0 - x) / 2.0)
        out[:, i, 1] = _quantile7(xs, 1.0 - (1.0 - x) / 2.0)
    return out


def _sorted_vars(df: pd.DataFrame, pattern: str) -> List[str]:
    """`sort(names(df)[occursin.(pattern, names(df))])`: substring match, then a LEXICOGRAPHIC sort -- as the reference has it,
    `s̲ₜ[10]` comes before `s̲ₜ[2]`, so with 10 or more time steps the columns of the result are not in time order."""
    return sorted(c for c in map(str, df.columns) if pattern in c)


def _flat(x: np.ndarray, flatten: bool) -> np.ndarray:
    """`vcat(eachslice(x, dims=3)...)`: the n_ppc slices stacked row-wise."""
    return x.transpose(2, 0, 1).reshape(-1, x.shape[1]) if flatten else x


def freq_bc_ppc(df: pd.DataFrame, n_ppc: int, *, param: Optional[Dict[str, str]] = None, model: str = "lognormal",
                flatten: bool = True, rng: Optional[np.random.Generator] = None) -> np.ndarray:
    """src/stats.jl:152-213: frequency trajectories f_{t+1} = f_t exp(s - sbar_t + noise), [n, n_steps + 1, n_ppc] (flattened:
    [n_ppc n, n_steps + 1]).  model "lognormal": the std column is sigma; "normal": it is log sigma.  Column order: `_sorted_vars`."""
    param = param or {"bc_mean_fitness": "s⁽ᵐ⁾", "bc_std_fitness": "σ⁽ᵐ⁾", "bc_freq": "f̲⁽ᵐ⁾[1]", "population_mean_fitness": "s̲ₜ"}
    rng = rng or np.random.default_rng()
    mean_vars = _sorted_vars(df, param["population_mean_fitness"])
    f = np.empty((len(df), len(mean_vars) + 1, n_ppc))
    f[:, 0, :] = df[param["bc_freq"]].to_numpy(dtype=np.float64)[:, None]
    s = df[param["bc_mean_fitness"]].to_numpy(dtype=np.float64)
    sd = df[param["bc_std_fitness"]].to_numpy(dtype=np.float64)
    for i, var in enumerate(mean_vars):
        if model == "lognormal":
            scale = sd
        elif model == "normal":
            scale = np.exp(sd)
        else:
            raise BarBayError("model must be :normal or :lognormal")
        mu = s - df[var].to_numpy(dtype=np.float64)
        f[:, i + 1, :] = f[:, i, :] * np.exp(rng.normal(mu[:, None], scale[:, None], (len(df), n_ppc)))
    return _flat(f, flatten)


def logfreq_ratio_bc_ppc(df: pd.DataFrame, n_ppc: int, *, param: Optional[Dict[str, str]] = None, flatten: bool = True,
                         rng: Optional[np.random.Generator] = None) -> np.ndarray:
    """src/stats.jl:377-418: log(f_{t+1} / f_t) ~ N(s - sbar_t, exp(log sigma)) per sample row, [n, n_steps, n_ppc] (flattened:
    [n_ppc n, n_steps]).  Column order: `_sorted_vars`."""
    param = param or {"bc_mean_fitness": "s⁽ᵐ⁾", "bc_std_fitness": "σ⁽ᵐ⁾", "population_mean_fitness": "s̲ₜ"}
    rng = rng or np.random.default_rng()
    mean_vars = _sorted_vars(df, param["population_mean_fitness"])
    out = np.empty((len(df), len(mean_vars), n_ppc))
    s = df[param["bc_mean_fitness"]].to_numpy(dtype=np.float64)
    sd = np.exp(df[param["bc_std_fitness"]].to_numpy(dtype=np.float64))
    for i, var in enumerate(mean_vars):
        mu = s - df[var].to_numpy(dtype=np.float64)
        out[:, i, :] = rng.normal(mu[:, None], sd[:, None], (len(df), n_ppc))
    return _flat(out, flatten)


def logfreq_ratio_popmean_ppc(df: pd.DataFrame, n_ppc: int, *, param: Optional[Dict[str, str]] = None, flatten: bool = True,
                              rng: Optional[np.random.Generator] = None) -> np.ndarray:
    """src/stats.jl:571-621: neutral log(f_{t+1} / f_t) ~ N(-sbar_t, exp(log sigmabar_t)), [n, n_steps, n_ppc] (flattened:
    [n_ppc n, n_steps]).  The default names are the reference's (`sₜ`, `σₜ`); column order: `_sorted_vars`."""
    param = param or {"population_mean_fitness": "sₜ", "population_std_fitness": "σₜ"}
    rng = rng or np.random.default_rng()
    mean_vars = _sorted_vars(df, param["population_mean_fitness"])
    std_vars = _sorted_vars(df, param["population_std_fitness"])
    if len(mean_vars) != len(std_vars):
        raise BarBayError("The number of mean and standard deviation variables does not match")
    out = np.empty((len(df), len(mean_vars), n_ppc))
    for i, var in enumerate(mean_vars):
        mu = -df[var].to_numpy(dtype=np.float64)
        sd = np.exp(df[std_vars[i]].to_numpy(dtype=np.float64))
        out[:, i, :] = rng.normal(mu[:, None], sd[:, None], (len(df), n_ppc))
    return _flat(out, flatten)


def logfreq_ratio_multienv_ppc(df: pd.DataFrame, n_ppc: int, envs: Sequence, *, param: Optional[Dict[str, str]] = None,
                               flatten: bool = True, rng: Optional[np.random.Generator] = None) -> np.ndarray:
    """src/stats.jl:789-864: step t uses the fitness of the environment of the LATER time point, envs[t + 1].
    [n, n_steps, n_ppc] (flattened: [n_ppc n, n_steps]).  Column order: `_sorted_vars`."""
    param = param or {"bc_mean_fitness": "s̲⁽ᵐ⁾", "bc_std_fitness": "σ̲⁽ᵐ⁾", "population_mean_fitness": "s̲ₜ"}
    rng = rng or np.random.default_rng()
    envs = list(envs)
    env_unique = list(dict.fromkeys(envs))
    env_idx = [env_unique.index(e) for e in envs]
    mean_vars = _sorted_vars(df, param["population_mean_fitness"])
    s_vars = _sorted_vars(df, param["bc_mean_fitness"])
    sd_vars = _sorted_vars(df, param["bc_std_fitness"])
    if len(s_vars) != len(env_unique) or len(sd_vars) != len(env_unique):
        raise BarBayError("# of mutant-related variables does not match # of environments")
    if len(envs) != len(mean_vars) + 1:
        raise BarBayError("Number of given environments does not match time points in chain")
    out = np.empty((len(df), len(mean_vars), n_ppc))
    for i, var in enumerate(mean_vars):
        e = env_idx[i + 1]
        mu = df[s_vars[e]].to_numpy(dtype=np.float64) - df[var].to_numpy(dtype=np.float64)
        sd = np.exp(df[sd_vars[e]].to_numpy(dtype=np.float64))
        out[:, i, :] = rng.normal(mu[:, None], sd[:, None], (len(df), n_ppc))
    return _flat(out, flatten)


@contextmanager
def _engine_at_fit(data: pd.DataFrame, df_advi: pd.DataFrame, model, model_kwargs: Optional[Dict], seed: int, device: int, cols: Dict):
    """An engine for `model` on `data` holding the variational parameters of `df_advi` (what `vi.advi` returned for the same data and
    model: its first D rows, in the model's order): (engine, model instance, DataArrays, model name)."""
    from . import vi
    mname = getattr(model, "__name__", str(model))
    model_kwargs = dict(model_kwargs or {})
    arrays = utils.data_to_arrays(data, **cols)
    if "multienv" in mname:
        model_kwargs = {"envs": arrays.envs, **model_kwargs}
    if "genotype" in mname:
        model_kwargs = {"genotypes": arrays.genotypes, **model_kwargs}
    bayes_model = model(arrays.bc_count, arrays.bc_total, arrays.n_neutral, arrays.n_bc, **model_kwargs)
    with vi.make_engine(bayes_model, vi.ADVI(), vi.TruncatedADAGrad(), seed, device) as e:
        names = []
        for sym, (_, lo, hi) in zip(bayes_model.var_symbols(), e.layout()):
            names += [f"{sym}[{x}]" for x in range(1, hi - lo + 1)]
        D = e.D
        if len(df_advi) < D or list(df_advi["varname"].iloc[:D]) != names:
            raise BarBayError("df_advi does not hold this model's variational parameters in its first rows (vi.advi on the same data and model)")
        mu = df_advi["mean"].to_numpy(dtype=np.float64)[:D]
        sd = np.maximum(df_advi["std"].to_numpy(dtype=np.float64)[:D], np.finfo(np.float64).tiny)
        e.set_params(mu, sd + np.log(-np.expm1(-sd)))                   # omega = softplus^-1(std)
        yield e, bayes_model, arrays, mname


def _envs_per_rep(arrays, mname: str, R: int):
    envs = arrays.envs
    has_env = "multienv" in mname
    return has_env, (envs if (has_env and isinstance(envs, list) and envs and isinstance(envs[0], (list, tuple))) else [envs] * R)


def _env_labels(arrays, mname: str, R: int):
    """(has environments, their labels in the model's numbering: first appearance over the replicates' time points)."""
    has_env, per_env = _envs_per_rep(arrays, mname, R)
    labels: List = []
    if has_env:
        for env in (x for r in range(R) for x in per_env[r]):
            if env not in labels:
                labels.append(env)
    return has_env, labels


def logfreq_ratio_ppc_bands(data: pd.DataFrame, df_advi: pd.DataFrame, *, model, model_kwargs: Optional[Dict] = None,
                            quantiles: Sequence[float] = (0.95, 0.675, 0.05), n_samples: int = 1000, n_ppc: int = 10, seed: int = 0,
                            id_col="barcode", time_col="time", count_col="count", neutral_col="neutral",
                            rep_col: Optional[str] = None, env_col: Optional[str] = None, genotype_col: Optional[str] = None,
                            device: int = 0) -> pd.DataFrame:
    """The guide's validation workflow (docs/src/index.md:398-580) for EVERY barcode and time step in one device call (`bb_ppc_bands`).

    `df_advi` is what `vi.advi` returned for `data` and `model`: its first D rows (the variational parameters, in the model's
    order) give the posterior N(mean, std).  Each (row, step) gets n_samples posterior draws x n_ppc predictive draws of the
    log-frequency ratio; the bands are `matrix_quantile_range` of those K = n_samples n_ppc values (K <= 16384).

    Returns a tidy frame, one line per (row, step, quantile): `id` ("neutral" for the population-mean row, else the barcode),
    `rep` ("R1", ...), `env` (the later time point's environment; None without environments), `time` (the later time point's index,
    1 .. T_r - 1), `quantile`, `lower`, `upper`, and `n_outside`: the row's finite observed ratios outside its widest band (per row,
    repeated on its lines) -- sort by it to rank the barcodes the fit does not explain."""
    cols = dict(id_col=id_col, time_col=time_col, count_col=count_col, neutral_col=neutral_col, rep_col=rep_col,
                env_col=env_col, genotype_col=genotype_col)
    with _engine_at_fit(data, df_advi, model, model_kwargs, seed, device, cols) as (e, bayes_model, arrays, mname):
        bands, nout = e.ppc_bands(quantiles, n_samples=n_samples, n_ppc=n_ppc, seed=seed)
    n_rows, n_steps, n_q, _ = bands.shape
    R, nb = len(bayes_model.counts), bayes_model.n_bc
    has_env, per_env = _envs_per_rep(arrays, mname, R)
    row = np.arange(n_rows)
    rep = np.where(row < R, row, (row - R) // max(nb, 1))
    ids = np.asarray(["neutral"] * R + [b for _ in range(R) for b in arrays.bc_ids], dtype=object)
    rr, tt, qq = np.meshgrid(row, np.arange(n_steps), np.arange(n_q), indexing="ij")
    keep = ~np.isnan(bands[..., 0])
    rr, tt, qq = rr[keep], tt[keep], qq[keep]
    out = pd.DataFrame({
        "id": ids[rr],
        "rep": [f"R{r + 1}" for r in rep[rr]],
        "env": [per_env[r][t + 1] for r, t in zip(rep[rr], tt)] if has_env else None,
        "time": tt + 1,
        "quantile": np.asarray(quantiles, dtype=np.float64)[qq],
        "lower": bands[..., 0][keep],
        "upper": bands[..., 1][keep],
        "n_outside": nout[rr],
    })
    return out


def freq_ppc_bands(data: pd.DataFrame, df_advi: pd.DataFrame, *, model, mode: str = "trajectory", model_kwargs: Optional[Dict] = None,
                   quantiles: Sequence[float] = (0.95, 0.675, 0.05), n_samples: int = 1000, n_ppc: Optional[int] = None, seed: int = 0,
                   id_col="barcode", time_col="time", count_col="count", neutral_col="neutral",
                   rep_col: Optional[str] = None, env_col: Optional[str] = None, genotype_col: Optional[str] = None,
                   device: int = 0) -> pd.DataFrame:
    """The observed frequency trajectory of EVERY barcode, neutrals included, against what the fit predicts (`bb_freq_bands`).

    mode "trajectory": `freq_bc_ppc` (src/stats.jl:152-213) for all barcodes at once -- from each of n_samples posterior draws the
    initial frequency exp(loglambda) / sum exp(loglambda) of the draw, then n_ppc (default 10) trajectories
    f_{t+1} = f_t exp(N(s - sbar_t, sigma)); the errors accumulate over time, so a barcode may leave these bands while every single
    step stays inside its `logfreq_ratio_ppc_bands` band.  mode "posterior" (n_ppc = 1): the posterior of the model's own frequencies
    at every time point.  `df_advi` as for `logfreq_ratio_ppc_bands`; K = n_samples n_ppc <= 16384.

    Returns a tidy frame, one line per (barcode, time point, quantile): `id`, `neutral`, `rep` ("R1", ...), `env` (the time point's
    environment; None without environments), `time` (0-based index of the time point), `quantile`, `lower`, `upper`, `observed`
    (count / total of the time point) and `n_outside`: the barcode's time points whose observed frequency lies outside its widest band
    (per barcode and replicate, repeated on its lines) -- sort by it to rank the barcodes the fit does not explain."""
    if mode not in ("trajectory", "posterior"):
        raise BarBayError('mode must be "trajectory" or "posterior"')
    if n_ppc is None:
        n_ppc = 10 if mode == "trajectory" else 1
    cols = dict(id_col=id_col, time_col=time_col, count_col=count_col, neutral_col=neutral_col, rep_col=rep_col,
                env_col=env_col, genotype_col=genotype_col)
    with _engine_at_fit(data, df_advi, model, model_kwargs, seed, device, cols) as (e, bayes_model, arrays, mname):
        bands, nout = e.freq_bands(quantiles, mode=mode, n_samples=n_samples, n_ppc=n_ppc, seed=seed)
    n_rows, n_cols, n_q, _ = bands.shape
    R, nn = len(bayes_model.counts), arrays.n_neutral
    B = n_rows // R
    has_env, per_env = _envs_per_rep(arrays, mname, R)
    ids = np.asarray(list(arrays.neutral_ids) + list(arrays.bc_ids), dtype=object)      # the data columns: neutrals first
    obs = np.full((n_rows, n_cols), np.nan)
    for r, (c, n) in enumerate(zip(bayes_model.counts, bayes_model.totals)):
        with np.errstate(divide="ignore", invalid="ignore"):
            obs[r * B:(r + 1) * B, :c.shape[0]] = (np.asarray(c, dtype=np.float64) / np.asarray(n, dtype=np.float64)[:, None]).T
    rr, tt, qq = np.meshgrid(np.arange(n_rows), np.arange(n_cols), np.arange(n_q), indexing="ij")
    keep = np.broadcast_to((np.arange(n_cols)[None, :] < np.repeat([c.shape[0] for c in bayes_model.counts], B)[:, None])[..., None],
                           rr.shape)
    rr, tt, qq = rr[keep], tt[keep], qq[keep]
    rep, col = rr // B, rr % B
    return pd.DataFrame({
        "id": ids[col],
        "neutral": col < nn,
        "rep": [f"R{r + 1}" for r in rep],
        "env": [per_env[r][t] for r, t in zip(rep, tt)] if has_env else None,
        "time": tt,
        "quantile": np.asarray(quantiles, dtype=np.float64)[qq],
        "lower": bands[..., 0][keep],
        "upper": bands[..., 1][keep],
        "observed": obs[rr, tt],
        "n_outside": nout[rr],
    })


def logfreq_ratio_ppc_scores(data: pd.DataFrame, df_advi: pd.DataFrame, *, model, model_kwargs: Optional[Dict] = None,
                             n_samples: int = 1000, seed: int = 0,
                             id_col="barcode", time_col="time", count_col="count", neutral_col="neutral",
                             rep_col: Optional[str] = None, env_col: Optional[str] = None, genotype_col: Optional[str] = None,
                             device: int = 0) -> pd.DataFrame:
    """How well the fit predicts EVERY observed log-frequency ratio, neutrals included, in one device call (`bb_ppc_score`): the
    log predictive density of the ratio and its probability integral transform (PIT), the normal predictive of each of n_samples
    posterior draws averaged in closed form -- no predictive draws, so the scores rank barcodes that `n_outside` cannot tell apart
    and do not depend on a quantile.  `df_advi` as for `logfreq_ratio_ppc_bands`; n_samples <= 16384; at equal seed the draws are
    those of the band calls.

    Returns a tidy frame, one line per (barcode, replicate, step) that exists: `id`, `neutral`, `rep` ("R1", ...), `env` (the later
    time point's environment; None without environments), `time` (the later time point's index, 1 .. T_r - 1), `observed` (the
    ratio; NaN, as every score of the line, where either count is 0), `pred_mean`, `pred_sd`, `lpd`, `p_waic`, `pit`, `pit_upper`
    (the predictive CDF at the ratio and its complement, each accurate where it is tiny), and per barcode and replicate, repeated
    on its lines, `row_lpd` (the sum of its scored steps' lpd: sort ascending to rank the barcodes the fit does not explain) and
    `n_scored`.  `pit_histogram` of the frame shows the calibration."""
    cols = dict(id_col=id_col, time_col=time_col, count_col=count_col, neutral_col=neutral_col, rep_col=rep_col,
                env_col=env_col, genotype_col=genotype_col)
    with _engine_at_fit(data, df_advi, model, model_kwargs, seed, device, cols) as (e, bayes_model, arrays, mname):
        res = e.ppc_score(n_samples=n_samples, seed=seed)
    n_rows, n_steps = res["lpd"].shape
    R, nn = len(bayes_model.counts), arrays.n_neutral
    B = n_rows // R
    has_env, per_env = _envs_per_rep(arrays, mname, R)
    ids = np.asarray(list(arrays.neutral_ids) + list(arrays.bc_ids), dtype=object)      # the data columns: neutrals first
    rr, tt = np.meshgrid(np.arange(n_rows), np.arange(n_steps), indexing="ij")
    keep = np.arange(n_steps)[None, :] < np.repeat([c.shape[0] - 1 for c in bayes_model.counts], B)[:, None]
    rr, tt = rr[keep], tt[keep]
    rep, col = rr // B, rr % B
    out = {
        "id": ids[col],
        "neutral": col < nn,
        "rep": [f"R{r + 1}" for r in rep],
        "env": [per_env[r][t + 1] for r, t in zip(rep, tt)] if has_env else None,
        "time": tt + 1,
    }
    for k in ("observed", "pred_mean", "pred_sd", "lpd", "p_waic", "pit", "pit_upper"):
        out[k] = res[k][keep]
    out["row_lpd"] = res["row_lpd"][rr]
    out["n_scored"] = res["n_scored"][rr]
    return pd.DataFrame(out)


def logfreq_ratio_loo(data: pd.DataFrame, df_advi: pd.DataFrame, *, model, model_kwargs: Optional[Dict] = None,
                      n_samples: int = 1000, seed: int = 0,
                      id_col="barcode", time_col="time", count_col="count", neutral_col="neutral",
                      rep_col: Optional[str] = None, env_col: Optional[str] = None, genotype_col: Optional[str] = None,
                      device: int = 0) -> pd.DataFrame:
    """Which barcodes does the fit lean on too hard, and how well would it have predicted each one had it not seen it?  Pareto-
    smoothed importance-sampling leave-one-out (PSIS-LOO; Vehtari, Gelman, Gabry 2017) on the draws and log densities of
    `logfreq_ratio_ppc_scores`, in one device call (`bb_ppc_loo`), a barcode's whole trajectory left out at a time.
    `df_advi` as for `logfreq_ratio_ppc_bands`; n_samples <= 8192.

    Returns one line per barcode and replicate, labelled as `logfreq_ratio_ppc_scores` labels them (`id`, `neutral`, `rep`):
    `elpd_loo` (the log predictive density of the barcode's scored ratios, jointly, under the fit without them: what
    `loo_compare` sums), `p_loo` (in-sample minus leave-one-out: the effective number of parameters the barcode takes up), `khat`
    (the fitted shape of the importance ratios' tail; +Inf: not fitted, too few draws or ratios beyond the range of exp),
    `n_eff` (the effective number of draws behind the estimate), `khat_max_cell` (the largest khat when a single ratio of the
    barcode is left out), `n_scored`, and `flag`: khat above min(1 - 1 / log10(n_samples), 0.7) (Vehtari et al. 2024) -- the
    estimate for that barcode is unreliable and the fit depends on it unduly; a barcode without a scored step (NaN) is not flagged.
    `.attrs`: "elpd_loo" (the total over the scored barcodes), "se" (sqrt(N var) of the N per-barcode values), "p_loo",
    "n_flagged" and "khat_threshold"."""
    cols = dict(id_col=id_col, time_col=time_col, count_col=count_col, neutral_col=neutral_col, rep_col=rep_col,
                env_col=env_col, genotype_col=genotype_col)
    with _engine_at_fit(data, df_advi, model, model_kwargs, seed, device, cols) as (e, bayes_model, arrays, mname):
        res = e.ppc_loo(n_samples=n_samples, seed=seed)
    n_rows = res["row_elpd_loo"].shape[0]
    R, nn = len(bayes_model.counts), arrays.n_neutral
    B = n_rows // R
    ids = np.asarray(list(arrays.neutral_ids) + list(arrays.bc_ids), dtype=object)      # the data columns: neutrals first
    row = np.arange(n_rows)
    rep, col = row // B, row % B
    thr = min(1.0 - 1.0 / math.log10(n_samples), 0.7)
    out = pd.DataFrame({
        "id": ids[col],
        "neutral": col < nn,
        "rep": [f"R{r + 1}" for r in rep],
        "elpd_loo": res["row_elpd_loo"],
        "p_loo": res["row_p_loo"],
        "khat": res["row_khat"],
        "n_eff": res["row_n_eff"],
        "khat_max_cell": res["row_khat_max"],
        "n_scored": res["n_scored"],
        "flag": res["row_khat"] > thr,
    })
    ok = res["n_scored"] > 0
    v = res["row_elpd_loo"][ok]
    out.attrs.update({"elpd_loo": float(v.sum()), "se": float(math.sqrt(len(v) * v.var(ddof=1))) if len(v) > 1 else float("nan"),
                      "p_loo": float(res["row_p_loo"][ok].sum()), "n_flagged": int(out["flag"].sum()), "khat_threshold": thr})
    return out


def loo_compare(a: pd.DataFrame, b: pd.DataFrame, top: int = 10) -> Dict:
    """Which of two fits predicts the data better?  `a`, `b`: frames of `logfreq_ratio_loo` over the same barcodes (two models, or
    two settings, on the same data); raises `BarBayError` if their row labels (`id`, `rep`) differ.  The comparison is paired:
    d_i = elpd_loo(b)_i - elpd_loo(a)_i per barcode, over the barcodes scored in both.  Returns a dict: "elpd_diff" = sum d_i
    (positive: b predicts better), "se_diff" = sqrt(N var d), "n" = N, "n_flagged" (barcodes flagged in either frame: their d_i are
    not to be trusted) and "rows": the `top` barcodes with the largest |d_i|, the ones that drive the difference (`id`, `rep`,
    `elpd_a`, `elpd_b`, `elpd_diff`, `flag`)."""
    keys = ["id", "rep"]
    if len(a) != len(b) or any(list(a[k]) != list(b[k]) for k in keys):
        raise BarBayError("loo_compare: the two frames do not have the same rows (id, rep)")
    ea, eb = a["elpd_loo"].to_numpy(dtype=np.float64), b["elpd_loo"].to_numpy(dtype=np.float64)
    ok = ~(np.isnan(ea) | np.isnan(eb))
    d = eb[ok] - ea[ok]
    n = int(ok.sum())
    flag = (a["flag"].to_numpy(dtype=bool) | b["flag"].to_numpy(dtype=bool))[ok]
    rows = pd.DataFrame({"id": a["id"].to_numpy()[ok], "rep": a["rep"].to_numpy()[ok], "elpd_a": ea[ok], "elpd_b": eb[ok],
                         "elpd_diff": d, "flag": flag})
    rows = rows.iloc[np.argsort(-np.abs(d), kind="stable")[:top]].reset_index(drop=True)
    return {"elpd_diff": float(d.sum()), "se_diff": float(math.sqrt(n * d.var(ddof=1))) if n > 1 else float("nan"), "n": n,
            "n_flagged": int(flag.sum()), "rows": rows}


def fitness_marginals(data: pd.DataFrame, df_advi: pd.DataFrame, *, model, model_kwargs: Optional[Dict] = None,
                      n_samples: int = 1000, probs: Sequence[float] = (0.025, 0.5, 0.975), threshold: float = 0.0, seed: int = 0,
                      id_col="barcode", time_col="time", count_col="count", neutral_col="neutral",
                      rep_col: Optional[str] = None, env_col: Optional[str] = None, genotype_col: Optional[str] = None,
                      device: int = 0, chain=None) -> pd.DataFrame:
    """Can the +- on a mutant's fitness be trusted?  Mean-field ADVI underestimates posterior standard deviations, and the fitness
    `vi.advi` reports is q's own mean and sd.  Given everything else a mutant's fitness has an exactly Gaussian full conditional;
    averaging it over n_samples joint draws of everything else gives the Rao-Blackwellised (RB) marginal, one exact Gibbs half-step
    away from q (`bb_fitness_rb`, one device call).  Were q the true posterior the two would agree; `sd_ratio` = rb_sd / q_sd says,
    per mutant, how much of the uncertainty mean-field cut away comes back.  `df_advi` as for `logfreq_ratio_ppc_bands`; at equal
    seed the draws are those of the band and score calls.  `chain`: the `chain` array of `mcmc.mcmc_sample` ([walkers, steps, D],
    or [draws, D]) -- its draws, pooled over the walkers, replace q's (at most 8672 of them): the same call then Rao-Blackwellises
    the chain's fitness estimates, and q_mean / q_sd are the chain's own.

    Returns one line per fitness unit (replicate, mutant, environment): `id`, `rep` ("R1", ...), `env` (None without environments),
    `n_steps` (the time steps that inform the unit; 0: its conditional is the prior), `q_mean`, `q_sd` (the draws' own fitness),
    `rb_mean`, `rb_sd`, `sd_ratio`, `p_pos`, `p_neg` (the RB probability of a fitness above / below `threshold`, each accurate
    where it is tiny) and one column per probability of `probs`, named q2.5, q50, q97.5, ...: the quantiles of the RB marginal."""
    cols = dict(id_col=id_col, time_col=time_col, count_col=count_col, neutral_col=neutral_col, rep_col=rep_col,
                env_col=env_col, genotype_col=genotype_col)
    probs = [float(p) for p in np.atleast_1d(probs)] if probs is not None else []
    with _engine_at_fit(data, df_advi, model, model_kwargs, seed, device, cols) as (e, bayes_model, arrays, mname):
        draws = None
        if chain is not None:
            draws = np.asarray(chain, dtype=np.float64)
            if draws.ndim not in (2, 3) or draws.shape[-1] != e.D:
                raise BarBayError(f"chain must be [walkers, steps, {e.D}] or [draws, {e.D}]")
            draws = draws.reshape(-1, e.D)
        res = e.fitness_rb(n_samples=n_samples, probs=probs, threshold=threshold, seed=seed, draws=draws)
    R, nb = len(bayes_model.counts), bayes_model.n_bc
    n_units = res["rb_mean"].shape[0]
    E = n_units // max(R * nb, 1)
    has_env, labels = _env_labels(arrays, mname, R)
    u = np.arange(n_units)
    rep, m, env = u // max(E * nb, 1), (u // max(E, 1)) % max(nb, 1), u % max(E, 1)
    out = {
        "id": np.asarray(list(arrays.bc_ids), dtype=object)[m],
        "rep": [f"R{r + 1}" for r in rep],
        "env": [labels[x] for x in env] if has_env else None,
        "n_steps": res["n_steps"],
    }
    for k in ("q_mean", "q_sd", "rb_mean", "rb_sd"):
        out[k] = res[k]
    with np.errstate(divide="ignore", invalid="ignore"):
        out["sd_ratio"] = res["rb_sd"] / res["q_sd"]
    out["p_pos"], out["p_neg"] = res["p_pos"], res["p_neg"]
    for i, p in enumerate(probs):
        out[f"q{100.0 * p:g}"] = res["quantiles"][:, i]
    return pd.DataFrame(out)


def hyperfitness_marginals(data: pd.DataFrame, df_advi: pd.DataFrame, *, model, model_kwargs: Optional[Dict] = None,
                           n_samples: int = 1000, probs: Sequence[float] = (0.025, 0.5, 0.975), threshold: float = 0.0, seed: int = 0,
                           id_col="barcode", time_col="time", count_col="count", neutral_col="neutral",
                           rep_col: Optional[str] = None, env_col: Optional[str] = None, genotype_col: Optional[str] = None,
                           device: int = 0, chain=None) -> pd.DataFrame:
    """`fitness_marginals` for the number a hierarchical fit is made for: the hyper-fitness theta, the fitness of a genotype
    (`genotype_fitness_normal`) or of a mutant across its replicates (`replicate_fitness_normal`,
    `multienv_replicate_fitness_normal`) -- the `bc_hyperfitness` rows of the fit's frame.  q factorises theta away from the
    theta_tilde, logtau and logsigma of every member of its group and from their loglambda rows, so its +- is the least to be
    trusted; given everything else theta's full conditional is exactly Gaussian (the prior and the members' log-frequency-ratio
    terms), and averaging it over n_samples joint draws of everything else gives the Rao-Blackwellised marginal (`bb_theta_rb`,
    one device call).  Arguments as for `fitness_marginals`; a model without a theta raises `BarBayError`.

    Returns one line per theta entry, in the order and with the labels of the frame's `bc_hyperfitness` rows: `genotype` (genotype
    model, else None), `id` and `env` (replicate kinds, else None; `env` None without environments), `n_members` (the group's
    mutants or replicates), `n_steps` (the time steps of all of them that inform theta; 0: its conditional is the prior), `q_mean`,
    `q_sd`, `rb_mean`, `rb_sd`, `sd_ratio`, `p_pos`, `p_neg` and one column per probability of `probs`, as `fitness_marginals`."""
    cols = dict(id_col=id_col, time_col=time_col, count_col=count_col, neutral_col=neutral_col, rep_col=rep_col,
                env_col=env_col, genotype_col=genotype_col)
    probs = [float(p) for p in np.atleast_1d(probs)] if probs is not None else []
    with _engine_at_fit(data, df_advi, model, model_kwargs, seed, device, cols) as (e, bayes_model, arrays, mname):
        n_groups = e.theta_rb_shape()
        if n_groups == 0:
            raise BarBayError(f"{mname} has no hyper-fitness: hyperfitness_marginals applies to the hierarchical models (fitness_marginals serves every model)")
        draws = None
        if chain is not None:
            draws = np.asarray(chain, dtype=np.float64)
            if draws.ndim not in (2, 3) or draws.shape[-1] != e.D:
                raise BarBayError(f"chain must be [walkers, steps, {e.D}] or [draws, {e.D}]")
            draws = draws.reshape(-1, e.D)
        res = e.theta_rb(n_samples=n_samples, probs=probs, threshold=threshold, seed=seed, draws=draws)
    R, nb = len(bayes_model.counts), bayes_model.n_bc
    none = np.full(n_groups, None, dtype=object)
    if "genotype" in mname:
        out = {"genotype": np.asarray(list(dict.fromkeys(arrays.genotypes)), dtype=object), "id": none, "env": none}
    else:
        E = n_groups // max(nb, 1)
        has_env, labels = _env_labels(arrays, mname, R)
        g = np.arange(n_groups)
        out = {"genotype": none, "id": np.asarray(list(arrays.bc_ids), dtype=object)[g // max(E, 1)],
               "env": np.asarray(labels, dtype=object)[g % max(E, 1)] if has_env else none}
    out["n_members"], out["n_steps"] = res["n_members"], res["n_steps"]
    for k in ("q_mean", "q_sd", "rb_mean", "rb_sd"):
        out[k] = res[k]
    with np.errstate(divide="ignore", invalid="ignore"):
        out["sd_ratio"] = res["rb_sd"] / res["q_sd"]
    out["p_pos"], out["p_neg"] = res["p_pos"], res["p_neg"]
    for i, p in enumerate(probs):
        out[f"q{100.0 * p:g}"] = res["quantiles"][:, i]
    return pd.DataFrame(out)


def _contrast_pairs(labels: List, between: str, reference) -> List[Dict]:
    """The contrasts `between` names over the element labels (tuples; the genotype model's hyper level: plain labels)."""
    from itertools import combinations
    axis = {"id": 0, "rep": 1, "env": -1, "genotype": None}[between]
    if axis is None:                                                  # every other genotype minus the reference
        if reference not in labels:
            raise BarBayError(f"reference {reference!r} is no genotype of the data")
        return [{x: 1.0, reference: -1.0} for x in labels if x != reference]
    cells: Dict = {}                                                  # the other coordinates -> the labels that differ in `axis` only
    for x in labels:
        cells.setdefault(x[:axis] + x[axis + 1:] if axis >= 0 else x[:-1], []).append(x)
    out = []
    if between == "id":
        if not any(x[0] == reference for x in labels):
            raise BarBayError(f"reference {reference!r} is no mutant of the data")
        for group in cells.values():
            ref = [x for x in group if x[0] == reference]
            out += [{x: 1.0, ref[0]: -1.0} for x in group if ref and x[0] != reference]
    else:
        for group in cells.values():
            out += [{b: 1.0, a: -1.0} for a, b in combinations(group, 2)]      # later label minus earlier
    return out


def fitness_contrasts(data: pd.DataFrame, df_advi: pd.DataFrame, *, model, level: str = "fitness", contrasts: Optional[Sequence[Dict]] = None,
                      between: Optional[str] = None, reference=None, model_kwargs: Optional[Dict] = None,
                      n_samples: int = 1000, probs: Sequence[float] = (0.025, 0.5, 0.975), threshold: float = 0.0, seed: int = 0,
                      id_col="barcode", time_col="time", count_col="count", neutral_col="neutral",
                      rep_col: Optional[str] = None, env_col: Optional[str] = None, genotype_col: Optional[str] = None,
                      device: int = 0, chain=None) -> pd.DataFrame:
    """Differences (and any other linear contrasts) of fitnesses with an honest +-: is a mutant fitter in environment B than in A,
    fitter than the wild type, do two replicates agree?  The difference of two `fitness_marginals` rows with their variances added
    is wrong: every fitness of a replicate is measured against the same population mean fitness, whose uncertainty each marginal
    carries and which cancels in a difference of two mutants of one replicate (and adds up in a sum).  Distinct fitnesses are
    conditionally independent given everything else, so the contrast's full conditional is exactly Gaussian, and averaging it over
    the joint draws gives its Rao-Blackwellised marginal (`bb_contrast_rb`, one device call).

    level "fitness": the elements are the rows of `fitness_marginals`, labelled (id, rep, env) (env None without environments);
    level "hyper": those of `hyperfitness_marginals`, labelled genotype (genotype model) or (id, env).  One call serves one level: a
    fitness and the hyper-fitness of its own group are not conditionally independent.

    Give either `contrasts`, a list of dicts {label: weight} (every label at most once per contrast), or `between`:
    "env" -- for every (id, rep) (hyper: every id) every pair of environments, later label minus earlier; "rep" -- for every
    (id, env) every pair of replicates; "id" with `reference` -- every other mutant minus the reference mutant within each
    (rep, env); "genotype" with `reference` (level "hyper", genotype model) -- every other genotype minus the reference genotype.
    The remaining arguments as for `fitness_marginals`.  At the hyper level a term re-walks its whole group for every contrast that
    names it: every genotype against a reference is cheap, all pairs of a thousand genotypes are not.

    Returns one line per contrast: `contrast` (its number), `terms` ("+1 (id, rep, env) -1 (...)"), `n_terms`, `min_steps` (the
    smallest n_steps over the terms; 0: some term's conditional is its prior), `q_mean`, `q_sd` (the draws' own contrast),
    `rb_mean`, `rb_sd`, `sd_ratio` = rb_sd / q_sd, `indep_sd` = sqrt(sum w^2 rb_sd_k^2) from the terms' own marginals at the same
    seed (what adding variances would give), `common_mode` = rb_sd / indep_sd (below 1: shared uncertainty cancels; above: it adds
    up), `p_pos`, `p_neg` (the RB probability of a contrast above / below `threshold`) and the quantile columns of
    `fitness_marginals`."""
    cols = dict(id_col=id_col, time_col=time_col, count_col=count_col, neutral_col=neutral_col, rep_col=rep_col,
                env_col=env_col, genotype_col=genotype_col)
    probs = [float(p) for p in np.atleast_1d(probs)] if probs is not None else []
    if level not in ("fitness", "hyper"):
        raise BarBayError('level must be "fitness" or "hyper"')
    if (contrasts is None) == (between is None):
        raise BarBayError("give exactly one of contrasts= and between=")
    if between is not None and between not in ("env", "rep", "id", "genotype"):
        raise BarBayError('between must be "env", "rep", "id" or "genotype"')
    with _engine_at_fit(data, df_advi, model, model_kwargs, seed, device, cols) as (e, bayes_model, arrays, mname):
        R, nb = len(bayes_model.counts), bayes_model.n_bc
        has_env, envs = _env_labels(arrays, mname, R)
        E = max(len(envs), 1) if has_env else 1
        env_of = lambda x: envs[x] if has_env else None
        ids = list(arrays.bc_ids)
        geno = "genotype" in mname
        if level == "fitness":
            labels = [(ids[m], f"R{r + 1}", env_of(x)) for r in range(R) for m in range(nb) for x in range(E)]
        elif e.theta_rb_shape() == 0:
            raise BarBayError(f'{mname} has no hyper-fitness: level="hyper" applies to the hierarchical models')
        elif geno:
            labels = list(dict.fromkeys(arrays.genotypes))
        else:
            labels = [(ids[m], env_of(x)) for m in range(nb) for x in range(E)]
        if between is not None:
            if (between == "genotype") != (geno and level == "hyper") or (between == "env" and not has_env) or (between == "rep" and (level == "hyper" or R < 2)):
                raise BarBayError(f'between="{between}" cannot be served at level "{level}" of {mname}')
            if between in ("id", "genotype") and reference is None:
                raise BarBayError(f'between="{between}" needs reference=')
            contrasts = _contrast_pairs(labels, between, reference)
        index = {x: i for i, x in enumerate(labels)}
        terms = []
        for c, con in enumerate(contrasts):
            for x in con:
                if x not in index:
                    form = "genotype" if geno and level == "hyper" else "(id, env)" if level == "hyper" else "(id, rep, env)"
                    raise BarBayError(f"contrast {c}: unknown label {x!r} (level {level!r}: {form})")
            terms.append([(index[x], float(w)) for x, w in con.items()])
        draws = None
        if chain is not None:
            draws = np.asarray(chain, dtype=np.float64)
            if draws.ndim not in (2, 3) or draws.shape[-1] != e.D:
                raise BarBayError(f"chain must be [walkers, steps, {e.D}] or [draws, {e.D}]")
            draws = draws.reshape(-1, e.D)
        kw = dict(n_samples=n_samples, threshold=threshold, seed=seed, draws=draws)
        res = e.contrast_rb(terms, space="fitness" if level == "fitness" else "theta", probs=probs, **kw)
        own = (e.fitness_rb if level == "fitness" else e.theta_rb)(probs=(), **kw)["rb_sd"]
    fmt = lambda x: "(" + ", ".join(str(v) for v in x) + ")" if isinstance(x, tuple) else str(x)
    out = {
        "contrast": np.arange(len(terms)),
        "terms": [" ".join(f"{w:+g} {fmt(labels[k])}" for k, w in t) for t in terms],
        "n_terms": [len(t) for t in terms],
        "min_steps": res["min_steps"],
    }
    for k in ("q_mean", "q_sd", "rb_mean", "rb_sd"):
        out[k] = res[k]
    out["indep_sd"] = np.asarray([math.sqrt(sum((w * own[k]) ** 2 for k, w in t)) for t in terms], dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out["sd_ratio"] = res["rb_sd"] / res["q_sd"]
        out["common_mode"] = res["rb_sd"] / out["indep_sd"]
    out["p_pos"], out["p_neg"] = res["p_pos"], res["p_neg"]
    for i, p in enumerate(probs):
        out[f"q{100.0 * p:g}"] = res["quantiles"][:, i]
    order = ["contrast", "terms", "n_terms", "min_steps", "q_mean", "q_sd", "rb_mean", "rb_sd", "sd_ratio", "indep_sd", "common_mode", "p_pos", "p_neg"]
    return pd.DataFrame({k: out[k] for k in order + [k for k in out if k not in order]})


def _fitness_sets(bayes_model, arrays, mname: str, by: str, groups: Optional[Dict]):
    """The sets of `fitness_distribution` and `fitness_ranking`: (rep, env, genotype, group) -> the set's fitness units (the rows of
    `fitness_marginals`), in unit order; and what labels a unit: (R, nb, E, ids, envs or None, genotypes or None)."""
    R, nb = len(bayes_model.counts), bayes_model.n_bc
    has_env, envs = _env_labels(arrays, mname, R)
    E = max(len(envs), 1) if has_env else 1
    ids = list(arrays.bc_ids)
    geno = arrays.genotypes if isinstance(arrays.genotypes, list) else None
    if by == "genotype" and geno is None:
        raise BarBayError('by="genotype" needs the genotypes of the mutants: give genotype_col=')
    if by == "env" and not has_env:
        raise BarBayError(f'by="env" cannot be served by {mname}: it has no environments (by="rep_env", "rep" or "all")')
    if groups is not None:
        known = set(ids)
        unknown = next((k for k in groups if k not in known), None)
        if unknown is not None:
            raise BarBayError(f"groups: {unknown!r} is no mutant of the data")
        if not groups:
            raise BarBayError("groups names no mutant")
    sets: Dict = {}                                                # (rep, env, genotype, group) -> units, in unit order
    for r in range(R):
        for m in range(nb):
            if groups is not None and ids[m] not in groups:
                continue
            for x in range(E):
                key = (f"R{r + 1}" if by in ("rep_env", "rep") else None,
                       envs[x] if has_env and by in ("rep_env", "env") else None,
                       geno[m] if by == "genotype" else None,
                       groups[ids[m]] if groups is not None else None)
                sets.setdefault(key, []).append(x + E * m + E * nb * r)
    return sets, (R, nb, E, ids, envs if has_env else None, geno)


def fitness_distribution(data: pd.DataFrame, df_advi: pd.DataFrame, *, model, by: str = "rep_env", groups: Optional[Dict] = None,
                         grid: Optional[Sequence[float]] = None, model_kwargs: Optional[Dict] = None,
                         n_samples: int = 1000, probs: Sequence[float] = (0.025, 0.5, 0.975), seed: int = 0,
                         id_col="barcode", time_col="time", count_col="count", neutral_col="neutral",
                         rep_col: Optional[str] = None, env_col: Optional[str] = None, genotype_col: Optional[str] = None,
                         device: int = 0, chain=None) -> pd.DataFrame:
    """The distribution of fitness effects of a library with an honest +-: which fraction of the lineages of an environment, a
    replicate, a genotype or a user class has a fitness below (above) x, and how sure is that curve?  It cannot be read off the
    `fitness_marginals` rows: every fitness of a replicate is measured against the same population mean fitness, whose uncertainty
    moves the whole curve left or right together -- the coupling mean-field q has cut, and the other side of `fitness_contrasts`'
    argument: there the common mode cancels, here it adds up over the set.  Per joint draw of everything else the units' exact
    Gaussian conditionals give the expected fraction below x and its (Poisson-binomial) variance; `bb_dfe_rb` averages both over
    the draws in one device call.

    `by`: one set of fitness units (the rows of `fitness_marginals`) per "rep_env" (replicate, environment), "env" (over the
    replicates), "rep" (over the environments), "genotype" (a genotype's mutants, every replicate and environment; needs
    `genotype_col`) or "all".  `groups`: a dict mutant label -> class; every set is then split by class and mutants it does not name
    are left out.  `grid`: ascending thresholds x, at most 64; default 32 equally spaced points from min(mean - 3 std) to
    max(mean + 3 std) over the `bc_fitness` rows of `df_advi`.  The remaining arguments as for `fitness_marginals`.

    Returns one line per (set, grid point): the set's labels `rep`, `env`, `genotype`, `group` (None where the set spans them),
    `n_units`, `x`, `below_mean`, `above_mean` (the posterior mean of the fraction at or below / above x), `between_sd` (its sd
    between the draws: what the units share), `within_sd` (sqrt of the mean conditional variance: what each unit's own conditional
    leaves open), `q_below_mean`, `q_below_sd` (the ECDF of q's own draws at x: mean and sd over the draws), `total_sd` =
    sqrt(between_sd^2 + within_sd^2), `common_mode` = between_sd / within_sd (above 1: the shared part dominates) and, per
    probability of `probs`, the quantiles over the draws of the fraction below and above x: below_q2.5, ..., above_q2.5, ..."""
    cols = dict(id_col=id_col, time_col=time_col, count_col=count_col, neutral_col=neutral_col, rep_col=rep_col,
                env_col=env_col, genotype_col=genotype_col)
    probs = [float(p) for p in np.atleast_1d(probs)] if probs is not None else []
    if by not in ("rep_env", "env", "rep", "genotype", "all"):
        raise BarBayError('by must be "rep_env", "env", "rep", "genotype" or "all"')
    if grid is None:
        fit = df_advi[df_advi["vartype"] == "bc_fitness"] if "vartype" in df_advi else df_advi.iloc[:0]
        if len(fit) == 0:
            raise BarBayError("df_advi has no bc_fitness rows to span a default grid: give grid=")
        lo, hi = float((fit["mean"] - 3.0 * fit["std"]).min()), float((fit["mean"] + 3.0 * fit["std"]).max())
        if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
            raise BarBayError("the bc_fitness rows of df_advi span no finite range: give grid=")
        grid = np.linspace(lo, hi, 32)
    grid = np.asarray(grid, dtype=np.float64).reshape(-1)
    if grid.shape[0] < 1 or grid.shape[0] > 64 or not np.all(np.isfinite(grid)) or not np.all(np.diff(grid) > 0):
        raise BarBayError("grid must hold 1 to 64 finite, strictly ascending thresholds")
    with _engine_at_fit(data, df_advi, model, model_kwargs, seed, device, cols) as (e, bayes_model, arrays, mname):
        sets, _labels = _fitness_sets(bayes_model, arrays, mname, by, groups)
        draws = None
        if chain is not None:
            draws = np.asarray(chain, dtype=np.float64)
            if draws.ndim not in (2, 3) or draws.shape[-1] != e.D:
                raise BarBayError(f"chain must be [walkers, steps, {e.D}] or [draws, {e.D}]")
            draws = draws.reshape(-1, e.D)
        keys = list(sets)
        res = e.dfe_rb([sets[k] for k in keys], grid, probs=probs, n_samples=n_samples, seed=seed, draws=draws)
    ns, ng = len(keys), grid.shape[0]
    out = {name: np.repeat(np.asarray([k[i] for k in keys], dtype=object), ng) for i, name in enumerate(("rep", "env", "genotype", "group"))}
    out["n_units"] = np.repeat(res["n_units"], ng)
    out["x"] = np.tile(grid, ns)
    for k in ("below_mean", "above_mean", "between_sd", "within_sd", "q_below_mean", "q_below_sd"):
        out[k] = res[k].reshape(-1)
    out["total_sd"] = np.sqrt(out["between_sd"] ** 2 + out["within_sd"] ** 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        out["common_mode"] = out["between_sd"] / out["within_sd"]
    for side in ("below", "above"):
        for i, p in enumerate(probs):
            out[f"{side}_q{100.0 * p:g}"] = res[f"{side}_bands"][:, :, i].reshape(-1)
    return pd.DataFrame(out)


def fitness_ranking(data: pd.DataFrame, df_advi: pd.DataFrame, *, model, by: str = "rep_env", groups: Optional[Dict] = None,
                    top: Sequence[int] = (1, 10), probs: Sequence[float] = (0.025, 0.5, 0.975), source: str = "conditional",
                    model_kwargs: Optional[Dict] = None, n_samples: int = 1000, seed: int = 0,
                    id_col="barcode", time_col="time", count_col="count", neutral_col="neutral",
                    rep_col: Optional[str] = None, env_col: Optional[str] = None, genotype_col: Optional[str] = None,
                    device: int = 0, chain=None) -> pd.DataFrame:
    """Which lineages are the fittest, and how sure is that list?  A rank is a function of all the fitnesses of a set at once, so
    it needs joint draws -- and mean-field q's own are the wrong ones: q has cut every coupling, so ranks formed from them are
    overconfident wherever units share something (a replicate's population mean fitness; theta and tau of the hierarchical models).
    Given everything else the fitness units are conditionally independent with exactly Gaussian conditionals, so redrawing every
    unit of a joint draw from its conditional is one exact blocked Gibbs update of the whole fitness block, the joint draw with the
    shared uncertainty back in it; `bb_fitness_rank` ranks every set on every such draw in one device call.

    `by`, `groups`: the sets, exactly as for `fitness_distribution`.  `top`: list lengths k (at most 8); `probs`: quantiles of the
    rank over the draws; `source`: "conditional" (the redraw) or "draws" (q's own draws, or the chain's: what the coupling adds is
    the difference between the two).  The remaining arguments as for `fitness_marginals`.

    Returns one line per (set, unit), the sets in `fitness_distribution`'s order and a set's units in unit order: `id`, `rep`,
    `env` (the unit's own; None without environments), `genotype` (None without genotypes), `group` (None without `groups`),
    `n_units` (the size of the set the line belongs to: the one the columns `by` names and `group` identify), `rank` (1-based
    position within the set by `rank_mean`, ties by unit order), `rank_mean` (1-based: 1 is the fittest), `rank_sd`, one column
    rank_q2.5, rank_q50, ... per probability (1-based) and one column p_top1, p_top10, ... per k: the posterior probability that
    the unit is among the k fittest of its set."""
    cols = dict(id_col=id_col, time_col=time_col, count_col=count_col, neutral_col=neutral_col, rep_col=rep_col,
                env_col=env_col, genotype_col=genotype_col)
    probs = [float(p) for p in np.atleast_1d(probs)] if probs is not None else []
    if by not in ("rep_env", "env", "rep", "genotype", "all"):
        raise BarBayError('by must be "rep_env", "env", "rep", "genotype" or "all"')
    if source not in ("conditional", "draws"):
        raise BarBayError('source must be "conditional" or "draws"')
    tops = list(np.atleast_1d(top).reshape(-1)) if top is not None else []
    if any(not isinstance(k, (int, np.integer)) or isinstance(k, (bool, np.bool_)) for k in tops):
        raise BarBayError("top must hold whole list lengths")
    tops = [int(k) for k in tops]
    if len(tops) > 8 or any(k < 1 or k > 2 ** 31 - 1 for k in tops) or len(set(tops)) != len(tops):
        raise BarBayError("top must hold at most 8 distinct list lengths k, each in 1 .. 2^31 - 1")
    with _engine_at_fit(data, df_advi, model, model_kwargs, seed, device, cols) as (e, bayes_model, arrays, mname):
        sets, (R, nb, E, ids, envs, geno) = _fitness_sets(bayes_model, arrays, mname, by, groups)
        draws = None
        if chain is not None:
            draws = np.asarray(chain, dtype=np.float64)
            if draws.ndim not in (2, 3) or draws.shape[-1] != e.D:
                raise BarBayError(f"chain must be [walkers, steps, {e.D}] or [draws, {e.D}]")
            draws = draws.reshape(-1, e.D)
        keys = list(sets)
        res = e.fitness_rank([sets[k] for k in keys], top=tops, probs=probs, source=source, n_samples=n_samples, seed=seed, draws=draws)
    u = np.concatenate([np.asarray(sets[k], dtype=np.int64) for k in keys])
    rep, m, env = u // (E * nb), (u // E) % nb, u % E
    ptr = res["set_ptr"]
    rank = np.empty(u.shape[0], dtype=np.int64)
    for c in range(len(keys)):
        a, b = int(ptr[c]), int(ptr[c + 1])
        rank[a + np.argsort(res["rank_mean"][a:b], kind="stable")] = np.arange(1, b - a + 1)
    out = {
        "id": np.asarray(ids, dtype=object)[m],
        "rep": [f"R{r + 1}" for r in rep],
        "env": [envs[x] for x in env] if envs is not None else None,
        "genotype": [geno[x] for x in m] if geno is not None else None,
        "group": [groups[ids[x]] for x in m] if groups is not None else None,
        "n_units": np.repeat(res["n_units"], np.diff(ptr)),
        "rank": rank,
        "rank_mean": res["rank_mean"] + 1.0,
        "rank_sd": res["rank_sd"],
    }
    for i, p in enumerate(probs):
        out[f"rank_q{100.0 * p:g}"] = res["quantiles"][:, i] + 1.0
    for i, k in enumerate(tops):
        out[f"p_top{k}"] = res["p_top"][:, i]
    return pd.DataFrame(out)


def popmean_marginals(data: pd.DataFrame, df_advi: pd.DataFrame, *, model, model_kwargs: Optional[Dict] = None,
                      n_samples: int = 1000, probs: Sequence[float] = (0.025, 0.5, 0.975), threshold: float = 0.0, seed: int = 0,
                      id_col="barcode", time_col="time", count_col="count", neutral_col="neutral",
                      rep_col: Optional[str] = None, env_col: Optional[str] = None, genotype_col: Optional[str] = None,
                      device: int = 0, chain=None) -> pd.DataFrame:
    """`fitness_marginals` for the population mean fitness -- the `pop_mean_fitness` rows of the fit's frame, the quantity every
    mutant's fitness is relative to and the one latent every barcode's log-frequency-ratio term reads.  q factorises it away from
    all of them; given everything else its full conditional is exactly Gaussian in every model (the prior and the terms of every
    barcode of the replicate at the step, neutrals and mutants), and averaging it over n_samples joint draws of everything else
    gives the Rao-Blackwellised marginal (`bb_popmean_rb`, one device call).  Arguments as for `fitness_marginals`.

    Returns one line per `pop_mean_fitness` row of the frame, in that order and with those rows' own labels (every column of the
    frame but `mean` and `std`); then `n_members` (neutrals + mutants), `q_mean`, `q_sd`, `rb_mean`, `rb_sd`, `sd_ratio`, `p_pos`,
    `p_neg` and one column per probability of `probs`, as `hyperfitness_marginals`."""
    cols = dict(id_col=id_col, time_col=time_col, count_col=count_col, neutral_col=neutral_col, rep_col=rep_col,
                env_col=env_col, genotype_col=genotype_col)
    probs = [float(p) for p in np.atleast_1d(probs)] if probs is not None else []
    with _engine_at_fit(data, df_advi, model, model_kwargs, seed, device, cols) as (e, bayes_model, arrays, mname):
        n_groups = e.popmean_rb_shape()
        draws = None
        if chain is not None:
            draws = np.asarray(chain, dtype=np.float64)
            if draws.ndim not in (2, 3) or draws.shape[-1] != e.D:
                raise BarBayError(f"chain must be [walkers, steps, {e.D}] or [draws, {e.D}]")
            draws = draws.reshape(-1, e.D)
        blk = df_advi.iloc[:e.D]
        blk = blk[blk["vartype"] == "pop_mean_fitness"]
        if len(blk) != n_groups:
            raise BarBayError(f"df_advi holds {len(blk)} pop_mean_fitness rows, the model has {n_groups}")
        res = e.popmean_rb(n_samples=n_samples, probs=probs, threshold=threshold, seed=seed, draws=draws)
    out = blk.drop(columns=["mean", "std"]).reset_index(drop=True)
    out["n_members"] = res["n_members"]
    for k in ("q_mean", "q_sd", "rb_mean", "rb_sd"):
        out[k] = res[k]
    with np.errstate(divide="ignore", invalid="ignore"):
        out["sd_ratio"] = res["rb_sd"] / res["q_sd"]
    out["p_pos"], out["p_neg"] = res["p_pos"], res["p_neg"]
    for i, p in enumerate(probs):
        out[f"q{100.0 * p:g}"] = res["quantiles"][:, i]
    return out


def noise_marginals(data: pd.DataFrame, df_advi: pd.DataFrame, *, model, block: str = "bc", model_kwargs: Optional[Dict] = None,
                    n_samples: int = 1000, probs: Sequence[float] = (0.025, 0.5, 0.975), seed: int = 0,
                    id_col="barcode", time_col="time", count_col="count", neutral_col="neutral",
                    rep_col: Optional[str] = None, env_col: Optional[str] = None, genotype_col: Optional[str] = None,
                    device: int = 0, chain=None) -> pd.DataFrame:
    """`fitness_marginals` for the noise scales: `block="bc"` the `bc_std` rows of the fit's frame (logsigma of a mutant's
    log-frequency-ratio terms), `block="pop"` the `pop_std` rows (logsigma of a time step's neutral terms) -- the numbers that say
    which barcodes and which time steps are noisy, and the latents where a mean-field Gaussian is at its worst: too narrow, and
    symmetric on the log scale where the true marginal is skewed.  The full conditional of a log-scale is not Gaussian but
    one-dimensional and log-concave; it is integrated numerically per draw and averaged over n_samples joint draws of everything
    else (`bb_logsigma_rb`, one device call; at most 5781 draws).  Arguments as for `fitness_marginals`, without a threshold.

    Returns one line per row of the block, in the frame's order and with those rows' own labels (every column of the frame but
    `mean` and `std`); then `n_terms` (the terms that inform the scale; 0: its conditional is the prior), `q_mean`, `q_sd` (the
    draws' own logsigma), `rb_mean`, `rb_sd`, `sd_ratio` = rb_sd / q_sd, `mode_mean`, `sigma_mean` (the RB mean of sigma itself), one
    column per probability of `probs` named q2.5, q50, ... (quantiles of logsigma) and their exp as sigma_q2.5, sigma_q50, ..."""
    if block not in ("bc", "pop"):
        raise BarBayError(f"block must be 'bc' or 'pop', got {block!r}")
    cols = dict(id_col=id_col, time_col=time_col, count_col=count_col, neutral_col=neutral_col, rep_col=rep_col,
                env_col=env_col, genotype_col=genotype_col)
    probs = [float(p) for p in np.atleast_1d(probs)] if probs is not None else []
    vartype = "bc_std" if block == "bc" else "pop_std"
    with _engine_at_fit(data, df_advi, model, model_kwargs, seed, device, cols) as (e, bayes_model, arrays, mname):
        n_entries = e.logsigma_rb_shape(block)
        draws = None
        if chain is not None:
            draws = np.asarray(chain, dtype=np.float64)
            if draws.ndim not in (2, 3) or draws.shape[-1] != e.D:
                raise BarBayError(f"chain must be [walkers, steps, {e.D}] or [draws, {e.D}]")
            draws = draws.reshape(-1, e.D)
        blk = df_advi.iloc[:e.D]
        blk = blk[blk["vartype"] == vartype]
        if len(blk) != n_entries:
            raise BarBayError(f"df_advi holds {len(blk)} {vartype} rows, the model has {n_entries}")
        res = e.logsigma_rb(block=block, n_samples=n_samples, probs=probs, seed=seed, draws=draws)
    out = blk.drop(columns=["mean", "std"]).reset_index(drop=True)
    out["n_terms"] = res["n_terms"]
    for k in ("q_mean", "q_sd", "rb_mean", "rb_sd"):
        out[k] = res[k]
    with np.errstate(divide="ignore", invalid="ignore"):
        out["sd_ratio"] = res["rb_sd"] / res["q_sd"]
    out["mode_mean"], out["sigma_mean"] = res["mode_mean"], res["sigma_mean"]
    for i, p in enumerate(probs):
        out[f"q{100.0 * p:g}"] = res["quantiles"][:, i]
    for i, p in enumerate(probs):
        out[f"sigma_q{100.0 * p:g}"] = np.exp(res["quantiles"][:, i])
    return out


def deviation_marginals(data: pd.DataFrame, df_advi: pd.DataFrame, *, model, mode: str = "collapsed", model_kwargs: Optional[Dict] = None,
                        n_samples: int = 1000, probs: Sequence[float] = (0.025, 0.5, 0.975), seed: int = 0,
                        id_col="barcode", time_col="time", count_col="count", neutral_col="neutral",
                        rep_col: Optional[str] = None, env_col: Optional[str] = None, genotype_col: Optional[str] = None,
                        device: int = 0, chain=None) -> pd.DataFrame:
    """`fitness_marginals` for logtau, the deviation scale of the hierarchical models (the `bc_deviations` rows of the fit's frame):
    how far a barcode or a replicate stands off its group, and the block where a mean-field Gaussian is least trustworthy -- the
    fitness is theta + exp(logtau) theta_tilde, so logtau and theta_tilde enter the likelihood through their product only.
    `mode="collapsed"` (the default) integrates theta_tilde out against its prior: the hierarchical-variance posterior;
    `mode="full"` is the full conditional given everything else, theta_tilde included.  Neither is log-concave and either can have
    two modes, one at the prior and one at the least-squares tau; the conditional is integrated numerically per draw on one grid
    over all of them and averaged over n_samples joint draws of everything else (`bb_logtau_rb`, one device call; at most 5781
    draws).  Arguments as for `fitness_marginals`, without a threshold.  A model without a logtau raises `BarBayError`.

    Returns one line per logtau row, in the frame's order and with those rows' own labels (every column of the frame but `mean`
    and `std`); then `n_terms` (0: the conditional is the prior), `q_mean`, `q_sd` (the draws' own logtau), `rb_mean`, `rb_sd`,
    `sd_ratio` = rb_sd / q_sd, `mode_mean`, `tau_mean` (the RB mean of tau itself), `pool_mean` (of 1 / (1 + n w tau^2): 1 the unit
    sits on its group, 0 it is on its own), `n_two_modes` (the draws whose conditional kept two modes), one column per probability
    of `probs` named q2.5, q50, ... (quantiles of logtau) and their exp as tau_q2.5, tau_q50, ..."""
    if mode not in ("full", "collapsed"):
        raise BarBayError(f"mode must be 'full' or 'collapsed', got {mode!r}")
    cols = dict(id_col=id_col, time_col=time_col, count_col=count_col, neutral_col=neutral_col, rep_col=rep_col,
                env_col=env_col, genotype_col=genotype_col)
    probs = [float(p) for p in np.atleast_1d(probs)] if probs is not None else []
    with _engine_at_fit(data, df_advi, model, model_kwargs, seed, device, cols) as (e, bayes_model, arrays, mname):
        n_entries = e.logtau_rb_shape()
        if n_entries == 0:
            raise BarBayError(f"deviation_marginals applies to the hierarchical models only: {mname} has no logtau")
        draws = None
        if chain is not None:
            draws = np.asarray(chain, dtype=np.float64)
            if draws.ndim not in (2, 3) or draws.shape[-1] != e.D:
                raise BarBayError(f"chain must be [walkers, steps, {e.D}] or [draws, {e.D}]")
            draws = draws.reshape(-1, e.D)
        blk = df_advi.iloc[:e.D]
        blk = blk[blk["vartype"] == "bc_deviations"]
        if len(blk) != n_entries:
            raise BarBayError(f"df_advi holds {len(blk)} bc_deviations rows, the model has {n_entries}")
        res = e.logtau_rb(mode=mode, n_samples=n_samples, probs=probs, seed=seed, draws=draws)
    out = blk.drop(columns=["mean", "std"]).reset_index(drop=True)
    out["n_terms"] = res["n_terms"]
    for k in ("q_mean", "q_sd", "rb_mean", "rb_sd"):
        out[k] = res[k]
    with np.errstate(divide="ignore", invalid="ignore"):
        out["sd_ratio"] = res["rb_sd"] / res["q_sd"]
    for k in ("mode_mean", "tau_mean", "pool_mean", "n_two_modes"):
        out[k] = res[k]
    for i, p in enumerate(probs):
        out[f"q{100.0 * p:g}"] = res["quantiles"][:, i]
    for i, p in enumerate(probs):
        out[f"tau_q{100.0 * p:g}"] = np.exp(res["quantiles"][:, i])
    return out


def abundance_marginals(data: pd.DataFrame, df_advi: pd.DataFrame, *, model, barcodes: Optional[Sequence] = None,
                        model_kwargs: Optional[Dict] = None, n_samples: int = 1000, probs: Sequence[float] = (0.025, 0.5, 0.975), seed: int = 0,
                        id_col="barcode", time_col="time", count_col="count", neutral_col="neutral",
                        rep_col: Optional[str] = None, env_col: Optional[str] = None, genotype_col: Optional[str] = None,
                        device: int = 0, chain=None) -> pd.DataFrame:
    """`fitness_marginals` for the log-rates loglambda (the `log_poisson` rows of the fit's frame, most of its latents): which
    low-count trajectories the fit's frequency bands can be trusted for.  For a barcode read a handful of times the full conditional
    of its log-rate is skewed like a log-gamma density and need not have a single mode; mean-field gives it a symmetric +- and cuts
    its coupling to the barcode's fitness, to the noise scale and, through the time point's normaliser, to every other barcode.  The
    conditional is integrated numerically per draw on one grid over all its modes and averaged over n_samples joint draws of
    everything else (`bb_loglambda_rb`, one device call; at most 5781 draws).  `barcodes`: the ids wanted (every replicate of them;
    default all) -- the conditionals still read every barcode.  Other arguments as for `noise_marginals`.

    Returns one line per (id, rep, time point), in the frame's order and with those rows' own labels (every column of the frame but
    `mean` and `std`); then `time` (0-based index of the time point), `n_reads` (the observed count), `n_sides` (the steps that
    bound the time point), `q_mean`, `q_sd` (the draws' own loglambda), `rb_mean`, `rb_sd`, `sd_ratio` = rb_sd / q_sd,
    `lambda_mean` (the RB mean of lambda itself), `mode_mean` and one column per probability of `probs` named q2.5, q50, ...
    (quantiles of loglambda)."""
    cols = dict(id_col=id_col, time_col=time_col, count_col=count_col, neutral_col=neutral_col, rep_col=rep_col,
                env_col=env_col, genotype_col=genotype_col)
    probs = [float(p) for p in np.atleast_1d(probs)] if probs is not None else []
    with _engine_at_fit(data, df_advi, model, model_kwargs, seed, device, cols) as (e, bayes_model, arrays, mname):
        n_rows, n_cols = e.loglambda_rb_shape()
        draws = None
        if chain is not None:
            draws = np.asarray(chain, dtype=np.float64)
            if draws.ndim not in (2, 3) or draws.shape[-1] != e.D:
                raise BarBayError(f"chain must be [walkers, steps, {e.D}] or [draws, {e.D}]")
            draws = draws.reshape(-1, e.D)
        Ts = [np.asarray(c).shape[0] for c in bayes_model.counts]
        R = len(Ts)
        B = n_rows // R
        blk = df_advi.iloc[:e.D]
        blk = blk[blk["vartype"] == "log_poisson"]
        if len(blk) != B * sum(Ts):
            raise BarBayError(f"df_advi holds {len(blk)} log_poisson rows, the model has {B * sum(Ts)}")
        rows = None
        if barcodes is not None:
            ids = list(arrays.neutral_ids) + list(arrays.bc_ids)          # the data columns: neutrals first
            want = set(barcodes)
            missing = want - set(ids)
            if missing:
                raise BarBayError(f"barcodes not in the data: {sorted(missing, key=str)[:5]}")
            colsel = [b for b, x in enumerate(ids) if x in want]
            rows = np.array([r * B + b for r in range(R) for b in colsel], dtype=np.int64)
        res = e.loglambda_rb(n_samples=n_samples, probs=probs, seed=seed, draws=draws, rows=rows)
    rr = np.arange(n_rows) if rows is None else rows
    rep, col = rr // B, rr % B
    T_of = np.asarray(Ts)[rep]
    start = np.concatenate([[0], np.cumsum(np.asarray(Ts) * B)])[rep] + col * T_of      # the row's first line in the block
    live = np.arange(n_cols)[None, :] < T_of[:, None]
    at = (start[:, None] + np.arange(n_cols)[None, :])[live]
    out = blk.drop(columns=["mean", "std"]).iloc[at].reset_index(drop=True)
    out["time"] = np.broadcast_to(np.arange(n_cols)[None, :], live.shape)[live]
    for k in ("n_reads", "n_sides", "q_mean", "q_sd", "rb_mean", "rb_sd"):
        out[k] = res[k][live]
    with np.errstate(divide="ignore", invalid="ignore"):
        out["sd_ratio"] = res["rb_sd"][live] / res["q_sd"][live]
    out["lambda_mean"], out["mode_mean"] = res["lambda_mean"][live], res["mode_mean"][live]
    for i, p in enumerate(probs):
        out[f"q{100.0 * p:g}"] = res["quantiles"][..., i][live]
    return out


def pit_histogram(scores: pd.DataFrame, bins: int = 10) -> pd.DataFrame:
    """Calibration of the predictive: counts of the `pit` column of `logfreq_ratio_ppc_scores` in `bins` equal bins of [0, 1], for
    the neutral and the mutant barcodes separately (unscored lines left out).  Flat: calibrated; U-shaped: the predictive is too
    narrow (how mean-field ADVI fails); a hump: too wide.  Returns one line per bin: `lower`, `upper`, `neutral`, `mutant`."""
    if bins < 1:
        raise BarBayError("bins must be >= 1")
    edges = np.linspace(0.0, 1.0, bins + 1)
    pit = scores["pit"].to_numpy(dtype=np.float64)
    neu = scores["neutral"].to_numpy(dtype=bool)
    ok = ~np.isnan(pit)
    return pd.DataFrame({
        "lower": edges[:-1],
        "upper": edges[1:],
        "neutral": np.histogram(pit[ok & neu], bins=edges)[0],
        "mutant": np.histogram(pit[ok & ~neu], bins=edges)[0],
    })
