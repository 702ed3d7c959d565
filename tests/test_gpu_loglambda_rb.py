"""bb_loglambda_rb (Rao-Blackwellised loglambda marginals, barbay.jl_amd/csrc/bb_llrb.h) on the device: the emulation's cases and
the golden at the sample cap, the identity also against the device's own gradient, a statistical check against independent numpy
draws, and the user entry point end to end."""
import os

import numpy as np
import pandas as pd
import pytest

import _loglambda_rb_cases as lc

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("name", sorted(lc.golden_cases()))
def test_marginals_match_golden(hip_lib, name):
    lc.check_golden(hip_lib, name, "device")


def test_two_kept_modes_match_golden(hip_lib):
    lc.check_bimodal(hip_lib, "device")


@pytest.mark.parametrize("name", lc.IDENTITY)
def test_derivative_at_the_draw_is_the_gradient_of_the_log_joint(hip_lib, name):
    lc.check_identity(hip_lib, name, device=True)


def test_rows_subset_equals_the_rows_of_the_full_call(hip_lib):
    lc.check_rows_subset(hip_lib)


def test_no_rows_means_every_row(hip_lib):
    lc.check_all_rows(hip_lib)


def test_independent_of_launch_mode_and_repeatable(hip_lib):
    lc.check_launch_modes(hip_lib)


@pytest.mark.parametrize("name", lc.GROUP_CASES)
def test_group_handle_equals_single_device(hip_lib, name):
    lc.check_group_handle(hip_lib, name)


def test_buffer_reuse_across_calls_and_sizes(hip_lib):
    lc.check_buffer_reuse(hip_lib)


def test_handle_untouched(hip_lib):
    lc.check_handle_untouched(hip_lib)


@pytest.mark.parametrize("name", ["genotype_regrouped", "multienv_replicate", "replicate_ragged_method", "fitness_matrix_prior"])
def test_own_draws_equal_the_same_draws_passed_in(hip_lib, name):
    lc.check_internal_against_explicit_draws(hip_lib, name)


def test_nan_stays_in_the_entries_that_read_it(hip_lib):
    lc.check_nan_stays(hip_lib)


def test_loglambda_rb_errors(hip_lib):
    lc.check_errors(hip_lib)


def test_marginal_against_a_large_numpy_sample(hip_lib):
    lc.check_statistics(hip_lib)


def test_abundance_marginals_end_to_end():
    """`stats.abundance_marginals` on a short fit of the single-dataset example with one barcode's counts cut to <= 3 before the fit:
    one line per log_poisson row of the fit frame, labelled as the frame labels them, in their order, all finite, quantiles ordered;
    `barcodes=` gives the same lines as the full frame holds; a chain of the wrong width is refused; and, a sign only, the low-count
    barcode's rb_sd is at least the median's at every time point."""
    import barbay_jl_amd as bb
    data = pd.read_csv(os.path.join(GOLD, "data001_single.csv"))
    mutants = [b for b in data["barcode"].unique() if not data.loc[data["barcode"] == b, "neutral"].iloc[0]]
    low = mutants[3]
    sel = data["barcode"] == low
    data.loc[sel, "count"] = np.minimum(data.loc[sel, "count"], np.resize([0, 1, 3], int(sel.sum())))
    model = bb.model.fitness_normal
    df = bb.vi.advi(data=data, model=model, advi=bb.vi.ADVI(1, 200), verbose=False, seed=1)
    out = bb.stats.abundance_marginals(data, df, model=model, n_samples=64, seed=3)
    blk = df[df["vartype"] == "log_poisson"].reset_index(drop=True)
    probs = ["q2.5", "q50", "q97.5"]
    labels = [c for c in blk.columns if c not in ("mean", "std")]
    tail = ["time", "n_reads", "n_sides", "q_mean", "q_sd", "rb_mean", "rb_sd", "sd_ratio", "lambda_mean", "mode_mean"] + probs
    assert list(out.columns) == labels + tail and len(out) == len(blk) > 0
    for c in labels:
        assert list(out[c]) == list(blk[c]), c
    assert np.isfinite(out[tail].to_numpy(dtype=np.float64)).all()
    assert (out["rb_sd"] > 0).all() and (out["q_sd"] > 0).all() and out["n_sides"].isin([1, 2]).all()
    T = data["time"].nunique()
    assert list(out["time"][:T]) == list(range(T)) and (out["n_sides"][out["time"].isin([0, T - 1])] == 1).all()
    cnt = data.pivot(index="barcode", columns="time", values="count")
    first = out.iloc[:T]
    assert list(first["n_reads"]) == [int(v) for v in cnt.loc[first["id"].iloc[0]].sort_index()]
    assert (np.diff(out[probs].to_numpy(), axis=1) > 0).all() and (out["lambda_mean"] > 0).all()
    print("sd_ratio: median", out["sd_ratio"].median(), "min", out["sd_ratio"].min(), "max", out["sd_ratio"].max())
    some = [low, mutants[0], data.loc[data["neutral"], "barcode"].iloc[0]]
    sub = bb.stats.abundance_marginals(data, df, model=model, barcodes=some, n_samples=64, seed=3)
    ref = out[out["id"].isin(some)].reset_index(drop=True)
    assert len(sub) == 3 * T
    pd.testing.assert_frame_equal(sub, ref, check_exact=True)
    lows = out[out["id"] == low]
    assert (lows["n_reads"] <= 3).all() and (lows["rb_sd"].to_numpy() >= out["rb_sd"].median()).all()
    with pytest.raises(bb.BarBayError):
        bb.stats.abundance_marginals(data, df, model=model, chain=np.zeros((4, len(blk))))
    with pytest.raises(bb.BarBayError):
        bb.stats.abundance_marginals(data, df, model=model, barcodes=["no such barcode"])


def test_abundance_marginals_several_replicates_of_unequal_length():
    """The replicate example with the last time point of its second replicate removed: the lines follow the log_poisson rows of the
    fit frame through replicates of unequal length (labels, `rep` among them, in the frame's order), `time` restarts per barcode
    and replicate, n_reads is the data's count of (id, rep, time point), and `barcodes=` picks every replicate of an id."""
    import barbay_jl_amd as bb
    data = pd.read_csv(os.path.join(GOLD, "data002_hier-rep.csv"))
    reps = sorted(data["rep"].unique())
    data = data[~((data["rep"] == reps[1]) & (data["time"] == data["time"].max()))].reset_index(drop=True)
    model = bb.model.replicate_fitness_normal
    df = bb.vi.advi(data=data, model=model, advi=bb.vi.ADVI(1, 100), verbose=False, seed=1, rep_col="rep")
    out = bb.stats.abundance_marginals(data, df, model=model, n_samples=16, seed=3, rep_col="rep", probs=(0.5,))
    blk = df[df["vartype"] == "log_poisson"].reset_index(drop=True)
    labels = [c for c in blk.columns if c not in ("mean", "std")]
    assert len(out) == len(blk) == len(data)
    for c in labels:
        assert list(out[c]) == list(blk[c]), c
    Ts = {r: data.loc[data["rep"] == r, "time"].nunique() for r in reps}
    assert len(set(Ts.values())) == 2
    key = data.sort_values("time").groupby(["barcode", "rep"])["count"].apply(list)
    for (bc, r), grp in out.groupby(["id", "rep"], sort=False):
        assert list(grp["time"]) == list(range(Ts[r])) and list(grp["n_reads"]) == key[(bc, r)], (bc, r)
        assert list(grp["n_sides"]) == [1] + [2] * (Ts[r] - 2) + [1]
    assert np.isfinite(out[["rb_mean", "rb_sd", "q50"]].to_numpy()).all()
    some = [out["id"].iloc[-1], out["id"].iloc[0]]
    sub = bb.stats.abundance_marginals(data, df, model=model, barcodes=some, n_samples=16, seed=3, rep_col="rep", probs=(0.5,))
    pd.testing.assert_frame_equal(sub, out[out["id"].isin(some)].reset_index(drop=True), check_exact=True)
    assert len(sub) == 2 * sum(Ts.values())
