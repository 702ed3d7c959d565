"""bb_logsigma_rb (Rao-Blackwellised noise-scale marginals, barbay.jl_amd/csrc/bb_lsrb.h) restated in numpy from the rule of
include/barbay_hip.h, and the cases the emulation and GPU tests share.  The draws, their keying and the normalisers are `_rb_cases`';
the BC block's entries are bb_fitness_rb's units, the POP block's entries bb_popmean_rb's groups (neutral members only).

Expected values: tests/golden/logsigma_rb_<block>_<case>_n<samples>.npz, a 50-digit mpmath evaluation of the SAME rule (Newton in the
log domain, the trapezoid grid with its refinement m_j and right extent r_j, the Euler-Maclaurin-corrected CDF, the 40-step bisection) on this restatement's float64 per-draw
inputs (l_j, SS_j, n, a, 1/b^2), written by tests/golden/make_logsigma_rb_golden.py.  The moments have a golden at every n_samples
for the entries `golden_cases` names.  A 50-digit bisection costs 40 x 3 CDFs of 129 nodes or more per draw, so the quantiles have a
50-digit golden at n_samples = 2 (three entries) and 111 (one entry) and are compared with the float64 restatement elsewhere (two
entries).
Bounds, by `_rb_cases`' construction (relative to max(|x|, 1)): the larger of 1e-12 and 8 x the float64 restatement's own measured
error against the goldens (MEASURED / Q_MEASURED below).  n_terms and the NaN pattern are exact.

Inputs: `_rb_cases.params` -- loglambda means at ln(count + 1/2), posterior sd 0.03 -- so the residuals d_t are the data's: over the
cases |d_t| lies between about 1e-3 and 3, far above the rounding of the cancelling difference (1e-16 x |ln Z| ~ 1e-15), and SS_j
between about 1e-4 and 40.  d_t is still a cancelling difference, and SS enters the mode through ln SS: the amplification shows in
`rb_mean` / `mode_mean` (see the table), not in `rb_sd`.

The rule against the truth (check 2): tests/golden/logsigma_rb_truth.npz holds, for per-draw (n, SS, a, b) taken from the cases and
14 further parameter sets (n 0 .. 1000, SS 1e-300 .. 1e6, b 0.2 .. 3), `mpmath.quad` of the density itself at 40 digits: ln Z, E, V and the CDF at l* + {-2.3, -0.7, 0.11,
1.9, 4.4} delta.  `check_truth` compares the float64 restatement with it: 4e-12 (E in units of delta; ln Z absolute; V relative)
and 3e-5 absolute for the CDF; what the sets give is in `check_truth`'s docstring.

Measured, largest error over a case's entries against the golden, float64 restatement / host emulation / MI355X, in units of 1e-16
(each test prints its own line;
'-': the emulation does not run the case, its entries times draws being too many for a quick test; the device run is kept in
profiles/logsigma_rb/gpu_logsigma_rb_tests.log, the table in errors.txt there):

case                                                    q_mean                  q_sd               rb_mean                 rb_sd            sigma_mean             mode_mean             quantiles
bc_fitness_chunk_n111                          3.8/    -/  3.8       0.1/    -/  0.1       2.7/    -/  5.4       1.1/    -/  1.1       1.1/    -/  0.6       2.5/    -/  3.2      10.3/    -/ 10.3
bc_fitness_chunk_n2                            0.0/  0.0/  0.0       0.0/  1.1/  1.1       2.0/  2.0/  2.0       3.3/  3.3/  3.3       2.8/  2.8/  2.8       2.0/  2.0/  2.0       7.0/  7.0/  7.0
bc_fitness_matrix_prior_n1000                  1.9/  5.8/  5.8       0.1/  0.1/  0.1       2.0/  2.0/  2.0       1.1/  1.1/  1.1       1.5/  1.5/  1.5       2.5/  3.8/  3.8         -/202.1/ 11.1
bc_fitness_matrix_prior_n111                   5.3/  5.3/  5.3       0.1/  0.3/  0.3       5.7/  8.0/  8.0       1.1/  1.1/  1.1       4.4/  3.6/  3.7      11.6/ 10.3/ 11.1     163.2/163.2/ 69.9
bc_fitness_matrix_prior_n2                     0.0/  1.9/  1.9       0.0/  1.1/  1.1       2.0/  4.8/  4.8       2.2/  3.3/  2.2       8.3/  8.3/  8.3      12.9/ 12.9/ 18.8     226.5/217.6/ 63.3
bc_fitness_n1000                               3.5/    -/  3.5       0.1/    -/  0.1       2.3/    -/  2.3       1.1/    -/  1.1       2.5/    -/  2.5       4.2/    -/  2.6         -/    -/  8.9
bc_fitness_n111                                5.7/  5.7/  5.7       0.1/  0.1/  0.1       5.2/  5.2/  5.2       1.1/  2.2/  2.2       5.1/  3.8/  5.1       4.2/  5.6/  5.6       7.8/  7.8/  7.8
bc_fitness_n2                                  0.0/  2.2/  2.2       0.0/  2.2/  2.2       2.2/  8.0/  6.4       2.8/  3.3/  3.3       5.1/  3.8/  5.1       4.4/  5.9/  7.2      12.8/ 10.0/ 10.0
bc_fitness_tiny_n1000                          1.9/  1.9/  1.9       0.1/  0.1/  0.1       3.5/  4.6/  4.6       1.1/  0.0/  0.0       0.8/  0.8/  1.1       2.1/  2.1/  2.1         -/ 11.1/  3.3
bc_fitness_tiny_n2049                          1.9/  1.9/  1.9       0.0/  0.0/  0.0       2.3/  3.1/  3.1       0.0/  0.0/  0.0       0.6/  0.6/  0.6       2.7/  2.1/  2.1         -/ 11.1/  3.3
bc_fitness_tiny_n5781                          3.8/  3.8/  3.8       0.1/  0.1/  0.1       3.1/  3.1/  3.1       1.1/  1.1/  1.1       1.1/  1.1/  0.6       4.1/  4.2/  4.2         -/ 11.7/  3.0
bc_genotype_matrix_prior_n1000                 1.9/    -/  1.9       0.1/    -/  0.1       3.6/    -/  3.6       0.6/    -/  0.6       1.3/    -/  1.3       1.9/    -/  1.7         -/    -/ 31.1
bc_genotype_matrix_prior_n111                  6.2/  6.2/  6.2       0.1/  0.2/  0.2       7.0/  7.0/  7.0       1.1/  1.1/  2.2       5.0/  3.3/  4.4       9.6/  9.6/ 11.2       4.4/  4.4/  4.4
bc_genotype_matrix_prior_n2                    0.0/  2.0/  2.0       0.0/  2.2/  2.2       2.0/  3.7/  2.6       1.7/  1.7/  2.2       7.5/  7.5/  3.3      20.7/ 15.2/ 16.0      34.4/ 33.3/ 33.3
bc_genotype_regrouped_n1000                    1.9/    -/  1.9       0.1/    -/  0.1       2.1/    -/  2.1       0.6/    -/  0.6       1.3/    -/  2.5       5.9/    -/  5.9         -/    -/  0.0
bc_genotype_regrouped_n111                     6.2/  6.2/  6.2       0.1/  0.2/  0.2       5.5/  5.5/  5.5       1.1/  1.7/  1.7       7.2/  7.2/  7.2       6.6/  5.2/  5.7       5.6/  5.6/  6.7
bc_genotype_regrouped_n2                       0.0/  2.0/  2.0       0.0/  2.2/  2.2       2.1/  4.4/  3.3       3.3/  3.3/  3.9       4.8/  7.2/  7.7       6.7/  7.8/  7.8       8.3/  8.3/  3.9
bc_multienv_env0_only_first_n1000              4.0/    -/  4.0       0.1/    -/  0.0       2.8/    -/  2.8       0.0/    -/  0.0       9.4/    -/  9.4       1.3/    -/  0.0         -/    -/ 13.3
bc_multienv_env0_only_first_n111               6.5/  6.5/  6.5       0.1/  0.1/  0.1       6.1/  5.7/  5.7       3.3/  2.2/  3.3       8.1/  8.1/  8.1       6.7/  8.1/  8.1      13.0/ 13.0/  4.3
bc_multienv_env0_only_first_n2                 0.0/  1.9/  1.9       0.0/  1.1/  1.1       2.2/  7.1/  7.1       3.3/  3.3/  3.3       5.1/  5.1/  6.3       4.4/  6.1/  6.1      10.0/ 10.0/  7.8
bc_multienv_n1000                              4.0/    -/  5.8       0.1/    -/  0.0       2.2/    -/  2.2       1.1/    -/  1.1       3.3/    -/  3.3       3.3/    -/  5.9         -/    -/  0.0
bc_multienv_n111                               7.1/  7.1/  7.1       0.1/  0.2/  0.2       6.7/  7.0/  7.0       3.3/  3.3/  3.3       5.3/  5.3/  5.3       5.9/  5.6/  5.6       8.8/  8.8/  8.8
bc_multienv_n2                                 0.0/  2.0/  2.0       0.0/  1.1/  1.1       2.2/ 10.0/ 10.0       5.6/  5.6/  5.6       7.8/  7.8/  7.8       6.1/  6.1/  8.0       5.0/  4.4/  8.9
bc_multienv_replicate_n1000                    3.4/    -/  3.4       0.1/    -/  0.1       3.3/    -/  3.3       3.3/    -/  3.3       1.1/    -/  1.1       3.1/    -/  3.1         -/    -/  8.9
bc_multienv_replicate_n111                     7.1/  7.1/  7.1       0.1/  0.2/  0.2       7.7/  7.7/ 10.2       3.3/  3.3/  3.3       6.4/  6.7/  6.7       6.5/  7.1/  7.1       1.7/  1.7/  1.7
bc_multienv_replicate_n2                       0.0/  2.2/  2.2       0.0/  1.1/  1.1       2.2/ 12.5/ 12.5       5.6/  7.8/  7.8       9.3/  9.3/  9.3       9.8/  8.7/  9.8       8.8/  8.8/  8.8
bc_replicate_ragged_method_n1000               1.7/    -/  1.7       0.0/    -/  0.1       4.4/    -/  4.4       0.6/    -/  1.1       3.9/    -/  3.9       4.4/    -/  4.4         -/    -/  0.0
bc_replicate_ragged_method_n111                6.6/  6.6/  6.6       0.1/  0.1/  0.1       6.1/  7.2/  7.2       1.1/  2.2/  2.2       6.1/  5.0/  5.6       6.3/  6.3/  6.3       9.2/ 27.8/ 27.8
bc_replicate_ragged_method_n2                  0.0/  0.0/  0.0       0.0/  1.1/  1.1       2.1/ 15.9/ 15.9       3.3/  4.4/  4.4       9.5/  9.5/  8.2       7.4/ 12.9/ 12.9      22.2/ 22.2/ 14.4
bc_replicate_ragged_n1000                      1.7/    -/  1.7       0.0/    -/  0.1       4.4/    -/  4.4       0.6/    -/  1.1       3.9/    -/  3.9       4.4/    -/  4.4         -/    -/  0.0
bc_replicate_ragged_n111                       6.6/  6.6/  6.6       0.1/  0.1/  0.1       6.1/  7.2/  7.2       1.1/  2.2/  2.2       6.1/  5.0/  5.6       6.3/  6.3/  6.3       9.2/ 27.8/ 27.8
bc_replicate_ragged_n2                         0.0/  0.0/  0.0       0.0/  1.1/  1.1       2.1/ 15.9/ 15.9       3.3/  4.4/  4.4       9.5/  9.5/  8.2       7.4/ 12.9/ 12.9      22.2/ 22.2/ 14.4
pop_fitness_matrix_prior_n1000                 5.5/  5.5/  5.5       0.0/  0.1/  0.1       2.6/  2.6/  2.6       0.0/  0.6/  0.6       0.8/  0.8/  0.8      17.3/ 17.3/ 19.8         -/ 95.0/165.3
pop_fitness_matrix_prior_n111                  1.8/  1.8/  1.8       0.1/  0.1/  0.1       2.6/  1.3/  1.3       0.6/  1.1/  1.1       0.6/  0.6/  0.3      29.6/ 28.4/ 18.5     162.1/162.1/236.0
pop_fitness_matrix_prior_n2                    0.0/  0.0/  0.0       0.0/  0.0/  0.0       1.4/  1.4/  1.4       0.6/  0.6/  1.1       1.7/  1.7/  1.7      19.5/  9.6/  8.7      99.2/ 83.3/269.8
pop_fitness_n1000                              1.9/  1.9/  1.9       0.0/  0.1/  0.1       1.8/  1.8/  1.8       0.3/  0.6/  0.6       1.1/  1.1/  1.1       5.3/  5.3/  5.3         -/  2.6/  4.4
pop_fitness_n111                               3.4/  3.4/  3.4       0.1/  0.1/  0.1       2.1/  3.1/  3.1       0.6/  0.6/  0.6       1.7/  1.7/  1.7       3.3/  3.3/  3.3       1.8/  1.8/  5.6
pop_fitness_n2                                 0.0/  0.0/  0.0       0.0/  0.0/  0.0       1.6/  1.6/  1.6       0.6/  0.6/  0.6       2.2/  3.3/  2.2      12.6/ 12.6/ 12.6      50.0/ 50.0/ 48.8
pop_fitness_n260_n111                          2.2/  2.2/  2.2       0.0/  0.0/  0.0       1.3/  1.3/  1.3       0.1/  0.1/  0.2       0.8/  0.8/  0.8      73.0/ 73.0/ 70.4      50.7/ 50.7/ 50.7
pop_fitness_n260_n2                            0.0/  1.8/  1.8       0.0/  1.1/  1.1       1.3/  0.0/  0.0       0.2/  0.4/  0.4       0.6/  0.6/  0.6     517.5/517.5/517.5     524.6/527.3/527.3
pop_fitness_tiny_n1000                         1.8/  1.8/  1.8       0.0/  0.0/  0.0       4.1/  2.9/  2.9       0.0/  0.0/  1.1       0.6/  0.6/  0.8       1.3/  1.3/  1.3         -/  0.0/  0.0
pop_fitness_tiny_n2049                         0.0/  0.0/  0.0       0.0/  0.1/  0.1       1.4/  1.4/  1.4       1.1/  1.1/  1.1       0.6/  1.1/  0.6       2.6/  1.2/  1.2         -/  0.0/  0.0
pop_fitness_tiny_n5781                         1.8/  1.8/  1.8       0.0/  0.0/  0.0       1.4/  1.4/  1.4       2.2/  2.2/  1.1       1.1/  1.1/  1.1       1.3/  1.3/  1.3         -/  0.0/ 17.8
pop_genotype_matrix_prior_n1000                5.6/  5.6/  5.6       0.1/  0.1/  0.1       4.4/  4.4/  4.4       0.8/  0.8/  0.6       1.7/  1.7/  1.7      61.1/ 61.1/ 71.1         -/  0.0/  0.0
pop_genotype_matrix_prior_n111                 2.0/  2.0/  2.0       0.1/  0.2/  0.2       3.6/  3.6/  3.6       0.3/  0.0/  0.6       1.7/  1.7/  1.7      67.7/ 67.7/ 83.3      60.1/ 65.7/ 10.1
pop_genotype_matrix_prior_n2                   0.0/  0.0/  0.0       0.0/  0.0/  0.0       0.0/  2.2/  2.2       0.6/  1.1/  1.4       1.7/  1.7/  1.7      56.8/ 56.8/ 56.8     401.9/401.9/397.5
pop_genotype_regrouped_n1000                   5.6/  5.6/  5.6       0.1/  0.1/  0.1       2.6/  3.8/  2.6       0.6/  0.6/  0.6       1.7/  1.7/  1.7       3.6/  2.2/  2.2         -/ 35.0/ 35.0
pop_genotype_regrouped_n111                    2.0/  2.0/  2.0       0.1/  0.2/  0.2       3.8/  3.8/  3.8       0.3/  0.3/  0.6       1.1/  0.6/  0.6       2.5/  1.8/  4.4      18.9/ 34.7/ 34.7
pop_genotype_regrouped_n2                      0.0/  0.0/  0.0       0.0/  0.0/  0.0       1.2/  1.2/  1.8       0.6/  0.6/  0.6       0.8/  2.2/  2.2       8.8/  7.8/  7.8      40.0/ 46.7/ 46.7
pop_multienv_env0_only_first_n1000             4.0/  4.0/  4.0       0.1/  0.1/  0.1       1.5/  2.4/  2.4       0.6/  0.6/  0.6       0.8/  0.6/  0.8       3.9/  6.5/  5.2         -/ 15.4/ 15.4
pop_multienv_env0_only_first_n111              4.2/  4.2/  4.2       0.1/  0.1/  0.1       4.4/  4.4/  4.4       0.6/  0.6/  0.6       0.6/  1.1/  0.6       2.3/  2.3/  2.3       1.9/  1.9/  5.7
pop_multienv_env0_only_first_n2                0.0/  0.0/  0.0       0.0/  0.0/  0.0       0.0/  0.0/  0.0       1.1/  1.1/  0.6       0.8/  1.1/  1.7       2.1/  2.1/  2.1       5.8/  5.8/ 10.2
pop_multienv_n1000                             5.3/  5.3/  5.3       0.1/  0.1/  0.1       4.0/  4.0/  4.0       0.6/  0.6/  0.6       1.1/  0.6/  1.1       3.1/  3.1/  3.1         -/ 53.3/ 12.1
pop_multienv_n111                              4.4/  4.4/  4.4       0.1/  0.1/  0.1       2.2/  2.2/  2.2       1.1/  1.1/  1.1       2.8/  2.8/  1.7       3.8/  2.4/  3.8      12.2/ 12.2/ 12.2
pop_multienv_n2                                0.0/  0.0/  0.0       0.0/  0.0/  0.0       2.0/  2.0/  2.0       0.6/  0.6/  1.1       2.2/  2.2/  1.1       3.0/  3.0/  3.0      28.9/ 20.9/ 20.9
pop_multienv_replicate_n1000                   5.5/  5.5/  5.5       0.1/  0.1/  0.1       5.6/  4.2/  4.2       1.1/  1.1/  0.6       1.1/  1.1/  1.7       2.2/  2.2/  3.3         -/ 15.2/ 11.4
pop_multienv_replicate_n111                    3.8/  2.0/  2.0       0.1/  0.1/  0.1       5.3/  5.3/  5.3       1.1/  0.6/  1.1       2.2/  3.3/  1.1       3.4/  3.3/  3.4      14.4/ 14.4/ 14.4
pop_multienv_replicate_n2                      0.0/  1.9/  1.9       0.0/  1.1/  1.1       1.7/  1.8/  1.8       1.7/  1.1/  1.1       4.4/  4.4/  4.4       8.9/  8.9/  8.9      18.9/ 18.9/ 18.9
pop_replicate_ragged_method_n1000              5.6/  5.6/  5.6       0.1/  0.1/  0.1       4.6/  4.6/  4.6       1.1/  1.1/  0.6       1.1/  1.7/  1.7       5.7/  4.4/  5.7         -/  0.0/ 17.8
pop_replicate_ragged_method_n111               3.9/  3.9/  3.9       0.1/  0.1/  0.1       3.8/  3.7/  3.7       0.6/  0.6/  0.6       2.2/  2.2/  2.2       5.1/  5.7/  5.7      10.0/  2.0/  6.0
pop_replicate_ragged_method_n2                 0.0/  0.0/  0.0       0.0/  1.1/  1.1       1.6/  1.6/  1.6       1.7/  1.7/  1.1       3.3/  3.3/  2.2       7.8/  7.8/  7.8      17.8/ 11.1/ 32.8
pop_replicate_ragged_n1000                     5.6/  5.6/  5.6       0.1/  0.1/  0.1       4.3/  4.3/  4.3       1.1/  0.6/  0.6       2.2/  2.2/  2.2       5.5/  5.5/  5.5         -/  0.0/  0.0
pop_replicate_ragged_n111                      3.9/  3.9/  3.9       0.1/  0.1/  0.1       7.0/  5.6/  5.6       1.1/  0.6/  1.1       2.2/  2.2/  3.3       4.4/  5.6/  5.5      25.5/ 25.5/ 32.2
pop_replicate_ragged_n2                        0.0/  0.0/  0.0       0.0/  1.1/  1.1       1.8/  1.8/  1.8       1.7/  1.7/  1.7       2.2/  2.2/  2.2       5.6/  5.6/  5.6      57.7/ 57.7/ 57.7
(largest entry: restatement 524.6e-16, emulation 527.3e-16, MI355X 527.3e-16; the bound is 1e-12 = 10000e-16;
 the largest belong to mode_mean and the quantiles of n = 260 .. 1000 terms: l* = a + (e^t - n) / ib2 cancels n, and the bisection's bracket moves with l*)
"""
import ctypes as C
import functools
import os

import numpy as np

import _ppc_cases as pc
import _rb_cases as rc
import _score_cases as sc
from conftest import make_engine
from barbay_jl_amd import _capi
from oracle import fixtures
from oracle.spec import ModelSpec

UNITS = _capi.LS_UNITS
BLOCKS = ("bc", "pop")
CHUNK = _capi.BB_POPMEAN_RB_CHUNK
MAXN = _capi.BB_LOGSIGMA_RB_MAX_SAMPLES
MEASURED = 5.2e-14        # the float64 restatement's largest error of the six moments against the goldens (make_logsigma_rb_golden.py --measure)
Q_MEASURED = 5.3e-14      # ... and of the quantiles (n_samples = 2 and 111): the bracket moves with the modes
SEED, PROBS, NS = rc.SEED, rc.PROBS, rc.NS
HIER = rc.HIER
ITER, LEFT, RIGHT, RIGHT_MAX, TAIL, REFINE_MAX = 40, 10, 22, 64, -40.0, 64
TRUTH_AT = (-2.3, -0.7, 0.11, 1.9, 4.4)
TRUTH_TOL, TRUTH_CTOL = 4e-12, 3e-5

SHAPES = tuple(pc.CASES) + ("replicate_ragged_method", "multienv_env0_only_first", "genotype_matrix_prior", "fitness_matrix_prior")
# shapes whose entries are too many to work whole in the emulation at every size: a handful of entries has a golden
SOME = {("bc", "fitness_chunk"): (0, 1, 137, 279), ("pop", "fitness_n260"): None}
TINY = "fitness_tiny"


def quirk_of(case):
    return case == "replicate_ragged_method"


def uses_priors(case):
    return case.endswith("matrix_prior")


@functools.lru_cache(maxsize=None)
def spec(case):
    if case in pc.CASES:
        return pc.spec(case)
    if case == "replicate_ragged_method":
        return pc.spec("replicate_ragged")
    if case in ("multienv_env0_only_first", "fitness_chunk"):
        return rc.spec(case)
    if case == TINY:                                              # the large n_samples: five BC entries, three POP entries
        return fixtures.synthetic("fitness", B=8, T=4, n_neutral=3, seed=3)
    if case == "fitness_n260":                                    # n_neutral = 260 crosses the member chunk of the POP block
        return fixtures.synthetic("fitness", B=268, T=3, n_neutral=260, seed=3)
    if case == "fitness_matrix_prior":                            # Matrix form of both logsigma priors
        g = np.random.default_rng(2)
        return fixtures.synthetic("fitness", B=30, T=4, n_neutral=5, seed=3,
                                  logsigma_bc_prior=(g.normal(-1.0, 1.0, 25), g.uniform(0.2, 3.0, 25)),
                                  logsigma_pop_prior=(g.normal(-1.0, 1.0, 3), g.uniform(0.2, 3.0, 3)))
    if case == "genotype_matrix_prior":                           # ... on a handle that regroups its mutants: the prior follows them
        sp, g = pc.spec("genotype_regrouped"), np.random.default_rng(4)
        return ModelSpec(kind=sp.kind, counts=sp.counts, totals=sp.totals, n_neutral=sp.n_neutral, n_bc=sp.n_bc, geno_idx=sp.geno_idx,
                         priors=dict(logsigma_bc_prior=(g.normal(-1.0, 1.0, sp.n_bc), g.uniform(0.2, 3.0, sp.n_bc)),
                                     logsigma_pop_prior=(g.normal(-1.0, 1.0, sp.n_time[0] - 1), g.uniform(0.2, 3.0, sp.n_time[0] - 1))))
    raise KeyError(case)


def n_entries(sp, block):
    lo, hi = sp.offsets()["logsigma_bc" if block == "bc" else "logsigma_pop"]
    return hi - lo


def golden_cases():
    """name -> (block, case, n_samples, entries with a golden or None for all)."""
    out = {}
    for blk in BLOCKS:
        for c in SHAPES:
            ne = n_entries(spec(c), blk)
            few = tuple(sorted({0, 3, ne // 2, ne - 1}))         # (3: a sharp one of `_rb_cases.params` in the BC block)
            for n in NS:
                out[f"{blk}_{c}_n{n}"] = (blk, c, n, None if n * ne <= 16000 else few)
        for n in (1000, 2049, MAXN):                              # more draws than threads and no multiple of 64; the cap
            out[f"{blk}_{TINY}_n{n}"] = (blk, TINY, n, (0, 2))
    for n in (2, 111):
        out[f"bc_fitness_chunk_n{n}"] = ("bc", "fitness_chunk", n, SOME[("bc", "fitness_chunk")])
        out[f"pop_fitness_n260_n{n}"] = ("pop", "fitness_n260", n, None)
    return out


def emu_cases():
    """The golden cases the host emulation works (it works every entry of a call): those of at most 30 000 entry-draws."""
    return sorted(k for k, (blk, c, n, _) in golden_cases().items() if n * n_entries(spec(c), blk) <= 30000)


def golden_path(name):
    return os.path.join(rc.GOLD, f"logsigma_rb_{name}.npz")


@functools.lru_cache(maxsize=None)
def inputs(case):
    sp = spec(case)
    mu, om = rc.params(sp)
    mu.setflags(write=False)
    om.setflags(write=False)
    return sp, mu, om


def engine(lib, case, mu=None, om=None, **kw):
    if quirk_of(case):
        kw["ragged_method"] = True
    if uses_priors(case):
        kw["use_priors"] = True
    if mu is None:
        return make_engine(spec(case), lib, **kw)
    return pc._handle(lib, spec(case), mu, om, **kw)


# ---- the restatement: per-draw inputs ------------------------------------------------------------------------------------------
def _logz(sp, ll, ts, n):
    out = {}
    for t in ts:
        Z = None                                                  # chunks of 256 columns in index order, then the chunks in order
        for b0 in range(0, sp.B, 256):
            part = np.zeros(n)
            for b in range(b0, min(b0 + 256, sp.B)):
                part = part + np.exp(ll(b, t))
            Z = part if Z is None else Z + part
        out[t] = np.log(Z)
    return out


def cond_inputs(sp, D, n, block, entries=None, quirk=False, chunk=CHUNK):
    """{entry: (l [n], SS [n], n_terms, a, ib2)} from the draws D(i) -> [n] of the caller's latents: the header's formulas."""
    off = sp.offsets()
    B, nb, nn, R = sp.B, sp.n_bc, sp.n_neutral, sp.n_rep
    E = rc.n_env(sp)
    hier = sp.kind in HIER
    pm, ps = sp.prior_arrays()
    want = set(range(n_entries(sp, block)) if entries is None else (int(x) for x in entries))
    out = {}
    lo_l, g0 = off["loglambda"][0], 0
    for r in range(R):
        T = sp.n_time[r]
        ll = lambda b, t, lo_l=lo_l, T=T: D(lo_l + b * T + t)
        if block == "pop":
            ks = [k for k in range(T - 1) if g0 + k in want]
            logZ = _logz(sp, ll, (range(T) if quirk else sorted({k + d for k in ks for d in (0, 1)})) if ks else (), n)
            for k in ks:
                g = g0 + k
                sb = D(off["s_pop"][0] + g)
                SS = np.zeros(n)
                for i0 in range(0, nn, chunk):
                    part = np.zeros(n)
                    for i in range(i0, min(i0 + chunk, nn)):
                        t, b = k, i
                        if quirk:
                            x = k * nn + i
                            t, b = x % (T - 1), x // (T - 1)
                        d = ((ll(b, t + 1) - ll(b, t)) - (logZ[t + 1] - logZ[t])) + sb
                        part = part + d * d
                    SS = SS + part
                i = off["logsigma_pop"][0] + g
                out[g] = (D(i), SS, nn, pm[i], 1.0 / (ps[i] * ps[i]))
        else:
            rows = sorted({(x - E * nb * r) // E for x in want if E * nb * r <= x < E * nb * (r + 1)})
            logZ = _logz(sp, ll, range(T) if rows else (), n)
            sbar = [D(off["s_pop"][0] + g0 + t) for t in range(T - 1)]
            for mm in rows:
                b = nn + mm
                for e in range(E):
                    em = e + E * mm
                    u = em + E * nb * r
                    if u not in want:
                        continue
                    if not hier:
                        s, ent = D(off["s_bc"][0] + em), em
                    else:
                        th = int(sp.geno_idx[mm]) if sp.kind == "genotype" else em
                        ent = mm if sp.kind == "genotype" else u
                        s = D(off["theta"][0] + th) + np.exp(D(off["logtau"][0] + ent)) * D(off["theta_tilde"][0] + ent)
                    SS, cnt = np.zeros(n), 0
                    for t in range(T - 1):
                        if rc.env_of(sp, r, t) != e:
                            continue
                        d = (((ll(b, t + 1) - ll(b, t)) - (logZ[t + 1] - logZ[t])) + sbar[t]) - s
                        SS = SS + d * d
                        cnt += 1
                    i = off["logsigma_bc"][0] + ent
                    assert ent == u
                    out[u] = (D(i), SS, cnt, pm[i], 1.0 / (ps[i] * ps[i]))
        lo_l += T * B
        g0 += T - 1
    return out


# ---- the restatement: the rule, float64 ----------------------------------------------------------------------------------------
class Cond:
    """The conditionals of one entry's draws about their modes (arrays over the draws)."""

    def __init__(self, SS, n, a, ib2):
        SS = np.asarray(SS, dtype=np.float64)
        with np.errstate(all="ignore"):
            c2 = 2.0 / ib2
            lnK = np.log(SS) - 2.0 * a + c2 * n
            t = np.where(lnK >= c2, np.log(lnK / c2), lnK)
            active = SS != 0.0
            for _ in range(50):
                if not active.any():
                    break
                et = np.exp(t)
                step = ((t + c2 * et) - lnK) / (1.0 + c2 * et)
                t = np.where(active, t - step, t)
                active = active & ~(np.abs(step) <= 2.0 ** -40 * (1.0 + np.abs(t)))
            lm = np.where(SS == 0.0, a - n / ib2, a + (np.exp(t) - n) / ib2)
            self.a, self.ib2, self.n, self.SS, self.lm = a, ib2, float(n), SS, lm
            self.W = np.where(SS == 0.0, 0.0, SS * np.exp(-2.0 * lm))
            self.c1 = ib2 * (lm - a) + n
            self.dl = 1.0 / np.sqrt(ib2 + 2.0 * self.W)
            # the grid: step delta / (4 m), m = max(1, ceil(2 delta)) (a NaN delta: 1); right extent 22 r delta, r doubling until the
            # density has fallen to exp(TAIL) of the mode's
            m = np.ceil(2.0 * self.dl)
            self.m = np.where(m >= 1.0, np.minimum(m, float(REFINE_MAX)), 1.0)
            self.r = np.ones_like(self.dl)
            while True:
                more = (self.r < RIGHT_MAX) & (np.log(self.p(RIGHT * self.r * self.dl)[0]) > TAIL)
                if not more.any():
                    break
                self.r = np.where(more, 2.0 * self.r, self.r)
            self.s = self.dl / (4.0 * self.m)
            self.nleft, self.nright = LEFT * 4 * self.m, RIGHT * self.r * 4 * self.m
            self.lo, self.hi = lm - 10.0 * self.dl, lm + self.nright * self.s

    def p(self, u, sel=slice(None)):
        W, c1 = self.W[sel], self.c1[sel]
        W, c1 = (W[:, None], c1[:, None]) if np.ndim(u) == 2 else (W, c1)
        x = np.expm1(-2.0 * u)
        tail = np.where(W != 0.0, 0.5 * W * np.where(W != 0.0, x, 0.0), 0.0)
        return np.exp(-(u * c1) - 0.5 * self.ib2 * (u * u) - tail), x

    def dh(self, u, em1, sel=slice(None)):
        W = self.W[sel]
        return -((self.lm[sel] + u) - self.a) * self.ib2 - self.n + np.where(W != 0.0, W * (em1 + 1.0), 0.0)

    def moments(self):
        """(Z, E, V, S) per draw."""
        with np.errstate(all="ignore"):
            s = self.s
            z, m1, m2, se = (np.zeros_like(s) for _ in range(4))
            for nl, nr in sorted(set(zip(self.nleft.tolist(), self.nright.tolist()))):      # the draws of one grid shape together
                sel = np.nonzero((self.nleft == nl) & (self.nright == nr))[0]
                nodes, sg = int(nl + nr), s[sel]
                zz = mm1 = mm2 = sse = np.zeros_like(sg)
                for k in range(nodes + 1):
                    uk = float(k - int(nl)) * sg
                    p, _ = self.p(uk, sel)
                    if k in (0, nodes):
                        p = p * 0.5
                    zz = zz + p
                    mm1 = mm1 + p * uk
                    mm2 = mm2 + p * (uk * uk)
                    sse = sse + p * np.exp(uk)
                z[sel], m1[sel], m2[sel], se[sel] = zz, mm1, mm2, sse
            r1 = m1 / z
            return s * z, self.lm + r1, m2 / z - r1 * r1, np.exp(self.lm) * (se / z)

    def cdf(self, x, Z):
        """C_j(x) per draw."""
        with np.errstate(all="ignore"):
            C = np.where(x >= self.hi, 1.0, 0.0)
            sel = np.nonzero((x > self.lo) & (x < self.hi))[0]
            if sel.size:
                dl, lm = self.dl[sel], self.lm[sel]
                ulo, s = -10.0 * dl, self.s[sel]
                r = x - (lm + ulo)
                N = np.maximum(np.ceil(r / s), 1.0)
                sx = r / N
                p0, e0 = self.p(ulo, sel)
                ux = x - lm
                p1, e1 = self.p(ux, sel)
                i = np.arange(1, int(N.max()))[None, :]
                pin, _ = self.p(ulo[:, None] + i * sx[:, None], sel)
                terms = np.concatenate([(0.5 * p0)[:, None], np.where(i < N[:, None], pin, 0.0)], axis=1)
                acc = np.cumsum(terms, axis=1)[:, -1] + 0.5 * p1              # ascending i: the zeros behind N change nothing
                v = (sx * acc - sx * sx / 12.0 * (self.dh(ux, e1, sel) * p1 - self.dh(ulo, e0, sel) * p0)) / Z[sel]
                C[sel] = np.where(v < 0.0, 0.0, np.where(v > 1.0, 1.0, v))
            return C


def reduce_sum(x):
    """bb_score_reduce's order: lane partials of the strided draws, 16 waves per lane column, then the 64 columns."""
    NT = 1024
    x = np.asarray(x, dtype=np.float64)
    lanes = np.zeros(NT)
    for j0 in range(0, x.shape[0], NT):
        seg = x[j0:j0 + NT]
        lanes[:seg.shape[0]] = lanes[:seg.shape[0]] + seg
    cols = lanes[:64].copy()
    for w in range(1, NT // 64):
        cols = cols + lanes[64 * w:64 * (w + 1)]
    s = cols[0]
    for g in range(1, 64):
        s = s + cols[g]
    return float(s)


def entry64(l, SS, n, a, ib2, probs, want_q=True):
    """The outputs of one entry from its float64 per-draw inputs: the header's rule as it stands."""
    ns = l.shape[0]
    c = Cond(SS, n, a, ib2)
    Z, E, V, S = c.moments()
    with np.errstate(all="ignore"):
        qm, rm = reduce_sum(l) / ns, reduce_sum(E) / ns
        vals = [qm, np.sqrt(reduce_sum((l - qm) ** 2) / ns), rm, np.sqrt(reduce_sum(V) / ns + reduce_sum((E - rm) ** 2) / ns),
                reduce_sum(S) / ns, reduce_sum(c.lm) / ns]
    qs = []
    ok = bool(np.all(np.isfinite(c.lm)) and np.all(np.isfinite(c.dl)) and np.all(np.isfinite(Z)))
    for p in (probs if want_q else ()):
        if not ok:
            qs.append(np.nan)
            continue
        lo, hi = float(c.lo.min()), float(c.hi.max())
        for _ in range(ITER):
            x = lo + (hi - lo) / 2.0
            if reduce_sum(c.cdf(x, Z)) / ns < p:
                lo = x
            else:
                hi = x
        qs.append(lo + (hi - lo) / 2.0)
    return vals, qs


def draws_of(sp, mu, omega, n, seed, draws=None):
    return rc.Rows(draws) if draws is not None else sc.Draws(seed, mu, pc.softplus(omega), n)


def restate(sp, block, mu, omega, n, seed, probs=PROBS, draws=None, entries=None, entry=entry64, quirk=False, chunk=CHUNK, want_q=True):
    """bb_logsigma_rb at (mu, omega) -- or at the explicit `draws` [n, D] -- for `entries` (all): a dict as Engine.logsigma_rb returns,
    the entries' rows only.  `entry`: the evaluation of one entry (the golden generator passes its 50-digit one)."""
    with np.errstate(all="ignore"):
        D = draws_of(sp, mu, omega, n, seed, draws)
        entries = np.arange(n_entries(sp, block)) if entries is None else np.asarray(entries)
        ci = cond_inputs(sp, D, n, block, entries=entries, quirk=quirk, chunk=chunk)
        out = {k: np.empty(len(entries)) for k in UNITS}
        out["quantiles"] = np.full((len(entries), len(probs)), np.nan)
        out["n_terms"] = np.array([ci[int(u)][2] for u in entries], dtype=np.int32)
        for x, u in enumerate(entries):
            l, SS, nt, a, ib2 = ci[int(u)]
            vals, qs = entry(l, SS, nt, a, ib2, probs, want_q)
            for k, v in zip(UNITS, vals):
                out[k][x] = float(v)
            if want_q and len(probs):
                out["quantiles"][x] = [float(q) for q in qs]
    return out


@functools.lru_cache(maxsize=None)
def golden(name):
    with np.load(golden_path(name)) as f:
        g = {k: f[k] for k in f.files}
    for v in g.values():
        v.setflags(write=False)
    return g


# ---- comparison -----------------------------------------------------------------------------------------------------------------
def errors(got, ref, keys=UNITS + ("quantiles",)):
    """Largest error per output relative to max(|x|, 1); the NaN pattern and n_terms must be equal."""
    err = {}
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        assert a.shape == b.shape, (k, a.shape, b.shape)
        assert np.array_equal(np.isnan(a), np.isnan(b)), k
        ok = ~np.isnan(b)
        err[k] = float(np.max(np.abs(a[ok] - b[ok]) / np.maximum(np.abs(b[ok]), 1.0))) if ok.any() else 0.0
    assert np.array_equal(got["n_terms"], ref["n_terms"])
    return err


def tolerances():
    return max(1e-12, 8.0 * MEASURED), max(1e-12, 8.0 * Q_MEASURED)


def assert_within(err, who):
    tol, qtol = tolerances()
    for k, v in err.items():
        assert v <= (qtol if k == "quantiles" else tol), (who, k, v)


def report(name, label, err):
    print(f"logsigma_rb case {name:40s} {label:12s} " + " ".join(f"{k} {err[k] / 1e-16:7.1f}" for k in err) + "  (1e-16)")


def take(res, entries):
    return res if entries is None else {k: v[list(entries)] for k, v in res.items()}


def lrb(e, block, n, **kw):
    kw.setdefault("probs", PROBS)
    kw.setdefault("seed", SEED)
    return e.logsigma_rb(block=block, n_samples=n, **kw)


# ---- 1. golden values ----------------------------------------------------------------------------------------------------------
def check_golden(lib, name, label):
    blk, case, n, entries = golden_cases()[name]
    sp, mu, om = inputs(case)
    ref = golden(name)
    ne = n_entries(sp, blk)
    ents = list(range(ne)) if entries is None else list(entries)
    # The quantiles' reference where there is no 50-digit one: the restatement, two entries.  Never a prior-only entry: with a = 0 its
    # median lies exactly on a midpoint of the bisection, a tie F(x) = p that rounding decides, and the two branches end a final
    # bracket (3e-11 b) apart.  `check_prior_only` holds those entries' quantiles to the bound that fits them.
    qrest = [u for u, nt in zip(ents, ref["n_terms"]) if nt > 0][:2]
    r64 = restate(sp, blk, mu, om, n, SEED, entries=ents, quirk=quirk_of(case), want_q=False)
    mom = {k: ref[k] for k in UNITS + ("n_terms",)}
    e0 = errors(r64, mom, UNITS)
    with engine(lib, case, mu, om) as e:
        got = lrb(e, blk, n)
    assert got["quantiles"].shape == (ne, len(PROBS)) and np.all(np.diff(got["quantiles"], axis=1) > 0)
    err = errors(take(got, ents), mom, UNITS)
    if "quantiles" in ref:                                        # 50-digit bisection (n = 2)
        qe = [int(x) for x in ref["q_entries"]]
        rq = restate(sp, blk, mu, om, n, SEED, entries=qe, quirk=quirk_of(case))
        e0["quantiles"] = errors({"quantiles": rq["quantiles"], "n_terms": 0}, {"quantiles": ref["quantiles"], "n_terms": 0}, ("quantiles",))["quantiles"]
        err["quantiles"] = errors({"quantiles": got["quantiles"][qe], "n_terms": 0}, {"quantiles": ref["quantiles"], "n_terms": 0}, ("quantiles",))["quantiles"]
    else:
        rq = restate(sp, blk, mu, om, n, SEED, entries=qrest, quirk=quirk_of(case))
        err["quantiles"] = errors({"quantiles": got["quantiles"][qrest], "n_terms": 0}, {"quantiles": rq["quantiles"], "n_terms": 0}, ("quantiles",))["quantiles"]
    report(name, "restatement", e0)
    report(name, label, err)
    assert_within(e0, "restatement")
    assert_within(err, label)


# ---- 2. the rule against the truth -------------------------------------------------------------------------------------------------
def truth_path():
    return os.path.join(rc.GOLD, "logsigma_rb_truth.npz")


def check_truth():
    """The float64 restatement's ln Z, E, V and C against `mpmath.quad` of the density itself (stored by the golden maker), on the
    cases' own per-draw (n, SS, a, b) -- three entries of every block and shape, 54 sets -- and on 14 further sets spanning n from 0
    to 1000, SS from 1e-300 to 1e6 and b from 0.2 to 3.  Bounds: 4e-12 for the moments (ln Z absolute, E in units of delta, V
    relative), 3e-5 absolute for C.  Measured:
      the cases' own sets     ln Z 9.7e-16   E 2.0e-15 delta   V 1.7e-15   C 3.8e-06
      the 14 further sets     ln Z 8.9e-16   E 4.0e-14 delta   V 1.3e-15   C 3.7e-06
    With a fixed step of delta / 4 and a right end at l* + 22 delta the same sets gave up to 3.1e-12 / 6.6e-12 / 7.9e-12 (own) and
    1.7e-08 / 5.8e-08 / 8.5e-08 (further: n = 1, SS = 1e-6, b = 3, delta = 1.19): prior-dominated entries, whose left cutoff a
    step above 1/8 does not resolve and whose right tail reaches beyond 22 delta.  That is what the header's m_j and r_j are for."""
    t = golden("truth")
    n_extra = 14                                                  # the first sets of the file: `make_logsigma_rb_golden.FURTHER_SETS`
    worst = [{"lnZ": 0.0, "E": 0.0, "V": 0.0, "C": 0.0} for _ in range(2)]
    for i in range(t["n"].shape[0]):
        c = Cond(np.array([t["SS"][i]]), float(t["n"][i]), float(t["a"][i]), float(t["ib2"][i]))
        Z, E, V, _ = c.moments()
        w = worst[0 if i >= n_extra else 1]
        assert abs(c.lm[0] - t["mode"][i]) <= 1e-12 * max(1.0, abs(t["mode"][i]))
        w["lnZ"] = max(w["lnZ"], abs(np.log(Z[0]) - t["lnZ"][i]))
        w["E"] = max(w["E"], abs(E[0] - t["E"][i]) / c.dl[0])
        w["V"] = max(w["V"], abs(V[0] / t["V"][i] - 1.0))
        for k, m in enumerate(TRUTH_AT):
            w["C"] = max(w["C"], abs(c.cdf(c.lm[0] + m * c.dl[0], Z)[0] - t["C"][i, k]))
    for label, w in zip(("the cases' own sets", "the further sets"), worst):
        print(f"logsigma_rb rule against mpmath.quad, {label}:", " ".join(f"{k} {v:.2e}" for k, v in w.items()))
    for label, w in zip(("the cases' own sets", "the further sets"), worst):
        assert w["lnZ"] <= TRUTH_TOL and w["E"] <= TRUTH_TOL and w["V"] <= TRUTH_TOL and w["C"] <= TRUTH_CTOL, (label, w)


# ---- 3. the identity against the log-joint -----------------------------------------------------------------------------------------
IDENTITY = SHAPES + ("fitness_chunk", "fitness_n260")


def check_identity(lib, name, device=False):
    """A point z passed as one explicit draw to both blocks; z' = z with every logsigma entry at its mode_mean: the gradient of the
    log-joint at z' is zero there to within 2^-30 (ib2 + 2n)(1 + |l*|)."""
    from oracle import literal
    quirk = quirk_of(name)
    sp = spec(name)
    off = sp.offsets()
    pm, ps = sp.prior_arrays()
    g = np.random.default_rng(8)
    with engine(lib, name, seed=1) as e:
        for scale in (0.3, 1.0):
            z = g.normal(0.0, scale, sp.D)
            z2, res = z.copy(), {}
            for blk, key in (("bc", "logsigma_bc"), ("pop", "logsigma_pop")):
                sl = slice(*off[key])
                assert e.logsigma_rb_shape(blk) == sl.stop - sl.start == n_entries(sp, blk)
                got = e.logsigma_rb(block=blk, probs=(), draws=z)
                ref = restate(sp, blk, None, None, 1, 0, probs=(), draws=z[None, :], quirk=quirk)
                assert np.array_equal(got["n_terms"], ref["n_terms"])
                assert np.all(got["q_sd"] == 0.0) and np.array_equal(got["q_mean"], z[sl])
                z2[sl] = got["mode_mean"]
                res[blk] = (sl, got)
            grad = literal.logjoint_and_grad(z2, sp, **(dict(ragged_quirk=True) if quirk else {}))[1]
            gd = e.logdensity_grad(z2)[1] if device else None
            for blk, (sl, got) in res.items():
                bound = 2.0 ** -30 * (1.0 / ps[sl] ** 2 + 2.0 * got["n_terms"]) * (1.0 + np.abs(got["mode_mean"]))
                worst = np.max(np.abs(grad[sl]) / bound)
                print(f"logsigma_rb identity {name:26s} {blk:3s} sd {scale}: |dlogp/dl| at the modes at most {worst:.2e} of the bound")
                assert np.all(np.abs(grad[sl]) <= bound), (blk, worst)
                if device:
                    assert np.all(np.abs(gd[sl]) <= bound), blk


# ---- 4. prior-only entries -----------------------------------------------------------------------------------------------------
def check_prior_only(lib, n=111):
    """multienv_env0_only_first: the units of environment 0 have n = 0; their conditional is the prior N(a, b)."""
    from scipy.special import ndtri
    case = "multienv_env0_only_first"
    sp, mu, om = inputs(case)
    E = rc.n_env(sp)
    u0 = np.arange(0, n_entries(sp, "bc"), E)
    pm, ps = sp.prior_arrays()
    sl = slice(*sp.offsets()["logsigma_bc"])
    a, b = pm[sl][u0], ps[sl][u0]
    with engine(lib, case, mu, om) as e:
        got = lrb(e, "bc", n, probs=(0.001, 0.025, 0.5, 0.975, 0.999))
    assert np.all(got["n_terms"][u0] == 0) and np.all(got["n_terms"][u0 + 1] == 2)
    assert np.all(np.abs(got["rb_mean"][u0] - a) <= 1e-13 * np.maximum(np.abs(a), 1.0))
    assert np.all(np.abs(got["mode_mean"][u0] - a) <= 1e-13 * np.maximum(np.abs(a), 1.0))
    assert np.all(np.abs(got["rb_sd"][u0] / b - 1.0) <= 1e-12)
    for i, p in enumerate((0.001, 0.025, 0.5, 0.975, 0.999)):
        zq = ndtri(p)
        phi = np.exp(-0.5 * zq * zq) / np.sqrt(2.0 * np.pi)
        d = np.abs(got["quantiles"][u0, i] - (a + b * zq))
        print(f"logsigma_rb prior-only quantile p = {p}: error at most {d.max():.2e}, bound {np.min(3e-5 * b / phi):.2e}")
        assert np.all(d <= 3e-5 * b / phi), p


# ---- 5. family checks ------------------------------------------------------------------------------------------------------------
def same_bytes(a, b):
    return rc.same_bytes(a, b)


def both(e, n, **kw):
    out = {}
    for blk in BLOCKS:
        out.update({f"{blk}_{k}": v for k, v in lrb(e, blk, n, **kw).items()})
    return out


def check_launch_modes(lib, case="genotype_regrouped"):
    import barbay_jl_amd as bb
    sp, mu, om = inputs(case)
    out = []
    for mode in (1, 0):
        with bb.Engine(sp.kind, sp.counts, sp.n_neutral, sp.n_bc, env_idx=sp.env_idx, geno_idx=sp.geno_idx, seed=4, launch_mode=mode, _lib=lib) as e:
            e.set_params(mu, om)
            out.append(both(e, 64, seed=2))
            out.append(both(e, 64, seed=2))
    assert all(same_bytes(out[0], o) for o in out[1:])


GROUP_CASES = pc.GROUP_CASES


def check_group_handle(lib, case):
    sp, mu, om = inputs(case)
    with pc._handle(lib, sp, mu, om, device_ids=[0, 0]) as e:
        a = both(e, 33)
    with pc._handle(lib, sp, mu, om) as e:
        b = both(e, 33)
    assert same_bytes(a, b)


def check_buffer_reuse(lib):
    """The call interleaved with the other post-fit calls at changing sizes and across its two blocks on one handle: every result is
    byte for byte what a fresh handle gives."""
    sp, mu, om = inputs(TINY)
    qs = (0.95, 0.675, 0.05)
    dr = rc.materialise(sp, mu, om, 7, 3)
    calls = [lambda e: lrb(e, "bc", 111),
             lambda e: e.ppc_bands(qs, n_samples=111, n_ppc=7, seed=SEED),
             lambda e: lrb(e, "pop", 1000),
             lambda e: rc.rb(e, 200),
             lambda e: lrb(e, "bc", 2),
             lambda e: e.popmean_rb(n_samples=111, seed=SEED),
             lambda e: lrb(e, "pop", 7, draws=dr),
             lambda e: rc.rb(e, 2049, probs=(0.5,)),
             lambda e: lrb(e, "bc", 2049, probs=(0.5,)),
             lambda e: lrb(e, "pop", 2),
             lambda e: lrb(e, "bc", 111)]
    with pc._handle(lib, sp, mu, om) as e:
        got = [pc._bits(f(e)) for f in calls]
    for i, f in enumerate(calls):
        with pc._handle(lib, sp, mu, om) as e:
            assert got[i] == pc._bits(f(e)), i
    assert got[0] == got[-1]


def check_handle_untouched(lib):
    sp = spec("genotype_regrouped")
    with make_engine(sp, lib, seed=5) as a, make_engine(sp, lib, seed=5) as b:
        both(b, 16)
        for x, y in zip(a.get_params(), b.get_params()):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
        a.run(5)
        both(b, 8, seed=1)
        b.run(5)
        for x, y in zip(a.get_params(), b.get_params()):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64))


def check_internal_against_explicit_draws(lib, case, n=33):
    sp, mu, om = inputs(case)
    dr = rc.materialise(sp, mu, om, n, SEED)
    with engine(lib, case, mu, om) as e:
        for blk in BLOCKS:
            a, b = lrb(e, blk, n), lrb(e, blk, n, draws=dr)
            assert same_bytes(b, lrb(e, blk, 5, draws=dr))          # n_samples is the row count; the argument is ignored
            err = errors(a, b)
            report(f"{blk}_{case}_n{n}", "own/explicit", err)
            assert_within(err, "explicit draws")


def check_nan_stays(lib, case="multienv_replicate", n=33):
    """A NaN mean of one mutant's theta_tilde: exactly that unit's BC entry has NaN conditionals (its own draws have not); a NaN mean
    of one logsigma_pop entry: its q_mean / q_sd alone.  No other entry of either block changes a bit."""
    sp, mu, om = inputs(case)
    E, m, r, env = rc.n_env(sp), 5, 1, 0
    u = env + E * m + E * sp.n_bc * r
    off = sp.offsets()
    mu2 = mu.copy()
    mu2[off["theta_tilde"][0] + u] = np.nan
    g = 2
    mu2[off["logsigma_pop"][0] + g] = np.nan
    with pc._handle(lib, sp, mu, om) as e:
        base = {blk: lrb(e, blk, n) for blk in BLOCKS}
    with pc._handle(lib, sp, mu2, om) as e:
        got = {blk: lrb(e, blk, n) for blk in BLOCKS}
    rest = np.setdiff1d(np.arange(n_entries(sp, "bc")), [u])
    assert same_bytes({k: v[rest] for k, v in got["bc"].items()}, {k: v[rest] for k, v in base["bc"].items()})
    for k in ("rb_mean", "rb_sd", "sigma_mean", "mode_mean", "quantiles"):
        assert np.all(np.isnan(got["bc"][k][u])), k
    keep = ("q_mean", "q_sd", "n_terms")
    assert same_bytes({k: got["bc"][k][[u]] for k in keep}, {k: base["bc"][k][[u]] for k in keep})
    rest = np.setdiff1d(np.arange(n_entries(sp, "pop")), [g])
    assert same_bytes({k: v[rest] for k, v in got["pop"].items()}, {k: v[rest] for k, v in base["pop"].items()})
    assert np.isnan(got["pop"]["q_mean"][g]) and np.isnan(got["pop"]["q_sd"][g])
    keep = ("rb_mean", "rb_sd", "sigma_mean", "mode_mean", "quantiles", "n_terms")
    assert same_bytes({k: got["pop"][k][[g]] for k in keep}, {k: base["pop"][k][[g]] for k in keep})


def check_more_quantiles(lib, label, case=TINY, n=111):
    """Four and eight quantiles, 0.001 and 0.999 among them, against the restatement."""
    sp, mu, om = inputs(case)
    for probs in ((0.001, 0.25, 0.75, 0.999), (0.001, 0.025, 0.16, 0.5, 0.84, 0.975, 0.99, 0.999)):
        for blk in BLOCKS:
            ref = restate(sp, blk, mu, om, n, SEED, probs=probs)
            with engine(lib, case, mu, om) as e:
                got = lrb(e, blk, n, probs=probs)
            err = errors(got, ref)
            report(f"{blk}_{case}_n{n}_q{len(probs)}", label, err)
            assert_within(err, label)


# ---- 6. errors ------------------------------------------------------------------------------------------------------------------
OUTS = UNITS + ("quantiles", "n_terms")


def raw(engine_, n_samples, block=0, probs=PROBS, seed=SEED, draws=None, null=(), want=OUTS, n_quantiles=None):
    """bb_logsigma_rb through ctypes with only the outputs in `want` non-NULL; `null` names arguments passed as NULL."""
    ne = engine_.logsigma_rb_shape("bc" if block != 1 else "pop")
    p = np.ascontiguousarray(probs, dtype=np.float64)
    o = _capi.bb_logsigma_rb_opts()
    o.block, o.n_samples, o.n_quantiles, o.seed = block, n_samples, len(p) if n_quantiles is None else n_quantiles, seed
    o.probs = None if "probs" in null or not len(p) else _capi._ptr(p)
    if draws is not None:
        o.draws = _capi._ptr(draws)
    res, out = {}, _capi.bb_logsigma_rb_out()
    for k in want:
        if k == "n_terms":
            res[k] = np.full(ne, -7, dtype=np.int32)
            setattr(out, k, res[k].ctypes.data_as(C.POINTER(C.c_int32)))
        else:
            res[k] = np.full((ne, len(p)) if k == "quantiles" else ne, -7.0)
            setattr(out, k, _capi._ptr(res[k]))
    rcode = engine_._lib.bb_logsigma_rb(None if "h" in null else engine_._h, None if "o" in null else C.byref(o),
                                        None if "out" in null else C.byref(out))
    return rcode, res


def check_errors(lib):
    """Every BB_ERR_INVALID and BB_ERR_UNSUPPORTED of the contract, with a message.  NOT exercised: BB_ERR_DEVICE for what the device
    cannot allocate (a test on a shared machine does not take the device's whole memory)."""
    sp, mu, om = inputs(TINY)
    INVALID, UNSUPPORTED = -1, _capi.BB_ERR_UNSUPPORTED
    msg = lambda: lib.bb_last_error().decode()
    dr = rc.materialise(sp, mu, om, 3, 1)
    with pc._handle(lib, sp, mu, om) as e:
        for null in ("h", "o", "out"):
            assert raw(e, 10, null=(null,))[0] == INVALID and msg(), null
        for blk in (-1, 2, 7):
            assert raw(e, 10, block=blk)[0] == INVALID and "block" in msg(), blk
            assert lib.bb_logsigma_rb_shape(e._h, blk, C.byref(C.c_int64(0))) == INVALID and "block" in msg()
        for nq in (-1, 9):
            assert raw(e, 10, n_quantiles=nq)[0] == INVALID and "n_quantiles" in msg(), nq
        assert raw(e, 10, null=("probs",), n_quantiles=3)[0] == INVALID and "probs" in msg()
        for bad in (0.0, 1.0, -0.1, 1.5, np.nan):
            assert raw(e, 10, probs=(0.5, bad))[0] == INVALID and "prob" in msg(), bad
        for n in (1, 0, -3, MAXN + 1):
            assert raw(e, n)[0] == UNSUPPORTED and "n_samples" in msg(), n
        for n in (0, MAXN + 1):
            assert raw(e, n, draws=dr)[0] == UNSUPPORTED and "n_samples" in msg(), n
        for blk, name in enumerate(BLOCKS):
            assert raw(e, 1, block=blk, draws=dr)[0] == 0 and raw(e, 3, block=blk, draws=dr)[0] == 0      # one explicit draw is served
            assert raw(e, 16, block=blk, want=())[0] == 0                                # an all-NULL out
            assert raw(e, 16, block=blk, probs=())[0] == 0                               # no quantiles
            full = lrb(e, name, 16)
            assert same_bytes(raw(e, 16, block=blk)[1], full)
            for k in OUTS:                                                               # every output NULL except one
                rcode, one = raw(e, 16, block=blk, want=(k,))
                assert rcode == 0 and same_bytes(one, {k: full[k]}), k
        for call, word in ((lambda: e.logsigma_rb(n_samples=1), "n_samples"), (lambda: e.logsigma_rb(block="tau"), "block"),
                           (lambda: e.logsigma_rb(draws=np.zeros((3, sp.D + 1))), "draws")):
            try:
                call()
            except _capi.BarBayHipError as ex:
                assert word in str(ex)
            else:
                raise AssertionError("no error")
