// bb_score.h -- predictive log score and probability integral transform (PIT) of every observed log-frequency ratio on the device.
// Entry point bb_ppc_score (include/barbay_hip.h); no reference counterpart: the reference stops at the bands.
//
// Rows: row = r B + b, b the data column (neutrals first, then the mutants in the caller's order), as bb_freq.h; steps t < T_r - 1.
// A sample j < n_samples is the joint posterior draw of bb_ppc.h (same keying, BB_STREAM_PPC_PARAM), and the predictive of a step
// given draw j is N(mu_j, sigma_j): a neutral row has mu_j = -sbar_{r,t,j}, sigma_j = exp(logsigmabar_{r,t,j}) (bb_block_ppc_pop's
// table), a mutant row the (s - sbar, sigma) of bb_block_ppc's row (bb_ppc_row_par).  There is no predictive draw and no selection:
// with y the observed ratio (formed on the host, NaN where a count is 0), z_j = (y - mu_j) / sigma_j and
// l_j = -z_j^2 / 2 - ln sigma_j - ln(2 pi) / 2, the density and both tails of the CDF are averaged over j in closed form.
//
// One block program, bb_block_score: one workgroup of BB_SCORE_NT threads per row, row += nblocks; per scored step three sweeps over
// the samples, each followed by one reduction of three quantities:
//   A  mu_j, sigma_j, l_j (kept in LDS)                      -> sum mu, sum sigma^2, sum l
//   B  the tails erfc(-z_j / sqrt 2) / 2, erfc(z_j / sqrt 2) / 2  -> their sums, m = max l (a NaN l makes m NaN)
//   C  centred second moments and the log-sum-exp            -> sum (mu - mean)^2, sum (l - lbar)^2, sum exp(l - m)
// Sums: lane i adds its samples i, i + NT, ... in ascending order; the NT partials are added across the waves (partial g + 64 w,
// w ascending, into g < 64: consecutive doubles per lane, no LDS bank conflict) and the 64 sums in order by one lane.  The order
// is a function of n_samples alone -- not of the grid, the launch mode or the handle's latent order -- and there are no atomics.
// erfc, exp and log are the platform's (ocml on the device, libm in the emulation): both tails through erfc, never as 1 - the
// other, so each keeps its relative accuracy where it is tiny; non-finite parameters propagate by IEEE rules (bb_exp clamps).
// Barrier-separated passes, so the host emulation (BB_EMU) runs the same source.
#pragma once
#include "bb_ppc.h"

#define BB_SCORE_NT 1024                   // threads of the block program (the reduction order is defined on it)
#define BB_SCORE_CELLS 6                   // per-cell results on the device: pred_mean, pred_sd, lpd, p_waic, pit, pit_upper

struct ScoreArgs {
    PpcArgs P;                // as for bb_block_ppc, with n_rows = R B, n_steps = max_r T_r - 1, nb = the mutants, n_ppc = 1; no targets
    const double* y;          // [n_rows][n_steps] observed ratios, NaN: unscored
    double* cell;             // [BB_SCORE_CELLS][n_rows n_steps]
    double* rowsum;           // [2][n_rows]: row_lpd, row_p_waic
    int* n_scored;            // [n_rows]
    long long B, nn;          // data columns, of which neutral
};

// LDS: l[n_samples] | three arrays of BB_SCORE_NT partials | scalars [16]: 0 .. 8 the nine reductions, 12 .. 14 the row's sums (lane 0's)
BB_HD long long bb_score_lds_doubles(int ns) { return (long long)ns + 3 * BB_SCORE_NT + 16; }
static_assert(BB_SCORE_NT % 64 == 0, "the partials are added across whole waves");

// the larger of a and b; a NaN stays
BB_DEV double bb_score_max(double a, double b) { return (b > a || b != b) ? b : a; }

// The three arrays of partials red[3][BB_SCORE_NT] into out[0 .. 3): sums, the third the maximum where max2.  Ends with a barrier.
BB_DEV void bb_score_reduce(BBCtx& cx, double* red, double* out, bool max2) {
    BB_PASS(cx, tid) {
        if (tid < 3 * 64) {
            double* a = red + (tid >> 6) * BB_SCORE_NT + (tid & 63);
            double s = a[0];
            if (max2 && (tid >> 6) == 2) for (int w = 1; w < BB_SCORE_NT / 64; ++w) s = bb_score_max(s, a[64 * w]);
            else for (int w = 1; w < BB_SCORE_NT / 64; ++w) s += a[64 * w];
            a[0] = s;
        }
    }
    BB_SYNC(cx);
    BB_PASS(cx, tid) {
        if (tid < 3) {
            const double* a = red + tid * BB_SCORE_NT;
            double s = a[0];
            if (max2 && tid == 2) for (int g = 1; g < 64; ++g) s = bb_score_max(s, a[g]);
            else for (int g = 1; g < 64; ++g) s += a[g];
            out[tid] = s;
        }
    }
    BB_SYNC(cx);
}

BB_DEV void bb_block_score(BBCtx& cx, const ScoreArgs& A, int nblocks) {
    const PpcArgs& P = A.P;
    const int ns = P.n_samples;
    double* ell = cx.lds;
    double* red = cx.lds + ns;
    double* st = red + 3 * BB_SCORE_NT;
    const long long ncell = P.n_rows * P.n_steps;
    double* par = P.par + (long long)cx.block * P.E * 2 * ns;
    const double rsqrt2 = 0.70710678118654752440, half_log2pi = 0.5 * BB_LOG2PI;
    for (long long row = cx.block; row < P.n_rows; row += nblocks) {
        const int r = (int)(row / A.B);
        const long long b = row % A.B;
        const bool neu = b < A.nn;
        const int T = P.T[r];
        if (!neu) bb_ppc_row_par(cx, P, par, r, b - A.nn);
        BB_PASS(cx, tid) { if (tid == 0) { st[12] = 0.0; st[13] = 0.0; st[14] = 0.0; } }
        for (int t = 0; t < P.n_steps; ++t) {
            const long long c = row * P.n_steps + t;
            const double y = t < T - 1 ? A.y[c] : (double)NAN;
            if (y != y) {                    // no such step, or a zero count: unscored
                BB_PASS(cx, tid) { if (tid < BB_SCORE_CELLS) A.cell[tid * ncell + c] = NAN; }
                continue;
            }
            const int e = (P.kind == 1 || P.kind == 4) ? P.env_idx[P.tcum[r] + t + 1] : 0;
            const double* sbar = P.pop + (long long)(2 * (P.off_t[r] + t)) * ns;
            const double* s_e = par + (long long)(2 * e) * ns;
            // sweep A: the log densities into LDS; first moments
            BB_PASS(cx, tid) {
                double s0 = 0.0, s1 = 0.0, s2 = 0.0;
                for (int j = tid; j < ns; j += BB_SCORE_NT) {
                    const double mu = neu ? -sbar[j] : s_e[j] - sbar[j];
                    const double sd = neu ? sbar[ns + j] : s_e[ns + j];
                    const double z = (y - mu) / sd;
                    const double l = (-0.5 * z * z - log(sd)) - half_log2pi;
                    ell[j] = l;
                    s0 += mu;
                    s1 += sd * sd;
                    s2 += l;
                }
                red[tid] = s0; red[BB_SCORE_NT + tid] = s1; red[2 * BB_SCORE_NT + tid] = s2;
            }
            BB_SYNC(cx);
            bb_score_reduce(cx, red, st, false);
            // sweep B: both tails; the largest log density
            BB_PASS(cx, tid) {
                double s0 = 0.0, s1 = 0.0, mx = -INFINITY;
                for (int j = tid; j < ns; j += BB_SCORE_NT) {
                    const double mu = neu ? -sbar[j] : s_e[j] - sbar[j];
                    const double sd = neu ? sbar[ns + j] : s_e[ns + j];
                    const double u = (y - mu) / sd * rsqrt2;
                    s0 += 0.5 * erfc(-u);
                    s1 += 0.5 * erfc(u);
                    mx = bb_score_max(mx, ell[j]);
                }
                red[tid] = s0; red[BB_SCORE_NT + tid] = s1; red[2 * BB_SCORE_NT + tid] = mx;
            }
            BB_SYNC(cx);
            bb_score_reduce(cx, red, st + 3, true);
            // sweep C: centred second moments, the log-sum-exp about the maximum
            BB_PASS(cx, tid) {
                const double pm = st[0] / ns, lbar = st[2] / ns, m = st[5];
                double s0 = 0.0, s1 = 0.0, s2 = 0.0;
                for (int j = tid; j < ns; j += BB_SCORE_NT) {
                    const double dm = (neu ? -sbar[j] : s_e[j] - sbar[j]) - pm, dl = ell[j] - lbar;
                    s0 += dm * dm;
                    s1 += dl * dl;
                    s2 += exp(ell[j] - m);
                }
                red[tid] = s0; red[BB_SCORE_NT + tid] = s1; red[2 * BB_SCORE_NT + tid] = s2;
            }
            BB_SYNC(cx);
            bb_score_reduce(cx, red, st + 6, false);
            BB_PASS(cx, tid) {
                if (tid == 0) {
                    const double lpd = (st[5] + log(st[8])) - log((double)ns), pw = st[7] / (ns - 1);
                    A.cell[0 * ncell + c] = st[0] / ns;
                    A.cell[1 * ncell + c] = sqrt(st[1] / ns + st[6] / ns);
                    A.cell[2 * ncell + c] = lpd;
                    A.cell[3 * ncell + c] = pw;
                    A.cell[4 * ncell + c] = st[3] / ns;
                    A.cell[5 * ncell + c] = st[4] / ns;
                    st[12] += lpd;
                    st[13] += pw;
                    st[14] += 1.0;
                }
            }
        }
        BB_PASS(cx, tid) {
            if (tid == 0) {
                A.rowsum[row] = st[12];
                A.rowsum[P.n_rows + row] = st[13];
                A.n_scored[row] = (int)st[14];
            }
        }
        BB_SYNC(cx);                         // (the next row's parameter table overwrites what sweep C read)
    }
}
