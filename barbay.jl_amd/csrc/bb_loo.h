// bb_loo.h -- Pareto-smoothed importance-sampling leave-one-out (PSIS-LOO) predictive scores of the observed log-frequency ratios on
// the device: per cell (one observation left out) and per row (a barcode's whole trajectory left out).
// Entry point bb_ppc_loo (include/barbay_hip.h, which states the formulas; Vehtari, Gelman, Gabry 2017; Vehtari et al. 2024; the fit
// of the generalised Pareto distribution is Zhang and Stephens 2009).  No reference counterpart.
//
// Rows, steps, observed ratios and draws are bb_score.h's.  One block program, bb_block_loo: one workgroup of BB_SCORE_NT threads
// per row, row += nblocks.  Per row the parameter table of bb_ppc_row_par; per scored step sweep A of bb_block_score (the log
// densities l_j into LDS, the same expression, so the same bytes) and then bb_loo_psis on them; meanwhile lane i adds l_j of its
// samples j = i, i + NT, ... into registers (at most 8 at the cap), writes the sums l^row_j to LDS after the last step and
// bb_loo_psis runs once more on them: one routine serves both levels.
//
// bb_loo_psis(l[n]) in passes:
//   1  count of non-finite l_j, max l_j (for lpd, bb_score_max's NaN rule), A = max -l_j        one reduction
//   2  lw_j = r_j = (-l_j) - A.  M = min(n / 5, the smallest c with c^2 >= 9 n).  M < 5: nothing to smooth.
//   3  the threshold (T, jT) = the M-th largest of the pairs (r_j, j): a radix select over the order-preserving 64-bit key of
//      r_j, 8-bit digits from the top, then (only where the last bucket holds ties) over j's two digits; one 256-bin LDS histogram
//      (integer atomics) and a scan from the top by one lane per digit, the two histograms alternating so a digit costs two barriers
//   4  the tail {(r_j, j) >= (T, jT)}, exactly M draws, appended to an LDS list (integer atomic counter: the list's order is not
//      fixed, its content is); c = max of the rest                                             one reduction
//   5  the list ranked by counting (lane s counts the pairs below its own, M <= 272 comparisons) into rho_1 <= ... <= rho_M with
//      their draws: the result is defined by the (r_j, j) order, whatever order the list had
//   6  x_i = exp(rho_i) - exp(c); smoothed iff c >= -690 and x* = x_{(M + 2) / 4} > 0
//   7  the fit: theta_i (lane i < m); log1p(-theta_i x_k) for a chunk of 3 NT / M values of i at a time over all lanes into the
//      partials' LDS, then lane i adds its M terms in ascending k; the weights w_i (lane i, m terms each, ascending);
//      theta^ = sum theta_i w_i, kappa(theta^) and the rest by lane 0, ascending
//   8  the tail's lw replaced (lane i < M)
//   9  max (lw + l), max lw; sum exp(lw + l - max), sum exp(lw - max), sum exp(l - max l); sum wt^2     three reductions
// Every sum over j: lane i adds its samples i, i + NT, ... ascending, then bb_score_reduce's order over the NT partials
// (bb_loo_reduce below is that routine with a choice of which of the three are maxima).  No atomics on doubles.
// exp, log, log1p, expm1, sqrt are the platform's (ocml on the device, libm in the emulation), for the reason bb_score.h gives.
// Barrier-separated passes, so the host emulation (BB_EMU) runs the same source.
//
// LDS at n_samples = n: l[n] | lw[n] | three arrays of BB_SCORE_NT partials (24 KiB; the fit's log1p terms while it runs) |
// tail list r[272] | sorted rho, then x [272] | list's draws [272 int] | sorted draws [272 int] | theta[48] | L[48] | scalars[32]:
// 16 n + 32128 bytes; at the cap n = 8192 that is 163200 of the 163840 bytes (160 KiB) a workgroup can have, one workgroup per CU;
// at n = 1000 it is 48128 bytes, three workgroups per CU by LDS -- but the 16 waves of a workgroup at 127 VGPRs (four waves per
// SIMD) fill a CU's registers, so one workgroup per CU runs at every n, as for k_score.
#pragma once
#include "bb_score.h"
#ifdef BB_EMU
#include <vector>
#endif

#define BB_LOO_NSAMP_CAP 8192              // == BB_LOO_MAX_SAMPLES of the public header (bb_analysis.h asserts it)
#define BB_LOO_TAIL_MAX 272                // M at the cap: min(8192 / 5, ceil(3 sqrt 8192)) = min(1638, 272)
#define BB_LOO_GRID_MAX 48                 // m = 30 + floor(sqrt M) <= 46
#define BB_LOO_CELLS 5                     // per-cell results on the device: elpd_loo, p_loo, khat, n_eff, lpd
#define BB_LOO_ROWS 6                      // per-row: row_elpd_loo, row_p_loo, row_khat, row_n_eff, row_elpd_cells, row_khat_max
#define BB_LOO_PER_LANE (BB_LOO_NSAMP_CAP / BB_SCORE_NT)
#define BB_LOO_SCALARS 32
#define BB_LOO_LDS_DOUBLES(ns) (2 * (long long)(ns) + 3 * BB_SCORE_NT + 3 * BB_LOO_TAIL_MAX + 2 * BB_LOO_GRID_MAX + BB_LOO_SCALARS)
static_assert(BB_LOO_LDS_DOUBLES(BB_LOO_NSAMP_CAP) * 8 <= 160 * 1024, "l and lw of a cell at the cap fit the LDS of a workgroup");
static_assert(BB_LOO_TAIL_MAX * BB_LOO_TAIL_MAX >= 9 * BB_LOO_NSAMP_CAP && (BB_LOO_TAIL_MAX - 1) * (BB_LOO_TAIL_MAX - 1) < 9 * BB_LOO_NSAMP_CAP
              && BB_LOO_TAIL_MAX <= BB_LOO_NSAMP_CAP / 5, "BB_LOO_TAIL_MAX is M at the cap");
static_assert(30 + 16 <= BB_LOO_GRID_MAX && 16 * 16 <= BB_LOO_TAIL_MAX && 17 * 17 > BB_LOO_TAIL_MAX, "m <= 46");
static_assert(BB_LOO_TAIL_MAX <= BB_SCORE_NT && 2 * 256 * 4 <= BB_LOO_TAIL_MAX * 8, "a lane per tail draw; a histogram fits a tail array");

struct LooArgs {
    PpcArgs P;                // as ScoreArgs
    const double* y;          // [n_rows][n_steps] observed ratios, NaN: unscored
    double* cell;             // [BB_LOO_CELLS][n_rows n_steps]
    double* rowv;             // [BB_LOO_ROWS][n_rows]
    int* n_scored;            // [n_rows]
    long long B, nn;          // data columns, of which neutral
};

// scalars: 0 .. 2, 3 .. 5, 6 .. 8, 9 .. 11 the four reductions' results; 12 c; 13 theta^; 14 sigma^; 15 khat;
// 16 .. 20 the routine's results elpd_loo, p_loo, khat, n_eff, lpd; 24 .. 27 (as integers) the select's state; 28 .. 31 the row's sums
struct LooLds {
    double *ell, *lw, *red, *tk, *xs, *th, *LL, *st;
    int *ti, *si;
    unsigned long long* su;   // [0] key prefix T, [1] rank from the top inside the bucket, [2] j prefix, [3] the bucket's count
    unsigned* cnt;            // the tail list's length
};
BB_DEV LooLds bb_loo_lds(double* lds, int ns) {
    LooLds W;
    W.ell = lds;
    W.lw = lds + ns;
    W.red = W.lw + ns;
    W.tk = W.red + 3 * BB_SCORE_NT;
    W.xs = W.tk + BB_LOO_TAIL_MAX;
    W.ti = (int*)(W.xs + BB_LOO_TAIL_MAX);
    W.si = W.ti + BB_LOO_TAIL_MAX;
    W.th = W.xs + 2 * BB_LOO_TAIL_MAX;
    W.LL = W.th + BB_LOO_GRID_MAX;
    W.st = W.LL + BB_LOO_GRID_MAX;
    W.su = (unsigned long long*)(W.st + 24);
    W.cnt = (unsigned*)(W.st + 23);
    return W;
}

// bb_score_reduce with a choice of maxima: the three arrays of partials red[3][BB_SCORE_NT] into out[0 .. 3), array a the maximum
// (bb_score_max: a NaN stays) where bit a of maxmask is set, else the sum in bb_score_reduce's order.  Ends with a barrier.
BB_DEV void bb_loo_reduce(BBCtx& cx, double* red, double* out, int maxmask) {
    BB_PASS(cx, tid) {
        if (tid < 3 * 64) {
            double* a = red + (tid >> 6) * BB_SCORE_NT + (tid & 63);
            double s = a[0];
            if ((maxmask >> (tid >> 6)) & 1) for (int w = 1; w < BB_SCORE_NT / 64; ++w) s = bb_score_max(s, a[64 * w]);
            else for (int w = 1; w < BB_SCORE_NT / 64; ++w) s += a[64 * w];
            a[0] = s;
        }
    }
    BB_SYNC(cx);
    BB_PASS(cx, tid) {
        if (tid < 3) {
            const double* a = red + tid * BB_SCORE_NT;
            double s = a[0];
            if ((maxmask >> tid) & 1) for (int g = 1; g < 64; ++g) s = bb_score_max(s, a[g]);
            else for (int g = 1; g < 64; ++g) s += a[g];
            out[tid] = s;
        }
    }
    BB_SYNC(cx);
}

// tail length M of n draws
BB_DEV int bb_loo_tail(int n) {
    int c = 0;
    while (c * c < 9 * n) ++c;               // (n <= 8192: at most 272 steps, once per block)
    const int f = n / 5;
    return f < c ? f : c;
}

// PSIS of the n log densities W.ell (left as they are); W.lw gets the log weights; the five results go to W.st[16 .. 21).  M = bb_loo_tail(n).
// Called by every thread; begins after a barrier that made W.ell visible and ends with one.
BB_DEV void bb_loo_psis(BBCtx& cx, const LooLds& W, int n, int M) {
    double *ell = W.ell, *lw = W.lw, *red = W.red, *st = W.st;
    unsigned* hist0 = (unsigned*)W.tk;       // the two histograms live in the tail arrays, which are filled only after the select
    unsigned* hist1 = (unsigned*)W.xs;
    // 1: non-finite count, max l, max -l
    BB_PASS(cx, tid) {
        double nf = 0.0, mx = -INFINITY, ma = -INFINITY;
        for (int j = tid; j < n; j += BB_SCORE_NT) {
            const double l = ell[j];
            nf += isfinite(l) ? 0.0 : 1.0;
            mx = bb_score_max(mx, l);
            ma = bb_score_max(ma, -l);
        }
        red[tid] = nf; red[BB_SCORE_NT + tid] = mx; red[2 * BB_SCORE_NT + tid] = ma;
        if (tid < 256) hist0[tid] = 0;
        if (tid == 0) { W.su[0] = 0; W.su[1] = (unsigned long long)M; W.su[2] = 0; W.su[3] = 0; *W.cnt = 0; st[15] = INFINITY; }
    }
    BB_SYNC(cx);
    bb_loo_reduce(cx, red, st, 6);
    const bool finite = st[0] == 0.0;
    if (!finite) {
        // a non-finite l_j: lpd by bb_block_score's arithmetic (NaN where an l_j is), every other result NaN
        BB_PASS(cx, tid) {
            const double m = st[1];
            double s2 = 0.0;
            for (int j = tid; j < n; j += BB_SCORE_NT) s2 += exp(ell[j] - m);
            red[tid] = 0.0; red[BB_SCORE_NT + tid] = 0.0; red[2 * BB_SCORE_NT + tid] = s2;
        }
        BB_SYNC(cx);
        bb_loo_reduce(cx, red, st + 6, 0);
        BB_PASS(cx, tid) {
            if (tid == 0) {
                st[16] = NAN; st[17] = NAN; st[18] = NAN; st[19] = NAN;
                st[20] = (st[1] + log(st[8])) - log((double)n);
            }
        }
        BB_SYNC(cx);
        return;
    }
    // 2: the raw log ratios
    BB_PASS(cx, tid) {
        const double A = st[2];
        for (int j = tid; j < n; j += BB_SCORE_NT) lw[j] = (-ell[j]) - A;
    }
    BB_SYNC(cx);
    if (M >= 5) {
        // 3: radix select of the M-th largest (r_j, j); digits 0 .. 7 of the key, then 8, 9 of j where the key's bucket holds ties
        for (int p = 0; p < 10; ++p) {
            unsigned* hist = (p & 1) ? hist1 : hist0;
            unsigned* hnext = (p & 1) ? hist0 : hist1;
            const unsigned long long pre = W.su[0], jpre = W.su[2];
            BB_PASS(cx, tid) {
                for (int j = tid; j < n; j += BB_SCORE_NT) {
                    const unsigned long long k = bb_ppc_key(lw[j]);
                    unsigned d;
                    bool in;
                    if (p < 8) { in = p == 0 || (k >> (64 - 8 * p)) == pre; d = (unsigned)(k >> (56 - 8 * p)) & 255u; }
                    else if (p == 8) { in = k == pre; d = (unsigned)j >> 8; }
                    else { in = k == pre && ((unsigned long long)j >> 8) == jpre; d = (unsigned)j & 255u; }
                    if (in) BB_LDS_ADD_U32(&hist[d], 1u);
                }
            }
            BB_SYNC(cx);
            // the scan from the top by one lane (one lane per bin, each adding the bins above its own, was measured: the kernel
            // took 218 ms in place of 162 ms on C2 at 1000 draws)
            BB_PASS(cx, tid) {
                if (tid < 256) hnext[tid] = 0;
                if (tid == 0) {
                    unsigned long long need = W.su[1];
                    int d = 255;
                    unsigned c = 0;
                    for (; d > 0; --d) {
                        c = hist[d];
                        if (need <= c) break;
                        need -= c;
                    }
                    if (d == 0) c = hist[0];
                    W.su[1] = need;
                    W.su[3] = c;
                    if (p < 8) W.su[0] = (pre << 8) | (unsigned long long)d;
                    else W.su[2] = (jpre << 8) | (unsigned long long)d;
                }
            }
            BB_SYNC(cx);
            if (p == 7 && W.su[3] == 1) break;       // no ties at T: jT = 0
        }
        // 4: the tail into the list, c = max of the rest
        const unsigned long long T = W.su[0], jT = W.su[2];
        BB_PASS(cx, tid) {
            double mc = -INFINITY;
            for (int j = tid; j < n; j += BB_SCORE_NT) {
                const unsigned long long k = bb_ppc_key(lw[j]);
                if (k > T || (k == T && (unsigned long long)j >= jT)) {
#ifdef BB_EMU
                    const unsigned s = (*W.cnt)++;
#else
                    const unsigned s = atomicAdd(W.cnt, 1u);
#endif
                    if (s < (unsigned)BB_LOO_TAIL_MAX) { W.tk[s] = lw[j]; W.ti[s] = j; }     // (s < M by construction; the bound guards the arrays)
                } else mc = bb_score_max(mc, lw[j]);
            }
            red[tid] = 0.0; red[BB_SCORE_NT + tid] = 0.0; red[2 * BB_SCORE_NT + tid] = mc;
        }
        BB_SYNC(cx);
        bb_loo_reduce(cx, red, st + 3, 4);
        // 5 and 6: rank by counting; x_i = exp(rho_i) - exp(c)
        BB_PASS(cx, tid) {
            if (tid == 0) st[12] = st[5];
            if (tid < M) {
                const double r = W.tk[tid];
                const int j = W.ti[tid];
                int rank = 0;
                for (int s = 0; s < M; ++s) rank += (W.tk[s] < r || (W.tk[s] == r && W.ti[s] < j)) ? 1 : 0;
                W.xs[rank] = exp(r) - exp(st[5]);
                W.si[rank] = j;
            }
        }
        BB_SYNC(cx);
        const double cc = st[12], xstar = W.xs[(M + 2) / 4 - 1], xM = W.xs[M - 1];
        if (cc >= -690.0 && xstar > 0.0) {
            // 7: the generalised Pareto fit
            int m = 30;
            while ((m - 29) * (m - 29) <= M) ++m;        // m = 30 + floor(sqrt M)
            BB_PASS(cx, tid) {
                if (tid < m) W.th[tid] = 1.0 / xM + (1.0 - sqrt((double)m / ((double)tid + 0.5))) / (3.0 * xstar);
            }
            BB_SYNC(cx);
            const int G = 3 * BB_SCORE_NT / M;
            for (int i0 = 0; i0 < m; i0 += G) {
                const int g = m - i0 < G ? m - i0 : G;
                BB_PASS(cx, tid) {
                    for (int e = tid; e < g * M; e += BB_SCORE_NT) red[e] = log1p(-W.th[i0 + e / M] * W.xs[e % M]);
                }
                BB_SYNC(cx);
                BB_PASS(cx, tid) {
                    if (tid < g) {
                        const double* a = red + tid * M;
                        double s = a[0];
                        for (int k = 1; k < M; ++k) s += a[k];
                        const double kap = s / (double)M;
                        W.LL[i0 + tid] = (double)M * ((log(-W.th[i0 + tid] / kap) - kap) - 1.0);
                    }
                }
                BB_SYNC(cx);
            }
            BB_PASS(cx, tid) {
                if (tid < m) {
                    const double Li = W.LL[tid];
                    double s = exp(W.LL[0] - Li);
                    for (int j = 1; j < m; ++j) s += exp(W.LL[j] - Li);
                    red[tid] = W.th[tid] * (1.0 / s);
                }
            }
            BB_SYNC(cx);
            BB_PASS(cx, tid) {
                if (tid == 0) {
                    double s = red[0];
                    for (int i = 1; i < m; ++i) s += red[i];
                    st[13] = s;
                }
            }
            BB_SYNC(cx);
            BB_PASS(cx, tid) { if (tid < M) red[tid] = log1p(-st[13] * W.xs[tid]); }
            BB_SYNC(cx);
            BB_PASS(cx, tid) {
                if (tid == 0) {
                    double s = red[0];
                    for (int k = 1; k < M; ++k) s += red[k];
                    const double kraw = s / (double)M;
                    st[14] = -kraw / st[13];
                    st[15] = ((double)M * kraw + 5.0) / ((double)M + 10.0);
                }
            }
            BB_SYNC(cx);
            // 8: the smoothed tail
            BB_PASS(cx, tid) {
                if (tid < M) {
                    const double kh = st[15], p = ((double)tid + 0.5) / (double)M;
                    const double v = log(st[14] * expm1(-kh * log1p(-p)) / kh + exp(cc));
                    const int j = W.si[tid];
                    if ((unsigned)j < (unsigned)n) lw[j] = v > 0.0 ? 0.0 : v;       // (always: the ranks are a permutation; the bound guards the array)
                }
            }
            BB_SYNC(cx);
        }
    }
    // 9: the estimates
    BB_PASS(cx, tid) {
        double m1 = -INFINITY, m2 = -INFINITY;
        for (int j = tid; j < n; j += BB_SCORE_NT) {
            m1 = bb_score_max(m1, lw[j] + ell[j]);
            m2 = bb_score_max(m2, lw[j]);
        }
        red[tid] = m1; red[BB_SCORE_NT + tid] = m2; red[2 * BB_SCORE_NT + tid] = 0.0;
    }
    BB_SYNC(cx);
    bb_loo_reduce(cx, red, st + 3, 3);
    BB_PASS(cx, tid) {
        const double m1 = st[3], m2 = st[4], m = st[1];
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (int j = tid; j < n; j += BB_SCORE_NT) {
            s0 += exp((lw[j] + ell[j]) - m1);
            s1 += exp(lw[j] - m2);
            s2 += exp(ell[j] - m);
        }
        red[tid] = s0; red[BB_SCORE_NT + tid] = s1; red[2 * BB_SCORE_NT + tid] = s2;
    }
    BB_SYNC(cx);
    bb_loo_reduce(cx, red, st + 6, 0);
    BB_PASS(cx, tid) {
        const double lse = st[4] + log(st[7]);
        double s0 = 0.0;
        for (int j = tid; j < n; j += BB_SCORE_NT) {
            const double wt = exp(lw[j] - lse);
            s0 += wt * wt;
        }
        red[tid] = s0; red[BB_SCORE_NT + tid] = 0.0; red[2 * BB_SCORE_NT + tid] = 0.0;
    }
    BB_SYNC(cx);
    bb_loo_reduce(cx, red, st + 9, 0);
    BB_PASS(cx, tid) {
        if (tid == 0) {
            const double lpd = (st[1] + log(st[8])) - log((double)n);
            const double elpd = (st[3] + log(st[6])) - (st[4] + log(st[7]));
            st[16] = elpd;
            st[17] = lpd - elpd;
            st[18] = st[15];
            st[19] = 1.0 / st[9];
            st[20] = lpd;
        }
    }
    BB_SYNC(cx);
}

// lane tid's k-th running sum l^row_j, j = tid + k NT: registers on the device, an array over all lanes in the emulation (whose
// passes run the lanes one after another)
#ifdef BB_EMU
#define BB_LOO_ACC(k, tid) acc[(k) * BB_SCORE_NT + (tid)]
#define BB_LOO_ACC_DECL std::vector<double> acc((size_t)BB_LOO_NSAMP_CAP)
#else
#define BB_LOO_ACC(k, tid) acc[k]
#define BB_LOO_ACC_DECL double acc[BB_LOO_PER_LANE]
#endif

BB_DEV void bb_block_loo(BBCtx& cx, const LooArgs& A, int nblocks) {
    const PpcArgs& P = A.P;
    const int ns = P.n_samples;
    const LooLds W = bb_loo_lds(cx.lds, ns);
    double *ell = W.ell, *st = W.st;
    const long long ncell = P.n_rows * P.n_steps;
    double* par = P.par + (long long)cx.block * P.E * 2 * ns;
    const double half_log2pi = 0.5 * BB_LOG2PI;
    const int M = bb_loo_tail(ns);
    BB_LOO_ACC_DECL;
    for (long long row = cx.block; row < P.n_rows; row += nblocks) {
        const int r = (int)(row / A.B);
        const long long b = row % A.B;
        const bool neu = b < A.nn;
        const int T = P.T[r];
        if (!neu) bb_ppc_row_par(cx, P, par, r, b - A.nn);
        BB_PASS(cx, tid) { if (tid == 0) { st[28] = 0.0; st[29] = -INFINITY; st[30] = 0.0; } }
        int scored = 0;
        for (int t = 0; t < P.n_steps; ++t) {
            const long long c = row * P.n_steps + t;
            const double y = t < T - 1 ? A.y[c] : (double)NAN;
            if (y != y) {                    // no such step, or a zero count: unscored
                BB_PASS(cx, tid) { if (tid < BB_LOO_CELLS) A.cell[tid * ncell + c] = NAN; }
                continue;
            }
            const int e = (P.kind == 1 || P.kind == 4) ? P.env_idx[P.tcum[r] + t + 1] : 0;
            const double* sbar = P.pop + (long long)(2 * (P.off_t[r] + t)) * ns;
            const double* s_e = par + (long long)(2 * e) * ns;
            const bool first = scored == 0;
            // sweep A of bb_block_score: the log densities into LDS, and into the row's running sums
            BB_PASS(cx, tid) {
#ifndef BB_EMU
#pragma unroll
#endif
                for (int k = 0; k < BB_LOO_PER_LANE; ++k) {
                    const int j = tid + k * BB_SCORE_NT;
                    if (j < ns) {
                        const double mu = neu ? -sbar[j] : s_e[j] - sbar[j];
                        const double sd = neu ? sbar[ns + j] : s_e[ns + j];
                        const double z = (y - mu) / sd;
                        const double l = (-0.5 * z * z - log(sd)) - half_log2pi;
                        ell[j] = l;
                        BB_LOO_ACC(k, tid) = first ? l : BB_LOO_ACC(k, tid) + l;
                    }
                }
            }
            BB_SYNC(cx);
            bb_loo_psis(cx, W, ns, M);
            BB_PASS(cx, tid) {
                if (tid < BB_LOO_CELLS) A.cell[tid * ncell + c] = st[16 + tid];
                if (tid == 0) {
                    st[28] += st[16];
                    st[29] = bb_score_max(st[29], st[18]);
                    st[30] += 1.0;
                }
            }
            ++scored;
        }
        if (scored) {
            BB_SYNC(cx);                     // (the last cell's results are read above, the routine's first pass writes scalars)
            BB_PASS(cx, tid) {
#ifndef BB_EMU
#pragma unroll
#endif
                for (int k = 0; k < BB_LOO_PER_LANE; ++k) {
                    const int j = tid + k * BB_SCORE_NT;
                    if (j < ns) ell[j] = BB_LOO_ACC(k, tid);
                }
            }
            BB_SYNC(cx);
            bb_loo_psis(cx, W, ns, M);
        }
        BB_PASS(cx, tid) {
            if (tid < 4) A.rowv[tid * P.n_rows + row] = scored ? st[16 + tid] : (double)NAN;
            if (tid == 0) {
                A.rowv[4 * P.n_rows + row] = scored ? st[28] : (double)NAN;
                A.rowv[5 * P.n_rows + row] = scored ? st[29] : (double)NAN;
                A.n_scored[row] = (int)st[30];
            }
        }
        BB_SYNC(cx);                         // (the next row's parameter table and scalars overwrite what was read)
    }
}
