// bb_lsrb.h -- Rao-Blackwellised marginals of the noise scales logsigma_bc and logsigma_pop on the device.  Entry point bb_logsigma_rb
// (include/barbay_hip.h, where the rule is defined); no reference counterpart.
//
// Given everything else a log-scale l enters the log-joint through its Gaussian prior N(a, b) and n Gaussian terms of scale e^l whose
// residuals d do not read l: h(l) = -(l - a)^2 ib2 / 2 - n l - (SS / 2) e^{-2l}, SS the sum of the d^2.  Not Gaussian, but
// one-dimensional and strictly log-concave, so per draw j of everything else (bb_rb.h's draws: same keying, or the caller's rows) the
// conditional is integrated numerically: the mode l*_j by a Newton iteration in the log domain, then trapezoid nodes on
// [l* - 10 delta, l* + 22 r delta] at a step of delta / 4 or finer (bb_ls_grid), delta the curvature scale at the mode.  The
// per-draw moments are averaged over j; the quantiles are those of the mixture of the per-draw CDFs, by bisection.
//
// Phases of a call (bb_analysis.h): bb_rb.h's front as it stands -- bb_block_ppc_pop (sbar_{t,j}; BC only), bb_block_freq_zpart /
// _zsum, bb_block_rb_logz (ln Z in place) -- then
//   BC   bb_block_ls_bc   : one workgroup of BB_SCORE_NT threads per mutant row (r, m), row += nblocks.  Per environment e (entry
//        u = bb_fitness_rb's unit) one walk over the row's loglambda draws, the unit's s_j in a register (so no accumulator is indexed
//        by a run-time environment: that would be scratch memory): SS_j += d_t^2 for the steps of e, ascending t, from 0.0, into the
//        block's slice of a global table; then bb_ls_mixture.
//   POP  bb_block_ls_pop_part : one workgroup per (group g = (r, k), chunk of BB_POP_CHUNK consecutive neutral members),
//        work += nblocks; per draw the chunk's sum of d_i^2 from 0.0 in index order, the ragged method's pairing as in
//        bb_block_pop_part, into part[work][n_samples].
//        bb_block_ls_pop  : one workgroup per group; per draw the chunk partials from 0.0 in chunk order; then bb_ls_mixture.
//   bb_ls_mixture, shared (draw j is lane j mod BB_SCORE_NT's in every sweep, so a lane reads only table entries it wrote):
//     A  per draw the mode, delta, the grid: l*, delta, Z into LDS; l, E, V, S, hi into the block's table -> sum l, sum E, sum V
//     A' (no arithmetic on the grid)                                                                       -> sum S, sum l*, max hi_j
//     B  centred second moments                                            -> sum (l - q_mean)^2, sum (E - rb_mean)^2, max -lo_j
//     Q  bisection of the mixture CDF, BB_LS_ITER steps, up to three quantiles per sweep as bb_rb_mixture does; a draw whose
//        [lo_j, hi_j] does not hold the midpoint adds 0 or 1 and evaluates nothing.
// The maximum of hi_j takes NaN for a draw whose Z_j is not finite, so that the bracket is finite exactly when every l*_j, delta_j
// and Z_j is.  Sums and maxima in bb_score_reduce's order; exp, expm1, log, sqrt, ceil are the platform's, as in bb_rb.h.
// Barrier-separated passes, so the host emulation (BB_EMU) runs the same source.
#pragma once
#include "bb_rb.h"

#define BB_LS_ITER 40                      // bisection steps
#define BB_LS_LEFT 10                      // the grid starts at lo = l* - 10 delta ...
#define BB_LS_RIGHT 22                     // ... and ends at hi = l* + 22 r delta, r = 1, 2, 4 .. BB_LS_RIGHT_MAX: the first at which the
#define BB_LS_RIGHT_MAX 64                 //     density has fallen to exp(BB_LS_TAIL) of its mode's
#define BB_LS_TAIL (-40.0)
#define BB_LS_REFINE_MAX 64                // the step is delta / (4 m), m = ceil(2 delta) up to this (a delta of 32 is no log-scale's)
#define BB_LS_TAB 6                        // per-block global table [6][n_samples]: SS_j, l_j, E_j, V_j, S_j, hi_j
// LDS: l*[n_samples] | delta[n_samples] | Z[n_samples] | three arrays of BB_SCORE_NT partials | scalars (bb_rb.h's st[] layout)
#define BB_LS_LDS_DOUBLES(ns) (3 * (long long)(ns) + 3 * BB_SCORE_NT + BB_RB_SCALARS)
// the largest n_samples whose layout fits the 160 KiB of LDS a workgroup can have
#define BB_LS_SAMPLES_CAP ((160 * 1024 / 8 - 3 * BB_SCORE_NT - BB_RB_SCALARS) / 3)
static_assert(BB_LS_LDS_DOUBLES(BB_LS_SAMPLES_CAP) * 8 <= 160 * 1024 && BB_LS_LDS_DOUBLES(BB_LS_SAMPLES_CAP + 1) * 8 > 160 * 1024,
              "BB_LS_SAMPLES_CAP is the largest count that fits");
static_assert(BB_LS_SAMPLES_CAP == 5781, "3 x 5781 doubles of (l*, delta, Z) + 24 KiB of partials + 512 B of scalars <= 160 KiB");

struct LsArgs {
    RbArgs A;                 // as for bb_block_rb: F, probs, nq, n_z; unit [BB_RB_OUT][n_entries]: q_mean, q_sd, rb_mean, rb_sd, sigma_mean,
                              // mode_mean; quant [n_entries][8]; n_steps [n_entries]: n_terms; n_units = n_entries;
                              // ytab [gridDim][BB_LS_TAB][n_samples]; A.F.P.pri_*: the block's prior, indexed by entry
    const int* neu_t;         // POP: bb_block_pop_part's pairing table, nullptr: t = k, b = i
    const int* neu_b;
    double* part;             // POP: [(g1 - g0) nchunks][n_samples] chunk partials of the groups in flight
    long long g0, g1;         // POP: the groups in flight
    int nchunks;              // POP: chunks of a group: ceil(nn / BB_POP_CHUNK)
};

// the conditional of one draw about its mode: everything the grid and the CDF read
struct LsCond {
    double a, ib2, n;         // the prior (mean, 1 / std^2), the number of terms
    double lm, W, c1;         // l*, W = SS e^{-2 l*}, c1 = ib2 (l* - a) + n  (= W at an exact root)
};

// p(u) = exp(h(l* + u) - h(l*)), in the form without cancelling large terms:
// h(l* + u) - h(l*) = -u c1 - ib2 u^2 / 2 - (W / 2) expm1(-2u);  *em1 = expm1(-2u)
BB_DEV double bb_ls_p(const LsCond& c, double u, double* em1) {
    const double x = expm1(-2.0 * u);
    *em1 = x;
    const double tail = c.W != 0.0 ? 0.5 * c.W * x : 0.0;      // (no term at all where SS = 0: 0 x inf would be NaN)
    return exp(-(u * c.c1) - 0.5 * c.ib2 * (u * u) - tail);
}
// h'(l* + u) = -(l* + u - a) ib2 - n + W e^{-2u}
BB_DEV double bb_ls_dh(const LsCond& c, double u, double em1) {
    return -((c.lm + u) - c.a) * c.ib2 - c.n + (c.W != 0.0 ? c.W * (em1 + 1.0) : 0.0);
}

// the mode of draw j's conditional (the header's rule) and with it c.lm, c.W, c.c1; returns delta
BB_DEV double bb_ls_mode(LsCond& c, double SS) {
    double lm;
    if (SS == 0.0) {
        lm = c.a - c.n / c.ib2;
    } else {
        const double c2 = 2.0 / c.ib2, lnK = log(SS) - 2.0 * c.a + c2 * c.n;
        double t = lnK >= c2 ? log(lnK / c2) : lnK;
        for (int it = 0; it < 50; ++it) {
            const double et = exp(t), step = ((t + c2 * et) - lnK) / (1.0 + c2 * et);
            t -= step;
            if (fabs(step) <= 9.094947017729282e-13 * (1.0 + fabs(t))) break;      // 2^-40
        }
        lm = c.a + (exp(t) - c.n) / c.ib2;
    }
    c.lm = lm;
    c.W = SS == 0.0 ? 0.0 : SS * exp(-2.0 * lm);
    c.c1 = c.ib2 * (lm - c.a) + c.n;
    return 1.0 / sqrt(c.ib2 + 2.0 * c.W);
}

// m of bb_ls_grid: max(1, ceil(2 delta)), at most BB_LS_REFINE_MAX (and 1 for a NaN delta)
BB_DEV double bb_ls_refine(double dl) {
    const double m = ceil(2.0 * dl);
    return m >= 1.0 ? (m <= (double)BB_LS_REFINE_MAX ? m : (double)BB_LS_REFINE_MAX) : 1.0;
}

// The grid of one draw: the step s = delta / (4 m), m = max(1, ceil(2 delta)), so that s <= 1/8 whatever delta is -- the factor
// exp(-(SS / 2) e^{-2l}) cuts the density off on the left over a width of about 1/2 in l, which a step of delta / 4 alone does not
// resolve where delta is near a wide prior's b -- and the right extent 22 r delta (BB_LS_RIGHT above).  *nleft, *nright: intervals
// left and right of the mode, which is a node.
BB_DEV double bb_ls_grid(const LsCond& c, double dl, int* nleft, int* nright) {
    const double m = bb_ls_refine(dl);
    int r = 1;
    double e;
    while (r < BB_LS_RIGHT_MAX && log(bb_ls_p(c, (double)(BB_LS_RIGHT * r) * dl, &e)) > BB_LS_TAIL) r *= 2;
    const int m4 = 4 * (int)m;
    *nleft = BB_LS_LEFT * m4;
    *nright = BB_LS_RIGHT * r * m4;
    return dl / (double)m4;
}

// draw j's CDF at x, times Z_j: the trapezoid on N + 1 equidistant nodes from lo_j to x less the first Euler-Maclaurin end term;
// lo_j < x < hi_j
BB_DEV double bb_ls_cdf_z(const LsCond& c, double dl, double x) {
    const double mm = bb_ls_refine(dl);
    const double ulo = -10.0 * dl, r = x - (c.lm + ulo), s = dl / (4.0 * mm);
    double N = ceil(r / s);
    N = N >= 1.0 ? N : 1.0;
    const double sx = r / N;
    const int n = (int)N;
    double e0, e1;
    const double p0 = bb_ls_p(c, ulo, &e0), ux = x - c.lm, p1 = bb_ls_p(c, ux, &e1);
    double acc = 0.5 * p0, e;
    for (int i = 1; i < n; ++i) acc += bb_ls_p(c, ulo + (double)i * sx, &e);
    acc += 0.5 * p1;
    return sx * acc - sx * sx / 12.0 * (bb_ls_dh(c, ux, e1) * p1 - bb_ls_dh(c, ulo, e0) * p0);
}

// The mixture of an entry's conditionals, shared by both blocks: ss[j] holds SS_j (the caller's pass, same lane), latent(j) gives
// the entry's own draw l_j; the six results go to unit[k n_units + u], the nq quantiles to quant[u][BB_RB_MAX_Q].  tab: the block's
// [BB_LS_TAB][ns] table, row 0 == ss.  Ends with a barrier: the next entry's sweep A overwrites what this one read.
template <class Latent>
BB_DEV void bb_ls_mixture(BBCtx& cx, int ns, int nq, const double* probs, double a, double ib2, int nterms, double* tab, double* lds,
                          double* unit, long long n_units, long long u, double* quant, Latent&& latent) {
    double* ms = lds;
    double* dls = lds + ns;
    double* zz = lds + 2 * (long long)ns;
    double* red = lds + 3 * (long long)ns;
    double* st = red + 3 * BB_SCORE_NT;
    const double* ss = tab;
    double* lj = tab + ns;
    double* ej = tab + 2 * (long long)ns;
    double* vj = tab + 3 * (long long)ns;
    double* sgj = tab + 4 * (long long)ns;
    double* hij = tab + 5 * (long long)ns;
    // sweep A: mode, grid and per-draw moments; first sums
    BB_PASS(cx, tid) {
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
        for (int j = tid; j < ns; j += BB_SCORE_NT) {
            LsCond c;
            c.a = a; c.ib2 = ib2; c.n = (double)nterms;
            const double dl = bb_ls_mode(c, ss[j]);
            int nleft = 0, nright = 0;
            const double s = bb_ls_grid(c, dl, &nleft, &nright);
            const int nodes = nleft + nright;
            double z = 0.0, m1 = 0.0, m2 = 0.0, se = 0.0;
            for (int k = 0; k <= nodes; ++k) {
                const double uk = (double)(k - nleft) * s;
                double e;
                double p = bb_ls_p(c, uk, &e);
                if (k == 0 || k == nodes) p *= 0.5;
                z += p;
                m1 += p * uk;
                m2 += p * (uk * uk);
                se += p * exp(uk);
            }
            const double Z = s * z, r1 = m1 / z, E = c.lm + r1, V = m2 / z - r1 * r1, S = exp(c.lm) * (se / z);
            const double l = latent(j);
            ms[j] = c.lm; dls[j] = dl; zz[j] = Z;
            lj[j] = l; ej[j] = E; vj[j] = V; sgj[j] = S; hij[j] = c.lm + (double)nright * s;
            a0 += l;
            a1 += E;
            a2 += V;
        }
        red[tid] = a0; red[BB_SCORE_NT + tid] = a1; red[2 * BB_SCORE_NT + tid] = a2;
    }
    BB_SYNC(cx);
    bb_score_reduce(cx, red, st, false);
    // sweep A': the other first sums; the largest hi_j (NaN where Z_j is not finite)
    BB_PASS(cx, tid) {
        double a0 = 0.0, a1 = 0.0, mx = -INFINITY;
        for (int j = tid; j < ns; j += BB_SCORE_NT) {
            a0 += sgj[j];
            a1 += ms[j];
            mx = bb_score_max(mx, isfinite(zz[j]) ? hij[j] : (double)NAN);
        }
        red[tid] = a0; red[BB_SCORE_NT + tid] = a1; red[2 * BB_SCORE_NT + tid] = mx;
    }
    BB_SYNC(cx);
    bb_score_reduce(cx, red, st + 3, true);
    // sweep B: centred second moments; the smallest lo_j (as the largest of -lo_j)
    BB_PASS(cx, tid) {
        const double qm = st[0] / ns, rm = st[1] / ns;
        double a0 = 0.0, a1 = 0.0, mx = -INFINITY;
        for (int j = tid; j < ns; j += BB_SCORE_NT) {
            const double d0 = lj[j] - qm, d1 = ej[j] - rm;
            a0 += d0 * d0;
            a1 += d1 * d1;
            mx = bb_score_max(mx, -(ms[j] - 10.0 * dls[j]));
        }
        red[tid] = a0; red[BB_SCORE_NT + tid] = a1; red[2 * BB_SCORE_NT + tid] = mx;
    }
    BB_SYNC(cx);
    bb_score_reduce(cx, red, st + 6, true);
    BB_PASS(cx, tid) {
        if (tid == 0) {
            unit[0 * n_units + u] = st[0] / ns;
            unit[1 * n_units + u] = sqrt(st[6] / ns);
            unit[2 * n_units + u] = st[1] / ns;
            unit[3 * n_units + u] = sqrt(st[2] / ns + st[7] / ns);
            unit[4 * n_units + u] = st[3] / ns;
            unit[5 * n_units + u] = st[4] / ns;
            const double lo = -st[8], hi = st[5];
            st[15] = (nq > 0 && isfinite(lo) && isfinite(hi)) ? 1.0 : 0.0;
            for (int i = 0; i < nq; ++i) { st[16 + i] = lo; st[24 + i] = hi; }
        }
    }
    BB_SYNC(cx);
    if (nq > 0 && st[15] == 0.0) {   // a non-finite l*_j, delta_j or Z_j: no bracket
        BB_PASS(cx, tid) { if (tid < nq) quant[u * BB_RB_MAX_Q + tid] = NAN; }
    } else if (nq > 0) {
        for (int it = 0; it < BB_LS_ITER; ++it) {
            for (int q0 = 0; q0 < nq; q0 += 3) {
                // sweep Q: the mixture CDF at the midpoints of up to three brackets
                BB_PASS(cx, tid) {
                    const int nx = nq - q0 < 3 ? nq - q0 : 3;
                    double acc[3] = {0.0, 0.0, 0.0}, xs[3];
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        const int qi = i < nx ? q0 + i : q0;
                        xs[i] = st[16 + qi] + (st[24 + qi] - st[16 + qi]) / 2.0;
                    }
                    for (int j = tid; j < ns; j += BB_SCORE_NT) {
                        LsCond c;
                        c.a = a; c.ib2 = ib2; c.n = (double)nterms;
                        const double lm = ms[j], dl = dls[j], lo = lm - 10.0 * dl, hi = hij[j];
                        bool have = false;
#pragma unroll
                        for (int i = 0; i < 3; ++i) {
                            if (i >= nx) continue;
                            const double x = xs[i];
                            if (x <= lo) continue;                       // C_j = 0
                            if (x >= hi) { acc[i] += 1.0; continue; }    // C_j = 1
                            if (!have) {
                                const double SS = ss[j];
                                c.lm = lm;
                                c.W = SS == 0.0 ? 0.0 : SS * exp(-2.0 * lm);
                                c.c1 = ib2 * (lm - a) + c.n;
                                have = true;
                            }
                            const double C = bb_ls_cdf_z(c, dl, x) / zz[j];
                            acc[i] += C < 0.0 ? 0.0 : (C > 1.0 ? 1.0 : C);
                        }
                    }
                    red[tid] = acc[0]; red[BB_SCORE_NT + tid] = acc[1]; red[2 * BB_SCORE_NT + tid] = acc[2];
                }
                BB_SYNC(cx);
                bb_score_reduce(cx, red, st + 12, false);
                BB_PASS(cx, tid) {
                    if (tid < 3 && q0 + tid < nq) {
                        const int i = q0 + tid;
                        const double x = st[16 + i] + (st[24 + i] - st[16 + i]) / 2.0;
                        if (st[12 + tid] / ns < probs[i]) st[16 + i] = x;
                        else st[24 + i] = x;
                    }
                }
                BB_SYNC(cx);
            }
        }
        BB_PASS(cx, tid) { if (tid < nq) quant[u * BB_RB_MAX_Q + tid] = st[16 + tid] + (st[24 + tid] - st[16 + tid]) / 2.0; }
    }
    BB_SYNC(cx);
}

BB_DEV void bb_block_ls_bc(BBCtx& cx, const LsArgs& L, int nblocks) {
    const RbArgs& A = L.A;
    const FreqArgs& F = A.F;
    const PpcArgs& P = F.P;
    const int ns = P.n_samples, E = P.E;
    double* tab = A.ytab + (long long)cx.block * BB_LS_TAB * ns;
    const bool hier = P.kind >= 2, menv = P.kind == 1 || P.kind == 4;
    for (long long row = cx.block; row < P.n_rows; row += nblocks) {
        const int r = (int)(row / P.nb);
        const long long m = row % P.nb;
        const int T = P.T[r];
        const long long ll = F.off_l[r] + (F.nn + m) * T;
        const double* Z = F.Z + (long long)P.tcum[r] * ns;      // ln Z (bb_block_rb_logz)
        const double* sbar = P.pop + (long long)(2 * P.off_t[r]) * ns;
        for (int e = 0; e < E; ++e) {
            const long long em = e + (long long)E * m, u = em + (long long)E * P.nb * r;
            const long long th = P.kind == 2 ? P.geno_idx[m] : em, uu = P.kind == 2 ? m : u, ent = hier ? uu : em;
            int nu = 0;
            for (int t = 0; t + 1 < T; ++t) nu += !menv || P.env_idx[P.tcum[r] + t + 1] == e;
            // pass S: the unit's SS_j in one walk over the row's loglambda draws, its fitness draw in a register
            BB_PASS(cx, tid) {
                if (tid == 0) A.n_steps[ent] = nu;
                for (int j = tid; j < ns; j += BB_SCORE_NT) {
                    double s;
                    if (!hier) s = bb_ppc_param(P, P.lo_s + em, j);
                    else s = bb_ppc_param(P, P.lo_s + th, j) + exp(bb_ppc_param(P, P.lo_lt + uu, j)) * bb_ppc_param(P, P.lo_tt + uu, j);
                    double SS = 0.0, l0 = bb_ppc_param(P, ll, j), z0 = Z[j];
                    for (int t = 0; t + 1 < T; ++t) {
                        const double l1 = bb_ppc_param(P, ll + t + 1, j), z1 = Z[(long long)(t + 1) * ns + j];
                        if (!menv || P.env_idx[P.tcum[r] + t + 1] == e) {
                            const double d = (((l1 - l0) - (z1 - z0)) + sbar[(long long)(2 * t) * ns + j]) - s;
                            SS += d * d;
                        }
                        l0 = l1;
                        z0 = z1;
                    }
                    tab[j] = SS;
                }
            }
            const double a = P.pri_mean_e ? P.pri_mean_e[ent] : P.pri_mean, ib2 = P.pri_ivar_e ? P.pri_ivar_e[ent] : P.pri_ivar;
            bb_ls_mixture(cx, ns, A.nq, A.probs, a, ib2, nu, tab, cx.lds, A.unit, A.n_units, ent, A.quant,
                          [&](int j) { return bb_ppc_param(P, P.lo_ls + ent, j); });
        }
    }
}

BB_DEV void bb_block_ls_pop_part(BBCtx& cx, const LsArgs& L, int nblocks) {
    const FreqArgs& F = L.A.F;
    const PpcArgs& P = F.P;
    const int ns = P.n_samples;
    const long long nn = F.nn, nwork = (L.g1 - L.g0) * L.nchunks;
    for (long long wk = cx.block; wk < nwork; wk += nblocks) {
        const long long g = L.g0 + wk / L.nchunks;
        const int c = (int)(wk % L.nchunks);
        int r = 0;
        while (r + 1 < P.R && g >= P.off_t[r + 1]) ++r;
        const int k = (int)(g - P.off_t[r]), T = P.T[r];
        const long long i0 = (long long)c * BB_POP_CHUNK, i1 = i0 + BB_POP_CHUNK < nn ? i0 + BB_POP_CHUNK : nn;
        const double* Z = F.Z + (long long)P.tcum[r] * ns;      // ln Z (bb_block_rb_logz)
        double* part = L.part + wk * ns;
        BB_PASS(cx, tid) {
            for (int j = tid; j < ns; j += BB_SCORE_NT) {
                const double sb = bb_ppc_param(P, P.lo_spop + g, j);
                double SS = 0.0;
                for (long long i = i0; i < i1; ++i) {
                    int t = k;
                    long long b = i;
                    if (L.neu_t) { t = L.neu_t[g * nn + i]; b = L.neu_b[g * nn + i]; }
                    const long long ll = F.off_l[r] + b * T + t;
                    const double l0 = bb_ppc_param(P, ll, j), l1 = bb_ppc_param(P, ll + 1, j);
                    const double d = ((l1 - l0) - (Z[(long long)(t + 1) * ns + j] - Z[(long long)t * ns + j])) + sb;
                    SS += d * d;
                }
                part[j] = SS;
            }
        }
    }
}

BB_DEV void bb_block_ls_pop(BBCtx& cx, const LsArgs& L, int nblocks) {
    const RbArgs& A = L.A;
    const PpcArgs& P = A.F.P;
    const int ns = P.n_samples;
    double* tab = A.ytab + (long long)cx.block * BB_LS_TAB * ns;
    for (long long g = L.g0 + cx.block; g < L.g1; g += nblocks) {
        const double* part = L.part + (g - L.g0) * L.nchunks * ns;
        BB_PASS(cx, tid) {
            if (tid == 0) A.n_steps[g] = (int)A.F.nn;
            for (int j = tid; j < ns; j += BB_SCORE_NT) {
                double SS = 0.0;
                for (int c = 0; c < L.nchunks; ++c) SS += part[(long long)c * ns + j];
                tab[j] = SS;
            }
        }
        const double a = P.pri_mean_e ? P.pri_mean_e[g] : P.pri_mean, ib2 = P.pri_ivar_e ? P.pri_ivar_e[g] : P.pri_ivar;
        bb_ls_mixture(cx, ns, A.nq, A.probs, a, ib2, (int)A.F.nn, tab, cx.lds, A.unit, A.n_units, g, A.quant,
                      [&](int j) { return bb_ppc_param(P, P.lo_lspop + g, j); });
    }
}
