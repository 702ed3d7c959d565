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
//        block's slice of a global table; then bb_grid_mixture (bb_gridmix.h: the sweeps, the NaN rule, the quantiles) over LsMix.
//   POP  bb_block_ls_pop_part : one workgroup per (group g = (r, k), chunk of BB_POP_CHUNK consecutive neutral members),
//        work += nblocks; per draw the chunk's sum of d_i^2 from 0.0 in index order, the ragged method's pairing as in
//        bb_block_pop_part, into part[work][n_samples].
//        bb_block_ls_pop  : one workgroup per group; per draw the chunk partials from 0.0 in chunk order; then the same.
// exp, expm1, log, sqrt, ceil are the platform's, as in bb_rb.h.
#pragma once
#include "bb_gridmix.h"

#define BB_LS_LEFT 10                      // the grid starts at lo = l* - 10 delta ...
#define BB_LS_RIGHT 22                     // ... and ends at hi = l* + 22 r delta, r = 1, 2, 4 .. BB_LS_RIGHT_MAX: the first at which the
#define BB_LS_RIGHT_MAX 64                 //     density has fallen to exp(BB_GRID_TAIL) of its mode's
#define BB_LS_TAB 6                        // per-block global table [6][n_samples]: SS_j, l_j, E_j, V_j, S_j, hi_j

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

// m of bb_ls_grid: max(1, ceil(2 delta)), at most BB_GRID_REFINE_MAX (and 1 for a NaN delta)
BB_DEV double bb_ls_refine(double dl) { return bb_grid_refine(ceil(2.0 * dl)); }

// The grid of one draw: the step s = delta / (4 m), m = max(1, ceil(2 delta)), so that s <= 1/8 whatever delta is -- the factor
// exp(-(SS / 2) e^{-2l}) cuts the density off on the left over a width of about 1/2 in l, which a step of delta / 4 alone does not
// resolve where delta is near a wide prior's b -- and the right extent 22 r delta (BB_LS_RIGHT above).  *nleft, *nright: intervals
// left and right of the mode, which is a node.
BB_DEV double bb_ls_grid(const LsCond& c, double dl, int* nleft, int* nright) {
    const double m = bb_ls_refine(dl);
    int r = 1;
    double e;
    while (r < BB_LS_RIGHT_MAX && log(bb_ls_p(c, (double)(BB_LS_RIGHT * r) * dl, &e)) > BB_GRID_TAIL) r *= 2;
    const int m4 = 4 * (int)m;
    *nleft = BB_LS_LEFT * m4;
    *nright = BB_LS_RIGHT * r * m4;
    return dl / (double)m4;
}

// The conditionals of one entry for bb_grid_mixture, shared by both blocks: row 0 of the block's table holds SS_j (the caller's
// pass, same lane), parameter `own` of the draws is the entry's own l_j.  Nothing but the sweeps' rows is kept: lo_j = l* - 10 delta
// and the coefficients are formed again from (l*, delta) in LDS and SS_j.
struct LsMix : GridRows {
    typedef LsCond Cond;
    static constexpr int NX = 1;          // sigma_mean
    static constexpr bool L_KEPT = false;
    const PpcArgs& P;
    long long own;
    double a, ib2;            // the entry's prior
    int nterms;
    const double* ss;

    BB_MEM LsMix(const PpcArgs& P_, long long own_, double a_, double ib2_, int nterms_, double* tab) : P(P_), own(own_), a(a_), ib2(ib2_), nterms(nterms_), ss(tab) {
        const long long ns = P.n_samples;
        l = tab + ns; E = tab + 2 * ns; V = tab + 3 * ns; x0 = tab + 4 * ns; hi = tab + 5 * ns;
        x1 = two = nullptr;
    }
    BB_MEM double setup(int j, LsCond& c, double* w, int* nleft, int* nright, bool*) const {
        c.a = a; c.ib2 = ib2; c.n = (double)nterms;
        const double dl = bb_ls_mode(c, ss[j]);
        *w = dl;
        return bb_ls_grid(c, dl, nleft, nright);
    }
    BB_MEM double p(const LsCond& c, double u, double* em1) const { return bb_ls_p(c, u, em1); }
    BB_MEM void extras(const LsCond&, double p, double u, double, double* se, double*) const { *se += p * exp(u); }
    BB_MEM double finish0(const LsCond& c, double z, double se) const { return exp(c.lm) * (se / z); }
    BB_MEM double finish1(const LsCond&, double, double x) const { return x; }
    BB_MEM double mode(const LsCond& c) const { return c.lm; }
    BB_MEM double latent(int j) const { return bb_ppc_param(P, own, j); }
    BB_MEM void keep(int, const LsCond&, double, double, int) const {}
    BB_MEM double lo(int, double lm, double dl) const { return lm - 10.0 * dl; }
    BB_MEM void reopen(int j, LsCond& c, double lm) const {
        const double SS = ss[j];
        c.a = a; c.ib2 = ib2; c.n = (double)nterms;
        c.lm = lm;
        c.W = SS == 0.0 ? 0.0 : SS * exp(-2.0 * lm);
        c.c1 = ib2 * (lm - a) + c.n;
    }
    // (the lower end as an offset, and the step, once more from delta: lo_j is not read here)
    BB_MEM double cdf_z(const LsCond& c, double dl, double, double x) const {
        const double mm = bb_ls_refine(dl);
        const double ulo = -10.0 * dl, r = x - (c.lm + ulo), s = dl / (4.0 * mm), ux = x - c.lm;
        return bb_grid_cdf_z(r, s, ulo, ux, [&](double u, double* em1) { return bb_ls_p(c, u, em1); },
                             [&](bool upper, double em1) { return bb_ls_dh(c, upper ? ux : ulo, em1); });
    }
};

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
            bb_grid_mixture(cx, ns, A.nq, A.probs, cx.lds, A.unit, A.n_units, ent, A.quant, LsMix(P, P.lo_ls + ent, a, ib2, nu, tab));
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
        bb_grid_mixture(cx, ns, A.nq, A.probs, cx.lds, A.unit, A.n_units, g, A.quant, LsMix(P, P.lo_lspop + g, a, ib2, (int)A.F.nn, tab));
    }
}
