// bb_ltrb.h -- Rao-Blackwellised marginals of the deviation scales logtau of the hierarchical kinds on the device.  Entry point
// bb_logtau_rb (include/barbay_hip.h, where the rule is defined); no reference counterpart.
//
// Non-centred, s_u = theta_g(u) + e^{logtau_u} theta_tilde_u: given everything else l = logtau_u enters the log-joint through its
// Gaussian prior N(a, b) and the unit's n Gaussian terms, whose mean reads e^l theta_tilde_u (BB_LOGTAU_FULL):
//   h(l) = -(l - a)^2 ib2 / 2 - A e^{2l} + B e^l,   A = n w tt^2 / 2,  B = w tt Y,  Y = y - n theta;
// with theta_tilde_u integrated out against its N(0, 1) prior (BB_LOGTAU_COLLAPSED):
//   h_c(l) = -(l - a)^2 ib2 / 2 - ln V / 2 - q / (2V),   V = e^{2l} + v,  v = 1 / (n w),  q = (Y / n)^2.
// Neither is log-concave; either has at most two modes.  Per draw j of everything else (bb_rb.h's draws: same keying, or the caller's
// rows) the modes are found from the segments on which h' is monotone (bb_lt_modes), one trapezoid grid is laid over the kept ones
// (bb_lt_setup) and the conditional is integrated on it; the per-draw moments are averaged over j, the quantiles are those of the
// mixture of the per-draw CDFs, by bisection.
//
// Phases of a call (bb_analysis.h): bb_rb.h's front as it stands -- bb_block_ppc_pop, bb_block_freq_zpart / _zsum, bb_block_rb_logz --
// then
//   bb_block_lt : one workgroup of BB_SCORE_NT threads per mutant row (r, m), row += nblocks.  Per environment e (entry = the unit's
//        place in the caller's logtau block) one walk over the row's loglambda draws, y in a register (no accumulator is indexed by a
//        run-time environment: that would be scratch memory): y_j += gamma_t + sbar_t for the steps of e, ascending t, from 0.0; the
//        draw's two coefficients (A, B) or (v, q) into the block's slice of a global table; then bb_grid_mixture (bb_gridmix.h: the
//        sweeps, the NaN rule, the quantiles) over LtMix<MODE>, whose two extras are tau and the pooling factor.
// exp, expm1, log, log1p, sqrt, ceil are the platform's, as in bb_rb.h.
#pragma once
#include "bb_gridmix.h"

#define BB_LT_FULL 0                       // == BB_LOGTAU_FULL / BB_LOGTAU_COLLAPSED of include/barbay_hip.h
#define BB_LT_COLLAPSED 1
#define BB_LT_SEG_ITER 60                  // bisection steps of a zero of h_c''
#define BB_LT_OUT 8                        // per-entry results: q_mean, q_sd, rb_mean, rb_sd, tau_mean, pool_mean, mode_mean, n_two_modes
#define BB_LT_TAB 10                       // per-block global table [10][n_samples]: c0_j, c1_j, l_j, E_j, V_j, T_j, P_j, lo_j, hi_j, two_j

struct LtArgs {
    RbArgs A;                 // as for bb_block_rb: F, probs, nq, n_z; unit [BB_LT_OUT][n_entries]; quant [n_entries][8]; n_steps [n_entries]:
                              // n_terms; n_units = n_entries; ytab [gridDim][BB_LT_TAB][n_samples]; A.F.P.pri_mean / pri_ivar: logtau's prior
    int mode;                 // BB_LT_FULL or BB_LT_COLLAPSED (the host picks the kernel instance by it)
};

// the conditional of one draw about its anchor l* (the global mode): everything the grid and the CDF read.  The mode of the call
// (FULL / COLLAPSED) is a template parameter of everything below: one kernel instance each, no mode branch in a node
struct LtCond {
    double a, ib2;            // the prior (mean, 1 / std^2)
    double c0, c1;            // FULL: A, B;  COLLAPSED: v, q
    double nw;                // n w
    bool prior;               // n == 0: no term, the coefficients are not read
    double lm, g1, nws;       // l*, g1 = ib2 (l* - a), nws = n w e^{2 l*}
    double k0, k1;            // FULL: A2 = A e^{2 l*}, D1 = B e^{l*} - 2 A2;  COLLAPSED: rho = s* / V*, kap = q / (2 V*)
};

// COLLAPSED: d/dl of (V - v)(q - V) / V^2 as a function of s = e^{2l}: 2 s (c v - s k) / V^3, c = q - v, k = q + v
BB_DEV double bb_lt_G(const LtCond& c, double s) {
    const double V = s + c.c0;
    return 2.0 * (s / V) * (((c.c1 - c.c0) * c.c0 - s * (c.c1 + c.c0)) / V) / V;
}
// h'(l)
template <int MODE>
BB_DEV double bb_lt_d1(const LtCond& c, double l) {
    const double g = -(l - c.a) * c.ib2;
    if (c.prior) return g;
    if (MODE == BB_LT_FULL) {
        const double x = exp(l);
        return g + x * (c.c1 - 2.0 * c.c0 * x);
    }
    const double s = exp(2.0 * l), V = s + c.c0;
    return g + (s / V) * ((c.c1 - V) / V);
}
// h''(l)
template <int MODE>
BB_DEV double bb_lt_d2(const LtCond& c, double l) {
    if (c.prior) return -c.ib2;
    if (MODE == BB_LT_FULL) {
        const double x = exp(l);
        return -c.ib2 + x * (c.c1 - 4.0 * c.c0 * x);
    }
    return -c.ib2 + bb_lt_G(c, exp(2.0 * l));
}

// the root of h' in [lo, hi], on which h' falls, from x
template <int MODE>
BB_DEV double bb_lt_solve(const LtCond& c, double lo, double hi, double x) {
    return bb_grid_solve(lo, hi, x, [&](double l) { return bb_lt_d1<MODE>(c, l); }, [&](double l) { return bb_lt_d2<MODE>(c, l); });
}

// the local maxima of h, ascending: one or two (the header's segments); returns their number
template <int MODE>
BB_DEV int bb_lt_modes(const LtCond& c, double* m0, double* m1) {
    const double a = c.a, ib2 = c.ib2;
    if (c.prior) { *m0 = a; return 1; }
    double L, U, l1 = 0.0, l2 = 0.0;
    bool split = false;
    if (MODE == BB_LT_FULL) {
        const double A = c.c0, B = c.c1;
        if (B > 0.0) {
            const double t = log(B / (2.0 * A));
            L = t < a ? t : a;
            U = t < a ? a : t;
            const double disc = B * B - 16.0 * A * ib2;
            if (disc > 0.0) {
                const double r = sqrt(disc);
                l1 = log(2.0 * ib2 / (B + r));
                l2 = log((B + r) / (8.0 * A));
                split = true;
            }
        } else {
            const double ea = exp(a);
            L = a - ea * (2.0 * A * ea - B) / ib2;
            U = a;
        }
    } else {
        const double v = c.c0, q = c.c1, cc = q - v, k = q + v;
        L = a - 1.0 / ib2;
        U = a;
        if (cc > 0.0) {
            const double t = log(cc) / 2.0;
            U = t > a ? t : a;
            const double sp = v * cc / ((cc + k) + sqrt(cc * cc + cc * k + k * k));
            if (bb_lt_G(c, sp) > ib2) {
                double lo = ib2 * v * v / (2.0 * cc), hi = sp;
                for (int it = 0; it < BB_LT_SEG_ITER; ++it) {
                    const double mid = sqrt(lo * hi);
                    if (bb_lt_G(c, mid) < ib2) lo = mid;
                    else hi = mid;
                }
                l1 = log(sqrt(lo * hi)) / 2.0;
                lo = sp;
                hi = cc * v / k;
                for (int it = 0; it < BB_LT_SEG_ITER; ++it) {
                    const double mid = sqrt(lo * hi);
                    if (bb_lt_G(c, mid) > ib2) lo = mid;
                    else hi = mid;
                }
                l2 = log(sqrt(lo * hi)) / 2.0;
                split = true;
            }
        }
    }
    int nm = 0;
    if (split) {
        if (bb_lt_d1<MODE>(c, l1) < 0.0) { *m0 = bb_lt_solve<MODE>(c, L, l1, L); nm = 1; }
        if (bb_lt_d1<MODE>(c, l2) > 0.0) { *(nm ? m1 : m0) = bb_lt_solve<MODE>(c, l2, U, U); ++nm; }
    }
    if (nm == 0) { *m0 = bb_lt_solve<MODE>(c, L, U, U); nm = 1; }
    return nm;
}

// the anchor and what the density about it reads
template <int MODE>
BB_DEV void bb_lt_anchor(LtCond& c, double lm) {
    c.lm = lm;
    c.g1 = c.ib2 * (lm - c.a);
    c.nws = 0.0; c.k0 = 0.0; c.k1 = 0.0;
    if (c.prior) return;
    const double s = exp(2.0 * lm);
    c.nws = c.nw * s;
    if (MODE == BB_LT_FULL) {
        const double x = exp(lm);
        c.k0 = c.c0 * (x * x);
        c.k1 = c.c1 * x - 2.0 * c.k0;
    } else {
        const double V = s + c.c0;
        c.k0 = s / V;
        c.k1 = c.c1 / (2.0 * V);
    }
}

// ln p(u) = h(l* + u) - h(l*), in the form without cancelling large terms; *e2 = e^{2u}
//   FULL       -u g1 - ib2 u^2 / 2 + e1 (D1 - A2 e1),                        e1 = expm1(u)
//   COLLAPSED  -u g1 - ib2 u^2 / 2 - log1p(y) / 2 + kap y / (1 + y),         y = rho expm1(2u)
template <int MODE>
BB_DEV double bb_lt_lnp(const LtCond& c, double u, double* e2) {
    double g = -(u * c.g1) - c.ib2 * (u * u) / 2.0;
    if (c.prior) { *e2 = 1.0; return g; }
    if (MODE == BB_LT_FULL) {
        const double e1 = expm1(u);
        *e2 = (e1 + 1.0) * (e1 + 1.0);
        return g + e1 * (c.k1 - c.k0 * e1);
    }
    const double E2 = expm1(2.0 * u), y = c.k0 * E2;
    *e2 = E2 + 1.0;
    g = g - log1p(y) / 2.0 + c.k1 * (y / (1.0 + y));
    return g;
}

// The modes, the anchor and the grid of one draw: returns the step s; *nleft, *nright: intervals left and right of the global mode,
// which is a node; *two: two modes kept.
template <int MODE>
BB_DEV double bb_lt_setup(LtCond& c, int* nleft, int* nright, bool* two) {
    double m0 = 0.0, m1 = 0.0, e;
    const int nm = bb_lt_modes<MODE>(c, &m0, &m1);
    double left = m0, right = m0, glob = m0;
    bool kept2 = false;
    if (nm == 2) {
        bb_lt_anchor<MODE>(c, m0);
        const double d = bb_lt_lnp<MODE>(c, m1 - m0, &e);
        glob = d > 0.0 ? m1 : m0;
        kept2 = fabs(d) <= -BB_GRID_TAIL;
        left = kept2 ? m0 : glob;
        right = kept2 ? m1 : glob;
    }
    bb_lt_anchor<MODE>(c, glob);
    const double dl0 = 1.0 / sqrt(-bb_lt_d2<MODE>(c, left)), dl1 = kept2 ? 1.0 / sqrt(-bb_lt_d2<MODE>(c, right)) : dl0;
    const double dmin = !kept2 || !(dl1 < dl0) ? dl0 : dl1;
    *two = kept2;
    // (left, right and the ends in absolute coordinates, the anchor subtracted last)
    return bb_grid_layout(left, right, dl0, dl1, dmin, c.lm, nleft, nright, [&](double u) { return bb_lt_lnp<MODE>(c, u, &e); });
}

// The conditionals of one entry for bb_grid_mixture: rows 0 and 1 of the block's table hold the draws' coefficients, row 6 (P_j's)
// n w until sweep A has read it, same lane (pass Y of bb_block_lt); parameter `own` of the draws is the entry's own l_j.
template <int MODE>
struct LtMix : GridRows {
    typedef LtCond Cond;
    static constexpr int NX = 2;          // tau_mean, pool_mean; n_two_modes
    static constexpr bool L_KEPT = false;
    const PpcArgs& P;
    long long own;
    double a, ib2;            // logtau's prior
    int nterms;
    const double *c0j, *c1j;
    double* loj;

    BB_MEM LtMix(const PpcArgs& P_, long long own_, double a_, double ib2_, int nterms_, double* tab) : P(P_), own(own_), a(a_), ib2(ib2_), nterms(nterms_) {
        const long long ns = P.n_samples;
        c0j = tab; c1j = tab + ns;
        l = tab + 2 * ns; E = tab + 3 * ns; V = tab + 4 * ns; x0 = tab + 5 * ns; x1 = tab + 6 * ns;
        loj = tab + 7 * ns; hi = tab + 8 * ns; two = tab + 9 * ns;
    }
    BB_MEM void cond(LtCond& c, int j, double nw) const {
        c.a = a; c.ib2 = ib2; c.prior = nterms == 0;
        c.c0 = c0j[j]; c.c1 = c1j[j]; c.nw = nw;
    }
    BB_MEM double setup(int j, LtCond& c, double* w, int* nleft, int* nright, bool* kept2) const {
        cond(c, j, nterms > 0 ? x1[j] : 0.0);
        const double s = bb_lt_setup<MODE>(c, nleft, nright, kept2);
        *w = s;
        return s;
    }
    BB_MEM double p(const LtCond& c, double u, double* e2) const { return exp(bb_lt_lnp<MODE>(c, u, e2)); }
    BB_MEM void extras(const LtCond& c, double p, double u, double e2, double* se, double* sp) const {
        *se += p * exp(u);
        *sp += p * (c.prior ? 1.0 : 1.0 / (1.0 + c.nws * e2));
    }
    BB_MEM double finish0(const LtCond& c, double z, double se) const { return exp(c.lm) * (se / z); }
    BB_MEM double finish1(const LtCond&, double z, double sp) const { return sp / z; }
    BB_MEM double mode(const LtCond& c) const { return c.lm; }
    BB_MEM double latent(int j) const { return bb_ppc_param(P, own, j); }
    BB_MEM void keep(int j, const LtCond&, double lm, double s, int nleft) const { loj[j] = lm - (double)nleft * s; }
    BB_MEM double lo(int j, double, double) const { return loj[j]; }
    BB_MEM void reopen(int j, LtCond& c, double lm) const {
        cond(c, j, 0.0);      // (n w: the pooling factor's alone)
        bb_lt_anchor<MODE>(c, lm);
    }
    // (h' takes the absolute point)
    BB_MEM double cdf_z(const LtCond& c, double s, double lo, double x) const {
        return bb_grid_cdf_z(x - lo, s, lo - c.lm, x - c.lm, [&](double u, double* e2) { return exp(bb_lt_lnp<MODE>(c, u, e2)); },
                             [&](bool upper, double) { return bb_lt_d1<MODE>(c, upper ? x : lo); });
    }
};

template <int MODE>
BB_DEV void bb_block_lt(BBCtx& cx, const LtArgs& L, int nblocks) {
    const RbArgs& A = L.A;
    const FreqArgs& F = A.F;
    const PpcArgs& P = F.P;
    const int ns = P.n_samples, E = P.E;
    double* tab = A.ytab + (long long)cx.block * BB_LT_TAB * ns;
    double* c0j = tab;
    double* c1j = tab + ns;
    double* pj = tab + 6 * (long long)ns;
    const bool menv = P.kind == 4;
    for (long long row = cx.block; row < P.n_rows; row += nblocks) {
        const int r = (int)(row / P.nb);
        const long long m = row % P.nb;
        const int T = P.T[r];
        const long long ll = F.off_l[r] + (F.nn + m) * T;
        const double* Z = F.Z + (long long)P.tcum[r] * ns;      // ln Z (bb_block_rb_logz)
        const double* sbar = P.pop + (long long)(2 * P.off_t[r]) * ns;
        for (int e = 0; e < E; ++e) {
            const long long em = e + (long long)E * m, u = em + (long long)E * P.nb * r;
            const long long th = P.kind == 2 ? P.geno_idx[m] : em, ent = P.kind == 2 ? m : u;
            int nu = 0;
            for (int t = 0; t + 1 < T; ++t) nu += !menv || P.env_idx[P.tcum[r] + t + 1] == e;
            // pass Y: the unit's y_j in one walk over the row's loglambda draws; the draw's two coefficients
            BB_PASS(cx, tid) {
                if (tid == 0) A.n_steps[ent] = nu;
                for (int j = tid; j < ns; j += BB_SCORE_NT) {
                    double c0 = 0.0, c1 = 0.0;
                    if (nu > 0) {                // (a unit without a term reads neither its logsigma nor anything else)
                        double y = 0.0, l0 = bb_ppc_param(P, ll, j), z0 = Z[j];
                        for (int t = 0; t + 1 < T; ++t) {
                            const double l1 = bb_ppc_param(P, ll + t + 1, j), z1 = Z[(long long)(t + 1) * ns + j];
                            if (!menv || P.env_idx[P.tcum[r] + t + 1] == e) y += ((l1 - l0) - (z1 - z0)) + sbar[(long long)(2 * t) * ns + j];
                            l0 = l1;
                            z0 = z1;
                        }
                        const double w = exp(-2.0 * bb_ppc_param(P, P.lo_ls + ent, j)), Y = y - (double)nu * bb_ppc_param(P, P.lo_s + th, j);
                        if (MODE == BB_LT_FULL) {
                            const double tt = bb_ppc_param(P, P.lo_tt + ent, j);
                            c0 = 0.5 * ((double)nu * w) * (tt * tt);
                            c1 = (w * tt) * Y;
                        } else {
                            c0 = 1.0 / ((double)nu * w);
                            c1 = (Y / (double)nu) * (Y / (double)nu);
                        }
                        pj[j] = (double)nu * w;      // (n w: sweep A reads it back, same lane, before it stores P_j here)
                    }
                    c0j[j] = c0;
                    c1j[j] = c1;
                }
            }
            bb_grid_mixture(cx, ns, A.nq, A.probs, cx.lds, A.unit, A.n_units, ent, A.quant, LtMix<MODE>(P, P.lo_lt + ent, P.pri_mean, P.pri_ivar, nu, tab));
        }
    }
}
