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
//        draw's two coefficients (A, B) or (v, q) into the block's slice of a global table; then, draw j being lane j mod
//        BB_SCORE_NT's in every sweep, so that a lane reads only table entries it wrote:
//     A  per draw the modes, the grid, the moments: l*, s, Z into LDS; l, E, V, T, P, lo, hi, two into the table -> sum l, E, V
//     A' (no arithmetic on the grid)                                                            -> sum T, P, l*;  sum two, max hi_j
//     B  centred second moments                                         -> sum (l - q_mean)^2, sum (E - rb_mean)^2, max -lo_j
//     Q  bisection of the mixture CDF, BB_LT_ITER steps, up to three quantiles per sweep as bb_rb_mixture does; a draw whose
//        [lo_j, hi_j] does not hold the midpoint adds 0 or 1 and evaluates nothing.
// The maximum of hi_j takes NaN for a draw whose Z_j is not finite, so that the bracket is finite exactly when every l*_j, s_j and
// Z_j is.  Sums and maxima in bb_score_reduce's order; exp, expm1, log, log1p, sqrt, ceil are the platform's, as in bb_rb.h.
// Barrier-separated passes, so the host emulation (BB_EMU) runs the same source.
#pragma once
#include "bb_rb.h"

#define BB_LT_FULL 0                       // == BB_LOGTAU_FULL / BB_LOGTAU_COLLAPSED of include/barbay_hip.h
#define BB_LT_COLLAPSED 1
#define BB_LT_ITER 40                      // bisection steps of a quantile
#define BB_LT_TAIL (-40.0)                 // a mode is kept, and the grid ends, at exp(BB_LT_TAIL) of the global maximum
#define BB_LT_REACH 8                      // an end lies 8 r delta beyond its outer mode, r = 1, 2, 4 .. BB_LT_REACH_MAX
#define BB_LT_REACH_MAX 4096
#define BB_LT_REFINE_MAX 64                // the step is delta / (4 m), m = ceil(2 delta) up to this
#define BB_LT_NODES_MAX 8192               // intervals of a draw's grid; beyond it the step is widened by a whole factor
#define BB_LT_MODE_ITER 100                // steps of the safeguarded iteration of one segment
#define BB_LT_SEG_ITER 60                  // bisection steps of a zero of h_c''
#define BB_LT_SLACK 9.5367431640625e-07   // 2^-20, taken off a quotient before ceil: a whole number but for rounding does not tip over
#define BB_LT_OUT 8                        // per-entry results: q_mean, q_sd, rb_mean, rb_sd, tau_mean, pool_mean, mode_mean, n_two_modes
#define BB_LT_TAB 10                       // per-block global table [10][n_samples]: c0_j, c1_j, l_j, E_j, V_j, T_j, P_j, lo_j, hi_j, two_j
// LDS: l*[n_samples] | s[n_samples] | Z[n_samples] | three arrays of BB_SCORE_NT partials | scalars (bb_rb.h's st[] layout)
#define BB_LT_LDS_DOUBLES(ns) (3 * (long long)(ns) + 3 * BB_SCORE_NT + BB_RB_SCALARS)
// the largest n_samples whose layout fits the 160 KiB of LDS a workgroup can have
#define BB_LT_SAMPLES_CAP ((160 * 1024 / 8 - 3 * BB_SCORE_NT - BB_RB_SCALARS) / 3)
static_assert(BB_LT_LDS_DOUBLES(BB_LT_SAMPLES_CAP) * 8 <= 160 * 1024 && BB_LT_LDS_DOUBLES(BB_LT_SAMPLES_CAP + 1) * 8 > 160 * 1024,
              "BB_LT_SAMPLES_CAP is the largest count that fits");
static_assert(BB_LT_SAMPLES_CAP == 5781, "3 x 5781 doubles of (l*, s, Z) + 24 KiB of partials + 512 B of scalars <= 160 KiB");

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

// the root of h' in [lo, hi], on which h' falls, from x: Newton, a bisection step wherever Newton's leaves the bracket
template <int MODE>
BB_DEV double bb_lt_solve(const LtCond& c, double lo, double hi, double x) {
    for (int it = 0; it < BB_LT_MODE_ITER; ++it) {
        const double g = bb_lt_d1<MODE>(c, x);
        if (g == 0.0 || g != g) return x + g;      // (a NaN h': the mode is NaN)
        if (g > 0.0) lo = x;
        else hi = x;
        const double cv = bb_lt_d2<MODE>(c, x);
        double xn = x - g / cv;
        if (!(cv < 0.0 && xn >= lo && xn <= hi)) xn = lo + (hi - lo) / 2.0;
        const double step = xn - x;
        x = xn;
        if (fabs(step) <= 9.094947017729282e-13 * (1.0 + fabs(x))) break;      // 2^-40
    }
    const double g = bb_lt_d1<MODE>(c, x), cv = bb_lt_d2<MODE>(c, x), xn = x - g / cv;      // one more Newton step where it stays inside: the
    return cv < 0.0 && xn >= lo && xn <= hi ? xn : x;                             // iteration's last step bounds the error by 2^-40 only
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

// an interval count from a quotient: ceil(x - 2^-20) where 1 <= x <= 1e9, else 1 (a NaN included)
BB_DEV long long bb_lt_count(double x) {
    return (x >= 1.0 && x <= 1e9) ? (long long)ceil(x - BB_LT_SLACK) : 1;
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
        kept2 = fabs(d) <= -BB_LT_TAIL;
        left = kept2 ? m0 : glob;
        right = kept2 ? m1 : glob;
    }
    bb_lt_anchor<MODE>(c, glob);
    const double dl0 = 1.0 / sqrt(-bb_lt_d2<MODE>(c, left)), dl1 = kept2 ? 1.0 / sqrt(-bb_lt_d2<MODE>(c, right)) : dl0;
    const double dmin = !kept2 || !(dl1 < dl0) ? dl0 : dl1;
    double m = isfinite(dmin) ? ceil(2.0 * dmin - BB_LT_SLACK) : 1.0;
    m = m >= 1.0 ? (m <= (double)BB_LT_REFINE_MAX ? m : (double)BB_LT_REFINE_MAX) : 1.0;
    const double s = dmin / (4.0 * m);
    int r = 1;
    while (r < BB_LT_REACH_MAX && bb_lt_lnp<MODE>(c, (left - (double)(BB_LT_REACH * r) * dl0) - c.lm, &e) > BB_LT_TAIL) r *= 2;
    const double end0 = left - (double)(BB_LT_REACH * r) * dl0;
    r = 1;
    while (r < BB_LT_REACH_MAX && bb_lt_lnp<MODE>(c, (right + (double)(BB_LT_REACH * r) * dl1) - c.lm, &e) > BB_LT_TAIL) r *= 2;
    const double end1 = right + (double)(BB_LT_REACH * r) * dl1;
    const long long nl = bb_lt_count((c.lm - end0) / s), nr = bb_lt_count((end1 - c.lm) / s);
    const long long f = (nl + nr + BB_LT_NODES_MAX - 1) / BB_LT_NODES_MAX;
    *nleft = (int)((nl + f - 1) / f);
    *nright = (int)((nr + f - 1) / f);
    *two = kept2;
    return s * (double)f;
}

// draw j's CDF at x, times Z_j: the trapezoid on N + 1 equidistant nodes from lo_j to x less the first Euler-Maclaurin end term;
// lo_j < x < hi_j
template <int MODE>
BB_DEV double bb_lt_cdf_z(const LtCond& c, double s, double lo, double x) {
    const double r = x - lo, ulo = lo - c.lm;
    double N = ceil(r / s);
    N = N >= 1.0 ? N : 1.0;
    const double sx = r / N;
    const int n = (int)N;
    double e;
    const double ux = x - c.lm, p0 = exp(bb_lt_lnp<MODE>(c, ulo, &e)), p1 = exp(bb_lt_lnp<MODE>(c, ux, &e));
    double acc = 0.5 * p0;
    for (int i = 1; i < n; ++i) acc += exp(bb_lt_lnp<MODE>(c, ulo + (double)i * sx, &e));
    acc += 0.5 * p1;
    return sx * acc - sx * sx / 12.0 * (bb_lt_d1<MODE>(c, x) * p1 - bb_lt_d1<MODE>(c, lo) * p0);
}

BB_DEV void bb_lt_cond(LtCond& c, int nterms, double a, double ib2, double c0, double c1, double nw) {
    c.a = a; c.ib2 = ib2; c.prior = nterms == 0;
    c.c0 = c0; c.c1 = c1; c.nw = nw;
}

template <int MODE>
BB_DEV void bb_block_lt(BBCtx& cx, const LtArgs& L, int nblocks) {
    const RbArgs& A = L.A;
    const FreqArgs& F = A.F;
    const PpcArgs& P = F.P;
    const int ns = P.n_samples, E = P.E, nq = A.nq;
    const long long n_units = A.n_units;
    double* tab = A.ytab + (long long)cx.block * BB_LT_TAB * ns;
    double* ms = cx.lds;
    double* ssj = cx.lds + ns;
    double* zz = cx.lds + 2 * (long long)ns;
    double* red = cx.lds + 3 * (long long)ns;
    double* st = red + 3 * BB_SCORE_NT;
    double* c0j = tab;
    double* c1j = tab + ns;
    double* lj = tab + 2 * (long long)ns;
    double* ej = tab + 3 * (long long)ns;
    double* vj = tab + 4 * (long long)ns;
    double* tj = tab + 5 * (long long)ns;
    double* pj = tab + 6 * (long long)ns;
    double* loj = tab + 7 * (long long)ns;
    double* hij = tab + 8 * (long long)ns;
    double* twoj = tab + 9 * (long long)ns;
    const bool menv = P.kind == 4;
    const double a = P.pri_mean, ib2 = P.pri_ivar;
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
            // sweep A: modes, grid and per-draw moments; first sums
            BB_PASS(cx, tid) {
                double a0 = 0.0, a1 = 0.0, a2 = 0.0;
                for (int j = tid; j < ns; j += BB_SCORE_NT) {
                    LtCond c;
                    bb_lt_cond(c, nu, a, ib2, c0j[j], c1j[j], nu > 0 ? pj[j] : 0.0);
                    int nleft = 0, nright = 0;
                    bool two = false;
                    const double s = bb_lt_setup<MODE>(c, &nleft, &nright, &two);
                    const int nodes = nleft + nright;
                    double z = 0.0, m1 = 0.0, m2 = 0.0, se = 0.0, sp = 0.0;
                    for (int k = 0; k <= nodes; ++k) {
                        const double uk = (double)(k - nleft) * s;
                        double e2;
                        double p = exp(bb_lt_lnp<MODE>(c, uk, &e2));
                        if (k == 0 || k == nodes) p *= 0.5;
                        z += p;
                        m1 += p * uk;
                        m2 += p * (uk * uk);
                        se += p * exp(uk);
                        sp += p * (c.prior ? 1.0 : 1.0 / (1.0 + c.nws * e2));
                    }
                    const double Zj = s * z, r1 = m1 / z, Ej = c.lm + r1, Vj = m2 / z - r1 * r1, Tj = exp(c.lm) * (se / z), Pj = sp / z;
                    const double l = bb_ppc_param(P, P.lo_lt + ent, j);
                    ms[j] = c.lm; ssj[j] = s; zz[j] = Zj;
                    lj[j] = l; ej[j] = Ej; vj[j] = Vj; tj[j] = Tj; pj[j] = Pj;
                    loj[j] = c.lm - (double)nleft * s; hij[j] = c.lm + (double)nright * s; twoj[j] = two ? 1.0 : 0.0;
                    a0 += l;
                    a1 += Ej;
                    a2 += Vj;
                }
                red[tid] = a0; red[BB_SCORE_NT + tid] = a1; red[2 * BB_SCORE_NT + tid] = a2;
            }
            BB_SYNC(cx);
            bb_score_reduce(cx, red, st, false);
            // sweep A': the other first sums
            BB_PASS(cx, tid) {
                double a0 = 0.0, a1 = 0.0, a2 = 0.0;
                for (int j = tid; j < ns; j += BB_SCORE_NT) {
                    a0 += tj[j];
                    a1 += pj[j];
                    a2 += ms[j];
                }
                red[tid] = a0; red[BB_SCORE_NT + tid] = a1; red[2 * BB_SCORE_NT + tid] = a2;
            }
            BB_SYNC(cx);
            bb_score_reduce(cx, red, st + 3, false);
            // sweep A'': the draws with two modes; the largest hi_j (NaN where Z_j is not finite)
            BB_PASS(cx, tid) {
                double a0 = 0.0, mx = -INFINITY;
                for (int j = tid; j < ns; j += BB_SCORE_NT) {
                    a0 += twoj[j];
                    mx = bb_score_max(mx, isfinite(zz[j]) ? hij[j] : (double)NAN);
                }
                red[tid] = a0; red[BB_SCORE_NT + tid] = 0.0; red[2 * BB_SCORE_NT + tid] = mx;
            }
            BB_SYNC(cx);
            bb_score_reduce(cx, red, st + 6, true);
            // sweep B: centred second moments; the smallest lo_j (as the largest of -lo_j)
            BB_PASS(cx, tid) {
                const double qm = st[0] / ns, rm = st[1] / ns;
                double a0 = 0.0, a1 = 0.0, mx = -INFINITY;
                for (int j = tid; j < ns; j += BB_SCORE_NT) {
                    const double d0 = lj[j] - qm, d1 = ej[j] - rm;
                    a0 += d0 * d0;
                    a1 += d1 * d1;
                    mx = bb_score_max(mx, -loj[j]);
                }
                red[tid] = a0; red[BB_SCORE_NT + tid] = a1; red[2 * BB_SCORE_NT + tid] = mx;
            }
            BB_SYNC(cx);
            bb_score_reduce(cx, red, st + 9, true);
            BB_PASS(cx, tid) {
                if (tid == 0) {
                    A.unit[0 * n_units + ent] = st[0] / ns;
                    A.unit[1 * n_units + ent] = sqrt(st[9] / ns);
                    A.unit[2 * n_units + ent] = st[1] / ns;
                    A.unit[3 * n_units + ent] = sqrt(st[2] / ns + st[10] / ns);
                    A.unit[4 * n_units + ent] = st[3] / ns;
                    A.unit[5 * n_units + ent] = st[4] / ns;
                    A.unit[6 * n_units + ent] = st[5] / ns;
                    A.unit[7 * n_units + ent] = st[6];
                    const double lo = -st[11], hi = st[8];
                    st[15] = (nq > 0 && isfinite(lo) && isfinite(hi)) ? 1.0 : 0.0;
                    for (int i = 0; i < nq; ++i) { st[16 + i] = lo; st[24 + i] = hi; }
                }
            }
            BB_SYNC(cx);
            if (nq > 0 && st[15] == 0.0) {   // a non-finite l*_j, s_j or Z_j: no bracket
                BB_PASS(cx, tid) { if (tid < nq) A.quant[ent * BB_RB_MAX_Q + tid] = NAN; }
            } else if (nq > 0) {
                for (int it = 0; it < BB_LT_ITER; ++it) {
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
                                LtCond c;
                                const double lo = loj[j], hi = hij[j];
                                bool have = false;
#pragma unroll
                                for (int i = 0; i < 3; ++i) {
                                    if (i >= nx) continue;
                                    const double x = xs[i];
                                    if (x <= lo) continue;                       // C_j = 0
                                    if (x >= hi) { acc[i] += 1.0; continue; }    // C_j = 1
                                    if (!have) {
                                        bb_lt_cond(c, nu, a, ib2, c0j[j], c1j[j], 0.0);      // (n w: the pooling factor's alone)
                                        bb_lt_anchor<MODE>(c, ms[j]);
                                        have = true;
                                    }
                                    const double C = bb_lt_cdf_z<MODE>(c, ssj[j], lo, x) / zz[j];
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
                                if (st[12 + tid] / ns < A.probs[i]) st[16 + i] = x;
                                else st[24 + i] = x;
                            }
                        }
                        BB_SYNC(cx);
                    }
                }
                BB_PASS(cx, tid) { if (tid < nq) A.quant[ent * BB_RB_MAX_Q + tid] = st[16 + tid] + (st[24 + tid] - st[16 + tid]) / 2.0; }
            }
            BB_SYNC(cx);
        }
    }
}
