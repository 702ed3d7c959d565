// bb_llrb.h -- Rao-Blackwellised marginals of the log-rates loglambda on the device.  Entry point bb_loglambda_rb
// (include/barbay_hip.h, where the conditional and the rule are defined); no reference counterpart.
//
// Given everything else, x = ll_{r,t,b} enters the log-joint through its Gaussian prior, its own Poisson term R x - e^x, and the
// ratio terms of the one or two steps its time point bounds: its own barcode's directly, every other barcode's of the time point
// through the row normaliser.  About a base point x (the draw x0, later a mode), with xi the offset from it and
//   delta(xi) = log1p(f0 expm1(xi)) = ln Z_t(x + xi) - ln Z_t(x),   f0 = e^x / Z_t,   f(xi) = delta'(xi) = f0 e^xi / (1 + f0 expm1(xi)),
// the two sides fold into five coefficients (a missing side adds exact zeros):
//   As = A_t + A_{t-1},  Bs = B_t - B_{t-1},  ws = w_{b,t} + w_{b,t-1},  wr = w_{b,t} rho_{b,t} - w_{b,t-1} rho_{b,t-1}
//   g(xi) = h(x + xi) - h(x) = -ib2 xi (xi + 2 (x - a)) / 2 + R xi - e^x expm1(xi) - Bs delta - As delta^2 / 2 - ws xi^2 / 2 + xi wr + ws xi delta
// and moving the base to x + u keeps the form: f0 <- f(u), Bs <- Bs + As delta(u) - ws u, wr <- wr + ws (delta(u) - u) (bb_ll_anchor).
// g is not log-concave in general: the modes are sought by a scan of g' over a bracket that provably holds every zero of it
// (bb_ll_bracket), each refined by a safeguarded Newton iteration; one trapezoid grid per draw is laid over the kept ones
// (bb_ll_setup), as bb_ltrb.h does for logtau.
//
// Phases of a call (bb_analysis.h): bb_rb.h's front as it stands -- bb_block_ppc_pop (sbar_{g,j}), bb_block_freq_zpart / _zsum,
// bb_block_rb_logz (ln Z in place) -- then
//   bb_block_ll_part : one workgroup of BB_SCORE_NT threads per (step g = (r, k), chunk of BB_FREQ_CHUNK consecutive data columns),
//        work += nblocks.  Per draw the chunk's (A, B) = (sum w_i, sum w_i rho_i) from 0.0 in index order (bb_ll_wrho: the weight and
//        the residual of one barcode at one step, as bb_block_pop_part forms them, the ragged method's pairing inverted in place),
//        into part[work][2][n_samples].
//   bb_block_ll_sum  : per (step, draw) the chunk partials from 0.0 in chunk order (bb_rb_chunk_sum) into ab[nt1][2][n_samples].
//   bb_block_ll      : one workgroup per requested row (r, b), x += nblocks, walking its T_r time points; entry = x n_cols + t.
//     C  per draw the base point's coefficients (x0, f0, As, Bs, ws, wr) into the block's slice of a global table; then
//        bb_grid_mixture (bb_gridmix.h: the sweeps, the NaN rule, the quantiles) over LlMix, whose extra is lambda.
// exp, expm1, log, log1p, sqrt, ceil are the platform's, as in bb_rb.h.
#pragma once
#include "bb_gridmix.h"

#define BB_LL_SCAN_MIN 16                  // cells of the mode scan: ceil(8 width) within these, so a cell is 1/8 wide or narrower
#define BB_LL_SCAN_MAX 1024                //   on a bracket up to 128 wide
#define BB_LL_PAD 0.125                    // added to either end of the bracket
#define BB_LL_LOW_ITER 30                  // bisection steps of the bracket's lower end
#define BB_LL_TAB 11                       // per-block global table [11][n_samples]: As, ws, Bs, wr, f0, x0, E, V, Lam, lo, hi

struct LlArgs {
    RbArgs A;                 // as for bb_block_rb: F, probs, nq, n_z; unit [BB_RB_OUT][n_entries]: q_mean, q_sd, rb_mean, rb_sd, lambda_mean,
                              // mode_mean; quant [n_entries][8]; n_units = n_entries = n_req n_cols; ytab [gridDim][BB_LL_TAB][n_samples]
    const long long* rows;    // [n_req] the requested bb_freq_bands rows, ascending; nullptr: row x = x
    const double* ent;        // [3][n_entries]: the entry's prior mean a, 1 / std^2, its count R (cells t >= T_r: not read)
    double* part;             // [(g1 - g0) nchunks][2][n_samples] chunk partials (A, B) of the steps in flight
    double* ab;               // [nt1][2][n_samples] the tables A_k, B_k, step g = off_t[r] + k
    long long n_req, g0, g1;  // rows asked for; the steps in flight
    int n_cols, quirk;        // columns of the result (max_r T_r); 1: the ragged method's pairing of the neutral terms
};

// the conditional of one draw about a base point x: everything the mode search, the grid and the CDF read
struct LlCond {
    double a, ib2, R;         // the prior (mean, 1 / std^2), the count
    double As, ws;            // both sides' sum of weights, the barcode's own
    double x, ex, f0, Bs, wr; // the base point, e^x, its frequency, and the two coefficients that move with it
};

// delta(u), f(u), expm1(u)
BB_DEV void bb_ll_df(const LlCond& c, double u, double* em, double* dl, double* f) {
    const double e = expm1(u), y = c.f0 * e;
    *em = e;
    *dl = log1p(y);
    *f = c.f0 * (e + 1.0) / (1.0 + y);
}
// g(u) = h(x + u) - h(x), in the form without cancelling large terms
BB_DEV double bb_ll_lnp(const LlCond& c, double u, double* em) {
    double dl, f;
    bb_ll_df(c, u, em, &dl, &f);
    return -(0.5 * c.ib2) * (u * (u + 2.0 * (c.x - c.a))) + c.R * u - c.ex * *em - c.Bs * dl - (0.5 * c.As) * (dl * dl) - (0.5 * c.ws) * (u * u) +
           u * c.wr + c.ws * (u * dl);
}
// g'(u) and g''(u)
BB_DEV void bb_ll_d12(const LlCond& c, double u, double* g, double* cv) {
    double em, dl, f;
    bb_ll_df(c, u, &em, &dl, &f);
    const double ff = f * (1.0 - f), eu = c.ex * (em + 1.0);
    *g = -c.ib2 * (u + (c.x - c.a)) + c.R - eu - (c.Bs + c.As * dl) * f - c.ws * u + c.wr + c.ws * (dl + u * f);
    *cv = -c.ib2 - eu - c.Bs * ff - c.As * (f * f + dl * ff) - c.ws + c.ws * (2.0 * f + u * ff);
}
BB_DEV double bb_ll_d1(const LlCond& c, double u) {
    double g, cv;
    bb_ll_d12(c, u, &g, &cv);
    return g;
}

// the base point moved to x + u
BB_DEV void bb_ll_anchor(LlCond& c, double u) {
    double em, dl, f;
    bb_ll_df(c, u, &em, &dl, &f);
    c.Bs = c.Bs + c.As * dl - c.ws * u;
    c.wr = c.wr + c.ws * (dl - u);
    c.f0 = f;
    c.x = c.x + u;
    c.ex = exp(c.x);
}

// CL(L) / sl - L of bb_ll_bracket: not negative exactly where L <= 0 is certified as a lower end
BB_DEV double bb_ll_low(const LlCond& c, double L, double C0, double Bp, double sl) {
    const double e = expm1(L);
    return (C0 - c.ex * (e + 1.0) - Bp * (c.f0 * (e + 1.0) / (1.0 + c.f0 * e))) / sl - L;
}
// [*lo, *hi] holds every zero of g': below lo g' > 0, above hi g' < 0 (the header's bounds), BB_LL_PAD added
BB_DEV void bb_ll_bracket(const LlCond& c, double* lo, double* hi) {
    const double d0 = c.x - c.a, Bp = c.Bs > 0.0 ? c.Bs : 0.0, Bm = c.Bs < 0.0 ? -c.Bs : 0.0;
    const double C0 = -c.ib2 * d0 + c.R + c.wr + c.ws * log1p(-c.f0), sl = c.ib2 + c.ws * (1.0 - c.f0);
    double l = bb_ll_low(c, 0.0, C0, Bp, sl), h = 0.0;
    if (l < 0.0) {                                  // (l is certified; 0 is not: the largest certified end between them, to 2^-30 of l)
        double up = 0.0;
        for (int it = 0; it < BB_LL_LOW_ITER; ++it) {
            const double mid = l + (up - l) / 2.0;
            if (bb_ll_low(c, mid, C0, Bp, sl) >= 0.0) l = mid;
            else up = mid;
        }
    } else if (l == l) l = 0.0;
    const double K = c.R + Bm + c.wr - c.ib2 * d0;
    if (K > 0.0) {
        const double h1 = K / c.ib2, h2 = log(K / c.ex);
        h = h1 < h2 ? h1 : h2;
        h = h > 0.0 ? h : 0.0;
    } else if (K != K) h = K;
    *lo = l - BB_LL_PAD;
    *hi = h + BB_LL_PAD;
}

// a local maximum of g in [lo, hi], g'(lo) > 0 >= g'(hi), from x
BB_DEV double bb_ll_solve(const LlCond& c, double lo, double hi, double x) {
    double g, cv;                                   // (g' and g'' come together)
    return bb_grid_solve(lo, hi, x, [&](double u) { bb_ll_d12(c, u, &g, &cv); return g; }, [&](double) { return cv; });
}

// The modes, the anchor and the grid of one draw; c comes in about the draw x0 and leaves about the global mode x*.  Returns the
// step s; *nleft, *nright: intervals left and right of the global mode, which is a node.
BB_DEV double bb_ll_setup(LlCond& c, int* nleft, int* nright) {
    double blo, bhi, e;
    bb_ll_bracket(c, &blo, &bhi);
    const double width = bhi - blo;
    int nc = BB_LL_SCAN_MIN;
    if (width * 8.0 > (double)BB_LL_SCAN_MIN) nc = width * 8.0 < (double)BB_LL_SCAN_MAX ? (int)ceil(width * 8.0) : BB_LL_SCAN_MAX;
    const double cw = width / (double)nc;
    // first scan: the highest mode
    double best = 0.0, gbest = -INFINITY, g0 = bb_ll_d1(c, blo);
    bool any = false;
    if (!(width == width) || !(g0 == g0)) { best = width + g0; any = true; nc = 0; }      // (a NaN bracket or g': the mode is NaN)
    const double gfirst = g0;
    for (int i = 0; i < nc; ++i) {
        const double e0 = blo + (double)i * cw, e1 = i + 1 < nc ? blo + (double)(i + 1) * cw : bhi, g1 = bb_ll_d1(c, e1);
        if (g0 > 0.0 && !(g1 > 0.0)) {
            const double m = bb_ll_solve(c, e0, e1, e0 + (e1 - e0) / 2.0), v = bb_ll_lnp(c, m, &e);
            if (!any || v > gbest || v != v) { best = m; gbest = v; }
            any = true;
        }
        g0 = g1;
    }
    if (!any) { best = gfirst > 0.0 ? bhi : blo; gbest = bb_ll_lnp(c, best, &e); }      // (no sign change: rounding at an end of the bracket)
    // second scan: the modes within exp(BB_GRID_TAIL) of it -- the outermost two and the smallest curvature scale
    double left = best, right = best, dl0 = 0.0, dl1 = 0.0, dmin = INFINITY, gg, cv;
    bool kept = false;
    g0 = gfirst;
    for (int i = 0; i < nc && any; ++i) {
        const double e0 = blo + (double)i * cw, e1 = i + 1 < nc ? blo + (double)(i + 1) * cw : bhi, g1 = bb_ll_d1(c, e1);
        if (g0 > 0.0 && !(g1 > 0.0)) {
            const double m = bb_ll_solve(c, e0, e1, e0 + (e1 - e0) / 2.0), v = bb_ll_lnp(c, m, &e);
            if (gbest - v <= -BB_GRID_TAIL) {
                bb_ll_d12(c, m, &gg, &cv);
                const double d = 1.0 / sqrt(-cv);
                if (!kept) { left = m; dl0 = d; }
                right = m; dl1 = d;
                if (d < dmin) dmin = d;
                kept = true;
            }
        }
        g0 = g1;
    }
    if (!kept) {
        bb_ll_d12(c, best, &gg, &cv);
        dl0 = dl1 = dmin = 1.0 / sqrt(-cv);
    }
    left -= best;
    right -= best;
    bb_ll_anchor(c, best);
    // (left, right and the ends as offsets from the global mode)
    return bb_grid_layout(left, right, dl0, dl1, dmin, 0.0, nleft, nright, [&](double u) { return bb_ll_lnp(c, u, &e); });
}

// the weight and the residual of data column i at step k of replicate r, draw j (the header's w_{i,k}, rho_{i,k})
BB_DEV void bb_ll_wrho(const LlArgs& L, int r, int k, long long i, int j, double* w, double* rho) {
    const FreqArgs& F = L.A.F;
    const PpcArgs& P = F.P;
    const int ns = P.n_samples, T = P.T[r];
    const double* Z = F.Z + (long long)P.tcum[r] * ns;      // ln Z (bb_block_rb_logz)
    const long long ll = F.off_l[r] + i * T + k;
    const double l0 = bb_ppc_param(P, ll, j), l1 = bb_ppc_param(P, ll + 1, j);
    const double gam = (l1 - l0) - (Z[(long long)(k + 1) * ns + j] - Z[(long long)k * ns + j]);
    if (i < F.nn) {
        // the group whose s_pop / logsigma_pop the term reads: (r, k), or under the ragged method's pairing the group that
        // bb_block_pop_part's table gives the member (t, b) = (k, i): element x = i (T - 1) + k of the time-fastest vector
        const long long g = P.off_t[r] + (L.quirk ? (i * (T - 1) + k) / F.nn : (long long)k);
        *w = exp(-2.0 * bb_ppc_param(P, P.lo_lspop + g, j));
        *rho = gam + bb_ppc_param(P, P.lo_spop + g, j);
    } else {
        const int E = P.E, e = (P.kind == 1 || P.kind == 4) ? P.env_idx[P.tcum[r] + k + 1] : 0;
        const long long m = i - F.nn, em = e + (long long)E * m, u = em + (long long)E * P.nb * r;
        double s, ls;
        if (P.kind < 2) {
            s = bb_ppc_param(P, P.lo_s + em, j);
            ls = bb_ppc_param(P, P.lo_ls + em, j);
        } else {
            const long long th = P.kind == 2 ? P.geno_idx[m] : em, uu = P.kind == 2 ? m : u;
            const double tau = exp(bb_ppc_param(P, P.lo_lt + uu, j));
            s = bb_ppc_param(P, P.lo_s + th, j) + tau * bb_ppc_param(P, P.lo_tt + uu, j);
            ls = bb_ppc_param(P, P.lo_ls + uu, j);
        }
        *w = exp(-2.0 * ls);
        *rho = (gam + P.pop[(long long)(2 * (P.off_t[r] + k)) * ns + j]) - s;
    }
}

BB_DEV void bb_block_ll_part(BBCtx& cx, const LlArgs& L, int nblocks) {
    const FreqArgs& F = L.A.F;
    const PpcArgs& P = F.P;
    const int ns = P.n_samples, nch = F.nchunks;
    const long long nwork = (L.g1 - L.g0) * nch;
    for (long long wk = cx.block; wk < nwork; wk += nblocks) {
        const long long g = L.g0 + wk / nch;
        const int c = (int)(wk % nch);
        int r = 0;
        while (r + 1 < P.R && g >= P.off_t[r + 1]) ++r;
        const int k = (int)(g - P.off_t[r]);
        const long long i0 = (long long)c * BB_FREQ_CHUNK, i1 = i0 + BB_FREQ_CHUNK < F.B ? i0 + BB_FREQ_CHUNK : F.B;
        double* part = L.part + wk * 2 * ns;
        BB_PASS(cx, tid) {
            for (int j = tid; j < ns; j += BB_SCORE_NT) {
                double SA = 0.0, SB = 0.0;
                for (long long i = i0; i < i1; ++i) {
                    double w, rho;
                    bb_ll_wrho(L, r, k, i, j, &w, &rho);
                    SA += w;
                    SB += w * rho;
                }
                part[j] = SA;
                part[ns + j] = SB;
            }
        }
    }
}

BB_DEV void bb_block_ll_sum(BBCtx& cx, const LlArgs& L, int nblocks) {
    const int ns = L.A.F.P.n_samples, nch = L.A.F.nchunks;
    const long long n = (L.g1 - L.g0) * ns;
    BB_PASS(cx, tid) {
        for (long long x = (long long)cx.block * cx.nthr + tid; x < n; x += (long long)nblocks * cx.nthr) {
            const long long gi = x / ns;
            const int j = (int)(x % ns);
            double SA, SB;
            bb_rb_chunk_sum(L.part + gi * nch * 2 * ns, nch, ns, j, SA, SB);
            L.ab[((L.g0 + gi) * 2) * ns + j] = SA;
            L.ab[((L.g0 + gi) * 2 + 1) * ns + j] = SB;
        }
    }
}

// The conditionals of one entry for bb_grid_mixture: rows 0 .. 5 of the block's table hold the draws' coefficients about the draw
// itself (pass C of bb_block_ll), x0 among them; sweep A puts the ones that move with the base point back about the global mode.
struct LlMix : GridRows {
    typedef LlCond Cond;
    static constexpr int NX = 1;          // lambda_mean
    static constexpr bool L_KEPT = true;  // pass C put x0 there
    double a, ib2, R;         // the entry's prior and count
    const double *Asj, *wsj;
    double *Bsj, *wrj, *f0j, *loj;

    BB_MEM LlMix(double a_, double ib2_, double R_, double* tab, long long ns) : a(a_), ib2(ib2_), R(R_) {
        Asj = tab; wsj = tab + ns; Bsj = tab + 2 * ns; wrj = tab + 3 * ns; f0j = tab + 4 * ns;
        l = tab + 5 * ns; E = tab + 6 * ns; V = tab + 7 * ns; x0 = tab + 8 * ns; loj = tab + 9 * ns; hi = tab + 10 * ns;
        x1 = two = nullptr;
    }
    BB_MEM void cond(LlCond& c, int j, double x) const {
        c.a = a; c.ib2 = ib2; c.R = R; c.As = Asj[j]; c.ws = wsj[j];
        c.x = x; c.ex = exp(x); c.f0 = f0j[j]; c.Bs = Bsj[j]; c.wr = wrj[j];
    }
    BB_MEM double setup(int j, LlCond& c, double* w, int* nleft, int* nright, bool*) const {
        cond(c, j, l[j]);
        const double s = bb_ll_setup(c, nleft, nright);
        *w = s;
        return s;
    }
    BB_MEM double p(const LlCond& c, double u, double* em) const { return exp(bb_ll_lnp(c, u, em)); }
    BB_MEM void extras(const LlCond&, double p, double, double em, double* se, double*) const { *se += p * (em + 1.0); }
    BB_MEM double finish0(const LlCond& c, double z, double se) const { return c.ex * (se / z); }
    BB_MEM double finish1(const LlCond&, double, double x) const { return x; }
    BB_MEM double mode(const LlCond& c) const { return c.x; }
    BB_MEM double latent(int j) const { return l[j]; }
    BB_MEM void keep(int j, const LlCond& c, double lm, double s, int nleft) const {
        Bsj[j] = c.Bs; wrj[j] = c.wr; f0j[j] = c.f0;
        loj[j] = lm - (double)nleft * s;
    }
    BB_MEM double lo(int j, double, double) const { return loj[j]; }
    BB_MEM void reopen(int j, LlCond& c, double lm) const { cond(c, j, lm); }
    // (h' takes the offset)
    BB_MEM double cdf_z(const LlCond& c, double s, double lo, double x) const {
        const double ulo = lo - c.x, ux = x - c.x;
        return bb_grid_cdf_z(x - lo, s, ulo, ux, [&](double u, double* em) { return exp(bb_ll_lnp(c, u, em)); },
                             [&](bool upper, double) { return bb_ll_d1(c, upper ? ux : ulo); });
    }
};

BB_DEV void bb_block_ll(BBCtx& cx, const LlArgs& L, int nblocks) {
    const RbArgs& A = L.A;
    const FreqArgs& F = A.F;
    const PpcArgs& P = F.P;
    const int ns = P.n_samples;
    const long long n_units = A.n_units;
    double* tab = A.ytab + (long long)cx.block * BB_LL_TAB * ns;
    double* Asj = tab;
    double* wsj = tab + ns;
    double* Bsj = tab + 2 * (long long)ns;
    double* wrj = tab + 3 * (long long)ns;
    double* f0j = tab + 4 * (long long)ns;
    double* lj = tab + 5 * (long long)ns;
    for (long long x = cx.block; x < L.n_req; x += nblocks) {
        const long long row = L.rows ? L.rows[x] : x;
        const int r = (int)(row / F.B);
        const long long b = row % F.B;
        const int T = P.T[r];
        const long long ll = F.off_l[r] + b * T;
        for (int t = 0; t < T; ++t) {
            const long long ent = x * L.n_cols + t;
            const double a = L.ent[ent], ib2 = L.ent[n_units + ent], Rc = L.ent[2 * n_units + ent];
            const double* Zt = F.Z + (long long)(P.tcum[r] + t) * ns;
            // pass C: the coefficients about the draw itself
            BB_PASS(cx, tid) {
                for (int j = tid; j < ns; j += BB_SCORE_NT) {
                    const double x0 = bb_ppc_param(P, ll + t, j);
                    double As = 0.0, Bs = 0.0, ws = 0.0, wr = 0.0, w, rho;
                    if (t + 1 < T) {
                        const double* ab = L.ab + (long long)(2 * (P.off_t[r] + t)) * ns;
                        bb_ll_wrho(L, r, t, b, j, &w, &rho);
                        As = ab[j]; Bs = ab[ns + j]; ws = w; wr = w * rho;
                    }
                    if (t >= 1) {
                        const double* ab = L.ab + (long long)(2 * (P.off_t[r] + t - 1)) * ns;
                        bb_ll_wrho(L, r, t - 1, b, j, &w, &rho);
                        As = As + ab[j]; Bs = Bs - ab[ns + j]; ws = ws + w; wr = wr - w * rho;
                    }
                    Asj[j] = As; wsj[j] = ws; Bsj[j] = Bs; wrj[j] = wr;
                    f0j[j] = exp(x0 - Zt[j]);
                    lj[j] = x0;
                }
            }
            bb_grid_mixture(cx, ns, A.nq, A.probs, cx.lds, A.unit, n_units, ent, A.quant, LlMix(a, ib2, Rc, tab, ns));
        }
    }
}
