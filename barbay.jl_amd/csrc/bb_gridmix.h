// bb_gridmix.h -- the mixture of per-draw conditionals that are integrated on a grid: what bb_lsrb.h (logsigma), bb_ltrb.h (logtau)
// and bb_llrb.h (loglambda) share.  Each of them states one conditional -- one-dimensional, not Gaussian -- and its mode search; the
// trapezoid sums, the averages over the draws and the quantiles of the mixture are formed here, once.
//
// A conditional is a struct M derived from GridRows (the table rows the sweeps read and write), made per entry by its block program
// after the pass that fills the draws' coefficients into the block's table, with
//   M::Cond, M::NX     draw j's conditional about its mode (registers only); the number of extra functionals averaged: 1, or 2 and
//                      with them the count of the draws that kept two modes
//   setup(j, c, &w, &nleft, &nright, &two) -> s     the mode(s) and the grid from the table: step s, intervals left and right of the
//                      mode, which is a node; w: what the second LDS array keeps of the draw (its curvature scale or its step)
//   p(c, u, &aux)      the density at the offset u from the mode, as a multiple of the mode's; aux: a by-product extras / dh reuse
//   extras(c, p, u, aux, &x0, &x1), finish0(c, z, x0), finish1(c, z, x1)     a node's terms of the extra sums; a sum -> its functional
//   mode(c), latent(j), L_KEPT, keep(j, c, lm, s, nleft)       l*_j; the entry's own draw l_j (L_KEPT: it is in row l already); what
//                      else sweep Q reads back later
//   lo(j, lm, w), reopen(j, c, lm), cdf_z(c, w, lo, x)         sweep Q: lo_j, the cheaper rebuild of c, Z_j C_j(x) (bb_grid_cdf_z);
//                      lm, w: the draw's two LDS entries, read once per draw before the midpoints are looked at
// all inlined: nothing is dispatched at run time.  Where the three differ in floating-point order each keeps its own expression in
// these members; nothing here rounds differently from what the three headers did on their own.
//
// bb_grid_mixture, one workgroup of BB_SCORE_NT threads per entry (draw j is lane j mod BB_SCORE_NT's in every sweep, so a lane
// reads only table and LDS entries it wrote):
//   A   per draw the mode, the grid, the moments: l*, w, Z into LDS; l, E, V, the extras, hi (keep: lo, ...) into the table
//                                                                                                    -> sum l, sum E, sum V
//   A'  (no arithmetic on the grid)  NX = 1:                                                          -> sum x0, sum l*, max hi_j
//                                    NX = 2:                               -> sum x0, sum x1, sum l*;  sum two_j, (none), max hi_j
//   B   centred second moments                                     -> sum (l - q_mean)^2, sum (E - rb_mean)^2, max -lo_j
//   Q   bisection of the mixture CDF (bb_grid_bisect, BB_GRID_ITER steps); a draw whose [lo_j, hi_j] does not hold the midpoint adds 0
//       or 1 and evaluates nothing, the others rebuild c once for up to three midpoints.
// The maximum of hi_j takes NaN for a draw whose Z_j is not finite, so that the bracket is finite exactly when every l*_j, w_j and
// Z_j is; without a finite bracket every quantile of the entry is NaN.  st[] (bb_rb.h's layout): 0 .. 2 sweep A, 3 .. 5 (NX = 2:
// 3 .. 8) sweep A', then sweep B's three; 12 .. the bisection's.  Results: unit[k n_units + u], k = q_mean, q_sd, rb_mean, rb_sd, the
// extras' means, mode_mean (NX = 2: and the count of two-mode draws); quant[u][BB_RB_MAX_Q].
// Sums and maxima in bb_score_reduce's order; exp, expm1, log, log1p, sqrt, ceil are the platform's, as in bb_rb.h.  No per-thread
// array is indexed at run time (that would be scratch memory).  Barrier-separated passes, so the host emulation (BB_EMU) runs the
// same source.
#pragma once
#include "bb_rb.h"

#define BB_GRID_ITER 40                    // bisection steps of a quantile
#define BB_GRID_TAIL (-40.0)               // a mode is kept, and the grid ends, at exp(BB_GRID_TAIL) of the global maximum
#define BB_GRID_REACH 8                    // bb_grid_layout: an end lies 8 r delta beyond its outer mode, r = 1, 2, 4 .. BB_GRID_REACH_MAX
#define BB_GRID_REACH_MAX 4096
#define BB_GRID_REFINE_MAX 64              // the step is delta / (4 m), m = ceil(2 delta) up to this (a delta of 32 is no log-scale's)
#define BB_GRID_NODES_MAX 8192             // intervals of a draw's grid; beyond it the step is widened by a whole factor
#define BB_GRID_MODE_ITER 100              // steps of bb_grid_solve
#define BB_GRID_SLACK 9.5367431640625e-07 // 2^-20, taken off a quotient before ceil: a whole number but for rounding does not tip over
// LDS: l*[n_samples] | w[n_samples] | Z[n_samples] | three arrays of BB_SCORE_NT partials | scalars (bb_rb.h's st[] layout)
#define BB_GRID_LDS_DOUBLES(ns) (3 * (long long)(ns) + 3 * BB_SCORE_NT + BB_RB_SCALARS)
// the largest n_samples whose layout fits the 160 KiB of LDS a workgroup can have
#define BB_GRID_SAMPLES_CAP ((160 * 1024 / 8 - 3 * BB_SCORE_NT - BB_RB_SCALARS) / 3)
static_assert(BB_GRID_LDS_DOUBLES(BB_GRID_SAMPLES_CAP) * 8 <= 160 * 1024 && BB_GRID_LDS_DOUBLES(BB_GRID_SAMPLES_CAP + 1) * 8 > 160 * 1024,
              "BB_GRID_SAMPLES_CAP is the largest count that fits");
static_assert(BB_GRID_SAMPLES_CAP == 5781, "3 x 5781 doubles of (l*, w, Z) + 24 KiB of partials + 512 B of scalars <= 160 KiB");

// a member function of a conditional (BB_DEV is a free function's: static in the emulation)
#ifdef BB_EMU
#define BB_MEM inline
#else
#define BB_MEM __device__ __forceinline__
#endif

// the rows [n_samples] of the block's table that the sweeps themselves read and write (x1, two: NX = 2 only)
struct GridRows {
    double *l, *E, *V, *x0, *x1, *hi, *two;
};

// m of the step delta / (4 m) from ceil(2 delta): within 1 .. BB_GRID_REFINE_MAX, and 1 for a NaN
BB_DEV double bb_grid_refine(double m) {
    return m >= 1.0 ? (m <= (double)BB_GRID_REFINE_MAX ? m : (double)BB_GRID_REFINE_MAX) : 1.0;
}
// an interval count from a quotient: ceil(x - 2^-20) where 1 <= x <= 1e9, else 1 (a NaN included)
BB_DEV long long bb_grid_count(double x) {
    return (x >= 1.0 && x <= 1e9) ? (long long)ceil(x - BB_GRID_SLACK) : 1;
}

// the root of h' in [lo, hi], on which h' falls through zero, from x: Newton, a bisection step wherever Newton's leaves the bracket.
// d1(x): h'; d2(x): h'', asked for right after d1 at the same x and only where h' is neither zero nor NaN
template <class D1, class D2>
BB_DEV double bb_grid_solve(double lo, double hi, double x, D1&& d1, D2&& d2) {
    for (int it = 0; it < BB_GRID_MODE_ITER; ++it) {
        const double g = d1(x);
        if (g == 0.0 || g != g) return x + g;      // (a NaN h': the mode is NaN)
        if (g > 0.0) lo = x;
        else hi = x;
        const double cv = d2(x);
        double xn = x - g / cv;
        if (!(cv < 0.0 && xn >= lo && xn <= hi)) xn = lo + (hi - lo) / 2.0;
        const double step = xn - x;
        x = xn;
        if (fabs(step) <= 9.094947017729282e-13 * (1.0 + fabs(x))) break;      // 2^-40
    }
    const double g = d1(x), cv = d2(x), xn = x - g / cv;      // one more Newton step where it stays inside: the iteration's last
    return cv < 0.0 && xn >= lo && xn <= hi ? xn : x;          // step bounds the error by 2^-40 only
}

// The grid over the kept modes of a conditional with more than one: the outermost two (left, right; curvature scales dl0, dl1), the
// smallest scale dmin.  The step is dmin / (4 m); an end is the first of 8 r delta beyond its outer mode at which lnp(u), u the
// offset from the anchor, has fallen to BB_GRID_TAIL; more than BB_GRID_NODES_MAX intervals widen the step by a whole factor.
// left, right and the ends are coordinates of which the anchor is `origin`.  Returns the step; *nleft, *nright: intervals left and
// right of the anchor, which is a node.
template <class LnP>
BB_DEV double bb_grid_layout(double left, double right, double dl0, double dl1, double dmin, double origin, int* nleft, int* nright, LnP&& lnp) {
    const double m = bb_grid_refine(isfinite(dmin) ? ceil(2.0 * dmin - BB_GRID_SLACK) : 1.0);
    const double s = dmin / (4.0 * m);
    int r = 1;
    while (r < BB_GRID_REACH_MAX && lnp((left - (double)(BB_GRID_REACH * r) * dl0) - origin) > BB_GRID_TAIL) r *= 2;
    const double end0 = left - (double)(BB_GRID_REACH * r) * dl0;
    r = 1;
    while (r < BB_GRID_REACH_MAX && lnp((right + (double)(BB_GRID_REACH * r) * dl1) - origin) > BB_GRID_TAIL) r *= 2;
    const double end1 = right + (double)(BB_GRID_REACH * r) * dl1;
    const long long nl = bb_grid_count((origin - end0) / s), nr = bb_grid_count((end1 - origin) / s);
    const long long f = (nl + nr + BB_GRID_NODES_MAX - 1) / BB_GRID_NODES_MAX;
    *nleft = (int)((nl + f - 1) / f);
    *nright = (int)((nr + f - 1) / f);
    return s * (double)f;
}

// A draw's CDF at x, times Z_j: the trapezoid on N + 1 equidistant nodes from lo_j to x, N = ceil(r / s), r = x - lo_j, less the
// first Euler-Maclaurin end term; lo_j < x < hi_j.  ulo, ux: the offsets of lo_j and x from the mode; p(u, &aux) the density,
// dh(upper, aux) h' at x (upper) or at lo_j, aux what p gave there.
template <class P, class DH>
BB_DEV double bb_grid_cdf_z(double r, double s, double ulo, double ux, P&& p, DH&& dh) {
    double N = ceil(r / s);
    N = N >= 1.0 ? N : 1.0;
    const double sx = r / N;
    const int n = (int)N;
    double e0, e1, e;
    const double p0 = p(ulo, &e0), p1 = p(ux, &e1);
    double acc = 0.5 * p0;
    for (int i = 1; i < n; ++i) acc += p(ulo + (double)i * sx, &e);
    acc += 0.5 * p1;
    return sx * acc - sx * sx / 12.0 * (dh(true, e1) * p1 - dh(false, e0) * p0);
}

// The quantiles of a mixture by bisection: st[15] says whether the brackets st[16 + i] .. st[24 + i] are finite (if not, every
// quantile is NaN); STEPS times, for up to three quantiles per sweep, cdf(j, nx, xs, acc) adds draw j's CDF at the midpoints
// xs[0 .. nx) into acc[0 .. nx), the sums go to st[12 ..], and a bracket whose mean CDF is below probs[i] moves its lower end to the
// midpoint, any other its upper.  q[0 .. nq): the last midpoints.  Ends with a barrier.
// (bb_rb_mixture keeps its own copy of this loop, BB_RB_ITER steps of erfc: on this driver k_rb, k_rb_theta and k_rb_pop take 22 to
// 37 more VGPRs -- profiles/gridmix/kernel_resources.txt.)
template <int STEPS, class Cdf>
BB_DEV void bb_grid_bisect(BBCtx& cx, int ns, int nq, const double* probs, double* red, double* st, double* q, Cdf&& cdf) {
    if (nq > 0 && st[15] == 0.0) {
        BB_PASS(cx, tid) { if (tid < nq) q[tid] = NAN; }
    } else if (nq > 0) {
        for (int it = 0; it < STEPS; ++it) {
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
                    for (int j = tid; j < ns; j += BB_SCORE_NT) cdf(j, nx, xs, acc);
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
        BB_PASS(cx, tid) { if (tid < nq) q[tid] = st[16 + tid] + (st[24 + tid] - st[16 + tid]) / 2.0; }
    }
    BB_SYNC(cx);
}

// The mixture of entry u's conditionals m (the file's head).  lds: BB_GRID_LDS_DOUBLES(ns).  Ends with a barrier: the next entry's
// sweep A overwrites what this one read.
template <class M>
BB_DEV void bb_grid_mixture(BBCtx& cx, int ns, int nq, const double* probs, double* lds, double* unit, long long n_units, long long u,
                            double* quant, const M& m) {
    typedef typename M::Cond Cond;
    constexpr int NX = M::NX, SB = NX == 1 ? 6 : 9;      // st[SB ..]: sweep B's sums
    double* ms = lds;
    double* wj = lds + ns;
    double* zz = lds + 2 * (long long)ns;
    double* red = lds + 3 * (long long)ns;
    double* st = red + 3 * BB_SCORE_NT;
    // sweep A: mode, grid and per-draw moments; first sums
    BB_PASS(cx, tid) {
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
        for (int j = tid; j < ns; j += BB_SCORE_NT) {
            Cond c;
            int nleft = 0, nright = 0;
            bool two = false;
            double w;
            const double s = m.setup(j, c, &w, &nleft, &nright, &two);
            const int nodes = nleft + nright;
            double z = 0.0, m1 = 0.0, m2 = 0.0, x0 = 0.0, x1 = 0.0;
            for (int k = 0; k <= nodes; ++k) {
                const double uk = (double)(k - nleft) * s;
                double aux;
                double p = m.p(c, uk, &aux);
                if (k == 0 || k == nodes) p *= 0.5;
                z += p;
                m1 += p * uk;
                m2 += p * (uk * uk);
                m.extras(c, p, uk, aux, &x0, &x1);
            }
            const double lm = m.mode(c), Z = s * z, r1 = m1 / z, E = lm + r1, V = m2 / z - r1 * r1;
            x0 = m.finish0(c, z, x0);
            if (NX == 2) x1 = m.finish1(c, z, x1);
            const double l = m.latent(j);
            ms[j] = lm; wj[j] = w; zz[j] = Z;
            if (!M::L_KEPT) m.l[j] = l;
            m.E[j] = E; m.V[j] = V; m.x0[j] = x0; m.hi[j] = lm + (double)nright * s;
            if (NX == 2) { m.x1[j] = x1; m.two[j] = two ? 1.0 : 0.0; }
            m.keep(j, c, lm, s, nleft);
            a0 += l;
            a1 += E;
            a2 += V;
        }
        red[tid] = a0; red[BB_SCORE_NT + tid] = a1; red[2 * BB_SCORE_NT + tid] = a2;
    }
    BB_SYNC(cx);
    bb_score_reduce(cx, red, st, false);
    // sweep A': the other first sums; the largest hi_j (NaN where Z_j is not finite)
    if (NX == 2) {
        BB_PASS(cx, tid) {
            double a0 = 0.0, a1 = 0.0, a2 = 0.0;
            for (int j = tid; j < ns; j += BB_SCORE_NT) {
                a0 += m.x0[j];
                a1 += m.x1[j];
                a2 += ms[j];
            }
            red[tid] = a0; red[BB_SCORE_NT + tid] = a1; red[2 * BB_SCORE_NT + tid] = a2;
        }
        BB_SYNC(cx);
        bb_score_reduce(cx, red, st + 3, false);
    }
    BB_PASS(cx, tid) {
        double a0 = 0.0, a1 = 0.0, mx = -INFINITY;
        for (int j = tid; j < ns; j += BB_SCORE_NT) {
            if (NX == 2) {
                a0 += m.two[j];
            } else {
                a0 += m.x0[j];
                a1 += ms[j];
            }
            mx = bb_score_max(mx, isfinite(zz[j]) ? m.hi[j] : (double)NAN);
        }
        red[tid] = a0; red[BB_SCORE_NT + tid] = a1; red[2 * BB_SCORE_NT + tid] = mx;
    }
    BB_SYNC(cx);
    bb_score_reduce(cx, red, st + SB - 3, true);
    // sweep B: centred second moments; the smallest lo_j (as the largest of -lo_j)
    BB_PASS(cx, tid) {
        const double qm = st[0] / ns, rm = st[1] / ns;
        double a0 = 0.0, a1 = 0.0, mx = -INFINITY;
        for (int j = tid; j < ns; j += BB_SCORE_NT) {
            const double d0 = m.l[j] - qm, d1 = m.E[j] - rm;
            a0 += d0 * d0;
            a1 += d1 * d1;
            mx = bb_score_max(mx, -m.lo(j, ms[j], wj[j]));
        }
        red[tid] = a0; red[BB_SCORE_NT + tid] = a1; red[2 * BB_SCORE_NT + tid] = mx;
    }
    BB_SYNC(cx);
    bb_score_reduce(cx, red, st + SB, true);
    BB_PASS(cx, tid) {
        if (tid == 0) {
            unit[0 * n_units + u] = st[0] / ns;
            unit[1 * n_units + u] = sqrt(st[SB] / ns);
            unit[2 * n_units + u] = st[1] / ns;
            unit[3 * n_units + u] = sqrt(st[2] / ns + st[SB + 1] / ns);
            for (int k = 0; k <= NX; ++k) unit[(4 + k) * n_units + u] = st[3 + k] / ns;      // the extras, then l*
            if (NX == 2) unit[7 * n_units + u] = st[6];
            const double lo = -st[SB + 2], hi = st[SB - 1];
            st[15] = (nq > 0 && isfinite(lo) && isfinite(hi)) ? 1.0 : 0.0;
            for (int i = 0; i < nq; ++i) { st[16 + i] = lo; st[24 + i] = hi; }
        }
    }
    BB_SYNC(cx);
    // sweep Q
    bb_grid_bisect<BB_GRID_ITER>(cx, ns, nq, probs, red, st, quant + u * BB_RB_MAX_Q, [&](int j, int nx, const double* xs, double* acc) {
        Cond c;
        const double lm = ms[j], w = wj[j], lo = m.lo(j, lm, w), hi = m.hi[j];
        bool have = false;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if (i >= nx) continue;
            const double x = xs[i];
            if (x <= lo) continue;                       // C_j = 0
            if (x >= hi) { acc[i] += 1.0; continue; }    // C_j = 1
            if (!have) {
                m.reopen(j, c, lm);
                have = true;
            }
            const double C = m.cdf_z(c, w, lo, x) / zz[j];
            acc[i] += C < 0.0 ? 0.0 : (C > 1.0 ? 1.0 : C);
        }
    });
}
