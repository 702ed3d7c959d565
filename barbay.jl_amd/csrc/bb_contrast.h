// bb_contrast.h -- Rao-Blackwellised marginals of linear contrasts of fitnesses on the device.  Entry point bb_contrast_rb
// (include/barbay_hip.h, where the formulas are); no reference counterpart.
//
// Given everything else, distinct fitness units (and distinct groups theta_g) are conditionally independent: no term of the log-joint
// holds two of them.  The conditional of a contrast sum_k w_k x_k of distinct elements is therefore N(M_j, sd_j) with
// M_j = sum_k w_k m_{k,j}, sd_j^2 = sum_k w_k^2 sd_{k,j}^2, the (m, sd) of bb_fitness_rb (BB_CONTRAST_FITNESS) or bb_theta_rb
// (BB_CONTRAST_THETA), and bb_rb_mixture (bb_rb.h) applies to (d_j, M_j, sd_j), d_j = sum_k w_k s_{k,j}, as it stands.
//
// After the phases every call of bb_rb.h starts with (bb_block_ppc_pop, the normalisers, bb_block_rb_logz):
//   bb_block_contrast : one workgroup of BB_SCORE_NT threads per contrast, c += nblocks.  The fill of bb_rb_mixture walks the
//        contrast's terms in the caller's order, (d, M, V) from 0.0 in registers; a term's (s, m, sd) of draw j are one thread's:
//        FITNESS  bb_contrast_unit: one walk over the unit's loglambda row, the steps of the unit's environment summed and counted
//                 (bb_rb_member_y, which bb_block_theta_part walks a member with), then bb_block_rb's conditional.
//        THETA    bb_contrast_group: the group's members through the chunk map of bb_theta_rb (bb_analysis.h: theta_map), a chunk's
//                 (SP, SN) from 0.0, the chunks from 0.0 in chunk order, then bb_block_theta's conditional.  No partial tables and no
//                 groups in flight: a group is re-walked by every contrast that names it.
//        d_j lives in the block's [n_samples] slice of P.par, (M_j, sd_j) in LDS: bb_rb.h's layout and cap.
// Term validation and min_steps are the host's (bb_analysis.h).
#pragma once
#include "bb_rb.h"

struct ContrastArgs {
    ThetaArgs H;              // H.A as for bb_block_rb: unit [BB_RB_OUT][n_contrasts], quant [n_contrasts][8], n_units = n_contrasts,
                              // ytab [gridDim][n_samples]: d_j of the contrast being worked; F.P.pri_*: the s_bc prior as bb_fitness_rb
                              // (FITNESS) or bb_theta_rb (THETA) sets it.  THETA: grp_c0, grp_nst, chk_m0, mem_row, mem_nu; part unused
    const int* term_ptr;      // [n_contrasts + 1] CSR: the terms of contrast c are [term_ptr[c], term_ptr[c + 1])
    const int* term_idx;      // [n_terms] unit (FITNESS) or group (THETA)
    const double* term_w;     // [n_terms]
    int space;                // 0: BB_CONTRAST_FITNESS, 1: BB_CONTRAST_THETA
};

// (s_j, m_j, sd_j) of bb_fitness_rb's unit u = e + E m + E nb r
BB_DEV void bb_contrast_unit(const FreqArgs& F, long long u, int j, double& s, double& mm, double& sd) {
    const PpcArgs& P = F.P;
    const int E = P.E;
    const bool hier = P.kind >= 2, menv = P.kind == 1 || P.kind == 4;
    const int e = (int)(u % E), r = (int)(u / ((long long)E * P.nb));
    const long long m = u / E % P.nb, em = e + (long long)E * m;
    int nu;
    const double y = bb_rb_member_y(F, r, m, e, menv, j, nu);
    double a, ib2, ls, tau = 0.0;
    if (!hier) {
        s = bb_ppc_param(P, P.lo_s + em, j);
        ls = bb_ppc_param(P, P.lo_ls + em, j);
        a = P.pri_mean_e ? P.pri_mean_e[em] : P.pri_mean;
        ib2 = P.pri_ivar_e ? P.pri_ivar_e[em] : P.pri_ivar;
    } else {
        const long long th = P.kind == 2 ? P.geno_idx[m] : em, uu = P.kind == 2 ? m : u;
        a = bb_ppc_param(P, P.lo_s + th, j);
        tau = exp(bb_ppc_param(P, P.lo_lt + uu, j));
        s = a + tau * bb_ppc_param(P, P.lo_tt + uu, j);
        ib2 = 1.0 / (tau * tau);
        ls = bb_ppc_param(P, P.lo_ls + uu, j);
    }
    if (nu == 0) {               // no step uses the unit: the conditional is the prior
        mm = a;
        sd = hier ? tau : 1.0 / sqrt(ib2);
    } else {
        const double w = exp(-2.0 * ls), Pj = ib2 + (double)nu * w;
        mm = (a * ib2 + w * y) / Pj;
        sd = 1.0 / sqrt(Pj);
    }
}

// (theta_j, m_j, sd_j) of bb_theta_rb's group g
BB_DEV void bb_contrast_group(const ThetaArgs& H, long long g, int j, double& s, double& mm, double& sd) {
    const FreqArgs& F = H.A.F;
    const PpcArgs& P = F.P;
    const int E = P.E, e = P.kind == 2 ? 0 : (int)(g % E);
    const bool menv = P.kind == 4;
    const double a = P.pri_mean_e ? P.pri_mean_e[g] : P.pri_mean, ib2 = P.pri_ivar_e ? P.pri_ivar_e[g] : P.pri_ivar;
    double SP = 0.0, SN = 0.0;
    for (int c = H.grp_c0[g]; c < H.grp_c0[g + 1]; ++c) {
        double cP = 0.0, cN = 0.0;
        for (int x = H.chk_m0[c]; x < H.chk_m0[c + 1]; ++x) {
            if (H.mem_nu[x] == 0) continue;       // the log-joint has no term for the member
            const long long row = H.mem_row[x];
            const int r = (int)(row / P.nb);
            const long long m = row % P.nb;
            int nu;
            const double y = bb_rb_member_y(F, r, m, e, menv, j, nu);
            const long long uu = P.kind == 2 ? m : e + (long long)E * m + (long long)E * P.nb * r;
            const double w = exp(-2.0 * bb_ppc_param(P, P.lo_ls + uu, j));
            const double tau = exp(bb_ppc_param(P, P.lo_lt + uu, j)), tt = bb_ppc_param(P, P.lo_tt + uu, j);
            cP += (double)nu * w;
            cN += w * (y - (double)nu * (tau * tt));
        }
        SP += cP;
        SN += cN;
    }
    if (H.grp_nst[g] == 0) {         // no contributing member: the conditional is the prior
        mm = a;
        sd = 1.0 / sqrt(ib2);
    } else {
        const double Pj = ib2 + SP;
        mm = (a * ib2 + SN) / Pj;
        sd = 1.0 / sqrt(Pj);
    }
    s = bb_ppc_param(P, P.lo_s + g, j);
}

BB_DEV void bb_block_contrast(BBCtx& cx, const ContrastArgs& C, int nblocks) {
    const RbArgs& A = C.H.A;
    const int ns = A.F.P.n_samples;
    double* mj = cx.lds;
    double* sdj = cx.lds + ns;
    double* red = cx.lds + 2 * (long long)ns;
    double* st = red + 3 * BB_SCORE_NT;
    double* dj = A.ytab + (long long)cx.block * ns;
    const bool theta = C.space == 1;
    for (long long c = cx.block; c < A.n_units; c += nblocks) {
        const int k0 = C.term_ptr[c], k1 = C.term_ptr[c + 1];
        bb_rb_mixture(cx, ns, A.nq, A.probs, A.threshold, dj, mj, sdj, red, st, A.unit, A.n_units, c, A.quant, [&](int j, double& s, double& mm, double& sd) {
            double d = 0.0, M = 0.0, V = 0.0;
            for (int k = k0; k < k1; ++k) {
                const double w = C.term_w[k];
                double ts, tm, tsd;
                if (theta) bb_contrast_group(C.H, C.term_idx[k], j, ts, tm, tsd);
                else bb_contrast_unit(A.F, C.term_idx[k], j, ts, tm, tsd);
                const double ws = w * tsd;
                d += w * ts;
                M += w * tm;
                V += ws * ws;
            }
            s = d;
            mm = M;
            sd = sqrt(V);
        });
    }
}
