// bb_rb.h -- Rao-Blackwellised marginals of the mutants' fitness on the device.  Entry point bb_fitness_rb (include/barbay_hip.h,
// where the formulas are); no reference counterpart.
//
// Given everything else, a mutant's fitness s_u enters the log-joint through a Gaussian prior and Gaussian log-frequency-ratio terms
// only (model_fitness_normal.jl:262-270 and its four siblings), so its full conditional is N(m, sd) in closed form.  A sample
// j < n_samples is the joint posterior draw of bb_ppc.h (same keying, BB_STREAM_PPC_PARAM) or row j of the caller's draws; the
// conditionals N(m_j, sd_j) of a unit u = (r, m, e) are averaged over j: moments, both tails at a threshold, quantiles of the mixture.
//
// Phases of a call (bb_analysis.h): bb_block_ppc_pop (sbar_{t,j}), bb_block_freq_zpart / _zsum (Z_{r,t,j}, every time point, summed by
// bb_freq.h's rule), bb_block_rb_logz (ln Z in place, once: the rows of a replicate all read the same ones), then the row program:
//   bb_block_rb : one workgroup of BB_SCORE_NT threads per mutant row (r, m), row += nblocks.
//     Y  per draw one walk over the row's T_r loglambda draws: gamma_t = (ll_{t+1} - ll_t) - (log Z_{t+1} - log Z_t) and
//        y_e += gamma_t + sbar_t for e = env(t + 1), ascending t.  The E running sums of a draw live in the block's slice of a global
//        table ytab[E + 1][n_samples] (row E: the unit's s_j), not in a per-thread array: indexed by a run-time environment such an
//        array would be scratch memory.  A draw j is always lane j mod NT's, so every table entry is read by the thread that wrote it.
//     per environment e (unit u = e + E m + E nb r), bb_rb_mixture, shared with bb_block_theta:
//     A  s_j, m_j, sd_j (m, sd kept in LDS)            -> sum s, sum m, sum sd^2
//     B  centred second moments                        -> sum (s - q_mean)^2, sum (m - rb_mean)^2, max m
//     C  both tails at the threshold, through erfc     -> their sums, max -m
//     D  (n_quantiles > 0)                             -> max sd
//     Q  bisection of the mixture CDF, 64 iterations: the reduction has three slots, so one sweep over the draws advances up to three
//        quantiles, ceil(n_q / 3) sweeps per iteration; every quantile of the unit moves in the same iteration.
// Sums and maxima in bb_score_reduce's order (bb_score.h): a function of n_samples alone, no atomics.  exp, log, erfc, sqrt are the
// platform's (ocml on the device, libm in the emulation), as in bb_score.h: non-finite parameters propagate by IEEE rules into the
// units that use them (bb_exp, which clamps, is used only where bb_ppc.h / bb_freq.h use it: the tables this file reads as they are).
// Barrier-separated passes, so the host emulation (BB_EMU) runs the same source.
//
// Entry point bb_theta_rb: the same for the hyper-fitness theta_g of the hierarchical kinds, whose conditional sums over the members
// of a group g (a genotype's mutants; a mutant's replicates).  After the phases above, in place of bb_block_rb:
//   bb_block_theta_part : one workgroup of BB_SCORE_NT threads per chunk of BB_THETA_CHUNK consecutive members of a group,
//        chunk += nblocks.  Per draw it walks the chunk's members in order; a member's loglambda row once (bb_rb_member_y: pass Y's body, the
//        steps of the group's environment only, y in a register), cP = n_u w, cN = w (y - n_u (tau theta_tilde)); a member with n_u = 0 is
//        skipped.  The chunk's (SP, SN), from 0.0, go to the partial table part[chunk][2][n_samples].
//   bb_block_theta      : one workgroup per group, g += nblocks.  Per draw the group's chunk partials from 0.0 in chunk order, the
//        prior (a, 1 / b^2) added, theta_j, m_j, sd_j written where bb_block_rb writes them; then bb_rb_mixture.
// The chunk map (group -> first chunk and sum of n_u, chunk -> group and first member, member -> mutant row r nb + m and n_u) is built
// on the host (bb_analysis.h); the order of every sum is the map's, not the grid's.
//
// Entry point bb_popmean_rb: the same for the population mean fitness sbar_g of a group g = (r, k), replicate r and step k, whose
// conditional sums over every barcode of the replicate: members i < nn the neutral terms, i >= nn the mutants at step k.  No
// bb_block_ppc_pop (the conditional does not read sbar; its own draws are read from the latent); after the normalisers and
// bb_block_rb_logz:
//   bb_block_pop_part   : one workgroup of BB_SCORE_NT threads per (group, chunk of BB_POP_CHUNK consecutive members),
//        work += nblocks.  Per draw it walks the chunk's members in index order, (SP, SN) in registers: a member's two loglambda
//        draws of step t and the step's ln Z give gamma; neutral: cP = w, cN = -(w gamma), w = exp(-2 logsigmabar_{g,j}) from the
//        latent's draw; mutant: its bb_fitness_rb unit u of environment env_r(k + 1), cP = w_u, cN = w_u (s_u - gamma).  A neutral
//        member is data column i at step k, or under the ragged method's pairing (quirk) the (t, b) the host's table names.
//        The simple form: a loglambda entry is drawn by both groups whose step it bounds (per-step accumulators of one walk over
//        the row would be indexed at run time: scratch memory).
//   bb_block_pop        : one workgroup per group.  Per draw the chunk partials from 0.0 in chunk order (bb_rb_chunk_sum, shared
//        with bb_block_theta), the prior (a, 1 / b^2) of s_pop[g] added, sbar_j the latent's draw; then bb_rb_mixture.
#pragma once
#include "bb_freq.h"
#include "bb_score.h"

#define BB_RB_MAX_Q 8
#define BB_RB_OUT 6                        // per-unit results on the device: q_mean, q_sd, rb_mean, rb_sd, p_pos, p_neg
#define BB_RB_ITER 64                      // bisection steps
#define BB_RB_SCALARS 64                   // st[]: 0 .. 11 the reductions A .. D, 12 .. 14 a sweep's CDF sums, 15 bracket finite,
                                           // 16 .. 23 lo, 24 .. 31 hi (the rest: padding to a whole 512 bytes)
// LDS: m[n_samples] | sd[n_samples] | three arrays of BB_SCORE_NT partials (bb_score_reduce's layout) | scalars
#define BB_RB_LDS_DOUBLES(ns) (2 * (long long)(ns) + 3 * BB_SCORE_NT + BB_RB_SCALARS)
// the largest n_samples whose layout fits the 160 KiB of LDS a workgroup can have
#define BB_RB_SAMPLES_CAP ((160 * 1024 / 8 - 3 * BB_SCORE_NT - BB_RB_SCALARS) / 2)
static_assert(BB_RB_LDS_DOUBLES(BB_RB_SAMPLES_CAP) * 8 <= 160 * 1024 && BB_RB_LDS_DOUBLES(BB_RB_SAMPLES_CAP + 1) * 8 > 160 * 1024,
              "BB_RB_SAMPLES_CAP is the largest count that fits");
static_assert(BB_RB_SAMPLES_CAP == 8672, "2 x 8672 doubles of (m, sd) + 24 KiB of partials + 512 B of scalars = 160 KiB exactly");

struct RbArgs {
    FreqArgs F;               // posterior mode, every normaliser row; F.P: n_rows = R nb (the mutant rows), nb = the mutants, n_ppc = 1
    double* ytab;             // [gridDim][E + 1][n_samples] per-block scratch: y_{e,j}, then s_j of the unit being worked
    double* unit;             // [BB_RB_OUT][n_units]
    double* quant;            // [n_units][BB_RB_MAX_Q]
    int* n_steps;             // [n_units]
    double probs[BB_RB_MAX_Q];
    double threshold;
    long long n_units;
    int nq;
    int n_z;                  // rows of F.Z: every time point of every replicate
};

#define BB_THETA_CHUNK 64                   // == BB_THETA_RB_CHUNK of include/barbay_hip.h: members per partial sum of a group

struct ThetaArgs {
    RbArgs A;                 // as for bb_block_rb; unit [BB_RB_OUT][n_groups], quant [n_groups][8], n_units = n_groups, ytab [gridDim][n_samples]:
                              // theta_j of the group being worked; A.F.P.pri_*: the prior of theta (s_bc_prior), indexed by g
    const int* grp_c0;        // [n_groups + 1] group -> its first chunk
    const int* grp_nst;       // [n_groups] sum of n_u over the group's members (0: the conditional is the prior)
    const int* chk_grp;       // [n_chunks] chunk -> its group
    const int* chk_m0;        // [n_chunks + 1] chunk -> its first member
    const int* mem_row;       // [n_members] member -> mutant row r nb + m (m: the caller's mutant)
    const int* mem_nu;        // [n_members] member -> its n_u: the replicate's steps in the group's environment
    double* part;             // [c1 - c0][2][n_samples] chunk partials (SP, SN) of the groups in flight
    long long g0, g1;         // the groups in flight
    int c0, c1;               // ... and their chunks: grp_c0[g0], grp_c0[g1]
};

#define BB_POP_CHUNK 256                    // == BB_POPMEAN_RB_CHUNK of include/barbay_hip.h: members per partial sum of a group

struct PopArgs {
    RbArgs A;                 // as for bb_block_rb; unit [BB_RB_OUT][n_groups], quant [n_groups][8], n_units = n_groups = F.P.nt1, ytab [gridDim][n_samples]:
                              // sbar_j of the group being worked; A.F.P.pri_*: the prior of sbar (s_pop_prior), indexed by g
    const int* neu_t;         // [n_groups][nn] ragged-method pairing: neutral member i of group g -> its step t and data column b;
    const int* neu_b;         // nullptr: t = k, b = i
    double* part;             // [(g1 - g0) nchunks][2][n_samples] chunk partials (SP, SN) of the groups in flight
    long long g0, g1;         // the groups in flight
    int nchunks;              // chunks of a group: ceil((nn + nb) / BB_POP_CHUNK), the same for every group
};

// the normalisers F.Z[Ttot][n_samples] replaced by their logarithms, once per call: every mutant row of a replicate reads the same ones
BB_DEV void bb_block_rb_logz(BBCtx& cx, const RbArgs& A, int nblocks) {
    const long long n = (long long)A.n_z * A.F.P.n_samples;
    BB_PASS(cx, tid) {
        for (long long x = (long long)cx.block * cx.nthr + tid; x < n; x += (long long)nblocks * cx.nthr) A.F.Z[x] = log(A.F.Z[x]);
    }
}

// The mixture of a unit's conditionals, shared by bb_block_rb and bb_block_theta: fill(j, s, m, sd) gives draw j's (s_j, m_j, sd_j),
// which sweep A stores (draw j is lane j mod BB_SCORE_NT's in every sweep) and sums; the six results go to unit[k n_units + u], the nq
// quantiles to quant[u][BB_RB_MAX_Q]: sweeps A .. D and Q of the file's head.  (fill runs inside sweep A, not in a pass of its own
// before it: bb_block_rb then keeps the registers it had before the sweeps were shared.)  Ends with a barrier: the next
// unit's sweep A overwrites what this one read.
template <class Fill>
BB_DEV void bb_rb_mixture(BBCtx& cx, int ns, int nq, const double* probs, double s0, double* sj, double* mj, double* sdj, double* red, double* st,
                          double* unit, long long n_units, long long u, double* quant, Fill&& fill) {
    const double rsqrt2 = 0.70710678118654752440;
    // sweep A: the conditionals into LDS; first moments
    BB_PASS(cx, tid) {
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
        for (int j = tid; j < ns; j += BB_SCORE_NT) {
            double s, mm, sd;
            fill(j, s, mm, sd);
            sj[j] = s;
            mj[j] = mm;
            sdj[j] = sd;
            a0 += s;
            a1 += mm;
            a2 += sd * sd;
        }
        red[tid] = a0; red[BB_SCORE_NT + tid] = a1; red[2 * BB_SCORE_NT + tid] = a2;
    }
    BB_SYNC(cx);
    bb_score_reduce(cx, red, st, false);
    // sweep B: centred second moments; the largest mean
    BB_PASS(cx, tid) {
        const double qm = st[0] / ns, rm = st[1] / ns;
        double a0 = 0.0, a1 = 0.0, mx = -INFINITY;
        for (int j = tid; j < ns; j += BB_SCORE_NT) {
            const double ds = sj[j] - qm, dm = mj[j] - rm;
            a0 += ds * ds;
            a1 += dm * dm;
            mx = bb_score_max(mx, mj[j]);
        }
        red[tid] = a0; red[BB_SCORE_NT + tid] = a1; red[2 * BB_SCORE_NT + tid] = mx;
    }
    BB_SYNC(cx);
    bb_score_reduce(cx, red, st + 3, true);
    // sweep C: both tails at the threshold; the smallest mean (as the largest of -m)
    BB_PASS(cx, tid) {
        double a0 = 0.0, a1 = 0.0, mx = -INFINITY;
        for (int j = tid; j < ns; j += BB_SCORE_NT) {
            const double v = (mj[j] - s0) / sdj[j] * rsqrt2;
            a0 += 0.5 * erfc(-v);
            a1 += 0.5 * erfc(v);
            mx = bb_score_max(mx, -mj[j]);
        }
        red[tid] = a0; red[BB_SCORE_NT + tid] = a1; red[2 * BB_SCORE_NT + tid] = mx;
    }
    BB_SYNC(cx);
    bb_score_reduce(cx, red, st + 6, true);
    if (nq > 0) {
        // sweep D: the largest sd
        BB_PASS(cx, tid) {
            double mx = -INFINITY;
            for (int j = tid; j < ns; j += BB_SCORE_NT) mx = bb_score_max(mx, sdj[j]);
            red[tid] = 0.0; red[BB_SCORE_NT + tid] = 0.0; red[2 * BB_SCORE_NT + tid] = mx;
        }
        BB_SYNC(cx);
        bb_score_reduce(cx, red, st + 9, true);
    }
    BB_PASS(cx, tid) {
        if (tid == 0) {
            unit[0 * n_units + u] = st[0] / ns;
            unit[1 * n_units + u] = sqrt(st[3] / ns);
            unit[2 * n_units + u] = st[1] / ns;
            unit[3 * n_units + u] = sqrt(st[2] / ns + st[4] / ns);
            unit[4 * n_units + u] = st[6] / ns;
            unit[5 * n_units + u] = st[7] / ns;
            const double lo = -st[8] - 40.0 * st[11], hi = st[5] + 40.0 * st[11];
            st[15] = (nq > 0 && isfinite(lo) && isfinite(hi)) ? 1.0 : 0.0;
            for (int i = 0; i < nq; ++i) { st[16 + i] = lo; st[24 + i] = hi; }
        }
    }
    BB_SYNC(cx);
    if (nq > 0 && st[15] == 0.0) {   // a non-finite m_j or sd_j: no bracket
        BB_PASS(cx, tid) { if (tid < nq) quant[u * BB_RB_MAX_Q + tid] = NAN; }
    } else if (nq > 0) {
        for (int it = 0; it < BB_RB_ITER; ++it) {
            for (int q0 = 0; q0 < nq; q0 += 3) {
                // sweep Q: the mixture CDF at the midpoints of up to three brackets
                BB_PASS(cx, tid) {
                    const int i1 = q0 + 1 < nq ? q0 + 1 : q0, i2 = q0 + 2 < nq ? q0 + 2 : q0;
                    const double x0 = st[16 + q0] + (st[24 + q0] - st[16 + q0]) / 2.0;
                    const double x1 = st[16 + i1] + (st[24 + i1] - st[16 + i1]) / 2.0;
                    const double x2 = st[16 + i2] + (st[24 + i2] - st[16 + i2]) / 2.0;
                    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
                    for (int j = tid; j < ns; j += BB_SCORE_NT) {
                        const double mm = mj[j], sd = sdj[j];
                        a0 += 0.5 * erfc(-((x0 - mm) / sd * rsqrt2));
                        if (q0 + 1 < nq) a1 += 0.5 * erfc(-((x1 - mm) / sd * rsqrt2));
                        if (q0 + 2 < nq) a2 += 0.5 * erfc(-((x2 - mm) / sd * rsqrt2));
                    }
                    red[tid] = a0; red[BB_SCORE_NT + tid] = a1; red[2 * BB_SCORE_NT + tid] = a2;
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

BB_DEV void bb_block_rb(BBCtx& cx, const RbArgs& A, int nblocks) {
    const FreqArgs& F = A.F;
    const PpcArgs& P = F.P;
    const int ns = P.n_samples, E = P.E, nq = A.nq;
    double* mj = cx.lds;
    double* sdj = cx.lds + ns;
    double* red = cx.lds + 2 * (long long)ns;
    double* st = red + 3 * BB_SCORE_NT;
    double* ytab = A.ytab + (long long)cx.block * (E + 1) * ns;
    double* sj = ytab + (long long)E * ns;
    const bool hier = P.kind >= 2, menv = P.kind == 1 || P.kind == 4;
    const double s0 = A.threshold;
    for (long long row = cx.block; row < P.n_rows; row += nblocks) {
        const int r = (int)(row / P.nb);
        const long long m = row % P.nb;
        const int T = P.T[r];
        const long long ll = F.off_l[r] + (F.nn + m) * T;
        const double* Z = F.Z + (long long)P.tcum[r] * ns;      // ln Z (bb_block_rb_logz)
        const double* sbar = P.pop + (long long)(2 * P.off_t[r]) * ns;
        // pass Y: every environment's y_j in one walk over the row's loglambda draws
        BB_PASS(cx, tid) {
            for (int j = tid; j < ns; j += BB_SCORE_NT) {
                for (int e = 0; e < E; ++e) ytab[(long long)e * ns + j] = 0.0;
                double l0 = bb_ppc_param(P, ll, j), z0 = Z[j];
                for (int t = 0; t + 1 < T; ++t) {
                    const double l1 = bb_ppc_param(P, ll + t + 1, j), z1 = Z[(long long)(t + 1) * ns + j];
                    const int e = menv ? P.env_idx[P.tcum[r] + t + 1] : 0;
                    ytab[(long long)e * ns + j] += ((l1 - l0) - (z1 - z0)) + sbar[(long long)(2 * t) * ns + j];
                    l0 = l1;
                    z0 = z1;
                }
            }
        }
        for (int e = 0; e < E; ++e) {
            const long long em = e + (long long)E * m, u = em + (long long)E * P.nb * r;
            int nu = 0;
            for (int t = 0; t + 1 < T; ++t) nu += !menv || P.env_idx[P.tcum[r] + t + 1] == e;
            const double* y = ytab + (long long)e * ns;
            BB_PASS(cx, tid) { if (tid == 0) A.n_steps[u] = nu; }
            bb_rb_mixture(cx, ns, nq, A.probs, s0, sj, mj, sdj, red, st, A.unit, A.n_units, u, A.quant, [&](int j, double& s, double& mm, double& sd) {
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
                    mm = (a * ib2 + w * y[j]) / Pj;
                    sd = 1.0 / sqrt(Pj);
                }
            });
        }
    }
}

// y_j of mutant row (r, m) in environment e, and in nu the steps summed: one walk over the row's loglambda draws (pass Y's body for
// one environment, y in a register), ascending t, the later time point's environment.  Shared with bb_contrast.h.
BB_DEV double bb_rb_member_y(const FreqArgs& F, int r, long long m, int e, bool menv, int j, int& nu) {
    const PpcArgs& P = F.P;
    const int ns = P.n_samples, T = P.T[r];
    const long long ll = F.off_l[r] + (F.nn + m) * T;
    const double* Z = F.Z + (long long)P.tcum[r] * ns;      // ln Z (bb_block_rb_logz)
    const double* sbar = P.pop + (long long)(2 * P.off_t[r]) * ns;
    double y = 0.0, l0 = bb_ppc_param(P, ll, j), z0 = Z[j];
    nu = 0;
    for (int t = 0; t + 1 < T; ++t) {
        const double l1 = bb_ppc_param(P, ll + t + 1, j), z1 = Z[(long long)(t + 1) * ns + j];
        if (!menv || P.env_idx[P.tcum[r] + t + 1] == e) {
            y += ((l1 - l0) - (z1 - z0)) + sbar[(long long)(2 * t) * ns + j];
            ++nu;
        }
        l0 = l1;
        z0 = z1;
    }
    return y;
}

BB_DEV void bb_block_theta_part(BBCtx& cx, const ThetaArgs& H, int nblocks) {
    const FreqArgs& F = H.A.F;
    const PpcArgs& P = F.P;
    const int ns = P.n_samples, E = P.E;
    const bool menv = P.kind == 4;
    for (long long c = (long long)H.c0 + cx.block; c < H.c1; c += nblocks) {
        const int e = P.kind == 2 ? 0 : H.chk_grp[c] % E, x0 = H.chk_m0[c], x1 = H.chk_m0[c + 1];
        double* part = H.part + (c - H.c0) * 2 * ns;
        BB_PASS(cx, tid) {
            for (int j = tid; j < ns; j += BB_SCORE_NT) {
                double SP = 0.0, SN = 0.0;
                for (int x = x0; x < x1; ++x) {
                    const long long row = H.mem_row[x];
                    const int r = (int)(row / P.nb);
                    const long long m = row % P.nb;
                    const int nu = H.mem_nu[x];
                    if (nu == 0) continue;       // the log-joint has no term for the member
                    int walked;                  // (== nu)
                    const double y = bb_rb_member_y(F, r, m, e, menv, j, walked);
                    const long long uu = P.kind == 2 ? m : e + (long long)E * m + (long long)E * P.nb * r;
                    const double w = exp(-2.0 * bb_ppc_param(P, P.lo_ls + uu, j));
                    const double tau = exp(bb_ppc_param(P, P.lo_lt + uu, j)), tt = bb_ppc_param(P, P.lo_tt + uu, j);
                    SP += (double)nu * w;
                    SN += w * (y - (double)nu * (tau * tt));
                }
                part[j] = SP;
                part[ns + j] = SN;
            }
        }
    }
}

// a group's (SP, SN) of draw j: its nc chunk partials part[c][2][ns], from 0.0 in chunk order
BB_DEV void bb_rb_chunk_sum(const double* part, int nc, int ns, int j, double& SP, double& SN) {
    SP = 0.0;
    SN = 0.0;
    for (int c = 0; c < nc; ++c) {
        SP += part[(long long)c * 2 * ns + j];
        SN += part[((long long)c * 2 + 1) * ns + j];
    }
}

BB_DEV void bb_block_theta(BBCtx& cx, const ThetaArgs& H, int nblocks) {
    const RbArgs& A = H.A;
    const PpcArgs& P = A.F.P;
    const int ns = P.n_samples;
    double* mj = cx.lds;
    double* sdj = cx.lds + ns;
    double* red = cx.lds + 2 * (long long)ns;
    double* st = red + 3 * BB_SCORE_NT;
    double* sj = A.ytab + (long long)cx.block * ns;
    for (long long g = H.g0 + cx.block; g < H.g1; g += nblocks) {
        const int c0 = H.grp_c0[g], c1 = H.grp_c0[g + 1], nst = H.grp_nst[g];
        const double a = P.pri_mean_e ? P.pri_mean_e[g] : P.pri_mean, ib2 = P.pri_ivar_e ? P.pri_ivar_e[g] : P.pri_ivar;
        bb_rb_mixture(cx, ns, A.nq, A.probs, A.threshold, sj, mj, sdj, red, st, A.unit, A.n_units, g, A.quant, [&](int j, double& s, double& mm, double& sd) {
            double SP, SN;
            bb_rb_chunk_sum(H.part + (long long)(c0 - H.c0) * 2 * ns, c1 - c0, ns, j, SP, SN);
            if (nst == 0) {                  // no contributing member: the conditional is the prior
                mm = a;
                sd = 1.0 / sqrt(ib2);
            } else {
                const double Pj = ib2 + SP;
                mm = (a * ib2 + SN) / Pj;
                sd = 1.0 / sqrt(Pj);
            }
            s = bb_ppc_param(P, P.lo_s + g, j);
        });
    }
}

BB_DEV void bb_block_pop_part(BBCtx& cx, const PopArgs& H, int nblocks) {
    const FreqArgs& F = H.A.F;
    const PpcArgs& P = F.P;
    const int ns = P.n_samples, E = P.E;
    const bool hier = P.kind >= 2, menv = P.kind == 1 || P.kind == 4;
    const long long nn = F.nn, nmem = F.nn + P.nb, nwork = (H.g1 - H.g0) * H.nchunks;
    for (long long wk = cx.block; wk < nwork; wk += nblocks) {
        const long long g = H.g0 + wk / H.nchunks;
        const int c = (int)(wk % H.nchunks);
        int r = 0;
        while (r + 1 < P.R && g >= P.off_t[r + 1]) ++r;
        const int k = (int)(g - P.off_t[r]), T = P.T[r];
        const int e = menv ? P.env_idx[P.tcum[r] + k + 1] : 0;
        const long long i0 = (long long)c * BB_POP_CHUNK, i1 = i0 + BB_POP_CHUNK < nmem ? i0 + BB_POP_CHUNK : nmem;
        const double* Z = F.Z + (long long)P.tcum[r] * ns;      // ln Z (bb_block_rb_logz)
        double* part = H.part + wk * 2 * ns;
        BB_PASS(cx, tid) {
            for (int j = tid; j < ns; j += BB_SCORE_NT) {
                double SP = 0.0, SN = 0.0;
                const double wn = i0 < nn ? exp(-2.0 * bb_ppc_param(P, P.lo_lspop + g, j)) : 0.0;
                for (long long i = i0; i < i1; ++i) {
                    int t = k;
                    long long b = i;
                    if (i < nn && H.neu_t) { t = H.neu_t[g * nn + i]; b = H.neu_b[g * nn + i]; }
                    const long long ll = F.off_l[r] + b * T + t;
                    const double l0 = bb_ppc_param(P, ll, j), l1 = bb_ppc_param(P, ll + 1, j);
                    const double gam = (l1 - l0) - (Z[(long long)(t + 1) * ns + j] - Z[(long long)t * ns + j]);
                    if (i < nn) {
                        SP += wn;
                        SN += -(wn * gam);
                    } else {
                        const long long m = i - nn, em = e + (long long)E * m, u = em + (long long)E * P.nb * r;
                        double s, ls;
                        if (!hier) {
                            s = bb_ppc_param(P, P.lo_s + em, j);
                            ls = bb_ppc_param(P, P.lo_ls + em, j);
                        } else {
                            const long long th = P.kind == 2 ? P.geno_idx[m] : em, uu = P.kind == 2 ? m : u;
                            const double tau = exp(bb_ppc_param(P, P.lo_lt + uu, j));
                            s = bb_ppc_param(P, P.lo_s + th, j) + tau * bb_ppc_param(P, P.lo_tt + uu, j);
                            ls = bb_ppc_param(P, P.lo_ls + uu, j);
                        }
                        const double w = exp(-2.0 * ls);
                        SP += w;
                        SN += w * (s - gam);
                    }
                }
                part[j] = SP;
                part[ns + j] = SN;
            }
        }
    }
}

BB_DEV void bb_block_pop(BBCtx& cx, const PopArgs& H, int nblocks) {
    const RbArgs& A = H.A;
    const PpcArgs& P = A.F.P;
    const int ns = P.n_samples;
    double* mj = cx.lds;
    double* sdj = cx.lds + ns;
    double* red = cx.lds + 2 * (long long)ns;
    double* st = red + 3 * BB_SCORE_NT;
    double* sj = A.ytab + (long long)cx.block * ns;
    for (long long g = H.g0 + cx.block; g < H.g1; g += nblocks) {
        const double* part = H.part + (g - H.g0) * H.nchunks * 2 * ns;
        const double a = P.pri_mean_e ? P.pri_mean_e[g] : P.pri_mean, ib2 = P.pri_ivar_e ? P.pri_ivar_e[g] : P.pri_ivar;
        bb_rb_mixture(cx, ns, A.nq, A.probs, A.threshold, sj, mj, sdj, red, st, A.unit, A.n_units, g, A.quant, [&](int j, double& s, double& mm, double& sd) {
            double SP, SN;
            bb_rb_chunk_sum(part, H.nchunks, ns, j, SP, SN);
            const double Pj = ib2 + SP;
            mm = (a * ib2 + SN) / Pj;
            sd = 1.0 / sqrt(Pj);
            s = bb_ppc_param(P, P.lo_spop + g, j);
        });
    }
}
