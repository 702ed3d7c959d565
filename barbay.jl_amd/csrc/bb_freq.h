// bb_freq.h -- posterior predictive bands of the frequency TRAJECTORIES on the device (BarBay.stats.freq_bc_ppc, src/stats.jl:152-213,
// followed by matrix_quantile_range), and the posterior bands of the model's returned frequencies F = Lambda ./ sum(Lambda, dims=2)
// (src/model_fitness_normal.jl:209-212).  Entry point bb_freq_bands (include/barbay_hip.h).
//
// Rows: row = r B + b, b the data column (neutrals first, then the mutants in the caller's order); columns: the time points.
// A sample j < n_samples is the joint posterior draw of bb_ppc.h (same keying, BB_STREAM_PPC_PARAM).  Frequency of a draw:
//   F_{r,t,b,j} = exp(ll_{r,t,b,j}) / Z_{r,t,j},   Z_{r,t,j} = sum_{b' < B} exp(ll_{r,t,b',j})
//   BB_FREQ_POSTERIOR  : column t holds the n_samples values F_{r,t,b,j}
//   BB_FREQ_TRAJECTORY : column 0 holds f_0[k'] = F_{r,0,b,j}, k' = j n_ppc + k; column t + 1 is
//                        f_{t+1}[k'] = f_t[k'] exp(mu_j + sd_j N(row | t << 32, k' >> 1, BB_STREAM_FREQ_PRED)), the product carried in f;
//                        neutral row: mu = -sbar_{r,t}, sd = exp(logsigmabar_{r,t}); mutant row: the (s - sbar, sigma) of bb_block_ppc's row
//
// Three block programs (bb_block_ppc_pop of bb_ppc.h fills the population-mean table first, as it is):
//   bb_block_freq_zpart : partial normalisers.  The B barcodes of a (replicate, time point) are cut into chunks of BB_FREQ_CHUNK = 256
//                         consecutive data columns; one thread sums a chunk's exp(ll) for a pair of samples in index order.
//   bb_block_freq_zsum  : Z = the chunk partials added in chunk order.  The summation order is thus a function of B alone -- not of the
//                         grid, the launch mode or the handle's internal latent order -- and no atomics are involved.
//                         Trajectory mode needs (and fills) only each replicate's t = 0 rows of Z.
//   bb_block_freq       : one workgroup per row, row += nblocks.  The column lives in LDS for the whole row: written from exp(ll) / Z
//                         (every column in posterior mode, column 0 of a trajectory), multiplied in place for the later columns of a
//                         trajectory; after each column bb_ppc_select (bb_ppc.h, shared with bb_block_ppc) reads it and writes the bands.
//                         A trajectory may underflow to +0: a valid key, reported as is.  Where the carried product meets 0 inf (or a
//                         frequency inf / inf) the value is NaN; it is stored as THE positive quiet NaN, whose key orders above +inf on
//                         every platform (numpy's sort order), and the bands' non-finite rule then applies.
// Barrier-separated passes, so the host emulation (BB_EMU) runs the same source.
#pragma once
#include "bb_ppc.h"

#define BB_STREAM_FREQ_PRED 0xFFFFFFE2u
#define BB_FREQ_CHUNK 256                  // barcodes per partial sum of the normaliser
#define BB_FREQ_MODE_TRAJECTORY 0          // == BB_FREQ_TRAJECTORY / BB_FREQ_POSTERIOR of include/barbay_hip.h
#define BB_FREQ_MODE_POSTERIOR 1

struct FreqArgs {
    PpcArgs P;                // as for bb_block_ppc, with n_rows = R B, n_steps = the number of columns (max_r T_r), nb = the mutants
    double* Z;                // [Ttot][n_samples] normalisers, row = tcum[r] + t
    double* zpart;            // [nchunks][z1 - z0][n_samples] chunk partials of the normaliser rows in flight
    long long B, nn;          // data columns, of which neutral
    long long off_l[BB_MAX_REP];   // caller's flat index of loglambda (r, t = 0, b = 0); (r, t, b) sits at off_l[r] + b T_r + t
    int mode, nchunks;
    int nz, z0, z1;           // normaliser rows: nz in all (trajectory: one per replicate, its t = 0; posterior: Ttot), [z0, z1) in flight
};

BB_DEV double bb_freq_canon(double x) { return x != x ? (double)NAN : x; }

// normaliser row i -> its replicate and time point
BB_DEV void bb_freq_zrow(const FreqArgs& F, int i, int* r, int* t) {
    if (F.mode == BB_FREQ_MODE_TRAJECTORY) { *r = i; *t = 0; return; }
    int rr = 0;
    while (rr + 1 < F.P.R && F.P.tcum[rr + 1] <= i) ++rr;
    *r = rr;
    *t = i - F.P.tcum[rr];
}

BB_DEV void bb_block_freq_zpart(BBCtx& cx, const FreqArgs& F, int nblocks) {
    const PpcArgs& P = F.P;
    const int ns = P.n_samples, np2 = (ns + 1) >> 1, nzb = F.z1 - F.z0;
    const long long n = (long long)F.nchunks * nzb * np2;
    BB_PASS(cx, tid) {
        for (long long x = (long long)cx.block * cx.nthr + tid; x < n; x += (long long)nblocks * cx.nthr) {
            const int jp = (int)(x % np2);
            const long long ci = x / np2;
            const int ii = (int)(ci % nzb), c = (int)(ci / nzb);
            int r, t;
            bb_freq_zrow(F, F.z0 + ii, &r, &t);
            const int T = P.T[r];
            const long long b0 = (long long)c * BB_FREQ_CHUNK, b1 = b0 + BB_FREQ_CHUNK < F.B ? b0 + BB_FREQ_CHUNK : F.B;
            double s0 = 0.0, s1 = 0.0;
            if (P.draws) {                   // explicit draws (bb_fitness_rb): the same chunk, the same order
                const int j1 = 2 * jp + 1 < ns ? 2 * jp + 1 : 2 * jp;
                for (long long b = b0; b < b1; ++b) {
                    const long long i = F.off_l[r] + b * T + t;
                    s0 += bb_exp(bb_ppc_param(P, i, 2 * jp));
                    s1 += bb_exp(bb_ppc_param(P, i, j1));
                }
            } else {
                for (long long b = b0; b < b1; ++b) {
                    const long long i = F.off_l[r] + b * T + t;
                    double e0, e1;
                    bb_normal_pair(P.seed, (unsigned long long)i, (unsigned)jp, BB_STREAM_PPC_PARAM, &e0, &e1);
                    const double m = P.mean[i], sg = P.sigma[i];
                    s0 += bb_exp(fma(sg, e0, m));
                    s1 += bb_exp(fma(sg, e1, m));
                }
            }
            double* o = F.zpart + ci * ns;
            o[2 * jp] = s0;
            if (2 * jp + 1 < ns) o[2 * jp + 1] = s1;
        }
    }
}

BB_DEV void bb_block_freq_zsum(BBCtx& cx, const FreqArgs& F, int nblocks) {
    const PpcArgs& P = F.P;
    const int ns = P.n_samples, nzb = F.z1 - F.z0;
    const long long n = (long long)nzb * ns;
    BB_PASS(cx, tid) {
        for (long long x = (long long)cx.block * cx.nthr + tid; x < n; x += (long long)nblocks * cx.nthr) {
            const int ii = (int)(x / ns), j = (int)(x % ns);
            int r, t;
            bb_freq_zrow(F, F.z0 + ii, &r, &t);
            double z = F.zpart[(long long)ii * ns + j];
            for (int c = 1; c < F.nchunks; ++c) z += F.zpart[((long long)c * nzb + ii) * ns + j];
            F.Z[(long long)(P.tcum[r] + t) * ns + j] = z;
        }
    }
}

// LDS: as bb_block_ppc (bb_ppc_lds_doubles(K))
BB_DEV void bb_block_freq(BBCtx& cx, const FreqArgs& F, int nblocks) {
    const PpcArgs& P = F.P;
    double* col = cx.lds;
    const PpcSel S = bb_ppc_sel(cx.lds, P.K);
    const int ns = P.n_samples;
    const bool traj = F.mode == BB_FREQ_MODE_TRAJECTORY;
    double* par = P.par + (long long)cx.block * P.E * 2 * ns;
    for (long long row = cx.block; row < P.n_rows; row += nblocks) {
        const int r = (int)(row / F.B);
        const long long b = row % F.B;
        const bool neu = b < F.nn;
        const int T = P.T[r];
        const long long ll = F.off_l[r] + b * T;
        if (traj && !neu) bb_ppc_row_par(cx, P, par, r, b - F.nn);
        for (int t = 0; t < P.n_steps; ++t) {
            double* out = P.bands + (row * P.n_steps + t) * P.n_q * 2;
            if (t >= T) {                    // ragged replicate: no such time point
                BB_PASS(cx, tid) { if (tid < 2 * P.n_q) out[tid] = NAN; }
                continue;
            }
            if (!traj || t == 0) {
                // pass: the draws' frequencies at time point t, each n_ppc times
                const double* Z = F.Z + (long long)(P.tcum[r] + t) * ns;
                BB_PASS(cx, tid) {
                    for (int j = tid; j < ns; j += cx.nthr) {
                        const double f = bb_freq_canon(bb_exp(bb_ppc_param(P, ll + t, j)) / Z[j]);
                        const int k0 = j * P.n_ppc, k1 = k0 + P.n_ppc;
                        for (int k = k0; k < k1; ++k) col[k] = f;
                    }
                    bb_ppc_select_reset(P, S, tid);
                }
            } else {
                // pass: step t - 1 -> t multiplied into the column; predictive pairs (k' >> 1) cover k' = 2p, 2p + 1
                const int st = t - 1;
                const int e = (P.kind == 1 || P.kind == 4) ? P.env_idx[P.tcum[r] + t] : 0;
                const double* sbar = P.pop + (long long)(2 * (P.off_t[r] + st)) * ns;
                BB_PASS(cx, tid) {
                    const unsigned long long q = (unsigned long long)row | ((unsigned long long)st << 32);
                    for (int j = tid; j < ns; j += cx.nthr) {
                        const double mu = neu ? -sbar[j] : par[(long long)(2 * e) * ns + j] - sbar[j];
                        const double sd = neu ? sbar[ns + j] : par[(long long)(2 * e + 1) * ns + j];
                        const int k0 = j * P.n_ppc, k1 = k0 + P.n_ppc;
                        for (int kk = k0 & ~1; kk < k1; kk += 2) {
                            double a, c;
                            bb_normal_pair(P.seed, q, (unsigned)(kk >> 1), BB_STREAM_FREQ_PRED, &a, &c);
                            if (kk >= k0) col[kk] = bb_freq_canon(col[kk] * bb_exp(fma(sd, a, mu)));
                            if (kk + 1 < k1) col[kk + 1] = bb_freq_canon(col[kk + 1] * bb_exp(fma(sd, c, mu)));
                        }
                    }
                    bb_ppc_select_reset(P, S, tid);
                }
            }
            BB_SYNC(cx);
            bb_ppc_select(cx, P, S, col, out);
        }
    }
}
