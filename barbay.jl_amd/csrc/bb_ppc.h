// bb_ppc.h -- posterior predictive bands of the log-frequency ratios on the device (BarBay.stats.logfreq_ratio_popmean_ppc /
// logfreq_ratio_bc_ppc / logfreq_ratio_multienv_ppc followed by matrix_quantile_range, src/stats.jl:55-1000).
//
// Rows (caller order): r < R the population-mean row of replicate r, predictive N(-sbar_t, exp(logsigmabar_t)); R + r nb + m mutant m
// in replicate r, predictive N(s_{m,r,env(t+1)} - sbar_t, exp(logsigma_{m,r,env(t+1)})).  A sample j < n_samples is one joint draw
// from the mean-field posterior N(mean, sigma) (caller's flat layout); every sample gets n_ppc predictive draws per (row, step), so a
// (row, step) column holds K = n_samples n_ppc values.  Keying (include/barbay_hip.h, bb_ppc_bands):
//   parameter draw j of latent i : bb_normal_pair(seed, i, j >> 1, BB_STREAM_PPC_PARAM), cosine branch for even j, sine for odd
//   predictive draw k' = j n_ppc + k of (row, t) : bb_normal_pair(seed, row | t << 32, k' >> 1, BB_STREAM_PPC_PRED), same branches
//
// Two block programs:
//   bb_block_ppc_pop : the population-mean draws sbar_{g,j}, exp(logsigmabar_{g,j}) once per call into a [nt1][2][n_samples] table
//                      (every row of a replicate reads them);
//   bb_block_ppc     : one workgroup per row.  Per row the per-sample (s_j, sigma_j) of every environment go once into the block's
//                      slice of a global scratch table; per step the K draws go into LDS and the order statistics the quantiles need
//                      are SELECTED, not sorted: a radix select over the order-preserving 64-bit key, 8-bit digits from the top, one
//                      LDS histogram (16-bit bins, two per word) per distinct prefix among the targets -- all targets resolve in the same
//                      passes; a target whose bucket holds one element is fetched by one more pass.  Quantiles as StatsBase.quantile
//                      (type 7): h = (K - 1) p, a + gamma (b - a) between the order statistics floor(h), floor(h) + 1.
// The selection (bb_ppc_select) and the row's parameter table (bb_ppc_row_par) are functions of their own: bb_block_freq (bb_freq.h) calls them too.
// Written as barrier-separated passes like the step programs, so the host emulation (BB_EMU) runs the same source.
#pragma once
#include "bb_block.h"

#define BB_STREAM_PPC_PARAM 0xFFFFFFE0u
#define BB_STREAM_PPC_PRED 0xFFFFFFE1u
#define BB_PPC_MAX_K 16384
#define BB_PPC_MAX_Q 8
#define BB_PPC_MAX_TGT (4 * BB_PPC_MAX_Q)          // order statistics one column needs at most
#define BB_PPC_HWORDS 128                          // histogram words per prefix group: 256 bins of 16 bits

#ifdef BB_EMU
#define BB_LDS_ADD_U32(p, v) (*(p) += (v))
#else
#define BB_LDS_ADD_U32(p, v) atomicAdd((p), (v))
#endif

struct PpcArgs {
    const double* mean;       // [D] posterior mean / sigma, CALLER's flat order
    const double* sigma;
    double* pop;              // [nt1][2][n_samples]: sbar draw, exp(logsigmabar draw)
    double* par;              // [gridDim][E][2][n_samples] per-block scratch: s_j, exp(logsigma_j) of the row being worked
    double* bands;            // [n_rows][n_steps][n_q][2]
    const int* env_idx;       // [Ttot] (multienv kinds) or nullptr
    const int* geno_idx;      // [nb] caller order (genotype model) or nullptr
    long long n_rows, nb;
    long long lo_spop, lo_lspop, lo_s, lo_tt, lo_lt, lo_ls;   // caller offsets of the blocks (lo_tt / lo_lt: hierarchical kinds)
    int kind, R, E, nt1, n_steps, n_samples, n_ppc, K, n_q, n_tgt;
    int T[BB_MAX_REP], off_t[BB_MAX_REP], tcum[BB_MAX_REP];
    int tgt[BB_PPC_MAX_TGT];                 // the distinct order statistics (0-based ranks), ascending
    int plo[2 * BB_PPC_MAX_Q];               // band end e (= 2 qi + upper): index into tgt of its lower order statistic (upper: +1)
    double gam[2 * BB_PPC_MAX_Q];            // ... and its interpolation weight
    unsigned long long seed;
    // bb_fitness_rb / bb_theta_rb / bb_popmean_rb (bb_rb.h) only; all zero in every other call, which then runs exactly as before
    const double* draws;      // [n_samples][D] explicit draws in the caller's order, read in place of the Philox draw; nullptr: none
    long long D;              // ... and their row length
    const double* pri_mean_e; // the call's prior (s_bc; bb_popmean_rb: s_pop), Matrix form (device, caller order = the handle's for the blocks that have one): mean,
    const double* pri_ivar_e; // 1 / std^2; nullptr: the Vector form below
    double pri_mean, pri_ivar;
};

// parameter draw j of the caller's latent i
BB_DEV double bb_ppc_param(const PpcArgs& P, long long i, int j) {
    if (P.draws) return P.draws[(long long)j * P.D + i];      // (a strided read: sample-major rows, as a chain comes)
    double a, b;
    bb_normal_pair(P.seed, (unsigned long long)i, (unsigned)(j >> 1), BB_STREAM_PPC_PARAM, &a, &b);
    return fma(P.sigma[i], (j & 1) ? b : a, P.mean[i]);
}

BB_DEV unsigned long long bb_ppc_key(double x) {
    unsigned long long u;
    memcpy(&u, &x, 8);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
BB_DEV double bb_ppc_unkey(unsigned long long k) {
    const unsigned long long u = (k >> 63) ? (k ^ 0x8000000000000000ull) : ~k;
    double x;
    memcpy(&x, &u, 8);
    return x;
}

BB_DEV void bb_block_ppc_pop(BBCtx& cx, const PpcArgs& P, int nblocks) {
    const long long n = (long long)P.nt1 * P.n_samples;
    BB_PASS(cx, tid) {
        for (long long x = (long long)cx.block * cx.nthr + tid; x < n; x += (long long)nblocks * cx.nthr) {
            const int g = (int)(x / P.n_samples), j = (int)(x % P.n_samples);
            P.pop[((long long)g * 2) * P.n_samples + j] = bb_ppc_param(P, P.lo_spop + g, j);
            P.pop[((long long)g * 2 + 1) * P.n_samples + j] = bb_exp(bb_ppc_param(P, P.lo_lspop + g, j));
        }
    }
}

// LDS: col[K] doubles | hist [BB_PPC_MAX_TGT][BB_PPC_HWORDS] u32 | state (PpcSel)
BB_HD long long bb_ppc_lds_doubles(int K) { return (long long)K + BB_PPC_MAX_TGT * BB_PPC_HWORDS / 2 + 6 * BB_PPC_MAX_TGT + 8; }

// the select's LDS state behind the column
struct PpcSel {
    unsigned* hist;
    unsigned long long* tpre;      // target: key prefix so far
    unsigned long long* gpre;      // group: prefix
    double* tval;                  // target: value once resolved
    int* trank;                    // target: rank inside its prefix bucket
    int* tgrp;                     // target: its group, -1 resolved
    int* tst;                      // target: 0 active, 1 unique in its bucket (fetch), 2 whole key known
    int* tsh;                      // target: shift its prefix ends at
    int* sc;                       // [0] groups, [1] shift of the next digit, [2] all resolved, [3] any fetch
};
BB_DEV PpcSel bb_ppc_sel(double* lds, int K) {
    PpcSel S;
    S.hist = (unsigned*)(lds + K);
    S.tpre = (unsigned long long*)(lds + K + BB_PPC_MAX_TGT * BB_PPC_HWORDS / 2);
    S.gpre = S.tpre + BB_PPC_MAX_TGT;
    S.tval = (double*)(S.gpre + BB_PPC_MAX_TGT);
    S.trank = (int*)(S.tval + BB_PPC_MAX_TGT);
    S.tgrp = S.trank + BB_PPC_MAX_TGT;
    S.tst = S.tgrp + BB_PPC_MAX_TGT;
    S.tsh = S.tst + BB_PPC_MAX_TGT;
    S.sc = S.tsh + BB_PPC_MAX_TGT;
    return S;
}
// start of a column's selection; called by every thread inside the pass that fills the column (the barrier after it is the caller's)
BB_DEV void bb_ppc_select_reset(const PpcArgs& P, const PpcSel& S, int tid) {
    if (tid < P.n_tgt) { S.tpre[tid] = 0; S.trank[tid] = P.tgt[tid]; S.tgrp[tid] = 0; S.tst[tid] = 0; }
    if (tid == 0) { S.gpre[0] = 0; S.sc[0] = 1; S.sc[1] = 56; S.sc[2] = 0; S.sc[3] = 0; }
}

// The band ends out[n_q][2] of the column col[P.K] (LDS; read, never written): the order statistics P.tgt by radix select, then
// StatsBase.quantile's interpolation.  Shared by bb_block_ppc and bb_block_freq (bb_freq.h).  Ends with a barrier.
BB_DEV void bb_ppc_select(BBCtx& cx, const PpcArgs& P, const PpcSel& S, const double* col, double* out) {
    unsigned* hist = S.hist;
    unsigned long long *tpre = S.tpre, *gpre = S.gpre;
    double* tval = S.tval;
    int *trank = S.trank, *tgrp = S.tgrp, *tst = S.tst, *tsh = S.tsh, *sc = S.sc;
#ifdef BB_PPC_DRAW_ONLY
    // diagnostic build (tools/ppc_time.py, the draw-only floor): no selection, the targets read unordered entries
    BB_PASS(cx, tid) { if (tid < P.n_tgt) tval[tid] = col[P.tgt[tid]]; }
    BB_SYNC(cx);
#else
    // radix select, 8-bit digits from the top
    for (;;) {
        const int ng = sc[0], sh = sc[1];
        BB_PASS(cx, tid) { for (int w = tid; w < ng * BB_PPC_HWORDS; w += cx.nthr) hist[w] = 0; }
        BB_SYNC(cx);
        BB_PASS(cx, tid) {
            for (int i = tid; i < P.K; i += cx.nthr) {
                const unsigned long long k = bb_ppc_key(col[i]);
                const unsigned long long pre = sh == 56 ? 0ull : k >> (sh + 8);
                int gi = 0;
                while (gi < ng && gpre[gi] != pre) ++gi;
                if (gi < ng) {
                    const unsigned d = (unsigned)(k >> sh) & 255u;
                    BB_LDS_ADD_U32(&hist[gi * BB_PPC_HWORDS + (d >> 1)], 1u << (16 * (d & 1)));
                }
            }
        }
        BB_SYNC(cx);
        BB_PASS(cx, tid) {
            if (tid < P.n_tgt && tst[tid] == 0) {
                const unsigned* hg = hist + tgrp[tid] * BB_PPC_HWORDS;
                int rk = trank[tid], d = 0;
                unsigned c = 0;
                for (; d < 256; ++d) {
                    c = (hg[d >> 1] >> (16 * (d & 1))) & 0xFFFFu;
                    if (rk < (int)c) break;
                    rk -= (int)c;
                }
                trank[tid] = rk;
                tpre[tid] = (tpre[tid] << 8) | (unsigned long long)d;
                tsh[tid] = sh;
                if (sh == 0) { tst[tid] = 2; tval[tid] = bb_ppc_unkey(tpre[tid]); }
                else if (c == 1) tst[tid] = 1;
            }
        }
        BB_SYNC(cx);
        BB_PASS(cx, tid) {
            if (tid == 0) {
                int n = 0, fetch = 0;
                for (int x = 0; x < P.n_tgt; ++x) {
                    if (tst[x] != 0) { tgrp[x] = -1; fetch |= tst[x] == 1; continue; }
                    int gi = 0;
                    while (gi < n && gpre[gi] != tpre[x]) ++gi;
                    if (gi == n) gpre[n++] = tpre[x];
                    tgrp[x] = gi;
                }
                sc[0] = n; sc[1] = sh - 8; sc[2] = n == 0; sc[3] = fetch;
            }
        }
        BB_SYNC(cx);
        if (sc[2]) break;
    }
    // targets alone in their bucket: the one element with that prefix
    if (sc[3]) {
        BB_PASS(cx, tid) {
            for (int i = tid; i < P.K; i += cx.nthr) {
                const unsigned long long k = bb_ppc_key(col[i]);
                for (int x = 0; x < P.n_tgt; ++x)
                    if (tst[x] == 1 && (k >> tsh[x]) == tpre[x]) tval[x] = col[i];
            }
        }
        BB_SYNC(cx);
    }
#endif
    // band ends: StatsBase.quantile's interpolation between the two order statistics
    BB_PASS(cx, tid) {
        if (tid < 2 * P.n_q) {
            const double a = tval[P.plo[tid]], b = tval[P.plo[tid] + 1], gm = P.gam[tid];
            out[tid] = (isfinite(a) && isfinite(b)) ? a + gm * (b - a) : (1.0 - gm) * a + gm * b;
        }
    }
    BB_SYNC(cx);
}

// Probability e's quantile from the order statistics a selection left in S.tval: StatsBase.quantile's interpolation with the
// product fused on both backends, for the callers that plan per probability and pass bb_ppc_select no `out` (bb_block_chain_stats,
// bb_block_dfe).  bb_ppc_select's own band ends keep a + gamma (b - a) as written above: their bytes are what they were.
BB_DEV double bb_ppc_interp(const PpcArgs& P, const PpcSel& S, int e) {
    const double a = S.tval[P.plo[e]], b = S.tval[P.plo[e] + 1], gm = P.gam[e];
    return (isfinite(a) && isfinite(b)) ? fma(gm, b - a, a) : (1.0 - gm) * a + gm * b;
}

// per-sample parameters (s_j, exp(logsigma_j)) of mutant m in replicate r, every environment, into the block's scratch slice par[E][2][n_samples]
BB_DEV void bb_ppc_row_par(BBCtx& cx, const PpcArgs& P, double* par, int r, long long m) {
    const int ns = P.n_samples, E = P.E;
    BB_PASS(cx, tid) {
        for (int x = tid; x < E * ns; x += cx.nthr) {
            const int e = x / ns, j = x % ns;
            double s, ls;
            if (P.kind == 0) { s = bb_ppc_param(P, P.lo_s + m, j); ls = bb_ppc_param(P, P.lo_ls + m, j); }
            else if (P.kind == 1) { s = bb_ppc_param(P, P.lo_s + e + (long long)E * m, j); ls = bb_ppc_param(P, P.lo_ls + e + (long long)E * m, j); }
            else {
                const long long th = P.kind == 2 ? P.geno_idx[m] : e + (long long)E * m;
                const long long u = P.kind == 2 ? m : e + (long long)E * m + (long long)E * P.nb * r;
                s = bb_ppc_param(P, P.lo_s + th, j) + bb_exp(bb_ppc_param(P, P.lo_lt + u, j)) * bb_ppc_param(P, P.lo_tt + u, j);
                ls = bb_ppc_param(P, P.lo_ls + u, j);
            }
            par[(long long)(2 * e) * ns + j] = s;
            par[(long long)(2 * e + 1) * ns + j] = bb_exp(ls);
        }
    }
    BB_SYNC(cx);
}

BB_DEV void bb_block_ppc(BBCtx& cx, const PpcArgs& P, int nblocks) {
    double* col = cx.lds;
    const PpcSel S = bb_ppc_sel(cx.lds, P.K);
    const int ns = P.n_samples, E = P.E;
    double* par = P.par + (long long)cx.block * E * 2 * ns;
    for (long long row = cx.block; row < P.n_rows; row += nblocks) {
        const bool popr = row < P.R;
        const int r = popr ? (int)row : (int)((row - P.R) / P.nb);
        const long long m = popr ? 0 : (row - P.R) % P.nb;
        if (!popr) bb_ppc_row_par(cx, P, par, r, m);
        for (int t = 0; t < P.n_steps; ++t) {
            double* out = P.bands + (row * P.n_steps + t) * P.n_q * 2;
            if (t >= P.T[r] - 1) {           // ragged replicate: no such step
                BB_PASS(cx, tid) { if (tid < 2 * P.n_q) out[tid] = NAN; }
                continue;
            }
            const int g = P.off_t[r] + t;
            const int e = (P.kind == 1 || P.kind == 4) ? P.env_idx[P.tcum[r] + t + 1] : 0;
            const double* sbar = P.pop + (long long)(2 * g) * ns;
            // pass: the K draws of the column; predictive pairs (k' >> 1) cover k' = 2p, 2p + 1
            BB_PASS(cx, tid) {
                const unsigned long long q = (unsigned long long)row | ((unsigned long long)t << 32);
                for (int j = tid; j < ns; j += cx.nthr) {
                    const double mu = popr ? -sbar[j] : par[(long long)(2 * e) * ns + j] - sbar[j];
                    const double sd = popr ? sbar[ns + j] : par[(long long)(2 * e + 1) * ns + j];
                    const int k0 = j * P.n_ppc, k1 = k0 + P.n_ppc;
                    for (int kk = k0 & ~1; kk < k1; kk += 2) {
                        double a, b;
                        bb_normal_pair(P.seed, q, (unsigned)(kk >> 1), BB_STREAM_PPC_PRED, &a, &b);
                        if (kk >= k0) col[kk] = fma(sd, a, mu);
                        if (kk + 1 < k1) col[kk + 1] = fma(sd, b, mu);
                    }
                }
                bb_ppc_select_reset(P, S, tid);
            }
            BB_SYNC(cx);
            bb_ppc_select(cx, P, S, col, out);
        }
    }
}
