// bb_chain.h -- chain diagnostics on the device: mean, sd, MCSE, ESS (Geyer's initial monotone sequence), split-R-hat and exact
// quantiles of every column of a host chain[n_chains][n_draws][n_cols] -- what MCMCChains' summarystats / quantile report for the
// chain the reference's mcmc_sample returns (src/mcmc.jl:151-158).  Entry point bb_chain_summary; the per-column definitions are
// the contract in include/barbay_hip.h.
//
// The host array is column-fastest, so a column is strided by n_cols doubles.  Slabs of columns are uploaded as [K][ld] rows
// (K = n_chains n_draws, a 2-D copy) and two block programs run per slab:
//   bb_block_chain_transpose : [K][ld] -> [sc][K] through a 32 x 32 LDS tile (rows padded to 33 doubles); both sides move runs of 32
//                              consecutive doubles, nothing gathers at stride n_cols.
//   bb_block_chain_stats     : one workgroup per column.  The column goes into LDS once (NaNs canonical, as bb_freq.h), then
//       1. bb_ppc_select (bb_ppc.h) takes the order statistics of the raw column;
//       2. pooled mean (a compensated sum: a mean near 0 keeps its digits), the column shifted in place by it, and the corrected
//          two-pass sum of squares (sd), so a column 1e6 + 1e-3 noise keeps its digits and everything after works on small numbers;
//       3. segment statistics (bb_chain_seg) of the 2W half chains: split-R-hat;
//       4. segment statistics of the W chains: Wbar, var+, and the chains centred in place about their own means;
//       5. autocovariances in batches of BB_CHAIN_LAGS lags -- a lag belongs to BB_CHAIN_NT / BB_CHAIN_LAGS lanes, the chains inside --
//          and after each batch the Geyer sum advances; the first batch that holds the truncation is the last one computed.
//     A non-finite or constant column skips 2 .. 5.
// Sums: every reduction adds per-lane partials (strided, ascending) in runs of 16 and the runs in order (bb_chain_gsum), lanes per
// segment chosen from (W, N) and the block size BB_CHAIN_NT alone -- a column's results do not depend on the grid, the slab or its
// neighbours, and there are no atomics on doubles.
// Barrier-separated passes, so the host emulation (BB_EMU) runs the same source.
#pragma once
#include "bb_ppc.h"

#define BB_CHAIN_NT 512                    // threads of the stats program (the reduction orders are defined on it)
#define BB_CHAIN_LAGS 32                   // lags per batch == BB_CHAIN_LAG_BATCH of include/barbay_hip.h
#define BB_CHAIN_TILE 32                   // transpose tile
#define BB_CHAIN_TNT 256                   // threads of the transpose program
#define BB_CHAIN_QSTRIDE 8                 // quantile slots per column on the device == BB_CHAIN_MAX_Q

struct ChainArgs {
    PpcArgs P;                // the select's fields only: K, n_tgt, tgt; n_q = 0 (no bands); plo, gam: per probability, read here
    const double* slab;       // [K][ld] as uploaded: columns c0 .. c0 + sc of the caller's array
    double* colT;             // [sc][K]
    double* stat;             // [5][ld]: mean, sd, mcse, ess, rhat
    double* quant;            // [sc][BB_CHAIN_QSTRIDE]
    int* nlags;               // [sc]
    long long sc, ld;
    int W, N, nq, lag_max;    // lag_max: the last lag the Geyer sum may use, min(N - 1, max_lag)
    double ess_cap;           // K log10(K)
};

// LDS: the select's (bb_ppc_lds_doubles(K)) | scalars [16] | sums [BB_CHAIN_NT].  Outside the select its histogram words
// (BB_PPC_MAX_TGT * BB_PPC_HWORDS / 2 = 4 * BB_CHAIN_NT doubles) are four more arrays of sums.
BB_HD long long bb_chain_lds_doubles(int K) { return bb_ppc_lds_doubles(K) + 16 + BB_CHAIN_NT; }
static_assert(BB_PPC_MAX_TGT * BB_PPC_HWORDS / 2 >= 4 * BB_CHAIN_NT, "the histogram words hold four arrays of sums");
static_assert(BB_CHAIN_NT % BB_CHAIN_LAGS == 0 && BB_CHAIN_LAGS % 2 == 0 && BB_CHAIN_NT / BB_CHAIN_LAGS <= 16, "lag batch");

BB_DEV void bb_block_chain_transpose(BBCtx& cx, const ChainArgs& C, int nblocks) {
    double* tile = cx.lds;                   // [32][33]
    const long long K = C.P.K, tc = (C.sc + BB_CHAIN_TILE - 1) / BB_CHAIN_TILE, tr = (K + BB_CHAIN_TILE - 1) / BB_CHAIN_TILE;
    for (long long t = cx.block; t < tc * tr; t += nblocks) {
        const long long r0 = (t / tc) * BB_CHAIN_TILE, c0 = (t % tc) * BB_CHAIN_TILE;
        BB_PASS(cx, tid) {
            const int x = tid & 31;
            for (int y = tid >> 5; y < BB_CHAIN_TILE; y += cx.nthr >> 5)
                if (r0 + y < K && c0 + x < C.sc) tile[y * 33 + x] = C.slab[(r0 + y) * C.ld + c0 + x];
        }
        BB_SYNC(cx);
        BB_PASS(cx, tid) {
            const int x = tid & 31;
            for (int y = tid >> 5; y < BB_CHAIN_TILE; y += cx.nthr >> 5)
                if (c0 + y < C.sc && r0 + x < K) C.colT[(c0 + y) * K + r0 + x] = tile[x * 33 + y];
        }
        BB_SYNC(cx);
    }
}

// Sums of the G consecutive entries a[g G .. (g + 1) G) of every group g into a[g G] (b, c likewise unless null): runs of 16 in index
// order, then the runs in order.  G a power of two <= nthr.  Ends with a barrier.
BB_DEV void bb_chain_gsum(BBCtx& cx, double* a, double* b, double* c, int G) {
    const int R = G < 16 ? G : 16;
    if (R > 1) {
        BB_PASS(cx, tid) {
            if (tid % R == 0) {
                double s = a[tid];
                for (int i = 1; i < R; ++i) s += a[tid + i];
                a[tid] = s;
                if (b) { s = b[tid]; for (int i = 1; i < R; ++i) s += b[tid + i]; b[tid] = s; }
                if (c) { s = c[tid]; for (int i = 1; i < R; ++i) s += c[tid + i]; c[tid] = s; }
            }
        }
        BB_SYNC(cx);
    }
    if (G > 16) {
        BB_PASS(cx, tid) {
            if (tid % G == 0) {
                double s = a[tid];
                for (int i = 1; i < G / 16; ++i) s += a[tid + 16 * i];
                a[tid] = s;
                if (b) { s = b[tid]; for (int i = 1; i < G / 16; ++i) s += b[tid + 16 * i]; b[tid] = s; }
                if (c) { s = c[tid]; for (int i = 1; i < G / 16; ++i) s += c[tid + 16 * i]; c[tid] = s; }
            }
        }
        BB_SYNC(cx);
    }
}

// a + b = s + (what the rounding of s lost)
BB_DEV void bb_chain_two_sum(double& s, double& e, double b) {
    const double a = s, t = a + b, bb = t - a;
    e += (a - (t - bb)) + (b - bb);
    s = t;
}
// Compensated sum of all nthr entries of a (their lost parts in e) into a[0]: the runs of bb_chain_gsum, every addition's rounding
// error carried along and added back at the end -- a pooled sum that cancels (a mean near 0) keeps its digits.  Ends with a barrier.
BB_DEV void bb_chain_gsum_comp(BBCtx& cx, double* a, double* e) {
    BB_PASS(cx, tid) {
        if (tid % 16 == 0) {
            double s = a[tid], c = e[tid];
            for (int i = 1; i < 16; ++i) { bb_chain_two_sum(s, c, a[tid + i]); c += e[tid + i]; }
            a[tid] = s; e[tid] = c;
        }
    }
    BB_SYNC(cx);
    BB_PASS(cx, tid) {
        if (tid == 0) {
            double s = a[0], c = e[0];
            for (int i = 16; i < cx.nthr; i += 16) { bb_chain_two_sum(s, c, a[i]); c += e[i]; }
            a[0] = s + c;
        }
    }
    BB_SYNC(cx);
}

struct ChainLds {
    double *ra, *rb, *a0, *a1, *a2;    // five arrays of BB_CHAIN_NT sums
    double* st;                        // scalars: 1 mean, 2 sd, 3 Wbar, 4 var+, 5 rhat, 6 sum of P, 7 last P, 8 / 9 segment results
    int* ist;                          // 0 non-finite seen, 1 two different values seen, 2 pairs summed, 3 Geyer sum finished
};

// Segment statistics of the shifted column y: S segments of length L, segment s starting at (s / hs) N + (s % hs) (N - L) (hs = 1: the
// chains, L = N; hs = 2: their halves).  With m_s, v_s the mean and corrected variance of segment s:
//   st[8] = mean_s v_s, st[9] = [S > 1] the variance of the m_s taken with S - 1 (about their mean: one pass is safe, y is centred).
// G lanes share a segment, G the largest power of two <= min(nthr / S, L) (1: a lane takes whole segments, s = tid, tid + nthr, ...).
// centre: y -= m_s in place afterwards.  Ends with a barrier.
BB_DEV void bb_chain_seg(BBCtx& cx, const ChainLds& Y, double* y, int N, int S, int L, int hs, bool centre) {
    int G = 1;
    while (2 * G <= cx.nthr / S && 2 * G <= L) G *= 2;
    if (G == 1) {
        BB_PASS(cx, tid) {
            double w = 0.0, d = 0.0, dd = 0.0;
            for (int s = tid; s < S; s += cx.nthr) {
                double* p = y + (s / hs) * N + (s % hs) * (N - L);
                double sum = 0.0, ss = 0.0;
                for (int n = 0; n < L; ++n) sum += p[n];
                const double m = sum / L;
                for (int n = 0; n < L; ++n) ss += (p[n] - m) * (p[n] - m);
                w += ss / (L - 1);
                d += m;
                dd += m * m;
                if (centre) for (int n = 0; n < L; ++n) p[n] -= m;
            }
            Y.a0[tid] = w; Y.a1[tid] = d; Y.a2[tid] = dd;
        }
        BB_SYNC(cx);
    } else {
        BB_PASS(cx, tid) {
            const int s = tid / G, l = tid % G;
            double sum = 0.0;
            if (s < S) {
                const double* p = y + (s / hs) * N + (s % hs) * (N - L);
                for (int n = l; n < L; n += G) sum += p[n];
            }
            Y.ra[tid] = sum;
        }
        BB_SYNC(cx);
        bb_chain_gsum(cx, Y.ra, nullptr, nullptr, G);
        BB_PASS(cx, tid) {
            const int s = tid / G, l = tid % G;
            double ss = 0.0;
            if (s < S) {
                const double* p = y + (s / hs) * N + (s % hs) * (N - L);
                const double m = Y.ra[s * G] / L;
                for (int n = l; n < L; n += G) ss += (p[n] - m) * (p[n] - m);
            }
            Y.rb[tid] = ss;
        }
        BB_SYNC(cx);
        bb_chain_gsum(cx, Y.rb, nullptr, nullptr, G);
        BB_PASS(cx, tid) {
            const bool own = tid < S;                // thread t collects segment t (S G <= nthr)
            const double m = own ? Y.ra[tid * G] / L : 0.0;
            Y.a0[tid] = own ? Y.rb[tid * G] / (L - 1) : 0.0;
            Y.a1[tid] = m;
            Y.a2[tid] = m * m;
            const int s = tid / G, l = tid % G;
            if (centre && s < S) {
                double* p = y + (s / hs) * N + (s % hs) * (N - L);
                const double ms = Y.ra[s * G] / L;
                for (int n = l; n < L; n += G) p[n] -= ms;
            }
        }
        BB_SYNC(cx);
    }
    bb_chain_gsum(cx, Y.a0, Y.a1, Y.a2, cx.nthr);
    BB_PASS(cx, tid) {
        if (tid == 0) {
            const double dbar = Y.a1[0] / S;
            const double b = S > 1 ? (Y.a2[0] - Y.a1[0] * dbar) / (S - 1) : 0.0;
            Y.st[8] = Y.a0[0] / S;
            Y.st[9] = b > 0.0 ? b : 0.0;
        }
    }
    BB_SYNC(cx);
}

BB_DEV void bb_block_chain_stats(BBCtx& cx, const ChainArgs& C, int nblocks) {
    const PpcArgs& P = C.P;
    const int K = P.K, W = C.W, N = C.N;
    double* col = cx.lds;
    const PpcSel S = bb_ppc_sel(cx.lds, K);
    ChainLds Y;
    Y.ra = (double*)S.hist;
    Y.rb = Y.ra + BB_CHAIN_NT;
    Y.a0 = Y.rb + BB_CHAIN_NT;
    Y.a1 = Y.a0 + BB_CHAIN_NT;
    Y.st = cx.lds + bb_ppc_lds_doubles(K);
    Y.ist = (int*)(Y.st + 12);
    Y.a2 = Y.st + 16;
    const int lpl = cx.nthr / BB_CHAIN_LAGS;         // lanes per lag
    for (long long c = cx.block; c < C.sc; c += nblocks) {
        const double* src = C.colT + c * K;
        BB_PASS(cx, tid) { if (tid < 4) Y.ist[tid] = 0; }
        BB_SYNC(cx);
        BB_PASS(cx, tid) {
            const double x0 = src[0];
            bool nonfin = false, differ = false;
            for (int i = tid; i < K; i += cx.nthr) {
                const double x = bb_freq_canon(src[i]);
                nonfin |= !isfinite(x);
                differ |= x != x0;
                col[i] = x;
            }
            if (nonfin) Y.ist[0] = 1;
            if (differ) Y.ist[1] = 1;
            bb_ppc_select_reset(P, S, tid);
        }
        BB_SYNC(cx);
        const bool nonfin = Y.ist[0] != 0, constant = Y.ist[1] == 0;
        if (C.nq > 0) {
            // the order statistics stay in the select's state; the interpolation of bb_ppc_select's bands, fused on both backends
            bb_ppc_select(cx, P, S, col, nullptr);
            BB_PASS(cx, tid) {
                if (tid < C.nq) C.quant[c * BB_CHAIN_QSTRIDE + tid] = bb_ppc_interp(P, S, tid);
            }
            BB_SYNC(cx);
        }
        if (nonfin || constant) {
            BB_PASS(cx, tid) {
                if (tid == 0) {
                    C.stat[0 * C.ld + c] = nonfin ? (double)NAN : col[0];
                    C.stat[1 * C.ld + c] = nonfin ? (double)NAN : 0.0;
                    C.stat[2 * C.ld + c] = NAN;
                    C.stat[3 * C.ld + c] = NAN;
                    C.stat[4 * C.ld + c] = NAN;
                    C.nlags[c] = 0;
                }
            }
            BB_SYNC(cx);
            continue;
        }
        // pooled mean; the column shifted by it; corrected two-pass sum of squares
        BB_PASS(cx, tid) {
            double s = 0.0, e = 0.0;
            for (int i = tid; i < K; i += cx.nthr) bb_chain_two_sum(s, e, col[i]);
            Y.ra[tid] = s;
            Y.rb[tid] = e;
        }
        BB_SYNC(cx);
        bb_chain_gsum_comp(cx, Y.ra, Y.rb);
        BB_PASS(cx, tid) {
            const double sh = Y.ra[0] / K;
            double s = 0.0, ss = 0.0;
            for (int i = tid; i < K; i += cx.nthr) {
                const double v = col[i] - sh;
                col[i] = v;
                s += v;
                ss += v * v;
            }
            Y.a1[tid] = s;
            Y.a0[tid] = ss;
            if (tid == 0) Y.st[1] = sh;
        }
        BB_SYNC(cx);
        bb_chain_gsum(cx, Y.a1, Y.a0, nullptr, cx.nthr);
        BB_PASS(cx, tid) {
            if (tid == 0) {
                const double sy = Y.a1[0], ss = Y.a0[0] - sy * (sy / K);
                Y.st[2] = sqrt((ss > 0.0 ? ss : 0.0) / (K - 1));
            }
        }
        BB_SYNC(cx);
        // split-R-hat: the 2W halves of length N / 2
        bb_chain_seg(cx, Y, col, N, 2 * W, N / 2, 2, false);
        BB_PASS(cx, tid) {
            if (tid == 0) {
                const int L = N / 2;
                const double vp = (double)(L - 1) / L * Y.st[8] + Y.st[9];
                Y.st[5] = sqrt(vp / Y.st[8]);
            }
        }
        BB_SYNC(cx);
        // the W chains: Wbar, var+; chains centred in place
        bb_chain_seg(cx, Y, col, N, W, N, 1, true);
        BB_PASS(cx, tid) {
            if (tid == 0) {
                Y.st[3] = Y.st[8];
                Y.st[4] = (double)(N - 1) / N * Y.st[8] + Y.st[9];
                Y.st[6] = 0.0;
                Y.st[7] = 0.0;
            }
        }
        BB_SYNC(cx);
        // autocovariances in lag batches, the Geyer sum after each
        for (int t0 = 0;; t0 += BB_CHAIN_LAGS) {
            BB_PASS(cx, tid) {
                const int t = t0 + tid / lpl, j = tid % lpl;
                double s = 0.0;
                if (t <= C.lag_max)
                    for (int w = 0; w < W; ++w) {
                        const double* p = col + w * N;
                        for (int n = j; n < N - t; n += lpl) s += p[n] * p[n + t];
                    }
                Y.ra[tid] = s;
            }
            BB_SYNC(cx);
            bb_chain_gsum(cx, Y.ra, nullptr, nullptr, lpl);
            BB_PASS(cx, tid) {
                if (tid == 0) {
                    const double wbar = Y.st[3], vp = Y.st[4], kn = (double)W * N;
                    double sum = Y.st[6], prev = Y.st[7];
                    int np = Y.ist[2], done = 0;
                    for (int q = 0; q < BB_CHAIN_LAGS; q += 2) {
                        const int k = (t0 + q) / 2;
                        if (2 * k + 1 > C.lag_max) { done = 1; break; }
                        const double r0 = 1.0 - (wbar - Y.ra[q * lpl] / kn) / vp, r1 = 1.0 - (wbar - Y.ra[(q + 1) * lpl] / kn) / vp;
                        double pk = r0 + r1;
                        if (!(pk > 0.0)) { done = 1; break; }
                        if (k > 0 && pk > prev) pk = prev;
                        sum += pk;
                        prev = pk;
                        ++np;
                    }
                    if (t0 + BB_CHAIN_LAGS + 1 > C.lag_max) done = 1;
                    Y.st[6] = sum; Y.st[7] = prev;
                    Y.ist[2] = np; Y.ist[3] = done;
                }
            }
            BB_SYNC(cx);
            if (Y.ist[3]) break;
        }
        BB_PASS(cx, tid) {
            if (tid == 0) {
                const double tau = -1.0 + 2.0 * Y.st[6], kn = (double)W * N;
                const double e0 = kn / tau, ess = e0 < C.ess_cap ? e0 : C.ess_cap;
                C.stat[0 * C.ld + c] = Y.st[1];
                C.stat[1 * C.ld + c] = Y.st[2];
                C.stat[2 * C.ld + c] = Y.st[2] / sqrt(ess);
                C.stat[3 * C.ld + c] = ess;
                C.stat[4 * C.ld + c] = Y.st[5];
                C.nlags[c] = 2 * Y.ist[2];
            }
        }
        BB_SYNC(cx);
    }
}
