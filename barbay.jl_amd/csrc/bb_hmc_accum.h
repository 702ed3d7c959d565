// bb_hmc_accum.h -- streaming moments of the HMC session's state (bb_hmc_accum_*, include/barbay_hip.h): what a chain summary and a
// windowed metric adaptation need of the draws, formed where the draws are.
//
// For walker w < W and segment s < S <= BB_HMC_MAX_SEGMENTS the buffer holds two rows of the session's even stride Dz, the handle's latent
// order: the running mean and m2 = the sum of squared deviations of the states added to (w, s) so far, at ((w S + s) 2 + {0, 1}) Dz.  The
// counts n[w][s] are the host's (one per row pair: the same for every latent).
//   k_hmc_accum        one Welford step of every walker the call adds, x = z[w][i], n the new count, inv_n = 1.0 / n from the host:
//                        d = x - mean;  mean = mean + d * inv_n;  m2 = m2 + d * (x - mean)
//                      every product and sum rounded on its own (no contraction: a host restatement is bit-exact).  Reads z, mean, m2,
//                      writes mean, m2: 40 B per latent, 16-byte accesses, the grid and the pairs of k_hmc_kick_drift.  No LDS, no atomics.
//                      The pad entry of an odd D stays 0 / 0 (its z is 0).
//   k_hmc_accum_stats  one thread per pair of latents loops over the live chains c = (w, s), n_c > 0, w ascending then s ascending, twice:
//                        pass 1, each sum onto 0.0 in that order:  sum_c n_c m_c,  sum_c m_c,  sum_c M2_c,  sum_c M2_c / (n_c - 1)
//                                mean = (sum n_c m_c) / K,  mbar = (sum m_c) / C,  within = (sum M2_c / (n_c - 1)) / C
//                        pass 2:  sum_c n_c ((m_c - mean) (m_c - mean)),  sum_c (m_c - mbar) (m_c - mbar)
//                                m2_pooled = (sum M2_c) + the first,  between = the second / (C - 1), 0 for C = 1
//                      again without contraction; the divisions are IEEE.  A latent whose chains all have M2_c = 0 and one and the same mean
//                      is constant: mean = that value, the three other rows 0, exactly.  No cross-lane step: a latent's four results do not
//                      depend on the grid.
// Barrier-separated passes, so the host emulation (BB_EMU) runs the same source.
#pragma once
#include "bb_hmc.h"

#define BB_HMC_MAX_SEGMENTS 8

struct HmcAccSlot { int seg, pad; double inv_n; };      // per call, per walker: the segment it is added to (-1: not added) and 1 / new count
struct HmcAccLive { int row, pad; double n; };          // per stats call, per live chain: w S + s and its count

struct HmcAccArgs {
    double* rows;                     // [W][S][2][Dz] mean | m2
    const HmcAccSlot* slot;           // [W]
    const HmcAccLive* live;           // [C]
    double* out;                      // [4][Dz] mean | m2_pooled | within | between
    int S, C;
    double K;                         // sum of the live counts
};

// grid = chunk + nchunk * walker, BB_HMC_NT threads
BB_DEV void bb_block_hmc_accum(BBCtx& cx, const HmcArgs& H, const HmcAccArgs& A) {
    const int w = cx.block / H.nchunk, chunk = cx.block - w * H.nchunk;
    const int seg = A.slot[w].seg;
    if (seg < 0) return;                                           // (block-uniform)
    const double inv_n = A.slot[w].inv_n;
    const double* z = H.z + (long long)w * H.Dz;
    double* mean = A.rows + ((long long)w * A.S + seg) * 2 * H.Dz;
    double* m2 = mean + H.Dz;
    BB_PASS(cx, tid) {
        bb_hmc_for_pairs(cx, tid, H, chunk, [&](long long i0) {
            const bb_d2 x = *(const bb_d2*)(z + i0);
            bb_d2 m = *(const bb_d2*)(mean + i0), q = *(const bb_d2*)(m2 + i0);
            {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
                const double d0 = x.x - m.x, d1 = x.y - m.y;
                m.x = m.x + d0 * inv_n;
                m.y = m.y + d1 * inv_n;
                q.x = q.x + d0 * (x.x - m.x);
                q.y = q.y + d1 * (x.y - m.y);
            }
            *(bb_d2*)(mean + i0) = m;
            *(bb_d2*)(m2 + i0) = q;
        });
    }
    BB_SYNC(cx);
}

// grid = ceil(Dz / (2 BB_HMC_NT)), BB_HMC_NT threads: thread t of block b takes the pair at 2 (b BB_HMC_NT + t)
BB_DEV void bb_block_hmc_accum_stats(BBCtx& cx, const HmcArgs& H, const HmcAccArgs& A) {
    BB_PASS(cx, tid) {
        const long long i0 = 2 * ((long long)cx.block * cx.nthr + tid);
        if (i0 < H.Dz) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
            const double Cd = (double)A.C;
            bb_d2 snm{0.0, 0.0}, sm{0.0, 0.0}, sq{0.0, 0.0}, sw{0.0, 0.0};
            const bb_d2 first = *(const bb_d2*)(A.rows + (long long)A.live[0].row * 2 * H.Dz + i0);
            bool k0 = true, k1 = true;                             // the latent is constant so far
            for (int c = 0; c < A.C; ++c) {
                const double* mean = A.rows + (long long)A.live[c].row * 2 * H.Dz + i0;
                const double n = A.live[c].n, nm1 = n - 1.0;
                const bb_d2 m = *(const bb_d2*)mean, q = *(const bb_d2*)(mean + H.Dz);
                snm.x = snm.x + n * m.x;  snm.y = snm.y + n * m.y;
                sm.x = sm.x + m.x;        sm.y = sm.y + m.y;
                sq.x = sq.x + q.x;        sq.y = sq.y + q.y;
                sw.x = sw.x + q.x / nm1;  sw.y = sw.y + q.y / nm1;
                k0 = k0 && q.x == 0.0 && m.x == first.x;
                k1 = k1 && q.y == 0.0 && m.y == first.y;
            }
            bb_d2 mu{snm.x / A.K, snm.y / A.K};
            const bb_d2 mbar{sm.x / Cd, sm.y / Cd};
            bb_d2 sp{0.0, 0.0}, sb{0.0, 0.0};
            for (int c = 0; c < A.C; ++c) {
                const double n = A.live[c].n;
                const bb_d2 m = *(const bb_d2*)(A.rows + (long long)A.live[c].row * 2 * H.Dz + i0);
                const double a0 = m.x - mu.x, a1 = m.y - mu.y, b0 = m.x - mbar.x, b1 = m.y - mbar.y;
                sp.x = sp.x + n * (a0 * a0);  sp.y = sp.y + n * (a1 * a1);
                sb.x = sb.x + b0 * b0;        sb.y = sb.y + b1 * b1;
            }
            bb_d2 pooled{sq.x + sp.x, sq.y + sp.y}, within{sw.x / Cd, sw.y / Cd}, between{0.0, 0.0};
            if (A.C > 1) { between.x = sb.x / (Cd - 1.0); between.y = sb.y / (Cd - 1.0); }
            if (k0) { mu.x = first.x; pooled.x = within.x = between.x = 0.0; }
            if (k1) { mu.y = first.y; pooled.y = within.y = between.y = 0.0; }
            *(bb_d2*)(A.out + i0) = mu;
            *(bb_d2*)(A.out + H.Dz + i0) = pooled;
            *(bb_d2*)(A.out + 2 * H.Dz + i0) = within;
            *(bb_d2*)(A.out + 3 * H.Dz + i0) = between;
        }
    }
    BB_SYNC(cx);
}
