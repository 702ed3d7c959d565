// bb_logp.h -- log p(data, z_w) and its gradient for a batch of W points in one call: the service an ensemble HMC / NUTS driver
// asks of the model (bb_logdensity_grad_batch, include/barbay_hip.h).
//
// The log-joint is evaluated directly at the caller's points: nothing is drawn, no softplus, no eps sigma, no entropy term, and
// the handle's variational state is neither read nor written.  The tile map is the two-kernel step's (NB barcodes per tile, n_tiles
// tiles); the grid is 1-D, block = tile + n_tiles * w, and each block runs the block programs of bb_block.h on a view of ITS point:
//   bb_block_logp_moments : stages the point's latents of the tile in LDS, forms the tile's K partial moment rows and its partial
//                           log-joint (prior quadratics, - logsigma_eff terms, Poisson terms; row K - 2) -> part[w][k][tile];
//                           tile 0 also copies the point's global latents to zg[w]
//   bb_block_logp_grad    : adds the point's rows in tile order (bb_finalize_sum: 16 strided sums and one chain above 16 tiles, one
//                           chain otherwise), finishes the global quantities, gathers d log p / d z of the tile's latents -> grad[w];
//                           tile 0 writes the global blocks' gradients and logp[w]
//   bb_block_logp_geno    : genotype model: the theta block -- the per-genotype sums of d log p / d s_eff (bb_block_geno_sum on the
//                           point's ds[w]) minus the prior term, grid = geno blocks * W
// Every sum runs in an order fixed by the model shape and the tile map, no atomics: a point's result does not depend on W, on its
// slot or on the other points.  Barrier-separated passes, so the host emulation (BB_EMU) runs the same source.
#pragma once
#include "bb_block.h"

struct LogpArgs {
    const double* z;          // [W][Dz] the points, the handle's latent order
    double* grad;             // [W][Dz]
    double* logp;             // [W]
    double* part;             // [W][K][nt] partial moment rows
    double* zg;               // [W][2 nt1] global latents of every point (what bb_finalize_sum stages)
    double* ds;               // [W][nbs] genotype model: d log p / d s_eff per mutant
    double* gsum;             // [W][Gs]  ... summed per genotype
    long long Dz, nbs, Gs;    // row strides (even: pairs stay 16-byte aligned)
    int nt, W;                // tiles per point, points
    double c0;                // constant of the log-joint: prior and likelihood normalisers, lgamma terms
    const int* lf_n;          // nullptr (bb_logdensity_grad_batch), or [W] (bb_hmc.h): point w is evaluated only while lf_k < lf_n[w]
    int lf_k;
};

// a point that is not to be evaluated: its blocks leave at once (block-uniform: a block works on one point)
BB_DEV bool bb_logp_idle(const LogpArgs& B, int w) { return B.lf_n && B.lf_k >= B.lf_n[w]; }

// the view of point w's buffers the block programs of bb_block.h take as their state
BB_DEV DevState bb_logp_view(const DevModel& M, const LogpArgs& B, int w) {
    DevState S{};
    S.ztheta = const_cast<double*>(B.z) + (long long)w * B.Dz + M.blk_lo[BK_S];      // (genotype model: theta is read where it lies)
    S.ds = B.ds + (long long)w * B.nbs;
    S.gsum = B.gsum + (long long)w * B.Gs;
    return S;
}

// the pair (i0, i0 + 1) of a point
BB_DEV void bb_logp_load_pair(const double* z, long long i0, bool a0, bool a1, double* z0, double* z1) {
    *z0 = 0.0; *z1 = 0.0;
    if (a0 && a1) { const bb_d2 v = *(const bb_d2*)(z + i0); *z0 = v.x; *z1 = v.y; }
    else if (a0) *z0 = z[i0];
    else *z1 = z[i0 + 1];
}

BB_DEV double bb_logp_prior_quad(const DevModel& M, int blk, long long i, double z) {
    double pm, iv;
    bb_prior_of(M, blk, i - M.blk_lo[blk], &pm, &iv);
    return -0.5 * (z - pm) * (z - pm) * iv;
}

template <int KIND>
BB_DEV void bb_block_logp_moments(BBCtx& cx0, const DevModel& M, const LogpArgs& B, const RunArgs& A, int NB) {
    const int w = cx0.block / B.nt;
    if (bb_logp_idle(B, w)) return;
    BBCtx cx{cx0.nthr, cx0.block - w * B.nt, cx0.lds};
    const BBLds L = bb_lds_layout(M.R, M.E, KIND, M.Ttot, M.nt1, M.K, NB, cx.nthr);
    double* lds = cx.lds;
    const BBTile t = bb_tile(M, A, cx.block, NB);
    const double* z = B.z + (long long)w * B.Dz;
    const DevState S = bb_logp_view(M, B, w);

    BBSeg* sg = (BBSeg*)(lds + L.seg);
    int* li = (int*)(lds + L.misc);
    BB_PASS(cx, tid) {
        if (tid == 0) li[0] = bb_build_segs<KIND>(sg, M, L, t, cx.block == 0);
        for (int k = tid; k < M.K; k += cx.nthr) lds[L.wk + k] = 0.0;
    }
    BB_SYNC(cx);
    // pass S: the tile's latents of the point into LDS, with their prior quadratics (tile 0: the global blocks, and the genotype
    // model's theta block, too)
    BB_PASS(cx, tid) {
        double el = 0.0;
        bb_for_pairs(cx, tid, sg, li[0], [&](const BBSeg& s, long long i0, bool a0, bool a1) {
            double z0, z1;
            bb_logp_load_pair(z, i0, a0, a1, &z0, &z1);
            if (a0) el += bb_logp_prior_quad(M, s.blk, i0, z0);
            if (a1) el += bb_logp_prior_quad(M, s.blk, i0 + 1, z1);
            if (s.kind >= SK_GS) {
                double* zg = B.zg + (long long)w * 2 * M.nt1 + (s.kind == SK_GLS ? M.nt1 : 0);
                if (a0) zg[i0 - s.lo] = z0;
                if (a1) zg[i0 + 1 - s.lo] = z1;
            } else {
                if (a0) lds[s.ldsoff + (i0 - s.lo)] = z0;
                if (a1) lds[s.ldsoff + (i0 + 1 - s.lo)] = z1;
            }
        });
        if (KIND == 2 && cx.block == 0)
            for (long long i = M.blk_lo[BK_S] + tid; i < M.blk_hi[BK_S]; i += cx.nthr) el += bb_logp_prior_quad(M, BK_S, i, z[i]);
        lds[L.acc + BB_NQ * cx.nthr + tid] = el;
    }
    BB_SYNC(cx);
    // pass E: effective fitness / precision per unit, - logsigma_eff per likelihood term
    BB_PASS(cx, tid) {
        const double el = bb_effective_tables<KIND>(cx, tid, M, S, L, t, true);
        lds[L.acc + BB_NQ * cx.nthr + tid] += el;
    }
    BB_SYNC(cx);
    bb_pass_moments<KIND>(cx, M, S, L, t, NB, true);
    bb_row_sum(cx, lds + L.acc + BB_NQ * cx.nthr, cx.nthr, lds + L.part, lds + L.wk + (M.K - 2));
    BB_PASS(cx, tid) {
        double* part = B.part + (long long)w * M.K * B.nt;
        for (int k = tid; k < M.K; k += cx.nthr) part[(long long)k * B.nt + cx.block] = lds[L.wk + k];
    }
    BB_SYNC(cx);
}

template <int KIND>
BB_DEV void bb_block_logp_grad(BBCtx& cx0, const DevModel& M, const LogpArgs& B, const RunArgs& A0, int NB) {
    const int w = cx0.block / B.nt;
    if (bb_logp_idle(B, w)) return;
    BBCtx cx{cx0.nthr, cx0.block - w * B.nt, cx0.lds};
    const BBLds L = bb_lds_layout(M.R, M.E, KIND, M.Ttot, M.nt1, M.K, NB, cx.nthr);
    double* lds = cx.lds;
    const BBTile t = bb_tile(M, A0, cx.block, NB);
    const double* z = B.z + (long long)w * B.Dz;
    double* grad = B.grad + (long long)w * B.Dz;
    const DevState S = bb_logp_view(M, B, w);
    RunArgs A = A0;
    A.red = B.part + (long long)w * M.K * B.nt;       // the point's rows, added in tile order
    A.nred = B.nt;
    A.with_elbo = 1;

    bb_finalize<KIND, false>(cx, M, S, A, L, B.zg + (long long)w * 2 * M.nt1);

    BBSeg* sg = (BBSeg*)(lds + L.seg);
    int* li = (int*)(lds + L.misc);
    BB_PASS(cx, tid) {
        if (tid == 0) li[0] = bb_build_segs<KIND>(sg, M, L, t, cx.block == 0);
    }
    BB_SYNC(cx);
    BB_PASS(cx, tid) {
        bb_for_pairs(cx, tid, sg, li[0], [&](const BBSeg& s, long long i0, bool a0, bool a1) {
            if (s.kind >= SK_GS) return;
            double z0, z1;
            bb_logp_load_pair(z, i0, a0, a1, &z0, &z1);
            if (a0) lds[s.ldsoff + (i0 - s.lo)] = z0;
            if (a1) lds[s.ldsoff + (i0 + 1 - s.lo)] = z1;
        });
    }
    BB_SYNC(cx);
    BB_PASS(cx, tid) { bb_effective_tables<KIND>(cx, tid, M, S, L, t, false); }
    BB_SYNC(cx);
    bb_pass_residuals_units<KIND>(cx, M, S, L, t, NB);
    // pass G: likelihood part from the LDS tables, prior part on the spot
    BB_PASS(cx, tid) {
        bb_for_pairs(cx, tid, sg, li[0], [&](const BBSeg& s, long long i0, bool a0, bool a1) {
            double z0, z1, pm, iv, g0 = 0.0, g1 = 0.0;
            bb_logp_load_pair(z, i0, a0, a1, &z0, &z1);
            const long long blo = M.blk_lo[s.blk];
            if (a0) { bb_prior_of(M, s.blk, i0 - blo, &pm, &iv); g0 = bb_glik<KIND, false>(lds, M, L, t, NB, s, i0 - s.lo, z0) - (z0 - pm) * iv; }
            if (a1) { bb_prior_of(M, s.blk, i0 + 1 - blo, &pm, &iv); g1 = bb_glik<KIND, false>(lds, M, L, t, NB, s, i0 + 1 - s.lo, z1) - (z1 - pm) * iv; }
            if (a0 && a1) *(bb_d2*)(grad + i0) = bb_d2{g0, g1};
            else if (a0) grad[i0] = g0;
            else grad[i0 + 1] = g1;
        });
        if (cx.block == 0 && tid == 0) {
            double v = lds[L.wk + M.K - 2] + lds[L.wk + M.K - 1] + B.c0;
            for (int r = 0; r < M.R; ++r) v += lds[L.misc + 16 + r];
            B.logp[w] = v;
        }
    }
    BB_SYNC(cx);
}

// LDS: nthr doubles (bb_block_geno_sum)
BB_DEV void bb_block_logp_geno(BBCtx& cx0, const DevModel& M, const LogpArgs& B, int gsb) {
    const int w = cx0.block / gsb;
    if (bb_logp_idle(B, w)) return;
    BBCtx cx{cx0.nthr, cx0.block - w * gsb, cx0.lds};
    const double* z = B.z + (long long)w * B.Dz;
    double* grad = B.grad + (long long)w * B.Dz;
    const DevState S = bb_logp_view(M, B, w);
    bb_block_geno_sum(cx, M, S, gsb, 0, M.nb);
    // every thread finishes the genotypes whose sum it has just written
    const int per_block = cx.nthr / 8;
    for (long long g0 = (long long)cx.block * per_block; g0 < M.G; g0 += (long long)gsb * per_block) {
        BB_PASS(cx, tid) {
            const long long g = g0 + tid;
            if (tid < per_block && g < M.G) {
                const long long i = M.blk_lo[BK_S] + g;
                double pm, iv;
                bb_prior_of(M, BK_S, g, &pm, &iv);
                grad[i] = S.gsum[g] - (z[i] - pm) * iv;
            }
        }
    }
}
