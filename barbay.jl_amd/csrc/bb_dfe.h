// bb_dfe.h -- posterior of the distribution of fitness effects of a set of units, with the uncertainty its units share, on the device.
// Entry point bb_dfe_rb (include/barbay_hip.h, where the formulas are); no reference counterpart.
//
// Given everything else, distinct fitness units are conditionally independent (bb_contrast.h's fact), each N(m_{u,j}, sd_{u,j}) per
// draw j: bb_fitness_rb's conditional, through bb_contrast_unit.  The number of a set's units below a threshold x is then
// Poisson-binomial given the rest: the fraction below x has conditional mean L_j = mean_u pl_{u,j} and conditional variance
// V_j = sum_u pl_{u,j} pu_{u,j} / n^2.  What moves L_j from draw to draw is what the units share -- sbar_t above all -- and that is
// the part mean-field q's own draws C_j = mean_u [s_{u,j} <= x] do not see.
//
// After the phases every call of bb_rb.h starts with (bb_block_ppc_pop, the normalisers, bb_block_rb_logz), per slab of
// (sets x grid points) whose chunk partials fit the bound of bb_analysis.h:
//   bb_block_dfe_part : one workgroup of BB_DFE_PART_NT threads per (chunk of BB_DFE_CHUNK_UNITS consecutive units of a set, group of
//        BB_DFE_GROUP grid points, tile of BB_DFE_PART_NT draws), work += nblocks; a thread owns one draw.  It walks the chunk's units
//        in the caller's order, a unit's loglambda row once per group (bb_contrast_unit), and adds the unit's pl, pu, pl pu and
//        [s <= x] to the group's (SL, SU, SV, SC), from 0.0, held in registers: the group is a compile-time count (8, and 4 + 2 + 1
//        for what is left of the grid), never an array indexed at run time, which would be scratch memory (bb_rb.h).  A grid point's
//        sums do not read its neighbours', so they do not depend on the group it fell into.  No cross-lane step, no barrier.
//        part[chunk][grid point][4][n_samples].
//   bb_block_dfe      : one workgroup of BB_SCORE_NT threads per (set, grid point), cell += nblocks.  Per draw the set's chunk
//        partials from 0.0 in chunk order; L_j into LDS, (U_j, V_j, C_j) into the block's [3][n_samples] slice of a global table
//        (draw j is always lane j mod NT's); two reductions (sum L, sum U, sum C | centred squares of L and C, sum V) in
//        bb_score_reduce's order; then bb_ppc_select over the column of L_j and, the column refilled, of U_j: ONE column in LDS at a
//        time, which is what keeps the cap at bb_fitness_rb's.  A non-finite sum of L or U: NaN bands (the selection orders NaNs).
// The chunk map (set -> first chunk, chunk -> set) and every check of the sets are the host's (bb_analysis.h); the order of every
// sum is the map's, not the grid's, the slabs' or the groups'.
#pragma once
#include "bb_contrast.h"

#define BB_DFE_CHUNK_UNITS 128             // == BB_DFE_CHUNK of include/barbay_hip.h: units per partial sum of a set
#define BB_DFE_PART_NT 256                 // threads of bb_block_dfe_part = draws of a tile (no result depends on it)
#define BB_DFE_GROUP 8                     // grid points a walk over a unit's row serves (no result depends on it)
#define BB_DFE_OUT 6                       // per-cell results on the device: below_mean, above_mean, between_sd, within_sd, q_below_mean, q_below_sd
#define BB_DFE_SCALARS 16                  // st[]: 0 .. 5 the two reductions, 6 bands wanted and finite
// LDS: one column [n_samples] with the select's state behind it (bb_ppc_lds_doubles(n_samples)) | three arrays of BB_SCORE_NT partials | scalars
#define BB_DFE_SEL_DOUBLES (BB_PPC_MAX_TGT * BB_PPC_HWORDS / 2 + 6 * BB_PPC_MAX_TGT + 8)      // bb_ppc_lds_doubles(K) - K
#define BB_DFE_LDS_DOUBLES(ns, cols) ((long long)(cols) * (ns) + BB_DFE_SEL_DOUBLES + 3 * BB_SCORE_NT + BB_DFE_SCALARS)
// the largest n_samples: the front of the call is bb_fitness_rb's, so never more than its cap; the layout itself, one column at a
// time, would fit 15144.  With L_j and U_j both in LDS it would be 7572.
#define BB_DFE_LDS_FIT(cols) ((160 * 1024 / 8 - BB_DFE_SEL_DOUBLES - 3 * BB_SCORE_NT - BB_DFE_SCALARS) / (cols))
#define BB_DFE_SAMPLES_CAP (BB_DFE_LDS_FIT(1) < BB_RB_SAMPLES_CAP ? BB_DFE_LDS_FIT(1) : BB_RB_SAMPLES_CAP)
static_assert(BB_DFE_LDS_DOUBLES(BB_DFE_LDS_FIT(1), 1) * 8 <= 160 * 1024 && BB_DFE_LDS_DOUBLES(BB_DFE_LDS_FIT(1) + 1, 1) * 8 > 160 * 1024,
              "BB_DFE_LDS_FIT(1) is the largest count whose one-column layout fits");
static_assert(BB_DFE_LDS_FIT(1) == 15144 && BB_DFE_LDS_FIT(2) == 7572 && BB_DFE_SAMPLES_CAP == 8672,
              "one column at a time: bb_fitness_rb's 8672 draws fit (84.1 KiB + 16 KiB of histograms + 24 KiB of partials); two columns would not");
static_assert(BB_DFE_SAMPLES_CAP <= BB_PPC_MAX_K, "the select's 16-bit histogram bins");

struct DfeArgs {
    RbArgs A;                 // F, F.P as for bb_block_rb (pri_*: the s_bc prior as bb_fitness_rb sets it; tgt, plo, gam: per probability,
                              // n_q = 0: the select forms no bands of its own); nq, probs; ytab (F.P.par) [gridDim of k_dfe][3][n_samples]: U_j, V_j, C_j of
                              // the cell being worked; unit, quant, n_steps unused
    const int* set_ptr;       // [n_sets + 1] CSR: the units of set s are set_idx[set_ptr[s] .. set_ptr[s + 1])
    const int* set_idx;       // [n_idx] units of bb_fitness_rb
    const int* set_c0;        // [n_sets + 1] set -> its first chunk
    const int* chk_set;       // [n_chunks] chunk -> its set
    const double* grid;       // [n_grid] thresholds
    double* part;             // [c1 - c0][g1 - g0][4][n_samples] chunk partials (SL, SU, SV, SC) of the slab in flight
    double* cell;             // [BB_DFE_OUT][n_sets n_grid]
    double* bands;            // [2][n_sets n_grid][BB_RB_MAX_Q]: below, above
    long long s0, s1;         // the sets in flight
    int c0, c1;               // ... their chunks: set_c0[s0], set_c0[s1]
    int g0, g1;               // ... and the grid points in flight
    int n_grid;
    long long n_cells;        // n_sets n_grid
};

// G grid points x[0 .. G) of one draw: the units set_idx[x0 .. x1) in order, their sums from 0.0 to part[g][4][ns]
template <int G>
BB_DEV void bb_dfe_part_group(const DfeArgs& D, int x0, int x1, int j, const double* x, double* part) {
    const double rsqrt2 = 0.70710678118654752440;
    const int ns = D.A.F.P.n_samples;
    double SL[G], SU[G], SV[G], SC[G], xg[G];
#pragma unroll
    for (int g = 0; g < G; ++g) { SL[g] = 0.0; SU[g] = 0.0; SV[g] = 0.0; SC[g] = 0.0; xg[g] = x[g]; }
    for (int k = x0; k < x1; ++k) {
        double s, mm, sd;
        bb_contrast_unit(D.A.F, D.set_idx[k], j, s, mm, sd);
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const double v = (mm - xg[g]) / sd * rsqrt2;         // bb_rb_mixture's sweep C
            const double pl = 0.5 * erfc(v), pu = 0.5 * erfc(-v);
            SL[g] += pl;
            SU[g] += pu;
            SV[g] = fma(pl, pu, SV[g]);                          // (fused on both backends)
            SC[g] += s <= xg[g] ? 1.0 : 0.0;
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        double* p = part + (long long)g * 4 * ns;
        p[0] = SL[g];
        p[ns] = SU[g];
        p[2 * (long long)ns] = SV[g];
        p[3 * (long long)ns] = SC[g];
    }
}

BB_DEV void bb_block_dfe_part(BBCtx& cx, const DfeArgs& D, int nblocks) {
    const int ns = D.A.F.P.n_samples, gw = D.g1 - D.g0;
    const int ngrp = (gw + BB_DFE_GROUP - 1) / BB_DFE_GROUP, ntile = (ns + cx.nthr - 1) / cx.nthr;
    const long long nwork = (long long)(D.c1 - D.c0) * ngrp * ntile;
    for (long long wk = cx.block; wk < nwork; wk += nblocks) {
        const int tile = (int)(wk % ntile), grp = (int)(wk / ntile % ngrp);
        const long long c = D.c0 + wk / ntile / ngrp;
        const int set = D.chk_set[c];
        const int x0 = D.set_ptr[set] + (int)(c - D.set_c0[set]) * BB_DFE_CHUNK_UNITS;
        const int x1 = x0 + BB_DFE_CHUNK_UNITS < D.set_ptr[set + 1] ? x0 + BB_DFE_CHUNK_UNITS : D.set_ptr[set + 1];
        const int ga = grp * BB_DFE_GROUP, gb = ga + BB_DFE_GROUP < gw ? ga + BB_DFE_GROUP : gw;
        BB_PASS(cx, tid) {
            const int j = tile * cx.nthr + tid;
            if (j < ns) {
                const double* x = D.grid + D.g0;
                double* part = D.part + (c - D.c0) * gw * 4 * ns + j;
                int g = ga;
                if (gb - g == BB_DFE_GROUP) {
                    bb_dfe_part_group<BB_DFE_GROUP>(D, x0, x1, j, x + g, part + (long long)g * 4 * ns);
                } else {                     // what is left of the grid: 4 + 2 + 1
                    if ((gb - g) & 4) { bb_dfe_part_group<4>(D, x0, x1, j, x + g, part + (long long)g * 4 * ns); g += 4; }
                    if ((gb - g) & 2) { bb_dfe_part_group<2>(D, x0, x1, j, x + g, part + (long long)g * 4 * ns); g += 2; }
                    if ((gb - g) & 1) bb_dfe_part_group<1>(D, x0, x1, j, x + g, part + (long long)g * 4 * ns);
                }
            }
        }
    }
}
static_assert(BB_DFE_GROUP == 8, "bb_block_dfe_part splits what is left of the grid as 4 + 2 + 1");

BB_DEV void bb_block_dfe(BBCtx& cx, const DfeArgs& D, int nblocks) {
    const RbArgs& A = D.A;
    const PpcArgs& P = A.F.P;
    const int ns = P.n_samples, nq = A.nq, gw = D.g1 - D.g0;
    double* col = cx.lds;
    const PpcSel S = bb_ppc_sel(cx.lds, ns);
    double* red = cx.lds + ns + BB_DFE_SEL_DOUBLES;
    double* st = red + 3 * BB_SCORE_NT;
    double* uj = A.ytab + (long long)cx.block * 3 * ns;
    double* vj = uj + ns;
    double* cj = vj + ns;
    const long long ncell = D.n_cells, nwork = (D.s1 - D.s0) * gw;
    for (long long wk = cx.block; wk < nwork; wk += nblocks) {
        const long long set = D.s0 + wk / gw;
        const int gl = (int)(wk % gw), c0 = D.set_c0[set], nc = D.set_c0[set + 1] - c0;
        const long long o = set * D.n_grid + D.g0 + gl;
        const double n = (double)(D.set_ptr[set + 1] - D.set_ptr[set]);
        const long long cstride = (long long)gw * 4 * ns;
        const double* part = D.part + (long long)(c0 - D.c0) * cstride + (long long)gl * 4 * ns;
        // sweep A: the draw's fractions; first moments
        BB_PASS(cx, tid) {
            double a0 = 0.0, a1 = 0.0, a2 = 0.0;
            for (int j = tid; j < ns; j += BB_SCORE_NT) {
                double SL = 0.0, SU = 0.0, SV = 0.0, SC = 0.0;
                for (int c = 0; c < nc; ++c) {
                    const double* p = part + c * cstride + j;
                    SL += p[0];
                    SU += p[ns];
                    SV += p[2 * (long long)ns];
                    SC += p[3 * (long long)ns];
                }
                const double L = SL / n, U = SU / n, C = SC / n;
                col[j] = L;
                uj[j] = U;
                vj[j] = SV / (n * n);
                cj[j] = C;
                a0 += L;
                a1 += U;
                a2 += C;
            }
            red[tid] = a0; red[BB_SCORE_NT + tid] = a1; red[2 * BB_SCORE_NT + tid] = a2;
        }
        BB_SYNC(cx);
        bb_score_reduce(cx, red, st, false);
        // sweep B: centred second moments of L and C; the mean conditional variance
        BB_PASS(cx, tid) {
            const double lm = st[0] / ns, cm = st[2] / ns;
            double a0 = 0.0, a1 = 0.0, a2 = 0.0;
            for (int j = tid; j < ns; j += BB_SCORE_NT) {
                const double dl = col[j] - lm, dc = cj[j] - cm;
                a0 += dl * dl;
                a1 += dc * dc;
                a2 += vj[j];
            }
            red[tid] = a0; red[BB_SCORE_NT + tid] = a1; red[2 * BB_SCORE_NT + tid] = a2;
        }
        BB_SYNC(cx);
        bb_score_reduce(cx, red, st + 3, false);
        BB_PASS(cx, tid) {
            if (tid == 0) {
                D.cell[0 * ncell + o] = st[0] / ns;
                D.cell[1 * ncell + o] = st[1] / ns;
                D.cell[2 * ncell + o] = sqrt(st[3] / ns);
                D.cell[3 * ncell + o] = sqrt(st[5] / ns);
                D.cell[4 * ncell + o] = st[2] / ns;
                D.cell[5 * ncell + o] = sqrt(st[4] / ns);
                st[6] = (nq > 0 && isfinite(st[0]) && isfinite(st[1])) ? 1.0 : 0.0;
            }
            bb_ppc_select_reset(P, S, tid);
        }
        BB_SYNC(cx);
        if (nq > 0 && st[6] == 0.0) {        // a non-finite L_j or U_j
            BB_PASS(cx, tid) {
                if (tid < 2 * nq) D.bands[((tid / nq) * ncell + o) * BB_RB_MAX_Q + tid % nq] = NAN;
            }
        } else if (nq > 0) {
            for (int side = 0; side < 2; ++side) {
                if (side == 1) {             // the column again: U_j
                    BB_PASS(cx, tid) {
                        for (int j = tid; j < ns; j += BB_SCORE_NT) col[j] = uj[j];
                        bb_ppc_select_reset(P, S, tid);
                    }
                    BB_SYNC(cx);
                }
                // the order statistics stay in the select's state; the interpolation is bb_ppc_interp's, as for bb_block_chain_stats
                bb_ppc_select(cx, P, S, col, nullptr);
                BB_PASS(cx, tid) {
                    if (tid < nq) D.bands[(side * ncell + o) * BB_RB_MAX_Q + tid] = bb_ppc_interp(P, S, tid);
                }
                BB_SYNC(cx);
            }
        }
        BB_SYNC(cx);                         // (the next cell's sweep A overwrites what this one read)
    }
}
