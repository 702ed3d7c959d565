// bb_rank.h -- posterior ranks of the fitness units of a set and top-k membership, with the uncertainty the units share, on the device.
// Entry point bb_fitness_rank (include/barbay_hip.h, where the formulas and the order are); no reference counterpart.
//
// A rank is a function of all the fitnesses of a set at once, so it needs joint draws.  Given everything else, distinct fitness units
// are conditionally independent (bb_contrast.h's fact), each exactly N(m_{u,j}, sd_{u,j}): redrawing every unit of draw j from its
// conditional is one exact blocked Gibbs update of the whole fitness block -- the joint draw with the coupling through sbar_t, theta
// and tau back in it, where mean-field q's own s_{u,j} have none.  The sampling counterpart of bb_fitness_rb.
//
// After the phases every call of bb_rb.h starts with (BB_RANK_CONDITIONAL only: bb_block_ppc_pop, the normalisers, bb_block_rb_logz),
// per slab of sets and tile of draws (bb_analysis.h):
//   bb_block_rank_val   : one workgroup of BB_RANK_VAL_NT threads per (BB_RANK_VAL_UNITS consecutive positions of the slab, tile of
//        BB_RANK_VAL_NT draws), work += nblocks; a thread owns one draw and walks the positions in order (bb_contrast_unit, or for
//        BB_RANK_DRAWS the draw's own fitness alone: no normaliser is read).  It writes the 64-bit sort key of the value: -0.0
//        canonicalised, the order-preserving integer of the double complemented (ascending key = descending value), every NaN the
//        all-ones key.  No cross-lane step, no barrier.
//   bb_block_rank_sort  : one workgroup per (run of at most `run` consecutive positions of a set, draw), work += nblocks.  The run's
//        (key, position in the set) pairs into LDS -- keys [run] of 8 bytes, then positions [run] of 4: 96 KiB at BB_RANK_RUN = 8192 --
//        padded to the power of two with (all ones, INT_MAX), which follows every real pair; a bitonic network orders them by
//        (key, position), a strict total order, so the network being unstable does not matter.  A set of one run: rank[position] =
//        index.  A set of several: the sorted keys go back where the run's keys were, the positions beside them.
//   bb_block_rank_merge : (sets of several runs) one workgroup per (run, draw).  An element's rank is its index in its own run plus,
//        for every other run of the set, the number of that run's pairs ordered before it -- runs are consecutive positions, so that
//        is the count of keys <= its own in an earlier run and of keys < its own in a later one: a binary search in the run's sorted keys.
//   bb_block_rank_stats : one workgroup of BB_SCORE_NT threads per position, k += nblocks.  The column of n_samples ranks as doubles
//        in LDS (bb_block_dfe's one-column layout, hence its cap); sum (exact: integers) -> rank_mean; centred squares -> rank_sd;
//        the counts r_j < top[i], three per reduction, -> p_top, all in bb_score_reduce's order; bb_ppc_select + bb_ppc_interp.
// Table layout: a set's keys [draw of the tile][position in the set] -- bb_block_rank_sort and _merge read a run's keys coalesced,
// bb_block_rank_val writes them with the stride of the set; -DBB_RANK_POSITION_MAJOR lays them [position][draw] instead, coalesced
// in bb_block_rank_val and strided in the sort.  Measured (tools/rank_rate.py, profiles/rank_rb/): one set of 49 000 units sorts and
// merges 2.1 ms faster draw-major, at 0.1 ms more for the values; 49 sets of 1 000 differ by 0.16 ms at most the other way.
// The ranks are [position][n_samples] either way: bb_block_rank_stats reads a row.  Ranks are integers fixed by the order: nothing
// here depends on the layout, the run length, the slabs or the grid.
// The run map (set -> first run, run -> set) and every check of the sets are the host's (bb_analysis.h).
#pragma once
#include "bb_dfe.h"

#define BB_RANK_RUN_KEYS 8192               // == BB_RANK_RUN of include/barbay_hip.h: keys one workgroup sorts in LDS
#define BB_RANK_SORT_NT 1024                // threads of bb_block_rank_sort / _merge at most (no result depends on it)
#define BB_RANK_VAL_NT 256                  // threads of bb_block_rank_val = draws of its tile (no result depends on it)
#define BB_RANK_VAL_UNITS 128               // positions a thread of bb_block_rank_val walks (no result depends on it)
#define BB_RANK_TOPS 8                      // == BB_RANK_MAX_TOP
#define BB_STREAM_RANK 0xFFFFFFE3u          // the conditional redraw's normal: N(u, j >> 1, this)
#define BB_RANK_PAD_POS 0x7FFFFFFF
// LDS of the sort: keys [run] | positions [run]
#define BB_RANK_SORT_LDS_DOUBLES(run) ((long long)(run) + (run) / 2)
static_assert(BB_RANK_SORT_LDS_DOUBLES(BB_RANK_RUN_KEYS) * 8 == 96 * 1024, "12 bytes a pair: 96 KiB of the 160 KiB at the full run");
static_assert((BB_RANK_RUN_KEYS & (BB_RANK_RUN_KEYS - 1)) == 0 && BB_RANK_RUN_KEYS >= 2 * BB_RANK_SORT_NT, "a power of two; every thread has a pair to compare");
// LDS of the summaries: bb_block_dfe's one-column layout, so its cap
#define BB_RANK_STATS_LDS_DOUBLES(ns) BB_DFE_LDS_DOUBLES(ns, 1)
#define BB_RANK_SAMPLES_CAP BB_DFE_SAMPLES_CAP
static_assert(BB_RANK_STATS_LDS_DOUBLES(BB_RANK_SAMPLES_CAP) * 8 <= 160 * 1024 && BB_RANK_SAMPLES_CAP == 8672 && BB_RANK_SAMPLES_CAP <= BB_RB_SAMPLES_CAP,
              "one column of ranks beside the select's state and the partials; never more draws than bb_fitness_rb's front takes");
static_assert(BB_RANK_SAMPLES_CAP <= BB_PPC_MAX_K, "the select's 16-bit histogram bins");

struct RankArgs {
    RbArgs A;                 // F, F.P as for bb_block_rb (pri_*: the s_bc prior as bb_fitness_rb sets it; tgt, plo, gam: per probability,
                              // n_q = 0); nq; ytab, unit, quant, n_steps unused
    const int* set_ptr;       // [n_sets + 1] CSR: the positions of set s are [set_ptr[s], set_ptr[s + 1])
    const int* set_idx;       // [n_idx] units of bb_fitness_rb
    const int* set_r0;        // [n_sets + 1] set -> its first run
    const int* run_set;       // [n_runs] run -> its set
    unsigned long long* key;  // the keys of the positions and draws in flight (layout: bb_rank_at)
    int* spos;                // beside a sorted key: its position in the set (sets of several runs)
    int* rank;                // [k1 - k0][n_samples]
    double* unit;             // [2][n_idx]: rank_mean, rank_sd
    double* ptop;             // [n_idx][BB_RANK_TOPS]
    double* quant;            // [n_idx][BB_RB_MAX_Q]
    long long n_idx;
    long long s0, s1;         // the sets in flight
    int k0, k1;               // ... their positions: set_ptr[s0], set_ptr[s1]
    int r0, r1;               // ... their runs: set_r0[s0], set_r0[s1]
    int j0, j1;               // the draws in flight
    int run;                  // the run length: a power of two, 64 .. BB_RANK_RUN_KEYS
    int lds_run;              // pairs the sort's LDS holds: the longest run in flight, padded to the power of two
    int source;               // 0: the conditional redraw, 1: the draws' own fitness
    int n_top;
    int top[BB_RANK_TOPS];
};

// where the key of position k (of n) of the set starting at position sp0, draw j0 + jl, lives
BB_DEV long long bb_rank_at(const RankArgs& R, int sp0, int n, int k, int jl) {
    const int jw = R.j1 - R.j0;
#ifdef BB_RANK_POSITION_MAJOR
    (void)n;
    return ((long long)(sp0 - R.k0) + k) * jw + jl;
#else
    return (long long)(sp0 - R.k0) * jw + (long long)jl * n + k;
#endif
}

// ascending key = the order of include/barbay_hip.h: descending value, -0.0 == +0.0, every NaN last
BB_DEV unsigned long long bb_rank_key(double v) {
    if (v != v) return ~0ull;
    unsigned long long u;
    memcpy(&u, &v, 8);
    if ((u << 1) == 0) u = 0;
    return ~((u >> 63) ? ~u : (u | 0x8000000000000000ull));
}

// s_{u,j} alone, as bb_contrast_unit forms it
BB_DEV double bb_rank_unit_s(const PpcArgs& P, long long u, int j) {
    const int E = P.E;
    const long long m = u / E % P.nb, em = (int)(u % E) + (long long)E * m;
    if (P.kind < 2) return bb_ppc_param(P, P.lo_s + em, j);
    const long long th = P.kind == 2 ? P.geno_idx[m] : em, uu = P.kind == 2 ? m : u;
    const double a = bb_ppc_param(P, P.lo_s + th, j);
    const double tau = exp(bb_ppc_param(P, P.lo_lt + uu, j));
    return a + tau * bb_ppc_param(P, P.lo_tt + uu, j);
}

BB_DEV void bb_block_rank_val(BBCtx& cx, const RankArgs& R, int nblocks) {
    const FreqArgs& F = R.A.F;
    const PpcArgs& P = F.P;
    const int jw = R.j1 - R.j0, npos = R.k1 - R.k0;
    const int ntile = (jw + cx.nthr - 1) / cx.nthr;
    const long long nwork = (long long)((npos + BB_RANK_VAL_UNITS - 1) / BB_RANK_VAL_UNITS) * ntile;
    for (long long wk = cx.block; wk < nwork; wk += nblocks) {
        const int tile = (int)(wk % ntile);
        const int x0 = R.k0 + (int)(wk / ntile) * BB_RANK_VAL_UNITS;
        const int x1 = x0 + BB_RANK_VAL_UNITS < R.k1 ? x0 + BB_RANK_VAL_UNITS : R.k1;
        BB_PASS(cx, tid) {
            const int jl = tile * cx.nthr + tid, j = R.j0 + jl;
            if (jl < jw) {
                long long lo = R.s0, hi = R.s1;           // the set of position x0: the last whose first position is <= x0
                while (hi - lo > 1) {
                    const long long mid = lo + (hi - lo) / 2;
                    if (R.set_ptr[mid] <= x0) lo = mid; else hi = mid;
                }
                long long set = lo;
                for (int k = x0; k < x1; ++k) {
                    while (k >= R.set_ptr[set + 1]) ++set;
                    const long long u = R.set_idx[k];
                    double v;
                    if (R.source == 1) {
                        v = bb_rank_unit_s(P, u, j);
                    } else {
                        double s, mm, sd, n0, n1;
                        bb_contrast_unit(F, u, j, s, mm, sd);
                        bb_normal_pair(P.seed, (unsigned long long)u, (unsigned)(j >> 1), BB_STREAM_RANK, &n0, &n1);
                        v = fma(sd, (j & 1) ? n1 : n0, mm);
                    }
                    const int sp0 = R.set_ptr[set];
                    R.key[bb_rank_at(R, sp0, R.set_ptr[set + 1] - sp0, k - sp0, jl)] = bb_rank_key(v);
                }
            }
        }
    }
}

BB_DEV void bb_block_rank_sort(BBCtx& cx, const RankArgs& R, int nblocks) {
    const int ns = R.A.F.P.n_samples, jw = R.j1 - R.j0;
    unsigned long long* K = (unsigned long long*)cx.lds;
    int* Q = (int*)(K + R.lds_run);
    const long long nwork = (long long)(R.r1 - R.r0) * jw;
    for (long long wk = cx.block; wk < nwork; wk += nblocks) {
        const int jl = (int)(wk % jw), j = R.j0 + jl;
        const int run = R.r0 + (int)(wk / jw), set = R.run_set[run];
        const int sp0 = R.set_ptr[set], n = R.set_ptr[set + 1] - sp0;
        const int a0 = (run - R.set_r0[set]) * R.run;             // the run's first position in the set
        const int len = a0 + R.run < n ? R.run : n - a0;
        const bool single = R.set_r0[set + 1] - R.set_r0[set] == 1;
        int p2 = 2;
        while (p2 < len) p2 <<= 1;
        BB_PASS(cx, tid) {
            for (int x = tid; x < p2; x += cx.nthr) {
                K[x] = x < len ? R.key[bb_rank_at(R, sp0, n, a0 + x, jl)] : ~0ull;
                Q[x] = x < len ? a0 + x : BB_RANK_PAD_POS;
            }
        }
        BB_SYNC(cx);
        for (int kk = 2; kk <= p2; kk <<= 1) {
            for (int jj = kk >> 1; jj > 0; jj >>= 1) {
                BB_PASS(cx, tid) {
                    for (int t = tid; t < p2 / 2; t += cx.nthr) {
                        const int i = ((t & ~(jj - 1)) << 1) | (t & (jj - 1)), l = i | jj;
                        const unsigned long long ka = K[i], kb = K[l];
                        const int pa = Q[i], pb = Q[l];
                        const bool after = ka > kb || (ka == kb && pa > pb);       // the pair at i is ordered after the pair at l
                        if (after == ((i & kk) == 0)) { K[i] = kb; K[l] = ka; Q[i] = pb; Q[l] = pa; }
                    }
                }
                BB_SYNC(cx);
            }
        }
        BB_PASS(cx, tid) {
            for (int x = tid; x < len; x += cx.nthr) {
                if (single) {
                    R.rank[((long long)(sp0 - R.k0) + Q[x]) * ns + j] = x;
                } else {
                    const long long at = bb_rank_at(R, sp0, n, a0 + x, jl);
                    R.key[at] = K[x];
                    R.spos[at] = Q[x];
                }
            }
        }
        BB_SYNC(cx);                         // (the next run's load overwrites what this one read)
    }
}

BB_DEV void bb_block_rank_merge(BBCtx& cx, const RankArgs& R, int nblocks) {
    const int ns = R.A.F.P.n_samples, jw = R.j1 - R.j0;
    const long long nwork = (long long)(R.r1 - R.r0) * jw;
    for (long long wk = cx.block; wk < nwork; wk += nblocks) {
        const int jl = (int)(wk % jw), j = R.j0 + jl;
        const int run = R.r0 + (int)(wk / jw), set = R.run_set[run];
        const int nrun = R.set_r0[set + 1] - R.set_r0[set], mine = run - R.set_r0[set];
        if (nrun == 1) continue;
        const int sp0 = R.set_ptr[set], n = R.set_ptr[set + 1] - sp0;
        const int a0 = mine * R.run, len = a0 + R.run < n ? R.run : n - a0;
        BB_PASS(cx, tid) {
            for (int x = tid; x < len; x += cx.nthr) {
                const long long at = bb_rank_at(R, sp0, n, a0 + x, jl);
                const unsigned long long key = R.key[at];
                int r = x;
                for (int q = 0; q < nrun; ++q) {
                    if (q == mine) continue;
                    const int b0 = q * R.run, bl = b0 + R.run < n ? R.run : n - b0;
                    int lo = 0, hi = bl;       // the first of run q's keys that is > key (an earlier run) or >= key (a later one)
                    while (lo < hi) {
                        const int mid = lo + (hi - lo) / 2;
                        const unsigned long long km = R.key[bb_rank_at(R, sp0, n, b0 + mid, jl)];
                        if (q < mine ? km <= key : km < key) lo = mid + 1; else hi = mid;
                    }
                    r += lo;
                }
                R.rank[((long long)(sp0 - R.k0) + R.spos[at]) * ns + j] = r;
            }
        }
    }
}

BB_DEV void bb_block_rank_stats(BBCtx& cx, const RankArgs& R, int nblocks) {
    const PpcArgs& P = R.A.F.P;
    const int ns = P.n_samples, nq = R.A.nq;
    double* col = cx.lds;
    const PpcSel S = bb_ppc_sel(cx.lds, ns);
    double* red = cx.lds + ns + BB_DFE_SEL_DOUBLES;
    double* st = red + 3 * BB_SCORE_NT;
    for (long long k = R.k0 + cx.block; k < R.k1; k += nblocks) {
        const int* rk = R.rank + (k - R.k0) * ns;
        BB_PASS(cx, tid) {
            double a0 = 0.0;
            for (int j = tid; j < ns; j += BB_SCORE_NT) {
                const double r = (double)rk[j];
                col[j] = r;
                a0 += r;
            }
            red[tid] = a0; red[BB_SCORE_NT + tid] = 0.0; red[2 * BB_SCORE_NT + tid] = 0.0;
            bb_ppc_select_reset(P, S, tid);
        }
        BB_SYNC(cx);
        bb_score_reduce(cx, red, st, false);
        BB_PASS(cx, tid) {
            const double mean = st[0] / ns;
            double a0 = 0.0;
            for (int j = tid; j < ns; j += BB_SCORE_NT) {
                const double d = col[j] - mean;
                a0 += d * d;
            }
            red[tid] = a0; red[BB_SCORE_NT + tid] = 0.0; red[2 * BB_SCORE_NT + tid] = 0.0;
        }
        BB_SYNC(cx);
        bb_score_reduce(cx, red, st + 3, false);
        BB_PASS(cx, tid) {
            if (tid == 0) {
                R.unit[k] = st[0] / ns;
                R.unit[R.n_idx + k] = sqrt(st[3] / ns);
            }
        }
        for (int i0 = 0; i0 < R.n_top; i0 += 3) {        // the counts below top[i0 .. i0 + 3): exact in any order
            BB_PASS(cx, tid) {
                const double t0 = (double)R.top[i0];              // (a list length past n_top: 0, below which no rank lies)
                const double t1 = i0 + 1 < R.n_top ? (double)R.top[i0 + 1] : 0.0, t2 = i0 + 2 < R.n_top ? (double)R.top[i0 + 2] : 0.0;
                double c0 = 0.0, c1 = 0.0, c2 = 0.0;
                for (int j = tid; j < ns; j += BB_SCORE_NT) {
                    const double r = col[j];
                    c0 += r < t0 ? 1.0 : 0.0;
                    c1 += r < t1 ? 1.0 : 0.0;
                    c2 += r < t2 ? 1.0 : 0.0;
                }
                red[tid] = c0; red[BB_SCORE_NT + tid] = c1; red[2 * BB_SCORE_NT + tid] = c2;
            }
            BB_SYNC(cx);
            bb_score_reduce(cx, red, st + 6, false);
            BB_PASS(cx, tid) {
                if (tid < 3 && i0 + tid < R.n_top) R.ptop[k * BB_RANK_TOPS + i0 + tid] = st[6 + tid] / ns;
            }
            BB_SYNC(cx);
        }
        if (nq > 0) {
            // the order statistics stay in the select's state; the interpolation is bb_ppc_interp's, as for bb_block_dfe
            bb_ppc_select(cx, P, S, col, nullptr);
            BB_PASS(cx, tid) {
                if (tid < nq) R.quant[k * BB_RB_MAX_Q + tid] = bb_ppc_interp(P, S, tid);
            }
        }
        BB_SYNC(cx);                         // (the next position's sweep overwrites what this one read)
    }
}
