// bb_nuts.h -- the D-sized objects of a No-U-Turn tree on the device (bb_nuts_begin / bb_nuts_start / bb_nuts_leaf / bb_nuts_take,
// include/barbay_hip.h): both ends of the trajectory, the U-turn checkpoints, the subtree's and the transition's candidate.  The tree's
// decisions stay with the caller, per walker, on the scalars a leaf brings back.
//
// The rows live beside an open HMC session (bb_hmc.h), in a buffer of their own.  Per walker w, BB_NUTS_ROWS(max_depth) = 10 + 2 max_depth
// rows of the session's even stride Dz, the handle's latent order:
//   0 .. 2   the edge of side -1: z, r, g          3 .. 5   the edge of side +1: z, r, g
//   6, 7     the subtree's candidate: z, g         8, 9     the transition's candidate: z, g
//   10 + 2 k, 11 + 2 k   checkpoint slot k < max_depth: z, r
// The travelling end of the trajectory is the session's proposal rows (zp, gp, r): a leaf's evaluation is bb_hmc_step's, idle walkers
// leaving through LogpArgs.lf_n.  One leaf of the walkers with an op, on the handle's stream:
//   k_nuts_open    source = the edge of side v (the first leaf of a doubling) or the travelling rows; e = v eps:
//                  r = fma(e / 2, g, r), z = fma(e inv_mass, r, z) -> the travelling rows.  Reads z, r, g, writes z, r: 40 B per latent
//   k_logp_moments, k_logp_grad (, k_logp_geno) of bb_logp.h on the travelling rows: logp_leaf, g at z
//   k_nuts_close   r = fma(e / 2, g, r), written back; the chunk partials of sum inv_mass r r and, for each of the op's n_check stored
//                  points (z_c, r_c) -- a checkpoint slot or the opposite edge --, of a = sum (z - z_c) (inv_mass r_c) and
//                  b = sum (z - z_c) (inv_mass r); optionally (z, r) -> one checkpoint slot; on a doubling's last leaf (z, r, g) -> the edge
//                  of side v
//   k_nuts_reduce  the chunk partials in chunk order, one lane per sum; the kinetic energy halved; logp_leaf beside them
//   (the host reads 2 + 2 (max_depth + 1) doubles per walker and decides)
// and k_nuts_take copies leaf -> subtree candidate -> transition candidate -> the session's state as the caller's flags say.
//
// Order of the sums: bb_hmc.h's.  A chunk is BB_HMC_CHUNK consecutive latents; thread t starts every sum at 0.0 and takes the pairs
// 2 t + 2 BB_HMC_NT j, j = 0, 1, ..., the even latent then the odd one, as acc = fma(x, y, acc) with
//   kinetic: x = inv_mass_i r_i, y = r_i       a: x = z_i - z_c,i, y = inv_mass_i r_c,i       b: x = z_i - z_c,i, y = inv_mass_i r_i
// (the difference and the product each rounded on their own); the threads' sums are folded by halving, the chunks added in chunk order
// onto 0.0.  No atomics: a walker's sums do not depend on the number of walkers, on its slot's neighbours or on the launch.
// Barrier-separated passes, so the host emulation (BB_EMU) runs the same source.
#pragma once
#include "bb_hmc.h"

#define BB_NUTS_MAX_DEPTH_DEV 10                     // = BB_NUTS_MAX_DEPTH of the ABI
#define BB_NUTS_EDGE_OPP_DEV (-2)                    // = BB_NUTS_EDGE_OPP: a check against the edge of side -v
#define BB_NUTS_PAIRS (BB_HMC_CHUNK / (2 * BB_HMC_NT))      // pairs of latents a thread holds of its chunk
#define BB_NUTS_TAKE_LEAF 1                          // = BB_NUTS_TAKE_* of the ABI
#define BB_NUTS_TAKE_SUB 2
#define BB_NUTS_TAKE_STATE 4

struct NutsOp {                       // one walker's part of a call
    int dir;                          // -1, +1; 0: no part in this call (its blocks leave at once)
    int first, last;                  // the first / last leaf of its doubling
    int store;                        // -1, or the checkpoint slot that takes this leaf's (z, r)
    int n_check;
    int flags;                        // k_nuts_take: BB_NUTS_TAKE_*
    int check[BB_NUTS_MAX_DEPTH_DEV + 2];      // slots, or BB_NUTS_EDGE_OPP_DEV (one entry of padding)
    double eps;
    double logp;                      // k_nuts_take: the log-joint that goes with the transition's candidate
};

struct NutsArgs {
    double* rows;                     // [W][R][Dz]
    double* part;                     // [W][nchunk][NS] chunk partials, sum s: 0 kinetic, 1 + 2 j: a_j, 2 + 2 j: b_j
    double* out;                      // [W][NS + 1]: kinetic | logp_leaf | a_0, b_0, a_1, b_1, ...
    const NutsOp* op;                 // [W]
    int R, NS, max_depth;
};

BB_DEV double* bb_nuts_row(const HmcArgs& H, const NutsArgs& N, int w, int idx) {
    return N.rows + ((long long)w * N.R + idx) * H.Dz;
}
BB_DEV int bb_nuts_edge(int dir) { return dir > 0 ? 3 : 0; }

// grid = chunk + nchunk * walker, BB_HMC_NT threads, LDS: BB_HMC_NT doubles.  bb_block_hmc_momentum's draw and sum; (z, r, g) to both edges
BB_DEV void bb_block_nuts_momentum(BBCtx& cx, const HmcArgs& H, const NutsArgs& N) {
    const int w = cx.block / H.nchunk, chunk = cx.block - w * H.nchunk;
    if (N.op[w].dir == 0) return;                                  // (block-uniform)
    const long long row = (long long)w * H.Dz;
    const unsigned stream = BB_HMC_STREAM0_DEV + (unsigned)w;
    double* const em = bb_nuts_row(H, N, w, 0);
    double* const ep = em + 3 * H.Dz;
    BB_PASS(cx, tid) {
        double acc = 0.0;
        bb_hmc_for_pairs(cx, tid, H, chunk, [&, em, ep](long long i0) {
            double n0, n1 = 0.0, t;
            if (!H.cidx) bb_normal_pair(H.seed, (unsigned long long)(i0 >> 1), H.transition, stream, &n0, &n1);
            else {
                const long long c0 = H.cidx[i0];
                bb_normal_pair(H.seed, (unsigned long long)(c0 >> 1), H.transition, stream, &n0, &t);
                if (c0 & 1) n0 = t;
                if (i0 + 1 < H.D) {
                    const long long c1 = H.cidx[i0 + 1];
                    bb_normal_pair(H.seed, (unsigned long long)(c1 >> 1), H.transition, stream, &t, &n1);
                    if (!(c1 & 1)) n1 = t;
                }
            }
            const bb_d2 sd = *(const bb_d2*)(H.isd + i0), im = *(const bb_d2*)(H.inv_mass + i0);
            const bb_d2 r = bb_d2{n0 * sd.x, n1 * sd.y};          // (the pad entry: isd = 0)
            acc = fma(im.x * r.x, r.x, acc);
            acc = fma(im.y * r.y, r.y, acc);
            const double zx = H.z[row + i0], zy = H.z[row + i0 + 1], gx = H.g[row + i0], gy = H.g[row + i0 + 1];      // (one 16-byte load each)
            *(bb_d2*)(em + i0) = bb_d2{zx, zy};
            *(bb_d2*)(em + H.Dz + i0) = r;
            *(bb_d2*)(em + 2 * H.Dz + i0) = bb_d2{gx, gy};
            *(bb_d2*)(ep + i0) = bb_d2{zx, zy};
            *(bb_d2*)(ep + H.Dz + i0) = r;
            *(bb_d2*)(ep + 2 * H.Dz + i0) = bb_d2{gx, gy};
        });
        cx.lds[tid] = acc;
    }
    BB_SYNC(cx);
    bb_hmc_fold(cx, H.kpart + (long long)w * H.nchunk + chunk);
}

// the opening half kick and the drift of one leaf, from the edge or from the travelling rows, into the travelling rows
BB_DEV void bb_block_nuts_open(BBCtx& cx, const HmcArgs& H, const NutsArgs& N) {
    const int w = cx.block / H.nchunk, chunk = cx.block - w * H.nchunk;
    const int dir = N.op[w].dir;
    if (dir == 0) return;                                          // (block-uniform)
    const long long row = (long long)w * H.Dz;
    const double e = (double)dir * N.op[w].eps, half = 0.5 * e;
    const double* edge = bb_nuts_row(H, N, w, bb_nuts_edge(dir));
    const bool first = N.op[w].first != 0;
    const double *sz = first ? edge : H.zp + row, *sr = first ? edge + H.Dz : H.r + row, *sg = first ? edge + 2 * H.Dz : H.gp + row;
    BB_PASS(cx, tid) {
        bb_hmc_for_pairs(cx, tid, H, chunk, [&](long long i0) {
            const bb_d2 g = *(const bb_d2*)(sg + i0), im = *(const bb_d2*)(H.inv_mass + i0);
            bb_d2 r = *(const bb_d2*)(sr + i0), z = *(const bb_d2*)(sz + i0);
            r.x = fma(half, g.x, r.x);
            r.y = fma(half, g.y, r.y);
            z.x = fma(e * im.x, r.x, z.x);
            z.y = fma(e * im.y, r.y, z.y);
            *(bb_d2*)(H.r + row + i0) = r;
            *(bb_d2*)(H.zp + row + i0) = z;
        });
    }
    BB_SYNC(cx);
}

// ns sums of the threads (lds[s * nthr + tid]) folded by halving, each as bb_hmc_fold folds one -> out[0 .. ns)
BB_DEV void bb_nuts_fold(BBCtx& cx, int ns, double* out) {
    for (int s = cx.nthr >> 1; s > 0; s >>= 1) {
        BB_PASS(cx, tid) {
            if (tid < s)
                for (int q = 0; q < ns; ++q) cx.lds[q * cx.nthr + tid] += cx.lds[q * cx.nthr + tid + s];
        }
        BB_SYNC(cx);
    }
    BB_PASS(cx, tid) {
        if (tid < ns) out[tid] = cx.lds[tid * cx.nthr];
    }
    BB_SYNC(cx);
}

// the closing half kick of one leaf, its energy and U-turn sums, its stores.  LDS: (1 + 2 n_check) * BB_HMC_NT doubles, n_check the
// largest of the call.  A thread keeps its BB_NUTS_PAIRS pairs of (z, r, inv_mass r) in registers and walks the op's stored points.
BB_DEV void bb_block_nuts_close(BBCtx& cx, const HmcArgs& H, const NutsArgs& N) {
    const int w = cx.block / H.nchunk, chunk = cx.block - w * H.nchunk;
    const NutsOp& op = N.op[w];
    const int dir = op.dir;
    if (dir == 0) return;                                          // (block-uniform)
    const long long row = (long long)w * H.Dz;
    const double half = 0.5 * ((double)dir * op.eps);
    const int nc = op.n_check, store = op.store;
    const bool last = op.last != 0;
    const long long lo = (long long)chunk * BB_HMC_CHUNK;
    const long long hi = lo + BB_HMC_CHUNK < H.Dz ? lo + BB_HMC_CHUNK : H.Dz;
    double* ck = store >= 0 ? bb_nuts_row(H, N, w, 10 + 2 * store) : nullptr;
    double* edge = bb_nuts_row(H, N, w, bb_nuts_edge(dir));
    BB_PASS(cx, tid) {
        bb_d2 z[BB_NUTS_PAIRS], r[BB_NUTS_PAIRS], m[BB_NUTS_PAIRS], im[BB_NUTS_PAIRS];
        double acc = 0.0;
#pragma unroll
        for (int q = 0; q < BB_NUTS_PAIRS; ++q) {
            const long long i0 = lo + 2 * tid + (long long)q * 2 * BB_HMC_NT;
            if (i0 >= hi) continue;
            const bb_d2 g = *(const bb_d2*)(H.gp + row + i0);
            im[q] = *(const bb_d2*)(H.inv_mass + i0);
            z[q] = *(const bb_d2*)(H.zp + row + i0);
            r[q] = *(const bb_d2*)(H.r + row + i0);
            r[q].x = fma(half, g.x, r[q].x);
            r[q].y = fma(half, g.y, r[q].y);
            m[q] = bb_d2{im[q].x * r[q].x, im[q].y * r[q].y};
            acc = fma(m[q].x, r[q].x, acc);
            acc = fma(m[q].y, r[q].y, acc);
            *(bb_d2*)(H.r + row + i0) = r[q];
            if (ck) {
                *(bb_d2*)(ck + i0) = z[q];
                *(bb_d2*)(ck + H.Dz + i0) = r[q];
            }
            if (last) {
                *(bb_d2*)(edge + i0) = z[q];
                *(bb_d2*)(edge + H.Dz + i0) = r[q];
                *(bb_d2*)(edge + 2 * H.Dz + i0) = g;
            }
        }
        cx.lds[tid] = acc;
        for (int j = 0; j < nc; ++j) {
            const int c = op.check[j];
            const double* pz = bb_nuts_row(H, N, w, c == BB_NUTS_EDGE_OPP_DEV ? bb_nuts_edge(-dir) : 10 + 2 * c);
            const double* pr = pz + H.Dz;
            double a = 0.0, b = 0.0;
#pragma unroll
            for (int q = 0; q < BB_NUTS_PAIRS; ++q) {
                const long long i0 = lo + 2 * tid + (long long)q * 2 * BB_HMC_NT;
                if (i0 >= hi) continue;
                const bb_d2 zc = *(const bb_d2*)(pz + i0), rc = *(const bb_d2*)(pr + i0);
                const double dx = z[q].x - zc.x, dy = z[q].y - zc.y;
                a = fma(dx, im[q].x * rc.x, a);
                a = fma(dy, im[q].y * rc.y, a);
                b = fma(dx, m[q].x, b);
                b = fma(dy, m[q].y, b);
            }
            cx.lds[(1 + 2 * j) * cx.nthr + tid] = a;
            cx.lds[(2 + 2 * j) * cx.nthr + tid] = b;
        }
    }
    BB_SYNC(cx);
    bb_nuts_fold(cx, 1 + 2 * nc, N.part + ((long long)w * H.nchunk + chunk) * N.NS);
}

// grid = walkers, one wave: lane s adds sum s's chunk partials in chunk order onto 0.0; the kinetic energy is halved; logp_leaf beside them
BB_DEV void bb_block_nuts_reduce(BBCtx& cx, const HmcArgs& H, const NutsArgs& N) {
    const int w = cx.block;
    if (N.op[w].dir == 0) return;
    const int ns = 1 + 2 * N.op[w].n_check;
    const double* part = N.part + (long long)w * H.nchunk * N.NS;
    double* out = N.out + (long long)w * (N.NS + 1);
    BB_PASS(cx, tid) {
        if (tid < ns) {
            double acc = 0.0;
            int c = 0;
            for (; c + 16 <= H.nchunk; c += 16) {                  // (16 loads in flight, then their adds in chunk order)
                double v[16];
#pragma unroll
                for (int q = 0; q < 16; ++q) v[q] = part[(long long)(c + q) * N.NS + tid];
#pragma unroll
                for (int q = 0; q < 16; ++q) acc += v[q];
            }
            for (; c < H.nchunk; ++c) acc += part[(long long)c * N.NS + tid];
            if (tid == 0) {
                out[0] = 0.5 * acc;
                out[1] = H.scal[2ll * H.Wp + w];
            } else out[tid + 1] = acc;
        }
    }
    BB_SYNC(cx);
}

// the copies the caller's flags ask for, in this order: leaf -> subtree candidate, subtree candidate -> transition candidate,
// transition candidate -> the session's state (with the log-joint the caller kept for it)
BB_DEV void bb_block_nuts_take(BBCtx& cx, const HmcArgs& H, const NutsArgs& N) {
    const int w = cx.block / H.nchunk, chunk = cx.block - w * H.nchunk;
    const int f = N.op[w].flags;
    if (f == 0) return;                                            // (block-uniform)
    const long long row = (long long)w * H.Dz;
    double *sub = bb_nuts_row(H, N, w, 6), *cand = bb_nuts_row(H, N, w, 8);
    BB_PASS(cx, tid) {
        bb_hmc_for_pairs(cx, tid, H, chunk, [&](long long i0) {
            bb_d2 z, g;
            if (f & BB_NUTS_TAKE_LEAF) {
                z = *(const bb_d2*)(H.zp + row + i0);
                g = *(const bb_d2*)(H.gp + row + i0);
                *(bb_d2*)(sub + i0) = z;
                *(bb_d2*)(sub + H.Dz + i0) = g;
            }
            if (f & BB_NUTS_TAKE_SUB) {
                if (!(f & BB_NUTS_TAKE_LEAF)) {
                    z = *(const bb_d2*)(sub + i0);
                    g = *(const bb_d2*)(sub + H.Dz + i0);
                }
                *(bb_d2*)(cand + i0) = z;
                *(bb_d2*)(cand + H.Dz + i0) = g;
            }
            if (f & BB_NUTS_TAKE_STATE) {
                if (!(f & BB_NUTS_TAKE_SUB)) {
                    z = *(const bb_d2*)(cand + i0);
                    g = *(const bb_d2*)(cand + H.Dz + i0);
                }
                *(bb_d2*)(H.z + row + i0) = z;
                *(bb_d2*)(H.g + row + i0) = g;
            }
        });
        if ((f & BB_NUTS_TAKE_STATE) && chunk == 0 && tid == 0) H.logp[w] = N.op[w].logp;
    }
    BB_SYNC(cx);
}
