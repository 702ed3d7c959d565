// bb_hmc.h -- Hamiltonian Monte Carlo with a diagonal metric and a fixed number of leapfrogs per transition, the state of every
// walker resident on the device (bb_hmc_begin / bb_hmc_step / bb_hmc_get / bb_hmc_end, include/barbay_hip.h).
//
// A session holds, per walker w, rows of the even stride Dz of bb_logp.h in the handle's latent order: the state z, g = d log p / d z
// at z and logp; the proposal z', g'; the momentum r.  inv_mass and 1 / sqrt(inv_mass) are [Dz] tables in the same order.  One
// transition is, on the handle's stream:
//   k_hmc_momentum      r = n * (1 / sqrt(inv_mass)), n = N(caller's index i, transition, BB_HMC_STREAM0 + w); z' = z, g' = g; the chunk
//                       partials of kinetic0
//   per leapfrog k = 0 .. max_w n_leapfrog[w] - 1, for the walkers with k < n_leapfrog[w] (the others' blocks leave at once):
//     k_hmc_kick_drift  r = fma(eps/2, g', r)  (k > 0: twice, the closing half kick of leapfrog k - 1 and the opening one of k, in
//                       registers), z' = fma(eps inv_mass, r, z')
//     k_logp_moments, k_logp_grad (, k_logp_geno) of bb_logp.h on the proposal rows: logp_prop, g' at z'
//     k_hmc_kick_energy walkers with n_leapfrog[w] == k + 1 only: r = fma(eps/2, g', r) and the chunk partials of kinetic1
//   k_hmc_reduce        the chunk partials in chunk order, one wave per walker
//   (the host reads kinetic0, kinetic1, logp_prop: 3 W doubles, decides, writes W flags)
//   k_hmc_keep          z = z', g = g', logp = logp_prop of the accepted walkers
//
// Order of the sums  sum_i inv_mass_i r_i r_i  (i in the handle's latent order): a chunk is BB_HMC_CHUNK consecutive latents.  Thread t of
// the chunk's BB_HMC_NT threads starts at 0.0 and takes the latents 2 t + 2 BB_HMC_NT j and 2 t + 2 BB_HMC_NT j + 1 of the chunk, j = 0, 1, ...,
// in that order, each as acc = fma(inv_mass_i r_i, r_i, acc); the threads' sums are folded by halving, p[t] += p[t + s] for s = BB_HMC_NT / 2,
// ..., 1.  The chunks are then added in chunk order onto 0.0 by one lane, and the total is halved.  No atomics: a walker's sums do not depend
// on the number of walkers, on its slot's neighbours or on the launch.
// Barrier-separated passes, so the host emulation (BB_EMU) runs the same source.
#pragma once
#include "bb_logp.h"

#define BB_HMC_CHUNK 2048
#define BB_HMC_NT 256
#define BB_HMC_STREAM0_DEV 0xFFFFFF00u      // = BB_HMC_STREAM0 of the ABI: walker w draws on stream BB_HMC_STREAM0 + w

struct HmcArgs {
    double *z, *g, *zp, *gp, *r;      // [W][Dz] state, its gradient, proposal, its gradient, momentum
    double *logp;                     // [W] log-joint of the state
    double *scal;                     // [3][Wp] kinetic0 | kinetic1 | logp_prop: what a transition brings back
    const double *inv_mass, *isd;     // [Dz] the metric and 1 / sqrt of it, the handle's order (the pad entry: 1, 0)
    const long long* cidx;            // [D] caller's index of internal latent i; nullptr: identity
    double* kpart;                    // [W][nchunk] chunk partials of the kinetic energy being summed
    const double* eps;                // [W] per-walker step size of this transition
    const int* nleap;                 // [W] ... and number of leapfrogs
    const int* accept;                // [W] the host's decisions (k_hmc_keep)
    long long D, Dz;
    int nchunk, W, Wp;
    unsigned long long seed;
    unsigned transition;
};

// the pairs (i0, i0 + 1) of chunk `chunk` thread `tid` takes, in the order of the sums
template <class F>
BB_DEV void bb_hmc_for_pairs(const BBCtx& cx, int tid, const HmcArgs& H, int chunk, F&& f) {
    const long long lo = (long long)chunk * BB_HMC_CHUNK;
    const long long hi = lo + BB_HMC_CHUNK < H.Dz ? lo + BB_HMC_CHUNK : H.Dz;
    for (long long i0 = lo + 2 * tid; i0 < hi; i0 += 2 * cx.nthr) f(i0);
}

// the threads' partial sums (already in lds[0 .. nthr)) folded by halving -> *out
BB_DEV void bb_hmc_fold(BBCtx& cx, double* out) {
    for (int s = cx.nthr >> 1; s > 0; s >>= 1) {
        BB_PASS(cx, tid) {
            if (tid < s) cx.lds[tid] += cx.lds[tid + s];
        }
        BB_SYNC(cx);
    }
    BB_PASS(cx, tid) {
        if (tid == 0) *out = cx.lds[0];
    }
    BB_SYNC(cx);
}

// grid = chunk + nchunk * walker, BB_HMC_NT threads, LDS: BB_HMC_NT doubles
BB_DEV void bb_block_hmc_momentum(BBCtx& cx, const HmcArgs& H) {
    const int w = cx.block / H.nchunk, chunk = cx.block - w * H.nchunk;
    const long long row = (long long)w * H.Dz;
    const unsigned stream = BB_HMC_STREAM0_DEV + (unsigned)w;
    BB_PASS(cx, tid) {
        double acc = 0.0;
        bb_hmc_for_pairs(cx, tid, H, chunk, [&](long long i0) {
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
            *(bb_d2*)(H.r + row + i0) = r;
            *(bb_d2*)(H.zp + row + i0) = *(const bb_d2*)(H.z + row + i0);
            *(bb_d2*)(H.gp + row + i0) = *(const bb_d2*)(H.g + row + i0);
        });
        cx.lds[tid] = acc;
    }
    BB_SYNC(cx);
    bb_hmc_fold(cx, H.kpart + (long long)w * H.nchunk + chunk);
}

// leapfrog k of the walkers that have one: the opening half kick (k > 0: behind the closing one of leapfrog k - 1) and the drift
BB_DEV void bb_block_hmc_kick_drift(BBCtx& cx, const HmcArgs& H, int k) {
    const int w = cx.block / H.nchunk, chunk = cx.block - w * H.nchunk;
    if (k >= H.nleap[w]) return;                                   // (block-uniform)
    const long long row = (long long)w * H.Dz;
    const double eps = H.eps[w], half = 0.5 * eps;
    BB_PASS(cx, tid) {
        bb_hmc_for_pairs(cx, tid, H, chunk, [&](long long i0) {
            const bb_d2 g = *(const bb_d2*)(H.gp + row + i0), im = *(const bb_d2*)(H.inv_mass + i0);
            bb_d2 r = *(const bb_d2*)(H.r + row + i0), z = *(const bb_d2*)(H.zp + row + i0);
            if (k > 0) { r.x = fma(half, g.x, r.x); r.y = fma(half, g.y, r.y); }
            r.x = fma(half, g.x, r.x);
            r.y = fma(half, g.y, r.y);
            z.x = fma(eps * im.x, r.x, z.x);
            z.y = fma(eps * im.y, r.y, z.y);
            *(bb_d2*)(H.r + row + i0) = r;
            *(bb_d2*)(H.zp + row + i0) = z;
        });
    }
    BB_SYNC(cx);
}

// the walkers whose last leapfrog was k: the closing half kick and the chunk partials of kinetic1.  LDS: BB_HMC_NT doubles
BB_DEV void bb_block_hmc_kick_energy(BBCtx& cx, const HmcArgs& H, int k) {
    const int w = cx.block / H.nchunk, chunk = cx.block - w * H.nchunk;
    if (H.nleap[w] != k + 1) return;                               // (block-uniform)
    const long long row = (long long)w * H.Dz;
    const double half = 0.5 * H.eps[w];
    BB_PASS(cx, tid) {
        double acc = 0.0;
        bb_hmc_for_pairs(cx, tid, H, chunk, [&](long long i0) {
            const bb_d2 g = *(const bb_d2*)(H.gp + row + i0), im = *(const bb_d2*)(H.inv_mass + i0);
            bb_d2 r = *(const bb_d2*)(H.r + row + i0);
            r.x = fma(half, g.x, r.x);
            r.y = fma(half, g.y, r.y);
            acc = fma(im.x * r.x, r.x, acc);
            acc = fma(im.y * r.y, r.y, acc);
        });
        cx.lds[tid] = acc;
    }
    BB_SYNC(cx);
    bb_hmc_fold(cx, H.kpart + (long long)w * H.nchunk + chunk);
}

// grid = walkers, one wave: 0.5 * (the chunk partials in chunk order) -> scal[which][w].  k >= 0: the walkers whose last leapfrog was k
// only.  LDS: 64 doubles
BB_DEV void bb_block_hmc_reduce(BBCtx& cx, const HmcArgs& H, int which, int k) {
    const int w = cx.block;
    if (k >= 0 && H.nleap[w] != k + 1) return;
    const double* part = H.kpart + (long long)w * H.nchunk;
    double acc = 0.0;                                              // (thread 0's alone is used)
    for (int c0 = 0; c0 < H.nchunk; c0 += cx.nthr) {
        BB_PASS(cx, tid) {
            if (c0 + tid < H.nchunk) cx.lds[tid] = part[c0 + tid];
        }
        BB_SYNC(cx);
        const int n = H.nchunk - c0 < cx.nthr ? H.nchunk - c0 : cx.nthr;
        for (int c = 0; c < n; ++c) acc += cx.lds[c];
        BB_SYNC(cx);
    }
    BB_PASS(cx, tid) {
        if (tid == 0) H.scal[(long long)which * H.Wp + w] = 0.5 * acc;
    }
    BB_SYNC(cx);
}

// the accepted walkers take their proposal
BB_DEV void bb_block_hmc_keep(BBCtx& cx, const HmcArgs& H) {
    const int w = cx.block / H.nchunk, chunk = cx.block - w * H.nchunk;
    if (!H.accept[w]) return;                                      // (block-uniform)
    const long long row = (long long)w * H.Dz;
    BB_PASS(cx, tid) {
        bb_hmc_for_pairs(cx, tid, H, chunk, [&](long long i0) {
            *(bb_d2*)(H.z + row + i0) = *(const bb_d2*)(H.zp + row + i0);
            *(bb_d2*)(H.g + row + i0) = *(const bb_d2*)(H.gp + row + i0);
        });
        if (chunk == 0 && tid == 0) H.logp[w] = H.scal[2ll * H.Wp + w];
    }
    BB_SYNC(cx);
}
