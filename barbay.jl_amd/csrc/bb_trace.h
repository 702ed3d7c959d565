// bb_trace.h -- the convergence monitor's device side: the optimiser's iterates kept as a chain in a device ring and judged where
// they lie.  Entry points bb_trace_begin / bb_trace_end / bb_trace_count / bb_trace_get / bb_trace_summary and bb_run under a
// trace; the contract is in include/barbay_hip.h.
//
// The ring is [capacity][2 D] doubles, row s mod capacity holding snapshot s = (mu | omega) in the handle's internal order: a row is
// the 2 D columns of bb_trace_summary as they are worked on.  Three block programs:
//   bb_block_trace_snapshot : (mu, omega) -> one ring row, on the handle's stream behind the step that ends a trace interval.
//   bb_block_trace_gather   : the window's K rows (they may straddle the wrap), columns c0 .. c0 + sc -> the [K][ld] slab that
//                             bb_block_chain_transpose reads; it stands where bb_chain_summary uploads.  Both sides move runs of
//                             consecutive doubles.
//   bb_block_trace_verdict  : one workgroup per (layout block, part): integer counts and max / min over the block's contiguous internal
//                             range of the per-column statistics -- no order matters, no atomics.
// Barrier-separated passes, so the host emulation (BB_EMU) runs the same source.
#pragma once
#include "bb_chain.h"

#define BB_TRACE_NT 256                    // threads of the snapshot and gather programs
#define BB_TRACE_VNT 1024                  // threads of the verdict program
#define BB_TRACE_MAX_BLOCKS 8              // layout blocks a model can have (BK_COUNT = 7)

struct TraceArgs {
    double* ring;             // [cap][D2]
    long long D, D2;          // latents, 2 D
    int cap;
    const double* mu;         // snapshot: the handle's parameters, [D] each
    const double* om;
    long long slot;           // ... and the row they go to
    double* slab;             // gather: [K][ld]
    long long first, c0, sc, ld;
    int K;
};

struct TraceVerdictArgs {
    const double* stat;       // [5][D2]: mean, sd, mcse, ess, rhat of every column, the handle's internal order
    long long D, D2;
    int nblk;
    long long lo[BB_TRACE_MAX_BLOCKS], hi[BB_TRACE_MAX_BLOCKS];     // the layout blocks' internal ranges
    double rhat_max;
    long long* cnt;           // [2 nblk][3]: n_nonfinite, n_const, n_above
    double* val;              // [2 nblk][3]: max_rhat, min_ess, max_mcse_rel
};

BB_HD long long bb_trace_verdict_lds_doubles() { return 6 * BB_TRACE_VNT; }

BB_DEV void bb_block_trace_snapshot(BBCtx& cx, const TraceArgs& T, int nblocks) {
    double* dst = T.ring + T.slot * T.D2;
    BB_PASS(cx, tid) {
        for (long long i = (long long)cx.block * cx.nthr + tid; i < T.D2; i += (long long)nblocks * cx.nthr)
            dst[i] = i < T.D ? T.mu[i] : T.om[i - T.D];
    }
}

// slab[k][x] = ring[(first + k) mod cap][c0 + x], a workgroup taking runs of nthr columns of one row
BB_DEV void bb_block_trace_gather(BBCtx& cx, const TraceArgs& T, int nblocks) {
    const long long runs = (T.sc + cx.nthr - 1) / cx.nthr;
    for (long long w = cx.block; w < (long long)T.K * runs; w += nblocks) {
        const long long k = w / runs, x0 = (w % runs) * cx.nthr;
        const double* src = T.ring + ((T.first + k) % T.cap) * T.D2 + T.c0 + x0;
        double* dst = T.slab + k * T.ld + x0;
        BB_PASS(cx, tid) {
            if (x0 + tid < T.sc) dst[tid] = src[tid];
        }
    }
}

// workgroup b + nblk part: block b's mu (part 0) or omega (part 1) columns
BB_DEV void bb_block_trace_verdict(BBCtx& cx, const TraceVerdictArgs& V) {
    const int b = cx.block % V.nblk, part = cx.block / V.nblk;
    double* mxr = cx.lds;
    double* mne = mxr + cx.nthr;
    double* mxm = mne + cx.nthr;
    long long* cnt = (long long*)(mxm + cx.nthr);          // [3][nthr]
    const double *mean = V.stat, *sd = mean + V.D2, *mcse = sd + V.D2, *ess = mcse + V.D2, *rhat = ess + V.D2;
    BB_PASS(cx, tid) {
        long long nf = 0, nc = 0, na = 0;
        double r = -INFINITY, e = INFINITY, m = -INFINITY;
        for (long long i = V.lo[b] + tid; i < V.hi[b]; i += cx.nthr) {
            const long long c = part ? V.D + i : i;
            nf += mean[c] != mean[c];
            nc += sd[c] == 0.0;
            const double rh = rhat[c], es = ess[c];
            if (isfinite(rh)) {
                na += rh > V.rhat_max;
                r = fmax(r, rh);
            }
            if (isfinite(es)) e = fmin(e, es);
            double sp, sg;
            bb_softplus_sigmoid_fast(mean[V.D + i], &sp, &sg);
            const double rel = bb_div(part ? mcse[c] * sg : mcse[c], sp);
            if (isfinite(rel)) m = fmax(m, rel);
        }
        mxr[tid] = r; mne[tid] = e; mxm[tid] = m;
        cnt[tid] = nf; cnt[cx.nthr + tid] = nc; cnt[2 * cx.nthr + tid] = na;
    }
    BB_SYNC(cx);
    BB_PASS(cx, tid) {
        if (tid < 3) {                                       // lane k: count k and value k
            long long n = 0;
            double v = tid == 1 ? INFINITY : -INFINITY;
            const double* a = cx.lds + tid * cx.nthr;
            for (int i = 0; i < cx.nthr; ++i) {
                n += cnt[tid * cx.nthr + i];
                v = tid == 1 ? fmin(v, a[i]) : fmax(v, a[i]);
            }
            V.cnt[3 * cx.block + tid] = n;
            V.val[3 * cx.block + tid] = isfinite(v) ? v : (double)NAN;
        }
    }
}
