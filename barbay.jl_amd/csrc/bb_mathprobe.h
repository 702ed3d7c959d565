// bb_mathprobe.h -- test-only block program behind bb_debug_math: one function of bb_math.h (or the Box-Muller step of bb_block.h)
// evaluated element-wise on caller-chosen arguments, so that tests/test_gpu_math.py judges the DEVICE build of the header -- hardware
// rcp / rsq seeds, the v_fma_f64 Horner blocks with their scalar coefficient operands, the __constant__ tables, the device
// ldexp / frexp / rint -- against a 50-digit reference.  It calls the BB_DEV functions themselves and restates nothing; no other
// kernel includes or calls it.  The same source is the emulation's loop (tests/test_emu_math.py).
#pragma once
#include "bb_block.h"

BB_DEV void bb_block_math(BBCtx& cx, int fn, long long n, const double* x, const double* y, double* out0, double* out1, int nblocks) {
    BB_PASS(cx, tid) {
        for (long long i = (long long)cx.block * cx.nthr + tid; i < n; i += (long long)nblocks * cx.nthr) {
            const double a = x[i];
            double r0 = 0.0, r1 = 0.0;
            switch (fn) {
            case BB_MATH_EXP: r0 = bb_exp(a); break;
            case BB_MATH_LOG: r0 = bb_log(a); break;
            case BB_MATH_RCP: r0 = bb_rcp(a); break;
            case BB_MATH_DIV: r0 = bb_div(a, y[i]); break;
            case BB_MATH_SQRT: r0 = bb_sqrt(a); break;
            case BB_MATH_SOFTPLUS_SIGMOID: bb_softplus_sigmoid_fast(a, &r0, &r1); break;
            case BB_MATH_SINCOSPI: bb_sincospi_02(a, &r0, &r1); break;
            case BB_MATH_EXP_NONPOS: r0 = bb_exp_nonpos(a); break;
            case BB_MATH_LOG_1TO2: r0 = bb_log_1to2(a); break;
            case BB_MATH_BOX_MULLER: {                      // the two 64-bit words are the bit patterns of x[i] and y[i]
                unsigned long long wa, wb;
                memcpy(&wa, x + i, 8);
                memcpy(&wb, y + i, 8);
                bb_box_muller(wa, wb, &r0, &r1);
                break;
            }
            default: break;
            }
            out0[i] = r0;
            if (out1) out1[i] = r1;
        }
    }
    BB_SYNC(cx);
}
