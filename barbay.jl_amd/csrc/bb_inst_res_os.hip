// bb_inst_res_os.hip -- the k_res instances with the optimiser compiled in (OS = true: TruncatedADAGrad, resum_every == 0 -- bb_opt_apply<0, 0>),
// one translation unit of the library (see bb_inst.h).  One for every compile-time-T instance of bb_inst_res_k*.hip (their BR_T lines: keep
// the two lists alike), one GPU and cross-GPU; under the generic instance's name -- which form a handle runs is bb_stats.opt_compiled.
#include "bb_inst.h"
bb_res_kernel bb_res_instance_os(int kind, int P, int nthr, bool xg, int T, const char** nm) {
    if (nm) *nm = "";
    const int NTr = nthr > 512 ? 1024 : (nthr > 256 ? 512 : 256);        // (the register budgets of bb_inst_res.inc)
#define BR_OS(K, PP, NT, TT) if (kind == (K) && P == (PP) && NTr == (NT) && T == (TT)) { \
        if (xg) { if (nm) *nm = "k_res<" #K "," #PP "," #NT ",true," #TT ",false,false>"; return k_res<K, PP, NT, true, TT, false, false, true>; } \
        if (nm) *nm = "k_res<" #K "," #PP "," #NT ",false," #TT ",false,false>"; return k_res<K, PP, NT, false, TT, false, false, true>; }
    BR_OS(0, 1, 1024, 8) BR_OS(0, 1, 1024, 6) BR_OS(0, 1, 512, 8) BR_OS(0, 2, 512, 8)
    BR_OS(1, 1, 1024, 8) BR_OS(1, 1, 1024, 6) BR_OS(1, 1, 512, 6) BR_OS(1, 2, 512, 6)
    BR_OS(2, 1, 1024, 8) BR_OS(2, 2, 512, 8) BR_OS(2, 3, 512, 8)
    BR_OS(3, 2, 512, 6) BR_OS(3, 3, 512, 6)
    BR_OS(4, 3, 512, 6)
#undef BR_OS
    return nullptr;
}
