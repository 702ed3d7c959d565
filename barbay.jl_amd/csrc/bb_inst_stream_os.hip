// bb_inst_stream_os.hip -- the k_stream instances of bb_inst_stream.hip with the optimiser compiled in (OS = true: TruncatedADAGrad,
// resum_every == 0 -- bb_opt_apply<0, 0>), one translation unit of the library (see bb_inst.h).  Keep the two lists alike; the names
// are the generic instances' -- which form a handle runs is bb_stats.opt_compiled.
#include "bb_inst.h"
bb_stream_kernel bb_stream_instance_os(int kind, int nthr, int T, const char** nm) {
    if (nm) *nm = "";
#define BS_CASE(K, NT, TT) if (kind == (K) && nthr == (NT) && T == (TT)) { if (nm) *nm = "k_stream<" #K "," #NT "," #TT ">"; return k_stream<K, NT, TT, false, true>; }
    BS_CASE(0, 1024, 8) BS_CASE(1, 1024, 8) BS_CASE(2, 1024, 8) BS_CASE(3, 1024, 8) BS_CASE(4, 1024, 8)
    BS_CASE(0, 1024, 6) BS_CASE(1, 1024, 6) BS_CASE(2, 1024, 6) BS_CASE(3, 1024, 6) BS_CASE(4, 1024, 6)
    BS_CASE(0, 1024, 4) BS_CASE(1, 1024, 4) BS_CASE(2, 1024, 4)
    BS_CASE(0, 512, 8) BS_CASE(1, 512, 8) BS_CASE(2, 512, 8) BS_CASE(3, 512, 6) BS_CASE(4, 512, 6)
#undef BS_CASE
    return nullptr;
}
