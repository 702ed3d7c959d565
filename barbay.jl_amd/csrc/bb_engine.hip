// bb_engine.hip -- host side of the C ABI declared in include/barbay_hip.h: the handle, the resident launchers, groups and the cross-GPU
// leg; what a step launches is in bb_step.h, the launch plan in bb_plan.h, handle creation in bb_create.h, the run path (bb_run and its
// kin) in bb_run.h, the post-fit entry points (hier fitness, log-density batch, bands, scores, chain summary) in bb_analysis.h and the HMC
// session in bb_hmc_host.h with its streaming moments in bb_hmc_accum_host.h and its NUTS tree in bb_nuts_host.h, all included below.
//
// Owns device memory, the HIP stream, captured hipGraphs of the step loop, and (optionally) an
// RCCL communicator.  The compute is the block programs of bb_block.h launched as kernels.
//
// Built twice from this one source:
//   hipcc --offload-arch=gfx950           -> libbarbay_hip.so   (the product)
//   g++ -DBB_EMU -x c++                   -> tests/_emu/libbb_emu.so (sequential host emulation of
//                                            the same block programs; test-only debugging aid)
#include "../../include/barbay_hip.h"
#include "bb_block.h"
#include "bb_persist.h"
#include "bb_resident.h"
#include "bb_stream.h"
#include "bb_inst.h"
#include "bb_hier.h"
#include "bb_ppc.h"
#include "bb_freq.h"
#include "bb_score.h"
#include "bb_loo.h"
#include "bb_rb.h"
#include "bb_contrast.h"
#include "bb_dfe.h"
#include "bb_rank.h"
#include "bb_lsrb.h"
#include "bb_ltrb.h"
#include "bb_llrb.h"
#include "bb_chain.h"
#include "bb_trace.h"
#include "bb_logp.h"
#include "bb_hmc.h"
#include "bb_hmc_accum.h"
#include "bb_nuts.h"
#include "bb_mathprobe.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <string>
#include <type_traits>
#include <vector>

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
static int bb_fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}
extern "C" const char* bb_last_error(void) { return g_err; }

// the backend: device memory, kernel launches, streams, peers, the communicator -- HIP or the host emulation; the small kernels
#include "bb_backend.h"

extern "C" const char* bb_version(void) { return BB_BACKEND_VERSION; }

// ------------------------------------------------------------------------------------------------
// handle
// ------------------------------------------------------------------------------------------------
// Every entry point that takes a handle runs with the handle's device current and restores the caller's on exit: the
// caller may have switched devices since bb_create (torch.cuda.set_device, other handles on other GPUs in this process).
#define BB_ENTER(h) DevGuard bb_dev_guard_((h)->o.device)
#define BB_GROUP_UNSUPPORTED(h, what) \
    do { if (!(h)->shards.empty()) return bb_fail(BB_ERR_UNSUPPORTED, what " is not available on a multi-device handle (n_devices > 1)"); } while (0)

// The environment switches, read once by bb_create and kept in the handle; a multi-device handle's shards get the
// group's copy.  read_tuning says how each one is read.
struct BBTuning {
    bool no_hist_pack, no_host_tables, no_res, no_persist, no_stream, force_stream, any_parity, force_allreduce, p2p_self;
    bool no_graph, graph_collective, no_regroup, no_reorder, nb_set, lead_set;
    int nb, res_nb, ng, lead, nthr, row_l2, opt_spec;
};

static BBTuning read_tuning() {
    auto set = [](const char* n) { return getenv(n) != nullptr; };
    auto num = [](const char* n, int unset) { const char* v = getenv(n); return v ? atoi(v) : unset; };
    auto on = [&](const char* n) { return num(n, 0) > 0; };
    BBTuning t{};
    t.no_hist_pack = on("BB_NO_HIST_PACK");
    t.no_host_tables = on("BB_NO_HOST_TABLES");
    t.no_res = on("BB_NO_RES");
    t.no_persist = on("BB_NO_PERSIST");
    t.no_stream = on("BB_NO_STREAM");
    t.force_stream = on("BB_TUNE_STREAM");
    t.any_parity = on("BB_TUNE_AP");
    t.force_allreduce = on("BB_FORCE_ALLREDUCE");
    t.p2p_self = on("BB_P2P_SELF");
    t.no_graph = set("BB_NO_GRAPH");                  // (these four: set at all, "0" included)
    t.graph_collective = set("BB_GRAPH_COLLECTIVE");
    t.no_regroup = set("BB_NO_REGROUP");
    t.no_reorder = set("BB_NO_REORDER");
    t.nb_set = set("BB_TUNE_NB");                     // (odd: the resident tile map takes "set at all", the two-kernel map a value > 0)
    t.nb = num("BB_TUNE_NB", 0);
    t.res_nb = num("BB_TUNE_RES_NB", 0);              // (> 0: the resident launch's own tile size)
    t.ng = num("BB_TUNE_NG", 0);                      // (first_hop_groups takes 8, 16 or 32 where the shape allows)
    t.lead_set = set("BB_TUNE_LEAD");
    t.lead = num("BB_TUNE_LEAD", 65);
    if (t.lead < 10 || t.lead > 100) t.lead = 100;
    t.nthr = num("BB_TUNE_NTHR", 0) >= 64 ? num("BB_TUNE_NTHR", 0) / 64 * 64 : 0;
    t.row_l2 = num("BB_TUNE_ROW_L2", 1) == 0 ? 0 : 1;   // (odd: any value that reads as 0, "off" too, turns it off)
    t.opt_spec = num("BB_TUNE_OPT_SPEC", 1) == 0 ? 0 : 1;   // (likewise: 0 keeps the generic resident instances, A/B runs)
    return t;
}

// What bb_run launches, planned by plan_launch (bb_plan.h) whenever the handle's shape or cross-GPU leg changes.
enum { IMPL_TWO_KERNEL = 0, IMPL_PERSIST = 1, IMPL_RES = 2, IMPL_STREAM = 3 };     // (= bb_stats.resident_kernel)
struct LaunchPlan {
    int impl = IMPL_TWO_KERNEL;        // k_sample + k_update / k_persist (bb_persist.h) / k_res (bb_resident.h) / k_stream (bb_stream.h)
    int P = 0;                         // pair slots per thread of the resident launch (0: none)
    int NB = 0, NBL = 0, nblk = 0;     // its tile map: barcodes per tile, per leader tile (0: uniform), tiles (k_persist: the two-kernel map)
    int ng = 8, pf = 0;                // k_res / k_stream: groups of the exchange's first hop (RunArgs.ng), window slot fetch (RunArgs.pf: 0 or 1)
    bool ms = false;                   // several samples per step or the ELBO trace (the MS instances)
    bool os = false;                   // k_res / k_stream: the instance has the optimiser compiled in (bb_stats.opt_compiled)
    const void* fn = nullptr;          // the resident kernel instance (none in the emulation)
    std::string name;                  // ... as bb_kernel_name reports it
    const char* why = nullptr;         // why no resident launch where one was wanted
};

// A device buffer of the handle's that grows on demand and keeps no contents across calls; bb_destroy frees them all.
struct DevBuf {
    double* p = nullptr;
    size_t cap = 0;                    // doubles
    int grow(size_t n) {
        if (cap >= n) return 0;
        if (p) dfree(p);
        p = nullptr;
        cap = 0;
        void* q = nullptr;
        int rc = dmalloc(&q, n * 8);
        if (!rc) { p = (double*)q; cap = n; }
        return rc;
    }
    void release() {                   // (the next grow allocates afresh)
        if (p) dfree(p);
        p = nullptr;
        cap = 0;
    }
};
enum {
    BUF_EPS,       // bb_elbo_grad: device copy of caller-supplied draws
    BUF_DBG,       // bb_debug_normals, bb_debug_math
    BUF_BANDS,     // bb_ppc_bands / bb_freq_bands: parameters, tables, scratch and bands of the last call
    BUF_LOGP,      // bb_logdensity_grad_batch: the points, their gradients and log-joints, partial rows of the last call
    BUF_CHAIN,     // bb_chain_summary: the slab as uploaded, its transpose and the slab's results
    BUF_HMC,       // bb_hmc_*: the session's walkers (state, proposal, momentum), metric and evaluation scratch; kept from begin to end
    BUF_HMC_ACC,   // bb_hmc_accum_*: the session's running moments per (walker, segment), the tables of a call and the four rows of the statistics
    BUF_NUTS,      // bb_nuts_*: per walker the tree's edges, candidates and checkpoints, the chunk partials, the scalars and the table of a call
    BUF_COUNT
};

struct bb_handle {
    DevModel M{};
    DevState S{};
    bb_advi_opts o{};
    std::vector<bb_block_range> blocks;
    std::vector<void*> owned;          // device allocations
    long long dev_bytes = 0;           // ... and their total size
    int NB = 0, nthr = 0, nblk = 0, ngeno_blk = 0;
    int tile_cap = 0;                  // tiles the exchange, stamp, xsel and tile-table buffers hold: nblk + 8 (k_res's own map may need a few more)
    size_t lds_doubles = 0;            // dynamic LDS of the two-kernel path
    size_t lds_doubles_p0 = 0;         // ... of the resident launch (adds the lambda table)
    size_t lds_doubles_p = 0;          // ... plus the drawn-ahead normals and the cached counts (16 + 8 B per pair)
    long long b_lo = 0, b_hi = 0;      // barcode shard
    int cus = 256;                     // compute units of the device (one resident workgroup each)
    int g_lo = 0, g_hi = 0;            // genotype model: the genotypes whose theta this shard owns (all of them unless cut at genotype boundaries)
    std::vector<int> geno_ptr_h;       // genotype model: CSR offsets over genotypes (sorted geno_idx: first mutant of every genotype)
    long long* d_tile_b = nullptr;     // genotype model, k_res: the tile table (DevState.tile_b / tile_g)
    int* d_tile_g = nullptr;
    long long step = 0;                // host mirror of the device step counter
    int sample = 0;                    // next MC sample inside the current step (split-phase API)
    double elbo_const = 0.0;
    std::vector<double> ld_omega, ld_zero;   // bb_logdensity_grad: constant omega / eps arguments
    // cross-GPU leg of the resident launch (bb_p2p_*)
    void* p2p_inbox = nullptr;               // this rank's inbox (fine-grained device memory)
    size_t p2p_rows_bytes = 0, p2p_bytes = 0, p2p_gran_off = 0;
    double* d_segtab = nullptr;        // host-built tables of the resident launches (host_tables, install_plan)
    int* d_ldstab = nullptr;
    size_t segtab_cap = 0, ldstab_cap = 0;
    void* p2p_peer[BB_MAX_WORLD] = {};       // peers' inboxes as mapped here
    bool p2p_ready = false, p2p_on = false;
    unsigned p2p_seq = 0;                    // probe sequence number (tokens only ever grow)
    unsigned epoch0 = 0;                     // base of the ready / inbox words: grows whenever the step counter restarts
    long long req_steps = 0;                 // steps ASKED of the resident launch since the last restart (equal on all ranks, whatever a timeout left undone)
    bool p2p_first = false;                  // the next resident launch is the first since the cross-GPU leg was switched on (longer poll limit)
    unsigned* hstatus = nullptr;             // host-mapped status words (DevState.hstatus is their device address)
    double* bak_mu = nullptr;          // bb_elbo_grad: saved parameters
    double* bak_om = nullptr;
    DevBuf buf[BUF_COUNT];             // the calls' own device buffers (BUF_*)
    std::vector<double> logp_host;     // bb_logdensity_grad_batch: host staging (rows padded to an even length, the handle's latent order)
    // the HMC session (bb_hmc_*, bb_hmc_host.h): on while hmc_on is set; the device pointers of hmc / hmc_eval lie in buf[BUF_HMC]
    bool hmc_on = false, hmc_ever = false;      // (hmc_ever: a session was begun at some time -- what bb_hmc_end asks)
    HmcArgs hmc{};
    LogpArgs hmc_eval{};               // the evaluation of the proposal rows (its z, grad, logp, lf_* are set per launch)
    double* hmc_tab = nullptr;         // device: eps [Wp] | n_leapfrog [Wp ints] of the transition; hmc.accept lies behind
    std::vector<double> hmc_logp;      // host mirror of the walkers' logp
    // its streaming moments (bb_hmc_accum_*, bb_hmc_accum_host.h): on while acc_on is set; the device pointers of acc lie in buf[BUF_HMC_ACC]
    bool acc_on = false;
    HmcAccArgs acc{};
    std::vector<long long> acc_n;      // [W][S] states added so far
    // its NUTS tree (bb_nuts_*, bb_nuts_host.h): on while nuts_on is set; the device pointers of nuts lie in buf[BUF_NUTS]
    bool nuts_on = false, nuts_started = false;      // (nuts_started: a bb_nuts_start since the last bb_nuts_begin / bb_hmc_step)
    NutsArgs nuts{};
    int* nuts_lf = nullptr;            // device: [Wp] 1 where the walker takes part in the call (LogpArgs.lf_n); behind nuts.op
    std::vector<double> nuts_eps;      // [W] of the transition
    std::vector<char> nuts_live, nuts_moving, nuts_has_sub, nuts_has_cand;      // [W] started; a leaf / a candidate exists since the start
    std::vector<double> nuts_lp_leaf, nuts_lp_sub, nuts_lp_cand;              // host mirrors of the log-joints that go with those rows
    // the iterate trace (bb_trace_*, bb_trace.h): on while trace_ring is set
    double* trace_ring = nullptr;      // [trace_cap][2 D], the handle's own allocation (bb_trace_end frees it)
    int trace_every = 0, trace_cap = 0;
    long long trace_t = 0;             // steps bb_run has taken since begin / the last reset
    long long trace_taken = 0;         // snapshots recorded since then
    bbStream stream{};
    bool opened = false;               // the stream is open (bb_create sets it: until then the handle holds nothing on a device)
    double last_run_ms = 0, avg_sample_ms = 0, avg_update_ms = 0;
    int launches_last_run = 0;
    int graph_launches = 0;            // hipGraphLaunch calls of the last bb_run (bb_debug_graph_launches)
    int64_t bytes_sample = 0, bytes_update = 0;
    BackendState be;                   // the product's graph of the step loop, run timer and communicator
    BBTuning tune{};                   // the environment switches as bb_create found them
    LaunchPlan plan;
    BRLay Yh{};                        // k_res / k_stream: the LDS carve-up (host copy) and device copy
    BRLay* dY = nullptr;
    DevModel* dM = nullptr;            // device copies of the descriptors for the persistent launch
    DevState* dS = nullptr;
    BBLds* dL = nullptr;               // ... and of the resident launch's LDS carve-up (host copy: Lp)
    BBLds Lp{};
    // single-process multi-device handle (bb_advi_opts.n_devices > 1): all the work is in the shards, one per device
    std::vector<bb_handle*> shards;
    bool group_resident = false;       // the shards run resident launches with in-process peer-mapped inboxes
    double* theta_buf = nullptr;       // genotype model: staging of the theta rows gathered from their owners (theta_sync_*)
    bool theta_stale = false;          // a resident run left the theta_g this shard does not own out of date
    bool in_group = false;             // this handle is a shard of a group: its peers' inboxes are plain pointers, not IPC mappings
    // genotype model handed over with geno_idx NOT in consecutive runs (utils.data_to_arrays keeps barcodes in order of appearance,
    // src/utils.jl:692-731): the handle works on the mutants grouped by genotype and presents the caller's order at the ABI.
    // cidx[i] = the caller's flat index of internal latent i (empty: identity); perm_m[m'] = the caller's mutant of internal mutant m'
    std::vector<long long> cidx;
    std::vector<int> perm_m;
    bool use_reduce() const { return o.world_size > 1 || M.kind == BB_MODEL_GENOTYPE || tune.force_allreduce; }
};

template <class T>
static int dalloc(bb_handle* h, T** p, size_t count) {
    void* q = nullptr;
    int rc = dmalloc(&q, count * sizeof(T));
    if (rc) return rc;
    h->owned.push_back(q);
    h->dev_bytes += (long long)(count * sizeof(T));
    *p = (T*)q;
    return dzero(q, count * sizeof(T), h->stream);
}

// f(std::integral_constant<int, KIND>{}) for the model kind: the host-side instances of templates over it
template <class F>
static void by_kind(int kind, F&& f) {
    switch (kind) {
    case 0: f(std::integral_constant<int, 0>{}); break;
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, 4>{});
    }
}

// what one step launches: make_args, ensure_scratch, the launchers, the two exchanges, step_sample and its stages; theta gather; set_step, reset_optimizer
#include "bb_step.h"

// resident launches (bb_persist.h, bb_resident.h, bb_stream.h), the plan: the kernel lookup, plan_launch and its stages (the decision),
// install_plan (the one place that changes the handle), sync_descriptors, resident_args
#include "bb_plan.h"

// ------------------------------------------------------------------------------------------------
// resident launches: in the emulation
// ------------------------------------------------------------------------------------------------
#ifdef BB_EMU
// Host emulation of the resident launch, phase by phase so that several handles (the ranks of a sharded run, all in
// this process) can be stepped in lock step: phase 0 prologue, 1 sample + publish + draw-ahead, 2 leaders,
// 3 consume + update, 4 epilogue.
struct EmuPersist {
    bb_handle* h = nullptr;
    std::vector<double> lds;
    std::vector<unsigned char> st;      // BBPst<P>[nblk * nthr]
    RunArgs A;
    int ok = 1;
};

template <int KIND, int PP>
static void emu_persist_phase(EmuPersist& E, int phase, long long it, long long nsteps) {
    bb_handle* h = E.h;
    const RunArgs& A = E.A;
    BBPst<PP>* st = (BBPst<PP>*)E.st.data();
    auto cxof = [&](int b) { return BBCtx{h->nthr, b, E.lds.data() + (size_t)b * (h->lds_doubles_p + 64), &h->Lp}; };
    const BBLds L = bb_lds_layout(h->M.R, h->M.E, KIND, h->M.Ttot, h->M.nt1, h->M.K, h->NB, h->nthr, 1);
    const unsigned long long step = (unsigned long long)(h->step + it);
    const unsigned abs_epoch = A.xepoch0 + (unsigned)(step + 1), epoch = abs_epoch;
    const int par = (int)(step & 1);
    const bool xg = h->p2p_on;
    if (phase == 0) {
        for (int b = 0; b < h->nblk; ++b) {
            BBCtx cx = cxof(b);
            bbp_prologue<KIND, PP>(cx, h->M, h->S, A, h->NB, st + (size_t)b * h->nthr);
            bbp_draw_ahead<KIND, PP>(cx, h->M, A, h->NB, st + (size_t)b * h->nthr, (unsigned long long)h->step);
        }
    } else if (phase == 1) {
        for (int b = 0; b < h->nblk; ++b) {
            BBCtx cx = cxof(b);
            bbp_sample<KIND, PP>(cx, h->M, h->S, A, h->NB, st + (size_t)b * h->nthr, step);
            bbp_publish_row(cx, h->M, h->S, L, epoch);
            bbp_draw_ahead<KIND, PP>(cx, h->M, A, h->NB, st + (size_t)b * h->nthr, step + 1);
        }
    } else if (phase == 2) {
        for (int g = 0; g < bbp_groups(A); ++g) {
            BBCtx cx = cxof(g);
            if (xg) bbp_leader_reduce<true>(cx, h->M, h->S, A, L, par, epoch, &E.ok, abs_epoch);
            else bbp_leader_reduce<false>(cx, h->M, h->S, A, L, par, epoch, &E.ok, abs_epoch);
        }
    } else if (phase == 3) {
        for (int b = 0; b < h->nblk; ++b) {
            BBCtx cx = cxof(b);
            bbp_prefetch_slot<KIND, PP>(cx, h->M, h->S, A, h->NB, st + (size_t)b * h->nthr, bb_slot_of(A, step).slot);
            bbp_residual_ahead<KIND>(cx, h->M, h->NB, A);
            if (xg) bbp_consume<true>(cx, h->M, h->S, A, L, par, epoch, &E.ok, abs_epoch);
            else bbp_consume<false>(cx, h->M, h->S, A, L, par, epoch, &E.ok, abs_epoch);
            bbp_finish<KIND>(cx, h->M, h->S, A, h->NB);
            bbp_update<KIND, PP>(cx, h->M, h->S, A, h->NB, st + (size_t)b * h->nthr, bb_slot_of(A, step));
        }
    } else {
        for (int b = 0; b < h->nblk; ++b) {
            BBCtx cx = cxof(b);
            bbp_epilogue<KIND, PP>(cx, h->M, h->S, A, h->NB, st + (size_t)b * h->nthr, (unsigned long long)(h->step + nsteps), E.ok == 0);
        }
    }
}

// (OS: the forms with the optimiser compiled in, where the plan chose them -- the same templates as the product's instances)
template <int KIND, int PP, bool AP, bool OS = false>
static void emu_res_phase(EmuPersist& E, int phase, long long it, long long nsteps) {
    bb_handle* h = E.h;
    const RunArgs& A = E.A;
    BRSt<PP>* st = (BRSt<PP>*)E.st.data();
    auto cxof = [&](int b) { return BBCtx{h->nthr, b, E.lds.data() + (size_t)b * (h->lds_doubles_p + 64), nullptr}; };
    const BRLay& Y = h->Yh;
    // `it` counts the exchanges of this run: step (h->step + it / NS), sample it % NS (the MS instances' arithmetic; NS == 1 otherwise)
    const int NS = A.S < 1 ? 1 : A.S;
    const bool MSrun = NS > 1 || A.elbo_every > 0;
    const unsigned long long step = (unsigned long long)(h->step + it / NS);
    const int smp = (int)(it % NS);
    const bool last = smp == NS - 1;
    const unsigned long long xc = MSrun ? step * (unsigned long long)NS + (unsigned long long)smp : step;
    const int buf = (int)(xc & 1);
    const bool want_el = MSrun && A.elbo_every > 0 && step % (unsigned long long)A.elbo_every == 0;
    const int ring = A.elbo_every > 0 ? (int)((step / (unsigned long long)A.elbo_every) % BB_ELBO_RING) : 0;
    const bool xg = h->p2p_on;
    const BBSlot wslot = bb_slot_of(A, step);
    for (int b = 0; b < (phase == 2 ? bbp_groups(A) : h->plan.nblk); ++b) {
        BBCtx cx = cxof(b);
        BRSt<PP>* sb = st + (size_t)b * h->nthr;
        if (phase == 0) {
            br_prologue<KIND, PP, AP>(cx, h->M, h->S, A, Y, h->plan.NB, sb);
            br_draw_ahead<KIND, PP, AP>(cx, A, Y, sb, (unsigned long long)h->step);
        } else if (phase == 1) {
            if (MSrun) br_sample<KIND, PP, true>(cx, h->M, h->S, A, Y, sb, buf, wslot.slot, last, want_el);
            else br_sample<KIND, PP, false, false, OS>(cx, h->M, h->S, A, Y, sb, buf, wslot.slot);
            const unsigned epoch = A.xepoch0 + (unsigned)(xc + 1);
            if (MSrun) br_moments<KIND, PP, true>(cx, h->M, h->S, Y, sb, buf, epoch, want_el);
            else br_moments<KIND, PP, false>(cx, h->M, h->S, Y, sb, buf, epoch);
            br_xchg_publish<KIND, PP, AP, false, OS>(cx, h->M, h->S, A, Y, sb, xc, wslot.slot, last ? step + 1 : step, last ? 0u : (unsigned)(smp + 1), last);
        } else if (phase == 2) {
            if (xg) br_xchg_lead<true>(cx, h->M, h->S, A, Y, xc, &E.ok);
            else br_xchg_lead<false>(cx, h->M, h->S, A, Y, xc, &E.ok);
        } else if (phase == 3) {
            if (xg && MSrun) br_xchg_consume<KIND, PP, true, true>(cx, h->M, h->S, A, Y, sb, xc, &E.ok, want_el, ring, smp);
            else if (xg) br_xchg_consume<KIND, PP, true, false>(cx, h->M, h->S, A, Y, sb, xc, &E.ok);
            else if (MSrun) br_xchg_consume<KIND, PP, false, true>(cx, h->M, h->S, A, Y, sb, xc, &E.ok, want_el, ring, smp);
            // (the one-wave consume + finish where the product's OS instances run it: resident_instance has checked one replicate, ng <= 8)
            else if (OS && !AP && KIND <= 2 && uniform_T(h->M) == 8) br_xchg_consume<KIND, PP, false, false, br_fin_T<KIND, PP, false, 8, AP, false, OS>()>(cx, h->M, h->S, A, Y, sb, xc, &E.ok);
            else if (OS && !AP && KIND <= 2 && uniform_T(h->M) == 6) br_xchg_consume<KIND, PP, false, false, br_fin_T<KIND, PP, false, 6, AP, false, OS>()>(cx, h->M, h->S, A, Y, sb, xc, &E.ok);
            else br_xchg_consume<KIND, PP, false, false>(cx, h->M, h->S, A, Y, sb, xc, &E.ok);
            // (the compile-time-T forms of the G pass where the product has them, so that the emulation covers that code too)
            if (MSrun) br_update<KIND, PP, 0, AP, true>(cx, h->M, h->S, A, Y, sb, wslot, buf, h->plan.NB, smp, NS);
            else if (!AP && uniform_T(h->M) == 8) br_update<KIND, PP, 8, false, false, false, OS>(cx, h->M, h->S, A, Y, sb, wslot, buf, h->plan.NB);
            else if (!AP && uniform_T(h->M) == 6) br_update<KIND, PP, 6, false, false, false, OS>(cx, h->M, h->S, A, Y, sb, wslot, buf, h->plan.NB);
            else br_update<KIND, PP, 0, AP, false, false, OS>(cx, h->M, h->S, A, Y, sb, wslot, buf, h->plan.NB);
        } else {
            br_epilogue<KIND, PP, AP>(cx, h->S, sb, (unsigned long long)(h->step + nsteps), E.ok == 0);
        }
    }
}

template <int KIND, int TT, bool MS, bool OS = false>
static void emu_stream_phase(EmuPersist& E, int phase, long long it, long long nsteps) {
    bb_handle* h = E.h;
    const RunArgs& A = E.A;
    BSG* gs = (BSG*)E.st.data();
    auto cxof = [&](int b) { return BBCtx{h->nthr, b, E.lds.data() + (size_t)b * (h->lds_doubles_p + 64), nullptr}; };
    const BRLay& Y = h->Yh;
    // `it` counts the exchanges of this run: step (h->step + it / NS), sample it % NS (as emu_res_phase)
    const int NS = MS ? (A.S < 1 ? 1 : A.S) : 1;
    const unsigned long long step = (unsigned long long)(h->step + it / NS);
    const int smp = (int)(it % NS);
    const unsigned long long xc = step * (unsigned long long)NS + (unsigned long long)smp;
    auto rec = [&](unsigned long long st_) { return MS && A.elbo_every > 0 && st_ % (unsigned long long)A.elbo_every == 0; };
    const bool want_el = rec(step);
    const int ring = A.elbo_every > 0 ? (int)((step / (unsigned long long)A.elbo_every) % BB_ELBO_RING) : 0;
    const BSMs ms = MS ? bs_ms_of(A, step, smp, NS, want_el, rec(step + 1)) : bs_ms_plain((unsigned)step);
    BRSt<1>* nost = nullptr;
    for (int b = 0; b < (phase == 2 ? bbp_groups(A) : h->plan.nblk); ++b) {
        BBCtx cx = cxof(b);
        BSG* gb = gs + (size_t)b * h->nthr;
        int* bad_any = (int*)(cx.lds + Y.L.misc) + 3;
        if (phase == 0) {
            br_tile_setup<KIND>(cx, h->M, h->S, A, Y, h->plan.NB, KIND <= 2 ? h->nthr / 16 : h->nthr / 64);
            *bad_any = 0;
            // (the launch's first sample; later ones: inside the G passes)
            bs_sample0<KIND, TT, MS>(cx, h->M, h->S, A, Y, h->plan.NB, h->plan.P, (unsigned)h->step, gb, (int)(((unsigned long long)h->step * (unsigned long long)NS) & 1ull), rec((unsigned long long)h->step));
        } else if (phase == 1) {
            bs_moments<KIND, TT, MS>(cx, h->M, h->S, A, Y, h->plan.NB, h->plan.P, (unsigned)step, gb, ms.buf, want_el);
            br_row_publish<1, MS>(cx, h->M, h->S, Y, nost, A.xepoch0 + (unsigned)(xc + 1), want_el);
        } else if (phase == 2) {
            br_xchg_lead<false>(cx, h->M, h->S, A, Y, xc, &E.ok);
        } else if (phase == 3) {
            br_xchg_consume<KIND, 1, false, MS>(cx, h->M, h->S, A, Y, nost, xc, &E.ok, want_el, ring, smp);
            bs_update_l<KIND, TT, MS, OS>(cx, h->M, h->S, A, Y, h->plan.NB, h->plan.P, (unsigned)step, bb_slot_of(A, step), bad_any, gb, ms);
            bs_update_u<KIND, TT, MS, OS>(cx, h->M, h->S, A, Y, h->plan.NB, h->plan.P, (unsigned)step, bb_slot_of(A, step), bad_any, gb, ms);
        } else {
            if (*bad_any) h->S.hstatus[1] = 1u;
            if (b == 0) { h->S.ctr[0] = (unsigned long long)(h->step + nsteps); h->S.ctr[1] = h->S.ctr[0]; }
        }
    }
}

static void emu_persist_dispatch(EmuPersist& E, int phase, long long it, long long nsteps) {
    const LaunchPlan& p = E.h->plan;
    if (p.impl == IMPL_STREAM) {
        const int T = uniform_T(E.h->M);
        auto byT = [&](auto kindc) {
            constexpr int KIND = decltype(kindc)::value;
            if (p.os) {          // (one-sample instances only: resident_instance)
                if (T == 8) emu_stream_phase<KIND, 8, false, true>(E, phase, it, nsteps);
                else if (T == 6) emu_stream_phase<KIND, 6, false, true>(E, phase, it, nsteps);
                else emu_stream_phase<KIND, 4, false, true>(E, phase, it, nsteps);
            }
            else if (T == 8) p.ms ? emu_stream_phase<KIND, 8, true>(E, phase, it, nsteps) : emu_stream_phase<KIND, 8, false>(E, phase, it, nsteps);
            else if (T == 6) p.ms ? emu_stream_phase<KIND, 6, true>(E, phase, it, nsteps) : emu_stream_phase<KIND, 6, false>(E, phase, it, nsteps);
            else p.ms ? emu_stream_phase<KIND, 4, true>(E, phase, it, nsteps) : emu_stream_phase<KIND, 4, false>(E, phase, it, nsteps);
        };
        by_kind(E.h->M.kind, byT);
        return;
    }
    if (p.impl == IMPL_RES) {
        const bool ap = br_any_parity(E.h->M);
        auto byP = [&](auto kindc) {
            constexpr int KIND = decltype(kindc)::value;
            if (p.os) {          // (never MS: resident_instance)
                switch (p.P) {
                case 1: ap ? emu_res_phase<KIND, 1, true, true>(E, phase, it, nsteps) : emu_res_phase<KIND, 1, false, true>(E, phase, it, nsteps); break;
                case 2: ap ? emu_res_phase<KIND, 2, true, true>(E, phase, it, nsteps) : emu_res_phase<KIND, 2, false, true>(E, phase, it, nsteps); break;
                case 3: ap ? emu_res_phase<KIND, 3, true, true>(E, phase, it, nsteps) : emu_res_phase<KIND, 3, false, true>(E, phase, it, nsteps); break;
                default: ap ? emu_res_phase<KIND, 4, true, true>(E, phase, it, nsteps) : emu_res_phase<KIND, 4, false, true>(E, phase, it, nsteps);
                }
            }
            else switch (p.P) {
            case 1: ap ? emu_res_phase<KIND, 1, true>(E, phase, it, nsteps) : emu_res_phase<KIND, 1, false>(E, phase, it, nsteps); break;
            case 2: ap ? emu_res_phase<KIND, 2, true>(E, phase, it, nsteps) : emu_res_phase<KIND, 2, false>(E, phase, it, nsteps); break;
            case 3: ap ? emu_res_phase<KIND, 3, true>(E, phase, it, nsteps) : emu_res_phase<KIND, 3, false>(E, phase, it, nsteps); break;
            default: ap ? emu_res_phase<KIND, 4, true>(E, phase, it, nsteps) : emu_res_phase<KIND, 4, false>(E, phase, it, nsteps);
            }
        };
        by_kind(E.h->M.kind, byP);
        return;
    }
    by_kind(E.h->M.kind, [&](auto kindc) {
        constexpr int KIND = decltype(kindc)::value;
        if constexpr (KIND != BB_MODEL_GENOTYPE) {          // (the genotype model has no k_persist)
            switch (p.P) {
            case 1: emu_persist_phase<KIND, 1>(E, phase, it, nsteps); break;
            case 2: emu_persist_phase<KIND, 2>(E, phase, it, nsteps); break;
            case 3: emu_persist_phase<KIND, 3>(E, phase, it, nsteps); break;
            default: emu_persist_phase<KIND, 4>(E, phase, it, nsteps);
            }
        }
    });
}

static size_t emu_rst_bytes(int P) {
    return P == 1 ? sizeof(BRSt<1>) : (P == 2 ? sizeof(BRSt<2>) : (P == 3 ? sizeof(BRSt<3>) : sizeof(BRSt<4>)));
}
static size_t emu_pst_bytes(int P) {
    return P == 1 ? sizeof(BBPst<1>) : (P == 2 ? sizeof(BBPst<2>) : (P == 3 ? sizeof(BBPst<3>) : sizeof(BBPst<4>)));
}

static int emu_run_group(bb_handle** hs, int n, long long nsteps) {
    std::vector<EmuPersist> es((size_t)n);
    for (int i = 0; i < n; ++i) {
        bb_handle* h = hs[i];
        const LaunchPlan& p = h->plan;
        es[i].h = h;
        es[i].A = resident_args(h);
        es[i].lds.assign((size_t)std::max(h->nblk, p.nblk) * (h->lds_doubles_p + 64), 0.0);
        es[i].st.assign((size_t)std::max(h->nblk, p.nblk) * h->nthr * (p.impl == IMPL_STREAM ? sizeof(BSG) : (p.impl == IMPL_RES ? emu_rst_bytes(p.P) : emu_pst_bytes(p.P))), 0);
        emu_persist_dispatch(es[i], 0, 0, nsteps);
    }
    const long long NS = std::max(hs[0]->o.samples_per_step, 1);
    for (long long it = 0; it < nsteps * NS; ++it)
        for (int phase = 1; phase <= 3; ++phase)
            for (int i = 0; i < n; ++i) emu_persist_dispatch(es[i], phase, it, nsteps);
    int rc = 0;
    for (int i = 0; i < n; ++i) {
        emu_persist_dispatch(es[i], 4, 0, nsteps);
        if (!es[i].ok) rc = bb_fail(BB_ERR_DEVICE, "emulated exchange found a missing row");
        hs[i]->step += nsteps;
    }
    return rc;
}

// test hook of the emulation build: the ranks of a sharded resident run, stepped in lock step in one process
extern "C" int bb_emu_run_group(bb_handle** hs, int32_t n, int64_t nsteps) {
    if (!hs || n < 1 || nsteps < 0) return bb_fail(BB_ERR_INVALID, "bad argument");
    for (int i = 0; i < n; ++i)
        if (!hs[i] || hs[i]->plan.impl == IMPL_TWO_KERNEL) return bb_fail(BB_ERR_INVALID, "handle %d has no resident launch", i);
    for (int i = 0; i < n; ++i) hs[i]->req_steps += nsteps * std::max(hs[i]->o.samples_per_step, 1);
    int rc = emu_run_group(hs, n, nsteps);
    if (!rc) rc = theta_sync_local(hs, n);          // (genotype model: theta_g back from its owner, as bb_run does through RCCL)
    return rc;
}

static int resident_launch(bb_handle* h, RunArgs, long long nsteps) {
    if (h->p2p_on) return bb_fail(BB_ERR_UNSUPPORTED, "emulation: step the ranks of a sharded resident run with bb_emu_run_group");
    return emu_run_group(&h, 1, nsteps);
}
static void resident_timeout_ack(bb_handle*) {}

// ------------------------------------------------------------------------------------------------
// ... and on the device
// ------------------------------------------------------------------------------------------------
#else
static int resident_launch(bb_handle* h, RunArgs A, long long nsteps) {
    const LaunchPlan& p = h->plan;
    int rc = 0;
    // No per-launch memsets: ready words carry base + step + 1 and only grow; the timeout word is sticky (a launch that finds it
    // set leaves at once, so a queue of launches behind a timed-out one neither runs nor skips steps); every launch takes its
    // first step from the device counter.
    if (h->p2p_first && nsteps > 0) { A.spin_limit = 1u << 25; h->p2p_first = false; }   // launch skew between the ranks' processes
    do {                                                  // (nsteps == 0: one launch that only loads and stores the state)
        const int n = (int)std::min<long long>(nsteps, 4096);
        if (++h->be.launch_seq == 0u) h->be.launch_seq = 1u;
        A.launch_tag = h->be.launch_seq;
        if (p.impl == IMPL_STREAM) hipLaunchKernelGGL((bb_stream_kernel)p.fn, dim3(p.nblk), dim3(h->nthr), h->lds_doubles_p * 8, h->stream,
                                                      (const DevModel*)h->dM, (const DevState*)h->dS, (const BRLay*)h->dY, A, p.NB, n, p.P);
        else if (p.impl == IMPL_RES) hipLaunchKernelGGL((bb_res_kernel)p.fn, dim3(p.nblk), dim3(h->nthr), h->lds_doubles_p * 8, h->stream, (const DevModel*)h->dM, (const DevState*)h->dS, (const BRLay*)h->dY, A, p.NB, n);
        else hipLaunchKernelGGL((bb_persist_kernel)p.fn, dim3(p.nblk), dim3(h->nthr), h->lds_doubles_p * 8, h->stream, (const DevModel*)h->dM, (const DevState*)h->dS, (const BBLds*)h->dL, A, p.NB, n);
        rc = launch_check();
        h->step += n;
        nsteps -= n;
        A.spin_limit = 1u << 23;
    } while (nsteps > 0 && !rc);
    return rc;
}
// a launch timed out: the steps that were completed, and the acknowledgement that lets later launches run again
static void resident_timeout_ack(bb_handle* h) {
    unsigned long long c[2];
    if (!d2h(c, h->S.ctr, sizeof c, h->stream)) h->step = (long long)c[0];
    if (!dzero(h->S.gbar, 32 * 10 * 4, h->stream)) (void)dsync(h->stream);
}
#endif

static int launch_persistent(bb_handle* h, long long nsteps) {
    h->req_steps += nsteps * std::max(h->o.samples_per_step, 1);      // (exchanges asked: the rows' epochs count them)
    return resident_launch(h, resident_args(h), nsteps);
}

// a zero-step launch loads the kernel's code object now (seconds on a cold process), not while the peers already poll;
// the first real launch still gets a longer poll limit (launch skew between the ranks' processes)
static int resident_warm(bb_handle* h) {
#ifdef BB_EMU
    return BB_OK;
#else
    h->p2p_first = true;
    const long long keep = h->req_steps;
    int rc = launch_persistent(h, 0);
    h->req_steps = keep;
    return rc ? rc : dsync(h->stream);
#endif
}

// after the stream has drained: the launches' status words (host-mapped, no copy)
static int check_persistent(bb_handle* h) {
    if (!h->hstatus) return 0;
    volatile unsigned* st = h->hstatus;
    if (st[0] != 0) {
        st[0] = 0;
        resident_timeout_ack(h);
        return bb_fail(BB_ERR_DEVICE, "an exchange of the resident launch timed out (not all %d workgroups resident -- device shared or masked? -- or a peer "
                                      "rank stalled); %lld steps completed; set launch_mode = 1 or re-initialise", h->nblk, h->step);
    }
    if (st[1] != 0) {
        st[1] = 0;
        return bb_fail(BB_ERR_NONFINITE, "the variational parameters went non-finite (NaN / Inf) during the run; %lld steps done", h->step);
    }
    return 0;
}

#include "bb_create.h"      // handle creation: bb_default_opts, create_inner and its stages, the caller's order, bb_create; hist_rows, owned_ranges

// how steps are strung together: graphs, run_enqueue / run_finish, bb_run, bb_run_profiled, bb_elbo_grad, bb_logdensity_grad, the ELBO trace, split-phase steps
#include "bb_run.h"

// caller indices of the latents THIS handle owns on a sharded run (its barcodes' latents; genotype model: theta of its own genotypes) -- what
// a gather of the ranks' posteriors takes from this rank.  The replicated global blocks are not in the list.  idx: [bb_num_latents(h)].
extern "C" int bb_get_owned(bb_handle* h, int64_t* idx, int64_t* n) {
    if (!h || !idx || !n) return bb_fail(BB_ERR_INVALID, "null argument");
    std::vector<std::pair<long long, long long>> rg;
    if (h->shards.empty()) owned_ranges(h, rg);
    else for (bb_handle* sh : h->shards) owned_ranges(sh, rg);
    int64_t c = 0;
    for (auto& r : rg)
        for (long long i = r.first; i < r.second; ++i) idx[c++] = h->cidx.empty() ? i : h->cidx[(size_t)i];
    *n = c;
    return BB_OK;
}

extern "C" int bb_get_permutation(bb_handle* h, int64_t* caller_index) {
    if (!h || !caller_index) return bb_fail(BB_ERR_INVALID, "null argument");
    for (long long i = 0; i < h->M.D; ++i) caller_index[i] = h->cidx.empty() ? i : h->cidx[(size_t)i];
    return BB_OK;
}

static void p2p_release(bb_handle* h);
static void group_destroy(bb_handle* g);
extern "C" void bb_destroy(bb_handle* h) {
    if (!h) return;
    if (!h->shards.empty()) { group_destroy(h); return; }
    if (!h->opened) { delete h; return; }      // under construction, refused before its stream was open (or a group without a shard yet)
    BB_ENTER(h);
    stream_quiesce(h->stream, h->be);
    p2p_release(h);
    hostmap_free(h->hstatus);
    for (void* p : h->owned) dfree(p);
    for (DevBuf& b : h->buf) if (b.p) dfree(b.p);
    if (h->trace_ring) dfree(h->trace_ring);
    stream_close(h->stream);
    delete h;
}

extern "C" int64_t bb_num_latents(const bb_handle* h) { return h ? h->M.D : 0; }

extern "C" int bb_get_layout(const bb_handle* h, bb_block_range* blocks, int32_t* n) {
    if (!h || !blocks || !n) return bb_fail(BB_ERR_INVALID, "null argument");
    *n = (int32_t)h->blocks.size();
    for (size_t i = 0; i < h->blocks.size(); ++i) blocks[i] = h->blocks[i];
    return BB_OK;
}

// ------------------------------------------------------------------------------------------------
// single-process multi-device handle (bb_advi_opts.n_devices > 1; SURVEY.md 8b: "multi-GPU is driven inside the library by
// one host thread").  The group handle owns one shard handle per device (rank i of n on device_ids[i]); their inboxes are wired
// in process (hipDeviceEnablePeerAccess + plain pointers, no IPC), the resident launches of all shards are enqueued before any
// is waited for.  Where the resident launch is not possible (a shard refuses: genotype model, S > 1, ELBO recording ...) the
// group falls back to the split-phase step with the K moments summed on the host -- correct everywhere, slow.
// ------------------------------------------------------------------------------------------------
static int p2p_alloc_inbox(bb_handle* h);
static int p2p_wire(bb_handle* h, void* const* bases);
static int p2p_probe_launch(bb_handle* h, unsigned** res);
static int p2p_probe_collect(bb_handle* h, unsigned* res, int32_t* ok);
static void group_destroy(bb_handle* g) {
    for (bb_handle* sh : g->shards) bb_destroy(sh);
    g->shards.clear();
    delete g;
}

static int group_create(const bb_model_desc* md, const bb_advi_opts* opts, const CreateCtx& cx, bb_handle** out) {
    const int n = opts->n_devices;          // (2..BB_MAX_WORLD, rank 0 of 1: check_request)
    HandleOwner own(new bb_handle());
    bb_handle* g = own.get();
    g->o = *opts;
    g->o.device = opts->device_ids ? opts->device_ids[0] : 0;
    g->tune = cx.tune;
    int rc = 0;
    for (int i = 0; i < n && !rc; ++i) {
        bb_advi_opts o = *opts;
        o.n_devices = 1;
        o.device_ids = nullptr;
        o.device = opts->device_ids ? opts->device_ids[i] : i;
        o.rank = i;
        o.world_size = n;
        o.launch_mode = opts->launch_mode == 1 ? 1 : 0;      // (a shard alone cannot run resident before its inbox is wired: mode 2 is enforced below, on the group)
        bb_handle* sh = nullptr;
        rc = create_inner(md, &o, cx, &sh);
        if (!rc) { sh->in_group = true; g->shards.push_back(sh); }
        if (!rc && memcmp(sh->M.blk_lo, g->shards[0]->M.blk_lo, sizeof sh->M.blk_lo))
            rc = bb_fail(BB_ERR_INVALID, "shard %d lays the latents out differently from shard 0", i);
    }
    if (rc) return rc;
    g->M = g->shards[0]->M;                      // (host-side copies of shapes and block ranges; the device pointers inside are shard 0's)
    g->blocks = g->shards[0]->blocks;
    g->b_lo = 0;
    g->b_hi = g->M.B;
    // resident launches with in-process peer-mapped inboxes, if every shard can (and the caller did not ask for two kernels)
    bool ok = opts->launch_mode != 1;
    for (int i = 0; i < n && ok; ++i)
        for (int j = 0; j < n && ok; ++j) {
            const int di = g->shards[i]->o.device, dj = g->shards[j]->o.device;
            if (di != dj && !peer_enable(di, dj)) ok = false;
        }
    void* bases[BB_MAX_WORLD] = {};
    for (int i = 0; i < n && ok; ++i) {
        BB_ENTER(g->shards[i]);
        ok = p2p_alloc_inbox(g->shards[i]) == BB_OK;
        bases[i] = g->shards[i]->p2p_inbox;
    }
    for (int i = 0; i < n && ok; ++i) { BB_ENTER(g->shards[i]); ok = p2p_wire(g->shards[i], bases) == BB_OK; }
    if (ok) {                                    // transport probe: all devices at once
        unsigned* res[BB_MAX_WORLD] = {};
        for (int i = 0; i < n; ++i) { BB_ENTER(g->shards[i]); if (p2p_probe_launch(g->shards[i], &res[i]) != BB_OK) ok = false; }
        for (int i = 0; i < n; ++i) {
            BB_ENTER(g->shards[i]);
            int32_t good = 0;
            if (p2p_probe_collect(g->shards[i], res[i], &good) != BB_OK || !good) ok = false;
        }
    }
    if (ok) for (int i = 0; i < n && ok; ++i) ok = bb_p2p_enable(g->shards[i], 1) == BB_OK;
    // the two resident kernels speak different inbox protocols (k_res: tagged entries, k_persist: rows + ready words): all shards the same one
    if (ok) for (int i = 1; i < n && ok; ++i) ok = (g->shards[i]->plan.impl >= IMPL_RES) == (g->shards[0]->plan.impl >= IMPL_RES);
    if (!ok) for (bb_handle* sh : g->shards) if (sh->p2p_ready) (void)bb_p2p_enable(sh, 0);
    g->group_resident = ok;
    if (!ok && opts->launch_mode == 2) {
        const std::string why(g_err);                 // (bb_fail formats INTO g_err: the message must not be its own argument)
        return bb_fail(BB_ERR_UNSUPPORTED, "launch_mode = 2: the shards cannot run resident launches with peer-mapped inboxes: %s", why.c_str());
    }
    *out = own.release();
    return BB_OK;
}

// resident: the shards' launches are all enqueued before any is waited for (the emulation steps them in lock step)
static int group_run_resident(bb_handle* g, int64_t n_steps) {
#ifdef BB_EMU
    return bb_emu_run_group(g->shards.data(), (int)g->shards.size(), n_steps);
#else
    int rc = 0, rc2 = 0;
    for (bb_handle* sh : g->shards) { BB_ENTER(sh); if ((rc = run_enqueue(sh, n_steps))) break; }
    for (bb_handle* sh : g->shards) { BB_ENTER(sh); const int r = run_finish(sh); if (r && !rc2) rc2 = r; }      // (wait for whatever was launched, also after an error)
    if (!rc) rc = rc2;
    if (!rc) rc = theta_sync_local(g->shards.data(), (int)g->shards.size());     // (genotype model: theta_g back from its owner)
    return rc;
#endif
}

static int group_run(bb_handle* g, int64_t n_steps) {
    int rc = 0;
    if (g->group_resident) {
        rc = group_run_resident(g, n_steps);
    } else {
        // the two-kernel step over all shards, the exchanges summed on the host in place of the RCCL all-reduces
        const int S = g->o.samples_per_step < 1 ? 1 : g->o.samples_per_step, n = (int)g->shards.size();
        std::vector<RunArgs> As((size_t)n);
        for (bb_handle* sh : g->shards) { BB_ENTER(sh); if ((rc = ensure_scratch(sh))) return rc; }
        for (int64_t it = 0; it < n_steps && !rc; ++it) {
            for (int smp = 0; smp < S && !rc; ++smp) {
                for (int i = 0; i < n; ++i) { const bb_handle* sh = g->shards[i]; As[i] = make_args(sh, sh->step, smp, S, true, elbo_wanted(sh, sh->step)); }
                rc = step_sample(g->shards.data(), n, As.data(), host_sum_exchange);
            }
            for (bb_handle* sh : g->shards) sh->step++;
        }
        for (bb_handle* sh : g->shards) { BB_ENTER(sh); const int r = dsync(sh->stream); if (r && !rc) rc = r; }
    }
    g->step = g->shards[0]->step;
    return rc;
}

static int group_get_params(bb_handle* g, double* mu, double* omega) {
    const size_t D = (size_t)g->M.D;
    std::vector<double> tm(D), to(D);
    int rc = bb_get_params(g->shards[0], mu, omega);      // replicated blocks (and its own shard) from shard 0
    for (size_t i = 1; i < g->shards.size() && !rc; ++i) {
        if ((rc = bb_get_params(g->shards[i], tm.data(), to.data()))) break;
        std::vector<std::pair<long long, long long>> rg;
        owned_ranges(g->shards[i], rg);
        for (auto& r : rg) {
            std::copy(tm.begin() + r.first, tm.begin() + r.second, mu + r.first);
            std::copy(to.begin() + r.first, to.begin() + r.second, omega + r.first);
        }
    }
    return rc;
}

extern "C" int bb_init_meanfield(bb_handle* h) {
    if (!h) return bb_fail(BB_ERR_INVALID, "null handle");
    if (!h->shards.empty()) { int rc = 0; for (bb_handle* sh : h->shards) if (!rc) rc = bb_init_meanfield(sh); h->step = 0; return rc; }
    BB_ENTER(h);
    h->theta_stale = false;
    trace_reset(h);
    const int nb = (int)std::min<long long>(((h->M.D + 1) / 2 + 255) / 256, 1024);
    const int rc = launch(h->stream, k_init, nb, 256, 0, h->M, h->S, h->o.seed);
    return rc ? rc : reset_optimizer(h);
}

extern "C" int bb_set_params(bb_handle* h, const double* mu, const double* omega) {
    if (!h || !mu || !omega) return bb_fail(BB_ERR_INVALID, "null argument");
    std::vector<double> pm, po;
    if (!h->cidx.empty()) {          // the caller's order -> the handle's
        pm.resize(h->cidx.size()); po.resize(h->cidx.size());
        perm_gather(h, mu, pm.data()); perm_gather(h, omega, po.data());
        mu = pm.data(); omega = po.data();
    }
    if (!h->shards.empty()) { int rc = 0; for (bb_handle* sh : h->shards) if (!rc) rc = bb_set_params(sh, mu, omega); h->step = 0; return rc; }
    BB_ENTER(h);
    int rc;
    h->theta_stale = false;
    trace_reset(h);
    if ((rc = h2d(h->S.mu, mu, (size_t)h->M.D * 8, h->stream))) return rc;
    if ((rc = h2d(h->S.om, omega, (size_t)h->M.D * 8, h->stream))) return rc;
    return reset_optimizer(h);
}

static int get_params_raw(bb_handle* h, double* mu, double* omega) {
    if (!h->shards.empty()) return group_get_params(h, mu, omega);
    BB_ENTER(h);
    int rc;
    if ((rc = dsync(h->stream))) return rc;
    if ((rc = d2h(mu, h->S.mu, (size_t)h->M.D * 8, h->stream))) return rc;
    return d2h(omega, h->S.om, (size_t)h->M.D * 8, h->stream);
}
extern "C" int bb_get_params(bb_handle* h, double* mu, double* omega) {
    if (!h || !mu || !omega) return bb_fail(BB_ERR_INVALID, "null argument");
    if (h->cidx.empty()) return get_params_raw(h, mu, omega);
    std::vector<double> a(h->cidx.size()), b(h->cidx.size());
    int rc = get_params_raw(h, a.data(), b.data());
    if (rc) return rc;
    perm_scatter(h, a.data(), mu);
    perm_scatter(h, b.data(), omega);
    return BB_OK;
}

static double host_softplus(double om) { return std::max(om, 0.0) + log1p(exp(-fabs(om))); }

extern "C" int bb_get_posterior(bb_handle* h, double* mean, double* sigma) {
    if (!h || !mean || !sigma) return bb_fail(BB_ERR_INVALID, "null argument");
    BB_ENTER(h);
    int rc = bb_get_params(h, mean, sigma);
    if (rc) return rc;
    for (long long i = 0; i < h->M.D; ++i) sigma[i] = host_softplus(sigma[i]);   // sigma = softplus(omega), O(D) once at the end
    return BB_OK;
}

extern "C" int bb_debug_normals(bb_handle* h, int64_t step, uint32_t stream, int64_t lo, int64_t hi, double* out) {
    if (!h || !out || lo < 0 || hi < lo) return bb_fail(BB_ERR_INVALID, "bad argument");
    if (!h->shards.empty()) return bb_debug_normals(h->shards[0], step, stream, lo, hi, out);
    BB_ENTER(h);
    const size_t n = (size_t)(hi - lo);
    if (n == 0) return BB_OK;
    int rc;
    DevBuf& dbg = h->buf[BUF_DBG];
    if ((rc = dbg.grow(n))) return rc;
    const int nb = (int)std::min<size_t>((n / 2 + 256) / 256, 1024);
    if ((rc = launch(h->stream, k_normals, nb, 256, 0, h->o.seed, step, stream, lo, hi, dbg.p))) return rc;
    return d2h(out, dbg.p, n * 8, h->stream);
}

// operands, results and the kernel of bb_block_math (bb_mathprobe.h) in BUF_DBG: x, y, out0, out1, n doubles each
extern "C" int bb_debug_math(bb_handle* h, int32_t fn, int64_t n, const double* x, const double* y, double* out0, double* out1) {
    if (!h || fn < 0 || fn >= BB_MATH_COUNT || n < 0 || !x || !out0) return bb_fail(BB_ERR_INVALID, "bad argument");
    const bool two_in = fn == BB_MATH_DIV || fn == BB_MATH_BOX_MULLER;
    const bool two_out = fn == BB_MATH_SOFTPLUS_SIGMOID || fn == BB_MATH_SINCOSPI || fn == BB_MATH_BOX_MULLER;
    if ((two_in && !y) || (two_out && !out1)) return bb_fail(BB_ERR_INVALID, "function %d takes two operands / gives two results", (int)fn);
    if (!h->shards.empty()) return bb_debug_math(h->shards[0], fn, n, x, y, out0, out1);
    BB_ENTER(h);
    if (n == 0) return BB_OK;
    const size_t m = (size_t)n;
    int rc;
    DevBuf& dbg = h->buf[BUF_DBG];
    if ((rc = dbg.grow(4 * m))) return rc;
    double *dx = dbg.p, *dy = dbg.p + m, *d0 = dbg.p + 2 * m, *d1 = dbg.p + 3 * m;
    if ((rc = h2d(dx, x, m * 8, h->stream))) return rc;
    if (two_in && (rc = h2d(dy, y, m * 8, h->stream))) return rc;
    const int nb = (int)std::min<size_t>((m + 255) / 256, 1024);
    if ((rc = launch(h->stream, k_math, nb, 256, 0, (int)fn, (long long)n, dx, two_in ? dy : nullptr, d0, two_out ? d1 : nullptr))) return rc;
    if ((rc = d2h(out0, d0, m * 8, h->stream))) return rc;
    return two_out ? d2h(out1, d1, m * 8, h->stream) : BB_OK;
}

extern "C" int bb_debug_stamps(bb_handle* h, uint64_t* out, int64_t n) {
    if (!h || !out) return bb_fail(BB_ERR_INVALID, "bad argument");
    if (!h->shards.empty()) return bb_debug_stamps(h->shards[0], out, n);
    if (n < 0) { out[0] = (uint64_t)h->tile_cap; return BB_OK; }     // rows of the block-stamp area (the per-wave area follows it)
    BB_ENTER(h);
    const int64_t have = (int64_t)h->tile_cap * (32 + 64);
    int rc = dsync(h->stream);
    if (rc) return rc;
    return d2h(out, h->S.stamps, (size_t)std::min(n, have) * 8, h->stream);
}

// the optimiser's state as the device holds it (the handle's internal latent order, bb_get_permutation)
extern "C" int bb_debug_opt_state(bb_handle* h, double* acc_mu, double* acc_omega, float* lo) {
    if (!h || !acc_mu || !acc_omega || !lo) return bb_fail(BB_ERR_INVALID, "null argument");
    BB_GROUP_UNSUPPORTED(h, "bb_debug_opt_state");
    BB_ENTER(h);
    int rc;
    if ((rc = dsync(h->stream))) return rc;
    if ((rc = d2h(acc_mu, h->S.acc_mu, (size_t)h->M.D * 8, h->stream)) || (rc = d2h(acc_omega, h->S.acc_om, (size_t)h->M.D * 8, h->stream))) return rc;
    return d2h(lo, h->S.accl, (size_t)h->M.D * 2 * sizeof(float), h->stream);
}

extern "C" int bb_debug_graph_launches(bb_handle* h) {
    if (!h) return 0;
    if (!h->shards.empty()) return bb_debug_graph_launches(h->shards[0]);
    return h->graph_launches;
}

// ------------------------------------------------------------------------------------------------
// cross-GPU leg of the resident launch: inbox, IPC handles, transport probe, switch
// ------------------------------------------------------------------------------------------------
static size_t p2p_rows_bytes(const bb_handle* h) {
    const size_t n = (size_t)2 * h->o.world_size * 8 * (size_t)(h->M.K + 2 * h->M.nt1) * 8;
    return (n + 255) & ~(size_t)255;
}
// ready words: [2][world][8] lines of 128 B, then the probe's [world] lines
static size_t p2p_probe_words_off(const bb_handle* h) { return (size_t)32 * 2 * h->o.world_size * 8; }

static void p2p_release(bb_handle* h) {
    for (int r = 0; r < BB_MAX_WORLD; ++r)
        if (h->p2p_peer[r] && r != h->o.rank && !h->in_group) ipc_close(h->p2p_peer[r]);
    finegrained_free(h->p2p_inbox);
    h->p2p_inbox = nullptr;
    h->p2p_ready = h->p2p_on = false;
}

// this rank's inbox: fine-grained device memory (remote stores and local polls must meet in memory, not in either side's L2)
static int p2p_alloc_inbox(bb_handle* h) {
    // (BB_P2P_SELF=1, diagnostics: a whole-problem handle runs the inbox protocol against its own inbox -- tools/xg_self.py)
    if (h->o.world_size < 2 && !h->tune.p2p_self) return bb_fail(BB_ERR_INVALID, "the cross-GPU leg needs a sharded handle (world_size > 1)");
    if (h->o.world_size > BB_MAX_WORLD) return bb_fail(BB_ERR_UNSUPPORTED, "at most %d ranks", BB_MAX_WORLD);
    if (h->M.kind == BB_MODEL_GENOTYPE && !h->M.geno_sorted)
        return bb_fail(BB_ERR_UNSUPPORTED, "the genotype model's resident launch needs geno_idx in consecutive runs (shards must own whole genotypes)");
    if (h->p2p_inbox) return BB_OK;
    h->p2p_rows_bytes = p2p_rows_bytes(h);
    h->p2p_gran_off = (h->p2p_rows_bytes + (p2p_probe_words_off(h) + (size_t)32 * h->o.world_size) * 4 + 255) & ~(size_t)255;
    h->p2p_bytes = h->p2p_gran_off + 2 * h->p2p_rows_bytes + 16 * 16 * (size_t)(h->M.K + 2 * h->M.nt1);      // (tagged rows: 16 B per entry; + the polls' eight-rows-in-flight slack)
    return finegrained_alloc(&h->p2p_inbox, h->p2p_bytes, h->stream);
}

// every rank's inbox as seen from this rank (bases[own rank] = the local inbox)
static int p2p_wire(bb_handle* h, void* const* bases) {
    for (int r = 0; r < h->o.world_size; ++r) {
        if (!bases[r]) return bb_fail(BB_ERR_COMM, "rank %d's inbox did not map", r);
        h->p2p_peer[r] = bases[r];
        h->S.xout[r] = (double*)bases[r];
        h->S.xout_rdy[r] = (unsigned*)((char*)bases[r] + h->p2p_rows_bytes);
        h->S.xgr[r] = (bb_gran*)((char*)bases[r] + h->p2p_gran_off);
    }
    h->p2p_ready = true;
    return sync_descriptors(h);
}

extern "C" int bb_p2p_export(bb_handle* h, void* handle_out) {
    if (!h || !handle_out) return bb_fail(BB_ERR_INVALID, "null argument");
    if (!h->shards.empty()) return bb_fail(BB_ERR_UNSUPPORTED, "a multi-device handle wires its shards itself");
    BB_ENTER(h);
    memset(handle_out, 0, BB_P2P_HANDLE_BYTES);
    int rc = p2p_alloc_inbox(h);
    return rc ? rc : ipc_export(handle_out, h->p2p_inbox);
}

extern "C" int bb_p2p_import(bb_handle* h, const void* handles) {
    if (!h || !handles) return bb_fail(BB_ERR_INVALID, "null argument");
    if (!h->shards.empty()) return bb_fail(BB_ERR_UNSUPPORTED, "a multi-device handle wires its shards itself");
    BB_ENTER(h);
    if (!h->p2p_inbox) return bb_fail(BB_ERR_INVALID, "bb_p2p_export comes first");
    const int W = h->o.world_size;
    void* bases[BB_MAX_WORLD] = {};
    for (int r = 0; r < W; ++r) {
        int rc = 0;
        if (r == h->o.rank) bases[r] = h->p2p_inbox;
        else if ((rc = ipc_open(&bases[r], (const char*)handles + (size_t)r * BB_P2P_HANDLE_BYTES, h->p2p_peer[r]))) return rc;
    }
    return p2p_wire(h, bases);
}

// transport probe in two halves, so that one host thread can run it on several devices at once: every rank's kernel waits for
// the tokens of all the others
static int p2p_probe_launch(bb_handle* h, unsigned** res) {
    *res = nullptr;
    return probe_launch(h->stream, h->S, h->o.rank, h->o.world_size, p2p_probe_words_off(h), ++h->p2p_seq, res);
}
static int p2p_probe_collect(bb_handle* h, unsigned* res, int32_t* ok) {
    return probe_collect(h->stream, res, h->S, h->o.world_size, ok);
}

extern "C" int bb_p2p_selftest(bb_handle* h, int32_t* ok) {
    if (!h || !ok) return bb_fail(BB_ERR_INVALID, "null argument");
    if (!h->shards.empty()) return bb_fail(BB_ERR_UNSUPPORTED, "a multi-device handle wires its shards itself");
    BB_ENTER(h);
    *ok = 0;
    if (!h->p2p_ready) return bb_fail(BB_ERR_INVALID, "bb_p2p_import comes first");
    // Every rank's token carries the same sequence number only if all ranks call this the same number of times
    // (they do: the caller votes on the outcome), so a peer's token is predictable: replace the low byte.
    unsigned* res = nullptr;
    int rc = p2p_probe_launch(h, &res);
    if (rc) { probe_free(res); return rc; }
    return p2p_probe_collect(h, res, ok);
}

extern "C" int bb_p2p_enable(bb_handle* h, int32_t on) {
    if (!h) return bb_fail(BB_ERR_INVALID, "null argument");
    BB_GROUP_UNSUPPORTED(h, "bb_p2p_enable");
    BB_ENTER(h);
    if (on && !h->p2p_ready) return bb_fail(BB_ERR_INVALID, "bb_p2p_import comes first");
    Planned plan;
    int rc = plan_or_refuse(h, on ? 2 : h->o.launch_mode, on != 0, plan);      // (the cross-GPU leg needs a resident launch: an error says why not)
    // ... and the handle was never touched.  (Switching the leg OFF is never refused: without the leg the handle plans as it did in
    // bb_create, which a launch_mode = 2 handle has passed.)
    if (rc) return rc;
    h->p2p_on = on != 0;
    if ((rc = install_plan(h, plan))) h->p2p_on = false;      // (what install_plan leaves then, the two-kernel step, runs without the cross-GPU leg)
    { const int rcs = sync_descriptors(h); if (!rc) rc = rcs; }
    if (rc) return rc;
    return h->p2p_on ? resident_warm(h) : BB_OK;
}

// the post-fit entry points: bb_hier_fitness, bb_logdensity_grad_batch, bb_ppc_bands, bb_freq_bands, bb_chain_summary
#include "bb_analysis.h"

// the HMC session: bb_hmc_begin, bb_hmc_step, bb_hmc_get, bb_hmc_end (bb_hmc.h)
#include "bb_hmc_host.h"
// its streaming moments and the metric: bb_hmc_accum_*, bb_hmc_set_metric, bb_hmc_get_metric (bb_hmc_accum.h)
#include "bb_hmc_accum_host.h"
// its NUTS tree: bb_nuts_begin, bb_nuts_start, bb_nuts_leaf, bb_nuts_take (bb_nuts.h)
#include "bb_nuts_host.h"

extern "C" int bb_get_stats(bb_handle* h, bb_stats* s) {
    if (!h || !s) return bb_fail(BB_ERR_INVALID, "null argument");
    BB_ENTER(h);
    if (!h->shards.empty()) {       // shard 0's figures; what adds up over the shards is added up
        int rc = bb_get_stats(h->shards[0], s);
        for (size_t i = 1; i < h->shards.size() && !rc; ++i) {
            bb_stats t;
            if ((rc = bb_get_stats(h->shards[i], &t))) break;
            s->bytes_per_step += t.bytes_per_step; s->bytes_sample += t.bytes_sample; s->bytes_update += t.bytes_update;
            s->n_blocks += t.n_blocks;
            s->rows_same_xcd += t.rows_same_xcd;
            s->device_bytes += t.device_bytes;
            s->last_run_ms = std::max(s->last_run_ms, t.last_run_ms);
            s->persistent_pairs = std::min(s->persistent_pairs, t.persistent_pairs);
            s->resident_kernel = std::min(s->resident_kernel, t.resident_kernel);
            s->opt_compiled = std::min(s->opt_compiled, t.opt_compiled);
        }
        s->shard_lo = 0;
        s->shard_hi = h->M.B;
        s->geno_lo = 0;
        s->geno_hi = h->M.G;
        return rc;
    }
    memset(s, 0, sizeof *s);
    s->n_latents = h->M.D;
    s->n_moments = h->M.K;
    s->steps_done = h->step;
    s->shard_lo = h->b_lo;
    s->shard_hi = h->b_hi;
    s->geno_lo = h->g_lo;
    s->geno_hi = h->g_hi;
    s->device_bytes = h->dev_bytes;
    s->window_row = h->M.Dh;
    s->bytes_sample = h->bytes_sample;
    s->bytes_update = h->bytes_update;
    s->bytes_per_step = h->bytes_update;   // theta read once when the two sweeps are fused (96 D + 4 TBR)
    s->last_run_ms = h->last_run_ms;
    s->avg_sample_ms = h->avg_sample_ms;
    s->avg_update_ms = h->avg_update_ms;
    s->n_blocks = h->plan.nblk;
    s->block_threads = h->nthr;
    s->lds_bytes = (int32_t)((h->plan.impl != IMPL_TWO_KERNEL ? h->lds_doubles_p : h->lds_doubles) * 8);
    s->persistent_pairs = h->plan.P;
    s->launches_last_run = h->launches_last_run;
    s->resident_kernel = h->plan.impl;
    s->opt_compiled = h->plan.os ? 1 : 0;
    if (h->plan.impl >= IMPL_RES) {          // (k_res / k_stream: what the tiles of the last launch decided about their row stores)
        std::vector<int> sel((size_t)h->plan.nblk);
        int rc = d2h(sel.data(), h->S.xsel, sel.size() * sizeof(int), h->stream);
        if (rc) return rc;
        for (int v : sel) s->rows_same_xcd += v > 0 ? 1 : 0;
    }
    return BB_OK;
}

// The kernel bb_run launches, as text: the template instance in declaration order -- k_res<KIND, P, NT, XG, TT, AP, MS>,
// k_stream<KIND, NT, TT>, k_persist<KIND, P, NT[, XG]> -- or "k_sample + k_update" for the two-kernel step.  Tests and bench.py
// print / assert THIS instead of reconstructing the instance from bb_stats.
extern "C" int bb_kernel_name(bb_handle* h, char* buf, int64_t len) {
    if (!h || !buf || len < 2) return bb_fail(BB_ERR_INVALID, "null argument / no room");
    if (!h->shards.empty()) return bb_kernel_name(h->shards[0], buf, len);
    snprintf(buf, (size_t)len, "%s", h->plan.name.c_str());
    return BB_OK;
}

// ------------------------------------------------------------------------------------------------
// sharded execution
// ------------------------------------------------------------------------------------------------
extern "C" int bb_comm_make_id(void* id_out) {
    if (!id_out) return bb_fail(BB_ERR_INVALID, "null argument");
    return comm_make_id(id_out);
}

extern "C" int bb_comm_init(bb_handle* h, const void* id_in) {
    if (!h || !id_in) return bb_fail(BB_ERR_INVALID, "null argument");
    BB_GROUP_UNSUPPORTED(h, "bb_comm_init");
    BB_ENTER(h);
    return comm_init(h->be, id_in, h->o.device, h->o.world_size, h->o.rank);
}
