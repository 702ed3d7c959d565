// bb_plan.h -- resident launches (bb_persist.h, bb_resident.h, bb_stream.h): the plan.  Which of the four step implementations bb_run
// launches and with what tile map is DECIDED first -- plan_launch, a function of the handle and a launch mode that changes no handle
// field and allocates or copies nothing on the device -- and INSTALLED once: install_plan, the one place that writes the plan's handle
// fields and device tables.  Included by bb_engine.hip (after the handle and bb_step.h, before the resident launchers).

// the time-point count where all replicates share it (the compile-time-T instances), else 0
static int uniform_T(const DevModel& M) {
    for (int r = 1; r < M.R; ++r) if (M.T[r] != M.T[0]) return 0;
    return M.T[0];
}

// The resident kernel instances (bb_inst.h) and their names, one function per question -- k_stream or k_res with P pair slots; k_persist
// (xg: the cross-GPU instances) -- each with three bodies: the emulation runs the block programs as host functions, so it only names
// the launch (the compile-time T / AP / MS are the product's); experiment builds (tools/xp.py) hold only the instances the C2 / C4
// workloads use, in this one translation unit; the product looks the instance up in bb_inst_*.hip.
// os: the instance has the optimiser compiled in (k_res / k_stream<.., OS = true>, bb_opt_apply<0, 0>) -- wanted where the handle runs
// TruncatedADAGrad with resum_every == 0 and one sample per step without the ELBO trace (BB_TUNE_OPT_SPEC=0: never), chosen where the
// shape has such an instance: the compile-time-T k_res instances, k_stream's; the emulation has both forms of every one-sample shape.
// The one-GPU OS instances of k_res for the fitness / multienv / genotype kinds with a compile-time T run the one-wave consume + finish
// (br_consume_finish, k_res's br_fin_T): it is written for ONE replicate and one polling thread group -- `ng` first-hop groups, 8 at most.
// Where a launch has more of either, the generic instance runs.
static bool fin_chain_shape(const bb_handle* h, bool xg, bool stream, int P) {
    const int T = uniform_T(h->M);
    return !stream && !xg && !br_any_parity(h->M) && h->M.kind <= 2 && P <= 2 && (T == 8 || T == 6);
}
static const void* resident_instance(const bb_handle* h, bool xg, bool stream, int P, bool ms, int ng, std::string& name, bool& os) {
    const int kind = h->M.kind, nthr = h->nthr, T = uniform_T(h->M);
    const bool ap = br_any_parity(h->M);
    const bool fin_ok = !fin_chain_shape(h, xg, stream, P) || (h->M.R == 1 && ng <= 8);
    const bool want_os = h->tune.opt_spec != 0 && !ms && h->o.optimizer == BB_OPT_TRUNCATED_ADAGRAD && h->o.resum_every == 0 && fin_ok;
    os = false;
#if defined(BB_EMU)
    os = want_os;
    char nm[64];
    if (stream) snprintf(nm, sizeof nm, "emu:k_stream<%d,%d,%d%s>", kind, nthr, T, ms ? ",true" : "");
    else snprintf(nm, sizeof nm, "emu:k_res<%d,%d,%d,%s,*,%s,%s>", kind, P, nthr, xg ? "true" : "false", ap ? "true" : "false", ms ? "true" : "false");
    name = nm;
    return nullptr;
#elif defined(BB_FAST_BUILD)
    name = "(experiment build)";
    if (xg || ms) return nullptr;
    auto fn = [](auto k) { return (const void*)k; };
    if (stream) {
        if (nthr == 1024 && kind == 0 && T == 8) return fn(k_stream<0, 1024, 8>);
        if (nthr == 1024 && kind == 2 && T == 8) return fn(k_stream<2, 1024, 8>);
        if (nthr == 1024 && kind == 3 && T == 6) return fn(k_stream<3, 1024, 6>);
        return nullptr;
    }
    if (ap) {
        if (nthr > 512 && P == 1 && kind == 0) return fn(k_res<0, 1, 1024, false, 0, true>);
        if (nthr > 256 && nthr <= 512 && P == 3 && kind == 3) return fn(k_res<3, 3, 512, false, 0, true>);
        return nullptr;
    }
    // (the OS forms of the C2 / C4 / C5-rank instances, so that stamps and A/B runs are of the instance the product launches)
    if (want_os && nthr > 512 && P == 1) {
        os = true;
        if (kind == 0 && T == 8) return fn(k_res<0, 1, 1024, false, 8, false, false, true>);
        if (kind == 1 && T == 6) return fn(k_res<1, 1, 1024, false, 6, false, false, true>);
        if (kind == 2 && T == 8) return fn(k_res<2, 1, 1024, false, 8, false, false, true>);
        os = false;
    }
    if (nthr > 512 && P == 1 && kind == 0) return T == 8 ? fn(k_res<0, 1, 1024, false, 8>) : fn(k_res<0, 1, 1024, false>);
    if (nthr > 512 && P == 1 && kind == 1) return T == 6 ? fn(k_res<1, 1, 1024, false, 6>) : fn(k_res<1, 1, 1024, false>);
    if (nthr > 256 && nthr <= 512 && P == 2 && kind == 0) return T == 8 ? fn(k_res<0, 2, 512, false, 8>) : fn(k_res<0, 2, 512, false>);
    if (nthr > 256 && nthr <= 512 && P == 3 && kind == 3) return T == 6 ? fn(k_res<3, 3, 512, false, 6>) : fn(k_res<3, 3, 512, false>);
    if (nthr > 256 && nthr <= 512 && P == 2 && kind == 3) return T == 6 ? fn(k_res<3, 2, 512, false, 6>) : fn(k_res<3, 2, 512, false>);
    if (nthr > 512 && P == 1 && kind == 2) return T == 8 ? fn(k_res<2, 1, 1024, false, 8>) : fn(k_res<2, 1, 1024, false>);
    return nullptr;
#else
    const char* nm = "";
    const void* k = nullptr;
    if (want_os) k = stream ? (const void*)bb_stream_instance_os(kind, nthr, T, &nm) : (ap ? nullptr : (const void*)bb_res_instance_os(kind, P, nthr, xg, T, &nm));
    if (k) os = true;
    else if (stream) k = ms ? (const void*)bb_stream_instance_ms(kind, nthr, T, &nm) : (const void*)bb_stream_instance(kind, nthr, T, &nm);
    else switch (kind) {
        case 0: k = (const void*)bb_res_instance_k0(P, nthr, xg, T, ap, ms, &nm); break;
        case 1: k = (const void*)bb_res_instance_k1(P, nthr, xg, T, ap, ms, &nm); break;
        case 2: k = (const void*)bb_res_instance_k2(P, nthr, xg, T, ap, ms, &nm); break;
        case 3: k = (const void*)bb_res_instance_k3(P, nthr, xg, T, ap, ms, &nm); break;
        default: k = (const void*)bb_res_instance_k4(P, nthr, xg, T, ap, ms, &nm);
    }
    name = nm;
    return k;
#endif
}
static const void* persist_instance(const bb_handle* h, bool xg, int P, std::string& name) {
#if defined(BB_EMU)
    char nm[48];
    snprintf(nm, sizeof nm, "emu:k_persist<%d,%d,%d>", h->M.kind, P, h->nthr);
    name = nm;
    return nullptr;
#elif defined(BB_FAST_BUILD)
    name = "(experiment build)";
    if (!xg && h->nthr > 512 && P == 1 && h->M.kind == 0) return (const void*)k_persist<0, 1, 1024>;
    return nullptr;
#else
    const char* nm = "";
    const void* k = (const void*)bb_persist_instance(h->M.kind, P, h->nthr, xg, &nm);
    name = nm;
    return k;
#endif
}

// pairs a tile can hold: every segment contributes count/2 + 1 at most
static long long tile_pairs_bound(const DevModel& M, long long NB) {
    long long p = 0;
    for (int r = 0; r < M.R; ++r) p += NB * M.T[r] / 2 + 1;
    if (M.kind == 0 || M.kind == 1) p += 2 * (NB * M.E / 2 + 1);
    else if (M.kind == 2) p += 3 * (NB / 2 + 1);
    else if (M.kind == 3) p += (NB / 2 + 1) + 3ll * M.R * (NB / 2 + 1);
    else p += (NB * M.E / 2 + 1) + 3ll * M.R * (NB * M.E / 2 + 1);
    p += 2 * (M.nt1 / 2 + 1);
    return p;
}

// device copies of the descriptors (kernels read them through pointers); re-sent whenever the host copy changes
static int sync_descriptors(bb_handle* h) {
    int rc;
    if (!h->dM && ((rc = dalloc(h, &h->dM, 1)) || (rc = dalloc(h, &h->dS, 1)) || (rc = dalloc(h, &h->dL, 1)))) return rc;
    if ((rc = h2d(h->dM, &h->M, sizeof(DevModel), h->stream)) || (rc = h2d(h->dS, &h->S, sizeof(DevState), h->stream))) return rc;
    h->Lp = bb_lds_layout(h->M.R, h->M.E, h->M.kind, h->M.Ttot, h->M.nt1, h->M.K, h->NB, h->nthr, 1);   // the resident launch's carve-up
    if ((rc = h2d(h->dL, &h->Lp, sizeof(BBLds), h->stream))) return rc;
    if (!h->dY && (rc = dalloc(h, &h->dY, 1))) return rc;
    return h2d(h->dY, &h->Yh, sizeof(BRLay), h->stream);
}

// ------------------------------------------------------------------------------------------------
// the decision
// ------------------------------------------------------------------------------------------------
// What plan_launch decided: the plan and what install_plan puts into the handle and onto the device beside it.  While a candidate is
// being built it also carries what one stage hands the next.
struct Planned {
    LaunchPlan plan;
    bool xg = false;                   // the cross-GPU leg is (to be) on
    int NB0 = 0, nblk0 = 0;            // k_res / k_stream: the base tile map (before leader tiles and genotype cuts)
    BRLay Y{};                         // ... the LDS carve-up
    size_t lds_doubles = 0;            // dynamic LDS of the resident launch
    std::vector<long long> tb;         // genotype model, k_res: the tile table (build_geno_tiles)
    std::vector<int> tg;
    bool scratch = false;              // the launch needs the sample scratch (ensure_scratch)
    std::vector<double> segtab;        // the host-built tables (host_tables; empty: the kernels build their own)
    std::vector<int> ldstab;
    int segtab_stride = 0;
};

// the two-kernel step on the handle's own tile map: the plan where nothing resident is wanted or possible, and every candidate's start
static LaunchPlan two_kernel_plan(const bb_handle* h) {
    LaunchPlan p;
    p.NB = h->NB;
    p.nblk = h->nblk;
    p.name = step_kernels_name(h->M.kind);
    // several MC samples per step (Turing.ADVI(samples_per_step, ..), src/vi.jl:98) and ELBO recording: k_res's MS instances (round 4: sharded too --
    // every sample is an exchange of its own, the inbox epochs count exchanges)
    p.ms = h->o.samples_per_step != 1 || h->o.elbo_every != 0;
    return p;
}

// the base tile map of k_res / k_stream
static void base_tile_map(const bb_handle* h, Planned& c) {
    const bool nb_set = h->tune.nb_set;
    const int res_nb = h->tune.res_nb;
    const long long nbar = std::max<long long>(h->b_hi - h->b_lo, 1);
    // The two-kernel step may run more tiles than the device has compute units (its tiles must fit LDS with ITS tables: config 5 on one
    // GPU runs 512 of them); a resident launch needs every tile resident -- one per compute unit: its own base map then
    c.NB0 = h->NB;
    c.nblk0 = h->nblk;
    if (c.nblk0 > h->cus && !nb_set) { c.NB0 = (int)((nbar + h->cus - 1) / h->cus); c.nblk0 = (int)((nbar + c.NB0 - 1) / c.NB0); }
    // BB_TUNE_RES_NB (tests): the resident launch's own tile size -- a cut of a BASELINE problem with the full-size tile geometry even where
    // the two-kernel step's tables would not fit such a tile (config 5 on one GPU: 782 barcodes per tile)
    if (res_nb > 0) { c.NB0 = res_nb; c.nblk0 = (int)((nbar + c.NB0 - 1) / c.NB0); }
    c.plan.NB = c.NB0;
    c.plan.NBL = 0;
    c.plan.nblk = c.nblk0;
}

// Groups of the exchange's first hop.  Round 2: 16 on one GPU (a leader then fetched its 16 members' rows in one round of loads, the
// consume ran on two thread groups).  Round 3, tagged rows + leaders that poll their members in chunks of eight on as many thread
// groups as the tile has (bbp_leader_reduce_tg, PAR): 8 groups of 32 are ONE round of polls where the tile has four thread groups, and
// every tile's consume is one thread group's eight loads -- C2 82.7 -> 83.5 k steps/s, C4 94.1 -> 94.9 k, C3 57.1 -> 57.7 k against 16
// (profiles/r03g_parallel_leaders).  The cross-GPU inbox protocol is laid out for 8.  BB_TUNE_NG overrides (8 or 16).
static bool first_hop_groups(const bb_handle* h, Planned& c) {
    const int want = h->tune.ng;
    if (h->M.K + 2 * h->M.nt1 > h->nthr) return false;      // (one thread per row entry: bbp_consume_tg / _tgx, the leaders' chunk sums)
    const int KK = h->M.K + 2 * h->M.nt1;
    const bool can16 = !c.xg && c.nblk0 >= 64 && KK <= 128 && h->nthr >= 2 * (KK <= 64 ? 64 : 128);
    int ng = (can16 && h->nthr < 4 * ((KK + 63) & ~63)) ? 16 : 8;
    if (want == 8 || (want == 16 && !c.xg && KK <= 128 && h->nthr >= 2 * (KK <= 64 ? 64 : 128))) ng = want;
    // a leader takes its members' rows in batches of eight loads per lane -- 32 groups of 8 on a full grid: one batch, one round trip
    // (the tile's consume then runs on four thread groups)
    if (want == 32 && !c.xg && c.nblk0 >= 64 && h->nthr >= 4 * ((KK + 63) & ~63)) ng = 32;
    c.plan.ng = ng;
    return true;
}

// tile map: leaders (tiles 0 .. 7) hold `frac` of a tile's barcodes (br_tile); BB_TUNE_LEAD=100 keeps all tiles alike
static void leader_tiles(const bb_handle* h, Planned& c) {
    const int pct = h->tune.lead;
    const bool lead_set = h->tune.lead_set, nb_fixed = h->tune.nb_set || h->tune.res_nb > 0;
    const int ng = c.plan.ng;
    if (!(pct < 100 && c.nblk0 >= 2 * ng && (!nb_fixed || lead_set))) return;
    const long long nbar = std::max<long long>(h->b_hi - h->b_lo, 1);
    int NB = c.NB0;
    if (!nb_fixed) {
        const double tiles = (double)c.nblk0 - (double)ng * (1.0 - pct / 100.0);      // in units of a full tile
        NB = (int)std::ceil((double)nbar / tiles);
    }
    const int NBL = std::max(1, (int)(NB * (pct / 100.0)));
    const long long rest = nbar - (long long)ng * NBL;
    const int nblk = ng + (int)((std::max<long long>(rest, 0) + NB - 1) / NB);
    const long long p_uni = (br_tile_span(h->M, c.NB0, true) + h->nthr - 1) / h->nthr, p_new = (br_tile_span(h->M, NB, true) + h->nthr - 1) / h->nthr;
    // stay uniform where rounding pushed the map over the grid that fits, or the slightly larger tiles need another pair slot
    if (nblk > c.nblk0 + (nb_fixed ? 8 : 0) || p_new > p_uni) return;
    c.plan.NB = NB;
    c.plan.NBL = NBL;
    c.plan.nblk = nblk;
}

// Genotype model: the tile table of k_res (br_tile_geno) -- tiles of at most NB barcodes (the first ng, the leaders: NBL, if > 0) whose
// cuts inside the mutants fall on genotype boundaries; tg[i] = first genotype tile i owns.  False if a genotype does not fit a tile.
static bool build_geno_tiles(const bb_handle* h, int NB, int NBL, int ng, std::vector<long long>& tb, std::vector<int>& tg) {
    const DevModel& M = h->M;
    const std::vector<int>& ptr = h->geno_ptr_h;
    auto geno_of = [&](long long m) { return (int)(std::upper_bound(ptr.begin(), ptr.end(), (int)m) - ptr.begin()) - 1; };
    auto gcut = [&](long long b) { return (b <= M.nn || b <= h->b_lo) ? h->g_lo : (b >= h->b_hi ? h->g_hi : geno_of(b - M.nn)); };
    tb.clear();
    tg.clear();
    long long b = h->b_lo;
    while (b < h->b_hi) {
        const int cap = (NBL > 0 && tb.size() < (size_t)ng) ? NBL : NB;
        long long e = std::min<long long>(b + cap, h->b_hi);
        if (e < h->b_hi && e > M.nn) {
            e = M.nn + ptr[(size_t)geno_of(e - M.nn)];       // back to the first mutant of the genotype the cut fell into
            if (e <= b) return false;
        }
        tb.push_back(b);
        tg.push_back(gcut(b));
        b = e;
    }
    if (tb.empty()) { tb.push_back(h->b_lo); tg.push_back(h->g_lo); }
    tb.push_back(h->b_hi);
    tg.push_back(h->g_hi);
    for (size_t i = 0; i + 1 < tg.size(); ++i) if (tg[i + 1] - tg[i] > NB) return false;      // (theta stage table: NB entries)
    return NB < 32768;
}

// genotype model: the tile table, cut on genotype boundaries
static bool geno_tile_table(const bb_handle* h, Planned& c) {
    const bool nb_fixed = h->tune.nb_set || h->tune.res_nb > 0;
    if (h->M.kind != BB_MODEL_GENOTYPE) return true;
    // cuts on genotype boundaries leave tiles partly empty: grow the tile until the map fits the grid again
    const int limit = std::max(c.nblk0, std::min(c.nblk0 + 8, h->cus));
    const int NB = c.plan.NB, NBL = c.plan.NBL, ng = c.plan.ng;
    bool ok = false;
    for (int grow = 0; grow <= NB / 2 + 8 && !ok; ++grow) {
        const int nb = NB + grow, nbl = NBL > 0 ? std::max(1, (int)((long long)NBL * nb / NB)) : 0;
        if (build_geno_tiles(h, nb, nbl, ng, c.tb, c.tg) && (int)c.tb.size() - 1 <= limit) { ok = true; c.plan.NB = nb; c.plan.NBL = nbl; }
        else if (nb_fixed && NBL > 0 && build_geno_tiles(h, nb, 0, ng, c.tb, c.tg) && (int)c.tb.size() - 1 <= limit) { ok = true; c.plan.NB = nb; c.plan.NBL = 0; }
    }
    if (!ok) return false;
    c.plan.nblk = (int)c.tb.size() - 1;
    return !(c.xg && c.plan.nblk < 8);
}

// pair slots per thread, against the k_stream fallback
static bool pair_slots(const bb_handle* h, Planned& c) {
    const bool force_stream = h->tune.force_stream, no_stream = h->tune.no_stream;
    if (!c.xg && h->M.Dh != h->M.Dp) return false;      // (packed window rows: only the cross-GPU instances read the segments' differences)
    c.plan.P = (int)((br_tile_span(h->M, c.plan.NB, true) + h->nthr - 1) / h->nthr);
    c.plan.impl = IMPL_RES;
    // more pair slots than the register file holds: k_stream (bb_stream.h) -- the same tile map, the per-pair state streamed
    const int Pmax = h->nthr > 512 ? 2 : (h->nthr > 256 ? 3 : 4);
    if (!force_stream && c.plan.P <= Pmax) return true;        // (BB_TUNE_STREAM, tests: small shapes through k_stream)
    const int T0 = uniform_T(h->M);
    // every replicate the same even T (instances: 4, 6, 8), flat-index-aligned pairs, one GPU; several samples per step / the ELBO trace:
    // the MS instances (T = 6, 8 at 1024 threads; tests: 512).  A barcode takes a power-of-two number of lanes there: T = 6 four.
    const int Ps = (int)((br_tile_span(h->M, c.plan.NB, true, true) + h->nthr - 1) / h->nthr);
    if (!no_stream && !br_any_parity(h->M) && (T0 == 8 || T0 == 6 || T0 == 4) && h->nthr % 64 == 0 && !c.xg && Ps <= 64) {
        c.plan.impl = IMPL_STREAM;
        c.plan.P = Ps;
        c.scratch = h->o.samples_per_step > 1;      // (the samples' gradient sums live in gacc_mu / gacc_om)
        return true;
    }
    return c.plan.P <= Pmax;
}

// When the window slot is fetched (RunArgs.pf).  In the exchange's shadow (round 2) its 32 B per latent of HBM reads compete with
// the exchange's own loads and stores: at the start of the S pass instead, C2 73.1 -> 77.7 k steps/s, C4 87.1 -> 89.1 k
// (profiles/r03b_tagged_rows/prefetch_timing_on_lean_kernel.txt) -- where the slot buffer fits beside the moment contributions.
// (At the end of the previous step's G pass instead: tied with the start of the S pass on C2 and C4, same file.  Behind the exchange,
//  where there is no room for a slot buffer of its own: 6 % slower on C3 than in the exchange's shadow.)
static bool window_fetch_layout(const bb_handle* h, Planned& c) {
    const bool stream = c.plan.impl == IMPL_STREAM;
    const int xrows = c.xg ? 8 * h->o.world_size : 0;
    c.plan.pf = h->o.optimizer == BB_OPT_TRUNCATED_ADAGRAD && !stream ? 1 : 0;
    c.Y = br_layout(h->M, c.plan.NB, h->nthr, c.plan.P, xrows, c.plan.pf == 1, stream);
    if (c.plan.pf != 0 && (size_t)c.Y.total * 8 > 160 * 1024) { c.plan.pf = 0; c.Y = br_layout(h->M, c.plan.NB, h->nthr, c.plan.P, xrows, false); }      // (no room for a slot buffer of its own: in the exchange's shadow)
    c.lds_doubles = (size_t)c.Y.total;
    return c.lds_doubles * 8 <= 160 * 1024;
}

// the kernel instance, whether its grid fits resident on the device, and the handle's buffers the tile map
static bool instance_fits(const bb_handle* h, Planned& c) {
    c.plan.fn = resident_instance(h, c.xg, c.plan.impl == IMPL_STREAM, c.plan.P, c.plan.ms, c.plan.ng, c.plan.name, c.plan.os);
    if (resident_fit(c.plan.fn, h->nthr, c.lds_doubles * 8, c.plan.nblk, h->cus)) return false;
    return c.plan.nblk <= h->tile_cap;       // (else: more tiles than the exchange, stamp, xsel and tile-table buffers hold)
}

// The tables a tile of k_res / k_stream needs before its first step, built HERE instead of in every launch's prologue (where
// thread 0 of each tile spent 3.4 us on its segment table behind a chain of scalar loads, and the per-lane descriptor loads of the
// LDS tables another 1.8 us -- profiles/r03z_round3_final/fixed_cost.txt): per tile its segment table (br_build_segs, the same code),
// once the tile-independent LDS tables (br_table_*).  BB_NO_HOST_TABLES=1: the kernels build them (A/B).
template <int KIND>
static void host_tables_kind(const bb_handle* h, const RunArgs& A, const DevState& Sh, Planned& c) {
    for (int b = 0; b < A.nblk; ++b) {
        const BBTile t = KIND == 2 ? br_tile_geno(h->M, Sh, b, c.plan.NB) : br_tile(h->M, A, b, c.plan.NB);
        const int g0 = KIND == 2 ? Sh.tile_g[b] : 0, g1 = KIND == 2 ? Sh.tile_g[b + 1] : 0;
        double* rec = c.segtab.data() + (size_t)b * c.segtab_stride;
        const int n = br_build_segs<KIND>((BRSeg*)rec, h->M, c.Y, t, b == 0, g0, g1);
        ((int*)(rec + c.segtab_stride - 1))[0] = n;
    }
}
static void host_tables(const bb_handle* h, Planned& c) {
    const bool off = h->tune.no_host_tables;
    if (off) return;
    const DevModel& M = h->M;
    c.segtab_stride = BR_SEG_DOUBLES * (4 + 4 * M.R + 1) + 1;
    RunArgs A = make_args(h, 0, 0, 1, true, false);
    A.nblk = c.plan.nblk; A.nbl = c.plan.NBL; A.ng = c.plan.ng;
    DevState Sh = h->S;
    Sh.tile_b = c.tb.data();
    Sh.tile_g = c.tg.data();
    c.segtab.assign((size_t)c.plan.nblk * c.segtab_stride, 0.0);
    by_kind(M.kind, [&](auto kindc) { host_tables_kind<decltype(kindc)::value>(h, A, Sh, c); });
    const int K = M.K, Tt = M.Ttot, R = M.R;
    c.ldstab.assign((size_t)3 * K + 4 * Tt + 4 * R + 4, 0);
    for (int j = 0; j < K; ++j) br_table_row(M, c.Y, j, &c.ldstab[2 * j], &c.ldstab[2 * K + j]);
    for (int j = 0; j < Tt; ++j) br_table_time(M, c.Y.L, j, &c.ldstab[3 * K + 4 * j]);
    for (int r = 0; r < R; ++r) br_table_rep(M, c.Y, r, &c.ldstab[3 * K + 4 * Tt + 4 * r]);
}

// the owner-computes launch (bb_resident.h) where the shape allows it; BB_NO_RES=1 keeps k_persist (A/B runs)
// any_parity: also the AP instances (odd time-point counts, odd loglambda offset).  Measured (C2-sized fitness_normal with 7 / 5
// time points, the fifth model): they are 1 - 5 % SLOWER than k_persist -- parity is a run-time property of every pair there,
// 45 spilled registers and two Philox draws in divergent lanes -- so plan_launch asks for them only where k_persist cannot
// run: the genotype model (whose other choice is the two-kernel step) or after k_persist has refused the shape.
// k_res or k_stream for this handle's shape, with its own tile map: true and `out` filled in where one fits
static bool plan_resident(const bb_handle* h, bool xg, bool any_parity, Planned& out) {
    const bool no_res = h->tune.no_res;
    if (no_res || !br_eligible(h->M) || (!any_parity && br_any_parity(h->M))) return false;
    Planned c;
    c.plan = two_kernel_plan(h);
    c.xg = xg;
    base_tile_map(h, c);
    if (!first_hop_groups(h, c)) return false;
    leader_tiles(h, c);
    if (!geno_tile_table(h, c) || !pair_slots(h, c) || !window_fetch_layout(h, c) || !instance_fits(h, c)) return false;
    host_tables(h, c);
    out = std::move(c);
    return true;
}

// k_persist on the two-kernel step's tile map: nullptr and `out` filled in, or why not
static const char* plan_persist(const bb_handle* h, bool xg, Planned& out) {
    Planned c;
    c.plan = two_kernel_plan(h);
    c.xg = xg;
    if (c.plan.ms) return h->o.samples_per_step != 1 ? "samples_per_step != 1 and the shape has no owner-computes instance" : "ELBO recording is on and the shape has no owner-computes instance";
    if (h->M.kind == BB_MODEL_GENOTYPE)
        return h->M.geno_sorted ? "genotype model: no tile map with whole genotypes per tile fits the device" : "genotype model: geno_idx is not in consecutive runs (a tile must hold whole genotypes)";
    int P = (int)((tile_pairs_bound(h->M, h->NB) + h->nthr - 1) / h->nthr);
    if (P == 3 && h->nthr > 512) P = 4;      // (no 3-pair instance at 1024 threads; 4 is refused just below)
    if (xg && P != 1) return "sharded resident launch holds one pair per thread";
    if (P > (h->nthr > 512 ? 2 : 4)) return "tile too large for the register-resident state";
    c.lds_doubles = h->lds_doubles_p0 + (size_t)3 * P * h->nthr;        // drawn-ahead normals (16 B / pair) + cached counts (8 B)
    c.plan.impl = IMPL_PERSIST;
    c.plan.P = P;
    c.plan.fn = persist_instance(h, xg, P, c.plan.name);
    if (c.lds_doubles * 8 > PERSIST_LDS_CAP) return "tile does not fit LDS with the lambda table";
    if (const char* why = resident_fit(c.plan.fn, h->nthr, c.lds_doubles * 8, h->nblk, h->cus)) return why;
    out = std::move(c);
    return nullptr;
}

// The plan for launch_mode `mode` (0: resident where possible, 1: two kernels, 2: resident or plan.why says why not) with the
// cross-GPU leg on (xg) or off.  The candidates in the order they are tried; the first that fits is the plan.
static Planned plan_launch(const bb_handle* h, int mode, bool xg) {
    const bool no_persist = h->tune.no_persist, force_allreduce = h->tune.force_allreduce, any_parity = h->tune.any_parity;
    Planned c;
    c.plan = two_kernel_plan(h);
    c.xg = xg;
    if (mode == 1 || (no_persist && mode == 0)) return c;      // no resident launch wanted
    auto two_kernels = [&](const char* why) { c.plan.why = why; return c; };
    // what rules out every resident launch (k_res's own tile map never has fewer tiles than this one)
    if (force_allreduce || (h->o.world_size != 1 && !xg)) return two_kernels("sharded run");
    if (xg && h->nblk < 8) return two_kernels("fewer than 8 tiles on this rank");
    // 1. k_res or k_stream; the any-parity instances only where k_persist is no choice
    const bool ap_first = c.plan.ms || h->M.kind == BB_MODEL_GENOTYPE || any_parity;
    Planned r;
    if (plan_resident(h, xg, ap_first, r)) return r;
    // 2. k_persist
    const char* why = plan_persist(h, xg, r);
    if (!why) return r;
    // 3. k_persist cannot (tile too large for its state, no instance, sharded with more than one pair per thread ...): k_res's
    // any-parity instances as the second chance
    if (!ap_first && plan_resident(h, xg, true, r)) return r;
    // 4. the two-kernel step, and why
    return two_kernels(why);
}
// ... as bb_create and bb_p2p_enable ask for it: launch_mode 2 without a resident launch is an error that says why not
static int plan_or_refuse(const bb_handle* h, int mode, bool xg, Planned& out) {
    out = plan_launch(h, mode, xg);
    return mode == 2 && out.plan.why ? bb_fail(BB_ERR_UNSUPPORTED, "launch_mode = 2 (persistent) not possible: %s", out.plan.why) : 0;
}

// ------------------------------------------------------------------------------------------------
// the installation
// ------------------------------------------------------------------------------------------------
// Everything a plan changes in the handle and on the device: the genotype tile table, the LDS carve-up and size, the sample scratch,
// the host-built tables, h->plan.  The callers send the descriptors afterwards (sync_descriptors).  A failed allocation or copy
// leaves the two-kernel plan and null table pointers.
static int install_plan(bb_handle* h, const Planned& c) {
    h->plan = two_kernel_plan(h);
    h->S.segtab = nullptr;
    h->S.ldstab = nullptr;
    h->S.segtab_stride = 0;
    if (c.plan.impl == IMPL_TWO_KERNEL) { h->plan = c.plan; return 0; }
    int rc;
    if (!c.tb.empty()) {
        if (!h->d_tile_b && ((rc = dalloc(h, &h->d_tile_b, (size_t)h->tile_cap + 2)) || (rc = dalloc(h, &h->d_tile_g, (size_t)h->tile_cap + 2)))) return rc;
        if ((rc = h2d(h->d_tile_b, c.tb.data(), c.tb.size() * 8, h->stream)) || (rc = h2d(h->d_tile_g, c.tg.data(), c.tg.size() * 4, h->stream))) return rc;
        h->S.tile_b = h->d_tile_b;
        h->S.tile_g = h->d_tile_g;
    }
    if (c.scratch && (rc = ensure_scratch(h))) return rc;
    if (!c.segtab.empty()) {
        // (the handle keeps one buffer of each, sized for the largest tile map it has seen)
        if (c.segtab.size() > h->segtab_cap) { double* d = nullptr; if ((rc = dalloc(h, &d, c.segtab.size()))) return rc; h->d_segtab = d; h->segtab_cap = c.segtab.size(); }
        if (c.ldstab.size() > h->ldstab_cap) { int* d = nullptr; if ((rc = dalloc(h, &d, c.ldstab.size()))) return rc; h->d_ldstab = d; h->ldstab_cap = c.ldstab.size(); }
        if ((rc = h2d(h->d_segtab, c.segtab.data(), c.segtab.size() * 8, h->stream)) || (rc = h2d(h->d_ldstab, c.ldstab.data(), c.ldstab.size() * 4, h->stream))) return rc;
        h->S.segtab = h->d_segtab;
        h->S.segtab_stride = c.segtab_stride;
        h->S.ldstab = h->d_ldstab;
    }
    if (c.plan.impl >= IMPL_RES) h->Yh = c.Y;
    h->lds_doubles_p = c.lds_doubles;
    h->plan = c.plan;
    return 0;
}


// the arguments of the planned resident launch: its tile map (k_persist's is the two-kernel one), every sample an exchange of its own
// (k_persist runs one sample per step)
static RunArgs resident_args(const bb_handle* h) {
    RunArgs A = make_args(h, h->step, 0, h->o.samples_per_step, true, false);
    A.nblk = h->plan.nblk; A.nbl = h->plan.NBL; A.ng = h->plan.ng; A.pf = h->plan.pf;
    return A;
}
