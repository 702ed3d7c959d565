// bb_analysis.h -- host side of the post-fit entry points: bb_hier_fitness (bb_hier.h), bb_logdensity_grad_batch (bb_logp.h),
// bb_ppc_bands (bb_ppc.h), bb_freq_bands (bb_freq.h), bb_ppc_score (bb_score.h), bb_ppc_loo (bb_loo.h), bb_fitness_rb, bb_theta_rb, bb_popmean_rb (bb_rb.h),
// bb_contrast_rb (bb_contrast.h), bb_dfe_rb (bb_dfe.h), bb_fitness_rank (bb_rank.h), bb_logsigma_rb (bb_lsrb.h), bb_logtau_rb (bb_ltrb.h), bb_loglambda_rb (bb_llrb.h; the three over bb_gridmix.h), bb_chain_summary (bb_chain.h) and the iterate trace's bb_trace_* (bb_trace.h).  None of them touches the step loop.
// Included only by bb_engine.hip, once, after the handle's own entry points, which it uses: the same translation unit, built by
// hipcc and by g++ -DBB_EMU -x c++ like the rest of the engine.

// the handle whose device, stream and buffers a post-fit call works on: a group samples on its first shard
static bb_handle* sampling_handle(bb_handle* h) { return h->shards.empty() ? h : h->shards[0]; }

// One statement of a device buffer's layout.  A layout is a function that names every sub-buffer once, in order, as the pointer it
// lands in and its length in doubles (an int array behind the doubles: its length rounded up to whole doubles); carve() runs it
// once to size the buffer and once more, after the buffer has grown, to place the pointers.
struct Carve {
    double* base;              // nullptr: the sizing pass
    size_t n = 0;              // doubles taken so far
    template <class T>
    void operator()(T*& p, size_t doubles) {
        if (base) p = (T*)(base + n);
        n += doubles;
    }
};
template <class L>
static int carve(DevBuf& b, L&& layout) {
    Carve size{nullptr};
    layout(size);
    int rc = b.grow(size.n);
    if (rc) return rc;
    Carve place{b.p};
    layout(place);
    return BB_OK;
}

// The order statistics StatsBase.quantile takes (Statistics._quantile, alpha = beta = 1) for n probabilities of a column of K:
// aleph = K p + (1 - p), j = clamp(trunc(aleph), 1, K - 1), gamma = clamp(aleph - j, 0, 1), a + gamma (b - a) between the (1-based)
// order statistics j and j + 1.  P.gam[e] = gamma, P.tgt[0 .. n_tgt) = the distinct 0-based ranks in ascending order, P.plo[e] = the
// index into tgt of entry e's lower order statistic.
static void quantile_plan(long long K, const double* probs, int n, PpcArgs& P) {
    std::vector<int> lo((size_t)n), ranks;
    for (int e = 0; e < n; ++e) {
        const double p = probs[e];
        const double aleph = (double)K * p + (1.0 - p);
        const long long j = std::min<long long>(std::max<long long>((long long)aleph, 1), K - 1);
        P.gam[e] = std::min(std::max(aleph - (double)j, 0.0), 1.0);
        lo[(size_t)e] = (int)(j - 1);
        ranks.push_back((int)(j - 1));
        ranks.push_back((int)j);
    }
    std::sort(ranks.begin(), ranks.end());
    ranks.erase(std::unique(ranks.begin(), ranks.end()), ranks.end());
    P.n_tgt = (int)ranks.size();
    for (int x = 0; x < P.n_tgt; ++x) P.tgt[x] = ranks[(size_t)x];
    for (int e = 0; e < n; ++e) P.plo[e] = (int)(std::lower_bound(ranks.begin(), ranks.end(), lo[(size_t)e]) - ranks.begin());
}

// ---- derived fitness of the hierarchical models (bb_hier.h) ---------------------------------------------------------------------
extern "C" int64_t bb_hier_units(const bb_handle* h) {
    if (!h || h->M.kind < BB_MODEL_GENOTYPE) return 0;
    return h->M.blk_hi[BK_TT] - h->M.blk_lo[BK_TT];
}

static int hier_fitness_raw(bb_handle* h, int32_t n_samples, uint64_t seed, double* median, double* stdv) {
    if (!h->shards.empty()) {
        // the whole posterior onto shard 0 (entries it does not own are dead weight there: never read by its tiles), then its sampler
        bb_handle* s0 = h->shards[0];
        const size_t D = (size_t)h->M.D;
        std::vector<double> mu(D), om(D);
        int rc = group_get_params(h, mu.data(), om.data());
        BB_ENTER(s0);
        if (!rc) rc = h2d(s0->S.mu, mu.data(), D * 8, s0->stream);
        if (!rc) rc = h2d(s0->S.om, om.data(), D * 8, s0->stream);
        return rc ? rc : hier_fitness_raw(s0, n_samples, seed, median, stdv);
    }
    BB_ENTER(h);
    if (h->M.kind < BB_MODEL_GENOTYPE) return bb_fail(BB_ERR_INVALID, "bb_hier_fitness applies to the hierarchical models only");
    if (n_samples < 2 || n_samples > 16384) return bb_fail(BB_ERR_UNSUPPORTED, "n_samples must be in 2..16384");
    // (a shard of a sharded run keeps full-length parameter arrays but only its own barcodes' entries are current: the caller makes them
    //  whole first -- bb_set_params with the gathered vector, as barbay.jl_amd.vi does -- the draws are then those of a whole-problem handle)
    const long long n = bb_hier_units(h);
    const size_t D = (size_t)h->M.D;
    int rc;
    if ((rc = ensure_scratch(h))) return rc;
    // posterior sigma = softplus(omega) into the (free between steps) z scratch array
    std::vector<double> om(D);
    if ((rc = dsync(h->stream)) || (rc = d2h(om.data(), h->S.om, D * 8, h->stream))) return rc;
    for (size_t i = 0; i < D; ++i) om[i] = host_softplus(om[i]);
    if ((rc = h2d(h->S.zsv, om.data(), D * 8, h->stream))) return rc;
    HierArgs H;
    memset(&H, 0, sizeof H);
    H.mean = h->S.mu;
    H.sigma = h->S.zsv;
    H.median_out = h->S.asv;           // n <= D: scratch arrays are free between steps
    H.std_out = h->S.hsv;
    H.n_units = n;
    H.lo_theta = h->M.blk_lo[BK_S];
    H.lo_tt = h->M.blk_lo[BK_TT];
    H.lo_lt = h->M.blk_lo[BK_LT];
    H.theta_mod = h->M.kind == BB_MODEL_GENOTYPE ? 0 : (h->M.blk_hi[BK_S] - h->M.blk_lo[BK_S]);
    H.geno_idx = h->M.geno_idx;
    H.n_samples = n_samples;
    H.n_pad = 2;
    while (H.n_pad < n_samples) H.n_pad <<= 1;
    H.seed = seed;
    const int nthr = H.n_pad >= 2048 ? 1024 : 256;
    const size_t lds = (size_t)H.n_pad + nthr + 8;
    const int nb = (int)std::min<long long>(n, 2048);
    if ((rc = launch(h->stream, k_hier, nb, nthr, lds, H))) return rc;
    if ((rc = d2h(median, H.median_out, (size_t)n * 8, h->stream))) return rc;
    return d2h(stdv, H.std_out, (size_t)n * 8, h->stream);
}
extern "C" int bb_hier_fitness(bb_handle* h, int32_t n_samples, uint64_t seed, double* median, double* stdv) {
    if (!h || !median || !stdv) return bb_fail(BB_ERR_INVALID, "null argument");
    if (h->perm_m.empty()) return hier_fitness_raw(h, n_samples, seed, median, stdv);
    const size_t n = h->perm_m.size();          // (genotype model: one unit per mutant)
    std::vector<double> a(n), b(n);
    int rc = hier_fitness_raw(h, n_samples, seed, a.data(), b.data());
    if (rc) return rc;
    for (size_t m = 0; m < n; ++m) { median[(size_t)h->perm_m[m]] = a[m]; stdv[(size_t)h->perm_m[m]] = b[m]; }
    return BB_OK;
}

// ---- log-joint and gradient at a batch of points (bb_logp.h) --------------------------------------------------------------------
// the launches that evaluate B's points (B.W of them) into B.logp and B.grad; shared with the HMC session (bb_hmc_host.h)
static int logp_launch(bb_handle* h, const LogpArgs& B) {
    const DevModel& M = h->M;
    const RunArgs A = make_args(h, 0, 0, 1, false, true);
    const int grid = h->nblk * B.W;
    int rc = 0;
    by_kind(M.kind, [&](auto kindc) {
        constexpr int KIND = decltype(kindc)::value;
        rc = launch(h->stream, k_logp_moments<KIND>, grid, h->nthr, h->lds_doubles, desc_ptr(h->dM, &h->M), B, A, h->NB);
        if (!rc) rc = launch(h->stream, k_logp_grad<KIND>, grid, h->nthr, h->lds_doubles, desc_ptr(h->dM, &h->M), B, A, h->NB);
    });
    if (rc) return rc;
    if (M.kind == BB_MODEL_GENOTYPE) {
        const int gsb = (int)std::min<long long>((M.G + 31) / 32, 1024);      // 32 genotypes per 256-thread block (as k_geno_sum)
        if ((rc = launch(h->stream, k_logp_geno, gsb * B.W, 256, 256, desc_ptr(h->dM, &h->M), B, gsb))) return rc;
    }
    return BB_OK;
}
// the constant of the log-joint (the ELBO's constant carries the entropy's: not part of the log-joint)
static double logp_const(const bb_handle* h) { return h->elbo_const - 0.5 * (double)h->M.D * (1.0 + BB_LOG2PI); }
// n_points points in one call: three launches on buffers of the handle's own, the variational state untouched.  Caller's order <->
// the handle's order once per batch, on the host.
extern "C" int bb_logdensity_grad_batch(bb_handle* h, int32_t n_points, const double* z, double* logp, double* grad) {
    if (!h || !z) return bb_fail(BB_ERR_INVALID, "null argument");
    if (n_points < 1 || n_points > BB_LOGP_MAX_BATCH) return bb_fail(BB_ERR_INVALID, "n_points = %d is outside 1 .. %d", (int)n_points, BB_LOGP_MAX_BATCH);
    BB_GROUP_UNSUPPORTED(h, "bb_logdensity_grad_batch");
    if (h->o.world_size > 1) return bb_fail(BB_ERR_UNSUPPORTED, "bb_logdensity_grad_batch is not available on a sharded handle (world_size > 1)");
    BB_ENTER(h);
    const DevModel& M = h->M;
    const size_t W = (size_t)n_points, D = (size_t)M.D, Dz = (D + 1) & ~(size_t)1, Wp = (W + 1) & ~(size_t)1;
    const bool geno = M.kind == BB_MODEL_GENOTYPE;
    const size_t nbs = geno ? ((size_t)M.nb + 1) & ~(size_t)1 : 0, Gs = geno ? ((size_t)M.G + 1) & ~(size_t)1 : 0;
    int rc;
    LogpArgs B{};
    double* dz = nullptr;
    rc = carve(h->buf[BUF_LOGP], [&](Carve& c) {      // (every length even: pairs stay 16-byte aligned)
        c(dz, W * Dz);
        c(B.grad, W * Dz);
        c(B.logp, Wp);                                 // (behind the gradients: one copy brings both back)
        c(B.part, (W * (size_t)M.K * (size_t)h->nblk + 1) & ~(size_t)1);
        c(B.zg, W * 2 * (size_t)M.nt1);
        c(B.ds, W * nbs);
        c(B.gsum, W * Gs);
    });
    if (rc) return rc;
    B.z = dz;
    B.Dz = (long long)Dz; B.nbs = (long long)nbs; B.Gs = (long long)Gs;
    B.nt = h->nblk; B.W = n_points;
    B.c0 = logp_const(h);
    const bool direct = h->cidx.empty() && Dz == D;    // rows can be copied as they are
    if (!direct) {
        h->logp_host.resize(W * Dz + Wp);
        for (size_t w = 0; w < W; ++w) {
            double* row = h->logp_host.data() + w * Dz;
            if (h->cidx.empty()) memcpy(row, z + w * D, D * 8);
            else perm_gather(h, z + w * D, row);
            if (Dz > D) row[D] = 0.0;
        }
    }
    if ((rc = h2d(dz, direct ? z : h->logp_host.data(), W * Dz * 8, h->stream))) return rc;
    if ((rc = logp_launch(h, B))) return rc;
    if (!grad) return logp ? d2h(logp, B.logp, W * 8, h->stream) : dsync(h->stream);
    if (direct) {
        if ((rc = d2h(grad, B.grad, W * D * 8, h->stream))) return rc;
        return logp ? d2h(logp, B.logp, W * 8, h->stream) : BB_OK;
    }
    if ((rc = d2h(h->logp_host.data(), B.grad, (W * Dz + Wp) * 8, h->stream))) return rc;
    for (size_t w = 0; w < W; ++w) {
        const double* row = h->logp_host.data() + w * Dz;
        if (h->cidx.empty()) memcpy(grad + w * D, row, D * 8);
        else perm_scatter(h, row, grad + w * D);
    }
    if (logp) memcpy(logp, h->logp_host.data() + W * Dz, W * 8);
    return BB_OK;
}

// ---- posterior predictive bands (bb_ppc.h) ----------------------------------------------------------------------------------
static long long ppc_rows(const bb_handle* h) { return (long long)h->M.R * (1 + h->M.nb); }
// time points of the longest replicate: the columns of the frequency bands, one more than the steps of the ratio bands
static int freq_cols(const bb_handle* h) {
    int n = 0;
    for (int r = 0; r < h->M.R; ++r) n = std::max(n, h->M.T[r]);
    return n;
}
static int ppc_steps(const bb_handle* h) { return freq_cols(h) - 1; }
// caller offset of a block of the reference's layout (h->blocks lists the caller's order), -1 if the model has none
static long long ppc_block(const bb_handle* h, const char* name) {
    for (const bb_block_range& b : h->blocks) if (!strcmp(b.name, name)) return b.lo;
    return -1;
}

extern "C" int bb_ppc_shape(const bb_handle* h, int64_t* n_rows, int32_t* n_steps) {
    if (!h || !n_rows || !n_steps) return bb_fail(BB_ERR_INVALID, "null argument");
    *n_rows = ppc_rows(h);
    *n_steps = ppc_steps(h);
    return BB_OK;
}

// option checks shared by bb_ppc_bands and bb_freq_bands; *K = n_samples n_ppc
static int ppc_check(int32_t n_samples, int32_t n_ppc, int32_t n_q, const double* q, long long* K) {
    if (n_q < 1 || n_q > BB_PPC_MAX_Q) return bb_fail(BB_ERR_INVALID, "n_quantiles must be in 1..%d", BB_PPC_MAX_Q);
    for (int i = 0; i < n_q; ++i)
        if (!(q[i] >= 0.0 && q[i] <= 1.0)) return bb_fail(BB_ERR_INVALID, "All quantiles must be between zero and one");
    if (n_samples < 1 || n_ppc < 1) return bb_fail(BB_ERR_UNSUPPORTED, "n_samples and n_ppc must be >= 1");
    *K = (long long)n_samples * n_ppc;
    if (*K < 2 || *K > BB_PPC_MAX_K) return bb_fail(BB_ERR_UNSUPPORTED, "n_samples * n_ppc = %lld must be in 2..%d", *K, BB_PPC_MAX_K);
    return BB_OK;
}
// What bb_ppc_bands and bb_freq_bands share.  The sampling handle's device is current for as long as this lives.
struct BandsCall {
    bb_handle* dh;                 // the handle that samples
    DevGuard guard;
    std::vector<double> prm;       // mean | sigma = softplus(omega), the caller's layout
    std::vector<int> geno;         // genotype model: geno_idx in the caller's mutant order (caller_geno), once it has been fetched
    size_t nbands = 0;             // doubles of the result
    long long nblk = 0;            // grid of the row program (k_ppc / k_freq, 1024 threads)
    int npop = 0;                  // grid of k_ppc_pop
    explicit BandsCall(bb_handle* h) : dh(sampling_handle(h)), guard(dh->o.device) {}
};
// The front of a band call: the options checked, the posterior gathered, everything of P but the device pointers (the model's shape,
// the blocks' caller offsets, the targets of n_rows x n_steps bands), the grids.  quantiles == nullptr: the front of a call that takes
// the same draws but forms no bands (bb_fitness_rb): no band options to check, no targets, K = n_samples n_ppc >= 1 as its caller checked.
static int bands_prologue(bb_handle* h, int32_t n_samples, int32_t n_ppc, int32_t n_q, const double* quantiles, uint64_t seed,
                          long long n_rows, int n_steps, PpcArgs& P, BandsCall& B) {
    long long K = (long long)n_samples * n_ppc;
    int rc = quantiles ? ppc_check(n_samples, n_ppc, n_q, quantiles, &K) : BB_OK;
    if (rc) return rc;
    const DevModel& M = B.dh->M;
    const size_t D = (size_t)h->M.D;
    B.prm.resize(2 * D);           // (a multi-device handle gathers its parameters)
    if ((rc = bb_get_params(h, B.prm.data(), B.prm.data() + D))) return rc;
    for (size_t i = D; i < 2 * D; ++i) B.prm[i] = host_softplus(B.prm[i]);
    memset(&P, 0, sizeof P);
    P.kind = M.kind;
    P.R = M.R;
    P.E = (M.kind == BB_MODEL_MULTIENV || M.kind == BB_MODEL_MULTIENV_REPLICATE) ? M.E : 1;
    P.nt1 = M.nt1;
    P.nb = M.nb;
    P.n_samples = n_samples;
    P.n_ppc = n_ppc;
    P.K = (int)K;
    P.n_q = n_q;
    P.seed = seed;
    P.n_rows = n_rows;
    P.n_steps = n_steps;
    P.env_idx = M.env_idx;
    for (int r = 0; r < M.R; ++r) { P.T[r] = M.T[r]; P.off_t[r] = M.off_t[r]; P.tcum[r] = M.tcum[r]; }
    const bool hier = M.kind >= BB_MODEL_GENOTYPE;
    P.lo_spop = ppc_block(h, "s_pop");
    P.lo_lspop = ppc_block(h, "logsigma_pop");
    P.lo_s = ppc_block(h, hier ? "theta" : "s_bc");
    P.lo_ls = ppc_block(h, "logsigma_bc");
    P.lo_tt = hier ? ppc_block(h, "theta_tilde") : 0;
    P.lo_lt = hier ? ppc_block(h, "logtau") : 0;
    if (P.lo_spop < 0 || P.lo_lspop < 0 || P.lo_s < 0 || P.lo_ls < 0 || P.lo_tt < 0 || P.lo_lt < 0) return bb_fail(BB_ERR_INVALID, "unexpected block layout");
    // band end e = 2 qi + upper of the central mass q: the tail probabilities (1 - q) / 2 and 1 - (1 - q) / 2
    if (quantiles) {
        double probs[2 * BB_PPC_MAX_Q];
        for (int e = 0; e < 2 * n_q; ++e) {
            const double q = quantiles[e >> 1];
            probs[e] = (e & 1) ? 1.0 - (1.0 - q) / 2.0 : (1.0 - q) / 2.0;
        }
        quantile_plan(K, probs, 2 * n_q, P);
        B.nbands = (size_t)n_rows * n_steps * n_q * 2;
    }
    // row program: two workgroups per CU at most, the per-block scratch (P.par) bounded to 256 MiB
    B.nblk = std::min<long long>(n_rows, 2LL * B.dh->cus);
    while (B.nblk > 1 && (size_t)B.nblk * P.E * 2 * (size_t)n_samples * 8 > ((size_t)256 << 20)) B.nblk = (B.nblk + 1) / 2;
    B.npop = (int)std::max<long long>(1, std::min<long long>(((long long)P.nt1 * n_samples + 255) / 256, 1024));
    return BB_OK;
}
// B.geno: geno_idx in the caller's mutant order (the handle keeps its own, regrouped one), fetched once per call
static int caller_geno(const bb_handle* h, BandsCall& B) {
    const DevModel& M = B.dh->M;
    if (!B.geno.empty() || M.nb == 0) return BB_OK;
    std::vector<int> gi((size_t)M.nb);
    int rc = d2h(gi.data(), M.geno_idx, (size_t)M.nb * 4, B.dh->stream);
    if (rc) return rc;
    B.geno = gi;
    if (!h->perm_m.empty()) for (long long m = 0; m < M.nb; ++m) B.geno[(size_t)h->perm_m[(size_t)m]] = gi[(size_t)m];
    return BB_OK;
}
// The device buffer of a band call, `extra` naming what the call puts between the row scratch and the bands; then what needs the
// pointers: mean | sigma uploaded and, genotype model, geno_idx in the caller's mutant order (the handle keeps its own, regrouped one).
template <class X>
static int bands_buffers(const bb_handle* h, PpcArgs& P, BandsCall& B, X&& extra) {
    bb_handle* dh = B.dh;
    const DevModel& M = dh->M;
    const size_t D = (size_t)h->M.D, ns = (size_t)P.n_samples;
    double* post = nullptr;
    int* dg = nullptr;
    int rc = carve(dh->buf[BUF_BANDS], [&](Carve& c) {
        c(post, 2 * D);                                // mean | sigma
        c(P.pop, (size_t)P.nt1 * 2 * ns);              // [nt1][2][ns]
        c(P.par, (size_t)B.nblk * P.E * 2 * ns);       // [nblk][E][2][ns]
        extra(c);
        c(P.bands, B.nbands);
        c(dg, ((size_t)M.nb + 1) / 2 + 8);             // [nb] ints
    });
    if (rc) return rc;
    P.mean = post;
    P.sigma = post + D;
    if ((rc = h2d(post, B.prm.data(), 2 * D * 8, dh->stream)) || M.kind != BB_MODEL_GENOTYPE) return rc;
    if ((rc = caller_geno(h, B))) return rc;
    P.geno_idx = dg;
    return h2d(dg, B.geno.data(), (size_t)M.nb * 4, dh->stream);
}

// The walk over the observed counts that both n_outside computations make.  The handle's counts are in its own barcode order ([B][T_r]
// per replicate at M.cnt_off[r]), the bands' rows in the caller's: for every replicate r (T time points) and barcode,
// f(r, T, col, c, n, outside) gets the caller's data column col (neutrals first; a mutant through perm_m), the barcode's counts c[T],
// the replicate's totals n[T] and outside(row, t, x): does x lie outside the band of the largest q at (row, t)?
template <class F>
static int observed_walk(const bb_handle* h, const BandsCall& B, const PpcArgs& P, const double* quantiles, const double* bands, F&& f) {
    const DevModel& M = B.dh->M;
    long long cnt = 0;
    for (int r = 0; r < M.R; ++r) cnt += (long long)M.T[r] * M.B;
    std::vector<unsigned> c((size_t)cnt);
    int rc = d2h(c.data(), M.counts, (size_t)cnt * 4, B.dh->stream);
    if (rc) return rc;
    int qx = 0;
    for (int i = 1; i < P.n_q; ++i) if (quantiles[i] > quantiles[qx]) qx = i;
    auto outside = [&](long long row, int t, double x) {
        const double* bd = bands + (((size_t)row * P.n_steps + t) * P.n_q + qx) * 2;
        return x < bd[0] || x > bd[1];
    };
    for (int r = 0; r < M.R; ++r) {
        const int T = M.T[r];
        const unsigned* cr = c.data() + M.cnt_off[r];
        std::vector<double> n((size_t)T, 0.0);
        for (long long bc = 0; bc < M.B; ++bc)
            for (int t = 0; t < T; ++t) n[(size_t)t] += (double)cr[bc * T + t];
        for (long long bc = 0; bc < M.B; ++bc) {
            const long long col = bc < M.nn || h->perm_m.empty() ? bc : M.nn + (long long)h->perm_m[(size_t)(bc - M.nn)];
            f(r, T, col, cr + bc * T, n.data(), outside);
        }
    }
    return BB_OK;
}

extern "C" int bb_ppc_bands(bb_handle* h, const bb_ppc_opts* o, double* bands, int64_t* n_outside) {
    if (!h || !o || !bands || !o->quantiles) return bb_fail(BB_ERR_INVALID, "null argument");
    BandsCall B(h);
    bb_handle* dh = B.dh;
    const DevModel& M = dh->M;
    PpcArgs P;
    int rc = bands_prologue(h, o->n_samples, o->n_ppc, o->n_quantiles, o->quantiles, o->seed, ppc_rows(h), ppc_steps(h), P, B);
    if (rc || (rc = bands_buffers(h, P, B, [](Carve&) {}))) return rc;
    if ((rc = launch(dh->stream, k_ppc_pop, B.npop, 256, 0, P))) return rc;
    if ((rc = launch(dh->stream, k_ppc, (int)B.nblk, 1024, (size_t)bb_ppc_lds_doubles(P.K), P))) return rc;
    if ((rc = d2h(bands, P.bands, B.nbands * 8, dh->stream))) return rc;
    if (!n_outside) return BB_OK;
    // observed log-frequency ratios outside the band of the largest q (finite ratios only: both counts > 0); a replicate's neutrals
    // all count into its population-mean row
    for (long long row = 0; row < P.n_rows; ++row) n_outside[row] = 0;
    return observed_walk(h, B, P, o->quantiles, bands, [&](int r, int T, long long col, const unsigned* c, const double* n, auto& outside) {
        const long long row = col < M.nn ? r : P.R + (long long)r * M.nb + (col - M.nn);
        for (int t = 0; t + 1 < T; ++t) {
            if (!c[t] || !c[t + 1]) continue;
            if (outside(row, t, log((double)c[t + 1] / n[t + 1]) - log((double)c[t] / n[t]))) n_outside[row]++;
        }
    });
}

// ---- frequency-trajectory bands (bb_freq.h) -----------------------------------------------------------------------------------
static_assert(BB_FREQ_TRAJECTORY == BB_FREQ_MODE_TRAJECTORY && BB_FREQ_POSTERIOR == BB_FREQ_MODE_POSTERIOR, "mode numbering");
extern "C" int bb_freq_shape(const bb_handle* h, int64_t* n_rows, int32_t* n_cols) {
    if (!h || !n_rows || !n_cols) return bb_fail(BB_ERR_INVALID, "null argument");
    *n_rows = (long long)h->M.R * h->M.B;
    *n_cols = freq_cols(h);
    return BB_OK;
}

// The normalisers' side of F (F.P filled by bands_prologue): the shape, the loglambda offsets and *zb, the normaliser rows in flight
// (their chunk partials bounded to 256 MiB).  Shared by bb_freq_bands and bb_fitness_rb.
static int freq_plan(const bb_handle* h, const DevModel& M, int mode, FreqArgs& F, int* zb) {
    F.mode = mode;
    F.B = M.B;
    F.nn = M.nn;
    F.nchunks = (int)((M.B + BB_FREQ_CHUNK - 1) / BB_FREQ_CHUNK);
    F.nz = mode == BB_FREQ_TRAJECTORY ? M.R : M.Ttot;
    const long long lo_l = ppc_block(h, "loglambda");
    if (lo_l < 0) return bb_fail(BB_ERR_INVALID, "unexpected block layout");
    for (int r = 0; r < M.R; ++r) F.off_l[r] = lo_l + (long long)M.tcum[r] * M.B;
    *zb = F.nz;
    while (*zb > 1 && (size_t)F.nchunks * *zb * (size_t)F.P.n_samples * 8 > ((size_t)256 << 20)) *zb = (*zb + 1) / 2;
    return BB_OK;
}
// F.Z filled, zb normaliser rows at a time (F.Z and F.zpart placed by the caller's layout)
static int freq_normalisers(bb_handle* dh, FreqArgs& F, int zb) {
    const size_t ns = (size_t)F.P.n_samples, np2 = (ns + 1) / 2;
    int rc;
    for (F.z0 = 0; F.z0 < F.nz; F.z0 = F.z1) {
        F.z1 = std::min(F.nz, F.z0 + zb);
        const size_t nzb = (size_t)(F.z1 - F.z0);
        const int g1 = (int)std::max<size_t>(1, std::min<size_t>(((size_t)F.nchunks * nzb * np2 + 255) / 256, 65536));
        const int g2 = (int)std::max<size_t>(1, std::min<size_t>((nzb * ns + 255) / 256, 4096));
        if ((rc = launch(dh->stream, k_freq_zpart, g1, 256, 0, F))) return rc;
        if ((rc = launch(dh->stream, k_freq_zsum, g2, 256, 0, F))) return rc;
    }
    return BB_OK;
}

extern "C" int bb_freq_bands(bb_handle* h, const bb_freq_opts* o, double* bands, int64_t* n_outside) {
    if (!h || !o || !bands || !o->quantiles) return bb_fail(BB_ERR_INVALID, "null argument");
    if (o->mode != BB_FREQ_TRAJECTORY && o->mode != BB_FREQ_POSTERIOR) return bb_fail(BB_ERR_INVALID, "mode must be BB_FREQ_TRAJECTORY or BB_FREQ_POSTERIOR");
    BandsCall B(h);
    bb_handle* dh = B.dh;
    const DevModel& M = dh->M;
    FreqArgs F;
    memset(&F, 0, sizeof F);
    PpcArgs& P = F.P;
    int rc = bands_prologue(h, o->n_samples, o->n_ppc, o->n_quantiles, o->quantiles, o->seed, (long long)M.R * M.B, freq_cols(h), P, B);
    if (rc) return rc;
    if (o->mode == BB_FREQ_POSTERIOR && o->n_ppc != 1) return bb_fail(BB_ERR_INVALID, "BB_FREQ_POSTERIOR takes n_ppc = 1");      // (the shared checks report first)
    int zb;
    if ((rc = freq_plan(h, M, o->mode, F, &zb))) return rc;
    const size_t ns = (size_t)P.n_samples;
    rc = bands_buffers(h, P, B, [&](Carve& c) {
        c(F.Z, (size_t)M.Ttot * ns);                   // [Ttot][ns]
        c(F.zpart, (size_t)F.nchunks * zb * ns);       // [nchunks][zb][ns]
    });
    if (rc || (rc = freq_normalisers(dh, F, zb))) return rc;
    if (o->mode == BB_FREQ_TRAJECTORY && (rc = launch(dh->stream, k_ppc_pop, B.npop, 256, 0, P))) return rc;
    if ((rc = launch(dh->stream, k_freq, (int)B.nblk, 1024, (size_t)bb_ppc_lds_doubles(P.K), F))) return rc;
    if ((rc = d2h(bands, P.bands, B.nbands * 8, dh->stream))) return rc;
    if (!n_outside) return BB_OK;
    // observed frequencies R_{t,b} / n_t (zero counts included) outside the band of the largest q
    return observed_walk(h, B, P, o->quantiles, bands, [&](int r, int T, long long col, const unsigned* c, const double* n, auto& outside) {
        const long long row = (long long)r * M.B + col;
        int64_t cnt = 0;
        for (int t = 0; t < T; ++t) cnt += outside(row, t, (double)c[t] / n[t]);
        n_outside[row] = cnt;
    });
}

// Phase times of a call (diagnostics, tools/*_rate.py: -DBB_SCORE_TIMES, -DBB_LOO_TIMES, -DBB_RB_TIMES, -DBB_LLRB_TIMES, -DBB_CHAIN_TIMES, -DBB_TRACE_TIMES): lap(i, into) drains the
// stream, stamps ct[i] and adds the time since ct[i - 1] to ms[into] (into < 0: the stamp alone).  ON == false: nothing at all.
template <bool ON>
struct PhaseTimes {
    bbStream stream;
    timespec ct[8];
    double ms[7] = {0, 0, 0, 0, 0, 0, 0};
    void lap(int i, int into) {
        if (!ON) return;
        (void)dsync(stream);
        clock_gettime(CLOCK_MONOTONIC, &ct[i]);
        if (into >= 0) ms[into] += (ct[i].tv_sec - ct[i - 1].tv_sec) * 1e3 + (ct[i].tv_nsec - ct[i - 1].tv_nsec) * 1e-6;
    }
};
#ifdef BB_SCORE_TIMES
typedef PhaseTimes<true> ScoreTimes;
#else
typedef PhaseTimes<false> ScoreTimes;
#endif
#ifdef BB_RB_TIMES
typedef PhaseTimes<true> RbTimes;
#else
typedef PhaseTimes<false> RbTimes;
#endif
#ifdef BB_LLRB_TIMES
typedef PhaseTimes<true> LlrbTimes;
#else
typedef PhaseTimes<false> LlrbTimes;
#endif
#ifdef BB_CHAIN_TIMES
typedef PhaseTimes<true> ChainTimes;
#else
typedef PhaseTimes<false> ChainTimes;
#endif
#ifdef BB_TRACE_TIMES
typedef PhaseTimes<true> TraceTimes;
#else
typedef PhaseTimes<false> TraceTimes;
#endif

// ---- predictive log score and PIT of the observed ratios (bb_score.h) -----------------------------------------------------------
static_assert(BB_SCORE_MAX_SAMPLES == BB_PPC_MAX_K, "bb_ppc_score limits");
extern "C" int bb_score_shape(const bb_handle* h, int64_t* n_rows, int32_t* n_steps) {
    if (!h || !n_rows || !n_steps) return bb_fail(BB_ERR_INVALID, "null argument");
    *n_rows = (long long)h->M.R * h->M.B;
    *n_steps = ppc_steps(h);
    return BB_OK;
}

extern "C" int bb_ppc_score(bb_handle* h, const bb_score_opts* o, const bb_score_out* out) {
    if (!h || !o || !out) return bb_fail(BB_ERR_INVALID, "null argument");
    if (o->n_samples < 2 || o->n_samples > BB_SCORE_MAX_SAMPLES) return bb_fail(BB_ERR_UNSUPPORTED, "n_samples must be in 2..%d", BB_SCORE_MAX_SAMPLES);
    BandsCall B(h);
    bb_handle* dh = B.dh;
    const DevModel& M = dh->M;
    ScoreArgs A;
    memset(&A, 0, sizeof A);
    PpcArgs& P = A.P;
    const long long n_rows = (long long)M.R * M.B;
    const int n_steps = ppc_steps(h);
    const double no_band = 0.0;              // (the shared prologue plans one band; nothing selects here)
    int rc = bands_prologue(h, o->n_samples, 1, 1, &no_band, o->seed, n_rows, n_steps, P, B);
    if (rc) return rc;
    B.nbands = 0;
    A.B = M.B;
    A.nn = M.nn;
    ScoreTimes pt{dh->stream};   // tools/ppc_score_rate.py: the call's phases, each drained before the next starts
    pt.lap(0, -1);
    // the observed ratios, formed once here exactly as n_outside's walk forms them; NaN: a zero count, or no such step
    const size_t ncell = (size_t)n_rows * n_steps;
    std::vector<double> y(ncell, (double)NAN);
    rc = observed_walk(h, B, P, &no_band, nullptr, [&](int r, int T, long long col, const unsigned* c, const double* n, auto&) {
        double* yr = y.data() + ((size_t)r * M.B + col) * n_steps;
        for (int t = 0; t + 1 < T; ++t)
            if (c[t] && c[t + 1]) yr[t] = log((double)c[t + 1] / n[t + 1]) - log((double)c[t] / n[t]);
    });
    if (rc) return rc;
    pt.lap(1, 0);
    double* dy = nullptr;
    rc = bands_buffers(h, P, B, [&](Carve& c) {
        c(dy, ncell);                                  // [n_rows][n_steps]
        c(A.cell, BB_SCORE_CELLS * ncell);             // [6][n_rows][n_steps]
        c(A.rowsum, 2 * (size_t)n_rows);               // [2][n_rows]
        c(A.n_scored, ((size_t)n_rows + 1) / 2);       // [n_rows] ints
    });
    if (rc || (rc = h2d(dy, y.data(), ncell * 8, dh->stream))) return rc;
    A.y = dy;
    pt.lap(2, 1);
    if ((rc = launch(dh->stream, k_ppc_pop, B.npop, 256, 0, P))) return rc;
    pt.lap(3, 2);
    if ((rc = launch(dh->stream, k_score, (int)B.nblk, BB_SCORE_NT, (size_t)bb_score_lds_doubles(P.n_samples), A))) return rc;
    pt.lap(4, 3);
    if (out->observed) memcpy(out->observed, y.data(), ncell * 8);
    double* cells[BB_SCORE_CELLS] = {out->pred_mean, out->pred_sd, out->lpd, out->p_waic, out->pit, out->pit_upper};
    for (int k = 0; k < BB_SCORE_CELLS; ++k)
        if (cells[k] && (rc = d2h(cells[k], A.cell + (size_t)k * ncell, ncell * 8, dh->stream))) return rc;
    if (out->row_lpd && (rc = d2h(out->row_lpd, A.rowsum, (size_t)n_rows * 8, dh->stream))) return rc;
    if (out->row_p_waic && (rc = d2h(out->row_p_waic, A.rowsum + n_rows, (size_t)n_rows * 8, dh->stream))) return rc;
    if (out->n_scored && (rc = d2h(out->n_scored, A.n_scored, (size_t)n_rows * 4, dh->stream))) return rc;
    rc = dsync(dh->stream);
    pt.lap(5, 4);
#ifdef BB_SCORE_TIMES
    fprintf(stderr, "[bb_ppc_score %lld x %d, %d samples] observed %.3f ms, upload %.3f ms, pop %.3f ms, score %.3f ms, download %.3f ms\n", n_rows, n_steps, (int)o->n_samples, pt.ms[0], pt.ms[1], pt.ms[2], pt.ms[3], pt.ms[4]);
#endif
    return rc;
}

// ---- PSIS leave-one-out predictive scores of the observed ratios (bb_loo.h), in bb_ppc_score's frame ---------------------------------
static_assert(BB_LOO_MAX_SAMPLES == BB_LOO_NSAMP_CAP && 2 * BB_LOO_MAX_SAMPLES == BB_SCORE_MAX_SAMPLES, "bb_ppc_loo limits");
#ifdef BB_LOO_TIMES
typedef PhaseTimes<true> LooTimes;
#else
typedef PhaseTimes<false> LooTimes;
#endif
extern "C" int bb_loo_shape(const bb_handle* h, int64_t* n_rows, int32_t* n_steps) { return bb_score_shape(h, n_rows, n_steps); }

extern "C" int bb_ppc_loo(bb_handle* h, const bb_loo_opts* o, const bb_loo_out* out) {
    if (!h || !o || !out) return bb_fail(BB_ERR_INVALID, "null argument");
    if (o->n_samples < 2 || o->n_samples > BB_LOO_MAX_SAMPLES) return bb_fail(BB_ERR_UNSUPPORTED, "n_samples must be in 2..%d", BB_LOO_MAX_SAMPLES);
    BandsCall B(h);
    bb_handle* dh = B.dh;
    const DevModel& M = dh->M;
    LooArgs A;
    memset(&A, 0, sizeof A);
    PpcArgs& P = A.P;
    const long long n_rows = (long long)M.R * M.B;
    const int n_steps = ppc_steps(h);
    const double no_band = 0.0;              // (the shared prologue plans one band; nothing selects here)
    int rc = bands_prologue(h, o->n_samples, 1, 1, &no_band, o->seed, n_rows, n_steps, P, B);
    if (rc) return rc;
    B.nbands = 0;
    A.B = M.B;
    A.nn = M.nn;
    LooTimes pt{dh->stream};     // tools/ppc_loo_rate.py: the call's phases, each drained before the next starts
    pt.lap(0, -1);
    // the observed ratios, formed exactly as bb_ppc_score forms them; NaN: a zero count, or no such step
    const size_t ncell = (size_t)n_rows * n_steps;
    std::vector<double> y(ncell, (double)NAN);
    rc = observed_walk(h, B, P, &no_band, nullptr, [&](int r, int T, long long col, const unsigned* c, const double* n, auto&) {
        double* yr = y.data() + ((size_t)r * M.B + col) * n_steps;
        for (int t = 0; t + 1 < T; ++t)
            if (c[t] && c[t + 1]) yr[t] = log((double)c[t + 1] / n[t + 1]) - log((double)c[t] / n[t]);
    });
    if (rc) return rc;
    pt.lap(1, 0);
    double* dy = nullptr;
    rc = bands_buffers(h, P, B, [&](Carve& c) {
        c(dy, ncell);                                  // [n_rows][n_steps]
        c(A.cell, BB_LOO_CELLS * ncell);               // [5][n_rows][n_steps]
        c(A.rowv, BB_LOO_ROWS * (size_t)n_rows);       // [6][n_rows]
        c(A.n_scored, ((size_t)n_rows + 1) / 2);       // [n_rows] ints
    });
    if (rc || (rc = h2d(dy, y.data(), ncell * 8, dh->stream))) return rc;
    A.y = dy;
    pt.lap(2, 1);
    if ((rc = launch(dh->stream, k_ppc_pop, B.npop, 256, 0, P))) return rc;
    pt.lap(3, 2);
    if ((rc = launch(dh->stream, k_loo, (int)B.nblk, BB_SCORE_NT, (size_t)BB_LOO_LDS_DOUBLES(P.n_samples), A))) return rc;
    pt.lap(4, 3);
    double* cells[BB_LOO_CELLS] = {out->elpd_loo, out->p_loo, out->khat, out->n_eff, out->lpd};
    for (int k = 0; k < BB_LOO_CELLS; ++k)
        if (cells[k] && (rc = d2h(cells[k], A.cell + (size_t)k * ncell, ncell * 8, dh->stream))) return rc;
    double* rows[BB_LOO_ROWS] = {out->row_elpd_loo, out->row_p_loo, out->row_khat, out->row_n_eff, out->row_elpd_cells, out->row_khat_max};
    for (int k = 0; k < BB_LOO_ROWS; ++k)
        if (rows[k] && (rc = d2h(rows[k], A.rowv + (size_t)k * n_rows, (size_t)n_rows * 8, dh->stream))) return rc;
    if (out->n_scored && (rc = d2h(out->n_scored, A.n_scored, (size_t)n_rows * 4, dh->stream))) return rc;
    rc = dsync(dh->stream);
    pt.lap(5, 4);
#ifdef BB_LOO_TIMES
    fprintf(stderr, "[bb_ppc_loo %lld x %d, %d samples] observed %.3f ms, upload %.3f ms, pop %.3f ms, loo %.3f ms, download %.3f ms\n", n_rows, n_steps, (int)o->n_samples, pt.ms[0], pt.ms[1], pt.ms[2], pt.ms[3], pt.ms[4]);
#endif
    return rc;
}

// ---- Rao-Blackwellised fitness marginals (bb_rb.h) ----------------------------------------------------------------------------------
static_assert(BB_RB_MAX_SAMPLES == BB_RB_SAMPLES_CAP && BB_RB_MAX_SAMPLES <= BB_PPC_MAX_K, "bb_fitness_rb limits");
static long long rb_units(const bb_handle* h) {
    const DevModel& M = h->M;
    const int E = (M.kind == BB_MODEL_MULTIENV || M.kind == BB_MODEL_MULTIENV_REPLICATE) ? M.E : 1;
    return (long long)M.R * M.nb * E;
}
extern "C" int bb_fitness_rb_shape(const bb_handle* h, int64_t* n_units) {
    if (!h || !n_units) return bb_fail(BB_ERR_INVALID, "null argument");
    *n_units = rb_units(h);
    return BB_OK;
}

// ---- what the six Rao-Blackwellised calls share ----------------------------------------------------------------------------------------
// the option checks: `cap` the call's largest n_samples, `threshold` nullptr for the calls that take none
static int rb_check(int nq, const double* probs, const double* draws, int ns, int cap, const double* threshold) {
    if (nq < 0 || nq > BB_RB_MAX_Q || (nq > 0 && !probs)) return bb_fail(BB_ERR_INVALID, "n_quantiles must be in 0..%d (with probs)", BB_RB_MAX_Q);
    for (int i = 0; i < nq; ++i)
        if (!(probs[i] > 0.0 && probs[i] < 1.0)) return bb_fail(BB_ERR_INVALID, "every prob must lie strictly between zero and one");
    if (threshold && !std::isfinite(*threshold)) return bb_fail(BB_ERR_INVALID, "threshold must be finite");
    const int ns_lo = draws ? 1 : 2;
    if (ns < ns_lo || ns > cap) return bb_fail(BB_ERR_UNSUPPORTED, "n_samples must be in %d..%d", ns_lo, cap);
    return BB_OK;
}

// The start of a call: the draws' plan (bands_prologue without bands: nothing selects here), every normaliser row of the posterior
// mode's plan, and of A what every call sets the same way.
static int rb_open(bb_handle* h, BandsCall& B, RbArgs& A, int ns, uint64_t seed, int nq, const double* probs, long long n_units, int* zb) {
    const DevModel& M = B.dh->M;
    int rc = bands_prologue(h, ns, 1, 0, nullptr, seed, (long long)M.R * M.nb, ppc_steps(h), A.F.P, B);
    if (rc || (rc = freq_plan(h, M, BB_FREQ_POSTERIOR, A.F, zb))) return rc;
    A.nq = nq;
    A.n_units = n_units;
    A.n_z = M.Ttot;
    for (int i = 0; i < nq; ++i) A.probs[i] = probs[i];
    return BB_OK;
}
// the caller's draws, if any, onto the device
static int rb_draws(bb_handle* dh, PpcArgs& P, double* ddraws, const double* draws, size_t ns, size_t D) {
    if (!draws) return BB_OK;
    if (int rc = h2d(ddraws, draws, ns * D * 8, dh->stream)) return rc;
    P.draws = ddraws;
    P.D = (long long)D;
    return BB_OK;
}
// the front on the device: sbar_{t,j} for the calls that read it (pop), the normalisers, their logarithms in place
static int rb_front(bb_handle* dh, const BandsCall& B, RbArgs& A, int zb, bool pop) {
    int rc;
    if (pop && (rc = launch(dh->stream, k_ppc_pop, B.npop, 256, 0, A.F.P))) return rc;
    if ((rc = freq_normalisers(dh, A.F, zb))) return rc;
    const int glz = (int)std::max<size_t>(1, std::min<size_t>(((size_t)dh->M.Ttot * (size_t)A.F.P.n_samples + 255) / 256, 4096));
    return launch(dh->stream, k_rb_logz, glz, 256, 0, A);      // (F.Z now holds ln Z: every row of a replicate reads the same ones)
}
// the grid of a mixture program of bb_gridmix.h: a block per row, two per CU at most, their [tab][ns] tables bounded to 256 MiB
static long long rb_mix_blocks(const bb_handle* dh, long long rows, int tab, size_t ns) {
    long long nblk = std::max<long long>(1, std::min<long long>(rows, 2LL * dh->cus));
    while (nblk > 1 && (size_t)nblk * tab * ns * 8 > ((size_t)256 << 20)) nblk = (nblk + 1) / 2;
    return nblk;
}
// The results back: row k of A.unit [n_rows][n] into units[k] where the caller gave one, A.quant [n][8] as [n][nq], A.n_steps where
// n_steps is asked for.  live: entries that are no cell of the model are NaN (bb_loglambda_rb: the program leaves them alone).
// Ends drained, whatever was asked for.
static int rb_download(bb_handle* dh, const RbArgs& A, size_t n, double* const* units, int n_rows, double* quantiles, int32_t* n_steps,
                       const char* live = nullptr) {
    int rc;
    for (int k = 0; k < n_rows; ++k) {
        if (!units[k] || !n) continue;
        if ((rc = d2h(units[k], A.unit + (size_t)k * n, n * 8, dh->stream))) return rc;
        for (size_t e = 0; live && e < n; ++e) if (!live[e]) units[k][e] = NAN;
    }
    if (quantiles && A.nq && n) {
        std::vector<double> q(BB_RB_MAX_Q * n);
        if ((rc = d2h(q.data(), A.quant, q.size() * 8, dh->stream))) return rc;
        for (size_t e = 0; e < n; ++e)
            for (int i = 0; i < A.nq; ++i) quantiles[e * A.nq + i] = !live || live[e] ? q[e * BB_RB_MAX_Q + i] : NAN;
    }
    if (n_steps && n && (rc = d2h(n_steps, A.n_steps, n * 4, dh->stream))) return rc;
    return dsync(dh->stream);
}
// The ragged method's pairing of the neutral terms, [2][nt1][nn] (t | b), empty where the model has none: neutral member i of group
// (r, k) is element x = k nn + i of the replicate's time-fastest vector.  ragged_upload: onto the device, the two halves named.
static std::vector<int> ragged_pairing(const DevModel& M) {
    std::vector<int> neu;
    if (!M.quirk) return neu;
    neu.resize(2 * (size_t)M.nt1 * (size_t)M.nn);
    int* nt = neu.data();
    int* nbv = nt + (size_t)M.nt1 * (size_t)M.nn;
    for (int r = 0; r < M.R; ++r)
        for (int k = 0; k + 1 < M.T[r]; ++k)
            for (long long i = 0; i < M.nn; ++i) {
                const long long x = (long long)k * M.nn + i, at = (long long)(M.off_t[r] + k) * M.nn + i;
                nt[at] = (int)(x % (M.T[r] - 1));
                nbv[at] = (int)(x / (M.T[r] - 1));
            }
    return neu;
}
static int ragged_upload(bb_handle* dh, const std::vector<int>& neu, int* dneu, const int*& neu_t, const int*& neu_b) {
    if (neu.empty()) return BB_OK;
    neu_t = dneu;
    neu_b = dneu + neu.size() / 2;
    return h2d(dneu, neu.data(), neu.size() * 4, dh->stream);
}

extern "C" int bb_fitness_rb(bb_handle* h, const bb_rb_opts* o, const bb_rb_out* out) {
    if (!h || !o || !out) return bb_fail(BB_ERR_INVALID, "null argument");
    const int nq = o->n_quantiles, ns = o->n_samples;
    if (int rc = rb_check(nq, o->probs, o->draws, ns, BB_RB_MAX_SAMPLES, &o->threshold)) return rc;
    BandsCall B(h);
    bb_handle* dh = B.dh;
    const DevModel& M = dh->M;
    RbArgs A;
    memset(&A, 0, sizeof A);
    FreqArgs& F = A.F;
    PpcArgs& P = F.P;
    const long long n_units = rb_units(h);
    int zb;
    int rc = rb_open(h, B, A, ns, o->seed, nq, o->probs, n_units, &zb);
    if (rc) return rc;
    if (M.kind == BB_MODEL_FITNESS || M.kind == BB_MODEL_MULTIENV) {         // (no regrouping for these kinds: the handle's order is the caller's)
        const DevPrior& dp = M.pri[BK_S];
        P.pri_mean = dp.mean; P.pri_ivar = dp.inv_var; P.pri_mean_e = dp.mean_e; P.pri_ivar_e = dp.inv_var_e;
    }
    A.threshold = o->threshold;
    RbTimes pt{dh->stream};      // tools/fitness_rb_rate.py: the call's phases, each drained before the next starts
    pt.lap(0, -1);
    const size_t nsz = (size_t)ns, D = (size_t)h->M.D, nu = (size_t)n_units;
    double* ddraws = nullptr;
    rc = bands_buffers(h, P, B, [&](Carve& c) {        // (P.par, [nblk][E][2][ns], holds the [nblk][E + 1][ns] table of bb_block_rb)
        c(F.Z, (size_t)M.Ttot * nsz);                  // [Ttot][ns]
        c(F.zpart, (size_t)F.nchunks * zb * nsz);      // [nchunks][zb][ns]
        c(A.unit, BB_RB_OUT * nu);                     // [6][n_units]
        c(A.quant, BB_RB_MAX_Q * nu);                  // [n_units][8]
        c(A.n_steps, (nu + 1) / 2);                    // [n_units] ints
        c(ddraws, o->draws ? nsz * D : 0);             // [ns][D]
    });
    if (rc) return rc;
    A.ytab = P.par;
    if ((rc = rb_draws(dh, P, ddraws, o->draws, nsz, D))) return rc;
    pt.lap(1, 0);
    if ((rc = launch(dh->stream, k_ppc_pop, B.npop, 256, 0, P))) return rc;
    pt.lap(2, 1);
    if ((rc = rb_front(dh, B, A, zb, false))) return rc;
    pt.lap(3, 2);
    if ((rc = launch(dh->stream, k_rb, (int)B.nblk, BB_SCORE_NT, (size_t)BB_RB_LDS_DOUBLES(ns), A))) return rc;
    pt.lap(4, 3);
    double* units[BB_RB_OUT] = {out->q_mean, out->q_sd, out->rb_mean, out->rb_sd, out->p_pos, out->p_neg};
    rc = rb_download(dh, A, nu, units, BB_RB_OUT, out->quantiles, out->n_steps);
    pt.lap(5, 4);
#ifdef BB_RB_TIMES
    fprintf(stderr, "[bb_fitness_rb %lld units, %d samples, %d quantiles] upload %.3f ms, pop %.3f ms, normalisers %.3f ms, rb %.3f ms, download %.3f ms\n", n_units, ns, nq, pt.ms[0], pt.ms[1], pt.ms[2], pt.ms[3], pt.ms[4]);
#endif
    return rc;
}

// ---- Rao-Blackwellised hyper-fitness marginals (bb_rb.h) -------------------------------------------------------------------------
static_assert(BB_THETA_RB_CHUNK == BB_THETA_CHUNK, "bb_theta_rb chunk");
static long long theta_groups(const bb_handle* h) {
    return h->M.kind < BB_MODEL_GENOTYPE ? 0 : h->M.blk_hi[BK_S] - h->M.blk_lo[BK_S];
}
extern "C" int bb_theta_rb_shape(const bb_handle* h, int64_t* n_groups) {
    if (!h || !n_groups) return bb_fail(BB_ERR_INVALID, "null argument");
    *n_groups = theta_groups(h);
    return BB_OK;
}

// The chunk map of bb_block_theta_part / bb_block_theta, in the caller's order: a group's members ascending (genotype: the caller's
// mutants m with geno_idx[m] == g; replicate kinds: r = 0 .. R - 1), cut into chunks of BB_THETA_CHUNK consecutive members.
struct ThetaMap {
    std::vector<int> grp_c0, grp_nst, grp_nmem, chk_grp, chk_m0, mem_row, mem_nu;
};
// nu[r E + e] = n_u of (replicate, environment): the replicate's steps whose later time point lies in e
static int env_steps(bb_handle* dh, int E, std::vector<int>& nu) {
    const DevModel& M = dh->M;
    std::vector<int> env;
    if (E > 1) {
        env.resize((size_t)M.Ttot);
        if (int rc = d2h(env.data(), M.env_idx, (size_t)M.Ttot * 4, dh->stream)) return rc;
    }
    nu.assign((size_t)M.R * E, 0);
    for (int r = 0; r < M.R; ++r)
        for (int t = 0; t + 1 < M.T[r]; ++t) nu[(size_t)r * E + (E > 1 ? env[(size_t)(M.tcum[r] + t + 1)] : 0)]++;
    return BB_OK;
}
static int theta_map(const bb_handle* h, BandsCall& B, int E, ThetaMap& tm) {
    bb_handle* dh = B.dh;
    const DevModel& M = dh->M;
    const long long G = theta_groups(h), nb = M.nb;
    const bool geno = M.kind == BB_MODEL_GENOTYPE;
    int rc;
    std::vector<int> nu;
    if ((rc = env_steps(dh, E, nu))) return rc;
    // members: first member of every group, then the rows
    std::vector<long long> m0((size_t)G + 1, 0);
    if (geno) {
        if ((rc = caller_geno(h, B))) return rc;
        const std::vector<int>& gi = B.geno;
        for (long long m = 0; m < nb; ++m) m0[(size_t)gi[(size_t)m] + 1]++;
        for (long long g = 0; g < G; ++g) m0[(size_t)g + 1] += m0[(size_t)g];
        tm.mem_row.resize((size_t)nb);
        std::vector<long long> at(m0.begin(), m0.end() - 1);
        for (long long m = 0; m < nb; ++m) tm.mem_row[(size_t)at[(size_t)gi[(size_t)m]]++] = (int)m;
    } else {
        if ((long long)M.R * nb * E > 2147483647LL) return bb_fail(BB_ERR_UNSUPPORTED, "bb_theta_rb: more than 2^31 members");
        tm.mem_row.resize((size_t)(G * M.R));
        for (long long g = 0; g < G; ++g) {
            m0[(size_t)g + 1] = (g + 1) * M.R;
            for (int r = 0; r < M.R; ++r) tm.mem_row[(size_t)(g * M.R + r)] = (int)(r * nb + g / E);
        }
    }
    tm.mem_nu.assign(tm.mem_row.size(), 0);
    tm.grp_c0.assign((size_t)G + 1, 0);
    tm.grp_nst.assign((size_t)G, 0);
    tm.grp_nmem.assign((size_t)G, 0);
    tm.chk_grp.clear();
    tm.chk_m0.clear();
    for (long long g = 0; g < G; ++g) {
        const long long a = m0[(size_t)g], b = m0[(size_t)g + 1];
        tm.grp_c0[(size_t)g] = (int)tm.chk_grp.size();
        tm.grp_nmem[(size_t)g] = (int)(b - a);
        for (long long x = a; x < b; x += BB_THETA_CHUNK) { tm.chk_grp.push_back((int)g); tm.chk_m0.push_back((int)x); }
        long long nst = 0;
        for (long long x = a; x < b; ++x) {
            tm.mem_nu[(size_t)x] = nu[(size_t)(tm.mem_row[(size_t)x] / nb) * E + (geno ? 0 : g % E)];
            nst += tm.mem_nu[(size_t)x];
        }
        tm.grp_nst[(size_t)g] = (int)nst;
    }
    tm.grp_c0[(size_t)G] = (int)tm.chk_grp.size();
    tm.chk_m0.push_back((int)m0[(size_t)G]);
    return BB_OK;
}

extern "C" int bb_theta_rb(bb_handle* h, const bb_rb_opts* o, const bb_theta_rb_out* out) {
    if (!h || !o || !out) return bb_fail(BB_ERR_INVALID, "null argument");
    const int nq = o->n_quantiles, ns = o->n_samples;
    if (int rc = rb_check(nq, o->probs, o->draws, ns, BB_RB_MAX_SAMPLES, &o->threshold)) return rc;
    if (h->M.kind < BB_MODEL_GENOTYPE)
        return bb_fail(BB_ERR_UNSUPPORTED, "bb_theta_rb applies to the hierarchical models only: model kind %d (%s) has no theta", (int)h->M.kind,
                       h->M.kind == BB_MODEL_FITNESS ? "BB_MODEL_FITNESS" : "BB_MODEL_MULTIENV");
    BandsCall B(h);
    bb_handle* dh = B.dh;
    const DevModel& M = dh->M;
    ThetaArgs H;
    memset(&H, 0, sizeof H);
    RbArgs& A = H.A;
    FreqArgs& F = A.F;
    PpcArgs& P = F.P;
    const long long n_groups = theta_groups(h);
    int zb;
    int rc = rb_open(h, B, A, ns, o->seed, nq, o->probs, n_groups, &zb);
    if (rc) return rc;
    {   // the prior of theta: the block is never regrouped (a genotype keeps its number, the replicate kinds keep the caller's order),
        // so a Matrix form lies in the handle as the caller gave it, indexed by g
        const DevPrior& dp = M.pri[BK_S];
        P.pri_mean = dp.mean; P.pri_ivar = dp.inv_var; P.pri_mean_e = dp.mean_e; P.pri_ivar_e = dp.inv_var_e;
    }
    A.threshold = o->threshold;
    RbTimes pt{dh->stream};      // tools/theta_rb_rate.py: the call's phases, each drained before the next starts
    pt.lap(0, -1);
    ThetaMap tm;
    if ((rc = theta_map(h, B, P.E, tm))) return rc;
    const size_t nsz = (size_t)ns, D = (size_t)h->M.D, ng = (size_t)n_groups, nchk = tm.chk_grp.size(), nmem = tm.mem_row.size();
    // the groups in flight: their chunk partials bounded to 256 MiB (a single group is worked whole whatever it takes)
    const size_t cap = std::max<size_t>(1, ((size_t)256 << 20) / (2 * nsz * 8));
    size_t slab_chunks = 1;
    std::vector<size_t> cut{0};                       // slab s: the groups [cut[s], cut[s + 1])
    while (cut.back() < ng) {
        const size_t g0 = cut.back();
        size_t g1 = g0 + 1;
        while (g1 < ng && (size_t)(tm.grp_c0[g1 + 1] - tm.grp_c0[g0]) <= cap) ++g1;
        slab_chunks = std::max(slab_chunks, (size_t)(tm.grp_c0[g1] - tm.grp_c0[g0]));
        cut.push_back(g1);
    }
    const int nblk = (int)std::max<long long>(1, std::min<long long>(n_groups, B.nblk));      // (P.par holds a [nblk][ns] table of theta_j)
    double* ddraws = nullptr;
    int* dmap = nullptr;
    const size_t nmap = (ng + 1) + ng + nchk + (nchk + 1) + 2 * nmem;
    rc = bands_buffers(h, P, B, [&](Carve& c) {
        c(F.Z, (size_t)M.Ttot * nsz);                  // [Ttot][ns]
        c(F.zpart, (size_t)F.nchunks * zb * nsz);      // [nchunks][zb][ns]
        c(H.part, slab_chunks * 2 * nsz);              // [chunks in flight][2][ns]
        c(A.unit, BB_RB_OUT * ng);                     // [6][n_groups]
        c(A.quant, BB_RB_MAX_Q * ng);                  // [n_groups][8]
        c(dmap, (nmap + 1) / 2);                       // the chunk map: ints
        c(ddraws, o->draws ? nsz * D : 0);             // [ns][D]
    });
    if (rc) return rc;
    A.ytab = P.par;
    {
        std::vector<int> hm;
        hm.reserve(nmap);
        int* p = dmap;
        auto put = [&](const int*& dst, const std::vector<int>& v) { dst = p; p += v.size(); hm.insert(hm.end(), v.begin(), v.end()); };
        put(H.grp_c0, tm.grp_c0); put(H.grp_nst, tm.grp_nst); put(H.chk_grp, tm.chk_grp); put(H.chk_m0, tm.chk_m0); put(H.mem_row, tm.mem_row); put(H.mem_nu, tm.mem_nu);
        if ((rc = h2d(dmap, hm.data(), nmap * 4, dh->stream))) return rc;
    }
    if ((rc = rb_draws(dh, P, ddraws, o->draws, nsz, D))) return rc;
    pt.lap(1, 0);
    if ((rc = launch(dh->stream, k_ppc_pop, B.npop, 256, 0, P))) return rc;
    pt.lap(2, 1);
    if ((rc = rb_front(dh, B, A, zb, false))) return rc;
    pt.lap(3, 2);
    for (size_t sl = 0; sl + 1 < cut.size(); ++sl) {
        const size_t g0 = cut[sl], g1 = cut[sl + 1];
        H.g0 = (long long)g0; H.g1 = (long long)g1;
        H.c0 = tm.grp_c0[g0]; H.c1 = tm.grp_c0[g1];
        pt.lap(4, -1);
        if (H.c1 > H.c0 && (rc = launch(dh->stream, k_rb_theta_part, std::min(H.c1 - H.c0, 1 << 20), BB_SCORE_NT, 0, H))) return rc;
        pt.lap(5, 3);
        if ((rc = launch(dh->stream, k_rb_theta, (int)std::min<long long>((long long)(g1 - g0), nblk), BB_SCORE_NT, (size_t)BB_RB_LDS_DOUBLES(ns), H))) return rc;
        pt.lap(6, 4);
    }
    double* units[BB_RB_OUT] = {out->q_mean, out->q_sd, out->rb_mean, out->rb_sd, out->p_pos, out->p_neg};
    rc = rb_download(dh, A, ng, units, BB_RB_OUT, out->quantiles, nullptr);
    if (rc) return rc;
    if (out->n_members) memcpy(out->n_members, tm.grp_nmem.data(), ng * 4);
    if (out->n_steps) memcpy(out->n_steps, tm.grp_nst.data(), ng * 4);
    pt.lap(7, 5);
#ifdef BB_RB_TIMES
    fprintf(stderr, "[bb_theta_rb %lld groups, %zu members, %zu chunks, %d samples, %d quantiles] map+upload %.3f ms, pop %.3f ms, normalisers %.3f ms, part %.3f ms, theta %.3f ms, download %.3f ms\n", n_groups, nmem, nchk, ns, nq, pt.ms[0], pt.ms[1], pt.ms[2], pt.ms[3], pt.ms[4], pt.ms[5]);
#endif
    return BB_OK;
}

// ---- Rao-Blackwellised fitness contrasts (bb_contrast.h) ------------------------------------------------------------------------------
// The terms checked: a well-formed CSR, every contrast with terms, every index inside the space and named once per contrast, every
// weight finite.  *n_terms = term_ptr[n_contrasts].
static int contrast_check(const bb_contrast_opts* o, long long n_space, const char* what, long long* n_terms) {
    const long long nc = o->n_contrasts;
    if (!o->term_ptr || !o->term_idx || !o->term_w) return bb_fail(BB_ERR_INVALID, "bb_contrast_rb: term_ptr, term_idx and term_w must not be null");
    if (o->term_ptr[0] != 0) return bb_fail(BB_ERR_INVALID, "bb_contrast_rb: term_ptr[0] = %lld, must be 0", (long long)o->term_ptr[0]);
    if (nc > 2147483647LL) return bb_fail(BB_ERR_UNSUPPORTED, "bb_contrast_rb: more than 2^31 - 1 terms");
    for (long long c = 0; c < nc; ++c) {
        if (o->term_ptr[c + 1] < o->term_ptr[c])
            return bb_fail(BB_ERR_INVALID, "bb_contrast_rb: contrast %lld: term_ptr decreases (%lld after %lld)", c, (long long)o->term_ptr[c + 1], (long long)o->term_ptr[c]);
        if (o->term_ptr[c + 1] == o->term_ptr[c]) return bb_fail(BB_ERR_INVALID, "bb_contrast_rb: contrast %lld has no terms", c);
    }
    if (o->term_ptr[nc] > 2147483647LL) return bb_fail(BB_ERR_UNSUPPORTED, "bb_contrast_rb: %lld terms, more than 2^31 - 1", (long long)o->term_ptr[nc]);
    std::vector<long long> seen;
    for (long long c = 0; c < nc; ++c) {
        const long long k0 = o->term_ptr[c], k1 = o->term_ptr[c + 1];
        for (long long k = k0; k < k1; ++k) {
            if (o->term_idx[k] < 0 || o->term_idx[k] >= n_space)
                return bb_fail(BB_ERR_INVALID, "bb_contrast_rb: contrast %lld, term %lld: %s %lld outside 0..%lld", c, k - k0, what, (long long)o->term_idx[k], n_space - 1);
            if (!std::isfinite(o->term_w[k])) return bb_fail(BB_ERR_INVALID, "bb_contrast_rb: contrast %lld, term %lld: the weight is not finite", c, k - k0);
        }
        seen.assign(o->term_idx + k0, o->term_idx + k1);
        std::sort(seen.begin(), seen.end());
        const auto dup = std::adjacent_find(seen.begin(), seen.end());
        if (dup != seen.end()) {
            long long k = k1 - 1;                      // the later of the two terms that name it
            while (o->term_idx[k] != *dup) --k;
            return bb_fail(BB_ERR_INVALID, "bb_contrast_rb: contrast %lld, term %lld: %s %lld is named twice", c, k - k0, what, *dup);
        }
    }
    *n_terms = o->term_ptr[nc];
    return BB_OK;
}

extern "C" int bb_contrast_rb(bb_handle* h, const bb_contrast_opts* o, const bb_contrast_out* out) {
    if (!h || !o || !out) return bb_fail(BB_ERR_INVALID, "null argument");
    const int nq = o->n_quantiles, ns = o->n_samples;
    if (int rc = rb_check(nq, o->probs, o->draws, ns, BB_RB_MAX_SAMPLES, &o->threshold)) return rc;
    if (o->space != BB_CONTRAST_FITNESS && o->space != BB_CONTRAST_THETA)
        return bb_fail(BB_ERR_INVALID, "bb_contrast_rb: unknown space %d", (int)o->space);
    const bool theta = o->space == BB_CONTRAST_THETA;
    if (theta && h->M.kind < BB_MODEL_GENOTYPE)
        return bb_fail(BB_ERR_UNSUPPORTED, "bb_contrast_rb: BB_CONTRAST_THETA applies to the hierarchical models only: model kind %d (%s) has no theta",
                       (int)h->M.kind, h->M.kind == BB_MODEL_FITNESS ? "BB_MODEL_FITNESS" : "BB_MODEL_MULTIENV");
    if (o->n_contrasts < 0) return bb_fail(BB_ERR_INVALID, "bb_contrast_rb: n_contrasts = %lld", (long long)o->n_contrasts);
    if (o->n_contrasts == 0) return BB_OK;
    long long n_terms = 0;
    if (int rc = contrast_check(o, theta ? theta_groups(h) : rb_units(h), theta ? "group" : "unit", &n_terms)) return rc;
    BandsCall B(h);
    bb_handle* dh = B.dh;
    const DevModel& M = dh->M;
    ContrastArgs C;
    memset(&C, 0, sizeof C);
    RbArgs& A = C.H.A;
    FreqArgs& F = A.F;
    PpcArgs& P = F.P;
    int zb;
    int rc = rb_open(h, B, A, ns, o->seed, nq, o->probs, o->n_contrasts, &zb);
    if (rc) return rc;
    if (theta || M.kind == BB_MODEL_FITNESS || M.kind == BB_MODEL_MULTIENV) {      // the s_bc prior, as bb_theta_rb / bb_fitness_rb set it
        const DevPrior& dp = M.pri[BK_S];
        P.pri_mean = dp.mean; P.pri_ivar = dp.inv_var; P.pri_mean_e = dp.mean_e; P.pri_ivar_e = dp.inv_var_e;
    }
    A.threshold = o->threshold;
    C.space = o->space;
    // min_steps, and for THETA the chunk map
    const size_t ncz = (size_t)o->n_contrasts, ntz = (size_t)n_terms;
    std::vector<int> elem_steps;                       // n_u of every unit, or the groups' n_steps
    ThetaMap tm;
    if (theta) {
        if ((rc = theta_map(h, B, P.E, tm))) return rc;
        elem_steps = tm.grp_nst;
    } else {
        std::vector<int> nu;
        if ((rc = env_steps(dh, P.E, nu))) return rc;
        const long long n_units = rb_units(h), per = (long long)P.E * M.nb;
        elem_steps.resize((size_t)n_units);
        for (long long u = 0; u < n_units; ++u) elem_steps[(size_t)u] = nu[(size_t)(u / per) * P.E + (size_t)(u % P.E)];
    }
    std::vector<int> hm;                               // term_ptr | term_idx | the chunk map
    hm.reserve(ncz + 1 + ntz);
    for (size_t c = 0; c <= ncz; ++c) hm.push_back((int)o->term_ptr[c]);
    for (size_t k = 0; k < ntz; ++k) hm.push_back((int)o->term_idx[k]);
    const std::vector<int>* maps[5] = {&tm.grp_c0, &tm.grp_nst, &tm.chk_m0, &tm.mem_row, &tm.mem_nu};
    size_t at[5];
    for (int i = 0; i < 5; ++i) { at[i] = hm.size(); hm.insert(hm.end(), maps[i]->begin(), maps[i]->end()); }
    const size_t nsz = (size_t)ns, D = (size_t)h->M.D, nmap = hm.size();
    const int nblk = (int)std::max<long long>(1, std::min<long long>(o->n_contrasts, B.nblk));      // (P.par holds a [nblk][ns] table of d_j)
    double* ddraws = nullptr;
    double* dw = nullptr;
    int* dmap = nullptr;
    rc = bands_buffers(h, P, B, [&](Carve& c) {
        c(F.Z, (size_t)M.Ttot * nsz);                  // [Ttot][ns]
        c(F.zpart, (size_t)F.nchunks * zb * nsz);      // [nchunks][zb][ns]
        c(A.unit, BB_RB_OUT * ncz);                    // [6][n_contrasts]
        c(A.quant, BB_RB_MAX_Q * ncz);                 // [n_contrasts][8]
        c(dw, ntz);                                    // [n_terms] weights
        c(dmap, (nmap + 1) / 2);                       // the CSR arrays and the chunk map: ints
        c(ddraws, o->draws ? nsz * D : 0);             // [ns][D]
    });
    if (rc) return rc;
    A.ytab = P.par;
    C.term_ptr = dmap;
    C.term_idx = dmap + ncz + 1;
    C.term_w = dw;
    if (theta) { C.H.grp_c0 = dmap + at[0]; C.H.grp_nst = dmap + at[1]; C.H.chk_m0 = dmap + at[2]; C.H.mem_row = dmap + at[3]; C.H.mem_nu = dmap + at[4]; }
    if ((rc = h2d(dmap, hm.data(), nmap * 4, dh->stream)) || (rc = h2d(dw, o->term_w, ntz * 8, dh->stream))) return rc;
    if ((rc = rb_draws(dh, P, ddraws, o->draws, nsz, D))) return rc;
    if ((rc = launch(dh->stream, k_ppc_pop, B.npop, 256, 0, P))) return rc;
    if ((rc = rb_front(dh, B, A, zb, false))) return rc;
    if ((rc = launch(dh->stream, k_rb_contrast, nblk, BB_SCORE_NT, (size_t)BB_RB_LDS_DOUBLES(ns), C))) return rc;
    double* units[BB_RB_OUT] = {out->q_mean, out->q_sd, out->rb_mean, out->rb_sd, out->p_pos, out->p_neg};
    if ((rc = rb_download(dh, A, ncz, units, BB_RB_OUT, out->quantiles, nullptr))) return rc;
    for (size_t c = 0; out->min_steps && c < ncz; ++c) {
        int lo = elem_steps[(size_t)o->term_idx[o->term_ptr[c]]];
        for (long long k = o->term_ptr[c] + 1; k < o->term_ptr[c + 1]; ++k) lo = std::min(lo, elem_steps[(size_t)o->term_idx[k]]);
        out->min_steps[c] = lo;
    }
    return BB_OK;
}

// ---- posterior of the fitness distribution of sets of units (bb_dfe.h) ---------------------------------------------------------------
static_assert(BB_DFE_CHUNK == BB_DFE_CHUNK_UNITS && BB_DFE_MAX_SAMPLES == BB_DFE_SAMPLES_CAP && BB_DFE_MAX_SAMPLES <= BB_RB_MAX_SAMPLES, "bb_dfe_rb limits");
// The sets of bb_dfe_rb and bb_fitness_rank (`who`) checked: a well-formed CSR, every set with units, every index inside the units
// and named once per set.  *n_idx = set_ptr[n_sets].
static int sets_check(const char* who, long long n_sets, const int64_t* set_ptr, const int64_t* set_idx, long long n_units, long long* n_idx) {
    const long long nc = n_sets;
    if (nc < 0) return bb_fail(BB_ERR_INVALID, "%s: n_sets = %lld", who, nc);
    *n_idx = 0;
    if (nc == 0) return BB_OK;
    if (!set_ptr || !set_idx) return bb_fail(BB_ERR_INVALID, "%s: set_ptr and set_idx must not be null", who);
    if (set_ptr[0] != 0) return bb_fail(BB_ERR_INVALID, "%s: set_ptr[0] = %lld, must be 0", who, (long long)set_ptr[0]);
    if (nc > 2147483647LL) return bb_fail(BB_ERR_UNSUPPORTED, "%s: more than 2^31 - 1 indices", who);
    for (long long c = 0; c < nc; ++c) {
        if (set_ptr[c + 1] < set_ptr[c])
            return bb_fail(BB_ERR_INVALID, "%s: set %lld: set_ptr decreases (%lld after %lld)", who, c, (long long)set_ptr[c + 1], (long long)set_ptr[c]);
        if (set_ptr[c + 1] == set_ptr[c]) return bb_fail(BB_ERR_INVALID, "%s: set %lld has no units", who, c);
    }
    if (set_ptr[nc] > 2147483647LL) return bb_fail(BB_ERR_UNSUPPORTED, "%s: %lld indices, more than 2^31 - 1", who, (long long)set_ptr[nc]);
    std::vector<long long> seen;
    for (long long c = 0; c < nc; ++c) {
        const long long k0 = set_ptr[c], k1 = set_ptr[c + 1];
        for (long long k = k0; k < k1; ++k)
            if (set_idx[k] < 0 || set_idx[k] >= n_units)
                return bb_fail(BB_ERR_INVALID, "%s: set %lld, position %lld: unit %lld outside 0..%lld", who, c, k - k0, (long long)set_idx[k], n_units - 1);
        seen.assign(set_idx + k0, set_idx + k1);
        std::sort(seen.begin(), seen.end());
        const auto dup = std::adjacent_find(seen.begin(), seen.end());
        if (dup != seen.end()) {
            long long k = k1 - 1;                      // the later of the two positions that name it
            while (set_idx[k] != *dup) --k;
            return bb_fail(BB_ERR_INVALID, "%s: set %lld, position %lld: unit %lld is named twice", who, c, k - k0, *dup);
        }
    }
    *n_idx = set_ptr[nc];
    return BB_OK;
}

// The grid and the sets checked: thresholds finite and strictly ascending; the sets by sets_check.
static int dfe_check(const bb_dfe_opts* o, long long n_units, long long* n_idx) {
    if (o->n_grid < 1 || o->n_grid > BB_DFE_MAX_GRID) return bb_fail(BB_ERR_INVALID, "bb_dfe_rb: n_grid = %d, must be in 1..%d", (int)o->n_grid, BB_DFE_MAX_GRID);
    if (!o->grid) return bb_fail(BB_ERR_INVALID, "bb_dfe_rb: grid must not be null");
    for (int g = 0; g < o->n_grid; ++g) {
        if (!std::isfinite(o->grid[g])) return bb_fail(BB_ERR_INVALID, "bb_dfe_rb: grid point %d is not finite", g);
        if (g > 0 && !(o->grid[g] > o->grid[g - 1])) return bb_fail(BB_ERR_INVALID, "bb_dfe_rb: grid point %d does not lie above grid point %d: the grid must be strictly ascending", g, g - 1);
    }
    if (o->reserved0 < 0) return bb_fail(BB_ERR_INVALID, "bb_dfe_rb: reserved0 = %d, must be 0", (int)o->reserved0);
    return sets_check("bb_dfe_rb", o->n_sets, o->set_ptr, o->set_idx, n_units, n_idx);
}

extern "C" int bb_dfe_rb(bb_handle* h, const bb_dfe_opts* o, const bb_dfe_out* out) {
    if (!h || !o || !out) return bb_fail(BB_ERR_INVALID, "null argument");
    const int nq = o->n_quantiles, ns = o->n_samples, ngr = o->n_grid;
    if (int rc = rb_check(nq, o->probs, o->draws, ns, BB_DFE_MAX_SAMPLES, nullptr)) return rc;
    if (nq > 0 && ns < 2) return bb_fail(BB_ERR_UNSUPPORTED, "bb_dfe_rb: n_quantiles > 0 needs n_samples >= 2: one draw has no quantiles over the draws");
    long long n_idx = 0;
    if (int rc = dfe_check(o, rb_units(h), &n_idx)) return rc;
    if (o->n_sets == 0) return BB_OK;
    BandsCall B(h);
    bb_handle* dh = B.dh;
    const DevModel& M = dh->M;
    DfeArgs D;
    memset(&D, 0, sizeof D);
    RbArgs& A = D.A;
    FreqArgs& F = A.F;
    PpcArgs& P = F.P;
    const size_t nset = (size_t)o->n_sets, nix = (size_t)n_idx, ncell = nset * (size_t)ngr;
    int zb;
    int rc = rb_open(h, B, A, ns, o->seed, nq, o->probs, (long long)ncell, &zb);
    if (rc) return rc;
    if (M.kind == BB_MODEL_FITNESS || M.kind == BB_MODEL_MULTIENV) {      // the s_bc prior, as bb_fitness_rb sets it
        const DevPrior& dp = M.pri[BK_S];
        P.pri_mean = dp.mean; P.pri_ivar = dp.inv_var; P.pri_mean_e = dp.mean_e; P.pri_ivar_e = dp.inv_var_e;
    }
    if (nq > 0) quantile_plan(ns, o->probs, nq, P);    // (P.n_q stays 0: the program interpolates per probability, as bb_chain_summary's)
    D.n_grid = ngr;
    D.n_cells = (long long)ncell;
    RbTimes pt{dh->stream};      // tools/dfe_rate.py: the call's phases, each drained before the next starts
    pt.lap(0, -1);
    // the chunk map: set -> first chunk, chunk -> set
    std::vector<int> hm;                               // set_ptr | set_idx | set_c0 | chk_set
    hm.reserve(2 * (nset + 1) + nix + nix / BB_DFE_CHUNK + nset);
    for (size_t c = 0; c <= nset; ++c) hm.push_back((int)o->set_ptr[c]);
    for (size_t k = 0; k < nix; ++k) hm.push_back((int)o->set_idx[k]);
    std::vector<int> set_c0(nset + 1, 0), chk_set;
    for (size_t c = 0; c < nset; ++c) {
        const long long n = o->set_ptr[c + 1] - o->set_ptr[c], nc = (n + BB_DFE_CHUNK - 1) / BB_DFE_CHUNK;
        set_c0[c + 1] = set_c0[c] + (int)nc;
        chk_set.insert(chk_set.end(), (size_t)nc, (int)c);
    }
    const size_t at_c0 = hm.size();
    hm.insert(hm.end(), set_c0.begin(), set_c0.end());
    const size_t at_cs = hm.size();
    hm.insert(hm.end(), chk_set.begin(), chk_set.end());
    // The slabs: sets [cut[s], cut[s + 1]) with all their grid points while their chunk partials, one [4][ns] table per (chunk,
    // grid point), stay within 256 MiB; a set too large for that takes its grid points grid_width at a time (a single (set, grid
    // point) is worked whole whatever it takes).
    const size_t nsz = (size_t)ns, D_ = (size_t)h->M.D, nmap = hm.size();
    const size_t cap = o->reserved0 > 0 ? (size_t)o->reserved0 : std::max<size_t>(1, ((size_t)256 << 20) / (4 * nsz * 8));
    auto grid_width = [&](size_t nchk) {               // grid points in flight of a slab of nchk chunks: all, or whole groups of the part program
        if (nchk * (size_t)ngr <= cap) return (size_t)ngr;
        const size_t gw = std::max<size_t>(1, cap / nchk);
        return gw > BB_DFE_GROUP ? gw - gw % BB_DFE_GROUP : gw;
    };
    std::vector<size_t> cut{0};
    size_t slab_tabs = 1, slab_cells = 1, n_slabs = 0;
    while (cut.back() < nset) {
        const size_t s0 = cut.back();
        size_t s1 = s0 + 1;
        while (s1 < nset && (size_t)(set_c0[s1 + 1] - set_c0[s0]) * (size_t)ngr <= cap) ++s1;
        const size_t nchk = (size_t)(set_c0[s1] - set_c0[s0]);
        const size_t gw = grid_width(nchk);
        n_slabs += ((size_t)ngr + gw - 1) / gw;
        slab_tabs = std::max(slab_tabs, nchk * gw);
        slab_cells = std::max(slab_cells, (s1 - s0) * gw);
        cut.push_back(s1);
    }
    const int nblk = (int)std::max<long long>(1, std::min<long long>((long long)slab_cells, 2LL * dh->cus));
    B.nblk = (3LL * nblk + 2 * P.E - 1) / (2 * P.E);   // (P.par, [B.nblk][E][2][ns], holds the [nblk][3][ns] table of bb_block_dfe and nothing else)
    double* ddraws = nullptr;
    double* dgrid = nullptr;
    int* dmap = nullptr;
    rc = bands_buffers(h, P, B, [&](Carve& c) {
        c(F.Z, (size_t)M.Ttot * nsz);                  // [Ttot][ns]
        c(F.zpart, (size_t)F.nchunks * zb * nsz);      // [nchunks][zb][ns]
        c(D.part, slab_tabs * 4 * nsz);                // [chunks in flight][grid points in flight][4][ns]
        c(D.cell, BB_DFE_OUT * ncell);                 // [6][n_sets n_grid]
        c(D.bands, nq ? 2 * ncell * BB_RB_MAX_Q : 0);  // [2][n_sets n_grid][8]
        c(dgrid, (size_t)ngr);                         // [n_grid]
        c(dmap, (nmap + 1) / 2);                       // the CSR arrays and the chunk map: ints
        c(ddraws, o->draws ? nsz * D_ : 0);            // [ns][D]
    });
    if (rc) return rc;
    A.ytab = P.par;
    D.set_ptr = dmap;
    D.set_idx = dmap + nset + 1;
    D.set_c0 = dmap + at_c0;
    D.chk_set = dmap + at_cs;
    D.grid = dgrid;
    if ((rc = h2d(dmap, hm.data(), nmap * 4, dh->stream)) || (rc = h2d(dgrid, o->grid, (size_t)ngr * 8, dh->stream))) return rc;
    if ((rc = rb_draws(dh, P, ddraws, o->draws, nsz, D_))) return rc;
    pt.lap(1, 0);
    if ((rc = launch(dh->stream, k_ppc_pop, B.npop, 256, 0, P))) return rc;
    pt.lap(2, 1);
    if ((rc = rb_front(dh, B, A, zb, false))) return rc;
    pt.lap(3, 2);
    const long long ntile = ((long long)ns + BB_DFE_PART_NT - 1) / BB_DFE_PART_NT;
    for (size_t sl = 0; sl + 1 < cut.size(); ++sl) {
        const size_t s0 = cut[sl], s1 = cut[sl + 1], nchk = (size_t)(set_c0[s1] - set_c0[s0]);
        const int gw = (int)grid_width(nchk);
        D.s0 = (long long)s0; D.s1 = (long long)s1;
        D.c0 = set_c0[s0]; D.c1 = set_c0[s1];
        for (int g0 = 0; g0 < ngr; g0 += gw) {
            D.g0 = g0; D.g1 = std::min(g0 + gw, ngr);
            const long long ngrp = (D.g1 - D.g0 + BB_DFE_GROUP - 1) / BB_DFE_GROUP, ncl = (long long)(s1 - s0) * (D.g1 - D.g0);
            pt.lap(4, -1);
            if ((rc = launch(dh->stream, k_dfe_part, (int)std::min<long long>((long long)nchk * ngrp * ntile, 1 << 20), BB_DFE_PART_NT, 0, D))) return rc;
            pt.lap(5, 3);
            if ((rc = launch(dh->stream, k_dfe, (int)std::min<long long>(ncl, nblk), BB_SCORE_NT, (size_t)BB_DFE_LDS_DOUBLES(ns, 1), D))) return rc;
            pt.lap(6, 4);
        }
    }
    double* cells[BB_DFE_OUT] = {out->below_mean, out->above_mean, out->between_sd, out->within_sd, out->q_below_mean, out->q_below_sd};
    for (int k = 0; k < BB_DFE_OUT; ++k)
        if (cells[k] && (rc = d2h(cells[k], D.cell + (size_t)k * ncell, ncell * 8, dh->stream))) return rc;
    double* bands[2] = {out->below_bands, out->above_bands};
    std::vector<double> q;
    for (int side = 0; side < 2 && nq; ++side) {
        if (!bands[side]) continue;
        q.resize(BB_RB_MAX_Q * ncell);
        if ((rc = d2h(q.data(), D.bands + (size_t)side * ncell * BB_RB_MAX_Q, q.size() * 8, dh->stream))) return rc;
        for (size_t e = 0; e < ncell; ++e)
            for (int i = 0; i < nq; ++i) bands[side][e * nq + i] = q[e * BB_RB_MAX_Q + i];
    }
    if ((rc = dsync(dh->stream))) return rc;
    for (size_t c = 0; out->n_units && c < nset; ++c) out->n_units[c] = o->set_ptr[c + 1] - o->set_ptr[c];
    pt.lap(7, 5);
#ifdef BB_RB_TIMES
    fprintf(stderr, "[bb_dfe_rb %zu sets, %zu indices, %zu chunks, %d grid points, %d samples, %d quantiles, %zu slabs] map+upload %.3f ms, pop %.3f ms, normalisers %.3f ms, part %.3f ms, dfe %.3f ms, download %.3f ms\n", nset, nix, chk_set.size(), ngr, ns, nq, n_slabs, pt.ms[0], pt.ms[1], pt.ms[2], pt.ms[3], pt.ms[4], pt.ms[5]);
#endif
    return BB_OK;
}

// ---- posterior ranks and top-k membership of the units of sets (bb_rank.h) -------------------------------------------------------------
static_assert(BB_RANK_RUN == BB_RANK_RUN_KEYS && BB_RANK_MAX_TOP == BB_RANK_TOPS && BB_RANK_MAX_SAMPLES == BB_RANK_SAMPLES_CAP && BB_RANK_MAX_SAMPLES <= BB_RB_MAX_SAMPLES,
              "bb_fitness_rank limits");
static_assert(BB_RANK_CONDITIONAL == 0 && BB_RANK_DRAWS == 1, "RankArgs.source");
#define BB_RANK_BYTES 16                 // per position and draw in flight: a key, a sorted position, a rank
extern "C" int bb_fitness_rank(bb_handle* h, const bb_rank_opts* o, const bb_rank_out* out) {
    if (!h || !o || !out) return bb_fail(BB_ERR_INVALID, "null argument");
    const int nq = o->n_quantiles, ns = o->n_samples, ntop = o->n_top;
    if (int rc = rb_check(nq, o->probs, o->draws, ns, BB_RANK_MAX_SAMPLES, nullptr)) return rc;
    if (nq > 0 && ns < 2) return bb_fail(BB_ERR_UNSUPPORTED, "bb_fitness_rank: n_quantiles > 0 needs n_samples >= 2: one draw has no quantiles over the draws");
    if (o->source != BB_RANK_CONDITIONAL && o->source != BB_RANK_DRAWS) return bb_fail(BB_ERR_INVALID, "bb_fitness_rank: source = %d, must be BB_RANK_CONDITIONAL or BB_RANK_DRAWS", (int)o->source);
    if (ntop < 0 || ntop > BB_RANK_MAX_TOP) return bb_fail(BB_ERR_INVALID, "bb_fitness_rank: n_top = %d, must be in 0..%d", ntop, BB_RANK_MAX_TOP);
    if (ntop > 0 && !o->top) return bb_fail(BB_ERR_INVALID, "bb_fitness_rank: top must not be null with n_top > 0");
    for (int i = 0; i < ntop; ++i)
        if (o->top[i] < 1 || o->top[i] > 2147483647LL) return bb_fail(BB_ERR_INVALID, "bb_fitness_rank: top[%d] = %lld, must be in 1..2^31 - 1", i, (long long)o->top[i]);
    if (o->reserved0 < 0 || (o->reserved0 > 0 && (o->reserved0 < 64 || o->reserved0 > BB_RANK_RUN || (o->reserved0 & (o->reserved0 - 1)))))
        return bb_fail(BB_ERR_INVALID, "bb_fitness_rank: reserved0 = %d, must be 0", (int)o->reserved0);
    if (o->reserved1 < 0) return bb_fail(BB_ERR_INVALID, "bb_fitness_rank: reserved1 = %d, must be 0", (int)o->reserved1);
    long long n_idx = 0;
    if (int rc = sets_check("bb_fitness_rank", o->n_sets, o->set_ptr, o->set_idx, rb_units(h), &n_idx)) return rc;
    if (o->n_sets == 0) return BB_OK;
    BandsCall B(h);
    bb_handle* dh = B.dh;
    const DevModel& M = dh->M;
    RankArgs R;
    memset(&R, 0, sizeof R);
    RbArgs& A = R.A;
    FreqArgs& F = A.F;
    PpcArgs& P = F.P;
    const size_t nset = (size_t)o->n_sets, nix = (size_t)n_idx;
    const bool cond = o->source == BB_RANK_CONDITIONAL;
    int zb;
    int rc = rb_open(h, B, A, ns, o->seed, nq, o->probs, n_idx, &zb);
    if (rc) return rc;
    if (M.kind == BB_MODEL_FITNESS || M.kind == BB_MODEL_MULTIENV) {      // the s_bc prior, as bb_fitness_rb sets it
        const DevPrior& dp = M.pri[BK_S];
        P.pri_mean = dp.mean; P.pri_ivar = dp.inv_var; P.pri_mean_e = dp.mean_e; P.pri_ivar_e = dp.inv_var_e;
    }
    if (nq > 0) quantile_plan(ns, o->probs, nq, P);    // (P.n_q stays 0: the program interpolates per probability, as bb_dfe_rb's)
    R.n_idx = n_idx;
    R.run = o->reserved0 > 0 ? o->reserved0 : BB_RANK_RUN;
    R.source = o->source;
    R.n_top = ntop;
    for (int i = 0; i < ntop; ++i) R.top[i] = (int)o->top[i];
    RbTimes pt{dh->stream};      // tools/rank_rate.py: the call's phases, each drained before the next starts
    pt.lap(0, -1);
    // the run map: set -> first run, run -> set
    std::vector<int> hm;                               // set_ptr | set_idx | set_r0 | run_set
    hm.reserve(2 * (nset + 1) + nix + nix / (size_t)R.run + nset);
    for (size_t c = 0; c <= nset; ++c) hm.push_back((int)o->set_ptr[c]);
    for (size_t k = 0; k < nix; ++k) hm.push_back((int)o->set_idx[k]);
    std::vector<int> set_r0(nset + 1, 0), run_set;
    for (size_t c = 0; c < nset; ++c) {
        const long long n = o->set_ptr[c + 1] - o->set_ptr[c], nr = (n + R.run - 1) / R.run;
        set_r0[c + 1] = set_r0[c] + (int)nr;
        run_set.insert(run_set.end(), (size_t)nr, (int)c);
    }
    const size_t at_r0 = hm.size();
    hm.insert(hm.end(), set_r0.begin(), set_r0.end());
    const size_t at_rs = hm.size();
    hm.insert(hm.end(), run_set.begin(), run_set.end());
    // The slabs: sets [cut[s], cut[s + 1]) with all their draws while their tables, BB_RANK_BYTES per position and draw, stay within
    // 256 MiB; a set too large for that is worked alone, its keys and sorted positions `width` draws at a time, its ranks whole.
    const size_t nsz = (size_t)ns, D_ = (size_t)h->M.D, nmap = hm.size();
    const size_t bound = o->reserved1 > 0 ? (size_t)o->reserved1 << 10 : (size_t)256 << 20;
    auto width = [&](size_t npos) {                    // draws in flight of a slab of npos positions
        if (npos * nsz * BB_RANK_BYTES <= bound) return nsz;
        return std::min(nsz, std::max<size_t>(1, bound / ((BB_RANK_BYTES - 4) * npos)));
    };
    std::vector<size_t> cut{0};
    size_t key_elems = 1, rank_elems = 1, n_slabs = 0;
    while (cut.back() < nset) {
        const size_t s0 = cut.back();
        size_t s1 = s0 + 1;
        while (s1 < nset && (size_t)(o->set_ptr[s1 + 1] - o->set_ptr[s0]) * nsz * BB_RANK_BYTES <= bound) ++s1;
        const size_t npos = (size_t)(o->set_ptr[s1] - o->set_ptr[s0]), jw = width(npos);
        n_slabs += (nsz + jw - 1) / jw;
        key_elems = std::max(key_elems, npos * jw);
        rank_elems = std::max(rank_elems, npos * nsz);
        cut.push_back(s1);
    }
    B.nblk = 0;                                        // (no row program: P.par is not used)
    double* ddraws = nullptr;
    int* dmap = nullptr;
    rc = bands_buffers(h, P, B, [&](Carve& c) {
        c(F.Z, cond ? (size_t)M.Ttot * nsz : 0);       // [Ttot][ns]
        c(F.zpart, cond ? (size_t)F.nchunks * zb * nsz : 0);      // [nchunks][zb][ns]
        c(R.key, key_elems);                           // the keys of the positions and draws in flight
        c(R.spos, (key_elems + 1) / 2);                // ... their sorted positions: ints
        c(R.rank, (rank_elems + 1) / 2);               // [positions in flight][ns] ints
        c(R.unit, 2 * nix);                            // [2][n_idx]
        c(R.ptop, ntop ? BB_RANK_TOPS * nix : 0);      // [n_idx][8]
        c(R.quant, nq ? BB_RB_MAX_Q * nix : 0);        // [n_idx][8]
        c(dmap, (nmap + 1) / 2);                       // the CSR arrays and the run map: ints
        c(ddraws, o->draws ? nsz * D_ : 0);            // [ns][D]
    });
    if (rc) return rc;
    R.set_ptr = dmap;
    R.set_idx = dmap + nset + 1;
    R.set_r0 = dmap + at_r0;
    R.run_set = dmap + at_rs;
    if ((rc = h2d(dmap, hm.data(), nmap * 4, dh->stream))) return rc;
    if ((rc = rb_draws(dh, P, ddraws, o->draws, nsz, D_))) return rc;
    pt.lap(1, 0);
    if (cond && (rc = rb_front(dh, B, A, zb, true))) return rc;
    pt.lap(2, 1);
    for (size_t sl = 0; sl + 1 < cut.size(); ++sl) {
        const size_t s0 = cut[sl], s1 = cut[sl + 1];
        R.s0 = (long long)s0; R.s1 = (long long)s1;
        R.k0 = (int)o->set_ptr[s0]; R.k1 = (int)o->set_ptr[s1];
        R.r0 = set_r0[s0]; R.r1 = set_r0[s1];
        const size_t npos = (size_t)(R.k1 - R.k0), jw = width(npos);
        long long longest = 1;
        bool several = false;
        for (size_t c = s0; c < s1; ++c) {
            longest = std::max<long long>(longest, o->set_ptr[c + 1] - o->set_ptr[c]);
            several |= set_r0[c + 1] - set_r0[c] > 1;
        }
        int p2 = 2;
        while (p2 < std::min<long long>(longest, R.run)) p2 <<= 1;
        R.lds_run = p2;
        const int snt = std::min(BB_RANK_SORT_NT, std::max(64, p2 / 2));
        for (size_t j0 = 0; j0 < nsz; j0 += jw) {
            R.j0 = (int)j0; R.j1 = (int)std::min(j0 + jw, nsz);
            const long long jn = R.j1 - R.j0, nval = (long long)((npos + BB_RANK_VAL_UNITS - 1) / BB_RANK_VAL_UNITS) * ((jn + BB_RANK_VAL_NT - 1) / BB_RANK_VAL_NT);
            const long long nsort = (long long)(R.r1 - R.r0) * jn;
            pt.lap(3, -1);
            if ((rc = launch(dh->stream, k_rank_val, (int)std::min<long long>(nval, 1 << 20), BB_RANK_VAL_NT, 0, R))) return rc;
            pt.lap(4, 2);
            if ((rc = launch(dh->stream, k_rank_sort, (int)std::min<long long>(nsort, 1 << 20), snt, (size_t)BB_RANK_SORT_LDS_DOUBLES(p2), R))) return rc;
            pt.lap(5, 3);
            if (several && (rc = launch(dh->stream, k_rank_merge, (int)std::min<long long>(nsort, 1 << 20), snt, 0, R))) return rc;
            pt.lap(6, 4);
        }
        pt.lap(3, -1);
        if ((rc = launch(dh->stream, k_rank_stats, (int)std::min<long long>((long long)npos, 8LL * dh->cus), BB_SCORE_NT, (size_t)BB_RANK_STATS_LDS_DOUBLES(ns), R))) return rc;
        pt.lap(4, 5);
        pt.lap(6, -1);
        if (out->ranks && (rc = d2h(out->ranks + (size_t)R.k0 * nsz, R.rank, npos * nsz * 4, dh->stream))) return rc;
        pt.lap(7, 6);
    }
    pt.lap(6, -1);
    if (out->rank_mean && (rc = d2h(out->rank_mean, R.unit, nix * 8, dh->stream))) return rc;
    if (out->rank_sd && (rc = d2h(out->rank_sd, R.unit + nix, nix * 8, dh->stream))) return rc;
    std::vector<double> q;
    if (out->p_top && ntop) {
        q.resize(BB_RANK_TOPS * nix);
        if ((rc = d2h(q.data(), R.ptop, q.size() * 8, dh->stream))) return rc;
        for (size_t e = 0; e < nix; ++e)
            for (int i = 0; i < ntop; ++i) out->p_top[e * ntop + i] = q[e * BB_RANK_TOPS + i];
    }
    if (out->quantiles && nq) {
        q.resize(BB_RB_MAX_Q * nix);
        if ((rc = d2h(q.data(), R.quant, q.size() * 8, dh->stream))) return rc;
        for (size_t e = 0; e < nix; ++e)
            for (int i = 0; i < nq; ++i) out->quantiles[e * nq + i] = q[e * BB_RB_MAX_Q + i];
    }
    if ((rc = dsync(dh->stream))) return rc;
    for (size_t c = 0; out->n_units && c < nset; ++c) out->n_units[c] = o->set_ptr[c + 1] - o->set_ptr[c];
    pt.lap(7, 6);
#ifdef BB_RB_TIMES
    fprintf(stderr, "[bb_fitness_rank source %d, %zu sets, %zu indices, %zu runs of %d, %d samples, %d quantiles, %d tops, %zu slabs] map+upload %.3f ms, front %.3f ms, values %.3f ms, sort %.3f ms, merge %.3f ms, summaries %.3f ms, download %.3f ms\n", (int)o->source, nset, nix, run_set.size(), R.run, ns, nq, ntop, n_slabs, pt.ms[0], pt.ms[1], pt.ms[2], pt.ms[3], pt.ms[4], pt.ms[5], pt.ms[6]);
#endif
    return BB_OK;
}

// ---- Rao-Blackwellised population-mean fitness marginals (bb_rb.h) ------------------------------------------------------------------
static_assert(BB_POPMEAN_RB_CHUNK == BB_POP_CHUNK, "bb_popmean_rb chunk");
extern "C" int bb_popmean_rb_shape(const bb_handle* h, int64_t* n_groups) {
    if (!h || !n_groups) return bb_fail(BB_ERR_INVALID, "null argument");
    *n_groups = h->M.blk_hi[BK_SPOP] - h->M.blk_lo[BK_SPOP];
    return BB_OK;
}

extern "C" int bb_popmean_rb(bb_handle* h, const bb_rb_opts* o, const bb_popmean_rb_out* out) {
    if (!h || !o || !out) return bb_fail(BB_ERR_INVALID, "null argument");
    const int nq = o->n_quantiles, ns = o->n_samples;
    if (int rc = rb_check(nq, o->probs, o->draws, ns, BB_RB_MAX_SAMPLES, &o->threshold)) return rc;
    BandsCall B(h);
    bb_handle* dh = B.dh;
    const DevModel& M = dh->M;
    PopArgs H;
    memset(&H, 0, sizeof H);
    RbArgs& A = H.A;
    FreqArgs& F = A.F;
    PpcArgs& P = F.P;
    const long long n_groups = M.nt1, nmem = M.nn + M.nb;
    if (nmem > 2147483647LL) return bb_fail(BB_ERR_UNSUPPORTED, "bb_popmean_rb: more than 2^31 members");
    int zb;
    int rc = rb_open(h, B, A, ns, o->seed, nq, o->probs, n_groups, &zb);
    if (rc) return rc;
    {   // the prior of sbar: the s_pop block is never regrouped, so a Matrix form lies in the handle as the caller gave it, indexed by g
        const DevPrior& dp = M.pri[BK_SPOP];
        P.pri_mean = dp.mean; P.pri_ivar = dp.inv_var; P.pri_mean_e = dp.mean_e; P.pri_ivar_e = dp.inv_var_e;
    }
    A.threshold = o->threshold;
    H.nchunks = (int)((nmem + BB_POP_CHUNK - 1) / BB_POP_CHUNK);
    RbTimes pt{dh->stream};      // tools/popmean_rb_rate.py: the call's phases, each drained before the next starts
    pt.lap(0, -1);
    const std::vector<int> neu = ragged_pairing(M);
    const size_t nsz = (size_t)ns, D = (size_t)h->M.D, ng = (size_t)n_groups, nch = (size_t)H.nchunks;
    // the groups in flight: their chunk partials bounded to 256 MiB (a single group is worked whole whatever it takes)
    const size_t slab = std::min(ng, std::max<size_t>(1, ((size_t)256 << 20) / (nch * 2 * nsz * 8)));
    const int nblk = (int)std::max<long long>(1, std::min<long long>(n_groups, B.nblk));      // (P.par holds a [nblk][ns] table of sbar_j)
    double* ddraws = nullptr;
    int* dneu = nullptr;
    rc = bands_buffers(h, P, B, [&](Carve& c) {
        c(F.Z, (size_t)M.Ttot * nsz);                  // [Ttot][ns]
        c(F.zpart, (size_t)F.nchunks * zb * nsz);      // [nchunks][zb][ns]
        c(H.part, slab * nch * 2 * nsz);               // [groups in flight][nchunks][2][ns]
        c(A.unit, BB_RB_OUT * ng);                     // [6][n_groups]
        c(A.quant, BB_RB_MAX_Q * ng);                  // [n_groups][8]
        c(dneu, (neu.size() + 1) / 2);                 // the flagged pairing: ints
        c(ddraws, o->draws ? nsz * D : 0);             // [ns][D]
    });
    if (rc) return rc;
    A.ytab = P.par;
    if ((rc = ragged_upload(dh, neu, dneu, H.neu_t, H.neu_b)) || (rc = rb_draws(dh, P, ddraws, o->draws, nsz, D))) return rc;
    pt.lap(1, 0);
    if ((rc = rb_front(dh, B, A, zb, false))) return rc;
    pt.lap(2, 1);
    for (size_t g0 = 0; g0 < ng; g0 += slab) {
        const size_t g1 = std::min(ng, g0 + slab);
        H.g0 = (long long)g0; H.g1 = (long long)g1;
        pt.lap(3, -1);
        if ((rc = launch(dh->stream, k_rb_pop_part, (int)std::min<size_t>((g1 - g0) * nch, (size_t)1 << 20), BB_SCORE_NT, 0, H))) return rc;
        pt.lap(4, 2);
        if ((rc = launch(dh->stream, k_rb_pop, (int)std::min<long long>((long long)(g1 - g0), nblk), BB_SCORE_NT, (size_t)BB_RB_LDS_DOUBLES(ns), H))) return rc;
        pt.lap(5, 3);
    }
    double* units[BB_RB_OUT] = {out->q_mean, out->q_sd, out->rb_mean, out->rb_sd, out->p_pos, out->p_neg};
    if ((rc = rb_download(dh, A, ng, units, BB_RB_OUT, out->quantiles, nullptr))) return rc;
    if (out->n_members) for (size_t g = 0; g < ng; ++g) out->n_members[g] = (int32_t)nmem;
    pt.lap(6, 4);
#ifdef BB_RB_TIMES
    fprintf(stderr, "[bb_popmean_rb %lld groups, %lld members, %d chunks each, %d samples, %d quantiles] upload %.3f ms, normalisers %.3f ms, part %.3f ms, pop %.3f ms, download %.3f ms\n", n_groups, nmem, H.nchunks, ns, nq, pt.ms[0], pt.ms[1], pt.ms[2], pt.ms[3], pt.ms[4]);
#endif
    return rc;
}

// ---- Rao-Blackwellised noise-scale marginals (bb_lsrb.h) ----------------------------------------------------------------------------
static_assert(BB_LOGSIGMA_RB_MAX_SAMPLES == BB_GRID_SAMPLES_CAP && BB_LOGSIGMA_RB_MAX_SAMPLES <= BB_RB_MAX_SAMPLES, "bb_logsigma_rb limits");
extern "C" int bb_logsigma_rb_shape(const bb_handle* h, int32_t block, int64_t* n_entries) {
    if (!h || !n_entries) return bb_fail(BB_ERR_INVALID, "null argument");
    if (block != BB_LOGSIGMA_BC && block != BB_LOGSIGMA_POP) return bb_fail(BB_ERR_INVALID, "block must be BB_LOGSIGMA_BC or BB_LOGSIGMA_POP");
    const int k = block == BB_LOGSIGMA_BC ? BK_LS : BK_LSPOP;
    *n_entries = h->M.blk_hi[k] - h->M.blk_lo[k];
    return BB_OK;
}

extern "C" int bb_logsigma_rb(bb_handle* h, const bb_logsigma_rb_opts* o, const bb_logsigma_rb_out* out) {
    if (!h || !o || !out) return bb_fail(BB_ERR_INVALID, "null argument");
    if (o->block != BB_LOGSIGMA_BC && o->block != BB_LOGSIGMA_POP) return bb_fail(BB_ERR_INVALID, "block must be BB_LOGSIGMA_BC or BB_LOGSIGMA_POP");
    const bool bc = o->block == BB_LOGSIGMA_BC;
    const int nq = o->n_quantiles, ns = o->n_samples;
    if (int rc = rb_check(nq, o->probs, o->draws, ns, BB_LOGSIGMA_RB_MAX_SAMPLES, nullptr)) return rc;
    BandsCall B(h);
    bb_handle* dh = B.dh;
    const DevModel& M = dh->M;
    LsArgs L;
    memset(&L, 0, sizeof L);
    RbArgs& A = L.A;
    FreqArgs& F = A.F;
    PpcArgs& P = F.P;
    const long long n_entries = bc ? rb_units(h) : M.nt1;
    if (M.nn > 2147483647LL) return bb_fail(BB_ERR_UNSUPPORTED, "bb_logsigma_rb: more than 2^31 neutral members");
    int zb;
    int rc = rb_open(h, B, A, ns, o->seed, nq, o->probs, n_entries, &zb);
    if (rc) return rc;
    // The block's prior, indexed by entry in the caller's order.  logsigma_pop is never regrouped; a Matrix-form logsigma_bc prior of a
    // regrouped genotype handle lies in the handle's mutant order and is brought back to the caller's through perm_m.
    const DevPrior& dp = M.pri[bc ? BK_LS : BK_LSPOP];
    P.pri_mean = dp.mean; P.pri_ivar = dp.inv_var; P.pri_mean_e = dp.mean_e; P.pri_ivar_e = dp.inv_var_e;
    const bool reorder = bc && dp.mean_e && !h->perm_m.empty();
    L.nchunks = (int)((M.nn + BB_POP_CHUNK - 1) / BB_POP_CHUNK);
    RbTimes pt{dh->stream};      // tools/logsigma_rb_rate.py: the call's phases, each drained before the next starts
    pt.lap(0, -1);
    const std::vector<int> neu = bc ? std::vector<int>() : ragged_pairing(M);
    const size_t nsz = (size_t)ns, D = (size_t)h->M.D, ne = (size_t)n_entries, nch = (size_t)L.nchunks;
    // POP: the groups in flight, their chunk partials bounded to 256 MiB (a single group is worked whole whatever it takes)
    const size_t slab = bc ? 0 : std::min(ne, std::max<size_t>(1, ((size_t)256 << 20) / (std::max<size_t>(1, nch) * nsz * 8)));
    const long long nblk = rb_mix_blocks(dh, bc ? (long long)M.R * M.nb : n_entries, BB_LS_TAB, nsz);
    double* ddraws = nullptr;
    double* dpri = nullptr;
    int* dneu = nullptr;
    rc = bands_buffers(h, P, B, [&](Carve& c) {
        c(F.Z, (size_t)M.Ttot * nsz);                  // [Ttot][ns]
        c(F.zpart, (size_t)F.nchunks * zb * nsz);      // [nchunks][zb][ns]
        c(A.ytab, (size_t)nblk * BB_LS_TAB * nsz);     // [nblk][BB_LS_TAB][ns]
        c(L.part, slab * nch * nsz);                   // [groups in flight][nchunks][ns]
        c(A.unit, BB_RB_OUT * ne);                     // [6][n_entries]
        c(A.quant, BB_RB_MAX_Q * ne);                  // [n_entries][8]
        c(A.n_steps, (ne + 1) / 2);                    // [n_entries] ints
        c(dpri, reorder ? 2 * ne : 0);                 // the prior in the caller's order: mean | 1 / std^2
        c(dneu, (neu.size() + 1) / 2);                 // the flagged pairing: ints
        c(ddraws, o->draws ? nsz * D : 0);             // [ns][D]
    });
    if (rc) return rc;
    if (reorder) {
        std::vector<double> in(2 * ne), cal(2 * ne);
        if ((rc = d2h(in.data(), dp.mean_e, ne * 8, dh->stream)) || (rc = d2h(in.data() + ne, dp.inv_var_e, ne * 8, dh->stream))) return rc;
        for (size_t m = 0; m < ne; ++m) { cal[(size_t)h->perm_m[m]] = in[m]; cal[ne + (size_t)h->perm_m[m]] = in[ne + m]; }
        if ((rc = h2d(dpri, cal.data(), 2 * ne * 8, dh->stream)) || (rc = dsync(dh->stream))) return rc;      // (cal is this scope's)
        P.pri_mean_e = dpri;
        P.pri_ivar_e = dpri + ne;
    }
    if ((rc = ragged_upload(dh, neu, dneu, L.neu_t, L.neu_b)) || (rc = rb_draws(dh, P, ddraws, o->draws, nsz, D))) return rc;
    pt.lap(1, 0);
    if ((rc = rb_front(dh, B, A, zb, bc))) return rc;
    pt.lap(2, 1);
    if (bc) {
        if (n_entries > 0 && (rc = launch(dh->stream, k_ls_bc, (int)nblk, BB_SCORE_NT, (size_t)BB_GRID_LDS_DOUBLES(ns), L))) return rc;
        pt.lap(3, 3);
        pt.lap(5, -1);
    } else {
        for (size_t g0 = 0; g0 < ne; g0 += slab) {
            const size_t g1 = std::min(ne, g0 + slab);
            L.g0 = (long long)g0; L.g1 = (long long)g1;
            pt.lap(3, -1);
            if (nch && (rc = launch(dh->stream, k_ls_pop_part, (int)std::min<size_t>((g1 - g0) * nch, (size_t)1 << 20), BB_SCORE_NT, 0, L))) return rc;
            pt.lap(4, 2);
            if ((rc = launch(dh->stream, k_ls_pop, (int)std::min<long long>((long long)(g1 - g0), nblk), BB_SCORE_NT, (size_t)BB_GRID_LDS_DOUBLES(ns), L))) return rc;
            pt.lap(5, 3);
        }
    }
    double* units[BB_RB_OUT] = {out->q_mean, out->q_sd, out->rb_mean, out->rb_sd, out->sigma_mean, out->mode_mean};
    rc = rb_download(dh, A, ne, units, BB_RB_OUT, out->quantiles, out->n_terms);
    pt.lap(6, 4);
#ifdef BB_RB_TIMES
    fprintf(stderr, "[bb_logsigma_rb %s %lld entries, %d samples, %d quantiles] upload %.3f ms, normalisers %.3f ms, part %.3f ms, mixture %.3f ms, download %.3f ms\n", bc ? "bc" : "pop", n_entries, ns, nq, pt.ms[0], pt.ms[1], pt.ms[2], pt.ms[3], pt.ms[4]);
#endif
    return rc;
}

// ---- Rao-Blackwellised logtau marginals (bb_ltrb.h) ---------------------------------------------------------------------------------
static_assert(BB_LOGTAU_RB_MAX_SAMPLES == BB_GRID_SAMPLES_CAP && BB_LOGTAU_RB_MAX_SAMPLES <= BB_RB_MAX_SAMPLES && BB_LOGTAU_FULL == BB_LT_FULL &&
              BB_LOGTAU_COLLAPSED == BB_LT_COLLAPSED, "bb_logtau_rb limits");
extern "C" int bb_logtau_rb_shape(const bb_handle* h, int64_t* n_entries) {
    if (!h || !n_entries) return bb_fail(BB_ERR_INVALID, "null argument");
    *n_entries = h->M.kind < BB_MODEL_GENOTYPE ? 0 : h->M.blk_hi[BK_LT] - h->M.blk_lo[BK_LT];
    return BB_OK;
}

extern "C" int bb_logtau_rb(bb_handle* h, const bb_logtau_rb_opts* o, const bb_logtau_rb_out* out) {
    if (!h || !o || !out) return bb_fail(BB_ERR_INVALID, "null argument");
    if (o->mode != BB_LOGTAU_FULL && o->mode != BB_LOGTAU_COLLAPSED) return bb_fail(BB_ERR_INVALID, "mode must be BB_LOGTAU_FULL or BB_LOGTAU_COLLAPSED");
    const int nq = o->n_quantiles, ns = o->n_samples;
    if (int rc = rb_check(nq, o->probs, o->draws, ns, BB_LOGTAU_RB_MAX_SAMPLES, nullptr)) return rc;
    if (h->M.kind == BB_MODEL_FITNESS || h->M.kind == BB_MODEL_MULTIENV)
        return bb_fail(BB_ERR_UNSUPPORTED, "bb_logtau_rb applies to the hierarchical models only: model kind %d (%s) has no logtau", (int)h->M.kind,
                       h->M.kind == BB_MODEL_FITNESS ? "BB_MODEL_FITNESS" : "BB_MODEL_MULTIENV");
    BandsCall B(h);
    bb_handle* dh = B.dh;
    const DevModel& M = dh->M;
    LtArgs L;
    memset(&L, 0, sizeof L);
    RbArgs& A = L.A;
    FreqArgs& F = A.F;
    PpcArgs& P = F.P;
    const long long n_entries = rb_units(h);      // (the logtau block has one entry per unit of bb_fitness_rb)
    if (n_entries != h->M.blk_hi[BK_LT] - h->M.blk_lo[BK_LT]) return bb_fail(BB_ERR_INVALID, "unexpected block layout");
    int zb;
    int rc = rb_open(h, B, A, ns, o->seed, nq, o->probs, n_entries, &zb);
    if (rc) return rc;
    const DevPrior& dp = M.pri[BK_LT];            // Vector form: one (mean, 1 / std^2) for every entry
    P.pri_mean = dp.mean; P.pri_ivar = dp.inv_var; P.pri_mean_e = nullptr; P.pri_ivar_e = nullptr;
    L.mode = o->mode;
    RbTimes pt{dh->stream};      // tools/logtau_rb_rate.py: the call's phases, each drained before the next starts
    pt.lap(0, -1);
    const size_t nsz = (size_t)ns, D = (size_t)h->M.D, ne = (size_t)n_entries;
    const long long nblk = rb_mix_blocks(dh, (long long)M.R * M.nb, BB_LT_TAB, nsz);
    double* ddraws = nullptr;
    rc = bands_buffers(h, P, B, [&](Carve& c) {
        c(F.Z, (size_t)M.Ttot * nsz);                  // [Ttot][ns]
        c(F.zpart, (size_t)F.nchunks * zb * nsz);      // [nchunks][zb][ns]
        c(A.ytab, (size_t)nblk * BB_LT_TAB * nsz);     // [nblk][BB_LT_TAB][ns]
        c(A.unit, BB_LT_OUT * ne);                     // [8][n_entries]
        c(A.quant, BB_RB_MAX_Q * ne);                  // [n_entries][8]
        c(A.n_steps, (ne + 1) / 2);                    // [n_entries] ints
        c(ddraws, o->draws ? nsz * D : 0);             // [ns][D]
    });
    if (rc || (rc = rb_draws(dh, P, ddraws, o->draws, nsz, D))) return rc;
    pt.lap(1, 0);
    if ((rc = rb_front(dh, B, A, zb, true))) return rc;
    pt.lap(2, 1);
    if (n_entries > 0 && (rc = o->mode == BB_LOGTAU_FULL ? launch(dh->stream, k_lt_full, (int)nblk, BB_SCORE_NT, (size_t)BB_GRID_LDS_DOUBLES(ns), L)
                                                        : launch(dh->stream, k_lt_collapsed, (int)nblk, BB_SCORE_NT, (size_t)BB_GRID_LDS_DOUBLES(ns), L))) return rc;
    pt.lap(3, 2);
    if (out->n_two_modes && ne) {                      // (counted in a double on the device: exact up to 2^53)
        std::vector<double> two(ne);
        if ((rc = d2h(two.data(), A.unit + (size_t)(BB_LT_OUT - 1) * ne, ne * 8, dh->stream))) return rc;
        for (size_t g = 0; g < ne; ++g) out->n_two_modes[g] = (int32_t)two[g];
    }
    double* units[BB_LT_OUT - 1] = {out->q_mean, out->q_sd, out->rb_mean, out->rb_sd, out->tau_mean, out->pool_mean, out->mode_mean};
    rc = rb_download(dh, A, ne, units, BB_LT_OUT - 1, out->quantiles, out->n_terms);
    pt.lap(4, 3);
#ifdef BB_RB_TIMES
    fprintf(stderr, "[bb_logtau_rb %s %lld entries, %d samples, %d quantiles] upload %.3f ms, normalisers %.3f ms, mixture %.3f ms, download %.3f ms\n", o->mode == BB_LOGTAU_FULL ? "full" : "collapsed", n_entries, ns, nq, pt.ms[0], pt.ms[1], pt.ms[2], pt.ms[3]);
#endif
    return rc;
}

// ---- Rao-Blackwellised loglambda marginals (bb_llrb.h) ------------------------------------------------------------------------------
static_assert(BB_LOGLAMBDA_RB_MAX_SAMPLES == BB_GRID_SAMPLES_CAP && BB_LOGLAMBDA_RB_MAX_SAMPLES <= BB_RB_MAX_SAMPLES, "bb_loglambda_rb limits");
extern "C" int bb_loglambda_rb_shape(const bb_handle* h, int64_t* n_rows, int32_t* n_cols) { return bb_freq_shape(h, n_rows, n_cols); }

extern "C" int bb_loglambda_rb(bb_handle* h, const bb_loglambda_rb_opts* o, const bb_loglambda_rb_out* out) {
    if (!h || !o || !out) return bb_fail(BB_ERR_INVALID, "null argument");
    const int nq = o->n_quantiles, ns = o->n_samples;
    if (int rc = rb_check(nq, o->probs, o->draws, ns, BB_LOGLAMBDA_RB_MAX_SAMPLES, nullptr)) return rc;
    BandsCall B(h);
    bb_handle* dh = B.dh;
    const DevModel& M = dh->M;
    const long long n_all = (long long)M.R * M.B;
    const int n_cols = freq_cols(h);
    const long long n_req = o->rows ? o->n_rows : n_all;
    if (o->rows) {
        if (n_req < 0) return bb_fail(BB_ERR_INVALID, "n_rows must not be negative");
        for (long long x = 0; x < n_req; ++x)
            if (o->rows[x] < 0 || o->rows[x] >= n_all || (x > 0 && o->rows[x] <= o->rows[x - 1]))
                return bb_fail(BB_ERR_INVALID, "rows must be bb_freq_bands rows in 0..%lld, strictly ascending", n_all - 1);
    }
    if (n_req == 0) return BB_OK;
    LlArgs L;
    memset(&L, 0, sizeof L);
    RbArgs& A = L.A;
    FreqArgs& F = A.F;
    PpcArgs& P = F.P;
    const size_t nsz = (size_t)ns, D = (size_t)h->M.D, nr = (size_t)n_req, ne = nr * (size_t)n_cols, ng = (size_t)M.nt1;
    int zb;
    int rc = rb_open(h, B, A, ns, o->seed, nq, o->probs, (long long)ne, &zb);
    if (rc) return rc;
    const size_t nch = (size_t)F.nchunks;
    L.n_req = n_req;
    L.n_cols = n_cols;
    L.quirk = M.quirk;
    LlrbTimes pt{dh->stream};    // tools/loglambda_rb_rate.py: the call's phases, each drained before the next starts
    pt.lap(0, -1);
    // The entries' constants, in the order of the result: the prior element and the count of (row, t).  Both lie in the handle in its
    // own barcode order ([B][T_r] per replicate, the mutants possibly regrouped); the rows are the caller's.
    const DevPrior& dp = M.pri[BK_L];
    long long ncnt = 0;
    for (int r = 0; r < M.R; ++r) ncnt += (long long)M.T[r] * M.B;
    std::vector<unsigned> cnt((size_t)ncnt);
    std::vector<double> pri;
    if ((rc = d2h(cnt.data(), M.counts, (size_t)ncnt * 4, dh->stream))) return rc;
    if (dp.mean_e) {
        pri.resize(2 * (size_t)ncnt);
        if ((rc = d2h(pri.data(), dp.mean_e, (size_t)ncnt * 8, dh->stream)) || (rc = d2h(pri.data() + ncnt, dp.inv_var_e, (size_t)ncnt * 8, dh->stream))) return rc;
    }
    std::vector<long long> own((size_t)M.nb);      // the caller's mutant -> the handle's
    for (long long m = 0; m < M.nb; ++m) own[(size_t)(h->perm_m.empty() ? m : h->perm_m[(size_t)m])] = m;
    std::vector<double> ent(3 * ne, 0.0);
    std::vector<int64_t> reads(ne, 0);
    std::vector<int32_t> sides(ne, 0);
    std::vector<char> live(ne, 0);                 // 0: a cell t >= T_r of a shorter replicate
    for (size_t x = 0; x < nr; ++x) {
        const long long row = o->rows ? o->rows[x] : (long long)x;
        const int r = (int)(row / M.B), T = M.T[r];
        const long long b = row % M.B, bc = b < M.nn ? b : M.nn + own[(size_t)(b - M.nn)];
        for (int t = 0; t < T; ++t) {
            const size_t e = x * (size_t)n_cols + t, at = (size_t)(M.cnt_off[r] + bc * T + t), pat = (size_t)(M.off_l[r] - M.blk_lo[BK_L] + bc * T + t);
            ent[e] = dp.mean_e ? pri[pat] : dp.mean;
            ent[ne + e] = dp.mean_e ? pri[(size_t)ncnt + pat] : dp.inv_var;
            ent[2 * ne + e] = (double)cnt[at];
            reads[e] = (int64_t)cnt[at];
            sides[e] = (t + 1 < T) + (t >= 1);
            live[e] = 1;
        }
    }
    // the steps in flight: their chunk partials bounded to 256 MiB (a single step is worked whole whatever it takes)
    const size_t slab = std::min(ng, std::max<size_t>(1, ((size_t)256 << 20) / (nch * 2 * nsz * 8)));
    const long long nblk = rb_mix_blocks(dh, n_req, BB_LL_TAB, nsz);
    double* ddraws = nullptr;
    double* dent = nullptr;
    long long* drows = nullptr;
    rc = bands_buffers(h, P, B, [&](Carve& c) {
        c(F.Z, (size_t)M.Ttot * nsz);                  // [Ttot][ns]
        c(F.zpart, (size_t)F.nchunks * zb * nsz);      // [nchunks][zb][ns]
        c(A.ytab, (size_t)nblk * BB_LL_TAB * nsz);     // [nblk][BB_LL_TAB][ns]
        c(L.part, slab * nch * 2 * nsz);               // [steps in flight][nchunks][2][ns]
        c(L.ab, ng * 2 * nsz);                         // [nt1][2][ns]
        c(A.unit, BB_RB_OUT * ne);                     // [6][n_entries]
        c(A.quant, BB_RB_MAX_Q * ne);                  // [n_entries][8]
        c(dent, 3 * ne);                               // [3][n_entries]: a, 1 / std^2, R
        c(drows, o->rows ? nr : 0);                    // [n_req] 64-bit rows
        c(ddraws, o->draws ? nsz * D : 0);             // [ns][D]
    });
    if (rc) return rc;
    if ((rc = h2d(dent, ent.data(), 3 * ne * 8, dh->stream))) return rc;
    L.ent = dent;
    if (o->rows) {
        static_assert(sizeof(long long) == sizeof(int64_t), "rows are passed on as they are");
        if ((rc = h2d(drows, o->rows, nr * 8, dh->stream))) return rc;
        L.rows = drows;
    }
    if ((rc = rb_draws(dh, P, ddraws, o->draws, nsz, D))) return rc;
    pt.lap(1, 0);
    if ((rc = rb_front(dh, B, A, zb, true))) return rc;
    pt.lap(2, 1);
    for (size_t g0 = 0; g0 < ng; g0 += slab) {
        const size_t g1 = std::min(ng, g0 + slab);
        L.g0 = (long long)g0; L.g1 = (long long)g1;
        if ((rc = launch(dh->stream, k_ll_part, (int)std::min<size_t>((g1 - g0) * nch, (size_t)1 << 20), BB_SCORE_NT, 0, L))) return rc;
        const int gs = (int)std::max<size_t>(1, std::min<size_t>(((g1 - g0) * nsz + 255) / 256, 4096));
        if ((rc = launch(dh->stream, k_ll_sum, gs, 256, 0, L))) return rc;
    }
    pt.lap(3, 2);
    if ((rc = launch(dh->stream, k_ll, (int)nblk, BB_SCORE_NT, (size_t)BB_GRID_LDS_DOUBLES(ns), L))) return rc;
    pt.lap(4, 3);
    double* units[BB_RB_OUT] = {out->q_mean, out->q_sd, out->rb_mean, out->rb_sd, out->lambda_mean, out->mode_mean};
    if ((rc = rb_download(dh, A, ne, units, BB_RB_OUT, out->quantiles, nullptr, live.data()))) return rc;
    if (out->n_reads) memcpy(out->n_reads, reads.data(), ne * sizeof(int64_t));
    if (out->n_sides) memcpy(out->n_sides, sides.data(), ne * sizeof(int32_t));
    pt.lap(5, 4);
#ifdef BB_LLRB_TIMES
    fprintf(stderr, "[bb_loglambda_rb %lld rows of %lld, %d columns, %d chunks, %d samples, %d quantiles] upload %.3f ms, normalisers %.3f ms, tables %.3f ms, entries %.3f ms, download %.3f ms\n", n_req, n_all, n_cols, F.nchunks, ns, nq, pt.ms[0], pt.ms[1], pt.ms[2], pt.ms[3], pt.ms[4]);
#endif
    return rc;
}

// ---- chain diagnostics (bb_chain.h) --------------------------------------------------------------------------------------------
static_assert(BB_CHAIN_MAX_K == BB_PPC_MAX_K && BB_CHAIN_MAX_Q == BB_CHAIN_QSTRIDE && BB_CHAIN_LAG_BATCH == BB_CHAIN_LAGS &&
              2 * BB_CHAIN_MAX_Q <= BB_PPC_MAX_TGT, "bb_chain_summary limits");

// What bb_chain_summary and bb_trace_summary share.  chain_plan: the options that shape the statistics into C, the slab width, and the
// device buffer -- the slab as filled, its transpose, the slab's results (they lie together and come back in one copy: stat | quant |
// nlags), then whatever `extra` names.  chain_slabs: the loop over slabs of columns, fill(c0) putting columns c0 .. c0 + C.sc into the
// slab and take(c0) collecting their results; pt's laps 0 .. 4 bracket the four phases of every slab.
struct ChainSlabs {
    double* slab = nullptr;        // [K][ld]
    long long ld = 0;
    size_t n_stat = 0, n_quant = 0, n_lags = 0, nres = 0;      // doubles of the slab's results
};
template <class X>
static int chain_plan(bb_handle* dh, int W, int N, int max_lag, int nq, const double* probs, long long slab_cols, long long n_cols,
                      ChainArgs& C, ChainSlabs& L, X&& extra) {
    const long long K = (long long)W * N;
    memset(&C, 0, sizeof C);
    PpcArgs& P = C.P;
    P.K = (int)K;
    C.W = W;
    C.N = N;
    C.lag_max = max_lag ? std::min(max_lag, N - 1) : N - 1;
    C.ess_cap = (double)K * log10((double)K);
    // the select takes the order statistics and forms no bands (n_q = 0): one pair per probability
    C.nq = nq;
    quantile_plan(K, probs, nq, P);
    // slab: the caller's column count, or what BB_CHAIN_SLAB_BYTES of slab rows hold (whole transpose tiles)
    long long ld = slab_cols;
    if (!ld) {
        ld = std::max<long long>(1, (long long)BB_CHAIN_SLAB_BYTES / (8 * K));
        if (ld >= BB_CHAIN_TILE) ld -= ld % BB_CHAIN_TILE;
    }
    ld = std::min<long long>(ld, n_cols);
    L.ld = ld;
    L.n_stat = 5 * (size_t)ld;
    L.n_quant = (size_t)BB_CHAIN_QSTRIDE * ld;
    L.n_lags = ((size_t)ld + 1) / 2;
    L.nres = L.n_stat + L.n_quant + L.n_lags;
    int rc = carve(dh->buf[BUF_CHAIN], [&](Carve& c) {
        c(L.slab, (size_t)K * ld);                     // [K][ld] as uploaded / gathered
        c(C.colT, (size_t)K * ld);                     // [ld][K]
        c(C.stat, L.n_stat);                           // mean, sd, mcse, ess, rhat [5][ld]
        c(C.quant, L.n_quant);                         // [ld][BB_CHAIN_QSTRIDE]
        c(C.nlags, L.n_lags);                          // [ld] ints
        extra(c);
    });
    if (rc) return rc;
    C.slab = L.slab;
    C.ld = ld;
    return BB_OK;
}
template <class F, class T, class PT>
static int chain_slabs(bb_handle* dh, ChainArgs& C, long long n_cols, F&& fill, T&& take, PT& pt) {
    const long long K = C.P.K, ld = C.ld;
    int rc;
    for (long long c0 = 0; c0 < n_cols; c0 += ld) {
        C.sc = std::min<long long>(ld, n_cols - c0);
        pt.lap(0, -1);
        if ((rc = fill(c0))) return rc;
        pt.lap(1, 0);
        const long long tiles = ((C.sc + BB_CHAIN_TILE - 1) / BB_CHAIN_TILE) * ((K + BB_CHAIN_TILE - 1) / BB_CHAIN_TILE);
        if ((rc = launch(dh->stream, k_chain_transpose, (int)std::min<long long>(tiles, 1 << 16), BB_CHAIN_TNT, BB_CHAIN_TILE * (BB_CHAIN_TILE + 1), C))) return rc;
        pt.lap(2, 1);
        if ((rc = launch(dh->stream, k_chain_stats, (int)std::min<long long>(C.sc, 1 << 20), BB_CHAIN_NT, (size_t)bb_chain_lds_doubles(C.P.K), C))) return rc;
        pt.lap(3, 2);
        if ((rc = take(c0))) return rc;
        pt.lap(4, 3);
    }
    return BB_OK;
}
extern "C" int bb_chain_summary(bb_handle* h, const bb_chain_opts* o, int64_t n_cols, const double* chain, const bb_chain_out* out) {
    if (!h || !o || !chain || !out) return bb_fail(BB_ERR_INVALID, "null argument");
    if (n_cols < 1) return bb_fail(BB_ERR_INVALID, "n_cols must be >= 1");
    if (o->n_chains < 1 || o->n_draws < 4) return bb_fail(BB_ERR_INVALID, "n_chains must be >= 1 and n_draws >= 4");
    const int nq = o->n_quantiles;
    if (nq < 0 || nq > BB_CHAIN_MAX_Q || (nq > 0 && !o->probs)) return bb_fail(BB_ERR_INVALID, "n_quantiles must be in 0..%d (with probs)", BB_CHAIN_MAX_Q);
    for (int i = 0; i < nq; ++i)
        if (!(o->probs[i] >= 0.0 && o->probs[i] <= 1.0)) return bb_fail(BB_ERR_INVALID, "All quantiles must be between zero and one");
    if (o->max_lag < 0 || o->slab_cols < 0) return bb_fail(BB_ERR_INVALID, "max_lag and slab_cols must be >= 0");
    const long long K = (long long)o->n_chains * o->n_draws;
    if (K > BB_CHAIN_MAX_K) return bb_fail(BB_ERR_UNSUPPORTED, "n_chains * n_draws = %lld must be <= %d", K, BB_CHAIN_MAX_K);
    bb_handle* dh = sampling_handle(h);      // (nothing of the model is read)
    BB_ENTER(dh);
    ChainArgs C;
    ChainSlabs L;
    int rc = chain_plan(dh, o->n_chains, o->n_draws, o->max_lag, nq, o->probs, o->slab_cols, n_cols, C, L, [](Carve&) {});
    if (rc) return rc;
    const long long ld = L.ld;
    std::vector<double> res(L.nres);
    double* outs[5] = {out->mean, out->sd, out->mcse, out->ess, out->rhat};
    ChainTimes pt{dh->stream};   // tools/chain_summary_rate.py: the call's phases, each drained before the next starts
    rc = chain_slabs(dh, C, n_cols,
        [&](long long c0) { return h2d_2d(L.slab, (size_t)ld * 8, chain + c0, (size_t)n_cols * 8, (size_t)C.sc * 8, (size_t)K, dh->stream); },
        [&](long long c0) {
            if (int r = d2h(res.data(), C.stat, L.nres * 8, dh->stream)) return r;
            for (int s = 0; s < 5; ++s)
                if (outs[s]) memcpy(outs[s] + c0, res.data() + (size_t)s * ld, (size_t)C.sc * 8);
            if (out->quantiles && nq)
                for (long long c = 0; c < C.sc; ++c) memcpy(out->quantiles + (size_t)(c0 + c) * nq, res.data() + L.n_stat + c * BB_CHAIN_QSTRIDE, (size_t)nq * 8);
            if (out->n_lags) memcpy(out->n_lags + c0, res.data() + L.n_stat + L.n_quant, (size_t)C.sc * 4);
            return 0;
        }, pt);
    if (rc) return rc;
#ifdef BB_CHAIN_TIMES
    fprintf(stderr, "[bb_chain_summary %lld x %lld, slabs of %lld] upload %.3f ms, transpose %.3f ms, stats %.3f ms, download %.3f ms\n", K, (long long)n_cols, ld, pt.ms[0], pt.ms[1], pt.ms[2], pt.ms[3]);
#endif
    return BB_OK;
}

// ---- the iterate trace (bb_trace.h): ring, snapshots, summary ------------------------------------------------------------------------
static_assert(BB_TRACE_MAX_SNAPSHOTS == BB_CHAIN_MAX_K, "a window of the whole ring is one pooled column");

extern "C" int bb_trace_begin(bb_handle* h, const bb_trace_opts* o) {
    if (!h || !o) return bb_fail(BB_ERR_INVALID, "null argument");
    BB_GROUP_UNSUPPORTED(h, "bb_trace_begin");
    if (h->o.world_size > 1) return bb_fail(BB_ERR_UNSUPPORTED, "bb_trace_begin is not available on a sharded handle (world_size > 1)");
    if (h->trace_ring) return bb_fail(BB_ERR_INVALID, "an iterate trace is on already (bb_trace_end first)");
    if (o->every < 1) return bb_fail(BB_ERR_INVALID, "every must be >= 1");
    if (o->capacity < 8 || o->capacity > BB_TRACE_MAX_SNAPSHOTS) return bb_fail(BB_ERR_INVALID, "capacity = %d is outside 8 .. %d", (int)o->capacity, BB_TRACE_MAX_SNAPSHOTS);
    BB_ENTER(h);
    void* p = nullptr;
    const size_t bytes = (size_t)o->capacity * 2 * (size_t)h->M.D * 8;
    if (dmalloc(&p, bytes)) {
        const std::string why(g_err);
        return bb_fail(BB_ERR_DEVICE, "bb_trace_begin: no room for a ring of %d snapshots (%zu bytes): %s", (int)o->capacity, bytes, why.c_str());
    }
    h->trace_ring = (double*)p;
    h->trace_every = o->every;
    h->trace_cap = o->capacity;
    trace_reset(h);
    return BB_OK;
}

extern "C" int bb_trace_end(bb_handle* h) {
    if (!h) return bb_fail(BB_ERR_INVALID, "null handle");
    if (!h->trace_ring) return BB_OK;
    BB_ENTER(h);
    const int rc = dsync(h->stream);
    dfree(h->trace_ring);
    h->trace_ring = nullptr;
    h->trace_every = h->trace_cap = 0;
    trace_reset(h);
    return rc;
}

static long long trace_first_live(const bb_handle* h) { return std::max<long long>(0, h->trace_taken - h->trace_cap); }
// snapshots first .. first + n - 1 must all be in the ring
static int trace_live(const bb_handle* h, const char* what, long long first, long long n) {
    if (!h->trace_ring) return bb_fail(BB_ERR_INVALID, "%s: no iterate trace is on (bb_trace_begin)", what);
    if (first < trace_first_live(h) || n < 0 || first + n > h->trace_taken)
        return bb_fail(BB_ERR_INVALID, "%s: snapshots %lld .. %lld are not all live: the ring holds %lld .. %lld (%lld taken, capacity %d)", what, first,
                       first + n - 1, trace_first_live(h), h->trace_taken - 1, h->trace_taken, h->trace_cap);
    return BB_OK;
}

extern "C" int bb_trace_count(bb_handle* h, int64_t* taken, int64_t* first_live) {
    if (!h) return bb_fail(BB_ERR_INVALID, "null handle");
    if (!h->trace_ring) return bb_fail(BB_ERR_INVALID, "bb_trace_count: no iterate trace is on (bb_trace_begin)");
    if (taken) *taken = h->trace_taken;
    if (first_live) *first_live = trace_first_live(h);
    return BB_OK;
}

extern "C" int bb_trace_get(bb_handle* h, int64_t first, int64_t n, double* mu, double* omega) {
    if (!h) return bb_fail(BB_ERR_INVALID, "null handle");
    if (int rc = trace_live(h, "bb_trace_get", first, n)) return rc;
    BB_ENTER(h);
    const size_t D = (size_t)h->M.D;
    std::vector<double> row(2 * D);
    int rc = dsync(h->stream);
    for (int64_t k = 0; k < n && !rc; ++k) {
        const size_t slot = (size_t)((first + k) % h->trace_cap);
        if ((rc = d2h(row.data(), h->trace_ring + slot * 2 * D, 2 * D * 8, h->stream))) break;
        double* dst[2] = {mu ? mu + (size_t)k * D : nullptr, omega ? omega + (size_t)k * D : nullptr};
        for (int part = 0; part < 2; ++part) {
            if (!dst[part]) continue;
            if (h->cidx.empty()) memcpy(dst[part], row.data() + part * D, D * 8);
            else perm_scatter(h, row.data() + part * D, dst[part]);
        }
    }
    return rc;
}

// internal range of layout block b: the handle's order keeps every block whole, so it is the internal block whose first latent the
// caller's range holds
static void trace_block_range(const bb_handle* h, size_t b, long long* lo, long long* hi) {
    const bb_block_range& r = h->blocks[b];
    *lo = r.lo;
    *hi = r.hi;
    if (h->cidx.empty()) return;
    for (int k = 0; k < BK_COUNT; ++k) {
        const long long klo = h->M.blk_lo[k], khi = h->M.blk_hi[k];
        if (khi > klo && h->cidx[(size_t)klo] >= r.lo && h->cidx[(size_t)klo] < r.hi) { *lo = klo; *hi = khi; return; }
    }
}

extern "C" int bb_trace_summary(bb_handle* h, const bb_trace_sum_opts* o, const bb_trace_sum_out* out) {
    if (!h || !o || !out) return bb_fail(BB_ERR_INVALID, "null argument");
    if (!h->trace_ring) return bb_fail(BB_ERR_INVALID, "bb_trace_summary: no iterate trace is on (bb_trace_begin)");
    if (o->n_chains < 1 || o->n_draws < 4) return bb_fail(BB_ERR_INVALID, "n_chains must be >= 1 and n_draws >= 4");
    if (o->max_lag < 0 || o->slab_cols < 0) return bb_fail(BB_ERR_INVALID, "max_lag and slab_cols must be >= 0");
    if (!(std::isfinite(o->rhat_max) && o->rhat_max >= 1.0)) return bb_fail(BB_ERR_INVALID, "rhat_max must be finite and >= 1");
    const long long K = (long long)o->n_chains * o->n_draws;
    if (K > BB_CHAIN_MAX_K) return bb_fail(BB_ERR_UNSUPPORTED, "n_chains * n_draws = %lld must be <= %d", K, BB_CHAIN_MAX_K);
    if (int rc = trace_live(h, "bb_trace_summary", o->first, K)) return rc;
    const size_t nblk = h->blocks.size();
    if (nblk > BB_TRACE_MAX_BLOCKS) return bb_fail(BB_ERR_INVALID, "unexpected block layout");
    BB_ENTER(h);
    const size_t D = (size_t)h->M.D, D2 = 2 * D;
    ChainArgs C;
    ChainSlabs L;
    TraceVerdictArgs V;
    memset(&V, 0, sizeof V);
    double* all = nullptr;         // the columns' statistics where the verdict reads them and the downloads start
    int* all_lags = nullptr;
    int rc = chain_plan(h, o->n_chains, o->n_draws, o->max_lag, 0, nullptr, o->slab_cols, (long long)D2, C, L, [&](Carve& c) {
        c(all, 5 * D2);                                // mean, sd, mcse, ess, rhat [5][2 D], the handle's internal order
        c(all_lags, (D2 + 1) / 2);                     // [2 D] ints
        c(V.val, 6 * nblk);                            // [2 nblk][3]
        c(V.cnt, 6 * nblk);                            // [2 nblk][3] 64-bit counts
    });
    if (rc) return rc;
    TraceArgs T;
    memset(&T, 0, sizeof T);
    T.ring = h->trace_ring;
    T.D = (long long)D;
    T.D2 = (long long)D2;
    T.cap = h->trace_cap;
    T.slab = L.slab;
    T.ld = L.ld;
    T.first = o->first;
    T.K = (int)K;
    TraceTimes pt{h->stream};    // tools/trace_cost.py: the call's phases, each drained before the next starts
    rc = chain_slabs(h, C, (long long)D2,
        [&](long long c0) {
            T.c0 = c0;
            T.sc = C.sc;
            const long long runs = (long long)K * ((C.sc + BB_TRACE_NT - 1) / BB_TRACE_NT);
            return launch(h->stream, k_trace_gather, (int)std::min<long long>(runs, 1 << 16), BB_TRACE_NT, 0, T);
        },
        [&](long long c0) {      // the slab's results to their columns' places (they stay on the device)
            for (size_t s = 0; s < 5; ++s)
                if (int r = d2d(all + s * D2 + c0, C.stat + s * (size_t)L.ld, (size_t)C.sc * 8, h->stream)) return r;
            return d2d(all_lags + c0, C.nlags, (size_t)C.sc * 4, h->stream);
        }, pt);
    if (rc) return rc;
    if (out->blocks) {
        V.stat = all;
        V.D = (long long)D;
        V.D2 = (long long)D2;
        V.nblk = (int)nblk;
        V.rhat_max = o->rhat_max;
        for (size_t b = 0; b < nblk; ++b) trace_block_range(h, b, &V.lo[b], &V.hi[b]);
        if ((rc = launch(h->stream, k_trace_verdict, 2 * (int)nblk, BB_TRACE_VNT, (size_t)bb_trace_verdict_lds_doubles(), V))) return rc;
    }
    pt.lap(5, 4);
    // downloads: only what was asked for, the handle's order -> the caller's per half
    double* outs[5] = {out->mean, out->sd, out->mcse, out->ess, out->rhat};
    std::vector<double> tmp;
    for (size_t s = 0; s < 5; ++s) {
        if (!outs[s]) continue;
        if (h->cidx.empty()) { if ((rc = d2h(outs[s], all + s * D2, D2 * 8, h->stream))) return rc; continue; }
        tmp.resize(D2);
        if ((rc = d2h(tmp.data(), all + s * D2, D2 * 8, h->stream))) return rc;
        perm_scatter(h, tmp.data(), outs[s]);
        perm_scatter(h, tmp.data() + D, outs[s] + D);
    }
    if (out->n_lags) {
        if (h->cidx.empty()) { if ((rc = d2h(out->n_lags, all_lags, D2 * 4, h->stream))) return rc; }
        else {
            std::vector<int> li(D2);
            if ((rc = d2h(li.data(), all_lags, D2 * 4, h->stream))) return rc;
            for (size_t i = 0; i < D; ++i) { out->n_lags[(size_t)h->cidx[i]] = li[i]; out->n_lags[D + (size_t)h->cidx[i]] = li[D + i]; }
        }
    }
    if (out->blocks) {
        std::vector<double> val(6 * nblk);
        std::vector<long long> cnt(6 * nblk);
        if ((rc = d2h(val.data(), V.val, val.size() * 8, h->stream)) || (rc = d2h(cnt.data(), V.cnt, cnt.size() * 8, h->stream))) return rc;
        for (size_t v = 0; v < 2 * nblk; ++v) {
            bb_trace_block& B = out->blocks[v];
            memset(&B, 0, sizeof B);
            memcpy(B.name, h->blocks[v % nblk].name, sizeof B.name);
            B.part = (int32_t)(v / nblk);
            B.n_cols = h->blocks[v % nblk].hi - h->blocks[v % nblk].lo;
            B.n_nonfinite = cnt[3 * v];
            B.n_const = cnt[3 * v + 1];
            B.n_above = cnt[3 * v + 2];
            B.max_rhat = val[3 * v];
            B.min_ess = val[3 * v + 1];
            B.max_mcse_rel = val[3 * v + 2];
        }
    }
    rc = dsync(h->stream);
    pt.lap(6, 5);
#ifdef BB_TRACE_TIMES
    fprintf(stderr, "[bb_trace_summary %lld x %zu, slabs of %lld] gather %.3f ms, transpose %.3f ms, stats %.3f ms, collect %.3f ms, verdict %.3f ms, download %.3f ms\n", K, D2, L.ld, pt.ms[0], pt.ms[1], pt.ms[2], pt.ms[3], pt.ms[4], pt.ms[5]);
#endif
    return rc;
}
