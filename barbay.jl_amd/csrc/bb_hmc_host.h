// bb_hmc_host.h -- host side of the HMC session (bb_hmc_begin, bb_hmc_step, bb_hmc_get, bb_hmc_end; the kernels: bb_hmc.h, the evaluations:
// bb_logp.h through logp_launch of bb_analysis.h).  Included only by bb_engine.hip, once, behind bb_analysis.h: the same translation unit,
// built by hipcc and by g++ -DBB_EMU -x c++ like the rest of the engine.
//
// The session lives in buf[BUF_HMC], carved once by bb_hmc_begin: nothing else grows that buffer, so the pointers in h->hmc hold until
// the next begin or bb_destroy (the streaming moments of bb_hmc_accum_host.h have buf[BUF_HMC_ACC] to themselves).  Per transition the
// host link carries eps and n_leapfrog (W entries each) up, 3 W doubles down, W flags up.

static int hmc_common_checks(bb_handle* h, const char* what) {
    if (!h->shards.empty()) return bb_fail(BB_ERR_UNSUPPORTED, "%s is not available on a multi-device handle (n_devices > 1)", what);
    if (h->o.world_size > 1) return bb_fail(BB_ERR_UNSUPPORTED, "%s is not available on a sharded handle (world_size > 1)", what);
    return BB_OK;
}

// rows of the handle's order, stride Dz, on the device -> the caller's [W][D]
static int hmc_rows_out(bb_handle* h, const double* dev, double* out) {
    const size_t W = (size_t)h->hmc.W, D = (size_t)h->hmc.D, Dz = (size_t)h->hmc.Dz;
    if (h->cidx.empty() && Dz == D) return d2h(out, dev, W * D * 8, h->stream);
    std::vector<double> rows(W * Dz);
    int rc = d2h(rows.data(), dev, W * Dz * 8, h->stream);
    if (rc) return rc;
    for (size_t w = 0; w < W; ++w) {
        if (h->cidx.empty()) memcpy(out + w * D, rows.data() + w * Dz, D * 8);
        else perm_scatter(h, rows.data() + w * Dz, out + w * D);
    }
    return BB_OK;
}

// The metric as the session holds it (bb_hmc_begin, bb_hmc_set_metric): inv_mass [Dz] | 1 / sqrt(inv_mass) [Dz] in the handle's order, from the
// caller's inv_mass [D] (nullptr: ones), every entry checked first.  1 / sqrt: the correctly rounded sqrt, then the division.  The pad entry
// of an odd D: inv_mass 1, 1 / sqrt 0 (its momentum is 0 and stays 0).
static int hmc_metric_rows(const bb_handle* h, const double* inv_mass, std::vector<double>& rows) {
    const size_t D = (size_t)h->M.D, Dz = (D + 1) & ~(size_t)1;
    if (inv_mass)
        for (size_t i = 0; i < D; ++i)
            if (!(std::isfinite(inv_mass[i]) && inv_mass[i] > 0.0))
                return bb_fail(BB_ERR_INVALID, "inv_mass[%lld] = %g is not finite and > 0", (long long)i, inv_mass[i]);
    rows.assign(2 * Dz, 0.0);
    double *him = rows.data(), *hsd = rows.data() + Dz;
    for (size_t i = 0; i < D; ++i) {
        const double v = inv_mass ? inv_mass[h->cidx.empty() ? i : (size_t)h->cidx[i]] : 1.0;
        him[i] = v;
        hsd[i] = 1.0 / std::sqrt(v);
    }
    if (Dz > D) { him[D] = 1.0; hsd[D] = 0.0; }
    return BB_OK;
}

extern "C" int bb_hmc_end(bb_handle* h) {
    if (!h) return bb_fail(BB_ERR_INVALID, "null argument");
    if (!h->hmc_ever) return bb_fail(BB_ERR_INVALID, "bb_hmc_end without a session: bb_hmc_begin comes first");
    h->hmc_on = h->acc_on = h->nuts_on = false;     // (a second end: BB_OK)
    if (h->buf[BUF_NUTS].p) {                       // the tree's rows are the one large thing a session leaves behind: up to 7.6 GB.  They go now
        BB_ENTER(h);
        int rc = dsync(h->stream);
        h->buf[BUF_NUTS].release();
        h->nuts = NutsArgs{};
        h->nuts_lf = nullptr;
        if (rc) return rc;
    }
    return BB_OK;
}

extern "C" int bb_hmc_begin(bb_handle* h, const bb_hmc_opts* o, const double* z0, double* logp) {
    if (!h || !o || !z0) return bb_fail(BB_ERR_INVALID, "null argument");
    int rc = hmc_common_checks(h, "bb_hmc_begin");
    if (rc) return rc;
    if (o->n_walkers < 1 || o->n_walkers > BB_HMC_MAX_WALKERS) return bb_fail(BB_ERR_INVALID, "n_walkers = %d is outside 1 .. %d", (int)o->n_walkers, BB_HMC_MAX_WALKERS);
    if (o->reserved0 != 0) return bb_fail(BB_ERR_INVALID, "bb_hmc_opts.reserved0 must be 0");
    const DevModel& M = h->M;
    const size_t W = (size_t)o->n_walkers, D = (size_t)M.D, Dz = (D + 1) & ~(size_t)1, Wp = (W + 1) & ~(size_t)1;
    std::vector<double> metric;
    if ((rc = hmc_metric_rows(h, o->inv_mass, metric))) return rc;
    BB_ENTER(h);
    h->hmc_on = h->acc_on = h->nuts_on = false;     // (a begin that fails leaves no session; the accumulators and the NUTS rows go with the session they were begun on)
    const bool geno = M.kind == BB_MODEL_GENOTYPE;
    const size_t nbs = geno ? ((size_t)M.nb + 1) & ~(size_t)1 : 0, Gs = geno ? ((size_t)M.G + 1) & ~(size_t)1 : 0;
    const size_t nchunk = (Dz + BB_HMC_CHUNK - 1) / BB_HMC_CHUNK;
    HmcArgs H{};
    LogpArgs B{};
    double *im = nullptr, *isd = nullptr, *tab = nullptr;
    long long* cidx = nullptr;
    int* accept = nullptr;
    size_t total = 0;
    rc = carve(h->buf[BUF_HMC], [&](Carve& c) {      // (every length even: pairs stay 16-byte aligned)
        c(H.z, W * Dz); c(H.g, W * Dz); c(H.zp, W * Dz); c(H.gp, W * Dz); c(H.r, W * Dz);
        c(H.logp, Wp);
        c(H.scal, 3 * Wp);
        c(im, Dz); c(isd, Dz);
        c(cidx, h->cidx.empty() ? 0 : Dz);
        c(H.kpart, (W * nchunk + 1) & ~(size_t)1);
        c(tab, Wp + Wp / 2);                           // eps | n_leapfrog (ints)
        c(accept, Wp / 2);
        c(B.part, (W * (size_t)M.K * (size_t)h->nblk + 1) & ~(size_t)1);
        c(B.zg, W * 2 * (size_t)M.nt1);
        c(B.ds, W * nbs);
        c(B.gsum, W * Gs);
        total = c.n;
    });
    if (rc) return rc;
    if ((rc = dzero(h->buf[BUF_HMC].p, total * 8, h->stream))) return rc;
    if ((rc = h2d(im, metric.data(), 2 * Dz * 8, h->stream))) return rc;      // (isd lies behind im)
    std::vector<double> host(W * Dz);
    if (!h->cidx.empty() && (rc = h2d(cidx, h->cidx.data(), D * sizeof(long long), h->stream))) return rc;
    for (size_t w = 0; w < W; ++w) {
        double* row = host.data() + w * Dz;
        if (h->cidx.empty()) memcpy(row, z0 + w * D, D * 8);
        else perm_gather(h, z0 + w * D, row);
        if (Dz > D) row[D] = 0.0;
    }
    if ((rc = h2d(H.z, host.data(), W * Dz * 8, h->stream))) return rc;
    H.inv_mass = im; H.isd = isd;
    H.cidx = h->cidx.empty() ? nullptr : cidx;
    H.eps = tab; H.nleap = (const int*)(tab + Wp); H.accept = accept;
    H.D = (long long)D; H.Dz = (long long)Dz;
    H.nchunk = (int)nchunk; H.W = (int)W; H.Wp = (int)Wp;
    H.seed = o->seed;
    B.Dz = (long long)Dz; B.nbs = (long long)nbs; B.Gs = (long long)Gs;
    B.nt = h->nblk; B.W = (int)W;
    B.c0 = logp_const(h);
    // logp and g at the start
    LogpArgs B0 = B;
    B0.z = H.z; B0.grad = H.g; B0.logp = H.logp;
    if ((rc = logp_launch(h, B0))) return rc;
    h->hmc_logp.assign(W, 0.0);
    if ((rc = d2h(h->hmc_logp.data(), H.logp, W * 8, h->stream))) return rc;
    if (logp) memcpy(logp, h->hmc_logp.data(), W * 8);
    h->hmc = H;
    h->hmc_eval = B;
    h->hmc_tab = tab;
    h->hmc_on = h->hmc_ever = true;
    return BB_OK;
}

extern "C" int bb_hmc_step(bb_handle* h, const bb_hmc_step_opts* o, const bb_hmc_step_out* out) {
    if (!h || !o) return bb_fail(BB_ERR_INVALID, "null argument");
    int rc = hmc_common_checks(h, "bb_hmc_step");
    if (rc) return rc;
    if (!h->hmc_on) return bb_fail(BB_ERR_INVALID, "bb_hmc_step without a session: bb_hmc_begin comes first");
    if (o->reserved0 != 0) return bb_fail(BB_ERR_INVALID, "bb_hmc_step_opts.reserved0 must be 0");
    if (!o->eps || !o->n_leapfrog || !o->log_u) return bb_fail(BB_ERR_INVALID, "null argument");
    HmcArgs H = h->hmc;
    const int W = H.W, Wp = H.Wp;
    int lmax = 0;
    for (int w = 0; w < W; ++w) {
        if (!(std::isfinite(o->eps[w]) && o->eps[w] > 0.0)) return bb_fail(BB_ERR_INVALID, "walker %d: eps = %g is not finite and > 0", w, o->eps[w]);
        if (o->n_leapfrog[w] < 1 || o->n_leapfrog[w] > BB_HMC_MAX_LEAPFROG)
            return bb_fail(BB_ERR_INVALID, "walker %d: n_leapfrog = %d is outside 1 .. %d", w, (int)o->n_leapfrog[w], BB_HMC_MAX_LEAPFROG);
        if (std::isnan(o->log_u[w])) return bb_fail(BB_ERR_INVALID, "walker %d: log_u is NaN", w);
        lmax = std::max(lmax, (int)o->n_leapfrog[w]);
    }
    BB_ENTER(h);
    h->nuts_started = false;           // (the travelling rows of a NUTS tree are redrawn: bb_nuts_start comes before its next leaf)
    // the transition's per-walker table: eps | n_leapfrog
    std::vector<double> tab((size_t)(Wp + Wp / 2), 0.0);
    memcpy(tab.data(), o->eps, (size_t)W * 8);
    {
        std::vector<int> nl((size_t)Wp, 0);
        for (int w = 0; w < W; ++w) nl[(size_t)w] = o->n_leapfrog[w];
        memcpy(tab.data() + Wp, nl.data(), (size_t)Wp * sizeof(int));
    }
    if ((rc = h2d(h->hmc_tab, tab.data(), tab.size() * 8, h->stream))) return rc;
    H.transition = o->transition;
    const int grid = H.nchunk * W;
    if ((rc = launch(h->stream, k_hmc_momentum, grid, BB_HMC_NT, BB_HMC_NT, H))) return rc;
    if ((rc = launch(h->stream, k_hmc_reduce, W, 64, 64, H, 0, -1))) return rc;
    LogpArgs B = h->hmc_eval;
    B.z = H.zp; B.grad = H.gp; B.logp = H.scal + 2 * (size_t)Wp;
    B.lf_n = H.nleap;
    for (int k = 0; k < lmax; ++k) {
        if ((rc = launch(h->stream, k_hmc_kick_drift, grid, BB_HMC_NT, 0, H, k))) return rc;
        B.lf_k = k;
        if ((rc = logp_launch(h, B))) return rc;
        bool ends = false;
        for (int w = 0; w < W; ++w) ends = ends || o->n_leapfrog[w] == k + 1;
        if (!ends) continue;
        if ((rc = launch(h->stream, k_hmc_kick_energy, grid, BB_HMC_NT, BB_HMC_NT, H, k))) return rc;
        if ((rc = launch(h->stream, k_hmc_reduce, W, 64, 64, H, 1, k))) return rc;
    }
    std::vector<double> scal((size_t)(3 * Wp));
    if ((rc = d2h(scal.data(), H.scal, scal.size() * 8, h->stream))) return rc;
    const double *k0 = scal.data(), *k1 = scal.data() + Wp, *lpp = scal.data() + 2 * (size_t)Wp;
    std::vector<int> acc((size_t)Wp, 0);
    bool any = false;
    for (int w = 0; w < W; ++w) {
        const double h0 = h->hmc_logp[(size_t)w] - k0[w], h1 = lpp[w] - k1[w];
        const bool fin = std::isfinite(h1), ok = fin && o->log_u[w] < h1 - h0;
        acc[(size_t)w] = ok ? 1 : 0;
        any = any || ok;
        if (out) {
            if (out->h0) out->h0[w] = h0;
            if (out->h1) out->h1[w] = h1;
            if (out->kinetic0) out->kinetic0[w] = k0[w];
            if (out->kinetic1) out->kinetic1[w] = k1[w];
            if (out->logp_prop) out->logp_prop[w] = lpp[w];
            if (out->accepted) out->accepted[w] = ok ? 1 : 0;
            if (out->divergent) out->divergent[w] = fin ? 0 : 1;
        }
    }
    if (any) {
        if ((rc = h2d(const_cast<int*>(H.accept), acc.data(), (size_t)Wp * sizeof(int), h->stream))) return rc;
        if ((rc = launch(h->stream, k_hmc_keep, grid, BB_HMC_NT, 0, H))) return rc;
        for (int w = 0; w < W; ++w) if (acc[(size_t)w]) h->hmc_logp[(size_t)w] = lpp[w];
    }
    if (out && out->logp) memcpy(out->logp, h->hmc_logp.data(), (size_t)W * 8);
    return BB_OK;
}

extern "C" int bb_hmc_get(bb_handle* h, double* z, double* logp, double* grad) {
    if (!h) return bb_fail(BB_ERR_INVALID, "null argument");
    int rc = hmc_common_checks(h, "bb_hmc_get");
    if (rc) return rc;
    if (!h->hmc_on) return bb_fail(BB_ERR_INVALID, "bb_hmc_get without a session: bb_hmc_begin comes first");
    BB_ENTER(h);
    if (z && (rc = hmc_rows_out(h, h->hmc.z, z))) return rc;
    if (grad && (rc = hmc_rows_out(h, h->hmc.g, grad))) return rc;
    if (logp && (rc = d2h(logp, h->hmc.logp, (size_t)h->hmc.W * 8, h->stream))) return rc;
    return (z || grad || logp) ? BB_OK : dsync(h->stream);
}
