// bb_hmc_accum_host.h -- host side of the session's streaming moments and of its metric (bb_hmc_accum_begin / add / reset / get / stats,
// bb_hmc_set_metric, bb_hmc_get_metric; the kernels: bb_hmc_accum.h).  Included only by bb_engine.hip, once, behind bb_hmc_host.h.
//
// The rows live in buf[BUF_HMC_ACC], carved by bb_hmc_accum_begin; the session's own buffer is not touched, so h->hmc's pointers hold.
// Per bb_hmc_accum_add the host link carries W (segment, 1 / n) entries up and nothing down; bb_hmc_accum_stats brings 4 Dz doubles down.

static int hmc_acc_checks(bb_handle* h, const char* what, bool need_acc) {
    int rc = hmc_common_checks(h, what);
    if (rc) return rc;
    if (!h->hmc_on) return bb_fail(BB_ERR_INVALID, "%s without a session: bb_hmc_begin comes first", what);
    if (need_acc && !h->acc_on) return bb_fail(BB_ERR_INVALID, "%s without accumulators: bb_hmc_accum_begin comes first (bb_hmc_begin and bb_hmc_end drop them)", what);
    return BB_OK;
}

// one row of the handle's order on the device -> the caller's [D]
static int hmc_row_out(bb_handle* h, const double* dev, double* out) {
    const size_t D = (size_t)h->hmc.D, Dz = (size_t)h->hmc.Dz;
    if (h->cidx.empty()) return d2h(out, dev, D * 8, h->stream);
    std::vector<double> row(Dz);
    int rc = d2h(row.data(), dev, Dz * 8, h->stream);
    if (rc) return rc;
    perm_scatter(h, row.data(), out);
    return BB_OK;
}

extern "C" int bb_hmc_accum_begin(bb_handle* h, const bb_hmc_accum_opts* o) {
    if (!h || !o) return bb_fail(BB_ERR_INVALID, "null argument");
    int rc = hmc_acc_checks(h, "bb_hmc_accum_begin", false);
    if (rc) return rc;
    if (o->n_segments < 1 || o->n_segments > BB_HMC_MAX_SEGMENTS) return bb_fail(BB_ERR_INVALID, "n_segments = %d is outside 1 .. %d", (int)o->n_segments, BB_HMC_MAX_SEGMENTS);
    if (o->reserved0 != 0) return bb_fail(BB_ERR_INVALID, "bb_hmc_accum_opts.reserved0 must be 0");
    BB_ENTER(h);
    h->acc_on = false;                 // (a begin that fails leaves no accumulators)
    const size_t W = (size_t)h->hmc.W, S = (size_t)o->n_segments, Dz = (size_t)h->hmc.Dz;
    HmcAccArgs A{};
    HmcAccSlot* slot = nullptr;
    HmcAccLive* live = nullptr;
    size_t total = 0;
    rc = carve(h->buf[BUF_HMC_ACC], [&](Carve& c) {      // (every length even: pairs stay 16-byte aligned)
        c(A.rows, W * S * 2 * Dz);
        c(A.out, 4 * Dz);
        c(slot, 2 * W);
        c(live, 2 * W * S);
        total = c.n;
    });
    if (rc) return rc;
    if ((rc = dzero(h->buf[BUF_HMC_ACC].p, total * 8, h->stream))) return rc;
    if ((rc = dsync(h->stream))) return rc;
    A.slot = slot; A.live = live;
    A.S = (int)S;
    h->acc = A;
    h->acc_n.assign(W * S, 0);
    h->acc_on = true;
    return BB_OK;
}

extern "C" int bb_hmc_accum_reset(bb_handle* h) {
    if (!h) return bb_fail(BB_ERR_INVALID, "null argument");
    int rc = hmc_acc_checks(h, "bb_hmc_accum_reset", true);
    if (rc) return rc;
    BB_ENTER(h);
    const size_t rows = (size_t)h->hmc.W * (size_t)h->acc.S * 2 * (size_t)h->hmc.Dz;
    if ((rc = dzero(h->acc.rows, rows * 8, h->stream))) return rc;
    if ((rc = dsync(h->stream))) return rc;
    std::fill(h->acc_n.begin(), h->acc_n.end(), 0ll);
    return BB_OK;
}

extern "C" int bb_hmc_accum_add(bb_handle* h, const int32_t* segment) {
    if (!h || !segment) return bb_fail(BB_ERR_INVALID, "null argument");
    int rc = hmc_acc_checks(h, "bb_hmc_accum_add", true);
    if (rc) return rc;
    const int W = h->hmc.W, S = h->acc.S;
    std::vector<HmcAccSlot> slot((size_t)W);
    bool any = false;
    for (int w = 0; w < W; ++w) {
        if (segment[w] < -1 || segment[w] >= S) return bb_fail(BB_ERR_INVALID, "walker %d: segment = %d is outside -1 .. %d", w, (int)segment[w], S - 1);
        slot[(size_t)w].seg = segment[w];
        slot[(size_t)w].pad = 0;
        slot[(size_t)w].inv_n = segment[w] < 0 ? 0.0 : 1.0 / (double)(h->acc_n[(size_t)w * S + segment[w]] + 1);
        any = any || segment[w] >= 0;
    }
    if (!any) return BB_OK;
    BB_ENTER(h);
    if ((rc = h2d(const_cast<HmcAccSlot*>(h->acc.slot), slot.data(), slot.size() * sizeof(HmcAccSlot), h->stream))) return rc;
    if ((rc = launch(h->stream, k_hmc_accum, h->hmc.nchunk * W, BB_HMC_NT, 0, h->hmc, h->acc))) return rc;
    if ((rc = dsync(h->stream))) return rc;
    for (int w = 0; w < W; ++w) if (segment[w] >= 0) ++h->acc_n[(size_t)w * S + segment[w]];
    return BB_OK;
}

extern "C" int bb_hmc_accum_get(bb_handle* h, int32_t walker, int32_t segment, double* mean, double* m2, int64_t* n) {
    if (!h) return bb_fail(BB_ERR_INVALID, "null argument");
    int rc = hmc_acc_checks(h, "bb_hmc_accum_get", true);
    if (rc) return rc;
    if (walker < 0 || walker >= h->hmc.W) return bb_fail(BB_ERR_INVALID, "walker = %d is outside 0 .. %d", (int)walker, h->hmc.W - 1);
    if (segment < 0 || segment >= h->acc.S) return bb_fail(BB_ERR_INVALID, "segment = %d is outside 0 .. %d", (int)segment, h->acc.S - 1);
    BB_ENTER(h);
    const size_t c = (size_t)walker * (size_t)h->acc.S + (size_t)segment, Dz = (size_t)h->hmc.Dz;
    if (mean && (rc = hmc_row_out(h, h->acc.rows + c * 2 * Dz, mean))) return rc;
    if (m2 && (rc = hmc_row_out(h, h->acc.rows + (c * 2 + 1) * Dz, m2))) return rc;
    if (n) *n = (int64_t)h->acc_n[c];
    return BB_OK;
}

extern "C" int bb_hmc_accum_stats(bb_handle* h, const bb_hmc_accum_out* out) {
    if (!h || !out) return bb_fail(BB_ERR_INVALID, "null argument");
    int rc = hmc_acc_checks(h, "bb_hmc_accum_stats", true);
    if (rc) return rc;
    const int W = h->hmc.W, S = h->acc.S;
    std::vector<HmcAccLive> live;
    long long K = 0;
    for (int w = 0; w < W; ++w)
        for (int s = 0; s < S; ++s) {
            const long long n = h->acc_n[(size_t)w * S + s];
            if (n == 1) return bb_fail(BB_ERR_INVALID, "walker %d, segment %d holds one state: a chain of the statistics needs two or none", w, s);
            if (n > 0) { live.push_back(HmcAccLive{w * S + s, 0, (double)n}); K += n; }
        }
    if (live.empty()) return bb_fail(BB_ERR_INVALID, "bb_hmc_accum_stats: no state has been added");
    BB_ENTER(h);
    const size_t D = (size_t)h->hmc.D, Dz = (size_t)h->hmc.Dz;
    HmcAccArgs A = h->acc;
    A.C = (int)live.size();
    A.K = (double)K;
    if ((rc = h2d(const_cast<HmcAccLive*>(A.live), live.data(), live.size() * sizeof(HmcAccLive), h->stream))) return rc;
    const int grid = (int)((Dz / 2 + BB_HMC_NT - 1) / BB_HMC_NT);
    if ((rc = launch(h->stream, k_hmc_accum_stats, grid, BB_HMC_NT, 0, h->hmc, A))) return rc;
    std::vector<double> rows(4 * Dz);
    if ((rc = d2h(rows.data(), A.out, rows.size() * 8, h->stream))) return rc;
    if (out->n_total) *out->n_total = (int64_t)K;
    // the derived statistics, fp64, the handle's order; then each wanted row into the caller's order
    const double *mean = rows.data(), *m2p = mean + Dz, *within = m2p + Dz, *between = within + Dz;
    const double C = (double)live.size(), Kd = (double)K, nbar = Kd / C, cap = Kd * std::log10(Kd), nan = std::nan("");
    std::vector<double> col(D);
    auto emit = [&](double* dst, auto&& f) {
        if (!dst) return;
        for (size_t i = 0; i < D; ++i) col[i] = f(i);
        if (h->cidx.empty()) memcpy(dst, col.data(), D * 8);
        else perm_scatter(h, col.data(), dst);
    };
    auto fin = [&](size_t i) { return std::isfinite(mean[i]) && std::isfinite(m2p[i]) && std::isfinite(within[i]) && std::isfinite(between[i]); };
    auto sd = [&](size_t i) { return std::sqrt(m2p[i] / (Kd - 1.0)); };
    auto mcse = [&](size_t i) { return std::sqrt(between[i] / C); };
    // (a constant latent, m2_pooled == 0: sd = 0 and no rhat, mcse, ess; one chain: likewise none of the three)
    auto spread = [&](size_t i) { return fin(i) && live.size() > 1 && m2p[i] != 0.0; };
    emit(out->mean, [&](size_t i) { return fin(i) ? mean[i] : nan; });
    emit(out->sd, [&](size_t i) { return fin(i) ? sd(i) : nan; });
    emit(out->mcse, [&](size_t i) { return spread(i) ? mcse(i) : nan; });
    emit(out->ess, [&](size_t i) {
        if (!spread(i)) return nan;
        const double s = sd(i), e = mcse(i);
        return std::min(s * s / (e * e), cap);
    });
    emit(out->rhat, [&](size_t i) {
        if (!spread(i)) return nan;
        const double varp = (nbar - 1.0) / nbar * within[i] + between[i];
        return std::sqrt(varp / within[i]);
    });
    emit(out->within, [&](size_t i) { return within[i]; });
    emit(out->between, [&](size_t i) { return between[i]; });
    return BB_OK;
}

extern "C" int bb_hmc_set_metric(bb_handle* h, const double* inv_mass) {
    if (!h) return bb_fail(BB_ERR_INVALID, "null argument");
    int rc = hmc_acc_checks(h, "bb_hmc_set_metric", false);
    if (rc) return rc;
    std::vector<double> metric;
    if ((rc = hmc_metric_rows(h, inv_mass, metric))) return rc;
    BB_ENTER(h);
    return h2d(const_cast<double*>(h->hmc.inv_mass), metric.data(), metric.size() * 8, h->stream);      // (isd lies behind inv_mass)
}

extern "C" int bb_hmc_get_metric(bb_handle* h, double* inv_mass) {
    if (!h || !inv_mass) return bb_fail(BB_ERR_INVALID, "null argument");
    int rc = hmc_acc_checks(h, "bb_hmc_get_metric", false);
    if (rc) return rc;
    BB_ENTER(h);
    return hmc_row_out(h, h->hmc.inv_mass, inv_mass);
}
