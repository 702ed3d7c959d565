// bb_nuts_host.h -- host side of the device-resident NUTS tree (bb_nuts_begin, bb_nuts_start, bb_nuts_leaf, bb_nuts_take; the kernels:
// bb_nuts.h, the evaluations: bb_logp.h through logp_launch of bb_analysis.h).  Included only by bb_engine.hip, once, behind
// bb_hmc_accum_host.h.
//
// The rows live in buf[BUF_NUTS], carved by bb_nuts_begin; the session's own buffer is not touched, so h->hmc's pointers hold.  Per leaf
// the host link carries one table up (W ops and W ints) and W (2 + 2 (max_depth + 1)) doubles down; a take carries the table up.
// The log-joints of the leaf, the subtree's candidate and the transition's candidate are mirrored on the host, as the session's are.

static_assert(sizeof(NutsOp) % 8 == 0, "the op table is carved in doubles");
static_assert(BB_NUTS_MAX_DEPTH == BB_NUTS_MAX_DEPTH_DEV && BB_NUTS_EDGE_OPP == BB_NUTS_EDGE_OPP_DEV, "bb_nuts.h restates the ABI's constants");

static int nuts_checks(bb_handle* h, const char* what, bool need_nuts) {
    int rc = hmc_common_checks(h, what);
    if (rc) return rc;
    if (!h->hmc_on) return bb_fail(BB_ERR_INVALID, "%s without a session: bb_hmc_begin comes first", what);
    if (need_nuts && !h->nuts_on) return bb_fail(BB_ERR_INVALID, "%s without the tree's rows: bb_nuts_begin comes first (bb_hmc_begin and bb_hmc_end drop them)", what);
    return BB_OK;
}

// the call's table: W ops, then W ints (1: the walker takes part) for the evaluation's idle mechanism
static int nuts_upload(bb_handle* h, const std::vector<NutsOp>& ops) {
    const size_t W = (size_t)h->hmc.W, Wp = (size_t)h->hmc.Wp, opd = W * sizeof(NutsOp) / 8;
    std::vector<double> stage(opd + Wp / 2, 0.0);
    std::vector<int> live(Wp, 0);
    for (size_t w = 0; w < W; ++w) live[w] = ops[w].dir != 0 ? 1 : 0;
    memcpy(stage.data(), ops.data(), W * sizeof(NutsOp));
    memcpy(stage.data() + opd, live.data(), Wp * sizeof(int));
    return h2d(const_cast<NutsOp*>(h->nuts.op), stage.data(), stage.size() * 8, h->stream);
}

extern "C" int bb_nuts_begin(bb_handle* h, const bb_nuts_opts* o) {
    if (!h || !o) return bb_fail(BB_ERR_INVALID, "null argument");
    int rc = nuts_checks(h, "bb_nuts_begin", false);
    if (rc) return rc;
    if (o->max_depth < 1 || o->max_depth > BB_NUTS_MAX_DEPTH) return bb_fail(BB_ERR_INVALID, "max_depth = %d is outside 1 .. %d", (int)o->max_depth, BB_NUTS_MAX_DEPTH);
    if (o->reserved0 != 0) return bb_fail(BB_ERR_INVALID, "bb_nuts_opts.reserved0 must be 0");
    BB_ENTER(h);
    h->nuts_on = h->nuts_started = false;      // (a begin that fails leaves no rows)
    const size_t W = (size_t)h->hmc.W, Wp = (size_t)h->hmc.Wp, Dz = (size_t)h->hmc.Dz, nchunk = (size_t)h->hmc.nchunk;
    NutsArgs N{};
    N.max_depth = o->max_depth;
    N.R = 10 + 2 * N.max_depth;
    N.NS = 1 + 2 * (N.max_depth + 1);
    NutsOp* op = nullptr;
    int* live = nullptr;
    size_t total = 0;
    rc = carve(h->buf[BUF_NUTS], [&](Carve& c) {      // (every length even: pairs stay 16-byte aligned)
        c(N.rows, W * (size_t)N.R * Dz);
        c(N.part, (W * nchunk * (size_t)N.NS + 1) & ~(size_t)1);
        c(N.out, (W * (size_t)(N.NS + 1) + 1) & ~(size_t)1);
        c(op, W * sizeof(NutsOp) / 8);
        c(live, Wp / 2);                               // (behind the ops: one copy brings both up)
        total = c.n;
    });
    if (rc) return rc;
    if ((rc = dzero(h->buf[BUF_NUTS].p, total * 8, h->stream))) return rc;
    if ((rc = dsync(h->stream))) return rc;
    N.op = op;
    h->nuts = N;
    h->nuts_lf = live;
    h->nuts_eps.assign(W, 0.0);
    h->nuts_live.assign(W, 0);
    h->nuts_on = true;
    return BB_OK;
}

extern "C" int bb_nuts_start(bb_handle* h, uint32_t transition, const double* eps, const int32_t* live, double* kinetic0) {
    if (!h || !eps || !live) return bb_fail(BB_ERR_INVALID, "null argument");
    int rc = nuts_checks(h, "bb_nuts_start", true);
    if (rc) return rc;
    HmcArgs H = h->hmc;
    const int W = H.W;
    bool any = false;
    for (int w = 0; w < W; ++w) {
        if (!live[w]) continue;
        if (!(std::isfinite(eps[w]) && eps[w] > 0.0)) return bb_fail(BB_ERR_INVALID, "walker %d: eps = %g is not finite and > 0", w, eps[w]);
        any = true;
    }
    BB_ENTER(h);
    h->nuts_started = false;
    std::vector<NutsOp> ops((size_t)W, NutsOp{});
    for (int w = 0; w < W; ++w) {
        ops[(size_t)w].dir = live[w] ? 1 : 0;
        ops[(size_t)w].store = -1;
        h->nuts_live[(size_t)w] = live[w] ? 1 : 0;
        h->nuts_eps[(size_t)w] = live[w] ? eps[w] : 0.0;
    }
    const size_t Wz = (size_t)W;
    h->nuts_moving.assign(Wz, 0); h->nuts_has_sub.assign(Wz, 0); h->nuts_has_cand.assign(Wz, 0);
    h->nuts_lp_leaf.assign(Wz, 0.0); h->nuts_lp_sub.assign(Wz, 0.0); h->nuts_lp_cand.assign(Wz, 0.0);
    if (kinetic0) std::fill(kinetic0, kinetic0 + W, 0.0);
    if (any) {
        if ((rc = nuts_upload(h, ops))) return rc;
        H.transition = transition;
        if ((rc = launch(h->stream, k_nuts_momentum, H.nchunk * W, BB_HMC_NT, BB_HMC_NT, H, h->nuts))) return rc;
        if ((rc = launch(h->stream, k_hmc_reduce, W, 64, 64, H, 0, -1))) return rc;
        std::vector<double> k0(Wz);
        if ((rc = d2h(k0.data(), H.scal, Wz * 8, h->stream))) return rc;
        if (kinetic0)
            for (int w = 0; w < W; ++w) if (live[w]) kinetic0[w] = k0[(size_t)w];
    }
    h->nuts_started = true;
    return BB_OK;
}

extern "C" int bb_nuts_leaf(bb_handle* h, const bb_nuts_leaf_opts* o, const bb_nuts_leaf_out* out) {
    if (!h || !o) return bb_fail(BB_ERR_INVALID, "null argument");
    int rc = nuts_checks(h, "bb_nuts_leaf", true);
    if (rc) return rc;
    if (!h->nuts_started) return bb_fail(BB_ERR_INVALID, "bb_nuts_leaf before bb_nuts_start (a bb_hmc_step redraws the travelling rows: a start comes after it)");
    if (o->reserved0 != 0) return bb_fail(BB_ERR_INVALID, "bb_nuts_leaf_opts.reserved0 must be 0");
    if (!o->dir || !o->first || !o->last || !o->store || !o->n_check || !o->check) return bb_fail(BB_ERR_INVALID, "null argument");
    const HmcArgs& H = h->hmc;
    const NutsArgs& N = h->nuts;
    const int W = H.W, md = N.max_depth, CS = BB_NUTS_MAX_DEPTH + 1;
    std::vector<NutsOp> ops((size_t)W, NutsOp{});
    int ncmax = 0;
    bool any = false;
    for (int w = 0; w < W; ++w) {
        NutsOp& p = ops[(size_t)w];
        p.store = -1;
        const int dir = o->dir[w];
        if (dir < -1 || dir > 1) return bb_fail(BB_ERR_INVALID, "walker %d: dir = %d is not -1, 0 or +1", w, dir);
        if (dir == 0) continue;
        if (!h->nuts_live[(size_t)w]) return bb_fail(BB_ERR_INVALID, "walker %d was not live in bb_nuts_start", w);
        if (!o->first[w] && !h->nuts_moving[(size_t)w]) return bb_fail(BB_ERR_INVALID, "walker %d: the first leaf after bb_nuts_start needs first = 1", w);
        if (o->store[w] < -1 || o->store[w] >= md) return bb_fail(BB_ERR_INVALID, "walker %d: store = %d is outside -1 .. %d", w, (int)o->store[w], md - 1);
        if (o->n_check[w] < 0 || o->n_check[w] > md + 1) return bb_fail(BB_ERR_INVALID, "walker %d: n_check = %d is outside 0 .. %d", w, (int)o->n_check[w], md + 1);
        for (int j = 0; j < o->n_check[w]; ++j) {
            const int c = o->check[w * CS + j];
            if (c != BB_NUTS_EDGE_OPP && (c < 0 || c >= md)) return bb_fail(BB_ERR_INVALID, "walker %d: check[%d] = %d is no slot 0 .. %d nor BB_NUTS_EDGE_OPP", w, j, c, md - 1);
            if (c >= 0 && c == o->store[w]) return bb_fail(BB_ERR_INVALID, "walker %d: slot %d is both stored and checked in one op", w, c);
            p.check[j] = c;
        }
        p.dir = dir; p.first = o->first[w] ? 1 : 0; p.last = o->last[w] ? 1 : 0;
        p.store = o->store[w]; p.n_check = o->n_check[w];
        p.eps = h->nuts_eps[(size_t)w];
        ncmax = std::max(ncmax, p.n_check);
        any = true;
    }
    const size_t NO = (size_t)N.NS + 1;
    std::vector<double> res((size_t)W * NO, 0.0);
    if (any) {
        BB_ENTER(h);
        if ((rc = nuts_upload(h, ops))) return rc;
        const int grid = H.nchunk * W;
        if ((rc = launch(h->stream, k_nuts_open, grid, BB_HMC_NT, 0, H, N))) return rc;
        LogpArgs B = h->hmc_eval;
        B.z = H.zp; B.grad = H.gp; B.logp = H.scal + 2 * (size_t)H.Wp;
        B.lf_n = h->nuts_lf; B.lf_k = 0;
        if ((rc = logp_launch(h, B))) return rc;
        if ((rc = launch(h->stream, k_nuts_close, grid, BB_HMC_NT, (size_t)(1 + 2 * ncmax) * BB_HMC_NT, H, N))) return rc;
        if ((rc = launch(h->stream, k_nuts_reduce, W, 64, 0, H, N))) return rc;
        if ((rc = d2h(res.data(), N.out, res.size() * 8, h->stream))) return rc;
    }
    for (int w = 0; w < W; ++w) {
        const NutsOp& p = ops[(size_t)w];
        const double* r = res.data() + (size_t)w * NO;
        if (p.dir != 0) {
            h->nuts_moving[(size_t)w] = 1;
            h->nuts_lp_leaf[(size_t)w] = r[1];
        }
        if (!out) continue;
        if (out->kinetic) out->kinetic[w] = p.dir ? r[0] : 0.0;
        if (out->logp_leaf) out->logp_leaf[w] = p.dir ? r[1] : 0.0;
        for (int j = 0; j < md + 1; ++j) {
            const bool on = p.dir != 0 && j < p.n_check;
            if (out->a) out->a[w * (md + 1) + j] = on ? r[2 + 2 * j] : 0.0;
            if (out->b) out->b[w * (md + 1) + j] = on ? r[3 + 2 * j] : 0.0;
        }
    }
    return BB_OK;
}

extern "C" int bb_nuts_take(bb_handle* h, const int32_t* flags) {
    if (!h || !flags) return bb_fail(BB_ERR_INVALID, "null argument");
    int rc = nuts_checks(h, "bb_nuts_take", true);
    if (rc) return rc;
    if (!h->nuts_started) return bb_fail(BB_ERR_INVALID, "bb_nuts_take before bb_nuts_start");
    const HmcArgs& H = h->hmc;
    const int W = H.W, all = BB_NUTS_TAKE_LEAF | BB_NUTS_TAKE_SUB | BB_NUTS_TAKE_STATE;
    std::vector<NutsOp> ops((size_t)W, NutsOp{});
    bool any = false;
    for (int w = 0; w < W; ++w) {
        const int f = flags[w];
        const size_t i = (size_t)w;
        if (f & ~all) return bb_fail(BB_ERR_INVALID, "walker %d: flags = %d holds bits that are no BB_NUTS_TAKE_*", w, f);
        if (!f) continue;
        if (!h->nuts_live[i]) return bb_fail(BB_ERR_INVALID, "walker %d was not live in bb_nuts_start", w);
        if ((f & BB_NUTS_TAKE_LEAF) && !h->nuts_moving[i]) return bb_fail(BB_ERR_INVALID, "walker %d: no leaf to take since bb_nuts_start", w);
        if ((f & BB_NUTS_TAKE_SUB) && !(f & BB_NUTS_TAKE_LEAF) && !h->nuts_has_sub[i]) return bb_fail(BB_ERR_INVALID, "walker %d: no subtree candidate to take since bb_nuts_start", w);
        if ((f & BB_NUTS_TAKE_STATE) && !(f & BB_NUTS_TAKE_SUB) && !h->nuts_has_cand[i]) return bb_fail(BB_ERR_INVALID, "walker %d: no transition candidate to take since bb_nuts_start", w);
        any = true;
    }
    if (!any) return BB_OK;
    // the mirrors of the log-joints, in the kernel's order
    std::vector<double> sub = h->nuts_lp_sub, cand = h->nuts_lp_cand, state = h->hmc_logp;
    for (int w = 0; w < W; ++w) {
        const int f = flags[w];
        const size_t i = (size_t)w;
        ops[i].store = -1;
        ops[i].flags = f;
        if (f & BB_NUTS_TAKE_LEAF) sub[i] = h->nuts_lp_leaf[i];
        if (f & BB_NUTS_TAKE_SUB) cand[i] = sub[i];
        if (f & BB_NUTS_TAKE_STATE) state[i] = cand[i];
        ops[i].logp = state[i];
    }
    BB_ENTER(h);
    if ((rc = nuts_upload(h, ops))) return rc;
    if ((rc = launch(h->stream, k_nuts_take, H.nchunk * W, BB_HMC_NT, 0, H, h->nuts))) return rc;
    if ((rc = dsync(h->stream))) return rc;
    for (int w = 0; w < W; ++w) {
        const size_t i = (size_t)w;
        if (flags[w] & BB_NUTS_TAKE_LEAF) h->nuts_has_sub[i] = 1;
        if (flags[w] & BB_NUTS_TAKE_SUB) h->nuts_has_cand[i] = 1;
    }
    h->nuts_lp_sub = sub; h->nuts_lp_cand = cand; h->hmc_logp = state;
    return BB_OK;
}
