// bb_step.h -- what one step of the two-kernel path launches, included once by bb_engine.hip (after the handle, before bb_plan.h: it needs
// nothing from the plan): the kernels' arguments and scratch, one launcher per kernel, the two exchanges, and step_sample, the ONE
// definition of a Monte-Carlo sample, which bb_run, the group's host-summed fallback, bb_elbo_grad and the split-phase entry points are
// built from (bb_run.h, bb_engine.hip).  Also the genotype model's theta gather and the step counter / optimiser restart.

// reduced: the update reads the K totals after a reduction (k_reduce follows k_sample) -- always on a sharded or genotype handle, and
// where the caller of the split-phase API hands the totals back reduced; otherwise it sums the tiles' partial rows itself
static RunArgs make_args(const bb_handle* h, long long step, int sample, int S, bool apply, bool with_elbo, bool reduced = false) {
    RunArgs A;
    memset(&A, 0, sizeof A);
    A.b_lo = h->b_lo;
    A.b_hi = h->b_hi;
    A.rank = h->o.rank;
    A.world = h->o.world_size;
    A.xepoch0 = h->epoch0;
    A.spin_limit = 1u << 23;                  // ~1 us per poll: seconds, not milliseconds
    A.row_l2 = h->tune.row_l2;
    A.nblk = h->nblk;
    A.nblk_alloc = h->tile_cap - 8;            // (the device adds the 8 back: BB_STAMP_WAVE)
    A.ng = 8;
    A.par = (int)(step & 1);
    A.sample = sample;
    A.S = S;
    A.first_sample = sample == 0;
    A.last_sample = sample == S - 1;
    A.apply = apply ? 1 : 0;
    A.with_elbo = with_elbo ? 1 : 0;
    A.count_globals = h->o.rank == 0;
    A.opt = h->o.optimizer;
    A.W = h->o.window;
    A.resum_every = h->o.resum_every;
    A.elbo_every = h->o.elbo_every;
    A.eta = h->o.eta;
    A.tau = h->o.tau;
    A.pre = h->o.pre;
    A.post = h->o.post;
    A.seed = h->o.seed;
    A.elbo_const = h->elbo_const;
    if (reduced || h->use_reduce()) { A.red = h->S.totals; A.nred = 1; }
    else { A.red = h->S.partials; A.nred = h->nblk; }
    return A;
}

// Per-sample scratch of the two-kernel step (z, eps sigmoid, sigmoid / softplus), the S > 1 / gradient-export accumulators and
// bb_elbo_grad's saved parameters: 7 arrays of D doubles, allocated on first use -- every entry point that can reach the
// two-kernel launchers calls this first (never from inside a stream capture); the resident launches use none of them.
static int ensure_scratch(bb_handle* h) {
    if (h->S.zsv) return BB_OK;
    // ONE slab carved into the seven arrays: a failed allocation leaves nothing behind (seven separate ones left the earlier arrays
    // in h->owned with stale pointers in S, and a retry allocated them all again -- ADVICE r03)
    const size_t D = (size_t)h->M.D, n = (D + 2 + 1) & ~(size_t)1;
    double* slab = nullptr;
    int rc = dalloc(h, &slab, 7 * n);
    if (rc) return rc;
    h->S.zsv = slab; h->S.asv = slab + n; h->S.hsv = slab + 2 * n; h->S.gacc_mu = slab + 3 * n; h->S.gacc_om = slab + 4 * n;
    h->bak_mu = slab + 5 * n; h->bak_om = slab + 6 * n;
    return h->dS ? h2d(h->dS, &h->S, sizeof(DevState), h->stream) : BB_OK;      // (kernels read the descriptor through its device copy)
}
static int need_scratch(const bb_handle* h) { return h->S.zsv ? 0 : bb_fail(BB_ERR_DEVICE, "internal: the two-kernel step's scratch arrays were not allocated (ensure_scratch)"); }

// the small kernels of the two-kernel step (k_sample / k_update: the instance of the model kind, descriptors through pointers)
template <class F>
static int launch_tiles(bb_handle* h, const RunArgs& A, F&& kernel_of) {
    int rc = need_scratch(h);
    if (!rc) by_kind(h->M.kind, [&](auto kindc) {
        rc = launch(h->stream, kernel_of(kindc), h->nblk, h->nthr, h->lds_doubles, desc_ptr(h->dM, &h->M), desc_ptr(h->dS, &h->S), A, h->NB);
    });
    return rc;
}
static int launch_sample(bb_handle* h, const RunArgs& A) { return launch_tiles(h, A, [](auto k) { return k_sample<decltype(k)::value>; }); }
static int launch_update(bb_handle* h, const RunArgs& A) { return launch_tiles(h, A, [](auto k) { return k_update<decltype(k)::value>; }); }
static int launch_reduce(bb_handle* h) { return launch(h->stream, k_reduce, 1, 256, (size_t)16 * h->M.K, h->M, h->S, h->nblk, h->ngeno_blk); }
static int launch_geno(bb_handle* h, const RunArgs& A, int do_update, int do_sample, int upd_par) {
    const int rc = need_scratch(h);
    return rc ? rc : launch(h->stream, k_geno, h->ngeno_blk, 256, 256 + 64, h->M, h->S, A, do_update, do_sample, upd_par);
}
static int launch_geno_sum(bb_handle* h) {
    const long long m_lo = std::max(h->b_lo, h->M.nn) - h->M.nn, m_hi = std::max(h->b_hi, h->M.nn) - h->M.nn;
    const int gsb = (int)std::min<long long>((h->M.G + 31) / 32, 1024);      // 32 genotypes per 256-thread block
    return launch(h->stream, k_geno_sum, gsb, 256, 256, h->M, h->S, m_lo, m_hi);
}

static int allreduce(bb_handle* h, double* buf, size_t n) {
    if (h->o.world_size == 1 && !h->tune.force_allreduce) return 0;
    return comm_allreduce(h->be, h->stream, buf, n, h->o.world_size);
}

// One MC sample: [k_geno sample] k_sample [k_reduce] | exchange K totals | k_update [k_geno_sum | exchange G sums | k_geno update]
// (bracketed: the genotype model, or when reducing).  exchange(hs, n, len, &DevState::buf) sums buf[0..len) over the n handles' problem:
// through the one handle's communicator (a no-op on an unsharded handle without BB_FORCE_ALLREDUCE) ...
static int comm_exchange(bb_handle* const* hs, int, size_t len, double* DevState::*buf) { return allreduce(hs[0], hs[0]->S.*buf, len); }
// ... or, handles of one process (the shards of a multi-device handle), on the host in shard order 0, 1, 2, ...
static int host_sum_exchange(bb_handle* const* hs, int n, size_t len, double* DevState::*buf) {
    std::vector<double> part(len), total(len, 0.0);
    int rc;
    for (int i = 0; i < n; ++i) {
        BB_ENTER(hs[i]);
        if ((rc = d2h(part.data(), hs[i]->S.*buf, len * 8, hs[i]->stream))) return rc;
        for (size_t k = 0; k < len; ++k) total[k] += part[k];
    }
    for (int i = 0; i < n; ++i) { BB_ENTER(hs[i]); if ((rc = h2d(hs[i]->S.*buf, total.data(), len * 8, hs[i]->stream))) return rc; }
    return 0;
}

// hs[i]'s device for its launches; the caller of a single handle has entered it already (a hipGetDevice per launch shows on the eager path)
#define BB_ENTER_ONE_OF(hs, n, i) DevGuard bb_dev_guard_((n) > 1 ? (hs)[i]->o.device : -1)
// first half of one MC sample on one handle: draw + moments (+ reduce to totals where the update reads them reduced: make_args)
static int sample_half(bb_handle* h, const RunArgs& A) {
    int rc;
    if (h->M.kind == BB_MODEL_GENOTYPE && (rc = launch_geno(h, A, 0, 1, 0))) return rc;
    if ((rc = launch_sample(h, A))) return rc;
    if (A.red == h->S.totals && (rc = launch_reduce(h))) return rc;
    return 0;
}
// second half, the K totals in place on every handle: gradient + update (+ the genotype block's exchange and update)
template <class X>
static int update_half(bb_handle* const* hs, int n, const RunArgs* As, X&& exchange) {
    const bool geno = hs[0]->M.kind == BB_MODEL_GENOTYPE;
    int rc;
    for (int i = 0; i < n; ++i) {
        BB_ENTER_ONE_OF(hs, n, i);
        if ((rc = launch_update(hs[i], As[i]))) return rc;
        if (geno && (rc = launch_geno_sum(hs[i]))) return rc;
    }
    if (!geno) return 0;
    if ((rc = exchange(hs, n, (size_t)hs[0]->M.G, &DevState::gsum))) return rc;
    for (int i = 0; i < n; ++i) { BB_ENTER_ONE_OF(hs, n, i); if ((rc = launch_geno(hs[i], As[i], 1, 0, As[i].par))) return rc; }
    return 0;
}
// one MC sample of the two-kernel step on n handles that form one problem (n = 1: the handle itself; n > 1: the shards of a group)
template <class X>
static int step_sample(bb_handle* const* hs, int n, const RunArgs* As, X&& exchange) {
    int rc;
    for (int i = 0; i < n; ++i) { BB_ENTER_ONE_OF(hs, n, i); if ((rc = sample_half(hs[i], As[i]))) return rc; }
    if ((rc = exchange(hs, n, (size_t)hs[0]->M.K, &DevState::totals))) return rc;
    return update_half(hs, n, As, exchange);
}
static int step_sample(bb_handle* h, const RunArgs& A) { return step_sample(&h, 1, &A, comm_exchange); }      // ... on the one handle

static bool elbo_wanted(const bb_handle* h, long long step) { return h->o.elbo_every > 0 && step % h->o.elbo_every == 0; }

// one whole step: its S samples
static int enqueue_step(bb_handle* h, long long step) {
    const int S = h->o.samples_per_step;
    int rc;
    for (int s = 0; s < S; ++s)
        if ((rc = step_sample(h, make_args(h, step, s, S, true, elbo_wanted(h, step))))) return rc;
    return 0;
}

// Genotype model with the shards cut at genotype boundaries: a resident run updates theta_g on its owner only.  Gathering the
// owners' copies (parameters, optimiser accumulators, window rows) = summing rows that hold zeros for what a shard does not own.
static size_t theta_rows(const bb_handle* h) { return 6 + (h->o.optimizer == BB_OPT_TRUNCATED_ADAGRAD ? 2 * (size_t)h->o.window : 0); }
static bool theta_partial(const bb_handle* h) { return h->M.kind == BB_MODEL_GENOTYPE && (h->g_lo > 0 || h->g_hi < h->M.G); }
static int theta_pack(bb_handle* h, int unpack) {
    const size_t n = theta_rows(h) * (size_t)h->M.G;
    int rc;
    if (!h->theta_buf && (rc = dalloc(h, &h->theta_buf, n))) return rc;
    const int W = h->o.optimizer == BB_OPT_TRUNCATED_ADAGRAD ? h->o.window : 0;
    const int nb = (int)std::min<size_t>((n + 255) / 256, 512);
    return launch(h->stream, k_theta_pack, nb, 256, 0, h->M, h->S, h->theta_buf, h->g_lo, h->g_hi, W, unpack);
}
// ranks of a multi-process run: through the RCCL communicator (collective: every rank is here after the same bb_run)
static int theta_sync_comm(bb_handle* h) {
    int rc;
    if ((rc = theta_pack(h, 0))) return rc;
    if ((rc = allreduce(h, h->theta_buf, theta_rows(h) * (size_t)h->M.G))) return rc;
    if ((rc = theta_pack(h, 1))) return rc;
    h->theta_stale = false;
    return dsync(h->stream);
}
// handles of one process (the shards of a multi-device handle; the emulation's ranks): summed on the host
static int theta_sync_local(bb_handle* const* hs, int n) {
    if (n < 2 || !theta_partial(hs[0])) return 0;
    const size_t len = theta_rows(hs[0]) * (size_t)hs[0]->M.G;
    std::vector<double> part(len), total(len, 0.0);
    int rc;
    for (int i = 0; i < n; ++i) {
        BB_ENTER(hs[i]);
        if ((rc = theta_pack(hs[i], 0)) || (rc = d2h(part.data(), hs[i]->theta_buf, len * 8, hs[i]->stream))) return rc;
        for (size_t k = 0; k < len; ++k) total[k] += part[k];
    }
    for (int i = 0; i < n; ++i) {
        BB_ENTER(hs[i]);
        if ((rc = h2d(hs[i]->theta_buf, total.data(), len * 8, hs[i]->stream)) || (rc = theta_pack(hs[i], 1)) || (rc = dsync(hs[i]->stream))) return rc;
        hs[i]->theta_stale = false;
    }
    return 0;
}

static int set_step(bb_handle* h, long long step) {
    unsigned long long c[2] = {(unsigned long long)step, (unsigned long long)step};
    h->step = step;
    h->sample = 0;
    return h2d(h->S.ctr, c, sizeof c, h->stream);
}

static int reset_optimizer(bb_handle* h) {
    const size_t D = (size_t)h->M.D;
    int rc;
    if ((rc = dzero(h->S.accl, (2 * D + 8) * 4, h->stream))) return rc;
    if (h->o.optimizer == BB_OPT_TRUNCATED_ADAGRAD) {
        if ((rc = dzero(h->S.hist, (size_t)h->o.window * 2 * (size_t)h->M.Dh * 8, h->stream))) return rc;
        if ((rc = dzero(h->S.acc_mu, D * 8, h->stream))) return rc;
        if ((rc = dzero(h->S.acc_om, D * 8, h->stream))) return rc;
    } else {
        std::vector<double> a(D, 1e-8);   // AdvancedVI: acc = fill(1e-8, size(x))
        if ((rc = h2d(h->S.acc_mu, a.data(), D * 8, h->stream))) return rc;
        if ((rc = h2d(h->S.acc_om, a.data(), D * 8, h->stream))) return rc;
    }
    std::vector<double> nanv(BB_ELBO_RING, NAN);
    if ((rc = h2d(h->S.elbo_ring, nanv.data(), nanv.size() * 8, h->stream))) return rc;
    // ready / inbox words never repeat, also across restarts: the base moves by the steps ASKED of the resident launch since
    // the last restart -- the same number on every rank of a sharded run, wherever a timeout may have stopped each of them
    h->epoch0 += (unsigned)h->req_steps + 1u;
    h->req_steps = 0;
    return set_step(h, 0);
}
