// bb_create.h -- handle creation, included once by bb_engine.hip: check_request refuses what needs no device to refuse, create_inner
// builds one handle in named stages under an owner that releases a half-built one on every early return, CallerOrder regroups a
// scattered genotype model and presents the caller's order, bb_create ties them together.
#include <memory>

extern "C" void bb_default_opts(bb_advi_opts* o) {
    memset(o, 0, sizeof *o);
    o->samples_per_step = 1;
    o->optimizer = BB_OPT_TRUNCATED_ADAGRAD;
    o->eta = 0.1;
    o->tau = 40.0;
    o->window = 100;
    o->resum_every = 0;
    o->pre = 1.0;
    o->post = 0.9;
    o->seed = 0;
    o->device = 0;
    o->rank = 0;
    o->world_size = 1;
    o->steps_per_graph = 0;
    o->elbo_every = 0;
    o->n_devices = 1;
    o->device_ids = nullptr;
}

// a handle under construction: bb_destroy releases whatever it holds so far; release() into *out on success
struct HandleDeleter { void operator()(bb_handle* h) const { bb_destroy(h); } };
typedef std::unique_ptr<bb_handle, HandleDeleter> HandleOwner;

// a zeroed device array of the handle's filled from `src`
template <class T, class F>
static int upload(bb_handle* h, F** field, const T* src, size_t n) {
    T* d = nullptr;
    int rc;
    if ((rc = dalloc(h, &d, n)) || (rc = h2d(d, src, n * sizeof(T), h->stream))) return rc;
    *field = d;
    return 0;
}

static void add_block(bb_handle* h, const char* name, int kind, long long n, long long* off) {
    bb_block_range b;
    memset(&b, 0, sizeof b);
    snprintf(b.name, sizeof b.name, "%s", name);
    b.lo = *off;
    b.hi = *off + n;
    h->blocks.push_back(b);
    h->M.blk_lo[kind] = b.lo;
    h->M.blk_hi[kind] = b.hi;
    *off += n;
}

// every mean finite, every std finite and > 0; the message names the prior and, Matrix form, the element in the CALLER's order
static int check_prior(const bb_prior* p, const char* name) {
    if (!p || !p->mean || !p->std || p->n == 0) return 0;
    if (p->n == 1) {
        if (!(p->std[0] > 0) || !std::isfinite(p->std[0])) return bb_fail(BB_ERR_INVALID, "%s: std must be > 0 and finite", name);
        if (!std::isfinite(p->mean[0])) return bb_fail(BB_ERR_INVALID, "%s: mean must be finite", name);
        return 0;
    }
    for (long long i = 0; i < (long long)p->n; ++i) {
        if (!(p->std[i] > 0) || !std::isfinite(p->std[i])) return bb_fail(BB_ERR_INVALID, "%s: std[%lld] must be > 0 and finite", name, i);
        if (!std::isfinite(p->mean[i])) return bb_fail(BB_ERR_INVALID, "%s: mean[%lld] must be finite", name, i);
    }
    return 0;
}

static int upload_prior(bb_handle* h, int kind, const bb_prior* p, double dmean, double dstd, const char* name,
                        bool vector_only, double* sum_log_std) {
    const long long n = h->M.blk_hi[kind] - h->M.blk_lo[kind];
    DevPrior& dp = h->M.pri[kind];
    dp.mean_e = nullptr;
    dp.inv_var_e = nullptr;
    if (!p || !p->mean || !p->std || p->n == 0) {
        dp.mean = dmean;
        dp.inv_var = 1.0 / (dstd * dstd);
        *sum_log_std += (double)n * log(dstd);
        return 0;
    }
    if (p->n == 1) {
        if (int rc = check_prior(p, name)) return rc;
        dp.mean = p->mean[0];
        dp.inv_var = 1.0 / (p->std[0] * p->std[0]);
        *sum_log_std += (double)n * log(p->std[0]);
        return 0;
    }
    if (vector_only) return bb_fail(BB_ERR_INVALID, "%s accepts only the Vector form [mean, std]", name);
    if (p->n != n) return bb_fail(BB_ERR_INVALID, "%s: Matrix form needs %lld rows, got %lld", name, n, (long long)p->n);
    if (int rc = check_prior(p, name)) return rc;
    std::vector<double> iv((size_t)n);
    for (long long i = 0; i < n; ++i) {
        iv[(size_t)i] = 1.0 / (p->std[i] * p->std[i]);
        *sum_log_std += log(p->std[i]);
    }
    int rc;
    if ((rc = upload(h, &dp.mean_e, p->mean, (size_t)n)) || (rc = upload(h, &dp.inv_var_e, iv.data(), (size_t)n))) return rc;
    dp.mean = 0;
    dp.inv_var = 0;
    return 0;
}

// what bb_create hands create_inner (and a multi-device handle's shards): the switches, and whether to lay the loglambda block out in
// FRONT of the per-genotype / per-mutant blocks (the handle's internal order; the caller's stays the reference's source order)
struct CreateCtx { BBTuning tune; bool loglambda_first; };
static int group_create(const bb_model_desc* md, const bb_advi_opts* opts, const CreateCtx& cx, bb_handle** out);

// The per-mutant blocks of a model kind, in flat order: what a barcode shard owns a cut of besides its loglambda.  Mutants [m, m') of
// block `blk`, replicate r, are the latents blk_lo[blk] + (r * nb + [m, m')) * E; per_rep: one such range per replicate, else r = 0 only.
// (The genotype model's theta is per genotype, not per mutant: hist_rows and owned_ranges place it themselves.)
struct ShardBlock { int blk; bool per_rep; };
static std::vector<ShardBlock> shard_blocks(const DevModel& M) {
    if (M.kind == BB_MODEL_FITNESS || M.kind == BB_MODEL_MULTIENV) return {{BK_S, false}, {BK_LS, false}};
    if (M.kind == BB_MODEL_GENOTYPE) return {{BK_TT, false}, {BK_LT, false}, {BK_LS, false}};
    return {{BK_S, false}, {BK_TT, true}, {BK_LT, true}, {BK_LS, true}};
}

// Rows of the TruncatedADAGrad window on a SHARDED handle (DevModel.Dh): the window is 2 x window doubles per latent -- a hundred
// times everything else a handle holds -- and a shard only ever updates its own barcodes' latents, the replicated blocks and (genotype
// model) the genotype block: one contiguous range of the flat vector per (block, replicate), the ranges every tile's segment table
// is cut from (bb_build_segs / br_build_segs).  A row packs those ranges one after the other; a segment carries the difference
// between a latent's flat index and its entry (bb_hdelta), so the kernels pay one subtraction per pair.  Differences are even: pairs
// stay whole and 16-byte aligned.  BB_NO_HIST_PACK=1 keeps full rows.
static void hist_rows(bb_handle* h) {
    DevModel& M = h->M;
    M.Dh = M.Dp;
    for (int k = 0; k < BK_COUNT; ++k) M.hd0[k] = M.hd1[k] = 0;
    for (int r = 0; r < BB_MAX_REP; ++r) M.hdl[r] = 0;
    if (h->o.world_size <= 1 || h->tune.no_hist_pack || M.Dp >= (1ll << 31)) return;      // (a segment keeps its difference in an int)
    const long long b0 = h->b_lo, nbt = h->b_hi - h->b_lo;
    const long long m0 = std::max(h->b_lo, M.nn) - M.nn, nmt = (std::max(h->b_hi, M.nn) - M.nn) - m0;
    long long c = 0;          // next free entry of the row
    // one range [a, a + len): starts on an entry of a's parity; two entries of slack (an edge pair's other half is read, never used)
    auto place = [&](long long a, long long len) { const long long at = c + ((a - c) & 1); c = at + len + 2; return a - at; };
    // R ranges of one block, `stride` apart in the flat vector, `len` long: packed `lp` apart with lp of the stride's parity
    auto place_r = [&](int blk, long long a0, long long stride, long long len, int R) {
        const long long lp = len + 2 + ((stride - (len + 2)) & 1);
        const long long at = c + ((a0 - c) & 1);
        M.hd0[blk] = a0 - at;
        M.hd1[blk] = stride - lp;
        c = at + (long long)R * lp;
    };
    M.hd0[BK_SPOP] = place(M.blk_lo[BK_SPOP], M.blk_hi[BK_SPOP] - M.blk_lo[BK_SPOP]);
    M.hd0[BK_LSPOP] = place(M.blk_lo[BK_LSPOP], M.blk_hi[BK_LSPOP] - M.blk_lo[BK_LSPOP]);
    if (M.kind == BB_MODEL_GENOTYPE) M.hd0[BK_S] = place(M.blk_lo[BK_S], M.G);      // (every rank updates every theta_g on the all-reduce step; the resident launch only its own)
    for (const ShardBlock& sb : shard_blocks(M)) {
        if (sb.per_rep) place_r(sb.blk, M.blk_lo[sb.blk] + m0 * M.E, M.nb * M.E, nmt * M.E, M.R);
        else M.hd0[sb.blk] = place(M.blk_lo[sb.blk] + m0 * M.E, nmt * M.E);
    }
    for (int r = 0; r < M.R; ++r) M.hdl[r] = place(M.off_l[r] + b0 * M.T[r], nbt * M.T[r]);
    const long long Dh = (c + 7) & ~7ll;
    if (Dh >= M.Dp) {          // nothing gained (a shard that owns almost everything): full rows, no differences
        for (int k = 0; k < BK_COUNT; ++k) M.hd0[k] = M.hd1[k] = 0;
        for (int r = 0; r < BB_MAX_REP; ++r) M.hdl[r] = 0;
        return;
    }
    M.Dh = Dh;
}

// the ranges of the flat vector (the handle's order) a shard owns: its barcodes' latents and (genotype model) theta of its own genotypes
static void owned_ranges(const bb_handle* sh, std::vector<std::pair<long long, long long>>& out) {
    const DevModel& M = sh->M;
    const long long b_lo = sh->b_lo, b_hi = sh->b_hi;
    const long long m_lo = std::max(b_lo, M.nn) - M.nn, m_hi = std::max(b_hi, M.nn) - M.nn;
    for (int r = 0; r < M.R; ++r) out.push_back({M.off_l[r] + b_lo * M.T[r], M.off_l[r] + b_hi * M.T[r]});
    // theta of its own genotypes (sharded by genotype where the cuts allow, else all shards hold all of it)
    if (M.kind == BB_MODEL_GENOTYPE && sh->g_hi > sh->g_lo) out.push_back({M.blk_lo[BK_S] + sh->g_lo, M.blk_lo[BK_S] + sh->g_hi});
    if (m_hi <= m_lo) return;
    const std::vector<ShardBlock> blocks = shard_blocks(M);
    auto cut = [&](int blk, int r) { out.push_back({M.blk_lo[blk] + (r * M.nb + m_lo) * M.E, M.blk_lo[blk] + (r * M.nb + m_hi) * M.E}); };
    for (const ShardBlock& sb : blocks) if (!sb.per_rep) cut(sb.blk, 0);
    for (int r = 0; r < M.R; ++r)
        for (const ShardBlock& sb : blocks) if (sb.per_rep) cut(sb.blk, r);
}

// ---- the stages of create_inner; first every check that needs neither a device nor the layout -------------------------------
static int check_request(const bb_model_desc* md, const bb_advi_opts* opts) {
    if (md->kind < 0 || md->kind > 4) return bb_fail(BB_ERR_INVALID, "unknown model kind %d", md->kind);
    if (md->n_rep < 1 || md->n_rep > BB_MAX_REP) return bb_fail(BB_ERR_INVALID, "n_rep must be in 1..%d", BB_MAX_REP);
    if (md->kind != BB_MODEL_REPLICATE && md->kind != BB_MODEL_MULTIENV_REPLICATE && md->n_rep != 1)
        return bb_fail(BB_ERR_INVALID, "only the replicate models take n_rep > 1");
    if (md->n_neutral < 1 || md->n_bc < 1) return bb_fail(BB_ERR_INVALID, "need at least one neutral and one mutant barcode");
    if (!md->n_time || !md->counts || !md->totals) return bb_fail(BB_ERR_INVALID, "n_time/counts/totals missing");
    if (opts->samples_per_step < 1) return bb_fail(BB_ERR_INVALID, "samples_per_step must be >= 1");
    if (opts->optimizer != BB_OPT_TRUNCATED_ADAGRAD && opts->optimizer != BB_OPT_DECAYED_ADAGRAD)
        return bb_fail(BB_ERR_INVALID, "unknown optimizer %d", opts->optimizer);
    if (opts->optimizer == BB_OPT_TRUNCATED_ADAGRAD && opts->window < 1) return bb_fail(BB_ERR_INVALID, "window must be >= 1");
    // the optimiser constants go to the kernels as they are (DevState.optc): any sign (eta = 0 freezes a run), but finite
    if (!std::isfinite(opts->eta)) return bb_fail(BB_ERR_INVALID, "eta must be finite");
    if (!std::isfinite(opts->tau)) return bb_fail(BB_ERR_INVALID, "tau must be finite");
    if (!std::isfinite(opts->pre)) return bb_fail(BB_ERR_INVALID, "pre must be finite");
    if (!std::isfinite(opts->post)) return bb_fail(BB_ERR_INVALID, "post must be finite");
    if (opts->world_size < 1 || opts->rank < 0 || opts->rank >= opts->world_size)
        return bb_fail(BB_ERR_INVALID, "bad rank/world_size %d/%d", opts->rank, opts->world_size);
    if (opts->n_devices > 1) {          // a multi-device handle (group_create)
        if (opts->n_devices > BB_MAX_WORLD) return bb_fail(BB_ERR_UNSUPPORTED, "at most %d devices per handle", BB_MAX_WORLD);
        if (opts->world_size != 1 || opts->rank != 0) return bb_fail(BB_ERR_INVALID, "n_devices > 1 needs rank 0 / world_size 1 (the handle shards by itself)");
    }
    int Ttot = 0;
    for (int r = 0; r < md->n_rep; ++r) {
        const int T = md->n_time[r];
        if (T < 2 || T > 255) return bb_fail(BB_ERR_INVALID, "n_time[%d] = %d outside 2..255", r, T);
        Ttot += T;
    }
    if (md->kind == BB_MODEL_MULTIENV || md->kind == BB_MODEL_MULTIENV_REPLICATE) {
        if (md->n_env < 1 || !md->env_idx) return bb_fail(BB_ERR_INVALID, "multienv models need n_env >= 1 and env_idx");
        for (int t = 0; t < Ttot; ++t)
            if (md->env_idx[t] < 0 || md->env_idx[t] >= md->n_env) return bb_fail(BB_ERR_INVALID, "env_idx[%d] out of range", t);
    }
    if (md->kind == BB_MODEL_GENOTYPE) {
        if (md->n_geno < 1 || !md->geno_idx) return bb_fail(BB_ERR_INVALID, "genotype model needs n_geno >= 1 and geno_idx");
        for (long long m = 0; m < md->n_bc; ++m)
            if (md->geno_idx[m] < 0 || md->geno_idx[m] >= md->n_geno) return bb_fail(BB_ERR_INVALID, "geno_idx[%lld] out of range", m);
    }
    return 0;
}

// the DevModel scalars, the per-replicate offsets and division magics, K
static void set_shapes(bb_handle* h, const bb_model_desc* md) {
    DevModel& M = h->M;
    M.kind = md->kind;
    M.R = md->n_rep;
    M.E = (md->kind == BB_MODEL_MULTIENV || md->kind == BB_MODEL_MULTIENV_REPLICATE) ? md->n_env : 1;
    M.G = md->kind == BB_MODEL_GENOTYPE ? md->n_geno : 0;
    M.nn = md->n_neutral;
    M.nb = md->n_bc;
    M.B = M.nn + M.nb;
    M.quirk = (md->kind == BB_MODEL_REPLICATE && (md->flags & BB_FLAG_RAGGED_METHOD)) ? 1 : 0;
    M.Ttot = 0; M.nt1 = 0; M.K = 0;
    for (int r = 0; r < M.R; ++r) {
        const int T = md->n_time[r];
        M.T[r] = T;
        M.Tmagic[r] = (unsigned)(0x100000000ull / (unsigned)T) + 1u;
        M.Tmagic1[r] = T > 2 ? (unsigned)(0x100000000ull / (unsigned)(T - 1)) + 1u : 0u;   // T - 1 == 1: no division
        M.off_t[r] = M.nt1;
        M.cnt_off[r] = (long long)M.Ttot * M.B;
        M.kq[r] = M.K;
        M.kqa[r] = M.K + T + 5 * (T - 1);
        M.tcum[r] = M.Ttot;
        M.Ttot += T;
        M.nt1 += T - 1;
        M.K += 6 * T - 5 + (M.quirk ? 2 * (T - 1) * (T - 1) : 0);
    }
    M.K += 2;
}

static long long n_cells(const DevModel& M) { return (long long)M.Ttot * M.B; }          // counts, and loglambda latents, of the whole problem

// flat layout, source order (model_*.jl `~` statements)
static void lay_out(bb_handle* h, const CreateCtx& cx) {
    DevModel& M = h->M;
    long long off = 0;
    for (int k = 0; k < BK_COUNT; ++k) M.blk_lo[k] = M.blk_hi[k] = 0;
    add_block(h, "s_pop", BK_SPOP, M.nt1, &off);
    add_block(h, "logsigma_pop", BK_LSPOP, M.nt1, &off);
    if (M.kind == BB_MODEL_FITNESS || M.kind == BB_MODEL_MULTIENV) {
        add_block(h, "s_bc", BK_S, M.nb * M.E, &off);
        add_block(h, "logsigma_bc", BK_LS, M.nb * M.E, &off);
    } else {
        const long long E_ = M.kind == BB_MODEL_MULTIENV_REPLICATE ? M.E : 1;
        if (cx.loglambda_first) add_block(h, "loglambda", BK_L, n_cells(M), &off);          // (internal order only: bb_create)
        add_block(h, "theta", BK_S, M.kind == BB_MODEL_GENOTYPE ? M.G : M.nb * E_, &off);
        add_block(h, "theta_tilde", BK_TT, M.nb * M.R * E_, &off);
        add_block(h, "logtau", BK_LT, M.nb * M.R * E_, &off);
        add_block(h, "logsigma_bc", BK_LS, M.nb * M.R * E_, &off);
    }
    if (!(cx.loglambda_first && M.kind >= BB_MODEL_GENOTYPE)) add_block(h, "loglambda", BK_L, n_cells(M), &off);
    M.D = off;
    M.Dp = (off + 7) & ~7ll;
    for (int r = 0, o = 0; r < M.R; ++r) { M.off_l[r] = M.blk_lo[BK_L] + (long long)o * M.B; o += M.T[r]; }
}

// counts: validate totals == row sums (Multinomial support, Distributions.jl), to uint32; *sum_lgamma: the ELBO constant's lgamma terms
static int load_counts(bb_handle* h, const bb_model_desc* md, double* sum_lgamma) {
    DevModel& M = h->M;
    std::vector<unsigned> c32((size_t)n_cells(M));
    *sum_lgamma = 0.0;
    long long co = 0, to = 0;
    for (int r = 0; r < M.R; ++r) {
        const int T = M.T[r];
        for (int t = 0; t < T; ++t) {
            long long s = 0;
            for (long long b = 0; b < M.B; ++b) {
                const int64_t v = md->counts[co + b * T + t];
                if (v < 0 || v > 0xFFFFFFFFll) return bb_fail(BB_ERR_INVALID, "count out of range at rep %d t %d barcode %lld", r, t, b);
                c32[(size_t)(co + b * T + t)] = (unsigned)v;
                s += v;
                *sum_lgamma += lgamma((double)v + 1.0);
            }
            if (s != md->totals[to + t])
                return bb_fail(BB_ERR_INVALID, "totals[rep %d, t %d] = %lld but the counts sum to %lld (the reference's Multinomial term is -Inf there)",
                               r, t, (long long)md->totals[to + t], s);
        }
        co += (long long)T * M.B;
        to += T;
    }
    return upload(h, &M.counts, c32.data(), c32.size());
}

// the moment pivot (DevModel::piv): a function of the whole problem's counts, the same on every shard
static int load_pivot(bb_handle* h, const bb_model_desc* md) {
    DevModel& M = h->M;
    std::vector<double> piv((size_t)M.Ttot, 0.0);
    long long co = 0;
    for (int r = 0; r < M.R; ++r) {
        const int T = M.T[r];
        const long long nb_ = M.nn > 0 ? M.nn : M.B;        // (no neutrals: all barcodes)
        for (int t = 0; t + 1 < T; ++t) {
            double s = 0.0;
            for (long long b = 0; b < nb_; ++b)
                s += log((double)md->counts[co + b * T + t + 1] + 0.5) - log((double)md->counts[co + b * T + t] + 0.5);
            piv[(size_t)(M.tcum[r] + t)] = s / (double)nb_;
        }
        co += (long long)T * M.B;
    }
    return upload(h, &M.piv, piv.data(), piv.size());
}

// env_idx; geno_idx and the genotype CSR (geno_ptr / geno_mem: the mutants of every genotype), geno_sorted, the host's geno_ptr_h
static int load_indices(bb_handle* h, const bb_model_desc* md) {
    DevModel& M = h->M;
    int rc;
    if ((M.kind == BB_MODEL_MULTIENV || M.kind == BB_MODEL_MULTIENV_REPLICATE) && (rc = upload(h, &M.env_idx, md->env_idx, (size_t)M.Ttot))) return rc;
    if (M.kind != BB_MODEL_GENOTYPE) return 0;
    if ((rc = upload(h, &M.geno_idx, md->geno_idx, (size_t)M.nb))) return rc;
    std::vector<int> ptr((size_t)M.G + 1, 0), mem((size_t)M.nb);
    for (long long m = 0; m < M.nb; ++m) ptr[(size_t)md->geno_idx[m] + 1]++;
    for (int g = 0; g < M.G; ++g) ptr[(size_t)g + 1] += ptr[(size_t)g];
    std::vector<int> fill(ptr.begin(), ptr.end() - 1);
    for (long long m = 0; m < M.nb; ++m) mem[(size_t)fill[(size_t)md->geno_idx[m]]++] = (int)m;
    if ((rc = upload(h, &M.geno_ptr, ptr.data(), ptr.size())) || (rc = upload(h, &M.geno_mem, mem.data(), mem.size()))) return rc;
    M.geno_sorted = std::is_sorted(md->geno_idx, md->geno_idx + M.nb) ? 1 : 0;
    h->geno_ptr_h = ptr;
    return 0;
}

// priors (defaults: model_fitness_normal.jl:125-129, ..._genotypes.jl:162); *sum_log_std: the ELBO constant's prior normalisers
static int load_priors(bb_handle* h, const bb_model_desc* md, double* sum_log_std) {
    int rc;
    *sum_log_std = 0.0;
    if ((rc = upload_prior(h, BK_SPOP, &md->s_pop_prior, 0.0, 2.0, "s_pop_prior", false, sum_log_std))) return rc;
    if ((rc = upload_prior(h, BK_LSPOP, &md->logsigma_pop_prior, 0.0, 1.0, "logsigma_pop_prior", false, sum_log_std))) return rc;
    if ((rc = upload_prior(h, BK_S, &md->s_bc_prior, 0.0, 2.0, "s_bc_prior", false, sum_log_std))) return rc;
    if ((rc = upload_prior(h, BK_LS, &md->logsigma_bc_prior, 0.0, 1.0, "logsigma_bc_prior", false, sum_log_std))) return rc;
    if ((rc = upload_prior(h, BK_L, &md->loglambda_prior, 3.0, 3.0, "loglambda_prior", false, sum_log_std))) return rc;
    if (h->M.kind < BB_MODEL_GENOTYPE) return 0;
    if ((rc = upload_prior(h, BK_TT, nullptr, 0.0, 1.0, "theta_tilde", true, sum_log_std))) return rc;
    return upload_prior(h, BK_LT, &md->logtau_prior, -2.0, 1.0, "logtau_prior", true, sum_log_std);
}

// the barcode shard of this rank, and (genotype model) the genotypes whose theta it owns
static void cut_shard(bb_handle* h, const bb_model_desc* md) {
    const DevModel& M = h->M;
    h->b_lo = M.B * h->o.rank / h->o.world_size;
    h->b_hi = M.B * (h->o.rank + 1) / h->o.world_size;
    h->g_lo = 0;
    h->g_hi = M.G;
    if (M.kind == BB_MODEL_GENOTYPE && M.geno_sorted && h->o.world_size > 1) {
        // Genotypes in consecutive runs: cut the shards at genotype boundaries, so that every rank holds ALL mutants of the
        // genotypes it owns -- d/dtheta_g is then a rank-local sum.  The cut moves back to the first mutant
        // of the genotype it fell into; genotypes without mutants go with the one before.
        auto snap = [&](long long b, int* g) {
            if (b <= 0) { *g = 0; return (long long)0; }
            if (b >= M.B) { *g = M.G; return M.B; }
            if (b <= M.nn) { *g = 0; return b; }
            const int gg = md->geno_idx[b - M.nn];
            *g = gg;
            return M.nn + (long long)h->geno_ptr_h[(size_t)gg];
        };
        h->b_lo = snap(h->b_lo, &h->g_lo);
        h->b_hi = snap(h->b_hi, &h->g_hi);
        if (h->b_lo <= M.nn) h->g_lo = 0;          // (genotype ranges tile [0, G): whoever owns the first mutant also owns the empty ones before it)
    }
}

// the launch geometry: barcodes per tile, threads per workgroup, the LDS the block programs need
static int pick_geometry(bb_handle* h) {
    const DevModel& M = h->M;
    // One workgroup per CU (XCD-agnostic: every tile is independent), sized so that the whole
    // shard is resident at once: NB = ceil(barcodes / CUs) barcodes per tile, up to 1024 threads
    // (16 waves per CU) working a tile's ~NB*(T+2) latents.  BB_TUNE_* env vars override for experiments.
    int maxT = 0;
    for (int r = 0; r < M.R; ++r) maxT = std::max(maxT, M.T[r]);
    h->cus = dev_cus(h->o.device, h->cus);
    const long long nbar = std::max<long long>(h->b_hi - h->b_lo, 1);
    int NB = (int)std::max<long long>((nbar + h->cus - 1) / h->cus, 32);
    if (h->tune.nb > 0) NB = h->tune.nb;
    const size_t lds_cap = (size_t)160 * 1024;
    int nthr = 0;
    for (;;) {
        // one pair of latents per thread is the sweet spot; counted with the segments' rounding (tile_pairs_bound), the
        // number the resident launch sizes its per-thread state by (a tile of 257 pairs on 256 threads would need two)
        const long long pairs = tile_pairs_bound(M, NB);
        // > 1 pair per thread: 512 threads (256-VGPR budget, up to 4 pairs) beat 1024 threads with spills (C3: 28.8k vs 18.8k steps/s)
        // (768 threads x 2 pairs was tried for C3: 138 spills at 168 VGPRs, 23.0k vs 28.8k steps/s for 512 x 3)
        nthr = pairs > 2048 ? 1024 : (pairs > 1024 ? 512 : (pairs > 512 ? 1024 : (pairs > 256 ? 512 : 256)));
        if (h->tune.nthr) nthr = h->tune.nthr;
        while (nthr < maxT) nthr <<= 1;
        const size_t need = (size_t)bb_lds_layout(M.R, M.E, M.kind, M.Ttot, M.nt1, M.K, NB, nthr).total * 8;
        if ((need <= lds_cap && (long long)NB * maxT < 65536) || NB <= 8) break;
        NB = (NB + 1) / 2;
    }
    const size_t need = (size_t)bb_lds_layout(M.R, M.E, M.kind, M.Ttot, M.nt1, M.K, NB, nthr).total * 8;
    if (need > 160 * 1024 || nthr > 1024 || (long long)NB * maxT >= 65536)
        return bb_fail(BB_ERR_UNSUPPORTED, "a tile of %d barcodes needs %zu bytes of LDS / %d threads (n_time or n_rep too large for this build)", NB, need, nthr);
    h->NB = NB;
    h->nthr = nthr;
    h->lds_doubles = need / 8;
    h->lds_doubles_p0 = (size_t)bb_lds_layout(M.R, M.E, M.kind, M.Ttot, M.nt1, M.K, NB, nthr, 1).total;
    h->nblk = (int)((nbar + NB - 1) / NB);
    h->tile_cap = h->nblk + 8;
    h->ngeno_blk = M.G > 0 ? (int)std::min<long long>(((M.G + 1) / 2 + 255) / 256, 64) : 0;
    return 0;
}

// the DevState arrays (all zeroed), the optimiser constants, the window's rows (hist_rows), the host-mapped status words
static int alloc_state(bb_handle* h) {
    const DevModel& M = h->M;
    DevState& S = h->S;
    const bb_advi_opts& o = h->o;
    const size_t D = (size_t)M.D, row = (size_t)(M.K + 2 * M.nt1);
    const double optc[8] = {o.eta, o.tau, o.pre, o.post, 0, 0, 0, 0};
    int rc;
    if ((rc = dalloc(h, &S.mu, D + 2)) || (rc = dalloc(h, &S.om, D + 2)) || (rc = dalloc(h, &S.acc_mu, D + 2)) || (rc = dalloc(h, &S.acc_om, D + 2)) ||
        (rc = dalloc(h, &S.accl, 2 * D + 8)) || (rc = upload(h, &S.optc, optc, 8)))
        return rc;
    // (zsv, asv, hsv, gacc_*, bak_*: per-sample scratch of the two-kernel step and of bb_elbo_grad -- ensure_scratch, on first use: a
    //  shard that only ever runs the resident launch never pays their 7 x 8 D bytes)
    hist_rows(h);
    if (o.optimizer == BB_OPT_TRUNCATED_ADAGRAD && (rc = dalloc(h, &S.hist, (size_t)o.window * 2 * (size_t)M.Dh + 8))) return rc;   // (+ 8: an edge pair's prefetch reads both halves)
    if ((rc = dalloc(h, &S.partials, (size_t)M.K * (size_t)h->nblk)) || (rc = dalloc(h, &S.totals, (size_t)M.K)) ||
        (rc = dalloc(h, &S.zg, (size_t)2 * M.nt1)) || (rc = dalloc(h, &S.gbar, (size_t)32 * 10)) ||
        (rc = hostmap_alloc(&h->hstatus, &S.hstatus, 16)) ||
        (rc = dalloc(h, &S.prow, (size_t)h->tile_cap * row)) || (rc = dalloc(h, &S.xrow, (size_t)2 * BB_NG_MAX * row)) ||
        // (+ 16 groups x 16: a leader's eight loads in flight run past its last member, bb_gran_poll8)
        (rc = dalloc(h, &S.grow, (size_t)(h->tile_cap + 16 * BB_NG_MAX) * bb_row_stride(M.K + 2 * M.nt1))) ||
        (rc = dalloc(h, &S.gxrow, (size_t)2 * BB_NG_MAX * row)) || (rc = dalloc(h, &S.rdy, (size_t)32 * (h->tile_cap + 2 * BB_NG_MAX))) ||
        (rc = dalloc(h, &S.xtab, (size_t)BB_NG_MAX)) || (rc = dalloc(h, &S.xsel, (size_t)h->tile_cap)) ||
        (rc = dalloc(h, &S.ztheta, (size_t)std::max(M.G, 1))) || (rc = dalloc(h, &S.gsum, (size_t)std::max(M.G, 1))) ||
        (rc = dalloc(h, &S.ds, (size_t)M.nb)) || (rc = dalloc(h, &S.geno_el, (size_t)std::max(h->ngeno_blk, 1))) ||
        (rc = dalloc(h, &S.elbo_ring, (size_t)BB_ELBO_RING)) || (rc = dalloc(h, &S.elbo_sample, (size_t)o.samples_per_step + 64)) ||
        (rc = dalloc(h, &S.ctr, (size_t)2)) || (rc = dalloc(h, &S.stamps, (size_t)h->tile_cap * (32 + 64))))
        return rc;
    S.eps_in = nullptr;
    return 0;
}

// One handle on one device from a request check_request has accepted (bb_create; group_create, per shard).
static int create_inner(const bb_model_desc* md, const bb_advi_opts* opts, const CreateCtx& cx, bb_handle** out) {
    HandleOwner own(new bb_handle());
    bb_handle* h = own.get();
    h->o = *opts;
    h->tune = cx.tune;
    if (h->o.resum_every < 0) h->o.resum_every = 0;      // 0 = the default schedule (bb_slot_of)
    int rc;
    if ((rc = dev_check(opts->device))) return rc;
    BB_ENTER(h);
    if ((rc = stream_open(&h->stream, h->be))) return rc;
    h->opened = true;
    DevModel& M = h->M;
    double sum_lgamma = 0.0, sum_log_std = 0.0;
    set_shapes(h, md);
    lay_out(h, cx);
    if ((rc = load_counts(h, md, &sum_lgamma)) || (rc = load_pivot(h, md)) || (rc = load_indices(h, md)) || (rc = load_priors(h, md, &sum_log_std))) return rc;
    // constant part of the ELBO: prior normalisers, likelihood normalisers, lgamma terms, entropy constant
    const double nlik = (double)M.nt1 * (double)M.B;
    h->elbo_const = -sum_log_std - 0.5 * BB_LOG2PI * (double)M.D - sum_lgamma - 0.5 * BB_LOG2PI * nlik + 0.5 * (double)M.D * (1.0 + BB_LOG2PI);
    cut_shard(h, md);
    if ((rc = pick_geometry(h)) || (rc = alloc_state(h))) return rc;
    // algorithmic bytes per step on this shard: theta r+w, optimiser state r+w, counts
    const double frac = (double)(h->b_hi - h->b_lo) / (double)M.B;
    const double Dsh = (double)M.D * frac, cnts = 4.0 * (double)n_cells(M) * frac;
    h->bytes_sample = (int64_t)(16.0 * Dsh + cnts);
    h->bytes_update = (int64_t)((16.0 + 16.0 + (opts->optimizer == BB_OPT_TRUNCATED_ADAGRAD ? 64.0 : 32.0)) * Dsh + cnts);
    Planned plan;
    if ((rc = plan_or_refuse(h, h->o.launch_mode, false, plan))) return rc;
    (void)install_plan(h, plan);      // (an allocation or copy that fails there leaves the two-kernel plan: the handle is created with it)
    if ((rc = sync_descriptors(h)) || (rc = bb_init_meanfield(h))) return rc;
    *out = own.release();
    return BB_OK;
}

// ---- caller's order <-> the handle's order (genotype model with geno_idx not in runs) ------------------------------------------
static void perm_gather(const bb_handle* h, const double* caller, double* internal) {
    const size_t D = h->cidx.size();
    for (size_t i = 0; i < D; ++i) internal[i] = caller[(size_t)h->cidx[i]];
}
static void perm_scatter(const bb_handle* h, const double* internal, double* caller) {
    const size_t D = h->cidx.size();
    for (size_t i = 0; i < D; ++i) caller[(size_t)h->cidx[i]] = internal[i];
}

// The order the handle works in where it is not the caller's (genotype model only), for a request check_request has accepted: decide()
// says whether to regroup the mutants and whether loglambda goes first, and makes the description create_inner gets; install() writes
// the caller's layout and the map internal -> caller into the finished handle.
struct CallerOrder {
    bool regroup = false, loglambda_first = false;
    bb_model_desc md{};                    // what create_inner gets: the caller's description, or its regrouped copies (below)
    std::vector<int> perm;                 // perm[m'] = the caller's mutant of internal mutant m'
    std::vector<int64_t> counts2;          // the regrouped copies md points into
    std::vector<int32_t> geno2;
    std::vector<double> lsm, lss, llm, lls;
    long long src(long long b) const { return b < md.n_neutral ? b : md.n_neutral + perm[(size_t)(b - md.n_neutral)]; }   // the caller's barcode of internal barcode b

    int decide(const bb_model_desc* caller, const BBTuning& tune) {
        md = *caller;
        if (md.kind != BB_MODEL_GENOTYPE || md.n_bc <= 1) return 0;
        const long long nn = md.n_neutral, nb = md.n_bc, B = nn + nb;
        const int T = md.n_time[0];
        // Round 4: the genotype model's flat vector s_pop | logsigma_pop | theta (G) | theta_tilde | logtau | logsigma_bc (n_bc each) | loglambda puts
        // loglambda at an ODD index whenever G + n_bc is odd; k_res's pairs (b, 2k), (b, 2k+1) are then not pairs (2q, 2q+1) of the flat index and
        // the any-parity instances ran (two Philox draws in divergent lanes, 8-byte accesses, 40 spilled registers: C5's rank shape 14.95 against
        // 12.8 us).  The library owns an internal order anyway: it lays loglambda out right behind the two global blocks (offset 2 (T - 1): even
        // for even T) and presents the reference's order at every entry point, as for the regrouped mutants.  BB_NO_REORDER=1: as handed over.
        loglambda_first = !(T & 1) && ((md.n_geno + nb) & 1) && !tune.no_reorder;
        regroup = !tune.no_regroup && !std::is_sorted(caller->geno_idx, caller->geno_idx + nb);
        if (!regroup) return 0;
        perm.resize((size_t)nb);
        for (long long m = 0; m < nb; ++m) perm[(size_t)m] = (int)m;
        std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return caller->geno_idx[a] < caller->geno_idx[b]; });
        counts2.resize((size_t)B * T);
        for (long long b = 0; b < B; ++b) memcpy(&counts2[(size_t)b * T], caller->counts + src(b) * T, (size_t)T * sizeof(int64_t));
        geno2.resize((size_t)nb);
        for (long long m = 0; m < nb; ++m) geno2[(size_t)m] = caller->geno_idx[perm[(size_t)m]];
        md.counts = counts2.data();
        md.geno_idx = geno2.data();
        // Matrix-form priors of the per-mutant and per-(time, barcode) blocks move with their barcodes (checked first: a message names
        // the element where the caller put it)
        if (md.logsigma_bc_prior.n == nb && check_prior(&md.logsigma_bc_prior, "logsigma_bc_prior")) return BB_ERR_INVALID;
        if (md.loglambda_prior.n == (int64_t)B * T && check_prior(&md.loglambda_prior, "loglambda_prior")) return BB_ERR_INVALID;
        // rows of `w` elements: internal row i is the caller's row from(i)
        auto move_rows = [](bb_prior& p, long long rows, long long w, auto from, std::vector<double>& mean, std::vector<double>& std_) {
            if (!p.mean || !p.std || p.n != rows * w) return;
            mean.resize((size_t)(rows * w));
            std_.resize((size_t)(rows * w));
            for (long long i = 0; i < rows; ++i)
                for (long long j = 0; j < w; ++j) { mean[(size_t)(i * w + j)] = p.mean[from(i) * w + j]; std_[(size_t)(i * w + j)] = p.std[from(i) * w + j]; }
            p.mean = mean.data();
            p.std = std_.data();
        };
        move_rows(md.logsigma_bc_prior, nb, 1, [&](long long m) { return (long long)perm[(size_t)m]; }, lsm, lss);
        move_rows(md.loglambda_prior, B, T, [&](long long b) { return src(b); }, llm, lls);
        return 0;
    }

    // the caller's layout: the reference's source order (what bb_get_layout reports), and the map internal -> caller
    void install(bb_handle* h) const {
        if (!regroup && !loglambda_first) return;
        const DevModel& M = h->M;
        const long long nn = M.nn, nb = M.nb, B = M.B;
        const int T = M.T[0];
        if (regroup) h->perm_m = perm;
        const int order[BK_COUNT] = {BK_SPOP, BK_LSPOP, BK_S, BK_TT, BK_LT, BK_LS, BK_L};
        long long clo[BK_COUNT] = {0};
        std::vector<bb_block_range> cb;
        long long off = 0;
        for (int k : order) {
            bb_block_range b;
            memset(&b, 0, sizeof b);
            for (const bb_block_range& ib : h->blocks) if (ib.lo == M.blk_lo[k] && ib.hi == M.blk_hi[k] && ib.hi > ib.lo) snprintf(b.name, sizeof b.name, "%s", ib.name);
            clo[k] = off;
            b.lo = off;
            b.hi = off + (M.blk_hi[k] - M.blk_lo[k]);
            off = b.hi;
            cb.push_back(b);
        }
        h->blocks = cb;
        h->cidx.resize((size_t)M.D);
        for (int k : order)
            for (long long j = 0; j < M.blk_hi[k] - M.blk_lo[k]; ++j) h->cidx[(size_t)(M.blk_lo[k] + j)] = clo[k] + j;
        if (regroup) {
            for (int k : {BK_TT, BK_LT, BK_LS})
                for (long long m = 0; m < nb; ++m) h->cidx[(size_t)(M.blk_lo[k] + m)] = clo[k] + perm[(size_t)m];
            for (long long b = nn; b < B; ++b)
                for (int t = 0; t < T; ++t) h->cidx[(size_t)(M.blk_lo[BK_L] + b * T + t)] = clo[BK_L] + src(b) * T + t;
        }
    }
};

// The reference hands barcodes over in order of appearance (utils.data_to_arrays, src/utils.jl:692-731), so a genotype's mutants
// are scattered; the resident launch and genotype-aligned shards need them in consecutive runs (a tile / shard owns whole
// genotypes and their theta).  The library groups them itself -- a stable sort of the mutants by genotype -- works in that order
// and presents the caller's at every entry point that takes or returns a latent vector (bb_get_params / posterior / set_params /
// elbo_grad / logdensity_grad / hier_fitness; bb_get_permutation tells the mapping).  The engine's normal stream is keyed by the
// INTERNAL index (bb_debug_normals likewise).
extern "C" int bb_create(const bb_model_desc* md, const bb_advi_opts* opts, bb_handle** out) {
    if (!md || !opts || !out) return bb_fail(BB_ERR_INVALID, "null argument");
    *out = nullptr;
    int rc;
    if ((rc = check_request(md, opts))) return rc;
    CreateCtx cx{read_tuning(), false};
    CallerOrder order;
    if ((rc = order.decide(md, cx.tune))) return rc;
    cx.loglambda_first = order.loglambda_first;
    if ((rc = opts->n_devices > 1 ? group_create(&order.md, opts, cx, out) : create_inner(&order.md, opts, cx, out))) return rc;
    order.install(*out);
    return BB_OK;
}
