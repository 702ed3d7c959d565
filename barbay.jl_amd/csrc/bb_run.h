// bb_run.h -- how steps are strung together, included once by bb_engine.hip (after the resident launchers and handle creation): captured
// graphs of the two-kernel step loop, bb_run in its two halves, bb_run_profiled, bb_elbo_grad / bb_logdensity_grad (samples that do not
// apply), the ELBO trace, and the split-phase bb_step_moments / bb_step_apply.  What a step launches is bb_step.h's.

// Captured graphs of the step loop: as many whole graphs of the remaining steps as fit, `done` moved past them.  Whole steps only,
// starting on an even step (static ping-pong parity); the elbo_every pattern must repeat with the graph -> only when ELBO recording
// is off; no collectives inside.  The emulation has none: every step is enqueued on its own.
#ifndef BB_EMU
static int build_graph(bb_handle* h, int steps) {
    BackendState& be = h->be;
    if (be.graph && be.graph_steps == steps) return 0;
    if (be.graph) { (void)hipGraphExecDestroy(be.graph); be.graph = nullptr; }
    hipGraph_t g = nullptr;
    BB_HIP(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
    int rc = 0;
    for (int i = 0; i < steps && !rc; ++i) rc = enqueue_step(h, i);   // parity of i == parity of the real step (even start)
    hipError_t e = hipStreamEndCapture(h->stream, &g);
    if (rc || e != hipSuccess) {
        if (g) (void)hipGraphDestroy(g);
        (void)hipGetLastError();
        be.graph_failed = true;      // not an error: bb_run launches eagerly instead
        return 0;
    }
    e = hipGraphInstantiate(&be.graph, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e != hipSuccess) { be.graph = nullptr; (void)hipGetLastError(); be.graph_failed = true; return 0; }
    be.graph_steps = steps;
    return 0;
}
static int run_graphs(bb_handle* h, int64_t n_steps, int64_t& done) {
    int rc = 0;
    int gs = h->o.steps_per_graph == 0 ? 50 : h->o.steps_per_graph;
    // A sharded step (with its RCCL all-reduce) can be captured too (BB_GRAPH_COLLECTIVE=1; equal results, no gain
    // measured: the step is GPU-bound), but multi-rank capture could not be exercised on the one-GPU boxes this was
    // developed on, so sharded runs launch eagerly by default.
    const bool graph_ok = gs > 0 && h->o.elbo_every == 0 && !h->be.graph_failed && !h->tune.no_graph &&
                          ((h->o.world_size == 1 && !h->tune.force_allreduce) || h->tune.graph_collective);
    if (!graph_ok) return 0;
    gs &= ~1;
    if (gs < 2) gs = 2;
    if ((h->step & 1) && done < n_steps) { if ((rc = enqueue_step(h, h->step))) return rc; h->step++; done++; }
    if (n_steps - done >= gs) {
        if ((rc = build_graph(h, gs))) return rc;
        while (h->be.graph && n_steps - done >= gs) {
            BB_HIP(hipGraphLaunch(h->be.graph, h->stream));
            h->graph_launches++;
            h->step += gs;
            done += gs;
        }
    }
    return 0;
}
#else
static int run_graphs(bb_handle*, int64_t, int64_t&) { return 0; }
#endif

// bb_run in two halves (a multi-device handle enqueues on all its shards before it waits for any).  The first half in its parts, for
// bb_run under a trace (below): run_open -- what must hold, and what is reset, before a call's first launch -- and run_steps, the
// launches of n_steps steps as one bb_run call makes them.
static int run_open(bb_handle* h) {
    if (h->sample != 0) return bb_fail(BB_ERR_INVALID, "a split-phase step is in flight");
    int rc = 0;
    if (h->plan.impl == IMPL_TWO_KERNEL && (rc = ensure_scratch(h))) return rc;
    if (h->hstatus) h->hstatus[1] = 0;          // divergence flag of THIS run (nothing of this handle is in flight here)
    if ((rc = timer_start(h->be, h->stream))) return rc;
    h->launches_last_run = 0;
    h->graph_launches = 0;
    return 0;
}
static int run_steps(bb_handle* h, int64_t n_steps) {
    int rc = 0;
    int64_t done = 0;
    if (h->plan.impl != IMPL_TWO_KERNEL && n_steps > 0) {
        if ((rc = launch_persistent(h, n_steps))) return rc;
        done = n_steps;
        h->launches_last_run += (int)((n_steps + 4095) / 4096);
        if (theta_partial(h)) h->theta_stale = true;         // only the owner's theta_g moved (bb_run / group_run gather it afterwards)
    } else if (h->theta_stale && n_steps > 0 && (rc = theta_sync_comm(h))) return rc;
    if ((rc = run_graphs(h, n_steps, done))) return rc;
    for (; done < n_steps; ++done) {
        if ((rc = enqueue_step(h, h->step))) return rc;
        h->step++;
    }
    return 0;
}
static int run_enqueue(bb_handle* h, int64_t n_steps) {
    int rc = run_open(h);
    if (!rc) rc = run_steps(h, n_steps);
    return rc ? rc : timer_stop(h->be, h->stream);
}
static int run_finish(bb_handle* h) {
    int rc = timer_wait(h->be, h->stream, &h->last_run_ms);
    return rc ? rc : check_persistent(h);
}

// ---- bb_run under an iterate trace (bb_trace.h; the contract: include/barbay_hip.h) ---------------------------------------------
static void trace_reset(bb_handle* h) { h->trace_t = 0; h->trace_taken = 0; }
#define BB_TRACE_REFUSED(h, what) \
    do { if ((h)->trace_ring) return bb_fail(BB_ERR_UNSUPPORTED, what " is not available while an iterate trace is on (bb_trace_end first)"); } while (0)

// (mu, omega) as they stand on the stream into the ring's next row
static int trace_snapshot(bb_handle* h) {
    TraceArgs T;
    memset(&T, 0, sizeof T);
    T.ring = h->trace_ring;
    T.D = h->M.D;
    T.D2 = 2 * T.D;
    T.cap = h->trace_cap;
    T.mu = h->S.mu;
    T.om = h->S.om;
    T.slot = h->trace_taken % h->trace_cap;
    const int grid = (int)std::max<long long>(1, std::min<long long>((T.D2 + 4 * BB_TRACE_NT - 1) / (4 * BB_TRACE_NT), 2048));
    const int rc = launch(h->stream, k_trace_snapshot, grid, BB_TRACE_NT, 0, T);
    if (!rc) h->trace_taken++;
    return rc;
}

// n_steps > 0 steps cut at the trace's boundaries, a snapshot behind every piece that ends on one.  Every piece makes the launches of a
// bb_run call of its length (run_steps).  The two-kernel step reports through words nobody reads before the stream has drained
// (check_persistent's non-finite flag), so its pieces and snapshots go out back to back under one run_open / run_finish; a resident
// launch may time out, and what follows a timed-out launch must not be in flight already: there every piece is waited for.
static int run_traced(bb_handle* h, int64_t n_steps) {
    const int64_t every = h->trace_every;
    const bool chained = h->plan.impl == IMPL_TWO_KERNEL;
    int rc = 0, nonfinite = 0;
    std::string why;
    if (chained && (rc = run_open(h))) return rc;
    for (int64_t left = n_steps; left > 0;) {
        const int64_t piece = std::min<int64_t>(left, every - h->trace_t % every);
        if ((rc = chained ? run_steps(h, piece) : run_enqueue(h, piece))) return rc;
        h->trace_t += piece;
        left -= piece;
        if (h->trace_t % every == 0) rc = trace_snapshot(h);
        if (!chained) {
            const int r = run_finish(h);                     // (waits for whatever was launched, also after an error)
            if (r == BB_ERR_NONFINITE) { if (!nonfinite) why = g_err; nonfinite = r; }      // the steps were taken: the run goes on
            else if (r && !rc) rc = r;
        }
        if (rc) return rc;
    }
    if (chained) {
        if ((rc = timer_stop(h->be, h->stream))) return rc;
        return run_finish(h);
    }
    if (nonfinite) snprintf(g_err, sizeof g_err, "%s", why.c_str());
    return nonfinite;
}

static int group_run(bb_handle* g, int64_t n_steps);      // (bb_engine.hip's groups, after this file: group_run needs run_enqueue / run_finish above)

extern "C" int bb_run(bb_handle* h, int64_t n_steps) {
    if (!h || n_steps < 0) return bb_fail(BB_ERR_INVALID, "bad argument");
    if (!h->shards.empty()) return group_run(h, n_steps);
#ifdef BB_HOST_TIMES          // diagnostics (tools/launch_probe.py): where the host's share of a run goes
    timespec ht0, ht1, ht2, ht3;
    clock_gettime(CLOCK_MONOTONIC, &ht0);
#endif
    BB_ENTER(h);
    if (h->trace_ring && n_steps > 0) return run_traced(h, n_steps);
#ifdef BB_HOST_TIMES
    clock_gettime(CLOCK_MONOTONIC, &ht1);
#endif
    int rc = run_enqueue(h, n_steps);
    if (rc) return rc;
#ifdef BB_HOST_TIMES
    clock_gettime(CLOCK_MONOTONIC, &ht2);
#endif
    rc = run_finish(h);
#ifdef BB_HOST_TIMES
    clock_gettime(CLOCK_MONOTONIC, &ht3);
    auto us = [](const timespec& a, const timespec& b) { return (b.tv_sec - a.tv_sec) * 1e6 + (b.tv_nsec - a.tv_nsec) * 1e-3; };
    fprintf(stderr, "[bb_run %lld] device guard %.1f us, enqueue %.1f us, wait + status %.1f us, events %.1f us\n", (long long)n_steps, us(ht0, ht1), us(ht1, ht2), us(ht2, ht3), h->last_run_ms * 1e3);
#endif
    if (h->theta_stale && comm_ready(h->be)) {
        // Collective, so EVERY rank takes it whatever its own launch reported: the timeout word and the non-finite flag run_finish
        // looks at are this rank's alone, and a rank that returned early here would leave the clean ranks inside ncclAllReduce.
        // The rank's own error is reported afterwards (the gathered theta rows of a failed run mean nothing, but nobody hangs).
        const std::string why(g_err);
        const int rc2 = theta_sync_comm(h);
        if (rc) snprintf(g_err, sizeof g_err, "%s", why.c_str());
        else rc = rc2;
    }
    return rc;
}

// bb_run_profiled: the two halves of every sample of the single-GPU two-kernel step (no reduce, no genotype block: k_sample, k_update)
// between events of their own (the emulation has no clock worth reading: a plain run)
#ifdef BB_EMU
static int run_profiled(bb_handle* h, int64_t n_steps) { return bb_run(h, n_steps); }
#else
static int run_profiled(bb_handle* h, int64_t n_steps) {
    if (h->use_reduce()) return bb_fail(BB_ERR_UNSUPPORTED, "bb_run_profiled covers the single-GPU two-kernel step only");
    { const int rcs = ensure_scratch(h); if (rcs) return rcs; }
    const int S = h->o.samples_per_step;
    const size_t nl = (size_t)n_steps * S;
    std::vector<hipEvent_t> ev(3 * nl);
    for (auto& e : ev) BB_HIP(hipEventCreate(&e));
    int rc = 0;
    for (int64_t i = 0; i < n_steps && !rc; ++i) {
        for (int s = 0; s < S && !rc; ++s) {
            const RunArgs A = make_args(h, h->step, s, S, true, elbo_wanted(h, h->step));
            const size_t k = 3 * ((size_t)i * S + s);
            BB_HIP(hipEventRecord(ev[k], h->stream));
            rc = sample_half(h, A);
            BB_HIP(hipEventRecord(ev[k + 1], h->stream));
            if (!rc) rc = update_half(&h, 1, &A, comm_exchange);
            BB_HIP(hipEventRecord(ev[k + 2], h->stream));
        }
        h->step++;
    }
    BB_HIP(hipStreamSynchronize(h->stream));
    double ts = 0, tu = 0;
    for (size_t k = 0; k < nl; ++k) {
        float a = 0, b = 0;
        BB_HIP(hipEventElapsedTime(&a, ev[3 * k], ev[3 * k + 1]));
        BB_HIP(hipEventElapsedTime(&b, ev[3 * k + 1], ev[3 * k + 2]));
        ts += a;
        tu += b;
    }
    for (auto& e : ev) (void)hipEventDestroy(e);
    if (nl) { h->avg_sample_ms = ts / nl; h->avg_update_ms = tu / nl; }
    return rc;
}
#endif
extern "C" int bb_run_profiled(bb_handle* h, int64_t n_steps) {
    if (!h || n_steps < 0) return bb_fail(BB_ERR_INVALID, "bad argument");
    BB_GROUP_UNSUPPORTED(h, "bb_run_profiled");
    BB_TRACE_REFUSED(h, "bb_run_profiled");
    BB_ENTER(h);
    return run_profiled(h, n_steps);
}

static int elbo_grad_raw(bb_handle* h, const double* mu, const double* omega, const double* eps, int32_t S, double* elbo, double* grad_mu, double* grad_omega) {
    BB_GROUP_UNSUPPORTED(h, "bb_elbo_grad");
    BB_ENTER(h);
    if (h->o.world_size > 1 && !eps) return bb_fail(BB_ERR_UNSUPPORTED, "bb_elbo_grad on a sharded handle needs explicit eps");
    const size_t D = (size_t)h->M.D;
    int rc;
    // what can fail before the handle is touched: scratch, the copy of the parameters to put back, room for the draws, and for the
    // per-sample ELBO values where S is more than the handle's own buffer holds
    if ((rc = ensure_scratch(h))) return rc;
    if ((rc = d2d(h->bak_mu, h->S.mu, D * 8, h->stream)) || (rc = d2d(h->bak_om, h->S.om, D * 8, h->stream))) return rc;
    if (eps && (rc = h->buf[BUF_EPS].grow((size_t)S * D))) return rc;
    void* es = nullptr;
    if (S > h->o.samples_per_step + 64 && (rc = dmalloc(&es, (size_t)S * 8))) return rc;
    // from here on the handle holds the caller's point and buffers: every path goes through the restore below
    double* const saved_es = h->S.elbo_sample;
    std::vector<double> ev((size_t)S);
    auto eval = [&]() -> int {
        int r;
        if ((r = h2d(h->S.mu, mu, D * 8, h->stream)) || (r = h2d(h->S.om, omega, D * 8, h->stream))) return r;
        if (eps) {
            if ((r = h2d(h->buf[BUF_EPS].p, eps, (size_t)S * D * 8, h->stream))) return r;
            h->S.eps_in = h->buf[BUF_EPS].p;
        }
        if (es) h->S.elbo_sample = (double*)es;
        if ((r = sync_descriptors(h))) return r;
        for (int s = 0; s < S; ++s)
            if ((r = step_sample(h, make_args(h, h->step, s, S, false, true)))) return r;
        return d2h(ev.data(), h->S.elbo_sample, (size_t)S * 8, h->stream);
    };
    rc = eval();
    h->S.elbo_sample = saved_es;
    if (es) dfree(es);
    h->S.eps_in = nullptr;
    { int rcs = sync_descriptors(h); if (!rc) rc = rcs; }
    if (!rc && grad_mu) rc = d2h(grad_mu, h->S.gacc_mu, D * 8, h->stream);
    if (!rc && grad_omega) rc = d2h(grad_omega, h->S.gacc_om, D * 8, h->stream);
    int rc2 = d2d(h->S.mu, h->bak_mu, D * 8, h->stream);
    int rc3 = d2d(h->S.om, h->bak_om, D * 8, h->stream);
    int rc4 = dsync(h->stream);
    if (rc) return rc;
    if (rc2 || rc3 || rc4) return rc2 ? rc2 : (rc3 ? rc3 : rc4);
    if (elbo) {
        double v = 0;
        for (int s = 0; s < S; ++s) v += ev[(size_t)s];
        *elbo = v / S;
    }
    return BB_OK;
}
extern "C" int bb_elbo_grad(bb_handle* h, const double* mu, const double* omega, const double* eps, int32_t S,
                            double* elbo, double* grad_mu, double* grad_omega) {
    if (!h || !mu || !omega || S < 1) return bb_fail(BB_ERR_INVALID, "bad argument");
    if (h->cidx.empty()) return elbo_grad_raw(h, mu, omega, eps, S, elbo, grad_mu, grad_omega);
    const size_t D = h->cidx.size();
    std::vector<double> pm(D), po(D), pe, gm(D), go(D);
    perm_gather(h, mu, pm.data());
    perm_gather(h, omega, po.data());
    if (eps) { pe.resize((size_t)S * D); for (int s = 0; s < S; ++s) perm_gather(h, eps + (size_t)s * D, pe.data() + (size_t)s * D); }
    int rc = elbo_grad_raw(h, pm.data(), po.data(), eps ? pe.data() : nullptr, S, elbo, grad_mu ? gm.data() : nullptr, grad_omega ? go.data() : nullptr);
    if (rc) return rc;
    if (grad_mu) perm_scatter(h, gm.data(), grad_mu);
    if (grad_omega) perm_scatter(h, go.data(), grad_omega);
    return BB_OK;
}

// log-joint density and its gradient at a point of the unconstrained latent space: the ELBO machinery with the
// draw pinned to the mean (eps = 0) and sigma = softplus(omega) = 1, minus the entropy terms -- what an HMC / NUTS
// sampler asks of a model (`LogDensityProblems.logdensity_and_gradient`; the reference's src/mcmc.jl:86-160 path)
extern "C" int bb_logdensity_grad(bb_handle* h, const double* z, double* logp, double* grad) {
    if (!h || !z) return bb_fail(BB_ERR_INVALID, "null argument");
    BB_ENTER(h);
    const size_t D = (size_t)h->M.D;
    const double om1 = 0.54132485461291810;                  // log(e - 1): softplus = 1
    if (h->ld_omega.size() != D) { h->ld_omega.assign(D, om1); h->ld_zero.assign(D, 0.0); }
    double elbo = 0.0;
    int rc = bb_elbo_grad(h, z, h->ld_omega.data(), h->ld_zero.data(), 1, &elbo, grad, nullptr);
    if (rc) return rc;
    if (logp) *logp = elbo - 0.5 * (double)D * (1.0 + BB_LOG2PI) - (double)D * log(log1p(exp(om1)));
    return BB_OK;
}

extern "C" int bb_get_elbo_trace(bb_handle* h, int64_t first_step, int64_t n, double* out) {
    if (!h || !out || n < 0) return bb_fail(BB_ERR_INVALID, "bad argument");
    if (!h->shards.empty()) return bb_get_elbo_trace(h->shards[0], first_step, n, out);      // (every shard forms the same estimate from the same totals)
    BB_ENTER(h);
    if (h->o.elbo_every <= 0) return bb_fail(BB_ERR_INVALID, "ELBO recording is off (elbo_every = 0)");
    std::vector<double> ring(BB_ELBO_RING);
    int rc = dsync(h->stream);
    if (rc) return rc;
    if ((rc = d2h(ring.data(), h->S.elbo_ring, ring.size() * 8, h->stream))) return rc;
    const int64_t ev = h->o.elbo_every;
    const int64_t newest = h->step > 0 ? (h->step - 1) / ev : -1;
    for (int64_t k = 0; k < n; ++k) {
        const int64_t st = first_step + k * ev;
        const int64_t idx = st / ev;
        const bool have = st % ev == 0 && st >= 0 && st < h->step && idx > newest - BB_ELBO_RING;
        out[k] = have ? ring[(size_t)(idx % BB_ELBO_RING)] : NAN;
    }
    return BB_OK;
}

// The split-phase step: the two halves of step_sample with the caller as the exchange of the K totals -- bb_step_moments hands out this
// handle's totals, bb_step_apply takes them back summed over the caller's shards (so both halves run with the totals reduced: make_args).
static RunArgs split_phase_args(const bb_handle* h) { return make_args(h, h->step, h->sample, h->o.samples_per_step, true, elbo_wanted(h, h->step), true); }

extern "C" int bb_step_moments(bb_handle* h, double* partial) {
    if (!h || !partial) return bb_fail(BB_ERR_INVALID, "null argument");
    BB_GROUP_UNSUPPORTED(h, "bb_step_moments");
    BB_TRACE_REFUSED(h, "bb_step_moments");
    BB_ENTER(h);
    if (h->M.kind == BB_MODEL_GENOTYPE && h->o.world_size > 1)
        return bb_fail(BB_ERR_UNSUPPORTED, "split-phase stepping of the sharded genotype model needs a second exchange; use bb_comm_init + bb_run");
    int rc;
    if ((rc = ensure_scratch(h))) return rc;
    if ((rc = sample_half(h, split_phase_args(h)))) return rc;
    return d2h(partial, h->S.totals, (size_t)h->M.K * 8, h->stream);
}

extern "C" int bb_step_apply(bb_handle* h, const double* total) {
    if (!h || !total) return bb_fail(BB_ERR_INVALID, "null argument");
    BB_GROUP_UNSUPPORTED(h, "bb_step_apply");
    BB_TRACE_REFUSED(h, "bb_step_apply");
    BB_ENTER(h);
    const RunArgs A = split_phase_args(h);
    int rc;
    if ((rc = ensure_scratch(h))) return rc;
    if ((rc = h2d(h->S.totals, total, (size_t)h->M.K * 8, h->stream))) return rc;
    if ((rc = update_half(&h, 1, &A, comm_exchange))) return rc;
    if (++h->sample == A.S) { h->sample = 0; h->step++; }
    return dsync(h->stream);
}
