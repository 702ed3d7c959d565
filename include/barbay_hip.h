/* barbay_hip.h -- C ABI of the MI355X-native ADVI engine behind BarBay.vi.advi().
 *
 * Drop-in boundary: the one line this library replaces in the reference is
 *     q = Turing.vi(bayes_model, advi; optimizer=opt)          (src/vi.jl:201)
 * Everything before it (src/vi.jl:103-198) produces the inputs described by
 * bb_model_desc / bb_advi_opts; everything after it (src/vi.jl:203-234,
 * src/utils.jl:1042-1078, 1409-1462) reads only q.dist.m, q.dist.σ and
 * q.transform.ranges_out, which bb_get_posterior / bb_get_layout return.
 *
 * Conventions
 *  - plain C, no C++ exceptions cross the boundary; every int-returning entry
 *    point returns BB_OK (0) or a negative BB_ERR_* code, with a thread-local
 *    message available from bb_last_error().
 *  - the caller owns every host array it passes; the library copies what it
 *    needs during the call and never retains a host pointer.
 *  - the flat latent vector is the concatenation of the model's `~` blocks in
 *    source order with Julia column-major indexing.
 *  - one handle = one host thread at a time; it drives one GPU, or bb_advi_opts.n_devices GPUs of the node.
 */
#ifndef BARBAY_HIP_H
#define BARBAY_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BB_OK 0
#define BB_ERR_INVALID (-1)   /* bad argument / inconsistent description     */
#define BB_ERR_DEVICE (-2)    /* HIP runtime error                           */
#define BB_ERR_COMM (-3)      /* RCCL error / communicator not initialised   */
#define BB_ERR_UNSUPPORTED (-4)
#define BB_ERR_NONFINITE (-5) /* bb_run: the steps were taken, but the variational parameters (or the exchanged
                                 moments) went NaN / Inf on the way -- the reference has no such guard and would
                                 return the NaN posterior silently                      */

/* model kinds: BarBay.model.* entries on the hot path */
#define BB_MODEL_FITNESS 0    /* fitness_normal            src/model_fitness_normal.jl:120-272 */
#define BB_MODEL_MULTIENV 1   /* multienv_fitness_normal   src/model_multienv_fitness_normal.jl:133-303 */
#define BB_MODEL_GENOTYPE 2   /* genotype_fitness_normal   src/model_fitness_normal_hierarchical_genotypes.jl:151-330 */
#define BB_MODEL_REPLICATE 3  /* replicate_fitness_normal  src/model_fitness_normal_hierarchical_replicates.jl:145-332 (3-D)
                                 and :407-638 (ragged); equal n_time[] == the 3-D method */

#define BB_MODEL_MULTIENV_REPLICATE 4 /* multienv_replicate_fitness_normal
                                 src/model_multienv_fitness_normal_hierarchical_replicates.jl:158-363 (3-D), :449-687 (ragged) */

/* bb_model_desc.flags */
#define BB_FLAG_RAGGED_METHOD 1 /* BB_MODEL_REPLICATE called as the reference's Vector{Matrix} method
                                  (src/model_fitness_normal_hierarchical_replicates.jl:407-638): its neutral
                                  likelihood pairs data element (t, b) with population index
                                  (t + (T_r-1) b) div n_neutral (`repeat(.., inner=n_neutral)`, :599-605, against a
                                  time-fastest data vector :549).  Reproduced as written when this flag is set;
                                  without it the 3-D method's self-consistent pairing (:307-311) is evaluated. */

/* optimisers selectable at src/vi.jl:99 (AdvancedVI 0.2) */
#define BB_OPT_TRUNCATED_ADAGRAD 0
#define BB_OPT_DECAYED_ADAGRAD 1

/* A prior argument of a model (`VecOrMat{Float64}`, model_fitness_normal.jl:125-129):
 * n == 0 or a null pointer: the reference's default for the block;
 * n == 1  : Vector form [mean, std] shared by the block;
 * n == len: Matrix form, mean[i], std[i] per element of the block, in the block's own order as the CALLER lays it out (loglambda:
 *           t fastest per barcode, replicate-major; the per-mutant blocks of the multienv / replicate kinds: one element per
 *           (mutant, environment) / (mutant, replicate)).  Where the library regroups a genotype model's mutants or moves a block
 *           (bb_get_permutation) the elements move with their latents.
 * Every mean must be finite and every std finite and > 0, else bb_create returns BB_ERR_INVALID and bb_last_error names the prior
 * (Matrix form: and the element, "s_pop_prior: std[3] ..."); any other n is BB_ERR_INVALID too ("Matrix form needs <len> rows"). */
typedef struct bb_prior {
    const double* mean;
    const double* std;
    int64_t n;
} bb_prior;

/* What `model(R, n_t, n_neutral, n_bc; kwargs...)` receives (src/vi.jl:172-178),
 * in the layout src/utils.jl:48-61 (DataArrays) hands over. */
typedef struct bb_model_desc {
    int32_t kind;            /* BB_MODEL_*                                                */
    int32_t n_rep;           /* replicates (1 unless BB_MODEL_REPLICATE / _MULTIENV_REPLICATE) */
    int64_t n_neutral;       /* neutral barcodes: columns 0..n_neutral-1 (utils.jl:431)   */
    int64_t n_bc;            /* mutant barcodes                                           */
    const int32_t* n_time;   /* [n_rep] time points per replicate                         */
    const int64_t* counts;   /* replicate-major; each T_r x B column-major (t fastest)    */
    const int64_t* totals;   /* replicate-major; [T_r] = row sums of counts               */
    int32_t n_env;           /* BB_MODEL_MULTIENV: number of distinct environments        */
    const int32_t* env_idx;  /* [sum_r T_r] 0-based env of each time point, replicate-major
                                (indexin(envs, unique(envs)); the 3-D multienv_replicate method
                                repeats its one env list per replicate)                   */
    int32_t n_geno;          /* BB_MODEL_GENOTYPE: number of distinct genotypes           */
    const int32_t* geno_idx; /* [n_bc] 0-based genotype of each mutant                    */
    bb_prior s_pop_prior;        /* default [0,2] */
    bb_prior logsigma_pop_prior; /* default [0,1] */
    bb_prior s_bc_prior;         /* default [0,2]; theta prior for the hierarchical models */
    bb_prior logsigma_bc_prior;  /* default [0,1] */
    bb_prior loglambda_prior;    /* default [3,3] */
    bb_prior logtau_prior;       /* default [-2,1]; Vector form only (as in the reference): n > 1 is BB_ERR_INVALID */
    int32_t flags;               /* BB_FLAG_*                                              */
} bb_model_desc;

/* Turing.ADVI(samples_per_step, max_iters) + optimiser + engine options.
 * eta, tau, pre, post are the handle's own: they are copied into a device table at bb_create and every launch of the handle (two-kernel
 * step, resident launches, split-phase step) reads them from there, so handles with different constants can live side by side.  Each
 * must be finite, else BB_ERR_INVALID; no sign is imposed (eta = 0 takes the steps and leaves the parameters where they are). */
typedef struct bb_advi_opts {
    int32_t samples_per_step; /* S >= 1                                                  */
    int32_t optimizer;        /* BB_OPT_*                                                */
    double eta;               /* both optimisers, default 0.1: step = eta / (tau + sqrt(s)) or eta / (sqrt(acc) + 1e-8) */
    double tau;               /* TruncatedADAGrad, default 40                            */
    int32_t window;           /* TruncatedADAGrad n, default 100                         */
    int32_t resum_every;      /* TruncatedADAGrad: 1 = re-add the whole window every step
                                 (same arithmetic as the reference's sum(g2)); k > 1 =
                                 running sum, exact re-add every k steps; 0 (default) =
                                 running sum, never re-added: a compensated (two-sum)
                                 accumulator whose low-order part is a float, so what is
                                 lost per step is 2^-77 of the sum AT THAT STEP -- it stays
                                 behind when the sum later falls by orders of magnitude.
                                 Measured against the correctly rounded window sum
                                 (tools/window_sum_accuracy.py ->
                                 profiles/window_sum_accuracy_10k.json): 0 at 100 steps,
                                 3e-11 at 1 000, 7e-8 at 5 000, 3e-8 at 10 000 (relative,
                                 worst latent); the step size eta / (tau + sqrt(s)) moves
                                 by at most 1e-8 of itself.  k > 1 bounds it.             */
    double pre;               /* DecayedADAGrad, default 1.0: acc = post acc + pre g^2   */
    double post;              /* DecayedADAGrad, default 0.9                             */
    uint64_t seed;            /* Philox key (DESIGN.md "RNG stream")                     */
    int32_t device;           /* HIP device ordinal                                      */
    int32_t rank;             /* barcode shard owned by this handle                      */
    int32_t world_size;       /* number of shards (1 = whole problem)                    */
    int32_t steps_per_graph;  /* steps captured per hipGraph (0 = default, <0 = eager)   */
    int32_t elbo_every;       /* evaluate the ELBO every k-th step (0 = never)           */
    int32_t launch_mode;      /* 0 = auto; 1 = two kernels per sample (graph / eager);
                                 2 = ONE resident launch for the whole step loop (k_res /
                                 k_stream / k_persist, bb_stats.resident_kernel; the exchange
                                 of the moment rows runs inside it) -- on one GPU also with
                                 samples_per_step > 1 and ELBO recording (k_res's MS
                                 instances), on a sharded handle with the rows pushed into
                                 the peers' inboxes; error if the shape has no such launch  */
    int32_t n_devices;        /* > 1: ONE handle drives this many GPUs from the calling host
                                 thread: the barcodes shard over the devices,
                                 the resident launches run concurrently and exchange their
                                 group rows through peer-mapped inboxes (xGMI); rank /
                                 world_size must then be 0 / 1.  0 or 1 = one device.       */
    const int32_t* device_ids;/* [n_devices] HIP ordinals, or NULL = 0 .. n_devices-1       */
} bb_advi_opts;

typedef struct bb_handle bb_handle;

typedef struct bb_block_range {
    char name[24];  /* s_pop, logsigma_pop, s_bc, logsigma_bc, theta, theta_tilde, logtau, loglambda */
    int64_t lo;     /* 0-based, half-open: q.transform.ranges_out[i] == lo+1 : hi                     */
    int64_t hi;
} bb_block_range;

typedef struct bb_stats {
    int64_t n_latents;         /* D                                                      */
    int64_t n_moments;         /* K doubles all-reduced per MC sample                    */
    int64_t steps_done;
    int64_t shard_lo, shard_hi;/* barcode range owned by this handle                     */
    int64_t bytes_per_step;    /* algorithmic HBM bytes per step on this shard           */
    int64_t bytes_sample, bytes_update; /* its split over the two kernels                */
    double last_run_ms;        /* HIP-event time of the last bb_run                      */
    double avg_sample_ms;      /* per-launch averages from the last bb_run_profiled      */
    double avg_update_ms;
    int32_t n_blocks, block_threads, lds_bytes;
    int32_t persistent_pairs;  /* > 0: bb_run uses the resident launch with this many latent pairs per thread */
    int32_t launches_last_run; /* kernel launches of the last bb_run (resident launch: <= 4096 steps each)       */
    int32_t resident_kernel;   /* which resident launch bb_run uses: 0 none (two kernels per sample), 1 k_persist
                                  (LDS-staged passes), 2 k_res (the owner of a latent computes; bb_resident.h), 3 k_stream
                                  (k_res's tile map with the per-pair state streamed: tiles beyond the register file; bb_stream.h) */
    int32_t geno_lo, geno_hi;  /* genotype model: the genotypes whose theta THIS handle owns (0 .. n_geno unless the run is
                                  sharded and geno_idx is non-decreasing: shards are then cut at genotype boundaries, and after
                                  a resident run only the owner's copy of theta_g is current)                          */
    int64_t device_bytes;      /* device memory this handle allocated (a multi-device handle: all its shards)          */
    int64_t window_row;        /* entries of one row of the TruncatedADAGrad window: n_latents rounded up to 8 on a
                                  whole-problem handle; a shard keeps only the latents it updates (folded rows)        */
    int32_t rows_same_xcd;     /* k_res / k_stream: tiles of the last launch that found themselves on their exchange group
                                  leader's XCD and stored their row through the L2 they share (of n_blocks; 0 with
                                  BB_TUNE_ROW_L2=0 in the environment, which keeps every row store write-through)        */
    int32_t reserved0;
    int32_t opt_compiled;      /* 1: the resident launch is an instance with the optimiser compiled in (TruncatedADAGrad with
                                  resum_every == 0: no run-time choice of optimiser or re-add schedule in the step loop); 0: the
                                  generic instance (resum_every >= 1, DecayedADAGrad, shapes without such an instance,
                                  BB_TUNE_OPT_SPEC=0 in the environment, no resident launch).  Same results either way;
                                  bb_kernel_name does not tell the two apart                                             */
    int32_t reserved1;
} bb_stats;

const char* bb_version(void);
const char* bb_last_error(void);

void bb_default_opts(bb_advi_opts* opts);

/* Build device state for one model instance.  Validates the description
 * (shapes, totals == row sums, index ranges) and copies everything it needs.
 * Shape limits: n_time[r] outside 2..255 is BB_ERR_INVALID.  A shape whose two-kernel tile of 8 barcodes needs more than the
 * 160 KiB of LDS of a compute unit (bb_lds_layout: the need grows with n_time x n_rep x n_env) is BB_ERR_UNSUPPORTED, "a tile of 8
 * barcodes needs N bytes of LDS / n threads (n_time or n_rep too large for this build)".  Largest uniform n_time accepted: fitness
 * and genotype 96; multienv with 4 environments 95; replicate with 2 / 4 / 8 / 16 replicates 47 / 22 / 9 / 5; multienv_replicate
 * with 16 replicates 4, with 4 replicates and 4 environments 20 ("Limits the reference does not have"). */
int bb_create(const bb_model_desc* model, const bb_advi_opts* opts, bb_handle** out);
void bb_destroy(bb_handle* h);

int64_t bb_num_latents(const bb_handle* h);
/* blocks[0..*n_blocks): one range per `~` block in source order (<= 8). */
int bb_get_layout(const bb_handle* h, bb_block_range* blocks, int32_t* n_blocks);

/* Turing.meanfield initialisation (mu0 = randn(D), sigma0 = softplus.(randn(D)))
 * drawn from the engine's own init streams; resets optimiser state and step. */
int bb_init_meanfield(bb_handle* h);
/* Explicit variational parameters theta = [mu; omega], sigma = softplus(omega);
 * resets optimiser state and step. */
int bb_set_params(bb_handle* h, const double* mu, const double* omega);
int bb_get_params(bb_handle* h, double* mu, double* omega);
/* Genotype model: the reference hands barcodes over in order of appearance (utils.data_to_arrays, src/utils.jl:692-731), so a
 * genotype's mutants are scattered over geno_idx.  The library then groups them itself (stable sort of the mutants by genotype:
 * the resident launch and genotype-aligned shards need consecutive runs), works in that order and presents the CALLER's order at
 * every entry point that takes or returns a latent vector.  Likewise the loglambda block: where n_geno + n_bc is odd it would start at
 * an odd flat index, so internally it sits in front of the theta block (the resident launch's 16-byte pairs stay whole).  caller_index[i] = the caller's flat index of the handle's internal
 * latent i (identity when nothing was regrouped); the engine's normal stream (bb_debug_normals, bb_elbo_grad with eps = NULL,
 * bb_run) is keyed by the INTERNAL index.  caller_index: [bb_num_latents(h)]. */
int bb_get_permutation(bb_handle* h, int64_t* caller_index);
/* Sharded runs: the CALLER's flat indices of the latents this handle owns -- its barcodes' loglambda and per-mutant latents, genotype model:
 * theta of its own genotypes (bb_stats.geno_lo / geno_hi) -- i.e. what a gather of the ranks' posteriors takes from this rank; the
 * replicated global blocks are not listed (every rank holds them).  idx: [bb_num_latents(h)], *n entries are written. */
int bb_get_owned(bb_handle* h, int64_t* idx, int64_t* n);

/* AdvancedVI.optimize!: n_steps iterations of
 *   grad(-ELBO) with S reparameterised samples -> optimiser -> theta -= delta. */
int bb_run(bb_handle* h, int64_t n_steps);
/* After BB_ERR_DEVICE from a resident launch (an exchange timed out: bb_last_error says so) the handle's step counter is the
 * device's, but a step may have been left half-way: with samples_per_step > 1 the gradient sums of the samples already taken are
 * discarded and that step's exchange numbers are issued again.  Re-initialise (bb_init_meanfield / bb_set_params) or set
 * launch_mode = 1 before running on; a retry without either is deterministic but unspecified.  BB_ERR_NONFINITE: the steps were taken. */
/* Same arithmetic, launched eagerly with a HIP event pair around every kernel
 * so that per-kernel durations can be reported (bb_stats.avg_*_ms). */
int bb_run_profiled(bb_handle* h, int64_t n_steps);

/* q.dist.m and q.dist.sigma (= softplus(omega)) -- what utils.advi_to_df reads
 * (src/utils.jl:1060).  With world_size > 1 only this handle's shard (and the
 * replicated global blocks) is meaningful; see bb_get_stats().shard_*. */
int bb_get_posterior(bb_handle* h, double* mean, double* sigma);

/* Deterministic test hook: ELBO estimate and its gradient at theta = [mu; omega]
 * with caller-supplied standard-normal draws eps (S x D row-major; NULL = the
 * Philox stream of the current step).  Does not touch optimiser state. */
int bb_elbo_grad(bb_handle* h, const double* mu, const double* omega, const double* eps,
                 int32_t n_samples, double* elbo, double* grad_mu, double* grad_omega);

/* ---- cross-GPU leg of the resident launch (sharded runs, one process per GPU) ----------------------
 * Without it a sharded run steps with two kernels + one ncclAllReduce per MC sample (bb_comm_init).
 * With it the whole step loop of every rank is ONE launch: group leaders push their moment rows into
 * every rank's INBOX over xGMI (peer-mapped fine-grained memory) and every rank adds the same rows in
 * the same order.  Protocol, on every rank, same order:
 *   bb_p2p_export(h, handle)            this rank's inbox as an IPC handle (BB_P2P_HANDLE_BYTES)
 *   (caller all-gathers the handles, rank-major)
 *   bb_p2p_import(h, handles)           maps the peers' inboxes
 *   bb_p2p_selftest(h, &ok)             tokens through every mapped inbox, bounded wait
 *   (caller ANDs `ok` over the ranks)
 *   bb_p2p_enable(h, all_ok)            non-zero: bb_run uses the resident launch from now on;
 *                                       BB_ERR_UNSUPPORTED if this shard cannot (caller ANDs again and
 *                                       calls bb_p2p_enable(h, 0) everywhere if any rank refused)
 * All ranks must then call bb_run with the same step counts.  No reference counterpart. */
#define BB_P2P_HANDLE_BYTES 64
int bb_p2p_export(bb_handle* h, void* handle_out);
int bb_p2p_import(bb_handle* h, const void* handles);
int bb_p2p_selftest(bb_handle* h, int32_t* ok);
int bb_p2p_enable(bb_handle* h, int32_t on);

/* log p(data, z) of the model (normalisers included) and its gradient at a point z
 * of the flat latent vector -- the `logdensity_and_gradient` service an HMC / NUTS
 * sampler needs (the reference's MCMC entry, src/mcmc.jl:86-160, samples the same
 * Turing model).  logp / grad may be NULL.  Does not touch the variational state.
 * Accuracy: logp is good to a few 2^-53 of the SUM OF THE MAGNITUDES of its addends (R*l, lambda,
 * lgamma(R+1), every quadratic and normaliser), not of |logp|: at posterior-like points of deep
 * data |logp| is orders of magnitude below that sum.
 * On a sharded handle the gradient is this shard's part (global blocks replicated). */
int bb_logdensity_grad(bb_handle* h, const double* z, double* logp, double* grad);

/* The same service for n_points points in one call -- what an ensemble sampler that steps its walkers in lock-step needs
 * (the reference's `ensemble` argument of Turing.sample, src/mcmc.jl:78-82, 151-153).  Kernels of its own (csrc/bb_logp.h)
 * evaluate the log-joint directly at the points, on buffers of the handle's own.
 *  - logp[w] and grad[w] are the model's log-joint, normalisers included, and its gradient at z[w]: the quantities
 *    bb_logdensity_grad documents.  Either output may be NULL.
 *  - They are a function of z[w] alone: bit-identical for every n_points, every slot w, every launch mode the handle was
 *    created with, and whatever else is in the batch.  No atomics: every sum over barcodes or tiles runs in an order fixed
 *    by the model shape and the handle's tile map (a tile's partial sums, then the tiles in tile order).
 *  - The handle's mu, omega, optimiser state, step counter and RNG position are untouched, bitwise: a bb_run after the
 *    call equals one on a fresh handle.
 *  - A point whose log-joint is not finite returns that value (-Inf / NaN) in logp[w]; it is not an error and does not
 *    disturb the other points.
 *  - n_points outside 1 .. BB_LOGP_MAX_BATCH, or a null h / z: BB_ERR_INVALID.
 *  - Sharded handles (world_size > 1) and multi-device handles (n_devices > 1): BB_ERR_UNSUPPORTED.
 * All model kinds run batched, the genotype model included (its theta block in a third launch over genotypes x points);
 * where the handle regrouped a genotype model's mutants, the points and gradients are permuted once per batch on the host. */
#define BB_LOGP_MAX_BATCH 64
int bb_logdensity_grad_batch(bb_handle* h, int32_t n_points, const double* z /* [n_points][D], caller's order */,
                             double* logp /* [n_points] or NULL */, double* grad /* [n_points][D] or NULL */);

/* ---- device-resident HMC trajectories (csrc/bb_hmc.h) ---------------------------------------------------------------------------
 * Hamiltonian Monte Carlo with a diagonal metric and a fixed number of leapfrogs per transition, chosen per walker by the caller.
 * Position, momentum and gradient of every walker stay on the device from bb_hmc_begin to bb_hmc_end; one bb_hmc_step makes one
 * transition of all walkers and brings back scalars only; bb_hmc_get downloads the walkers' positions when a draw is kept.  The NUTS
 * tree of barbay.jl_amd.mcmc.nuts_ensemble stays on the host (bb_logdensity_grad_batch); bb_nuts_* below keeps a tree's vectors beside
 * this session.  No reference counterpart: the reference samples with
 * Turing.NUTS (src/mcmc.jl:86-160).
 *
 * bb_hmc_begin: a session of n_walkers walkers at z0 on a buffer of its own -- a bb_logdensity_grad_batch between two steps does not
 *  disturb a session, nor a session that call.  Per walker the device holds z, g = d log p / d z, logp, the proposal z', g' and the
 *  momentum r, rows of even stride in the handle's latent order.  inv_mass (NULL: ones) and 1 / sqrt(inv_mass) -- both formed on the host,
 *  correctly rounded sqrt, then the division -- are uploaded in that order, and the caller-index map where the handle regrouped
 *  (bb_get_permutation).  logp and g at z0 come from the kernels of bb_logdensity_grad_batch: logp[w] is what that call returns at z0[w],
 *  bit for bit.  A start whose logp is not finite is reported in logp and is not an error.  A second bb_hmc_begin replaces the session;
 *  bb_destroy frees it.
 * bb_hmc_step: one transition of every walker w, in this arithmetic (fma: one rounding):
 *  - momentum: the latent with the CALLER's index i draws n = the normal (i, step = transition, stream = BB_HMC_STREAM0 + w) of the engine's
 *    stream at `seed` (pair q = i >> 1: even i the cosine branch, odd i the sine branch; bb_debug_normals on a handle created with the
 *    same seed returns it), r_i = n * (1 / sqrt(inv_mass_i)), kinetic0 = 0.5 * sum_i inv_mass_i r_i r_i;
 *  - trajectory: half = 0.5 * eps[w]; n_leapfrog[w] times { r = fma(half, g, r); z = fma(eps[w] * inv_mass_i, r, z) with the product rounded
 *    once; logp_prop, g at z; r = fma(half, g, r) };
 *  - kinetic1 as kinetic0 from the final r; h0 = logp - kinetic0, h1 = logp_prop - kinetic1; divergent = h1 is not finite;
 *    accepted = h1 is finite && log_u[w] < h1 - h0, decided on the host side of the call from the downloaded scalars.  An accepted walker's
 *    (z', g', logp_prop) become its state; a rejected walker's state is bitwise what it was.  log_u = +Inf never accepts (a probe),
 *    -Inf accepts whenever h1 is finite.
 *  - order of the sums over i: the handle's latent order cut into chunks of BB_HMC_CHUNK (2048) latents.  Thread t of a chunk's 256 starts at
 *    0.0 and takes latents 2 t + 512 j and 2 t + 512 j + 1 of the chunk, j = 0, 1, ..., as acc = fma(inv_mass_i r_i, r_i, acc); the threads'
 *    sums are folded by halving (p[t] += p[t + s], s = 128, ..., 1); the chunks are added in chunk order onto 0.0; the total is halved.
 *    No atomics.
 *  - a walker whose n_leapfrog is used up takes no part in the further evaluations of the call (its workgroups leave at once).
 *  - independence: a walker's outputs and new state are a function of its own (z, eps, n_leapfrog, log_u), inv_mass, seed, transition and
 *    its session index w alone: bit-identical whatever n_walkers, whatever the other walkers' arguments or a non-finite neighbour,
 *    whatever the handle's launch mode and whatever was called before.  The handle's mu, omega, optimiser state, step counter and RNG
 *    position are untouched, bitwise.
 * bb_hmc_get: the walkers' current z, logp and g, caller's order; bb_hmc_get's logp and grad equal bb_logdensity_grad_batch at its z.
 * bb_hmc_end: closes the session (a second bb_hmc_end: BB_OK); the session's buffer (40 W D bytes) and the accumulators' stay with the handle
 *  until bb_destroy, the NUTS tree's rows (bb_nuts_begin below: up to 7.6 GB) are freed here.
 * Errors: BB_ERR_INVALID -- a null h, o or z0; n_walkers outside 1 .. BB_HMC_MAX_WALKERS; an inv_mass entry that is not finite or not > 0
 *  (the message names its index); an eps that is not finite or not > 0, an n_leapfrog outside 1 .. BB_HMC_MAX_LEAPFROG or a NaN log_u (the
 *  message names the walker); reserved0 != 0; bb_hmc_step or bb_hmc_get without a session, bb_hmc_end on a handle that never had one.  BB_ERR_UNSUPPORTED -- sharded
 *  (world_size > 1) and multi-device (n_devices > 1) handles.  BB_ERR_DEVICE -- the device cannot allocate the session: nothing is kept. */
#define BB_HMC_MAX_WALKERS   BB_LOGP_MAX_BATCH      /* 64 */
#define BB_HMC_MAX_LEAPFROG  1024
#define BB_HMC_STREAM0       0xFFFFFF00u            /* walker w draws on stream BB_HMC_STREAM0 + w; 0xFFFFFF00..3F are used by nothing else */
#define BB_HMC_CHUNK         2048
typedef struct bb_hmc_opts {
    int32_t n_walkers;          /* 1 .. BB_HMC_MAX_WALKERS */
    int32_t reserved0;          /* 0 */
    uint64_t seed;              /* Philox key of the momentum draws */
    const double* inv_mass;     /* [D], caller's order, finite and > 0; NULL: ones */
} bb_hmc_opts;
typedef struct bb_hmc_step_opts {
    uint32_t transition;        /* Philox `step` of this transition's momenta */
    int32_t reserved0;          /* 0 */
    const double* eps;          /* [W] finite, > 0 */
    const int32_t* n_leapfrog;  /* [W] 1 .. BB_HMC_MAX_LEAPFROG */
    const double* log_u;        /* [W]; +Inf: never accept (a probe), -Inf: accept whenever h1 is finite; NaN is invalid */
} bb_hmc_step_opts;
typedef struct bb_hmc_step_out {   /* every pointer may be NULL; [W] */
    double *h0, *h1, *kinetic0, *kinetic1, *logp_prop, *logp;   /* logp: of the state the walker holds AFTER the call */
    int32_t *accepted, *divergent;                               /* divergent: h1 not finite */
} bb_hmc_step_out;
int bb_hmc_begin(bb_handle* h, const bb_hmc_opts* o, const double* z0 /* [W][D] caller's order */, double* logp /* [W] or NULL */);
int bb_hmc_step(bb_handle* h, const bb_hmc_step_opts* o, const bb_hmc_step_out* out /* or NULL */);
int bb_hmc_get(bb_handle* h, double* z /* [W][D] or NULL */, double* logp /* [W] or NULL */, double* grad /* [W][D] or NULL */);
int bb_hmc_end(bb_handle* h);

/* ---- streaming moments of the HMC session and its metric (csrc/bb_hmc_accum.h) ---------------------------------------------------
 * Summaries of the draws and a windowed adaptation of the metric without the draws leaving the device: per walker w and segment
 * s < n_segments the device keeps the running mean and m2 (sum of squared deviations) of the states ADDED to (w, s), two rows of the
 * session's stride in the handle's latent order, in a buffer of their own; the counts n[w][s] stay on the host.  Nothing of size D
 * crosses the host link per draw.  No reference counterpart.
 *
 * bb_hmc_accum_begin: needs a session; allocates and zeroes W x n_segments x 2 rows (and four rows for the statistics); a second call
 *  replaces them.  bb_hmc_begin and bb_hmc_end drop the accumulators; bb_destroy frees the buffer.
 * bb_hmc_accum_add: walker w's CURRENT state x = z[w] goes to segment[w] (-1: this walker is not added), one Welford step per latent with
 *  n the new count of (w, segment[w]) and inv_n = 1.0 / n formed on the host:
 *      d = x - mean;   mean = mean + d * inv_n;   m2 = m2 + d * (x - mean)
 *  every product and sum rounded on its own (no fused multiply-add), so a host restatement is bit-exact.  The pass reads z, mean, m2 and
 *  writes mean, m2 (40 B per latent), on the grid of bb_hmc_step's elementwise kernels.
 * bb_hmc_accum_reset: all counts and rows to zero.   bb_hmc_accum_get: one (walker, segment)'s rows in the caller's order and its count.
 * bb_hmc_accum_stats: over the live chains c = (w, s) with n_c > 0 -- C of them, K = sum n_c, m_c and M2_c their rows -- the device forms,
 *  per latent, every sum onto 0.0 over c in the order w ascending then s ascending, every operation rounded on its own:
 *      mean      = (sum n_c m_c) / K
 *      m2_pooled = (sum M2_c) + (sum n_c ((m_c - mean) (m_c - mean)))
 *      within    = (sum M2_c / (n_c - 1)) / C
 *      between   = (sum (m_c - mbar) (m_c - mbar)) / (C - 1),  mbar = (sum m_c) / C the unweighted mean of the chain means;  0 for C = 1
 *  (a latent whose chains all hold M2_c = 0 and one and the same mean is constant: mean = that value, the other three rows 0 exactly), and
 *  the host side of the call derives, in fp64 with std::sqrt:
 *      sd   = sqrt(m2_pooled / (K - 1))                                  (StatsBase.std of the pooled draws)
 *      rhat = sqrt(var+ / within),  var+ = (Nbar - 1) / Nbar within + between,  Nbar = K / C
 *      mcse = sqrt(between / C)
 *      ess  = min(sd sd / (mcse mcse), K log10 K)
 *  With n_segments = 2 and equal halves these are the pooled mean, the sd and the split-R-hat of bb_chain_summary.  ess is NOT that call's
 *  (Geyer's) estimate: it is a batch-means estimate whose batches are the C chains -- the variance of the chain means against the pooled
 *  variance -- and its own relative error is about sqrt(2 / (C - 1)): with 4 walkers and 2 segments, +-50 %.  It wants chains (segments)
 *  longer than the autocorrelation time and says nothing about mixing inside a segment.  Quantiles cannot be streamed exactly and are
 *  not offered.
 *  One live chain (C = 1): rhat = mcse = ess = NaN.  A constant latent: sd = 0 exactly, rhat = mcse = ess = NaN.  A latent with a
 *  non-finite accumulator: NaN in mean, sd, mcse, ess and rhat of that latent, no other latent disturbed, no error.  `within` and
 *  `between` are the raw rows, for callers who combine sessions.
 * bb_hmc_set_metric: replaces the session's metric in mid-session: inv_mass is validated, turned into 1 / sqrt(inv_mass), permuted and padded
 *  as by bb_hmc_begin (the same code) and uploaded, 2 x the padded D doubles; z, g, logp and the accumulators are untouched.  A step after
 *  it equals the step of a session begun at the same z with that inv_mass.   bb_hmc_get_metric: the session's inv_mass, caller's order.
 *
 * Invariants: a (walker, segment)'s rows are a function of that walker's added states and their order alone -- bit-identical whatever W,
 *  whatever the other walkers' segment arguments and whatever the handle's launch mode (no atomics, no cross-lane sums: a latent is one
 *  lane's).  No call here changes the session's z, g or logp, the later results of bb_hmc_step (bb_hmc_set_metric: but through the
 *  metric), or the handle's mu, omega, optimiser state, step counter and RNG position, bitwise.
 * Errors: BB_ERR_INVALID -- a null argument; no session; no accumulators (bb_hmc_accum_add / reset / get / stats before
 *  bb_hmc_accum_begin, or after a bb_hmc_begin / bb_hmc_end); n_segments outside 1 .. BB_HMC_MAX_SEGMENTS; reserved0 != 0; a segment outside
 *  -1 .. n_segments - 1 (the message names the walker); a walker or segment of bb_hmc_accum_get out of range; bb_hmc_accum_stats with a live
 *  chain of n_c = 1 (the message names walker and segment) or with nothing added; an inv_mass entry that is not finite or not > 0 (the
 *  message names its index).  BB_ERR_UNSUPPORTED -- sharded and multi-device handles, as for bb_hmc_*.  BB_ERR_DEVICE -- the device
 *  cannot allocate the rows: nothing is kept. */
#define BB_HMC_MAX_SEGMENTS 8
typedef struct bb_hmc_accum_opts {
    int32_t n_segments;         /* 1 .. BB_HMC_MAX_SEGMENTS */
    int32_t reserved0;          /* 0 */
} bb_hmc_accum_opts;
typedef struct bb_hmc_accum_out {      /* every pointer may be NULL; [D], caller's order */
    double *mean, *sd, *mcse, *ess, *rhat;
    double *within, *between;          /* the raw rows, for callers who combine sessions */
    int64_t* n_total;                  /* one value: K */
} bb_hmc_accum_out;
int bb_hmc_accum_begin(bb_handle* h, const bb_hmc_accum_opts* o);
int bb_hmc_accum_add(bb_handle* h, const int32_t* segment /* [W]: 0 .. n_segments - 1, or -1 = this walker is not added */);
int bb_hmc_accum_reset(bb_handle* h);
int bb_hmc_accum_get(bb_handle* h, int32_t walker, int32_t segment, double* mean /* [D] or NULL */, double* m2 /* [D] or NULL */, int64_t* n /* or NULL */);
int bb_hmc_accum_stats(bb_handle* h, const bb_hmc_accum_out* out);
int bb_hmc_set_metric(bb_handle* h, const double* inv_mass /* [D] caller's order, finite and > 0; NULL: ones */);
int bb_hmc_get_metric(bb_handle* h, double* inv_mass /* [D] caller's order */);

/* ---- the No-U-Turn tree of an HMC session on the device (csrc/bb_nuts.h) ---------------------------------------------------------
 * Every D-sized object of a NUTS transition (Hoffman & Gelman 2014, algorithm 6) stays on the device, beside the session: both ends of
 * the trajectory, the U-turn checkpoints of an iteratively built subtree, the subtree's candidate and the transition's candidate.  The
 * caller keeps the tree's control flow, per walker, on the scalars a leaf brings back (barbay.jl_amd.mcmc.nuts_device is such a caller).
 * The reference samples with Turing.NUTS (src/mcmc.jl:86-160); it has no counterpart of these calls.
 *
 * bb_nuts_begin: needs a session; allocates and zeroes, in a buffer of its own, 10 + 2 max_depth rows per walker of the session's even
 *  stride, the handle's latent order: the two edges (z, r, g each), the subtree's candidate (z, g), the transition's candidate (z, g),
 *  max_depth checkpoint slots (z, r each) -- 8 (10 + 2 max_depth) D bytes per walker, 7.6 GB for 64 walkers of D = 498 014 at depth
 *  10.  A second call replaces them.  bb_hmc_end drops them AND frees their buffer, the one large thing a session would otherwise leave with the
 *  handle; bb_hmc_begin drops them and keeps the buffer for the next bb_nuts_begin (a handle that never calls bb_hmc_end keeps it until
 *  bb_destroy).
 * bb_nuts_start: a transition begins for the walkers with live[w] != 0: the momentum r and kinetic0 of bb_hmc_step at the same
 *  `transition` (the same normals, products and order of the sum: bit for bit), and (z, r, g) of the session's state written to both
 *  edges.  The session's z, g and logp are not touched.  kinetic0 of a walker that is not live: 0.
 * bb_nuts_leaf: one leapfrog of every walker with dir[w] != 0, e = dir[w] * eps[w] (the eps of bb_nuts_start), fma: one rounding:
 *  - the leaf starts from the edge of side dir[w] where first[w] != 0, else from where the walker's last leaf ended (the travelling rows,
 *    which are the session's proposal rows);
 *  - r = fma(e / 2, g, r); z = fma(e * inv_mass_i, r, z), the product rounded once; logp_leaf and g at z by the kernels of
 *    bb_logdensity_grad_batch; r = fma(e / 2, g, r);
 *  - kinetic = 0.5 * sum_i inv_mass_i r_i r_i in bb_hmc_step's order;
 *  - for j < n_check[w], against the stored point (z_c, r_c) = checkpoint slot check[w][j], or the edge of side -dir[w] for
 *    BB_NUTS_EDGE_OPP:   a[w][j] = sum_i (z_i - z_c,i) * (inv_mass_i * r_c,i),   b[w][j] = sum_i (z_i - z_c,i) * (inv_mass_i * r_i),
 *    the difference and the product each rounded on their own, then acc = fma(difference, product, acc), in the latent order, fold and
 *    chunk order of the kinetic sum (bb_hmc_step above).  No atomics;
 *  - store[w] >= 0: (z, r) of the leaf is written to that checkpoint slot; last[w] != 0: (z, r, g) to the edge of side dir[w].
 *  A walker with dir[w] == 0 takes no part (its workgroups leave at once) and its outputs are 0; so are a, b beyond n_check[w].
 * bb_nuts_take: per walker, the copies its flags ask for, in this order: BB_NUTS_TAKE_LEAF the last leaf's (z, g, logp) becomes the
 *  subtree's candidate; BB_NUTS_TAKE_SUB the subtree's candidate becomes the transition's; BB_NUTS_TAKE_STATE the transition's candidate
 *  becomes the session's z, g and logp -- what bb_hmc_get, bb_hmc_accum_add and the next bb_nuts_start then read.
 * Interleaving: a bb_hmc_step between two transitions is legal (it redraws the travelling rows, so a bb_nuts_start must follow it before
 *  the next leaf); bb_logdensity_grad_batch, bb_hmc_get and the bb_hmc_accum_* calls may come anywhere.
 * Independence: a walker's leaf outputs and rows are a function of its own state, ops, eps, inv_mass, seed, transition and session index
 *  alone: bit-identical whatever n_walkers, the other walkers' ops or a non-finite neighbour, the handle's launch mode and what was
 *  called before.  The handle's mu, omega, optimiser state, step counter and RNG position are untouched, bitwise.
 * Errors: BB_ERR_INVALID -- a null argument; no session; no bb_nuts_begin (or a bb_hmc_begin / bb_hmc_end since); a leaf or a take before
 *  bb_nuts_start; max_depth outside 1 .. BB_NUTS_MAX_DEPTH; reserved0 != 0; and, the message naming the walker: an eps of a live walker
 *  that is not finite or not > 0, a dir outside -1 .. 1, a leaf or take of a walker that was not live, a first leaf without first, a
 *  store outside -1 .. max_depth - 1, an n_check outside 0 .. max_depth + 1, a check that is neither a slot nor BB_NUTS_EDGE_OPP, a slot
 *  both stored and checked in one op, flags beyond the three bits, a take of a candidate that does not exist yet.  BB_ERR_UNSUPPORTED --
 *  sharded and multi-device handles, as for bb_hmc_*.  BB_ERR_DEVICE -- the device cannot allocate the rows: nothing is kept. */
#define BB_NUTS_MAX_DEPTH   10
#define BB_NUTS_EDGE_OPP    (-2)
#define BB_NUTS_TAKE_LEAF   1
#define BB_NUTS_TAKE_SUB    2
#define BB_NUTS_TAKE_STATE  4
typedef struct bb_nuts_opts {
    int32_t max_depth;          /* 1 .. BB_NUTS_MAX_DEPTH: the number of checkpoint slots */
    int32_t reserved0;          /* 0 */
} bb_nuts_opts;
typedef struct bb_nuts_leaf_opts {
    const int32_t* dir;         /* [W] -1, +1; 0: the walker is idle */
    const int32_t* first;       /* [W] != 0: the first leaf of its doubling (start from the edge of side dir) */
    const int32_t* last;        /* [W] != 0: the last leaf of its doubling (becomes the edge of side dir) */
    const int32_t* store;       /* [W] -1, or the checkpoint slot that takes the leaf */
    const int32_t* n_check;     /* [W] 0 .. max_depth + 1 */
    const int32_t* check;       /* [W][BB_NUTS_MAX_DEPTH + 1]: slots, or BB_NUTS_EDGE_OPP */
    int32_t reserved0;          /* 0 */
} bb_nuts_leaf_opts;
typedef struct bb_nuts_leaf_out {      /* every pointer may be NULL */
    double *logp_leaf, *kinetic;       /* [W] */
    double *a, *b;                     /* [W][max_depth + 1] */
} bb_nuts_leaf_out;
int bb_nuts_begin(bb_handle* h, const bb_nuts_opts* o);
int bb_nuts_start(bb_handle* h, uint32_t transition, const double* eps /* [W] */, const int32_t* live /* [W] */, double* kinetic0 /* [W] or NULL */);
int bb_nuts_leaf(bb_handle* h, const bb_nuts_leaf_opts* o, const bb_nuts_leaf_out* out /* or NULL */);
int bb_nuts_take(bb_handle* h, const int32_t* flags /* [W]: BB_NUTS_TAKE_* or 0 */);

/* ELBO estimates recorded by bb_run (elbo_every > 0): values of steps
 * first_step, first_step + elbo_every, ... ; NaN where not recorded/kept. */
int bb_get_elbo_trace(bb_handle* h, int64_t first_step, int64_t n, double* out);

/* `process_hierarchical_samples!` of utils.advi_to_df (src/utils.jl:1284-1343) on the device, for the hierarchical
 * models (genotype, replicate, multienv_replicate): for every unit of the theta_tilde block, n_samples draws of
 * theta + exp(logtau) * theta_tilde from the current mean-field posterior; median (reported by the reference under
 * the column name `mean`) and corrected std.  n_samples <= 16384.  median / std: [bb_hier_units(h)].
 * On a shard of a sharded run (world_size > 1) only the shard's own entries of the parameter arrays are current: pass the gathered
 * vector through bb_set_params first (a multi-device handle, n_devices > 1, does that itself). */
int64_t bb_hier_units(const bb_handle* h);
int bb_hier_fitness(bb_handle* h, int32_t n_samples, uint64_t seed, double* median, double* std);

/* Posterior predictive bands of the log-frequency ratios ln(f_{t+1}/f_t) -- BarBay.stats.logfreq_ratio_popmean_ppc /
 * logfreq_ratio_bc_ppc / logfreq_ratio_multienv_ppc followed by matrix_quantile_range (src/stats.jl:55-1000) -- for every row
 * of the run at once, from the current mean-field posterior N(mu, softplus(omega)).
 *
 * Rows, in the caller's order (bb_ppc_shape: n_rows = n_rep (1 + n_bc), n_steps = max_r T_r - 1):
 *   r < n_rep               population mean of replicate r: N(-sbar_t, exp(logsigmabar_t)) (model_fitness_normal.jl:250-257)
 *   n_rep + r n_bc + m      mutant m (caller's order) in replicate r: N(s_{m,r,env(t+1)} - sbar_t, exp(logsigma_{m,r,env(t+1)})),
 *                           s = s_bc (fitness / multienv) or theta + exp(logtau) theta_tilde (hierarchical kinds, the model's
 *                           own indexing); env(t+1) = env of the later time point (stats.jl:843-852).
 * sbar_t, logsigmabar_t are replicate r's own (no BB_FLAG_RAGGED_METHOD pairing here); steps t >= T_r - 1 of a shorter
 * replicate are NaN.
 *
 * Draws: sample j < n_samples is one joint draw of the posterior; it gets n_ppc predictive draws per (row, step), so every
 * (row, step) column holds K = n_samples n_ppc values.  With N(q, c, s) = bb_normal_pair(seed, q, c, s) (Philox4x32-10 counter
 * (q_lo, q_hi, c, s), Box-Muller; an even index takes the cosine branch, an odd one the sine branch):
 *   parameter draw j of latent i (the CALLER's flat index):  mu_i + sigma_i N(i, j >> 1, 0xFFFFFFE0)
 *   predictive draw k' = j n_ppc + k of (row, t):            N(row | t << 32, k' >> 1, 0xFFFFFFE1)
 * so a parameter draw is shared by every row and step that uses the latent (one row of the reference's sample frame), and
 * nothing depends on the launch geometry, the handle's internal latent order or its device count.
 *
 * Bands: bands[row][t][i][0 / 1] = the (1 - q_i) / 2 and 1 - (1 - q_i) / 2 quantiles of the column, StatsBase.quantile's
 * definition (type 7: h = (K - 1) p, linear between the order statistics floor(h) and floor(h) + 1), exact order statistics.
 * n_outside[row] (may be NULL): finite observed ratios ln(R_{t+1,b} / n_{t+1}) - ln(R_{t,b} / n_t) (both counts > 0, n_t the
 * totals the handle was created with) strictly outside the band of the largest q -- a mutant row counts its barcode's steps,
 * a population-mean row those of every neutral barcode of its replicate.
 *
 * Limits: 1 <= n_quantiles <= 8 and every q in [0, 1], else BB_ERR_INVALID; n_samples, n_ppc >= 1 and 2 <= K <= 16384 (one
 * column in LDS), else BB_ERR_UNSUPPORTED.  At K = 16384 the Monte-Carlo standard error of a 2.5 % quantile is about 0.02
 * predictive standard deviations.  A multi-device handle (n_devices > 1) gathers the posterior onto its first device; a shard
 * of a sharded run (world_size > 1) needs the gathered vector through bb_set_params first, as bb_hier_fitness. */
typedef struct bb_ppc_opts {
    int32_t n_samples;        /* posterior samples j                                   */
    int32_t n_ppc;            /* predictive draws per sample, row and step             */
    int32_t n_quantiles;      /* 1 .. 8                                                */
    int32_t reserved0;
    const double* quantiles;  /* [n_quantiles] band masses q                           */
    uint64_t seed;            /* Philox key                                            */
} bb_ppc_opts;
int bb_ppc_shape(const bb_handle* h, int64_t* n_rows, int32_t* n_steps);
int bb_ppc_bands(bb_handle* h, const bb_ppc_opts* o, double* bands /* [n_rows][n_steps][n_quantiles][2] */,
                 int64_t* n_outside /* [n_rows] or NULL */);

/* Posterior predictive bands of the frequency TRAJECTORIES f_{t+1} = f_t exp(N(s - sbar_t, sigma)) -- BarBay.stats.freq_bc_ppc
 * (src/stats.jl:152-213) followed by matrix_quantile_range -- and the posterior bands of the frequencies the model itself returns,
 * F = Lambda ./ sum(Lambda, dims=2) with Lambda = exp.(logLambda) (src/model_fitness_normal.jl:209-212), for every barcode of the
 * run at once, neutral barcodes included, from the current mean-field posterior.
 *
 * Rows, in the caller's order (bb_freq_shape: n_rows = n_rep (n_neutral + n_bc), n_cols = max_r T_r):
 *   row = r B + b, B = n_neutral + n_bc, b the data column: neutrals first, then the mutants as the caller handed them over (also
 *   where the library regrouped a genotype model).  Columns are TIME POINTS t < T_r, not steps; columns t >= T_r of a shorter
 *   replicate are NaN.
 *
 * Sample j < n_samples is the joint posterior draw of bb_ppc_bands: latent i (the caller's flat index) is
 * mu_i + sigma_i N(i, j >> 1, 0xFFFFFFE0), so at equal seed the two calls share their parameter draws.  Frequency of a draw:
 *   F_{r,t,b,j} = exp(ll_{r,t,b,j}) / Z_{r,t,j},   Z_{r,t,j} = sum_{b' < B} exp(ll_{r,t,b',j}),
 * ll the loglambda latent of (r, t, b) in the layout bb_get_layout reports.  Z is summed in chunks of 256 consecutive data columns,
 * each in index order, the chunk sums then added in chunk order: the order is a function of B alone and nothing depends on the launch
 * geometry, the launch mode, the handle's internal latent order or its device count.
 *
 * BB_FREQ_POSTERIOR:  column t holds the K = n_samples values F_{r,t,b,j}; n_ppc must be 1, else BB_ERR_INVALID.
 * BB_FREQ_TRAJECTORY: K = n_samples n_ppc, k' = j n_ppc + k.  Column 0 is f_0[k'] = F_{r,0,b,j}; column t + 1 is
 *   f_{t+1}[k'] = f_t[k'] exp(mu_j + sd_j N(row | t << 32, k' >> 1, 0xFFFFFFE2)), the product carried in f as the reference multiplies.
 *   A neutral row has mu = -sbar_{r,t}, sd = exp(logsigmabar_{r,t}); a mutant row the (s - sbar_{r,t}, sigma) of its bb_ppc_bands row:
 *   the environment of the later time point, theta + exp(logtau) theta_tilde for the hierarchical kinds.  sbar is replicate r's own
 *   (no BB_FLAG_RAGGED_METHOD pairing, as in bb_ppc_bands).  A trajectory may underflow to 0 or overflow to +Inf; that is reported as
 *   is.  Where the carried product then meets 0 * Inf the value is NaN: it orders above +Inf in its column (as numpy's sort has it),
 *   and the band ends that touch it are NaN by the non-finite rule.
 *
 * Bands: bands[row][t][i][0 / 1] = the (1 - q_i) / 2 and 1 - (1 - q_i) / 2 quantiles of the column; definition, interpolation and
 * non-finite rule as bb_ppc_bands (exact order statistics).  n_outside[row] (may be NULL): the time points t < T_r whose observed
 * frequency R_{t,b} / n_t (zero counts included; n_t the totals the handle was created with) lies strictly outside the band of the
 * largest q.
 *
 * Limits as bb_ppc_bands: 1 <= n_quantiles <= 8 and every q in [0, 1], else BB_ERR_INVALID; n_samples, n_ppc >= 1 and
 * 2 <= K <= 16384, else BB_ERR_UNSUPPORTED; an unknown mode is BB_ERR_INVALID.  A multi-device handle (n_devices > 1) gathers the
 * posterior onto its first device; a shard of a sharded run (world_size > 1) needs the gathered vector through bb_set_params first. */
#define BB_FREQ_TRAJECTORY 0
#define BB_FREQ_POSTERIOR 1
typedef struct bb_freq_opts {
    int32_t mode;             /* BB_FREQ_*                                             */
    int32_t n_samples;        /* posterior samples j                                   */
    int32_t n_ppc;            /* predictive trajectories per sample and row            */
    int32_t n_quantiles;      /* 1 .. 8                                                */
    const double* quantiles;  /* [n_quantiles] band masses q                           */
    uint64_t seed;            /* Philox key                                            */
} bb_freq_opts;
int bb_freq_shape(const bb_handle* h, int64_t* n_rows, int32_t* n_cols);
int bb_freq_bands(bb_handle* h, const bb_freq_opts* o, double* bands /* [n_rows][n_cols][n_quantiles][2] */,
                  int64_t* n_outside /* [n_rows] or NULL */);

/* Predictive log score and probability integral transform (PIT) of every OBSERVED log-frequency ratio, per barcode and step, from
 * the current mean-field posterior -- the per-barcode verdict the bands' n_outside only counts.  No reference counterpart.  The
 * predictive of a step given posterior draw j is N(mu_j, sigma_j), so its density and CDF at the observed ratio are averaged over
 * the draws in closed form: no predictive draws, no selection, no Monte-Carlo error from the predictive layer.
 *
 * Rows (bb_score_shape: n_rows = n_rep (n_neutral + n_bc), n_steps = max_r T_r - 1) are the barcode rows of bb_freq_bands:
 *   row = r B + b, B = n_neutral + n_bc, b the data column: neutrals first, then the mutants as the caller handed them over (also
 *   where the library regrouped a genotype model).  Cells t >= T_r - 1 of a shorter replicate are NaN in every output.
 *
 * Cell (row, t).  Observed ratio y = ln(R_{t+1,b} / n_{t+1}) - ln(R_{t,b} / n_t), formed once on the host as bb_ppc_bands forms it
 * for n_outside; where either count is 0 the cell is unscored and every output of the cell is NaN.  Per-draw parameters, j < n_samples:
 *   a neutral barcode has (mu_j, sigma_j) = (-sbar_{r,t,j}, exp(logsigmabar_{r,t,j}));
 *   a mutant exactly the (s - sbar_t, sigma) of its bb_ppc_bands row n_rep + r n_bc + m: the environment of the later time point,
 *   theta + exp(logtau) theta_tilde for the hierarchical kinds.
 * Draw j of latent i (the caller's flat index) is mu_i + sigma_i N(i, j >> 1, 0xFFFFFFE0), the draw of bb_ppc_bands: at equal seed
 * the three post-fit calls share their joint draws.  With z_j = (y - mu_j) / sigma_j, l_j = -z_j^2 / 2 - ln sigma_j - ln(2 pi) / 2
 * and n = n_samples:
 *   observed   y, the value that was scored
 *   pred_mean  mean_j mu_j
 *   pred_sd    sqrt(mean_j sigma_j^2 + mean_j (mu_j - pred_mean)^2), two-pass and centred
 *   lpd        the log predictive density  m + ln sum_j exp(l_j - m) - ln n,  m = max_j l_j
 *   p_waic     sum_j (l_j - lbar)^2 / (n - 1), lbar = mean_j l_j, two-pass and centred (the cell's term of WAIC's penalty)
 *   pit        mean_j erfc(-z_j / sqrt 2) / 2, the predictive CDF at y
 *   pit_upper  mean_j erfc( z_j / sqrt 2) / 2, the upper tail; both through erfc, never as 1 - the other: each keeps its relative
 *              accuracy where it is tiny, and a calibrated predictive has both uniform on (0, 1)
 * Per row: row_lpd and row_p_waic are the sums over the row's scored cells in step order, n_scored their number.
 * Non-finite parameters propagate by IEEE rules into the cells that use them (a NaN l_j makes m, and with it lpd, NaN); that is
 * not an error and disturbs no other cell.
 *
 * A cell's results are a function of y, the handle's (mu, sigma), n_samples and seed alone: every sum runs in an order fixed by
 * n_samples, bit-identical whatever the grid, the launch mode, the handle's internal latent order, the device count or the calls
 * made on the handle before; no atomics on doubles.  The handle's mu, omega, optimiser state, step counter and RNG position are
 * untouched, bitwise.  BB_ERR_INVALID: a null h, o or out; BB_ERR_UNSUPPORTED: n_samples outside 2 .. BB_SCORE_MAX_SAMPLES (a
 * step's log densities in LDS).  A multi-device handle (n_devices > 1) gathers the posterior onto its first device; a shard of a
 * sharded run (world_size > 1) needs the gathered vector through bb_set_params first, as bb_ppc_bands. */
#define BB_SCORE_MAX_SAMPLES 16384
typedef struct bb_score_opts {
    int32_t n_samples;        /* posterior samples j, 2 .. BB_SCORE_MAX_SAMPLES        */
    int32_t reserved0;
    uint64_t seed;            /* Philox key                                            */
} bb_score_opts;
typedef struct bb_score_out {     /* every pointer may be NULL                         */
    double *observed, *pred_mean, *pred_sd, *lpd, *p_waic, *pit, *pit_upper;      /* [n_rows][n_steps] */
    double *row_lpd, *row_p_waic;    /* [n_rows]                                       */
    int32_t* n_scored;        /* [n_rows]                                              */
} bb_score_out;
int bb_score_shape(const bb_handle* h, int64_t* n_rows, int32_t* n_steps);
int bb_ppc_score(bb_handle* h, const bb_score_opts* o, const bb_score_out* out);

/* Pareto-smoothed importance-sampling leave-one-out (PSIS-LOO) predictive scores of the observed log-frequency ratios: what the
 * fit would have predicted for an observation had it not seen it, and a diagnostic khat per observation that says where that
 * estimate (and the fit) leans on one observation too hard -- which bb_ppc_score's in-sample lpd and p_waic cannot tell.  Vehtari,
 * Gelman, Gabry 2017; Vehtari et al. 2024; the generalised Pareto fit is Zhang and Stephens 2009, as the loo package's gpdfit.  No
 * reference counterpart.
 *
 * Rows, steps (bb_loo_shape == bb_score_shape), observed ratios y, draws j < n = n_samples and the log densities l_j of a scored
 * cell are exactly bb_ppc_score's; an unscored cell is NaN in every output.  At equal seed and n_samples lpd is bb_ppc_score's
 * lpd, byte for byte.
 *
 * PSIS(l), l_j finite:
 *   1  a_j = -l_j, A = max_j a_j, r_j = a_j - A <= 0.
 *   2  M = min(floor(n / 5), c), c the smallest integer with c^2 >= 9 n (ceil(3 sqrt n) in integers; r_eff = 1: q's draws are
 *      independent).
 *   3  The draws ordered by (r_j, j) ascending: rho_1 <= ... <= rho_M the M largest, c the largest not among them (order
 *      statistic n - M).
 *   4  The tail is smoothed iff M >= 5 and c >= -690 and x* > 0, where x_i = exp(rho_i) - exp(c), x* = x_{floor(M / 4 + 1 / 2)}
 *      (= x_{(M + 2) / 4} in integers).  Otherwise the weights stay raw and khat = +Inf.  (-690 keeps the decision off exp's
 *      underflow: a 50-digit evaluation and a double decide alike.)
 *   5  m = 30 + floor(sqrt M);  theta_i = 1 / x_M + (1 - sqrt(m / (i - 1/2))) / (3 x*), i = 1 .. m;
 *      kappa(theta) = (sum_{k = 1 .. M} log1p(-theta x_k)) / M;  L_i = M ((log(-theta_i / kappa(theta_i)) - kappa(theta_i)) - 1);
 *      w_i = 1 / sum_{j = 1 .. m} exp(L_j - L_i);  theta^ = sum_i theta_i w_i;  k_raw = kappa(theta^);  sigma^ = -k_raw / theta^;
 *      khat = (M k_raw + 5) / (M + 10).
 *   6  The draw of tail rank i gets lw = min(log(sigma^ expm1(-khat log1p(-p_i)) / khat + exp(c)), 0), p_i = (i - 1/2) / M (the
 *      minimum as "v > 0 ? 0 : v": a NaN stays); every other draw keeps lw_j = r_j.
 *   7  elpd_loo = LSE_j(lw_j + l_j) - LSE_j(lw_j), LSE(v) = max v + log sum_j exp(v_j - max v);
 *      n_eff = 1 / sum_j wt_j^2, wt_j = exp(lw_j - LSE(lw));  lpd = LSE(l) - log n as bb_ppc_score forms it;
 *      p_loo = lpd - elpd_loo;  khat.
 *   8  A non-finite l_j makes elpd_loo, p_loo, khat and n_eff of that cell NaN and disturbs no other cell; lpd is then what
 *      bb_ppc_score gives (NaN where an l_j is NaN or +Inf).  Anything else non-finite inside the fit propagates by IEEE rules.
 * Order of the sums: every sum and maximum over j in bb_ppc_score's reduction order; every sum over the tail (k) or the theta grid
 * (i, j) starts from its first term and adds the others in ascending index.  No atomics on doubles.
 *
 * Per cell (one observation left out), [n_rows][n_steps]: elpd_loo, p_loo, khat, n_eff, lpd = PSIS of the cell's l.
 * Per row (a barcode's whole trajectory left out), [n_rows]: row_elpd_loo, row_p_loo, row_khat, row_n_eff = PSIS of
 *   l^row_j = the sum over the row's scored steps, in step order, of l_{t,j} (row_p_loo against the log-mean-exp of l^row) -- "would
 *   the model have predicted this lineage?", the number model comparison should sum; row_elpd_cells = the sum of the cells'
 *   elpd_loo in step order; row_khat_max = the largest of the cells' khat (a NaN stays); n_scored.  A row without a scored cell has
 *   NaN in all six and n_scored = 0; a row with one scored cell has row_* equal to that cell's, byte for byte.
 *
 * Results are a function of y, the handle's (mu, sigma), n_samples and seed alone, bit-identical whatever the grid, the launch mode,
 * the handle's internal latent order, the device count or the calls made on the handle before.  The handle's mu, omega, optimiser
 * state, step counter and RNG position are untouched, bitwise.  BB_ERR_INVALID: a null h, o or out; BB_ERR_UNSUPPORTED: n_samples
 * outside 2 .. BB_LOO_MAX_SAMPLES (a cell's l and lw both in LDS: half of bb_ppc_score's cap).  Multi-device and sharded handles as
 * bb_ppc_score. */
#define BB_LOO_MAX_SAMPLES 8192
typedef struct bb_loo_opts {
    int32_t n_samples;        /* posterior samples j, 2 .. BB_LOO_MAX_SAMPLES          */
    int32_t reserved0;
    uint64_t seed;            /* Philox key                                            */
} bb_loo_opts;
typedef struct bb_loo_out {       /* every pointer may be NULL                         */
    double *elpd_loo, *p_loo, *khat, *n_eff, *lpd;                                /* [n_rows][n_steps] */
    double *row_elpd_loo, *row_p_loo, *row_khat, *row_n_eff, *row_elpd_cells, *row_khat_max;      /* [n_rows] */
    int32_t* n_scored;        /* [n_rows]                                              */
} bb_loo_out;
int bb_loo_shape(const bb_handle* h, int64_t* n_rows, int32_t* n_steps);
int bb_ppc_loo(bb_handle* h, const bb_loo_opts* o, const bb_loo_out* out);

/* Rao-Blackwellised (RB) marginals of the mutants' fitness -- how far the "+-" of the mean-field posterior can be trusted, per
 * mutant.  No reference counterpart.  Given everything else, a mutant's fitness enters the log-joint only through a Gaussian prior
 * and Gaussian log-frequency-ratio terms (model_fitness_normal.jl:262-270 and its four siblings), so its full conditional is
 * exactly N(m, sd) in all five model kinds.  Averaging that conditional over joint draws of everything else gives the RB marginal:
 * one exact Gibbs half-step away from q.  Were q the true posterior the RB marginal would equal q's own; where mean-field has cut
 * the coupling of a fitness to its loglambda row, sbar_t, logsigma, theta and tau, the RB marginal has that uncertainty back in it,
 * and rb_sd / q_sd says by how much.  Given the draws of an MCMC chain instead, the same call Rao-Blackwellises the chain's
 * fitness estimates.
 *
 * Units (bb_fitness_rb_shape: n_units): u = (r, m, e), replicate, mutant in the caller's order, environment, numbered in the order
 * of the caller's s_bc block (kinds FITNESS, MULTIENV) or theta_tilde block (hierarchical kinds): u = e + E m + E n_bc r, E = n_env
 * for the multi-environment kinds and 1 otherwise; the genotype model has u = m (the order of bb_hier_fitness).  The steps of a
 * unit are T_u = { t < T_r - 1 : env_r(t + 1) = e } (the later time point's environment, as in bb_ppc_bands), n_u their number.
 *
 * Per draw j < n = n_samples, with ll the loglambda draw of (r, t, b), b = n_neutral + m, and Z_{r,t,j} = sum_b' exp(ll_{r,t,b',j})
 * summed by bb_freq_bands' rule (chunks of 256 consecutive data columns in index order, then the chunks in chunk order):
 *   gamma_{t,j} = (ll_{r,t+1,b,j} - ll_{r,t,b,j}) - (ln Z_{r,t+1,j} - ln Z_{r,t,j})
 *   y_j  = sum_{t in T_u} (gamma_{t,j} + sbar_{r,t,j}), in ascending t
 *   w_j  = exp(-2 logsigma_{u,j}), logsigma_u the unit's logsigma_bc entry
 *   (a_j, b_j), the prior of s_u given the rest: FITNESS, MULTIENV: the s_bc prior (mean, std) of the element as the handle holds
 *          it (Vector or Matrix form; the handle holds 1 / std^2, which is what enters below), the same for every draw;
 *          hierarchical kinds: (theta_j, exp(logtau_{u,j})), theta the unit's hyper-fitness: theta[geno_idx[m]] for the genotype
 *          model, theta[e + E m] for the replicate kinds
 *   P_j  = 1 / b_j^2 + n_u w_j;   m_j = (a_j / b_j^2 + w_j y_j) / P_j;   sd_j = 1 / sqrt(P_j)
 *   s_j  = the unit's fitness in draw j: the s_bc draw, or theta_j + exp(logtau_j) theta_tilde_j.
 * A unit with n_u = 0 (an environment that never occurs as a later time point) has the prior as its conditional: m_j = a_j and
 * sd_j = b_j, taken as they are (for the s_bc prior: 1 / sqrt(1 / std^2)).
 * The identity all this rests on, at any point z:  P (m - s_u) = dlogp/ds_u (FITNESS, MULTIENV);  exp(logtau_u) P (m - s_u) =
 * dlogp/dtheta_tilde_u (hierarchical kinds).  BB_FLAG_RAGGED_METHOD alters the neutral term only, so flagged handles are served alike.
 *
 * Outputs per unit (every pointer may be NULL):
 *   n_steps    n_u
 *   q_mean, q_sd     mean and sd of s_j over the draws: two-pass, centred, divisor n
 *   rb_mean    mean_j m_j
 *   rb_sd      sqrt(mean_j sd_j^2 + mean_j (m_j - rb_mean)^2), two-pass and centred
 *   p_pos      mean_j erfc(-(m_j - s0) / (sd_j sqrt 2)) / 2, the RB probability of s_u > s0 = threshold
 *   p_neg      mean_j erfc(+(m_j - s0) / (sd_j sqrt 2)) / 2; both through erfc, never as 1 - the other (bb_ppc_score's rule)
 *   quantiles  quantiles[u][i], the probs[i] quantile of the mixture F(x) = mean_j erfc(-(x - m_j) / (sd_j sqrt 2)) / 2 by
 *              bisection: lo = min_j m_j - 40 max_j sd_j, hi = max_j m_j + 40 max_j sd_j; 64 times x = lo + (hi - lo) / 2,
 *              F(x) < p ? lo = x : hi = x; the result is the last bracket's midpoint.  A unit with a non-finite m_j or sd_j reports
 *              NaN quantiles.
 * Non-finite parameters propagate by IEEE rules into the units that use them; they disturb no other unit and are not an error.
 *
 * Draws.  draws == NULL: the joint draw of bb_ppc_bands, latent i (the caller's flat index) = mu_i + sigma_i N(i, j >> 1,
 * 0xFFFFFFE0): at equal seed all four post-fit calls share their draws; n_samples in 2 .. BB_RB_MAX_SAMPLES.  draws != NULL: a host
 * array [n_samples][D] in the caller's order (an MCMC chain, say), uploaded whole and read in place of the Philox draw; n_samples
 * in 1 .. BB_RB_MAX_SAMPLES, and with n_samples = 1 the outputs are the conditional at that point (rb_mean = m, rb_sd = sd).  What
 * the device cannot allocate is BB_ERR_DEVICE, and nothing is computed.  This path is no hot path: a latent's draws lie D doubles
 * apart and are read with that stride.  BB_RB_MAX_SAMPLES is the largest count for which a unit's (m_j, sd_j) and the reductions'
 * partials fit the 160 KiB of LDS (derived next to the layout, csrc/bb_rb.h).
 *
 * A unit's results are a function of the handle's (mu, sigma) (or the supplied draws), the s_bc priors, n_samples, seed, threshold
 * and probs: bit-identical whatever the grid, the launch mode, the handle's internal latent order, the device count, n_units or
 * the calls made before.  No atomics on doubles; every sum over the draws runs in bb_ppc_score's order.  The handle's mu, omega,
 * optimiser state, step counter and RNG position are untouched, bitwise.  BB_ERR_INVALID: a null h, o or out; n_quantiles outside
 * 0 .. 8; probs null with n_quantiles > 0; a prob outside (0, 1) or NaN; a non-finite threshold.  BB_ERR_UNSUPPORTED: n_samples
 * outside its range.  Multi-device and sharded handles: as bb_ppc_bands (the first device works on the gathered posterior; a shard
 * needs bb_set_params first).
 * The conditional of theta, the hyper-fitness of the hierarchical kinds: bb_theta_rb, below; that of the population mean fitness
 * sbar_t: bb_popmean_rb, below that; those of logsigma_bc and logsigma_pop: bb_logsigma_rb; that of logtau: bb_logtau_rb; that of
 * loglambda: bb_loglambda_rb.  Out of scope: any change to what the fit or an MCMC run report by default. */
#define BB_RB_MAX_SAMPLES 8672
typedef struct bb_rb_opts {
    int32_t n_samples;        /* draws j, 2 (1 with draws) .. BB_RB_MAX_SAMPLES        */
    int32_t n_quantiles;      /* 0 .. 8                                                */
    const double* probs;      /* [n_quantiles] probabilities in (0, 1)                 */
    double threshold;         /* s0 of p_pos / p_neg                                   */
    uint64_t seed;            /* Philox key (draws == NULL)                            */
    const double* draws;      /* host, [n_samples][D] in the caller's order, or NULL   */
} bb_rb_opts;
typedef struct bb_rb_out {        /* every pointer may be NULL; [n_units] unless noted */
    double *q_mean, *q_sd, *rb_mean, *rb_sd, *p_pos, *p_neg;
    double* quantiles;        /* [n_units][n_quantiles]                                */
    int32_t* n_steps;         /* n_u                                                   */
} bb_rb_out;
int bb_fitness_rb_shape(const bb_handle* h, int64_t* n_units);
int bb_fitness_rb(bb_handle* h, const bb_rb_opts* o, const bb_rb_out* out);

/* Rao-Blackwellised marginals of the hyper-fitness theta -- the fitness of a genotype (BB_MODEL_GENOTYPE) or of a mutant across its
 * replicates (BB_MODEL_REPLICATE, BB_MODEL_MULTIENV_REPLICATE): the number a hierarchical fit is made for, and the one whose
 * mean-field "+-" is least to be trusted, since q factorises theta_g away from the theta_tilde, logtau and logsigma of every member
 * and from their loglambda rows and sbar_t.  No reference counterpart.  The models are non-centred, s_u = theta_g(u) +
 * exp(logtau_u) theta_tilde_u: theta_g enters the log-joint through its Gaussian prior (s_bc_prior, Vector or Matrix form) and,
 * linearly, through the Gaussian log-frequency-ratio terms of its members, so its full conditional given everything else is
 * N(m, sd) in closed form, and bb_fitness_rb's averaging over joint draws applies as it stands.
 *
 * Groups (bb_theta_rb_shape: n_groups = the length of the caller's theta block; 0 for BB_MODEL_FITNESS / BB_MODEL_MULTIENV):
 *   BB_MODEL_GENOTYPE: g is the genotype; its members are the mutants m with geno_idx[m] == g in ascending caller's m; a member's
 *          unit (bb_fitness_rb's numbering) is u = m.
 *   BB_MODEL_REPLICATE / _MULTIENV_REPLICATE: g = e + E m, the theta block's own order; its members are the replicates
 *          r = 0 .. n_rep - 1, ascending; a member's unit is u = g + E n_bc r.
 *
 * Per draw j and member with unit u: n_u, y_{u,j} and w_{u,j} = exp(-2 logsigma_{u,j}) are exactly bb_fitness_rb's (the same gamma,
 * the same ln Z by the 256-column rule, ascending t, the later time point's environment).  With tau = exp(logtau_{u,j}) and
 * theta_tilde_{u,j}:
 *   cP = n_u w;   cN = w (y - n_u (tau theta_tilde))
 * A member with n_u = 0 is skipped, not multiplied by zero: the log-joint has no term for it, and a non-finite logsigma of such a
 * member does not reach the group.
 * Order of the sums: a group's members are cut into chunks of BB_THETA_RB_CHUNK consecutive members; a chunk's (SP, SN) start at 0.0
 * and take their members' (cP, cN) in order; the group's (SP_j, SN_j) start at 0.0 and take the chunks in chunk order.  No atomics
 * on doubles.
 * Conditional, with (a, 1 / b^2) the s_bc_prior element of theta[g] as the handle holds it (the same for every draw):
 *   P_j = 1 / b^2 + SP_j;   m_j = (a / b^2 + SN_j) / P_j;   sd_j = 1 / sqrt(P_j)
 * A group with no contributing member (none, or every n_u = 0) has the prior as its conditional: m_j = a, sd_j = 1 / sqrt(1 / b^2)
 * (bb_fitness_rb's n_u = 0 rule).  theta_j is the draw of theta[g] itself.
 * The identity all this rests on, at any point z:  P (m - theta_g) = dlogp/dtheta_g.  BB_FLAG_RAGGED_METHOD alters the neutral term
 * only, so flagged handles are served alike.
 *
 * Outputs per group (every pointer may be NULL):
 *   n_members  the members of the group;   n_steps  the sum of n_u over them
 *   q_mean, q_sd     mean and sd of theta_j over the draws, as bb_fitness_rb's of s_j
 *   rb_mean, rb_sd, p_pos, p_neg, quantiles    from (m_j, sd_j) by bb_fitness_rb's formulas word for word, the 64-step bisection
 *              and its bracket included; a group with a non-finite m_j or sd_j reports NaN quantiles.
 * Non-finite parameters propagate by IEEE rules into the groups that use them; they disturb no other group and are not an error.
 *
 * The options are bb_fitness_rb's, with the same meaning and limits (draws, seed and keying included; BB_RB_MAX_SAMPLES because a
 * group's (m_j, sd_j) live in LDS as a unit's do).  A group's results are a function of the handle's (mu, sigma) (or the supplied
 * draws), the s_bc prior, geno_idx, n_samples, seed, threshold and probs: bit-identical whatever the grid, the launch mode, the
 * handle's internal latent order (the library regroups a genotype model's mutants), the device count or the calls made before.
 * The handle's mu, omega, optimiser state, step counter and RNG position are untouched, bitwise.  BB_ERR_INVALID /
 * BB_ERR_UNSUPPORTED for the options exactly as bb_fitness_rb; BB_ERR_UNSUPPORTED, the message naming the model kind, for
 * BB_MODEL_FITNESS / BB_MODEL_MULTIENV.  The chunk partials [chunks][2][n_samples] of the groups in flight are bounded to 256 MiB
 * (the groups are worked in slabs; a single group is worked whole).  Multi-device and sharded handles: as bb_ppc_bands.
 * The conditionals of logsigma: bb_logsigma_rb; of logtau: bb_logtau_rb. */
#define BB_THETA_RB_CHUNK 64
typedef struct bb_theta_rb_out {  /* every pointer may be NULL; [n_groups] unless noted */
    double *q_mean, *q_sd, *rb_mean, *rb_sd, *p_pos, *p_neg;
    double* quantiles;            /* [n_groups][n_quantiles]                           */
    int32_t* n_members;           /* members of the group                              */
    int32_t* n_steps;             /* sum of n_u over the members                       */
} bb_theta_rb_out;
int bb_theta_rb_shape(const bb_handle* h, int64_t* n_groups);
int bb_theta_rb(bb_handle* h, const bb_rb_opts* o, const bb_theta_rb_out* out);

/* Rao-Blackwellised marginals of linear contrasts of fitnesses -- the number a barcode experiment is run for: is mutant m fitter in
 * environment B than in A, is genotype g fitter than the wild type, do two replicates agree, is one lineage fitter than another on
 * average.  No reference counterpart.  A contrast cannot be had from two marginals by adding their variances: every fitness of a
 * replicate is measured against the same population mean sbar_t, whose uncertainty each marginal carries (bb_fitness_rb's sd_ratio)
 * and which cancels, draw by draw, in a difference of two mutants of one replicate -- and adds up in their sum.
 *
 * The fact it rests on.  Given everything else a fitness unit enters the log-joint through its own prior and its own
 * log-frequency-ratio terms only; no term holds two units.  The joint full conditional of distinct units is therefore the product of
 * bb_fitness_rb's N(m_{u,j}, sd_{u,j}) (its n_u = 0 rule and the hierarchical kinds' N(theta_j, tau_j) prior included), and the same
 * holds for distinct groups of bb_theta_rb, whose conditional never reads another theta.  A unit and the theta of its own group
 * are NOT conditionally independent: one call serves one space.
 *
 * Spaces: BB_CONTRAST_FITNESS -- the terms name units u of bb_fitness_rb (0 .. n_units - 1, every model kind);
 * BB_CONTRAST_THETA -- groups g of bb_theta_rb (0 .. n_groups - 1, the hierarchical kinds).
 * Contrasts: CSR.  Contrast c has the terms k = term_ptr[c] .. term_ptr[c + 1] - 1, element term_idx[k] with weight term_w[k]; at
 * least one term, every element named at most once per contrast (a repeated element would make V below wrong), finite weights.
 *
 * Per draw j, a term's (s_{k,j}, m_{k,j}, sd_{k,j}) are exactly those of bb_fitness_rb / bb_theta_rb for that unit / group: the same
 * gamma, the same ln Z by the 256-column rule, ascending t, the later time point's environment, the n_u = 0 rule; for theta the
 * members in chunks of BB_THETA_RB_CHUNK, a chunk's (SP, SN) from 0.0 in member order, the chunks from 0.0 in chunk order, members
 * with n_u = 0 skipped.  Then, each sum starting at 0.0 and taking the contrast's terms in the caller's order:
 *   d_j = sum_k w_k s_{k,j}              the draw's own value of the contrast
 *   M_j = sum_k w_k m_{k,j}
 *   V_j = sum_k (w_k sd_{k,j}) (w_k sd_{k,j});   sd_j = sqrt(V_j)
 * (the term values are w * s, w * m and (w * sd) * (w * sd), as written).  The conditional of the contrast is exactly N(M_j, sd_j).
 *
 * Outputs per contrast (every pointer may be NULL), bb_fitness_rb's read for the contrast:
 *   min_steps  the smallest n_u (THETA: group n_steps) over the terms; 0: some term's conditional is its prior
 *   q_mean, q_sd     mean and sd of d_j over the draws: two-pass, centred, divisor n
 *   rb_mean, rb_sd, p_pos, p_neg, quantiles    from (M_j, sd_j) by bb_fitness_rb's formulas word for word, the 64-step bisection,
 *              its bracket and its NaN rule included.  A one-term contrast of weight 1.0 differs from the unit's own marginal only
 *              by sqrt(sd * sd) in place of sd: an ulp at most.
 * Non-finite parameters propagate by IEEE rules into the contrasts that name a unit or group that uses them; they disturb no other
 * contrast and are not an error.
 *
 * Options: n_samples, n_quantiles, probs, threshold, seed and draws are bb_rb_opts' exactly (the keying included: at equal seed the
 * draws are bb_fitness_rb's; n_samples = 1 is allowed with draws; BB_RB_MAX_SAMPLES because (M_j, sd_j) live in LDS).
 *
 * Cost.  One workgroup per contrast; nothing is shared between contrasts.  A FITNESS term walks its unit's loglambda row once per
 * draw.  A THETA term re-walks the rows of its whole group once per draw, for every contrast that names it: fine for "every
 * genotype against a reference" (the reference is walked once per contrast), quadratic for "all pairs" of a thousand genotypes.
 *
 * A contrast's results are a function of the handle's (mu, sigma) (or the supplied draws), the priors, geno_idx, n_samples, seed,
 * threshold, probs and that contrast's own terms in their order: bit-identical whatever the grid, the launch mode, the other
 * contrasts of the call, their number or their order, the device count or the calls made before.  (Permuting the terms within a
 * contrast reorders three floating-point sums and may change low bits.)  No atomics on doubles.  The handle's mu, omega, optimiser
 * state, step counter and RNG position are untouched, bitwise.
 * BB_ERR_INVALID: a null h, o or out; the option errors of bb_fitness_rb; an unknown space; n_contrasts < 0; with n_contrasts > 0 a
 * null term_ptr, term_idx or term_w, term_ptr[0] != 0 or a decreasing term_ptr, a contrast without terms, an index outside the
 * space, an element named twice in one contrast, a non-finite weight.  BB_ERR_UNSUPPORTED: n_samples outside its range;
 * BB_CONTRAST_THETA on BB_MODEL_FITNESS / BB_MODEL_MULTIENV; more than 2^31 - 1 terms.  The message (bb_last_error) names the
 * contrast and the term within it, both 0-based.  n_contrasts == 0 is BB_OK and computes nothing.  Multi-device and sharded
 * handles: as bb_ppc_bands.  Out of scope: contrasts that mix the spaces, or over sbar, logsigma, logtau or loglambda. */
#define BB_CONTRAST_FITNESS 0   /* terms index bb_fitness_rb's units  */
#define BB_CONTRAST_THETA   1   /* terms index bb_theta_rb's groups   */
typedef struct bb_contrast_opts {
    int32_t space;            /* BB_CONTRAST_FITNESS or BB_CONTRAST_THETA              */
    int32_t n_samples;        /* draws j, 2 (1 with draws) .. BB_RB_MAX_SAMPLES        */
    int32_t n_quantiles;      /* 0 .. 8                                                */
    int32_t reserved0;
    const double* probs;      /* [n_quantiles] probabilities in (0, 1)                 */
    double threshold;         /* s0 of p_pos / p_neg                                   */
    uint64_t seed;            /* Philox key (draws == NULL)                            */
    const double* draws;      /* host, [n_samples][D] in the caller's order, or NULL   */
    int64_t n_contrasts;
    const int64_t* term_ptr;  /* [n_contrasts + 1], CSR, term_ptr[0] == 0, non-decreasing */
    const int64_t* term_idx;  /* [term_ptr[n_contrasts]] unit / group numbers          */
    const double* term_w;     /* [term_ptr[n_contrasts]] weights                       */
} bb_contrast_opts;
typedef struct bb_contrast_out {  /* every pointer may be NULL; [n_contrasts] unless noted */
    double *q_mean, *q_sd, *rb_mean, *rb_sd, *p_pos, *p_neg;
    double* quantiles;        /* [n_contrasts][n_quantiles]                            */
    int32_t* min_steps;       /* smallest n_u (THETA: group n_steps) over the terms    */
} bb_contrast_out;
int bb_contrast_rb(bb_handle* h, const bb_contrast_opts* o, const bb_contrast_out* out);

/* Posterior of the distribution of fitness effects (DFE) of a set of fitness units -- the population-level answer a barcode
 * experiment is run for: which fraction of a library, an environment, a replicate or a genotype class lies below (above) a fitness
 * x, and how sure we are of that curve.  No reference counterpart.  It cannot be had from the per-unit marginals: every fitness of
 * a replicate is measured against the same sbar_t, whose uncertainty moves the whole curve left or right together, and mean-field
 * q has cut exactly that coupling.  This is bb_contrast_rb's argument on the other side: there the common mode cancels, here it
 * adds up over the units of the set.
 *
 * The fact it rests on is bb_contrast_rb's: given everything else, distinct fitness units are conditionally independent, each
 * N(m_{u,j}, sd_{u,j}).  Given draw j of the rest, the number of a set's n units at or below x is therefore Poisson-binomial with
 * mean n L_j and variance n^2 V_j (below), and by the law of total variance the posterior variance of the FRACTION below x is
 * between_sd^2 + within_sd^2: what the units share (between the draws) and what each unit's own conditional leaves open (within).
 *
 * Sets: CSR.  Set c names the units set_idx[set_ptr[c] .. set_ptr[c + 1]) in bb_fitness_rb's numbering (every model kind); at
 * least one unit, every unit at most once per set (a repeated unit is not independent of itself: V_j would be wrong).
 * Grid: n_grid (1 .. BB_DFE_MAX_GRID) finite, strictly ascending thresholds x_g.
 *
 * Per draw j, a unit's (s_{u,j}, m_{u,j}, sd_{u,j}) are exactly bb_fitness_rb's: the same gamma, the same ln Z by the 256-column
 * rule, ascending t, the later time point's environment, the n_u = 0 rule, the hierarchical kinds' N(theta_j, tau_j) prior.  Then,
 * bb_fitness_rb's tails word for word, both through erfc:
 *   v = (m - x_g) / sd * rsqrt2;   pl = 0.5 erfc(v);   pu = 0.5 erfc(-v);   c = (s <= x_g)
 * Order of the sums: the set's units, in the caller's order, are cut into chunks of BB_DFE_CHUNK.  A chunk's (SL, SU, SV, SC)
 * start at 0.0 and take their units' pl, pu, pl pu and c in order (SV = fma(pl, pu, SV): the product is not rounded on its own);
 * the set's sums start at 0.0 and take the chunks in chunk order.  With n the set's size:
 *   L_j = SL / n    U_j = SU / n    V_j = SV / (n n)    C_j = SC / n
 * Outputs per (set, grid point), every sum over j in bb_ppc_score's reduction order, divisor n_samples:
 *   below_mean, above_mean   mean_j L_j, mean_j U_j: the posterior mean of the fraction at or below (above) x_g
 *   between_sd               sqrt(mean_j (L_j - below_mean)^2), two-pass, centred
 *   within_sd                sqrt(mean_j V_j)
 *   q_below_mean, q_below_sd the same two of C_j: what q's own draws say by themselves (the ECDF of the draws)
 *   below_bands, above_bands the probs quantiles over j of L_j and of U_j, by the rule of bb_ppc_bands (StatsBase.quantile, type 7:
 *                            order statistics by selection, a + gamma (b - a)); n_quantiles > 0 needs n_samples >= 2
 *   n_units [n_sets]         the sets' sizes
 * total variance of the fraction: between_sd^2 + within_sd^2; between_sd / within_sd > 1 says the shared part dominates.
 * A non-finite parameter makes the eight Rao-Blackwellised outputs of the sets that name a unit using it NaN (q_below_* stay what
 * the comparison gives); it disturbs no other set and is not an error.
 *
 * Options: n_samples, n_quantiles, probs, seed and draws are bb_rb_opts' exactly (the keying included: at equal seed the draws are
 * bb_fitness_rb's; n_samples = 1 is allowed with draws and no quantiles).  BB_DFE_MAX_SAMPLES: one workgroup holds the column of
 * L_j, then of U_j -- one after the other, not both -- in LDS beside the selection's histograms; both at once would cap at 7572.
 * reserved0: 0.  (Tests: a positive value bounds the chunk partials in flight to that many [4][n_samples] tables in place of
 * 256 MiB; no result depends on it.)
 *
 * Cost: units x draws x grid points x 2 erfc, and a unit's loglambda row walked once per draw and group of 8 grid points.  The
 * chunk partials [chunks][grid points][4][n_samples] in flight are bounded to 256 MiB by working (sets x grid points) in slabs.
 *
 * A cell's results are a function of the handle's (mu, sigma) (or the supplied draws), the priors, geno_idx, the set's own units
 * in their order, x_g, n_samples, seed and probs: bit-identical whatever the other sets and grid points of the call, their number
 * or order, the slabs, the launch grid, the launch mode, the device count or the calls made before.  (Permuting the units within a
 * set reorders floating-point sums and may change low bits.)  No atomics on doubles.  The handle's mu, omega, optimiser state,
 * step counter and RNG position are untouched, bitwise.
 * BB_ERR_INVALID: a null h, o or out; the probs / n_quantiles errors of bb_fitness_rb; n_grid outside 1 .. BB_DFE_MAX_GRID; a
 * null, non-finite or not strictly ascending grid; reserved0 < 0; n_sets < 0; with n_sets > 0 a null set_ptr or set_idx,
 * set_ptr[0] != 0 or a decreasing set_ptr, an empty set, an index outside the units, a unit named twice in one set.
 * BB_ERR_UNSUPPORTED: n_samples outside its range; n_quantiles > 0 with one draw; more than 2^31 - 1 indices.  The message
 * (bb_last_error) names the set and the position within it, both 0-based.  n_sets == 0 is BB_OK and writes nothing.  Multi-device
 * and sharded handles: as bb_ppc_bands.  Out of scope: quantiles of the DFE itself (invert below_mean along the grid), the set
 * mean (a bb_contrast_rb with weights 1 / n), sets over theta. */
#define BB_DFE_CHUNK 128          /* units per partial sum of a set                        */
#define BB_DFE_MAX_GRID 64
#define BB_DFE_MAX_SAMPLES 8672   /* <= BB_RB_MAX_SAMPLES                                  */
typedef struct bb_dfe_opts {
    int32_t n_samples;        /* draws j, 2 (1 with draws) .. BB_DFE_MAX_SAMPLES       */
    int32_t n_quantiles;      /* 0 .. 8                                                */
    int32_t n_grid;           /* 1 .. BB_DFE_MAX_GRID                                  */
    int32_t reserved0;        /* 0                                                     */
    const double* probs;      /* [n_quantiles], in (0, 1): quantiles over the draws    */
    const double* grid;       /* [n_grid] finite, strictly ascending thresholds x_g    */
    uint64_t seed;            /* Philox key (draws == NULL)                            */
    const double* draws;      /* host, [n_samples][D] in the caller's order, or NULL   */
    int64_t n_sets;
    const int64_t* set_ptr;   /* [n_sets + 1], CSR, set_ptr[0] == 0, increasing        */
    const int64_t* set_idx;   /* [set_ptr[n_sets]] units of bb_fitness_rb              */
} bb_dfe_opts;
typedef struct bb_dfe_out {   /* every pointer may be NULL; [n_sets][n_grid] unless noted */
    double *below_mean, *above_mean, *between_sd, *within_sd, *q_below_mean, *q_below_sd;
    double *below_bands, *above_bands;           /* [n_sets][n_grid][n_quantiles]      */
    int64_t* n_units;                            /* [n_sets]                           */
} bb_dfe_out;
int bb_dfe_rb(bb_handle* h, const bb_dfe_opts* o, const bb_dfe_out* out);

/* Posterior ranks of the fitness units of a set and top-k membership -- which lineages are the fittest, and how sure are we of
 * that list: the rank of every unit within its set per joint draw, and over the draws its mean, sd, quantiles and the probability
 * of lying among the k fittest.  No reference counterpart.  A rank is a function of all the fitnesses of a set at once, so it
 * needs joint draws; the marginals do not give it, and mean-field q's own joint draws are the wrong ones: q has cut every
 * coupling, so ranks formed from them are overconfident wherever units share something (a replicate's sbar_t; theta and tau of
 * the hierarchical kinds).  The repair is bb_contrast_rb's fact: given everything else, distinct fitness units are conditionally
 * independent, each exactly N(m_{u,j}, sd_{u,j}).  Drawing every unit of draw j from its conditional is therefore one exact
 * blocked Gibbs update of the whole fitness block -- the joint draw with the shared uncertainty back in it, the sampling
 * counterpart of what bb_fitness_rb does for the marginals.
 *
 * Sets: CSR exactly as bb_dfe_opts (units in bb_fitness_rb's numbering, at least one per set, each at most once per set).
 * Outputs are indexed by position k in set_idx, since a unit may sit in several sets; n_idx = set_ptr[n_sets].
 *
 * Values per draw j.  (s_{u,j}, m_{u,j}, sd_{u,j}) are bb_fitness_rb's exactly: the same draws and keying (stream 0xFFFFFFE0;
 * draws read in their place), the same gamma, ln Z by the 256-column rule, ascending t, the later time point's environment, the
 * n_u = 0 rule, the hierarchical kinds' N(theta_j, tau_j) prior.  The value that is ranked:
 *   BB_RANK_DRAWS        v = s_{u,j}; the normalisers are not formed
 *   BB_RANK_CONDITIONAL  v = fma(sd_{u,j}, N(u, j >> 1, 0xFFFFFFE3), m_{u,j}); N is the Philox normal pair at `seed` (with explicit
 *                        draws too), u the unit's number (not its position in a set), an even j the cosine branch and an odd j the
 *                        sine branch.  A unit has one value per draw whichever sets name it: the sets of a call are ranked on one
 *                        joint draw.
 * Order.  Within a set, position a ranks before position b when v_a > v_b; or v_a is a number and v_b is NaN; or neither holds
 * either way and a < b (equal values, -0.0 and +0.0 being equal, and both NaN).  So a NaN ranks after every number, -Inf after
 * every finite value, ties go to the caller's order; the ranks r of a (set, draw) are a permutation of 0 .. n - 1 and rank 0 is
 * the fittest.  Non-finite parameters are not an error: they rank as stated and disturb no set that does not name a unit using them.
 *
 * Over the draws, per position (r_j the int32 rank, divisor n_samples):
 *   rank_mean  (sum_j r_j) / n_samples: the sum of integers is exact, one rounding
 *   rank_sd    sqrt(mean_j (r_j - rank_mean)^2), two-pass and centred, in bb_ppc_score's reduction order
 *   p_top      p_top[k][i] = #{j : r_j < top[i]} / n_samples: exact; 1 where top[i] >= n
 *   quantiles  the probs quantiles over j of r_j as doubles, by the rule of bb_ppc_bands (type 7: exact order statistics by
 *              selection, a + gamma (b - a)); n_quantiles > 0 needs n_samples >= 2
 *   ranks      r_j itself, [n_idx][n_samples]
 *   n_units    [n_sets] the sets' sizes
 *
 * Working memory: a set of at most BB_RANK_RUN units is sorted by one workgroup per draw in LDS; a larger one in runs of
 * BB_RANK_RUN whose sorted keys are then searched for every element (csrc/bb_rank.h).  The tables in flight (per position and
 * draw a key, a sorted position and a rank: 16 bytes) are bounded to 256 MiB by working the sets in slabs; a set that alone
 * exceeds the bound is worked alone, its keys in tiles of draws, its int32 rank table whole.  reserved0, reserved1: 0.  (Tests:
 * reserved0 > 0 replaces the run length by that power of two in 64 .. BB_RANK_RUN; reserved1 > 0 replaces the bound, in KiB.  No
 * result depends on either.)  BB_RANK_MAX_SAMPLES: one workgroup holds the column of a position's ranks in LDS beside the
 * selection's histograms (bb_dfe_rb's layout and cap).
 *
 * A position's results are a function of the handle's (mu, sigma) (or the supplied draws), the priors, geno_idx, its own set's
 * units in their order, n_samples, seed, source, top and probs: bit-identical whatever the other sets, their number or order,
 * the slabs, the run length, the launch grid or mode, the device count or the calls made before.  Ranks are integers defined by a
 * strict total order: every correct algorithm gives the same ones.  No atomics on doubles.  The handle's mu, omega, optimiser
 * state, step counter and RNG position are untouched, bitwise.
 * BB_ERR_INVALID: a null h, o or out; the probs / n_quantiles errors of bb_fitness_rb; an unknown source; n_top outside
 * 0 .. BB_RANK_MAX_TOP; top null with n_top > 0; a top[i] outside 1 .. 2^31 - 1; a negative reserved0 or reserved1 (or a
 * reserved0 that is no power of two in 64 .. BB_RANK_RUN); the set errors of bb_dfe_rb, word for word.  BB_ERR_UNSUPPORTED:
 * n_samples outside its range; n_quantiles > 0 with one draw; more than 2^31 - 1 indices.  n_sets == 0 is BB_OK and writes
 * nothing.  What the device cannot allocate is BB_ERR_DEVICE, and nothing is computed.  Multi-device and sharded handles: as
 * bb_ppc_bands.  Out of scope: ranks of theta, Rao-Blackwellised pairwise ordering probabilities (O(n^2)). */
#define BB_RANK_CONDITIONAL 0     /* s*_{u,j}: every unit redrawn from its conditional  */
#define BB_RANK_DRAWS       1     /* s_{u,j}: the draws' own fitness                    */
#define BB_RANK_MAX_TOP     8
#define BB_RANK_RUN         8192  /* keys one workgroup sorts in LDS                    */
#define BB_RANK_MAX_SAMPLES 8672  /* <= BB_RB_MAX_SAMPLES                               */
typedef struct bb_rank_opts {
    int32_t n_samples;        /* draws j, 2 (1 with draws) .. BB_RANK_MAX_SAMPLES       */
    int32_t n_quantiles;      /* 0 .. 8                                                 */
    int32_t n_top;            /* 0 .. BB_RANK_MAX_TOP                                   */
    int32_t source;           /* BB_RANK_*                                              */
    int32_t reserved0;        /* 0 (tests: run length, above)                           */
    int32_t reserved1;        /* 0 (tests: bound of the tables in flight, KiB)          */
    const double* probs;      /* [n_quantiles], in (0, 1): quantiles over the draws     */
    const int64_t* top;       /* [n_top] list lengths k, 1 .. 2^31 - 1                  */
    uint64_t seed;            /* Philox key                                             */
    const double* draws;      /* host, [n_samples][D] in the caller's order, or NULL    */
    int64_t n_sets;
    const int64_t* set_ptr;   /* CSR exactly as bb_dfe_opts                             */
    const int64_t* set_idx;   /* units of bb_fitness_rb                                 */
} bb_rank_opts;
typedef struct bb_rank_out {  /* every pointer may be NULL; n_idx = set_ptr[n_sets]     */
    double *rank_mean, *rank_sd;   /* [n_idx]                                           */
    double* p_top;                 /* [n_idx][n_top]                                    */
    double* quantiles;             /* [n_idx][n_quantiles]                              */
    int32_t* ranks;                /* [n_idx][n_samples]: the rank draws themselves     */
    int64_t* n_units;              /* [n_sets]                                          */
} bb_rank_out;
int bb_fitness_rank(bb_handle* h, const bb_rank_opts* o, const bb_rank_out* out);

/* Rao-Blackwellised marginals of the population mean fitness sbar_t -- the pop_mean_fitness rows of a fit, the quantity every
 * reported mutant fitness is relative to, and the one latent that every barcode's log-frequency-ratio term reads: q factorises it
 * away from all of them.  No reference counterpart.  sbar_g enters the log-joint through its Gaussian prior (s_pop_prior, Vector or
 * Matrix form) and, linearly, through the Gaussian log-frequency-ratio terms of every barcode of its replicate at its step, so its
 * full conditional given everything else is N(m, sd) in closed form in all five model kinds, and bb_fitness_rb's averaging over
 * joint draws applies as it stands.
 *
 * Groups (bb_popmean_rb_shape: n_groups = the length of the caller's s_pop block; every model kind has groups): g = (r, k),
 * replicate r and step k < T_r - 1, numbered in the order of that block: replicate-major, k ascending.
 *
 * Members of a group, i = 0 .. n_neutral + n_bc - 1 (n_members; the same for every group):
 *   i < n_neutral   a neutral term.  Without BB_FLAG_RAGGED_METHOD: the neutral data column b = i at step t = k.  With the flag
 *          (BB_MODEL_REPLICATE only): the neutral data element x = k n_neutral + i of the replicate's time-fastest vector, that
 *          is t = x mod (T_r - 1), b = x div (T_r - 1) -- the reference's `repeat(.., inner=n_neutral)` pairing
 *          (model_fitness_normal_hierarchical_replicates.jl:599-605), the one a flagged handle's fit evaluates.
 *   i >= n_neutral  mutant m = i - n_neutral, in the caller's order, at step t = k.
 *
 * Per draw j and member, with gamma_{t,b,j} = (ll_{r,t+1,b,j} - ll_{r,t,b,j}) - (ln Z_{r,t+1,j} - ln Z_{r,t,j}) exactly
 * bb_fitness_rb's (the same ln Z by the 256-column rule, the same draws):
 *   neutral term:  w = exp(-2 logsigmabar_{g,j}), the draw of the group's logsigma_pop latent through the platform exp (not the
 *          clamped table of bb_ppc_bands);  cP = w;  cN = -(w gamma)
 *   mutant term, u the mutant's bb_fitness_rb unit for environment env_r(k + 1):  s_{u,j} the unit's fitness draw (the s_bc draw,
 *          or theta_j + exp(logtau_j) theta_tilde_j: bb_fitness_rb's s_j word for word);  w = exp(-2 logsigma_{u,j});  cP = w;
 *          cN = w (s_{u,j} - gamma)
 * Order of the sums: the members are cut into chunks of BB_POPMEAN_RB_CHUNK consecutive member indices; a chunk's (SP, SN) start at
 * 0.0 and take their members' (cP, cN) in index order (every member adds its own cP: the neutral w is not multiplied by a count);
 * the group's (SP_j, SN_j) start at 0.0 and take the chunks in chunk order.  No atomics on doubles.
 * Conditional, with (a, 1 / b^2) the s_pop_prior element of the group as the handle holds it (the same for every draw):
 *   P_j = 1 / b^2 + SP_j;   m_j = (a / b^2 + SN_j) / P_j;   sd_j = 1 / sqrt(P_j)
 * The conditional does not read sbar_g itself.  The identity all this rests on, at any point z:  P (m - sbar_g) = dlogp/dsbar_g.
 *
 * Outputs per group (every pointer may be NULL):
 *   n_members  n_neutral + n_bc
 *   q_mean, q_sd     mean and sd of the group's own sbar draws over j, as bb_fitness_rb's of s_j
 *   rb_mean, rb_sd, p_pos, p_neg, quantiles    from (m_j, sd_j) by bb_fitness_rb's formulas word for word, the 64-step bisection,
 *              its bracket and its NaN rule included.
 * Non-finite parameters propagate by IEEE rules into the groups that use them; they disturb no other group and are not an error.
 *
 * The options are bb_fitness_rb's, with the same meaning and limits (draws, seed and keying included; BB_RB_MAX_SAMPLES because a
 * group's (m_j, sd_j) live in LDS as a unit's do).  A group's results are a function of the handle's (mu, sigma) (or the supplied
 * draws), the s_pop prior, n_samples, seed, threshold and probs: bit-identical whatever the grid, the launch mode, the handle's
 * internal latent order, the device count or the calls made before.  The handle's mu, omega, optimiser state, step counter and
 * RNG position are untouched, bitwise.  BB_ERR_INVALID / BB_ERR_UNSUPPORTED for the options exactly as bb_fitness_rb.  The chunk
 * partials [chunks][2][n_samples] of the groups in flight are bounded to 256 MiB (the groups are worked in slabs; a single group
 * is worked whole).  Multi-device and sharded handles: as bb_ppc_bands.
 * The conditionals of logsigma: bb_logsigma_rb; of logtau: bb_logtau_rb. */
#define BB_POPMEAN_RB_CHUNK 256
typedef struct bb_popmean_rb_out {   /* every pointer may be NULL; [n_groups] unless noted */
    double *q_mean, *q_sd, *rb_mean, *rb_sd, *p_pos, *p_neg;
    double* quantiles;               /* [n_groups][n_quantiles]                        */
    int32_t* n_members;              /* n_neutral + n_bc                               */
} bb_popmean_rb_out;
int bb_popmean_rb_shape(const bb_handle* h, int64_t* n_groups);
int bb_popmean_rb(bb_handle* h, const bb_rb_opts* o, const bb_popmean_rb_out* out);

/* Rao-Blackwellised marginals of the noise scales logsigma_bc and logsigma_pop -- the latents where a mean-field Gaussian is at its
 * worst (too narrow, and symmetric on the log scale where the true marginal is skewed), and the numbers that say which barcodes and
 * which time steps are noisy.  No reference counterpart.  Given everything else a log-scale l enters the log-joint through its
 * Gaussian prior N(a, b) and n Gaussian terms of standard deviation e^l whose residuals do not read l.  The conditional is not
 * Gaussian, but it is one-dimensional and strictly log-concave, so it is integrated numerically per draw, by the rule below.
 *
 * Entries (bb_logsigma_rb_shape: n_entries = the length of the caller's logsigma_bc or logsigma_pop block):
 *   BB_LOGSIGMA_BC   unit u of bb_fitness_rb, same numbering, same T_u and n_u.  Prior (a, 1 / b^2): the logsigma_bc_prior element
 *          as the handle holds it (Vector or Matrix form; a Matrix form follows its mutant through the genotype regrouping).
 *          n = n_u;  SS_j = sum_{t in T_u} d_t^2,  d_t = (gamma_{t,j} + sbar_{r,t,j}) - s_{u,j},  in ascending t from 0.0; gamma,
 *          ln Z, sbar and s_{u,j} are bb_fitness_rb's word for word.
 *   BB_LOGSIGMA_POP  group g = (r, k) of bb_popmean_rb, same numbering.  Prior: the logsigma_pop_prior element.  n = n_neutral;
 *          d_i = gamma_{t,b,j} + sbar_{g,j} over the neutral members i < n_neutral of bb_popmean_rb's group g word for word (the
 *          BB_FLAG_RAGGED_METHOD pairing included), sbar_g the draw of the group's own s_pop latent; SS_j is summed in chunks of
 *          BB_POPMEAN_RB_CHUNK consecutive member indices, a chunk from 0.0 in index order, the chunks from 0.0 in chunk order.
 * No atomics on doubles.  Either way, with ib2 = 1 / b^2, the log conditional density of draw j up to a constant is
 *   h_j(l)  = -(l - a)^2 ib2 / 2 - n l - (SS_j / 2) e^{-2l}
 *   h_j'(l) = -(l - a) ib2 - n + SS_j e^{-2l},     -h_j''(l) = ib2 + 2 SS_j e^{-2l} > 0
 * The identity all this rests on, at any point z: h'(l) at z's own value of the latent = dlogp/dl (bb_logdensity_grad's entry).
 *
 * The rule (this is the definition, as the 64-step bisection is bb_fitness_rb's).
 * Mode l*_j, the root of h_j':  SS_j == 0: l* = a - n / ib2 exactly.  Otherwise c2 = 2 / ib2, lnK = ln SS_j - 2a + c2 n, and
 *   G(t) = t + c2 e^t - lnK = 0 is solved by Newton from t0 = ln(lnK / c2) if lnK >= c2, else t0 = lnK (G(t0) >= 0, G convex and
 *   increasing: the iteration descends monotonically): step = G(t) / (1 + c2 e^t), t <- t - step, until |step| <= 2^-40 (1 + |t|)
 *   with the new t, or 50 steps; then l* = a + (e^t - n) / ib2.  (Newton on h' itself overflows at n = 1000.)
 * Grid:  W_j = SS_j e^{-2 l*} (0 where SS_j == 0),  delta_j = 1 / sqrt(ib2 + 2 W_j).  With p(u) = exp(h_j(l* + u) - h_j(l*)), the
 *   exponent evaluated as -u c1 - ib2 u^2 / 2 - (W_j / 2) expm1(-2u), c1 = ib2 (l* - a) + n, which is the same number without the
 *   cancelling large terms:
 *   step   s_j = delta_j / (4 m_j),  m_j = max(1, ceil(2 delta_j)), at most 64 (1 for a NaN delta_j): delta / 4 wherever
 *          delta_j <= 1/2, and never above 1/8 -- the factor exp(-(SS / 2) e^{-2l}) cuts the density off on the left over a width of
 *          about 1/2 in l whatever delta is, and delta / 4 alone does not resolve that where delta is near a wide prior's b;
 *   ends   lo_j = l* - 10 delta_j;  hi_j = l* + 22 r_j delta_j, r_j the first of 1, 2, 4 .. 64 with ln p(22 r delta_j) <= -40 (64
 *          if none; the right tail is the slow one: it decays at the prior's curvature only, and 22 delta is not far enough where
 *          delta is well below b and n is small);
 *   nodes  u_k = (k - 40 m_j) s_j about the mode, k = 0 .. (10 + 22 r_j) 4 m_j, so x_k = l* + u_k runs from lo_j to hi_j = l* +
 *          (88 r_j m_j) s_j and the mode is a node; p_k = p(u_k); trapezoid weights w_k = s_j, halved at both ends.
 *   For delta_j <= 1/2 with the tail test met at r = 1 this is 129 nodes at delta / 4 on [l* - 10 delta, l* + 22 delta].
 * Per-draw moments (sums in ascending k; the common factor s_j taken out of the ratios):
 *   Z_j = sum w p;   E_j = l* + (sum w p u) / Z_j;   V_j = (sum w p u^2) / Z_j - (E_j - l*)^2  (= sum w p (x - E_j)^2 / Z_j);
 *   S_j = e^{l*} (sum w p e^u) / Z_j, the conditional mean of sigma itself.
 * Per-draw CDF C_j(x):  0 for x <= lo_j, 1 for x >= hi_j; between them N = max(1, ceil((x - lo_j) / s_j)), s_x = (x - lo_j) / N,
 *   the trapezoid of p on the N + 1 nodes u = -10 delta_j + i s_x, i < N, and u = x - l* (ends halved, ascending i), less the first
 *   Euler-Maclaurin end term s_x^2 / 12 (h_j'(x) p(x) - h_j'(lo_j) p(lo_j)), divided by Z_j, clamped to [0, 1].
 *
 * Outputs per entry (every pointer may be NULL; sums over the draws in bb_ppc_score's order):
 *   n_terms    n
 *   q_mean, q_sd     of the latent's own draws, as bb_fitness_rb's of s_j
 *   rb_mean    mean_j E_j
 *   rb_sd      sqrt(mean_j V_j + mean_j (E_j - rb_mean)^2), two-pass and centred
 *   sigma_mean mean_j S_j
 *   mode_mean  mean_j l*_j
 *   quantiles  quantiles[entry][i], the probs[i] quantile of the mixture F(x) = mean_j C_j(x): lo = min_j lo_j, hi = max_j hi_j;
 *              40 times x = lo + (hi - lo) / 2, F(x) < p ? lo = x : hi = x; the result is the last bracket's midpoint; NaN if any
 *              l*_j, delta_j or Z_j is non-finite.  Quantiles are of logsigma; their exp are sigma's.
 * An entry with n = 0 has the prior as its conditional through the same rule (SS = 0: l* = a, delta = b).  Non-finite parameters
 * propagate by IEEE rules into the entries that use them; they disturb no other entry and are not an error.
 *
 * Options: block selects the latent block; draws, seed and the keying are bb_rb_opts' exactly (n_samples = 1 is allowed with
 * draws).  BB_LOGSIGMA_RB_MAX_SAMPLES is the largest count for which (l*_j, delta_j, Z_j) -- three arrays where bb_fitness_rb has
 * two -- and the reductions' partials fit the 160 KiB of LDS (derived next to the layout, csrc/bb_lsrb.h).
 * An entry's results are a function of the handle's (mu, sigma) (or the supplied draws), the two logsigma priors, n_samples, seed
 * and probs: bit-identical whatever the grid, the launch mode, the handle's internal latent order, the device count or the calls
 * made before.  The handle's mu, omega, optimiser state, step counter and RNG position are untouched, bitwise.  BB_ERR_INVALID /
 * BB_ERR_UNSUPPORTED for the options as bb_fitness_rb (there is no threshold), and BB_ERR_INVALID for an unknown block.  The POP
 * block's chunk partials [chunks][n_samples] of the groups in flight are bounded to 256 MiB (slabs; a single group is worked
 * whole).  Multi-device and sharded handles: as bb_ppc_bands.
 * The conditional of logtau, which is not log-concave in logtau and needs another bracket: bb_logtau_rb, below; that of loglambda:
 * bb_loglambda_rb, below that. */
#define BB_LOGSIGMA_BC 0
#define BB_LOGSIGMA_POP 1
#define BB_LOGSIGMA_RB_MAX_SAMPLES 5781
typedef struct bb_logsigma_rb_opts {
    int32_t block;            /* BB_LOGSIGMA_BC or BB_LOGSIGMA_POP                     */
    int32_t n_samples;        /* draws j, 2 (1 with draws) .. BB_LOGSIGMA_RB_MAX_SAMPLES */
    int32_t n_quantiles;      /* 0 .. 8                                                */
    int32_t reserved0;
    const double* probs;      /* [n_quantiles] probabilities in (0, 1)                 */
    uint64_t seed;            /* Philox key (draws == NULL)                            */
    const double* draws;      /* host, [n_samples][D] in the caller's order, or NULL   */
} bb_logsigma_rb_opts;
typedef struct bb_logsigma_rb_out {  /* every pointer may be NULL; [n_entries] unless noted */
    double *q_mean, *q_sd, *rb_mean, *rb_sd, *sigma_mean, *mode_mean;
    double* quantiles;               /* [n_entries][n_quantiles]                       */
    int32_t* n_terms;                /* n                                              */
} bb_logsigma_rb_out;
int bb_logsigma_rb_shape(const bb_handle* h, int32_t block, int64_t* n_entries);
int bb_logsigma_rb(bb_handle* h, const bb_logsigma_rb_opts* o, const bb_logsigma_rb_out* out);

/* Rao-Blackwellised marginals of logtau, the deviation scale of the hierarchical kinds (BB_MODEL_GENOTYPE, BB_MODEL_REPLICATE,
 * BB_MODEL_MULTIENV_REPLICATE) -- the block where a mean-field Gaussian is least trustworthy: the fitness is non-centred,
 * s_u = theta_g(u) + e^{logtau_u} theta_tilde_u, so logtau_u and theta_tilde_u enter the likelihood through their product only (the
 * funnel); and the number that says how strongly a replicate or a barcode is pooled towards its group.  No reference counterpart.
 *
 * Entries (bb_logtau_rb_shape: n_entries = the length of the caller's logtau block; 0 for BB_MODEL_FITNESS / BB_MODEL_MULTIENV):
 * unit u of bb_fitness_rb, same numbering, same T_u and n = n_u.  Per draw j: y_j (gamma, ln Z, sbar, ascending t from 0.0, the
 * later time point's environment), w_j = exp(-2 logsigma_{u,j}), theta_j (the unit's hyper-fitness) and tt_j = theta_tilde_{u,j}
 * are bb_fitness_rb's word for word; Y_j = y_j - n theta_j.  Prior (a, ib2 = 1 / b^2): the logtau_prior the handle holds (Vector
 * form).  With x = e^l the log conditional density of draw j up to a constant is, by mode,
 *   BB_LOGTAU_FULL       given everything else, theta_tilde included:   A = (1/2) (n w) (tt tt),  B = (w tt) Y
 *       h(l)   = -(l - a)^2 ib2 / 2 - A x^2 + B x
 *       h'(l)  = -(l - a) ib2 + x (B - 2A x),      h''(l) = -ib2 + x (B - 4A x)
 *     The identity this rests on, at any point z: h' at z's own logtau_u = dlogp/dlogtau_u (bb_logdensity_grad's entry).
 *   BB_LOGTAU_COLLAPSED  theta_tilde_u integrated out against its N(0, 1) prior (tt is not read): v = 1 / (n w),  q = (Y / n)^2,
 *     c = q - v,  k = q + v,  s = x^2,  V = s + v
 *       h(l)   = -(l - a)^2 ib2 / 2 - ln V / 2 - q / (2V)
 *       h'(l)  = -(l - a) ib2 + (s / V) ((q - V) / V),      h''(l) = -ib2 + G(s),  G(s) = 2 (s / V) ((c v - s k) / V) / V
 *     exp(h(l)) = the integral over tt of exp(h_FULL(l; tt)) N(tt; 0, 1), up to a factor free of l.
 * An entry with n = 0 has the prior as its conditional through the same rule (h = -(l - a)^2 ib2 / 2, the data terms dropped); its
 * w, tt, theta are not read, so a non-finite logsigma of such a unit does not reach it (bb_theta_rb's skip rule).
 * Neither h is log-concave (over parameters of use about 60 % of the draws are not), and either can have two modes: one near the
 * prior and one near the least-squares tau.  h' has at most three zeros.
 *
 * The rule (this is the definition, as bb_logsigma_rb's is its own).  Per draw:
 * Segments.  The zeros l1 < l2 of h'', between which h' rises and outside of which it falls, and bounds L <= every zero of h' <= U:
 *   FULL       B > 0:  t = ln(B / (2A)), L = min(a, t), U = max(a, t);  disc = B B - 16 A ib2; if disc > 0: r = sqrt(disc),
 *              l1 = ln(2 ib2 / (B + r)), l2 = ln((B + r) / (8A)) (the roots of 4A x^2 - B x + ib2).  Otherwise (B <= 0, or NaN):
 *              no l1, l2 (h is strictly log-concave); U = a, L = a - e^a (2A e^a - B) / ib2.
 *   COLLAPSED  L = a - 1 / ib2 (h' >= -(l - a) ib2 - 1), U = a; if c > 0: U = max(a, ln(c) / 2), and G has its one maximum over
 *              s > 0 at sp = v c / ((c + k) + sqrt(c c + c k + k k)); if G(sp) > ib2, the two solutions of G(s) = ib2 by 60
 *              bisection steps each on the geometric mean, mid = sqrt(lo hi): the first from lo = ib2 v v / (2c), hi = sp with
 *              G(mid) < ib2 ? lo = mid : hi = mid; the second from lo = sp, hi = c v / k with G(mid) > ib2 ? lo = mid : hi = mid;
 *              l1, l2 = ln(sqrt(lo hi)) / 2 of the final brackets.
 *   n = 0      one mode, l = a exactly; no iteration.
 * Modes.  solve(lo, hi, x): up to 100 times  g = h'(x); g == 0 or NaN: done, the mode x + g;  g > 0 ? lo = x : hi = x;  xn = x - g / h''(x), replaced
 *   by lo + (hi - lo) / 2 unless h''(x) < 0 and lo <= xn <= hi;  step = xn - x, x = xn;  stop once |step| <= 2^-40 (1 + |x|);
 *   then once more xn = x - h'(x) / h''(x), taken if h''(x) < 0 and lo <= xn <= hi (the last step bounds the error by 2^-40 only).
 *   With l1, l2: if h'(l1) < 0 the left mode solve(L, l1, L); if h'(l2) > 0 the right mode solve(l2, U, U).  Without them, or if
 *   neither test holds: the one mode solve(L, U, U).  (The starts are the ends from which Newton on a convex or concave falling h'
 *   approaches monotonically; the bracket guards the rest.)
 * Kept modes.  With two modes, d = ln p(right - left) about the left one (p below); the global mode l* is the right one if d > 0,
 *   else the left; both are kept iff |d| <= 40, else l* alone.  delta of a kept mode: 1 / sqrt(-h''(mode)).
 * Density about l*:  p(u) = exp(h(l* + u) - h(l*)), the exponent in the form without cancelling large terms, g1 = ib2 (l* - a):
 *   FULL       -u g1 - ib2 u^2 / 2 + e1 (D1 - A2 e1),   e1 = expm1(u),  A2 = A (x* x*),  D1 = B x* - 2 A2,  x* = e^{l*}
 *   COLLAPSED  -u g1 - ib2 u^2 / 2 - log1p(y) / 2 + kap (y / (1 + y)),   y = rho expm1(2u),  rho = s* / V*,  kap = q / (2 V*)
 *   n = 0      -u g1 - ib2 u^2 / 2
 * Grid, one per draw, over all kept modes:  dmin the smaller delta;  m = max(1, ceil(2 dmin - 2^-20)), at most 64 (1 for a non-finite
 *   dmin);  s0 = dmin / (4 m): a quarter of the smallest curvature scale, never above 1/8.  Ends: left of the leftmost kept mode ml
 *   (its delta dl) e0 = ml - 8 r dl, r the first of 1, 2, 4 .. 4096 with ln p(e0 - l*) <= -40 (4096 if none); right of the
 *   rightmost likewise with its own delta.  nl = ceil((l* - e0) / s0 - 2^-20), nr = ceil((e1 - l*) / s0 - 2^-20), each 1 unless the quotient is within
 *   1 .. 1e9 (the 2^-20: with one mode the quotients are whole numbers but for rounding, which must not tip them over);
 *   f = ceil((nl + nr) / 8192) (integer), s = f s0, nleft = ceil(nl / f), nright = ceil(nr / f): at most 8194 nodes per draw, the
 *   hard cap, f > 1 only where a mode is narrower than about 1e-3 of the span (the step is then wider than a quarter delta and the
 *   moments lose accuracy; not met in the tests).  Nodes u_k = (k - nleft) s, k = 0 .. nleft + nright, so lo_j = l* - nleft s,
 *   hi_j = l* + nright s and the GLOBAL mode is a node.  The other kept mode need not be one: the integrand is analytic and has
 *   decayed to e^-40 at both ends, so the trapezoid's error is set by the step against the narrowest feature, not by where the
 *   nodes fall.  Weights s, halved at both ends.
 * Per-draw moments (sums in ascending k):  z = sum w p,  Z_j = s z;  E_j = l* + (sum w p u) / z;  V_j = (sum w p u^2) / z -
 *   (E_j - l*)^2;  T_j = e^{l*} (sum w p exp(u)) / z;  P_j = (sum w p / (1 + (n w e^{2 l*}) e^{2u})) / z, with e^{2u} = (e1 + 1)^2
 *   (FULL) or expm1(2u) + 1 (COLLAPSED), and the factor 1 for n = 0 (so P_j = 1 exactly).
 * Per-draw CDF C_j(x):  0 for x <= lo_j, 1 for x >= hi_j; between them N = max(1, ceil((x - lo_j) / s)), s_x = (x - lo_j) / N, the
 *   trapezoid of p on the N + 1 nodes u = (lo_j - l*) + i s_x, i < N, and u = x - l* (ends halved, ascending i), less the first
 *   Euler-Maclaurin end term s_x^2 / 12 (h'(x) p(x) - h'(lo_j) p(lo_j)), divided by Z_j, clamped to [0, 1].
 *
 * Outputs per entry (every pointer may be NULL; sums over the draws in bb_ppc_score's order):
 *   n_terms     n
 *   q_mean, q_sd     of the latent's own draws, as bb_fitness_rb's of s_j
 *   rb_mean     mean_j E_j
 *   rb_sd       sqrt(mean_j V_j + mean_j (E_j - rb_mean)^2), two-pass and centred
 *   tau_mean    mean_j T_j, the RB mean of tau itself
 *   pool_mean   mean_j P_j, the pooling factor 1 / (1 + n w tau^2): 1 the unit sits on its group, 0 it is on its own
 *   mode_mean   mean_j l*_j (the global modes)
 *   n_two_modes the draws whose conditional kept two modes
 *   quantiles   quantiles[entry][i], the probs[i] quantile of the mixture F(x) = mean_j C_j(x): lo = min_j lo_j, hi = max_j hi_j;
 *               40 times x = lo + (hi - lo) / 2, F(x) < p ? lo = x : hi = x; the result is the last bracket's midpoint; NaN if any
 *               l*_j, s_j or Z_j is non-finite.  Quantiles are of logtau; their exp are tau's.
 * Non-finite parameters propagate by IEEE rules into the entries that use them; they disturb no other entry and are not an error.
 * (A finite corner that is not served: tt so small that A underflows to 0 while B > 0 -- |tt| below 1e-150 -- has U = inf.)
 *
 * Options: mode selects the conditional; draws, seed and the keying are bb_rb_opts' exactly (n_samples = 1 is allowed with draws).
 * BB_LOGTAU_RB_MAX_SAMPLES is the largest count for which (l*_j, s_j, Z_j) and the reductions' partials fit the 160 KiB of LDS
 * (derived next to the layout, csrc/bb_ltrb.h).  An entry's results are a function of the handle's (mu, sigma) (or the supplied
 * draws), the logtau prior, n_samples, seed, mode and probs: bit-identical whatever the grid, the launch mode, the handle's
 * internal latent order, the device count or the calls made before.  No atomics on doubles.  The handle's mu, omega, optimiser
 * state, step counter and RNG position are untouched, bitwise.  BB_ERR_INVALID / BB_ERR_UNSUPPORTED for the options as
 * bb_logsigma_rb, BB_ERR_INVALID for an unknown mode, BB_ERR_UNSUPPORTED, the message naming the model kind, for BB_MODEL_FITNESS /
 * BB_MODEL_MULTIENV.  Multi-device and sharded handles: as bb_ppc_bands.
 * The conditional of loglambda: bb_loglambda_rb, below.  Out of scope: a Matrix-form logtau_prior (the reference has none). */
#define BB_LOGTAU_FULL 0
#define BB_LOGTAU_COLLAPSED 1
#define BB_LOGTAU_RB_MAX_SAMPLES 5781
typedef struct bb_logtau_rb_opts {
    int32_t mode;             /* BB_LOGTAU_FULL or BB_LOGTAU_COLLAPSED                 */
    int32_t n_samples;        /* draws j, 2 (1 with draws) .. BB_LOGTAU_RB_MAX_SAMPLES */
    int32_t n_quantiles;      /* 0 .. 8                                                */
    int32_t reserved0;
    const double* probs;      /* [n_quantiles] probabilities in (0, 1)                 */
    uint64_t seed;            /* Philox key (draws == NULL)                            */
    const double* draws;      /* host, [n_samples][D] in the caller's order, or NULL   */
} bb_logtau_rb_opts;
typedef struct bb_logtau_rb_out {    /* every pointer may be NULL; [n_entries] unless noted */
    double *q_mean, *q_sd, *rb_mean, *rb_sd, *tau_mean, *pool_mean, *mode_mean;
    double* quantiles;               /* [n_entries][n_quantiles]                       */
    int32_t* n_terms;                /* n                                              */
    int32_t* n_two_modes;            /* draws with two kept modes                      */
} bb_logtau_rb_out;
int bb_logtau_rb_shape(const bb_handle* h, int64_t* n_entries);
int bb_logtau_rb(bb_handle* h, const bb_logtau_rb_opts* o, const bb_logtau_rb_out* out);

/* Rao-Blackwellised marginals of loglambda, the log-rates: T B of the D latents, and the block where a Gaussian q is most doubtful
 * for the barcodes read a handful of times -- the full conditional of such a log-rate is skewed like a log-gamma density, and
 * mean-field cuts its coupling to the barcode's fitness, to the noise scale and, through the row normaliser, to every other
 * barcode of the time point.  No reference counterpart (the terms: src/model_fitness_normal.jl:209-270 and its four siblings).
 *
 * Entries (bb_loglambda_rb_shape: n_rows, n_cols = bb_freq_shape's): (row, t), row = r B + b the rows of bb_freq_bands (b the data
 * column, neutrals first, then the mutants in the caller's order), t < T_r the time point.  Per draw j (bb_fitness_rb's draws) let
 * x0 be the draw of ll_{r,t,b}, L_t = ln Z_{r,t,j} by the 256-column rule of bb_freq_bands (bb_fitness_rb's ln Z word for word) and
 * f0 = exp(x0 - L_t).  For a candidate x:  xi = x - x0,  delta(xi) = log1p(f0 expm1(xi)) = ln Z_t(x) - L_t.
 * A step k of the replicate joins the time points k and k + 1.  Every data column i has at step k a weight w_{i,k}, a mean mu_{i,k}
 * and a residual rho_{i,k} = gamma_{i,k} - mu_{i,k},  gamma_{i,k} = (ll_{k+1,i} - ll_{k,i}) - (L_{k+1} - L_k), bb_fitness_rb's gamma:
 *   neutral i            w = exp(-2 logsigmabar_g),  rho = gamma + sbar_g,  g the group whose s_pop / logsigma_pop entries
 *                        bb_popmean_rb's group table pairs with (k, i): g = (r, k); under BB_FLAG_RAGGED_METHOD the group
 *                        (r, (i (T_r - 1) + k) div n_neutral), the inverse of that table's (t, b) = (x mod (T_r - 1), x div (T_r - 1));
 *   mutant i = n_neutral + m   its bb_fitness_rb unit u of environment env_r(k + 1):  w = exp(-2 logsigma_u),
 *                        rho = (gamma + sbar_{r,k}) - s_u,  s_u the unit's fitness draw (theta + exp(logtau) theta_tilde for the
 *                        hierarchical kinds), the order of operations bb_logsigma_rb's d_t.
 * Two tables per (r, k, j):  A_k = sum_i w_{i,k},  B_k = sum_i w_{i,k} rho_{i,k}, over all data columns in chunks of 256
 * consecutive columns, a chunk from 0.0 in index order, the chunks from 0.0 in chunk order.  No atomics on doubles.
 * With (a, ib2 = 1 / std^2) the loglambda_prior element as the handle holds it (Vector or Matrix form; a Matrix form follows its
 * latent through any regrouping) and R = counts_{r,t,b}, the log conditional density of draw j is, up to a constant,
 *   h(x) - h(x0) = -ib2/2 [(x - a)^2 - (x0 - a)^2] + R xi - e^{x0} expm1(xi)
 *      - 1/2 [  2 B_t delta     + A_t delta^2     + w_{b,t}   (xi^2 - 2 xi (rho_{b,t}   + delta)) ]      (only if t < T_r - 1)
 *      - 1/2 [ -2 B_{t-1} delta + A_{t-1} delta^2 + w_{b,t-1} (xi^2 + 2 xi (rho_{b,t-1} - delta)) ]      (only if t >= 1)
 * (the Poisson total and the multinomial collapse exactly to R x - e^x; the terms in delta are the ratio terms of every barcode
 * of the time point, reached through the normaliser; no "total minus own term" subtraction is needed).
 * The identity this rests on, at any point z:  h'(x0) = dlogp/dll_{r,t,b} (bb_logdensity_grad's entry)
 *   = -ib2 (x0 - a) + R - e^{x0} - (B_t f0 - w_{b,t} rho_{b,t}) + (B_{t-1} f0 - w_{b,t-1} rho_{b,t-1}),  the brackets as above.
 * h is not log-concave in general: the normaliser terms add the curvature -(A delta'^2 + (A delta +- B) delta''), whose second
 * piece takes the sign of the summed residuals and can rival the Poisson curvature e^x for counts of a few reads.
 *
 * The rule (this is the definition, as bb_logtau_rb's is its own).  Per draw:
 * Folded form.  A missing side contributes exact zeros to  As = A_t + A_{t-1},  Bs = B_t - B_{t-1},  ws = w_{b,t} + w_{b,t-1},
 *   wr = w_{b,t} rho_{b,t} - w_{b,t-1} rho_{b,t-1}  (each: the t side, then the t - 1 side).  About a base point x (first x0) with
 *   its f0 = e^x / Z_t(x), u the offset from it, em = expm1(u), delta = log1p(f0 em), f = delta' = f0 (em + 1) / (1 + f0 em):
 *     g(u)   = -(ib2/2) (u (u + 2 (x - a))) + R u - e^x em - Bs delta - (As/2) delta^2 - (ws/2) u^2 + u wr + ws (u delta)
 *     g'(u)  = -ib2 (u + (x - a)) + R - e^x (em + 1) - (Bs + As delta) f - ws u + wr + ws (delta + u f)
 *     g''(u) = -ib2 - e^x (em + 1) - Bs ff - As (f f + delta ff) - ws + ws (2 f + u ff),   ff = f (1 - f)
 *   which is h(x + u) - h(x) without a difference of large terms.  Moving the base to x + u keeps the form (anchor):
 *     Bs <- Bs + As delta(u) - ws u,   wr <- wr + ws (delta(u) - u),   f0 <- f(u),   x <- x + u,   e^x recomputed.
 * Bracket, about x0, holding every zero of g'.  With Bp = max(Bs, 0), Bm = max(-Bs, 0), sl = ib2 + ws (1 - f0),
 *   C0 = -ib2 (x0 - a) + R + wr + ws log1p(-f0) and  low(L) = (C0 - e^{x0} e^L - Bp f(L)) / sl - L:  for u < L <= 0 one has
 *   e^u <= e^L, f(u) <= f(L), 1 - f(u) >= 1 - f0, delta >= log1p(-f0), -As delta f >= 0, so g'(u) >= -sl u + sl (low(L) + L) > 0
 *   wherever low(L) >= 0; low falls as L rises.  l = low(0); if l < 0 (else lo = 0): l is such an L and 0 is not; 30 times
 *   mid = l + (up - l) / 2 from up = 0, low(mid) >= 0 ? l = mid : up = mid; lo = l - 1/8.  (The end follows e^x down: a draw far
 *   above its count -- a fit far from converged -- would otherwise put lo at -e^{x0} / sl.)  For u > 0: f <= 1, delta <= u, As >= ws, so
 *   g'(u) <= K - ib2 u and g'(u) <= K - e^{x0} e^u with K = R + Bm + wr - ib2 (x0 - a):  hi = max(0, min(K / ib2,
 *   ln(K / e^{x0}))) + 1/8  (K <= 0: hi = 1/8).
 *   (A frequency f0 of exactly 1 -- a lone barcode -- is not served: lo = -inf and the entry is NaN.)
 * Mode search.  nc = ceil(8 (hi - lo)) cells, at least 16, at most 1024, of equal width, the last ending at hi exactly; g' at the
 *   nc + 1 edges in ascending order.  A cell with g' > 0 at its left edge and not at its right holds a mode: solve(e0, e1, the
 *   cell's midpoint) as bb_logtau_rb's solve word for word (Newton on g' with g'', a bisection step wherever Newton's leaves the
 *   bracket, 2^-40 (1 + |u|), 100 steps, one more Newton step).  No such cell (rounding at an end): the mode is hi if g'(lo) > 0,
 *   else lo.  The global mode u* is the first of the highest g(mode).  Kept modes: those with g(u*) - g(mode) <= 40; delta of a
 *   kept mode: 1 / sqrt(-g''(mode)).  (Two modes inside one cell of 1/8 are taken as the one the iteration reaches; the grid
 *   below still covers both.)  The base is then moved to x* = x0 + u*.
 * Grid, one per draw, over all kept modes, as bb_logtau_rb's:  dmin the smallest delta;  m = max(1, ceil(2 dmin - 2^-20)), at
 *   most 64;  s0 = dmin / (4 m).  Ends: left of the leftmost kept mode ml (its delta dl) e0 = ml - 8 r dl, r the first of 1, 2,
 *   4 .. 4096 with g(e0) <= -40 about x*; right of the rightmost likewise.  nl = ceil(-e0 / s0 - 2^-20), nr = ceil(e1 / s0 - 2^-20),
 *   each 1 unless the quotient is within 1 .. 1e9;  f = ceil((nl + nr) / 8192), s = f s0, nleft = ceil(nl / f), nright = ceil(nr / f).
 *   Nodes u_k = (k - nleft) s, k = 0 .. nleft + nright; p_k = exp(g(u_k)); weights s, halved at both ends; the global mode is a node.
 * Per-draw moments (sums in ascending k):  z = sum w p,  Z_j = s z;  E_j = x* + (sum w p u) / z;  V_j = (sum w p u^2) / z -
 *   (E_j - x*)^2;  Lam_j = e^{x*} (sum w p (em + 1)) / z, the conditional mean of lambda = e^x itself.
 * Per-draw CDF C_j(x): bb_logtau_rb's word for word (lo_j = x* - nleft s, hi_j = x* + nright s; N = max(1, ceil((x - lo_j) / s))
 *   nodes re-spaced to end at x, less the first Euler-Maclaurin end term s_x^2 / 12 (g'(x) p(x) - g'(lo_j) p(lo_j)), over Z_j,
 *   clamped to [0, 1]).
 *
 * Outputs per entry, [n_rows][n_cols] (every pointer may be NULL; sums over the draws in bb_ppc_score's order):
 *   n_reads     R;  n_sides  1 or 2: how many steps bound the time point
 *   q_mean, q_sd     of the latent's own draws, as bb_fitness_rb's of s_j
 *   rb_mean     mean_j E_j
 *   rb_sd       sqrt(mean_j V_j + mean_j (E_j - rb_mean)^2), two-pass and centred
 *   lambda_mean mean_j Lam_j
 *   mode_mean   mean_j x*_j (the global modes)
 *   quantiles   quantiles[entry][i], the probs[i] quantile of the mixture F(x) = mean_j C_j(x): lo = min_j lo_j, hi = max_j hi_j;
 *               40 times x = lo + (hi - lo) / 2, F(x) < p ? lo = x : hi = x; the result is the last bracket's midpoint; NaN if any
 *               x*_j, s_j or Z_j is non-finite.
 * Cells with t >= T_r of a shorter replicate are NaN (n_reads, n_sides: 0).  Non-finite parameters propagate by IEEE rules into
 * the entries that use them and disturb no others: a NaN in one loglambda reaches every entry of its time point (through Z) and
 * of the time points its steps join, and nothing of another replicate.
 *
 * Options: bb_logsigma_rb_opts' fields without block; draws, seed and the keying are bb_rb_opts' exactly (n_samples = 1 is allowed
 * with draws).  rows == NULL: every row.  Otherwise the n_rows listed bb_freq_bands rows, each in range and strictly ascending
 * (else BB_ERR_INVALID), and the outputs are [n_rows][n_cols]; the tables always sum over all barcodes, so a row's results do
 * not depend on which other rows were asked for.  BB_LOGLAMBDA_RB_MAX_SAMPLES is the largest count for which (x*_j, s_j, Z_j) and
 * the reductions' partials fit the 160 KiB of LDS (derived next to the layout, csrc/bb_llrb.h).  An entry's results are a function
 * of the handle's (mu, sigma) (or the supplied draws), the priors, the counts, n_samples, seed and probs: bit-identical whatever the
 * grid, the launch mode, the handle's internal latent order (the genotype regrouping, loglambda in front of theta), the device
 * count, rows or the calls made before.  The handle's mu, omega, optimiser state, step counter and RNG position are untouched,
 * bitwise.  The chunk partials [chunks][2][n_samples] of the steps in flight are bounded to 256 MiB (slabs; a single step is
 * worked whole).  BB_ERR_INVALID / BB_ERR_UNSUPPORTED for the options as bb_logsigma_rb.  Multi-device and sharded handles: as
 * bb_ppc_bands. */
#define BB_LOGLAMBDA_RB_MAX_SAMPLES 5781
typedef struct bb_loglambda_rb_opts {
    int32_t n_samples;        /* draws j, 2 (1 with draws) .. BB_LOGLAMBDA_RB_MAX_SAMPLES */
    int32_t n_quantiles;      /* 0 .. 8                                                */
    const double* probs;      /* [n_quantiles] probabilities in (0, 1)                 */
    uint64_t seed;            /* Philox key (draws == NULL)                            */
    const double* draws;      /* host, [n_samples][D] in the caller's order, or NULL   */
    const int64_t* rows;      /* [n_rows] bb_freq_bands rows, strictly ascending, or NULL: all */
    int64_t n_rows;           /* length of rows (ignored when rows == NULL)            */
} bb_loglambda_rb_opts;
typedef struct bb_loglambda_rb_out { /* every pointer may be NULL; [n_rows][n_cols] unless noted */
    double *q_mean, *q_sd, *rb_mean, *rb_sd, *lambda_mean, *mode_mean;
    double* quantiles;               /* [n_rows][n_cols][n_quantiles]                  */
    int64_t* n_reads;                /* R                                              */
    int32_t* n_sides;                /* 1 or 2                                         */
} bb_loglambda_rb_out;
int bb_loglambda_rb_shape(const bb_handle* h, int64_t* n_rows, int32_t* n_cols);
int bb_loglambda_rb(bb_handle* h, const bb_loglambda_rb_opts* o, const bb_loglambda_rb_out* out);

/* Chain diagnostics on the device -- what MCMCChains' summarystats / quantile report for the chain the reference's mcmc_sample
 * returns (src/mcmc.jl:151-158): mean, std, MCSE, ESS, R-hat and quantiles of every column of a HOST array
 * chain[n_chains][n_draws][n_cols] (what mcmc_sample of the host layer writes).  n_cols is any positive count, not necessarily
 * bb_num_latents(h): derived quantities can be summarised too.  The handle supplies the device and the stream; nothing of the model
 * is read.
 *
 * Per column, with x_{c,n} the draws of chain c < W = n_chains, n < N = n_draws, and K = W N:
 *   mean, sd   pooled mean, and the corrected (/ (K - 1)) standard deviation about it, two-pass and centred (a column
 *              1e6 + 1e-3 noise keeps its digits).
 *   autocovariance, with m_c the mean of chain c:  a_c(t) = (1/N) sum_{n < N - t} (x_{c,n} - m_c)(x_{c,n+t} - m_c)   (biased)
 *   variances  s2_c = a_c(0) N / (N - 1);  Wbar = mean_c s2_c;  var+ = (N - 1)/N Wbar + [W > 1] Var_c(m_c), the variance of the
 *              chain means taken with W - 1.
 *   ess        Geyer's initial monotone sequence (BDA3 section 11.5, Vehtari et al. 2021):
 *              rho_t = 1 - (Wbar - mean_c a_c(t)) / var+;  P_k = rho_{2k} + rho_{2k+1};  the sum runs over k = 0, 1, ... while
 *              P_k > 0, 2k + 1 <= N - 1 and 2k + 1 <= max_lag (max_lag = 0 means N - 1); before P_k is added it is replaced by
 *              min(P_k, P_{k-1});  tau = -1 + 2 sum P_k;  ess = min(K / tau, K log10(K)).
 *   n_lags     2 x (number of P_k summed).
 *   mcse       sd / sqrt(ess).
 *   rhat       split-R-hat: N' = floor(N / 2), every chain gives the halves [0, N') and [N - N', N) (an odd N drops the middle
 *              draw); rhat = sqrt(var+ / Wbar) computed over those 2W chains of length N'.
 *   quantiles  StatsBase.quantile (type 7) of the pooled K draws at each probs[i] (probabilities, NOT band masses): exact order
 *              statistics; interpolation and non-finite rule as bb_ppc_bands (a NaN orders above +Inf).
 *   A constant column reports its value as mean, sd = 0 exactly, ess = mcse = rhat = NaN and n_lags = 0.  A column holding a
 *   non-finite value reports NaN for the five moment statistics and n_lags = 0, its quantiles by the non-finite rule; it
 *   disturbs no other column and is not an error.
 *
 * The autocovariances are computed BB_CHAIN_LAG_BATCH lags at a time and only up to the batch that holds the truncation.
 * Columns are uploaded in slabs of slab_cols columns (0: as many as BB_CHAIN_SLAB_BYTES of uploaded doubles hold, in whole
 * multiples of 32) and transposed on the device.  The byte budget bounds the library's choice only: an explicit slab_cols is taken
 * as it is (at most n_cols) and the handle then keeps 2 x 8 K slab_cols bytes of device memory for the slab and its transpose --
 * 256 KiB a column at K = BB_CHAIN_MAX_K; what the device cannot allocate fails as BB_ERR_DEVICE and computes nothing.
 *
 * A column's results are a function of its K values, n_chains, n_draws, max_lag and probs alone: bit-identical whatever n_cols,
 * the column's position, slab_cols, the grid or the other columns.  No atomics on doubles; every sum runs in an order fixed by
 * (W, N).  The handle's mu, omega, optimiser state, step counter and RNG position are untouched, bitwise.
 * BB_ERR_INVALID: a null h / o / chain / out; n_cols < 1; n_chains < 1; n_draws < 4; n_quantiles outside 0 .. BB_CHAIN_MAX_Q (or
 * probs null with n_quantiles > 0); a prob outside [0, 1] or NaN; a negative max_lag or slab_cols.  BB_ERR_UNSUPPORTED:
 * n_chains n_draws > BB_CHAIN_MAX_K (one pooled column in LDS).  A multi-device handle (n_devices > 1) works on its first device;
 * a shard of a sharded run works as any other handle. */
#define BB_CHAIN_MAX_K 16384
#define BB_CHAIN_MAX_Q 8
#define BB_CHAIN_LAG_BATCH 32
#define BB_CHAIN_SLAB_BYTES (64 << 20)
typedef struct bb_chain_opts {
    int32_t n_chains;         /* W >= 1                                                */
    int32_t n_draws;          /* N >= 4 per chain; W N <= BB_CHAIN_MAX_K               */
    int32_t n_quantiles;      /* 0 .. BB_CHAIN_MAX_Q                                   */
    int32_t max_lag;          /* 0 = N - 1; else the Geyer sum stops at lag <= max_lag */
    const double* probs;      /* [n_quantiles] probabilities in [0, 1]                 */
    int64_t slab_cols;        /* 0 = library's choice; else columns per slab, as given */
} bb_chain_opts;
typedef struct bb_chain_out {     /* every pointer may be NULL; [n_cols] unless noted  */
    double *mean, *sd, *mcse, *ess, *rhat;
    double* quantiles;        /* [n_cols][n_quantiles]                                 */
    int32_t* n_lags;          /* lags that entered the ESS sum                         */
} bb_chain_out;
int bb_chain_summary(bb_handle* h, const bb_chain_opts* o, int64_t n_cols,
                     const double* chain /* host, [n_chains][n_draws][n_cols] */, const bb_chain_out* out);

/* Convergence monitor: the optimiser's iterates kept as a chain on the device (Dhaka et al. 2020, "Robust, accurate stochastic
 * optimization for variational inference": the run is stationary when split-R-hat of the iterates is near 1, and the average of
 * the stationary iterates, with its MCSE, is reported in place of the last one).  No reference counterpart: the reference runs
 * max_iters steps and reports the last iterate (src/vi.jl:201).  A handle on which no trace was begun behaves as without these calls.
 *
 * bb_trace_begin allocates a ring of `capacity` snapshots (8 .. BB_TRACE_MAX_SNAPSHOTS) on the handle's device; a snapshot is the
 * handle's (mu, omega), 2 D doubles, in the handle's internal order.  every >= 1.  Outside those ranges, or a null h / o:
 * BB_ERR_INVALID.  What the device cannot allocate is BB_ERR_DEVICE, and no trace is on.  A second begin on a handle under trace is
 * BB_ERR_INVALID.  Sharded handles (world_size > 1) and multi-device handles (n_devices > 1): BB_ERR_UNSUPPORTED (after a resident
 * run only the owner's theta is current on them).
 *
 * bb_run(h, n) under a trace.  Let t be the steps bb_run has taken since begin (or since the last reset, below).  Snapshot s
 * (0-based, kept in slot s mod capacity) is (mu, omega) after trace step (s + 1) every.  The call makes exactly the launches that
 * consecutive bb_run calls make when cut at those boundaries (every = 3, t = 1, n = 6: pieces of 2, 3 and 1 steps), and after a
 * piece that ends on a boundary a snapshot kernel on the handle's stream copies the two arrays into the ring.  The result is, bit
 * for bit, what an untraced twin handle holds after the same sequence of bb_run calls: parameters, optimiser state, step counter,
 * ELBO ring, bb_stats.steps_done.  (A cut run is not promised to equal an uncut one bit for bit: bb_run never promised that.)
 * BB_ERR_NONFINITE: the steps are taken and the snapshots recorded, non-finite values included.  BB_ERR_DEVICE from a piece ends
 * the call there.  On the two-kernel step (bb_stats.resident_kernel == 0) the pieces and snapshots are enqueued back to back and
 * the host waits once; a resident launch reports through status words the host reads after the stream has drained, so there the
 * host waits after every piece.
 *
 * While a trace is on: bb_init_meanfield and bb_set_params discard the snapshots and set t to 0 (the trace stays on);
 * bb_run_profiled, bb_step_moments and bb_step_apply are refused with BB_ERR_UNSUPPORTED; every other entry point is unaffected and
 * leaves the trace as it is.  bb_destroy frees the ring.
 *
 * bb_trace_end frees the ring; without a trace it is BB_OK.  bb_trace_count: *taken = the snapshots recorded since begin or the
 * last reset, *first_live = max(0, taken - capacity), the oldest snapshot the ring still holds (either pointer may be NULL; no
 * trace on: BB_ERR_INVALID).  bb_trace_get returns snapshots first .. first + n - 1 in the caller's latent order (either array may
 * be NULL); all of them must be live, else BB_ERR_INVALID with a message naming the live range.
 *
 * bb_trace_summary runs the statistics of bb_chain_summary on the ring, on the device, with nothing uploaded.  The window is the
 * W N = n_chains n_draws live snapshots from `first`, chain c the consecutive segment first + c N .. first + (c + 1) N - 1; it may
 * straddle the ring's wrap.  There are 2 D columns: column i < D is mu of the caller's latent i, column D + i its omega.
 * max_lag and slab_cols as bb_chain_opts'.  Per-column outputs (each [2 D], each pointer may be NULL; what is NULL is not
 * downloaded) equal, bit for bit, bb_chain_summary's with the same n_chains, n_draws, max_lag and no quantiles on the host array
 * [W][N][2 D] built from bb_trace_get: the same two kernels run on slabs a device-side gather fills from the ring (a column's result
 * does not depend on its position or its slab, so the slabs are cut in the handle's internal order).
 *
 * blocks (may be NULL): [2 n_blocks] verdicts, n_blocks that of bb_get_layout: the mu part of every layout block in layout order,
 * then the omega parts, reduced on the device over the block's columns with integer counts and max / min only (no order matters):
 *   n_cols        columns of the part (the block's length)
 *   n_nonfinite   columns whose mean is NaN (a non-finite value in the window)
 *   n_const       columns with sd == 0
 *   n_above       columns with a finite rhat > rhat_max
 *   max_rhat, min_ess   over the columns where they are finite; NaN if there are none
 *   max_mcse_rel  the MCSE of the averaged iterate in units that mean something, the max over the columns where it is finite
 *                 (NaN if none): for a mu column i, mcse_i / softplus(mean_{D+i}), the error of the mean in posterior sds; for an
 *                 omega column, mcse_{D+i} sigmoid(mean_{D+i}) / softplus(mean_{D+i}), the relative error of sigma by the delta
 *                 method (softplus and sigmoid those of the step kernels).
 * The handle's mu, omega, optimiser state, step counter and RNG position are untouched, bitwise; so is the ring.
 * BB_ERR_INVALID: a null h / o / out; no trace on; a window not wholly live (the message names the live range); n_chains < 1;
 * n_draws < 4; a negative max_lag or slab_cols; rhat_max not finite or < 1.  BB_ERR_UNSUPPORTED: W N > BB_CHAIN_MAX_K. */
#define BB_TRACE_MAX_SNAPSHOTS 16384            /* == BB_CHAIN_MAX_K */
typedef struct bb_trace_opts {
    int32_t every;            /* a snapshot after every `every` steps, >= 1            */
    int32_t capacity;         /* snapshots the ring holds, 8 .. BB_TRACE_MAX_SNAPSHOTS */
} bb_trace_opts;
typedef struct bb_trace_sum_opts {
    int64_t first;            /* first snapshot of the window                          */
    int32_t n_chains;         /* W >= 1 consecutive segments                           */
    int32_t n_draws;          /* N >= 4 snapshots per segment; W N <= BB_CHAIN_MAX_K   */
    int32_t max_lag;          /* as bb_chain_opts                                      */
    int32_t reserved0;
    int64_t slab_cols;        /* as bb_chain_opts                                      */
    double rhat_max;          /* n_above's threshold, finite and >= 1                  */
} bb_trace_sum_opts;
typedef struct bb_trace_block {
    char name[24];            /* the layout block's name                               */
    int32_t part;             /* 0 mu, 1 omega                                         */
    int32_t reserved0;
    int64_t n_cols, n_nonfinite, n_const, n_above;
    double max_rhat, min_ess, max_mcse_rel;
} bb_trace_block;
typedef struct bb_trace_sum_out {     /* every pointer may be NULL                     */
    double *mean, *sd, *mcse, *ess, *rhat;      /* [2 D]                               */
    int32_t* n_lags;                  /* [2 D]                                         */
    bb_trace_block* blocks;           /* [2 n_blocks]                                  */
} bb_trace_sum_out;
int bb_trace_begin(bb_handle* h, const bb_trace_opts* o);
int bb_trace_end(bb_handle* h);
int bb_trace_count(bb_handle* h, int64_t* taken, int64_t* first_live);
int bb_trace_get(bb_handle* h, int64_t first, int64_t n, double* mu /* [n][D] */, double* omega /* [n][D] */);
int bb_trace_summary(bb_handle* h, const bb_trace_sum_opts* o, const bb_trace_sum_out* out);

/* The engine's normal stream for (step, stream) over latents [lo, hi), for checks. */
int bb_debug_normals(bb_handle* h, int64_t step, uint32_t stream, int64_t lo, int64_t hi, double* out);

/* One fp64 function of the kernels' math header (csrc/bb_math.h), or the Box-Muller step of the normal stream, evaluated on the
 * device at n caller-chosen arguments, for accuracy checks: out0[i] (and out1[i]) = fn(x[i] (, y[i])).  Arguments outside a
 * function's stated domain give what the kernels would get.
 *   fn                          operands                                   results
 *   BB_MATH_EXP, _LOG, _RCP, _SQRT, _EXP_NONPOS, _LOG_1TO2    x            out0
 *   BB_MATH_DIV                 x / y                                      out0
 *   BB_MATH_SOFTPLUS_SIGMOID    x                                          out0 = softplus, out1 = sigmoid
 *   BB_MATH_SINCOSPI            x in [0, 2)                                out0 = sin(pi x), out1 = cos(pi x)
 *   BB_MATH_BOX_MULLER          the two 64-bit words of a Philox output,   out0, out1 = the pair of normals (cosine, sine branch)
 *                               as the bit patterns of x[i] and y[i]
 * y and out1 may be NULL where fn does not use them.  BB_ERR_INVALID: unknown fn, n < 0, a NULL pointer fn needs.  n = 0: no launch. */
#define BB_MATH_EXP 0
#define BB_MATH_LOG 1
#define BB_MATH_RCP 2
#define BB_MATH_DIV 3
#define BB_MATH_SQRT 4
#define BB_MATH_SOFTPLUS_SIGMOID 5
#define BB_MATH_SINCOSPI 6
#define BB_MATH_EXP_NONPOS 7
#define BB_MATH_LOG_1TO2 8
#define BB_MATH_BOX_MULLER 9
#define BB_MATH_COUNT 10
int bb_debug_math(bb_handle* h, int32_t fn, int64_t n, const double* x, const double* y, double* out0, double* out1);

/* s_memtime stamps at the pass boundaries of the last launches, [n_blocks][32]; all zero unless
 * the library was built with -DBB_STAMPS (diagnostic build, never the shipped one). */
int bb_debug_stamps(bb_handle* h, uint64_t* out, int64_t n);

/* Test hook: the optimiser's state beside the parameters, as the device holds it after the last run, in the handle's INTERNAL latent
 * order (bb_get_permutation) -- acc_mu, acc_omega [D]: TruncatedADAGrad's running window sums / DecayedADAGrad's accumulators;
 * lo [2 D]: the low-order parts of the compensated window sums, (mu, omega) per latent.  Not on a multi-device handle. */
int bb_debug_opt_state(bb_handle* h, double* acc_mu, double* acc_omega, float* lo);

/* hipGraphLaunch calls of the last bb_run on this handle: 0 when the run was a resident launch or went eagerly (ELBO recording on,
 * steps_per_graph < 0, fewer steps than one graph, or a capture that failed), and always 0 in the emulation. */
int bb_debug_graph_launches(bb_handle* h);

int bb_get_stats(bb_handle* h, bb_stats* out);
/* The kernel bb_run launches on this handle, as text: the selected template instance with its arguments in declaration order --
 * "k_res<KIND,P,NT,XG,TT,AP,MS>" (bb_resident.h), "k_stream<KIND,NT,TT>" (bb_stream.h), "k_persist<KIND,P,NT[,XG]>" (bb_persist.h) --
 * or "k_sample<KIND> + k_update<KIND>" for the two-kernel step.  buf: [len], always terminated.  No reference counterpart. */
int bb_kernel_name(bb_handle* h, char* buf, int64_t len);

/* ---- sharded execution -------------------------------------------------------------
 * Barcodes shard over world_size handles (one process per GPU).  Per MC sample the
 * only exchange is the sum of K = bb_stats.n_moments doubles.
 *
 * (1) in-library: RCCL over xGMI.  Rank 0 makes an id, the caller broadcasts it
 *     (e.g. torch.distributed), every rank calls bb_comm_init; bb_run then issues one
 *     ncclAllReduce per sample on the engine's stream. */
#define BB_COMM_ID_BYTES 128
int bb_comm_make_id(void* id_out /* BB_COMM_ID_BYTES */);
int bb_comm_init(bb_handle* h, const void* id /* BB_COMM_ID_BYTES */);
/* (2) split-phase, caller-supplied reducer (MPI, gloo, Julia Distributed ...):
 *     bb_step_moments runs the sampling sweep of the next MC sample and returns this
 *     shard's K partial moments; the caller sums them over shards and passes the
 *     totals to bb_step_apply, which finishes the sample (and the step after the
 *     S-th sample). */
int bb_step_moments(bb_handle* h, double* partial /* K */);
int bb_step_apply(bb_handle* h, const double* total /* K */);

#ifdef __cplusplus
}
#endif
#endif /* BARBAY_HIP_H */
