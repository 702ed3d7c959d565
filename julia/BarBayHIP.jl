# BarBayHIP.jl -- reference-side binding of libbarbay_hip.so (include/barbay_hip.h).
#
# UNTESTED IN THIS REPOSITORY'S IMAGE (no `julia`); written against Julia 1.x `ccall` semantics and kept
# line-for-line with the Python binding barbay.jl_amd/_capi.py, which IS tested.  It replaces exactly
#     q = Turing.vi(bayes_model, advi; optimizer=opt)                      (BarBay.jl src/vi.jl:201)
# and returns an object with the three fields `BarBay.utils.advi_to_df` reads
# (`q.dist.m`, `q.dist.σ`, `q.transform.ranges_out`; src/utils.jl:1049, 1060).
module BarBayHIP

const LIB = get(ENV, "BARBAY_HIP_LIB", joinpath(@__DIR__, "..", "barbay.jl_amd", "lib", "libbarbay_hip.so"))

struct bb_prior
    mean::Ptr{Float64}
    std::Ptr{Float64}
    n::Int64
end
bb_prior() = bb_prior(C_NULL, C_NULL, 0)

struct bb_model_desc
    kind::Int32
    n_rep::Int32
    n_neutral::Int64
    n_bc::Int64
    n_time::Ptr{Int32}
    counts::Ptr{Int64}
    totals::Ptr{Int64}
    n_env::Int32
    env_idx::Ptr{Int32}
    n_geno::Int32
    geno_idx::Ptr{Int32}
    s_pop_prior::bb_prior
    logsigma_pop_prior::bb_prior
    s_bc_prior::bb_prior
    logsigma_bc_prior::bb_prior
    loglambda_prior::bb_prior
    logtau_prior::bb_prior
    flags::Int32
end

mutable struct bb_advi_opts
    samples_per_step::Int32
    optimizer::Int32
    eta::Float64
    tau::Float64
    window::Int32
    resum_every::Int32
    pre::Float64
    post::Float64
    seed::UInt64
    device::Int32
    rank::Int32
    world_size::Int32
    steps_per_graph::Int32
    elbo_every::Int32
    launch_mode::Int32
    n_devices::Int32
    device_ids::Ptr{Int32}
    bb_advi_opts() = new()
end

struct bb_block_range
    name::NTuple{24,UInt8}
    lo::Int64
    hi::Int64
end

check(rc) = rc == 0 || error("barbay_hip: " * unsafe_string(ccall((:bb_last_error, LIB), Cstring, ())))

# what advi_to_df needs from `q`
struct Dist; m::Vector{Float64}; σ::Vector{Float64}; end
struct Transform; ranges_out::Vector{UnitRange{Int}}; end
struct Posterior
    dist::Dist
    transform::Transform
    hier::Union{Nothing,NamedTuple}     # device-side `process_hierarchical_samples!` result (median, std per θ̃ unit), if any
end

const KIND = Dict("fitness_normal" => 0, "multienv_fitness_normal" => 1, "genotype_fitness_normal" => 2,
                  "replicate_fitness_normal" => 3, "multienv_replicate_fitness_normal" => 4)

"""
    group_genotypes(data; genotype_col=:genotype, neutral_col=:neutral) -> data

Stable reorder of a tidy frame's rows so that the mutant barcodes of one genotype are consecutive (genotypes in order of first
appearance).  NOT needed any more: `bb_create` groups the mutants itself where `geno_idx` is not in consecutive runs and presents
the caller's order at the ABI (`bb_get_permutation` tells the mapping); kept as a convenience.  Results are
keyed by barcode id, so the order is the caller's to choose.  (`data_to_arrays` keeps barcodes in order of appearance,
src/utils.jl:692-731.)  Works on any Tables.jl-style object with `getproperty` columns and `data[perm, :]` indexing (DataFrame).
"""
function group_genotypes(data; genotype_col::Symbol=:genotype, neutral_col::Symbol=:neutral)
    g = getproperty(data, genotype_col)
    neutral = getproperty(data, neutral_col)
    first_seen = Dict{eltype(g),Int}()
    for x in g
        get!(first_seen, x, length(first_seen) + 1)
    end
    key = [neutral[i] ? 0 : first_seen[g[i]] for i in eachindex(g)]        # neutrals keep their place in front
    return data[sortperm(key; alg=MergeSort), :]
end

# prior kwarg (`VecOrMat{Float64}`) -> (mean, std) vectors kept alive by the caller
_prior_arrays(p::Vector{Float64}) = ([p[1]], [p[2]])
_prior_arrays(p::Matrix{Float64}) = (p[:, 1], p[:, 2])

"""
    vi(model_name, R, n_t, n_neutral, n_bc; samples_per_step, max_iters, optimizer, priors..., envs, genotypes, seed)

Drop-in for `Turing.vi(bayes_model, advi; optimizer=opt)`.  `devices = collect(0:7)` runs the one call on all GPUs of the node.  `R` / `n_t` are `data_arrays.bc_count` /
`data_arrays.bc_total` exactly as `utils.data_to_arrays` returns them (Matrix, 3-D Array or Vector{Matrix}).
"""
function vi(model_name::String, R, n_t, n_neutral::Int, n_bc::Int;
            samples_per_step::Int=1, max_iters::Int=10_000,
            optimizer::Symbol=:TruncatedADAGrad, eta=0.1, tau=40.0, n=100, pre=1.0, post=0.9,
            priors::Dict{Symbol,<:Any}=Dict{Symbol,Any}(), envs=nothing, genotypes=nothing,
            seed::Integer=0, device::Integer=0, devices::Vector{<:Integer}=Int[], hier_samples::Integer=10_000, verbose::Bool=false)
    mats = R isa Vector ? R : (ndims(R) == 3 ? [R[:, :, r] for r in axes(R, 3)] : [R])
    tots = n_t isa Vector{<:Vector} ? n_t : (ndims(n_t) == 2 ? [n_t[:, r] for r in axes(n_t, 2)] : [n_t])
    n_time = Int32[size(m, 1) for m in mats]
    counts = reduce(vcat, vec.(mats))              # column-major T x B, t fastest: passed as is
    totals = reduce(vcat, tots)
    # env list per replicate, replicate-major (the 3-D multienv_replicate method repeats its one list per replicate)
    envs_rep = envs === nothing ? nothing : (envs isa Vector{<:Vector} ? envs : [envs for _ in mats])
    env_flat = envs_rep === nothing ? nothing : reduce(vcat, envs_rep)
    env_idx = env_flat === nothing ? Int32[] : Int32.(indexin(env_flat, unique(env_flat)) .- 1)
    geno_idx = genotypes === nothing ? Int32[] : Int32.(indexin(genotypes, unique(genotypes)) .- 1)
    pa = Dict(k => _prior_arrays(v) for (k, v) in priors)
    pr(k) = haskey(pa, k) ? bb_prior(pointer(pa[k][1]), pointer(pa[k][2]), length(pa[k][1])) : bb_prior()
    opts = bb_advi_opts()
    ccall((:bb_default_opts, LIB), Cvoid, (Ref{bb_advi_opts},), opts)
    opts.samples_per_step = samples_per_step
    opts.optimizer = optimizer == :TruncatedADAGrad ? 0 : 1
    opts.eta, opts.tau, opts.window, opts.pre, opts.post = eta, tau, n, pre, post
    opts.seed, opts.device = seed, device
    # devices = [0, 1, ..., 7]: this one call drives all of them (the barcodes shard over the devices inside the library,
    # resident launches exchanging over xGMI); empty or one entry: a single GPU
    dev_ids = Int32.(devices)
    if length(dev_ids) > 1
        opts.n_devices, opts.device_ids = length(dev_ids), pointer(dev_ids)
    elseif length(dev_ids) == 1
        opts.device = dev_ids[1]
    end
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve n_time counts totals env_idx geno_idx pa dev_ids begin
        md = bb_model_desc(KIND[model_name], length(mats), n_neutral, n_bc, pointer(n_time), pointer(counts),
                           pointer(totals), isempty(env_idx) ? 0 : maximum(env_idx) + 1,
                           isempty(env_idx) ? C_NULL : pointer(env_idx),
                           isempty(geno_idx) ? 0 : maximum(geno_idx) + 1,
                           isempty(geno_idx) ? C_NULL : pointer(geno_idx),
                           pr(:s_pop_prior), pr(:logσ_pop_prior), pr(:s_bc_prior), pr(:logσ_bc_prior),
                           pr(:logλ_prior), pr(:logτ_prior),
                           Int32(R isa Vector ? 1 : 0))   # BB_FLAG_RAGGED_METHOD: the Vector{Matrix} method was dispatched
        check(ccall((:bb_create, LIB), Cint, (Ref{bb_model_desc}, Ref{bb_advi_opts}, Ref{Ptr{Cvoid}}), md, opts, h))
    end
    try
        if verbose      # (`BarBay.vi.advi(...; verbose)`, src/vi.jl:122-124): which kernel the run launches -- bb_kernel_name
            nm = Vector{UInt8}(undef, 128)
            check(ccall((:bb_kernel_name, LIB), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Int64), h[], nm, 128))
            @info "BarBayHIP: " * unsafe_string(pointer(nm))
        end
        check(ccall((:bb_run, LIB), Cint, (Ptr{Cvoid}, Int64), h[], max_iters))
        D = ccall((:bb_num_latents, LIB), Int64, (Ptr{Cvoid},), h[])
        m, s = Vector{Float64}(undef, D), Vector{Float64}(undef, D)
        check(ccall((:bb_get_posterior, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), h[], m, s))
        blocks = Vector{bb_block_range}(undef, 8)
        nb = Ref{Int32}(0)
        check(ccall((:bb_get_layout, LIB), Cint, (Ptr{Cvoid}, Ptr{bb_block_range}, Ref{Int32}), h[], blocks, nb))
        ranges = [Int(b.lo)+1:Int(b.hi) for b in blocks[1:nb[]]]
        hier = nothing
        nu = ccall((:bb_hier_units, LIB), Int64, (Ptr{Cvoid},), h[])
        if nu > 0 && hier_samples > 0          # src/utils.jl:1284-1343 on the device: 10 000 draws per unit, median + std
            med, sd = Vector{Float64}(undef, nu), Vector{Float64}(undef, nu)
            check(ccall((:bb_hier_fitness, LIB), Cint, (Ptr{Cvoid}, Int32, UInt64, Ptr{Float64}, Ptr{Float64}),
                        h[], hier_samples, seed, med, sd))
            hier = (n_samples=hier_samples, median=med, std=sd)
        end
        return Posterior(Dist(m, s), Transform(ranges), hier)
    finally
        ccall((:bb_destroy, LIB), Cvoid, (Ptr{Cvoid},), h[])
    end
end

# Posterior predictive bands of the log-frequency ratios (bb_ppc_bands, include/barbay_hip.h): the device's
# logfreq_ratio_popmean_ppc / logfreq_ratio_bc_ppc / logfreq_ratio_multienv_ppc + matrix_quantile_range for every row at once.
# Field for field the Python binding's `bb_ppc_opts` (barbay.jl_amd/_capi.py).
struct bb_ppc_opts
    n_samples::Int32
    n_ppc::Int32
    n_quantiles::Int32
    reserved0::Int32
    quantiles::Ptr{Float64}
    seed::UInt64
end

"""
    ppc_bands(h, quantiles; n_samples=1000, n_ppc=10, seed=0, outside=true) -> (bands, n_outside)

`h` a live `bb_handle` (e.g. the one `vi` drives, before `bb_destroy`).  `bands[q, side, t, row]` (Julia order of the
C array [row][t][q][2]; side 1 lower, 2 upper; NaN past a shorter replicate's last step); rows: the n_rep population-mean
rows, then mutant m of replicate r at n_rep + r n_bc + m (0-based).  `n_outside[row]`: finite observed ratios outside the
band of the largest q, or `nothing`.
"""
function ppc_bands(h::Ptr{Cvoid}, quantiles::Vector{Float64}; n_samples::Int=1000, n_ppc::Int=10, seed::Integer=0,
                   outside::Bool=true)
    nr, nt = Ref{Int64}(0), Ref{Int32}(0)
    check(ccall((:bb_ppc_shape, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int32}), h, nr, nt))
    bands = Array{Float64}(undef, 2, length(quantiles), nt[], nr[])
    nout = outside ? zeros(Int64, nr[]) : nothing
    GC.@preserve quantiles begin
        o = bb_ppc_opts(Int32(n_samples), Int32(n_ppc), Int32(length(quantiles)), Int32(0), pointer(quantiles), UInt64(seed))
        check(ccall((:bb_ppc_bands, LIB), Cint, (Ptr{Cvoid}, Ref{bb_ppc_opts}, Ptr{Float64}, Ptr{Int64}),
                    h, o, bands, outside ? nout : C_NULL))
    end
    return bands, nout
end

# Frequency-trajectory bands (bb_freq_bands, include/barbay_hip.h): the device's freq_bc_ppc + matrix_quantile_range for every
# barcode at once, neutrals included, or the posterior of the model's own frequencies exp(loglambda) / sum.
# Field for field the Python binding's `bb_freq_opts` (barbay.jl_amd/_capi.py).
const BB_FREQ_TRAJECTORY = Int32(0)
const BB_FREQ_POSTERIOR = Int32(1)
struct bb_freq_opts
    mode::Int32
    n_samples::Int32
    n_ppc::Int32
    n_quantiles::Int32
    quantiles::Ptr{Float64}
    seed::UInt64
end

"""
    freq_bands(h, quantiles; mode=BB_FREQ_TRAJECTORY, n_samples=1000, n_ppc=10, seed=0, outside=true) -> (bands, n_outside)

`h` a live `bb_handle`.  `bands[side, q, t, row]` (Julia order of the C array [row][t][q][2]; side 1 lower, 2 upper; NaN past a
shorter replicate's last time point); rows: data column b of replicate r at r (n_neutral + n_bc) + b (0-based), neutrals first;
columns: time points.  `mode=BB_FREQ_POSTERIOR` takes `n_ppc=1`.  `n_outside[row]`: time points whose observed frequency lies
outside the band of the largest q, or `nothing`.
"""
function freq_bands(h::Ptr{Cvoid}, quantiles::Vector{Float64}; mode::Integer=BB_FREQ_TRAJECTORY, n_samples::Int=1000,
                    n_ppc::Int=10, seed::Integer=0, outside::Bool=true)
    nr, nt = Ref{Int64}(0), Ref{Int32}(0)
    check(ccall((:bb_freq_shape, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int32}), h, nr, nt))
    bands = Array{Float64}(undef, 2, length(quantiles), nt[], nr[])
    nout = outside ? zeros(Int64, nr[]) : nothing
    GC.@preserve quantiles begin
        o = bb_freq_opts(Int32(mode), Int32(n_samples), Int32(n_ppc), Int32(length(quantiles)), pointer(quantiles), UInt64(seed))
        check(ccall((:bb_freq_bands, LIB), Cint, (Ptr{Cvoid}, Ref{bb_freq_opts}, Ptr{Float64}, Ptr{Int64}),
                    h, o, bands, outside ? nout : C_NULL))
    end
    return bands, nout
end

# Predictive log score and PIT of every observed log-frequency ratio (bb_ppc_score, include/barbay_hip.h): the per-barcode verdict
# beside the bands.  Field for field the Python binding's `bb_score_opts` / `bb_score_out` (barbay.jl_amd/_capi.py).
# Like the rest of this file it remains unexecuted (no `julia` where this repository is built and tested).
const BB_SCORE_MAX_SAMPLES = 16384
struct bb_score_opts
    n_samples::Int32
    reserved0::Int32
    seed::UInt64
end
struct bb_score_out
    observed::Ptr{Float64}
    pred_mean::Ptr{Float64}
    pred_sd::Ptr{Float64}
    lpd::Ptr{Float64}
    p_waic::Ptr{Float64}
    pit::Ptr{Float64}
    pit_upper::Ptr{Float64}
    row_lpd::Ptr{Float64}
    row_p_waic::Ptr{Float64}
    n_scored::Ptr{Int32}
end

"""
    ppc_score(h; n_samples=1000, seed=0) -> NamedTuple

`h` a live `bb_handle`.  Returns `observed, pred_mean, pred_sd, lpd, p_waic, pit, pit_upper` (each n_steps x n_rows: Julia order of
the C array [row][t]; NaN where the replicate has no such step or a count is 0) and `row_lpd, row_p_waic, n_scored` (n_rows each);
rows: data column b of replicate r at r (n_neutral + n_bc) + b (0-based), neutrals first, as `freq_bands`.  The log predictive
density and both tails of the predictive CDF at every observed log-frequency ratio, the n_samples posterior draws (those of
`ppc_bands` at equal seed) averaged in closed form; 2 <= n_samples <= BB_SCORE_MAX_SAMPLES.
"""
function ppc_score(h::Ptr{Cvoid}; n_samples::Int=1000, seed::Integer=0)
    nr, nt = Ref{Int64}(0), Ref{Int32}(0)
    check(ccall((:bb_score_shape, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int32}), h, nr, nt))
    observed, pred_mean, pred_sd, lpd, p_waic, pit, pit_upper = (Matrix{Float64}(undef, nt[], nr[]) for _ in 1:7)
    row_lpd, row_p_waic = Vector{Float64}(undef, nr[]), Vector{Float64}(undef, nr[])
    n_scored = Vector{Int32}(undef, nr[])
    GC.@preserve observed pred_mean pred_sd lpd p_waic pit pit_upper row_lpd row_p_waic n_scored begin
        o = bb_score_opts(Int32(n_samples), Int32(0), UInt64(seed))
        out = bb_score_out(pointer(observed), pointer(pred_mean), pointer(pred_sd), pointer(lpd), pointer(p_waic), pointer(pit),
                           pointer(pit_upper), pointer(row_lpd), pointer(row_p_waic), pointer(n_scored))
        check(ccall((:bb_ppc_score, LIB), Cint, (Ptr{Cvoid}, Ref{bb_score_opts}, Ref{bb_score_out}), h, o, out))
    end
    return (observed=observed, pred_mean=pred_mean, pred_sd=pred_sd, lpd=lpd, p_waic=p_waic, pit=pit, pit_upper=pit_upper,
            row_lpd=row_lpd, row_p_waic=row_p_waic, n_scored=n_scored)
end

# Pareto-smoothed importance-sampling leave-one-out scores of the observed log-frequency ratios (bb_ppc_loo, include/barbay_hip.h),
# per cell and per barcode, with the khat diagnostic.  Field for field the Python binding's `bb_loo_opts` / `bb_loo_out`
# (barbay.jl_amd/_capi.py).  Like the rest of this file it remains unexecuted (no `julia` where this repository is built and tested).
const BB_LOO_MAX_SAMPLES = 8192
struct bb_loo_opts
    n_samples::Int32
    reserved0::Int32
    seed::UInt64
end
struct bb_loo_out
    elpd_loo::Ptr{Float64}
    p_loo::Ptr{Float64}
    khat::Ptr{Float64}
    n_eff::Ptr{Float64}
    lpd::Ptr{Float64}
    row_elpd_loo::Ptr{Float64}
    row_p_loo::Ptr{Float64}
    row_khat::Ptr{Float64}
    row_n_eff::Ptr{Float64}
    row_elpd_cells::Ptr{Float64}
    row_khat_max::Ptr{Float64}
    n_scored::Ptr{Int32}
end

"""
    ppc_loo(h; n_samples=1000, seed=0) -> NamedTuple

`h` a live `bb_handle`.  Returns `elpd_loo, p_loo, khat, n_eff, lpd` (each n_steps x n_rows: Julia order of the C array [row][t];
NaN where the cell is unscored; khat = Inf where the tail was not smoothed) and, the barcode's whole trajectory left out,
`row_elpd_loo, row_p_loo, row_khat, row_n_eff`, with `row_elpd_cells, row_khat_max, n_scored` (n_rows each); rows and draws as
`ppc_score`, whose `lpd` this call's `lpd` equals byte for byte at equal seed; 2 <= n_samples <= BB_LOO_MAX_SAMPLES.
"""
function ppc_loo(h::Ptr{Cvoid}; n_samples::Int=1000, seed::Integer=0)
    nr, nt = Ref{Int64}(0), Ref{Int32}(0)
    check(ccall((:bb_loo_shape, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int32}), h, nr, nt))
    elpd_loo, p_loo, khat, n_eff, lpd = (Matrix{Float64}(undef, nt[], nr[]) for _ in 1:5)
    row_elpd_loo, row_p_loo, row_khat, row_n_eff, row_elpd_cells, row_khat_max = (Vector{Float64}(undef, nr[]) for _ in 1:6)
    n_scored = Vector{Int32}(undef, nr[])
    GC.@preserve elpd_loo p_loo khat n_eff lpd row_elpd_loo row_p_loo row_khat row_n_eff row_elpd_cells row_khat_max n_scored begin
        o = bb_loo_opts(Int32(n_samples), Int32(0), UInt64(seed))
        out = bb_loo_out(pointer(elpd_loo), pointer(p_loo), pointer(khat), pointer(n_eff), pointer(lpd), pointer(row_elpd_loo),
                         pointer(row_p_loo), pointer(row_khat), pointer(row_n_eff), pointer(row_elpd_cells), pointer(row_khat_max),
                         pointer(n_scored))
        check(ccall((:bb_ppc_loo, LIB), Cint, (Ptr{Cvoid}, Ref{bb_loo_opts}, Ref{bb_loo_out}), h, o, out))
    end
    return (elpd_loo=elpd_loo, p_loo=p_loo, khat=khat, n_eff=n_eff, lpd=lpd, row_elpd_loo=row_elpd_loo, row_p_loo=row_p_loo,
            row_khat=row_khat, row_n_eff=row_n_eff, row_elpd_cells=row_elpd_cells, row_khat_max=row_khat_max, n_scored=n_scored)
end

# Rao-Blackwellised marginals of the mutants' fitness (bb_fitness_rb, include/barbay_hip.h): every unit's exact Gaussian full
# conditional averaged over joint draws of everything else -- how far the mean-field +- can be trusted, per mutant.  Field for
# field the Python binding's `bb_rb_opts` / `bb_rb_out` (barbay.jl_amd/_capi.py).
# Like the rest of this file it remains unexecuted (no `julia` where this repository is built and tested).
const BB_RB_MAX_SAMPLES = 8672
struct bb_rb_opts
    n_samples::Int32
    n_quantiles::Int32
    probs::Ptr{Float64}
    threshold::Float64
    seed::UInt64
    draws::Ptr{Float64}
end
struct bb_rb_out
    q_mean::Ptr{Float64}
    q_sd::Ptr{Float64}
    rb_mean::Ptr{Float64}
    rb_sd::Ptr{Float64}
    p_pos::Ptr{Float64}
    p_neg::Ptr{Float64}
    quantiles::Ptr{Float64}
    n_steps::Ptr{Int32}
end

"""
    fitness_rb_shape(h) -> Int

Fitness units of `fitness_rb`: u = e + E m + E n_bc r (0-based: replicate r, mutant m in the caller's order, environment e), the
order of the s_bc block (fitness, multienv) or the theta_tilde block (hierarchical kinds).
"""
function fitness_rb_shape(h::Ptr{Cvoid})
    n = Ref{Int64}(0)
    check(ccall((:bb_fitness_rb_shape, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}), h, n))
    return Int(n[])
end

"""
    fitness_rb(h; n_samples=1000, probs=[0.025, 0.5, 0.975], threshold=0.0, seed=0, draws=nothing) -> NamedTuple

`h` a live `bb_handle`.  Returns `n_steps, q_mean, q_sd, rb_mean, rb_sd, p_pos, p_neg` (n_units each) and `quantiles`
(length(probs) x n_units: Julia order of the C array [unit][i]).  `draws`: a D x n matrix (one draw per COLUMN: Julia's
column-major D x n is the ABI's [n][D]), an MCMC chain say, read in place of the posterior's own draws; n_samples is then its
column count.  2 (1 with draws) <= n_samples <= BB_RB_MAX_SAMPLES; every prob strictly inside (0, 1).
"""
function fitness_rb(h::Ptr{Cvoid}; n_samples::Int=1000, probs::Vector{Float64}=[0.025, 0.5, 0.975], threshold::Real=0.0,
                    seed::Integer=0, draws::Union{Nothing,Matrix{Float64}}=nothing)
    nu, nq = fitness_rb_shape(h), length(probs)
    if draws !== nothing
        D = ccall((:bb_num_latents, LIB), Int64, (Ptr{Cvoid},), h)
        size(draws, 1) == D || error("fitness_rb: draws must have $D rows")
        n_samples = size(draws, 2)
    end
    q_mean, q_sd, rb_mean, rb_sd, p_pos, p_neg = (Vector{Float64}(undef, nu) for _ in 1:6)
    quantiles = Matrix{Float64}(undef, nq, nu)
    n_steps = Vector{Int32}(undef, nu)
    GC.@preserve probs draws q_mean q_sd rb_mean rb_sd p_pos p_neg quantiles n_steps begin
        o = bb_rb_opts(Int32(n_samples), Int32(nq), nq > 0 ? pointer(probs) : Ptr{Float64}(C_NULL), Float64(threshold), UInt64(seed),
                       draws === nothing ? Ptr{Float64}(C_NULL) : pointer(draws))
        out = bb_rb_out(pointer(q_mean), pointer(q_sd), pointer(rb_mean), pointer(rb_sd), pointer(p_pos), pointer(p_neg),
                        nq > 0 ? pointer(quantiles) : Ptr{Float64}(C_NULL), pointer(n_steps))
        check(ccall((:bb_fitness_rb, LIB), Cint, (Ptr{Cvoid}, Ref{bb_rb_opts}, Ref{bb_rb_out}), h, o, out))
    end
    return (n_steps=n_steps, q_mean=q_mean, q_sd=q_sd, rb_mean=rb_mean, rb_sd=rb_sd, p_pos=p_pos, p_neg=p_neg, quantiles=quantiles)
end

# Rao-Blackwellised marginals of the hyper-fitness theta of the hierarchical models (bb_theta_rb, include/barbay_hip.h): the exact
# Gaussian full conditional of a genotype's fitness, or of a mutant's across its replicates, summed over the members of its group
# and averaged over the draws of `fitness_rb`.  Field for field the Python binding's `bb_theta_rb_out` (barbay.jl_amd/_capi.py);
# the options are `bb_rb_opts`.  Like the rest of this file it remains unexecuted.
const BB_THETA_RB_CHUNK = 64
struct bb_theta_rb_out
    q_mean::Ptr{Float64}
    q_sd::Ptr{Float64}
    rb_mean::Ptr{Float64}
    rb_sd::Ptr{Float64}
    p_pos::Ptr{Float64}
    p_neg::Ptr{Float64}
    quantiles::Ptr{Float64}
    n_members::Ptr{Int32}
    n_steps::Ptr{Int32}
end

"""
    theta_rb_shape(h) -> Int

Groups of `theta_rb`: the length of the theta block (genotypes; g = e + E m, 0-based, for the replicate kinds); 0 for the models
without a theta.
"""
function theta_rb_shape(h::Ptr{Cvoid})
    n = Ref{Int64}(0)
    check(ccall((:bb_theta_rb_shape, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}), h, n))
    return Int(n[])
end

"""
    theta_rb(h; n_samples=1000, probs=[0.025, 0.5, 0.975], threshold=0.0, seed=0, draws=nothing) -> NamedTuple

`h` a live `bb_handle` of a hierarchical model.  Returns `n_members, n_steps, q_mean, q_sd, rb_mean, rb_sd, p_pos, p_neg` (n_groups
each) and `quantiles` (length(probs) x n_groups).  Arguments as for `fitness_rb`.
"""
function theta_rb(h::Ptr{Cvoid}; n_samples::Int=1000, probs::Vector{Float64}=[0.025, 0.5, 0.975], threshold::Real=0.0,
                  seed::Integer=0, draws::Union{Nothing,Matrix{Float64}}=nothing)
    ng, nq = theta_rb_shape(h), length(probs)
    if draws !== nothing
        D = ccall((:bb_num_latents, LIB), Int64, (Ptr{Cvoid},), h)
        size(draws, 1) == D || error("theta_rb: draws must have $D rows")
        n_samples = size(draws, 2)
    end
    q_mean, q_sd, rb_mean, rb_sd, p_pos, p_neg = (Vector{Float64}(undef, ng) for _ in 1:6)
    quantiles = Matrix{Float64}(undef, nq, ng)
    n_members = Vector{Int32}(undef, ng)
    n_steps = Vector{Int32}(undef, ng)
    GC.@preserve probs draws q_mean q_sd rb_mean rb_sd p_pos p_neg quantiles n_members n_steps begin
        o = bb_rb_opts(Int32(n_samples), Int32(nq), nq > 0 ? pointer(probs) : Ptr{Float64}(C_NULL), Float64(threshold), UInt64(seed),
                       draws === nothing ? Ptr{Float64}(C_NULL) : pointer(draws))
        out = bb_theta_rb_out(pointer(q_mean), pointer(q_sd), pointer(rb_mean), pointer(rb_sd), pointer(p_pos), pointer(p_neg),
                              nq > 0 ? pointer(quantiles) : Ptr{Float64}(C_NULL), pointer(n_members), pointer(n_steps))
        check(ccall((:bb_theta_rb, LIB), Cint, (Ptr{Cvoid}, Ref{bb_rb_opts}, Ref{bb_theta_rb_out}), h, o, out))
    end
    return (n_members=n_members, n_steps=n_steps, q_mean=q_mean, q_sd=q_sd, rb_mean=rb_mean, rb_sd=rb_sd, p_pos=p_pos, p_neg=p_neg,
            quantiles=quantiles)
end

# Rao-Blackwellised marginals of linear contrasts of fitnesses (bb_contrast_rb, include/barbay_hip.h): distinct fitness units (or
# distinct hyper-fitnesses) are conditionally independent given everything else, so the contrast's conditional is exactly Gaussian
# per draw, and what the terms share cancels or adds up draw by draw.  Field for field the Python binding's `bb_contrast_opts` /
# `bb_contrast_out` (barbay.jl_amd/_capi.py).  Like the rest of this file it remains unexecuted.
const BB_CONTRAST_FITNESS = Int32(0)
const BB_CONTRAST_THETA = Int32(1)
struct bb_contrast_opts
    space::Int32
    n_samples::Int32
    n_quantiles::Int32
    reserved0::Int32
    probs::Ptr{Float64}
    threshold::Float64
    seed::UInt64
    draws::Ptr{Float64}
    n_contrasts::Int64
    term_ptr::Ptr{Int64}
    term_idx::Ptr{Int64}
    term_w::Ptr{Float64}
end
struct bb_contrast_out
    q_mean::Ptr{Float64}
    q_sd::Ptr{Float64}
    rb_mean::Ptr{Float64}
    rb_sd::Ptr{Float64}
    p_pos::Ptr{Float64}
    p_neg::Ptr{Float64}
    quantiles::Ptr{Float64}
    min_steps::Ptr{Int32}
end

"""
    contrast_rb(h, terms; space=:fitness, n_samples=1000, probs=[0.025, 0.5, 0.975], threshold=0.0, seed=0, draws=nothing) -> NamedTuple

`h` a live `bb_handle`.  `terms`: a vector of contrasts, each a vector of `index => weight` pairs with the 0-based unit numbers of
`fitness_rb` (`space=:fitness`) or group numbers of `theta_rb` (`space=:theta`); every element at most once per contrast.  Returns
`min_steps, q_mean, q_sd, rb_mean, rb_sd, p_pos, p_neg` (one per contrast) and `quantiles` (length(probs) x n_contrasts).  The
remaining arguments as for `fitness_rb`.
"""
function contrast_rb(h::Ptr{Cvoid}, terms::Vector{<:Vector{<:Pair}}; space::Symbol=:fitness, n_samples::Int=1000,
                     probs::Vector{Float64}=[0.025, 0.5, 0.975], threshold::Real=0.0, seed::Integer=0,
                     draws::Union{Nothing,Matrix{Float64}}=nothing)
    space in (:fitness, :theta) || error("contrast_rb: space must be :fitness or :theta")
    nc, nq = length(terms), length(probs)
    if draws !== nothing
        D = ccall((:bb_num_latents, LIB), Int64, (Ptr{Cvoid},), h)
        size(draws, 1) == D || error("contrast_rb: draws must have $D rows")
        n_samples = size(draws, 2)
    end
    term_ptr = Int64.(cumsum(vcat(0, length.(terms))))
    term_idx = Int64[first(p) for t in terms for p in t]
    term_w = Float64[last(p) for t in terms for p in t]
    q_mean, q_sd, rb_mean, rb_sd, p_pos, p_neg = (Vector{Float64}(undef, nc) for _ in 1:6)
    quantiles = Matrix{Float64}(undef, nq, nc)
    min_steps = Vector{Int32}(undef, nc)
    GC.@preserve probs draws term_ptr term_idx term_w q_mean q_sd rb_mean rb_sd p_pos p_neg quantiles min_steps begin
        o = bb_contrast_opts(space == :theta ? BB_CONTRAST_THETA : BB_CONTRAST_FITNESS, Int32(n_samples), Int32(nq), Int32(0),
                             nq > 0 ? pointer(probs) : Ptr{Float64}(C_NULL), Float64(threshold), UInt64(seed),
                             draws === nothing ? Ptr{Float64}(C_NULL) : pointer(draws), Int64(nc), pointer(term_ptr), pointer(term_idx),
                             pointer(term_w))
        out = bb_contrast_out(pointer(q_mean), pointer(q_sd), pointer(rb_mean), pointer(rb_sd), pointer(p_pos), pointer(p_neg),
                              nq > 0 ? pointer(quantiles) : Ptr{Float64}(C_NULL), pointer(min_steps))
        check(ccall((:bb_contrast_rb, LIB), Cint, (Ptr{Cvoid}, Ref{bb_contrast_opts}, Ref{bb_contrast_out}), h, o, out))
    end
    return (min_steps=min_steps, q_mean=q_mean, q_sd=q_sd, rb_mean=rb_mean, rb_sd=rb_sd, p_pos=p_pos, p_neg=p_neg, quantiles=quantiles)
end

# Posterior of the distribution of fitness effects of sets of fitness units (bb_dfe_rb, include/barbay_hip.h): per set and
# threshold x the fraction of the set's units at or below (above) x, the units' exact Gaussian conditionals averaged over the draws
# of `fitness_rb`, so that what the units share -- the population mean fitness above all -- moves the whole curve draw by draw.
# Field for field the Python binding's `bb_dfe_opts` / `bb_dfe_out` (barbay.jl_amd/_capi.py).  Like the rest of this file it
# remains unexecuted.
const BB_DFE_CHUNK = 128
const BB_DFE_MAX_GRID = 64
const BB_DFE_MAX_SAMPLES = 8672
struct bb_dfe_opts
    n_samples::Int32
    n_quantiles::Int32
    n_grid::Int32
    reserved0::Int32
    probs::Ptr{Float64}
    grid::Ptr{Float64}
    seed::UInt64
    draws::Ptr{Float64}
    n_sets::Int64
    set_ptr::Ptr{Int64}
    set_idx::Ptr{Int64}
end
struct bb_dfe_out
    below_mean::Ptr{Float64}
    above_mean::Ptr{Float64}
    between_sd::Ptr{Float64}
    within_sd::Ptr{Float64}
    q_below_mean::Ptr{Float64}
    q_below_sd::Ptr{Float64}
    below_bands::Ptr{Float64}
    above_bands::Ptr{Float64}
    n_units::Ptr{Int64}
end

"""
    dfe_rb(h, sets, grid; probs=[0.025, 0.5, 0.975], n_samples=1000, seed=0, draws=nothing) -> NamedTuple

`h` a live `bb_handle`.  `sets`: a vector of sets, each a vector of 0-based unit numbers of `fitness_rb`, every unit at most once
per set; `grid`: finite, strictly ascending thresholds, at most `BB_DFE_MAX_GRID`.  Returns `below_mean, above_mean, between_sd,
within_sd, q_below_mean, q_below_sd` (n_grid x n_sets), `below_bands, above_bands` (length(probs) x n_grid x n_sets) and `n_units`
(one per set).  The total variance of the fraction below a threshold is `between_sd^2 + within_sd^2`.  The remaining arguments as
for `fitness_rb`.
"""
function dfe_rb(h::Ptr{Cvoid}, sets::Vector{<:Vector{<:Integer}}, grid::Vector{Float64}; probs::Vector{Float64}=[0.025, 0.5, 0.975],
                n_samples::Int=1000, seed::Integer=0, draws::Union{Nothing,Matrix{Float64}}=nothing)
    nc, ng, nq = length(sets), length(grid), length(probs)
    if draws !== nothing
        D = ccall((:bb_num_latents, LIB), Int64, (Ptr{Cvoid},), h)
        size(draws, 1) == D || error("dfe_rb: draws must have $D rows")
        n_samples = size(draws, 2)
    end
    set_ptr = Int64.(cumsum(vcat(0, length.(sets))))
    set_idx = Int64[u for s in sets for u in s]
    below_mean, above_mean, between_sd, within_sd, q_below_mean, q_below_sd = (Matrix{Float64}(undef, ng, nc) for _ in 1:6)
    below_bands, above_bands = (Array{Float64,3}(undef, nq, ng, nc) for _ in 1:2)
    n_units = Vector{Int64}(undef, nc)
    GC.@preserve probs grid draws set_ptr set_idx below_mean above_mean between_sd within_sd q_below_mean q_below_sd below_bands above_bands n_units begin
        o = bb_dfe_opts(Int32(n_samples), Int32(nq), Int32(ng), Int32(0), nq > 0 ? pointer(probs) : Ptr{Float64}(C_NULL), pointer(grid),
                        UInt64(seed), draws === nothing ? Ptr{Float64}(C_NULL) : pointer(draws), Int64(nc), pointer(set_ptr), pointer(set_idx))
        out = bb_dfe_out(pointer(below_mean), pointer(above_mean), pointer(between_sd), pointer(within_sd), pointer(q_below_mean),
                         pointer(q_below_sd), nq > 0 ? pointer(below_bands) : Ptr{Float64}(C_NULL),
                         nq > 0 ? pointer(above_bands) : Ptr{Float64}(C_NULL), pointer(n_units))
        check(ccall((:bb_dfe_rb, LIB), Cint, (Ptr{Cvoid}, Ref{bb_dfe_opts}, Ref{bb_dfe_out}), h, o, out))
    end
    return (n_units=n_units, below_mean=below_mean, above_mean=above_mean, between_sd=between_sd, within_sd=within_sd,
            q_below_mean=q_below_mean, q_below_sd=q_below_sd, below_bands=below_bands, above_bands=above_bands)
end

# Posterior ranks of the fitness units of sets and their top-k membership (bb_fitness_rank, include/barbay_hip.h): per joint draw
# of `fitness_rb` every unit is redrawn from its exact Gaussian conditional (one blocked Gibbs update of the fitness block, so that
# what the units share moves them together) or taken as the draw's own fitness, and ranked within each set; rank 0 is the fittest.
# Field for field the Python binding's `bb_rank_opts` / `bb_rank_out` (barbay.jl_amd/_capi.py).  Like the rest of this file it
# remains unexecuted.
const BB_RANK_CONDITIONAL = 0
const BB_RANK_DRAWS = 1
const BB_RANK_MAX_TOP = 8
const BB_RANK_RUN = 8192
const BB_RANK_MAX_SAMPLES = 8672
struct bb_rank_opts
    n_samples::Int32
    n_quantiles::Int32
    n_top::Int32
    source::Int32
    reserved0::Int32
    reserved1::Int32
    probs::Ptr{Float64}
    top::Ptr{Int64}
    seed::UInt64
    draws::Ptr{Float64}
    n_sets::Int64
    set_ptr::Ptr{Int64}
    set_idx::Ptr{Int64}
end
struct bb_rank_out
    rank_mean::Ptr{Float64}
    rank_sd::Ptr{Float64}
    p_top::Ptr{Float64}
    quantiles::Ptr{Float64}
    ranks::Ptr{Int32}
    n_units::Ptr{Int64}
end

"""
    fitness_rank(h, sets; top=[1, 10], probs=[0.025, 0.5, 0.975], source=BB_RANK_CONDITIONAL, n_samples=1000, seed=0,
                 draws=nothing, want_ranks=false) -> NamedTuple

`h` a live `bb_handle`.  `sets` as for `dfe_rb`.  Results are indexed by position in the concatenated sets (`set_ptr`, 0-based
offsets): `rank_mean, rank_sd` (one per position; 0 is the fittest), `p_top` (length(top) x n_idx: the fraction of the draws with
rank < top[i]), `quantiles` (length(probs) x n_idx, over the draws of the rank), `n_units` (one per set) and, with `want_ranks`,
`ranks` (n_samples x n_idx, Int32).  The remaining arguments as for `fitness_rb`.
"""
function fitness_rank(h::Ptr{Cvoid}, sets::Vector{<:Vector{<:Integer}}; top::Vector{<:Integer}=[1, 10], probs::Vector{Float64}=[0.025, 0.5, 0.975],
                      source::Integer=BB_RANK_CONDITIONAL, n_samples::Int=1000, seed::Integer=0,
                      draws::Union{Nothing,Matrix{Float64}}=nothing, want_ranks::Bool=false)
    nc, nq, nt = length(sets), length(probs), length(top)
    if draws !== nothing
        D = ccall((:bb_num_latents, LIB), Int64, (Ptr{Cvoid},), h)
        size(draws, 1) == D || error("fitness_rank: draws must have $D rows")
        n_samples = size(draws, 2)
    end
    set_ptr = Int64.(cumsum(vcat(0, length.(sets))))
    set_idx = Int64[u for s in sets for u in s]
    top64 = Int64.(top)
    nix = length(set_idx)
    rank_mean, rank_sd = Vector{Float64}(undef, nix), Vector{Float64}(undef, nix)
    p_top, quantiles = Matrix{Float64}(undef, nt, nix), Matrix{Float64}(undef, nq, nix)
    ranks = Matrix{Int32}(undef, want_ranks ? n_samples : 0, nix)
    n_units = Vector{Int64}(undef, nc)
    GC.@preserve probs top64 draws set_ptr set_idx rank_mean rank_sd p_top quantiles ranks n_units begin
        o = bb_rank_opts(Int32(n_samples), Int32(nq), Int32(nt), Int32(source), Int32(0), Int32(0),
                         nq > 0 ? pointer(probs) : Ptr{Float64}(C_NULL), nt > 0 ? pointer(top64) : Ptr{Int64}(C_NULL), UInt64(seed),
                         draws === nothing ? Ptr{Float64}(C_NULL) : pointer(draws), Int64(nc), pointer(set_ptr), pointer(set_idx))
        out = bb_rank_out(pointer(rank_mean), pointer(rank_sd), nt > 0 ? pointer(p_top) : Ptr{Float64}(C_NULL),
                          nq > 0 ? pointer(quantiles) : Ptr{Float64}(C_NULL), want_ranks ? pointer(ranks) : Ptr{Int32}(C_NULL), pointer(n_units))
        check(ccall((:bb_fitness_rank, LIB), Cint, (Ptr{Cvoid}, Ref{bb_rank_opts}, Ref{bb_rank_out}), h, o, out))
    end
    return (set_ptr=set_ptr, n_units=n_units, rank_mean=rank_mean, rank_sd=rank_sd, p_top=p_top, quantiles=quantiles, ranks=ranks)
end

# Rao-Blackwellised marginals of the population mean fitness sbar_g, g = (replicate, step) (bb_popmean_rb, include/barbay_hip.h):
# the exact Gaussian full conditional of a step's population mean, summed over every barcode of the replicate (neutrals, then
# mutants) and averaged over the draws of `fitness_rb`.  Field for field the Python binding's `bb_popmean_rb_out`
# (barbay.jl_amd/_capi.py); the options are `bb_rb_opts`.  Like the rest of this file it remains unexecuted.
const BB_POPMEAN_RB_CHUNK = 256
struct bb_popmean_rb_out
    q_mean::Ptr{Float64}
    q_sd::Ptr{Float64}
    rb_mean::Ptr{Float64}
    rb_sd::Ptr{Float64}
    p_pos::Ptr{Float64}
    p_neg::Ptr{Float64}
    quantiles::Ptr{Float64}
    n_members::Ptr{Int32}
end

"""
    popmean_rb_shape(h) -> Int

Groups of `popmean_rb`: the length of the s_pop block, g = (replicate, step), replicate-major.
"""
function popmean_rb_shape(h::Ptr{Cvoid})
    n = Ref{Int64}(0)
    check(ccall((:bb_popmean_rb_shape, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}), h, n))
    return Int(n[])
end

"""
    popmean_rb(h; n_samples=1000, probs=[0.025, 0.5, 0.975], threshold=0.0, seed=0, draws=nothing) -> NamedTuple

`h` a live `bb_handle` of any model.  Returns `n_members, q_mean, q_sd, rb_mean, rb_sd, p_pos, p_neg` (n_groups each) and
`quantiles` (length(probs) x n_groups).  Arguments as for `fitness_rb`.
"""
function popmean_rb(h::Ptr{Cvoid}; n_samples::Int=1000, probs::Vector{Float64}=[0.025, 0.5, 0.975], threshold::Real=0.0,
                    seed::Integer=0, draws::Union{Nothing,Matrix{Float64}}=nothing)
    ng, nq = popmean_rb_shape(h), length(probs)
    if draws !== nothing
        D = ccall((:bb_num_latents, LIB), Int64, (Ptr{Cvoid},), h)
        size(draws, 1) == D || error("popmean_rb: draws must have $D rows")
        n_samples = size(draws, 2)
    end
    q_mean, q_sd, rb_mean, rb_sd, p_pos, p_neg = (Vector{Float64}(undef, ng) for _ in 1:6)
    quantiles = Matrix{Float64}(undef, nq, ng)
    n_members = Vector{Int32}(undef, ng)
    GC.@preserve probs draws q_mean q_sd rb_mean rb_sd p_pos p_neg quantiles n_members begin
        o = bb_rb_opts(Int32(n_samples), Int32(nq), nq > 0 ? pointer(probs) : Ptr{Float64}(C_NULL), Float64(threshold), UInt64(seed),
                       draws === nothing ? Ptr{Float64}(C_NULL) : pointer(draws))
        out = bb_popmean_rb_out(pointer(q_mean), pointer(q_sd), pointer(rb_mean), pointer(rb_sd), pointer(p_pos), pointer(p_neg),
                                nq > 0 ? pointer(quantiles) : Ptr{Float64}(C_NULL), pointer(n_members))
        check(ccall((:bb_popmean_rb, LIB), Cint, (Ptr{Cvoid}, Ref{bb_rb_opts}, Ref{bb_popmean_rb_out}), h, o, out))
    end
    return (n_members=n_members, q_mean=q_mean, q_sd=q_sd, rb_mean=rb_mean, rb_sd=rb_sd, p_pos=p_pos, p_neg=p_neg, quantiles=quantiles)
end

# Rao-Blackwellised marginals of the noise scales logsigma_bc / logsigma_pop (bb_logsigma_rb, include/barbay_hip.h): the
# one-dimensional, log-concave full conditional of a log-scale integrated numerically per draw and averaged over the draws of
# `fitness_rb`.  Field for field the Python binding's `bb_logsigma_rb_opts` / `bb_logsigma_rb_out` (barbay.jl_amd/_capi.py).  Like the
# rest of this file it remains unexecuted.
const BB_LOGSIGMA_BC = Int32(0)
const BB_LOGSIGMA_POP = Int32(1)
const BB_LOGSIGMA_RB_MAX_SAMPLES = 5781
struct bb_logsigma_rb_opts
    block::Int32
    n_samples::Int32
    n_quantiles::Int32
    reserved0::Int32
    probs::Ptr{Float64}
    seed::UInt64
    draws::Ptr{Float64}
end
struct bb_logsigma_rb_out
    q_mean::Ptr{Float64}
    q_sd::Ptr{Float64}
    rb_mean::Ptr{Float64}
    rb_sd::Ptr{Float64}
    sigma_mean::Ptr{Float64}
    mode_mean::Ptr{Float64}
    quantiles::Ptr{Float64}
    n_terms::Ptr{Int32}
end

logsigma_block(block::Symbol) = block === :bc ? BB_LOGSIGMA_BC : block === :pop ? BB_LOGSIGMA_POP : error("logsigma_rb: block must be :bc or :pop")

"""
    logsigma_rb_shape(h; block=:bc) -> Int

Entries of `logsigma_rb`: the length of the logsigma_bc (`:bc`) or logsigma_pop (`:pop`) block.
"""
function logsigma_rb_shape(h::Ptr{Cvoid}; block::Symbol=:bc)
    n = Ref{Int64}(0)
    check(ccall((:bb_logsigma_rb_shape, LIB), Cint, (Ptr{Cvoid}, Int32, Ref{Int64}), h, logsigma_block(block), n))
    return Int(n[])
end

"""
    logsigma_rb(h; block=:bc, n_samples=1000, probs=[0.025, 0.5, 0.975], seed=0, draws=nothing) -> NamedTuple

`h` a live `bb_handle` of any model.  Returns `n_terms, q_mean, q_sd, rb_mean, rb_sd, sigma_mean, mode_mean` (n_entries each) and
`quantiles` (length(probs) x n_entries; of logsigma, their `exp` are sigma's).  Arguments as for `fitness_rb`, without a threshold.
"""
function logsigma_rb(h::Ptr{Cvoid}; block::Symbol=:bc, n_samples::Int=1000, probs::Vector{Float64}=[0.025, 0.5, 0.975],
                     seed::Integer=0, draws::Union{Nothing,Matrix{Float64}}=nothing)
    ne, nq = logsigma_rb_shape(h; block=block), length(probs)
    if draws !== nothing
        D = ccall((:bb_num_latents, LIB), Int64, (Ptr{Cvoid},), h)
        size(draws, 1) == D || error("logsigma_rb: draws must have $D rows")
        n_samples = size(draws, 2)
    end
    q_mean, q_sd, rb_mean, rb_sd, sigma_mean, mode_mean = (Vector{Float64}(undef, ne) for _ in 1:6)
    quantiles = Matrix{Float64}(undef, nq, ne)
    n_terms = Vector{Int32}(undef, ne)
    GC.@preserve probs draws q_mean q_sd rb_mean rb_sd sigma_mean mode_mean quantiles n_terms begin
        o = bb_logsigma_rb_opts(logsigma_block(block), Int32(n_samples), Int32(nq), Int32(0), nq > 0 ? pointer(probs) : Ptr{Float64}(C_NULL),
                                UInt64(seed), draws === nothing ? Ptr{Float64}(C_NULL) : pointer(draws))
        out = bb_logsigma_rb_out(pointer(q_mean), pointer(q_sd), pointer(rb_mean), pointer(rb_sd), pointer(sigma_mean), pointer(mode_mean),
                                 nq > 0 ? pointer(quantiles) : Ptr{Float64}(C_NULL), pointer(n_terms))
        check(ccall((:bb_logsigma_rb, LIB), Cint, (Ptr{Cvoid}, Ref{bb_logsigma_rb_opts}, Ref{bb_logsigma_rb_out}), h, o, out))
    end
    return (n_terms=n_terms, q_mean=q_mean, q_sd=q_sd, rb_mean=rb_mean, rb_sd=rb_sd, sigma_mean=sigma_mean, mode_mean=mode_mean,
            quantiles=quantiles)
end

# Rao-Blackwellised marginals of logtau, the deviation scale of the hierarchical models (bb_logtau_rb, include/barbay_hip.h): the
# one-dimensional conditional of logtau -- not log-concave, up to two modes -- integrated numerically per draw on one grid over all
# kept modes and averaged over the draws of `fitness_rb`.  Field for field the Python binding's `bb_logtau_rb_opts` /
# `bb_logtau_rb_out` (barbay.jl_amd/_capi.py).  Like the rest of this file it remains unexecuted.
const BB_LOGTAU_FULL = Int32(0)
const BB_LOGTAU_COLLAPSED = Int32(1)
const BB_LOGTAU_RB_MAX_SAMPLES = 5781
struct bb_logtau_rb_opts
    mode::Int32
    n_samples::Int32
    n_quantiles::Int32
    reserved0::Int32
    probs::Ptr{Float64}
    seed::UInt64
    draws::Ptr{Float64}
end
struct bb_logtau_rb_out
    q_mean::Ptr{Float64}
    q_sd::Ptr{Float64}
    rb_mean::Ptr{Float64}
    rb_sd::Ptr{Float64}
    tau_mean::Ptr{Float64}
    pool_mean::Ptr{Float64}
    mode_mean::Ptr{Float64}
    quantiles::Ptr{Float64}
    n_terms::Ptr{Int32}
    n_two_modes::Ptr{Int32}
end

logtau_mode(mode::Symbol) = mode === :full ? BB_LOGTAU_FULL : mode === :collapsed ? BB_LOGTAU_COLLAPSED : error("logtau_rb: mode must be :full or :collapsed")

"""
    logtau_rb_shape(h) -> Int

Entries of `logtau_rb`: the length of the logtau block (0 for the models that have none).
"""
function logtau_rb_shape(h::Ptr{Cvoid})
    n = Ref{Int64}(0)
    check(ccall((:bb_logtau_rb_shape, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}), h, n))
    return Int(n[])
end

"""
    logtau_rb(h; mode=:collapsed, n_samples=1000, probs=[0.025, 0.5, 0.975], seed=0, draws=nothing) -> NamedTuple

`h` a live `bb_handle` of a hierarchical model.  `mode=:full`: the full conditional given everything else; `:collapsed`: with
theta_tilde integrated out against its prior.  Returns `n_terms, n_two_modes, q_mean, q_sd, rb_mean, rb_sd, tau_mean, pool_mean,
mode_mean` (n_entries each) and `quantiles` (length(probs) x n_entries; of logtau, their `exp` are tau's).  Arguments as for
`fitness_rb`, without a threshold.
"""
function logtau_rb(h::Ptr{Cvoid}; mode::Symbol=:collapsed, n_samples::Int=1000, probs::Vector{Float64}=[0.025, 0.5, 0.975],
                   seed::Integer=0, draws::Union{Nothing,Matrix{Float64}}=nothing)
    ne, nq = logtau_rb_shape(h), length(probs)
    if draws !== nothing
        D = ccall((:bb_num_latents, LIB), Int64, (Ptr{Cvoid},), h)
        size(draws, 1) == D || error("logtau_rb: draws must have $D rows")
        n_samples = size(draws, 2)
    end
    q_mean, q_sd, rb_mean, rb_sd, tau_mean, pool_mean, mode_mean = (Vector{Float64}(undef, ne) for _ in 1:7)
    quantiles = Matrix{Float64}(undef, nq, ne)
    n_terms = Vector{Int32}(undef, ne)
    n_two_modes = Vector{Int32}(undef, ne)
    GC.@preserve probs draws q_mean q_sd rb_mean rb_sd tau_mean pool_mean mode_mean quantiles n_terms n_two_modes begin
        o = bb_logtau_rb_opts(logtau_mode(mode), Int32(n_samples), Int32(nq), Int32(0), nq > 0 ? pointer(probs) : Ptr{Float64}(C_NULL),
                              UInt64(seed), draws === nothing ? Ptr{Float64}(C_NULL) : pointer(draws))
        out = bb_logtau_rb_out(pointer(q_mean), pointer(q_sd), pointer(rb_mean), pointer(rb_sd), pointer(tau_mean), pointer(pool_mean),
                               pointer(mode_mean), nq > 0 ? pointer(quantiles) : Ptr{Float64}(C_NULL), pointer(n_terms), pointer(n_two_modes))
        check(ccall((:bb_logtau_rb, LIB), Cint, (Ptr{Cvoid}, Ref{bb_logtau_rb_opts}, Ref{bb_logtau_rb_out}), h, o, out))
    end
    return (n_terms=n_terms, n_two_modes=n_two_modes, q_mean=q_mean, q_sd=q_sd, rb_mean=rb_mean, rb_sd=rb_sd, tau_mean=tau_mean,
            pool_mean=pool_mean, mode_mean=mode_mean, quantiles=quantiles)
end

# Log-joint and gradient at several points in one call (bb_logdensity_grad_batch, include/barbay_hip.h): what a sampler that
# steps an ensemble of walkers in lock-step asks of the model (`LogDensityProblems.logdensity_and_gradient`, W points at once).
const BB_LOGP_MAX_BATCH = 64
"""
    logdensity_grad_batch(h, Z) -> (logp, grad)

`Z` is D x W (one point per COLUMN: Julia's column-major D x W is the ABI's [W][D]), W <= BB_LOGP_MAX_BATCH, or a vector (W = 1).
Returns `logp` (W) and `grad` (D x W).  Column w's result is a function of `Z[:, w]` alone; the handle's variational state is untouched.
"""
function logdensity_grad_batch(h::Ptr{Cvoid}, Z::AbstractVecOrMat{Float64})
    Zc = Z isa AbstractVector ? reshape(collect(Z), :, 1) : Matrix{Float64}(Z)
    D = ccall((:bb_num_latents, LIB), Int64, (Ptr{Cvoid},), h)
    size(Zc, 1) == D || error("logdensity_grad_batch: Z must have $D rows")
    W = size(Zc, 2)
    logp, grad = Vector{Float64}(undef, W), Matrix{Float64}(undef, D, W)
    check(ccall((:bb_logdensity_grad_batch, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                h, W, Zc, logp, grad))
    return logp, grad
end

# Device-resident HMC trajectories (bb_hmc_begin / bb_hmc_step / bb_hmc_get / bb_hmc_end, include/barbay_hip.h): position, momentum and
# gradient of up to BB_HMC_MAX_WALKERS walkers stay on the device between the calls.  Field for field the Python binding's `bb_hmc_opts`,
# `bb_hmc_step_opts`, `bb_hmc_step_out` (barbay.jl_amd/_capi.py).  Like the rest of this file it has not been executed: no Julia here.
const BB_HMC_MAX_WALKERS = BB_LOGP_MAX_BATCH
const BB_HMC_MAX_LEAPFROG = 1024
const BB_HMC_STREAM0 = 0xFFFFFF00
struct bb_hmc_opts
    n_walkers::Int32
    reserved0::Int32
    seed::UInt64
    inv_mass::Ptr{Float64}
end
struct bb_hmc_step_opts
    transition::UInt32
    reserved0::Int32
    eps::Ptr{Float64}
    n_leapfrog::Ptr{Int32}
    log_u::Ptr{Float64}
end
struct bb_hmc_step_out
    h0::Ptr{Float64}
    h1::Ptr{Float64}
    kinetic0::Ptr{Float64}
    kinetic1::Ptr{Float64}
    logp_prop::Ptr{Float64}
    logp::Ptr{Float64}
    accepted::Ptr{Int32}
    divergent::Ptr{Int32}
end
"""
    hmc_begin(h, Z0; seed=0, inv_mass=nothing) -> logp

Opens the session at the columns of `Z0` (D x W, W <= BB_HMC_MAX_WALKERS, or a vector); `inv_mass` (D) is the diagonal metric (`nothing`:
ones).  Returns log p at the start points (a non-finite value is reported, not an error).  A second `hmc_begin` replaces the session.
"""
function hmc_begin(h::Ptr{Cvoid}, Z0::AbstractVecOrMat{Float64}; seed::Integer=0, inv_mass::Union{Nothing,AbstractVector{Float64}}=nothing)
    Zc = Z0 isa AbstractVector ? reshape(collect(Z0), :, 1) : Matrix{Float64}(Z0)
    D = ccall((:bb_num_latents, LIB), Int64, (Ptr{Cvoid},), h)
    size(Zc, 1) == D || error("hmc_begin: Z0 must have $D rows")
    im = inv_mass === nothing ? Float64[] : Vector{Float64}(inv_mass)
    inv_mass === nothing || length(im) == D || error("hmc_begin: inv_mass must have $D entries")
    W = size(Zc, 2)
    logp = Vector{Float64}(undef, W)
    GC.@preserve im begin
        o = bb_hmc_opts(Int32(W), Int32(0), UInt64(seed), inv_mass === nothing ? Ptr{Float64}(C_NULL) : pointer(im))
        check(ccall((:bb_hmc_begin, LIB), Cint, (Ptr{Cvoid}, Ref{bb_hmc_opts}, Ptr{Float64}, Ptr{Float64}), h, o, Zc, logp))
    end
    return logp
end
"""
    hmc_step(h, transition, eps, n_leapfrog, log_u) -> NamedTuple

One transition of every walker of the session; `eps`, `n_leapfrog`, `log_u` have one entry per walker.  Returns `h0, h1, kinetic0, kinetic1,
logp_prop, logp` (of the state held after the call), `accepted, divergent`.
"""
function hmc_step(h::Ptr{Cvoid}, transition::Integer, eps::AbstractVector{Float64}, n_leapfrog::AbstractVector{<:Integer}, log_u::AbstractVector{Float64})
    W = length(eps)
    length(n_leapfrog) == W && length(log_u) == W || error("hmc_step: eps, n_leapfrog and log_u need one entry per walker")
    e, nl, lu = Vector{Float64}(eps), Vector{Int32}(n_leapfrog), Vector{Float64}(log_u)
    h0, h1, k0, k1, lpp, lp = (Vector{Float64}(undef, W) for _ in 1:6)
    acc, dvg = Vector{Int32}(undef, W), Vector{Int32}(undef, W)
    GC.@preserve e nl lu h0 h1 k0 k1 lpp lp acc dvg begin
        o = bb_hmc_step_opts(UInt32(transition), Int32(0), pointer(e), pointer(nl), pointer(lu))
        out = bb_hmc_step_out(pointer(h0), pointer(h1), pointer(k0), pointer(k1), pointer(lpp), pointer(lp), pointer(acc), pointer(dvg))
        check(ccall((:bb_hmc_step, LIB), Cint, (Ptr{Cvoid}, Ref{bb_hmc_step_opts}, Ref{bb_hmc_step_out}), h, o, out))
    end
    return (h0=h0, h1=h1, kinetic0=k0, kinetic1=k1, logp_prop=lpp, logp=lp, accepted=acc, divergent=dvg)
end
"""
    hmc_get(h, W; grad=false) -> (Z, logp[, G])

The `W` walkers' current positions (D x W), log-densities and, with `grad`, gradients (D x W).
"""
function hmc_get(h::Ptr{Cvoid}, W::Integer; grad::Bool=false)
    D = ccall((:bb_num_latents, LIB), Int64, (Ptr{Cvoid},), h)
    Z, logp = Matrix{Float64}(undef, D, W), Vector{Float64}(undef, W)
    G = grad ? Matrix{Float64}(undef, D, W) : Matrix{Float64}(undef, 0, 0)
    check(ccall((:bb_hmc_get, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                h, Z, logp, grad ? pointer(G) : Ptr{Float64}(C_NULL)))
    return grad ? (Z, logp, G) : (Z, logp)
end
hmc_end(h::Ptr{Cvoid}) = check(ccall((:bb_hmc_end, LIB), Cint, (Ptr{Cvoid},), h))

# Streaming moments of the session's state and its metric (bb_hmc_accum_* / bb_hmc_set_metric / bb_hmc_get_metric, include/barbay_hip.h):
# per walker and segment a running mean and m2 on the device, pooled on request.  Field for field the Python binding's `bb_hmc_accum_opts`,
# `bb_hmc_accum_out` (barbay.jl_amd/_capi.py).  Like the rest of this file it has not been executed: no Julia here.
const BB_HMC_MAX_SEGMENTS = 8
struct bb_hmc_accum_opts
    n_segments::Int32
    reserved0::Int32
end
struct bb_hmc_accum_out
    mean::Ptr{Float64}
    sd::Ptr{Float64}
    mcse::Ptr{Float64}
    ess::Ptr{Float64}
    rhat::Ptr{Float64}
    within::Ptr{Float64}
    between::Ptr{Float64}
    n_total::Ptr{Int64}
end
"""
    hmc_accum_begin(h; n_segments=1)

Allocates and zeroes the running moments of the open session, `n_segments` <= BB_HMC_MAX_SEGMENTS per walker.  `hmc_begin` and `hmc_end`
drop them.
"""
hmc_accum_begin(h::Ptr{Cvoid}; n_segments::Integer=1) =
    check(ccall((:bb_hmc_accum_begin, LIB), Cint, (Ptr{Cvoid}, Ref{bb_hmc_accum_opts}), h, bb_hmc_accum_opts(Int32(n_segments), Int32(0))))
"""
    hmc_accum_add(h, segment)

One Welford step of every walker's current state into `segment[w]` (0-based as in the C ABI; -1: the walker is not added).
"""
hmc_accum_add(h::Ptr{Cvoid}, segment::AbstractVector{<:Integer}) =
    check(ccall((:bb_hmc_accum_add, LIB), Cint, (Ptr{Cvoid}, Ptr{Int32}), h, Vector{Int32}(segment)))
hmc_accum_reset(h::Ptr{Cvoid}) = check(ccall((:bb_hmc_accum_reset, LIB), Cint, (Ptr{Cvoid},), h))
"""
    hmc_accum_get(h, walker, segment) -> (mean, m2, n)

The rows of one (walker, segment), both 0-based, in the caller's order, and the number of states added to it.
"""
function hmc_accum_get(h::Ptr{Cvoid}, walker::Integer, segment::Integer)
    D = ccall((:bb_num_latents, LIB), Int64, (Ptr{Cvoid},), h)
    mean, m2, n = Vector{Float64}(undef, D), Vector{Float64}(undef, D), Ref{Int64}(0)
    check(ccall((:bb_hmc_accum_get, LIB), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ref{Int64}), h, walker, segment, mean, m2, n))
    return mean, m2, n[]
end
"""
    hmc_accum_stats(h) -> NamedTuple

Pooled `mean, sd, mcse, ess, rhat, within, between` (D each) and `n_total` of everything added.  `ess` is a batch-means estimate over the
live (walker, segment) chains, not Geyer's: its own relative error is about sqrt(2 / (C - 1)) for C chains (include/barbay_hip.h).
"""
function hmc_accum_stats(h::Ptr{Cvoid})
    D = ccall((:bb_num_latents, LIB), Int64, (Ptr{Cvoid},), h)
    mean, sd, mcse, ess, rhat, within, between = (Vector{Float64}(undef, D) for _ in 1:7)
    n = Ref{Int64}(0)
    GC.@preserve mean sd mcse ess rhat within between n begin
        out = bb_hmc_accum_out(pointer(mean), pointer(sd), pointer(mcse), pointer(ess), pointer(rhat), pointer(within), pointer(between),
                               Base.unsafe_convert(Ptr{Int64}, n))
        check(ccall((:bb_hmc_accum_stats, LIB), Cint, (Ptr{Cvoid}, Ref{bb_hmc_accum_out}), h, out))
    end
    return (mean=mean, sd=sd, mcse=mcse, ess=ess, rhat=rhat, within=within, between=between, n_total=n[])
end
"""
    hmc_set_metric(h, inv_mass=nothing)

Replaces the open session's diagonal metric (`nothing`: ones); positions, gradients and accumulators stay.
"""
function hmc_set_metric(h::Ptr{Cvoid}, inv_mass::Union{Nothing,AbstractVector{Float64}}=nothing)
    D = ccall((:bb_num_latents, LIB), Int64, (Ptr{Cvoid},), h)
    im = inv_mass === nothing ? Float64[] : Vector{Float64}(inv_mass)
    inv_mass === nothing || length(im) == D || error("hmc_set_metric: inv_mass must have $D entries")
    GC.@preserve im check(ccall((:bb_hmc_set_metric, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}), h, inv_mass === nothing ? Ptr{Float64}(C_NULL) : pointer(im)))
end
function hmc_get_metric(h::Ptr{Cvoid})
    D = ccall((:bb_num_latents, LIB), Int64, (Ptr{Cvoid},), h)
    im = Vector{Float64}(undef, D)
    check(ccall((:bb_hmc_get_metric, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}), h, im))
    return im
end

# The No-U-Turn tree of the open session on the device (bb_nuts_begin / bb_nuts_start / bb_nuts_leaf / bb_nuts_take, include/barbay_hip.h):
# both ends of the trajectory, the U-turn checkpoints and the candidates stay on the device; the caller decides on the scalars a leaf
# brings back.  Field for field the Python binding's `bb_nuts_opts`, `bb_nuts_leaf_opts`, `bb_nuts_leaf_out` (barbay.jl_amd/_capi.py).
# Like the rest of this file it has not been executed: no Julia here.
const BB_NUTS_MAX_DEPTH = 10
const BB_NUTS_EDGE_OPP = Int32(-2)
const BB_NUTS_TAKE_LEAF = Int32(1)
const BB_NUTS_TAKE_SUB = Int32(2)
const BB_NUTS_TAKE_STATE = Int32(4)
struct bb_nuts_opts
    max_depth::Int32
    reserved0::Int32
end
struct bb_nuts_leaf_opts
    dir::Ptr{Int32}
    first::Ptr{Int32}
    last::Ptr{Int32}
    store::Ptr{Int32}
    n_check::Ptr{Int32}
    check::Ptr{Int32}
    reserved0::Int32
end
struct bb_nuts_leaf_out
    logp_leaf::Ptr{Float64}
    kinetic::Ptr{Float64}
    a::Ptr{Float64}
    b::Ptr{Float64}
end

"""
    nuts_begin(h; max_depth=BB_NUTS_MAX_DEPTH)

Allocates and zeroes the tree's rows beside the open session: per walker 10 + 2 `max_depth` rows.  `hmc_begin` and `hmc_end` drop them.
"""
nuts_begin(h::Ptr{Cvoid}; max_depth::Integer=BB_NUTS_MAX_DEPTH) =
    check(ccall((:bb_nuts_begin, LIB), Cint, (Ptr{Cvoid}, Ref{bb_nuts_opts}), h, bb_nuts_opts(Int32(max_depth), Int32(0))))

"""
    nuts_start(h, transition, eps, live) -> kinetic0

A transition begins for the walkers with `live[w] != 0`: `hmc_step`'s momenta of `transition`, the state to both edges.
"""
function nuts_start(h::Ptr{Cvoid}, transition::Integer, eps::AbstractVector{Float64}, live::AbstractVector{<:Integer})
    W = length(eps)
    length(live) == W || error("nuts_start: eps and live need one entry per walker")
    e, lv, k0 = Vector{Float64}(eps), Vector{Int32}(live), Vector{Float64}(undef, W)
    check(ccall((:bb_nuts_start, LIB), Cint, (Ptr{Cvoid}, UInt32, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}), h, UInt32(transition), e, lv, k0))
    return k0
end

"""
    nuts_leaf(h, max_depth, dir, first, last, store, checks) -> NamedTuple

One leaf of every walker with `dir[w] != 0`; `checks[w]` lists the stored points the leaf is tested against (0-based checkpoint slots, or
BB_NUTS_EDGE_OPP).  Returns logp_leaf, kinetic (W) and a, b ((max_depth + 1) x W, column w the walker's).
"""
function nuts_leaf(h::Ptr{Cvoid}, max_depth::Integer, dir::AbstractVector{<:Integer}, first::AbstractVector{<:Integer},
                   last::AbstractVector{<:Integer}, store::AbstractVector{<:Integer}, checks::AbstractVector)
    W = length(dir)
    length(first) == W && length(last) == W && length(store) == W && length(checks) == W || error("nuts_leaf: one entry per walker")
    d, f, l, st = Vector{Int32}(dir), Vector{Int32}(first), Vector{Int32}(last), Vector{Int32}(store)
    nc = Int32[length(c) for c in checks]
    ck = zeros(Int32, BB_NUTS_MAX_DEPTH + 1, W)
    for w in 1:W, (j, c) in enumerate(checks[w])
        j <= BB_NUTS_MAX_DEPTH + 1 && (ck[j, w] = c)
    end
    lp, kin = Vector{Float64}(undef, W), Vector{Float64}(undef, W)
    a, b = Matrix{Float64}(undef, max_depth + 1, W), Matrix{Float64}(undef, max_depth + 1, W)
    GC.@preserve d f l st nc ck lp kin a b begin
        o = bb_nuts_leaf_opts(pointer(d), pointer(f), pointer(l), pointer(st), pointer(nc), pointer(ck), Int32(0))
        out = bb_nuts_leaf_out(pointer(lp), pointer(kin), pointer(a), pointer(b))
        check(ccall((:bb_nuts_leaf, LIB), Cint, (Ptr{Cvoid}, Ref{bb_nuts_leaf_opts}, Ref{bb_nuts_leaf_out}), h, o, out))
    end
    return (logp_leaf=lp, kinetic=kin, a=a, b=b)
end

"""
    nuts_take(h, flags)

Per walker the copies its flags ask for, in this order: BB_NUTS_TAKE_LEAF (leaf -> subtree candidate), BB_NUTS_TAKE_SUB (subtree candidate
-> transition candidate), BB_NUTS_TAKE_STATE (transition candidate -> the session's state).
"""
nuts_take(h::Ptr{Cvoid}, flags::AbstractVector{<:Integer}) =
    check(ccall((:bb_nuts_take, LIB), Cint, (Ptr{Cvoid}, Ptr{Int32}), h, Vector{Int32}(flags)))

# Chain diagnostics (bb_chain_summary, include/barbay_hip.h): MCMCChains' summarystats + quantile of a host chain, on the device.
# Field for field the Python binding's `bb_chain_opts` / `bb_chain_out` (barbay.jl_amd/_capi.py).
const BB_CHAIN_MAX_K = 16384
const BB_CHAIN_MAX_Q = 8
struct bb_chain_opts
    n_chains::Int32
    n_draws::Int32
    n_quantiles::Int32
    max_lag::Int32
    probs::Ptr{Float64}
    slab_cols::Int64
end
struct bb_chain_out
    mean::Ptr{Float64}
    sd::Ptr{Float64}
    mcse::Ptr{Float64}
    ess::Ptr{Float64}
    rhat::Ptr{Float64}
    quantiles::Ptr{Float64}
    n_lags::Ptr{Int32}
end

"""
    chain_summary(h, chain; probs=[0.025, 0.25, 0.5, 0.75, 0.975], max_lag=0, slab_cols=0) -> NamedTuple

`h` a live `bb_handle` (it lends its device; nothing of its model is read).  `chain` is D x N x W (Julia order of the C array
[n_chains][n_draws][n_cols]), or D x N for one chain; W N <= BB_CHAIN_MAX_K.  Returns `mean, sd, mcse, ess, rhat` (D each),
`quantiles` (length(probs) x D) and `n_lags` (D): pooled mean and std, MCSE, ESS by Geyer's initial monotone sequence, split-R-hat
and StatsBase type-7 quantiles of every column.
"""
function chain_summary(h::Ptr{Cvoid}, chain::AbstractArray{Float64}; probs::Vector{Float64}=[0.025, 0.25, 0.5, 0.75, 0.975],
                       max_lag::Integer=0, slab_cols::Integer=0)
    x = Array{Float64}(ndims(chain) == 2 ? reshape(chain, size(chain, 1), size(chain, 2), 1) : chain)
    D, N, W = size(x)
    nq = length(probs)
    mean, sd, mcse, ess, rhat = (Vector{Float64}(undef, D) for _ in 1:5)
    q = Matrix{Float64}(undef, nq, D)
    nl = Vector{Int32}(undef, D)
    GC.@preserve probs mean sd mcse ess rhat q nl begin
        o = bb_chain_opts(Int32(W), Int32(N), Int32(nq), Int32(max_lag), nq > 0 ? pointer(probs) : Ptr{Float64}(C_NULL), Int64(slab_cols))
        out = bb_chain_out(pointer(mean), pointer(sd), pointer(mcse), pointer(ess), pointer(rhat),
                           nq > 0 ? pointer(q) : Ptr{Float64}(C_NULL), pointer(nl))
        check(ccall((:bb_chain_summary, LIB), Cint, (Ptr{Cvoid}, Ref{bb_chain_opts}, Int64, Ptr{Float64}, Ref{bb_chain_out}),
                    h, o, D, x, out))
    end
    return (mean=mean, sd=sd, mcse=mcse, ess=ess, rhat=rhat, quantiles=q, n_lags=nl)
end

# The iterate trace (bb_trace_*, include/barbay_hip.h): (mu, omega) kept after every `every` steps of bb_run in a device ring, and
# split-R-hat / ESS / MCSE of a window of it computed where it lies, with a verdict per layout block.
# Field for field the Python binding's `bb_trace_opts` / `bb_trace_sum_opts` / `bb_trace_block` / `bb_trace_sum_out`.
const BB_TRACE_MAX_SNAPSHOTS = 16384
struct bb_trace_opts
    every::Int32
    capacity::Int32
end
struct bb_trace_sum_opts
    first::Int64
    n_chains::Int32
    n_draws::Int32
    max_lag::Int32
    reserved0::Int32
    slab_cols::Int64
    rhat_max::Float64
end
struct bb_trace_block
    name::NTuple{24,UInt8}
    part::Int32
    reserved0::Int32
    n_cols::Int64
    n_nonfinite::Int64
    n_const::Int64
    n_above::Int64
    max_rhat::Float64
    min_ess::Float64
    max_mcse_rel::Float64
end
struct bb_trace_sum_out
    mean::Ptr{Float64}
    sd::Ptr{Float64}
    mcse::Ptr{Float64}
    ess::Ptr{Float64}
    rhat::Ptr{Float64}
    n_lags::Ptr{Int32}
    blocks::Ptr{bb_trace_block}
end

trace_begin(h::Ptr{Cvoid}, every::Integer, capacity::Integer) =
    check(ccall((:bb_trace_begin, LIB), Cint, (Ptr{Cvoid}, Ref{bb_trace_opts}), h, bb_trace_opts(Int32(every), Int32(capacity))))
trace_end(h::Ptr{Cvoid}) = check(ccall((:bb_trace_end, LIB), Cint, (Ptr{Cvoid},), h))

"`(taken, first_live)`: snapshots recorded since `trace_begin` or the last reset, and the oldest one the ring still holds (0-based)."
function trace_count(h::Ptr{Cvoid})
    taken, live = Ref{Int64}(0), Ref{Int64}(0)
    check(ccall((:bb_trace_count, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}), h, taken, live))
    return (Int(taken[]), Int(live[]))
end

"Snapshots `first .. first + n - 1` (0-based) as `(mu, omega)`, each D x n, in the caller's latent order."
function trace_get(h::Ptr{Cvoid}, first::Integer, n::Integer)
    D = Int(ccall((:bb_num_latents, LIB), Int64, (Ptr{Cvoid},), h))
    mu, om = Matrix{Float64}(undef, D, n), Matrix{Float64}(undef, D, n)
    check(ccall((:bb_trace_get, LIB), Cint, (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Ptr{Float64}), h, first, n, mu, om))
    return (mu, om)
end

"""
    trace_summary(h, first, n_chains, n_draws; max_lag=0, slab_cols=0, rhat_max=1.1, columns=false) -> NamedTuple

The window of `n_chains * n_draws` snapshots from `first` (0-based), cut into `n_chains` consecutive segments.  Returns `blocks`, a
vector of `(name, part, n_cols, n_nonfinite, n_const, n_above, max_rhat, min_ess, max_mcse_rel)` -- the mu part of every layout
block, then the omega parts -- and, with `columns`, `mean, sd, mcse, ess, rhat, n_lags` (2 D each: mu of latent i at i, its omega at
D + i).
"""
function trace_summary(h::Ptr{Cvoid}, first::Integer, n_chains::Integer, n_draws::Integer; max_lag::Integer=0, slab_cols::Integer=0,
                       rhat_max::Real=1.1, columns::Bool=false)
    D = Int(ccall((:bb_num_latents, LIB), Int64, (Ptr{Cvoid},), h))
    lay = Vector{bb_block_range}(undef, 8)
    nb = Ref{Int32}(0)
    check(ccall((:bb_get_layout, LIB), Cint, (Ptr{Cvoid}, Ptr{bb_block_range}, Ref{Int32}), h, lay, nb))
    n = columns ? 2D : 0
    mean, sd, mcse, ess, rhat = (Vector{Float64}(undef, n) for _ in 1:5)
    nl = Vector{Int32}(undef, n)
    vb = Vector{bb_trace_block}(undef, 2 * nb[])
    p(v) = columns ? pointer(v) : Ptr{eltype(v)}(C_NULL)
    GC.@preserve mean sd mcse ess rhat nl vb begin
        o = bb_trace_sum_opts(Int64(first), Int32(n_chains), Int32(n_draws), Int32(max_lag), Int32(0), Int64(slab_cols), Float64(rhat_max))
        out = bb_trace_sum_out(p(mean), p(sd), p(mcse), p(ess), p(rhat), p(nl), pointer(vb))
        check(ccall((:bb_trace_summary, LIB), Cint, (Ptr{Cvoid}, Ref{bb_trace_sum_opts}, Ref{bb_trace_sum_out}), h, o, out))
    end
    name(b) = String(UInt8[c for c in b.name if c != 0x00])
    blocks = [(name=name(b), part=b.part == 0 ? :mu : :omega, n_cols=b.n_cols, n_nonfinite=b.n_nonfinite, n_const=b.n_const,
               n_above=b.n_above, max_rhat=b.max_rhat, min_ess=b.min_ess, max_mcse_rel=b.max_mcse_rel) for b in vb]
    return columns ? (blocks=blocks, mean=mean, sd=sd, mcse=mcse, ess=ess, rhat=rhat, n_lags=nl) : (blocks=blocks,)
end

end # module
