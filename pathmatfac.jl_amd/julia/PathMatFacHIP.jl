# PathMatFacHIP.jl -- Julia host shim: re-points PathMatFac's `mf_fit!` (src/fit.jl:9-38), the only caller of the
# un-vendored MatFac.fit! inner loop, at libpmf_hip.so (include/pmf_hip.h) through `ccall`.
#
# Everything above `mf_fit!` in src/fit.jl (mf_fit_adapt_lr!, init_theta!, init_factors!, fit_ard!,
# fit_feature_set_ard!, fit!, transform) runs unchanged: it only sees the history Dict this function returns
# ("term_code", "epochs", src/fit.jl:63,69) and the mutated model parameters.
# The closed-form stages between the gradient-descent stages (init_mu!, init_logsigma!, reweight_col_losses!,
# construct_minimal_regularizer, theta_delta_em, update_A!) are re-pointed too: each marshals the model, makes ONE library
# call (pmf_stage_* / pmf_fsard_update_A, or pmf_fsard_update_A_csr on the sparse S where L * K exceeds the dense entry's
# capacity; init_mu! goes through this file's mf_fit!) and copies back what changed.  The
# moments block inside init_batch_effects! (src/fit.jl:444-462) keeps MatFac's CPU helpers.
# So is the factor post-processing (whiten!, rotate_by_svd!, reorder_by_importance!, reweight_eb! of the L2 / Group terms):
# one pmf_stage_whiten / _rotate_by_svd / _reorder_by_importance / _lambda_max call each.
#
# Usage:   using PathMatFac; include("PathMatFacHIP.jl"); PathMatFacHIP.install!("/path/to/libpmf_hip.so")
#          model = PathMatFacModel(D; ...);  fit!(model; ...)         # no gpu(model): the library owns the device copy
#
# NOTE: Julia is not installed in the build container, so this file has not been executed there; it is the
# maintainer-side binding that INTEGRATION.md documents.  The Python ctypes binding (_lib.py) is its tested twin, and
# tests/test_julia_shim_static.py checks every `ccall` here (name, return type, argument count and types) and every struct
# against include/pmf_hip.h without running Julia.
module PathMatFacHIP

import PathMatFac
import SparseArrays
const PM = PathMatFac

const LIB = Ref{String}("libpmf_hip.so")
const CTX = IdDict{Any,Ptr{Cvoid}}()          # model => pmf_ctx*
const DATA_KEY = IdDict{Any,UInt}()           # model => objectid(model.data) last uploaded
const OPT_KEY = IdDict{Any,UInt}()            # model => objectid(opt) whose state lives on the device
const FSARD_DATA = IdDict{Any,Matrix{Float32}}()   # FeatureSetARDReg => the all-missing 1 x N matrix of its own context (update_A!)

const FSARD_DENSE_CAPACITY = 16384            # L * K that pmf_fsard_update_A accepts (A in one workgroup's LDS)

const TERM_CODES = ("max_epochs", "loss_increase", "abs_tol", "rel_tol", "nonfinite")
# bernoulli_sq_hinge and ordinal_sq_hinge3 are ONE kind of the library (PMF_NOISE_SQ_HINGE) with per-column thresholds
const NOISE_KIND = Dict("normal" => Cint(0), "bernoulli" => Cint(1), "poisson" => Cint(2),
                        "bernoulli_sq_hinge" => Cint(3), "ordinal_sq_hinge3" => Cint(3))

struct FitOpts            # pmf_fit_opts
    update_X::Cint; update_Y::Cint; update_col_layers::Cint; frozen_layers::Cint; frozen_regs::Cint
    max_epochs::Cint; epoch::Cint; tol_max_iters::Cint; keep_trace::Cint; verbosity::Cint; print_iter::Cint
    reserved::Cint; abs_tol::Cdouble; rel_tol::Cdouble; capacity::Int64
end

mutable struct FitResult  # pmf_fit_result
    term_code::Cint; epochs::Cint; n_trace::Cint; trace_cap::Cint
    final_loss::Cdouble; loss_trace::Ptr{Cdouble}; seconds::Cdouble
end

struct LbfgsOpts          # pmf_lbfgs_opts
    m::Cint; max_iter::Cint; backtrack_max_iter::Cint; keep_trace::Cint; verbosity::Cint; print_iter::Cint
    rel_tol::Cdouble; abs_tol::Cdouble; backtrack_shrinkage::Cdouble; c1::Cdouble; sy_min::Cdouble
end

mutable struct LbfgsResult  # pmf_lbfgs_result
    term_code::Cint; iters::Cint; loss_evals::Cint; grad_evals::Cint; resets::Cint; n_trace::Cint; trace_cap::Cint
    reserved::Cint; final_loss::Cdouble; seconds::Cdouble
    loss_trace::Ptr{Cdouble}; trial_trace::Ptr{Cint}; flag_trace::Ptr{Cint}
end

struct EmOpts             # pmf_em_opts
    update_priors::Cint; max_iter::Cint; verbosity::Cint; reserved::Cint; rtol::Cdouble
end

mutable struct EmResult   # pmf_em_result
    iters::Cint; n_diffs::Cint; diffs_cap::Cint; reserved::Cint; diffs::Ptr{Cdouble}; seconds::Cdouble
end

struct SimOpts            # pmf_sim_opts
    seed::UInt64; row_offset::Int64; noise::Cfloat; frac_missing::Cfloat
end

lasterr() = unsafe_string(ccall((:pmf_last_error, LIB[]), Cstring, ()))
chk(rc::Integer) = rc == 0 ? nothing : error("libpmf_hip: " * lasterr())
f32(a) = convert(Array{Float32}, a)
starts(rs) = Int64[r.start for r in rs]
stops(rs) = Int64[r.stop for r in rs]

# Arithmetic of the data pass's matrix products (include/pmf_hip.h): :f32 = exact f32 MFMA (default),
# :bf16x3 = split-bf16 products where a kernel variant exists (DESIGN.md 4.5).  No reference counterpart.
function set_precision!(model, mode::Symbol)
    code = mode == :f32 ? 0 : mode == :bf16x3 ? 1 : error("precision must be :f32 or :bf16x3")
    chk(ccall((:pmf_set_precision, LIB[]), Cint, (Ptr{Cvoid}, Cint), context!(model), code))
end
# (mode, fused launches that took the split-bf16 kernel so far)
function get_precision(model)
    mode = Ref{Cint}(0); n = Ref{Int64}(0)
    chk(ccall((:pmf_get_precision, LIB[]), Cint, (Ptr{Cvoid}, Ref{Cint}, Ref{Int64}), context!(model), mode, n))
    return (mode[] == 0 ? :f32 : :bf16x3), Int(n[])
end

# Storage type of the device copy of D (include/pmf_hip.h): :f32 (default) or :bf16 (BASELINE configs[4], "D stored
# bf16": rounded once at upload, everything else stays Float32).  Takes effect at the next upload of the data matrix.
const STORE = Ref{Cint}(0)
set_store!(mode::Symbol) = (STORE[] = mode == :f32 ? 0 : mode == :bf16 ? 1 : error("store must be :f32 or :bf16"); nothing)

# ---- multi-GPU: one Julia process per GPU (analyses/scripts/julia/script_util.jl:278-306), rows sharded ----------------
# Rank 0 creates the 128-byte RCCL id and hands it to the other ranks by any means (a file, MPI, Distributed.jl):
#     id = PathMatFacHIP.comm_unique_id()                       # rank 0
#     PathMatFacHIP.comm_init!(model, rank, nranks, id)         # every rank, before fit!
# From then on mf_fit! all-reduces grad(Y), the loss and the layer gradients inside pmf_fit (DESIGN.md 5); the
# statistics the host keeps between the GD stages go through comm_allreduce!.
# HIP devices visible to this process (pmf_device_count).  A launcher that pins one device per rank leaves ONE visible device,
# which is device 0 whatever the local rank: device_for_rank mirrors bench.py's map.
function device_count()
    n = Ref{Cint}(0)
    chk(ccall((:pmf_device_count, LIB[]), Cint, (Ref{Cint},), n))
    return Int(n[])
end
device_for_rank(local_rank::Integer) = (v = device_count(); v == 1 ? 0 : (local_rank < v ? Int(local_rank) :
    error("local rank $local_rank has no device: only $v visible")))
# kernel family of the last fused data pass (pmf_debug_last_kernel): 0 exact f32, 1 / 2 / 4 / 8 = split kernels sb / sb2 / sb4 / sb8
function last_kernel(model)
    k = Ref{Cint}(0)
    chk(ccall((:pmf_debug_last_kernel, LIB[]), Cint, (Ptr{Cvoid}, Ref{Cint}), context!(model), k))
    return Int(k[])
end

# bytes the data pass with these gradient flags addresses in each grow-only device buffer against the bytes allocated
# (pmf_debug_pass_extents): Dict(name => (need = ..., capacity = ...)); the pass is prepared, not launched
function pass_extents(model; update_X::Bool=false, update_Y::Bool=false)
    nmax = 16
    names = fill(Ptr{UInt8}(C_NULL), nmax); need = zeros(Int64, nmax); cap = zeros(Int64, nmax); n = Ref{Cint}(0)
    chk(ccall((:pmf_debug_pass_extents, LIB[]), Cint,
              (Ptr{Cvoid}, Cint, Cint, Ptr{Int64}, Cint, Ptr{Ptr{UInt8}}, Ptr{Int64}, Ptr{Int64}, Ref{Cint}),
              context!(model), update_X, update_Y, C_NULL, nmax, names, need, cap, n))
    return Dict(unsafe_string(names[i]) => (need = need[i], capacity = cap[i]) for i in 1:Int(n[]))
end

function comm_unique_id()
    id = zeros(UInt8, 128)
    GC.@preserve id chk(ccall((:pmf_comm_get_unique_id, LIB[]), Cint, (Ptr{UInt8},), id))
    return id
end
function comm_init!(model, rank::Integer, nranks::Integer, id::Vector{UInt8}; device::Integer=rank)
    ctx = context!(model; device=device)
    GC.@preserve id chk(ccall((:pmf_comm_init, LIB[]), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{UInt8}), ctx, rank, nranks, id))
end
comm_destroy!(model) = chk(ccall((:pmf_comm_destroy, LIB[]), Cint, (Ptr{Cvoid},), context!(model)))
comm_set_chunks!(model, n::Integer) = chk(ccall((:pmf_comm_set_chunks, LIB[]), Cint, (Ptr{Cvoid}, Cint), context!(model), n))
# sum (op = 0) or maximum (op = 1) over the ranks of a host array, in place (Float32 or Float64)
function comm_allreduce!(model, a::Array{T}; op::Integer=0) where {T<:Union{Float32,Float64}}
    GC.@preserve a chk(ccall((:pmf_comm_allreduce, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Cint, Cint),
                             context!(model), a, length(a), T == Float64 ? 1 : 0, op))
    return a
end

# rank, size, transport (0 none, 1 RCCL, 2 host-staged), column chunks of the last fit, reserved CUs, collectives issued
function comm_info(model)
    r = Ref{Cint}(0); n = Ref{Cint}(0); t = Ref{Cint}(0); ch = Ref{Cint}(0); cu = Ref{Cint}(0); nc = Ref{Int64}(0)
    chk(ccall((:pmf_comm_info, LIB[]), Cint, (Ptr{Cvoid}, Ref{Cint}, Ref{Cint}, Ref{Cint}, Ref{Cint}, Ref{Cint}, Ref{Int64}),
              context!(model), r, n, t, ch, cu, nc))
    return (rank = Int(r[]), nranks = Int(n[]), transport = Int(t[]), n_chunks = Int(ch[]), reserved_cus = Int(cu[]),
            n_collectives = Int(nc[]))
end

# fresh optimizer state on the device (a new optimizer object does this by itself in mf_fit!)
reset_optimizer_state!(model) = chk(ccall((:pmf_reset_optimizer_state, LIB[]), Cint, (Ptr{Cvoid},), context!(model)))

# Adopt the host's HIP stream (AMDGPU.jl: AMDGPU.stream().stream); C_NULL = the library's own non-blocking stream.
set_stream!(model, stream::Ptr{Cvoid}) = chk(ccall((:pmf_set_stream, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), context!(model), stream))

# update_A! of one FeatureSetARDReg view on the device (src/featureset_ard.jl:214-294): S is the view's L x N_v feature-set
# matrix (dense, row-major for the library = the transpose of Julia's column-major N_v x L), A / ssq_grad are K x L here
# (factor index contiguous).  Returns (best_loss, epochs_run); beta[:, cr] is updated on the device and returned in beta.
function fsard_update_A!(model, cr::UnitRange, S_t::Matrix{Float32}, alpha::Vector{Float32}, lambda::Vector{Float32},
                         A_t::Matrix{Float32}, ssq_t::Matrix{Float32}, beta::Matrix{Float32};
                         alpha0::Float32, v0::Float32, lr::Float32, max_epochs::Integer=1000, term_iter::Integer=50,
                         atol::Float64=1e-5, ctx::Ptr{Cvoid}=context!(model))
    best = Ref{Cdouble}(0.0); ep = Ref{Cint}(0)
    L = size(S_t, 2)
    GC.@preserve S_t alpha lambda A_t ssq_t beta chk(ccall((:pmf_fsard_update_A, LIB[]), Cint,
        (Ptr{Cvoid}, Int64, Int64, Cint, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Cfloat, Cfloat, Cfloat, Ptr{Cfloat},
         Ptr{Cfloat}, Cint, Cint, Cdouble, Ref{Cdouble}, Ref{Cint}, Ptr{Cfloat}),
        ctx, cr.start, cr.stop, L, S_t, alpha, lambda, alpha0, v0, lr, ssq_t, A_t, max_epochs, term_iter, atol,
        best, ep, beta))
    return best[], Int(ep[])
end

# The same on a sparse S, without the L * K <= 16384 bound of the dense entry (pmf_fsard_update_A_csr): S_t is the view's
# N_v x L transpose as a SparseMatrixCSC, whose colptr / rowval, shifted to 0-based, are the CSR of the L x N_v matrix
# (row indices ascend within a column of a SparseMatrixCSC, as the library wants the columns of a row).
function fsard_update_A_csr!(model, cr::UnitRange, S_t, alpha::Vector{Float32}, lambda::Vector{Float32},
                             A_t::Matrix{Float32}, ssq_t::Matrix{Float32}, beta::Matrix{Float32};
                             alpha0::Float32, v0::Float32, lr::Float32, max_epochs::Integer=1000, term_iter::Integer=50,
                             atol::Float64=1e-5, ctx::Ptr{Cvoid}=context!(model))
    best = Ref{Cdouble}(0.0); ep = Ref{Cint}(0)
    L = size(S_t, 2)
    rowptr = Vector{Int64}(S_t.colptr .- 1)
    col = Vector{Int32}(S_t.rowval .- 1)
    val = Vector{Float32}(S_t.nzval)
    if isempty(col)                       # (a pointer the library may look at, never through)
        col = Int32[0]; val = Float32[0]
    end
    GC.@preserve rowptr col val alpha lambda A_t ssq_t beta chk(ccall((:pmf_fsard_update_A_csr, LIB[]), Cint,
        (Ptr{Cvoid}, Int64, Int64, Cint, Ptr{Int64}, Ptr{Int32}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Cfloat, Cfloat, Cfloat,
         Ptr{Cfloat}, Ptr{Cfloat}, Cint, Cint, Cdouble, Ref{Cdouble}, Ref{Cint}, Ptr{Cfloat}),
        ctx, cr.start, cr.stop, L, rowptr, col, val, alpha, lambda, alpha0, v0, lr, ssq_t, A_t, max_epochs, term_iter, atol,
        best, ep, beta))
    return best[], Int(ep[])
end

context!(model; device::Integer=0) = data_context!(model, model.data; device=device)

# The context of `owner` (a PathMatFacModel, or -- for the functions that get a bare MatFacModel and the data, as
# theta_delta_em does -- the data array itself), with `data` resident on the device.
function data_context!(owner, data; device::Integer=0)
    ctx = get!(CTX, owner) do
        p = Ref{Ptr{Cvoid}}(C_NULL)
        chk(ccall((:pmf_create, LIB[]), Cint, (Cint, Ref{Ptr{Cvoid}}), device, p))
        p[]
    end
    key = objectid(data)
    if get(DATA_KEY, owner, UInt(0)) != key            # gpu(model): upload the data matrix once
        D = f32(data)
        M, N = size(D)
        GC.@preserve D chk(ccall((:pmf_set_data, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cfloat}, Int64, Int64, Cint),
                                 ctx, D, M, N, STORE[]))
        DATA_KEY[owner] = key
    end
    return ctx
end

# MatFac noise structs -> the ABI's names: NormalNoise -> "normal", BernoulliNoise -> "bernoulli", PoissonNoise -> "poisson",
# SquaredHingeNoise -> "bernoulli_sq_hinge", OrdinalSqHingeNoise -> "ordinal_sq_hinge3" (simulate_params.jl:224-238).
# (MatFac.jl is un-vendored: the per-column weight field set by MF.set_weight! (src/fit.jl:157,180) is assumed to be
#  `weight`; adjust this one accessor if the struct names it differently.)
const NOISE_STRUCT_NAMES = Dict("squaredhinge" => "bernoulli_sq_hinge", "ordinalsqhinge" => "ordinal_sq_hinge3")
function noise_name(n)
    s = lowercase(replace(string(nameof(typeof(n))), "Noise" => ""))
    return get(NOISE_STRUCT_NAMES, s, s)
end
# (t0, t1, t2) of a squared-hinge range: SquaredHingeNoise has none of its own -> (0, Inf, Inf); OrdinalSqHingeNoise keeps
# ext_thresholds = [-Inf, t1, t2, Inf] (simulate_params.jl:230-238), whose interior is sent behind a -Inf
function hinge_thresholds(n)
    noise_name(n) == "ordinal_sq_hinge3" || return Float32[0, Inf, Inf]
    t = f32(collect(n.ext_thresholds[2:end-1]))
    length(t) == 2 || error("ordinal_sq_hinge3 takes three classes, got $(length(t) + 1)")
    return Float32[-Inf, t[1], t[2]]
end
noise_weights(nm) = vcat([collect(n.weight) for n in nm.noises]...)

unwrap(l) = isa(l, PM.FrozenLayer) ? l.layer : l
unwrapreg(r) = isa(r, PM.FrozenRegularizer) ? r.reg : r

# one-hot CSC row_batches matrix -> 0-based batch index of every row (src/util.jl:200-210, 588-593)
function batch_of_row(rb)
    M, nb = size(rb)
    out = fill(Int32(-1), M)
    for b in 1:nb, i in PM.get_col_idx(rb, b)
        out[i] = b - 1
    end
    return out
end

# (`ccall` needs its function name as a literal: one call per branch, never a computed symbol)
function add_reg!(ctx, which::Symbol, reg, p::Float32=1f0)
    if isa(reg, Function)                               # x -> 0
        return
    elseif isa(reg, PM.L2Regularizer)
        w = f32(reg.weights)
        if which == :X
            GC.@preserve w chk(ccall((:pmf_add_xreg_l2, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cfloat}, Cfloat), ctx, w, p))
        else
            GC.@preserve w chk(ccall((:pmf_add_yreg_l2, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cfloat}, Cfloat), ctx, w, p))
        end
    elseif isa(reg, PM.GroupRegularizer)
        s, e = starts(reg.group_idx), stops(reg.group_idx)
        w = f32(hcat(reg.group_weights...))             # K x n_groups column-major == n_groups x K with K contiguous
        if which == :X
            GC.@preserve s e w chk(ccall((:pmf_add_xreg_group, LIB[]), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Int64}, Ptr{Int64}, Ptr{Cfloat}, Cfloat), ctx, length(s), s, e, w, p))
        else
            GC.@preserve s e w chk(ccall((:pmf_add_yreg_group, LIB[]), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Int64}, Ptr{Int64}, Ptr{Cfloat}, Cfloat), ctx, length(s), s, e, w, p))
        end
    elseif isa(reg, PM.ARDRegularizer) && which == :Y
        s, e = starts(reg.col_ranges), stops(reg.col_ranges)
        a, b = f32(collect(reg.alpha)), f32(collect(reg.beta))
        GC.@preserve s e a b chk(ccall((:pmf_add_yreg_ard, LIB[]), Cint,
            (Ptr{Cvoid}, Cint, Ptr{Int64}, Ptr{Int64}, Ptr{Cfloat}, Ptr{Cfloat}, Cfloat), ctx, length(s), s, e, a, b, p))
    elseif isa(reg, PM.FeatureSetARDReg) && which == :Y
        a, b = f32(reg.alpha), f32(reg.beta)
        GC.@preserve a b chk(ccall((:pmf_add_yreg_fsard, LIB[]), Cint,
            (Ptr{Cvoid}, Ptr{Cfloat}, Ptr{Cfloat}, Cfloat), ctx, a, b, p))
    elseif isa(reg, PM.CompositeRegularizer)
        for (r, q) in zip(reg.regularizers, reg.mixture_p)
            add_reg!(ctx, which, r, p * Float32(q))
        end
    else
        error("PathMatFacHIP: regularizer $(typeof(reg)) is not supported by the HIP path (Network/L1/SelectiveL1 are out of scope)")
    end
end

# with_regs = false: parameters, batch views and noise model only, X_reg / Y_reg cleared -- what the statistics passes need
# (init_batch_effects! keeps an X_reg of the wrong shape attached while it regresses Y, src/fit.jl:397-428)
function marshal!(ctx, mf; with_regs::Bool=true)
    X, Y = f32(mf.X), f32(mf.Y)
    K = size(X, 1)
    GC.@preserve X Y chk(ccall((:pmf_set_factors, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cfloat}, Ptr{Cfloat}, Cint), ctx, X, Y, K))
    layers = map(unwrap, mf.col_transform.layers)
    N = size(Y, 2)
    ls = isa(layers[1], PM.ColScale) ? f32(layers[1].logsigma) : zeros(Float32, N)
    mu = isa(layers[3], PM.ColShift) ? f32(layers[3].mu) : zeros(Float32, N)
    GC.@preserve ls mu chk(ccall((:pmf_set_col_params, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cfloat}, Ptr{Cfloat}), ctx, ls, mu))
    ba = isa(layers[2], PM.BatchScale) ? layers[2].logdelta : (isa(layers[4], PM.BatchShift) ? layers[4].theta : nothing)
    nviews = ba === nothing ? 0 : length(ba.col_ranges)
    chk(ccall((:pmf_set_n_batch_views, LIB[]), Cint, (Ptr{Cvoid}, Cint), ctx, nviews))
    for v in 1:nviews
        cr = ba.col_ranges[v]
        bor = batch_of_row(ba.row_batches[v])
        ld = isa(layers[2], PM.BatchScale) ? f32(layers[2].logdelta.values[v]) : zeros(Float32, size(ba.values[v]))
        th = isa(layers[4], PM.BatchShift) ? f32(layers[4].theta.values[v]) : zeros(Float32, size(ba.values[v]))
        GC.@preserve bor ld th chk(ccall((:pmf_set_batch_view, LIB[]), Cint,
            (Ptr{Cvoid}, Cint, Int64, Int64, Cint, Ptr{Int32}, Ptr{Cfloat}, Ptr{Cfloat}),
            ctx, v - 1, cr.start, cr.stop, size(ld, 1), bor, ld, th))
    end
    nm = mf.noise_model
    s, e = starts(nm.col_ranges), stops(nm.col_ranges)
    kinds = Cint[NOISE_KIND[noise_name(n)] for n in nm.noises]
    w = f32(noise_weights(nm))
    GC.@preserve s e kinds w chk(ccall((:pmf_set_noise, LIB[]), Cint,
        (Ptr{Cvoid}, Cint, Ptr{Int64}, Ptr{Int64}, Ptr{Cint}, Ptr{Cfloat}), ctx, length(s), s, e, kinds, w))
    hinge = findall(==(NOISE_KIND["ordinal_sq_hinge3"]), kinds)
    if !isempty(hinge)
        hs, he = s[hinge], e[hinge]
        thr = vcat([hinge_thresholds(nm.noises[r]) for r in hinge]...)
        GC.@preserve hs he thr chk(ccall((:pmf_set_noise_thresholds, LIB[]), Cint,
            (Ptr{Cvoid}, Cint, Ptr{Int64}, Ptr{Int64}, Ptr{Cfloat}), ctx, length(hs), hs, he, thr))
    end
    chk(ccall((:pmf_clear_xreg, LIB[]), Cint, (Ptr{Cvoid},), ctx)); with_regs && add_reg!(ctx, :X, mf.X_reg)
    chk(ccall((:pmf_clear_yreg, LIB[]), Cint, (Ptr{Cvoid},), ctx)); with_regs && add_reg!(ctx, :Y, mf.Y_reg)
    marshal_layer_regs!(ctx, mf.col_transform_reg, nviews)
    return nviews
end

function marshal_layer_regs!(ctx, sr, nviews)
    nul = Ptr{Cfloat}(C_NULL)
    if !isa(sr, PM.SequenceReg)
        return chk(ccall((:pmf_set_layer_regs, LIB[]), Cint, (Ptr{Cvoid}, Cint, Ptr{Int64}, Ptr{Int64},
            Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}),
            ctx, 0, C_NULL, C_NULL, nul, nul, nul, nul, nul, nul, nul, nul))
    end
    regs = map(unwrapreg, sr.regs)
    s, e = Int64[], Int64[]
    wls = cls = wmu = cmu = wld = cld = wth = cth = Float32[]
    if isa(regs[1], PM.ColParamReg) && isa(regs[3], PM.ColParamReg)
        s, e = starts(regs[1].col_ranges), stops(regs[1].col_ranges)
        wls, cls = f32(collect(regs[1].weights)), f32(collect(regs[1].centers))
        wmu, cmu = f32(collect(regs[3].weights)), f32(collect(regs[3].centers))
    end
    if nviews > 0 && isa(regs[2], PM.BatchArrayReg) && isa(regs[4], PM.BatchArrayReg)
        wld, cld = f32(vcat(regs[2].weights...)), f32(vcat(regs[2].centers...))
        wth, cth = f32(vcat(regs[4].weights...)), f32(vcat(regs[4].centers...))
    end
    p(a) = isempty(a) ? nul : pointer(a)
    GC.@preserve s e wls cls wmu cmu wld cld wth cth chk(ccall((:pmf_set_layer_regs, LIB[]), Cint,
        (Ptr{Cvoid}, Cint, Ptr{Int64}, Ptr{Int64}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat},
         Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}),
        ctx, length(s), s, e, p(wls), p(cls), p(wmu), p(cmu), p(wld), p(cld), p(wth), p(cth)))
end

mask(xs, T) = Cint(sum((isa(x, T) ? 1 : 0) << (i - 1) for (i, x) in enumerate(xs)))

"""Replacement for PathMatFac.mf_fit! (src/fit.jl:9-38)."""
function mf_fit!(model::PM.PathMatFacModel; update_X=false, update_Y=false, update_col_layers=false,
                 opt=nothing, lr=0.01, max_epochs=1000, epoch=1, rel_tol=1e-6, abs_tol=1e-9, tol_max_iters=3,
                 verbosity=1, print_iter=10, capacity=10^8, keep_history=true, kwargs...)
    ctx = context!(model)
    mf = model.matfac
    marshal!(ctx, mf)
    opt === nothing && (opt = PM.construct_optimizer(model, lr))
    if get(OPT_KEY, model, UInt(0)) != objectid(opt)     # new optimizer object => fresh state (src/fit.jl:55)
        # Flux.Optimise.Adam(eta, beta::Tuple, epsilon) -> kind 1 with its own betas; anything else is the AdaGrad that
        # construct_optimizer makes (src/fit.jl:41-43) -> kind 0, where the betas are not read
        is_adam = isdefined(PM, :Flux) && opt isa PM.Flux.Optimise.Adam
        b1, b2 = is_adam ? (Float32(opt.beta[1]), Float32(opt.beta[2])) : (0.9f0, 0.999f0)
        chk(ccall((:pmf_set_optimizer, LIB[]), Cint, (Ptr{Cvoid}, Cint, Cfloat, Cfloat, Cfloat, Cfloat),
                  ctx, is_adam ? 1 : 0, opt.eta, opt.epsilon, b1, b2))
        OPT_KEY[model] = objectid(opt)
    else                                                  # same optimizer, possibly halved eta (src/fit.jl:64)
        chk(ccall((:pmf_set_lr, LIB[]), Cint, (Ptr{Cvoid}, Cfloat), ctx, opt.eta))
    end
    frozen = mask(mf.col_transform.layers, PM.FrozenLayer) | mask(mf.col_transform.layers, Function)
    frozen_regs = isa(mf.col_transform_reg, PM.SequenceReg) ? mask(mf.col_transform_reg.regs, PM.FrozenRegularizer) : Cint(0)
    opts = FitOpts(update_X, update_Y, update_col_layers, frozen, frozen_regs, max_epochs, epoch, tol_max_iters,
                   keep_history, verbosity, print_iter, 0, abs_tol, rel_tol, capacity)
    trace = zeros(Cdouble, max(max_epochs - epoch + 1, 1))
    res = FitResult(0, 0, 0, length(trace), 0.0, pointer(trace), 0.0)
    GC.@preserve trace chk(ccall((:pmf_fit, LIB[]), Cint, (Ptr{Cvoid}, Ref{FitOpts}, Ref{FitResult}), ctx, opts, res))
    unmarshal!(ctx, mf, update_X, update_Y, update_col_layers)
    return Dict("term_code" => TERM_CODES[res.term_code + 1], "epochs" => Int(res.epochs),
                "loss" => trace[1:res.n_trace], "total_loss" => res.final_loss)
end

"""Replacement for PathMatFac.fit_lbfgs! (src/fit_lbfgs.jl:170-243) on the model's device context: L-BFGS over X and Y
(pmf_fit_lbfgs; DESIGN.md section 2, "Deviation 2 / L-BFGS").  X_reg / Y_reg are marshalled as in mf_fit!, where a plain
function counts as `x -> 0`: the closures init_factors! swaps in (src/fit.jl:266-267, 0.05 * sum(x .* x)) cannot be read
from outside, so its L-BFGS branch passes `factor_l2 = 0.1f0` instead, the weight of the library's L2 term
0.5 * w * sum(x .* x) that equals them.  Returns a Dict like mf_fit!'s."""
function fit_lbfgs!(model::PM.PathMatFacModel; m=10, max_iter=1000, rel_tol=1e-9, abs_tol=1e-6, backtrack_shrinkage=0.8,
                    print_prefix="", print_iter=10, verbosity=1, factor_l2=nothing, kwargs...)
    ctx = context!(model)
    mf = model.matfac
    marshal!(ctx, mf)
    if factor_l2 !== nothing
        w = fill(Float32(factor_l2), size(mf.X, 1))
        chk(ccall((:pmf_clear_xreg, LIB[]), Cint, (Ptr{Cvoid},), ctx))
        chk(ccall((:pmf_clear_yreg, LIB[]), Cint, (Ptr{Cvoid},), ctx))
        GC.@preserve w begin
            chk(ccall((:pmf_add_xreg_l2, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cfloat}, Cfloat), ctx, w, 1f0))
            chk(ccall((:pmf_add_yreg_l2, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cfloat}, Cfloat), ctx, w, 1f0))
        end
    end
    opts = LbfgsOpts(m, max_iter, 100, 1, verbosity, print_iter, rel_tol, abs_tol, backtrack_shrinkage, 1e-4, 1e-4)
    cap = max(max_iter, 1)
    loss, trials, flags = zeros(Cdouble, cap), zeros(Cint, cap), zeros(Cint, cap)
    res = LbfgsResult(0, 0, 0, 0, 0, 0, cap, 0, 0.0, 0.0, pointer(loss), pointer(trials), pointer(flags))
    GC.@preserve loss trials flags chk(ccall((:pmf_fit_lbfgs, LIB[]), Cint, (Ptr{Cvoid}, Ref{LbfgsOpts}, Ref{LbfgsResult}),
                                             ctx, opts, res))
    unmarshal!(ctx, mf, true, true, false)
    return Dict("term_code" => TERM_CODES[res.term_code + 1], "iters" => Int(res.iters), "loss" => loss[1:res.n_trace],
                "trials" => trials[1:res.n_trace], "flags" => flags[1:res.n_trace], "total_loss" => res.final_loss)
end

function unmarshal!(ctx, mf, update_X, update_Y, update_col_layers)
    if update_X || update_Y
        X, Y = similar(mf.X, Float32), similar(mf.Y, Float32)
        GC.@preserve X Y chk(ccall((:pmf_get_factors, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cfloat}, Ptr{Cfloat}), ctx, X, Y))
        update_X && (mf.X .= X)
        update_Y && (mf.Y .= Y)
    end
    if update_col_layers
        layers = map(unwrap, mf.col_transform.layers)
        N = size(mf.Y, 2)
        ls, mu = zeros(Float32, N), zeros(Float32, N)
        GC.@preserve ls mu chk(ccall((:pmf_get_col_params, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cfloat}, Ptr{Cfloat}), ctx, ls, mu))
        isa(layers[1], PM.ColScale) && (layers[1].logsigma .= ls)
        isa(layers[3], PM.ColShift) && (layers[3].mu .= mu)
        if isa(layers[4], PM.BatchShift)
            for v in 1:length(layers[4].theta.values)
                ld, th = similar(layers[2].logdelta.values[v], Float32), similar(layers[4].theta.values[v], Float32)
                GC.@preserve ld th chk(ccall((:pmf_get_batch_view, LIB[]), Cint,
                                             (Ptr{Cvoid}, Cint, Ptr{Cfloat}, Ptr{Cfloat}), ctx, v - 1, ld, th))
                layers[2].logdelta.values[v] .= ld
                layers[4].theta.values[v] .= th
            end
        end
    end
end

# ---- the closed-form stages, each ONE library call on the marshalled model (include/pmf_hip.h, pmf_stage_*) -------------
# Masked column / batch statistics of the model's rows (pmf_stats); batch arrays flat over (view, column, batch).
function stats(model::PM.PathMatFacModel; use_factors::Bool=false)
    ctx = context!(model)
    nviews = marshal!(ctx, model.matfac; with_regs=false)
    N = size(model.data, 2)
    nbt = nviews == 0 ? 0 : sum(length(v) for v in batch_array(model.matfac).values)
    n, s1, s2, se, sg = zeros(Float32, N), zeros(Float32, N), zeros(Float32, N), zeros(Float32, N), zeros(Float32, N)
    bc, bs = zeros(Float32, max(nbt, 1)), zeros(Float32, max(nbt, 1))
    GC.@preserve n s1 s2 se sg bc bs chk(ccall((:pmf_stats, LIB[]), Cint,
        (Ptr{Cvoid}, Cint, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}),
        ctx, use_factors, n, s1, s2, se, sg, bc, bs))
    return (n = n, sum = s1, sumsq = s2, sqerr = se, ssq_grad = sg, batch_count = bc[1:nbt], batch_sqerr = bs[1:nbt])
end

# the BatchArray that fixes the views (layers 2 and 4 share ranges and row batches), or nothing
function batch_array(mf)
    layers = map(unwrap, mf.col_transform.layers)
    return isa(layers[2], PM.BatchScale) ? layers[2].logdelta : (isa(layers[4], PM.BatchShift) ? layers[4].theta : nothing)
end

function noise_weights_from_device(ctx, N)
    w = zeros(Float32, N)
    GC.@preserve w chk(ccall((:pmf_get_noise_weights, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cfloat}), ctx, w))
    return w
end

"""Replacement for PathMatFac.init_logsigma! (src/fit.jl:125-148): pmf_stage_init_logsigma, logsigma copied back."""
function init_logsigma!(model::PM.PathMatFacModel; capacity=Int(10e8), history=nothing)
    ctx = context!(model)
    marshal!(ctx, model.matfac; with_regs=false)
    chk(ccall((:pmf_stage_init_logsigma, LIB[]), Cint, (Ptr{Cvoid},), ctx))
    N = size(model.data, 2)
    ls = zeros(Float32, N)
    GC.@preserve ls chk(ccall((:pmf_get_col_params, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cfloat}, Ptr{Cfloat}), ctx, ls, C_NULL))
    unwrap(model.matfac.col_transform.layers[1]).logsigma .= ls
    PM.history!(history; name="init_logsigma")
end

"""Replacement for PathMatFac.reweight_col_losses! (src/fit.jl:151-187): pmf_stage_reweight_col_losses, the noise
weights copied back through MF.set_weight!.  `M_total`: all samples when the rows are sharded over ranks."""
function reweight_col_losses!(model::PM.PathMatFacModel; capacity=Int(10e8), history=nothing,
                              M_total::Integer=size(model.data, 1))
    ctx = context!(model)
    marshal!(ctx, model.matfac; with_regs=false)
    chk(ccall((:pmf_stage_reweight_col_losses, LIB[]), Cint, (Ptr{Cvoid}, Int64), ctx, M_total))
    PM.MF.set_weight!(model.matfac.noise_model, noise_weights_from_device(ctx, size(model.data, 2)))
    PM.history!(history; name="reweight_col_losses")
end

"""Replacement for PathMatFac.construct_minimal_regularizer (src/regularizers.jl:750-774): one weight per column range of
the noise model from pmf_stage_minimal_group_weights, repeated over the K factors."""
function construct_minimal_regularizer(model; capacity=10^8, M_total::Integer=size(model.data, 1))
    ctx = context!(model)
    mf = model.matfac
    marshal!(ctx, mf; with_regs=false)
    nm = mf.noise_model
    K = size(mf.X, 1)
    gw = zeros(Float32, length(nm.col_ranges))
    GC.@preserve gw chk(ccall((:pmf_stage_minimal_group_weights, LIB[]), Cint, (Ptr{Cvoid}, Int64, Ptr{Cfloat}), ctx, M_total, gw))
    # One group per noise range, labelled by the noise struct's type name: downstream code looks groups up by exactly
    # these labels and ranges, so they have to be the ones the replaced function produces.
    labels = String[string(typeof(noise)) for noise in nm.noises]
    ranges = Tuple(first(r):last(r) for r in nm.col_ranges)
    return PM.GroupRegularizer(labels, ranges, Tuple(fill(w, K) for w in gw))
end

"""Replacement for PathMatFac.theta_delta_em (src/fit.jl:326-375).  It gets a MatFacModel copy and the data, so the
context is keyed by the data array: a SECOND context beside the model's own, with its own device copy of the data
(8 GB at 100000 x 20000) for the duration of the call.  It is released before the function returns (`keep_context=true`
keeps it for a host that calls the EM repeatedly on one matrix; release!(data) frees it then).  theta of every view and
delta2 come back; nothing else is copied."""
function theta_delta_em(matfac, delta2::Tuple, sigma2::AbstractVector, data::AbstractMatrix; update_priors=true,
                        capacity=10^8, batch_em_max_iter=100, batch_em_rtol=1e-8, verbosity=1, print_prefix="",
                        history=nothing, keep_context::Bool=false)
    try
        return theta_delta_em_on!(data_context!(data, data), matfac, delta2, sigma2; update_priors=update_priors,
                                  batch_em_max_iter=batch_em_max_iter, batch_em_rtol=batch_em_rtol, verbosity=verbosity,
                                  print_prefix=print_prefix, history=history)
    finally
        keep_context || release!(data)
    end
end

function theta_delta_em_on!(ctx, matfac, delta2, sigma2; update_priors, batch_em_max_iter, batch_em_rtol, verbosity,
                            print_prefix, history)
    nviews = marshal!(ctx, matfac; with_regs=false)
    theta = unwrap(matfac.col_transform.layers[4]).theta
    d2 = Float64[]
    for d in delta2
        append!(d2, vec(convert(Array{Float64}, d)))     # nb x N_v column-major per view: flat like theta
    end
    s2 = f32(collect(sigma2))
    diffs = zeros(Cdouble, max(batch_em_max_iter, 1))
    opts = EmOpts(update_priors, batch_em_max_iter, 0, 0, batch_em_rtol)
    res = EmResult(0, 0, length(diffs), 0, pointer(diffs), 0.0)
    GC.@preserve d2 s2 diffs chk(ccall((:pmf_stage_theta_delta_em, LIB[]), Cint,
        (Ptr{Cvoid}, Ref{EmOpts}, Ptr{Cfloat}, Ptr{Cdouble}, Ref{EmResult}), ctx, opts, s2, d2, res))
    new_delta2 = Any[]
    off = 0
    for v in 1:nviews
        th = zeros(Float32, size(theta.values[v]))
        GC.@preserve th chk(ccall((:pmf_get_batch_view, LIB[]), Cint, (Ptr{Cvoid}, Cint, Ptr{Cfloat}, Ptr{Cfloat}),
                                  ctx, v - 1, C_NULL, th))
        theta.values[v] .= th
        n = length(th)
        push!(new_delta2, reshape(d2[off+1:off+n], size(th)))
        off += n
    end
    trace = diffs[1:res.n_diffs]
    if verbosity > 0
        for (it, d) in enumerate(trace)
            println(print_prefix, "(", it, ") ||theta - theta'||^2/||theta||^2 : ", d)
        end
    end
    PM.history!(history; name="batch_effect_EM_procedure", diffs=trace)
    return theta.values, Tuple(new_delta2)
end

"""Replacement for PathMatFac.init_mu! (src/fit.jl:82-103): the per-column M-estimates are the minimisers over mu alone
with X'Y = 0, found by this file's mf_fit! on the ColShift layer with every other layer and every layer regularizer
frozen (rel_tol 1e-5, abs_tol 1e-3), as pathmatfac.jl_amd/fit.py:init_mu_ does it."""
function init_mu!(model::PM.PathMatFacModel; capacity=Int(10e8), lr_mu=0.1, max_epochs=500, verbosity=1,
                  print_prefix="", history=nothing, kwargs...)
    mf = model.matfac
    ct = mf.col_transform
    X0, Y0 = mf.X, mf.Y
    mf.X, mf.Y = zero(X0), zero(Y0)
    others = [l for l in (1, 2, 4) if !isa(ct.layers[l], PM.FrozenLayer)]
    PM.freeze_layer!(ct, others)
    sr = mf.col_transform_reg
    regs = isa(sr, PM.SequenceReg) ? [l for l in 1:4 if !isa(sr.regs[l], PM.FrozenRegularizer)] : Int[]
    isempty(regs) || PM.freeze_reg!(sr, regs)
    h = nothing
    try
        h = mf_fit!(model; opt=PM.construct_optimizer(model, lr_mu), update_col_layers=true, max_epochs=max_epochs,
                    rel_tol=1e-5, abs_tol=1e-3, verbosity=verbosity - 1, print_prefix=print_prefix, capacity=capacity)
    finally
        PM.unfreeze_layer!(ct, others)
        isempty(regs) || PM.unfreeze_reg!(sr, regs)
        mf.X, mf.Y = X0, Y0
    end
    history === nothing || PM.history!(history, h; name="init_mu")
end

"""Replacement for PathMatFac.update_A! (src/featureset_ard.jl:278-294): per view one pmf_fsard_update_A -- or, where
L * K exceeds that entry's capacity, one pmf_fsard_update_A_csr on the sparse S -- on a context of the regularizer's own
that holds Y (an all-missing one-row data matrix fixes N; X is a zero column).  `kernel`: :auto (the dense entry wherever it
accepts the shape, as the Python twin update_A_ chooses), :dense or :sparse."""
function update_A!(reg::PM.FeatureSetARDReg, Y::AbstractMatrix; max_epochs=1000, term_iter=20, atol=1e-5, verbosity=1,
                   print_prefix="", print_iter=100, kernel::Symbol=:auto)
    kernel in (:auto, :dense, :sparse) || throw(ArgumentError("update_A!: kernel must be :auto, :dense or :sparse"))
    K, N = size(Y)
    ctx = data_context!(reg, get!(() -> fill(NaN32, 1, N), FSARD_DATA, reg))
    X0, Y32 = zeros(Float32, K, 1), f32(Y)
    GC.@preserve X0 Y32 chk(ccall((:pmf_set_factors, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cfloat}, Ptr{Cfloat}, Cint), ctx, X0, Y32, K))
    chk(ccall((:pmf_clear_yreg, LIB[]), Cint, (Ptr{Cvoid},), ctx))
    add_reg!(ctx, :Y, reg)
    beta_all = f32(reg.beta)
    for (v, cr) in enumerate(reg.col_ranges)
        opt = reg.A_opts[v]
        L = size(reg.S[v], 1)
        sparse = kernel == :sparse || (kernel == :auto && L * K > FSARD_DENSE_CAPACITY)
        A_t = zeros(Float32, K, L)                          # update_A! starts every view from A = 0 (:286)
        ssq_t = f32(Matrix(transpose(opt.ssq_grad)))
        beta = zeros(Float32, K, length(cr))
        kw = (alpha0=Float32(reg.alpha0), v0=Float32(reg.v0), lr=Float32(opt.lr), max_epochs=max_epochs,
              term_iter=term_iter, atol=Float64(atol), ctx=ctx)
        best, _ = if sparse
            S_csc = SparseArrays.SparseMatrixCSC(transpose(reg.S[v]))     # N_v x L: its columns are the rows of S
            fsard_update_A_csr!(reg, cr, S_csc, f32(reg.alpha[cr]), f32(vec(opt.lambda)), A_t, ssq_t, beta; kw...)
        else
            S_t = f32(Matrix(transpose(reg.S[v])))         # N_v x L column-major = L x N_v row-major
            fsard_update_A!(reg, cr, S_t, f32(reg.alpha[cr]), f32(vec(opt.lambda)), A_t, ssq_t, beta; kw...)
        end
        reg.A[v] .= transpose(A_t)
        opt.ssq_grad .= transpose(ssq_t)
        beta_all[:, cr] .= beta
        verbosity > 1 && println(print_prefix, "    View ", v, ": final loss ", best)
    end
    reg.beta .= beta_all
end

# ---- factor post-processing, each ONE library call on the marshalled model (include/pmf_hip.h: pmf_stage_whiten, ----------
# pmf_stage_rotate_by_svd, pmf_stage_reorder_by_importance, pmf_stage_lambda_max).  X and Y stay on the device for the
# call; only what changed is copied back.  On a row-sharded model (comm_init!) the X-side sums are summed over the ranks
# inside the library: whiten! takes M_total, the L2 / Group reweight_eb! of the X regularizer take `model`.
const EB_DATA = IdDict{Any,Matrix{Float32}}()      # regularizer => the all-missing 1 x n matrix of its own context (reweight_eb!)

function factors_from_device!(ctx, mf)
    X, Y = similar(mf.X, Float32), similar(mf.Y, Float32)
    GC.@preserve X Y chk(ccall((:pmf_get_factors, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cfloat}, Ptr{Cfloat}), ctx, X, Y))
    mf.X .= X
    mf.Y .= Y
end

"""Replacement for PathMatFac.whiten! (src/fit.jl:504-527): pmf_stage_whiten; X, Y and logsigma copied back.
`M_total`: all samples when the rows are sharded over ranks."""
function whiten!(model::PM.PathMatFacModel; M_total::Integer=size(model.data, 1))
    ctx = context!(model)
    mf = model.matfac
    marshal!(ctx, mf; with_regs=false)
    crs = PM.ids_to_ranges(model.feature_views)
    s, e = starts(crs), stops(crs)
    GC.@preserve s e chk(ccall((:pmf_stage_whiten, LIB[]), Cint,
        (Ptr{Cvoid}, Int64, Cint, Ptr{Int64}, Ptr{Int64}, Ptr{Cdouble}, Ptr{Cdouble}), ctx, M_total, length(s), s, e, C_NULL, C_NULL))
    factors_from_device!(ctx, mf)
    l1 = unwrap(mf.col_transform.layers[1])
    if isa(l1, PM.ColScale)
        ls = zeros(Float32, size(mf.Y, 2))
        GC.@preserve ls chk(ccall((:pmf_get_col_params, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cfloat}, Ptr{Cfloat}), ctx, ls, C_NULL))
        l1.logsigma .= ls
    end
    return nothing
end

"""Replacement for PathMatFac.rotate_by_svd! (src/fit.jl:530-543): pmf_stage_rotate_by_svd (the library's own
eigen-decomposition of Y Y'; each singular vector signed so that its largest component is positive); X and Y copied back."""
function rotate_by_svd!(model::PM.PathMatFacModel)
    ctx = context!(model)
    marshal!(ctx, model.matfac; with_regs=false)
    chk(ccall((:pmf_stage_rotate_by_svd, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}), ctx, C_NULL, C_NULL))
    factors_from_device!(ctx, model.matfac)
    return nothing
end

"""Replacement for PathMatFac.reorder_by_importance! (src/fit.jl:546-555): pmf_stage_reorder_by_importance; X, Y and the
permutation come back, the regularizers (host state) are permuted here (reorder_reg!, :553-554)."""
function reorder_by_importance!(model::PM.PathMatFacModel)
    ctx = context!(model)
    mf = model.matfac
    marshal!(ctx, mf; with_regs=false)
    perm = zeros(Int32, size(mf.Y, 1))
    GC.@preserve perm chk(ccall((:pmf_stage_reorder_by_importance, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Int32}), ctx, perm))
    factors_from_device!(ctx, mf)
    srt_idx = Int.(perm) .+ 1
    PM.reorder_reg!(mf.Y_reg, srt_idx)
    PM.reorder_reg!(mf.X_reg, srt_idx)
    return nothing
end

# Largest eigenvalue of the Gram matrix of P[:, r] for every range r (= the largest squared singular value of the block).
# With `model`, P must be its X or its Y: the model's context is used (X: summed over the row shards).  Without, P goes
# to a context of the regularizer's own as the Y of an all-missing one-row data matrix, as update_A! does it.
function lambda_max(reg, P::AbstractMatrix, ranges; model=nothing)
    s, e = starts(ranges), stops(ranges)
    lam = zeros(Cdouble, length(s))
    if model !== nothing
        which = P === model.matfac.X ? 0 : (P === model.matfac.Y ? 1 : error("lambda_max: P is neither model.matfac.X nor model.matfac.Y"))
        ctx = context!(model)
        marshal!(ctx, model.matfac; with_regs=false)
    else
        K, n = size(P)
        ctx = data_context!(reg, get!(() -> fill(NaN32, 1, n), EB_DATA, reg))
        X0, P32 = zeros(Float32, K, 1), f32(P)
        GC.@preserve X0 P32 chk(ccall((:pmf_set_factors, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Cfloat}, Ptr{Cfloat}, Cint), ctx, X0, P32, K))
        which = 1
    end
    GC.@preserve s e lam chk(ccall((:pmf_stage_lambda_max, LIB[]), Cint,
        (Ptr{Cvoid}, Cint, Cint, Ptr{Int64}, Ptr{Int64}, Ptr{Cdouble}), ctx, which, length(s), s, e, lam))
    return lam
end

"""Replacement for PathMatFac.reweight_eb!(::L2Regularizer, ::AbstractMatrix) (src/regularizers.jl:39-47)."""
function reweight_eb!(reg::PM.L2Regularizer, X::AbstractMatrix; mixture_p=Float32(1.0), model=nothing)
    lam = lambda_max(reg, X, (1:size(X, 2),); model=model)
    reg.weights .= mixture_p / lam[1]
end

"""Replacement for PathMatFac.reweight_eb!(::GroupRegularizer, ::AbstractMatrix) (src/regularizers.jl:406-420)."""
function reweight_eb!(gr::PM.GroupRegularizer, X::AbstractMatrix; mixture_p=Float32(1.0), model=nothing)
    K = size(X, 1)
    lam = lambda_max(gr, X, gr.group_idx; model=model)
    gr.group_weights = Tuple(fill!(similar(X, K), mixture_p / l) for l in lam)
end

"""impute(model; include_batch_effects=false) (src/impute.jl:37-56) on the device: pmf_impute over the model's current
parameters.  `link=true` returns Z itself, `keep_observed=true` returns the observed entries of model.data and predicts
only the missing ones; `rows` (a UnitRange) bounds the host matrix.  Returns length(rows) x N Float32."""
function impute(model::PM.PathMatFacModel; include_batch_effects=false, link=false, keep_observed=false,
                rows::UnitRange=1:size(model.data, 1))
    ctx = context!(model)
    marshal!(ctx, model.matfac)
    flags = Cint((include_batch_effects ? 1 : 0) | (link ? 2 : 0) | (keep_observed ? 4 : 0))
    out = zeros(Float32, length(rows), size(model.data, 2))
    GC.@preserve out chk(ccall((:pmf_impute, LIB[]), Cint, (Ptr{Cvoid}, Cint, Int64, Int64, Ptr{Cfloat}, Int64),
                               ctx, flags, rows.start, rows.stop, out, length(rows)))
    return out
end

"""remove_batch_effect(model, Z) (src/remove_batch_effect.jl:3-16) on the device: pmf_remove_batch_effect with the model's
current column and batch parameters, against the layer order of src/layers.jl:240-253 (the reference's body inverts an
older one).  Z holds the values of `rows` (M x N by default); `link=true`: Z and the result are in link space;
`fill_missing=true`: missing entries take the batch-free prediction instead of NaN.  Returns length(rows) x N Float32."""
function remove_batch_effect(model::PM.PathMatFacModel, Z::AbstractMatrix; link=false, fill_missing=false,
                             rows::UnitRange=1:size(model.data, 1))
    size(Z) == (length(rows), size(model.data, 2)) || error("remove_batch_effect: Z must be length(rows) x N")
    ctx = context!(model)
    marshal!(ctx, model.matfac)
    flags = Cint((link ? 1 : 0) | (fill_missing ? 2 : 0))
    Z32 = f32(Z)
    out = zeros(Float32, length(rows), size(model.data, 2))
    GC.@preserve Z32 out chk(ccall((:pmf_remove_batch_effect, LIB[]), Cint,
                                   (Ptr{Cvoid}, Cint, Int64, Int64, Ptr{Cfloat}, Int64, Ptr{Cfloat}, Int64),
                                   ctx, flags, rows.start, rows.stop, Z32, length(rows), out, length(rows)))
    return out
end

"""simulate_data!(model; noise=0.1) (src/simulate_params.jl:244-255) on the device: model.data is overwritten by a draw from
the model's current parameters (pmf_simulate_data: the forward of all four layers, normal noise on the normal columns, the
class of the noise-free value on the squared-hinge columns, a 0 / 1 draw on logit-Bernoulli columns; a Poisson range is
refused).  `seed` fixes the Philox4x32-10 stream, `frac_missing` of the entries become NaN, `row_offset` is the global
index of the first local row of a row shard.  `resident=true` draws into the device's copy instead (pmf_simulate_data_resident)
and leaves model.data alone.  Returns model.data."""
function simulate_data!(model::PM.PathMatFacModel; noise=0.1, seed::Integer=0, frac_missing=0.0, row_offset::Integer=0,
                        resident::Bool=false, kwargs...)
    ctx = context!(model)
    marshal!(ctx, model.matfac)
    opts = Ref(SimOpts(UInt64(seed), Int64(row_offset), Cfloat(noise), Cfloat(frac_missing)))
    if resident
        chk(ccall((:pmf_simulate_data_resident, LIB[]), Cint, (Ptr{Cvoid}, Ref{SimOpts}), ctx, opts))
        return model.data
    end
    M, N = size(model.data)
    out = zeros(Float32, M, N)
    GC.@preserve out chk(ccall((:pmf_simulate_data, LIB[]), Cint, (Ptr{Cvoid}, Ref{SimOpts}, Int64, Int64, Ptr{Cfloat}, Int64),
                               ctx, opts, 1, M, out, M))
    model.data .= out
    delete!(DATA_KEY, model)      # the device copy is of the old values: the next context!(model) uploads the new ones
    return model.data
end

"""Point PathMatFac's drop-in boundary at the HIP library."""
function install!(libpath::AbstractString="libpmf_hip.so")
    LIB[] = libpath
    @eval PathMatFac mf_fit!(model::PathMatFacModel; kwargs...) = Main.PathMatFacHIP.mf_fit!(model; kwargs...)
    @eval PathMatFac init_mu!(model::PathMatFacModel; kwargs...) = Main.PathMatFacHIP.init_mu!(model; kwargs...)
    @eval PathMatFac init_logsigma!(model::PathMatFacModel; kwargs...) = Main.PathMatFacHIP.init_logsigma!(model; kwargs...)
    @eval PathMatFac reweight_col_losses!(model::PathMatFacModel; kwargs...) = Main.PathMatFacHIP.reweight_col_losses!(model; kwargs...)
    @eval PathMatFac construct_minimal_regularizer(model; kwargs...) = Main.PathMatFacHIP.construct_minimal_regularizer(model; kwargs...)
    @eval PathMatFac theta_delta_em(model::MF.MatFacModel, delta2::Tuple, sigma2::AbstractVector, data::AbstractMatrix; kwargs...) =
        Main.PathMatFacHIP.theta_delta_em(model, delta2, sigma2, data; kwargs...)
    @eval PathMatFac update_A!(reg::FeatureSetARDReg, Y::AbstractMatrix; kwargs...) = Main.PathMatFacHIP.update_A!(reg, Y; kwargs...)
    @eval PathMatFac whiten!(model::PathMatFacModel; kwargs...) = Main.PathMatFacHIP.whiten!(model; kwargs...)
    @eval PathMatFac rotate_by_svd!(model::PathMatFacModel; kwargs...) = Main.PathMatFacHIP.rotate_by_svd!(model; kwargs...)
    @eval PathMatFac reorder_by_importance!(model::PathMatFacModel; kwargs...) = Main.PathMatFacHIP.reorder_by_importance!(model; kwargs...)
    @eval PathMatFac reweight_eb!(reg::L2Regularizer, X::AbstractMatrix; kwargs...) = Main.PathMatFacHIP.reweight_eb!(reg, X; kwargs...)
    @eval PathMatFac reweight_eb!(reg::GroupRegularizer, X::AbstractMatrix; kwargs...) = Main.PathMatFacHIP.reweight_eb!(reg, X; kwargs...)
    @eval PathMatFac remove_batch_effect(model::PathMatFacModel, Z::AbstractMatrix; kwargs...) = Main.PathMatFacHIP.remove_batch_effect(model, Z; kwargs...)
    @eval PathMatFac simulate_data!(model::PathMatFacModel; kwargs...) = Main.PathMatFacHIP.simulate_data!(model; kwargs...)
    return nothing
end

function release!(model)
    haskey(CTX, model) && (ccall((:pmf_destroy, LIB[]), Cint, (Ptr{Cvoid},), CTX[model]); delete!(CTX, model))
    delete!(DATA_KEY, model); delete!(OPT_KEY, model); delete!(FSARD_DATA, model); delete!(EB_DATA, model)   # (the last two are keyed by a regularizer: release!(reg))
    return nothing
end

end # module
