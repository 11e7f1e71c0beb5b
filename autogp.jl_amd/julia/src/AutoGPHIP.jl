# AutoGPHIP.jl — Julia-side binding of libautogp_hip.so (include/autogp_hip.h).
#
# STATUS: source only.  Julia is not installed in the build container nor on the GPU box, so this file has never been
# executed; every executable test drives the same C ABI from Python/ctypes and from C++ (tools/native/).  Statements
# about Gen's internals below (how the dynamic DSL calls logpdf / logpdf_grad, what choice_gradients passes) are
# recalled from Gen 0.4's public source, which is not under /root/reference and could not be inspected here.
#
# It is the `ccall` layer a maintainer of AutoGP.jl adds to switch the hot call sites
#   src/Model.jl:135-136   (compute_cov_matrix_vectorized + `xs ~ mvnormal(zeros(n), K)`)
#   src/GP.jl:731-758      (Distributions.MvNormal(node, noise, ts, xs, ts_pred; ...))
#   src/GP.jl:904-993      (GP.infer_gp_sum)
# to the MI355X engine while `Inference.jl`, the SMC/MCMC moves and the public API stay untouched.
module AutoGPHIP

using LinearAlgebra
import Gen
import Distributions
import AutoGP
const GP = AutoGP.GP

# library: AUTOGP_HIP_LIB, else the path deps/build.jl recorded, else the loader's search path
const _DEPS = joinpath(@__DIR__, "..", "deps", "deps.jl")
isfile(_DEPS) && include(_DEPS)
const LIB = get(ENV, "AUTOGP_HIP_LIB", @isdefined(libautogp_hip) ? libautogp_hip : "libautogp_hip.so")
const COMM_ID_BYTES = 128

# ------------------------------------------------------------------------------------------------------------------
# contexts
# ------------------------------------------------------------------------------------------------------------------
mutable struct Engine
    ptr::Ptr{Cvoid}
    n_max::Int
    ts::Vector{Float64}     # host copies of the resident series: Gen hands (ts, xs) to logpdf on every call and
    xs::Vector{Float64}     # the shim must know whether they ARE the resident prefix
    lag_level::Int32        # last level given to agp_set_lag_tables (0 off, 1 tables, 2 / 3 structured sweeps); the library's default is 1
    lag_level_before::Int32 # ... and the one set_structured_sweeps!(eng, true) replaced
end

function check(eng::Union{Engine,Nothing}, rc::Cint)
    rc == 0 && return
    p = isnothing(eng) ? C_NULL : eng.ptr
    msg = unsafe_string(ccall((:agp_last_error, LIB), Cstring, (Ptr{Cvoid},), p))
    error("autogp_hip call failed ($rc): $msg")
end

destroy!(e::Engine) = (e.ptr != C_NULL && ccall((:agp_destroy, LIB), Cvoid, (Ptr{Cvoid},), e.ptr); e.ptr = C_NULL; nothing)

"the level the library starts from: AGP_LAG (0 .. 3), 1 when unset"
default_lag_level() = Int32(clamp(something(tryparse(Int, get(ENV, "AGP_LAG", "1")), 1), 0, 3))

"One engine per GPU."
function Engine(device::Integer=0)
    ref = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:agp_init, LIB), Cint, (Ref{Ptr{Cvoid}}, Cint), ref, device)
    check(nothing, rc)
    eng = Engine(ref[], 0, Float64[], Float64[], default_lag_level(), default_lag_level())
    finalizer(destroy!, eng)
    return eng
end

"""
One Julia process driving several GPUs (agp_init_multi: n contexts + one RCCL communicator over them).
`engine_for_thread(pool)` maps the calling Julia thread to a device, so that the reference's
`Threads.@threads for i=1:num_particles` loops (src/inference_smc_anneal_data.jl:133,240; src/api.jl:293,386) spread
their single-particle calls over the node: thread t always talks to device (t-1) % n_dev + 1, each device coalesces
its own callers.
"""
struct EnginePool
    engines::Vector{Engine}
end

function EnginePool(devices::AbstractVector{<:Integer})
    n = length(devices)
    ptrs = fill(C_NULL, n); ids = Int32.(collect(devices))
    GC.@preserve ptrs ids check(nothing, ccall((:agp_init_multi, LIB), Cint, (Ptr{Ptr{Cvoid}}, Ptr{Int32}, Int32), ptrs, ids, n))
    engines = [Engine(p, 0, Float64[], Float64[], default_lag_level(), default_lag_level()) for p in ptrs]
    foreach(e -> finalizer(destroy!, e), engines)
    return EnginePool(engines)
end

engine_for_thread(pool::EnginePool) = pool.engines[(Threads.threadid() - 1) % length(pool.engines) + 1]
engine_for_thread(eng::Engine) = eng

"Upload the rescaled observations once; later calls use prefixes ts[1:n] (data annealing).  Appending observations
(add_data!, src/api.jl:426-443) keeps the resident factors of `logpdf_batch_extend` valid."
function set_data!(eng::Engine, ts::Vector{Float64}, xs::Vector{Float64})
    @assert length(ts) == length(xs)
    GC.@preserve ts xs check(eng, ccall((:agp_set_data, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64), eng.ptr, ts, xs, length(ts)))
    eng.n_max = length(ts); eng.ts = copy(ts); eng.xs = copy(xs)
    return eng
end
set_data!(pool::EnginePool, ts::Vector{Float64}, xs::Vector{Float64}) = (foreach(e -> set_data!(e, ts, xs), pool.engines); pool)

"remove_data! (src/api.jl:449-468): delete the observations at the 1-based ascending positions `idx` of the resident series.  Resident
factors that contain removed positions are updated on the device (or dropped where refactoring is cheaper), so
`logpdf_batch(...; extend=true)` on the reduced series starts from them."
function remove_data!(eng::Engine, idx::AbstractVector{<:Integer})
    isempty(idx) && error("No such time points.")
    idx0 = Int64[i - 1 for i in idx]
    GC.@preserve idx0 check(eng, ccall((:agp_remove_data, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Int64), eng.ptr, idx0, length(idx0)))
    keep = setdiff(1:eng.n_max, idx)
    eng.ts = eng.ts[keep]; eng.xs = eng.xs[keep]; eng.n_max = length(keep)
    return eng
end

"(updated, dropped, rows_removed, panel_steps) of `remove_data!` since the engine was created"
function remove_stats(eng::Engine)
    out = zeros(Int64, 4)
    GC.@preserve out check(eng, ccall((:agp_get_remove_stats, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Int32), eng.ptr, out, 4))
    return (updated = out[1], dropped = out[2], rows_removed = out[3], panel_steps = out[4])
end

"Is (ts, xs) the prefix of the resident series?  O(n) comparisons next to an O(n^3) factorisation."
function is_resident_prefix(eng::Engine, ts::AbstractVector{<:Real}, xs::AbstractVector{<:Real})
    n = length(ts)
    (n == length(xs) && n <= eng.n_max) || return false
    @inbounds for i in 1:n
        (ts[i] == eng.ts[i] && xs[i] == eng.xs[i]) || return false
    end
    return true
end

# ------------------------------------------------------------------------------------------------------------------
# kernel tree -> postfix program (opcodes = GPConfig codes, src/GP.jl:1101-1108; 0 = WhiteNoise)
# ------------------------------------------------------------------------------------------------------------------
opcode(::GP.WhiteNoise) = 0x00; opcode(::GP.Constant) = 0x01; opcode(::GP.Linear) = 0x02
opcode(::GP.SquaredExponential) = 0x03; opcode(::GP.GammaExponential) = 0x04; opcode(::GP.Periodic) = 0x05
opcode(::GP.Plus) = 0x06; opcode(::GP.Times) = 0x07; opcode(::GP.ChangePoint) = 0x08

params(n::GP.WhiteNoise) = (n.value,)
params(n::GP.Constant) = (n.value,)
params(n::GP.Linear) = (n.intercept, n.bias, n.amplitude)
params(n::GP.SquaredExponential) = (n.lengthscale, n.amplitude)
params(n::GP.GammaExponential) = (n.lengthscale, n.gamma, n.amplitude)
params(n::GP.Periodic) = (n.lengthscale, n.period, n.amplitude)
params(n::GP.ChangePoint) = (n.location, n.scale)
params(::GP.BinaryOpNode) = ()

"Opcodes of the tree in `GP.unroll` order (left, right, node — src/GP.jl:112-113)."
structure(node::GP.Node) = UInt8[opcode(n) for n in GP.unroll(node)]
"Parameters in the same order, struct-field order within a node; entries keep their type (Float64 or a tracked Real)."
flat_params(node::GP.Node) = [v for n in GP.unroll(node) for v in params(n)]

"(ops, prm) of the C ABI."
encode(node::GP.Node) = (structure(node), Float64[Float64(v) for v in flat_params(node)])

function encode_batch(nodes::Vector{<:GP.Node})
    op_off = Int32[0]; prm_off = Int32[0]; ops = UInt8[]; prm = Float64[]
    for nd in nodes
        o, q = encode(nd)
        append!(ops, o); append!(prm, q)
        push!(op_off, length(ops)); push!(prm_off, length(prm))
    end
    isempty(prm) && push!(prm, 0.0)
    return op_off, ops, prm_off, prm
end

# ------------------------------------------------------------------------------------------------------------------
# value path
# ------------------------------------------------------------------------------------------------------------------
function logpdf_program(eng::Engine, ops::Vector{UInt8}, prm::Vector{Float64}, noise::Float64, n::Integer)
    np_ = length(prm)
    q = isempty(prm) ? [0.0] : prm
    out = Ref{Float64}(0.0); info = Ref{Int32}(0)
    GC.@preserve ops q check(eng, ccall((:agp_logpdf, LIB), Cint,
        (Ptr{Cvoid}, Int64, Ptr{UInt8}, Int32, Ptr{Float64}, Int32, Float64, Ref{Float64}, Ref{Int32}),
        eng.ptr, n, ops, length(ops), q, np_, noise, out, info))
    info[] > 0 && throw(LinearAlgebra.PosDefException(info[]))   # the reference aborts on non-PD too
    return out[]
end

"log N(xs[1:n]; 0, eval_cov(node, ts[1:n]) + noise*I) on the resident data — replaces src/Model.jl:135-136."
logpdf(eng::Engine, node::GP.Node, noise::Float64, n::Integer=eng.n_max) = logpdf_program(eng, encode(node)..., noise, n)

"All particles in one sweep."
function logpdf_batch(eng::Engine, nodes::Vector{<:GP.Node}, noises::Vector{Float64}, n::Integer=eng.n_max; extend::Bool=false)
    P = length(nodes)
    op_off, ops, prm_off, prm = encode_batch(nodes)
    out = Vector{Float64}(undef, P); info = Vector{Int32}(undef, P)
    # extend = true: agp_logpdf_batch_extend — factors stay resident, a later call on a longer prefix only computes the
    # new tile rows (the reweight step of data annealing, src/inference_smc_anneal_data.jl:206-217)
    GC.@preserve op_off ops prm_off prm noises out info begin
        rc = extend ?
            ccall((:agp_logpdf_batch_extend, LIB), Cint,
                (Ptr{Cvoid}, Int64, Int32, Ptr{Int32}, Ptr{UInt8}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                eng.ptr, n, P, op_off, ops, prm_off, prm, noises, out, info) :
            ccall((:agp_logpdf_batch, LIB), Cint,
                (Ptr{Cvoid}, Int64, Int32, Ptr{Int32}, Ptr{UInt8}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                eng.ptr, n, P, op_off, ops, prm_off, prm, noises, out, info)
        check(eng, rc)
    end
    return out, info
end

"Longest series of `logpdf_series_batch` (AGP_SERIES_MAX_N)."
const SERIES_MAX_N = 176

"Many short series in one fused launch (agp_logpdf_series_batch): `series` is a vector of `(ts, xs)` pairs of at most
`SERIES_MAX_N` points each, particle `p` scores `series[series_index[p]]` (1-based).  Needs no `set_data!` and leaves the
resident series, the factor store and every counter alone.  Returns `(logpdf, info)`."
function logpdf_series_batch(eng::Engine, series::Vector{<:Tuple{Vector{Float64},Vector{Float64}}}, nodes::Vector{<:GP.Node},
                             noises::Vector{Float64}, series_index::Vector{<:Integer})
    P = length(nodes)
    (length(noises) == P && length(series_index) == P) || throw(ArgumentError("one noise and one series index per particle required"))
    pt_off = Int64[0]; ts = Float64[]; xs = Float64[]
    for (s, (t, x)) in enumerate(series)
        length(t) == length(x) || throw(ArgumentError("series $s: ts and xs must have equal lengths"))
        length(t) <= SERIES_MAX_N || throw(ArgumentError("series $s has $(length(t)) points, more than SERIES_MAX_N ($SERIES_MAX_N)"))
        append!(ts, t); append!(xs, x); push!(pt_off, length(ts))
    end
    isempty(ts) && (push!(ts, 0.0); push!(xs, 0.0))
    sidx = Int32[Int32(i - 1) for i in series_index]
    op_off, ops, prm_off, prm = encode_batch(nodes)
    out = Vector{Float64}(undef, P); info = Vector{Int32}(undef, P)
    GC.@preserve pt_off ts xs sidx op_off ops prm_off prm noises out info check(eng, ccall((:agp_logpdf_series_batch, LIB), Cint,
        (Ptr{Cvoid}, Int32, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{UInt8}, Ptr{Int32}, Ptr{Float64},
         Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
        eng.ptr, length(series), pt_off, ts, xs, P, sidx, op_off, ops, prm_off, prm, noises, out, info))
    return out, info
end

"Longest series of `logpdf_long_series_batch` (AGP_LONG_SERIES_MAX_N)."
const LONG_SERIES_MAX_N = 512
"`flags` bit of agp_logpdf_long_series_batch: every non-empty series takes the long kernel (AGP_LONG_SERIES_ALL)."
const LONG_SERIES_ALL = Int32(1)

"`logpdf_series_batch` for series of at most `LONG_SERIES_MAX_N` points (agp_logpdf_long_series_batch): same arguments, same
statelessness, one call for a mixed family such as 135, 143 and 442 points.  A series of at most `SERIES_MAX_N` points runs in
`logpdf_series_batch`'s kernel (bit-identical results), a longer one in the long-series kernel, which keeps the factor in an HBM
workspace; `all_long = true` sends every non-empty series through the long kernel.  Returns `(logpdf, info)`."
function logpdf_long_series_batch(eng::Engine, series::Vector{<:Tuple{Vector{Float64},Vector{Float64}}}, nodes::Vector{<:GP.Node},
                                  noises::Vector{Float64}, series_index::Vector{<:Integer}; all_long::Bool=false)
    P = length(nodes)
    (length(noises) == P && length(series_index) == P) || throw(ArgumentError("one noise and one series index per particle required"))
    pt_off = Int64[0]; ts = Float64[]; xs = Float64[]
    for (s, (t, x)) in enumerate(series)
        length(t) == length(x) || throw(ArgumentError("series $s: ts and xs must have equal lengths"))
        length(t) <= LONG_SERIES_MAX_N || throw(ArgumentError("series $s has $(length(t)) points, more than LONG_SERIES_MAX_N ($LONG_SERIES_MAX_N)"))
        append!(ts, t); append!(xs, x); push!(pt_off, length(ts))
    end
    isempty(ts) && (push!(ts, 0.0); push!(xs, 0.0))
    sidx = Int32[Int32(i - 1) for i in series_index]
    op_off, ops, prm_off, prm = encode_batch(nodes)
    out = Vector{Float64}(undef, P); info = Vector{Int32}(undef, P)
    flags = all_long ? LONG_SERIES_ALL : Int32(0)
    GC.@preserve pt_off ts xs sidx op_off ops prm_off prm noises out info check(eng, ccall((:agp_logpdf_long_series_batch, LIB), Cint,
        (Ptr{Cvoid}, Int32, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{UInt8}, Ptr{Int32}, Ptr{Float64},
         Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Int32}),
        eng.ptr, length(series), pt_off, ts, xs, P, sidx, op_off, ops, prm_off, prm, noises, flags, out, info))
    return out, info
end

"Value and gradient of many short series in one fused launch (agp_logpdf_grad_series_batch): `logpdf_series_batch`'s twin for
`Gen.choice_gradients` / `Gen.map_optimize` of callers that hold one model per short series.  Same arguments, same statelessness.
Returns `(logpdf, grads, grad_noise, info)`; `grads[p]` is d logpdf / d theta in the order of `encode(kernels[p])[2]`, as in
`logpdf_grad_batch`; `logpdf` is bit-identical to `logpdf_series_batch`'s."
function logpdf_grad_series_batch(eng::Engine, series::Vector{<:Tuple{Vector{Float64},Vector{Float64}}}, kernels::Vector{<:GP.Node},
                                  noises::Vector{Float64}, series_index::Vector{<:Integer})
    P = length(kernels)
    (length(noises) == P && length(series_index) == P) || throw(ArgumentError("one noise and one series index per particle required"))
    pt_off = Int64[0]; ts = Float64[]; xs = Float64[]
    for (s, (t, x)) in enumerate(series)
        length(t) == length(x) || throw(ArgumentError("series $s: ts and xs must have equal lengths"))
        length(t) <= SERIES_MAX_N || throw(ArgumentError("series $s has $(length(t)) points, more than SERIES_MAX_N ($SERIES_MAX_N)"))
        append!(ts, t); append!(xs, x); push!(pt_off, length(ts))
    end
    isempty(ts) && (push!(ts, 0.0); push!(xs, 0.0))
    sidx = Int32[Int32(i - 1) for i in series_index]
    op_off, ops, prm_off, prm = encode_batch(kernels)
    out = Vector{Float64}(undef, P); info = Vector{Int32}(undef, P); gn = Vector{Float64}(undef, P)
    grad = zeros(Float64, max(1, Int(prm_off[end])))
    GC.@preserve pt_off ts xs sidx op_off ops prm_off prm noises out grad gn info check(eng, ccall((:agp_logpdf_grad_series_batch, LIB), Cint,
        (Ptr{Cvoid}, Int32, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{UInt8}, Ptr{Int32}, Ptr{Float64},
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
        eng.ptr, length(series), pt_off, ts, xs, P, sidx, op_off, ops, prm_off, prm, noises, out, grad, gn, info))
    grads = [grad[prm_off[p] + 1:prm_off[p + 1]] for p in 1:P]
    return out, grads, gn, info
end

"Transform classes of `mcmc_parameters_series_batch`: 0 wildcard, 1 period, 2 gamma (GPConfig.prior's entries), -1 FIXED."
hmc_classes(n::GP.GammaExponential) = Int32[0, 2, 0]
hmc_classes(n::GP.Periodic) = Int32[0, 1, 0]
hmc_classes(n::GP.ChangePoint) = Int32[0, -1]              # the scale stays what it is (src/Model.jl:121)
hmc_classes(n::GP.BinaryOpNode) = Int32[]
hmc_classes(n::GP.Node) = zeros(Int32, length(params(n)))
"`tf[class]` = (mu, sigma, scale) from a `GP.GPConfig`'s prior; scale 0: log-normal."
hmc_transform_table(prior) = Float64[prior[:wildcard][:mu] prior[:wildcard][:sigma] 0.0;
                                     prior[:period][:mu] prior[:period][:sigma] 0.0;
                                     prior[:gamma][:mu] prior[:gamma][:sigma] prior[:gamma][:scale]]
hmc_untransform(v, c, tf) = c < 0 ? v : tf[c + 1, 3] == 0 ? (log(v) - tf[c + 1, 1]) / tf[c + 1, 2] :
                            (log(v / (tf[c + 1, 3] - v)) - tf[c + 1, 1]) / tf[c + 1, 2]

"`mcmc_parameters!` / `rejuvenate_particle_parameters` (src/inference_smc_anneal_data.jl:33-76) for MANY short series in one call
(agp_hmc_series_batch): `n_hmc` iterations of an HMC move on every particle's numeric kernel parameters and one on its noise, in the
latent space of `config.prior`, the whole chain of a particle in one workgroup.  `seeds[p]` keys particle `p`'s Philox stream (not
Julia's RNG).  `hmc_config`: the reference's keys `:L_param`, `:eps_param`, `:L_noise`, `:eps_noise`, `:n_exit`; `infer_noise = false`
skips the noise moves.  Returns `(kernels, noises, logpdf, counts, info)`: the moved trees and noises, their log marginal
likelihoods (bit-identical to `logpdf_series_batch` of the returned trees), `counts[:, p]` = parameter moves accepted, tried, noise
moves accepted, trajectories rejected as not positive definite."
function mcmc_parameters_series_batch(eng::Engine, series::Vector{<:Tuple{Vector{Float64},Vector{Float64}}}, kernels::Vector{<:GP.Node},
                                      noises::Vector{Float64}, series_index::Vector{<:Integer}, n_hmc::Integer, seeds::Vector{<:Integer};
                                      config = GP.GPConfig(), hmc_config = Dict(), infer_noise::Bool = true, jitter::Float64 = 1e-5)
    P = length(kernels)
    (length(noises) == P && length(series_index) == P && length(seeds) == P) ||
        throw(ArgumentError("one noise, one series index and one seed per particle required"))
    pt_off = Int64[0]; ts = Float64[]; xs = Float64[]
    for (s, (t, x)) in enumerate(series)
        length(t) == length(x) || throw(ArgumentError("series $s: ts and xs must have equal lengths"))
        length(t) <= SERIES_MAX_N || throw(ArgumentError("series $s has $(length(t)) points, more than SERIES_MAX_N ($SERIES_MAX_N)"))
        append!(ts, t); append!(xs, x); push!(pt_off, length(ts))
    end
    isempty(ts) && (push!(ts, 0.0); push!(xs, 0.0))
    sidx = Int32[Int32(i - 1) for i in series_index]
    op_off, ops, prm_off, prm = encode_batch(kernels)
    tf = hmc_transform_table(config.prior)
    tfr = collect(vec(permutedims(tf)))                    # row-major (class, 3)
    cls = Int32[]
    for k in kernels, nd in GP.unroll(k)
        append!(cls, hmc_classes(nd))
    end
    isempty(cls) && push!(cls, Int32(0))
    z = Float64[hmc_untransform(prm[i], cls[i], tf) for i in eachindex(cls)]
    zn = Float64[hmc_untransform(v - jitter, 0, tf) for v in noises]
    sd = UInt64[UInt64(s) for s in seeds]
    nt = max(1, Int(prm_off[end]))
    oz = zeros(Float64, nt); oprm = zeros(Float64, nt); ozn = Vector{Float64}(undef, P); onz = Vector{Float64}(undef, P)
    lp = Vector{Float64}(undef, P); counts = zeros(Int32, 4, P); info = Vector{Int32}(undef, P)
    GC.@preserve pt_off ts xs sidx op_off ops prm_off z zn cls tfr sd oz ozn oprm onz lp counts info check(eng, ccall((:agp_hmc_series_batch, LIB), Cint,
        (Ptr{Cvoid}, Int32, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{UInt8}, Ptr{Int32}, Ptr{Float64},
         Ptr{Float64}, Ptr{Int32}, Int32, Ptr{Float64}, Int32, Float64, Int32, Int32, Float64, Int32, Float64, Int32, Ptr{UInt64}, Int32,
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}),
        eng.ptr, length(series), pt_off, ts, xs, P, sidx, op_off, ops, prm_off, z, zn, cls, 3, tfr, 0, jitter, n_hmc,
        get(hmc_config, :L_param, 10), get(hmc_config, :eps_param, .02), infer_noise ? get(hmc_config, :L_noise, 10) : 0,
        get(hmc_config, :eps_noise, .02), get(hmc_config, :n_exit, n_hmc), sd, 0, oz, ozn, oprm, onz, lp, counts, info, C_NULL))
    moved = GP.Node[node_from_flat(ops[op_off[p] + 1:op_off[p + 1]], oprm[prm_off[p] + 1:prm_off[p + 1]]) for p in 1:P]
    return moved, onz, lp, counts, info
end

"Forecasts of many short series in one fused launch (agp_predict_series_batch): `logpdf_series_batch`'s predictive twin, same
series / particle arguments and statelessness.  `queries[s]` holds series `s`'s own query times; particle `p` predicts on
`series[series_index[p]]` (1-based): mean = K21 K11^-1 x, var = diag(K22 - K21 K11^-1 K12) + noise_pred[p] (`nothing`: the
particle's noise).  Returns `(means, vars, logpdf, info)`; `means[p]` / `vars[p]` have the length of the particle's series' query
vector and `logpdf` is bit-identical to `logpdf_series_batch`'s."
function predict_series_batch(eng::Engine, series::Vector{<:Tuple{Vector{Float64},Vector{Float64}}}, queries::Vector{Vector{Float64}},
                              nodes::Vector{<:GP.Node}, noises::Vector{Float64}, series_index::Vector{<:Integer};
                              noise_pred::Union{Nothing,Vector{Float64}}=nothing)
    P = length(nodes)
    (length(noises) == P && length(series_index) == P) || throw(ArgumentError("one noise and one series index per particle required"))
    length(queries) == length(series) || throw(ArgumentError("one vector of query times per series required"))
    (noise_pred === nothing || length(noise_pred) == P) || throw(ArgumentError("one noise_pred per particle required"))
    all(i -> 1 <= i <= length(series), series_index) || throw(ArgumentError("series index outside 1:$(length(series))"))
    pt_off = Int64[0]; ts = Float64[]; xs = Float64[]; q_off = Int64[0]; tq = Float64[]
    for (s, (t, x)) in enumerate(series)
        length(t) == length(x) || throw(ArgumentError("series $s: ts and xs must have equal lengths"))
        length(t) <= SERIES_MAX_N || throw(ArgumentError("series $s has $(length(t)) points, more than SERIES_MAX_N ($SERIES_MAX_N)"))
        append!(ts, t); append!(xs, x); push!(pt_off, length(ts))
        append!(tq, queries[s]); push!(q_off, length(tq))
    end
    isempty(ts) && (push!(ts, 0.0); push!(xs, 0.0))
    isempty(tq) && push!(tq, 0.0)
    sidx = Int32[Int32(i - 1) for i in series_index]
    op_off, ops, prm_off, prm = encode_batch(nodes)
    total = sum(Int[length(queries[i]) for i in series_index])
    mean = Vector{Float64}(undef, max(1, total)); var = Vector{Float64}(undef, max(1, total))
    out_off = zeros(Int64, P + 1)
    out = Vector{Float64}(undef, P); info = Vector{Int32}(undef, P)
    np = noise_pred === nothing ? noises : noise_pred
    GC.@preserve pt_off ts xs q_off tq sidx op_off ops prm_off prm noises np mean var out_off out info check(eng, ccall((:agp_predict_series_batch, LIB), Cint,
        (Ptr{Cvoid}, Int32, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{UInt8},
         Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int32}),
        eng.ptr, length(series), pt_off, ts, xs, q_off, tq, P, sidx, op_off, ops, prm_off, prm, noises, np, mean, var, out_off, out, info))
    means = [mean[out_off[p] + 1:out_off[p + 1]] for p in 1:P]
    vars = [var[out_off[p] + 1:out_off[p + 1]] for p in 1:P]
    return means, vars, out, info
end

"Forecast bands of many short series in one call (agp_predict_quantile_series_batch): `predict_series_batch`, then on the device the
quantiles `q` of every series' own mixture of its particles' raw-space predictives, and that mixture's marginal mean and variance.
`weights[p]` is particle `p`'s weight inside the mixture of `series[series_index[p]]` (each series' weights sum to 1);
`y_transforms[s] = (slope, intercept)` of series `s` (`nothing`: (1, 0)).  Returns `(x, converged, iters, mean, var, logpdf, info)`:
`x[s]` is `m_s x length(q)`, `converged[s]` / `iters[s]` likewise, `mean[s]` / `var[s]` have length `m_s`.  A series without particles,
or with a particle whose info != 0, gets NaN and nothing converged."
function predict_quantile_series_batch(eng::Engine, series::Vector{<:Tuple{Vector{Float64},Vector{Float64}}},
                                       queries::Vector{Vector{Float64}}, nodes::Vector{<:GP.Node}, noises::Vector{Float64},
                                       series_index::Vector{<:Integer}, weights::Vector{Float64}, q::Vector{Float64};
                                       y_transforms::Union{Nothing,Vector{Tuple{Float64,Float64}}}=nothing,
                                       noise_pred::Union{Nothing,Vector{Float64}}=nothing, tol::Float64=1e-5, max_iter::Integer=10^6)
    P = length(nodes); S = length(series)
    (length(noises) == P && length(series_index) == P && length(weights) == P) ||
        throw(ArgumentError("one noise, one series index and one weight per particle required"))
    length(queries) == S || throw(ArgumentError("one vector of query times per series required"))
    (noise_pred === nothing || length(noise_pred) == P) || throw(ArgumentError("one noise_pred per particle required"))
    (y_transforms === nothing || length(y_transforms) == S) || throw(ArgumentError("one (slope, intercept) per series required"))
    all(i -> 1 <= i <= S, series_index) || throw(ArgumentError("series index outside 1:$S"))
    pt_off = Int64[0]; ts = Float64[]; xs = Float64[]; q_off = Int64[0]; tq = Float64[]
    for (s, (t, x)) in enumerate(series)
        length(t) == length(x) || throw(ArgumentError("series $s: ts and xs must have equal lengths"))
        length(t) <= SERIES_MAX_N || throw(ArgumentError("series $s has $(length(t)) points, more than SERIES_MAX_N ($SERIES_MAX_N)"))
        append!(ts, t); append!(xs, x); push!(pt_off, length(ts))
        append!(tq, queries[s]); push!(q_off, length(tq))
    end
    isempty(ts) && (push!(ts, 0.0); push!(xs, 0.0))
    isempty(tq) && push!(tq, 0.0)
    sidx = Int32[Int32(i - 1) for i in series_index]
    op_off, ops, prm_off, prm = encode_batch(nodes)
    slope = y_transforms === nothing ? ones(Float64, max(1, S)) : Float64[t[1] for t in y_transforms]
    icpt = y_transforms === nothing ? zeros(Float64, max(1, S)) : Float64[t[2] for t in y_transforms]
    nq = length(q); Q = Int(q_off[end])
    x = Vector{Float64}(undef, max(1, nq * Q)); conv = zeros(Int32, max(1, nq * Q)); iters = zeros(Int32, max(1, nq * Q))
    mean = Vector{Float64}(undef, max(1, Q)); var = Vector{Float64}(undef, max(1, Q))
    out = Vector{Float64}(undef, max(1, P)); info = zeros(Int32, max(1, P))
    np = noise_pred === nothing ? noises : noise_pred
    GC.@preserve pt_off ts xs q_off tq sidx op_off ops prm_off prm noises np weights slope icpt q x conv iters mean var out info check(eng, ccall((:agp_predict_quantile_series_batch, LIB), Cint,
        (Ptr{Cvoid}, Int32, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{UInt8},
         Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Float64,
         Int64, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
        eng.ptr, S, pt_off, ts, xs, q_off, tq, P, sidx, op_off, ops, prm_off, prm, noises, np, weights, slope, icpt, q, nq, tol,
        max_iter, x, conv, iters, mean, var, out, info))
    # series s's block is (nq, m_s) row-major: column-major it is the m_s x nq matrix
    block(a, s) = reshape(a[nq * q_off[s] + 1:nq * q_off[s + 1]], Int(q_off[s + 1] - q_off[s]), nq)
    xs_ = [block(x, s) for s in 1:S]
    cs_ = [block(conv, s) .!= 0 for s in 1:S]
    is_ = [block(iters, s) for s in 1:S]
    means = [mean[q_off[s] + 1:q_off[s + 1]] for s in 1:S]
    vars = [var[q_off[s] + 1:q_off[s + 1]] for s in 1:S]
    return xs_, cs_, is_, means, vars, out[1:P], info[1:P]
end

"`predict_series_batch` for series of at most `LONG_SERIES_MAX_N` points (agp_predict_long_series_batch): same arguments, same
returns, same statelessness, one call for a mixed family such as 135, 143 and 442 points.  A series of at most `SERIES_MAX_N` points
runs in `predict_series_batch`'s kernel (bit-identical results), a longer one in the long-series predictive kernel, which keeps the
factor and the solved query blocks in an HBM workspace; `all_long = true` sends every non-empty series through the long kernel.
`logpdf` is bit-identical to `logpdf_long_series_batch`'s under the same `all_long`."
function predict_long_series_batch(eng::Engine, series::Vector{<:Tuple{Vector{Float64},Vector{Float64}}}, queries::Vector{Vector{Float64}},
                                   nodes::Vector{<:GP.Node}, noises::Vector{Float64}, series_index::Vector{<:Integer};
                                   noise_pred::Union{Nothing,Vector{Float64}}=nothing, all_long::Bool=false)
    P = length(nodes)
    (length(noises) == P && length(series_index) == P) || throw(ArgumentError("one noise and one series index per particle required"))
    length(queries) == length(series) || throw(ArgumentError("one vector of query times per series required"))
    (noise_pred === nothing || length(noise_pred) == P) || throw(ArgumentError("one noise_pred per particle required"))
    all(i -> 1 <= i <= length(series), series_index) || throw(ArgumentError("series index outside 1:$(length(series))"))
    pt_off = Int64[0]; ts = Float64[]; xs = Float64[]; q_off = Int64[0]; tq = Float64[]
    for (s, (t, x)) in enumerate(series)
        length(t) == length(x) || throw(ArgumentError("series $s: ts and xs must have equal lengths"))
        length(t) <= LONG_SERIES_MAX_N || throw(ArgumentError("series $s has $(length(t)) points, more than LONG_SERIES_MAX_N ($LONG_SERIES_MAX_N)"))
        append!(ts, t); append!(xs, x); push!(pt_off, length(ts))
        append!(tq, queries[s]); push!(q_off, length(tq))
    end
    isempty(ts) && (push!(ts, 0.0); push!(xs, 0.0))
    isempty(tq) && push!(tq, 0.0)
    sidx = Int32[Int32(i - 1) for i in series_index]
    op_off, ops, prm_off, prm = encode_batch(nodes)
    total = sum(Int[length(queries[i]) for i in series_index])
    mean = Vector{Float64}(undef, max(1, total)); var = Vector{Float64}(undef, max(1, total))
    out_off = zeros(Int64, P + 1)
    out = Vector{Float64}(undef, P); info = Vector{Int32}(undef, P)
    np = noise_pred === nothing ? noises : noise_pred
    flags = all_long ? UInt32(LONG_SERIES_ALL) : UInt32(0)
    GC.@preserve pt_off ts xs q_off tq sidx op_off ops prm_off prm noises np mean var out_off out info check(eng, ccall((:agp_predict_long_series_batch, LIB), Cint,
        (Ptr{Cvoid}, Int32, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{UInt8},
         Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int32}, UInt32),
        eng.ptr, length(series), pt_off, ts, xs, q_off, tq, P, sidx, op_off, ops, prm_off, prm, noises, np, mean, var, out_off, out, info, flags))
    means = [mean[out_off[p] + 1:out_off[p + 1]] for p in 1:P]
    vars = [var[out_off[p] + 1:out_off[p + 1]] for p in 1:P]
    return means, vars, out, info
end

"`predict_quantile_series_batch` for series of at most `LONG_SERIES_MAX_N` points (agp_predict_quantile_long_series_batch): same
arguments and returns; the predictive launches are `predict_long_series_batch`'s (routing, workspace, `all_long`), the read-out kernels
behind them are `predict_quantile_series_batch`'s, unchanged."
function predict_quantile_long_series_batch(eng::Engine, series::Vector{<:Tuple{Vector{Float64},Vector{Float64}}},
                                            queries::Vector{Vector{Float64}}, nodes::Vector{<:GP.Node}, noises::Vector{Float64},
                                            series_index::Vector{<:Integer}, weights::Vector{Float64}, q::Vector{Float64};
                                            y_transforms::Union{Nothing,Vector{Tuple{Float64,Float64}}}=nothing,
                                            noise_pred::Union{Nothing,Vector{Float64}}=nothing, tol::Float64=1e-5, max_iter::Integer=10^6,
                                            all_long::Bool=false)
    P = length(nodes); S = length(series)
    (length(noises) == P && length(series_index) == P && length(weights) == P) ||
        throw(ArgumentError("one noise, one series index and one weight per particle required"))
    length(queries) == S || throw(ArgumentError("one vector of query times per series required"))
    (noise_pred === nothing || length(noise_pred) == P) || throw(ArgumentError("one noise_pred per particle required"))
    (y_transforms === nothing || length(y_transforms) == S) || throw(ArgumentError("one (slope, intercept) per series required"))
    all(i -> 1 <= i <= S, series_index) || throw(ArgumentError("series index outside 1:$S"))
    pt_off = Int64[0]; ts = Float64[]; xs = Float64[]; q_off = Int64[0]; tq = Float64[]
    for (s, (t, x)) in enumerate(series)
        length(t) == length(x) || throw(ArgumentError("series $s: ts and xs must have equal lengths"))
        length(t) <= LONG_SERIES_MAX_N || throw(ArgumentError("series $s has $(length(t)) points, more than LONG_SERIES_MAX_N ($LONG_SERIES_MAX_N)"))
        append!(ts, t); append!(xs, x); push!(pt_off, length(ts))
        append!(tq, queries[s]); push!(q_off, length(tq))
    end
    isempty(ts) && (push!(ts, 0.0); push!(xs, 0.0))
    isempty(tq) && push!(tq, 0.0)
    sidx = Int32[Int32(i - 1) for i in series_index]
    op_off, ops, prm_off, prm = encode_batch(nodes)
    slope = y_transforms === nothing ? ones(Float64, max(1, S)) : Float64[t[1] for t in y_transforms]
    icpt = y_transforms === nothing ? zeros(Float64, max(1, S)) : Float64[t[2] for t in y_transforms]
    nq = length(q); Q = Int(q_off[end])
    x = Vector{Float64}(undef, max(1, nq * Q)); conv = zeros(Int32, max(1, nq * Q)); iters = zeros(Int32, max(1, nq * Q))
    mean = Vector{Float64}(undef, max(1, Q)); var = Vector{Float64}(undef, max(1, Q))
    out = Vector{Float64}(undef, max(1, P)); info = zeros(Int32, max(1, P))
    np = noise_pred === nothing ? noises : noise_pred
    flags = all_long ? UInt32(LONG_SERIES_ALL) : UInt32(0)
    GC.@preserve pt_off ts xs q_off tq sidx op_off ops prm_off prm noises np weights slope icpt q x conv iters mean var out info check(eng, ccall((:agp_predict_quantile_long_series_batch, LIB), Cint,
        (Ptr{Cvoid}, Int32, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{UInt8},
         Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Float64,
         Int64, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, UInt32),
        eng.ptr, S, pt_off, ts, xs, q_off, tq, P, sidx, op_off, ops, prm_off, prm, noises, np, weights, slope, icpt, q, nq, tol,
        max_iter, x, conv, iters, mean, var, out, info, flags))
    # series s's block is (nq, m_s) row-major: column-major it is the m_s x nq matrix
    block(a, s) = reshape(a[nq * q_off[s] + 1:nq * q_off[s + 1]], Int(q_off[s + 1] - q_off[s]), nq)
    xs_ = [block(x, s) for s in 1:S]
    cs_ = [block(conv, s) .!= 0 for s in 1:S]
    is_ = [block(iters, s) for s in 1:S]
    means = [mean[q_off[s] + 1:q_off[s + 1]] for s in 1:S]
    vars = [var[q_off[s] + 1:q_off[s + 1]] for s in 1:S]
    return xs_, cs_, is_, means, vars, out[1:P], info[1:P]
end

"Held-out scores of many short series in one fused launch (agp_predict_logpdf_series_batch): `predict_proba` for callers that hold
one model per short series, with `predict_series_batch`'s series / query / particle arguments and statelessness.  `heldout[s]` holds
the RAW values observed at `queries[s]`; particle `p` scores them under its posterior predictive on `series[series_index[p]]`
(1-based; training plus held-out points of a series at most `SERIES_MAX_N`).  `y_transforms[s] = (slope, intercept)` of series `s`
(scaled = slope * raw + intercept, the space the series' `xs` are in; `nothing`: (1, 0)): the values are scaled here and the density
of the raw values gains `m log|slope|`.  `weights[p]` (or `nothing`) is particle `p`'s weight inside ITS series' mixture.  Returns
`(logpdf, terms, series_logp, info)`: `terms[p][j]` is the log-density of held-out point `j` given the training data and the points
before it (they sum to `logpdf[p]`); `series_logp[s]` the log of the series' mixture density at its held-out vector (`nothing`
without weights; NaN for a series without particles or with a failed particle, 0 where nothing is held out)."
function predict_proba_series_batch(eng::Engine, series::Vector{<:Tuple{Vector{Float64},Vector{Float64}}},
                                    queries::Vector{Vector{Float64}}, heldout::Vector{Vector{Float64}}, nodes::Vector{<:GP.Node},
                                    noises::Vector{Float64}, series_index::Vector{<:Integer};
                                    weights::Union{Nothing,Vector{Float64}}=nothing,
                                    y_transforms::Union{Nothing,Vector{Tuple{Float64,Float64}}}=nothing,
                                    noise_pred::Union{Nothing,Vector{Float64}}=nothing)
    P = length(nodes); S = length(series)
    (length(noises) == P && length(series_index) == P) || throw(ArgumentError("one noise and one series index per particle required"))
    (weights === nothing || length(weights) == P) || throw(ArgumentError("one weight per particle required"))
    (length(queries) == S && length(heldout) == S) ||
        throw(ArgumentError("one vector of query times and one of held-out values per series required"))
    (noise_pred === nothing || length(noise_pred) == P) || throw(ArgumentError("one noise_pred per particle required"))
    (y_transforms === nothing || length(y_transforms) == S) || throw(ArgumentError("one (slope, intercept) per series required"))
    all(i -> 1 <= i <= S, series_index) || throw(ArgumentError("series index outside 1:$S"))
    pt_off = Int64[0]; ts = Float64[]; xs = Float64[]; q_off = Int64[0]; tq = Float64[]; yq = Float64[]
    for (s, (t, x)) in enumerate(series)
        length(t) == length(x) || throw(ArgumentError("series $s: ts and xs must have equal lengths"))
        length(t) <= SERIES_MAX_N || throw(ArgumentError("series $s has $(length(t)) points, more than SERIES_MAX_N ($SERIES_MAX_N)"))
        length(heldout[s]) == length(queries[s]) ||
            throw(ArgumentError("series $s: $(length(queries[s])) held-out values required, one per query time"))
        a, b = y_transforms === nothing ? (1.0, 0.0) : y_transforms[s]
        append!(ts, t); append!(xs, x); push!(pt_off, length(ts))
        append!(tq, queries[s]); push!(q_off, length(tq))
        append!(yq, y_transforms === nothing ? heldout[s] : a .* heldout[s] .+ b)
    end
    isempty(ts) && (push!(ts, 0.0); push!(xs, 0.0))
    isempty(tq) && (push!(tq, 0.0); push!(yq, 0.0))
    sidx = Int32[Int32(i - 1) for i in series_index]
    op_off, ops, prm_off, prm = encode_batch(nodes)
    slope = y_transforms === nothing ? ones(Float64, max(1, S)) : Float64[t[1] for t in y_transforms]
    total = sum(Int[length(queries[i]) for i in series_index])
    out = Vector{Float64}(undef, max(1, P)); info = zeros(Int32, max(1, P))
    terms = Vector{Float64}(undef, max(1, total)); out_off = zeros(Int64, P + 1)
    mix = Vector{Float64}(undef, max(1, S))
    np = noise_pred === nothing ? noises : noise_pred
    w = weights === nothing ? Float64[] : weights
    GC.@preserve pt_off ts xs q_off tq yq sidx op_off ops prm_off prm noises np slope w out terms out_off mix info check(eng, ccall((:agp_predict_logpdf_series_batch, LIB), Cint,
        (Ptr{Cvoid}, Int32, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Int32}, Ptr{Int32},
         Ptr{UInt8}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
         Ptr{Int64}, Ptr{Float64}, Ptr{Int32}),
        eng.ptr, S, pt_off, ts, xs, q_off, tq, yq, P, sidx, op_off, ops, prm_off, prm, noises, np, slope,
        weights === nothing ? Ptr{Float64}(C_NULL) : pointer(w), out, terms, out_off,
        weights === nothing ? Ptr{Float64}(C_NULL) : pointer(mix), info))
    cut = [terms[out_off[p] + 1:out_off[p + 1]] for p in 1:P]
    return out[1:P], cut, (weights === nothing ? nothing : mix[1:S]), info[1:P]
end

"`predict_proba_series_batch` for training plus held-out points of a series of at most `LONG_SERIES_MAX_N` together
(agp_predict_logpdf_long_series_batch): same arguments, same returns, same statelessness — the tutorial's split of 144 training and 36
held-out points, or a held-out tail of the 442-point data set, beside the short series in one call.  A series whose joint length is at
most `SERIES_MAX_N` runs in `predict_proba_series_batch`'s kernel (bit-identical results), a longer one in the long-series kernel on
the joint points, its factor in an HBM workspace; `all_long = true` sends every particle with held-out points through the long kernel."
function predict_proba_long_series_batch(eng::Engine, series::Vector{<:Tuple{Vector{Float64},Vector{Float64}}},
                                         queries::Vector{Vector{Float64}}, heldout::Vector{Vector{Float64}}, nodes::Vector{<:GP.Node},
                                         noises::Vector{Float64}, series_index::Vector{<:Integer};
                                         weights::Union{Nothing,Vector{Float64}}=nothing,
                                         y_transforms::Union{Nothing,Vector{Tuple{Float64,Float64}}}=nothing,
                                         noise_pred::Union{Nothing,Vector{Float64}}=nothing, all_long::Bool=false)
    P = length(nodes); S = length(series)
    (length(noises) == P && length(series_index) == P) || throw(ArgumentError("one noise and one series index per particle required"))
    (weights === nothing || length(weights) == P) || throw(ArgumentError("one weight per particle required"))
    (length(queries) == S && length(heldout) == S) ||
        throw(ArgumentError("one vector of query times and one of held-out values per series required"))
    (noise_pred === nothing || length(noise_pred) == P) || throw(ArgumentError("one noise_pred per particle required"))
    (y_transforms === nothing || length(y_transforms) == S) || throw(ArgumentError("one (slope, intercept) per series required"))
    all(i -> 1 <= i <= S, series_index) || throw(ArgumentError("series index outside 1:$S"))
    pt_off = Int64[0]; ts = Float64[]; xs = Float64[]; q_off = Int64[0]; tq = Float64[]; yq = Float64[]
    for (s, (t, x)) in enumerate(series)
        length(t) == length(x) || throw(ArgumentError("series $s: ts and xs must have equal lengths"))
        length(t) <= LONG_SERIES_MAX_N || throw(ArgumentError("series $s has $(length(t)) points, more than LONG_SERIES_MAX_N ($LONG_SERIES_MAX_N)"))
        length(heldout[s]) == length(queries[s]) ||
            throw(ArgumentError("series $s: $(length(queries[s])) held-out values required, one per query time"))
        (isempty(queries[s]) || length(t) + length(queries[s]) <= LONG_SERIES_MAX_N) ||
            throw(ArgumentError("series $s has $(length(t)) training and $(length(queries[s])) held-out points, together more than LONG_SERIES_MAX_N ($LONG_SERIES_MAX_N)"))
        a, b = y_transforms === nothing ? (1.0, 0.0) : y_transforms[s]
        append!(ts, t); append!(xs, x); push!(pt_off, length(ts))
        append!(tq, queries[s]); push!(q_off, length(tq))
        append!(yq, y_transforms === nothing ? heldout[s] : a .* heldout[s] .+ b)
    end
    isempty(ts) && (push!(ts, 0.0); push!(xs, 0.0))
    isempty(tq) && (push!(tq, 0.0); push!(yq, 0.0))
    sidx = Int32[Int32(i - 1) for i in series_index]
    op_off, ops, prm_off, prm = encode_batch(nodes)
    slope = y_transforms === nothing ? ones(Float64, max(1, S)) : Float64[t[1] for t in y_transforms]
    total = sum(Int[length(queries[i]) for i in series_index])
    out = Vector{Float64}(undef, max(1, P)); info = zeros(Int32, max(1, P))
    terms = Vector{Float64}(undef, max(1, total)); out_off = zeros(Int64, P + 1)
    mix = Vector{Float64}(undef, max(1, S))
    np = noise_pred === nothing ? noises : noise_pred
    w = weights === nothing ? Float64[] : weights
    flags = all_long ? UInt32(LONG_SERIES_ALL) : UInt32(0)
    GC.@preserve pt_off ts xs q_off tq yq sidx op_off ops prm_off prm noises np slope w out terms out_off mix info check(eng, ccall((:agp_predict_logpdf_long_series_batch, LIB), Cint,
        (Ptr{Cvoid}, Int32, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Int32}, Ptr{Int32},
         Ptr{UInt8}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
         Ptr{Int64}, Ptr{Float64}, Ptr{Int32}, UInt32),
        eng.ptr, S, pt_off, ts, xs, q_off, tq, yq, P, sidx, op_off, ops, prm_off, prm, noises, np, slope,
        weights === nothing ? Ptr{Float64}(C_NULL) : pointer(w), out, terms, out_off,
        weights === nothing ? Ptr{Float64}(C_NULL) : pointer(mix), info, flags))
    cut = [terms[out_off[p] + 1:out_off[p + 1]] for p in 1:P]
    return out[1:P], cut, (weights === nothing ? nothing : mix[1:S]), info[1:P]
end

"Sample paths of many short series in one fused launch (agp_predict_sample_series_batch): `rand(predict_mvn(model, ds), n_samples)`
for callers that hold one model per short series, with `predict_proba_series_batch`'s series / query / particle arguments and
statelessness.  `weights[p]` is particle `p`'s weight inside ITS series' mixture; series `s` draws its `n_samples` paths under
`seeds[s]` exactly as the resident entry does under that seed.  `y_transforms[s] = (slope, intercept)` (`nothing`: (1, 0)); every
output is in raw space.  With `want_moments` the components of every series' mixture come back too.  Returns
`(x, component, means, covs, info)`: `x[s]` an `m_s × n_samples` matrix, column `j` being sample `j`; `component[s][j]` the 1-based
particle of that sample; `means[p]` / `covs[p]` (`nothing` without `want_moments`) the raw-space mean vector and `m_s × m_s`
covariance of particle `p`'s predictive.  A series with a failed particle is NaN in `x`."
function predict_rand_series_batch(eng::Engine, series::Vector{<:Tuple{Vector{Float64},Vector{Float64}}},
                                   queries::Vector{Vector{Float64}}, nodes::Vector{<:GP.Node}, noises::Vector{Float64},
                                   series_index::Vector{<:Integer}, weights::Vector{Float64}, n_samples::Integer,
                                   seeds::Vector{UInt64};
                                   y_transforms::Union{Nothing,Vector{Tuple{Float64,Float64}}}=nothing,
                                   noise_pred::Union{Nothing,Vector{Float64}}=nothing, want_moments::Bool=false)
    P = length(nodes); S = length(series); R = Int64(n_samples)
    R >= 0 || throw(ArgumentError("n_samples must not be negative"))
    (length(noises) == P && length(series_index) == P && length(weights) == P) ||
        throw(ArgumentError("one noise, one series index and one weight per particle required"))
    (length(queries) == S && length(seeds) == S) || throw(ArgumentError("one vector of query times and one seed per series required"))
    (noise_pred === nothing || length(noise_pred) == P) || throw(ArgumentError("one noise_pred per particle required"))
    (y_transforms === nothing || length(y_transforms) == S) || throw(ArgumentError("one (slope, intercept) per series required"))
    all(i -> 1 <= i <= S, series_index) || throw(ArgumentError("series index outside 1:$S"))
    pt_off = Int64[0]; ts = Float64[]; xs = Float64[]; q_off = Int64[0]; tq = Float64[]
    for (s, (t, x)) in enumerate(series)
        length(t) == length(x) || throw(ArgumentError("series $s: ts and xs must have equal lengths"))
        length(t) <= SERIES_MAX_N || throw(ArgumentError("series $s has $(length(t)) points, more than SERIES_MAX_N ($SERIES_MAX_N)"))
        append!(ts, t); append!(xs, x); push!(pt_off, length(ts))
        append!(tq, queries[s]); push!(q_off, length(tq))
    end
    isempty(ts) && (push!(ts, 0.0); push!(xs, 0.0))
    isempty(tq) && push!(tq, 0.0)
    sidx = Int32[Int32(i - 1) for i in series_index]
    op_off, ops, prm_off, prm = encode_batch(nodes)
    slope = y_transforms === nothing ? ones(Float64, max(1, S)) : Float64[t[1] for t in y_transforms]
    icpt = y_transforms === nothing ? zeros(Float64, max(1, S)) : Float64[t[2] for t in y_transforms]
    ms = Int[length(queries[i]) for i in series_index]
    Q = q_off[end]
    x = Vector{Float64}(undef, max(1, R * Q)); comp = zeros(Int32, max(1, S * R)); info = zeros(Int32, max(1, P))
    mean = Vector{Float64}(undef, max(1, sum(ms))); cov = Vector{Float64}(undef, max(1, sum(ms .^ 2)))
    out_off = zeros(Int64, P + 1); cov_off = zeros(Int64, P + 1)
    np = noise_pred === nothing ? noises : noise_pred
    sd = isempty(seeds) ? UInt64[0] : seeds
    GC.@preserve pt_off ts xs q_off tq sidx op_off ops prm_off prm noises np slope icpt weights sd x comp mean out_off cov cov_off info check(eng, ccall((:agp_predict_sample_series_batch, LIB), Cint,
        (Ptr{Cvoid}, Int32, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Int32, Ptr{Int32}, Ptr{Int32},
         Ptr{UInt8}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{UInt64},
         Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}, Ptr{Int32}),
        eng.ptr, S, pt_off, ts, xs, q_off, tq, P, sidx, op_off, ops, prm_off, prm, noises, np, slope, icpt, weights, R, sd,
        Ptr{Int32}(C_NULL), Ptr{Float64}(C_NULL), x, comp,
        want_moments ? pointer(mean) : Ptr{Float64}(C_NULL), out_off, want_moments ? pointer(cov) : Ptr{Float64}(C_NULL), cov_off, info))
    xs_ = [reshape(x[R * q_off[s] + 1:R * q_off[s + 1]], q_off[s + 1] - q_off[s], R) for s in 1:S]
    cs_ = [Int.(comp[(s - 1) * R + 1:s * R]) .+ 1 for s in 1:S]
    means = want_moments ? [mean[out_off[p] + 1:out_off[p + 1]] for p in 1:P] : nothing
    covs = want_moments ? [reshape(cov[cov_off[p] + 1:cov_off[p + 1]], ms[p], ms[p]) for p in 1:P] : nothing
    return xs_, cs_, means, covs, info[1:P]
end

"The components of `predict_mvn`'s MixtureModel for many short series in one fused launch: `(means, covs, info)` of
`predict_rand_series_batch` with no sample drawn — per particle the raw-space mean vector and `m_s × m_s` covariance of its posterior
predictive on its own series; with the weights they are every series' `MixtureModel(MvNormal.(means, covs), weights)`."
function predict_mvn_series_batch(eng::Engine, series::Vector{<:Tuple{Vector{Float64},Vector{Float64}}},
                                  queries::Vector{Vector{Float64}}, nodes::Vector{<:GP.Node}, noises::Vector{Float64},
                                  series_index::Vector{<:Integer}, weights::Vector{Float64};
                                  y_transforms::Union{Nothing,Vector{Tuple{Float64,Float64}}}=nothing,
                                  noise_pred::Union{Nothing,Vector{Float64}}=nothing)
    _, _, means, covs, info = predict_rand_series_batch(eng, series, queries, nodes, noises, series_index, weights, 0,
                                                        zeros(UInt64, length(series)); y_transforms=y_transforms,
                                                        noise_pred=noise_pred, want_moments=true)
    return means, covs, info
end

"(extended, from_scratch, tile_rows_reused, tile_rows_total, evicted_before_reuse, slots, callers, occupied, capacity_tile_rows, growth_copies) of the factor store"
function extend_stats(eng::Engine)
    out = zeros(Int64, 10)
    GC.@preserve out check(eng, ccall((:agp_extend_stats2, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Int32), eng.ptr, out, 10))
    return (extended = out[1], from_scratch = out[2], tile_rows_reused = out[3], tile_rows_total = out[4],
            evicted_before_reuse = out[5], slots = out[6], callers = out[7], occupied = out[8],
            capacity_tile_rows = out[9], growth_copies = out[10])
end

"(particles a predictive call served from a resident factor, particles whose K11 it factored itself): after
`logpdf_batch(...; extend=true)` on a prefix, `predict_marginal` / `predict_mvn` on the same prefix reuse L11 and alpha."
function predict_reuse_stats(eng::Engine)
    out = Vector{Int64}(undef, 2)
    GC.@preserve out check(eng, ccall((:agp_predict_reuse_stats, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}), eng.ptr, out))
    return (reused = out[1], factored = out[2])
end

"(particles of gradient sweeps served from a resident factor, particles the gradient sweep factored itself): every
leapfrog step of `Gen.hmc` is `update` (-> agp_logpdf) followed by `choice_gradients` (-> agp_logpdf_grad) at the same
parameters; the value call leaves its factor in the engine's store and the gradient call starts from it."
function grad_reuse_stats(eng::Engine)
    out = Vector{Int64}(undef, 2)
    GC.@preserve out check(eng, ccall((:agp_grad_reuse_stats, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}), eng.ptr, out))
    return (reused = out[1], factored = out[2])
end

"Whether the single-particle value calls keep their factors resident (default: on)."
set_factor_cache!(eng::Engine, on::Bool) =
    check(eng, ccall((:agp_set_factor_cache, LIB), Cint, (Ptr{Cvoid}, Int32), eng.ptr, on ? 1 : 0))

"Pre-size the factor store for `n_particles` particles of series of up to `n_cap` points (twice the population: a particle
mid-rejuvenation keeps its previous state).  Call once per fit, after `set_data!`: the single-particle entries are coalesced into
batches of whatever size the threads' arrival times give, and a store sized for those batches alone would evict a large
population's factors between Gen.hmc's `update` and `choice_gradients` (src/inference_smc_anneal_data.jl:63-67)."
reserve_store!(eng::Engine, n_cap::Integer, n_particles::Integer) =
    check(eng, ccall((:agp_extend_reserve, LIB), Cint, (Ptr{Cvoid}, Int64, Int32), eng.ptr, n_cap, 2 * n_particles))

"Opt-in structured arithmetic on regular time grids (`agp_set_lag_tables` level 2): particles whose kernel is a sum of stationary
subtrees and Linear leaves are scored by the Schur recursion and differentiated by the structured sweep — also through the
single-particle entries that Gen drives — instead of the dense Cholesky; the others keep the dense path and the factor store."
function set_structured_sweeps!(eng::Engine, on::Bool)
    # off = back to the level that was in force before (AGP_LAG=0 / set_lag_tables!(eng, 0) stay off), never a forced 1
    if on
        eng.lag_level < 2 && (eng.lag_level_before = eng.lag_level)
        return set_lag_tables!(eng, 2)
    end
    return eng.lag_level >= 2 ? set_lag_tables!(eng, eng.lag_level_before) : nothing
end

"The whole population over every GPU of the pool: shards by agp_shard_range, one sweep per device, log-weights
all-gathered over RCCL inside the library (agp_logpdf_batch_multi)."
function logpdf_batch(pool::EnginePool, nodes::Vector{<:GP.Node}, noises::Vector{Float64}, n::Integer=pool.engines[1].n_max; extend::Bool=false)
    P = length(nodes)
    op_off, ops, prm_off, prm = encode_batch(nodes)
    out = Vector{Float64}(undef, P); info = Vector{Int32}(undef, P)
    ptrs = [e.ptr for e in pool.engines]
    # extend = true: every device keeps the factors of its shard resident (agp_logpdf_batch_extend_multi)
    GC.@preserve ptrs op_off ops prm_off prm noises out info begin
        rc = extend ?
            ccall((:agp_logpdf_batch_extend_multi, LIB), Cint,
                (Ptr{Ptr{Cvoid}}, Int32, Int64, Int32, Ptr{Int32}, Ptr{UInt8}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                ptrs, length(ptrs), n, P, op_off, ops, prm_off, prm, noises, out, info) :
            ccall((:agp_logpdf_batch_multi, LIB), Cint,
                (Ptr{Ptr{Cvoid}}, Int32, Int64, Int32, Ptr{Int32}, Ptr{UInt8}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
                ptrs, length(ptrs), n, P, op_off, ops, prm_off, prm, noises, out, info)
        check(pool.engines[1], rc)
    end
    return out, info
end

"""
Value + gradient of the whole population over every engine of the pool (`agp_logpdf_grad_batch_multi`): what the HMC rejuvenation
threads over the particles (src/inference_smc_anneal_data.jl:240-252), split by the cost-aware plan inside the library and returned
in the caller's order: (logpdf, grads in `flat_params` order per particle, d/dnoise, info, owner).
"""
function logpdf_grad_batch(pool::EnginePool, nodes::Vector{<:GP.Node}, noises::Vector{Float64}, n::Integer=pool.engines[1].n_max)
    P = length(nodes)
    op_off, ops, prm_off, prm = encode_batch(nodes)
    out = Vector{Float64}(undef, P); gn = Vector{Float64}(undef, P); info = Vector{Int32}(undef, P); owner = Vector{Int32}(undef, max(P, 1))
    grad = zeros(max(Int(prm_off[end]), 1))
    ptrs = [e.ptr for e in pool.engines]
    GC.@preserve ptrs op_off ops prm_off prm noises out grad gn info owner begin
        rc = ccall((:agp_logpdf_grad_batch_multi, LIB), Cint,
            (Ptr{Ptr{Cvoid}}, Int32, Int64, Int32, Ptr{Int32}, Ptr{UInt8}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}),
            ptrs, length(ptrs), n, P, op_off, ops, prm_off, prm, noises, out, grad, gn, info, owner)
        check(pool.engines[1], rc)
    end
    grads = [grad[(prm_off[i] + 1):prm_off[i + 1]] for i in 1:P]
    return out, grads, gn, info, owner[1:P]
end

"""
Marginal predictive means / variances of the whole population over every engine of the pool (`agp_predict_batch_multi`; what
`predict` threads over the particles, src/api.jl:508,645): m x P matrices in the caller's particle order, and info.
"""
function predict_marginal_batch(pool::EnginePool, nodes::Vector{<:GP.Node}, noises::Vector{Float64}, ts_pred::Vector{Float64},
                                n::Integer=pool.engines[1].n_max; noise_pred::Union{Nothing,Vector{Float64}}=nothing)
    P = length(nodes); m = length(ts_pred)
    op_off, ops, prm_off, prm = encode_batch(nodes)
    mean = Matrix{Float64}(undef, m, P); var = Matrix{Float64}(undef, m, P); info = zeros(Int32, P)
    ptrs = [e.ptr for e in pool.engines]
    npred = isnothing(noise_pred) ? Float64[] : noise_pred
    GC.@preserve ptrs ts_pred op_off ops prm_off prm noises npred mean var info begin
        rc = ccall((:agp_predict_batch_multi, LIB), Cint,
            (Ptr{Ptr{Cvoid}}, Int32, Int64, Ptr{Float64}, Int64, Int32, Ptr{Int32}, Ptr{UInt8}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
             Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}),
            ptrs, length(ptrs), n, ts_pred, m, P, op_off, ops, prm_off, prm, noises, isnothing(noise_pred) ? C_NULL : pointer(npred),
            C_NULL, C_NULL, mean, var, C_NULL, info, C_NULL)
        check(pool.engines[1], rc)
    end
    return mean, var, info
end

# ------------------------------------------------------------------------------------------------------------------
# gradient path
# ------------------------------------------------------------------------------------------------------------------
"""
Value and gradient in one call: (logpdf, d/dθ in `flat_params(node)` order — transformed parameters, ChangePoint
contributes location and scale — and d/dnoise).  Single-particle entry: callers on different Julia threads are
coalesced into batched gradient sweeps inside the library.
"""
function logpdf_grad_program(eng::Engine, ops::Vector{UInt8}, prm::Vector{Float64}, noise::Float64, n::Integer)
    np_ = length(prm)
    q = isempty(prm) ? [0.0] : prm
    lp = Ref{Float64}(0.0); gn = Ref{Float64}(0.0); info = Ref{Int32}(0); grad = zeros(max(np_, 1))
    GC.@preserve ops q grad check(eng, ccall((:agp_logpdf_grad, LIB), Cint,
        (Ptr{Cvoid}, Int64, Ptr{UInt8}, Int32, Ptr{Float64}, Int32, Float64, Ref{Float64}, Ptr{Float64}, Ref{Float64}, Ref{Int32}),
        eng.ptr, n, ops, length(ops), q, np_, noise, lp, grad, gn, info))
    info[] > 0 && throw(LinearAlgebra.PosDefException(info[]))
    return lp[], grad[1:np_], gn[]
end
logpdf_grad(eng::Engine, node::GP.Node, noise::Float64, n::Integer=eng.n_max) = logpdf_grad_program(eng, encode(node)..., noise, n)

# ------------------------------------------------------------------------------------------------------------------
# predictive path
# ------------------------------------------------------------------------------------------------------------------
"Posterior predictive — replaces Distributions.MvNormal(node, noise, ts, xs, ts_pred; ...) (src/GP.jl:731-758)."
function predict_mvn(eng::Engine, node::GP.Node, noise::Float64, ts_pred::Vector{Float64};
        n::Integer=eng.n_max, noise_pred::Union{Nothing,Float64}=nothing,
        mean_train::Union{Nothing,Vector{Float64}}=nothing, mean_pred::Union{Nothing,Vector{Float64}}=nothing)
    ops, prm = encode(node); isempty(prm) && push!(prm, 0.0)
    m = length(ts_pred)
    op_off = Int32[0, length(ops)]; prm_off = Int32[0, length(prm)]
    mu = Vector{Float64}(undef, m); var = Vector{Float64}(undef, m); cov = Matrix{Float64}(undef, m, m)
    info = Int32[0]; nz = [noise]
    # every optional array is bound to a local that is listed in GC.@preserve; C_NULL stands for "absent"
    npv = isnothing(noise_pred) ? Float64[] : [noise_pred]
    mt = isnothing(mean_train) ? Float64[] : mean_train
    mp = isnothing(mean_pred) ? Float64[] : mean_pred
    GC.@preserve ops prm op_off prm_off ts_pred mu var cov nz npv mt mp info check(eng, ccall((:agp_predict_batch, LIB), Cint,
        (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64, Int32, Ptr{Int32}, Ptr{UInt8}, Ptr{Int32}, Ptr{Float64},
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
        eng.ptr, n, ts_pred, m, 1, op_off, ops, prm_off, prm, nz,
        isempty(npv) ? Ptr{Float64}(C_NULL) : pointer(npv),
        isempty(mt) ? Ptr{Float64}(C_NULL) : pointer(mt),
        isempty(mp) ? Ptr{Float64}(C_NULL) : pointer(mp),
        mu, var, cov, info))
    info[1] > 0 && throw(LinearAlgebra.PosDefException(info[1]))
    return Distributions.MvNormal(mu, LinearAlgebra.Symmetric(cov))
end

"""
Marginal predictive mean and variance only — what `Inference.predict` (src/inference_utils.jl:186-196) consumes through
`Distributions.quantile(dist, p)` = mu + sqrt(diag(cov)) * Phi^-1(p) (src/GP.jl:1006-1012).  Passing no covariance buffer
lets the engine skip the n m^2 update of the prediction block's off-diagonal tiles.  Returns (mean, var).
"""
function predict_marginal(eng::Engine, node::GP.Node, noise::Float64, ts_pred::Vector{Float64};
        n::Integer=eng.n_max, noise_pred::Union{Nothing,Float64}=nothing)
    ops, prm = encode(node)
    m = length(ts_pred)
    op_off = Int32[0, length(ops)]; prm_off = Int32[0, length(prm)]
    mu = Vector{Float64}(undef, m); var = Vector{Float64}(undef, m)
    info = Int32[0]; nz = [noise]
    npv = isnothing(noise_pred) ? Float64[] : [noise_pred]
    GC.@preserve ops prm op_off prm_off ts_pred mu var nz npv info check(eng, ccall((:agp_predict_batch, LIB), Cint,
        (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64, Int32, Ptr{Int32}, Ptr{UInt8}, Ptr{Int32}, Ptr{Float64},
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
        eng.ptr, n, ts_pred, m, 1, op_off, ops, prm_off, prm, nz,
        isempty(npv) ? Ptr{Float64}(C_NULL) : pointer(npv), Ptr{Float64}(C_NULL), Ptr{Float64}(C_NULL),
        mu, var, Ptr{Float64}(C_NULL), info))
    info[1] > 0 && throw(LinearAlgebra.PosDefException(info[1]))
    return mu, var
end

"""
Predictive log-density of held-out values for a population — `Distributions.logpdf.(components, [y])` of `predict_proba`
(src/api.jl:686-699) and the held-out likelihood of test/experiment_hmc.jl:125, on the (scaled) resident series.  The covariance
is never formed: the joint matrix is factored once per particle.  Returns (logp, info); logp[i] is NaN where info[i] != 0
(info in 1..n: K11 is not positive definite; n + k: leading minor k of the predictive covariance is not).
"""
function predict_logpdf_batch(eng::Engine, nodes::Vector{<:GP.Node}, noises::Vector{Float64}, ts_pred::Vector{Float64},
        y::Vector{Float64}; n::Integer=eng.n_max, noise_pred::Union{Nothing,Vector{Float64}}=nothing,
        mean_train::Union{Nothing,Vector{Float64}}=nothing, mean_pred::Union{Nothing,Vector{Float64}}=nothing)
    P = length(nodes); m = length(ts_pred)
    length(y) == m || throw(DimensionMismatch("y has $(length(y)) values, ts_pred $(m)"))
    op_off, ops, prm_off, prm = encode_batch(nodes)
    logp = Vector{Float64}(undef, P); info = zeros(Int32, P)
    npv = isnothing(noise_pred) ? Float64[] : noise_pred
    mt = isnothing(mean_train) ? Float64[] : mean_train
    mp = isnothing(mean_pred) ? Float64[] : mean_pred
    GC.@preserve ops prm op_off prm_off ts_pred y noises npv mt mp logp info check(eng, ccall((:agp_predict_logpdf_batch, LIB), Cint,
        (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Int32, Ptr{Int32}, Ptr{UInt8}, Ptr{Int32}, Ptr{Float64},
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
        eng.ptr, n, ts_pred, y, m, P, op_off, ops, prm_off, prm, noises,
        isempty(npv) ? Ptr{Float64}(C_NULL) : pointer(npv),
        isempty(mt) ? Ptr{Float64}(C_NULL) : pointer(mt),
        isempty(mp) ? Ptr{Float64}(C_NULL) : pointer(mp),
        logp, info))
    return logp, info
end

"""
`Distributions.logpdf(MvNormal(node, noise, ts, xs, ts_pred; noise_pred, mean), y)` (test/experiment_hmc.jl:125) for one particle
on the resident series; throws `PosDefException` like the reference's factorisation.
"""
function predict_logpdf(eng::Engine, node::GP.Node, noise::Float64, ts_pred::Vector{Float64}, y::Vector{Float64};
        n::Integer=eng.n_max, noise_pred::Union{Nothing,Float64}=nothing,
        mean_train::Union{Nothing,Vector{Float64}}=nothing, mean_pred::Union{Nothing,Vector{Float64}}=nothing)
    logp, info = predict_logpdf_batch(eng, [node], [noise], ts_pred, y; n=n,
        noise_pred=isnothing(noise_pred) ? nothing : [noise_pred], mean_train=mean_train, mean_pred=mean_pred)
    info[1] != 0 && throw(LinearAlgebra.PosDefException(info[1]))
    return logp[1]
end

"""
Quantiles of a Gaussian mixture per point — `Statistics.quantile(::MixtureModel, q; tol, max_iter)` (src/api.jl:559-596) on the
mixtures of `Normal(means[i, p], sqrt(vars[i, p]))` with `weights[p]` (means / vars m×P).  Returns (x, converged, iters), each m×nq;
the reference's `success` is `all(converged)`.
"""
function mixture_quantile(eng::Engine, means::Matrix{Float64}, vars::Matrix{Float64}, weights::Vector{Float64}, q::Vector{Float64};
        tol::Real=1e-5, max_iter::Integer=10^6)
    m, P = size(means)
    size(vars) == (m, P) && length(weights) == P || throw(DimensionMismatch("means $(size(means)), vars $(size(vars)), weights $(length(weights))"))
    nq = length(q)
    x = Matrix{Float64}(undef, m, nq); conv = zeros(Int32, m, nq); iters = zeros(Int32, m, nq)
    GC.@preserve means vars weights q x conv iters check(eng, ccall((:agp_mixture_quantile, LIB), Cint,
        (Ptr{Cvoid}, Int64, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Float64, Int64, Ptr{Float64},
         Ptr{Int32}, Ptr{Int32}),
        eng.ptr, m, P, means, vars, weights, q, nq, Float64(tol), Int64(max_iter), x, conv, iters))
    return x, conv .!= 0, iters
end

"""
`AutoGP.predict_quantile(model, ds, q; noise_pred, tol, max_iter)` (src/api.jl:547-557) for a population on the (scaled) resident
series: the marginal predictive of every particle mapped to the raw space of the linear `y_transform` (slope, intercept), the
mixture with `weights` (`AutoGP.particle_weights(model)`), searched per point on the device.  Returns (x, success) like the
reference; throws `PosDefException` where a particle has no predictive.
"""
function predict_quantile(eng::Engine, nodes::Vector{<:GP.Node}, noises::Vector{Float64}, weights::Vector{Float64},
        ts_pred::Vector{Float64}, q::Real; n::Integer=eng.n_max, noise_pred::Union{Nothing,Float64}=nothing,
        y_slope::Float64=1.0, y_intercept::Float64=0.0, tol::Real=1e-5, max_iter::Integer=10^6)
    (0 < q < 1) || error("Quantile must be in (0,1).")
    P = length(nodes); m = length(ts_pred)
    op_off, ops, prm_off, prm = encode_batch(nodes)
    qv = [Float64(q)]
    x = Vector{Float64}(undef, m); conv = zeros(Int32, m); iters = zeros(Int32, m); info = zeros(Int32, P)
    npv = isnothing(noise_pred) ? Float64[] : fill(noise_pred, P)
    GC.@preserve ops prm op_off prm_off ts_pred noises npv weights qv x conv iters info check(eng, ccall((:agp_predict_quantile_batch, LIB), Cint,
        (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64, Int32, Ptr{Int32}, Ptr{UInt8}, Ptr{Int32}, Ptr{Float64},
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Float64, Float64, Ptr{Float64}, Int64, Float64, Int64,
         Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}),
        eng.ptr, n, ts_pred, m, P, op_off, ops, prm_off, prm, noises,
        isempty(npv) ? Ptr{Float64}(C_NULL) : pointer(npv), Ptr{Float64}(C_NULL), Ptr{Float64}(C_NULL),
        weights, y_slope, y_intercept, qv, 1, Float64(tol), Int64(max_iter), x, conv, iters, info))
    k = findfirst(!=(0), info)
    isnothing(k) || throw(LinearAlgebra.PosDefException(info[k]))
    return x, all(!=(0), conv)
end

"""
`rand(AutoGP.predict_mvn(model, ds; noise_pred), N)` (src/api.jl:497-522 + Distributions' `rand`) for a population on the (scaled)
resident series: `N` samples of the mixture, with `weights` (`AutoGP.particle_weights(model)`), of every particle's predictive at
`ts_pred`, in the raw space of the linear `y_transform` (slope, intercept).  Returns an m×N matrix (a vector of length m for
`N = nothing`).  The draws come from a counter-based stream of `seed`, not from Julia's RNG: the distribution is the contract.
Throws `PosDefException` where a particle has no predictive.
"""
function predict_rand(eng::Engine, nodes::Vector{<:GP.Node}, noises::Vector{Float64}, weights::Vector{Float64},
        ts_pred::Vector{Float64}, N::Union{Nothing,Integer}=nothing; seed::Integer=0, n::Integer=eng.n_max,
        noise_pred::Union{Nothing,Float64}=nothing, y_slope::Float64=1.0, y_intercept::Float64=0.0)
    P = length(nodes); m = length(ts_pred); S = isnothing(N) ? 1 : Int(N)
    op_off, ops, prm_off, prm = encode_batch(nodes)
    x = Matrix{Float64}(undef, m, S); info = zeros(Int32, P)
    npv = isnothing(noise_pred) ? Float64[] : fill(noise_pred, P)
    GC.@preserve ops prm op_off prm_off ts_pred noises npv weights x info check(eng, ccall((:agp_predict_sample_batch, LIB), Cint,
        (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64, Int32, Ptr{Int32}, Ptr{UInt8}, Ptr{Int32}, Ptr{Float64},
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Float64, Float64, Int64, UInt64, Ptr{Int32},
         Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}),
        eng.ptr, n, ts_pred, m, P, op_off, ops, prm_off, prm, noises,
        isempty(npv) ? Ptr{Float64}(C_NULL) : pointer(npv), Ptr{Float64}(C_NULL), Ptr{Float64}(C_NULL),
        weights, y_slope, y_intercept, S, UInt64(seed), Ptr{Int32}(C_NULL), Ptr{Float64}(C_NULL), x, Ptr{Int32}(C_NULL), info))
    k = findfirst(!=(0), info)
    isnothing(k) || throw(LinearAlgebra.PosDefException(info[k]))
    return isnothing(N) ? x[:, 1] : x
end

"""
`Distributions.mean`, `var` and `cov` of `AutoGP.predict_mvn(model, ds; noise_pred)` (src/api.jl:497-522) for a population on the
(scaled) resident series: the moments of the mixture, with `weights` (`AutoGP.particle_weights(model)`), of every particle's
predictive at `ts_pred` in the raw space of the linear `y_transform` (slope, intercept), reduced over the particles on the device.
`lognormal=true`: of `MixtureModel(MvLogNormal.(components), weights)`, the direct-space view of a model fitted on `log.(y)`.
`want_cov=false` runs the marginal pass (`cov` is `nothing`).  Returns `(mean, var, cov)`; throws `PosDefException` where a particle
has no predictive.
"""
function predict_mvn_moments(eng::Engine, nodes::Vector{<:GP.Node}, noises::Vector{Float64}, weights::Vector{Float64},
        ts_pred::Vector{Float64}; n::Integer=eng.n_max, noise_pred::Union{Nothing,Float64}=nothing,
        y_slope::Float64=1.0, y_intercept::Float64=0.0, lognormal::Bool=false, want_cov::Bool=true)
    P = length(nodes); m = length(ts_pred)
    op_off, ops, prm_off, prm = encode_batch(nodes)
    mean = Vector{Float64}(undef, m); var = Vector{Float64}(undef, m); info = zeros(Int32, P)
    cov = want_cov ? Matrix{Float64}(undef, m, m) : Matrix{Float64}(undef, 0, 0)
    npv = isnothing(noise_pred) ? Float64[] : fill(noise_pred, P)
    GC.@preserve ops prm op_off prm_off ts_pred noises npv weights mean var cov info check(eng, ccall((:agp_predict_mixture_batch, LIB), Cint,
        (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64, Int32, Ptr{Int32}, Ptr{UInt8}, Ptr{Int32}, Ptr{Float64},
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Float64, Float64, Int32,
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
        eng.ptr, n, ts_pred, m, P, op_off, ops, prm_off, prm, noises,
        isempty(npv) ? Ptr{Float64}(C_NULL) : pointer(npv), Ptr{Float64}(C_NULL), Ptr{Float64}(C_NULL),
        weights, y_slope, y_intercept, Int32(lognormal ? 1 : 0), mean, var,
        want_cov ? pointer(cov) : Ptr{Float64}(C_NULL), info))
    k = findfirst(!=(0), info)
    isnothing(k) || throw(LinearAlgebra.PosDefException(info[k]))
    return mean, var, (want_cov ? cov : nothing)
end

"Sum-of-GPs posterior — replaces GP.infer_gp_sum (src/GP.jl:904-993); returns the same named tuple."
function infer_gp_sum(eng::Engine, nodes::Vector{<:GP.Node}, noise::Float64, ts_pred::Vector{Float64};
        n::Integer=eng.n_max, noise_pred::Union{Nothing,Float64}=nothing)
    M = length(nodes); p = length(ts_pred); ma = (M + 1) * p
    op_off, ops, prm_off, prm = encode_batch(nodes)
    mu = Vector{Float64}(undef, ma); cov = Matrix{Float64}(undef, ma, ma); info = Ref{Int32}(0)
    GC.@preserve op_off ops prm_off prm ts_pred mu cov check(eng, ccall((:agp_infer_gp_sum, LIB), Cint,
        (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64, Int32, Ptr{Int32}, Ptr{UInt8}, Ptr{Int32}, Ptr{Float64},
         Float64, Float64, Ptr{Float64}, Ptr{Float64}, Ref{Int32}),
        eng.ptr, n, ts_pred, p, M, op_off, ops, prm_off, prm, noise, isnothing(noise_pred) ? noise : noise_pred,
        mu, cov, info))
    info[] > 0 && throw(LinearAlgebra.PosDefException(info[]))
    mvn = Distributions.MvNormal(mu, LinearAlgebra.Symmetric(cov))
    return (mvn=mvn, indexes=(F=[((i-1)*p+1):(i*p) for i in 1:M], X=(M*p+1):(M*p+p)))
end

"CSR programs of P particles x M components (`splits[k]`: the component kernels of particle k, e.g. `GP.split_kernel_sop(node, T)`)."
function encode_splits(splits::AbstractVector)
    P = length(splits); M = P == 0 ? 0 : length(splits[1])
    all(s -> length(s) == M, splits) || error("every particle must have the same number of components")
    nodes = GP.Node[nd for s in splits for nd in s]
    return (P, M, encode_batch(nodes)...)
end

"""
`GP.infer_gp_sum` for every particle of a population in one call (`AutoGP.predict_mvn_sum`, src/api.jl:978-1034, calls it once per
particle): `splits[k]` holds particle k's component kernels, made with AutoGP's own `GP.split_kernel_sop`.  `noise_pred` nothing =
each particle's own noise.  Returns (mean, var, cov, info, indexes): mean / var of size ((M+1)p, P), cov of size ((M+1)p, (M+1)p,
P) when `want_cov`, else nothing; throws `PosDefException` where a particle's training block is not positive definite.
"""
function infer_gp_sum_batch(eng::Engine, splits::AbstractVector, noises::Vector{Float64}, ts_pred::Vector{Float64};
        n::Integer=eng.n_max, noise_pred::Union{Nothing,Float64}=nothing, want_cov::Bool=false)
    P, M, op_off, ops, prm_off, prm = encode_splits(splits)
    p = length(ts_pred); ma = (M + 1) * p
    mu = Matrix{Float64}(undef, ma, P); var = Matrix{Float64}(undef, ma, P); info = zeros(Int32, P)
    cov = want_cov ? Array{Float64}(undef, ma, ma, P) : Float64[]
    npv = isnothing(noise_pred) ? Float64[] : fill(noise_pred, P)
    GC.@preserve op_off ops prm_off prm ts_pred noises npv mu var cov info check(eng, ccall((:agp_infer_gp_sum_batch, LIB), Cint,
        (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64, Int32, Int32, Ptr{Int32}, Ptr{UInt8}, Ptr{Int32}, Ptr{Float64},
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
        eng.ptr, n, ts_pred, p, P, M, op_off, ops, prm_off, prm, noises,
        isempty(npv) ? Ptr{Float64}(C_NULL) : pointer(npv), mu, var, want_cov ? pointer(cov) : Ptr{Float64}(C_NULL), info))
    k = findfirst(!=(0), info)
    isnothing(k) || throw(LinearAlgebra.PosDefException(info[k]))
    return (mean=mu, var=var, cov=want_cov ? cov : nothing, info=info,
            indexes=(F=[((i-1)*p+1):(i*p) for i in 1:M], X=(M*p+1):(M*p+p)))
end

"""
The numbers of `AutoGP.predict_sum(model, ds, T; quantiles, noise_pred)` (src/api.jl:898-936) on the (scaled) resident series:
per particle the raw-space means of the rows (F_1 .. F_M, X) of the linear `y_transform` (slope, intercept), with
`predict_mvn_sum`'s intercept correction on F_1, and their marginal quantiles, all formed on the device.  Returns (mean, x, info):
mean of size ((M+1)p, P), x of size (length(quantiles), (M+1)p, P); throws `PosDefException` where a particle has no predictive.
"""
function predict_sum_batch(eng::Engine, splits::AbstractVector, noises::Vector{Float64}, ts_pred::Vector{Float64};
        quantiles::Vector{Float64}=Float64[], n::Integer=eng.n_max, noise_pred::Union{Nothing,Float64}=nothing,
        y_slope::Float64=1.0, y_intercept::Float64=0.0)
    all(q -> 0 < q < 1, quantiles) || error("Quantile must be in (0,1).")
    P, M, op_off, ops, prm_off, prm = encode_splits(splits)
    p = length(ts_pred); ma = (M + 1) * p; nq = length(quantiles)
    mu = Matrix{Float64}(undef, ma, P); x = Array{Float64}(undef, nq, ma, P); info = zeros(Int32, P)
    npv = isnothing(noise_pred) ? Float64[] : fill(noise_pred, P)
    GC.@preserve op_off ops prm_off prm ts_pred noises npv quantiles mu x info check(eng, ccall((:agp_predict_sum_batch, LIB), Cint,
        (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64, Int32, Int32, Ptr{Int32}, Ptr{UInt8}, Ptr{Int32}, Ptr{Float64},
         Ptr{Float64}, Ptr{Float64}, Float64, Float64, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
        eng.ptr, n, ts_pred, p, P, M, op_off, ops, prm_off, prm, noises,
        isempty(npv) ? Ptr{Float64}(C_NULL) : pointer(npv), y_slope, y_intercept,
        nq == 0 ? Ptr{Float64}(C_NULL) : pointer(quantiles), nq, mu, nq == 0 ? Ptr{Float64}(C_NULL) : pointer(x), info))
    k = findfirst(!=(0), info)
    isnothing(k) || throw(LinearAlgebra.PosDefException(info[k]))
    return mu, x, info
end

"Decompositions of many short series in one fused launch (agp_predict_sum_series_batch): `predict_sum_batch` for callers that hold
one model per short series, with `predict_series_batch`'s series / query arguments and statelessness.  `splits[p]` holds particle
`p`'s M component kernels (e.g. `GP.split_kernel_sop` of its kernel); particle `p` decomposes `series[series_index[p]]` (1-based) at
`queries[series_index[p]]`.  `y_transforms[s] = (slope, intercept)` of series `s` (scaled = slope * raw + intercept; `nothing`:
(1, 0)); `noise_pred` (`nothing`: each particle's noise) goes on the observable rows only.  Returns `(mean, var, x, logpdf, info)`:
`mean[p]` / `var[p]` of length (M+1) m_s are the raw means and variances of the rows F_1 .. F_M, X (the intercept counted once, on
F_1), `x[p]` of size (length(quantiles), (M+1) m_s) their Normal quantiles; throws `PosDefException` where a particle has no result."
function predict_sum_series_batch(eng::Engine, series::Vector{<:Tuple{Vector{Float64},Vector{Float64}}}, queries::Vector{Vector{Float64}},
                                  splits::AbstractVector, noises::Vector{Float64}, series_index::Vector{<:Integer};
                                  quantiles::Vector{Float64}=Float64[],
                                  y_transforms::Union{Nothing,Vector{Tuple{Float64,Float64}}}=nothing,
                                  noise_pred::Union{Nothing,Vector{Float64}}=nothing)
    all(q -> 0 < q < 1, quantiles) || error("Quantile must be in (0,1).")
    P, M, op_off, ops, prm_off, prm = encode_splits(splits)
    S = length(series)
    (length(noises) == P && length(series_index) == P) || throw(ArgumentError("one noise and one series index per particle required"))
    length(queries) == S || throw(ArgumentError("one vector of query times per series required"))
    (noise_pred === nothing || length(noise_pred) == P) || throw(ArgumentError("one noise_pred per particle required"))
    (y_transforms === nothing || length(y_transforms) == S) || throw(ArgumentError("one (slope, intercept) per series required"))
    all(i -> 1 <= i <= S, series_index) || throw(ArgumentError("series index outside 1:$S"))
    pt_off = Int64[0]; ts = Float64[]; xs = Float64[]; q_off = Int64[0]; tq = Float64[]
    for (s, (t, x)) in enumerate(series)
        length(t) == length(x) || throw(ArgumentError("series $s: ts and xs must have equal lengths"))
        length(t) <= SERIES_MAX_N || throw(ArgumentError("series $s has $(length(t)) points, more than SERIES_MAX_N ($SERIES_MAX_N)"))
        append!(ts, t); append!(xs, x); push!(pt_off, length(ts))
        append!(tq, queries[s]); push!(q_off, length(tq))
    end
    isempty(ts) && (push!(ts, 0.0); push!(xs, 0.0))
    isempty(tq) && push!(tq, 0.0)
    sidx = Int32[Int32(i - 1) for i in series_index]
    slope = y_transforms === nothing ? ones(Float64, max(1, S)) : Float64[t[1] for t in y_transforms]
    icpt = y_transforms === nothing ? zeros(Float64, max(1, S)) : Float64[t[2] for t in y_transforms]
    nq = length(quantiles)
    total = (M + 1) * sum(Int[length(queries[i]) for i in series_index])
    mean = Vector{Float64}(undef, max(1, total)); var = Vector{Float64}(undef, max(1, total))
    x = Vector{Float64}(undef, max(1, nq * total))
    out_off = zeros(Int64, P + 1)
    out = Vector{Float64}(undef, max(1, P)); info = zeros(Int32, max(1, P))
    np = noise_pred === nothing ? noises : noise_pred
    GC.@preserve pt_off ts xs q_off tq sidx op_off ops prm_off prm noises np slope icpt quantiles mean var x out_off out info check(eng, ccall((:agp_predict_sum_series_batch, LIB), Cint,
        (Ptr{Cvoid}, Int32, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Int32, Int32, Ptr{Int32}, Ptr{Int32},
         Ptr{UInt8}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64,
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int32}),
        eng.ptr, S, pt_off, ts, xs, q_off, tq, P, M, sidx, op_off, ops, prm_off, prm, noises, np, slope, icpt,
        nq == 0 ? Ptr{Float64}(C_NULL) : pointer(quantiles), nq, mean, var, nq == 0 ? Ptr{Float64}(C_NULL) : pointer(x), out_off, out, info))
    k = findfirst(!=(0), info[1:P])
    isnothing(k) || throw(LinearAlgebra.PosDefException(info[k]))
    means = [mean[out_off[p] + 1:out_off[p + 1]] for p in 1:P]
    vars = [var[out_off[p] + 1:out_off[p + 1]] for p in 1:P]
    xq = [reshape(x[nq * out_off[p] + 1:nq * out_off[p + 1]], nq, Int(out_off[p + 1] - out_off[p])) for p in 1:P]
    return means, vars, xq, out[1:P], info[1:P]
end

# ------------------------------------------------------------------------------------------------------------------
# multi-process deployment: one Julia process per GPU (Distributed / MPI), log-weights all-gathered through the engine
# ------------------------------------------------------------------------------------------------------------------
"rank 0: the 128-byte RCCL id to hand to the other ranks (any host channel)"
function comm_unique_id()
    id = Vector{UInt8}(undef, COMM_ID_BYTES)
    GC.@preserve id check(nothing, ccall((:agp_comm_get_unique_id, LIB), Cint, (Ptr{UInt8},), id))
    return id
end
function comm_init_rank!(eng::Engine, id::Vector{UInt8}, n_ranks::Integer, rank::Integer)
    @assert length(id) == COMM_ID_BYTES
    GC.@preserve id check(eng, ccall((:agp_comm_init_rank, LIB), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Int32, Int32), eng.ptr, id, n_ranks, rank))
end
"ranks RCCL itself reports for the engine's communicator (ncclCommCount); 0 without one"
function comm_count(eng::Engine)
    n = Ref{Int32}(0)
    check(eng, ccall((:agp_comm_count, LIB), Cint, (Ptr{Cvoid}, Ref{Int32}), eng.ptr, n))
    return Int(n[])
end
"block until every asynchronously enqueued sweep of the engine has completed (reports a latched in-kernel timeout)"
wait!(eng::Engine) = check(eng, ccall((:agp_wait, LIB), Cint, (Ptr{Cvoid},), eng.ptr))
"""
How the particles of the last batch sweep got their covariance tiles (`agp_get_eval_stats`): evaluated inside the factorisation
kernels as one-node programs / as chains in place / by the stack interpreter, prebuilt by the tile builder, and the multi-node chains
among the prebuilt.
"""
function eval_stats(eng::Engine)
    out = zeros(Int64, 5)
    check(eng, ccall((:agp_get_eval_stats, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}), eng.ptr, out))
    return (one_node = Int(out[1]), chain = Int(out[2]), stack = Int(out[3]), prebuilt = Int(out[4]), prebuilt_chain = Int(out[5]))
end
"""
One kernel program as a table-driven sweep compiles it (`agp_probe_program`; host code only): `(n_compiled, chain, depth, n_tables)`.
"""
function probe_program(ops::Vector{UInt8}, prm::Vector{Float64})
    n = Ref{Int32}(0); ch = Ref{Int32}(0); d = Ref{Int32}(0); nt = Ref{Int32}(0)
    rc = ccall((:agp_probe_program, LIB), Cint, (Ptr{UInt8}, Int32, Ptr{Float64}, Int32, Ref{Int32}, Ref{Int32}, Ref{Int32}, Ref{Int32}),
               ops, length(ops), isempty(prm) ? [0.0] : prm, length(prm), n, ch, d, nt)
    rc == 0 || error("agp_probe_program failed ($rc)")
    return (n_compiled = Int(n[]), chain = ch[] != 0, depth = Int(d[]), n_tables = Int(nt[]))
end
"""
Regular time grids (include/autogp_hip.h): `(is_regular, sorted_sweeps)`, the sweeps that read rank tables, the particles whose
gradient was contracted in the lag domain; the switches take effect at the next `set_data!` (lag tables) / sweep (the others).
"""
function lag_stats(eng::Engine)
    reg = Ref{Int32}(0); ns = Ref{Int64}(0); nr = Ref{Int64}(0); ng = Ref{Int64}(0); np = Ref{Int64}(0)
    nt = Ref{Int64}(0); nsg = Ref{Int64}(0); nsv = Ref{Int64}(0)
    check(eng, ccall((:agp_get_lag_stats, LIB), Cint, (Ptr{Cvoid}, Ref{Int32}, Ref{Int64}), eng.ptr, reg, ns))
    check(eng, ccall((:agp_get_lag_rank_stats, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}), eng.ptr, nr))
    check(eng, ccall((:agp_get_grad_lag_domain_stats, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}), eng.ptr, ng))
    check(eng, ccall((:agp_get_lag_predict_stats, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}), eng.ptr, np))
    check(eng, ccall((:agp_get_grad_toeplitz_stats, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}), eng.ptr, nt))
    check(eng, ccall((:agp_get_grad_structured_stats, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}), eng.ptr, nsg))
    check(eng, ccall((:agp_get_toeplitz_stats, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}), eng.ptr, nsv))
    return (regular = reg[] != 0, sorted_sweeps = Int(ns[]), rank_sweeps = Int(nr[]), lag_domain_gradients = Int(ng[]),
            lattice_predictions = Int(np[]), toeplitz_gradients = Int(nt[]), structured_gradients = Int(nsg[]),
            structured_values = Int(nsv[]))
end
set_lag_tables!(eng::Engine, on::Bool) = check(eng, ccall((:agp_set_lag_tables, LIB), Cint, (Ptr{Cvoid}, Int32), eng.ptr, on ? 1 : 0))
"level 2: additionally the OPT-IN structured value sweep (Toeplitz + rank-2 particles by the Schur algorithm; include/autogp_hip.h)"
function set_lag_tables!(eng::Engine, level::Integer)
    check(eng, ccall((:agp_set_lag_tables, LIB), Cint, (Ptr{Cvoid}, Int32), eng.ptr, Int32(level)))
    eng.lag_level = Int32(level)
    return nothing
end
set_lag_rank_tables!(eng::Engine, on::Bool) = check(eng, ccall((:agp_set_lag_rank_tables, LIB), Cint, (Ptr{Cvoid}, Int32), eng.ptr, on ? 1 : 0))
set_grad_lag_domain!(eng::Engine, on::Bool) = check(eng, ccall((:agp_set_grad_lag_domain, LIB), Cint, (Ptr{Cvoid}, Int32), eng.ptr, on ? 2 : 0))
"(lags_per_ordinal, table_entries, sweeps): compact lag tables of a long calendar lattice (monthly / quarterly / yearly dates)"
function compact_stats(eng::Engine)
    w = Ref{Int32}(0); ne = Ref{Int64}(0); ns = Ref{Int64}(0)
    check(eng, ccall((:agp_get_compact_stats, LIB), Cint, (Ptr{Cvoid}, Ref{Int32}, Ref{Int64}, Ref{Int64}), eng.ptr, w, ne, ns))
    return (lags_per_ordinal = Int(w[]), table_entries = Int(ne[]), sweeps = Int(ns[]))
end
"(bytes, fills): memory the engine filled with NaN bits so far (checking mode AGP_POISON=1; results are unchanged by it)"
function poison_stats(eng::Engine)
    b = Ref{Int64}(0); f = Ref{Int64}(0)
    check(eng, ccall((:agp_get_poison_stats, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}), eng.ptr, b, f))
    return (bytes = Int(b[]), fills = Int(f[]))
end
"(kind, n_lattice, spacing) of the resident series: kind 0 irregular, 1 regular grid, 2 lattice with gaps (calendar indices), 3 a longer lattice served by compact tables"
function lattice_stats(eng::Engine)
    kind = Ref{Int32}(0); nl = Ref{Int64}(0); h = Ref{Float64}(0.0)
    check(eng, ccall((:agp_get_lattice_stats, LIB), Cint, (Ptr{Cvoid}, Ref{Int32}, Ref{Int64}, Ref{Float64}), eng.ptr, kind, nl, h))
    return (kind = Int(kind[]), n_lattice = Int(nl[]), spacing = h[])
end
"block [lo, hi] (1-based, inclusive) of rank `rank` (0-based) — identical on every rank"
function shard_range(P::Integer, rank::Integer, n_ranks::Integer)
    lo = Ref{Int32}(0); hi = Ref{Int32}(0)
    ccall((:agp_shard_range, LIB), Cvoid, (Int32, Int32, Int32, Ref{Int32}, Ref{Int32}), P, rank, n_ranks, lo, hi)
    return (lo[] + 1):hi[]
end
"""
Cost-aware, duplicate-aware assignment of a population to ranks (`agp_shard_plan`; host code, identical on every rank): `sweep` 0 value,
1 gradient, 2 marginal prediction with `m_future` query points beyond the data, 3 opt-in structured value sweep; `lattice_kind` = the resident
series' kind (0 irregular, 1 regular grid, 2 lattice with gaps: `lattice_stats(eng)`).  Returns the 0-based owner rank of every particle,
every particle's modelled cost (units of one dense factorisation; 0 for copies) and the ranks' totals — as the Python wrapper does; a rank evaluates `findall(==(rank), owner)` and the gathered log-weights
are scattered back by the same vector.
"""
function shard_plan(nodes::Vector{<:GP.Node}, noises::Vector{Float64}, n::Integer, n_ranks::Integer;
                    sweep::Integer=1, lattice_kind::Integer=1, m_future::Integer=0)
    P = length(nodes)
    op_off, ops, prm_off, prm = encode_batch(nodes)
    owner = Vector{Int32}(undef, max(P, 1)); cost = Vector{Float64}(undef, max(P, 1)); rank_cost = Vector{Float64}(undef, n_ranks)
    rc = GC.@preserve op_off ops prm_off prm noises owner cost rank_cost ccall((:agp_shard_plan, LIB), Cint,
        (Int64, Int32, Ptr{Int32}, Ptr{UInt8}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Int32, Int32, Int64, Int32, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}),
        n, P, op_off, ops, prm_off, prm, noises, sweep, lattice_kind, m_future, n_ranks, owner, cost, rank_cost)
    rc == 0 || error("agp_shard_plan failed ($rc)")
    return owner[1:P], cost[1:P], rank_cost
end
"""
`lw` has one entry per particle of the WHOLE population with this rank's block filled; on return every rank holds
the complete vector — the input of compute_particle_weights / effective_sample_size / Gen.maybe_resample!
(src/inference_smc_anneal_data.jl:22-31,232).
"""
function allgather_logweights!(eng::Engine, lw::Vector{Float64})
    GC.@preserve lw check(eng, ccall((:agp_allgather_logweights, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int32), eng.ptr, lw, length(lw)))
    return lw
end

# ------------------------------------------------------------------------------------------------------------------
# Gen distributions: the trace-score term of src/Model.jl:136 evaluated on the GPU
# ------------------------------------------------------------------------------------------------------------------
# (1) Drop-in for the VALUE calls, tree-typed argument:
#         xs ~ gp_marginal(engine, covariance_fn, noise, ts)
#     Gen cannot differentiate through a GP.Node argument (has_argument_grads must be false for it), so this form is
#     for traces whose parameters are moved by value-only kernels (MH, involutive MCMC, resample-move reweighting).
#     It REFUSES to be used inside choice_gradients (tracked parameters), instead of silently dropping the
#     likelihood gradient.
struct GPMarginal <: Gen.Distribution{Vector{Float64}} end
const gp_marginal = GPMarginal()

reference_logpdf(xs, node, noise, ts) =
    Gen.logpdf(Gen.mvnormal, xs, zeros(length(ts)), GP.compute_cov_matrix_vectorized(node, noise, ts))

function Gen.logpdf(::GPMarginal, xs::Vector{Float64}, engs, node::GP.Node, noise::Real, ts::Vector{Float64})
    any(v -> !(v isa AbstractFloat || v isa Integer), flat_params(node)) &&
        error("gp_marginal received tracked kernel parameters (Gen.choice_gradients / hmc / map_optimize): use " *
              "gp_marginal_flat, whose logpdf_grad returns the engine's gradient")
    eng = engine_for_thread(engs)
    # Gen.simulate / generate without a constraint on :xs sample xs themselves (Gen.random below): such a trace is
    # scored on ITS xs, not on the resident series — through the reference's own arithmetic
    is_resident_prefix(eng, ts, xs) || return reference_logpdf(xs, node, Float64(noise), ts)
    return logpdf(eng, node, Float64(noise), length(ts))
end
Gen.random(::GPMarginal, engs, node, noise, ts) =
    Gen.random(Gen.mvnormal, zeros(length(ts)), GP.compute_cov_matrix_vectorized(node, noise, ts))
Gen.has_output_grad(::GPMarginal) = false
Gen.has_argument_grads(::GPMarginal) = (false, false, false, false)
Gen.is_discrete(::GPMarginal) = false

# (2) The differentiable form, flat arguments:
#         xs ~ gp_marginal_flat(engine, structure(covariance_fn), flat_params(covariance_fn), noise, ts)
#     `theta` is a Vector of Reals — exactly the values `covariance_prior` builds its nodes from
#     (transform_param(field, z, config), src/Model.jl:94,116), so under Gen.choice_gradients its entries are tracked
#     and Gen asks this distribution for argument gradients: has_argument_grads is true for theta and noise,
#     logpdf_grad returns the engine's d logpdf / d theta and d logpdf / d noise, and ReverseDiff carries them on
#     through transform_param to the latent N(0,1) choices that Gen.hmc / Gen.map_optimize move
#     (src/inference_smc_anneal_data.jl:63-67, src/Greedy.jl:95,370).  ChangePoint's fixed scale (.001, src/Model.jl:121)
#     is an untracked entry of theta: its gradient slot is computed and ignored.
struct GPMarginalFlat <: Gen.Distribution{Vector{Float64}} end
const gp_marginal_flat = GPMarginalFlat()

function node_from_flat(ops::Vector{UInt8}, theta::AbstractVector)
    stack = GP.Node[]; q = 0
    take(k) = (v = theta[q+1:q+k]; q += k; v)
    for o in ops
        if o == 0x00 push!(stack, GP.WhiteNoise(take(1)...))
        elseif o == 0x01 push!(stack, GP.Constant(take(1)...))
        elseif o == 0x02 push!(stack, GP.Linear(take(3)...))
        elseif o == 0x03 push!(stack, GP.SquaredExponential(take(2)...))
        elseif o == 0x04 push!(stack, GP.GammaExponential(take(3)...))
        elseif o == 0x05 push!(stack, GP.Periodic(take(3)...))
        else
            r = pop!(stack); l = pop!(stack)
            push!(stack, o == 0x06 ? GP.Plus(l, r) : o == 0x07 ? GP.Times(l, r) : GP.ChangePoint(l, r, take(2)...))
        end
    end
    return only(stack)
end

function Gen.logpdf(::GPMarginalFlat, xs::Vector{Float64}, engs, ops::Vector{UInt8}, theta::AbstractVector{<:Real},
                    noise::Real, ts::Vector{Float64})
    eng = engine_for_thread(engs)
    th = Float64[Float64(v) for v in theta]       # Gen passes VALUES here (arguments are untracked in logpdf)
    is_resident_prefix(eng, ts, xs) || return reference_logpdf(xs, node_from_flat(ops, th), Float64(noise), ts)
    return logpdf_program(eng, ops, th, Float64(noise), length(ts))
end

function Gen.logpdf_grad(::GPMarginalFlat, xs::Vector{Float64}, engs, ops::Vector{UInt8}, theta::AbstractVector{<:Real},
                         noise::Real, ts::Vector{Float64})
    eng = engine_for_thread(engs)
    th = Float64[Float64(v) for v in theta]
    is_resident_prefix(eng, ts, xs) ||
        error("gp_marginal_flat.logpdf_grad: (ts, xs) is not the prefix of the series uploaded with set_data!")
    _, g, gn = logpdf_grad_program(eng, ops, th, Float64(noise), length(ts))
    # (output grad, then one entry per argument: engine, ops, theta, noise, ts)
    return (nothing, nothing, nothing, g, gn, nothing)
end
Gen.random(::GPMarginalFlat, engs, ops, theta, noise, ts) =
    Gen.random(Gen.mvnormal, zeros(length(ts)),
               GP.compute_cov_matrix_vectorized(node_from_flat(ops, Float64[Float64(v) for v in theta]), Float64(noise), ts))
Gen.has_output_grad(::GPMarginalFlat) = false
Gen.has_argument_grads(::GPMarginalFlat) = (false, false, true, true, false)
Gen.is_discrete(::GPMarginalFlat) = false

# The patched model body (replaces src/Model.jl:131-138; covariance_prior itself is unchanged):
#
#   @gen function model(ts::Vector{Float64}, config::GPConfig)
#       covariance_fn = {:tree} ~ covariance_prior(1, config)
#       noise ~ normal(0, 1)
#       noise = transform_param(:noise, noise, config) + JITTER
#       xs ~ AutoGPHIP.gp_marginal_flat(ENGINES[], AutoGPHIP.structure(covariance_fn),
#                                       AutoGPHIP.flat_params(covariance_fn), noise, ts)
#       return covariance_fn
#   end

end # module
