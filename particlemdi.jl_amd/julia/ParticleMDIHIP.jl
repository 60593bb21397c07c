# ParticleMDIHIP.jl -- Julia glue for libpmdi_hip.so (include/pmdi_hip.h).
#
# STATUS: written against the C ABI but NOT executed anywhere in this repository's CI: neither
# the build container nor the GPU box has a julia binary (DESIGN.md).  The Python twin of this
# file (particlemdi.jl_amd/pmdi.py) drives the same ABI and is what the GPU tests exercise.
#
# Two drivers: `pmdi` replaces only the sweep (the reference's own Julia hyper-parameter functions stay, as the
# north star describes); `pmdi_device` runs the whole iteration on the device (pmdi_gibbs_*, pmdi_csv_*).
#
# What it does: `ParticleMDIHIP.pmdi(...)` has the signature, the asserts and the CSV output of
# `ParticleMDI.pmdi` (src/pmdi.jl:36-40, 50-55, 147-158, 377-383).  The hyper-parameter
# updates and label alignment are the reference's own functions, called from the installed
# ParticleMDI package (update_M!, update_γ!, update_Φ!, update_Z, update_v, align_labels!);
# only the block src/pmdi.jl:165-171,188-370 -- reset, known prefix, the conditional-SMC sweep,
# particle pick and feature selection -- is replaced by two ccalls.  If any dataTypes[k] is
# not one of the three built-in cluster types (a user-defined plugin type, README.md:48-88),
# the call is forwarded unchanged to ParticleMDI.pmdi: user types keep working on the
# reference's CPU loop.
module ParticleMDIHIP

using ParticleMDI
using DelimitedFiles, Distributions, Printf, Random
using NonUniformRandomVariateGeneration: sampleCategorical

const LIB = get(ENV, "PMDI_HIP_LIB", joinpath(@__DIR__, "..", "libpmdi_hip.so"))
const PMDI_ABI_VERSION = Int32(2)

# mirrors of the C structs in include/pmdi_hip.h
struct CDataset
    kind::Int32
    D::Int32
    ld::Int64
    xf::Ptr{Float64}
    xi::Ptr{Int64}
end

struct CConfig
    abi_version::Int32
    device::Int32
    K::Int32
    N::Int32
    P::Int32
    n_chains::Int32
    n::Int64
    seed::UInt64
    q1_mode::Int32
    q2_mode::Int32
    pool_cap::Int64
    block_threads::Int32
    reserved::Int32
    tuning::Ptr{Cvoid}      # const pmdi_tuning * (kernel-selection knobs); C_NULL = all automatic
end

struct CSweepStats
    n_operations::Int64
    n_resamples::Int64
    n_clones::Int64
    max_id::Int64
    sum_classes::Int64
    steps_fast::Int64
    steps_converted::Int64
    steps_fallback::Int64
end

device_kind(::Type{ParticleMDI.GaussianCluster}) = Int32(0)
device_kind(::Type{ParticleMDI.CategoricalCluster}) = Int32(1)
device_kind(::Type{ParticleMDI.NegBinomCluster}) = Int32(2)
device_kind(::Any) = Int32(-1)

function check(rc::Cint)
    rc == 0 && return
    msg = unsafe_string(ccall((:pmdi_last_error, LIB), Cstring, ()))
    error("libpmdi_hip: [$rc] $msg")
end

"""
    pmdi(dataFiles, dataTypes, N, particles, ρ, iter, outputFile; thin, featureSelect, dataNames,
         seed = rand(UInt64), device = 0)

Drop-in for `ParticleMDI.pmdi`; the sweep runs on an MI355X.
"""
function pmdi(dataFiles, dataTypes, N::Int64, particles::Int64, ρ::Float64, iter::Int64,
              outputFile::String; thin::Int64 = 1, featureSelect::Union{String, Nothing} = nothing,
              dataNames = nothing, seed::UInt64 = rand(UInt64), device::Integer = 0)
    kinds = [device_kind(t) for t in dataTypes]
    if any(k -> k < 0, kinds)
        # a user-defined cluster type: the reference's own loop handles it
        return ParticleMDI.pmdi(dataFiles, dataTypes, N, particles, ρ, iter, outputFile;
                                thin = thin, featureSelect = featureSelect, dataNames = dataNames)
    end
    K = length(dataFiles)
    n_obs = size(dataFiles[1], 1)
    dataNames === nothing && (dataNames = ["K$i" for i in 1:K])
    @assert length(dataTypes) == K "Number of datatypes not equal to number of datasets"
    @assert length(dataNames) == K "Number of data names not equal to number of datasets"
    @assert all(size(d, 1) == n_obs for d in dataFiles) "Datasets don't have same number of observations. Each row must correspond to the same underlying observational unit across datasets."
    @assert 0 < ρ < 1 "ρ must be between 0 and 1"
    @assert 1 < N <= n_obs "Number of clusters must be greater than 1 and not greater than the number of observations"
    @assert particles > 1 "Conditional particle filter requires 2 or more particles"
    n1 = floor(Int64, ρ * n_obs)
    @assert n1 >= 1 "floor(ρ·n) must be at least 1"

    # ---- device handle: data are copied to the GPU once ----
    mats = [kinds[k] == 0 ? convert(Matrix{Float64}, dataFiles[k]) : convert(Matrix{Int64}, dataFiles[k]) for k in 1:K]
    handle = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve mats begin
        ds = [CDataset(kinds[k], Int32(size(mats[k], 2)), Int64(n_obs),
                       kinds[k] == 0 ? pointer(mats[k]) : Ptr{Float64}(C_NULL),
                       kinds[k] == 0 ? Ptr{Int64}(C_NULL) : pointer(mats[k])) for k in 1:K]
        cfg = Ref(CConfig(PMDI_ABI_VERSION, Int32(device), Int32(K), Int32(N), Int32(particles), Int32(1),
                          Int64(n_obs), seed, Int32(0), Int32(0), Int64(0), Int32(0), Int32(0), C_NULL))
        check(ccall((:pmdi_create, LIB), Cint, (Ref{CConfig}, Ptr{CDataset}, Ref{Ptr{Cvoid}}), cfg, ds, handle))
    end
    h = handle[]

    try
        # ---- host state, exactly as the reference initialises it (src/pmdi.jl:59-96) ----
        M = fill(2.0, K)
        γc = rand(Gamma(1.0 / N, 1.0), N, K) .+ eps(Float64)
        npairs = K > 1 ? div(K * (K - 1), 2) : 1
        Φ = K > 1 ? rand(Gamma(1, 0.2), npairs) : zeros(1)
        s = Matrix{Int64}(undef, n_obs, K)
        for k in 1:K
            s[:, k] = sampleCategorical(n_obs, γc[:, k])
        end
        c_combn = Matrix{Int64}(undef, N^K, K)
        for k in 1:K
            c_combn[:, K - k + 1] = div.(0:(N^K - 1), N^(K - k)) .% N .+ 1
        end
        Γc = Matrix{Float64}(undef, N^K, K)
        for k in 1:K
            Γc[:, k] = log.(γc[:, k])[c_combn[:, k]]
        end
        Φ_index = K > 1 ? Matrix{Bool}(undef, N^K, npairs) : fill(1, (N, 1))
        if K > 1
            col = 1
            for k1 in 1:(K - 1), k2 in (k1 + 1):K
                Φ_index[:, col] = c_combn[:, k1] .== c_combn[:, k2]
                col += 1
            end
        end
        Z = ParticleMDI.update_Z(Φ, Φ_index, Γc)
        v = ParticleMDI.update_v(n_obs, Z)

        D = [size(d, 2) for d in dataFiles]
        flags = featureSelect === nothing ? ones(UInt8, sum(D)) : UInt8.(rand(Bool, sum(D)))
        featureFile = nothing
        if featureSelect !== nothing
            names = ["$(dataNames[k])_d$d" for k in 1:K for d in 1:D[k]]
            writedlm(featureSelect, reshape(names, 1, :), ',')
            featureFile = open(featureSelect, "a")
            writedlm(featureFile, reshape(Bool.(flags), 1, :), ',')
        end

        Φ_lab = ParticleMDI.calculate_Φ_lab(K)
        header = [[@sprintf("MassParameter_%d", k) for k in 1:K];
                  [@sprintf("phi_%d_%d", Φ_lab[i, 1], Φ_lab[i, 2]) for i in 1:size(Φ_lab, 1)];
                  "ll";
                  ["$(dataNames[k])_n$i" for k in 1:K for i in 1:n_obs]]
        writedlm(outputFile, reshape(header, 1, :), ',')
        fileid = open(outputFile, "a")
        t0 = time_ns()
        writedlm(fileid, [M; Φ; 0; s[1:(n_obs * K)]]', ',')

        order_obs = collect(1:n_obs)
        s_out = similar(s)
        logweight = zeros(Float64, particles)
        p_star = Ref{Int64}(0)
        stats = Ref(CSweepStats(0, 0, 0, 0, 0, 0, 0, 0))
        flags_out = similar(flags)
        for it in 1:iter
            shuffle!(order_obs)                                        # src/pmdi.jl:172
            ParticleMDI.update_M!(M, γc, K, N)                          # :176
            ParticleMDI.update_γ!(γc, Φ, v, M, s, Φ_index, c_combn, Γc, N, K)
            Π = γc ./ sum(γc, dims = 1)                                 # :179
            K > 1 && ParticleMDI.update_Φ!(Φ, v, s, Φ_index, γc, K, Γc)
            Z = ParticleMDI.update_Z(Φ, Φ_index, Γc)
            v = ParticleMDI.update_v(n_obs, Z)

            # ---- replaces src/pmdi.jl:165-171, 188-350, 373 ----
            check(ccall((:pmdi_sweep, LIB), Cint,
                        (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8},
                         Float64, Ptr{Int64}, Ptr{Float64}, Ref{Int64}, Ref{CSweepStats}, Ptr{Float64}),
                        h, it, s, order_obs, n1, Π, Φ, flags, it == 1 ? 0.0 : 1.0,
                        s_out, logweight, p_star, stats, C_NULL))
            if featureSelect !== nothing
                # ---- replaces src/pmdi.jl:354-370 ----
                check(ccall((:pmdi_feature_select, LIB), Cint,
                            (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{UInt8}, Ptr{Float64}),
                            h, it, s_out, flags_out, C_NULL))
                flags .= flags_out
            end
            s .= s_out                                                  # :373
            ParticleMDI.align_labels!(s, Φ, γc, N, K)                   # :375

            ll = (time_ns() - t0) / 1.0e9                               # :377
            if it % thin == 0
                writedlm(fileid, [M; Φ; ll; s[1:(n_obs * K)]]', ',')
                featureFile !== nothing && writedlm(featureFile, reshape(Bool.(flags), 1, :), ',')
            end
        end
        close(fileid)
        featureFile !== nothing && close(featureFile)
    finally
        ccall((:pmdi_destroy, LIB), Cint, (Ptr{Cvoid},), h)
    end
    return
end

"""
    pmdi_device(dataFiles, dataTypes, N, particles, ρ, iter, outputFile; thin, featureSelect, dataNames,
                seed = rand(UInt64), device = 0, q2_mode = 0)

The same run with EVERYTHING of an iteration on the MI355X (include/pmdi_hip.h, pmdi_gibbs_*): shuffle!(order_obs),
update_M!, update_γ!, update_Φ!, update_Z, update_v (evaluated without the N^K tables of src/pmdi.jl:69-92), the sweep,
feature selection and align_labels! (contingency tables) are device kernels; the CSV rows are written by the library's
byte-compatible writer (pmdi_csv_*).  Host-side draws become counter-based Philox variates keyed on `seed`
(SURVEY 8 rows f1, f2, f4).  `pmdi` above keeps the reference's own Julia functions for those parts.
"""
function pmdi_device(dataFiles, dataTypes, N::Int64, particles::Int64, ρ::Float64, iter::Int64,
                     outputFile::String; thin::Int64 = 1, featureSelect::Union{String, Nothing} = nothing,
                     dataNames = nothing, seed::UInt64 = rand(UInt64), device::Integer = 0, q2_mode::Integer = 0)
    kinds = [device_kind(t) for t in dataTypes]
    any(k -> k < 0, kinds) && return ParticleMDI.pmdi(dataFiles, dataTypes, N, particles, ρ, iter, outputFile;
                                                      thin = thin, featureSelect = featureSelect, dataNames = dataNames)
    K = length(dataFiles)
    n_obs = size(dataFiles[1], 1)
    dataNames === nothing && (dataNames = ["K$i" for i in 1:K])
    @assert length(dataNames) == K "Number of data names not equal to number of datasets"
    @assert length(dataTypes) == K "Number of datatypes not equal to number of datasets"
    @assert all(size(d, 1) == n_obs for d in dataFiles) "Datasets don't have same number of observations. Each row must correspond to the same underlying observational unit across datasets."
    @assert 0 < ρ < 1 "ρ must be between 0 and 1"
    @assert 1 < N <= n_obs "Number of clusters must be greater than 1 and not greater than the number of observations"
    @assert particles > 1 "Conditional particle filter requires 2 or more particles"
    mats = [kinds[k] == 0 ? convert(Matrix{Float64}, dataFiles[k]) : convert(Matrix{Int64}, dataFiles[k]) for k in 1:K]
    handle = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve mats begin
        ds = [CDataset(kinds[k], Int32(size(mats[k], 2)), Int64(n_obs),
                       kinds[k] == 0 ? pointer(mats[k]) : Ptr{Float64}(C_NULL),
                       kinds[k] == 0 ? Ptr{Int64}(C_NULL) : pointer(mats[k])) for k in 1:K]
        cfg = Ref(CConfig(PMDI_ABI_VERSION, Int32(device), Int32(K), Int32(N), Int32(particles), Int32(1),
                          Int64(n_obs), seed, Int32(0), Int32(q2_mode), Int64(0), Int32(0), Int32(0), C_NULL))
        check(ccall((:pmdi_create, LIB), Cint, (Ref{CConfig}, Ptr{CDataset}, Ref{Ptr{Cvoid}}), cfg, ds, handle))
    end
    h = handle[]
    g = Ref{Ptr{Cvoid}}(C_NULL)
    csv = Ref{Ptr{Cvoid}}(C_NULL)
    fcsv = Ref{Ptr{Cvoid}}(C_NULL)
    try
        check(ccall((:pmdi_gibbs_create, LIB), Cint, (Ptr{Cvoid}, Float64, Int32, Ref{Ptr{Cvoid}}),
                    h, ρ, featureSelect === nothing ? 0 : 1, g))                 # src/pmdi.jl:59-66, 95-96, 106-110
        # own the strings whose pointers cross the ABI (String(nm) of a SubString or Symbol is a temporary: rooting
        # `dataNames` would not keep it alive)
        strs = String[String(nm) for nm in dataNames]
        names = [Base.unsafe_convert(Cstring, st) for st in strs]
        GC.@preserve strs begin
            check(ccall((:pmdi_csv_open, LIB), Cint, (Cstring, Int32, Int64, Ptr{Cstring}, Ref{Ptr{Cvoid}}),
                        outputFile, K, n_obs, names, csv))                       # :147-156
            if featureSelect !== nothing
                D = Int32[size(d, 2) for d in dataFiles]
                check(ccall((:pmdi_csv_open_features, LIB), Cint, (Cstring, Int32, Ptr{Int32}, Ptr{Cstring}, Ref{Ptr{Cvoid}}),
                            featureSelect, K, D, names, fcsv))                   # :111
            end
        end
        flags = Vector{UInt8}(undef, sum(size(d, 2) for d in dataFiles))
        write_flags() = begin
            check(ccall((:pmdi_gibbs_get, LIB), Cint,
                        (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{UInt8}),
                        g[], 0, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, flags))
            check(ccall((:pmdi_csv_write_flags, LIB), Cint, (Ptr{Cvoid}, Ptr{UInt8}), fcsv[], flags))
        end
        featureSelect === nothing || write_flags()                                # :116
        t0 = time_ns()
        check(ccall((:pmdi_csv_write_gibbs, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Float64), csv[], g[], 0, 0.0))   # :158
        stats = Vector{Int64}(undef, 8)
        for it in 1:iter
            check(ccall((:pmdi_gibbs_iterate, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{UInt8}, Ptr{Cvoid}), g[], 1, C_NULL, C_NULL))   # :165-375
            check(ccall((:pmdi_gibbs_results, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int32}, Ptr{Int64}, Ptr{Float64}),
                        g[], stats, C_NULL, C_NULL, C_NULL))                     # synchronises; a kernel-side error surfaces here
            ll = (time_ns() - t0) / 1.0e9                                        # :377
            if it % thin == 0
                check(ccall((:pmdi_csv_write_gibbs, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Float64), csv[], g[], 0, ll))   # :379
                featureSelect === nothing || write_flags()                       # :381
            end
        end
    finally
        csv[] == C_NULL || ccall((:pmdi_csv_close, LIB), Cint, (Ptr{Cvoid},), csv[])
        fcsv[] == C_NULL || ccall((:pmdi_csv_close, LIB), Cint, (Ptr{Cvoid},), fcsv[])
        g[] == C_NULL || ccall((:pmdi_gibbs_destroy, LIB), Cint, (Ptr{Cvoid},), g[])
        ccall((:pmdi_destroy, LIB), Cint, (Ptr{Cvoid},), h)
    end
    return
end

# ---- streaming PSM accumulator and pooled runs (include/pmdi_hip.h, pmdi_psm_acc_*, pmdi_gibbs_run) --------------
# (like the rest of this file: written against include/pmdi_hip.h, not executed -- there is no Julia where this was built)
function psm_acc_create(K::Integer, n::Integer; n_labels::Integer = 0, device::Integer = 0)
    a = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:pmdi_psm_acc_create, LIB), Cint, (Int32, Int32, Int64, Int32, Ref{Ptr{Cvoid}}), device, K, n, n_labels, a))
    return a[]
end
psm_acc_destroy(a::Ptr{Cvoid}) = ccall((:pmdi_psm_acc_destroy, LIB), Cint, (Ptr{Cvoid},), a)
psm_acc_reset(a::Ptr{Cvoid}; stream::Ptr{Cvoid} = C_NULL) = check(ccall((:pmdi_psm_acc_reset, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), a, stream))
# samples: device pointer to UInt8 [S][K][n]
psm_acc_add_samples(a::Ptr{Cvoid}, samples::Ptr{Cvoid}, S::Integer; stream::Ptr{Cvoid} = C_NULL) =
    check(ccall((:pmdi_psm_acc_add_samples, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}), a, samples, S, stream))
psm_acc_add_gibbs(a::Ptr{Cvoid}, g::Ptr{Cvoid}; stream::Ptr{Cvoid} = C_NULL) =
    check(ccall((:pmdi_psm_acc_add_gibbs, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), a, g, stream))
# counts: device pointer to Int32 [K][n][n] on the accumulator's device (only i >= j is read)
psm_acc_merge(a::Ptr{Cvoid}, counts::Ptr{Cvoid}, S::Integer; stream::Ptr{Cvoid} = C_NULL) =
    check(ccall((:pmdi_psm_acc_merge, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}), a, counts, S, stream))
psm_acc_samples(a::Ptr{Cvoid}) = ccall((:pmdi_psm_acc_samples, LIB), Int64, (Ptr{Cvoid},), a)
# -> (device pointer to the full, symmetric Int32 [K][n][n], S): what psm_distance_device takes
function psm_acc_counts(a::Ptr{Cvoid}; stream::Ptr{Cvoid} = C_NULL)
    counts = Ref{Ptr{Cvoid}}(C_NULL); S = Ref{Int64}(0)
    check(ccall((:pmdi_psm_acc_counts, LIB), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Ref{Int64}, Ptr{Cvoid}), a, counts, S, stream))
    return counts[], S[]
end
gibbs_run(g::Ptr{Cvoid}, n_iter::Integer; burnin::Integer = 0, thin::Integer = 1, acc::Ptr{Cvoid} = C_NULL, stream::Ptr{Cvoid} = C_NULL) =
    check(ccall((:pmdi_gibbs_run, LIB), Cint, (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}), g, n_iter, burnin, thin, acc, stream))

"""
    pmdi_pooled(dataFiles, dataTypes, N, particles, ρ, iter, n_chains; burnin = 0, thin = 1, featureSelect = false,
                seed = rand(UInt64), device = 0, q2_mode = 0) -> (acc, counts, S)

`n_chains` independent chains on one MI355X, pooled on the device: after local iteration t > burnin with
(t - burnin - 1) % thin == 0 the allocations of every chain go into one streaming accumulator -- the rows
generate_psm(file, burnin + 1, thin) would keep of each chain's CSV, without the CSVs.  Returns the accumulator (the caller
destroys it with psm_acc_destroy when done with the counts), the device pointer to the Int32 [K][n][n] counts and S; hand the
last two to psm_distance_device / hclust_device / cutree.  Writes no files.  Untested twin of pmdi.py's pmdi_pooled.
"""
function pmdi_pooled(dataFiles, dataTypes, N::Int64, particles::Int64, ρ::Float64, iter::Int64, n_chains::Int64;
                     burnin::Int64 = 0, thin::Int64 = 1, featureSelect::Bool = false, seed::UInt64 = rand(UInt64),
                     device::Integer = 0, q2_mode::Integer = 0)
    kinds = [device_kind(t) for t in dataTypes]
    @assert all(k -> k >= 0, kinds) "pmdi_pooled needs cluster types with a device kernel"
    K = length(dataFiles)
    n_obs = size(dataFiles[1], 1)
    @assert length(dataTypes) == K "Number of datatypes not equal to number of datasets"
    @assert all(size(d, 1) == n_obs for d in dataFiles) "Datasets don't have same number of observations. Each row must correspond to the same underlying observational unit across datasets."
    @assert 0 < ρ < 1 "ρ must be between 0 and 1"
    @assert 1 < N <= n_obs "Number of clusters must be greater than 1 and not greater than the number of observations"
    @assert particles > 1 "Conditional particle filter requires 2 or more particles"
    @assert n_chains >= 1 "n_chains must be >= 1"
    @assert 0 <= burnin < iter "burnin must be >= 0 and smaller than iter"
    @assert thin >= 1 "thin must be >= 1"
    mats = [kinds[k] == 0 ? convert(Matrix{Float64}, dataFiles[k]) : convert(Matrix{Int64}, dataFiles[k]) for k in 1:K]
    handle = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve mats begin
        ds = [CDataset(kinds[k], Int32(size(mats[k], 2)), Int64(n_obs),
                       kinds[k] == 0 ? pointer(mats[k]) : Ptr{Float64}(C_NULL),
                       kinds[k] == 0 ? Ptr{Int64}(C_NULL) : pointer(mats[k])) for k in 1:K]
        cfg = Ref(CConfig(PMDI_ABI_VERSION, Int32(device), Int32(K), Int32(N), Int32(particles), Int32(n_chains),
                          Int64(n_obs), seed, Int32(0), Int32(q2_mode), Int64(0), Int32(0), Int32(0), C_NULL))
        check(ccall((:pmdi_create, LIB), Cint, (Ref{CConfig}, Ptr{CDataset}, Ref{Ptr{Cvoid}}), cfg, ds, handle))
    end
    h = handle[]
    g = Ref{Ptr{Cvoid}}(C_NULL)
    acc = C_NULL
    try
        check(ccall((:pmdi_gibbs_create, LIB), Cint, (Ptr{Cvoid}, Float64, Int32, Ref{Ptr{Cvoid}}), h, ρ, featureSelect ? 1 : 0, g))
        acc = psm_acc_create(K, n_obs; n_labels = N, device = device)
        gibbs_run(g[], iter; burnin = burnin, thin = thin, acc = acc)
        check(ccall((:pmdi_gibbs_results, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int32}, Ptr{Int64}, Ptr{Float64}),
                    g[], C_NULL, C_NULL, C_NULL, C_NULL))                        # synchronises; a kernel-side error surfaces here
        counts, S = psm_acc_counts(acc)
        return acc, counts, S
    catch
        acc == C_NULL || psm_acc_destroy(acc)
        rethrow()
    finally
        g[] == C_NULL || ccall((:pmdi_gibbs_destroy, LIB), Cint, (Ptr{Cvoid},), g[])
        ccall((:pmdi_destroy, LIB), Cint, (Ptr{Cvoid},), h)
    end
end

# ---- generate_psm's reading of an output file (src/output_analysis/consensus_map.jl:32-47), natively ----------
# returns (samples::Array{UInt8,3} of size (n_obs, K, rows kept) -- i.e. [row][k][i] in C order --, names)
function read_allocations(outputFile::String, burnin::Int64 = 0, thin::Int64 = 1)
    K = Ref{Int32}(0); n_obs = Ref{Int64}(0); n_iter = Ref{Int64}(0)
    names = Vector{UInt8}(undef, 1 << 16)
    check(ccall((:pmdi_csv_read_allocations, LIB), Cint,
                (Cstring, Int64, Int64, Ref{Int32}, Ref{Int64}, Ref{Int64}, Ptr{UInt8}, Int64, Ptr{UInt8}, Int32),
                outputFile, burnin, thin, K, n_obs, n_iter, C_NULL, 0, names, length(names)))
    samples = Array{UInt8, 3}(undef, n_obs[], K[], n_iter[])
    check(ccall((:pmdi_csv_read_allocations, LIB), Cint,
                (Cstring, Int64, Int64, Ref{Int32}, Ref{Int64}, Ref{Int64}, Ptr{UInt8}, Int64, Ptr{UInt8}, Int32),
                outputFile, burnin, thin, K, n_obs, n_iter, samples, length(samples), C_NULL, 0))
    return samples, split(unsafe_string(pointer(names)), '\n')
end

# ---- get_consensus_allocations (src/output_analysis/consensus_map.jl:92-105) on the device ----------------------
# (like the rest of this file: written against include/pmdi_hip.h, not executed -- there is no Julia where this was built)
const LINKAGES = Dict(:single => Int32(0), :average => Int32(1), :complete => Int32(2), :ward => Int32(3))

struct Hclust
    merges::Matrix{Int64}      # (n-1) x 2: -i observation i, +r the cluster made by row r
    heights::Vector{Float64}
    order::Vector{Int64}
end

# dist: device pointer to B distance matrices (n x n Float64 each; the lower triangle is read, the matrices are overwritten)
function hclust_device(dist::Ptr{Cvoid}, n::Integer, B::Integer = 1; linkage::Symbol = :ward, device::Integer = 0,
                       stream::Ptr{Cvoid} = C_NULL)
    merges = Array{Int64, 3}(undef, max(n - 1, 0), 2, B); heights = Matrix{Float64}(undef, max(n - 1, 0), B)
    order = Matrix{Int64}(undef, n, B)
    check(ccall((:pmdi_hclust_device, LIB), Cint,
                (Int32, Ptr{Cvoid}, Int32, Int64, Int32, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}, Ptr{Cvoid}),
                device, dist, B, n, LINKAGES[linkage], merges, heights, order, stream))
    return [Hclust(merges[:, :, b], heights[:, b], order[:, b]) for b in 1:B]
end

# counts: device pointer to the Int32 [K][n][n] output of pmdi_psm_counts_device (row_lo = 0, row_hi = n); which is 1-based,
# K + 1 = "Overall"; dist_out: device memory for n x n Float64
psm_distance_device(counts::Ptr{Cvoid}, S::Integer, K::Integer, n::Integer, which::Integer, dist_out::Ptr{Cvoid};
                    device::Integer = 0, stream::Ptr{Cvoid} = C_NULL) =
    check(ccall((:pmdi_psm_distance_device, LIB), Cint, (Int32, Ptr{Cvoid}, Int64, Int32, Int64, Int32, Ptr{Cvoid}, Ptr{Cvoid}),
                device, counts, S, K, n, which - 1, dist_out, stream))

function cutree(hc::Hclust; k::Union{Int64, Nothing} = nothing, h::Union{Float64, Nothing} = nothing)
    n = length(hc.order)
    labels = Vector{Int64}(undef, n)
    check(ccall((:pmdi_cutree, LIB), Cint, (Int64, Ptr{Int64}, Ptr{Float64}, Int64, Float64, Ptr{Int64}),
                n, hc.merges, hc.heights, k === nothing ? -1 : k, h === nothing ? NaN : h, labels))
    return labels
end

# ---- which clustering: candidates scored against the counts (pmdi_psm_score_device; not executed, as above) ----
# counts as in psm_distance_device; cand: device pointer to Int32 labels, candidate b at cand + b * ld (ld >= n); which is
# 1-based, K + 1 = "Overall".  Returns (agree, pairs, total, D); binder / pear follow include/pmdi_hip.h in BigInt, one division.
function psm_score_device(counts::Ptr{Cvoid}, S::Integer, K::Integer, n::Integer, which::Integer, cand::Ptr{Cvoid}, B::Integer,
                          ld::Integer = n; device::Integer = 0, stream::Ptr{Cvoid} = C_NULL)
    agree = Vector{Int64}(undef, B); pairs = Vector{Int64}(undef, B); total = Ref{Int64}(0)
    check(ccall((:pmdi_psm_score_device, LIB), Cint,
                (Int32, Ptr{Cvoid}, Int64, Int32, Int64, Int32, Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ref{Int64}, Ptr{Cvoid}),
                device, counts, S, K, n, which - 1, cand, B, ld, agree, pairs, total, stream))
    return agree, pairs, total[], S * (which == K + 1 ? K : 1)
end
binder(agree, pairs, total, D) = [Float64((big(D) * q + total - 2 * big(a)) // big(D)) for (a, q) in zip(agree, pairs)]
function pear(agree, pairs, total, D, n)
    P = big(n) * (n - 1) ÷ 2
    map(zip(agree, pairs)) do (a, q)
        den = (big(D) * q + total) * P - 2 * big(q) * total
        den == 0 ? NaN : Float64(2 * (big(a) * P - big(q) * total) // den)
    end
end

# ---- per-observation scores and the Binder descent (pmdi_psm_rowscore_device, pmdi_psm_refine_device; not executed, as above) ----
# own, size, rowtotal: device pointers to Int64 [B][n], Int32 [B][n], Int64 [n] that the call fills (asynchronous on stream).
function psm_rowscore_device(counts::Ptr{Cvoid}, S::Integer, K::Integer, n::Integer, which::Integer, cand::Ptr{Cvoid}, B::Integer,
                             own::Ptr{Cvoid}, size::Ptr{Cvoid}, rowtotal::Ptr{Cvoid}, ld::Integer = n;
                             device::Integer = 0, stream::Ptr{Cvoid} = C_NULL)
    check(ccall((:pmdi_psm_rowscore_device, LIB), Cint,
                (Int32, Ptr{Cvoid}, Int64, Int32, Int64, Int32, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                device, counts, S, K, n, which - 1, cand, B, ld, own, size, rowtotal, stream))
    return S * (which == K + 1 ? K : 1)
end
# own, size: one candidate's rows copied to the host; the Wade-Ghahramani bound and the per-observation confidence
vi_bound(own, size, rowtotal, D) =
    sum(log2.(Float64.(size)) .+ log2.(Float64.(rowtotal .+ D)) .+ log2(Float64(D)) .- 2 .* log2.(Float64.(own .+ D))) / length(own)
confidence(own, size, D) = Float64.(own .+ D) ./ Float64.(D .* size)
const REFINE_GMAX = 4096
# start: device pointer to Int32 slot labels 0..REFINE_GMAX-1, start b at start + b * ld; labels: device Int32 [B][n], filled.
# Returns (moves, sweeps) per start; synchronises.
function psm_refine_device(counts::Ptr{Cvoid}, S::Integer, K::Integer, n::Integer, which::Integer, start::Ptr{Cvoid}, B::Integer,
                           labels::Ptr{Cvoid}, ld::Integer = n; max_sweeps::Integer = 64, device::Integer = 0, stream::Ptr{Cvoid} = C_NULL)
    moves = Vector{Int64}(undef, B); sweeps = Vector{Int32}(undef, B)
    check(ccall((:pmdi_psm_refine_device, LIB), Cint,
                (Int32, Ptr{Cvoid}, Int64, Int32, Int64, Int32, Ptr{Cvoid}, Int64, Int64, Int32, Ptr{Cvoid}, Ptr{Int64}, Ptr{Int32}, Ptr{Cvoid}),
                device, counts, S, K, n, which - 1, start, B, ld, max_sweeps, labels, moves, sweeps, stream))
    return moves, sweeps
end

# ---- consensus_map (consensus_map.jl:125-196): block sums of the PSMs over a grouping (pmdi_psm_blocksum_device; not executed, as above) ----
# group: host Int32 group numbers 0..G-1, one per observation -- the pixel bins of hc.order, `group[hc.order] .= (0:n-1) .* H .÷ n`,
# or cluster labels .- 1; out: device pointer to Int64 [M][G][G], M = K + (K > 1), filled.  Returns the M divisors: the map of
# matrix m is out[m] ./ (D[m] .* (rows x columns of every pixel)).  Synchronises.
const BLOCKSUM_GMAX = 2048
function psm_blocksum_device(counts::Ptr{Cvoid}, S::Integer, K::Integer, n::Integer, group::Vector{Int32}, G::Integer, out::Ptr{Cvoid};
                             device::Integer = 0, stream::Ptr{Cvoid} = C_NULL)
    check(ccall((:pmdi_psm_blocksum_device, LIB), Cint,
                (Int32, Ptr{Cvoid}, Int64, Int32, Int64, Ptr{Int32}, Int32, Ptr{Cvoid}, Ptr{Cvoid}),
                device, counts, S, K, n, group, G, out, stream))
    return K > 1 ? vcat(fill(Int64(S), K), Int64(S) * K) : [Int64(S)]
end

# ---- plot_pmdi_data (feature_select_plots.jl:27-166): sums of a data matrix over a grouping of its rows (pmdi_data_groupsum_device;
# not executed, as above) ----
# x: device pointer to the ROW-MAJOR n x D matrix (element (i, d) at x[i * ld + d]: a Julia matrix transposed once), Float64 for
# kind = GaussianCluster, Int64 otherwise; group as above; mode: DATA_RAW, DATA_SQDEV (shift), DATA_ZBIN (shift, scale) or DATA_LEVELS
# (L); out: device pointer to Float64 or Int64 [G][D], or Int32 [G][D][L], filled.  Synchronises.
const DATA_RAW, DATA_SQDEV, DATA_ZBIN, DATA_LEVELS = Int32(0), Int32(1), Int32(2), Int32(3)
function data_groupsum_device(kind::Integer, x::Ptr{Cvoid}, n::Integer, D::Integer, group::Vector{Int32}, G::Integer, mode::Integer,
                              out::Ptr{Cvoid}; ld::Integer = D, shift::Union{Vector{Float64}, Nothing} = nothing,
                              scale::Union{Vector{Float64}, Nothing} = nothing, L::Integer = 0, device::Integer = 0,
                              stream::Ptr{Cvoid} = C_NULL)
    check(ccall((:pmdi_data_groupsum_device, LIB), Cint,
                (Int32, Int32, Ptr{Cvoid}, Int64, Int32, Int64, Ptr{Int32}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Cvoid}, Ptr{Cvoid}),
                device, kind, x, n, D, ld, group, G, mode, shift === nothing ? C_NULL : shift, scale === nothing ? C_NULL : scale, L, out, stream))
    return nothing
end

# ---- the cluster plugin protocol on the device (unit-level entry points) ----------------------
# calc_logprob / cluster_add! / calc_logmarginal for a batch of stand-alone clusters of dataset k;
# see pmdi_clusters_new, pmdi_cluster_add, pmdi_calc_logprob, pmdi_calc_logmarginal in the header.
function clusters_new(h::Ptr{Cvoid}, k::Integer, B::Integer)
    cb = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:pmdi_clusters_new, LIB), Cint, (Ptr{Cvoid}, Int32, Int32, Ref{Ptr{Cvoid}}), h, k - 1, B, cb))
    return cb[]
end
cluster_add!(cb::Ptr{Cvoid}, rows::Vector{Int64}, featureFlag::Vector{UInt8}) =
    check(ccall((:pmdi_cluster_add, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{UInt8}), cb, rows, featureFlag))
function calc_logprob(cb::Ptr{Cvoid}, rows::Vector{Int64}, featureFlag::Vector{UInt8})
    out = Vector{Float64}(undef, length(rows))
    check(ccall((:pmdi_calc_logprob, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{UInt8}, Ptr{Float64}), cb, rows, featureFlag, out))
    return out
end

end # module
