# Julia ccall shim over libsmlu.so.  No Julia in the image: tests/test_julia_shim.py checks it
# statically against include/smlu.h (struct layout, constructor arity, every ccall'd symbol and
# its argument count).  See INTEGRATION.md.
module SharedMemSparseLU

export ParallelSparseLU, cleanup_ParallelSparseLU!, allocate_shared, gmres!, ldiv_refined!
export lowrank!, lowrank_clear!, ldiv_lowrank!

using LinearAlgebra, SparseArrays, Libdl
import LinearAlgebra: ldiv!, lu!
import MPI                                     # declared by the reference (Project.toml:8)

const libsmlu = get(ENV, "SMLU_LIB", joinpath(@__DIR__, "..", "deps", "libsmlu.so"))

# entry point chosen at run time (ccall's literal (name, lib) form needs a constant name)
fnptr(name::Symbol) = Libdl.dlsym(Libdl.dlopen(libsmlu), name)

# must match `smlu_opts` in include/smlu.h field for field
mutable struct SmluOpts
    chunk_size::Int64; index_base::Int32; ordering::Int32; grid::NTuple{3,Int64}
    scale::Int32; relax::Int32; pivot_tol::Float64; diag_pivot_tol::Float64
    device::Int32; profile::Int32; leaf_size::Int64; use_mfma::Int32; refine::Int32; vendor_gemm::Int32
end
function default_opts()
    o = SmluOpts(0, 0, 0, (0, 0, 0), 0, 0, 0.0, 0.0, 0, 0, 0, 0, 0, 0)
    ccall((:smlu_default_opts, libsmlu), Cvoid, (Ref{SmluOpts},), o)
    return o                                   # index_base = 1: Julia's 1-based CSC as is
end

struct SmluError <: Exception; code::Int32; msg::String; end
function check(rc, h)
    rc == 0 && return
    msg = unsafe_string(ccall((:smlu_last_error_string, libsmlu), Cstring, (Ptr{Cvoid},), h))
    if rc == 1                                 # SMLU_SINGULAR, as UMFPACK's check=true
        col = ccall((:smlu_last_error_col, libsmlu), Int64, (Ptr{Cvoid},), h)
        throw(SingularException(col + 1))
    end
    rc < 0 && throw(SmluError(rc, msg))
end

mutable struct ParallelSparseLU{Tf,Ti}
    m::Ti; n::Ti
    handle::Ptr{Cvoid}
    colptr::Vector{Ti}; rowval::Vector{Ti}
    chunk_size::Ti
end

# Tf in (Float64, ComplexF64), Ti in (Int64, Int32): the reference is generic in both
# (src/SharedMemSparseLU.jl:43, :64; SURVEY §8f-4).  Int32 indices go through smlu_create_i32
# (real) or are widened here (complex); complex values go through smlu_create_z as interleaved
# (re, im) doubles -- the memory layout of Vector{ComplexF64}.
const SmluFloat = Union{Float64,ComplexF64}
const SmluInt = Union{Int64,Int32}

function ParallelSparseLU(A::SparseMatrixCSC{Tf,Ti}, chunk_size=nothing) where {Tf<:SmluFloat,Ti<:SmluInt}
    chunk_size = min(something(chunk_size, 8), A.n)           # :67-72
    o = default_opts(); o.chunk_size = chunk_size
    h = Ref{Ptr{Cvoid}}(C_NULL)
    if Tf === ComplexF64
        rc = ccall((:smlu_create_z, libsmlu), Int32,
                   (Int64, Ptr{Int64}, Ptr{Int64}, Ptr{ComplexF64}, Ref{SmluOpts}, Ref{Ptr{Cvoid}}),
                   A.n, Vector{Int64}(A.colptr), Vector{Int64}(A.rowval), A.nzval, o, h)
    elseif Ti === Int32
        rc = ccall((:smlu_create_i32, libsmlu), Int32,
                   (Int64, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ref{SmluOpts}, Ref{Ptr{Cvoid}}),
                   A.n, A.colptr, A.rowval, A.nzval, o, h)
    else
        rc = ccall((:smlu_create, libsmlu), Int32,
                   (Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ref{SmluOpts}, Ref{Ptr{Cvoid}}),
                   A.n, A.colptr, A.rowval, A.nzval, o, h)
    end
    if rc == 1 && h[] != C_NULL                   # singular: free the handle, then throw
        col = ccall((:smlu_last_error_col, libsmlu), Int64, (Ptr{Cvoid},), h[])
        ccall((:smlu_destroy, libsmlu), Cvoid, (Ptr{Cvoid},), h[])
        throw(SingularException(col + 1))
    end
    check(rc, h[])
    F = ParallelSparseLU{Tf,Ti}(A.m, A.n, h[], copy(A.colptr), copy(A.rowval), chunk_size)
    finalizer(cleanup_ParallelSparseLU!, F)
    return F
end

# Optional: hand UMFPACK's own analysis over so that pivot order and L/U pattern match it by
# construction (SURVEY §8f-1, §8(b)): the reference's lu(A) (:74) and its L, U, p, q, Rs
# extraction (:75-77, :93-94).  The library checks the pattern against the structural fill of
# (Rs.*A)[p, q] and exports F.L / F.U on exactly that pattern.
function ParallelSparseLU_umfpack(A::SparseMatrixCSC{Float64,Ti}, chunk_size=nothing) where {Ti<:SmluInt}
    U = lu(A)
    FL = U.L; FU = U.U
    o = default_opts(); o.chunk_size = min(something(chunk_size, 8), A.n); h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:smlu_create_with_pivots, libsmlu), Int32,
               (Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}, Ptr{Int64},
                Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ref{SmluOpts}, Ref{Ptr{Cvoid}}),
               A.n, Vector{Int64}(A.colptr), Vector{Int64}(A.rowval), A.nzval,
               Vector{Int64}(U.p), Vector{Int64}(U.q), U.Rs,
               Vector{Int64}(FL.colptr), Vector{Int64}(FL.rowval),
               Vector{Int64}(FU.colptr), Vector{Int64}(FU.rowval), o, h)
    check(rc, h[])
    F = ParallelSparseLU{Float64,Ti}(A.m, A.n, h[], copy(A.colptr), copy(A.rowval), o.chunk_size)
    finalizer(cleanup_ParallelSparseLU!, F)
    return F
end

# One process per GPU (the rank split the reference only sketches, :107, :128; MPI is its declared
# dependency, Project.toml:8).  Collective over `comm`: rank 0 creates the RCCL unique id, MPI
# broadcasts the 128 bytes, every rank builds its part of the partition on its node-local GPU and
# the library moves the blocks itself over RCCL/xGMI.  lu! and ldiv! below are then collective too
# (every rank calls them with the same values / right-hand side; x comes back complete everywhere).
function ParallelSparseLU(A::SparseMatrixCSC{Float64,Int64}, comm::MPI.Comm, chunk_size=nothing)
    rank = MPI.Comm_rank(comm); nranks = MPI.Comm_size(comm)
    id = zeros(UInt8, 128)
    rank == 0 && check(ccall((:smlu_rccl_unique_id, libsmlu), Int32, (Ptr{UInt8},), id), C_NULL)
    MPI.Bcast!(id, 0, comm)
    o = default_opts(); o.chunk_size = min(something(chunk_size, 8), A.n)
    o.device = MPI.Comm_rank(MPI.Comm_split_type(comm, MPI.COMM_TYPE_SHARED, rank))   # node-local GPU
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:smlu_dist_create_rccl, libsmlu), Int32,
               (Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ref{SmluOpts}, Int32, Int32, Ptr{UInt8},
                Ref{Ptr{Cvoid}}),
               A.n, A.colptr, A.rowval, A.nzval, o, rank, nranks, id, h)
    check(rc, h[])
    F = ParallelSparseLU{Float64,Int64}(A.m, A.n, h[], copy(A.colptr), copy(A.rowval), o.chunk_size)
    finalizer(cleanup_ParallelSparseLU!, F)
    return F
end

function lu!(F::ParallelSparseLU{Tf,Ti}, A::SparseMatrixCSC{Tf,Ti}) where {Tf,Ti}   # :245-279
    z = Tf === ComplexF64
    if A.colptr == F.colptr && A.rowval == F.rowval
        rc = ccall(fnptr(z ? :smlu_refactor_z : :smlu_refactor), Int32, (Ptr{Cvoid}, Ptr{Tf}),
                   F.handle, A.nzval)
    else                                                                          # :265-273
        rc = ccall(fnptr(z ? :smlu_refactor_csc_z : :smlu_refactor_csc), Int32,
                   (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Tf}),
                   F.handle, A.n, Vector{Int64}(A.colptr), Vector{Int64}(A.rowval), A.nzval)
        F.colptr = copy(A.colptr); F.rowval = copy(A.rowval)
    end
    check(rc, F.handle)
    return nothing
end

function ldiv!(x::AbstractVecOrMat, F::ParallelSparseLU{Tf}, b::AbstractVecOrMat) where {Tf}   # :286-342
    @boundscheck F.m == F.n || throw(DimensionMismatch("`F` is not square: F.m=$(F.m), F.n=$(F.n)"))
    @boundscheck size(x, 1) == F.n || throw(DimensionMismatch("`x` does not have same size as F: length(x)=$(length(x)), F.n=$(F.n)"))
    @boundscheck size(b, 1) == F.n || throw(DimensionMismatch("`b` does not have same size as F: length(b)=$(length(b)), F.n=$(F.n)"))
    bb = b isa Array{Tf} ? b : Array{Tf}(b)
    xx = x isa Array{Tf} ? x : similar(bb)
    if ndims(b) == 1
        check(ccall((:smlu_solve, libsmlu), Int32, (Ptr{Cvoid}, Ptr{Tf}, Ptr{Tf}), F.handle, bb, xx), F.handle)
    else                                       # several right-hand sides: one batched call
        ld = (Tf === ComplexF64 ? 2 : 1) * F.n  # leading dimension in doubles
        check(ccall((:smlu_solve_multi, libsmlu), Int32,
                    (Ptr{Cvoid}, Int64, Ptr{Tf}, Int64, Ptr{Tf}, Int64),
                    F.handle, size(b, 2), bb, ld, xx, ld), F.handle)
    end
    xx === x || copyto!(x, xx)
    return x
end

# transpose(F) \ b and F' \ b from the same factors (UMFPACK_At / UMFPACK_Aat): thin wrappers, no
# second analysis or factorization.  op: SMLU_OP_T = 1, SMLU_OP_H = 2 (include/smlu.h).
struct TransposedLU{Tf,Ti}; parent::ParallelSparseLU{Tf,Ti}; end
struct AdjointLU{Tf,Ti}; parent::ParallelSparseLU{Tf,Ti}; end
Base.transpose(F::ParallelSparseLU{Tf,Ti}) where {Tf,Ti} = TransposedLU{Tf,Ti}(F)
Base.adjoint(F::ParallelSparseLU{Tf,Ti}) where {Tf,Ti} = AdjointLU{Tf,Ti}(F)
Base.transpose(W::TransposedLU) = W.parent
Base.adjoint(W::AdjointLU) = W.parent

function _ldiv_trans!(op::Int32, x::AbstractVecOrMat, F::ParallelSparseLU{Tf}, b::AbstractVecOrMat) where {Tf}
    F.m == F.n || throw(DimensionMismatch("`F` is not square: F.m=$(F.m), F.n=$(F.n)"))
    size(x, 1) == F.n || throw(DimensionMismatch("`x` does not have same size as F: length(x)=$(length(x)), F.n=$(F.n)"))
    size(b, 1) == F.n || throw(DimensionMismatch("`b` does not have same size as F: length(b)=$(length(b)), F.n=$(F.n)"))
    bb = b isa Array{Tf} ? b : Array{Tf}(b)
    xx = x isa Array{Tf} ? x : similar(bb)
    if ndims(b) == 1
        check(ccall((:smlu_solve_trans, libsmlu), Int32, (Ptr{Cvoid}, Int32, Ptr{Tf}, Ptr{Tf}),
                    F.handle, op, bb, xx), F.handle)
    else                                       # several right-hand sides: batches of 16 in the library
        ld = (Tf === ComplexF64 ? 2 : 1) * F.n  # leading dimension in doubles
        check(ccall((:smlu_solve_trans_multi, libsmlu), Int32,
                    (Ptr{Cvoid}, Int32, Int64, Ptr{Tf}, Int64, Ptr{Tf}, Int64),
                    F.handle, op, size(b, 2), bb, ld, xx, ld), F.handle)
    end
    xx === x || copyto!(x, xx)
    return x
end
ldiv!(x::AbstractVecOrMat, W::TransposedLU, b::AbstractVecOrMat) = _ldiv_trans!(Int32(1), x, W.parent, b)
ldiv!(x::AbstractVecOrMat, W::AdjointLU, b::AbstractVecOrMat) = _ldiv_trans!(Int32(2), x, W.parent, b)

# ldiv_refined!(X, F, B; steps=-1), also on transpose(F) and F': the columns of B solved with iterative
# refinement run as a batch (smlu_solve_refined_multi): up to 16 columns share every pass over the
# factors and every residual pass over A, each column is refined by the rule of the single solve and
# is bitwise ldiv!(x, F, b) of that column.  steps = -1: the handle's own rule; 0: a plain batch;
# k > 0: up to k corrections per column.  Returns (steps, berr), one entry per column: the corrections
# applied and the last componentwise backward error measured (-1 when nothing was refined).
# RefineInfo must match the header's refinement record field for field.
struct RefineInfo; steps::Int32; stop::Int32; berr::Float64; resid::Float64; end
function _ldiv_refined!(op::Int32, X::AbstractMatrix, F::ParallelSparseLU{Tf}, B::AbstractMatrix, steps::Integer) where {Tf}
    F.m == F.n || throw(DimensionMismatch("`F` is not square: F.m=$(F.m), F.n=$(F.n)"))
    size(X) == size(B) || throw(DimensionMismatch("`X` has size $(size(X)), `B` has size $(size(B))"))
    size(B, 1) == F.n || throw(DimensionMismatch("`B` does not have same size as F: size(B, 1)=$(size(B, 1)), F.n=$(F.n)"))
    steps >= -1 || throw(ArgumentError("ldiv_refined!: steps must be -1, 0 or a step limit, got $steps"))
    bb = B isa Array{Tf} ? B : Array{Tf}(B)
    xx = X isa Array{Tf} ? X : similar(bb)
    info = Vector{RefineInfo}(undef, size(B, 2))
    ld = (Tf === ComplexF64 ? 2 : 1) * F.n      # leading dimension in doubles
    check(ccall((:smlu_solve_refined_multi, libsmlu), Int32,
                (Ptr{Cvoid}, Int32, Int32, Int64, Ptr{Tf}, Int64, Ptr{Tf}, Int64, Ptr{RefineInfo}),
                F.handle, op, Int32(steps), size(B, 2), bb, ld, xx, ld, info), F.handle)
    xx === X || copyto!(X, xx)
    return [i.steps for i in info], [i.berr for i in info]
end
ldiv_refined!(X::AbstractMatrix, F::ParallelSparseLU, B::AbstractMatrix; steps::Integer=-1) =
    _ldiv_refined!(Int32(0), X, F, B, steps)
ldiv_refined!(X::AbstractMatrix, W::TransposedLU, B::AbstractMatrix; steps::Integer=-1) =
    _ldiv_refined!(Int32(1), X, W.parent, B, steps)
ldiv_refined!(X::AbstractMatrix, W::AdjointLU, B::AbstractMatrix; steps::Integer=-1) =
    _ldiv_refined!(Int32(2), X, W.parent, B, steps)

# logabsdet(F), logdet(F), det(F) and cond(F, p) from the factors on the GPU (smlu_logabsdet*,
# smlu_rcond): no factor download.  The sign of a ComplexF64 factorization is its phase.
function LinearAlgebra.logabsdet(F::ParallelSparseLU{Tf}) where {Tf}
    la = Ref{Float64}(0.0)
    if Tf === ComplexF64
        ph = zeros(Float64, 2)
        check(ccall((:smlu_logabsdet_z, libsmlu), Int32, (Ptr{Cvoid}, Ref{Float64}, Ptr{Float64}),
                    F.handle, la, ph), F.handle)
        return la[], complex(ph[1], ph[2])
    end
    sg = Ref{Float64}(0.0)
    check(ccall((:smlu_logabsdet, libsmlu), Int32, (Ptr{Cvoid}, Ref{Float64}, Ref{Float64}),
                F.handle, la, sg), F.handle)
    return la[], sg[]
end
function LinearAlgebra.logdet(F::ParallelSparseLU{Tf}) where {Tf}
    la, sg = logabsdet(F)
    Tf === ComplexF64 && return complex(la, angle(sg))
    sg < 0 && throw(DomainError(sg, "determinant is negative: use logabsdet"))
    return la
end
function LinearAlgebra.det(F::ParallelSparseLU)
    la, sg = logabsdet(F)
    return sg * exp(la)
end
# cond(F, 1) / cond(F, Inf): ||A|| est||A^-1|| (LAPACK's dgecon / zgecon estimator); SMLU_NORM_ONE = 1,
# SMLU_NORM_INF = 2 (include/smlu.h).  No default p: LinearAlgebra's cond(A) is the 2-norm, which the
# factors do not give.
function LinearAlgebra.cond(F::ParallelSparseLU, p::Real)
    p == 1 || p == Inf || throw(ArgumentError("cond(F, p): p must be 1 or Inf, got $p"))
    r = Ref{Float64}(0.0)
    check(ccall((:smlu_rcond, libsmlu), Int32, (Ptr{Cvoid}, Int32, Ref{Float64}, Ptr{Float64}, Ptr{Float64}),
                F.handle, Int32(p == 1 ? 1 : 2), r, C_NULL, C_NULL), F.handle)
    return r[] == 0 ? Inf : inv(r[])
end

# gmres!(x, F, A, b): solve A x = b with the factors F already holds, when A's values have moved a
# little since lu!(F, .): restarted GMRES preconditioned by those factors, all on the GPU
# (smlu_solve_gmres; PARDISO's "iterate with the previous factorization").  A must have F's pattern;
# A = nothing takes the values F factored (GMRES-based refinement).  Returns (x, info); a run that
# stops short of rtol (status 3) does not throw: info.converged == 0 and x is the last iterate.
# The two structs must match the header's GMRES option and result records field for field.
mutable struct GmresOpts; rtol::Float64; restart::Int32; maxit::Int32; end
mutable struct GmresInfo
    converged::Int32; iters::Int32; cycles::Int32; solves::Int32
    relres::Float64; relres_est::Float64; berr::Float64; bnorm::Float64
end
function gmres!(x::AbstractVector, F::ParallelSparseLU{Float64}, A::Union{SparseMatrixCSC{Float64},Nothing},
                b::AbstractVector; rtol=1e-10, restart=30, maxiter=200)
    length(x) == length(b) == F.n || throw(DimensionMismatch("x, b and F sizes differ"))
    A === nothing || (A.colptr == F.colptr && A.rowval == F.rowval) ||
        throw(ArgumentError("gmres!: A must have the sparsity pattern F was created with"))
    o = GmresOpts(rtol, restart, maxiter)
    info = GmresInfo(0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0)
    bb = b isa Vector{Float64} ? b : Vector{Float64}(b)
    xx = x isa Vector{Float64} ? x : similar(bb)
    rc = ccall((:smlu_solve_gmres, libsmlu), Int32,
               (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{GmresOpts}, Ref{GmresInfo}),
               F.handle, Int32(0), A === nothing ? C_NULL : A.nzval, bb, xx, o, info)
    rc < 0 && check(rc, F.handle)
    xx === x || copyto!(x, xx)
    return x, info
end

# lowrank!(F, U, V): install the update A + U V' on the factors F already holds, U and V dense n x k,
# k <= 32 (smlu_lowrank_set; the Sherman-Morrison-Woodbury identity): for a matrix that changed by any
# amount in a few columns or rows, or a few dense rows or columns kept out of the pattern.  Returns
# info (rcond_c, pivot_min and gram_max of the capacitance matrix); a singular one (status 1) throws
# SingularException(0) and installs nothing.  lu!(F, .) drops the update.
# ldiv_lowrank!(x, F, b; steps=-1), also on transpose(F) and F': solve (A + U V') x = b, refined on the
# updated system (steps = -1: up to 3 corrections; 0: none).  Returns (x, info).
# LowrankInfo must match the header's low-rank record field for field.
mutable struct LowrankInfo
    k::Int32; steps::Int32; stop::Int32; solves::Int32
    berr::Float64; resid::Float64; rcond_c::Float64; pivot_min::Float64; gram_max::Float64
end
LowrankInfo() = LowrankInfo(0, 0, 0, 0, -1.0, -1.0, -1.0, -1.0, -1.0)
function lowrank!(F::ParallelSparseLU{Float64}, U::AbstractVecOrMat, V::AbstractVecOrMat)
    size(U) == size(V) || throw(DimensionMismatch("`U` has size $(size(U)), `V` has size $(size(V))"))
    size(U, 1) == F.n || throw(DimensionMismatch("`U` does not have same size as F: size(U, 1)=$(size(U, 1)), F.n=$(F.n)"))
    size(U, 2) <= 32 || throw(ArgumentError("lowrank!: the rank of an update is at most 32, got $(size(U, 2))"))
    uu = U isa Array{Float64} ? U : Array{Float64}(U)
    vv = V isa Array{Float64} ? V : Array{Float64}(V)
    info = LowrankInfo()
    rc = ccall((:smlu_lowrank_set, libsmlu), Int32,
               (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Ref{LowrankInfo}),
               F.handle, Int32(size(U, 2)), uu, Int64(F.n), vv, Int64(F.n), info)
    rc < 0 && check(rc, F.handle)
    rc == 1 && throw(SingularException(0))
    return info
end
lowrank_clear!(F::ParallelSparseLU) = (check(ccall((:smlu_lowrank_clear, libsmlu), Int32, (Ptr{Cvoid},), F.handle), F.handle); nothing)
function _ldiv_lowrank!(op::Int32, x::AbstractVector, F::ParallelSparseLU{Float64}, b::AbstractVector, steps::Integer)
    length(x) == length(b) == F.n || throw(DimensionMismatch("x, b and F sizes differ"))
    steps >= -1 || throw(ArgumentError("ldiv_lowrank!: steps must be -1, 0 or a step limit, got $steps"))
    bb = b isa Vector{Float64} ? b : Vector{Float64}(b)
    xx = x isa Vector{Float64} ? x : similar(bb)
    info = LowrankInfo()
    check(ccall((:smlu_solve_lowrank, libsmlu), Int32,
                (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ref{LowrankInfo}),
                F.handle, op, Int32(steps), bb, xx, info), F.handle)
    xx === x || copyto!(x, xx)
    return x, info
end
ldiv_lowrank!(x::AbstractVector, F::ParallelSparseLU, b::AbstractVector; steps::Integer=-1) =
    _ldiv_lowrank!(Int32(0), x, F, b, steps)
ldiv_lowrank!(x::AbstractVector, W::TransposedLU, b::AbstractVector; steps::Integer=-1) =
    _ldiv_lowrank!(Int32(1), x, W.parent, b, steps)
ldiv_lowrank!(x::AbstractVector, W::AdjointLU, b::AbstractVector; steps::Integer=-1) =
    _ldiv_lowrank!(Int32(2), x, W.parent, b, steps)

function _trisolve!(upper::Bool, F::ParallelSparseLU{Tf}, x::AbstractVector) where {Tf}
    xx = x isa Vector{Tf} ? x : Vector{Tf}(x)
    check(ccall(fnptr(upper ? :smlu_rsolve : :smlu_lsolve), Int32, (Ptr{Cvoid}, Ptr{Tf}), F.handle, xx),
          F.handle)
    xx === x || copyto!(x, xx)
    return nothing
end
lsolve!(F::ParallelSparseLU, x) = _trisolve!(false, F, x)                          # :349
rsolve!(F::ParallelSparseLU, x) = _trisolve!(true, F, x)                           # :374

# Optional parity mode: the reference's own dense-chunk layout (:101-243) on the GPU, refilled
# after each lu! (:265-276); ldiv! through it runs lsolve!/rsolve! chunk by chunk (:349-392).
chunked_setup!(F::ParallelSparseLU) = check(ccall((:smlu_chunked_setup, libsmlu), Int32,
    (Ptr{Cvoid}, Int64), F.handle, F.chunk_size), F.handle)
function chunked_ldiv!(x::AbstractVector, F::ParallelSparseLU{Tf}, b::AbstractVector) where {Tf}
    length(x) == length(b) == F.n || throw(DimensionMismatch("x, b and F sizes differ"))
    bb = Vector{Tf}(b); xx = Vector{Tf}(undef, F.n)
    check(ccall((:smlu_chunked_ldiv, libsmlu), Int32, (Ptr{Cvoid}, Ptr{Tf}, Ptr{Tf}),
                F.handle, bb, xx), F.handle)
    copyto!(x, xx)
end

function Base.getproperty(F::ParallelSparseLU{Tf,Ti}, s::Symbol) where {Tf,Ti}     # :45-52
    s in (:L, :U, :p, :q, :Rs) || return getfield(F, s)
    h = getfield(F, :handle)
    n = Int64(getfield(F, :n)); nl = Ref{Int64}(0); nu = Ref{Int64}(0)
    # ComplexF64: the complex factors, folded from the real-equivalent ones (smlu_get_factors_z)
    z = Tf === ComplexF64
    check(ccall(fnptr(z ? :smlu_get_sizes_z : :smlu_get_sizes), Int32,
                (Ptr{Cvoid}, Ptr{Int64}, Ref{Int64}, Ref{Int64}), h, C_NULL, nl, nu), h)
    Lp = Vector{Int64}(undef, n + 1); Li = Vector{Int64}(undef, nl[]); Lx = Vector{Tf}(undef, nl[])
    Up = Vector{Int64}(undef, n + 1); Ui = Vector{Int64}(undef, nu[]); Ux = Vector{Tf}(undef, nu[])
    p = Vector{Int64}(undef, n); q = Vector{Int64}(undef, n); Rs = Vector{Float64}(undef, n)
    check(ccall(fnptr(z ? :smlu_get_factors_z : :smlu_get_factors), Int32,
                (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ptr{Tf}, Ptr{Int64}, Ptr{Int64},
                 Ptr{Tf}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}),
                h, Lp, Li, Lx, Up, Ui, Ux, p, q, Rs), h)
    s === :L && return SparseMatrixCSC{Tf,Ti}(n, n, Vector{Ti}(Lp), Vector{Ti}(Li), Lx)   # L::SparseMatrixCSC{Tf,Ti}
    s === :U && return SparseMatrixCSC{Tf,Ti}(n, n, Vector{Ti}(Up), Vector{Ti}(Ui), Ux)
    s === :p && return Vector{Ti}(p)           # p::Vector{Ti}, q::Vector{Ti} as the reference (:49-50)
    s === :q && return Vector{Ti}(q)
    return Rs
end

function cleanup_ParallelSparseLU!(F::ParallelSparseLU)                             # :31
    h = getfield(F, :handle)
    h == C_NULL || ccall((:smlu_destroy, libsmlu), Cvoid, (Ptr{Cvoid},), h)
    setfield!(F, :handle, C_NULL)
    return nothing
end

allocate_shared(T, dims...) = zeros(T, dims...)   # exported but undefined in the reference

end
