/*
 * smlu.h — C-ABI of libsmlu.so, the MI355X-native (gfx950) sparse LU refactorize/solve
 * library that is a drop-in for the hot path of SharedMemSparseLU.jl
 * (reference snapshot 2024-10-20, /root/reference).
 *
 * Every entry point below names the reference interface it replaces (file:line in
 * /root/reference).  Plain C types only: int64_t indices, double values, opaque handles.
 *
 * Conventions
 *   - Matrices cross the boundary in CSC form (colptr[n+1], rowval[nnz], nzval[nnz]),
 *     1-based by default (Julia's SparseMatrixCSC{Float64,Int64}); set
 *     smlu_opts.index_base = 0 for 0-based (scipy / C) callers.
 *   - Host arrays are borrowed for the duration of the call only; the library copies
 *     what it needs and owns all device memory and one HIP stream per handle.
 *   - Status: 0 = SMLU_OK; positive = numerical status (singular / weak pivot);
 *     negative = usage, allocation or HIP errors.  smlu_last_error_string() explains.
 *   - Thread-compatible: distinct handles may be used concurrently; calls on one handle
 *     must be serialised (the reference's `wrk` vector is likewise shared per factor,
 *     src/SharedMemSparseLU.jl:318).
 */
#ifndef SMLU_H
#define SMLU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* libsmlu.so is built with -fvisibility=hidden: exactly the functions declared here are exported */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* ---- status codes ---------------------------------------------------------------- */
#define SMLU_OK                 0
#define SMLU_SINGULAR           1   /* zero pivot column (UMFPACK SingularException, src/SharedMemSparseLU.jl:74) */
#define SMLU_PIVOT_WEAK         2   /* a pivot failed the threshold test (growth > 1/pivot_tol) */
#define SMLU_NOT_CONVERGED      3   /* smlu_solve_gmres*: stopped short of rtol; x holds the last iterate */
#define SMLU_ERR_ARG          (-1)  /* bad argument / DimensionMismatch (src/SharedMemSparseLU.jl:288-290) */
#define SMLU_ERR_PATTERN      (-2)  /* refactor called with a different sparsity pattern, or a given L/U
                                       pattern outside the structural fill of (Rs.*A)[p,q] */
#define SMLU_ERR_ALLOC        (-3)  /* host or device allocation failed */
#define SMLU_ERR_HIP          (-4)  /* HIP runtime error */
#define SMLU_ERR_NODEVICE     (-5)  /* no gfx950 device visible: the library never falls back to the CPU */
#define SMLU_ERR_STATE        (-6)  /* handle has no numeric factorization / illegal device status */

/* ---- ordering choices ------------------------------------------------------------- */
#define SMLU_ORDER_AUTO         0   /* geometric ND if grid[] given, else graph nested dissection */
#define SMLU_ORDER_NATURAL      1
#define SMLU_ORDER_GEOMETRIC_ND 2   /* needs grid[0..2]: vertex v = i + nx*(j + ny*k) */
#define SMLU_ORDER_GRAPH_ND     3   /* BFS level-structure nested dissection on A+A' */
#define SMLU_ORDER_GIVEN        4   /* use smlu_create_with_pivots' p and q unchanged */
#define SMLU_ORDER_AMD          5   /* approximate minimum degree on A+A' (UMFPACK's symmetric-strategy kind) */

typedef struct smlu_opts {
    int64_t chunk_size;   /* reference `chunk_size` (src/SharedMemSparseLU.jl:64-72); accepted, clamped to n */
    int32_t index_base;   /* 1 (Julia, default) or 0 */
    int32_t ordering;     /* SMLU_ORDER_* */
    int64_t grid[3];      /* grid dimensions for SMLU_ORDER_GEOMETRIC_ND (0 = unset) */
    int32_t scale;        /* 1 = UMFPACK SUM row scaling Rs[i] = 1/sum_j |a_ij| (default), 0 = none */
    int32_t relax;        /* 1 = relaxed supernode amalgamation (default) */
    double  pivot_tol;    /* threshold partial pivoting tolerance (UMFPACK default 0.1) */
    double  diag_pivot_tol; /* diagonal preference: keep a_kk when |a_kk| >= diag_pivot_tol times the
                               largest candidate (default 0.001 = UMFPACK's symmetric-strategy
                               SYM_PIVOT_TOLERANCE); otherwise the largest candidate is taken */
    int32_t device;       /* HIP device ordinal (default 0) */
    int32_t profile;      /* 1 = record per-kernel-class HIP events during refactor/solve */
    int64_t leaf_size;    /* nested-dissection leaf size (default 64) */
    int32_t use_mfma;     /* 1 (default) = fp64 MFMA (v_mfma_f64_16x16x4) for the dense Schur
                             updates and the GEMM-form triangular solves; 0 = a comparison path:
                             the VALU 64x64 tile for k > 64 launches and k_step_trsm for the
                             triangular solves (results equal to rounding) */
    int32_t refine;       /* iterative-refinement steps in smlu_solve*: -1 (default) = up to 3 only
                             when the last factorization flagged weak pivots (the pivot-failure
                             fallback of the diagonal-tile pivoting); 0 = never;
                             k > 0 = up to k steps (LAPACK dgerfs' stop: componentwise backward error
                             <= 4 unit roundoffs or not halving) */
    int32_t vendor_gemm;  /* reserved, ignored (round 5 removed the vendor GEMM comparison path:
                             every GEMM runs on the hand-written MFMA tiles) */
} smlu_opts;

typedef struct smlu_handle smlu_handle;

/* Fill `opts` with the defaults listed above. */
void smlu_default_opts(smlu_opts* opts);

/* ParallelSparseLU(A, chunk_size) — src/SharedMemSparseLU.jl:64-98.
 * Host symbolic analysis (ordering, elimination tree, supernodes, level schedule), upload,
 * then the first numeric factorization on the GPU.  Returns SMLU_SINGULAR when A is
 * numerically singular (the reference's UMFPACK `lu(A)` throws SingularException). */
int smlu_create(int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval,
                const smlu_opts* opts, smlu_handle** out);

/* As smlu_create, but with the caller's row order p and column order q (1-based or 0-based
 * per opts), optionally Rs (NULL = compute) and optionally the L and U patterns (CSC colptr /
 * rowval; L with its unit diagonal first in each column, U with its diagonal last, rows
 * increasing; all four NULL = none).  Used by the Julia shim to hand over UMFPACK's own analysis
 * -- lu(A) and F.p, F.q, F.Rs, F.L, F.U, src/SharedMemSparseLU.jl:74-77, :93-94 -- so that pivot
 * order and L/U pattern match the reference by construction.  No pivoting
 * is performed on top of the given order.  A given pattern must lie inside the structural fill of
 * (Rs.*A)[p, q] (UMFPACK's may miss fill entries that came out exactly zero; smlu_stat
 * "pattern_dropped" counts them), else SMLU_ERR_PATTERN and no handle; smlu_get_factors then
 * exports exactly that pattern. */
int smlu_create_with_pivots(int64_t n, const int64_t* colptr, const int64_t* rowval,
                            const double* nzval, const int64_t* p, const int64_t* q,
                            const double* Rs, const int64_t* Lcolptr, const int64_t* Lrowval,
                            const int64_t* Ucolptr, const int64_t* Urowval, const smlu_opts* opts,
                            smlu_handle** out);

/* lu!(F, A) — src/SharedMemSparseLU.jl:245-279: numeric refactorization with the same
 * pattern, new values (nzval in A's original CSC order, host memory). */
int smlu_refactor(smlu_handle* h, const double* nzval);

/* Same, values already resident in device memory (HBM).  The pivoting mode is re-decided on the
 * new values (a dominance reduction on the device, read back with one stream synchronisation;
 * on a partitioned handle the ranks agree on it through the transport's allreduce). */
int smlu_refactor_device(smlu_handle* h, const double* d_nzval);

/* The caller's stream (a hipStream_t; NULL = the null stream, the default): every *_device
 * entry point orders its reads of caller memory after the work enqueued on that stream so far
 * (an event wait on the handle's stream, no host synchronisation), and returns with its outputs
 * complete.  Set it to the stream that produces the values / right-hand sides (the Python mirror
 * passes torch's current stream on every device call and resets it to NULL afterwards).
 * Lifetime: the handle keeps the raw stream until the next smlu_set_stream; the caller must
 * reset it (NULL) before destroying that stream.  No reference counterpart: Julia's arrays are
 * host memory. */
int smlu_set_stream(smlu_handle* h, void* stream);

/* lu!(F, A) where A's pattern may differ: re-analyses when it does (the reference's
 * `reallocate` branch, src/SharedMemSparseLU.jl:252-273). */
int smlu_refactor_csc(smlu_handle* h, int64_t n, const int64_t* colptr, const int64_t* rowval,
                      const double* nzval);

/* ldiv!(x, F, b) — src/SharedMemSparseLU.jl:286-342.  Host vectors of length n; x == b allowed. */
int smlu_solve(smlu_handle* h, const double* b, double* x);

/* Same with device pointers (x == b allowed). */
int smlu_solve_device(smlu_handle* h, const double* d_b, double* d_x);

/* r = b - A x with the handle's current A values (device pointers, length n; r may not alias
 * x or b) and its max-norm in *nrm (may be NULL).  The residual step of iterative refinement,
 * exported for callers that drive the partitioned solve (smlu_dist_*). */
int smlu_residual_device(smlu_handle* h, const double* d_x, const double* d_b, double* d_r, double* nrm);

/* ldiv! with nrhs right-hand sides: column j of B (ldb >= n) -> column j of X (ldx >= n),
 * host memory, X == B allowed.  The reference's ldiv! is generic over the vector type
 * (src/SharedMemSparseLU.jl:286); multiple RHS are SURVEY §8f-4.  "solve_passes" counts the forward
 * solve passes run on the handle so far, refinement corrections included: one per single-vector
 * solve, one per batch of up to 16 columns (the forward twin of "solve_trans_passes").
 * "solve_ms_last" after a call is the sum over the batches (columns) it ran. */
int smlu_solve_multi(smlu_handle* h, int64_t nrhs, const double* B, int64_t ldb, double* X, int64_t ldx);

/* Same with device pointers. */
int smlu_solve_multi_device(smlu_handle* h, int64_t nrhs, const double* d_B, int64_t ldb, double* d_X,
                            int64_t ldx);

/* Transposed and adjoint solves from the same factors: ldiv!(x, transpose(F), b) / ldiv!(x, F', b)
 * (UMFPACK_At / UMFPACK_Aat, SuperLU trans = 'T' / 'H').  No second analysis or factorization and
 * no extra factor memory: the factors of A are swept in the transposed direction.
 *   op = SMLU_OP_N forwards to the matching smlu_solve* entry point (bitwise its result);
 *   op = SMLU_OP_T solves A^T x = b;  op = SMLU_OP_H solves A^H x = b (a real handle: the same as T;
 *   a ComplexF64 handle: 2n interleaved doubles, as smlu_solve);  any other op: SMLU_ERR_ARG.
 * Conventions of smlu_solve*: x == b allowed, the _device forms are ordered after the caller's
 * stream (smlu_set_stream), iterative refinement by the same rule (residual b - A^T x with the
 * componentwise denominator |A^T||x| + |b|; "refine_steps" / "refine_berr"), "solve_ms_last" set.
 * Two solves of the same b are bitwise equal.  Single-GPU only: a partitioned handle (smlu_dist_*)
 * gives SMLU_ERR_STATE.  The _multi forms (ldb, ldx >= n; X == B allowed when ldb == ldx) take the
 * columns through the batched transposed kernels in batches of up to 16: each factor value is read
 * once per batch, and column j of X is bitwise smlu_solve_trans_device of column j alone.  When
 * refinement applies (see smlu_opts.refine) they run one refined transposed solve per column
 * instead.  "solve_ms_last" is the sum over the batches (columns);  "solve_trans_passes" counts the
 * transposed pass pairs (U^T then L^T) run on the handle so far, refinement corrections included:
 * one per single-vector solve, one per batch of up to 16 columns. */
#define SMLU_OP_N 0   /* A x = b   */
#define SMLU_OP_T 1   /* A^T x = b */
#define SMLU_OP_H 2   /* A^H x = b (real handle: same as T) */
int smlu_solve_trans(smlu_handle* h, int op, const double* b, double* x);
int smlu_solve_trans_device(smlu_handle* h, int op, const double* d_b, double* d_x);
int smlu_solve_trans_multi(smlu_handle* h, int op, int64_t nrhs, const double* B, int64_t ldb, double* X,
                           int64_t ldx);
int smlu_solve_trans_multi_device(smlu_handle* h, int op, int64_t nrhs, const double* d_B, int64_t ldb,
                                  double* d_X, int64_t ldx);

/* Several right-hand sides with iterative refinement, refined as a batch (dgerfs / dgsrfs refine each
 * column by its own rule; here up to 16 columns share every pass over the factors and over A).  The
 * smlu_solve_multi* / smlu_solve_trans_multi* entry points above keep refining column by column.
 *   op         SMLU_OP_N, SMLU_OP_T or SMLU_OP_H by the rules of smlu_solve_trans* (a real handle: H is
 *              T; a ComplexF64 handle: 2n interleaved doubles, ldb / ldx counted in doubles).
 *   max_steps  -1: the handle's own rule (smlu_opts.refine);  0: a plain batch, nothing refined;
 *              k > 0: up to k corrections per column;  below -1: SMLU_ERR_ARG.
 *   B, X       column j at B + j*ldb / X + j*ldx, ldb, ldx >= n;  X == B allowed when ldb == ldx.
 *   info       nrhs entries in host memory (both forms), may be NULL.
 * Checks as smlu_solve_trans_multi*: SMLU_ERR_ARG for a short leading dimension or a NULL pointer with
 * nrhs > 0, SMLU_ERR_STATE without a numeric factorization (none yet, or a singular one, as
 * smlu_logabsdet) or on a partitioned handle; nrhs = 0
 * returns SMLU_OK and touches nothing.  The _device form reads d_B after the caller's stream
 * (smlu_set_stream) and returns with d_X complete.
 * Per batch of up to 16 columns: one batched solve; then, up to the step limit, one batched residual
 * over the columns still active, one small record read by the host, the stopping rule of the single
 * refined solve applied to each column, and one batched solve of the surviving columns' residuals at
 * their own width.  A column that has stopped is not touched again.  Column j of X is bitwise what
 * smlu_solve_device / smlu_solve_trans_device gives for column j alone on a handle with the same
 * step limit, and info[j] is what "refine_steps", "refine_berr" and "refine_residual" hold after that
 * single solve (berr and resid: the last ones measured for the column; -1 when nothing was refined):
 *   stop  0 not refined;  1 berr <= 2^-51;  2 berr did not halve;  3 the step limit was reached.
 * smlu_stat: "solve_passes" / "solve_trans_passes" grow by 1 + the largest step count of each batch
 * (column by column: by the sum of 1 + steps);  "refine_batch_residuals" counts the batched residual
 * launches run on the handle so far;  "refine_steps", "refine_berr" and "refine_residual" hold the
 * largest over the call's columns, "solve_ms_last" the sum of the batches' first solves.
 * Work buffers (a stash of B, the residuals and the corrections, n x 16 doubles each, and 32 norm
 * words) belong to the handle: allocated on the first refining call, freed with the handle,
 * SMLU_ERR_ALLOC when they do not fit.  At n = 128^3 the three buffers take 0.8 GB together. */
typedef struct smlu_refine_info { int32_t steps; int32_t stop; double berr; double resid; } smlu_refine_info;
int smlu_solve_refined_multi(smlu_handle* h, int op, int max_steps, int64_t nrhs, const double* B, int64_t ldb,
                             double* X, int64_t ldx, smlu_refine_info* info);
int smlu_solve_refined_multi_device(smlu_handle* h, int op, int max_steps, int64_t nrhs, const double* d_B,
                                    int64_t ldb, double* d_X, int64_t ldx, smlu_refine_info* info);

/* logabsdet(F) / det(F) (Julia's LinearAlgebra on an lu object; umfpack_get_determinant; not in the
 * reference): log|det A| of the current factorization and its sign, from the factors on the device
 * -- the diagonal of U, Rs and the parities of the row and column orders and of every front's pivot
 * permutation -- with no factor export: a few words come back in one small copy.  *sign = +1 or -1.
 * Deterministic: two evaluations of one factorization are bitwise equal.  The result is cached per
 * factorization (smlu_stat "logabsdet_evals" counts the device evaluations so far), and every
 * refactor invalidates it.  SMLU_ERR_ARG: NULL handle or output.  SMLU_ERR_STATE: no numeric
 * factorization (none yet, or a singular one), a partitioned handle (smlu_dist_*), or a ComplexF64
 * handle (smlu_logabsdet_z). */
int smlu_logabsdet(smlu_handle* h, double* logabs, double* sign);

/* The same for a ComplexF64 handle: log|det A| and the phase det A / |det A| as (re, im), modulus 1.
 * Folded from the real-equivalent factors like smlu_get_factors_z (complex pivots
 * U_K[2k, 2k] - i U_K[2k, 2k+1], a factor i per row pair exchanged inside itself, the orders read
 * as permutations of pairs), so it needs pair-preserving pivots: SMLU_ERR_STATE when a
 * zero-free-diagonal row transversal was needed, as there, and on a real handle. */
int smlu_logabsdet_z(smlu_handle* h, double* logabs, double phase[2]);

/* Reciprocal condition estimate 1 / (||A|| * est||A^-1||) of the current factorization in the 1-norm
 * or the infinity norm (UMFPACK_RCOND, SuperLU dgscon, LAPACK dgecon / zgecon; Julia's cond(A, 1) is
 * its inverse; not in the reference).  ||A|| is exact, from the handle's device copy of the values
 * (complex handle: sums of complex moduli); est||A^-1|| is the Hager / Higham estimate as LAPACK's
 * dlacn2 / zlacn2 run it (at most 5 iterations, at most 11 solves with A and A^H), a lower bound of
 * the true norm.  It is a property of the factors: the solves are the plain factor solves, never
 * refined, whatever smlu_opts.refine says; each transposed one counts in "solve_trans_passes".  The
 * vectors stay on the device (the handle's own buffers, nothing is ordered on the caller's stream);
 * the host reads one 64-byte record per reduction.  Deterministic (bitwise) and cached per
 * factorization and norm.  *anorm / *ainvnorm (either may be NULL) receive the two factors;
 * *rcond = 1 / (anorm * ainvnorm), or 0 when either is 0.  smlu_stat: "rcond_solves" (solves run by
 * the last call, 0 for a cached answer; "rcond_solves_fwd" / "rcond_solves_adj" split them by
 * direction), "rcond_iters".  SMLU_ERR_ARG: NULL handle or rcond, unknown norm.  SMLU_ERR_STATE: no
 * numeric factorization (none yet, or a singular one), or a partitioned handle (transposed solves
 * are single-GPU). */
#define SMLU_NORM_ONE 1
#define SMLU_NORM_INF 2
int smlu_rcond(smlu_handle* h, int norm, double* rcond, double* anorm, double* ainvnorm);

/* Solve with stale factors: restarted, right-preconditioned GMRES(m) for op(A') x = b, where A' has the
 * handle's sparsity pattern and the caller's values and the preconditioner is the handle's current
 * factorization M = LU ~ op(A) (PARDISO's "iterate with the previous factorization"; what MUMPS and
 * UMFPACK users do by hand on the host; not in the reference).  A caller whose values moved a little
 * since the last smlu_refactor gets a solution to rtol without refactoring; with nzval = NULL (the
 * handle's own current values) it is GMRES-based refinement of the factored system, the stronger
 * remedy for a weak-pivot factorization than smlu_opts.refine's classical steps.
 *   op      SMLU_OP_N, SMLU_OP_T or SMLU_OP_H (a real handle: H is T); anything else: SMLU_ERR_ARG.
 *   nzval   nnz(A) doubles in A's original CSC order, as smlu_refactor[_device]; NULL: the handle's.
 *   b, x    n doubles; x == b allowed (the handle keeps its own copy of b).
 *   opts    NULL: the defaults of smlu_gmres_default_opts (rtol 1e-10, restart 30, maxit 200).
 *           restart in 1..32, maxit >= 1 (it counts Arnoldi steps), rtol finite and >= 0: else SMLU_ERR_ARG.
 *   info    may be NULL.
 * The _device form reads caller memory after the caller's stream (smlu_set_stream) and returns with x
 * complete.  All n-vectors stay on the device; the host reads one 64-byte record per iteration.
 * The algorithm is fixed, so results are reproducible (two identical calls are bitwise equal; the
 * host and device forms agree bitwise): x0 = 0; each cycle starts from the true residual
 * r = b - op(A') x, computed on the device with its 2-norm; an Arnoldi step is one plain factor solve
 * z = M^-1 v_j (never refined, whatever smlu_opts.refine says, as smlu_rcond), the product
 * w = op(A') z and classical Gram-Schmidt run twice against v_0..v_j; the Hessenberg column, the
 * Givens rotations and the residual estimate |g_{j+1}| are updated on the device.  A cycle ends when
 * the estimate is <= rtol ||b||_2, after `restart` steps, at maxit, or on a breakdown h_{j+1,j} = 0;
 * then x += M^-1 (V y), one more factor solve: info->solves == iters + cycles.  Convergence is
 * declared only on the true residual, relres = ||b - op(A') x||_2 / ||b||_2 <= rtol.  The run stops
 * with SMLU_NOT_CONVERGED (positive: x holds the last iterate, info is filled) when maxit is reached,
 * when a non-finite norm appears, or when a cycle that ended on its estimate leaves a true residual
 * above rtol that is not below half the previous cycle's (stagnation).  b = 0 gives x = 0, converged,
 * 0 iterations.
 *   info: converged (1 / 0), iters (Arnoldi steps), cycles, solves (factor solves), relres (true, of
 *   the returned x), relres_est (the last estimate / ||b||), berr (componentwise backward error
 *   max_i |r_i| / (|op(A')||x| + |b|)_i of the returned x against A'), bnorm (||b||_2).
 * The handle stays as it was: its values, factors, determinant and rcond caches and chunked layout
 * are untouched, and a later smlu_solve is bitwise what it was before.  Work buffers (restart + 1
 * basis columns of leading dimension n rounded up to even, a few n-vectors, the partials) belong to
 * the handle: allocated on first use, grown when restart grows, freed with it; SMLU_ERR_ALLOC when
 * they do not fit.  SMLU_ERR_STATE: no numeric factorization (none yet, or a singular one), a
 * partitioned handle (smlu_dist_*), or a ComplexF64 handle (out of scope: the complex Krylov process
 * on the real-equivalent factors is not implemented).  smlu_stat: "gmres_iters", "gmres_cycles",
 * "gmres_solves", "gmres_ms_last" (the last call); transposed preconditioner solves count in
 * "solve_trans_passes".  The preconditioner solves are the library's ordinary solve passes, so, as
 * after smlu_rcond, "solve_ms_last" holds the last of them and a profiling handle's "ms_solve" has
 * grown; and each of them ends in its own stream synchronisation and sweep-status read, as every
 * solve does: the one record per iteration is what the Krylov process itself adds to that. */
typedef struct smlu_gmres_opts { double rtol; int32_t restart; int32_t maxit; } smlu_gmres_opts;
typedef struct smlu_gmres_info { int32_t converged, iters, cycles, solves;
                                 double relres, relres_est, berr, bnorm; } smlu_gmres_info;
void smlu_gmres_default_opts(smlu_gmres_opts* opts);
int smlu_solve_gmres(smlu_handle* h, int op, const double* nzval, const double* b, double* x,
                     const smlu_gmres_opts* opts, smlu_gmres_info* info);
int smlu_solve_gmres_device(smlu_handle* h, int op, const double* d_nzval, const double* d_b, double* d_x,
                            const smlu_gmres_opts* opts, smlu_gmres_info* info);

/* Low-rank updates: solve op(A + U V^T) x = b from the handle's current factors of A, U and V dense
 * n x k with k <= SMLU_LOWRANK_MAX, by the Sherman-Morrison-Woodbury identity
 *   (A + U V^T)^-1 b = y0 - Y C^-1 (V^T y0),   y0 = A^-1 b,   Y = A^-1 U,   C = I + V^T Y  (k x k).
 * For a matrix that changed by any amount but only in a few columns or rows (a boundary condition
 * that flips, a few dense constraint rows kept out of the pattern, a bordered system), where GMRES on
 * the stale factors converges slowly and the only other exact route is a refactor (what MUMPS and
 * PARDISO users do by hand on the host; not in the reference).  All n-vectors stay on the device.
 *
 * smlu_lowrank_set[_device](h, k, U, ldu, V, ldv, info) installs the update: column j of U at
 * U + j*ldu, of V at V + j*ldv, ldu, ldv >= n.  U and V are copied into the handle, Y = A^-1 U is
 * computed by the plain factor solve in batches of 16 columns (never refined, whatever
 * smlu_opts.refine says, as smlu_rcond), C is formed and factored on the device by LU with partial
 * pivoting and its explicit inverse kept; the host reads one 64-byte record.  k = 0 is
 * smlu_lowrank_clear.  info (may be NULL): k, solves (factor solve passes run), rcond_c (1-norm
 * reciprocal condition of C from its explicit inverse), pivot_min (min |u_ii| of C's LU), gram_max
 * (max |(V^T Y)_ij|); the other fields are 0 / -1.  SMLU_ERR_ARG: NULL handle, k < 0,
 * k > SMLU_LOWRANK_MAX, a NULL pointer with k > 0, a leading dimension below n; a call refused for
 * its arguments or for the handle's state leaves an installed update as it was.  SMLU_SINGULAR
 * (positive): a pivot of C exactly zero, i.e. A + U V^T is singular as far as the factors can tell, or
 * a non-finite entry of C; then nothing is installed -- an earlier update is dropped as well -- and
 * the handle stays usable.  The _device form reads U and V after the caller's stream
 * (smlu_set_stream).  The handle stays as it was: a later smlu_solve* is bitwise what it was before,
 * and the determinant and rcond caches are untouched.  Every refactor (smlu_refactor*, _csc, _z*)
 * drops the installed update, because the factors are then of another matrix; the buffers are kept.
 *
 * smlu_solve_lowrank[_device](h, op, max_steps, b, x, info) solves op(A + U V^T) x = b; x == b allowed.
 *   op         SMLU_OP_N: the identity above.  SMLU_OP_T or SMLU_OP_H (a real handle: the same):
 *              op(A + U V^T) = A^T + V U^T, so y0 = A^-T b, x = y0 - Yt C^-T (U^T y0) with
 *              Yt = A^-T V, computed on the first transposed solve after a set (batches of 16) and
 *              kept; the stored C^-1 is used transposed.  Anything else: SMLU_ERR_ARG.
 *   max_steps  iterative refinement on the updated system: 0 none, m > 0 up to m corrections, -1 up
 *              to 3 (the identity is less stable than a plain solve, so refining is the default);
 *              below -1: SMLU_ERR_ARG.  A step computes r = b - op(A) x - U (V^T x) (T: V (U^T x)) and
 *              the componentwise backward error max_i |r_i| / (|op(A)||x| + |U| (|V|^T |x|) + |b|)_i on
 *              the device, and stops as the refined solve does: when berr <= 2^-51 (stop 1), when it
 *              fails to halve (stop 2), or at the step limit (stop 3); otherwise the correction is
 *              solved through the same identity and added.
 *   info       may be NULL: k (the rank in force), steps (corrections made), stop (as
 *              smlu_refine_info), solves (factor solves run: 1 + steps; the passes that compute Yt
 *              are not counted), berr and resid (max |r_i|) as last measured, -1 if never.
 * With no update installed it is the plain solve of that direction, refined by the same rule (k = 0).
 * Two identical sequences of calls are bitwise equal, and so are the host and device forms.
 * SMLU_ERR_STATE (both calls): no numeric factorization (none yet, or a singular one), a partitioned
 * handle (smlu_dist_*), or a ComplexF64 handle.  Buffers (U, V, Y, Yt after the first transposed solve:
 * k columns of leading dimension n rounded up to even; three n-vectors; the partials) belong to the
 * handle: allocated on first use, grown with k, freed with it; SMLU_ERR_ALLOC when they do not fit
 * (128^3 with k = 32: four n x 32 buffers, 2.1 GB).  smlu_stat: "lowrank_k" (rank in force),
 * "lowrank_solves", "lowrank_set_ms_last", "lowrank_ms_last" (the last call); the factor solves count
 * in "solve_passes" / "solve_trans_passes", one per batch of up to 16 columns, and "solve_ms_last"
 * holds the last of them, as after smlu_rcond. */
#define SMLU_LOWRANK_MAX 32
typedef struct smlu_lowrank_info {
  int32_t k, steps, stop, solves;        /* rank in force; corrections made; stop as smlu_refine_info; factor solves run */
  double berr, resid;                    /* last ones measured (-1: nothing measured) */
  double rcond_c, pivot_min, gram_max;   /* of C: 1-norm rcond from its explicit inverse; min |u_ii| of its LU; max |(V^T Y)_ij| */
} smlu_lowrank_info;
int smlu_lowrank_set(smlu_handle* h, int32_t k, const double* U, int64_t ldu, const double* V, int64_t ldv,
                     smlu_lowrank_info* info);
int smlu_lowrank_set_device(smlu_handle* h, int32_t k, const double* d_U, int64_t ldu, const double* d_V, int64_t ldv,
                            smlu_lowrank_info* info);
int smlu_lowrank_clear(smlu_handle* h);
int smlu_solve_lowrank(smlu_handle* h, int op, int max_steps, const double* b, double* x, smlu_lowrank_info* info);
int smlu_solve_lowrank_device(smlu_handle* h, int op, int max_steps, const double* d_b, double* d_x,
                              smlu_lowrank_info* info);

/* ParallelSparseLU(A::SparseMatrixCSC{Float64,Int32}) — Int32 index arrays;
 * converted to the Int64 path on the host. */
int smlu_create_i32(int64_t n, const int32_t* colptr, const int32_t* rowval, const double* nzval,
                    const smlu_opts* opts, smlu_handle** out);

/* ParallelSparseLU(A::SparseMatrixCSC{ComplexF64}) — the reference is generic in Tf
 * (src/SharedMemSparseLU.jl:43, :64, :286).  nzval holds 2*nnz doubles,
 * interleaved (re, im) per entry (Julia's ComplexF64 / C99 double complex layout).
 * The handle factors the real-equivalent K (2n x 2n, entry x+iy -> block [[x,-y],[y,x]] at rows
 * 2i,2i+1 / columns 2j,2j+1) on the real GPU path, so on a complex handle:
 *   - smlu_solve[_device], smlu_solve_multi[_device], smlu_residual_device, smlu_lsolve/rsolve
 *     and smlu_chunked_* take complex vectors as 2n interleaved doubles (ldb/ldx in doubles);
 *   - smlu_get_sizes / smlu_get_factors describe K's factors (n reported as 2n);
 *   - smlu_last_error_col reports the complex column;  smlu_stat(h, "complex") == 1.
 * The column order is computed on the complex pattern (opts.ordering; SMLU_ORDER_GIVEN is
 * refused) and kept pairwise, so each 2x2 block stays in one front. */
int smlu_create_z(int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval,
                  const smlu_opts* opts, smlu_handle** out);

/* lu!(F, A) for a complex handle (same pattern; host values, 2*nnz doubles interleaved). */
int smlu_refactor_z(smlu_handle* h, const double* nzval);

/* Same, complex values already in device memory (16-byte aligned); expanded into K on the GPU. */
int smlu_refactor_z_device(smlu_handle* h, const double* d_nzval);

/* lu!(F, A) for a complex handle where the pattern may differ (re-analysis, :252-273). */
int smlu_refactor_csc_z(smlu_handle* h, int64_t n, const int64_t* colptr, const int64_t* rowval,
                        const double* nzval);

/* lsolve!(F, x) — src/SharedMemSparseLU.jl:349-367: in place L \ x on an already
 * row-permuted and scaled host vector (x in the reference's F.p order). */
int smlu_lsolve(smlu_handle* h, double* x);

/* rsolve!(F, x) — src/SharedMemSparseLU.jl:374-392: in place U \ x. */
int smlu_rsolve(smlu_handle* h, double* x);

/* The reference's own dense-chunk solve layout on the GPU, a parity mode for
 * small banded systems: chunk geometry, negated rectangles and back-to-front U chunks as
 * get_chunking_parameters / allocate_chunks / fill_chunks! (src/SharedMemSparseLU.jl:101-243)
 * build them from the current factors (chunk_size <= 0: 8, as :67-70; clamped to n, :72).
 * smlu_chunked_ldiv is ldiv! (:286-342) with lsolve!/rsolve! (:349-392) done chunk by chunk
 * (trsv on the diagonal block, then x[rows] += Rect*x[cols]); x may alias b.  The chunks are
 * refilled automatically after a refactor (as lu! does, :265-276).  Refuses (SMLU_ERR_ALLOC)
 * layouts above 32 GB -- the reference's layout is dense and infeasible for large fill. */
int smlu_chunked_setup(smlu_handle* h, int64_t chunk_size);
int smlu_chunked_ldiv(smlu_handle* h, const double* b, double* x);
int smlu_chunked_ldiv_device(smlu_handle* h, const double* d_b, double* d_x);

/* Sizes for smlu_get_factors: n, nnz(L) (incl. unit diagonal), nnz(U). */
int smlu_get_sizes(smlu_handle* h, int64_t* n, int64_t* nnz_L, int64_t* nnz_U);

/* F.L, F.U, F.p, F.q, F.Rs (src/SharedMemSparseLU.jl:45-52; UMFPACK contract
 * F.L*F.U == (F.Rs .* A)[F.p, F.q], quoted at :305-316).  L: CSC, unit diagonal stored
 * first in each column, rows sorted.  U: CSC, rows sorted, diagonal last.  Indices use
 * opts.index_base.  Any pointer may be NULL to skip that output. */
int smlu_get_factors(smlu_handle* h, int64_t* Lcolptr, int64_t* Lrowval, double* Lnzval,
                     int64_t* Ucolptr, int64_t* Urowval, double* Unzval,
                     int64_t* p, int64_t* q, double* Rs);

/* The assembly tree of the handle's analysis (diagnostic: the tests' pivot-rule oracle replays
 * the GPU's pivot decisions on it).  first[nsup+1]: first column (pivot position) of each front;
 * parent[nsup] (-1: root; parents follow their children); rowptr[nsup+1] / rows[rowptr[nsup]]:
 * the update rows of each front (sorted positions); p0[n]: the row order before pivoting (new ->
 * old, 0-based: q, or q composed with the zero-free-diagonal transversal); mode[nsup]: pivot
 * candidates of the current schedule (0: small front, every fully-summed row; 1: blocked front,
 * every fully-summed row; 2: blocked front, the rows of the 64 x 64 diagonal tile).  The final row
 * order is p[k] = p0[first[s] + rowperm_s[k - first[s]]] for the pivot sequence chosen per front.
 * nsup = smlu_stat(h, "nsuper"); NULL pointers are skipped. */
int smlu_get_fronts(smlu_handle* h, int64_t* first, int64_t* parent, int64_t* rowptr, int64_t* rows,
                    int64_t* p0, int32_t* mode);

/* F.L, F.U, F.p, F.q, F.Rs of a ComplexF64 handle (src/SharedMemSparseLU.jl:47-52: L and U are
 * SparseMatrixCSC{ComplexF64}): the complex n x n factors, values as interleaved (re, im) doubles
 * (2*nnz), same conventions as smlu_get_factors (L unit diagonal first, U diagonal last, rows
 * sorted; F.L*F.U == (F.Rs .* A)[F.p, F.q]).  Folded from the real-equivalent factors: a complex
 * handle pivots K pair by pair (rows 2i, 2i+1 stay adjacent; the diagonal pair is kept when its
 * complex magnitude passes diag_pivot_tol, else the largest pair; inside a pair the larger entry
 * leads, a swap that folds back as a row rotation by -i), so the complex factors always exist
 * (SMLU_ERR_STATE only if a zero-free-diagonal row transversal was needed, which breaks pairs). */
int smlu_get_sizes_z(smlu_handle* h, int64_t* n, int64_t* nnz_L, int64_t* nnz_U);
int smlu_get_factors_z(smlu_handle* h, int64_t* Lcolptr, int64_t* Lrowval, double* Lnzval,
                       int64_t* Ucolptr, int64_t* Urowval, double* Unzval,
                       int64_t* p, int64_t* q, double* Rs);

/* cleanup_ParallelSparseLU!(F) — exported but undefined in the reference
 * (src/SharedMemSparseLU.jl:31): frees device memory, stream and host plan. */
void smlu_destroy(smlu_handle* h);

/* Diagnostics. */
const char* smlu_last_error_string(const smlu_handle* h);   /* h may be NULL: thread-global */
int64_t     smlu_last_error_col(const smlu_handle* h);      /* column of A (the caller's numbering, but 0-based
                                                               whatever index_base is) whose pivot was zero; -1 none */

/* Plan statistics (host symbolic analysis): keys are
 * "n","nnzA","nsuper","nlevels","nnzL","nnzU","nnzLU","flops","upd","front_max","ns_max",
 * "factor_bytes","scratch_bytes","launches","analysis_ms","refactor_ms_last","solve_ms_last",
 * "growth_max","dense_flops","gemm_flops","ms_gemm","ms_panel","ms_trsm","ms_assemble",
 * "ms_small","ms_solve","solve_passes","solve_trans_passes","rcond_solves","rcond_solves_fwd","rcond_solves_adj",
 * "rcond_iters","logabsdet_evals","gmres_iters","gmres_cycles","gmres_solves","gmres_ms_last",
 * "refine_steps","refine_berr","refine_residual","refine_batch_residuals",
 * "lowrank_k","lowrank_solves","lowrank_set_ms_last","lowrank_ms_last".
 * Returns NaN for an unknown key. */
double smlu_stat(const smlu_handle* h, const char* key);

/* ---- host-only symbolic analysis (no GPU needed; used by the CPU test suite) ------- */
typedef struct smlu_plan smlu_plan;
int  smlu_plan_create(int64_t n, const int64_t* colptr, const int64_t* rowval,
                      const smlu_opts* opts, smlu_plan** out);
double smlu_plan_stat(const smlu_plan* plan, const char* key);
/* Column order q (new -> old, 0-based) and the structural pattern of L (CSC, 0-based,
 * unit diagonal first) implied by the plan; NULL pointers are skipped. */
int  smlu_plan_pattern(const smlu_plan* plan, int64_t* q, int64_t* Lcolptr, int64_t* Lrowval);
/* Supernode partition: first column of each supernode (nsuper+1 entries), parent
 * supernode (-1 for roots) and level; NULL pointers are skipped. */
int  smlu_plan_supernodes(const smlu_plan* plan, int64_t* first, int64_t* parent, int64_t* level);
/* Update rows of every front (rowptr[nsup+1], rows[rowptr[nsup]], sorted positions) and the
 * row pre-order p0 (new -> old) of a host-only plan; NULL pointers are skipped. */
int  smlu_plan_fronts(const smlu_plan* plan, int64_t* rowptr, int64_t* rows, int64_t* p0);
void smlu_plan_destroy(smlu_plan* plan);

/* ---- multi-GPU partition ---------------------------------------------------
 * One process per GPU; every rank calls the same functions with the same matrix (collective).
 * The assembly tree is split by proportional mapping (each subtree set gets a contiguous rank
 * range sized by a cost model; sibling subtrees get disjoint ranges, so their shared fronts run
 * concurrently); a subtree on one rank is factored with no communication; each front above them
 * is shared by its range as a 1D block-cyclic column partition (blocks of 384 columns): the owner of a pivot
 * block factors it and broadcasts it (L block, pivots, tile inverses) to the group, every
 * member updates the column blocks it owns; the children's F22 columns move to the owners of
 * the parent's columns before its assembly.  Each rank allocates only its own fronts and
 * blocks.  Solves run the same partition (vector segments passed along the block owners, the
 * solution rows of each level shared); x comes out complete on every rank.  This replaces the
 * reference's MPI shared-memory column split (src/SharedMemSparseLU.jl:101-160, the rank split
 * intended at :107, :128).
 *
 * After creation a partitioned handle takes the ordinary entry points (smlu_refactor[_device],
 * smlu_solve[_device], smlu_solve_multi*, smlu_stat); all ranks must call them together.
 * smlu_get_factors, the chunked layout and smlu_refactor_csc are single-GPU only. */

/* Transport between the ranks, supplied by the caller (or the built-in RCCL one below).
 * device_memory = 1: buffers are device pointers ordered on `stream` (a hipStream_t), the
 * callbacks enqueue and return (RCCL); 0: host buffers, the library has synchronised its stream
 * and waits for the callback to complete (host-staged transports such as gloo / MPI).
 * exchange: for each of the npeer peers, send sbytes[i] bytes from sbuf[i] to peer[i] and
 *   receive rbytes[i] bytes from it into rbuf[i] (either may be 0); all must complete.
 * bcast: `bytes` from rank `root` to every rank of `group` (sorted, includes root).
 * allreduce_max: element-wise max of count doubles over all ranks (host memory).
 * Return 0 on success. */
typedef struct smlu_transport {
    void*   ctx;
    int32_t device_memory;
    int (*exchange)(void* ctx, int32_t npeer, const int32_t* peer, void* const* sbuf,
                    const int64_t* sbytes, void* const* rbuf, const int64_t* rbytes, void* stream);
    int (*bcast)(void* ctx, void* buf, int64_t bytes, int32_t root, int32_t gsize,
                 const int32_t* group, void* stream);
    int (*allreduce_max)(void* ctx, double* buf, int32_t count);
} smlu_transport;

/* ParallelSparseLU(A) on `nranks` GPUs (collective): analysis, this rank's allocation, the
 * first factorization.  `tr` is copied; its ctx must stay valid for the handle's life. */
int smlu_dist_create(int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval,
                     const smlu_opts* opts, int32_t rank, int32_t nranks, const smlu_transport* tr,
                     smlu_handle** out);

/* Built-in transport over RCCL (xGMI point-to-point): rank 0 calls smlu_rccl_unique_id and
 * shares the 128 bytes with the other ranks (MPI_Bcast in the Julia shim, torch.distributed in
 * the Python mirror); every rank then calls smlu_dist_create_rccl. */
int smlu_rccl_unique_id(uint8_t id[128]);
int smlu_dist_create_rccl(int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval,
                          const smlu_opts* opts, int32_t rank, int32_t nranks, const uint8_t id[128],
                          smlu_handle** out);

/* Host-only: the partition a handle of `nparts` ranks would use.  owner[s] = rank of front s,
 * -1 for a front shared by several ranks (its column blocks dealt over its group). */
int     smlu_plan_partition(const smlu_plan* plan, int32_t nparts, int32_t* owner, int64_t* nshared);
/* Host-only: device bytes rank `rank` of `nparts` allocates (factor store, scratch arena,
 * broadcast staging). */
int     smlu_plan_rank_memory(const smlu_plan* plan, int32_t nparts, int32_t rank, double* store_bytes,
                              double* scratch_bytes, double* stage_bytes);
/* Host-only: rank `rank`'s whole schedule of a `nparts`-rank handle, built by the same code as
 * smlu_dist_create but with no device (the pairing check of the collective schedule, e.g. 256^3
 * on 8 ranks in a CPU test).  Its communication steps in execution order, flattened into `ops`
 * (int64 words; ops = NULL: only *len): per step
 *   seq (0 factor, 1 forward solve, 2 backward solve), type (0 exchange, 1 broadcast), root, bytes, cnt,
 *   then cnt x (peer, sbytes, rbytes) for an exchange, or the cnt ranks of the group for a broadcast.
 * bytes[0..4]: device bytes the rank allocates in all, its factor store, its front scratch, its
 * staging + received-block buffer, and the pinned host staging of a host-memory transport; counts[0..2]:
 * factor launches, shared fronts the rank works on, owned column blocks. */
int     smlu_plan_rank_schedule(const smlu_plan* plan, int32_t nparts, int32_t rank, int64_t* ops, int64_t cap,
                                int64_t* len, double bytes[5], int64_t counts[3]);
/* Host-only critical-path projection of the partitioned factorization at `tflops` per GPU,
 * `gbs` GB/s per link and `lat_us` per message: returns the projected seconds, *t1 = one GPU. */
double  smlu_plan_project(const smlu_plan* plan, int32_t nparts, double tflops, double gbs, double lat_us,
                          double* t1);

/* ---- diagnostics (no reference counterpart; tools/determinism*.py) ----------------------
 * Reads of a one-GPU handle's factorization, for reproducibility checks: per supernode s a hash
 * of its factor values (L panel + U12 bit patterns) and one of its row permutation,
 * out[2s], out[2s+1] (2 * nsuper entries); its values as stored (L panel M x ns, ld M, then U12
 * ns x nu, ld ns); its offsets (Loff, Uoff, Foff (-1: no F22), M; 4 * nsuper entries); and
 * doubles [off, off+cnt) of the factor store (which 0) or the front scratch (which 1) -- cnt < 0
 * returns the buffer's length in *len.  Each synchronises the handle's stream first. */
int smlu_dev_front_hash(smlu_handle* h, unsigned long long* out);
int smlu_dev_front_values(smlu_handle* h, int64_t s, double* out);
int smlu_dev_front_offsets(smlu_handle* h, int64_t* out);
int smlu_dev_copy(smlu_handle* h, int which, int64_t off, int64_t cnt, double* out, int64_t* len);
/* Host-only: section hashes of rank `rank`'s schedule of a `nparts`-rank handle (launches, tasks,
 * work lists, communication steps), so that a CPU test sees any change of what is scheduled.
 * flags: bit 0 values not diagonally dominant, bit 1 pivmode = 1 (the re-pivoting refactor's
 * schedule), bit 2 pair-preserving pivots (complex handle), bit 3 use_mfma = 0.  Writes *len words
 * (out = NULL: only *len): 19 section hashes (node records | fac, fwd, bwd, fwdm, bwdm | segments |
 * comm | ilist, xt, ae, xc, ft, gptr, gent | gt, st_tasks, ur_tasks | scalars), the launch counts
 * per kind of fac, fwd and bwd, the numbers of exchange and broadcast steps, and the bit patterns
 * of gemm_flops, gemm22_flops, gemm_bytes and smlu_plan_rank_schedule's bytes[0..4]. */
int smlu_plan_schedule_digest(const smlu_plan* plan, int32_t nparts, int32_t rank, int32_t flags, uint64_t* out,
                              int64_t cap, int64_t* len);

/* ---- environment knobs (read by the library in one place, csrc/tune.cpp; nothing else in the
 * environment changes its numerics or schedule) ---------------------------------------------
 *   SMLU_OB=w          outer block width of the blocked fronts (multiple of 64; default 384)
 *   SMLU_T128MIN=t     128x128 MFMA tiles for GEMM launches with >= t output tiles (default 512)
 *   SMLU_SMALLK=0      no one-shot k <= 64 GEMM tile (tests: forces the 64x64 VALU tile, and the
 *                      GEMM-form TRSM onto the 128 tile when SMLU_T128MIN allows it)
 *   SMLU_FULLPIV_NS=k  largest front with full-candidate pivoting (tests; default: 512, or 0
 *                      for diagonally dominant values)
 *   SMLU_F22_GATHER_NU=u  blocked fronts with at least u update rows (default 512) have their F22
 *                      assembled inside the Schur GEMM's C prologue instead of by the assembly
 *                      kernel (one GPU, real values, 128 MFMA tile only; bitwise the same factors);
 *                      0 or negative: off.  smlu_stat: f22_gather_fronts, f22_gather_entries,
 *                      launches_mfma128_gather
 *   SMLU_F22_GATHER_CH=c  ... only fronts with at most c contributing children (default 8)
 *   SMLU_LSIDE_MIN=r   diagonal-tile fronts with at least r rows below the current outer block
 *                      (default 2048) solve and update those L rows on the handle's side stream,
 *                      off the panel chain, and join them before the block's trailing update (one
 *                      GPU, dominant values; bitwise the same factors); 0: off.  smlu_stat:
 *                      side_launches, side_rows
 *   SMLU_TRAIL_SPAN=s  trailing updates of the large diagonal-tile fronts in tree order: after j
 *                      finished outer blocks only the blocks of the next lowbit(j) block rows and
 *                      columns are updated, with k = lowbit(j) outer blocks, and every s-th boundary
 *                      updates everything right of it with k = s outer blocks (s a power of two,
 *                      default 2; 1: one k = OB update of everything per outer block, the order
 *                      before round 11; 0: no full update).  Same launches, same FMA sequence per element, bitwise the same
 *                      factors (one GPU, dominant values).  smlu_stat: trail_span, trail_fronts,
 *                      gemmo_kmax
 *   SMLU_TRAIL_NS=n    ... for fronts with at least n pivot columns (default 1024, and held at or
 *                      above 1024; 64 is accepted as the lower bound for tests)
 *   SMLU_SWEEP_SPIN=s  polls before a sync-free solve wait gives up and the solve is re-run on the
 *                      per-block schedule (default 2^22; 0 = at once, tests)
 *   SMLU_SOLVE_STEPS=1 per-block solve launches instead of the sync-free sweeps
 *   SMLU_NO_GRAPH      eager launches instead of captured hipGraphs
 *   SMLU_DEBUG_SYNC    synchronise after every launch (localises a failing kernel)
 *   SMLU_NO_REPIVOT    no re-pivoting refactor after weak diagonal-tile pivots (tests)
 * and, not a library knob: OMP_NUM_THREADS, when set, caps the host threads of the analysis
 * (otherwise the hardware threads, at most 32; the plan does not depend on the thread count).
 */

/* Library version string. */
const char* smlu_version(void);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif

#endif /* SMLU_H */
