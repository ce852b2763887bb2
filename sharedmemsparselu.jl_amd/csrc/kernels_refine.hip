// kernels_refine.hip — gfx950 kernels of the batched iterative refinement (smlu_solve_refined_multi*,
// solve.cpp): the residuals r = b - op(A) x of up to 16 columns in one pass over A, the
// correction x += d on a list of columns, and the record the host reads the norms from.
//
// k_residual_batch / k_residual_t_batch are k_residual / k_residual_t (kernels_solve.hip,
// kernels_solve_t.hip) with NR accumulator pairs per thread: thread i is row i (column i of the CSC
// for the transposed kernel) in workgroups of 256, each entry of A and its index are loaded once and
// applied to every active column, and for a given (row, column) the fma chain runs over the entries
// in the single kernel's order and ends in its tail formulas, so a column's residual, and the two
// maxima folded from it (a maximum does not depend on the order of its operands), are bitwise what
// the single kernel gives for that column alone.
#include "kernels_common.hpp"

namespace smlu {

// Slot s of a launch works on column c[s] of X and of the stash; n active slots (1..kMultiRhs).
struct RefCols {
  int32_t n;
  int32_t c[kMultiRhs];
};

// tail of k_residual for one (row, column): the residual, its denominator |op(A)||x| + |b| and the
// componentwise ratio (a zero residual counts 0, a zero denominator under a nonzero one HUGE_VAL)
__device__ __forceinline__ void residual_tail(double bi, double acc, double den, double& ri, double& wi) {
  ri = bi - acc;
  den += fabs(bi);
  wi = ri == 0.0 ? 0.0 : den > 0.0 ? fabs(ri) / den : HUGE_VAL;
}

// the two maxima of slot s into nrm[2 c], nrm[2 c + 1] (cleared by the host before the launch)
__device__ __forceinline__ void fold_norms(double ri, double wi, double* __restrict__ nrm, int c) {
  const double m = wave_max(fabs(ri));
  const double w = wave_max(wi);
  if ((threadIdx.x & 63) == 0 && m > 0.0) atomic_max_pos(nrm + 2 * c, m);
  if ((threadIdx.x & 63) == 0 && w > 0.0) atomic_max_pos(nrm + 2 * c + 1, w);
}

// x: the caller's X (column c at x + c*ldx); b: the stash of B (column c at b + c*n); r: the
// compact residuals (slot s at r + s*n).
template <int NR>
__global__ __launch_bounds__(256) void k_residual_batch(int64_t n, const int64_t* __restrict__ rowptr,
                                                        const int32_t* __restrict__ ent,
                                                        const int32_t* __restrict__ acol,
                                                        const double* __restrict__ a, const double* __restrict__ x,
                                                        int64_t ldx, const double* __restrict__ b,
                                                        double* __restrict__ r, double* __restrict__ nrm,
                                                        RefCols cols) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int na = cols.n;
  double ri[NR], wi[NR];
#pragma unroll
  for (int s = 0; s < NR; ++s) ri[s] = wi[s] = 0.0;
  if (i < n) {
    double acc[NR], den[NR];
#pragma unroll
    for (int s = 0; s < NR; ++s) acc[s] = den[s] = 0.0;
    for (int64_t e = rowptr[i]; e < rowptr[i + 1]; ++e) {
      const int32_t k = ent[e];
      const double av = a[k];
      const double aa = fabs(av);
      const int32_t c = acol[k];
#pragma unroll
      for (int s = 0; s < NR; ++s)
        if (s < na) {
          const double xk = x[cols.c[s] * ldx + c];
          acc[s] = fma(av, xk, acc[s]);
          den[s] = fma(aa, fabs(xk), den[s]);
        }
    }
#pragma unroll
    for (int s = 0; s < NR; ++s)
      if (s < na) {
        residual_tail(b[cols.c[s] * n + i], acc[s], den[s], ri[s], wi[s]);
        r[s * n + i] = ri[s];
      }
  }
#pragma unroll
  for (int s = 0; s < NR; ++s)
    if (s < na) fold_norms(ri[s], wi[s], nrm, cols.c[s]);
}

// The transposed residual r = b - A^T x by columns of A's CSC; conj: the residual of
// conj(K^T conj(.)) on a ComplexF64 handle's real-equivalent K (k_residual_t's sign rule).
template <int NR>
__global__ __launch_bounds__(256) void k_residual_t_batch(int64_t n, const int64_t* __restrict__ colptr,
                                                          const int32_t* __restrict__ arow,
                                                          const double* __restrict__ a, const double* __restrict__ x,
                                                          int64_t ldx, const double* __restrict__ b,
                                                          double* __restrict__ r, double* __restrict__ nrm, int conj,
                                                          RefCols cols) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int na = cols.n;
  double rj[NR], wj[NR];
#pragma unroll
  for (int s = 0; s < NR; ++s) rj[s] = wj[s] = 0.0;
  if (j < n) {
    double acc[NR], den[NR];
#pragma unroll
    for (int s = 0; s < NR; ++s) acc[s] = den[s] = 0.0;
    for (int64_t e = colptr[j]; e < colptr[j + 1]; ++e) {
      const int32_t i = arow[e];
      const double av = a[e];
      const double aa = fabs(av);
      const bool neg = conj && (i & 1);
#pragma unroll
      for (int s = 0; s < NR; ++s)
        if (s < na) {
          const double xv = x[cols.c[s] * ldx + i];
          const double xi = neg ? -xv : xv;
          acc[s] = fma(av, xi, acc[s]);
          den[s] = fma(aa, fabs(xi), den[s]);
        }
    }
    const bool negj = conj && (j & 1);
#pragma unroll
    for (int s = 0; s < NR; ++s)
      if (s < na) {
        residual_tail(b[cols.c[s] * n + j], negj ? -acc[s] : acc[s], den[s], rj[s], wj[s]);
        r[s * n + j] = rj[s];
      }
  }
#pragma unroll
  for (int s = 0; s < NR; ++s)
    if (s < na) fold_norms(rj[s], wj[s], nrm, cols.c[s]);
}

// X[:, c[s]] += D[:, s]: k_axpy1's one addition per element, on the listed columns only.
template <int NR>
__global__ __launch_bounds__(256) void k_axpy_cols(int64_t n, const double* __restrict__ d, double* __restrict__ x,
                                                   int64_t ldx, RefCols cols) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
#pragma unroll
  for (int s = 0; s < NR; ++s)
    if (s < cols.n) x[cols.c[s] * ldx + i] += d[s * n + i];
}

// The host's record of one residual round: the 2 * kMultiRhs norm words between two copies of the
// sequence number of the read (read_status' rule: a copy counts only when both stamps match).
__global__ void k_refine_record(const double* __restrict__ nrm, long long* __restrict__ rec, long long seq) {
  const int t = threadIdx.x;
  if (t < 2 * kMultiRhs) rec[1 + t] = __double_as_longlong(nrm[t]);
  if (t == 0) {
    rec[0] = seq;
    rec[2 * kMultiRhs + 1] = seq;
  }
}

// ---- host-side launch wrappers (solve.cpp) ---------------------------------------------------
// The width is the smallest of 1, 4, 8, 16 that holds the active columns (SMLU_BY_WIDTH's rule).
#define SMLU_R(K, ...)                                                          \
  do {                                                                          \
    const unsigned g = (unsigned)((n + 255) / 256);                             \
    if (cols.n == 1) K<1><<<g, 256, 0, st>>>(__VA_ARGS__, cols);                 \
    else if (cols.n <= 4) K<4><<<g, 256, 0, st>>>(__VA_ARGS__, cols);            \
    else if (cols.n <= 8) K<8><<<g, 256, 0, st>>>(__VA_ARGS__, cols);            \
    else K<16><<<g, 256, 0, st>>>(__VA_ARGS__, cols);                            \
    return hipGetLastError();                                                   \
  } while (0)

static bool fill_cols(RefCols& cols, int nact, const int32_t* list) {
  if (nact < 1 || nact > kMultiRhs) return false;
  cols.n = nact;
  for (int s = 0; s < kMultiRhs; ++s) {
    cols.c[s] = s < nact ? list[s] : 0;
    if (cols.c[s] < 0 || cols.c[s] >= kMultiRhs) return false;
  }
  return true;
}

hipError_t launch_residual_batch(hipStream_t st, int64_t n, const int64_t* rowptr, const int32_t* ent,
                                 const int32_t* acol, const double* a, const double* x, int64_t ldx, const double* b,
                                 double* r, double* nrm, int nact, const int32_t* list) {
  RefCols cols;
  if (!fill_cols(cols, nact, list)) return hipErrorInvalidValue;
  if (n <= 0) return hipSuccess;
  SMLU_R(k_residual_batch, n, rowptr, ent, acol, a, x, ldx, b, r, nrm);
}

hipError_t launch_residual_t_batch(hipStream_t st, int64_t n, const int64_t* colptr, const int32_t* arow,
                                   const double* a, const double* x, int64_t ldx, const double* b, double* r,
                                   double* nrm, int conj, int nact, const int32_t* list) {
  RefCols cols;
  if (!fill_cols(cols, nact, list)) return hipErrorInvalidValue;
  if (n <= 0) return hipSuccess;
  SMLU_R(k_residual_t_batch, n, colptr, arow, a, x, ldx, b, r, nrm, conj);
}

hipError_t launch_axpy_cols(hipStream_t st, int64_t n, const double* d, double* x, int64_t ldx, int nact,
                            const int32_t* list) {
  RefCols cols;
  if (!fill_cols(cols, nact, list)) return hipErrorInvalidValue;
  if (n <= 0) return hipSuccess;
  SMLU_R(k_axpy_cols, n, d, x, ldx);
}
#undef SMLU_R

hipError_t launch_refine_record(hipStream_t st, const double* nrm, long long* rec, long long seq) {
  k_refine_record<<<1, 64, 0, st>>>(nrm, rec, seq);
  return hipGetLastError();
}

}  // namespace smlu
