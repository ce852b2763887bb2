// kernels_krylov.hip — gfx950 kernels of the GMRES that is preconditioned by the handle's factors
// (smlu_solve_gmres*, krylov.cpp): the product with A's pattern and the caller's values,
// the true residual with its norm, and the Arnoldi step's three passes over the basis.
//
// The basis V holds restart + 1 columns of leading dimension ldv = n rounded up to even, the pad row
// kept zero, so every column starts 16-byte aligned and a lane loads two rows at once (np = ldv / 2
// pairs).  Reductions have the shape of kernels_diag.hip: dg_blocks(.) <= kDgMaxBlocks workgroups
// of 256 threads, a grid-stride in increasing index order, an LDS tree, one partial per workgroup
// and column, and a one-workgroup finisher that folds the partials in workgroup order.  No atomics:
// two runs on the same data are bitwise equal.  Ordering between the kernels is stream order.
//
// The small Krylov problem lives in KryState on the device: the finisher of the step's last pass
// appends the Hessenberg column, applies and extends the Givens rotations and writes the 64-byte
// record {seq, |g_{j+1}|, h_{j+1,j}, j, .., seq} the host reads once per iteration.
#include "kernels_common.hpp"

namespace smlu {

constexpr int kKryThreads = 256;

// device state of one cycle (doubles): the divisor of the next product (||r|| or h_{j+1,j}), the two
// Gram-Schmidt coefficient vectors, R (upper triangle, column j at R + 32 j), rotations, g and y
struct KryState {
  double scale;
  double coef1[kKryMaxRestart];
  double coef2[kKryMaxRestart];
  double R[kKryMaxRestart * kKryMaxRestart];
  double cs[kKryMaxRestart];
  double sn[kKryMaxRestart];
  double g[kKryMaxRestart + 1];
  double y[kKryMaxRestart];
};
static_assert(sizeof(KryState) == 8 * kKryStateWords, "KryState and krylov.cpp's allocation agree");

static inline int kry_blocks(int64_t n) {
  return (int)std::min<int64_t>(kDgMaxBlocks, std::max<int64_t>(1, (n + kKryThreads - 1) / kKryThreads));
}

__device__ __forceinline__ void kry_stamp(long long* rec, long long seq) {
  rec[0] = seq;
  rec[7] = seq;
}

// LDS tree over the workgroup's 256 values of NC columns, eight columns per round; thread 0 writes
// the sums to out[0..nc).  s holds 8 x 256 doubles.
template <int NC>
__device__ __forceinline__ void kry_block_sums(const double (&acc)[NC], int nc, double* s, double* out) {
  const int t = threadIdx.x;
#pragma unroll
  for (int c0 = 0; c0 < NC; c0 += 8) {
    if (c0 < nc) {
      __syncthreads();
#pragma unroll
      for (int c = 0; c < 8; ++c)
        if (c0 + c < NC) s[c * kKryThreads + t] = acc[c0 + c < NC ? c0 + c : 0];
      __syncthreads();
#pragma unroll
      for (int o = kKryThreads / 2; o > 0; o >>= 1) {
        if (t < o) {
#pragma unroll
          for (int c = 0; c < 8; ++c)
            if (c0 + c < NC) s[c * kKryThreads + t] += s[c * kKryThreads + t + o];
        }
        __syncthreads();
      }
      if (t < 8 && c0 + t < nc) out[c0 + t] = s[t * kKryThreads];
    }
  }
}

__device__ __forceinline__ double kry_block_sum(double v, double* s) {
  const int t = threadIdx.x;
  __syncthreads();
  s[t] = v;
  __syncthreads();
#pragma unroll
  for (int o = kKryThreads / 2; o > 0; o >>= 1) {
    if (t < o) s[t] += s[t + o];
    __syncthreads();
  }
  return s[0];
}

__device__ __forceinline__ double kry_block_max(double v, double* s) {
  const int t = threadIdx.x;
  __syncthreads();
  s[t] = v;
  __syncthreads();
#pragma unroll
  for (int o = kKryThreads / 2; o > 0; o >>= 1) {
    if (t < o) s[t] = fmax(s[t], s[t + o]);
    __syncthreads();
  }
  return s[0];
}

// ---- products with A's pattern and an explicit values pointer ---------------------------------
// (op(A') x)_i: T = false, row i through the row lists (rowptr / ent: entry ids in column order,
// acol: their columns), as k_residual; T = true, column i of the CSC (colptr / arow), as
// k_residual_t.  den: sum |a| |x| beside it.
template <bool T>
__device__ __forceinline__ double kry_row(int64_t i, const int64_t* __restrict__ ptr, const int32_t* __restrict__ ent,
                                          const int32_t* __restrict__ acol, const int32_t* __restrict__ arow,
                                          const double* __restrict__ a, const double* __restrict__ x, double* den) {
  double acc = 0.0, d = 0.0;
  for (int64_t e = ptr[i]; e < ptr[i + 1]; ++e) {
    const int64_t k = T ? e : (int64_t)ent[e];
    const double xk = x[T ? arow[k] : acol[k]];
    acc = fma(a[k], xk, acc);
    d = fma(fabs(a[k]), fabs(xk), d);
  }
  *den = d;
  return acc;
}

// w = (op(A') z) / scale and, in the same pass, the basis column the solve's input came from
// normalised in place: v /= scale (scale = ||r|| for v_0, h_{j,j-1} for v_j).  One thread per row.
template <bool T>
__global__ __launch_bounds__(kKryThreads) void k_kry_spmv(int64_t n, const int64_t* __restrict__ ptr,
                                                          const int32_t* __restrict__ ent,
                                                          const int32_t* __restrict__ acol,
                                                          const int32_t* __restrict__ arow,
                                                          const double* __restrict__ a, const double* __restrict__ z,
                                                          const KryState* __restrict__ st, double* __restrict__ v,
                                                          double* __restrict__ w) {
  const int64_t i = (int64_t)blockIdx.x * kKryThreads + threadIdx.x;
  if (i >= n) return;
  const double scale = st->scale;
  double den;
  const double acc = kry_row<T>(i, ptr, ent, acol, arow, a, z, &den);
  w[i] = acc / scale;
  v[i] = v[i] / scale;
}

// r = b - op(A') x into the basis' first column (x = nullptr: r = b), with the partials of ||r||^2
// and of the componentwise backward error max_i |r_i| / (|op(A')||x| + |b|)_i (k_residual's rule).
template <bool T>
__global__ __launch_bounds__(kKryThreads) void k_kry_resid(int64_t n, const int64_t* __restrict__ ptr,
                                                           const int32_t* __restrict__ ent,
                                                           const int32_t* __restrict__ acol,
                                                           const int32_t* __restrict__ arow,
                                                           const double* __restrict__ a, const double* __restrict__ x,
                                                           const double* __restrict__ b, double* __restrict__ r,
                                                           double* __restrict__ part) {
  __shared__ double sd[kKryThreads];
  double ss = 0.0, worst = 0.0;
  const int64_t stride = (int64_t)gridDim.x * kKryThreads;
  for (int64_t i = (int64_t)blockIdx.x * kKryThreads + threadIdx.x; i < n; i += stride) {
    double den = 0.0, acc = 0.0;
    if (x) acc = kry_row<T>(i, ptr, ent, acol, arow, a, x, &den);
    const double bi = b[i];
    const double ri = bi - acc;
    r[i] = ri;
    den += fabs(bi);
    ss = fma(ri, ri, ss);
    worst = fmax(worst, ri == 0.0 ? 0.0 : den > 0.0 ? fabs(ri) / den : HUGE_VAL);
  }
  ss = kry_block_sum(ss, sd);
  worst = kry_block_max(worst, sd);
  if (threadIdx.x == 0) {
    part[(int64_t)blockIdx.x * kKryPartStride] = ss;
    part[(int64_t)blockIdx.x * kKryPartStride + 1] = worst;
  }
}

// the partials in workgroup order -> ||r||; a new cycle's state (scale = g_0 = ||r||);
// rec = {seq, ||r||, berr}
__global__ __launch_bounds__(kKryThreads) void k_kry_resid_fin(int nparts, const double* __restrict__ part,
                                                               KryState* __restrict__ st, long long* __restrict__ rec,
                                                               long long seq) {
  __shared__ double sd[kKryThreads];
  double worst = 0.0;
  for (int b = threadIdx.x; b < nparts; b += kKryThreads) worst = fmax(worst, part[(int64_t)b * kKryPartStride + 1]);
  worst = kry_block_max(worst, sd);
  if (threadIdx.x == 0) {
    double ss = 0.0;
    for (int b = 0; b < nparts; ++b) ss += part[(int64_t)b * kKryPartStride];
    const double beta = sqrt(ss);
    st->scale = beta;
    st->g[0] = beta;
    rec[1] = __double_as_longlong(beta);
    rec[2] = __double_as_longlong(worst);
    kry_stamp(rec, seq);
  }
}

// ---- the Arnoldi step's passes over V ---------------------------------------------------------
// PASS 0: h = V^T w              (nc dot products; w loaded once, the sums stay in registers)
// PASS 1: w -= V coef1, then h2 = V^T w in the same pass
// PASS 2: w -= V coef2 into the next basis column `out`, with ||w||^2
// NC: columns the instantiation holds (nc <= NC).  A lane takes rows 2p and 2p + 1; the pad row
// (row n of an odd n) is stored as 0 whatever the coefficients are, so it stays zero for later calls.
template <int NC, int PASS>
__global__ __launch_bounds__(kKryThreads) void k_kry_pass(int64_t n, int64_t np, int64_t ldv, int nc,
                                                          const double* __restrict__ V, double* __restrict__ w,
                                                          const double* __restrict__ coef, double* __restrict__ out,
                                                          double* __restrict__ part) {
  __shared__ double sd[8 * kKryThreads];
  double acc[NC];
  double cf[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    acc[c] = 0.0;
    cf[c] = (PASS != 0 && c < nc) ? coef[c] : 0.0;
  }
  double ss = 0.0;
  const double2* __restrict__ V2 = reinterpret_cast<const double2*>(V);
  double2* __restrict__ w2 = reinterpret_cast<double2*>(w);
  const int64_t ld2 = ldv >> 1;
  const int64_t stride = (int64_t)gridDim.x * kKryThreads;
  for (int64_t p = (int64_t)blockIdx.x * kKryThreads + threadIdx.x; p < np; p += stride) {
    double2 wv = w2[p];
    double2 vv[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (c < nc) vv[c] = V2[c * ld2 + p];
    if (PASS != 0) {
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < nc) {
          wv.x = fma(-cf[c], vv[c].x, wv.x);
          wv.y = fma(-cf[c], vv[c].y, wv.y);
        }
    }
    if (PASS != 0 && 2 * p + 1 >= n) wv.y = 0.0;
    if (PASS == 1) w2[p] = wv;
    if (PASS == 2) {
      reinterpret_cast<double2*>(out)[p] = wv;
      ss = fma(wv.x, wv.x, ss);
      ss = fma(wv.y, wv.y, ss);
    } else {
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < nc) {
          acc[c] = fma(vv[c].x, wv.x, acc[c]);
          acc[c] = fma(vv[c].y, wv.y, acc[c]);
        }
    }
  }
  double* o = part + (int64_t)blockIdx.x * kKryPartStride;
  if (PASS == 2) {
    ss = kry_block_sum(ss, sd);
    if (threadIdx.x == 0) o[0] = ss;
  } else {
    kry_block_sums<NC>(acc, nc, sd, o);
  }
}

// finisher of passes 0 and 1: thread c folds column c's partials in workgroup order -> coef[c]
__global__ __launch_bounds__(kKryThreads) void k_kry_coef_fin(int nparts, int nc, const double* __restrict__ part,
                                                              double* __restrict__ coef) {
  const int c = threadIdx.x;
  if (c >= nc) return;
  double s = 0.0;
  for (int b = 0; b < nparts; ++b) s += part[(int64_t)b * kKryPartStride + c];
  coef[c] = s;
}

// finisher of pass 2, step j: h_{j+1,j} = ||w||; the Hessenberg column h = coef1 + coef2 through the
// rotations so far; the new rotation; g.  A zero h_{j+1,j} (breakdown) and a zero column give the
// identity rotation: nothing is divided by them.  scale = h_{j+1,j} for the next product.
// rec = {seq, |g_{j+1}|, h_{j+1,j}, j}
__global__ __launch_bounds__(64) void k_kry_hess_fin(int nparts, int j, const double* __restrict__ part,
                                                     KryState* __restrict__ st, long long* __restrict__ rec,
                                                     long long seq) {
  __shared__ double hc[kKryMaxRestart + 1];
  const int t = threadIdx.x;
  if (t <= j && t < kKryMaxRestart) hc[t] = st->coef1[t] + st->coef2[t];
  __syncthreads();
  if (t != 0) return;
  double ss = 0.0;
  for (int b = 0; b < nparts; ++b) ss += part[(int64_t)b * kKryPartStride];
  const double hn = sqrt(ss);
  for (int i = 0; i < j; ++i) {
    const double c = st->cs[i], s = st->sn[i];
    const double a = hc[i], b2 = hc[i + 1];
    hc[i] = fma(c, a, s * b2);
    hc[i + 1] = fma(-s, a, c * b2);
  }
  const double a = hc[j];
  const double d = hypot(a, hn);
  double c = 1.0, s = 0.0;
  if (d > 0.0 && hn != 0.0) {
    c = a / d;
    s = hn / d;
  }
  hc[j] = hn != 0.0 ? d : a;
  st->cs[j] = c;
  st->sn[j] = s;
  const double gj = st->g[j];
  st->g[j] = c * gj;
  const double gn = -s * gj;
  st->g[j + 1] = gn;
  for (int i = 0; i <= j; ++i) st->R[j * kKryMaxRestart + i] = hc[i];
  st->scale = hn;
  rec[1] = __double_as_longlong(fabs(gn));
  rec[2] = __double_as_longlong(hn);
  rec[3] = j;
  kry_stamp(rec, seq);
}

// R y = g for the cycle's k steps, column-oriented: thread i owns g_i
__global__ __launch_bounds__(64) void k_kry_backsolve(int k, KryState* __restrict__ st) {
  __shared__ double g[kKryMaxRestart];
  __shared__ double yi;
  const int t = threadIdx.x;
  if (t < k) g[t] = st->g[t];
  __syncthreads();
  for (int i = k - 1; i >= 0; --i) {
    if (t == i) {
      yi = g[i] / st->R[i * kKryMaxRestart + i];
      st->y[i] = yi;
    }
    __syncthreads();
    if (t < i) g[t] = fma(-st->R[i * kKryMaxRestart + t], yi, g[t]);
    __syncthreads();
  }
}

// u = V y over the cycle's k columns (one pass); the pad row is stored as 0
template <int NC>
__global__ __launch_bounds__(kKryThreads) void k_kry_combine(int64_t n, int64_t np, int64_t ldv, int k,
                                                             const double* __restrict__ V,
                                                             const KryState* __restrict__ st, double* __restrict__ u) {
  const int64_t p = (int64_t)blockIdx.x * kKryThreads + threadIdx.x;
  if (p >= np) return;
  const double2* __restrict__ V2 = reinterpret_cast<const double2*>(V);
  const int64_t ld2 = ldv >> 1;
  double2 s = make_double2(0.0, 0.0);
#pragma unroll
  for (int c = 0; c < NC; ++c)
    if (c < k) {
      const double yc = st->y[c];
      const double2 v = V2[c * ld2 + p];
      s.x = fma(yc, v.x, s.x);
      s.y = fma(yc, v.y, s.y);
    }
  if (2 * p + 1 >= n) s.y = 0.0;
  reinterpret_cast<double2*>(u)[p] = s;
}

// ---- launchers ------------------------------------------------------------------------------
#define SMLU_KRY(expr) \
  do {                 \
    expr;              \
    hipError_t _e = hipGetLastError(); \
    if (_e != hipSuccess) return _e;   \
  } while (0)

// by the smallest instantiation that holds nc columns
#define SMLU_KRY_NC(nc, CALL)      \
  do {                             \
    if ((nc) <= 4) CALL(4);        \
    else if ((nc) <= 8) CALL(8);   \
    else if ((nc) <= 16) CALL(16); \
    else CALL(32);                 \
  } while (0)

hipError_t launch_kry_spmv(hipStream_t st, bool trans, int64_t n, const int64_t* rowptr, const int32_t* ent,
                           const int32_t* acol, const int64_t* colptr, const int32_t* arow, const double* a,
                           const double* z, const void* state, double* v, double* w) {
  const int nb = (int)((n + kKryThreads - 1) / kKryThreads);
  const KryState* s = static_cast<const KryState*>(state);
  if (trans) SMLU_KRY((k_kry_spmv<true><<<nb, kKryThreads, 0, st>>>(n, colptr, ent, acol, arow, a, z, s, v, w)));
  else SMLU_KRY((k_kry_spmv<false><<<nb, kKryThreads, 0, st>>>(n, rowptr, ent, acol, arow, a, z, s, v, w)));
  return hipSuccess;
}

hipError_t launch_kry_resid(hipStream_t st, bool trans, int64_t n, const int64_t* rowptr, const int32_t* ent,
                            const int32_t* acol, const int64_t* colptr, const int32_t* arow, const double* a,
                            const double* x, const double* b, double* r, double* part, void* state, long long* rec,
                            long long seq) {
  const int nb = kry_blocks(n);
  if (trans) SMLU_KRY((k_kry_resid<true><<<nb, kKryThreads, 0, st>>>(n, colptr, ent, acol, arow, a, x, b, r, part)));
  else SMLU_KRY((k_kry_resid<false><<<nb, kKryThreads, 0, st>>>(n, rowptr, ent, acol, arow, a, x, b, r, part)));
  SMLU_KRY((k_kry_resid_fin<<<1, kKryThreads, 0, st>>>(nb, part, static_cast<KryState*>(state), rec, seq)));
  return hipSuccess;
}

// Arnoldi step j on w = op(A') M^-1 v_j against v_0..v_j (V, leading dimension ldv): classical
// Gram-Schmidt twice in three passes, the un-normalised v_{j+1} into column j + 1, the small
// problem's update and the record.
hipError_t launch_kry_arnoldi(hipStream_t st, int64_t n, int64_t ldv, int j, double* V, double* w, double* part, void* state,
                              long long* rec, long long seq) {
  if (j < 0 || j >= kKryMaxRestart || (ldv & 1) || ldv < n || ldv > n + 1) return hipErrorInvalidValue;
  const int64_t np = ldv >> 1;
  const int nb = kry_blocks(np);
  const int nc = j + 1;
  KryState* s = static_cast<KryState*>(state);
  double* out = V + (int64_t)(j + 1) * ldv;
#define KRY_P0(N) SMLU_KRY((k_kry_pass<N, 0><<<nb, kKryThreads, 0, st>>>(n, np, ldv, nc, V, w, nullptr, nullptr, part)))
#define KRY_P1(N) SMLU_KRY((k_kry_pass<N, 1><<<nb, kKryThreads, 0, st>>>(n, np, ldv, nc, V, w, s->coef1, nullptr, part)))
#define KRY_P2(N) SMLU_KRY((k_kry_pass<N, 2><<<nb, kKryThreads, 0, st>>>(n, np, ldv, nc, V, w, s->coef2, out, part)))
  SMLU_KRY_NC(nc, KRY_P0);
  SMLU_KRY((k_kry_coef_fin<<<1, kKryThreads, 0, st>>>(nb, nc, part, s->coef1)));
  SMLU_KRY_NC(nc, KRY_P1);
  SMLU_KRY((k_kry_coef_fin<<<1, kKryThreads, 0, st>>>(nb, nc, part, s->coef2)));
  SMLU_KRY_NC(nc, KRY_P2);
  SMLU_KRY((k_kry_hess_fin<<<1, 64, 0, st>>>(nb, j, part, s, rec, seq)));
#undef KRY_P0
#undef KRY_P1
#undef KRY_P2
  return hipSuccess;
}

// u = V y, y from R y = g over the cycle's k steps
hipError_t launch_kry_update(hipStream_t st, int64_t n, int64_t ldv, int k, const double* V, void* state, double* u) {
  if (k < 1 || k > kKryMaxRestart || (ldv & 1) || ldv < n || ldv > n + 1) return hipErrorInvalidValue;
  const int64_t np = ldv >> 1;
  const int nb = (int)((np + kKryThreads - 1) / kKryThreads);
  KryState* s = static_cast<KryState*>(state);
  SMLU_KRY((k_kry_backsolve<<<1, 64, 0, st>>>(k, s)));
#define KRY_C(N) SMLU_KRY((k_kry_combine<N><<<nb, kKryThreads, 0, st>>>(n, np, ldv, k, V, s, u)))
  SMLU_KRY_NC(k, KRY_C);
#undef KRY_C
  return hipSuccess;
}

}  // namespace smlu
