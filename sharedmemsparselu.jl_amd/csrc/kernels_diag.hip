// kernels_diag.hip — gfx950 kernels of the determinant (smlu_logabsdet*) and of the Hager/Higham
// condition estimate (smlu_rcond): reductions over the factor diagonal, the front permutations and
// A's values, and the estimator's elementwise steps (diag.cpp).
//
// Every reduction has the same fixed shape: a grid of dg_blocks(n) <= kDgMaxBlocks (one per CU)
// workgroups of 256 threads, each thread over the indices gid, gid + grid size, ... in increasing
// order, an LDS tree per workgroup, one 64-byte partial per workgroup, and a one-workgroup kernel
// that folds the partials in index order and writes the 64-byte record the host reads.  No atomics:
// for a given n the summation order is fixed, so two evaluations of the same data are bitwise equal.
// Ordering between the two kernels is stream order.
#include "kernels_common.hpp"

namespace smlu {

constexpr int kDgThreads = 256;

// one workgroup's partial result: up to three doubles and four integers
struct DgPart {
  double d[3];
  long long l[4];
  long long pad;
};
static_assert(sizeof(DgPart) == 64, "DgPart is one 64-byte line");

static inline int dg_blocks(int64_t n) {
  return (int)std::min<int64_t>(kDgMaxBlocks, std::max<int64_t>(1, (n + kDgThreads - 1) / kDgThreads));
}

// LDS tree over the workgroup's 256 values (the result in every thread); s is reused across calls
template <class T>
__device__ __forceinline__ T dg_block_sum(T v, T* s) {
  const int t = threadIdx.x;
  __syncthreads();
  s[t] = v;
  __syncthreads();
#pragma unroll
  for (int o = kDgThreads / 2; o > 0; o >>= 1) {
    if (t < o) s[t] += s[t + o];
    __syncthreads();
  }
  return s[0];
}

__device__ __forceinline__ double dg_block_max(double v, double* s) {
  const int t = threadIdx.x;
  __syncthreads();
  s[t] = v;
  __syncthreads();
#pragma unroll
  for (int o = kDgThreads / 2; o > 0; o >>= 1) {
    if (t < o) s[t] = fmax(s[t], s[t + o]);
    __syncthreads();
  }
  return s[0];
}

// largest value with the lowest index on a tie (idx < 0: no candidate)
__device__ __forceinline__ void dg_block_argmax(double& v, long long& idx, double* sv, long long* si) {
  const int t = threadIdx.x;
  __syncthreads();
  sv[t] = v;
  si[t] = idx;
  __syncthreads();
#pragma unroll
  for (int o = kDgThreads / 2; o > 0; o >>= 1) {
    if (t < o) {
      const double ov = sv[t + o];
      const long long oi = si[t + o];
      if (oi >= 0 && (si[t] < 0 || ov > sv[t] || (ov == sv[t] && oi < si[t]))) {
        sv[t] = ov;
        si[t] = oi;
      }
    }
    __syncthreads();
  }
  v = sv[0];
  idx = si[0];
}

// The host's record: rec[0] and rec[7] carry the sequence number of the read (read_status' rule:
// a copy counts only when both stamps match), rec[1..6] the payload.
__device__ __forceinline__ void dg_stamp(long long* rec, long long seq) {
  rec[0] = seq;
  rec[7] = seq;
}

// ---- determinant ----------------------------------------------------------------------------
// Index k of the factored matrix (K on a complex handle): log|u_kk| from its front's diagonal
// (store[Loff + j M + j]), log|Rs_k|, the negative u_kk and Rs_k, and the cycles of the front's row
// permutation by cycle leaders: thread k follows rowperm from its local index j until it is back at
// j (one cycle, counted by its smallest member) or meets a smaller index.  The walk is bounded by ns
// steps and stays inside [0, ns), so a rowperm that is no permutation cannot hang or stray.
// Z (ComplexF64 handle, pair-preserving pivots): even k also gives pair k/2's complex pivot
// u = U[2m, 2m] - i U[2m, 2m+1], its angle, whether the pair's rows were exchanged, and the cycles
// of the front's permutation of pairs; the signs of K's own pivots are not counted.
template <bool Z>
__global__ __launch_bounds__(kDgThreads) void k_dg_logdet(int64_t n, const int32_t* __restrict__ col2s,
                                                          const SNode* __restrict__ sn,
                                                          const double* __restrict__ store,
                                                          const double* __restrict__ Rs,
                                                          const int32_t* __restrict__ rowperm,
                                                          DgPart* __restrict__ part) {
  __shared__ double sd[kDgThreads];
  __shared__ long long sl[kDgThreads];
  double lu = 0, lr = 0, ang = 0;
  long long cyc = 0, neg = 0, sw = 0, negr = 0;
  const int64_t stride = (int64_t)gridDim.x * kDgThreads;
  for (int64_t k = (int64_t)blockIdx.x * kDgThreads + threadIdx.x; k < n; k += stride) {
    const SNode& s = sn[col2s[k]];
    const int64_t first = s.first, Loff = s.Loff, ns = s.ns, M = ns + s.nu, j = k - first;
    const double u = store[Loff + j * M + j];
    const double r = Rs[k];
    lu += log(fabs(u));
    lr += log(fabs(r));
    negr += r < 0;
    const int32_t* rp = rowperm + first;
    if (!Z) {
      neg += u < 0;
      int64_t c = rp[j];
      for (int64_t step = 0; c > j && c < ns && step < ns; ++step) c = rp[c];
      cyc += c == j;
    } else if ((k & 1) == 0 && j + 1 < ns) {
      const double b = store[Loff + (j + 1) * M + j];
      ang += atan2(-b, u);
      sw += rp[j] > rp[j + 1];
      const int64_t m = j >> 1, np = ns >> 1;
      int64_t c = rp[j] >> 1;
      for (int64_t step = 0; c > m && c < np && step < np; ++step) c = rp[2 * c] >> 1;
      cyc += c == m;
    }
  }
  lu = dg_block_sum(lu, sd);
  lr = dg_block_sum(lr, sd);
  ang = dg_block_sum(ang, sd);
  cyc = dg_block_sum(cyc, sl);
  neg = dg_block_sum(neg, sl);
  sw = dg_block_sum(sw, sl);
  negr = dg_block_sum(negr, sl);
  if (threadIdx.x == 0) {
    DgPart& o = part[blockIdx.x];
    o.d[0] = lu;
    o.d[1] = lr;
    o.d[2] = ang;
    o.l[0] = cyc;
    o.l[1] = neg;
    o.l[2] = sw;
    o.l[3] = negr;
  }
}

// The partials in index order -> rec: sum log|u|, sum log|Rs|, sum of angles, cycles,
// negative u | exchanged pairs << 32, negative Rs.
__global__ __launch_bounds__(kDgThreads) void k_dg_logdet_fin(int nparts, const DgPart* __restrict__ part,
                                                              long long* __restrict__ rec, long long seq) {
  __shared__ double sd[kDgThreads];
  __shared__ long long sl[kDgThreads];
  double d[3] = {0, 0, 0};
  long long l[4] = {0, 0, 0, 0};
  for (int b = threadIdx.x; b < nparts; b += kDgThreads) {
    for (int i = 0; i < 3; ++i) d[i] += part[b].d[i];
    for (int i = 0; i < 4; ++i) l[i] += part[b].l[i];
  }
  for (int i = 0; i < 3; ++i) d[i] = dg_block_sum(d[i], sd);
  for (int i = 0; i < 4; ++i) l[i] = dg_block_sum(l[i], sl);
  if (threadIdx.x == 0) {
    rec[1] = __double_as_longlong(d[0]);
    rec[2] = __double_as_longlong(d[1]);
    rec[3] = __double_as_longlong(d[2]);
    rec[4] = l[0];
    rec[5] = l[1] | (l[2] << 32);
    rec[6] = l[3];
    dg_stamp(rec, seq);
  }
}

// ---- ||A||_1 / ||A||_inf from the handle's current values -----------------------------------
// ROWS = false: thread j sums |a_ij| down column j (colptr); ROWS = true: along row j (the row
// lists rowptr / row_ent of entry ids).  Z: the matrix is K and j a complex index; the moduli come
// from K's even columns, where entry e is Re a and e + 1 (the next row of the pair) Im a; a row
// list is filtered by the parity of the entry's column (acol).
template <bool Z, bool ROWS>
__global__ __launch_bounds__(kDgThreads) void k_dg_norm(int64_t nc, const int64_t* __restrict__ ptr,
                                                        const int32_t* __restrict__ ent,
                                                        const int32_t* __restrict__ acol,
                                                        const double* __restrict__ a, DgPart* __restrict__ part) {
  __shared__ double sd[kDgThreads];
  double best = 0;
  const int64_t stride = (int64_t)gridDim.x * kDgThreads;
  for (int64_t j = (int64_t)blockIdx.x * kDgThreads + threadIdx.x; j < nc; j += stride) {
    const int64_t jj = Z ? 2 * j : j;
    double s = 0;
    if (!ROWS) {
      for (int64_t e = ptr[jj]; e < ptr[jj + 1]; e += Z ? 2 : 1) s += Z ? hypot(a[e], a[e + 1]) : fabs(a[e]);
    } else {
      for (int64_t t = ptr[jj]; t < ptr[jj + 1]; ++t) {
        const int64_t e = ent[t];
        if (!Z) s += fabs(a[e]);
        else if ((acol[e] & 1) == 0) s += hypot(a[e], a[e + 1]);
      }
    }
    best = fmax(best, s);
  }
  best = dg_block_max(best, sd);
  if (threadIdx.x == 0) part[blockIdx.x].d[0] = best;
}

__global__ __launch_bounds__(kDgThreads) void k_dg_norm_fin(int nparts, const DgPart* __restrict__ part,
                                                            long long* __restrict__ rec, long long seq) {
  __shared__ double sd[kDgThreads];
  double best = 0;
  for (int b = threadIdx.x; b < nparts; b += kDgThreads) best = fmax(best, part[b].d[0]);
  best = dg_block_max(best, sd);
  if (threadIdx.x == 0) {
    rec[1] = __double_as_longlong(best);
    dg_stamp(rec, seq);
  }
}

// ---- the estimator's vectors (dlacn2 / zlacn2) ----------------------------------------------
// mode 0: x = 1/n;  1: x = e_j;  2: x_i = (-1)^i (1 + i / (n - 1)).  Z: (value, 0) pairs.
template <bool Z>
__global__ __launch_bounds__(kDgThreads) void k_dg_vec(int64_t n, int mode, int64_t j, double* __restrict__ x) {
  const int64_t i = (int64_t)blockIdx.x * kDgThreads + threadIdx.x;
  if (i >= n) return;
  double v;
  if (mode == 0) v = 1.0 / (double)n;
  else if (mode == 1) v = i == j ? 1.0 : 0.0;
  else v = ((i & 1) ? -1.0 : 1.0) * (1.0 + (double)i / (double)(n - 1));
  if (Z) {
    x[2 * i] = v;
    x[2 * i + 1] = 0.0;
  } else {
    x[i] = v;
  }
}

// sum |y_i| and, when xi is given, the sign vector in the same pass: real xi_i = +1 for y_i >= 0,
// else -1; complex xi_i = y_i / |y_i|, or 1 when |y_i| is not above the smallest normal number.
// cmp: count the entries whose sign differs from the xi stored before (real case's stop test).
template <bool Z>
__global__ __launch_bounds__(kDgThreads) void k_dg_sign(int64_t n, const double* __restrict__ y, double* xi,
                                                        int cmp, DgPart* __restrict__ part) {
  __shared__ double sd[kDgThreads];
  __shared__ long long sl[kDgThreads];
  double sum = 0;
  long long changed = 0;
  const int64_t stride = (int64_t)gridDim.x * kDgThreads;
  for (int64_t i = (int64_t)blockIdx.x * kDgThreads + threadIdx.x; i < n; i += stride) {
    if (Z) {
      const double re = y[2 * i], im = y[2 * i + 1];
      const double a = hypot(re, im);
      sum += a;
      if (xi) {
        const bool big = a > 2.2250738585072014e-308;
        xi[2 * i] = big ? re / a : 1.0;
        xi[2 * i + 1] = big ? im / a : 0.0;
      }
    } else {
      const double v = y[i];
      sum += fabs(v);
      if (xi) {
        const double sg = v >= 0.0 ? 1.0 : -1.0;
        if (cmp) changed += xi[i] != sg;
        xi[i] = sg;
      }
    }
  }
  sum = dg_block_sum(sum, sd);
  changed = dg_block_sum(changed, sl);
  if (threadIdx.x == 0) {
    part[blockIdx.x].d[0] = sum;
    part[blockIdx.x].l[0] = changed;
  }
}

__global__ __launch_bounds__(kDgThreads) void k_dg_sign_fin(int nparts, const DgPart* __restrict__ part,
                                                            long long* __restrict__ rec, long long seq) {
  __shared__ double sd[kDgThreads];
  __shared__ long long sl[kDgThreads];
  double sum = 0;
  long long changed = 0;
  for (int b = threadIdx.x; b < nparts; b += kDgThreads) {
    sum += part[b].d[0];
    changed += part[b].l[0];
  }
  sum = dg_block_sum(sum, sd);
  changed = dg_block_sum(changed, sl);
  if (threadIdx.x == 0) {
    rec[1] = __double_as_longlong(sum);
    rec[2] = changed;
    dg_stamp(rec, seq);
  }
}

template <bool Z>
__device__ __forceinline__ double dg_modulus(const double* __restrict__ z, int64_t i) {
  return Z ? hypot(z[2 * i], z[2 * i + 1]) : fabs(z[i]);
}

// arg max |z_i|, the lowest index on a tie (idamax / izmax1)
template <bool Z>
__global__ __launch_bounds__(kDgThreads) void k_dg_argmax(int64_t n, const double* __restrict__ z,
                                                          DgPart* __restrict__ part) {
  __shared__ double sd[kDgThreads];
  __shared__ long long sl[kDgThreads];
  double best = 0;
  long long idx = -1;
  const int64_t stride = (int64_t)gridDim.x * kDgThreads;
  for (int64_t i = (int64_t)blockIdx.x * kDgThreads + threadIdx.x; i < n; i += stride) {
    const double a = dg_modulus<Z>(z, i);
    if (idx < 0 || a > best) {   // increasing i: the first of equal values stays
      best = a;
      idx = i;
    }
  }
  dg_block_argmax(best, idx, sd, sl);
  if (threadIdx.x == 0) {
    part[blockIdx.x].d[0] = best;
    part[blockIdx.x].l[0] = idx;
  }
}

// ... and |z_jlast| beside it (jlast < 0: none), for the test "the old index still holds the maximum"
template <bool Z>
__global__ __launch_bounds__(kDgThreads) void k_dg_argmax_fin(int nparts, const DgPart* __restrict__ part,
                                                              const double* __restrict__ z, int64_t jlast,
                                                              long long* __restrict__ rec, long long seq) {
  __shared__ double sd[kDgThreads];
  __shared__ long long sl[kDgThreads];
  double best = 0;
  long long idx = -1;
  for (int b = threadIdx.x; b < nparts; b += kDgThreads) {
    const double a = part[b].d[0];
    const long long i = part[b].l[0];
    if (i >= 0 && (idx < 0 || a > best || (a == best && i < idx))) {
      best = a;
      idx = i;
    }
  }
  dg_block_argmax(best, idx, sd, sl);
  if (threadIdx.x == 0) {
    rec[1] = idx < 0 ? 0 : idx;
    rec[2] = __double_as_longlong(best);
    rec[3] = __double_as_longlong(jlast >= 0 ? dg_modulus<Z>(z, jlast) : 0.0);
    dg_stamp(rec, seq);
  }
}

// ---- launchers ------------------------------------------------------------------------------
#define SMLU_DG(expr) \
  do {                \
    expr;             \
    hipError_t _e = hipGetLastError(); \
    if (_e != hipSuccess) return _e;   \
  } while (0)

hipError_t launch_dg_logdet(hipStream_t st, bool z, int64_t n, const int32_t* col2s, const SNode* sn,
                            const double* store, const double* Rs, const int32_t* rowperm, void* part,
                            long long* rec, long long seq) {
  const int nb = dg_blocks(n);
  DgPart* p = static_cast<DgPart*>(part);
  if (z) SMLU_DG((k_dg_logdet<true><<<nb, kDgThreads, 0, st>>>(n, col2s, sn, store, Rs, rowperm, p)));
  else SMLU_DG((k_dg_logdet<false><<<nb, kDgThreads, 0, st>>>(n, col2s, sn, store, Rs, rowperm, p)));
  SMLU_DG((k_dg_logdet_fin<<<1, kDgThreads, 0, st>>>(nb, p, rec, seq)));
  return hipSuccess;
}

hipError_t launch_dg_norm(hipStream_t st, bool z, bool rows, int64_t nc, const int64_t* ptr, const int32_t* ent,
                          const int32_t* acol, const double* a, void* part, long long* rec, long long seq) {
  const int nb = dg_blocks(nc);
  DgPart* p = static_cast<DgPart*>(part);
  if (z && rows) SMLU_DG((k_dg_norm<true, true><<<nb, kDgThreads, 0, st>>>(nc, ptr, ent, acol, a, p)));
  else if (z) SMLU_DG((k_dg_norm<true, false><<<nb, kDgThreads, 0, st>>>(nc, ptr, ent, acol, a, p)));
  else if (rows) SMLU_DG((k_dg_norm<false, true><<<nb, kDgThreads, 0, st>>>(nc, ptr, ent, acol, a, p)));
  else SMLU_DG((k_dg_norm<false, false><<<nb, kDgThreads, 0, st>>>(nc, ptr, ent, acol, a, p)));
  SMLU_DG((k_dg_norm_fin<<<1, kDgThreads, 0, st>>>(nb, p, rec, seq)));
  return hipSuccess;
}

hipError_t launch_dg_vec(hipStream_t st, bool z, int64_t n, int mode, int64_t j, double* x) {
  const int nb = (int)((n + kDgThreads - 1) / kDgThreads);
  if (z) SMLU_DG((k_dg_vec<true><<<nb, kDgThreads, 0, st>>>(n, mode, j, x)));
  else SMLU_DG((k_dg_vec<false><<<nb, kDgThreads, 0, st>>>(n, mode, j, x)));
  return hipSuccess;
}

hipError_t launch_dg_sign(hipStream_t st, bool z, int64_t n, const double* y, double* xi, int cmp, void* part,
                          long long* rec, long long seq) {
  const int nb = dg_blocks(n);
  DgPart* p = static_cast<DgPart*>(part);
  if (z) SMLU_DG((k_dg_sign<true><<<nb, kDgThreads, 0, st>>>(n, y, xi, cmp, p)));
  else SMLU_DG((k_dg_sign<false><<<nb, kDgThreads, 0, st>>>(n, y, xi, cmp, p)));
  SMLU_DG((k_dg_sign_fin<<<1, kDgThreads, 0, st>>>(nb, p, rec, seq)));
  return hipSuccess;
}

hipError_t launch_dg_argmax(hipStream_t st, bool z, int64_t n, const double* zv, int64_t jlast, void* part,
                            long long* rec, long long seq) {
  const int nb = dg_blocks(n);
  DgPart* p = static_cast<DgPart*>(part);
  if (z) {
    SMLU_DG((k_dg_argmax<true><<<nb, kDgThreads, 0, st>>>(n, zv, p)));
    SMLU_DG((k_dg_argmax_fin<true><<<1, kDgThreads, 0, st>>>(nb, p, zv, jlast, rec, seq)));
  } else {
    SMLU_DG((k_dg_argmax<false><<<nb, kDgThreads, 0, st>>>(n, zv, p)));
    SMLU_DG((k_dg_argmax_fin<false><<<1, kDgThreads, 0, st>>>(nb, p, zv, jlast, rec, seq)));
  }
  return hipSuccess;
}

}  // namespace smlu
