// kernels_lowrank.hip — gfx950 kernels of the low-rank update (smlu_lowrank_set*, smlu_solve_lowrank*,
// lowrank.cpp): op(A + U V^T) x = b from the factors of A by the Sherman-Morrison-Woodbury
// identity.  The staging copy of the caller's U and V, the Gram matrix G = V^T Y of Y = A^-1 U, the
// capacitance matrix C = I + G with its LU and explicit inverse, the k dot products of a solve, the
// correction x = y0 - Y (C^-1 t), and the residual of the updated system.
//
// U, V, Y and Yt hold k <= kLrMax columns of leading dimension ld = n rounded up to even, the pad row
// kept zero, and so do the handle's three n-vectors: every column starts 16-byte aligned and a lane
// loads two rows at once (np = ld / 2 pairs), as in kernels_krylov.hip.  Reductions have that file's
// shape: at most kDgMaxBlocks workgroups of 256 threads, a grid-stride in increasing index order, an
// LDS tree, one partial per workgroup and column, folded in workgroup order by whoever consumes it.
// No atomics: two runs on the same data are bitwise equal.  Ordering between the kernels is stream
// order.
#include "kernels_common.hpp"

namespace smlu {

constexpr int kLrThreads = 256;
constexpr int kLrTile = 8;   // the Gram kernel's register tile: kLrTile x kLrTile accumulators

// device state of the installed update (doubles): C^-1 and C row-major with row stride kLrMax, and
// max |G_ij|
struct LrState {
  double Cinv[kLrMax * kLrMax];
  double C[kLrMax * kLrMax];
  double gram_max;
  double spare;
};
static_assert(sizeof(LrState) == 8 * kLrStateWords, "LrState and lowrank.cpp's allocation agree");

static inline int lr_blocks(int64_t n) {
  return (int)std::min<int64_t>(kDgMaxBlocks, std::max<int64_t>(1, (n + kLrThreads - 1) / kLrThreads));
}

// LDS tree over the workgroup's 256 values of eight columns; thread t < 8 writes column t's sum to
// out[t].  s holds 8 x 256 doubles.
__device__ __forceinline__ void lr_block_sums8(const double* acc8, double* s, double* out) {
  const int t = threadIdx.x;
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 8; ++c) s[c * kLrThreads + t] = acc8[c];
  __syncthreads();
#pragma unroll
  for (int o = kLrThreads / 2; o > 0; o >>= 1) {
    if (t < o) {
#pragma unroll
      for (int c = 0; c < 8; ++c) s[c * kLrThreads + t] += s[c * kLrThreads + t + o];
    }
    __syncthreads();
  }
  if (t < 8) out[t] = s[t * kLrThreads];
}

__device__ __forceinline__ double lr_block_max(double v, double* s) {
  const int t = threadIdx.x;
  __syncthreads();
  s[t] = v;
  __syncthreads();
#pragma unroll
  for (int o = kLrThreads / 2; o > 0; o >>= 1) {
    if (t < o) s[t] = fmax(s[t], s[t + o]);
    __syncthreads();
  }
  return s[0];
}

// ---- staging ----------------------------------------------------------------------------------
// dst[c ld + i] = src[c lds + i], i < n, c = blockIdx.y: the caller's leading dimension may be odd
// and its pointer 8-byte aligned only, so one row per lane.  The pad row of dst is not touched.
__global__ __launch_bounds__(kLrThreads) void k_lr_stage(int64_t n, int64_t ld, const double* __restrict__ src,
                                                         int64_t lds, double* __restrict__ dst) {
  const int64_t c = blockIdx.y;
  const int64_t stride = (int64_t)gridDim.x * kLrThreads;
  for (int64_t i = (int64_t)blockIdx.x * kLrThreads + threadIdx.x; i < n; i += stride) dst[c * ld + i] = src[c * lds + i];
}

// ---- Gram matrix --------------------------------------------------------------------------------
// Tile (ti, tj) = blockIdx.y of G = V^T Y: G[8 ti + a, 8 tj + b] over this workgroup's rows, the 64
// sums in registers, so V and Y are streamed ceil(k / 8) times each.  Columns >= k count as zero.
// gpart[blockIdx.x][i kLrMax + j]: this workgroup's partial of G_ij.
__global__ __launch_bounds__(kLrThreads) void k_lr_gram(int64_t np, int64_t ld, int k, const double* __restrict__ V,
                                                        const double* __restrict__ Y, double* __restrict__ gpart) {
  __shared__ double sd[8 * kLrThreads];
  const int kt = (k + kLrTile - 1) / kLrTile;
  const int i0 = ((int)blockIdx.y / kt) * kLrTile, j0 = ((int)blockIdx.y % kt) * kLrTile;
  double acc[kLrTile * kLrTile];
#pragma unroll
  for (int e = 0; e < kLrTile * kLrTile; ++e) acc[e] = 0.0;
  const double2* __restrict__ V2 = reinterpret_cast<const double2*>(V);
  const double2* __restrict__ Y2 = reinterpret_cast<const double2*>(Y);
  const int64_t ld2 = ld >> 1;
  const int64_t stride = (int64_t)gridDim.x * kLrThreads;
  for (int64_t p = (int64_t)blockIdx.x * kLrThreads + threadIdx.x; p < np; p += stride) {
    double2 v[kLrTile], y[kLrTile];
#pragma unroll
    for (int a = 0; a < kLrTile; ++a) {
      v[a] = i0 + a < k ? V2[(int64_t)(i0 + a) * ld2 + p] : make_double2(0.0, 0.0);
      y[a] = j0 + a < k ? Y2[(int64_t)(j0 + a) * ld2 + p] : make_double2(0.0, 0.0);
    }
#pragma unroll
    for (int a = 0; a < kLrTile; ++a)
#pragma unroll
      for (int b = 0; b < kLrTile; ++b) {
        acc[a * kLrTile + b] = fma(v[a].x, y[b].x, acc[a * kLrTile + b]);
        acc[a * kLrTile + b] = fma(v[a].y, y[b].y, acc[a * kLrTile + b]);
      }
  }
  double* o = gpart + (int64_t)blockIdx.x * (kLrMax * kLrMax);
#pragma unroll
  for (int a = 0; a < kLrTile; ++a) lr_block_sums8(acc + a * kLrTile, sd, o + (i0 + a) * kLrMax + j0);
}

// finisher: entry (i, j) folded in workgroup order; C = I + G; max |G_ij|
__global__ __launch_bounds__(kLrThreads) void k_lr_gram_fin(int nparts, int k, const double* __restrict__ gpart,
                                                            LrState* __restrict__ st) {
  __shared__ double sd[kLrThreads];
  double gmax = 0.0;
  for (int e = threadIdx.x; e < kLrMax * kLrMax; e += kLrThreads) {
    const int i = e / kLrMax, j = e % kLrMax;
    double s = 0.0;
    if (i < k && j < k) {
      for (int b = 0; b < nparts; ++b) s += gpart[(int64_t)b * (kLrMax * kLrMax) + e];
      // a NaN must reach the record: fmax would drop it
      gmax = (fabs(s) > gmax || s != s) ? fabs(s) : gmax;
    }
    st->C[e] = (i == j ? 1.0 : 0.0) + s;
  }
  // NaN-propagating maximum of the workgroup
  const int t = threadIdx.x;
  sd[t] = gmax;
  __syncthreads();
  for (int o = kLrThreads / 2; o > 0; o >>= 1) {
    if (t < o) {
      const double a = sd[t], b = sd[t + o];
      sd[t] = (a != a || b != b) ? __builtin_nan("") : fmax(a, b);
    }
    __syncthreads();
  }
  if (t == 0) st->gram_max = sd[0];
}

// ---- capacitance matrix -------------------------------------------------------------------------
// One workgroup: LU of C (k x k) in LDS with partial pivoting (the first largest |.| of the column),
// the explicit inverse column by column, ||C||_1 ||C^-1||_1, min |u_ii|.
// rec = {seq, flag, rcond_c, pivot_min, gram_max, .., seq}; flag: 0 installed; 1 a pivot exactly zero
// (or not finite); 2 a non-finite entry of C.  With a flag C^-1 is not written.
__global__ __launch_bounds__(kLrThreads) void k_lr_capacitance(int k, LrState* __restrict__ st, long long* __restrict__ rec,
                                                               long long seq) {
  __shared__ double a[kLrMax][kLrMax + 1];
  __shared__ double x[kLrMax][kLrMax + 1];
  __shared__ double cn[kLrMax], xn[kLrMax];
  __shared__ int piv[kLrMax];
  __shared__ int flag;
  __shared__ double pmin;
  const int t = threadIdx.x;
  if (t == 0) {
    flag = 0;
    pmin = HUGE_VAL;
  }
  __syncthreads();
  bool bad = false;
  for (int e = t; e < kLrMax * kLrMax; e += kLrThreads) {
    const int i = e / kLrMax, j = e % kLrMax;
    const double v = (i < k && j < k) ? st->C[e] : (i == j ? 1.0 : 0.0);
    a[i][j] = v;
    bad = bad || !isfinite(v);
  }
  if (bad) flag = 2;   // every writer stores the same value
  __syncthreads();
  if (t < k) {
    double s = 0.0;
    for (int i = 0; i < k; ++i) s += fabs(a[i][t]);
    cn[t] = s;
  }
  __syncthreads();
  if (flag == 0) {
    for (int j = 0; j < k; ++j) {
      if (t == 0) {
        int p = j;
        double best = fabs(a[j][j]);
        for (int i = j + 1; i < k; ++i)
          if (fabs(a[i][j]) > best) {
            best = fabs(a[i][j]);
            p = i;
          }
        piv[j] = p;
        if (!(best > 0.0) || !isfinite(best)) flag = 1;
        pmin = fmin(pmin, best);
      }
      __syncthreads();
      if (flag != 0) break;   // uniform: read after the barrier
      const int p = piv[j];
      if (p != j && t < k) {
        const double u = a[j][t];
        a[j][t] = a[p][t];
        a[p][t] = u;
      }
      __syncthreads();
      if (t > j && t < k) a[t][j] = a[t][j] / a[j][j];
      __syncthreads();
      for (int e = t; e < kLrMax * kLrMax; e += kLrThreads) {
        const int i = e / kLrMax, c = e % kLrMax;
        if (i > j && c > j && i < k && c < k) a[i][c] = fma(-a[i][j], a[j][c], a[i][c]);
      }
      __syncthreads();
    }
  }
  __syncthreads();
  const bool ok = flag == 0;
  if (ok && t < k) {   // column t of C^-1: L U x = P e_t
    for (int i = 0; i < k; ++i) x[i][t] = i == t ? 1.0 : 0.0;
    for (int j = 0; j < k; ++j) {
      const int p = piv[j];
      const double u = x[j][t];
      x[j][t] = x[p][t];
      x[p][t] = u;
    }
    for (int i = 1; i < k; ++i) {
      double s = x[i][t];
      for (int m = 0; m < i; ++m) s = fma(-a[i][m], x[m][t], s);
      x[i][t] = s;
    }
    double nrm = 0.0;
    for (int i = k - 1; i >= 0; --i) {
      double s = x[i][t];
      for (int m = i + 1; m < k; ++m) s = fma(-a[i][m], x[m][t], s);
      s = s / a[i][i];
      x[i][t] = s;
      nrm += fabs(s);
    }
    xn[t] = nrm;
  }
  __syncthreads();
  if (ok)
    for (int e = t; e < kLrMax * kLrMax; e += kLrThreads) {
      const int i = e / kLrMax, j = e % kLrMax;
      st->Cinv[e] = (i < k && j < k) ? x[i][j] : 0.0;
    }
  if (t == 0) {
    double rcond = 0.0;
    if (ok) {
      double cmax = 0.0, xmax = 0.0;
      for (int j = 0; j < k; ++j) {
        cmax = fmax(cmax, cn[j]);
        xmax = fmax(xmax, xn[j]);
      }
      const double d = cmax * xmax;
      rcond = (d > 0.0 && isfinite(d)) ? 1.0 / d : 0.0;
    }
    rec[1] = flag;
    rec[2] = __double_as_longlong(rcond);
    rec[3] = __double_as_longlong(flag == 2 ? 0.0 : pmin);
    rec[4] = __double_as_longlong(st->gram_max);
    rec[0] = seq;
    rec[7] = seq;
  }
}

// ---- the solve's passes -----------------------------------------------------------------------
// part[blockIdx.x][c] = sum over this workgroup's rows of W[:, c] x, c < k: all k dot products in one
// pass, x loaded once, the sums in registers.  BOTH: beside them, in the same pass, the dots of the
// absolute values |W[:, c]| |x| into part[blockIdx.x][kLrMax + c] (the residual's denominator).
// NC: columns the instantiation holds (k <= NC); W is loaded eight columns at a time.
template <int NC, bool BOTH>
__global__ __launch_bounds__(kLrThreads) void k_lr_dots(int64_t np, int64_t ld, int k, const double* __restrict__ W,
                                                        const double* __restrict__ x, double* __restrict__ part) {
  __shared__ double sd[8 * kLrThreads];
  constexpr int NA = NC < 8 ? 8 : NC;   // the tree folds eight columns a round
  constexpr int CH = NC < 8 ? NC : 8;
  double acc[NA], acca[BOTH ? NA : 1];
#pragma unroll
  for (int c = 0; c < NA; ++c) {
    acc[c] = 0.0;
    if (BOTH) acca[c] = 0.0;
  }
  const double2* __restrict__ W2 = reinterpret_cast<const double2*>(W);
  const double2* __restrict__ x2 = reinterpret_cast<const double2*>(x);
  const int64_t ld2 = ld >> 1;
  const int64_t stride = (int64_t)gridDim.x * kLrThreads;
  for (int64_t p = (int64_t)blockIdx.x * kLrThreads + threadIdx.x; p < np; p += stride) {
    const double2 xv = x2[p];
    const double2 xa = make_double2(fabs(xv.x), fabs(xv.y));
#pragma unroll
    for (int c0 = 0; c0 < NC; c0 += CH) {
      double2 wv[CH];
#pragma unroll
      for (int c = 0; c < CH; ++c)
        if (c0 + c < k) wv[c] = W2[(c0 + c) * ld2 + p];
#pragma unroll
      for (int c = 0; c < CH; ++c)
        if (c0 + c < k) {
          acc[c0 + c] = fma(wv[c].x, xv.x, acc[c0 + c]);
          acc[c0 + c] = fma(wv[c].y, xv.y, acc[c0 + c]);
          if (BOTH) {
            acca[c0 + c] = fma(fabs(wv[c].x), xa.x, acca[c0 + c]);
            acca[c0 + c] = fma(fabs(wv[c].y), xa.y, acca[c0 + c]);
          }
        }
    }
  }
  double* o = part + (int64_t)blockIdx.x * kLrPartStride;
#pragma unroll
  for (int c0 = 0; c0 < NA; c0 += 8)
    if (c0 < k) {
      lr_block_sums8(acc + c0, sd, o + c0);
      if (BOTH) lr_block_sums8(acca + c0, sd, o + kLrMax + c0);
    }
}

// x = x - Yw c in place, c = C^-1 t (T: C^-T t), t the dots' partials folded in workgroup order by
// every workgroup for itself; the pad row is stored as 0.
template <int NC, bool T>
__global__ __launch_bounds__(kLrThreads) void k_lr_apply(int64_t n, int64_t np, int64_t ld, int k, int nparts,
                                                         const double* __restrict__ part,
                                                         const LrState* __restrict__ st, const double* __restrict__ Yw,
                                                         double* __restrict__ x) {
  __shared__ double tt[kLrMax], cc[kLrMax];
  const int t = threadIdx.x;
  if (t < k) {
    double s = 0.0;
    for (int b = 0; b < nparts; ++b) s += part[(int64_t)b * kLrPartStride + t];
    tt[t] = s;
  }
  __syncthreads();
  if (t < k) {
    double s = 0.0;
    for (int j = 0; j < k; ++j) s = fma(T ? st->Cinv[j * kLrMax + t] : st->Cinv[t * kLrMax + j], tt[j], s);
    cc[t] = s;
  }
  __syncthreads();
  double cf[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) cf[c] = c < k ? cc[c] : 0.0;
  const double2* __restrict__ Y2 = reinterpret_cast<const double2*>(Yw);
  double2* __restrict__ x2 = reinterpret_cast<double2*>(x);
  const int64_t ld2 = ld >> 1;
  const int64_t stride = (int64_t)gridDim.x * kLrThreads;
  for (int64_t p = (int64_t)blockIdx.x * kLrThreads + t; p < np; p += stride) {
    double2 xv = x2[p];
    double2 yv[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (c < k) yv[c] = Y2[c * ld2 + p];
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (c < k) {
        xv.x = fma(-cf[c], yv[c].x, xv.x);
        xv.y = fma(-cf[c], yv[c].y, xv.y);
      }
    if (2 * p + 1 >= n) xv.y = 0.0;
    x2[p] = xv;
  }
}

// (op(A) x)_i and (|op(A)| |x|)_i: kernels_krylov.hip's kry_row, the same order of the entries
template <bool T>
__device__ __forceinline__ double lr_row(int64_t i, const int64_t* __restrict__ ptr, const int32_t* __restrict__ ent,
                                         const int32_t* __restrict__ acol, const int32_t* __restrict__ arow,
                                         const double* __restrict__ a, const double* __restrict__ x, double* den) {
  double acc = 0.0, d = 0.0;
  for (int64_t e = ptr[i]; e < ptr[i + 1]; ++e) {
    const int64_t m = T ? e : (int64_t)ent[e];
    const double xm = x[T ? arow[m] : acol[m]];
    acc = fma(a[m], xm, acc);
    d = fma(fabs(a[m]), fabs(xm), d);
  }
  *den = d;
  return acc;
}

// r = b - op(A) x - W s with s = Wd^T x and sa = |Wd|^T |x| folded from the dots pass'
// partials (columns [0, k) and [kLrMax, kLrMax + k) of part) by every workgroup for itself; the
// product with W rides in the row loop.  Partials of max |r_i| and of the componentwise backward
// error max_i |r_i| / (|op(A)||x| + |W| sa + |b|)_i go to columns 2 kLrMax and 2 kLrMax + 1.
template <bool T>
__global__ __launch_bounds__(kLrThreads) void k_lr_resid(int64_t n, int64_t ld, int k, int nparts,
                                                         const int64_t* __restrict__ ptr, const int32_t* __restrict__ ent,
                                                         const int32_t* __restrict__ acol,
                                                         const int32_t* __restrict__ arow, const double* __restrict__ a,
                                                         const double* __restrict__ x, const double* __restrict__ b,
                                                         const double* __restrict__ W, double* __restrict__ r,
                                                         double* part) {
  __shared__ double sd[kLrThreads];
  __shared__ double s[2 * kLrMax];
  const int t = threadIdx.x;
  if (t < 2 * kLrMax) {
    const int c = t % kLrMax;
    double v = 0.0;
    if (c < k)
      for (int q = 0; q < nparts; ++q) v += part[(int64_t)q * kLrPartStride + t];
    s[t] = v;
  }
  __syncthreads();
  double rmax = 0.0, worst = 0.0;
  const int64_t stride = (int64_t)gridDim.x * kLrThreads;
  for (int64_t i = (int64_t)blockIdx.x * kLrThreads + t; i < n; i += stride) {
    double den;
    const double acc = lr_row<T>(i, ptr, ent, acol, arow, a, x, &den);
    double ws = 0.0;
    for (int c = 0; c < k; ++c) {
      const double w = W[(int64_t)c * ld + i];
      ws = fma(w, s[c], ws);
      den = fma(fabs(w), s[kLrMax + c], den);
    }
    const double bi = b[i];
    const double ri = (bi - acc) - ws;
    r[i] = ri;
    den += fabs(bi);
    // a NaN residual must not vanish in fmax
    rmax = (fabs(ri) > rmax || ri != ri) ? fabs(ri) : rmax;
    const double q = ri == 0.0 ? 0.0 : den > 0.0 ? fabs(ri) / den : HUGE_VAL;
    worst = (q > worst || q != q) ? q : worst;
  }
  // the two maxima; a NaN is carried as +inf through the tree (fmax drops NaN)
  rmax = lr_block_max(rmax != rmax ? HUGE_VAL : rmax, sd);
  worst = lr_block_max(worst != worst ? HUGE_VAL : worst, sd);
  if (t == 0) {
    part[(int64_t)blockIdx.x * kLrPartStride + 2 * kLrMax] = rmax;
    part[(int64_t)blockIdx.x * kLrPartStride + 2 * kLrMax + 1] = worst;
  }
}

// rec = {seq, max |r_i|, berr, .., seq}
__global__ __launch_bounds__(kLrThreads) void k_lr_resid_fin(int nparts, const double* __restrict__ part,
                                                             long long* __restrict__ rec, long long seq) {
  __shared__ double sd[kLrThreads];
  double rmax = 0.0, worst = 0.0;
  for (int b = threadIdx.x; b < nparts; b += kLrThreads) {
    rmax = fmax(rmax, part[(int64_t)b * kLrPartStride + 2 * kLrMax]);
    worst = fmax(worst, part[(int64_t)b * kLrPartStride + 2 * kLrMax + 1]);
  }
  rmax = lr_block_max(rmax, sd);
  worst = lr_block_max(worst, sd);
  if (threadIdx.x == 0) {
    rec[1] = __double_as_longlong(rmax);
    rec[2] = __double_as_longlong(worst);
    rec[0] = seq;
    rec[7] = seq;
  }
}

// ---- launchers ------------------------------------------------------------------------------
#define SMLU_LR(expr) \
  do {                \
    expr;             \
    hipError_t _e = hipGetLastError(); \
    if (_e != hipSuccess) return _e;   \
  } while (0)

// by the smallest instantiation that holds k columns
#define SMLU_LR_NC(k, CALL)       \
  do {                            \
    if ((k) <= 4) CALL(4);        \
    else if ((k) <= 8) CALL(8);   \
    else if ((k) <= 16) CALL(16); \
    else CALL(32);                \
  } while (0)

static inline bool lr_shape_ok(int64_t n, int64_t ld, int k) {
  return k >= 1 && k <= kLrMax && n >= 1 && !(ld & 1) && ld >= n && ld <= n + 1;
}

// k columns of the caller's matrix (leading dimension lds >= n) into dst (leading dimension ld)
hipError_t launch_lr_stage(hipStream_t st, int64_t n, int64_t ld, int k, const double* src, int64_t lds, double* dst) {
  if (!lr_shape_ok(n, ld, k) || lds < n) return hipErrorInvalidValue;
  SMLU_LR((k_lr_stage<<<dim3(lr_blocks(n), k), kLrThreads, 0, st>>>(n, ld, src, lds, dst)));
  return hipSuccess;
}

// C = I + V^T Y, its LU and inverse into the state, the record stamped seq.  gpart: kDgMaxBlocks x
// kLrMax^2 doubles.
hipError_t launch_lr_capacitance(hipStream_t st, int64_t n, int64_t ld, int k, const double* V, const double* Y,
                                 double* gpart, void* state, long long* rec, long long seq) {
  if (!lr_shape_ok(n, ld, k)) return hipErrorInvalidValue;
  const int64_t np = ld >> 1;
  const int nb = lr_blocks(np);
  const int kt = (k + kLrTile - 1) / kLrTile;
  LrState* s = static_cast<LrState*>(state);
  SMLU_LR((k_lr_gram<<<dim3(nb, kt * kt), kLrThreads, 0, st>>>(np, ld, k, V, Y, gpart)));
  SMLU_LR((k_lr_gram_fin<<<1, kLrThreads, 0, st>>>(nb, k, gpart, s)));
  SMLU_LR((k_lr_capacitance<<<1, kLrThreads, 0, st>>>(k, s, rec, seq)));
  return hipSuccess;
}

// x = x - Yw C^-1 (Wd^T x) in place (trans: C^-T): the dots pass and the apply pass.  x: ld doubles.
hipError_t launch_lr_correct(hipStream_t st, bool trans, int64_t n, int64_t ld, int k, const double* Wd, const double* Yw,
                             const void* state, double* part, double* x) {
  if (!lr_shape_ok(n, ld, k)) return hipErrorInvalidValue;
  const int64_t np = ld >> 1;
  const int nb = lr_blocks(np);
  const LrState* s = static_cast<const LrState*>(state);
#define LR_DOTS(N) SMLU_LR((k_lr_dots<N, false><<<nb, kLrThreads, 0, st>>>(np, ld, k, Wd, x, part)))
#define LR_APPLY_N(N) SMLU_LR((k_lr_apply<N, false><<<nb, kLrThreads, 0, st>>>(n, np, ld, k, nb, part, s, Yw, x)))
#define LR_APPLY_T(N) SMLU_LR((k_lr_apply<N, true><<<nb, kLrThreads, 0, st>>>(n, np, ld, k, nb, part, s, Yw, x)))
  SMLU_LR_NC(k, LR_DOTS);
  if (trans) SMLU_LR_NC(k, LR_APPLY_T);
  else SMLU_LR_NC(k, LR_APPLY_N);
#undef LR_DOTS
#undef LR_APPLY_N
#undef LR_APPLY_T
  return hipSuccess;
}

// r = b - op(A) x - W (Wd^T x) with its max-norm and the backward error of x in the record stamped
// seq; k = 0: the residual of A alone.  x, b, r: ld doubles with a zero pad row.
hipError_t launch_lr_resid(hipStream_t st, bool trans, int64_t n, int64_t ld, int k, const int64_t* rowptr,
                           const int32_t* ent, const int32_t* acol, const int64_t* colptr, const int32_t* arow,
                           const double* a, const double* x, const double* b, const double* W, const double* Wd, double* r,
                           double* part, long long* rec, long long seq) {
  if (k != 0 && !lr_shape_ok(n, ld, k)) return hipErrorInvalidValue;
  if (k < 0 || n < 1) return hipErrorInvalidValue;
  const int64_t np = ld >> 1;
  const int nbp = lr_blocks(np), nb = lr_blocks(n);
  if (k > 0) {
#define LR_DOTS2(N) SMLU_LR((k_lr_dots<N, true><<<nbp, kLrThreads, 0, st>>>(np, ld, k, Wd, x, part)))
    SMLU_LR_NC(k, LR_DOTS2);
#undef LR_DOTS2
  }
  if (trans)
    SMLU_LR((k_lr_resid<true><<<nb, kLrThreads, 0, st>>>(n, ld, k, nbp, colptr, ent, acol, arow, a, x, b, W, r, part)));
  else
    SMLU_LR((k_lr_resid<false><<<nb, kLrThreads, 0, st>>>(n, ld, k, nbp, rowptr, ent, acol, arow, a, x, b, W, r, part)));
  SMLU_LR((k_lr_resid_fin<<<1, kLrThreads, 0, st>>>(nb, part, rec, seq)));
  return hipSuccess;
}

}  // namespace smlu
