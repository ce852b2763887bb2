// kernels_solve_t.hip — the transposed / adjoint solve (A^T x = b, A^H x = b) from the factors of A.
// The handle holds (Rs .* A)[p0, q] = P_fronts^T L U, so A^T x = b is
//   w = b[q];  U^T y = w (leaves -> root);  z = (P_fronts^T L)^-T y (root -> leaves);  x[p0] = Rs[p0] .* z.
// Both passes walk the forward solve's per-block launch sequences (fwdm / bwdm) and reinterpret each
// launch by kind on the same work lists and workgroup counts (solve.cpp: run_solve_launch_t).
// Storage is column-major (L panel M x ns, ld M, U11 in its upper triangle; U12 ns x nu, ld ns), so in
// the transposed solve every product is a dot product along a contiguous column run: a 16-lane group
// takes a run 128 bytes at a time and reduces across its lanes in a fixed order (no floating-point
// atomics: two solves of the same b are bitwise equal).  The diagonal blocks are staged in LDS by
// coalesced loads and read back transposed with an odd stride (no bank conflicts), one row per lane.
// Every wait is stream order; no workgroup waits for another.
// One template per kernel on the batch width NR >= rh.n (1, 4, 8 or 16, as in kernels_solve.hip).
// Column r of the work vector is at x + r*rh.ldx, of the front vectors at vbuf + r*rh.ldv; launch
// geometry, work lists and workgroup counts do not depend on the width.  Every factor value (panel,
// U12, staged diagonal block) is loaded once per launch and applied to all columns of the batch: the
// substitution chains of the NR columns are interleaved step by step (tri64_rows), the dot products
// keep the loaded runs in registers and walk the columns inside the kernel.  Per column the
// operations and their order do not depend on NR (lane split of dots16, fma order, red16 / red16x16
// trees, 1/u_jj pre-scaling, rowperm scatter) and nothing is summed across columns, so column j of a
// batch is bitwise the one-column solve of that column.  Slots r >= rh.n run on zeros in registers
// and are never read from or written to memory; at NR = 1 the column count is the constant 1.
#include "kernels_common.hpp"

namespace smlu {

// the columns a kernel of width NR has to serve
template <int NR>
__device__ __forceinline__ int rhs_count(Rhs rh) {
  return NR == 1 ? 1 : rh.n;
}

// sum over the 16 lanes of a group (every lane of the wave takes part), the same tree on every call
__device__ __forceinline__ double red16(double a) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
  return a;
}

// Sixteen sums at once: lane e of a group holds partial sums a[0..15] of sixteen targets and leaves
// with the group's total of target e (recursive halving: 8 + 4 + 2 + 1 exchanges instead of 16 x 4,
// the additions of every target in the same fixed order on every call).  Both halves are read into
// values before the lane's choice between them, so the sixteen sums stay in registers however many
// column bodies the compiler sees at once.
__device__ __forceinline__ double red16x16(double (&a)[16], int e) {
#pragma unroll
  for (int h = 8; h > 0; h >>= 1) {
    const bool up = (e & h) != 0;
#pragma unroll
    for (int i = 0; i < h; ++i) {
      const double lo = a[i], hi = a[i + h];
      const double send = up ? lo : hi;
      const double keep = up ? hi : lo;
      a[i] = keep + __shfl_xor(send, h, 64);
    }
  }
  return a[0];
}

// 64 x 64 diagonal block D (ld M) -> sD[col * 65 + row] by all 256 threads (coalesced along a column)
__device__ __forceinline__ void stage_block_t(double* __restrict__ sD, const double* __restrict__ D, int64_t M,
                                              int bw, int tid) {
  for (int idx = tid; idx < bw * 64; idx += 256) {
    const int i = idx & 63, j = idx >> 6;
    if (i < bw) sD[j * 65 + i] = D[(int64_t)j * M + i];
  }
}

// tiny fronts: a per-wave LDS tile T[col * 33 + row] of 32 columns of the triangle (coalesced along
// the panel columns), read back one panel column per lane
constexpr int kTinyWaves = 2;
__device__ __forceinline__ void stage_tile_t(double* __restrict__ T, const double* __restrict__ Lp, int M, int ns,
                                             int c0, int cw, int lane) {
  for (int idx = lane; idx < ns * 32; idx += 64) {
    const int r = idx & 31, i = idx >> 5;
    if (r < cw) T[i * 33 + r] = Lp[(int64_t)i * M + c0 + r];
  }
}
__device__ __forceinline__ int pow2_at_least(int n) {
  int g = 1;
  while (g < n && g < 64) g <<= 1;
  return g;
}

// ---- dot products over contiguous runs: 16 lanes per run ------------------------------------
// a[r][u] += sum over idx = e, e + 16, ... < len of ptr[u][idx] * xv[r * ldxv + idx] (e = lane within
// the group): four strides of 16 per round, the loads of a round issued before its fmas and applied
// to every column (per column and target the same products in the same order).
template <int NR, int U>
__device__ __forceinline__ void dots16(const double* const (&ptr)[U], const bool (&ok)[U], const double* xv,
                                       int64_t ldxv, int nrhs, int64_t len, int e, double (&a)[NR][U]) {
  for (int64_t i0 = 0; i0 < len; i0 += 64) {
    double d[U][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t idx = i0 + e + 16 * k;
#pragma unroll
      for (int u = 0; u < U; ++u) d[u][k] = (ok[u] && idx < len) ? ptr[u][idx] : 0.0;
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      double xx[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int64_t idx = i0 + e + 16 * k;
        xx[k] = (r < nrhs && idx < len) ? xv[r * ldxv + idx] : 0.0;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int u = 0; u < U; ++u) a[r][u] = fma(d[u][k], xx[k], a[r][u]);
    }
  }
}

// v_r[t] -= <col(t)[0 : bw), ys[r]> for the targets t in [lo, hi), bw <= 64: 16 groups of 16 lanes
// (256 threads), four targets per group and round.  col(t) -> start of the target's contiguous run.
// One round of dots16, so the four runs of a group stay in registers while the columns go by.
template <int NR, class COL>
__device__ __forceinline__ void apply_dots(int64_t lo, int64_t hi, int bw, const double (*ys)[64],
                                           double* __restrict__ v, Rhs rh, int tid, COL&& col) {
  constexpr int U = 4;
  const int nr = rhs_count<NR>(rh);
  const int g = tid >> 4, e = tid & 15;
  for (int64_t t0 = lo; t0 < hi; t0 += 16 * U) {
    bool ok[U];
    double d[U][4];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t t = t0 + u * 16 + g;
      ok[u] = t < hi;
      const double* ptr = col(ok[u] ? t : lo);
#pragma unroll
      for (int k = 0; k < 4; ++k) d[u][k] = (ok[u] && e + 16 * k < bw) ? ptr[e + 16 * k] : 0.0;
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      if (r < nr) {   // the whole workgroup
        double xx[4], a[U];
#pragma unroll
        for (int k = 0; k < 4; ++k) xx[k] = e + 16 * k < bw ? ys[r][e + 16 * k] : 0.0;
#pragma unroll
        for (int u = 0; u < U; ++u) a[u] = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
          for (int u = 0; u < U; ++u) a[u] = fma(d[u][k], xx[k], a[u]);
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const double res = red16(a[u]);
          const int64_t t = t0 + u * 16 + g;
          if (e == 0 && ok[u]) v[r * rh.ldv + t] = v[r * rh.ldv + t] - res;
        }
      }
    }
  }
}

// One wave solves the staged block transposed for NR columns: the block read once per step, the NR
// chains interleaved.  Row `lane` of the transposed block is the block's column `lane`:
// sD[lane * 65 + j] (stride 65 across lanes).
//   !UPPER: U11^T y = x, non-unit lower (entries j <= lane), ascending;
//    UPPER: L11^T t = x, unit upper (entries j > lane), descending.
template <bool UPPER, int NR>
__device__ __forceinline__ void tri_lds_t(double (&xi)[NR], const double* __restrict__ sD, int bw, int lane) {
  const bool in = lane < bw;
  if (!UPPER) {
    const double dinv = in ? recip(sD[lane * 65 + lane]) : 1.0;
    for (int j = 0; j < bw; ++j) {
      const double sj = sD[lane * 65 + j];
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        xi[r] = lane == j ? xi[r] * dinv : xi[r];
        const double t = fma(-sj, readlane_f64(xi[r], j), xi[r]);
        xi[r] = (lane > j && in) ? t : xi[r];
      }
    }
  } else {
    for (int j = bw - 1; j > 0; --j) {
      const double sj = sD[lane * 65 + j];
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const double t = fma(-sj, readlane_f64(xi[r], j), xi[r]);
        xi[r] = lane < j ? t : xi[r];
      }
    }
  }
}

// Runs per 16-lane group and round in the long dot products (L21^T z[R]): NR x U accumulators per
// lane, held to 32 (a target's sum does not depend on which group or round takes it).
template <int NR>
struct LongRuns {
  static constexpr int U = NR >= 16 ? 2 : 4;
};

// ---- small fronts: one workgroup per front ---------------------------------------------------
// U^T step: y1 = U11^-T v1 in 64-column blocks; every block is applied to the rows after it, the
// front's own (panel columns) and the update rows (U12 columns): v[t] -= <col_t[jb : jb+bw), y_blk>.
template <int NR>
__global__ __launch_bounds__(256) void k_ut_front(const int32_t* __restrict__ list, const SNode* __restrict__ sn,
                                                  const int32_t* __restrict__ chlist,
                                                  const int32_t* __restrict__ relmap,
                                                  const double* __restrict__ store, double* __restrict__ x,
                                                  double* __restrict__ vbuf, Rhs rh) {
  const int nr = rhs_count<NR>(rh);
  __shared__ double sD[64 * 65];
  __shared__ double ys[NR][64];
  const SNode s = sn[list[blockIdx.x]];
  const int64_t M = (int64_t)s.ns + s.nu, ns = s.ns;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  double* v = vbuf + s.voff;
  // front vectors = own rows of x + the children's update vectors, children in order (no row
  // permutation: the columns of U are not pivoted)
  for (int64_t i = tid; i < M; i += 256)
#pragma unroll
    for (int r = 0; r < NR; ++r)
      if (r < nr) v[r * rh.ldv + i] = i < ns ? x[r * rh.ldx + s.first + i] : 0.0;
  __syncthreads();
  for (int c = s.chbeg; c < s.chend; ++c) {
    const SNode ch = sn[chlist[c]];
    const int32_t* rm = relmap + ch.rowptr;
    const double* cv = vbuf + ch.voff + ch.ns;
    for (int64_t i = tid; i < ch.nu; i += 256) {
      const int32_t t = rm[i];   // a child's rows are distinct
#pragma unroll
      for (int r = 0; r < NR; ++r)
        if (r < nr) v[r * rh.ldv + t] = v[r * rh.ldv + t] + cv[r * rh.ldv + i];
    }
    __syncthreads();
  }
  const double* Lp = store + s.Loff;
  const double* U12 = store + s.Uoff;
  for (int64_t jb = 0; jb < ns; jb += 64) {
    const int bw = (int)min<int64_t>(64, ns - jb);
    stage_block_t(sD, Lp + jb * M + jb, M, bw, tid);
    __syncthreads();
    if (wv == 0) {
      double xi[NR];
#pragma unroll
      for (int r = 0; r < NR; ++r) xi[r] = (lane < bw && r < nr) ? v[r * rh.ldv + jb + lane] : 0.0;
      tri_lds_t<false, NR>(xi, sD, bw, lane);
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        ys[r][lane] = lane < bw ? xi[r] : 0.0;
        if (lane < bw && r < nr) {
          v[r * rh.ldv + jb + lane] = xi[r];
          x[r * rh.ldx + s.first + jb + lane] = xi[r];
        }
      }
    }
    __syncthreads();
    apply_dots<NR>(jb + bw, M, bw, ys, v, rh, tid,
                   [&](int64_t t) { return t < ns ? Lp + t * M + jb : U12 + (t - ns) * ns + jb; });
    __syncthreads();
  }
}

// L^T step: v1 = y1 - L21^T z[R] (z[R] gathered into the front vector's update rows, then one dot
// product per panel column tail), L11^T in 64-column blocks from the last, result scattered through
// the front's row permutation.
template <int NR>
__global__ __launch_bounds__(256) void k_lt_front(const int32_t* __restrict__ list, const SNode* __restrict__ sn,
                                                  const int32_t* __restrict__ rows,
                                                  const int32_t* __restrict__ rowperm,
                                                  const double* __restrict__ store, double* __restrict__ x,
                                                  double* __restrict__ vbuf, Rhs rh) {
  const int nr = rhs_count<NR>(rh);
  __shared__ double sD[64 * 65];
  __shared__ double ys[NR][64];
  const SNode s = sn[list[blockIdx.x]];
  const int64_t M = (int64_t)s.ns + s.nu, ns = s.ns, nu = s.nu;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int32_t* R = rows + s.rowptr;
  const double* Lp = store + s.Loff;
  double* v = vbuf + s.voff;
  for (int64_t t = tid; t < nu; t += 256) {
    const int32_t rt = R[t];
#pragma unroll
    for (int r = 0; r < NR; ++r)
      if (r < nr) v[r * rh.ldv + ns + t] = x[r * rh.ldx + rt];
  }
  for (int64_t j = tid; j < ns; j += 256)
#pragma unroll
    for (int r = 0; r < NR; ++r)
      if (r < nr) v[r * rh.ldv + j] = x[r * rh.ldx + s.first + j];
  __syncthreads();
  if (nu > 0) {   // v1 = y1 - L21^T z[R]: the runs of a group loaded once per 64 entries for all columns
    constexpr int U = LongRuns<NR>::U;
    const int g = tid >> 4, e = tid & 15;
    for (int64_t j0 = 0; j0 < ns; j0 += 16 * U) {
      const double* ptr[U];
      bool ok[U];
      double a[NR][U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t j = j0 + u * 16 + g;
        ok[u] = j < ns;
        ptr[u] = Lp + (ok[u] ? j : 0) * M + ns;
#pragma unroll
        for (int r = 0; r < NR; ++r) a[r][u] = 0.0;
      }
      dots16<NR, U>(ptr, ok, v + ns, rh.ldv, nr, nu, e, a);
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        if (r < nr) {
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const double res = red16(a[r][u]);
            const int64_t j = j0 + u * 16 + g;
            if (e == 0 && ok[u]) v[r * rh.ldv + j] = v[r * rh.ldv + j] - res;
          }
        }
      }
    }
    __syncthreads();
  }
  for (int64_t jb = ((ns - 1) / 64) * 64; jb >= 0; jb -= 64) {
    const int bw = (int)min<int64_t>(64, ns - jb);
    stage_block_t(sD, Lp + jb * M + jb, M, bw, tid);
    __syncthreads();
    if (wv == 0) {
      double xi[NR];
#pragma unroll
      for (int r = 0; r < NR; ++r) xi[r] = (lane < bw && r < nr) ? v[r * rh.ldv + jb + lane] : 0.0;
      tri_lds_t<true, NR>(xi, sD, bw, lane);
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        ys[r][lane] = lane < bw ? xi[r] : 0.0;
        if (lane < bw && r < nr) v[r * rh.ldv + jb + lane] = xi[r];
      }
    }
    __syncthreads();
    apply_dots<NR>(0, jb, bw, ys, v, rh, tid, [&](int64_t t) { return Lp + t * M + jb; });
    __syncthreads();
  }
  // descendants read z at pre-pivot positions
  for (int64_t i = tid; i < ns; i += 256) {
    const int64_t dst = s.first + rowperm[s.first + i];
#pragma unroll
    for (int r = 0; r < NR; ++r)
      if (r < nr) x[r * rh.ldx + dst] = v[r * rh.ldv + i];
  }
}

// ---- tiny fronts (M <= 128 rows, ns <= 64 pivots): one wave per front, two fronts per workgroup,
// no workgroup barrier.  The triangle is staged 32 columns at a time into a per-wave LDS tile
// T[col * 33 + row] (coalesced along the panel columns) and read back one panel column per lane; the
// U12 / L21 products give G = 2^ceil(log2(len)) lanes to each contiguous run.
// The per-wave tile T is the only LDS (8 waves per CU).  Before the triangle is staged and after it
// has been used, T holds the front vectors of the batch, column r at T + r * 128 (M <= 128); during
// the chains they live in registers (two per lane and column).
constexpr int kTinyT = 64 * 33;
// accumulators per lane in the U12 / L21 products: NR columns x U runs
template <int NR>
struct TinyRuns {
  static constexpr int U = NR >= 16 ? 1 : NR >= 8 ? 2 : 4;
};

template <int NR>
__global__ __launch_bounds__(64 * kTinyWaves) void k_ut_tiny(const int32_t* __restrict__ list, int cnt,
                                                             const SNode* __restrict__ sn,
                                                             const int32_t* __restrict__ chlist,
                                                             const int32_t* __restrict__ relmap,
                                                             const double* __restrict__ store,
                                                             double* __restrict__ x, double* __restrict__ vbuf,
                                                             Rhs rh) {
  const int nr = rhs_count<NR>(rh);
  static_assert(NR * 128 <= kTinyT, "the batch's front vectors share the tile");
  constexpr int U = TinyRuns<NR>::U;
  __shared__ double sT[kTinyWaves][kTinyT];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t f = (int64_t)blockIdx.x * kTinyWaves + wv;
  if (f >= cnt) return;   // the whole wave
  const SNode s = sn[list[f]];
  const int ns = s.ns, nu = s.nu, M = ns + nu;
  const double* Lp = store + s.Loff;
  double* T = sT[wv];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    T[r * 128 + lane] = (lane < ns && r < nr) ? x[r * rh.ldx + s.first + lane] : 0.0;
    T[r * 128 + 64 + lane] = 0.0;
  }
  wave_lds_sync();
  for (int c = s.chbeg; c < s.chend; ++c) {   // parent += child, children in order
    const SNode ch = sn[chlist[c]];
    for (int q = lane; q < ch.nu; q += 64) {
      const int t = relmap[ch.rowptr + q];
#pragma unroll
      for (int r = 0; r < NR; ++r)
        if (r < nr) T[r * 128 + t] = T[r * 128 + t] + vbuf[r * rh.ldv + ch.voff + ch.ns + q];
    }
    wave_lds_sync();
  }
  // lanes >= ns carry update rows: the chain neither changes nor broadcasts them
  double val[NR], vhi[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    val[r] = T[r * 128 + lane];
    vhi[r] = T[r * 128 + 64 + lane];
  }
  wave_lds_sync();   // every lane read the vectors before the tile is staged over them
  for (int c0 = 0; c0 < ns; c0 += 32) {   // U11^T y = v1, ascending
    const int cw = min(32, ns - c0);
    stage_tile_t(T, Lp, M, ns, c0, cw, lane);
    wave_lds_sync();
    double l[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) l[j] = (lane < ns && j < cw) ? T[lane * 33 + j] : 0.0;
    const double dinv = (lane >= c0 && lane < c0 + cw) ? recip(T[lane * 33 + lane - c0]) : 1.0;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      if (j < cw) {
        const int gj = c0 + j;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          val[r] = lane == gj ? val[r] * dinv : val[r];
          const double t = fma(-l[j], readlane_f64(val[r], gj), val[r]);
          val[r] = (lane > gj && lane < ns) ? t : val[r];
        }
      }
    }
    wave_lds_sync();   // every lane read the tile before the next one is staged
  }
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    if (lane < ns && r < nr) x[r * rh.ldx + s.first + lane] = val[r];
    T[r * 128 + lane] = val[r];
    T[r * 128 + 64 + lane] = vhi[r];
  }
  wave_lds_sync();
  if (nu == 0) return;
  // update rows: v[ns + k] -= <U12 column k, y1>
  const double* U12 = store + s.Uoff;
  const int G = pow2_at_least(ns), per = 64 / G;
  const int g = lane / G, e = lane & (G - 1);
  double ye[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) ye[r] = e < ns ? T[r * 128 + e] : 0.0;
  for (int k0 = 0; k0 < nu; k0 += U * per) {   // U runs per group and round, loaded once for all columns
    double c[U], part[NR][U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = k0 + u * per + g;
      c[u] = (k < nu && e < ns) ? U12[(int64_t)k * ns + e] : 0.0;
    }
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int k = k0 + u * per + g;
        part[r][u] = (k < nu && e < ns) ? c[u] * ye[r] : 0.0;
      }
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
      for (int u = 0; u < U; ++u)
        for (int o = G >> 1; o > 0; o >>= 1) part[r][u] += __shfl_xor(part[r][u], o, 64);
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int k = k0 + u * per + g;
        if (e == 0 && k < nu && r < nr) vbuf[r * rh.ldv + s.voff + ns + k] = T[r * 128 + ns + k] - part[r][u];
      }
  }
}

template <int NR>
__global__ __launch_bounds__(64 * kTinyWaves) void k_lt_tiny(const int32_t* __restrict__ list, int cnt,
                                                             const SNode* __restrict__ sn,
                                                             const int32_t* __restrict__ rows,
                                                             const int32_t* __restrict__ rowperm,
                                                             const double* __restrict__ store,
                                                             double* __restrict__ x, Rhs rh) {
  const int nr = rhs_count<NR>(rh);
  static_assert(NR * 128 <= kTinyT, "the batch's front vectors share the tile");
  constexpr int U = TinyRuns<NR>::U;
  __shared__ double sT[kTinyWaves][kTinyT];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t f = (int64_t)blockIdx.x * kTinyWaves + wv;
  if (f >= cnt) return;   // the whole wave
  const SNode s = sn[list[f]];
  const int ns = s.ns, nu = s.nu, M = ns + nu;
  const double* Lp = store + s.Loff;
  double* T = sT[wv];   // column r: z[R] at T + r * 128, the products at T + r * 128 + nu (nu + ns <= 128)
  double val[NR];       // y1
#pragma unroll
  for (int r = 0; r < NR; ++r) val[r] = (lane < ns && r < nr) ? x[r * rh.ldx + s.first + lane] : 0.0;
  if (nu > 0) {   // v1 = y1 - L21^T z[R]
    for (int t = lane; t < nu; t += 64) {
      const int32_t rt = rows[s.rowptr + t];
#pragma unroll
      for (int r = 0; r < NR; ++r) T[r * 128 + t] = r < nr ? x[r * rh.ldx + rt] : 0.0;
    }
    wave_lds_sync();
    const int G = pow2_at_least(nu), per = 64 / G;
    const int g = lane / G, e = lane & (G - 1);
    for (int j0 = 0; j0 < ns; j0 += U * per) {   // U runs per group and round, loaded once for all columns
      double part[NR][U];
#pragma unroll
      for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int u = 0; u < U; ++u) part[r][u] = 0.0;
      for (int t = e; t < nu; t += G) {
        double c[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int j = j0 + u * per + g;
          c[u] = j < ns ? Lp[(int64_t)j * M + ns + t] : 0.0;
        }
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          const double zt = T[r * 128 + t];
#pragma unroll
          for (int u = 0; u < U; ++u) part[r][u] = fma(c[u], zt, part[r][u]);
        }
      }
#pragma unroll
      for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int u = 0; u < U; ++u)
          for (int o = G >> 1; o > 0; o >>= 1) part[r][u] += __shfl_xor(part[r][u], o, 64);
#pragma unroll
      for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int j = j0 + u * per + g;
          if (e == 0 && j < ns) T[r * 128 + nu + j] = part[r][u];
        }
    }
    wave_lds_sync();
#pragma unroll
    for (int r = 0; r < NR; ++r)
      if (lane < ns) val[r] = val[r] - T[r * 128 + nu + lane];
    wave_lds_sync();   // every lane read the products before the tile is staged over them
  }
  for (int c0 = ((ns - 1) / 32) * 32; c0 >= 0; c0 -= 32) {   // L11^T (unit upper), descending
    const int cw = min(32, ns - c0);
    stage_tile_t(T, Lp, M, ns, c0, cw, lane);
    wave_lds_sync();
    double l[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) l[j] = (lane < ns && j < cw) ? T[lane * 33 + j] : 0.0;
#pragma unroll
    for (int j = 31; j >= 0; --j) {
      if (j < cw) {
        const int gj = c0 + j;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          const double t = fma(-l[j], readlane_f64(val[r], gj), val[r]);
          val[r] = lane < gj ? t : val[r];
        }
      }
    }
    wave_lds_sync();
  }
  // the wave read its own rows of x above; descendants read z at pre-pivot positions
  if (lane < ns) {
    const int64_t dst = s.first + rowperm[s.first + lane];
#pragma unroll
    for (int r = 0; r < NR; ++r)
      if (r < nr) x[r * rh.ldx + dst] = val[r];
  }
}

// ---- micro fronts (M <= 8 rows: the leaves): eight lanes per front, 32 fronts per workgroup, as
// k_fwd_micro / k_bwd_micro.  Lane i owns row i of the transposed triangle, i.e. panel column i; a
// whole front is at most 64 contiguous doubles, so these reads stay inside one or two cache lines.
template <int NR>
__global__ __launch_bounds__(256) void k_ut_micro(const int32_t* __restrict__ list, int cnt,
                                                  const SNode* __restrict__ sn,
                                                  const int32_t* __restrict__ chlist,
                                                  const int32_t* __restrict__ relmap,
                                                  const double* __restrict__ store, double* __restrict__ x,
                                                  double* __restrict__ vbuf, Rhs rh) {
  const int nr = rhs_count<NR>(rh);
  __shared__ double sv[NR][32][8];
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 3, i = threadIdx.x & 7;
  const int64_t f = (int64_t)blockIdx.x * 32 + g;
  const bool act = f < cnt;
  SNode s{};
  if (act) s = sn[list[f]];
  const int ns = act ? s.ns : 0, nu = act ? s.nu : 0, M = ns + nu;
  const double* Lp = store + s.Loff;
  const double* U12 = store + s.Uoff;
  double l[8];   // row i of U11^T (i < ns) or column i - ns of U12 (update rows)
#pragma unroll
  for (int j = 0; j < 8; ++j)
    l[j] = (i < ns && j <= i) ? Lp[(int64_t)i * M + j] : (i >= ns && i < M && j < ns) ? U12[(int64_t)(i - ns) * ns + j] : 0.0;
  const int gb = lane & ~7;
#pragma unroll
  for (int r = 0; r < NR; ++r) sv[r][g][i] = (i < ns && r < nr) ? x[r * rh.ldx + s.first + i] : 0.0;
  wave_lds_sync();
  for (int c = act ? s.chbeg : 0; c < (act ? s.chend : 0); ++c) {   // parent += child, children in order
    const SNode ch = sn[chlist[c]];
    for (int q = i; q < ch.nu; q += 8) {
      const int t = relmap[ch.rowptr + q];
#pragma unroll
      for (int r = 0; r < NR; ++r)
        if (r < nr) sv[r][g][t] = sv[r][g][t] + vbuf[r * rh.ldv + ch.voff + ch.ns + q];
    }
    wave_lds_sync();
  }
  wave_lds_sync();
  double val[NR], acc[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    val[r] = i < M ? sv[r][g][i] : 0.0;
    acc[r] = 0.0;
  }
  double dinv = 1.0;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (i == j && i < ns) dinv = recip(l[j]);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      if (i == j && j < ns) val[r] = val[r] * dinv;
      const double yj = __shfl(val[r], gb + j, 64);
      if (j < ns) {
        if (i > j && i < ns) val[r] = fma(-l[j], yj, val[r]);
        else if (i >= ns) acc[r] = fma(l[j], yj, acc[r]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    if (r < nr) {
      if (i < ns) x[r * rh.ldx + s.first + i] = val[r];
      else if (i < M) vbuf[r * rh.ldv + s.voff + i] = val[r] - acc[r];
    }
  }
}

template <int NR>
__global__ __launch_bounds__(256) void k_lt_micro(const int32_t* __restrict__ list, int cnt,
                                                  const SNode* __restrict__ sn, const int32_t* __restrict__ rows,
                                                  const int32_t* __restrict__ rowperm,
                                                  const double* __restrict__ store, double* __restrict__ x,
                                                  Rhs rh) {
  const int nr = rhs_count<NR>(rh);
  const int lane = threadIdx.x & 63, i = threadIdx.x & 7;
  const int64_t f = (int64_t)blockIdx.x * 32 + (threadIdx.x >> 3);
  const bool act = f < cnt;
  SNode s{};
  if (act) s = sn[list[f]];
  const int ns = act ? s.ns : 0, nu = act ? s.nu : 0, M = ns + nu;
  const double* Lp = store + s.Loff;
  double l[8];   // panel column i below its diagonal: row i of L11^T, then of L21^T
#pragma unroll
  for (int j = 0; j < 8; ++j) l[j] = (i < ns && j > i && j < M) ? Lp[(int64_t)i * M + j] : 0.0;
  const int gb = lane & ~7;
  double val[NR], acc[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    val[r] = (i < ns && r < nr) ? x[r * rh.ldx + s.first + i] : 0.0;   // y1
    acc[r] = 0.0;
  }
#pragma unroll
  for (int j = 1; j < 8; ++j)                   // v1 = y1 - L21^T z[R], update rows in order
    if (i < ns && j >= ns && j < M) {
      const int32_t rt = rows[s.rowptr + j - ns];
#pragma unroll
      for (int r = 0; r < NR; ++r)
        if (r < nr) acc[r] = fma(l[j], x[r * rh.ldx + rt], acc[r]);
    }
#pragma unroll
  for (int r = 0; r < NR; ++r) val[r] = val[r] - (nu > 0 ? acc[r] : 0.0);
#pragma unroll
  for (int j = 7; j > 0; --j) {                 // L11^T, unit upper
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const double tj = __shfl(val[r], gb + j, 64);
      if (j < ns && i < j) val[r] = fma(-l[j], tj, val[r]);
    }
  }
  // every lane of the front read its y1 before the exchanges above; descendants read z at pre-pivot positions
  if (i < ns) {
    const int64_t dst = s.first + rowperm[s.first + i];
#pragma unroll
    for (int r = 0; r < NR; ++r)
      if (r < nr) x[r * rh.ldx + dst] = val[r];
  }
}

// ---- large fronts: one launch per step, workgroups by chunk -----------------------------------
// gather, one thread per front row in identity row order (k_fwd_pull's lists)
template <int NR>
__global__ __launch_bounds__(256) void k_pull_t(const FrontTile* __restrict__ ft, int nft,
                                                const SNode* __restrict__ sn, const int32_t* __restrict__ gptr,
                                                const int32_t* __restrict__ gent, const double* __restrict__ x,
                                                double* __restrict__ vbuf, Rhs rh) {
  const int nr = rhs_count<NR>(rh);
  const int64_t b = blockIdx.x;
  const int fi = find_front_tile(ft, nft, b);
  const SNode s = sn[ft[fi].s];
  const int64_t i = (b - ft[fi].wg0) * 256 + threadIdx.x;
  const int64_t M = (int64_t)s.ns + s.nu;
  if (i >= M) return;
  const int32_t* P = gptr + ft[fi].pad;
  const int32_t p0 = P[i], p1 = P[i + 1];
  double val[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) val[r] = (i < s.ns && r < nr) ? x[r * rh.ldx + s.first + i] : 0.0;
  for (int32_t p = p0; p < p1; ++p) {
    const int32_t ge = gent[p];
#pragma unroll
    for (int r = 0; r < NR; ++r)
      if (r < nr) val[r] = val[r] + vbuf[r * rh.ldv + ge];
  }
#pragma unroll
  for (int r = 0; r < NR; ++r)
    if (r < nr) vbuf[r * rh.ldv + s.voff + i] = val[r];
}

// One 64-column block step.  Every workgroup re-solves the block (transposed) from v, which no
// workgroup writes inside the block's range in this launch, and applies it to its chunk of 256
// targets: !UPPER (U^T): rows [jb + bw, M), panel column t for t < ns, U12 column t - ns after it;
// UPPER (L^T): rows [0, jb), panel column t.  Chunk 0 publishes the block into x (UPPER: through the
// front's row permutation).  Five waves.  The last one alone stages the block (64 coalesced column
// loads, one LDS tile, a wave-level hand-off) and runs the NR chains interleaved on its row of the
// transposed block (tri64_rows; U^T: columns pre-scaled by 1/u_jj, the results scaled once at the
// end).  The first four each give a 16-lane group sixteen consecutive targets and load their
// 64-entry runs and old values while the block is being solved; they then take the columns one after
// the other through the same sixteen accumulators, the runs staying in registers: lane e of a group
// ends up owning target e (red16x16 per column) and stores it.  Full blocks take loads without
// per-element guards (a chunk's last group re-reads the last target instead of masking).
template <bool UPPER, int NR>
__global__ __launch_bounds__(320) void k_tri_t(const FrontTile* __restrict__ ft, int nft, int step,
                                               const SNode* __restrict__ sn, const int32_t* __restrict__ rowperm,
                                               const double* __restrict__ store, double* __restrict__ x,
                                               double* __restrict__ vbuf, Rhs rh) {
  const int nr = rhs_count<NR>(rh);
  __shared__ double sD[64 * 65];
  __shared__ double ys[NR][64];
  const int64_t b = blockIdx.x;
  const int fi = find_front_tile(ft, nft, b);
  const SNode s = sn[ft[fi].s];
  const int64_t chunk = b - ft[fi].wg0;
  const int64_t M = (int64_t)s.ns + s.nu, ns = s.ns;
  const int64_t nblk = (ns + 63) / 64;
  const int64_t jb = UPPER ? (nblk - 1 - step) * 64 : (int64_t)step * 64;
  const int bw = (int)min<int64_t>(64, ns - jb);
  const double* Lp = store + s.Loff;
  const double* U12 = store + s.Uoff;
  double* v = vbuf + s.voff;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (wv == 4) {   // the chain wave (its own path: its 64 registers never live next to the targets' runs)
    const bool in = lane < bw;
    double xi[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) xi[r] = (in && r < nr) ? v[r * rh.ldv + jb + lane] : 0.0;
    const double* D = Lp + jb * M + jb;
    double row[64];
    if (bw == 64) {
#pragma unroll
      for (int j = 0; j < 64; ++j) row[j] = D[(int64_t)j * M + lane];
    } else {
#pragma unroll
      for (int j = 0; j < 64; ++j) row[j] = (in && j < bw) ? D[(int64_t)j * M + lane] : 0.0;
    }
#pragma unroll
    for (int j = 0; j < 64; ++j) sD[j * 65 + lane] = row[j];
    wave_lds_sync();
    const double dg = sD[lane * 65 + lane];
#pragma unroll
    for (int j = 0; j < 64; ++j) {
      const double t = sD[lane * 65 + j];   // row `lane` of the transposed block
      row[j] = (in && j < bw && (UPPER ? j > lane : j < lane)) ? t : 0.0;
    }
    if (UPPER) {
      tri64_rows<true, NR>(xi, row, 1.0, bw);
    } else {
      const double dinv = in ? recip(dg) : 1.0;
      tri64_scale_upper(row, dinv, bw);   // column j by 1/u_jj: the chains run on the unscaled u_j = u_jj y_j
      tri64_rows<false, NR>(xi, row, 1.0, bw);
#pragma unroll
      for (int r = 0; r < NR; ++r) xi[r] = xi[r] * dinv;
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      ys[r][lane] = in ? xi[r] : 0.0;
      if (chunk == 0 && in && r < nr) {
        if (UPPER) x[r * rh.ldx + s.first + rowperm[s.first + jb + lane]] = xi[r];
        else x[r * rh.ldx + s.first + jb + lane] = xi[r];
      }
    }
    __syncthreads();
    return;
  }
  const int g = tid >> 4, e = tid & 15;
  const int64_t lo = UPPER ? chunk * 256 : jb + bw + chunk * 256;
  const int64_t hi = UPPER ? min<int64_t>(jb, lo + 256) : min<int64_t>(M, lo + 256);
  const int64_t tm = lo + tid;   // the target this lane stores
  double d[16][4];
  double vold[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) vold[r] = 0.0;
  if (lo < hi) {
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int64_t t = min<int64_t>(lo + g * 16 + u, hi - 1);
      const double* ptr = (UPPER || t < ns) ? Lp + t * M + jb : U12 + (t - ns) * ns + jb;
      if (bw == 64) {
#pragma unroll
        for (int k = 0; k < 4; ++k) d[u][k] = ptr[e + 16 * k];
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) d[u][k] = e + 16 * k < bw ? ptr[e + 16 * k] : 0.0;
      }
    }
#pragma unroll
    for (int r = 0; r < NR; ++r)
      if (r < nr) vold[r] = v[r * rh.ldv + min<int64_t>(tm, hi - 1)];
  }
  __syncthreads();   // the chain wave has solved the block
  if (lo >= hi) return;
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    if (r < nr) {   // the whole workgroup
      double xx[4], a[16];
#pragma unroll
      for (int k = 0; k < 4; ++k) xx[k] = ys[r][e + 16 * k];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        a[u] = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) a[u] = fma(d[u][k], xx[k], a[u]);
      }
      const double res = red16x16(a, e);
      if (tm < hi) v[r * rh.ldv + tm] = vold[r] - res;
    }
  }
}

// v1[j] = y1[j] - <panel column j [ns, M), z[R]>: 64 columns per workgroup (four per 16-lane group),
// z[R] staged through LDS a chunk at a time: 512 entries for one column (4 KB), 2048 / NR per column
// for a batch (16 KB).  The chunk length only places barriers; a lane adds its entries in ascending
// order whatever it is.
template <int NR>
__global__ __launch_bounds__(256) void k_bwdu_t(const FrontTile* __restrict__ ft, int nft,
                                                const SNode* __restrict__ sn, const int32_t* __restrict__ rows,
                                                const double* __restrict__ store, const double* __restrict__ x,
                                                double* __restrict__ vbuf, Rhs rh) {
  const int nr = rhs_count<NR>(rh);
  constexpr int ZC = NR == 1 ? 512 : 2048 / NR;
  static_assert(ZC % 64 == 0, "a chunk is whole rounds of dots16");
  __shared__ double zs[NR][ZC];
  const int64_t b = blockIdx.x;
  const int fi = find_front_tile(ft, nft, b);
  const SNode s = sn[ft[fi].s];
  const int64_t chunk = b - ft[fi].wg0;
  const int64_t M = (int64_t)s.ns + s.nu, ns = s.ns, nu = s.nu;
  const int32_t* R = rows + s.rowptr;
  const double* Lp = store + s.Loff;
  const int tid = threadIdx.x, g = tid >> 4, e = tid & 15;
  constexpr int U = LongRuns<NR>::U;   // the workgroup's 64 columns, U per group at a time
  for (int u0 = 0; u0 < 4; u0 += U) {
    const double* ptr[U];
    bool ok[U];
    double a[NR][U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t j = chunk * 64 + (u0 + u) * 16 + g;
      ok[u] = j < ns;
      ptr[u] = Lp + (ok[u] ? j : 0) * M + ns;
#pragma unroll
      for (int r = 0; r < NR; ++r) a[r][u] = 0.0;
    }
    for (int64_t c0 = 0; c0 < nu; c0 += ZC) {
      const int cl = (int)min<int64_t>(ZC, nu - c0);
      __syncthreads();
      for (int t = tid; t < cl; t += 256) {
        const int32_t rt = R[c0 + t];
#pragma unroll
        for (int r = 0; r < NR; ++r) zs[r][t] = r < nr ? x[r * rh.ldx + rt] : 0.0;
      }
      __syncthreads();
      const double* pc[U];
#pragma unroll
      for (int u = 0; u < U; ++u) pc[u] = ptr[u] + c0;
      dots16<NR, U>(pc, ok, &zs[0][0], ZC, nr, cl, e, a);
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      if (r < nr) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const double res = red16(a[r][u]);
          const int64_t j = chunk * 64 + (u0 + u) * 16 + g;
          if (e == 0 && ok[u]) vbuf[r * rh.ldv + s.voff + j] = x[r * rh.ldx + s.first + j] - res;
        }
      }
    }
  }
}

// ---- permutations and the column-wise residual ------------------------------------------------
// conj (a ComplexF64 handle's plain transpose: A^T \ b = conj(A^H \ conj(b))): the imaginary slots,
// odd indices of the caller's interleaved vectors, change sign on the way in and out.
// wrk_r[k] = b_r[q[k]], column r of b at b + r*ldb
template <int NR>
__global__ void k_perm_in_t(int64_t n, const int64_t* __restrict__ q, const double* b, int64_t ldb,
                            double* __restrict__ wrk, int conj, Rhs rh) {
  const int nr = rhs_count<NR>(rh);
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) {
    const int64_t c = q[k];
    const bool neg = conj && (c & 1);
#pragma unroll
    for (int r = 0; r < NR; ++r)
      if (r < nr) {
        const double val = b[r * ldb + c];
        wrk[r * rh.ldx + k] = neg ? -val : val;
      }
  }
}
// x_r[p0[k]] = Rs[p0[k]] * wrk_r[k], column r of x at x + r*ldxo
template <int NR>
__global__ void k_perm_out_t(int64_t n, const int64_t* __restrict__ p0, const double* __restrict__ Rs,
                             const double* __restrict__ wrk, double* x, int64_t ldxo, int conj, Rhs rh) {
  const int nr = rhs_count<NR>(rh);
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) {
    const int64_t row = p0[k];
    const double sc = Rs[row];
    const bool neg = conj && (row & 1);
#pragma unroll
    for (int r = 0; r < NR; ++r)
      if (r < nr) {
        const double val = sc * wrk[r * rh.ldx + k];
        x[r * ldxo + row] = neg ? -val : val;
      }
  }
}
// r = b - A^T x by columns of A's CSC (entries of a column in row order, deterministic), max |r_j|
// into nrm[0] and the componentwise backward error max_j |r_j| / (|A^T| |x| + |b|)_j into nrm[1]
// (k_residual's rule).  conj: the residual of conj(K^T conj(.)), K the real-equivalent matrix.
__global__ __launch_bounds__(256) void k_residual_t(int64_t n, const int64_t* __restrict__ colptr,
                                                    const int32_t* __restrict__ arow, const double* __restrict__ a,
                                                    const double* __restrict__ x, const double* __restrict__ b,
                                                    double* __restrict__ r, double* __restrict__ nrm, int conj) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double rj = 0.0, wj = 0.0;
  if (j < n) {
    double acc = 0.0, den = 0.0;
    for (int64_t e = colptr[j]; e < colptr[j + 1]; ++e) {
      const int32_t i = arow[e];
      const double xv = x[i];
      const double xi = (conj && (i & 1)) ? -xv : xv;
      acc = fma(a[e], xi, acc);
      den = fma(fabs(a[e]), fabs(xi), den);
    }
    if (conj && (j & 1)) acc = -acc;
    rj = b[j] - acc;
    r[j] = rj;
    den += fabs(b[j]);
    wj = rj == 0.0 ? 0.0 : den > 0.0 ? fabs(rj) / den : HUGE_VAL;
  }
  const double m = wave_max(fabs(rj));
  const double w = wave_max(wj);
  if ((threadIdx.x & 63) == 0 && m > 0.0) atomic_max_pos(nrm, m);
  if ((threadIdx.x & 63) == 0 && w > 0.0) atomic_max_pos(nrm + 1, w);
}

// ---- host-side launch wrappers (solve.cpp) ---------------------------------------------------
// Every wrapper picks its instance with SMLU_BY_WIDTH (kernels_common.hpp).
hipError_t launch_ut_tiny(hipStream_t st, int cnt, const int32_t* list, const SNode* sn, const int32_t* chlist,
                          const int32_t* relmap, const double* store, double* x, double* vbuf, Rhs rh, int micro) {
  if (cnt <= 0) return hipSuccess;
  if (micro)   // every front of the list has M <= 8
    SMLU_BY_WIDTH(k_ut_micro, nblk(cnt, 32), 256, list, cnt, sn, chlist, relmap, store, x, vbuf);
  SMLU_BY_WIDTH(k_ut_tiny, nblk(cnt, kTinyWaves), 64 * kTinyWaves, list, cnt, sn, chlist, relmap, store, x, vbuf);
}
hipError_t launch_lt_tiny(hipStream_t st, int cnt, const int32_t* list, const SNode* sn, const int32_t* rows,
                          const int32_t* rowperm, const double* store, double* x, Rhs rh, int micro) {
  if (cnt <= 0) return hipSuccess;
  if (micro) SMLU_BY_WIDTH(k_lt_micro, nblk(cnt, 32), 256, list, cnt, sn, rows, rowperm, store, x);
  SMLU_BY_WIDTH(k_lt_tiny, nblk(cnt, kTinyWaves), 64 * kTinyWaves, list, cnt, sn, rows, rowperm, store, x);
}
hipError_t launch_ut_front(hipStream_t st, int cnt, const int32_t* list, const SNode* sn, const int32_t* chlist,
                           const int32_t* relmap, const double* store, double* x, double* vbuf, Rhs rh) {
  if (cnt <= 0) return hipSuccess;
  SMLU_BY_WIDTH(k_ut_front, cnt, 256, list, sn, chlist, relmap, store, x, vbuf);
}
hipError_t launch_lt_front(hipStream_t st, int cnt, const int32_t* list, const SNode* sn, const int32_t* rows,
                           const int32_t* rowperm, const double* store, double* x, double* vbuf, Rhs rh) {
  if (cnt <= 0) return hipSuccess;
  SMLU_BY_WIDTH(k_lt_front, cnt, 256, list, sn, rows, rowperm, store, x, vbuf);
}
hipError_t launch_pull_t(hipStream_t st, int64_t nwg, const FrontTile* ft, int nft, const SNode* sn,
                         const int32_t* gptr, const int32_t* gent, const double* x, double* vbuf, Rhs rh) {
  if (nwg <= 0) return hipSuccess;
  SMLU_BY_WIDTH(k_pull_t, (unsigned)nwg, 256, ft, nft, sn, gptr, gent, x, vbuf);
}
hipError_t launch_tri_t(hipStream_t st, bool upper, int64_t nwg, const FrontTile* ft, int nft, int step,
                        const SNode* sn, const int32_t* rowperm, const double* store, double* x, double* vbuf,
                        Rhs rh) {
  if (nwg <= 0) return hipSuccess;
  if (upper) SMLU_BY_WIDTH2(k_tri_t, true, (unsigned)nwg, 320, ft, nft, step, sn, rowperm, store, x, vbuf);
  SMLU_BY_WIDTH2(k_tri_t, false, (unsigned)nwg, 320, ft, nft, step, sn, rowperm, store, x, vbuf);
}
hipError_t launch_bwdu_t(hipStream_t st, int64_t nwg, const FrontTile* ft, int nft, const SNode* sn,
                         const int32_t* rows, const double* store, const double* x, double* vbuf, Rhs rh) {
  if (nwg <= 0) return hipSuccess;
  SMLU_BY_WIDTH(k_bwdu_t, (unsigned)nwg, 256, ft, nft, sn, rows, store, x, vbuf);
}
// column j of b at b + j*ldb, of x at x + j*ldxo; of the work vectors at wrk + j*rh.ldx
hipError_t launch_perm_in_t(hipStream_t st, int64_t n, const int64_t* q, const double* b, int64_t ldb, double* wrk,
                            int conj, Rhs rh) {
  if (n <= 0) return hipSuccess;
  SMLU_BY_WIDTH(k_perm_in_t, nblk(n, 256), 256, n, q, b, ldb, wrk, conj);
}
hipError_t launch_perm_out_t(hipStream_t st, int64_t n, const int64_t* p0, const double* Rs, const double* wrk,
                             double* x, int64_t ldxo, int conj, Rhs rh) {
  if (n <= 0) return hipSuccess;
  SMLU_BY_WIDTH(k_perm_out_t, nblk(n, 256), 256, n, p0, Rs, wrk, x, ldxo, conj);
}
hipError_t launch_residual_t(hipStream_t st, int64_t n, const int64_t* colptr, const int32_t* arow, const double* a,
                             const double* x, const double* b, double* r, double* nrm, int conj) {
  if (n <= 0) return hipSuccess;
  k_residual_t<<<nblk(n, 256), 256, 0, st>>>(n, colptr, arow, a, x, b, r, nrm, conj);
  return hipGetLastError();
}

}  // namespace smlu

