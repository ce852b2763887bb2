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
#include "kernels_solve_t.hpp"

namespace smlu {

// v[t] -= <col(t)[0 : bw), ys> for the targets t in [lo, hi): 16 groups of 16 lanes (256 threads),
// four targets per group and round.  col(t) -> start of the target's contiguous run.
template <class COL>
__device__ __forceinline__ void apply_dots(int64_t lo, int64_t hi, int bw, const double* ys, double* __restrict__ v,
                                           int tid, COL&& col) {
  constexpr int U = 4;
  const int g = tid >> 4, e = tid & 15;
  for (int64_t t0 = lo; t0 < hi; t0 += 16 * U) {
    const double* ptr[U];
    bool ok[U];
    double a[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t t = t0 + u * 16 + g;
      ok[u] = t < hi;
      ptr[u] = col(ok[u] ? t : lo);
      a[u] = 0.0;
    }
    dots16<U>(ptr, ok, ys, bw, e, a);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const double r = red16(a[u]);
      const int64_t t = t0 + u * 16 + g;
      if (e == 0 && ok[u]) v[t] = v[t] - r;
    }
  }
}

// One wave solves the staged block transposed.  Row `lane` of the transposed block is the block's
// column `lane`: sD[lane * 65 + j] (stride 65 across lanes).
//   !UPPER: U11^T y = x, non-unit lower (entries j <= lane), ascending;
//    UPPER: L11^T t = x, unit upper (entries j > lane), descending.
template <bool UPPER>
__device__ __forceinline__ double tri_lds_t(double xi, const double* __restrict__ sD, int bw, int lane) {
  const bool in = lane < bw;
  if (!UPPER) {
    const double dinv = in ? recip(sD[lane * 65 + lane]) : 1.0;
    for (int j = 0; j < bw; ++j) {
      xi = lane == j ? xi * dinv : xi;
      const double t = fma(-sD[lane * 65 + j], readlane_f64(xi, j), xi);
      xi = (lane > j && in) ? t : xi;
    }
  } else {
    for (int j = bw - 1; j > 0; --j) {
      const double t = fma(-sD[lane * 65 + j], readlane_f64(xi, j), xi);
      xi = lane < j ? t : xi;
    }
  }
  return xi;
}

// front vector = own rows of x + the children's update vectors (no row permutation: the columns of
// U are not pivoted); one workgroup
__device__ __forceinline__ void gather_front_t(const SNode& s, const SNode* __restrict__ sn,
                                               const int32_t* __restrict__ chlist, const int32_t* __restrict__ relmap,
                                               const double* __restrict__ x, double* __restrict__ vbuf, int tid) {
  const int64_t M = (int64_t)s.ns + s.nu, ns = s.ns;
  double* v = vbuf + s.voff;
  for (int64_t i = tid; i < M; i += 256) v[i] = i < ns ? x[s.first + i] : 0.0;
  __syncthreads();
  for (int c = s.chbeg; c < s.chend; ++c) {
    const SNode ch = sn[chlist[c]];
    const int32_t* rm = relmap + ch.rowptr;
    const double* cv = vbuf + ch.voff + ch.ns;
    for (int64_t i = tid; i < ch.nu; i += 256) v[rm[i]] = v[rm[i]] + cv[i];   // a child's rows are distinct
    __syncthreads();
  }
}

// ---- small fronts: one workgroup per front ---------------------------------------------------
// U^T step: y1 = U11^-T v1 in 64-column blocks; every block is applied to the rows after it, the
// front's own (panel columns) and the update rows (U12 columns): v[t] -= <col_t[jb : jb+bw), y_blk>.
__global__ __launch_bounds__(256) void k_ut_front(const int32_t* __restrict__ list, const SNode* __restrict__ sn,
                                                  const int32_t* __restrict__ chlist,
                                                  const int32_t* __restrict__ relmap,
                                                  const double* __restrict__ store, double* __restrict__ x,
                                                  double* __restrict__ vbuf) {
  __shared__ double sD[64 * 65];
  __shared__ double ys[64];
  const SNode s = sn[list[blockIdx.x]];
  const int64_t M = (int64_t)s.ns + s.nu, ns = s.ns;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  gather_front_t(s, sn, chlist, relmap, x, vbuf, tid);
  const double* Lp = store + s.Loff;
  const double* U12 = store + s.Uoff;
  double* v = vbuf + s.voff;
  for (int64_t jb = 0; jb < ns; jb += 64) {
    const int bw = (int)min<int64_t>(64, ns - jb);
    stage_block_t(sD, Lp + jb * M + jb, M, bw, tid);
    __syncthreads();
    if (wv == 0) {
      double xi = lane < bw ? v[jb + lane] : 0.0;
      xi = tri_lds_t<false>(xi, sD, bw, lane);
      ys[lane] = lane < bw ? xi : 0.0;
      if (lane < bw) {
        v[jb + lane] = xi;
        x[s.first + jb + lane] = xi;
      }
    }
    __syncthreads();
    apply_dots(jb + bw, M, bw, ys, v, tid,
               [&](int64_t t) { return t < ns ? Lp + t * M + jb : U12 + (t - ns) * ns + jb; });
    __syncthreads();
  }
}

// L^T step: v1 = y1 - L21^T z[R] (z[R] gathered into the front vector's update rows, then one dot
// product per panel column tail), L11^T in 64-column blocks from the last, result scattered through
// the front's row permutation.
__global__ __launch_bounds__(256) void k_lt_front(const int32_t* __restrict__ list, const SNode* __restrict__ sn,
                                                  const int32_t* __restrict__ rows,
                                                  const int32_t* __restrict__ rowperm,
                                                  const double* __restrict__ store, double* __restrict__ x,
                                                  double* __restrict__ vbuf) {
  __shared__ double sD[64 * 65];
  __shared__ double ys[64];
  const SNode s = sn[list[blockIdx.x]];
  const int64_t M = (int64_t)s.ns + s.nu, ns = s.ns, nu = s.nu;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int32_t* R = rows + s.rowptr;
  const double* Lp = store + s.Loff;
  double* v = vbuf + s.voff;
  for (int64_t t = tid; t < nu; t += 256) v[ns + t] = x[R[t]];
  for (int64_t j = tid; j < ns; j += 256) v[j] = x[s.first + j];
  __syncthreads();
  if (nu > 0) {
    const int g = tid >> 4, e = tid & 15;
    for (int64_t j0 = 0; j0 < ns; j0 += 64) {
      const double* ptr[4];
      bool ok[4];
      double a[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t j = j0 + u * 16 + g;
        ok[u] = j < ns;
        ptr[u] = Lp + (ok[u] ? j : 0) * M + ns;
        a[u] = 0.0;
      }
      dots16<4>(ptr, ok, v + ns, nu, e, a);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const double r = red16(a[u]);
        const int64_t j = j0 + u * 16 + g;
        if (e == 0 && ok[u]) v[j] = v[j] - r;
      }
    }
    __syncthreads();
  }
  for (int64_t jb = ((ns - 1) / 64) * 64; jb >= 0; jb -= 64) {
    const int bw = (int)min<int64_t>(64, ns - jb);
    stage_block_t(sD, Lp + jb * M + jb, M, bw, tid);
    __syncthreads();
    if (wv == 0) {
      double xi = lane < bw ? v[jb + lane] : 0.0;
      xi = tri_lds_t<true>(xi, sD, bw, lane);
      ys[lane] = lane < bw ? xi : 0.0;
      if (lane < bw) v[jb + lane] = xi;
    }
    __syncthreads();
    apply_dots(0, jb, bw, ys, v, tid, [&](int64_t t) { return Lp + t * M + jb; });
    __syncthreads();
  }
  // descendants read z at pre-pivot positions
  for (int64_t i = tid; i < ns; i += 256) x[s.first + rowperm[s.first + i]] = v[i];
}

// ---- tiny fronts (M <= 128 rows, ns <= 64 pivots): one wave per front, two
// fronts per workgroup, no workgroup barrier.  The triangle is staged 32 columns at a time into a
// per-wave LDS tile T[col * 33 + row] (coalesced along the panel columns) and read back one panel
// column per lane; the U12 / L21 products give G = 2^ceil(log2(len)) lanes to each contiguous run.
__global__ __launch_bounds__(64 * kTinyWaves) void k_ut_tiny(const int32_t* __restrict__ list, int cnt,
                                                             const SNode* __restrict__ sn,
                                                             const int32_t* __restrict__ chlist,
                                                             const int32_t* __restrict__ relmap,
                                                             const double* __restrict__ store,
                                                             double* __restrict__ x, double* __restrict__ vbuf) {
  __shared__ double sT[kTinyWaves][64 * 33];
  __shared__ double sv[kTinyWaves][128];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t f = (int64_t)blockIdx.x * kTinyWaves + wv;
  if (f >= cnt) return;   // the whole wave
  const SNode s = sn[list[f]];
  const int ns = s.ns, nu = s.nu, M = ns + nu;
  const double* Lp = store + s.Loff;
  double* T = sT[wv];
  double* v = sv[wv];
  v[lane] = lane < ns ? x[s.first + lane] : 0.0;
  v[64 + lane] = 0.0;
  wave_lds_sync();
  for (int c = s.chbeg; c < s.chend; ++c) {   // parent += child, children in order
    const SNode ch = sn[chlist[c]];
    for (int q = lane; q < ch.nu; q += 64) {
      const int t = relmap[ch.rowptr + q];
      v[t] = v[t] + vbuf[ch.voff + ch.ns + q];
    }
    wave_lds_sync();
  }
  double val = lane < ns ? v[lane] : 0.0;
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
        val = lane == gj ? val * dinv : val;
        const double t = fma(-l[j], readlane_f64(val, gj), val);
        val = (lane > gj && lane < ns) ? t : val;
      }
    }
    wave_lds_sync();   // every lane read the tile before the next one is staged
  }
  if (lane < ns) {
    x[s.first + lane] = val;
    v[lane] = val;
  }
  wave_lds_sync();
  if (nu == 0) return;
  // update rows: v[ns + k] -= <U12 column k, y1>
  const double* U12 = store + s.Uoff;
  const int G = pow2_at_least(ns), per = 64 / G;
  const int g = lane / G, e = lane & (G - 1);
  const double ye = e < ns ? v[e] : 0.0;
  for (int k0 = 0; k0 < nu; k0 += 4 * per) {   // four runs per group and round, their loads issued together
    double part[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = k0 + u * per + g;
      part[u] = (k < nu && e < ns) ? U12[(int64_t)k * ns + e] * ye : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      for (int o = G >> 1; o > 0; o >>= 1) part[u] += __shfl_xor(part[u], o, 64);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = k0 + u * per + g;
      if (e == 0 && k < nu) vbuf[s.voff + ns + k] = v[ns + k] - part[u];
    }
  }
}

__global__ __launch_bounds__(64 * kTinyWaves) void k_lt_tiny(const int32_t* __restrict__ list, int cnt,
                                                             const SNode* __restrict__ sn,
                                                             const int32_t* __restrict__ rows,
                                                             const int32_t* __restrict__ rowperm,
                                                             const double* __restrict__ store,
                                                             double* __restrict__ x) {
  __shared__ double sT[kTinyWaves][64 * 33];
  __shared__ double sz[kTinyWaves][128];
  __shared__ double sd[kTinyWaves][64];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t f = (int64_t)blockIdx.x * kTinyWaves + wv;
  if (f >= cnt) return;   // the whole wave
  const SNode s = sn[list[f]];
  const int ns = s.ns, nu = s.nu, M = ns + nu;
  const double* Lp = store + s.Loff;
  double* T = sT[wv];
  double val = lane < ns ? x[s.first + lane] : 0.0;   // y1
  if (nu > 0) {   // v1 = y1 - L21^T z[R]
    for (int t = lane; t < nu; t += 64) sz[wv][t] = x[rows[s.rowptr + t]];
    wave_lds_sync();
    const int G = pow2_at_least(nu), per = 64 / G;
    const int g = lane / G, e = lane & (G - 1);
    for (int j0 = 0; j0 < ns; j0 += 4 * per) {   // four runs per group and round, their loads issued together
      double part[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) part[u] = 0.0;
      for (int t = e; t < nu; t += G) {
        double c[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int j = j0 + u * per + g;
          c[u] = j < ns ? Lp[(int64_t)j * M + ns + t] : 0.0;
        }
        const double zt = sz[wv][t];
#pragma unroll
        for (int u = 0; u < 4; ++u) part[u] = fma(c[u], zt, part[u]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        for (int o = G >> 1; o > 0; o >>= 1) part[u] += __shfl_xor(part[u], o, 64);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = j0 + u * per + g;
        if (e == 0 && j < ns) sd[wv][j] = part[u];
      }
    }
    wave_lds_sync();
    if (lane < ns) val = val - sd[wv][lane];
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
        const double t = fma(-l[j], readlane_f64(val, gj), val);
        val = lane < gj ? t : val;
      }
    }
    wave_lds_sync();
  }
  // the wave read its own rows of x above; descendants read z at pre-pivot positions
  if (lane < ns) x[s.first + rowperm[s.first + lane]] = val;
}

// Micro fronts (M <= 8 rows: the leaves): eight lanes per front, 32 fronts per workgroup, as
// k_fwd_micro / k_bwd_micro.  Lane i owns row i of the transposed triangle, i.e. panel column i; a
// whole front is at most 64 contiguous doubles, so these reads stay inside one or two cache lines.
__global__ __launch_bounds__(256) void k_ut_micro(const int32_t* __restrict__ list, int cnt,
                                                  const SNode* __restrict__ sn, const int32_t* __restrict__ chlist,
                                                  const int32_t* __restrict__ relmap,
                                                  const double* __restrict__ store, double* __restrict__ x,
                                                  double* __restrict__ vbuf) {
  __shared__ double sv[32][8];
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
  sv[g][i] = i < ns ? x[s.first + i] : 0.0;
  wave_lds_sync();
  for (int c = act ? s.chbeg : 0; c < (act ? s.chend : 0); ++c) {   // parent += child, children in order
    const SNode ch = sn[chlist[c]];
    for (int q = i; q < ch.nu; q += 8) {
      const int t = relmap[ch.rowptr + q];
      sv[g][t] = sv[g][t] + vbuf[ch.voff + ch.ns + q];
    }
    wave_lds_sync();
  }
  wave_lds_sync();
  double val = i < M ? sv[g][i] : 0.0;
  double dinv = 1.0;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (i == j && i < ns) dinv = recip(l[j]);
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (i == j && j < ns) val = val * dinv;
    const double yj = __shfl(val, gb + j, 64);
    if (j < ns) {
      if (i > j && i < ns) val = fma(-l[j], yj, val);
      else if (i >= ns) acc = fma(l[j], yj, acc);
    }
  }
  if (i < ns) x[s.first + i] = val;
  else if (i < M) vbuf[s.voff + i] = val - acc;
}

__global__ __launch_bounds__(256) void k_lt_micro(const int32_t* __restrict__ list, int cnt,
                                                  const SNode* __restrict__ sn, const int32_t* __restrict__ rows,
                                                  const int32_t* __restrict__ rowperm,
                                                  const double* __restrict__ store, double* __restrict__ x) {
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
  double val = i < ns ? x[s.first + i] : 0.0;   // y1
  double acc = 0.0;
#pragma unroll
  for (int j = 1; j < 8; ++j)                   // v1 = y1 - L21^T z[R], update rows in order
    if (i < ns && j >= ns && j < M) acc = fma(l[j], x[rows[s.rowptr + j - ns]], acc);
  val = val - (nu > 0 ? acc : 0.0);
#pragma unroll
  for (int j = 7; j > 0; --j) {                 // L11^T, unit upper
    const double tj = __shfl(val, gb + j, 64);
    if (j < ns && i < j) val = fma(-l[j], tj, val);
  }
  // every lane of the front read its y1 before the exchanges above; descendants read z at pre-pivot positions
  if (i < ns) x[s.first + rowperm[s.first + i]] = val;
}

// ---- large fronts: one launch per step, workgroups by chunk -----------------------------------
// gather, one thread per front row in identity row order (k_fwd_pull's lists)
__global__ __launch_bounds__(256) void k_pull_t(const FrontTile* __restrict__ ft, int nft, const SNode* __restrict__ sn,
                                                const int32_t* __restrict__ gptr, const int32_t* __restrict__ gent,
                                                const double* __restrict__ x, double* __restrict__ vbuf) {
  const int64_t b = blockIdx.x;
  const int fi = find_front_tile(ft, nft, b);
  const SNode s = sn[ft[fi].s];
  const int64_t i = (b - ft[fi].wg0) * 256 + threadIdx.x;
  const int64_t M = (int64_t)s.ns + s.nu;
  if (i >= M) return;
  const int32_t* P = gptr + ft[fi].pad;
  const int32_t p0 = P[i], p1 = P[i + 1];
  double val = i < s.ns ? x[s.first + i] : 0.0;
  for (int32_t p = p0; p < p1; ++p) val = val + vbuf[gent[p]];
  vbuf[s.voff + i] = val;
}

// One 64-column block step.  Every workgroup re-solves the block (transposed) from v, which no
// workgroup writes inside the block's range in this launch, and applies it to its chunk of 256
// targets: !UPPER (U^T): rows [jb + bw, M), panel column t for t < ns, U12 column t - ns after it;
// UPPER (L^T): rows [0, jb), panel column t.  Chunk 0 publishes the block into x (UPPER: through the
// front's row permutation).  Five waves.  The last one alone stages the block (64 coalesced column
// loads, one LDS tile, a wave-level hand-off) and runs the chain on its row of the transposed block
// (tri64_row; U^T: columns pre-scaled by 1/u_jj, the result scaled once at the end).  The first four
// each give a 16-lane group sixteen consecutive targets and load their 64-entry runs and old values
// while the block is being solved; lane e of a group ends up owning target e (red16x16) and stores
// it.  Full blocks take loads without per-element guards (a chunk's last group re-reads the last
// target instead of masking).
template <bool UPPER>
__global__ __launch_bounds__(320) void k_tri_t(const FrontTile* __restrict__ ft, int nft, int step,
                                               const SNode* __restrict__ sn, const int32_t* __restrict__ rowperm,
                                               const double* __restrict__ store, double* __restrict__ x,
                                               double* __restrict__ vbuf) {
  __shared__ double sD[64 * 65];
  __shared__ double ys[64];
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
    double xi = in ? v[jb + lane] : 0.0;
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
      xi = tri64_row<true>(xi, row, 1.0, bw);
    } else {
      const double dinv = in ? recip(dg) : 1.0;
      tri64_scale_upper(row, dinv, bw);   // column j by 1/u_jj: the chain runs on the unscaled u_j = u_jj y_j
      xi = tri64_row<false>(xi, row, 1.0, bw) * dinv;
    }
    ys[lane] = in ? xi : 0.0;
    if (chunk == 0 && in) {
      if (UPPER) x[s.first + rowperm[s.first + jb + lane]] = xi;
      else x[s.first + jb + lane] = xi;
    }
    __syncthreads();
    return;
  }
  const int g = tid >> 4, e = tid & 15;
  const int64_t lo = UPPER ? chunk * 256 : jb + bw + chunk * 256;
  const int64_t hi = UPPER ? min<int64_t>(jb, lo + 256) : min<int64_t>(M, lo + 256);
  const int64_t tm = lo + tid;   // the target this lane stores
  double d[16][4];
  double vold = 0.0;
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
    vold = v[min<int64_t>(tm, hi - 1)];
  }
  __syncthreads();   // the chain wave has solved the block
  if (lo >= hi) return;
  double xx[4], a[16];
#pragma unroll
  for (int k = 0; k < 4; ++k) xx[k] = ys[e + 16 * k];
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    a[u] = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) a[u] = fma(d[u][k], xx[k], a[u]);
  }
  const double r = red16x16(a, e);
  if (tm < hi) v[tm] = vold - r;
}

// v1[j] = y1[j] - <panel column j [ns, M), z[R]>: 64 columns per workgroup (four per 16-lane group),
// z[R] staged through LDS 512 entries at a time.
__global__ __launch_bounds__(256) void k_bwdu_t(const FrontTile* __restrict__ ft, int nft, const SNode* __restrict__ sn,
                                                const int32_t* __restrict__ rows, const double* __restrict__ store,
                                                const double* __restrict__ x, double* __restrict__ vbuf) {
  constexpr int ZC = 512;
  __shared__ double zs[ZC];
  const int64_t b = blockIdx.x;
  const int fi = find_front_tile(ft, nft, b);
  const SNode s = sn[ft[fi].s];
  const int64_t chunk = b - ft[fi].wg0;
  const int64_t M = (int64_t)s.ns + s.nu, ns = s.ns, nu = s.nu;
  const int32_t* R = rows + s.rowptr;
  const double* Lp = store + s.Loff;
  const int tid = threadIdx.x, g = tid >> 4, e = tid & 15;
  const double* ptr[4];
  bool ok[4];
  double a[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t j = chunk * 64 + u * 16 + g;
    ok[u] = j < ns;
    ptr[u] = Lp + (ok[u] ? j : 0) * M + ns;
    a[u] = 0.0;
  }
  for (int64_t c0 = 0; c0 < nu; c0 += ZC) {
    const int cl = (int)min<int64_t>(ZC, nu - c0);
    __syncthreads();
    for (int t = tid; t < cl; t += 256) zs[t] = x[R[c0 + t]];
    __syncthreads();
    const double* pc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) pc[u] = ptr[u] + c0;
    dots16<4>(pc, ok, zs, cl, e, a);
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const double r = red16(a[u]);
    const int64_t j = chunk * 64 + u * 16 + g;
    if (e == 0 && ok[u]) vbuf[s.voff + j] = x[s.first + j] - r;
  }
}

// ---- permutations and the column-wise residual ------------------------------------------------
// conj (a ComplexF64 handle's plain transpose: A^T \ b = conj(A^H \ conj(b))): the imaginary slots,
// odd indices of the caller's interleaved vectors, change sign on the way in and out.
// wrk[k] = b[q[k]]
__global__ void k_perm_in_t(int64_t n, const int64_t* __restrict__ q, const double* __restrict__ b,
                            double* __restrict__ wrk, int conj) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) {
    const int64_t c = q[k];
    const double val = b[c];
    wrk[k] = (conj && (c & 1)) ? -val : val;
  }
}
// x[p0[k]] = Rs[p0[k]] * wrk[k]
__global__ void k_perm_out_t(int64_t n, const int64_t* __restrict__ p0, const double* __restrict__ Rs,
                             const double* __restrict__ wrk, double* __restrict__ x, int conj) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) {
    const int64_t r = p0[k];
    const double val = Rs[r] * wrk[k];
    x[r] = (conj && (r & 1)) ? -val : val;
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
// One right-hand side runs the kernels above; a batch (rh.n > 1) their variants of
// kernels_solve_tb.hip on the same lists and workgroup counts.
static inline unsigned nblk_t(int64_t n, int b) { return (unsigned)((n + b - 1) / b); }
hipError_t launch_ut_tiny(hipStream_t st, int cnt, const int32_t* list, const SNode* sn, const int32_t* chlist,
                          const int32_t* relmap, const double* store, double* x, double* vbuf, Rhs rh, int micro) {
  if (cnt <= 0) return hipSuccess;
  if (rh.n > 1) return launch_ut_tiny_b(st, cnt, list, sn, chlist, relmap, store, x, vbuf, rh, micro);
  if (micro) {   // every front of the list has M <= 8
    k_ut_micro<<<nblk_t(cnt, 32), 256, 0, st>>>(list, cnt, sn, chlist, relmap, store, x, vbuf);
    return hipGetLastError();
  }
  k_ut_tiny<<<nblk_t(cnt, kTinyWaves), 64 * kTinyWaves, 0, st>>>(list, cnt, sn, chlist, relmap, store, x, vbuf);
  return hipGetLastError();
}
hipError_t launch_lt_tiny(hipStream_t st, int cnt, const int32_t* list, const SNode* sn, const int32_t* rows,
                          const int32_t* rowperm, const double* store, double* x, Rhs rh, int micro) {
  if (cnt <= 0) return hipSuccess;
  if (rh.n > 1) return launch_lt_tiny_b(st, cnt, list, sn, rows, rowperm, store, x, rh, micro);
  if (micro) {
    k_lt_micro<<<nblk_t(cnt, 32), 256, 0, st>>>(list, cnt, sn, rows, rowperm, store, x);
    return hipGetLastError();
  }
  k_lt_tiny<<<nblk_t(cnt, kTinyWaves), 64 * kTinyWaves, 0, st>>>(list, cnt, sn, rows, rowperm, store, x);
  return hipGetLastError();
}
hipError_t launch_ut_front(hipStream_t st, int cnt, const int32_t* list, const SNode* sn, const int32_t* chlist,
                           const int32_t* relmap, const double* store, double* x, double* vbuf, Rhs rh) {
  if (cnt <= 0) return hipSuccess;
  if (rh.n > 1) return launch_ut_front_b(st, cnt, list, sn, chlist, relmap, store, x, vbuf, rh);
  k_ut_front<<<cnt, 256, 0, st>>>(list, sn, chlist, relmap, store, x, vbuf);
  return hipGetLastError();
}
hipError_t launch_lt_front(hipStream_t st, int cnt, const int32_t* list, const SNode* sn, const int32_t* rows,
                           const int32_t* rowperm, const double* store, double* x, double* vbuf, Rhs rh) {
  if (cnt <= 0) return hipSuccess;
  if (rh.n > 1) return launch_lt_front_b(st, cnt, list, sn, rows, rowperm, store, x, vbuf, rh);
  k_lt_front<<<cnt, 256, 0, st>>>(list, sn, rows, rowperm, store, x, vbuf);
  return hipGetLastError();
}
hipError_t launch_pull_t(hipStream_t st, int64_t nwg, const FrontTile* ft, int nft, const SNode* sn,
                         const int32_t* gptr, const int32_t* gent, const double* x, double* vbuf, Rhs rh) {
  if (nwg <= 0) return hipSuccess;
  if (rh.n > 1) return launch_pull_tb(st, nwg, ft, nft, sn, gptr, gent, x, vbuf, rh);
  k_pull_t<<<(unsigned)nwg, 256, 0, st>>>(ft, nft, sn, gptr, gent, x, vbuf);
  return hipGetLastError();
}
hipError_t launch_tri_t(hipStream_t st, bool upper, int64_t nwg, const FrontTile* ft, int nft, int step,
                        const SNode* sn, const int32_t* rowperm, const double* store, double* x, double* vbuf,
                        Rhs rh) {
  if (nwg <= 0) return hipSuccess;
  if (rh.n > 1) return launch_tri_tb(st, upper, nwg, ft, nft, step, sn, rowperm, store, x, vbuf, rh);
  if (upper) k_tri_t<true><<<(unsigned)nwg, 320, 0, st>>>(ft, nft, step, sn, rowperm, store, x, vbuf);
  else k_tri_t<false><<<(unsigned)nwg, 320, 0, st>>>(ft, nft, step, sn, rowperm, store, x, vbuf);
  return hipGetLastError();
}
hipError_t launch_bwdu_t(hipStream_t st, int64_t nwg, const FrontTile* ft, int nft, const SNode* sn,
                         const int32_t* rows, const double* store, const double* x, double* vbuf, Rhs rh) {
  if (nwg <= 0) return hipSuccess;
  if (rh.n > 1) return launch_bwdu_tb(st, nwg, ft, nft, sn, rows, store, x, vbuf, rh);
  k_bwdu_t<<<(unsigned)nwg, 256, 0, st>>>(ft, nft, sn, rows, store, x, vbuf);
  return hipGetLastError();
}
// column j of b at b + j*ldb, of x at x + j*ldxo; of the work vectors at wrk + j*rh.ldx
hipError_t launch_perm_in_t(hipStream_t st, int64_t n, const int64_t* q, const double* b, int64_t ldb, double* wrk,
                            int conj, Rhs rh) {
  if (n <= 0) return hipSuccess;
  if (rh.n > 1) return launch_perm_in_tb(st, n, q, b, ldb, wrk, conj, rh);
  k_perm_in_t<<<nblk_t(n, 256), 256, 0, st>>>(n, q, b, wrk, conj);
  return hipGetLastError();
}
hipError_t launch_perm_out_t(hipStream_t st, int64_t n, const int64_t* p0, const double* Rs, const double* wrk,
                             double* x, int64_t ldxo, int conj, Rhs rh) {
  if (n <= 0) return hipSuccess;
  if (rh.n > 1) return launch_perm_out_tb(st, n, p0, Rs, wrk, x, ldxo, conj, rh);
  k_perm_out_t<<<nblk_t(n, 256), 256, 0, st>>>(n, p0, Rs, wrk, x, conj);
  return hipGetLastError();
}
hipError_t launch_residual_t(hipStream_t st, int64_t n, const int64_t* colptr, const int32_t* arow, const double* a,
                             const double* x, const double* b, double* r, double* nrm, int conj) {
  if (n <= 0) return hipSuccess;
  k_residual_t<<<nblk_t(n, 256), 256, 0, st>>>(n, colptr, arow, a, x, b, r, nrm, conj);
  return hipGetLastError();
}

}  // namespace smlu
