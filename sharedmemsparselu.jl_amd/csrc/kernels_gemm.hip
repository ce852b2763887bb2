// kernels_gemm.hip — dense fp64 Schur-complement updates C -= A*B (MFMA 128 and 64 tiles; the VALU
// 64 tile k_gemm is the bitwise comparison tile and the use_mfma = 0 path).
#include "kernels_common.hpp"

namespace smlu {

// ------------------------------------------------------------------------------------
// Dense update C -= A*B (fp64 VALU).  64x64 output tile per 256-thread workgroup, 4x4 per
// thread, K staged through LDS in slices of 16 with register prefetch of the next slice.
// ------------------------------------------------------------------------------------
__device__ __forceinline__ int find_gemm_task(const GemmTask* __restrict__ t, int cnt, int64_t b) {
  int lo = 0, hi = cnt - 1;
  while (lo < hi) {
    int mid = (lo + hi + 1) >> 1;
    if (t[mid].tile0 <= b) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}


// Tile placement.  (1) XCD-aware remap (bijective for any grid): the workgroups that share an
// XCD (same blockIdx % 8) get one contiguous range of tile indices; with in-order dispatch the
// tiles an XCD runs at the same time are then neighbours.  (2) Grouped order inside a task:
// groups of 8 tile rows, column-major inside a group, so 64 neighbouring tiles form an 8 x 8
// block of C and share 8 A row blocks and 8 B column blocks in that XCD's L2.
__device__ __forceinline__ int64_t xcd_remap(int64_t b, int64_t nwg) {
  const int64_t q = nwg >> 3, r = nwg & 7, x = b & 7;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (b >> 3);
}
// Windowed XCD-aware placement for launches whose tasks differ in cost (the batched F22 updates:
// thousands of small-k tasks next to a few large-k ones).  Blocks are dealt round-robin to the 8
// XCDs and roughly 512 run at a time (256 CUs x 2), so within each window of 512 blocks the 64 of
// one XCD take 64 consecutive tiles (one 8 x 8 group of tile_rc: shared A and B panels in that L2),
// while consecutive groups go to different XCDs: every XCD gets a share of every task.  (xcd_remap's
// one contiguous range per XCD left XCDs idle behind the large-k tasks.)  Bijective; a partial last
// window keeps dispatch order.
__device__ __forceinline__ int64_t xcd_window_remap(int64_t b, int64_t nwg) {
  constexpr int64_t W = 512;
  if (b >= (nwg / W) * W) return b;
  const int64_t w0 = b - b % W, i = b % W;
  return w0 + (i & 7) * (W / 8) + (i >> 3);
}
template <int TS>
__device__ __forceinline__ void tile_rc(const GemmTask& t, int64_t tl, int& tm, int& tn) {
  constexpr int GM = 8;
  const int64_t tiles_n = (t.n + TS - 1) / TS;
  const int64_t g = tl / (GM * tiles_n);
  const int first = (int)(g * GM);
  const int gm = min(GM, t.tiles_m - first);
  const int64_t in = tl - g * GM * tiles_n;
  tm = first + (int)(in % gm);
  tn = (int)(in / gm);
}

// Growth check of a GEMM-form triangular solve (task.gsid >= 0): max |result| of the tile, folded
// into growth[0] and the front's weak-pivot bit exactly as k_step_trsm does for its L rows.
struct GrowthArgs {
  int32_t* info;
  double* growth;
  double piv_tol;
};
__device__ __forceinline__ void tile_growth(const GrowthArgs& ga, int sid, double g) {
  g = wave_max(g);
  if ((threadIdx.x & 63) == 0 && g > 0.0) {
    atomic_max_pos(&ga.growth[0], g);
    if (g > 1.0 / ga.piv_tol) atomicOr(&ga.info[sid], 2);
  }
}

#define GBM 64
#define GBN 64
#define GBK 16
// TRSM = true: the GEMM-form triangular-solve launches (growth epilogue; a separate symbol so
// that profiles tell them apart from the Schur-complement updates)
template <bool TRSM>
__global__ __launch_bounds__(256) void k_gemm(const GemmTask* __restrict__ tasks, int ntask, GrowthArgs ga) {
  __shared__ double As[2][GBK][GBM + 2];
  __shared__ double Bs[2][GBK][GBN + 2];
  const int64_t b = xcd_remap(blockIdx.x, gridDim.x);
  const GemmTask t = tasks[find_gemm_task(tasks, ntask, b)];
  const gdbl* gA = gbl(t.A);
  const gdbl* gB = gbl(t.B);
  gdbl* gC = gbl(t.C);
  int tm, tn;
  tile_rc<GBM>(t, b - t.tile0, tm, tn);
  const int m0 = tm * GBM, n0 = tn * GBN;
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;  // 16 x 16 threads, 4x4 each
  // accumulators start from C (its loads overlap the first K slice's), B is staged negated:
  // acc = C + sum(A * -B), and the epilogue is stores only
  double acc[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = n0 + ty + 16 * j;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = m0 + tx + 16 * i;
      acc[i][j] = (col < t.n && row < t.m) ? gC[(int64_t)col * t.ldc + row] : 0.0;
    }
  }
  // load mapping: A slice GBM x GBK: thread -> (row = tid & 63, kk = (tid >> 6) + 4*r), r<4
  //               B slice GBK x GBN: thread -> (kk = tid & 15, col = (tid >> 4) + 16*r), r<4
  const int ar = tid & 63, ak = tid >> 6;
  const int bk = tid & 15, bc = tid >> 4;
  double ra[4], rb[4];
  const int K = t.k;
  auto gload = [&](int k0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int kk = ak + 4 * r;
      int row = m0 + ar;
      ra[r] = (row < t.m && k0 + kk < K) ? gA[(int64_t)(k0 + kk) * t.lda + row] : 0.0;
      int col = n0 + bc + 16 * r;
      rb[r] = (col < t.n && k0 + bk < K) ? gB[(int64_t)col * t.ldb + k0 + bk] : 0.0;
    }
  };
  auto sstore = [&](int buf) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      As[buf][ak + 4 * r][ar] = ra[r];
      Bs[buf][bk][bc + 16 * r] = -rb[r];
    }
  };
  int nk = (K + GBK - 1) / GBK;
  gload(0);
  sstore(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) gload((kt + 1) * GBK);
#pragma unroll 4
    for (int kk = 0; kk < GBK; ++kk) {
      double a[4], bb[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = As[cur][kk][tx + 16 * i];
#pragma unroll
      for (int j = 0; j < 4; ++j) bb[j] = Bs[cur][kk][ty + 16 * j];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fma(a[i], bb[j], acc[i][j]);
    }
    if (kt + 1 < nk) sstore(cur ^ 1);
    __syncthreads();
  }
  double gmax = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = n0 + ty + 16 * j;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = m0 + tx + 16 * i;
      if (col < t.n && row < t.m) {
        gC[(int64_t)col * t.ldc + row] = acc[i][j];
        gmax = fmax(gmax, fabs(acc[i][j]));
      }
    }
  }
  if (TRSM && t.gsid >= 0) tile_growth(ga, t.gsid, gmax);
}

// The same 64 x 64 tile on the fp64 matrix cores (tile code 66, the default for k > 64 launches
// below the 128-tile threshold; SMLU_SMALLK=0 keeps k_gemm): identical staging and slices, each
// wave a 32 x 32 quadrant of 2 x 2 v_mfma_f64_16x16x4 blocks (lane l of block (i, j) holds
// C[16 i + (l & 15)][16 j + (l >> 4) + 4 r]); per element one fused multiply-add per k in
// ascending order, bitwise k_gemm's result.
typedef double v4d __attribute__((ext_vector_type(4)));
template <bool TRSM>
__global__ __launch_bounds__(256) void k_gemm64_mfma(const GemmTask* __restrict__ tasks, int ntask, GrowthArgs ga) {
  __shared__ double As[2][GBK][GBM + 2];
  __shared__ double Bs[2][GBK][GBN + 2];
  const int64_t b = xcd_remap(blockIdx.x, gridDim.x);
  const GemmTask t = tasks[find_gemm_task(tasks, ntask, b)];
  const gdbl* gA = gbl(t.A);
  const gdbl* gB = gbl(t.B);
  gdbl* gC = gbl(t.C);
  int tm, tn;
  tile_rc<GBM>(t, b - t.tile0, tm, tn);
  const int m0 = tm * GBM, n0 = tn * GBN;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = (wv & 1) * 32, wc = (wv >> 1) * 32;
  const int li = lane & 15, lk = lane >> 4;
  v4d acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = m0 + wr + 16 * i + li;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int col = n0 + wc + 16 * j + lk + 4 * r;
        acc[i][j][r] = (col < t.n && row < t.m) ? gC[(int64_t)col * t.ldc + row] : 0.0;
      }
  }
  const int ar = tid & 63, ak = tid >> 6;
  const int bk = tid & 15, bc = tid >> 4;
  double ra[4], rb[4];
  const int K = t.k;
  auto gload = [&](int k0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int kk = ak + 4 * r;
      const int row = m0 + ar;
      ra[r] = (row < t.m && k0 + kk < K) ? gA[(int64_t)(k0 + kk) * t.lda + row] : 0.0;
      const int col = n0 + bc + 16 * r;
      rb[r] = (col < t.n && k0 + bk < K) ? gB[(int64_t)col * t.ldb + k0 + bk] : 0.0;
    }
  };
  auto sstore = [&](int buf) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      As[buf][ak + 4 * r][ar] = ra[r];
      Bs[buf][bk][bc + 16 * r] = -rb[r];
    }
  };
  const int nk = (K + GBK - 1) / GBK;
  gload(0);
  sstore(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) gload((kt + 1) * GBK);
#pragma unroll
    for (int kq = 0; kq < GBK / 4; ++kq) {
      const int k = 4 * kq + lk;
      double fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) fa[i] = As[cur][k][wr + 16 * i + li];
#pragma unroll
      for (int j = 0; j < 2; ++j) fb[j] = Bs[cur][k][wc + 16 * j + li];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fb[j], fa[i], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < nk) sstore(cur ^ 1);
    __syncthreads();
  }
  double gmax = 0.0;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = m0 + wr + 16 * i + li;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int col = n0 + wc + 16 * j + lk + 4 * r;
        if (col < t.n && row < t.m) {
          gC[(int64_t)col * t.ldc + row] = acc[i][j][r];
          gmax = fmax(gmax, fabs(acc[i][j][r]));
        }
      }
  }
  if (TRSM && t.gsid >= 0) tile_growth(ga, t.gsid, gmax);
}

// Small-k variant of k_gemm (every task of the launch has k <= 64: the in-block updates and the
// GEMM-form triangular solves): the whole K extent of the A and B tiles is staged in one shot
// (32 loads per thread in flight together with the 16 C loads), so a launch pays one memory
// round trip instead of one per 16-deep slice.  Same per-element arithmetic as k_gemm.
// One 64 x 64 output tile [m0, m0+64) x [n0, n0+64) of an m x n task (k <= 64), by the whole
// 256-thread workgroup; returns the thread's max |result| (growth epilogue of the TRSM form).
// All loads (C, A, B) complete before the first store, so B == C (in place) is allowed.
// On the fp64 matrix cores (round 5; the VALU form it replaced took 1.1 ms more in-block update
// and 1.6 ms more GEMM-form TRSM time per 128^3 refactor): each wave a 32 x 32 quadrant of 2 x 2
// v_mfma_f64_16x16x4 blocks over the staged A / -B images (lane l of block (i, j) holds
// C[16 i + (l & 15)][16 j + (l >> 4) + 4 r]).  Per element the MFMA's chain is one fused
// multiply-add per k in ascending order, the zero-filled k >= K terms exact no-ops: bitwise the
// VALU tiles' result.
__device__ __forceinline__ double k64_tile_mfma(const gdbl* gA, int lda, const gdbl* gB, int ldb, gdbl* gC, int ldc,
                                                int m, int n, int K, int m0, int n0,
                                                double (&As)[64][GBM + 2], double (&Bs)[64][GBN + 2]) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = (wv & 1) * 32, wc = (wv >> 1) * 32;
  const int li = lane & 15, lk = lane >> 4;
  v4d acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = m0 + wr + 16 * i + li;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int col = n0 + wc + 16 * j + lk + 4 * r;
        acc[i][j][r] = (col < n && row < m) ? gC[(int64_t)col * ldc + row] : 0.0;
      }
  }
  // A: row = tid & 63, k = (tid >> 6) + 4r;  B: k = tid & 63, col = (tid >> 6) + 4r
  const int ar = tid & 63, ak = tid >> 6;
  double ra[16], rb[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int kk = ak + 4 * r, row = m0 + ar;
    ra[r] = (row < m && kk < K) ? gA[(int64_t)kk * lda + row] : 0.0;
    const int col = n0 + ak + 4 * r;
    rb[r] = (col < n && ar < K) ? gB[(int64_t)col * ldb + ar] : 0.0;
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    As[ak + 4 * r][ar] = ra[r];
    Bs[ar][ak + 4 * r] = -rb[r];
  }
  __syncthreads();
  auto kquad = [&](int kq) {
    const int k = 4 * kq + lk;
    double fa[2], fb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) fa[i] = As[k][wr + 16 * i + li];
#pragma unroll
    for (int j = 0; j < 2; ++j) fb[j] = Bs[k][wc + 16 * j + li];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fb[j], fa[i], acc[i][j], 0, 0, 0);
  };
  if (K == 64) {   // full panels (w = 64): straight-line
#pragma unroll
    for (int kq = 0; kq < 16; ++kq) kquad(kq);
  } else {
    const int nkq = (K + 3) >> 2;
    for (int kq = 0; kq < nkq; ++kq) kquad(kq);
  }
  double gmax = 0.0;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = m0 + wr + 16 * i + li;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int col = n0 + wc + 16 * j + lk + 4 * r;
        if (col < n && row < m) {
          gC[(int64_t)col * ldc + row] = acc[i][j][r];
          gmax = fmax(gmax, fabs(acc[i][j][r]));
        }
      }
  }
  return gmax;
}

template <bool TRSM>
__global__ __launch_bounds__(256) void k_gemm_k64(const GemmTask* __restrict__ tasks, int ntask, GrowthArgs ga) {
  __shared__ double As[64][GBM + 2];   // [k][row]
  __shared__ double Bs[64][GBN + 2];   // [k][col], negated
  const int64_t b = xcd_remap(blockIdx.x, gridDim.x);
  const GemmTask t = tasks[find_gemm_task(tasks, ntask, b)];
  int tm, tn;
  tile_rc<GBM>(t, b - t.tile0, tm, tn);
  const double gmax = k64_tile_mfma(gbl(t.A), t.lda, gbl(t.B), t.ldb, gbl(t.C), t.ldc, t.m, t.n, t.k, tm * GBM,
                                    tn * GBN, As, Bs);
  if (TRSM && t.gsid >= 0) tile_growth(ga, t.gsid, gmax);
}

// ------------------------------------------------------------------------------------
// 128 x 128 output tiles on the fp64 matrix cores (opts.use_mfma = 1, the default; use_mfma = 0
// runs every launch on the VALU 64 tile k_gemm), K staged through double-buffered LDS slices of
// 16.  v_mfma_f64_16x16x4_f64; each wave owns a 64x64 quadrant = 4x4
// blocks.  The product is formed as C^T = B^T A^T so that the accumulator's lane index runs
// along C's rows (column-major C stays coalesced): lane l of block (bi,bj) holds
// C[row = 16 bi + (l & 15)][col = 16 bj + (l >> 4) + 4 r], r = 0..3.
#define HBM_ 128
#define HBK_ 16
// c ? x : +0.0 as a bit mask (keeps the compiler from sinking the load into a branch)
__device__ __forceinline__ double sel0(bool c, double x) {
  return __longlong_as_double(__double_as_longlong(x) & (c ? -1LL : 0LL));
}
// F22 gathered in the C prologue (tile code 143, device.hpp: F22Gather / F22Child): the tile starts
// from the sum of the children's F22 entries -- what the assembly would have written to C -- formed
// per entry as ((+0.0 + c1) + c2) + ... in child order.  A child without the entry adds +0.0, which
// leaves the running sum's bits as they are (it starts at +0.0 and so is never -0.0).
struct GatherArgs {
  const F22Gather* tg;   // per task of the launch
  const F22Child* ch;
  const int32_t* inv;
  const double* scratch;
};
struct F22Tile {         // one task's children (cnt < 0: plain C load)
  const F22Child* ch;
  const int32_t* inv;
  const double* scratch;
  int cnt;
};
// entry (ri, cj) of a child's F22 (ld nuc); +0.0 where either index is -1.  The load itself is
// unconditional and in bounds (entry 0), the select a bit mask: no branch around a load.  Uniform
// base + 32-bit byte offset per lane (the builder gathers only from children with 8 nu^2 < 2^32),
// so an address costs one VGPR.
__device__ __forceinline__ double f22_child_val(const char* src, int nuc, int ri, int cj) {
  const bool ok = (ri | cj) >= 0;
  const uint32_t off = ok ? ((uint32_t)cj * (uint32_t)nuc + (uint32_t)ri) * 8u : 0u;
  return sel0(ok, *(const gdbl*)(src + off));
}
// The 4 NI entries rows ri[0..NI) x columns cj[0..3] of one child added into acc[i][j][r], as one
// group of loads: the scheduling fence keeps the next group's loads (and their 48 registers)
// behind this group's additions, so the prologue stays inside the tile's register budget.
template <int NI, int NJ>
__device__ __forceinline__ void f22_child_add(v4d (&acc)[NI][NJ], int j, const char* src, int nuc, const int (&ri)[NI],
                                              const int (&cj)[4]) {
  double v[NI][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int i = 0; i < NI; ++i) v[i][r] = f22_child_val(src, nuc, ri[i], cj[r]);
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int i = 0; i < NI; ++i) acc[i][j][r] += v[i][r];
  __builtin_amdgcn_sched_barrier(0);
}

// Pair types and global accessors of the v3 tile.
typedef double v2du __attribute__((ext_vector_type(2), aligned(8)));   // 8-byte aligned pairs (global)
typedef double v2d __attribute__((ext_vector_type(2)));                 // 16-byte aligned pairs (LDS)
// Global accesses: wave-uniform 64-bit base (SGPRs, recomputed by scalar ALU where used) + a
// per-lane 32-bit byte offset fixed for the whole tile, so no 64-bit per-lane address is live
// across the K loop (the v1 interior spilled its precomputed C addresses).
__device__ __forceinline__ v2d ldu2(const char* ubase, uint32_t off) {
  return *(const __attribute__((address_space(1))) v2du*)(ubase + off);
}
__device__ __forceinline__ void stu2(char* ubase, uint32_t off, v2d v) {
  *(__attribute__((address_space(1))) v2du*)(ubase + off) = v;
}

// ------------------------------------------------------------------------------------
// MFMA tile v3 (tile code 131): the v2 tile's output mapping and per-element arithmetic (acc = C,
// then one fp64 MFMA-FMA per k in ascending k: bitwise identical to v2 and the VALU tiles), with
// the K slices staged by LDS-DMA instead of registers:
//  * global_load_lds_dwordx4 (16 bytes per lane, lane-linear LDS destination): A as k-rows of
//    128 doubles (one 1 KB row per wave instruction, the v2 image [k][row]); B as 8 columns x 16 k
//    per wave instruction, image [col][k] with the k pairs of column c stored at pair slot
//    p ^ ((c >> 1) & 7) (the swizzle is applied to the per-lane SOURCE address, the LDS side stays
//    lane-linear), which makes the fragment reads -- 16 consecutive columns at one k per
//    half-wave -- bank-conflict free;
//  * B's sign flip is the MFMA's own neg modifier on the B fragment (exact: -b*a = b*(-a)), so no
//    staging VALU work and no staging registers: the 32 VGPRs v2 spent on the in-flight slice
//    hold a second fragment set instead.  In the interior tile the fragments of k-quad q+1 are read
//    behind the first MFMA of quad q and waited for behind its last (pinned by scheduling fences;
//    tools/isa_kloop.py --check reads it back from the assembly); the edge tiles leave the
//    placement to the compiler;
//  * one barrier per slice, which also retires the slice's DMA.  The next slice's DMA goes into
//    the other buffer, whose readers passed the previous barrier: in the interior tile behind the
//    first MFMAs of quad 0, two loads at a time, with the barrier between quads 2 and 3 (every
//    instantiation; the EB parameter no longer changes the interior loop); in the edge tiles at
//    the top of the slice with the barrier at its end;
//  * a partial last slice (K % 16) is staged through registers with zero fill, into the same
//    images (no guard in the compute loop).
// Interior tiles only; edge tiles take gemm128_mfma3_edge (same arithmetic).
// ------------------------------------------------------------------------------------
struct Mfma3Lds {
  double A[2][HBK_][HBM_];   // [buf][k][row]
  double B[2][HBM_][HBK_];   // [buf][col][k, pair-swizzled]
};
static_assert(sizeof(Mfma3Lds) == 65536, "v3 tile LDS image");
typedef __attribute__((address_space(3))) void lds_void;

__device__ __forceinline__ void glds16(const void* src, void* lds_dst) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (lds_void*)lds_dst, 16, 0, 0);
}

// A wave-uniform pointer pinned in scalar registers: base + (32-bit lane offset) then selects the
// scalar-base form of the load, and the base arithmetic stays on the scalar ALU.
__device__ __forceinline__ const char* uniform_ptr(const char* p) {
  const uint64_t v = reinterpret_cast<uint64_t>(p);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return reinterpret_cast<const char*>(((uint64_t)hi << 32) | lo);
}

// The same LDS-DMA load in its scalar-base form, global_load_lds_dwordx4 voff, s[base]: source =
// wave-uniform base + 32-bit lane offset, no vector ALU work per load.  (The compiler's selection
// of this form needs the zero extension of the offset in the load's own basic block, which loop
// hoisting defeats, hence the instruction by name.)  The compiler does not count this load in
// vmcnt: the barrier that publishes the slice needs its own s_waitcnt vmcnt(0).
__device__ __forceinline__ void glds16s(const char* ubase, uint32_t voff, void* lds_dst) {
  const uint32_t dst = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(lds_void*)lds_dst);
  asm volatile("s_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(uniform_ptr(ubase)), "{m0}"(dst) : "memory");
}

#ifdef SMLU_CLOCK_PROBE
// Dev build only (tools/gemm_clock.sh): where a slice of the interior K loop spends its cycles.
// Every wave stamps s_memtime at the segment ends and keeps per-segment scalar sums; wave 0 of
// workgroup 0 of an armed launch adds them to g_clock_probe[8 + 8 form + segment] (segment 6: slices,
// 7: launches).  The stamp drains the wave's LDS reads, so the build reads shares, not run time.
__device__ unsigned long long* g_clock_probe = nullptr;
struct KloopStamps {
  unsigned long long last, sum[6];
  unsigned n;
  static __device__ __forceinline__ unsigned long long now() {
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
  }
  __device__ __forceinline__ void start() {
    for (int b = 0; b < 6; ++b) sum[b] = 0;
    n = 0;
    last = now();
  }
  __device__ __forceinline__ void mark(int b) {
    const unsigned long long t = now();
    sum[b] += t - last;
    last = t;
    if (b == 5) ++n;
  }
  __device__ __forceinline__ void done(int form) const {
    unsigned long long* p = g_clock_probe;
    if (p && blockIdx.x == 0 && threadIdx.x == 0) {
      for (int b = 0; b < 6; ++b) atomicAdd(p + 8 + 8 * form + b, sum[b]);
      atomicAdd(p + 8 + 8 * form + 6, (unsigned long long)n);
      atomicAdd(p + 8 + 8 * form + 7, 1ull);
    }
  }
};
// segments: the slice's quad 0 with the fragment reads and DMA pieces behind its MFMAs; quads 1-2;
// the barrier with its vmcnt(0)/lgkmcnt(0); quad 3 with the next slice's first fragment reads.
// (KS_DMA, KS_PBW: the DMA block at the slice top and the exposed reads behind the barrier of the
// earlier loop form; zero now, kept so that reports of both forms read alike.)
enum { KS_DMA = 0, KS_Q0 = 1, KS_Q12 = 2, KS_BAR = 3, KS_PBW = 4, KS_Q3 = 5 };
#define KLOOP_DECL() KloopStamps ks
#define KLOOP_START() ks.start()
#define KLOOP_MARK(b) ks.mark(b)
#define KLOOP_DONE(form) ks.done(form)
#else
#define KLOOP_DECL()
#define KLOOP_START()
#define KLOOP_MARK(b)
#define KLOOP_DONE(form)
#endif

template <bool TRSM, bool EB, bool GATHER = false>
__device__ __forceinline__ void gemm128_mfma3_interior(const GemmTask& t, int m0, int n0, Mfma3Lds& S,
                                                       const GrowthArgs& ga, const F22Tile& fg = F22Tile{}) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = (wv & 1) * 64, wc = (wv >> 1) * 64;
  const int li = lane & 15, lk = lane >> 4;
  const int K = t.k;
  const int64_t lda = t.lda, ldb = t.ldb, ldc = t.ldc;
  const uint32_t c_lo = (uint32_t)(((int64_t)lk * ldc + 2 * li) * 8);
  auto cbase = [&](int ip, int j, int r) {
    return reinterpret_cast<char*>(t.C) + ((int64_t)(n0 + wc + 16 * j + 4 * r) * ldc + m0 + wr + 32 * ip) * 8;
  };
  // DMA sources of this lane.  A: k-row wv + 4q of the slice, rows m0 + 2 lane, +1.
  // B: wave instruction q covers columns 8 (wv + 4q) + [0, 8); lane -> column 8 (wv + 4q) + (lane >> 3),
  //    pair slot lane & 7 holding k pair (lane & 7) ^ ((column >> 1) & 7) = (lane & 7) ^ ((4 wv + (lane >> 4)) & 7).
  const int bpair = (lane & 7) ^ ((4 * wv + (lane >> 4)) & 7);
  const char* asrc = reinterpret_cast<const char*>(t.A) + ((int64_t)wv * lda + m0 + 2 * lane) * 8;
  const char* bsrc = reinterpret_cast<const char*>(t.B) + ((int64_t)(n0 + 8 * wv + (lane >> 3)) * ldb + 2 * bpair) * 8;
  auto issue = [&](int k0, int buf) {   // one full slice (k0 + 16 <= K): 4 + 4 DMA per wave
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      glds16(asrc + ((int64_t)(k0 + 4 * q) * lda) * 8, &S.A[buf][wv + 4 * q][0]);
      glds16(bsrc + ((int64_t)32 * q * ldb + k0) * 8, &S.B[buf][8 * (wv + 4 * q)][0]);
    }
  };
  // The same pieces one at a time (piece p of 8: A k-rows on even p, B columns on odd p), addressed
  // as wave-uniform base + 32-bit lane offset so that the per-slice address arithmetic is scalar.
  const char* asrc_u = reinterpret_cast<const char*>(t.A) + ((int64_t)wv * lda + m0) * 8;
  const char* bsrc_u = reinterpret_cast<const char*>(t.B) + ((int64_t)(n0 + 8 * wv) * ldb) * 8;
  const uint32_t a_lane = (uint32_t)lane * 16u;
  const uint32_t b_lane = ((uint32_t)(lane >> 3) * (uint32_t)ldb + 2u * (uint32_t)bpair) * 8u;   // < 64 ldb
  auto piece = [&](int k0, int buf, int p) {
    const int q = p >> 1;
    if (p & 1) glds16s(bsrc_u + ((int64_t)32 * q * ldb + k0) * 8, b_lane, &S.B[buf][8 * (wv + 4 * q)][0]);
    else glds16s(asrc_u + ((int64_t)(k0 + 4 * q) * lda) * 8, a_lane, &S.A[buf][wv + 4 * q][0]);
  };
  auto stage_tail = [&](int k0, int buf) {   // partial slice: guarded register loads, zero fill
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int ka = k0 + wv + 4 * q;
      const v2d a = ka < K ? ldu2(asrc + ((int64_t)(k0 + 4 * q) * lda) * 8, 0) : v2d{0.0, 0.0};
      *reinterpret_cast<v2d*>(&S.A[buf][wv + 4 * q][2 * lane]) = a;
      const gdbl* bp = gbl(reinterpret_cast<const double*>(bsrc + ((int64_t)32 * q * ldb + k0) * 8));
      const int kb = k0 + 2 * bpair;
      v2d b;
      b.x = kb < K ? bp[0] : 0.0;
      b.y = kb + 1 < K ? bp[1] : 0.0;
      *reinterpret_cast<v2d*>(&S.B[buf][8 * (wv + 4 * q)][2 * lane]) = b;
    }
  };
  v4d acc[4][4];
  if (GATHER && fg.cnt >= 0) {
    // C gathered from the children: the lane's rows m0 + wr + 32 ip + 2 li (+1) and columns
    // n0 + wc + 16 j + lk + 4 r.  One child at a time: its 4 row and 16 column indices first, then
    // the masked value loads; a child that misses this wave's quadrant is skipped (uniform test).
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
    for (int d = 0; d < fg.cnt; ++d) {
      const F22Child c = fg.ch[d];
      if (c.hi < m0 + wr || c.lo >= m0 + wr + 64 || c.hi < n0 + wc || c.lo >= n0 + wc + 64) continue;
      const int32_t* inv = fg.inv + c.inv;
      const char* src = reinterpret_cast<const char*>(fg.scratch + c.foff);
      int ri[4], cj[4][4];
#pragma unroll
      for (int ip = 0; ip < 2; ++ip) {
        ri[2 * ip] = inv[m0 + wr + 32 * ip + 2 * li];
        ri[2 * ip + 1] = inv[m0 + wr + 32 * ip + 2 * li + 1];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) cj[j][r] = inv[n0 + wc + 16 * j + lk + 4 * r];
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < 4; ++j) f22_child_add(acc, j, src, c.nu, ri, cj[j]);
    }
  } else {
#pragma unroll
    for (int ip = 0; ip < 2; ++ip)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const v2d c = ldu2(cbase(ip, j, r), c_lo);
          acc[2 * ip][j][r] = c.x;
          acc[2 * ip + 1][j][r] = c.y;
        }
  }
  // fragment addresses: A row pair wr + 32 ip + 2 li at k = 4 kq + lk; B column wc + 16 j + li at
  // k = 4 kq + lk, i.e. pair 2 kq + (lk >> 1), slot that ^ (li >> 1), element lk & 1
  const int a_off = (lk * HBM_ + wr + 2 * li);
  int b_off[4];
#pragma unroll
  for (int kq = 0; kq < 4; ++kq) b_off[kq] = (wc + li) * HBK_ + (((2 * kq + (lk >> 1)) ^ (li >> 1)) << 1) + (lk & 1);
  auto frags = [&](int cur, int kq, v2d (&fa)[2], double (&fb)[4]) {
    const double* As = &S.A[cur][0][0] + a_off + kq * 4 * HBM_;
    const double* Bs = &S.B[cur][0][0] + b_off[kq];
#pragma unroll
    for (int ip = 0; ip < 2; ++ip) fa[ip] = *reinterpret_cast<const v2d*>(As + 32 * ip);
#pragma unroll
    for (int j = 0; j < 4; ++j) fb[j] = Bs[16 * HBK_ * j];
  };
  // MFMA n (0..15) of a k-quad: accumulator (2 ip + (n & 1), j) with ip = n >> 3, j = (n >> 1) & 3.
  // Each accumulator takes exactly one MFMA per quad, quads in ascending k.   neg:[1,0,0]: C - B*A
  auto mf = [&](int n, const v2d (&fa)[2], const double (&fb)[4]) {
    const int ip = n >> 3, j = (n >> 1) & 3;
    if (n & 1) acc[2 * ip + 1][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fb[j], fa[ip].y, acc[2 * ip + 1][j], 0, 0, 1);
    else acc[2 * ip][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fb[j], fa[ip].x, acc[2 * ip][j], 0, 0, 1);
  };
  auto rest = [&](const v2d (&fa)[2], const double (&fb)[4]) {   // MFMAs 1..15 of a quad
#pragma unroll
    for (int n = 1; n < 16; ++n) mf(n, fa, fb);
  };
  // One slice.  The two fragment sets alternate by quad; the set that quad q + 1 needs is read right
  // behind quad q's FIRST MFMA -- its registers were last used by quad q - 1, whose MFMAs have all
  // been issued -- and waited for behind quad q's last one, 15 MFMAs later.  The next slice's eight
  // DMA pieces follow in pairs behind MFMAs 1, 3, 5 and 7 of quad 0 (their buffer is free since the
  // previous barrier), the last pair 40 MFMAs ahead of the vmcnt(0) in front of the barrier between
  // quads 2 and 3; behind that barrier come quad 3's first MFMA and only then the next slice's
  // quad-0 fragments.  The scheduling fences pin this order: every group of non-MFMA work has an
  // MFMA of this wave in flight.  The barrier and the reads behind it run on the last slice too (the
  // reads fetch stale LDS that nothing uses), so the loop body has no join that carries LDS reads:
  // only the DMA pieces and the partial slice's register staging sit under (uniform) branches.
  // Two slices per loop trip make the LDS buffer a compile-time constant, so every fragment address
  // is one per-lane register plus an immediate; with the scalar-base DMA form the loop has no
  // vector ALU instruction besides the MFMAs (each one costs the wave an issue slot it has to win
  // against the other workgroup's wave on the same SIMD).
  const int nk = (K + HBK_ - 1) / HBK_;
  const int nfull = K / HBK_;
  v2d fa0[2], fa1[2];
  double fb0[4], fb1[4];
  auto lds_wait = [] {   // s_waitcnt lgkmcnt(0) alone, in its place
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_sched_barrier(0);
  };
  if (nfull > 0) issue(0, 0);
  else stage_tail(0, 0);
  __syncthreads();
  frags(0, 0, fa0, fb0);
  lds_wait();
  KLOOP_DECL();
  KLOOP_START();
  auto body = [&](int kt, auto cur_c) {
    constexpr int cur = decltype(cur_c)::value;
    const int k1 = (kt + 1) * HBK_;
    const bool next_full = kt + 1 < nfull;
    mf(0, fa0, fb0);
    __builtin_amdgcn_sched_barrier(0);
    frags(cur, 1, fa1, fb1);
    if (kt + 1 < nk && !next_full) stage_tail(k1, cur ^ 1);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int n = 1; n < 16; ++n) {
      mf(n, fa0, fb0);
      if ((n & 1) && n < 8) {
        __builtin_amdgcn_sched_barrier(0);
        if (next_full) {
          piece(k1, cur ^ 1, n - 1);
          piece(k1, cur ^ 1, n);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    lds_wait();
    KLOOP_MARK(KS_Q0);
    mf(0, fa1, fb1);
    __builtin_amdgcn_sched_barrier(0);
    frags(cur, 2, fa0, fb0);
    __builtin_amdgcn_sched_barrier(0);
    rest(fa1, fb1);
    lds_wait();
    mf(0, fa0, fb0);
    __builtin_amdgcn_sched_barrier(0);
    frags(cur, 3, fa1, fb1);
    __builtin_amdgcn_sched_barrier(0);
    rest(fa0, fb0);
    KLOOP_MARK(KS_Q12);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_waitcnt(0x0070);   // vmcnt(0) lgkmcnt(0): this wave's DMA pieces have landed
    __syncthreads();
    __builtin_amdgcn_sched_barrier(0);
    KLOOP_MARK(KS_BAR);
    mf(0, fa1, fb1);
    __builtin_amdgcn_sched_barrier(0);
    frags(cur ^ 1, 0, fa0, fb0);
    __builtin_amdgcn_sched_barrier(0);
    rest(fa1, fb1);
    lds_wait();
    KLOOP_MARK(KS_Q3);
  };
  for (int kt = 0;; kt += 2) {   // two slices per trip: the LDS buffer is a compile-time constant
    body(kt, std::integral_constant<int, 0>{});
    if (kt + 1 >= nk) break;
    body(kt + 1, std::integral_constant<int, 1>{});
    if (kt + 2 >= nk) break;
  }
  KLOOP_DONE(EB ? 0 : 1);
  double gmax = 0.0;
#pragma unroll
  for (int ip = 0; ip < 2; ++ip)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const v2d c = v2d{acc[2 * ip][j][r], acc[2 * ip + 1][j][r]};
        stu2(cbase(ip, j, r), c_lo, c);
        if (TRSM) gmax = fmax(gmax, fmax(fabs(c.x), fabs(c.y)));
      }
  if (TRSM && t.gsid >= 0) tile_growth(ga, t.gsid, gmax);
}

// ------------------------------------------------------------------------------------
// Edge tiles of the v3 tile: lm = min(128, m - m0) live rows, ln = min(128, n - n0) live columns,
// not both 128.  Same LDS images, fragment reads and per-element arithmetic as the interior (acc = C
// or the gathered child sum, one MFMA multiply-add per k, ascending, B negated by the MFMA
// modifier), so the results are bitwise those of every other tile.  What differs:
//  * the four waves are laid over the live region (LAYOUT, chosen per workgroup from lm, ln):
//      0  lm > 64, ln > 64   2 x 2 quadrants of 64 x 64 (the interior's layout)
//      1  ln <= 64           four 32-row strips x 64 columns
//      2  lm <= 64           64 rows x four 32-column strips
//      3  both <= 64         2 x 2 of 32 x 32
//    and inside a wave the MFMA blocks beyond the live extent are skipped by uniform branches
//    around statically indexed accumulators (32-row granularity: an accumulator pair holds the
//    even and odd rows of a 32-row block; 16-column granularity);
//  * operand rows and columns outside the task are replaced by clamped (in-range) ones: a row of A
//    beyond m or a column of B beyond n feeds only outputs that are never stored.  B always goes by
//    LDS-DMA; A goes by LDS-DMA when every lane's 16-byte row pair lies inside the column (lm even
//    or 128) and through registers (two clamped 8-byte loads per lane) when m is odd.  The partial
//    last K slice is zero filled through registers as in the interior;
//  * C is loaded from clamped addresses without guards (an accumulator entry outside the task
//    holds some other entry's value and is never stored) and stored under one guard per row pair
//    and column; the growth maximum is taken over stored entries only.
// Every global access is inside the task's operands for every lane.
// ------------------------------------------------------------------------------------
template <bool TRSM, bool GATHER, int LAYOUT>
__device__ __forceinline__ void gemm128_mfma3_edge(const GemmTask& t, int m0, int n0, int lm, int ln, Mfma3Lds& S,
                                                   const GrowthArgs& ga, const F22Tile& fg) {
  constexpr int NIP = (LAYOUT == 0 || LAYOUT == 2) ? 2 : 1;   // 32-row blocks (accumulator pairs) per wave
  constexpr int NJ = (LAYOUT == 0 || LAYOUT == 1) ? 4 : 2;    // 16-column blocks per wave
  constexpr int BQ = (LAYOUT == 0 || LAYOUT == 2) ? 4 : 2;    // B staging steps per wave (columns >= 64 unread when ln <= 64)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = LAYOUT == 0 ? (wv & 1) * 64 : LAYOUT == 1 ? wv * 32 : LAYOUT == 2 ? 0 : (wv & 1) * 32;
  const int wc = LAYOUT == 0 ? (wv >> 1) * 64 : LAYOUT == 1 ? 0 : LAYOUT == 2 ? wv * 32 : (wv >> 1) * 32;
  const int li = lane & 15, lk = lane >> 4;
  const int K = t.k;
  const int64_t lda = t.lda, ldb = t.ldb;
  const uint32_t ldc = (uint32_t)t.ldc;
  // live blocks of this wave (uniform)
  const int nipl = min(NIP, max(0, (lm - wr + 31) >> 5));
  const int njl = min(NJ, max(0, (ln - wc + 15) >> 4));
  const bool live = nipl > 0 && njl > 0;
  // C: uniform tile origin + 32-bit byte offset per lane (tile-relative row rl, column cl; at most
  // 8 (127 ldc + 127) bytes: fits for any front that fits in memory)
  char* cb = reinterpret_cast<char*>(t.C) + ((int64_t)n0 * t.ldc + m0) * 8;
  v4d acc[2 * NIP][NJ];
  if (GATHER && fg.cnt >= 0) {
    // as in the interior, with the row and column indices read at clamped positions (-1 outside
    // the task) and the child test on this wave's live rows and columns
#pragma unroll
    for (int i = 0; i < 2 * NIP; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[i][j] = v4d{0.0, 0.0, 0.0, 0.0};
    if (live) {
#pragma unroll 1
      for (int d = 0; d < fg.cnt; ++d) {
        const F22Child c = fg.ch[d];
        if (c.hi < m0 + wr || c.lo >= m0 + wr + 32 * nipl || c.hi < n0 + wc || c.lo >= n0 + wc + 16 * njl) continue;
        const int32_t* inv = fg.inv + c.inv;
        const char* src = reinterpret_cast<const char*>(fg.scratch + c.foff);
        int ri[2 * NIP], cj[NJ][4];
#pragma unroll
        for (int i = 0; i < 2 * NIP; ++i) {
          const int row = m0 + wr + 32 * (i >> 1) + 2 * li + (i & 1);
          const int v = inv[min(row, t.m - 1)];
          ri[i] = row < t.m ? v : -1;
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int col = n0 + wc + 16 * j + lk + 4 * r;
            const int v = inv[min(col, t.n - 1)];
            cj[j][r] = col < t.n ? v : -1;
          }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          if (j < njl) f22_child_add(acc, j, src, c.nu, ri, cj[j]);
      }
    }
  } else {
#pragma unroll
    for (int ip = 0; ip < NIP; ++ip) {
      const int rl = wr + 32 * ip + 2 * li;
      const int rc = min(rl, lm - 2);   // pair start inside the column (lm >= 2)
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const uint32_t cl = (uint32_t)min(wc + 16 * j + lk + 4 * r, ln - 1);
          if (lm >= 2) {
            const v2d c = ldu2(cb, (cl * ldc + (uint32_t)rc) * 8u);
            acc[2 * ip][j][r] = rl > rc ? c.y : c.x;   // odd m: row m - 1 is the pair's second entry
            acc[2 * ip + 1][j][r] = c.y;
          } else {
            acc[2 * ip][j][r] = acc[2 * ip + 1][j][r] = *(const gdbl*)(cb + cl * ldc * 8u);
          }
        }
    }
  }
  // staging.  B by LDS-DMA: slot column 8 (wv + 4q) + (lane >> 3) from source column min(slot, ln - 1).
  const int bpair = (lane & 7) ^ ((4 * wv + (lane >> 4)) & 7);
  const char* bbase = reinterpret_cast<const char*>(t.B) + ((int64_t)n0 * ldb + 2 * bpair) * 8;
  auto bsrc = [&](int q, int k0) {
    return bbase + ((int64_t)min(8 * (wv + 4 * q) + (lane >> 3), ln - 1) * ldb + k0) * 8;
  };
  // A: k-row wv + 4q of the slice; by LDS-DMA the row pair min(2 lane, lm - 2), +1
  const bool a_dma = lm == HBM_ || !(lm & 1);
  const char* abase = reinterpret_cast<const char*>(t.A) + ((int64_t)wv * lda + m0) * 8;
  const uint32_t a_pair = (uint32_t)max(min(2 * lane, lm - 2), 0) * 8u;
  const uint32_t a_x = (uint32_t)min(2 * lane, lm - 1) * 8u, a_y = (uint32_t)min(2 * lane + 1, lm - 1) * 8u;
  auto issue = [&](int k0, int buf) {   // one full slice (k0 + 16 <= K)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (a_dma) glds16(abase + ((int64_t)(k0 + 4 * q) * lda) * 8 + a_pair, &S.A[buf][wv + 4 * q][0]);
      if (q < BQ) glds16(bsrc(q, k0), &S.B[buf][8 * (wv + 4 * q)][0]);
    }
  };
  auto tail_b = [&](int k0, int buf) {   // partial slice: guarded register loads, zero fill
#pragma unroll
    for (int q = 0; q < BQ; ++q) {
      const gdbl* bp = gbl(reinterpret_cast<const double*>(bsrc(q, k0)));
      const int kb = k0 + 2 * bpair;
      v2d b;
      b.x = kb < K ? bp[0] : 0.0;
      b.y = kb + 1 < K ? bp[1] : 0.0;
      *reinterpret_cast<v2d*>(&S.B[buf][8 * (wv + 4 * q)][2 * lane]) = b;
    }
  };
  v2d areg[4];
  auto load_a = [&](int k0) {   // A through registers: clamped rows, zero beyond K
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const char* p = abase + ((int64_t)(k0 + 4 * q) * lda) * 8;
      if (k0 + wv + 4 * q < K) areg[q] = v2d{*(const gdbl*)(p + a_x), *(const gdbl*)(p + a_y)};
      else areg[q] = v2d{0.0, 0.0};
    }
  };
  auto store_a = [&](int buf) {
#pragma unroll
    for (int q = 0; q < 4; ++q) *reinterpret_cast<v2d*>(&S.A[buf][wv + 4 * q][2 * lane]) = areg[q];
  };
  // fragments as in the interior, at this layout's wave origin
  const int a_off = (lk * HBM_ + wr + 2 * li);
  int b_off[4];
#pragma unroll
  for (int kq = 0; kq < 4; ++kq) b_off[kq] = (wc + li) * HBK_ + (((2 * kq + (lk >> 1)) ^ (li >> 1)) << 1) + (lk & 1);
  auto frags = [&](int cur, int kq, v2d (&fa)[NIP], double (&fb)[NJ]) {
    const double* As = &S.A[cur][0][0] + a_off + kq * 4 * HBM_;
    const double* Bs = &S.B[cur][0][0] + b_off[kq];
#pragma unroll
    for (int ip = 0; ip < NIP; ++ip) fa[ip] = *reinterpret_cast<const v2d*>(As + 32 * ip);
#pragma unroll
    for (int j = 0; j < NJ; ++j) fb[j] = Bs[16 * HBK_ * j];
  };
  auto quad = [&](const v2d (&fa)[NIP], const double (&fb)[NJ]) {
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      if (j < njl) {
#pragma unroll
        for (int ip = 0; ip < NIP; ++ip)
          if (ip < nipl) {   // neg:[1,0,0]: C - B*A
            acc[2 * ip][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fb[j], fa[ip].x, acc[2 * ip][j], 0, 0, 1);
            acc[2 * ip + 1][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fb[j], fa[ip].y, acc[2 * ip + 1][j], 0, 0, 1);
          }
      }
  };
  auto slice = [&](int cur) {
    v2d fa0[NIP], fa1[NIP];
    double fb0[NJ], fb1[NJ];
    frags(cur, 0, fa0, fb0);
    frags(cur, 1, fa1, fb1);
    quad(fa0, fb0);
    frags(cur, 2, fa0, fb0);
    quad(fa1, fb1);
    frags(cur, 3, fa1, fb1);
    quad(fa0, fb0);
    quad(fa1, fb1);
  };
  const int nk = (K + HBK_ - 1) / HBK_;
  const int nfull = K / HBK_;
  if (nfull > 0) issue(0, 0);
  else tail_b(0, 0);
  if (!(a_dma && nfull > 0)) {
    load_a(0);
    store_a(0);
  }
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    const bool next = kt + 1 < nk;
    const bool next_full = kt + 1 < nfull;
    const bool a_regs = next && !(a_dma && next_full);
    if (next_full) issue((kt + 1) * HBK_, cur ^ 1);
    if (next && !next_full) tail_b((kt + 1) * HBK_, cur ^ 1);
    if (a_regs) load_a((kt + 1) * HBK_);   // in flight during this slice's MFMAs
    if (live) slice(cur);
    if (a_regs) store_a(cur ^ 1);
    if (next) __syncthreads();
  }
  double gmax = 0.0;
#pragma unroll
  for (int ip = 0; ip < NIP; ++ip)
    if (ip < nipl) {
      const int rl = wr + 32 * ip + 2 * li;
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        if (j < njl) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int cl = wc + 16 * j + lk + 4 * r;
            const uint32_t off = ((uint32_t)cl * ldc + (uint32_t)rl) * 8u;
            const double x = acc[2 * ip][j][r], y = acc[2 * ip + 1][j][r];
            if (cl < ln && rl + 1 < lm) {
              stu2(cb, off, v2d{x, y});
              if (TRSM) gmax = fmax(gmax, fmax(fabs(x), fabs(y)));
            } else if (cl < ln && rl < lm) {
              *(gdbl*)(cb + off) = x;
              if (TRSM) gmax = fmax(gmax, fabs(x));
            }
          }
        }
    }
  if (TRSM && t.gsid >= 0) tile_growth(ga, t.gsid, gmax);
}

#ifdef SMLU_CLOCK_PROBE
// Dev build only (tools/gemm_clock.py): the shader clock the 128 tile runs at, from the
// workgroup's own counters -- sum of delta s_memtime (shader cycles) and of delta s_memrealtime
// (100 MHz constant clock) over every workgroup of the armed launches, per form (EB = F22, else
// trailing/in-block), accumulated by vector atomics from lane 0.
struct ClockMark {
  unsigned long long t0, r0;
  __device__ __forceinline__ ClockMark() : t0(__builtin_amdgcn_s_memtime()), r0(__builtin_amdgcn_s_memrealtime()) {}
  __device__ __forceinline__ void done(int form) const {
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    unsigned long long* p = g_clock_probe;
    if (p && threadIdx.x == 0) {
      atomicAdd(p + 4 * form, t1 - t0);
      atomicAdd(p + 4 * form + 1, r1 - r0);
      atomicAdd(p + 4 * form + 2, 1ull);
    }
  }
};
#endif
template <bool TRSM, bool EB = false, bool GATHER = false>
__global__ __launch_bounds__(256, 2) void k_gemm128_mfma3(const GemmTask* __restrict__ tasks, int ntask,
                                                          GrowthArgs ga, GatherArgs gx) {
#ifdef SMLU_CLOCK_PROBE
  const ClockMark mark;
#endif
  __shared__ __attribute__((aligned(16))) double lds[sizeof(Mfma3Lds) / sizeof(double)];
  const int64_t b = xcd_window_remap(blockIdx.x, gridDim.x);
  const int ti = find_gemm_task(tasks, ntask, b);
  const GemmTask t = tasks[ti];
  F22Tile fg{nullptr, nullptr, nullptr, -1};
  if (GATHER) {
    const F22Gather g = gx.tg[ti];
    fg = F22Tile{gx.ch + g.beg, gx.inv, gx.scratch, g.cnt};
  }
  int tm, tn;
  tile_rc<HBM_>(t, b - t.tile0, tm, tn);
  const int m0 = tm * HBM_, n0 = tn * HBM_;
  if (m0 + HBM_ <= t.m && n0 + HBM_ <= t.n) {
    gemm128_mfma3_interior<TRSM, EB, GATHER>(t, m0, n0, *reinterpret_cast<Mfma3Lds*>(lds), ga, fg);
  } else {
    // edge tile: the wave layout follows the live extents (uniform per workgroup)
    Mfma3Lds& S = *reinterpret_cast<Mfma3Lds*>(lds);
    const int lm = min(HBM_, t.m - m0), ln = min(HBM_, t.n - n0);
    if (lm > 64 && ln > 64) gemm128_mfma3_edge<TRSM, GATHER, 0>(t, m0, n0, lm, ln, S, ga, fg);
    else if (lm > 64) gemm128_mfma3_edge<TRSM, GATHER, 1>(t, m0, n0, lm, ln, S, ga, fg);
    else if (ln > 64) gemm128_mfma3_edge<TRSM, GATHER, 2>(t, m0, n0, lm, ln, S, ga, fg);
    else gemm128_mfma3_edge<TRSM, GATHER, 3>(t, m0, n0, lm, ln, S, ga, fg);
  }
#ifdef SMLU_CLOCK_PROBE
  mark.done(EB ? 0 : 1);
#endif
}

// ------------------------------------------------------------------------------------
// U rows of an outer block, fused (the end-of-block step of the GEMM-form fronts).  One
// 256-thread workgroup per 32-column block of the columns right of the block (L-panel columns or
// U12 columns) runs the whole sub-panel sequence on its columns with the block REGISTER-RESIDENT:
// the OB rows [ob0, ob1) x 32 columns (up to 384 x 32) are loaded once -- wave wv holds the 16-row
// blocks wv, wv + 4, ..., so sub-panel u's four row blocks are one per wave -- and for each 64-row
// sub-panel u:
//   T: C_u <- C_u - NL_u C_u (NL_u = I - L_uu^-1, tinv slot0 + u): the owner waves publish -C_u
//      in LDS, apply the MFMA GEMM form in their registers, publish the new -C_u;
//   R: every wave updates its row blocks below u inside the block, C_r -= L_ru C_u (k = 64), L
//      fragments straight from HBM/L2 (the next block's in flight during the current one's MFMAs).
// The block is stored once at the end: one HBM round trip per column block instead of one per
// sub-panel (round 4 re-loaded and re-stored the rows below u for every u, a latency chain of
// ~115 us per workgroup).  Per element the same operations in the same order as the per-sub-panel
// launches it replaces (acc = C, then one fp64 MFMA-FMA per k ascending with -C_u as the first
// operand), so the factors are bitwise unchanged.
// ------------------------------------------------------------------------------------
#define UR_NC 32    // columns per workgroup
#define UR_RB 6     // 16-row blocks per wave (OB <= 384 = 4 waves x 6 x 16)
#define UR_LD 36    // LDS row stride of -C_u [k][col] (doubles)
__global__ __launch_bounds__(256, 2) void k_urows(const URowTask* __restrict__ tasks, const SNode* __restrict__ sn,
                                                  double* __restrict__ store, const double* __restrict__ tinv) {
  __shared__ double Bs[64 * UR_LD];
  const URowTask t = tasks[blockIdx.x];
  const SNode s = sn[t.s];
  const int64_t M = (int64_t)s.ns + s.nu;
  const int64_t ld = t.ld;
  const int nc = t.ncols;                 // <= 32
  const int nrows = t.ob1 - t.ob0;        // <= 384
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  gdbl* const C = gbl(store + t.coff);   // (row, col) at col * ld + row
  const gdbl* const Lp = gbl(store + s.Loff);
  // this lane's element r of block (i, cb): row ob0 + 16 (wv + 4 i) + li, column 16 cb + lk + 4 r
  v4d acc[UR_RB][2];
#pragma unroll
  for (int i = 0; i < UR_RB; ++i) {
    const int lr = 16 * (wv + 4 * i) + li;
    const bool rin = lr < nrows;
    const int row = t.ob0 + (rin ? lr : 0);
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int col = 16 * cb + lk + 4 * r;
        const bool in = rin && col < nc;
        acc[i][cb][r] = sel0(in, C[(int64_t)(in ? col : 0) * ld + row]);
      }
  }
  // -C_u of this wave's block i into the LDS image [k = row within the sub-panel][col]
  auto publish = [&](int i) {
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
      for (int r = 0; r < 4; ++r) Bs[(16 * wv + li) * UR_LD + 16 * cb + lk + 4 * r] = -acc[i][cb][r];
  };
  const int nsub = (nrows + 63) >> 6;
#pragma unroll 1
  for (int u = 0; u < nsub; ++u) {
    const int kbu = t.ob0 + 64 * u;
    const int wu = min(64, t.ob1 - kbu);
    const int nkq = (wu + 3) >> 2;
    // ---- T: the four row blocks of sub-panel u are block i = u of each wave
    v4d tc[2];
#pragma unroll
    for (int i = 0; i < UR_RB; ++i)
      if (i == u) {
        publish(i);
        tc[0] = acc[i][0];
        tc[1] = acc[i][1];
      }
    // the wave's NL fragments (rows 16 wv + li of NL_u), all 16 k-quads in flight
    double na[16];
    {
      const gdbl* pn = gbl(tinv + (int64_t)(t.slot0 + u) * 8192) + lk * 64 + 16 * wv + li;
#pragma unroll
      for (int kq = 0; kq < 16; ++kq) na[kq] = sel0(16 * wv + li < wu && 4 * kq + lk < wu, pn[256 * kq]);
    }
    __syncthreads();   // -C_u published
#pragma unroll
    for (int kq = 0; kq < 16; ++kq) {
      if (kq >= nkq) continue;
      const int k = 4 * kq + lk;
#pragma unroll
      for (int cb = 0; cb < 2; ++cb)
        tc[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(Bs[k * UR_LD + 16 * cb + li], na[kq], tc[cb], 0, 0, 0);
    }
    __syncthreads();   // every wave is done reading the old -C_u
#pragma unroll
    for (int i = 0; i < UR_RB; ++i)
      if (i == u) {
        acc[i][0] = tc[0];
        acc[i][1] = tc[1];
        publish(i);
      }
    __syncthreads();   // new -C_u published
    // ---- R: this wave's row blocks below sub-panel u (blocks i > u), C_r -= L_ru C_u
    double fa[16], fn[16];
    auto lfrag = [&](int i, double (&f)[16]) {
      const int lr = 16 * (wv + 4 * i) + li;
      const bool rin = lr < nrows;
      const gdbl* pa = Lp + (int64_t)(kbu + lk) * M + t.ob0 + (rin ? lr : 0);
#pragma unroll
      for (int kq = 0; kq < 16; ++kq) {
        const bool kin = 4 * kq + lk < wu;
        f[kq] = sel0(rin && kin, pa[kin ? (int64_t)4 * kq * M : 0]);
      }
    };
    if (u + 1 < UR_RB && 16 * (wv + 4 * (u + 1)) < nrows) lfrag(u + 1, fa);
#pragma unroll
    for (int i = 1; i < UR_RB; ++i) {
      if (i <= u || 16 * (wv + 4 * i) >= nrows) continue;
      const bool more = i + 1 < UR_RB && 16 * (wv + 4 * (i + 1)) < nrows;
      if (more) lfrag(i + 1, fn);
#pragma unroll
      for (int kq = 0; kq < 16; ++kq) {
        if (kq >= nkq) continue;
        const int k = 4 * kq + lk;
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
          acc[i][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(Bs[k * UR_LD + 16 * cb + li], fa[kq], acc[i][cb], 0, 0, 0);
      }
      if (more)
#pragma unroll
        for (int kq = 0; kq < 16; ++kq) fa[kq] = fn[kq];
    }
    __syncthreads();   // Bs free for the next sub-panel
  }
#pragma unroll
  for (int i = 0; i < UR_RB; ++i) {
    const int lr = 16 * (wv + 4 * i) + li;
    if (16 * (wv + 4 * i) >= nrows) continue;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int col = 16 * cb + lk + 4 * r;
        if (lr < nrows && col < nc) C[(int64_t)col * ld + t.ob0 + lr] = acc[i][cb][r];
      }
  }
}

// ------------------------------------------------------------------------------------
// Inverses of a factored 64 x 64 diagonal tile for the GEMM-form triangular solves:
//   NL = I - L_kk^{-1} (L unit lower: the strictly lower part of the tile),
//   NU = I - U_kk^{-1} (U upper with its diagonal),
// column-major with ld 64 at tinv + slot * 8192 (NL) and + 4096 (NU).  A partial panel
// (w < 64) is padded with the identity, so NL/NU vanish outside the w x w block.
// 8 workgroups per front (4 for NL, 4 for NU); a wave computes 4 columns at once by column
// sweep: lane i holds row i, step j broadcasts the finished entry j by v_readlane and every
// lane below (L) / above (U) subtracts its tile entry times it -- one LDS read feeds 4 FMAs.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tri_inv(const int32_t* __restrict__ list, int step,
                                                 const SNode* __restrict__ sn,
                                                 double* __restrict__ store,
                                                 double* __restrict__ scratch,
                                                 double* __restrict__ tinv) {
  __shared__ double sD[64 * 65];   // tile [col][row], ld 65
  const int item = blockIdx.x >> 3, part = blockIdx.x & 7;
  const int sid = list[2 * item];
  const int64_t slot = list[2 * item + 1];
  const SNode s = sn[sid];
  FrontPtrs f = front_ptrs(s, store, scratch);
  const int64_t M = f.M;
  const int kb = step * s.nb;
  const int w = min(s.nb, (int)f.ns - kb);
  const gdbl* D = f.L + (int64_t)kb * M + kb;
  {
    double v[16];   // all 16 loads in flight before the LDS stores
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int idx = threadIdx.x + 256 * u, i = idx & 63, j = idx >> 6;
      v[u] = (i < w && j < w) ? D[(int64_t)j * M + i] : (i == j ? 1.0 : 0.0);
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int idx = threadIdx.x + 256 * u, i = idx & 63, j = idx >> 6;
      sD[j * 65 + i] = v[u];
    }
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const bool upper = part >= 4;
  const int c0 = ((part & 3) * 4 + wv) * 4;   // this wave's columns c0 .. c0+3
  double z[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) z[r] = lane == c0 + r ? 1.0 : 0.0;
  double* out = tinv + slot * 8192 + (upper ? 4096 : 0);
  if (!upper) {
    // L z = e_c: z_j is final at step j; rows i > j subtract L[i][j] z_j
#pragma unroll 4
    for (int j = 0; j < 63; ++j) {
      const double lij = sD[j * 65 + lane];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double zj = readlane_f64(z[r], j);
        if (lane > j) z[r] = fma(-lij, zj, z[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) out[(int64_t)(c0 + r) * 64 + lane] = lane > c0 + r ? -z[r] : 0.0;
  } else {
    // U y = e_c: y_j is final at step j after its division; rows i < j subtract U[i][j] y_j
    const double rd = recip(sD[lane * 65 + lane]);
#pragma unroll 4
    for (int j = 63; j >= 0; --j) {
      const double uij = sD[j * 65 + lane];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (lane == j) z[r] *= rd;
        const double yj = readlane_f64(z[r], j);
        if (lane < j) z[r] = fma(-uij, yj, z[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = c0 + r;
      out[(int64_t)c * 64 + lane] = lane == c ? 1.0 - z[r] : (lane < c ? -z[r] : 0.0);
    }
  }
}

#ifdef SMLU_CLOCK_PROBE
// arm != 0: zero the counters and arm the probe; arm == 0: copy the 24 counters out (8 clock sums,
// then 8 K-loop stamp sums per form) and disarm
extern "C" int smlu_dev_gemm_clock(int arm, unsigned long long* out) {
  static unsigned long long* buf = nullptr;
  if (!buf && hipMalloc(&buf, 24 * sizeof(unsigned long long)) != hipSuccess) return -1;
  unsigned long long* p = nullptr;
  if (arm) {
    if (hipMemset(buf, 0, 24 * sizeof(unsigned long long)) != hipSuccess) return -1;
    p = buf;
  } else {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (out && hipMemcpy(out, buf, 24 * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  }
  return hipMemcpyToSymbol(HIP_SYMBOL(g_clock_probe), &p, sizeof p) == hipSuccess ? 0 : -1;
}
#endif

// ------------------------------------------------------------------------------------
// Host-side launch wrappers (called from smlu.cpp)
// ------------------------------------------------------------------------------------
hipError_t launch_gemm_g(hipStream_t st, int64_t ntiles, const GemmTask* tasks, int ntask, int tile,
                         int64_t maxwg, int32_t* info, double* growth, double piv_tol) {
  if (ntiles <= 0) return hipSuccess;
  const GrowthArgs ga{info, growth, piv_tol};
  const GatherArgs gx{nullptr, nullptr, nullptr, nullptr};
  const bool trsm = info != nullptr;
  if (tile == 143) return hipErrorInvalidValue;   // the gathering F22 tile: launch_gemm_gather
  if (tile == 135 && trsm) k_gemm128_mfma3<true, true><<<(unsigned)ntiles, 256, 0, st>>>(tasks, ntask, ga, gx);
  else if (tile == 135) k_gemm128_mfma3<false, true><<<(unsigned)ntiles, 256, 0, st>>>(tasks, ntask, ga, gx);
  else if (tile == 131 && trsm) k_gemm128_mfma3<true><<<(unsigned)ntiles, 256, 0, st>>>(tasks, ntask, ga, gx);
  else if (tile == 131) k_gemm128_mfma3<false><<<(unsigned)ntiles, 256, 0, st>>>(tasks, ntask, ga, gx);
  else if (tile == 65 && trsm) k_gemm_k64<true><<<(unsigned)ntiles, 256, 0, st>>>(tasks, ntask, ga);
  else if (tile == 65) k_gemm_k64<false><<<(unsigned)ntiles, 256, 0, st>>>(tasks, ntask, ga);
  else if (tile == 66 && trsm) k_gemm64_mfma<true><<<(unsigned)ntiles, 256, 0, st>>>(tasks, ntask, ga);
  else if (tile == 66) k_gemm64_mfma<false><<<(unsigned)ntiles, 256, 0, st>>>(tasks, ntask, ga);
  else if (trsm) k_gemm<true><<<(unsigned)ntiles, 256, 0, st>>>(tasks, ntask, ga);
  else k_gemm<false><<<(unsigned)ntiles, 256, 0, st>>>(tasks, ntask, ga);
  return hipGetLastError();
}
hipError_t launch_gemm(hipStream_t st, int64_t ntiles, const GemmTask* tasks, int ntask, int tile,
                       int64_t maxwg) {
  return launch_gemm_g(st, ntiles, tasks, ntask, tile, maxwg, nullptr, nullptr, 1.0);
}
// an F22 launch of tile code 143: task i of the launch has its gather record at tg[i]
hipError_t launch_gemm_gather(hipStream_t st, int64_t ntiles, const GemmTask* tasks, int ntask, const F22Gather* tg,
                              const F22Child* ch, const int32_t* inv, const double* scratch) {
  if (ntiles <= 0) return hipSuccess;
  if (!tg || !scratch) return hipErrorInvalidValue;   // (ch, inv: empty when no gathered front has children)
  const GrowthArgs ga{nullptr, nullptr, 1.0};
  const GatherArgs gx{tg, ch, inv, scratch};
  k_gemm128_mfma3<false, true, true><<<(unsigned)ntiles, 256, 0, st>>>(tasks, ntask, ga, gx);
  return hipGetLastError();
}
hipError_t launch_urows(hipStream_t st, int cnt, const URowTask* tasks, const SNode* sn, double* store,
                        const double* tinv) {
  if (cnt <= 0) return hipSuccess;
  k_urows<<<(unsigned)cnt, 256, 0, st>>>(tasks, sn, store, tinv);   // OB <= 384 (QMAX): checked by the caller
  return hipGetLastError();
}
hipError_t launch_tri_inv(hipStream_t st, int cnt, int step, const int32_t* list, const SNode* sn,
                          double* store, double* scratch, double* tinv) {
  if (cnt <= 0) return hipSuccess;
  k_tri_inv<<<(unsigned)cnt * 8, 256, 0, st>>>(list, step, sn, store, scratch, tinv);
  return hipGetLastError();
}

}  // namespace smlu
