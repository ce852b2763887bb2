// kernels_solve_t.hpp — device helpers shared by the single-vector transposed-solve kernels
// (kernels_solve_t.hip) and their batched variants (kernels_solve_tb.hip): the 16-lane dot products,
// the fixed reduction trees and the LDS staging of the diagonal blocks.  A column of a batched solve
// goes through the same helpers in the same order, so it is bitwise the single-vector result.
#pragma once
#include "kernels_common.hpp"

namespace smlu {

// ---- dot products over contiguous runs: 16 lanes per run ------------------------------------
// a[u] += sum over idx = e, e + 16, ... < len of ptr[u][idx] * xv[idx] (e = lane within the group):
// four strides of 16 per round, the loads of a round issued before its fmas.
template <int U>
__device__ __forceinline__ void dots16(const double* const (&ptr)[U], const bool (&ok)[U], const double* xv,
                                       int64_t len, int e, double (&a)[U]) {
  for (int64_t i0 = 0; i0 < len; i0 += 64) {
    double d[U][4], xx[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t idx = i0 + e + 16 * k;
      xx[k] = idx < len ? xv[idx] : 0.0;
#pragma unroll
      for (int u = 0; u < U; ++u) d[u][k] = (ok[u] && idx < len) ? ptr[u][idx] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int u = 0; u < U; ++u) a[u] = fma(d[u][k], xx[k], a[u]);
  }
}
// sum over the 16 lanes of a group (every lane of the wave takes part), the same tree on every call
__device__ __forceinline__ double red16(double a) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
  return a;
}

// Sixteen sums at once: lane e of a group holds partial sums a[0..15] of sixteen targets and leaves
// with the group's total of target e (recursive halving: 8 + 4 + 2 + 1 exchanges instead of 16 x 4,
// the additions of every target in the same fixed order on every call).
__device__ __forceinline__ double red16x16(double (&a)[16], int e) {
#pragma unroll
  for (int h = 8; h > 0; h >>= 1) {
    const bool up = (e & h) != 0;
#pragma unroll
    for (int i = 0; i < h; ++i) {
      const double send = up ? a[i] : a[i + h];
      const double keep = up ? a[i + h] : a[i];
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

// batched launchers (kernels_solve_tb.hip), called by the launchers of kernels_solve_t.hip for rh.n > 1
hipError_t launch_ut_tiny_b(hipStream_t, int, const int32_t*, const SNode*, const int32_t*, const int32_t*,
                            const double*, double*, double*, Rhs, int);
hipError_t launch_lt_tiny_b(hipStream_t, int, const int32_t*, const SNode*, const int32_t*, const int32_t*,
                            const double*, double*, Rhs, int);
hipError_t launch_ut_front_b(hipStream_t, int, const int32_t*, const SNode*, const int32_t*, const int32_t*,
                             const double*, double*, double*, Rhs);
hipError_t launch_lt_front_b(hipStream_t, int, const int32_t*, const SNode*, const int32_t*, const int32_t*,
                             const double*, double*, double*, Rhs);
hipError_t launch_pull_tb(hipStream_t, int64_t, const FrontTile*, int, const SNode*, const int32_t*, const int32_t*,
                          const double*, double*, Rhs);
hipError_t launch_tri_tb(hipStream_t, bool, int64_t, const FrontTile*, int, int, const SNode*, const int32_t*,
                         const double*, double*, double*, Rhs);
hipError_t launch_bwdu_tb(hipStream_t, int64_t, const FrontTile*, int, const SNode*, const int32_t*, const double*,
                          const double*, double*, Rhs);
hipError_t launch_perm_in_tb(hipStream_t, int64_t, const int64_t*, const double*, int64_t, double*, int, Rhs);
hipError_t launch_perm_out_tb(hipStream_t, int64_t, const int64_t*, const double*, const double*, double*, int64_t,
                              int, Rhs);

}  // namespace smlu
