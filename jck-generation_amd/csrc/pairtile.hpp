// The Gram-tile geometry and staging shared by the pairwise units (pairstat.hip, knnindex.hip): a 64 x 64 tile per 256-thread
// workgroup, c in steps of 16 through LDS rows of 20 floats ((20 m + k) % 64 is conflict-free for the fragment reads of
// v_mfma_f32_16x16x4_f32).  Each unit keeps its own kernels; this header holds only what they must agree on.
#pragma once
#include "ops_internal.hpp"

namespace {

constexpr int PT = 64, PK = 16, PLD = 20, PKMAX = 8;
constexpr int P_MAX_ROWS = 1 << 30;

__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// rows r0 .. r0+63, columns k0 .. k0+15 of p[R][D] into S[row][k]; zero outside the matrix
__device__ __forceinline__ void stage_tile(float (*S)[PLD], const float* __restrict__ p, int R, int D, int r0, int k0, int vec, int tid) {
  if (vec) {
    const int row = tid >> 2, kq = (tid & 3) * 4, gr = r0 + row, c = k0 + kq;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (gr < R && c < D) v = *reinterpret_cast<const f32x4*>(p + (long long)gr * D + c);      // D % 4 == 0: c + 3 < D
    *reinterpret_cast<f32x4*>(&S[row][kq]) = v;
  } else {
    const int k = tid & 15, c = k0 + k;
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
      const int row = (tid >> 4) + 16 * ps, gr = r0 + row;
      S[row][k] = (gr < R && c < D) ? p[(long long)gr * D + c] : 0.f;
    }
  }
}

inline long long tiles_of(int n) { return ((long long)n + PT - 1) / PT; }
// 16-byte staging needs whole float4s in every row and both bases on a 16-byte boundary
inline int vec_ok(const float* a, const float* b, int D) { return D % 4 == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0; }

}  // namespace
