// The Gram-tile core of the pairwise units (pairstat.hip, knnindex.hip); each unit keeps only its epilogues.
//
// G[i][j] = sum_c a[i][c] * b[j][c] on the exact-fp32 MFMA (v_mfma_f32_16x16x4_f32, bitwise an fmaf chain - the convolutions of
// infer.hip use it for the same reason), 64 x 64 per 256-thread workgroup, each wave a 32 x 32 quarter as 2 x 2 accumulator
// fragments, c in steps of 16 through LDS rows of 20 floats ((20 m + k) % 64 is conflict-free for the fragment reads).  Rows past
// the matrix and columns past D are zero-filled; D % 4 != 0 or a base pointer off a 16-byte boundary stages with scalar loads
// instead of 16-byte ones.  A workgroup owns one 64-row block of `b` (the tile's columns) and walks 64-row tiles of `a` (the tile's
// rows): a lane then holds, per accumulator fragment, ONE column and four rows, so per-column state (the k smallest, a hit flag) is
// two columns per lane, and 8 lanes (4 per wave, 2 waves) share a column.  Squared row norms are an fp32 fmaf chain over c in
// order, taken from the staged tiles: the block's own once, a walked tile's when it passes.  The units form
// d^2 = max(0, (|a|^2 + |b|^2) - 2 G) in fp32, in that association.
//
//   TilePos      where a thread sits in the tile: the C/D layout of the MFMA is written down here and nowhere else
//   gram_tile    one 64 x 64 tile of G over all of D, with the norms
//   TopK         the PKMAX smallest values seen, ascending, with their indices where ties must go to the lower one
//   merge_columns  the lists of the 8 lanes that share a column become that column's list
#pragma once
#include "ops_internal.hpp"

namespace {

constexpr int PT = 64, PK = 16, PLD = 20, PKMAX = 8;
constexpr int P_MAX_ROWS = 1 << 30;
constexpr int P_IPAD = 0x7fffffff;        // index of a list's padding entry (value +inf): sorts after every real entry

__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ float qnan_f() { return __uint_as_float(0x7fc00000u); }

struct TilePos {
  int tid, lane, wave, wm, wn;                                          // wm, wn: this wave's 32 x 32 part of the tile
  __device__ __forceinline__ explicit TilePos(int t) : tid(t), lane(t & 63), wave(t >> 6), wm((wave >> 1) * 32), wn((wave & 1) * 32) {}
  // C/D of v_mfma_f32_16x16x4_f32, fragment (i, j), register r: row (a) = 4*(l>>4) + r, col (b) = l & 15
  __device__ __forceinline__ int row(int i, int r) const { return wm + i * 16 + (lane >> 4) * 4 + r; }
  __device__ __forceinline__ int col(int j) const { return wn + j * 16 + (lane & 15); }
  __device__ __forceinline__ int share() const { return (wave >> 1) * 4 + (lane >> 4); }   // 0..7 among the lanes that hold col(j)
};

// rows r0 .. r0+63, columns k0 .. k0+15 of p[R][D] into S[row][k] by scalar loads; zero outside the matrix
__device__ __forceinline__ void stage_tile(float (*S)[PLD], const float* __restrict__ p, int R, int D, int r0, int k0, int tid) {
  const int k = tid & 15, c = k0 + k;
#pragma unroll
  for (int ps = 0; ps < 4; ++ps) {
    const int row = (tid >> 4) + 16 * ps, gr = r0 + row;
    S[row][k] = (gr < R && c < D) ? p[(long long)gr * D + c] : 0.f;
  }
}

// the same tile by 16-byte loads: this thread's float4, zero outside the matrix.  The load itself is unconditional (from p when
// outside: D % 4 == 0 makes p[0..3] readable), so that several can be in flight.  The choice is between the two addresses, not
// between two offsets: that form costs pair_kernel<poly3> four VGPRs less, which is a wave per SIMD there.
__device__ __forceinline__ f32x4 load_tile_vec(const float* __restrict__ p, int R, int D, int r0, int k0, int tid) {
  const int gr = r0 + (tid >> 2), c = k0 + (tid & 3) * 4;
  const bool in = gr < R && c < D;
  const float* g = p + ((long long)gr * D + c);
  const f32x4 v = *reinterpret_cast<const f32x4*>(in ? g : p);
  return in ? v : f32x4{0.f, 0.f, 0.f, 0.f};
}

// acc = the tile of G at rows a0 .. a0+63 of a[Ra][D] (walked) and rows b0 .. b0+63 of b[Rb][D] (the workgroup's own block), KSUB
// 16-column steps staged per barrier pair into As[KSUB] / Bs[KSUB].  With NORMS, wave 0 leaves the walked rows' squared norms in nA
// and, on the workgroup's first tile, wave 1 the own block's in nB; the caller's barrier publishes them.  TilePos travels by value:
// by reference the allocator gives knn_cand_kernel 156 VGPRs instead of 150, which is 2 waves per SIMD instead of 3.
template <int KSUB, bool NORMS>
__device__ __forceinline__ void gram_tile(f32x4 (&acc)[2][2], float (*As)[PT][PLD], float (*Bs)[PT][PLD], float* nA, float* nB,
                                          const float* a, int Ra, int a0, const float* b, int Rb, int b0, int D, int vec, bool first,
                                          const TilePos t) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float nrm = 0.f;
  for (int k0 = 0; k0 < D; k0 += KSUB * PK) {
    if (vec) {                                                          // every load of the KSUB steps leaves before the first store waits
      f32x4 ra[KSUB], rb[KSUB];
#pragma unroll
      for (int s = 0; s < KSUB; ++s) {
        ra[s] = load_tile_vec(a, Ra, D, a0, k0 + s * PK, t.tid);
        rb[s] = load_tile_vec(b, Rb, D, b0, k0 + s * PK, t.tid);
      }
#pragma unroll
      for (int s = 0; s < KSUB; ++s) {
        *reinterpret_cast<f32x4*>(&As[s][t.tid >> 2][(t.tid & 3) * 4]) = ra[s];
        *reinterpret_cast<f32x4*>(&Bs[s][t.tid >> 2][(t.tid & 3) * 4]) = rb[s];
      }
    } else {
#pragma unroll
      for (int s = 0; s < KSUB; ++s)
        if (k0 + s * PK < D) {
          stage_tile(As[s], a, Ra, D, a0, k0 + s * PK, t.tid);
          stage_tile(Bs[s], b, Rb, D, b0, k0 + s * PK, t.tid);
        }
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < KSUB; ++s)
      if (k0 + s * PK < D) {
        if (NORMS) {
          if (t.wave == 0) {
#pragma unroll
            for (int k = 0; k < PK; ++k) { const float v = As[s][t.lane][k]; nrm = fmaf(v, v, nrm); }
          } else if (t.wave == 1 && first) {
#pragma unroll
            for (int k = 0; k < PK; ++k) { const float v = Bs[s][t.lane][k]; nrm = fmaf(v, v, nrm); }
          }
        }
#pragma unroll
        for (int kk = 0; kk < PK; kk += 4) {
          // v_mfma_f32_16x16x4_f32: lane l holds A[row l&15][k = l>>4], B[k = l>>4][col l&15]
          float fa[2], fb[2];
#pragma unroll
          for (int i = 0; i < 2; ++i) fa[i] = As[s][t.wm + i * 16 + (t.lane & 15)][kk + (t.lane >> 4)];
#pragma unroll
          for (int j = 0; j < 2; ++j) fb[j] = Bs[s][t.wn + j * 16 + (t.lane & 15)][kk + (t.lane >> 4)];
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
      }
    __syncthreads();
  }
  if (NORMS) {
    if (t.wave == 0) nA[t.lane] = nrm;
    else if (t.wave == 1 && first) nB[t.lane] = nrm;
  }
}

// the PKMAX smallest entries offered, ascending; with IDX by (value, index), so that equal values keep the lower index.  No NaN.
template <bool IDX>
struct TopK {
  float v[PKMAX];
  int i[IDX ? PKMAX : 1];
  static __device__ __forceinline__ bool less(float x, int xi, float e, int ei) { return x < e || (IDX && x == e && xi < ei); }
  __device__ __forceinline__ int idx(int t) const { return IDX ? i[t] : 0; }
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int t = 0; t < PKMAX; ++t) { v[t] = INFINITY; if (IDX) i[t] = P_IPAD; }
  }
  __device__ __forceinline__ void offer(float x, int xi = 0) {
    if (!less(x, xi, v[PKMAX - 1], idx(PKMAX - 1))) return;
#pragma unroll
    for (int t = 0; t < PKMAX; ++t) {
      const bool lt = less(x, xi, v[t], idx(t));
      const float lo = lt ? x : v[t], hi = lt ? v[t] : x;
      const int loi = lt ? xi : idx(t), hii = lt ? idx(t) : xi;
      v[t] = lo; x = hi;
      if (IDX) { i[t] = loi; xi = hii; }
    }
  }
  __device__ __forceinline__ void pop() {                               // the head leaves, a padding entry follows the rest
#pragma unroll
    for (int t = 0; t + 1 < PKMAX; ++t) { v[t] = v[t + 1]; if (IDX) i[t] = i[t + 1]; }
    v[PKMAX - 1] = INFINITY;
    if (IDX) i[PKMAX - 1] = P_IPAD;
  }
};

// L[j] is this lane's list for column t.col(j).  The 8 lanes that share a column hand their lists over through candV / candI
// (PT * 8 * PKMAX entries each, candI only with IDX) and thread c < PT leaves with column c's merged list in M.
template <bool IDX>
__device__ __forceinline__ void merge_columns(TopK<IDX>& M, const TopK<IDX> (&L)[2], float* candV, int* candI, const TilePos t) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int o = (t.col(j) * 8 + t.share()) * PKMAX;
#pragma unroll
    for (int e = 0; e < PKMAX; ++e) {
      candV[o + e] = L[j].v[e];
      if (IDX) candI[o + e] = L[j].i[e];
    }
  }
  __syncthreads();
  if (t.tid < PT) {
    M.clear();
    for (int s = 0; s < 8 * PKMAX; ++s) M.offer(candV[t.tid * 8 * PKMAX + s], IDX ? candI[t.tid * 8 * PKMAX + s] : 0);
  }
}

inline long long tiles_of(int n) { return ((long long)n + PT - 1) / PT; }
// 16-byte staging needs whole float4s in every row and both bases on a 16-byte boundary
inline int vec_ok(const float* a, const float* b, int D) { return D % 4 == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0; }

}  // namespace
