// Sliced Wasserstein distance on Laplacian-pyramid patches: the pyramid and the patch statistics of uint8 pictures, the
// projection of the normalised 7 x 7 x 3 descriptors onto directions, a row-wise key sort and the mean absolute difference of sorted
// rows.  No descriptor reaches HBM, no atomics on floats, every sum in an order fixed by the shape.
//
//   jck_swd_patch_stats_u8   sum / sum of squares per level and channel of the descriptor components of n pictures (fp64)
//   jck_swd_project_u8       proj[l][d][i P + p] = <normalised descriptor (i, p) of level l, dirs[d]>
//   jck_sort_rows_f32        ascending sort of every row of x[Rows][M], any M >= 1
//   jck_swd_rows             w[r] = mean_j |sa[r][j] - sb[r][j]| (fp64)
//   jck_sort_rows_ws_bytes, jck_sort_rows_tile, jck_swd_max_levels   host only
//
// Pyramid arithmetic.  The count for an fp32 separable pyramid (G_l exact up to l = 2 with 8, 16, 24 significant bits,
// up(G_1) 22 bits, Lap_1 = G_1 - up(G_2) 30 bits and therefore rounded, 5 + 5 + 1 roundings of at most 2^-17 each = 11 2^-17 < 2^-13)
// holds (at S = 128 with four levels that route gives 11 2^-17 for Lap_1, 10 2^-17 for the 32-bit G_3 and, with up's weights summing
// to 1, 10 + 5 + 5 + 1 = 21 roundings, 21 2^-17 < 2^-12, for Lap_2), but this unit does not need it: the pyramid is kept in FIXED POINT.  G_l is the integer G_l 2^(8 l) (the binomial weights
// without their divisors: at most 255 2^(8 l) < 2^32 for l <= 3, uint32), up(G_(l+1)) the integer sum of at most 3 x 3 taps with the
// weights {1,6,1} / {4,4} per axis (units 2^-(8 l + 14), below 2^46: uint64), Lap_l = (G_l << 14) - up(G_(l+1)) an int64 below 2^(8 l + 22)
// in magnitude.  All of that is exact in any order.  Each Laplacian value is converted to fp32 ONCE (round to nearest even) and scaled
// by a power of two, so every level of every size - the two middle levels at S = 128 included, whose exact values need 30 and 38 bits -
// is the fp64 value of the definition rounded to fp32, bit for bit: |Lap_fp32 - Lap| <= 2^-17 (half an ulp below 256), 0 at level 0 and
// wherever 24 bits suffice.  The coarsest level is G_(L-1) converted the same way (32 bits at S = 128, L = 4: one rounding).
//
// One workgroup of 256 threads per picture, one channel at a time:
//   planes    G_0 .. G_(L-1) of the channel as uint32 words in LDS, the 5-tap down filter separably through a scratch plane; then from
//             the finest level down each plane is overwritten by its Laplacian as fp32 (the next plane is still integers then).
//   stats     per level the P x 49 components of the channel, a thread's share in ascending order in fp64, a 64-lane xor butterfly,
//             the 4 waves in ascending order -> part[i][l][c][2]; a second launch adds the pictures: thread t the pictures t, t + 256,
//             ... ascending, then a binary tree over the 256 threads.  Every order is fixed by n and P.
//   project   per tile of 128 directions the channel's 49 components of them go to LDS (rows of 132 floats), per level and tile of 64
//             patches the normalised components fmul(fsub(x, mean), rstd) go to LDS as [k][64]; a thread owns 4 patches x 8
//             directions and walks k = 0 .. 48 with one fmaf per product, from zero.  The channel's partial dot product is stored
//             (c = 0) or added to what the same thread stored before (c = 1, 2): proj = (s_0 + s_1) + s_2, s_c a 49-term fmaf chain,
//             contraction off.  |proj - exact| <= 53 2^-24 sum_i |(x_i - mean) rstd d_i| (49 + 2 additions, 2 roundings of the
//             normalisation), the descriptors themselves as above.  Rows come out contiguous: P consecutive floats per row.
//   corners   a corner outside [0, s_l - 7] (checked by the whole workgroup first): that picture's P entries of every row, or its
//             part[] row, are NaN and nothing else of it is written.
// LDS per workgroup (static, by size class; planes + scratch (49 x 132 directions + 49 x 64 components, or the down filter's
// scratch plane) + 64 bytes of wave sums): S = 32: 5 120 + 38 416 + 64 = 43 600 bytes, S = 64: 21 504 + 38 416 + 64 = 59 984 (two
// workgroups per CU), S = 128: 87 040 + 38 416 + 64 = 125 520 (one workgroup per CU); the compiler reports 256 bytes more each, the
// barrier's or-reduction.  All three channels of a 128 x 128 level 0 in fp32 would be 196 KB: hence one channel at a time.
//
// Row sort: keys are the fp32 bit patterns under the sign-flip map (negative: all bits flipped, else the sign bit set), an order
// that is total: -0 < +0, -inf first, +inf after FLT_MAX, NaNs by their bits at the two ends.  Tiles of 2048 keys are sorted in LDS
// by a bitonic network (8 keys a thread: the strides below 8 in registers, the others through LDS), then ceil(log2(tiles)) merge
// passes between `out` and the workspace: a workgroup produces one tile of 2048 merged keys, its two ends found by a merge-path
// search in HBM, the keys merged from LDS by 8 per thread.  Equal keys have equal bits, so the result is the unique sorted row.
// The grid is rows x tiles in every launch.  `out` may equal `x`: a tile is read whole before anything of it is written, and the
// merge passes never read x.
#include "ops_internal.hpp"

namespace {

constexpr int SW_T = 256, SW_W = SW_T / 64, SW_LMAX = 4, SW_K = 49, SW_DESC = 147;
constexpr int SW_PT = 64, SW_DT = 128, SW_DLD = 132;                 // patch tile, direction tile, LDS row of a direction tile
constexpr int SW_SCR = SW_K * SW_DLD + SW_K * SW_PT;                  // words of scratch

struct SwP {
  const unsigned char* img;
  const int* pos;                                                     // [n][L][P][2] = (y, x)
  const float *dirs, *mean, *rstd;
  float* proj;
  double* part;                                                       // [n][L][3][2]
  long long ld;
  int n, S, L, P, D;
};

template <int SMAX> struct SwLds {
  static constexpr int PL = SMAX * SMAX + SMAX * SMAX / 4 + (SMAX >= 64 ? SMAX * SMAX / 16 : 0) + (SMAX >= 128 ? SMAX * SMAX / 64 : 0);
  static constexpr int WORDS = PL + SW_SCR + 16;
  static_assert(SW_SCR >= SMAX * SMAX / 2, "the down filter's scratch plane");
};

__device__ __forceinline__ int sw_level_off(int S, int l) {
  int off = 0;
  for (int j = 0; j < l; ++j) off += (S >> j) * (S >> j);
  return off;
}

// the planes of channel c: Laplacian levels 0 .. L-2 and G_(L-1), fp32, in pl; tmp: S * S / 2 words.  Ends with a barrier.
__device__ __forceinline__ void sw_pyramid(const unsigned char* __restrict__ img, int S, int L, int c, unsigned int* pl, unsigned int* tmp, int tid) {
  for (int i = tid; i < S * S; i += SW_T) pl[i] = img[3 * i + c];
  __syncthreads();
  int off = 0;
  for (int l = 0; l + 1 < L; ++l) {                                   // G_(l+1) = down(G_l), weights 1 4 6 4 1 per axis, mirror borders
    const int s = S >> l, m = s >> 1;
    const unsigned int* g = pl + off;
    unsigned int* gn = pl + off + s * s;
    for (int e = tid; e < s * m; e += SW_T) {
      const int y = e / m, j = e - y * m, x = 2 * j;
      const unsigned int* r = g + y * s;
      const int xm2 = j == 0 ? 2 : x - 2, xm1 = j == 0 ? 1 : x - 1, xp2 = x + 2 >= s ? s - 2 : x + 2;
      tmp[e] = r[xm2] + 4u * r[xm1] + 6u * r[x] + 4u * r[x + 1] + r[xp2];
    }
    __syncthreads();
    for (int e = tid; e < m * m; e += SW_T) {
      const int i = e / m, j = e - i * m, y = 2 * i;
      const int ym2 = i == 0 ? 2 : y - 2, ym1 = i == 0 ? 1 : y - 1, yp2 = y + 2 >= s ? s - 2 : y + 2;
      gn[e] = tmp[ym2 * m + j] + 4u * tmp[ym1 * m + j] + 6u * tmp[y * m + j] + 4u * tmp[(y + 1) * m + j] + tmp[yp2 * m + j];
    }
    __syncthreads();
    off += s * s;
  }
  off = 0;
  for (int l = 0; l + 1 < L; ++l) {                                   // Lap_l = G_l - up(G_(l+1)), in place, finest first
    const int s = S >> l, m = s >> 1;
    unsigned int* g = pl + off;
    const unsigned int* X = pl + off + s * s;
    const float scale = __uint_as_float((unsigned int)(127 - (8 * l + 14)) << 23);                   // 2^-(8 l + 14)
    for (int e = tid; e < s * s; e += SW_T) {
      const int y = e / s, x = e - y * s, i = y >> 1, j = x >> 1;
      const int ry[3] = {i == 0 ? 1 : i - 1, i, i == m - 1 ? m - 1 : i + 1};
      const int rx[3] = {j == 0 ? 1 : j - 1, j, j == m - 1 ? m - 1 : j + 1};
      const bool oy = y & 1, ox = x & 1;
      const unsigned int wy[3] = {oy ? 0u : 1u, oy ? 4u : 6u, oy ? 4u : 1u};
      const unsigned int wx[3] = {ox ? 0u : 1u, ox ? 4u : 6u, ox ? 4u : 1u};
      unsigned long long up = 0;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        unsigned long long rowsum = 0;
#pragma unroll
        for (int b = 0; b < 3; ++b) rowsum += (unsigned long long)wx[b] * X[ry[a] * m + rx[b]];
        up += wy[a] * rowsum;
      }
      const long long lap = (long long)((unsigned long long)g[e] << 14) - (long long)up;
      g[e] = __float_as_uint(__fmul_rn((float)lap, scale));
    }
    __syncthreads();
    off += s * s;
  }
  {
    const int s = S >> (L - 1);
    unsigned int* g = pl + off;
    const float scale = __uint_as_float((unsigned int)(127 - 8 * (L - 1)) << 23);
    for (int e = tid; e < s * s; e += SW_T) g[e] = __float_as_uint(__fmul_rn((float)g[e], scale));
    __syncthreads();
  }
}

// every corner of picture i inside its level?  (uniform over the workgroup)
__device__ __forceinline__ bool sw_corners_ok(const SwP& p, long long i, int tid) {
  int bad = 0;
  for (int e = tid; e < p.L * p.P; e += SW_T) {
    const int l = e / p.P, hi = (p.S >> l) - 7;
    const int y = p.pos[(i * p.L * p.P + e) * 2], x = p.pos[(i * p.L * p.P + e) * 2 + 1];
    bad |= (y < 0) | (x < 0) | (y > hi) | (x > hi);
  }
  return __syncthreads_or(bad) == 0;
}

template <int SMAX> __global__ __launch_bounds__(SW_T) void swd_stats_kernel(const SwP p) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) unsigned int lds[SwLds<SMAX>::WORDS];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long i = blockIdx.x;
  const int S = p.S, L = p.L, P = p.P;
  double* part = p.part + i * (L * 6);
  if (!sw_corners_ok(p, i, tid)) {
    if (tid < L * 6) part[tid] = __longlong_as_double(0x7ff8000000000000ll);
    return;
  }
  unsigned int* scr = lds + SwLds<SMAX>::PL;
  double* red = reinterpret_cast<double*>(lds + SwLds<SMAX>::PL + SW_SCR);                           // [SW_W][2]
  const unsigned char* img = p.img + i * (3ll * S * S);
  for (int c = 0; c < 3; ++c) {
    sw_pyramid(img, S, L, c, lds, scr, tid);
    for (int l = 0; l < L; ++l) {
      const int s = S >> l;
      const float* plane = reinterpret_cast<const float*>(lds + sw_level_off(S, l));
      const int* pos = p.pos + (i * L + l) * (2ll * P);
      double sum = 0.0, sq = 0.0;
      for (int e = tid; e < P * SW_K; e += SW_T) {
        const int q = e / SW_K, k = e - q * SW_K, dy = k / 7, dx = k - dy * 7;
        const double v = (double)plane[(pos[2 * q] + dy) * s + pos[2 * q + 1] + dx];
        sum = __dadd_rn(sum, v);
        sq = __dadd_rn(sq, __dmul_rn(v, v));
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) { sum = __dadd_rn(sum, __shfl_xor(sum, o, 64)); sq = __dadd_rn(sq, __shfl_xor(sq, o, 64)); }
      if (lane == 0) { red[2 * wave] = sum; red[2 * wave + 1] = sq; }
      __syncthreads();
      if (tid == 0) {
        double a = red[0], b = red[1];
#pragma unroll
        for (int w = 1; w < SW_W; ++w) { a = __dadd_rn(a, red[2 * w]); b = __dadd_rn(b, red[2 * w + 1]); }
        part[(l * 3 + c) * 2] = a;
        part[(l * 3 + c) * 2 + 1] = b;
      }
      __syncthreads();
    }
  }
}

// out[o] = sum_i part[i][o], o < L * 6: block o, thread t the pictures t, t + 256, ... ascending, then a tree over the threads
__global__ __launch_bounds__(SW_T) void swd_stats_sum_kernel(const double* __restrict__ part, int n, int L, double* __restrict__ sum, double* __restrict__ sumsq) {
#pragma clang fp contract(off)
  __shared__ double a[SW_T];
  const int t = (int)threadIdx.x, o = (int)blockIdx.x;
  double v = 0.0;
  for (long long i = t; i < n; i += SW_T) v = __dadd_rn(v, part[i * (L * 6) + o]);
  a[t] = v;
  __syncthreads();
  for (int st = SW_T / 2; st >= 1; st >>= 1) {
    if (t < st) a[t] = __dadd_rn(a[t], a[t + st]);
    __syncthreads();
  }
  if (t == 0) ((o & 1) ? sumsq : sum)[o >> 1] = a[0];
}

template <int SMAX> __global__ __launch_bounds__(SW_T) void swd_project_kernel(const SwP p) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) unsigned int lds[SwLds<SMAX>::WORDS];
  const int tid = (int)threadIdx.x;
  const long long i = blockIdx.x;
  const int S = p.S, L = p.L, P = p.P, D = p.D;
  float* out = p.proj + i * P;
  if (!sw_corners_ok(p, i, tid)) {
    const float nan = __uint_as_float(0x7fc00000u);
    for (long long e = tid; e < (long long)L * D * P; e += SW_T) out[(e / P) * p.ld + e % P] = nan;
    return;
  }
  unsigned int* scr = lds + SwLds<SMAX>::PL;
  float* Dt = reinterpret_cast<float*>(scr);                          // [49][SW_DLD]
  float* Xt = Dt + SW_K * SW_DLD;                                     // [49][SW_PT]
  const unsigned char* img = p.img + i * (3ll * S * S);
  const int pl16 = tid & 15, dg = tid >> 4;                           // compute: patches pl16 + 16 j, directions 4 dg + q and 64 + 4 dg + q
  const int gp = tid & 63, gk = tid >> 6;                             // gather: patch gp, components gk, gk + 4, ...
  for (int c = 0; c < 3; ++c) {
    sw_pyramid(img, S, L, c, lds, scr, tid);
    for (int d0 = 0; d0 < D; d0 += SW_DT) {
      __syncthreads();                                                // the tiles' last readers are done
      for (int e = tid; e < SW_DT * SW_K; e += SW_T) {
        const int dd = e / SW_K, k = e - dd * SW_K;
        Dt[k * SW_DLD + dd] = d0 + dd < D ? p.dirs[(long long)(d0 + dd) * SW_DESC + c * SW_K + k] : 0.f;
      }
      for (int l = 0; l < L; ++l) {
        const int s = S >> l;
        const float* plane = reinterpret_cast<const float*>(lds + sw_level_off(S, l));
        const int* pos = p.pos + (i * L + l) * (2ll * P);
        const float mean = p.mean[l * 3 + c], rstd = p.rstd[l * 3 + c];
        for (int p0 = 0; p0 < P; p0 += SW_PT) {
          __syncthreads();
          {
            const bool in = p0 + gp < P;
            const int y = in ? pos[2 * (p0 + gp)] : 0, x = in ? pos[2 * (p0 + gp) + 1] : 0;
            for (int k = gk; k < SW_K; k += SW_T / SW_PT) {
              const int dy = k / 7, dx = k - dy * 7;
              Xt[k * SW_PT + gp] = in ? __fmul_rn(__fsub_rn(plane[(y + dy) * s + x + dx], mean), rstd) : 0.f;
            }
          }
          __syncthreads();
          float acc[4][8];
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int q = 0; q < 8; ++q) acc[j][q] = 0.f;
          for (int k = 0; k < SW_K; ++k) {
            const float4 da = *reinterpret_cast<const float4*>(Dt + k * SW_DLD + 4 * dg);
            const float4 db = *reinterpret_cast<const float4*>(Dt + k * SW_DLD + 64 + 4 * dg);
            const float dv[8] = {da.x, da.y, da.z, da.w, db.x, db.y, db.z, db.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const float xv = Xt[k * SW_PT + pl16 + 16 * j];
#pragma unroll
              for (int q = 0; q < 8; ++q) acc[j][q] = __fmaf_rn(xv, dv[q], acc[j][q]);
            }
          }
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            const int d = d0 + (q < 4 ? 4 * dg + q : 64 + 4 * dg + q - 4);
            if (d < D) {
              float* row = out + ((long long)l * D + d) * p.ld;
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                const int pp = p0 + pl16 + 16 * j;
                if (pp < P) row[pp] = c == 0 ? acc[j][q] : __fadd_rn(row[pp], acc[j][q]);
              }
            }
          }
        }
      }
    }
  }
}

// ---- row sort ----------------------------------------------------------------------------------------------------------------
constexpr int SR_T = 256, SR_E = 8, SR_TILE = SR_T * SR_E;

__device__ __forceinline__ unsigned int sr_key(unsigned int u) { return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u); }
__device__ __forceinline__ unsigned int sr_bits(unsigned int k) { return k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu); }
__device__ __forceinline__ void sr_cmpswap(unsigned int& a, unsigned int& b, bool asc) {
  const unsigned int lo = a < b ? a : b, hi = a < b ? b : a;
  a = asc ? lo : hi;
  b = asc ? hi : lo;
}

// tile t of row r: the keys x[r][2048 t ..] sorted into dst at the same place
__global__ __launch_bounds__(SR_T) void sort_tile_kernel(const unsigned int* __restrict__ x, unsigned int* __restrict__ dst, long long M, int tiles) {
  __shared__ __attribute__((aligned(16))) unsigned int a[SR_TILE];
  const int tid = (int)threadIdx.x;
  const long long row = blockIdx.x / tiles, t = blockIdx.x % tiles, base = row * M + t * SR_TILE;
  const int cnt = (int)(M - t * SR_TILE < SR_TILE ? M - t * SR_TILE : SR_TILE);
#pragma unroll
  for (int r = 0; r < SR_E; ++r) {
    const int e = tid + r * SR_T;
    a[e] = e < cnt ? sr_key(x[base + e]) : 0xffffffffu;              // padding sorts last (a key of that value is the same bits)
  }
  __syncthreads();
  unsigned int v[SR_E];
#pragma unroll
  for (int r = 0; r < SR_E; ++r) v[r] = a[tid * SR_E + r];
#pragma unroll
  for (int k = 2; k <= SR_E; k <<= 1)
#pragma unroll
    for (int j = k >> 1; j >= 1; j >>= 1)
#pragma unroll
      for (int r = 0; r < SR_E; ++r)
        if ((r ^ j) > r) sr_cmpswap(v[r], v[r ^ j], ((tid * SR_E + r) & k) == 0);
#pragma unroll
  for (int r = 0; r < SR_E; ++r) a[tid * SR_E + r] = v[r];
  for (int k = 2 * SR_E; k <= SR_TILE; k <<= 1) {
    for (int j = k >> 1; j >= SR_E; j >>= 1) {
      __syncthreads();
#pragma unroll
      for (int q = 0; q < SR_E / 2; ++q) {
        const int pi = tid + q * SR_T, lo = ((pi & ~(j - 1)) << 1) | (pi & (j - 1)), hi = lo | j;
        unsigned int u = a[lo], w = a[hi];
        sr_cmpswap(u, w, (lo & k) == 0);
        a[lo] = u; a[hi] = w;
      }
    }
    __syncthreads();
    const bool asc = ((tid * SR_E) & k) == 0;
#pragma unroll
    for (int r = 0; r < SR_E; ++r) v[r] = a[tid * SR_E + r];
#pragma unroll
    for (int j = SR_E >> 1; j >= 1; j >>= 1)
#pragma unroll
      for (int r = 0; r < SR_E; ++r)
        if ((r ^ j) > r) sr_cmpswap(v[r], v[r ^ j], asc);
#pragma unroll
    for (int r = 0; r < SR_E; ++r) a[tid * SR_E + r] = v[r];
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < SR_E; ++r) {
    const int e = tid + r * SR_T;
    if (e < cnt) dst[base + e] = sr_bits(a[e]);
  }
}

// merge path: how many of the first d merged keys come from A (ties: A first)
template <typename KA, typename KB> __device__ __forceinline__ long long sr_split(long long d, long long la, long long lb, KA key_a, KB key_b) {
  long long lo = d > lb ? d - lb : 0, hi = d < la ? d : la;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (key_a(mid) <= key_b(d - 1 - mid)) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// one pass: runs of W sorted keys merge in pairs; workgroup (row, t) writes the merged keys 2048 t .. of its row
__global__ __launch_bounds__(SR_T) void sort_merge_kernel(const unsigned int* __restrict__ src, unsigned int* __restrict__ dst, long long M, int tiles, long long W) {
  __shared__ __attribute__((aligned(16))) unsigned int in[SR_TILE];
  __shared__ __attribute__((aligned(16))) unsigned int res[SR_TILE];
  __shared__ long long cut[2];
  const int tid = (int)threadIdx.x;
  const long long row = blockIdx.x / tiles, t = blockIdx.x % tiles;
  const unsigned int* s = src + row * M;
  const long long o0 = t * SR_TILE, ps = o0 / (2 * W) * (2 * W);
  const long long as = ps, bs = ps + W < M ? ps + W : M, be = ps + 2 * W < M ? ps + 2 * W : M;
  const long long la = bs - as, lb = be - bs;
  const long long d0 = o0 - ps, d1 = d0 + SR_TILE < la + lb ? d0 + SR_TILE : la + lb;
  if (tid < 2) {
    const unsigned int *A = s + as, *B = s + bs;
    cut[tid] = sr_split(tid ? d1 : d0, la, lb, [A](long long q) { return sr_key(A[q]); }, [B](long long q) { return sr_key(B[q]); });
  }
  __syncthreads();
  const long long a0 = cut[0], a1 = cut[1], b0 = d0 - a0, b1 = d1 - a1;
  const int na = (int)(a1 - a0), nb = (int)(b1 - b0), nt = na + nb;    // nt = d1 - d0 <= 2048
  for (int e = tid; e < nt; e += SR_T) in[e] = sr_key(e < na ? s[as + a0 + e] : s[bs + b0 + (e - na)]);
  __syncthreads();
  const int dd = tid * SR_E;
  if (dd < nt) {
    const unsigned int *A = in, *B = in + na;
    int ai = (int)sr_split(dd, na, nb, [A](long long q) { return A[q]; }, [B](long long q) { return B[q]; });
    int bi = dd - ai;
#pragma unroll
    for (int r = 0; r < SR_E; ++r) {
      if (dd + r < nt) {
        const bool take_a = bi >= nb || (ai < na && A[ai] <= B[bi]);
        res[dd + r] = take_a ? A[ai] : B[bi];
        ai += take_a; bi += !take_a;
      }
    }
  }
  __syncthreads();
  for (int e = tid; e < nt; e += SR_T) dst[row * M + o0 + e] = sr_bits(res[e]);
}

// w[r] = mean_j |sa[r][j] - sb[r][j]|: thread t the keys t, t + 256, ... ascending in fp64, then a tree over the threads
__global__ __launch_bounds__(SW_T) void swd_rows_kernel(const float* __restrict__ sa, const float* __restrict__ sb, long long M, double* __restrict__ w) {
#pragma clang fp contract(off)
  __shared__ double a[SW_T];
  const int t = (int)threadIdx.x;
  const float *ra = sa + blockIdx.x * M, *rb = sb + blockIdx.x * M;
  double v = 0.0;
  for (long long j = t; j < M; j += SW_T) v = __dadd_rn(v, fabs(__dsub_rn((double)ra[j], (double)rb[j])));
  a[t] = v;
  __syncthreads();
  for (int st = SW_T / 2; st >= 1; st >>= 1) {
    if (t < st) a[t] = __dadd_rn(a[t], a[t + st]);
    __syncthreads();
  }
  if (t == 0) w[blockIdx.x] = __ddiv_rn(a[0], (double)M);
}

inline int sw_max_levels(int S) { return S == 32 ? 2 : S == 64 ? 3 : S == 128 ? 4 : 0; }
inline long long sr_tiles(long long M) { return (M + SR_TILE - 1) / SR_TILE; }
constexpr long long SR_MAX_BLOCKS = 0x7fffffffll;

int sw_check(const char* who, const unsigned char* images, int n, int S, int L, const int* pos, int P) {
  if (!images || !pos) JCK_FAIL(JCK_E_ARG, std::string(who) + ": null argument");
  if (sw_max_levels(S) == 0) JCK_FAIL(JCK_E_ARG, std::string(who) + ": S must be 32, 64 or 128");
  if (L < 1 || L > sw_max_levels(S)) JCK_FAIL(JCK_E_ARG, std::string(who) + ": L must be 1 .. the number of levels with S >> (L-1) >= 16");
  if (P < 1 || P > (1 << 20)) JCK_FAIL(JCK_E_ARG, std::string(who) + ": P must be 1..2^20");
  if (n < 1) JCK_FAIL(JCK_E_ARG, std::string(who) + ": n must be >= 1");
  return JCK_OK;
}

}  // namespace

extern "C" int jck_swd_max_levels(int S) { return sw_max_levels(S); }
extern "C" int jck_sort_rows_tile(void) { return SR_TILE; }

extern "C" size_t jck_sort_rows_ws_bytes(int Rows, long long M) {
  if (Rows < 1 || M < 1 || sr_tiles(M) * Rows > SR_MAX_BLOCKS) return 0;
  return M <= SR_TILE ? 0 : (size_t)Rows * (size_t)M * sizeof(float);
}

extern "C" int jck_swd_patch_stats_u8(const unsigned char* images, int n, int S, int L, const int* pos, int P, double* part, double* sum,
                                      double* sumsq, void* stream) {
  JCK_TRY(sw_check("swd_patch_stats", images, n, S, L, pos, P));
  if (!part || !sum || !sumsq) JCK_FAIL(JCK_E_ARG, "swd_patch_stats: null argument");
  SwP p = {};
  p.img = images; p.pos = pos; p.part = part; p.n = n; p.S = S; p.L = L; p.P = P;
  const hipStream_t st = (hipStream_t)stream;
  if (S == 32) hipLaunchKernelGGL(swd_stats_kernel<32>, dim3((unsigned)n), dim3(SW_T), 0, st, p);
  else if (S == 64) hipLaunchKernelGGL(swd_stats_kernel<64>, dim3((unsigned)n), dim3(SW_T), 0, st, p);
  else hipLaunchKernelGGL(swd_stats_kernel<128>, dim3((unsigned)n), dim3(SW_T), 0, st, p);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(swd_stats_sum_kernel, dim3((unsigned)(L * 6)), dim3(SW_T), 0, st, (const double*)part, n, L, sum, sumsq);
  HIPCHK(hipGetLastError());
  return JCK_OK;
}

extern "C" int jck_swd_project_u8(const unsigned char* images, int n, int S, int L, const int* pos, int P, const float* dirs, int D,
                                  const float* mean, const float* rstd, float* proj, long long ld, void* stream) {
  JCK_TRY(sw_check("swd_project", images, n, S, L, pos, P));
  if (!dirs || !mean || !rstd || !proj) JCK_FAIL(JCK_E_ARG, "swd_project: null argument");
  if (D < 1 || D > (1 << 20)) JCK_FAIL(JCK_E_ARG, "swd_project: D must be 1..2^20");
  if (ld < (long long)n * P) JCK_FAIL(JCK_E_ARG, "swd_project: ld must be >= n * P");
  SwP p = {};
  p.img = images; p.pos = pos; p.dirs = dirs; p.mean = mean; p.rstd = rstd; p.proj = proj; p.ld = ld; p.n = n; p.S = S; p.L = L; p.P = P; p.D = D;
  const hipStream_t st = (hipStream_t)stream;
  if (S == 32) hipLaunchKernelGGL(swd_project_kernel<32>, dim3((unsigned)n), dim3(SW_T), 0, st, p);
  else if (S == 64) hipLaunchKernelGGL(swd_project_kernel<64>, dim3((unsigned)n), dim3(SW_T), 0, st, p);
  else hipLaunchKernelGGL(swd_project_kernel<128>, dim3((unsigned)n), dim3(SW_T), 0, st, p);
  HIPCHK(hipGetLastError());
  return JCK_OK;
}

extern "C" int jck_sort_rows_f32(const float* x, int Rows, long long M, float* out, void* ws, size_t ws_bytes, void* stream) {
  if (!x || !out) JCK_FAIL(JCK_E_ARG, "sort_rows: null argument");
  if (Rows < 1 || M < 1) JCK_FAIL(JCK_E_ARG, "sort_rows: Rows and M must be >= 1");
  const long long tiles = sr_tiles(M);
  if (tiles * Rows > SR_MAX_BLOCKS) JCK_FAIL(JCK_E_ARG, "sort_rows: Rows * ceil(M / 2048) must be below 2^31");
  const size_t need = jck_sort_rows_ws_bytes(Rows, M);
  if (need > 0 && (!ws || ws_bytes < need)) JCK_FAIL(JCK_E_ARG, "sort_rows: the workspace is smaller than jck_sort_rows_ws_bytes(Rows, M)");
  int passes = 0;
  while (((long long)SR_TILE << passes) < M) ++passes;
  const hipStream_t st = (hipStream_t)stream;
  unsigned int* bufs[2] = {reinterpret_cast<unsigned int*>(out), reinterpret_cast<unsigned int*>(ws)};
  int cur = passes & 1;                                               // the tile sort's target: `out` after an even number of passes
  const dim3 grid((unsigned)(tiles * Rows));
  hipLaunchKernelGGL(sort_tile_kernel, grid, dim3(SR_T), 0, st, reinterpret_cast<const unsigned int*>(x), bufs[cur], M, (int)tiles);
  HIPCHK(hipGetLastError());
  for (int ps = 0; ps < passes; ++ps) {
    hipLaunchKernelGGL(sort_merge_kernel, grid, dim3(SR_T), 0, st, (const unsigned int*)bufs[cur], bufs[cur ^ 1], M, (int)tiles, (long long)SR_TILE << ps);
    HIPCHK(hipGetLastError());
    cur ^= 1;
  }
  return JCK_OK;
}

extern "C" int jck_swd_rows(const float* sa, const float* sb, int Rows, long long M, double* w, void* stream) {
  if (!sa || !sb || !w) JCK_FAIL(JCK_E_ARG, "swd_rows: null argument");
  if (Rows < 1 || M < 1) JCK_FAIL(JCK_E_ARG, "swd_rows: Rows and M must be >= 1");
  hipLaunchKernelGGL(swd_rows_kernel, dim3((unsigned)Rows), dim3(SW_T), 0, (hipStream_t)stream, sa, sb, M, w);
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
