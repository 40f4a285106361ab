// Structural similarity of pairs of uint8 pictures: SSIM, a multi-scale SSIM over L <= 4 levels and the squared error, one workgroup
// per pair, no intermediate in HBM and no atomics on floats.
//
//   jck_ssim_pairs_u8     ssim[p], ms_ssim[p], sq_err[p] (and the per channel / level means of the cs and ss maps) of the pairs
//                         (a[ia[p]], b[ib[p]]) of NHWC pictures [n][S][S][3]
//   jck_ssim_max_levels   the largest admissible L for S (host only)
//
// The arithmetic: per channel and level the 11-tap Gaussian window (sigma 1.5, fp32 roundings of the fp64 weights) over
// the valid region gives the windowed means mx, my, exx, eyy, exy of x, y, x x, y y, x y; vx = exx - mx mx, vy = eyy - my my,
// vxy = exy - mx my (formed on x - kx and y - ky, kx and ky the two pictures' mean levels in the channel rounded to whole numbers);
// cs = (2 vxy + C2) / (vx + vy + C2), ss = (2 mx my + C1) / (mx mx + my my + C1) * cs; cs[c][l], ss[c][l] are the means of the two
// maps; the next level is the 2 x 2 mean of both planes.
//
// One workgroup of 512 threads (8 waves) per pair:
//   load      both pictures go to LDS as their bytes, once.  A picture starts at any byte: LDS byte (g & 15) + i holds byte i, so that
//             the 16-byte chunks of the aligned body are 16-byte aligned on both sides; the chunks that straddle the picture's ends
//             are moved byte by byte and nothing outside the picture is read.
//   sq_err    integer sums of (a - b)^2 over the LDS bytes, per thread in 32 bits, across threads in 64; with them the sum of each
//             picture's bytes per channel (integer LDS atomics), from which the centres kx, ky come.
//   levels    per channel, level l >= 1 of both planes is kept as the uint16 SUM of the 4^l bytes under each pixel (at most 64 * 255);
//             the value is that sum times 4^-l, exact in fp32.
//   maps      a wave owns a band of the map's rows.  VERTICAL pass first: a lane owns a column (two when the plane is wider than 64)
//             and walks down the band with the last 11 values of x and y in registers, so a plane row is read from LDS once per band:
//             lanes read consecutive pixels (bytes 3 apart or uint16s: at most 24 distinct dwords per 32 lanes, each in a bank of its
//             own), the tap weight is a literal.  The five vertical sums of a row go to the wave's own LDS row V[5][128]; the
//             HORIZONTAL pass reads them back, lane o the floats o .. o + 10 - consecutive lanes consecutive dwords, tap by tap with a
//             wave-uniform weight, so no access has a bank conflict.  The row is the wave's own: no workgroup barrier inside a level.
//             The map values are added per lane in row order.
//   means     a lane's sum over its rows in ascending order, then a 64-lane xor butterfly (32, 16, ... 1), then the 8 waves in ascending
//             order: an order fixed by S and l.  The mean is the correctly rounded quotient by the map's size.
//   combine   thread 0: ssim = mean_c ss[c][0]; ms[c] = prod_l max(cs[c][l], 0)^w_l * max(ss[c][L-1], 0)^w_(L-1); ms_ssim = mean_c.
// Every product and sum of the map formulas is rounded once (contraction off; the filter sums are explicit fmaf chains, the same code
// for x and y), so the outputs are bit-symmetric under swapping the two pictures and a pair of equal pictures gives 1.0f, 1.0f, 0.
// A pair's bits depend on its two pictures, S and L alone: nothing is shared between workgroups.
//
// LDS per workgroup (static, by the size class of S; pictures + levels + V rows + sums): <= 32: 6 176 + 1 344 + 10 240 + 448 = 18 208
// bytes and <= 64: 24 608 + 5 376 + 10 240 + 448 = 40 672 (two workgroups per CU: 16 waves of about 100 registers); <= 128:
// 98 336 + 21 504 + 20 480 + 448 = 140 768 (one workgroup per CU).
#include "ops_internal.hpp"

namespace {

constexpr int SS_T = 512, SS_W = SS_T / 64, SS_LMAX = 4;
constexpr int SS_PMAX = 1 << 24;
constexpr float SS_C1 = 6.5025f, SS_C2 = 58.5225f;         // (0.01 * 255)^2, (0.03 * 255)^2
// exp(-(j - 5)^2 / 4.5) / sum in fp64, rounded to fp32
#define SS_G0 1.028380124e-03f
#define SS_G1 7.598758209e-03f
#define SS_G2 3.600077331e-02f
#define SS_G3 1.093606874e-01f
#define SS_G4 2.130055428e-01f
#define SS_G5 2.660117149e-01f

struct SsP {
  const unsigned char *a, *b;
  const long long *ia, *ib;
  long long na, nb;
  int S, L;
  float w[SS_LMAX];
  float *ssim, *ms, *terms;
  long long* sq;
};

template <int SMAX> struct SsLds {
  static constexpr int NC = SMAX > 64 ? 2 : 1;                      // columns of a lane
  static constexpr int IMG = (3 * SMAX * SMAX + 31) & ~15;          // a picture's bytes behind a shift of up to 15
  static constexpr int N1 = (SMAX / 2) * (SMAX / 2), N2 = N1 / 4, N3 = N2 / 4;
  static constexpr int LEV = 2 * (N1 + N2 + N3) * 2;                // two planes of every level >= 1, uint16
  static constexpr int VLD = 64 * NC;
  static constexpr int VROW = 5 * VLD * 4;                          // a wave's five vertical sums of one row
  static constexpr int OFF_LEV = 2 * IMG, OFF_V = OFF_LEV + LEV, OFF_RED = OFF_V + SS_W * VROW;
  static constexpr int BYTES = OFF_RED + 448;                       // 16 wave sums, 8 wave squared errors, 24 terms, 6 byte sums
  __host__ __device__ static constexpr int lev_off(int l) { return l == 1 ? 0 : l == 2 ? 2 * N1 : 2 * (N1 + N2); }
  __host__ __device__ static constexpr int lev_plane(int l) { return l == 1 ? N1 : l == 2 ? N2 : N3; }
};

__device__ __forceinline__ float ss_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = __fadd_rn(v, __shfl_xor(v, o, 64));
  return v;
}

// Between a wave's stores to its own V row and its loads from it, and back: one wave's LDS operations complete in the order they
// were issued, so the compiler alone has to be kept from moving them across this point; no other wave touches the row.
__device__ __forceinline__ void ss_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// sum_j g_j v[j], j ascending
__device__ __forceinline__ float ss_tap11(const float (&v)[11]) {
  float s = __fmul_rn(SS_G0, v[0]);
  s = __fmaf_rn(SS_G1, v[1], s); s = __fmaf_rn(SS_G2, v[2], s); s = __fmaf_rn(SS_G3, v[3], s); s = __fmaf_rn(SS_G4, v[4], s);
  s = __fmaf_rn(SS_G5, v[5], s); s = __fmaf_rn(SS_G4, v[6], s); s = __fmaf_rn(SS_G3, v[7], s); s = __fmaf_rn(SS_G2, v[8], s);
  s = __fmaf_rn(SS_G1, v[9], s); s = __fmaf_rn(SS_G0, v[10], s);
  return s;
}

// The cs and ss maps of one level of one channel, added per lane.  LEVEL0: the planes are the pictures' bytes (pa, pb point at the
// channel's byte of pixel 0, pixels 3 bytes apart), else uint16 sums with `scale` = 4^-l.  s: the plane's side.  V: this wave's row.
// kx, ky: the centres taken off the two planes (whole numbers: the differences are exact).
template <int NC, bool LEVEL0> __device__ __forceinline__ void ss_maps(const void* pa, const void* pb, int s, float scale, float kx, float ky,
                                                                      float* V, int lane, int wave, float& sum_cs, float& sum_ss) {
#pragma clang fp contract(off)
  constexpr int VLD = 64 * NC;
  const int m = s - 10, rp = (m + SS_W - 1) / SS_W, y0 = wave * rp;
  float wx[NC][11], wy[NC][11];
#pragma unroll
  for (int k = 0; k < NC; ++k)
#pragma unroll
    for (int j = 0; j < 11; ++j) wx[k][j] = wy[k][j] = 0.f;
  float acs = 0.f, ass = 0.f;
  for (int it = 0; it < rp + 10; ++it) {
    const int y = y0 + it;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
#pragma unroll
      for (int j = 0; j < 10; ++j) { wx[k][j] = wx[k][j + 1]; wy[k][j] = wy[k][j + 1]; }
      const int col = lane + 64 * k;
      float vx = 0.f, vy = 0.f;
      if (y < s && col < s) {
        const int at = y * s + col;
        if (LEVEL0) {
          vx = __fsub_rn((float)((const unsigned char*)pa)[3 * at], kx);
          vy = __fsub_rn((float)((const unsigned char*)pb)[3 * at], ky);
        } else {
          vx = __fsub_rn(__fmul_rn((float)((const unsigned short*)pa)[at], scale), kx);
          vy = __fsub_rn(__fmul_rn((float)((const unsigned short*)pb)[at], scale), ky);
        }
      }
      wx[k][10] = vx; wy[k][10] = vy;
    }
    const bool row = it >= 10 && y - 10 < m;                        // wave-uniform: the window holds rows y - 10 .. y of map row y - 10
    if (row) {
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        const int col = lane + 64 * k;
        if (col < s) {
          float xx[11], yy[11], xy[11];
#pragma unroll
          for (int j = 0; j < 11; ++j) {
            xx[j] = __fmul_rn(wx[k][j], wx[k][j]); yy[j] = __fmul_rn(wy[k][j], wy[k][j]); xy[j] = __fmul_rn(wx[k][j], wy[k][j]);
          }
          V[0 * VLD + col] = ss_tap11(wx[k]);
          V[1 * VLD + col] = ss_tap11(wy[k]);
          V[2 * VLD + col] = ss_tap11(xx);
          V[3 * VLD + col] = ss_tap11(yy);
          V[4 * VLD + col] = ss_tap11(xy);
        }
      }
    }
    ss_wave_sync();
    if (row) {
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        const int o = lane + 64 * k;
        if (o < m) {
          float q[5];
#pragma unroll
          for (int f = 0; f < 5; ++f) {
            float t[11];
#pragma unroll
            for (int j = 0; j < 11; ++j) t[j] = V[f * VLD + o + j];
            q[f] = ss_tap11(t);
          }
          const float dx = q[0], dy = q[1];                           // the windowed means of x - kx, y - ky
          const float vx = __fsub_rn(q[2], __fmul_rn(dx, dx)), vy = __fsub_rn(q[3], __fmul_rn(dy, dy)), vxy = __fsub_rn(q[4], __fmul_rn(dx, dy));
          const float mx = __fadd_rn(dx, kx), my = __fadd_rn(dy, ky);
          const float mxx = __fmul_rn(mx, mx), myy = __fmul_rn(my, my), mxy = __fmul_rn(mx, my);
          const float cs = __fdiv_rn(__fadd_rn(__fmul_rn(2.f, vxy), SS_C2), __fadd_rn(__fadd_rn(vx, vy), SS_C2));
          const float lum = __fdiv_rn(__fadd_rn(__fmul_rn(2.f, mxy), SS_C1), __fadd_rn(__fadd_rn(mxx, myy), SS_C1));
          acs = __fadd_rn(acs, cs);
          ass = __fadd_rn(ass, __fmul_rn(lum, cs));
        }
      }
    }
    ss_wave_sync();
  }
  sum_cs = acs; sum_ss = ass;
}

__device__ __forceinline__ float ss_pow(float v, float w) { return v > 0.f ? exp2f(__fmul_rn(w, log2f(v))) : 0.f; }

template <int SMAX> __global__ __launch_bounds__(SS_T) void ssim_pairs_kernel(const SsP p) {
#pragma clang fp contract(off)
  typedef SsLds<SMAX> Ld;
  constexpr int NC = Ld::NC;
  __shared__ __attribute__((aligned(16))) unsigned char lds[Ld::BYTES];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long pair = blockIdx.x;
  const int S = p.S, L = p.L, n = 3 * S * S;
  const long long ia = p.ia[pair], ib = p.ib[pair];
  if (ia < 0 || ia >= p.na || ib < 0 || ib >= p.nb) {               // uniform: the whole workgroup leaves
    const float nan = __uint_as_float(0x7fc00000u);
    if (tid == 0) { p.ssim[pair] = nan; p.ms[pair] = nan; p.sq[pair] = -1; }
    if (p.terms && tid < 6 * L) p.terms[pair * (6 * L) + tid] = nan;
    return;
  }
  unsigned short* lev = reinterpret_cast<unsigned short*>(lds + Ld::OFF_LEV);
  float* V = reinterpret_cast<float*>(lds + Ld::OFF_V) + wave * (5 * Ld::VLD);
  float* red = reinterpret_cast<float*>(lds + Ld::OFF_RED);                          // [SS_W][2]
  unsigned long long* redq = reinterpret_cast<unsigned long long*>(lds + Ld::OFF_RED + 64);      // [SS_W]
  float* term = reinterpret_cast<float*>(lds + Ld::OFF_RED + 128);                   // [3][L][2]
  unsigned int* bsum = reinterpret_cast<unsigned int*>(lds + Ld::OFF_RED + 224);     // [2][3]: the sum of a picture's bytes per channel
  if (tid < 6) bsum[tid] = 0;

  int shift[2];
#pragma unroll
  for (int im = 0; im < 2; ++im) {
    const unsigned char* __restrict__ g = im ? p.b + ib * n : p.a + ia * n;
    const int sh = (int)(reinterpret_cast<uintptr_t>(g) & 15);
    unsigned char* dst = lds + im * Ld::IMG;                        // byte i of the picture at dst[sh + i]
    const int chunks = (sh + n + 15) >> 4;                          // 16 * chunks <= Ld::IMG
    for (int k = tid; k < chunks; k += SS_T) {
      const int lo = 16 * k - sh;                                   // LDS bytes 16k .. 16k + 15 = picture bytes lo .. lo + 15
      if (lo >= 0 && lo + 16 <= n) {
        *reinterpret_cast<uint4*>(dst + 16 * k) = *reinterpret_cast<const uint4*>(g + lo);
      } else {
        const int i0 = lo < 0 ? 0 : lo, i1 = lo + 16 < n ? lo + 16 : n;
        for (int i = i0; i < i1; ++i) dst[sh + i] = g[i];
      }
    }
    shift[im] = sh;
  }
  __syncthreads();
  const unsigned char* A = lds + shift[0];
  const unsigned char* B = lds + Ld::IMG + shift[1];

  {
    unsigned int e = 0, sa[3] = {0, 0, 0}, sb[3] = {0, 0, 0};       // at most 96 bytes a thread: below 2^23
    for (int i = tid; i < n; i += SS_T) {
      const int va = A[i], vb = B[i], ch = i % 3, d = va - vb;
      e += (unsigned int)(d * d);
#pragma unroll
      for (int c = 0; c < 3; ++c) { sa[c] += ch == c ? va : 0; sb[c] += ch == c ? vb : 0; }
    }
    unsigned long long q = e;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      q += __shfl_xor(q, o, 64);
#pragma unroll
      for (int c = 0; c < 3; ++c) { sa[c] += __shfl_xor(sa[c], o, 64); sb[c] += __shfl_xor(sb[c], o, 64); }
    }
    if (lane == 0) {
      redq[wave] = q;
#pragma unroll
      for (int c = 0; c < 3; ++c) { atomicAdd(&bsum[c], sa[c]); atomicAdd(&bsum[3 + c], sb[c]); }       // integers: any order
    }
  }
  __syncthreads();

  for (int c = 0; c < 3; ++c) {
    // each plane is centred on its picture's mean level in this channel, rounded to a whole number: vx, vy and vxy do not change with
    // the centres, and exx - mx mx no longer cancels digits that fp32 does not have (a flat picture is the worst case)
    const float kx = (float)((2u * bsum[c] + (unsigned)(S * S)) / (2u * (unsigned)(S * S)));
    const float ky = (float)((2u * bsum[3 + c] + (unsigned)(S * S)) / (2u * (unsigned)(S * S)));
    for (int l = 1; l < L; ++l) {                                   // the sums of level l from the bytes (l = 1) or from level l - 1
      const int s = S >> l, np = s * s;
      unsigned short* dst = lev + Ld::lev_off(l);
      const unsigned short* src = lev + Ld::lev_off(l > 1 ? l - 1 : 1);
      const int src_plane = Ld::lev_plane(l > 1 ? l - 1 : 1);
      for (int i = tid; i < 2 * np; i += SS_T) {
        const int im = i >= np, r = im ? i - np : i, y = r / s, x = r - y * s;
        unsigned int v;
        if (l == 1) {
          const unsigned char* q = (im ? B : A) + c;
          const int at = (2 * y * S + 2 * x) * 3;
          v = (unsigned int)q[at] + q[at + 3] + q[at + 3 * S] + q[at + 3 * S + 3];
        } else {
          const unsigned short* q = src + im * src_plane;
          const int at = 2 * y * (2 * s) + 2 * x;
          v = (unsigned int)q[at] + q[at + 1] + q[at + 2 * s] + q[at + 2 * s + 1];
        }
        dst[im * Ld::lev_plane(l) + r] = (unsigned short)v;
      }
      __syncthreads();
    }
    for (int l = 0; l < L; ++l) {
      const int s = S >> l, m = s - 10;
      float cs, ss;
      if (l == 0) ss_maps<NC, true>(A + c, B + c, s, 1.f, kx, ky, V, lane, wave, cs, ss);
      else ss_maps<NC, false>(lev + Ld::lev_off(l), lev + Ld::lev_off(l) + Ld::lev_plane(l), s, 1.f / (float)(1 << (2 * l)), kx, ky, V, lane, wave, cs, ss);
      cs = ss_wave_sum(cs); ss = ss_wave_sum(ss);
      if (lane == 0) { red[2 * wave] = cs; red[2 * wave + 1] = ss; }
      __syncthreads();
      if (tid == 0) {
        float tc = red[0], ts = red[1];
#pragma unroll
        for (int w = 1; w < SS_W; ++w) { tc = __fadd_rn(tc, red[2 * w]); ts = __fadd_rn(ts, red[2 * w + 1]); }
        const float cnt = (float)(m * m);
        term[(c * L + l) * 2] = __fdiv_rn(tc, cnt);
        term[(c * L + l) * 2 + 1] = __fdiv_rn(ts, cnt);
      }
      __syncthreads();                                              // red is free again, and every wave is done with this level's planes
    }
  }

  if (tid == 0) {
    unsigned long long q = 0;
    for (int w = 0; w < SS_W; ++w) q += redq[w];
    float ms[3];
    for (int c = 0; c < 3; ++c) {
      float v = 1.f;
      for (int l = 0; l < L; ++l) v = __fmul_rn(v, ss_pow(term[(c * L + l) * 2 + (l == L - 1 ? 1 : 0)], p.w[l]));
      ms[c] = v;
    }
    p.ssim[pair] = __fdiv_rn(__fadd_rn(__fadd_rn(term[1], term[2 * L + 1]), term[4 * L + 1]), 3.f);
    p.ms[pair] = __fdiv_rn(__fadd_rn(__fadd_rn(ms[0], ms[1]), ms[2]), 3.f);
    p.sq[pair] = (long long)q;
    if (p.terms)
      for (int i = 0; i < 6 * L; ++i) p.terms[pair * (6 * L) + i] = term[i];
  }
}

inline int ss_max_levels(int S) {
  if (S < 11 || S > 128) return 0;
  int L = 1;
  while (L < SS_LMAX && S % (1 << L) == 0 && (S >> L) >= 11) ++L;
  return L;
}

}  // namespace

extern "C" int jck_ssim_max_levels(int S) { return ss_max_levels(S); }

extern "C" int jck_ssim_pairs_u8(const unsigned char* a, long long na, const unsigned char* b, long long nb, int S, const long long* ia,
                                 const long long* ib, int P, int L, float* ssim, float* ms_ssim, long long* sq_err, float* terms,
                                 void* stream) {
  if (!a || !b || !ia || !ib || !ssim || !ms_ssim || !sq_err) JCK_FAIL(JCK_E_ARG, "ssim_pairs: null argument");
  if (S < 11 || S > 128) JCK_FAIL(JCK_E_ARG, "ssim_pairs: S must be 11..128");
  if (L < 1 || L > ss_max_levels(S)) JCK_FAIL(JCK_E_ARG, "ssim_pairs: L must be >= 1 with S % 2^(L-1) == 0 and S >> (L-1) >= 11");
  if (P < 1 || P > SS_PMAX) JCK_FAIL(JCK_E_ARG, "ssim_pairs: P must be 1..2^24");
  if (na < 1 || nb < 1) JCK_FAIL(JCK_E_ARG, "ssim_pairs: na and nb must be >= 1");
  static const double W5[5] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
  SsP p = {};
  p.a = a; p.b = b; p.ia = ia; p.ib = ib; p.na = na; p.nb = nb; p.S = S; p.L = L;
  p.ssim = ssim; p.ms = ms_ssim; p.sq = sq_err; p.terms = terms;
  double total = 0.0;
  for (int l = 0; l < L; ++l) total += W5[l];
  for (int l = 0; l < L; ++l) p.w[l] = (float)(W5[l] / total);
  const hipStream_t st = (hipStream_t)stream;
  if (S <= 32) hipLaunchKernelGGL(ssim_pairs_kernel<32>, dim3((unsigned)P), dim3(SS_T), 0, st, p);
  else if (S <= 64) hipLaunchKernelGGL(ssim_pairs_kernel<64>, dim3((unsigned)P), dim3(SS_T), 0, st, p);
  else hipLaunchKernelGGL(ssim_pairs_kernel<128>, dim3((unsigned)P), dim3(SS_T), 0, st, p);
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
