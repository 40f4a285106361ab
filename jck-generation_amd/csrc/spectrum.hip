// Power spectra of uint8 pictures: per picture the two-dimensional DFT of one centred, optionally windowed plane, its
// power, the radial profile and, over a set, the mean power plane.  Every transform lives in LDS; no atomics, every sum in an order
// fixed by S (and, for the mean plane, by n).
//
//   jck_spectrum_u8         prof[i][r], mean[i] and (optionally) mean2d[u][v] of n pictures
//   jck_spectrum_bins, jck_spectrum_grid, jck_spectrum_ws_bytes   host only
//
// Definition.  x uint8 [n][S][S][3], S in {32, 64, 128}.  Y = 77 R + 150 G + 29 B (plane 3, luma) or 256 * byte (planes 0..2), an
// integer in units of 1/256 byte level.  T = sum Y (< 2^30), mean = T / (256 S^2), c = S^2 Y - T (an int32, |c| < 2^30), converted to
// fp32 once and scaled by 2^-(8 + 2 log2 S): a constant picture is exactly 0.  With a window w (fp32 [S], built by the caller) the value
// is fmul(fmul(c, w[y]), w[x]).  F = DFT2(val), P = |F|^2 / (S^2 W) with W the window power (1 without one); the kernel multiplies by
// inv = 1 / (S^2 W), computed once in fp64 on the host.  Bin r of (u, v): fu = min(u, S - u), fv = min(v, S - v), d2 = fu^2 + fv^2,
// r^2 - r < d2 <= r^2 + r (r = 0 at d2 = 0): R = 24 / 46 / 92 bins.  prof[i][r] = (sum of P over bin r) / count[r].
//
// Kernel.  One workgroup per picture, 256 threads (1024 at S = 128, where a workgroup has the CU to itself) (with the mean plane: workgroup g of G = jck_spectrum_grid(S) takes the pictures
// g, g + G, ... in ascending order).
//   plane     the picture's bytes by aligned dword loads into region Z, then Y as int32 [S][S] in LDS (region F, below), T by a wave butterfly and the waves' sums: integers, exact in any order.
//   rows      the input is real: rows 2k and 2k + 1 are the real and imaginary part of ONE complex row z_k, S / 2 transforms of S
//             points.  z_k is written in bit-reversed order of x into region Z, rows of S + 1 complex words, and transformed in place
//             by log2 S radix-2 decimation-in-time stages.  A stage's S / 2 x S / 2 butterflies are spread with the transform index
//             fastest over the lanes: the lanes of a wave read one butterfly of 64 (32 at S = 64) transforms, S + 1 complex words
//             apart - an odd number of 8-byte words, so the 32 lanes of a ds_read_b64 group fall on 32 different bank pairs - and the
//             twiddle is one LDS word for the whole wave.
//   split     A_k[v] = (Z[v] + conj Z[S - v]) / 2 and B_k[v] = (Z[v] - conj Z[S - v]) / 2i, v = 0 .. S / 2, are the transforms of rows
//             2k and 2k + 1: only the half plane v <= S / 2 is formed, into region F as [S][S / 2 + 1] complex words, row y at the
//             bit-reversed position of y.  One addition and an exact halving per component.
//   columns   S / 2 + 1 transforms of S points down region F, the same stages; the column index is fastest over the lanes, so a wave
//             reads 64 CONSECUTIVE complex words per butterfly: the column pass walks no bank twice, by the order of the work, not by
//             padding (the row stride S / 2 + 1 is merely what the half plane needs).
//   power     P = (re^2 + im^2) * inv in fp64, written over its own complex word (8 bytes either way).  The columns v = 0 and S / 2 hold
//             both members of a mirror pair (u, S - u): both get (P[u] + P[S - u]) / 2, lower u first, so the plane is bit-symmetric
//             and the pair's error is no larger than the sum of its members' (no factor sqrt 2 from picking one of them).
//   bins      a host-built table lists the S^2 / 2 + 2 canonical points (v in 1 .. S/2 - 1: every u, weight 2; v in {0, S/2}: u <= S/2,
//             weight 2 for 0 < u < S/2, else 1) bin by bin, ascending (u, v) inside a bin.  Wave w of W sums the bins w, w + W, ...: lane l the
//             entries l, l + 64, ... ascending in fp64 (2 P is exact), then a 64-lane xor butterfly, then one division by count[r].
//   mean      with the mean plane the workgroup stores (first picture) or adds (later ones) its half plane into its own partial plane
//             ws[g][S][S / 2 + 1]; a second launch adds the partials g = 0 .. min(n, G) - 1 in ascending order per point, divides by n
//             and writes (u, v) from the half-plane point (u, v) or (S - u, S - v): mirror points hold equal bits.
// Twiddles exp(-2 pi i m / S), m < S / 2, and the bin table are built on the host in fp64 (twiddles rounded to fp32: mu = 2^-24) and
// copied once per device into a __device__ table; the kernel copies the twiddles to LDS.  No approximate intrinsics anywhere.
//
// LDS per workgroup (dynamic; F = S (S/2 + 1) 8, Z = S/2 (S + 1) 8, twiddles S/2 8, window S 4, 64 bytes of wave sums):
//   S =  32:   4 352 +  4 224 + 128 + 128 + 64 =   8 896 bytes
//   S =  64:  16 896 + 16 640 + 256 + 256 + 64 =  34 112 bytes   (four workgroups per CU)
//   S = 128:  66 560 + 66 048 + 512 + 512 + 64 = 133 696 bytes   (one workgroup per CU; above the default dynamic limit: sp_launch_lds)
//
// Error bound B(S) (tests/spectrum_ref.py restates it).  u = 2^-24.  A radix-2 Cooley-Tukey transform of t stages with twiddles
// accurate to mu has ||F^ - F||_2 <= e ||F||_2, e = t eta / (1 - t eta), eta = mu + gamma_4 (sqrt 2 + mu), gamma_4 = 4u / (1 - 4u)
// (Higham, Accuracy and Stability, Th. 24.2).  Rows then columns: (1 + e_1)^2 <= 1 / (1 - 2 t_1 eta), so t = 2 log2 S covers both passes;
// column v carries weight 1 or 2 in the full-plane norm, which a per-column relative bound does not notice.  The split is an isometry
// of the S / 2 complex rows onto the S real rows' transforms followed by one rounding per component: a factor (1 + u).  The input has at
// most three roundings (the conversion of c, two window products; the scaling is a power of two): e_in = (1 + u)^3 - 1.  Together
//   e = e_in + (1 + e_in) ((1 + e_fft)(1 + u) - 1),   sum |P^ - P| <= (2 e + e^2) E   by Cauchy-Schwarz, E = sum P of the exact plane,
// and the fp64 steps (the power's three roundings, bin sums, partial planes: fewer than 2^13 terms each) add 2^-40:
//   B(S) = (2 e + e^2)(1 + 2^-40) + 2^-40 = 8.41e-6, 1.000e-5, 1.159e-5 for S = 32, 64, 128  (the cap is 2e-5).
// The same bound holds for sum_r count[r] |prof^[r] - prof[r]| and for the mean plane of up to 2^12 pictures against the mean energy.
//
// Compiler's resource remarks (gfx950, -O3): spectrum_kernel<32 / 64 / 128> 52 / 58 / 58 VGPRs, 74 / 68 / 76 SGPRs, scratch 0, no static
// LDS (the dynamic figures above), 8 waves per SIMD by registers; spectrum_mean_kernel 14 VGPRs, 14 SGPRs, scratch 0.
#include <mutex>
#include <vector>

#include "ops_internal.hpp"

namespace {

constexpr int SP_T = 256;
struct __attribute__((aligned(8))) sp_c { float x, y; };              // a complex word

template <int S> struct SpCfg {
  static constexpr int LG = S == 32 ? 5 : S == 64 ? 6 : 7, LD = S / 2 + 1, ZS = S + 1, R = S == 32 ? 24 : S == 64 ? 46 : 92, NC = S * S / 2 + 2;
  static constexpr int F_WORDS = S * LD * 2, Z_WORDS = (S / 2) * ZS * 2, TW_WORDS = S, WIN_WORDS = S, RED_WORDS = 16;
  static constexpr int LDS_BYTES = 4 * (F_WORDS + Z_WORDS + TW_WORDS + WIN_WORDS + RED_WORDS);
  static constexpr int G = S == 128 ? 256 : 1024;                      // workgroups of a mean-plane launch
  static constexpr int T = S == 128 ? 1024 : 256;                      // threads: at S = 128 one workgroup fills the CU, so it brings 16 waves
  static_assert(T / 64 <= RED_WORDS, "one wave sum each");
  static_assert(F_WORDS >= S * S, "the integer plane lives in region F");
};

// twiddles, bin offsets, bin counts, and the canonical points bin by bin: LDS index u * LD + v, bit 16 = weight 2
template <int S> struct SpTab {
  sp_c tw[S / 2];
  int off[SpCfg<S>::R + 1];
  int cnt[SpCfg<S>::R];
  unsigned int ent[SpCfg<S>::NC];
};

__device__ SpTab<32> sp_tab32;
__device__ SpTab<64> sp_tab64;
__device__ SpTab<128> sp_tab128;

template <int S> __device__ __forceinline__ const SpTab<S>& sp_tab() {
  if constexpr (S == 32) return sp_tab32;
  else if constexpr (S == 64) return sp_tab64;
  else return sp_tab128;
}

struct SpP {
  const unsigned char* x;
  const float* win;                                                   // [S] or null
  double *prof, *mean, *part;                                         // part: [grid][S][LD] or null
  double inv;                                                         // 1 / (S^2 W)
  int n, plane;
};

typedef double __attribute__((may_alias)) sp_f64;                     // P is written over the complex word it came from

// log2 S radix-2 decimation-in-time stages over NT transforms of S points whose input is in bit-reversed order: element i of transform
// k at buf[k * TSTR + i * ESTR].  The transform index is fastest over the threads.  Starts after and ends with a barrier.
template <int S, int NT, int TSTR, int ESTR> __device__ __forceinline__ void sp_fft(sp_c* buf, const sp_c* tw, int tid) {
  constexpr int LG = SpCfg<S>::LG, SP_T = SpCfg<S>::T;
  for (int s = 0; s < LG; ++s) {
    const int h = 1 << s;
    for (int it = tid; it < NT * (S / 2); it += SP_T) {
      const int b = it / NT, k = it - b * NT;
      const int j = b & (h - 1), i0 = ((b - j) << 1) + j;
      const sp_c w = tw[j << (LG - 1 - s)];
      sp_c* p0 = buf + k * TSTR + i0 * ESTR;
      sp_c* p1 = p0 + h * ESTR;
      const sp_c a = *p0, c = *p1;
      const float tr = __fsub_rn(__fmul_rn(w.x, c.x), __fmul_rn(w.y, c.y));
      const float ti = __fadd_rn(__fmul_rn(w.x, c.y), __fmul_rn(w.y, c.x));
      *p0 = sp_c{__fadd_rn(a.x, tr), __fadd_rn(a.y, ti)};
      *p1 = sp_c{__fsub_rn(a.x, tr), __fsub_rn(a.y, ti)};
    }
    __syncthreads();
  }
}

template <int S> __global__ __launch_bounds__(SpCfg<S>::T) void spectrum_kernel(const SpP p) {
#pragma clang fp contract(off)
  using C = SpCfg<S>;
  constexpr int LG = C::LG, LD = C::LD, ZS = C::ZS, R = C::R, SP_T = C::T;
  extern __shared__ __attribute__((aligned(16))) unsigned int sp_lds[];
  sp_c* F = reinterpret_cast<sp_c*>(sp_lds);
  int* Yp = reinterpret_cast<int*>(sp_lds);
  sp_f64* Pw = reinterpret_cast<sp_f64*>(sp_lds);
  sp_c* Z = reinterpret_cast<sp_c*>(sp_lds + C::F_WORDS);
  sp_c* tw = reinterpret_cast<sp_c*>(sp_lds + C::F_WORDS + C::Z_WORDS);
  float* win = reinterpret_cast<float*>(sp_lds + C::F_WORDS + C::Z_WORDS + C::TW_WORDS);
  int* red = reinterpret_cast<int*>(sp_lds + C::F_WORDS + C::Z_WORDS + C::TW_WORDS + C::WIN_WORDS);
  const SpTab<S>& tab = sp_tab<S>();
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool windowed = p.win != nullptr;
  if (tid < S / 2) tw[tid] = tab.tw[tid];
  if (tid < S) win[tid] = windowed ? p.win[tid] : 1.f;
  const float scale = __uint_as_float((unsigned int)(127 - (8 + 2 * LG)) << 23);                     // 2^-(8 + 2 log2 S)
  bool first = true;
  for (long long i = blockIdx.x; i < p.n; i += gridDim.x, first = false) {
    const unsigned char* img = p.x + i * (3ll * S * S);
    // the picture's 3 S^2 bytes (a multiple of 4) as dwords into region Z: aligned loads whatever the address - dword j of the picture is
    // cut from the aligned dwords j and, at a byte offset, j + 1, both of which hold at least one byte of the picture
    const int off = (int)(reinterpret_cast<unsigned long long>(img) & 3);
    const unsigned int* src = reinterpret_cast<const unsigned int*>(img - off);
    unsigned int* raw = reinterpret_cast<unsigned int*>(Z);
    for (int j = tid; j < 3 * S * S / 4; j += SP_T) {
      unsigned int v = src[j];
      if (off) v = (v >> (8 * off)) | (src[j + 1] << (32 - 8 * off));
      raw[j] = v;
    }
    __syncthreads();
    int part_t = 0;
    const int pl = p.plane;
    auto value = [pl](unsigned int r, unsigned int g, unsigned int b) {
      return pl == 3 ? (int)(77u * r + 150u * g + 29u * b) : (int)(256u * (pl == 0 ? r : pl == 1 ? g : b));
    };
    for (int q = tid; q < S * S / 4; q += SP_T) {                       // four pixels = three dwords
      const unsigned int d0 = raw[3 * q], d1 = raw[3 * q + 1], d2 = raw[3 * q + 2];
      int4 y;
      y.x = value(d0 & 255u, (d0 >> 8) & 255u, (d0 >> 16) & 255u);
      y.y = value(d0 >> 24, d1 & 255u, (d1 >> 8) & 255u);
      y.z = value((d1 >> 16) & 255u, d1 >> 24, d2 & 255u);
      y.w = value((d2 >> 8) & 255u, (d2 >> 16) & 255u, d2 >> 24);
      *reinterpret_cast<int4*>(Yp + 4 * q) = y;
      part_t += (y.x + y.y) + (y.z + y.w);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) part_t += __shfl_xor(part_t, o, 64);
    if (lane == 0) red[wave] = part_t;
    __syncthreads();                                                  // the plane, the wave sums, the tables (first picture)
    int T = 0;
#pragma unroll
    for (int w = 0; w < SP_T / 64; ++w) T += red[w];
    if (tid == 0) p.mean[i] = __ddiv_rn((double)T, 256.0 * S * S);
    for (int e = tid; e < S * S; e += SP_T) {
      const int y = e >> LG, x = e & (S - 1);
      float v = __fmul_rn((float)(S * S * Yp[e] - T), scale);
      if (windowed) v = __fmul_rn(__fmul_rn(v, win[y]), win[x]);
      const int xr = (int)(__brev((unsigned int)x) >> (32 - LG));
      reinterpret_cast<float*>(Z)[((y >> 1) * ZS + xr) * 2 + (y & 1)] = v;
    }
    __syncthreads();
    sp_fft<S, S / 2, ZS, 1>(Z, tw, tid);
    for (int it = tid; it < (S / 2) * LD; it += SP_T) {
      const int k = it / LD, v = it - k * LD;
      const sp_c zv = Z[k * ZS + v], zm = Z[k * ZS + ((S - v) & (S - 1))];
      const int ra = (int)(__brev((unsigned int)(2 * k)) >> (32 - LG)), rb = (int)(__brev((unsigned int)(2 * k + 1)) >> (32 - LG));
      F[ra * LD + v] = sp_c{__fmul_rn(0.5f, __fadd_rn(zv.x, zm.x)), __fmul_rn(0.5f, __fsub_rn(zv.y, zm.y))};
      F[rb * LD + v] = sp_c{__fmul_rn(0.5f, __fadd_rn(zv.y, zm.y)), __fmul_rn(-0.5f, __fsub_rn(zv.x, zm.x))};
    }
    __syncthreads();
    sp_fft<S, LD, 1, LD>(F, tw, tid);
    for (int e = tid; e < S * LD; e += SP_T) {
      const int u = e / LD, v = e - u * LD;
      const bool edge = v == 0 || v == S / 2;
      const sp_c f = F[e];
      const double pe = __dmul_rn(__dadd_rn(__dmul_rn((double)f.x, (double)f.x), __dmul_rn((double)f.y, (double)f.y)), p.inv);
      if (!edge || u == 0 || u == S / 2) {
        Pw[e] = pe;
      } else if (u < S / 2) {                                         // the pair (u, S - u) of a self-mirrored column: one value for both
        const int m = (S - u) * LD + v;
        const sp_c g = F[m];
        const double pm = __dmul_rn(__dadd_rn(__dmul_rn((double)g.x, (double)g.x), __dmul_rn((double)g.y, (double)g.y)), p.inv);
        const double avg = __dmul_rn(0.5, __dadd_rn(pe, pm));
        Pw[e] = avg;
        Pw[m] = avg;
      }
    }
    __syncthreads();
    if (p.part) {
      double* mine = p.part + (long long)blockIdx.x * (S * LD);
      for (int e = tid; e < S * LD; e += SP_T) mine[e] = first ? Pw[e] : __dadd_rn(mine[e], Pw[e]);
    }
    double* prof = p.prof + i * R;
    for (int r = wave; r < R; r += SP_T / 64) {
      const int q1 = tab.off[r + 1];
      double acc = 0.0;
      for (int q = tab.off[r] + lane; q < q1; q += 64) {
        const unsigned int ent = tab.ent[q];
        const double v = Pw[ent & 0xffffu];
        acc = __dadd_rn(acc, (ent >> 16) ? __dadd_rn(v, v) : v);
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) acc = __dadd_rn(acc, __shfl_xor(acc, o, 64));
      if (lane == 0) prof[r] = __ddiv_rn(acc, (double)tab.cnt[r]);
    }
    __syncthreads();                                                  // the next picture overwrites the plane
  }
}

// mean2d[u][v] = (sum_g part[g][src]) / n, g ascending; src the half-plane point (u, v) or (S - u, S - v)
template <int S> __global__ __launch_bounds__(SP_T) void spectrum_mean_kernel(const double* __restrict__ part, int G, int n, double* __restrict__ out) {
#pragma clang fp contract(off)
  constexpr int LG = SpCfg<S>::LG, LD = SpCfg<S>::LD;
  const int e = (int)(blockIdx.x * SP_T + threadIdx.x);
  if (e >= S * S) return;
  const int u = e >> LG, v = e & (S - 1);
  const int src = v <= S / 2 ? u * LD + v : ((S - u) & (S - 1)) * LD + (S - v);
  double acc = part[src];
  for (int g = 1; g < G; ++g) acc = __dadd_rn(acc, part[(long long)g * (S * LD) + src]);
  out[e] = __ddiv_rn(acc, (double)n);
}

inline int sp_bins(int S) { return S == 32 ? 24 : S == 64 ? 46 : S == 128 ? 92 : 0; }
inline int sp_grid(int S) { return S == 32 ? SpCfg<32>::G : S == 64 ? SpCfg<64>::G : S == 128 ? SpCfg<128>::G : 0; }

inline int sp_bin_of(int u, int v, int S) {
  const int fu = std::min(u, S - u), fv = std::min(v, S - v), d2 = fu * fu + fv * fv;
  int r = 0;
  while (r * r + r < d2) ++r;
  return r;
}

template <int S> void sp_build(SpTab<S>& t) {
  constexpr int LD = SpCfg<S>::LD, R = SpCfg<S>::R;
  const double pi = 3.14159265358979323846;
  for (int m = 0; m < S / 2; ++m) {
    // exact at the multiples of a quarter turn, fp64 elsewhere: the rounding to fp32 leaves mu = 2^-24
    const double c = m == 0 ? 1.0 : 4 * m == S ? 0.0 : std::cos(2.0 * pi * m / S), s = m == 0 ? 0.0 : 4 * m == S ? 1.0 : std::sin(2.0 * pi * m / S);
    t.tw[m] = sp_c{(float)c, (float)-s};
  }
  std::vector<std::vector<unsigned int>> bins(R);
  for (int r = 0; r < R; ++r) t.cnt[r] = 0;
  for (int u = 0; u < S; ++u)
    for (int v = 0; v <= S / 2; ++v) {
      const bool edge = v == 0 || v == S / 2;
      if (edge && u > S / 2) continue;
      const bool twice = !edge || (u != 0 && u != S / 2);
      const int r = sp_bin_of(u, v, S);
      bins[r].push_back((unsigned int)(u * LD + v) | (twice ? 1u << 16 : 0u));
      t.cnt[r] += twice ? 2 : 1;
    }
  int q = 0;
  for (int r = 0; r < R; ++r) {
    t.off[r] = q;
    for (unsigned int e : bins[r]) t.ent[q++] = e;
  }
  t.off[R] = q;                                                       // = NC
}

// the raised dynamic-LDS limit of one instantiation, once (per device the attribute is set again: it belongs to the loaded code object)
template <auto KERN, class Params> int sp_launch_lds(dim3 grid, dim3 block, int lds, hipStream_t st, const Params& q, int dev) {
  static bool attr_done[64] = {};
  if (!attr_done[dev]) {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    attr_done[dev] = true;
  }
  hipLaunchKernelGGL(KERN, grid, block, lds, st, q);
  HIPCHK(hipGetLastError());
  return JCK_OK;
}

template <int S> int sp_upload(const void* symbol) {
  static SpTab<S> host;
  static bool built = false;
  if (!built) { sp_build<S>(host); built = true; }
  HIPCHK(hipMemcpyToSymbol(symbol, &host, sizeof(host)));
  return JCK_OK;
}

template <int S> int sp_run(const SpP& p, double* mean2d, hipStream_t st, int dev, const void* symbol) {
  static std::mutex mu;
  static bool ready[64] = {};
  {
    std::lock_guard<std::mutex> lock(mu);
    if (!ready[dev]) {
      JCK_TRY(sp_upload<S>(symbol));
      ready[dev] = true;
    }
    const int grid = p.part ? std::min(p.n, SpCfg<S>::G) : p.n;
    JCK_TRY((sp_launch_lds<spectrum_kernel<S>>(dim3((unsigned)grid), dim3(SpCfg<S>::T), SpCfg<S>::LDS_BYTES, st, p, dev)));
    if (p.part) {
      hipLaunchKernelGGL(spectrum_mean_kernel<S>, dim3((unsigned)(S * S / SP_T)), dim3(SP_T), 0, st, (const double*)p.part, grid, p.n, mean2d);
      HIPCHK(hipGetLastError());
    }
  }
  return JCK_OK;
}

}  // namespace

extern "C" int jck_spectrum_bins(int S) {
  const int R = sp_bins(S);
  if (R == 0) JCK_FAIL(JCK_E_ARG, "spectrum_bins: S must be 32, 64 or 128");
  return R;
}

extern "C" int jck_spectrum_grid(int S) {
  const int G = sp_grid(S);
  if (G == 0) JCK_FAIL(JCK_E_ARG, "spectrum_grid: S must be 32, 64 or 128");
  return G;
}

extern "C" size_t jck_spectrum_ws_bytes(int n, int S, int want_mean2d) {
  if (!want_mean2d || n < 1 || sp_grid(S) == 0) return 0;
  return (size_t)std::min(n, sp_grid(S)) * (size_t)S * (size_t)(S / 2 + 1) * sizeof(double);
}

extern "C" int jck_spectrum_u8(const unsigned char* x, int n, int S, int plane, const float* win, double win_power, double* prof, double* mean,
                               double* mean2d, void* ws, size_t ws_bytes, void* stream) {
  if (sp_bins(S) == 0) JCK_FAIL(JCK_E_ARG, "spectrum: S must be 32, 64 or 128");
  if (plane < 0 || plane > 3) JCK_FAIL(JCK_E_ARG, "spectrum: plane must be 0 (r), 1 (g), 2 (b) or 3 (luma)");
  if (n < 0) JCK_FAIL(JCK_E_ARG, "spectrum: n must be >= 0");
  if (!(win_power > 0.0) || !std::isfinite(win_power)) JCK_FAIL(JCK_E_ARG, "spectrum: win_power must be finite and positive");
  if (n == 0) return JCK_OK;
  if (!x || !prof || !mean) JCK_FAIL(JCK_E_ARG, "spectrum: null argument");
  const size_t need = jck_spectrum_ws_bytes(n, S, mean2d != nullptr);
  if (mean2d && (!ws || ws_bytes < need)) JCK_FAIL(JCK_E_ARG, "spectrum: the workspace is smaller than jck_spectrum_ws_bytes(n, S, 1)");
  if (mean2d && (reinterpret_cast<size_t>(ws) & 7)) JCK_FAIL(JCK_E_ARG, "spectrum: the workspace must be 8-byte aligned");
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64) JCK_FAIL(JCK_E_ARG, "spectrum: device index out of range");
  SpP p = {};
  p.x = x; p.win = win; p.prof = prof; p.mean = mean; p.part = mean2d ? static_cast<double*>(ws) : nullptr; p.n = n; p.plane = plane;
  p.inv = 1.0 / ((double)S * (double)S * win_power);
  const hipStream_t st = (hipStream_t)stream;
  if (S == 32) return sp_run<32>(p, mean2d, st, dev, &sp_tab32);
  if (S == 64) return sp_run<64>(p, mean2d, st, dev, &sp_tab64);
  return sp_run<128>(p, mean2d, st, dev, &sp_tab128);
}
