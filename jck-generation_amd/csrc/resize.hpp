// Device-resident input pipeline for any source size: Resize((S, S)) of a uint8 [3][Hs][Ws] image exactly as
// PIL.Image.resize(BILINEAR) does it - a horizontal, then a vertical pass of fixed-point taps (2^-22 units), EACH rounded to uint8 -,
// then ToTensor, Normalize(0.5, 0.5) and the instance-noise mix of img_prep_u8_kernel (ew.hpp), whose 2x special case this
// generalises.  The taps come from the host (jck_resize_taps_build in ops.hip: Pillow's double arithmetic in Pillow's order; layout
// in include/jckgan.h), so the kernel is integer arithmetic up to the uint8 value.
//
// One workgroup of 256 threads per (image, band of `band` output rows).  Stage 1: the horizontal pass of the source rows that the
// band's vertical taps touch, into LDS as uint8 [rows][3][S]; x = tid % S, so a wave walks a source row left to right and reads it
// contiguously (the mirror is applied in the address), and a thread keeps RESIZE_ROWS rows in flight per tap weight it loads.
// Stage 2, behind the one barrier: the vertical pass out of LDS.  A wave holds 64 neighbouring x of ONE output row, so a tap's
// weight is the same in every lane and its read is 64 consecutive bytes of one LDS row = 16 distinct dwords in 16 distinct banks,
// four lanes sharing each: no bank conflict at any row stride, no padding.  No atomics; an output row depends on its own image only.
//
// Both kernels are resize_band: the resize of the box of Hc x Wc source pixels whose top-left corner is (oy, ox) inside the Hs x Ws
// image, with the tap table of (Hc, Wc, S).  img_prep_u8_any_kernel is the whole image (Hc = Hs, Wc = Ws, corner 0, 0: the offsets
// fold away); img_prep_u8_box_kernel takes the box and one corner for all images or one per image, clamped into the image.
#pragma once
#include "common.hpp"
#include "philox.hpp"

constexpr int RESIZE_HDR = 8;            // header words of a tap table
constexpr int RESIZE_THREADS = 256;
constexpr int RESIZE_ROWS = 4;           // (source row, channel) items a thread accumulates per pass over its taps
constexpr int RESIZE_BAND = 16;          // output rows per workgroup (the launcher halves it while the LDS need exceeds 64 KiB)

__device__ __forceinline__ int resize_u8(int acc) { return min(max(acc >> 22, 0), 255); }

template <typename T>
__device__ __forceinline__ void resize_band(
    const unsigned char* __restrict__ data, const long long* __restrict__ idx, const unsigned char* __restrict__ flip,
    const float* __restrict__ noise, const unsigned* __restrict__ rng, unsigned rng_tensor, float keep, float mix,
    T* __restrict__ out_nhwc4, float* __restrict__ out_nchw, int Hs, int Ws, int Hc, int Wc, int oy, int ox, int S, int KX, int KY,
    int band, int max_rows, const int* __restrict__ taps) {
  extern __shared__ __attribute__((aligned(16))) unsigned char hrow[];      // [rows][3][S]: the band's source rows after the horizontal pass
  const int *xlo = taps + RESIZE_HDR, *xcnt = xlo + S, *xk = xcnt + S;
  const int *ylo = xk + KX * S, *ycnt = ylo + S, *yk = ycnt + S;
  const int bands = S / band;
  const long long n = blockIdx.x / bands;
  const int y0 = (int)(blockIdx.x % bands) * band;
  const int r0 = min(max(ylo[y0], 0), Hc - 1);
  const int nrows = min(min(max(ylo[y0 + band - 1] + ycnt[y0 + band - 1] - r0, 1), max_rows), Hc - r0);
  const int x = threadIdx.x % S, g = threadIdx.x / S, G = RESIZE_THREADS / S;
  const unsigned char* src = data + (idx ? idx[n] : n) * 3ll * Hs * Ws + (long long)oy * Ws + ox;      // the box's first pixel, channel 0
  const bool mirror = flip && flip[n];

  // ---- stage 1: horizontal pass of source rows r0 .. r0 + nrows - 1, three channels each ----
  {
    const int lo = xlo[x], cnt = min(xcnt[x], KX), items = nrows * 3;
    for (int base = g; base < items; base += G * RESIZE_ROWS) {
      const unsigned char* rp[RESIZE_ROWS];
      int acc[RESIZE_ROWS];
#pragma unroll
      for (int u = 0; u < RESIZE_ROWS; ++u) {
        const int it = min(base + u * G, items - 1), r = it / 3, c = it - 3 * r;
        rp[u] = src + ((long long)c * Hs + r0 + r) * Ws;
        acc[u] = 1 << 21;
      }
      for (int j = 0; j < cnt; ++j) {
        const int w = xk[j * S + x];
        int col = min(max(lo + j, 0), Wc - 1);
        if (mirror) col = Wc - 1 - col;                                // a flip mirrors inside the box
#pragma unroll
        for (int u = 0; u < RESIZE_ROWS; ++u) acc[u] += w * (int)rp[u][col];
      }
#pragma unroll
      for (int u = 0; u < RESIZE_ROWS; ++u) {
        const int it = base + u * G;
        if (it < items) hrow[it * S + x] = (unsigned char)resize_u8(acc[u]);
      }
    }
  }
  __syncthreads();

  // ---- stage 2: vertical pass out of LDS, normalise, noise, store ----
  const int H = S, W = S;
  for (int yy = g; yy < band; yy += G) {
    const int y = y0 + yy, lo = ylo[y] - r0, cnt = min(ycnt[y], KY);
    int acc[3] = {1 << 21, 1 << 21, 1 << 21};
    for (int j = 0; j < cnt; ++j) {
      const int w = yk[j * S + y];
      const unsigned char* p = hrow + min(max(lo + j, 0), nrows - 1) * 3 * S + x;
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] += w * (int)p[c * S];
    }
    const long long i = (n * H + y) * W + x;
    float v[4], nz[3] = {0.f, 0.f, 0.f};
    if (!noise && rng) pixel_normals(rng, rng_tensor, i, nz);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int u8 = resize_u8(acc[c]);
      const float t = ((float)u8 / 255.0f - 0.5f) / 0.5f;           // ToTensor, Normalize(0.5, 0.5): img_prep_u8_kernel's expression
      if (out_nchw) out_nchw[((n * 3 + c) * H + y) * W + x] = t;
      float o = __fmul_rn(keep, t);
      if (noise) o = __fmaf_rn(mix, noise[((n * 3 + c) * H + y) * W + x], o);
      else if (rng) o = __fmaf_rn(mix, nz[c], o);
      v[c] = o;
    }
    v[3] = 0.f;
    if (out_nhwc4) st4(out_nhwc4 + i * 4, v);
  }
}

template <typename T>
__global__ __launch_bounds__(RESIZE_THREADS) void img_prep_u8_any_kernel(
    const unsigned char* __restrict__ data, const long long* __restrict__ idx, const unsigned char* __restrict__ flip,
    const float* __restrict__ noise, const unsigned* __restrict__ rng, unsigned rng_tensor, float keep, float mix,
    T* __restrict__ out_nhwc4, float* __restrict__ out_nchw, int Hs, int Ws, int S, int KX, int KY, int band, int max_rows,
    unsigned magic, const int* __restrict__ taps) {
  // a table of another geometry (KX, KY are the launcher's own count for this one): nothing is read past it, nothing is written
  if ((unsigned)taps[0] != magic || taps[1] != Hs || taps[2] != Ws || taps[3] != S || taps[4] != KX || taps[5] != KY) return;
  resize_band<T>(data, idx, flip, noise, rng, rng_tensor, keep, mix, out_nhwc4, out_nchw, Hs, Ws, Hs, Ws, 0, 0, S, KX, KY, band, max_rows, taps);
}

// origin: int32 [B][2] = (y0, x0) per image, or NULL for the call's (oy, ox).  Nobody can check a device vector without a sync, so
// every corner is clamped to [0, Hs - Hc] x [0, Ws - Wc] here: no origin makes the kernel read outside its image.
template <typename T>
__global__ __launch_bounds__(RESIZE_THREADS) void img_prep_u8_box_kernel(
    const unsigned char* __restrict__ data, const long long* __restrict__ idx, const unsigned char* __restrict__ flip,
    const int* __restrict__ origin, const float* __restrict__ noise, const unsigned* __restrict__ rng, unsigned rng_tensor, float keep,
    float mix, T* __restrict__ out_nhwc4, float* __restrict__ out_nchw, int Hs, int Ws, int Hc, int Wc, int oy, int ox, int S, int KX,
    int KY, int band, int max_rows, unsigned magic, const int* __restrict__ taps) {
  if ((unsigned)taps[0] != magic || taps[1] != Hc || taps[2] != Wc || taps[3] != S || taps[4] != KX || taps[5] != KY) return;
  if (origin) {
    const long long n = blockIdx.x / (S / band);
    oy = origin[2 * n];
    ox = origin[2 * n + 1];
  }
  oy = min(max(oy, 0), Hs - Hc);
  ox = min(max(ox, 0), Ws - Wc);
  resize_band<T>(data, idx, flip, noise, rng, rng_tensor, keep, mix, out_nhwc4, out_nchw, Hs, Ws, Hc, Wc, oy, ox, S, KX, KY, band, max_rows, taps);
}
