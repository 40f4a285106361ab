// Memory-bound kernels of the DCGAN/CGAN step: layout conversion + instance noise, D head (4x4 valid conv to one
// logit + sigmoid + BCE with the -100 log clamp + gradient), tanh backward, gradient-penalty norm, the CGAN
// pieces (BatchNorm: bn.hpp, bn2.hpp; Adam and weight packing: ew_optim.hpp).  Everything is 16-byte vectorised along the NHWC channel axis; per-channel
// reductions use registers -> LDS -> per-workgroup partial rows summed in a fixed order (no float atomics anywhere:
// two runs of a step give bitwise identical gradients and scalars).
#pragma once
#include "common.hpp"
#include "philox.hpp"

// ------------------------------------------------------------------------------------------------------
// image prep: out[n][p][0..3] = keep * img[n][c][p] + mix * noise[n][c][p]   (NCHW f32 -> NHWC4 T)
// ------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void img_prep_kernel(const float* __restrict__ img, const float* __restrict__ noise, float keep, float mix,
                                T* __restrict__ out, int N, int HW, const unsigned* __restrict__ rng = nullptr, unsigned rng_tensor = 0) {
  const long long total = (long long)N * HW;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long n = i / HW;
    const int px = (int)(i - n * HW);
    float v[4], nz[3] = {0.f, 0.f, 0.f};
    if (rng) pixel_normals(rng, rng_tensor, i, nz);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const long long s = (n * 3 + c) * HW + px;
      float x = __fmul_rn(keep, img[s]);
      if (noise) x = __fmaf_rn(mix, noise[s], x);                  // explicit: the same rounding in every kernel that mixes noise
      else if (rng) x = __fmaf_rn(mix, nz[c], x);
      v[c] = x;
    }
    v[3] = 0.f;
    st4(out + i * 4, v);
  }
}

// Device-resident input pipeline: a uint8 dataset [Ntot][3][Hs][Ws] (the CIFAR pickle layout) stays in HBM and a batch is
// gathered by index and pushed through the reference's transform chain on the fly (preprocess/dcgan_data_preprocessor.py:
// 38-43): Resize(2x) as PIL does it for a bilinear upscale - horizontal pass, then vertical pass, EACH rounded to uint8 with
// the 3:1 / 1:3 weights (out = (3a + b + 2) >> 2; the clamped border taps reduce to a) -, ToTensor (/255),
// Normalize(0.5, 0.5), then the instance-noise mix of train/dcgan_trainer.py:160.  Bit-exact against PIL for the image
// (tests/golden/resize_u8.json).  out_nhwc4: [B][2Hs][2Ws][4] T (or nullptr); out_nchw: [B][3][2Hs][2Ws] fp32 transformed
// image WITHOUT noise (or nullptr).
__device__ __forceinline__ int up2_pil(int o, int L, int a_km1, int a_k, int a_kp1) {
  (void)L;
  return (o & 1) ? (3 * a_k + a_kp1 + 2) >> 2 : (a_km1 + 3 * a_k + 2) >> 2;
}
template <typename T>
__global__ void img_prep_u8_kernel(const unsigned char* __restrict__ data, const long long* __restrict__ idx,
                                   const float* __restrict__ noise, float keep, float mix, T* __restrict__ out_nhwc4,
                                   float* __restrict__ out_nchw, int B, int Hs, int Ws, const unsigned* __restrict__ rng = nullptr,
                                   unsigned rng_tensor = 0) {
  const int H = 2 * Hs, W = 2 * Ws;
  const long long total = (long long)B * H * W;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(i % W), y = (int)((i / W) % H);
    const long long n = i / ((long long)W * H);
    const unsigned char* src = data + (idx ? idx[n] : n) * 3ll * Hs * Ws;
    const int kx = x >> 1, ky = y >> 1;
    const int xm = max(kx - 1, 0), xp = min(kx + 1, Ws - 1), ym = max(ky - 1, 0), yp = min(ky + 1, Hs - 1);
    float v[4], nz[3] = {0.f, 0.f, 0.f};
    if (rng) pixel_normals(rng, rng_tensor, i, nz);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const unsigned char* pl = src + (long long)c * Hs * Ws;
      int hrow[3];                                                   // horizontal pass on source rows ym, ky, yp
      const int rows[3] = {ym, ky, yp};
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const unsigned char* row = pl + rows[r] * Ws;
        hrow[r] = up2_pil(x, Ws, row[xm], row[kx], row[xp]);
      }
      const int u8 = up2_pil(y, Hs, hrow[0], hrow[1], hrow[2]);
      const float t = ((float)u8 / 255.0f - 0.5f) / 0.5f;           // ToTensor, Normalize(0.5, 0.5)
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

// Evaluation branch (train/dcgan_trainer.py:202-206): fake = 0.5*fake + 0.5; F.resize(fake, [OH, OW]) (bilinear,
// align_corners = False: src = scale*(dst + 0.5) - 0.5 clamped at 0, as aten::upsample_bilinear2d computes it in fp32);
// (fake - mean[c]) / std[c].  One pass, NCHW fp32 in and out.
static __global__ void resize_norm_kernel(const float* __restrict__ in, float* __restrict__ out, int N, int C, int H, int W, int OH,
                                          int OW, float pre_scale, float pre_shift, const float* __restrict__ mean,
                                          const float* __restrict__ stdv) {
  const float sh = (float)H / (float)OH, sw = (float)W / (float)OW;
  const long long total = (long long)N * C * OH * OW;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int ox = (int)(i % OW), oy = (int)((i / OW) % OH);
    const long long nc = i / ((long long)OW * OH);
    const int c = (int)(nc % C);
    const float fy = fmaxf(sh * ((float)oy + 0.5f) - 0.5f, 0.f), fx = fmaxf(sw * ((float)ox + 0.5f) - 0.5f, 0.f);
    const int y0 = (int)fy, x0 = (int)fx;
    const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
    const float ly = fy - (float)y0, lx = fx - (float)x0, hy = 1.f - ly, hx = 1.f - lx;
    const float* p = in + nc * H * W;
    auto at = [&](int yy, int xx) { return __fmaf_rn(pre_scale, p[yy * W + xx], pre_shift); };
    const float top = __fmaf_rn(hx, at(y0, x0), __fmul_rn(lx, at(y0, x1)));
    const float bot = __fmaf_rn(hx, at(y1, x0), __fmul_rn(lx, at(y1, x1)));
    const float v = __fmaf_rn(hy, top, __fmul_rn(ly, bot));
    out[i] = (v - mean[c]) / stdv[c];
  }
}

// NHWC4 T -> NCHW f32 (module boundary)
template <typename T>
__global__ void nhwc4_to_nchw_kernel(const T* __restrict__ in, float* __restrict__ out, int N, int HW) {
  const long long total = (long long)N * HW;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long n = i / HW;
    const int px = (int)(i - n * HW);
    float v[4];
    ld4(in + i * 4, v);
#pragma unroll
    for (int c = 0; c < 3; ++c) out[(n * 3 + c) * HW + px] = v[c];
  }
}

// NHWC4 T in [-1, 1] (the tanh image) -> packed uint8 [N][HW][3]: u8 = (unsigned char)(min(max(x * 127.5 + 127.5, 0), 255) + 0.5),
// product and sum rounded separately in fp32.  NaN -> 0 (fmaxf returns its other operand).  Four pixels per thread: 16-byte loads,
// one 12-byte store.
template <typename T>
__global__ void img_to_u8_kernel(const T* __restrict__ in, unsigned char* __restrict__ out, long long total4) {
#pragma clang fp contract(off)
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total4; i += (long long)gridDim.x * blockDim.x) {
    float v[16];
    if constexpr (sizeof(T) == 2) {
      ld8(in + i * 16, reinterpret_cast<float(&)[8]>(v[0]));
      ld8(in + i * 16 + 8, reinterpret_cast<float(&)[8]>(v[8]));
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) ld4(in + i * 16 + k * 4, reinterpret_cast<float(&)[4]>(v[k * 4]));
    }
    unsigned w[3] = {0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      const float x = v[(k / 3) * 4 + k % 3];
      const unsigned b = (unsigned)(unsigned char)(fminf(fmaxf(x * 127.5f + 127.5f, 0.f), 255.f) + 0.5f);
      w[k >> 2] |= b << (8 * (k & 3));
    }
    struct alignas(4) U3 { unsigned a, b, c; };
    *reinterpret_cast<U3*>(out + i * 12) = U3{w[0], w[1], w[2]};
  }
}

// out = keep * x(NHWC4 T) + mix * noise(NCHW f32)
template <typename T>
__global__ void axpy_noise_kernel(const T* __restrict__ x, const float* __restrict__ noise, float keep, float mix,
                                  T* __restrict__ out, int N, int HW, const unsigned* __restrict__ rng = nullptr, unsigned rng_tensor = 0,
                                  const T* __restrict__ real = nullptr, const float* __restrict__ alpha = nullptr, T* __restrict__ xhat = nullptr) {
  // xhat != nullptr: the penalty's interpolate x_hat = alpha[n] * real + (1 - alpha[n]) * out in the same pass (interp_kernel's
  // arithmetic on the value as STORED in `out`: same bits as the two launches)
  const long long total = (long long)N * HW;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long n = i / HW;
    const int px = (int)(i - n * HW);
    float v[4], nz[3] = {0.f, 0.f, 0.f};
    ld4(x + i * 4, v);
    if (rng) pixel_normals(rng, rng_tensor, i, nz);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float r = keep * v[c];
      if (noise) r += mix * noise[(n * 3 + c) * HW + px];
      else if (rng) r += mix * nz[c];
      v[c] = r;
    }
    v[3] = 0.f;
    st4(out + i * 4, v);
    if (xhat) {
      const float al = alpha[n];
      float va[4], r[4];
      ld4(real + i * 4, va);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        T t;
        stf(&t, v[c]);
        r[c] = al * va[c] + ((1.f - al) * ldf(&t));
      }
      st4(xhat + i * 4, r);
    }
  }
}

// x_hat = alpha[n] * a + (1 - alpha[n]) * b        (NHWC4, train/dcgan_trainer.py:112)
template <typename T>
__global__ void interp_kernel(const T* __restrict__ a, const T* __restrict__ b, const float* __restrict__ alpha,
                              T* __restrict__ out, int N, int HW) {
  const long long total = (long long)N * HW;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const float al = alpha[i / HW];
    float va[4], vb[4], r[4];
    ld4(a + i * 4, va);
    ld4(b + i * 4, vb);
#pragma unroll
    for (int c = 0; c < 4; ++c) r[c] = al * va[c] + ((1.f - al) * vb[c]);
    st4(out + i * 4, r);
  }
}

// g_raw = scale * g * (1 - y^2)      (tanh backward fused with the 0.9 of the instance-noise mix)
template <typename T>
__global__ void tanh_bwd_kernel(const T* __restrict__ g, const T* __restrict__ y, float scale, T* __restrict__ out,
                                long long total4) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total4; i += (long long)gridDim.x * blockDim.x) {
    float vg[4], vy[4], r[4];
    ld4(g + i * 4, vg);
    ld4(y + i * 4, vy);
#pragma unroll
    for (int c = 0; c < 4; ++c) r[c] = scale * vg[c] * (1.f - vy[c] * vy[c]);
    st4(out + i * 4, r);
  }
}

// gradient penalty: (||g[n]||_2 - 1)^2 -> scal[slot][n]      one workgroup per image
// scal: per-image accumulator table [slots][scal_ld] - image n writes scal[slot*scal_ld + n] (plain store; the step tail
// sums the rows in a fixed order, so the logged scalars are bitwise reproducible)
template <typename T>
__global__ __launch_bounds__(256) void gp_norm_kernel(const T* __restrict__ g, int per_image4, float* __restrict__ scal,
                                                      int slot, int scal_ld, float* __restrict__ norms) {
  __shared__ float sm[4];
  const T* p = g + (long long)blockIdx.x * per_image4 * 4;
  float s = 0.f;
  for (int i = threadIdx.x; i < per_image4; i += 256) {
    float v[4];
    ld4(p + i * 4, v);
    s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
  }
  s = block_sum256(s, sm);
  if (threadIdx.x == 0) {
    const float nr = sqrtf(s);
    if (norms) norms[blockIdx.x] = nr;
    if (scal && slot >= 0) scal[(long long)slot * scal_ld + blockIdx.x] = (nr - 1.f) * (nr - 1.f);
  }
}

// ------------------------------------------------------------------------------------------------------
// D head: logit[n] = <a4[n,:], w[:]>,  p = sigmoid, BCE(p, t) with the -100 clamp, ds = dL/dlogit
//   mode 0: loss = mean BCE;  dp = (p - t) / max(p(1-p), 1e-12) / B;  ds = dp * p(1-p)      (ATen formulas)
//   mode 1: gradient-penalty pass, grad_outputs = ones:          ds = p(1-p)
// ------------------------------------------------------------------------------------------------------
// Several batches stacked row-wise (the real | fake | penalty groups of the batched D pass) go through ONE launch: group
// g = row / rows_per_group has its own target, mode and scalar slots; prob / ds are indexed by the stacked row, the scalar table
// by the row inside the group.
struct HeadGroups { float target[4]; int mode[4], slot_loss[4], slot_p[4]; int rows_per_group; };
template <typename T>
__global__ __launch_bounds__(256) void head_fwd_kernel(const T* __restrict__ a4, const float* __restrict__ w, int K,
                                                       const float* __restrict__ bias, const HeadGroups hg, float invB,
                                                       float* __restrict__ prob, float* __restrict__ ds,
                                                       float* __restrict__ scal, int scal_ld, T* __restrict__ g_out = nullptr) {
  // g_out (optional): the input gradient of the row, g_out[n][k] = ds[n] * w[k] (head_bwd_fused_kernel's / head_dgrad_kernel's
  // product), written by the workgroup that has just formed ds[n] - one launch less on the step's serial chain
  __shared__ float sm[4];
  __shared__ float sds;
  const int grp = blockIdx.x / hg.rows_per_group, nrow = blockIdx.x - grp * hg.rows_per_group;
  const float target = hg.target[grp];
  const int mode = hg.mode[grp], slot_loss = hg.slot_loss[grp], slot_p = hg.slot_p[grp];
  const T* x = a4 + (long long)blockIdx.x * K;
  float s = 0.f;
  for (int i = threadIdx.x * 8; i < K; i += 256 * 8) {
    float v[8];
    ld8(x + i, v);
    const f32x4 w0 = *reinterpret_cast<const f32x4*>(w + i), w1 = *reinterpret_cast<const f32x4*>(w + i + 4);
#pragma unroll
    for (int k = 0; k < 4; ++k) s += v[k] * w0[k] + v[4 + k] * w1[k];
  }
  s = block_sum256(s, sm);
  if (threadIdx.x == 0) {
    if (bias) s += bias[0];
    const float p = 1.f / (1.f + expf(-s));
    prob[blockIdx.x] = p;
    const float pq = p * (1.f - p);
    if (mode == 0) {
      const float lp = fmaxf(logf(p), -100.f), lq = fmaxf(logf(1.f - p), -100.f);
      const float loss = -(target * lp + (1.f - target) * lq);
      const float dp = (p - target) / fmaxf(pq, 1e-12f) * invB;
      sds = dp * pq;
      if (slot_loss >= 0) scal[(long long)slot_loss * scal_ld + nrow] = loss;
    } else {
      sds = pq;
    }
    ds[blockIdx.x] = sds;
    if (slot_p >= 0) scal[(long long)slot_p * scal_ld + nrow] = p;
  }
  if (!g_out) return;
  __syncthreads();
  const float d = sds;
  T* gr = g_out + (long long)blockIdx.x * K;
  for (int i = threadIdx.x * 8; i < K; i += 256 * 8) {
    const f32x4 w0 = *reinterpret_cast<const f32x4*>(w + i), w1 = *reinterpret_cast<const f32x4*>(w + i + 4);
    float o[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) { o[k] = d * w0[k]; o[4 + k] = d * w1[k]; }
    st8(gr + i, o);
  }
}

// D head at inference (jck_engine_score): logit[n] = <x[n,:], w> (+ bias), prob[n] = sigmoid(logit) - head_fwd_kernel's dot product and
// sigmoid without loss, gradient or scalar slots.  One workgroup per row, a fixed-order reduction, no atomics: a row's numbers do not
// depend on the rows beside it.
template <typename T>
__global__ __launch_bounds__(256) void score_head_kernel(const T* __restrict__ x, const float* __restrict__ w, int K, const float* __restrict__ bias,
                                                         float* __restrict__ logit, float* __restrict__ prob) {
  __shared__ float sm[4];
  const T* xr = x + (long long)blockIdx.x * K;
  float s = 0.f;
  for (int i = threadIdx.x * 8; i < K; i += 256 * 8) {
    float v[8];
    ld8(xr + i, v);
    const f32x4 w0 = *reinterpret_cast<const f32x4*>(w + i), w1 = *reinterpret_cast<const f32x4*>(w + i + 4);
#pragma unroll
    for (int k = 0; k < 4; ++k) s += v[k] * w0[k] + v[4 + k] * w1[k];
  }
  s = block_sum256(s, sm);
  if (threadIdx.x == 0) {
    if (bias) s += bias[0];
    logit[blockIdx.x] = s;
    if (prob) prob[blockIdx.x] = 1.f / (1.f + expf(-s));
  }
}

// Discriminator features (jck_grid_pool): an NHWC activation a [N][H][H][C] pooled to a grid x grid raster of w x w windows (w = H / grid),
// as fp32 in the activation's own order - cell-major, channel-minor: out[b * ld + col0 + (gy * grid + gx) * C + c].  mode 0: the
// window's maximum, a NaN in the window giving NaN (as aten's max_pool2d); mode 1: the fp32 sum in row-major window order times
// 1 / w^2.  One lane per (image, cell, 16 bytes of channels): a 16-byte load per window element, 16-byte stores, neighbouring lanes
// on neighbouring channels for both.  No LDS, no atomics: an output row depends on its own image alone.  Launched in workgroups of one
// wave: the shallow stage of a small batch has few lanes with long windows, and one-wave groups spread them over all CUs.
template <typename T>
__global__ __launch_bounds__(256) void grid_pool_kernel(const T* __restrict__ a, int H, int C, int grid, int mode, float* __restrict__ out,
                                                        long long ld, long long col0, long long total) {
  constexpr int V = 16 / (int)sizeof(T);                             // channels per lane: 8 (bf16) or 4 (fp32)
  const int w = H / grid, cu = C / V, cells = grid * grid;
  const float inv = 1.0f / (float)(w * w);
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int u = (int)(i % cu);
    const int cell = (int)((i / cu) % cells);
    const long long b = i / ((long long)cu * cells);
    const int gy = cell / grid, gx = cell - gy * grid;
    const T* p = a + ((b * H + (long long)gy * w) * H + (long long)gx * w) * C + u * V;
    float r[V];
#pragma unroll
    for (int k = 0; k < V; ++k) r[k] = mode == 0 ? -INFINITY : 0.f;
    for (int dy = 0; dy < w; ++dy) {
      const T* q = p + (long long)dy * H * C;
#pragma unroll 4                                                    // four loads of a window row in flight; the order of the sum is kept
      for (int dx = 0; dx < w; ++dx) {
        float v[V];
        if constexpr (V == 8) ld8(q + (long long)dx * C, v); else ld4(q + (long long)dx * C, v);
#pragma unroll
        for (int k = 0; k < V; ++k) r[k] = mode == 0 ? ((v[k] > r[k] || v[k] != v[k]) ? v[k] : r[k]) : __fadd_rn(r[k], v[k]);
      }
    }
    if (mode == 1) {
#pragma unroll
      for (int k = 0; k < V; ++k) r[k] = __fmul_rn(r[k], inv);
    }
    float* o = out + b * ld + col0 + (long long)cell * C + u * V;
    if constexpr (V == 8) st8(o, r); else st4(o, r);
  }
}

// g_a4[n][k] = ds[n] * w[k]
template <typename T>
__global__ void head_dgrad_kernel(const float* __restrict__ ds, const float* __restrict__ w, int K, T* __restrict__ g,
                                  long long total8) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total8; i += (long long)gridDim.x * blockDim.x) {
    const long long e = i * 8;
    const int k = (int)(e % K);
    const float d = ds[e / K];
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = d * w[k + j];
    st8(g + e, v);
  }
}

// part[y][k] = sum over this workgroup's images of ds[n] * a4[n][k]       (packed (h,w,c) order)
// grid (K/8/64, NS): 64 column units x 4 image lanes per workgroup, images strided over lanes and gridDim.y; the NS
// partial rows are summed in order by head_part_reduce_kernel (no float atomics: bitwise reproducible)
template <typename T>
__global__ __launch_bounds__(256) void head_wgrad_kernel(const float* __restrict__ ds, const T* __restrict__ a4, int B, int K,
                                                         float* __restrict__ part) {
  __shared__ float red[4][64][9];
  const int u = threadIdx.x & 63, ln = threadIdx.x >> 6;
  const int k = (blockIdx.x * 64 + u) * 8;
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (k < K)
    for (int n = blockIdx.y * 4 + ln; n < B; n += gridDim.y * 4) {
      float v[8];
      ld8(a4 + (long long)n * K + k, v);
      const float d = ds[n];
#pragma unroll
      for (int j = 0; j < 8; ++j) s[j] += d * v[j];
    }
#pragma unroll
  for (int j = 0; j < 8; ++j) red[ln][u][j] = s[j];
  __syncthreads();
  if (ln == 0 && k < K) {
    float o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (red[0][u][j] + red[1][u][j]) + (red[2][u][j] + red[3][u][j]);
    st8(part + (long long)blockIdx.y * K + k, o);
  }
}

// out (+)= sum_y part[y][k], y in order.  C == 0: out[k] (packed order, `accumulate` selects = / +=);  C > 0: the PyTorch
// layout of a [1][C][4][4] conv weight gradient, out[c*16 + t] += sum_y part[y][t*C + c]
static __global__ void head_part_reduce_kernel(const float* __restrict__ part, int NS, int K, int C, float* __restrict__ out,
                                               int accumulate) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  float s = 0.f;
  for (int y = 0; y < NS; ++y) s += part[(long long)y * K + k];
  if (C > 0) { const int t = k / C, c = k % C; out[c * 16 + t] += s; }
  else out[k] = accumulate ? out[k] + s : s;
}

// D.conv5 backward in one launch: g_a4[n][k] = ds[n] * w[k] and the partial weight-gradient rows
// part[y][k] = sum_{n of workgroup row y} ds[n] * a4[n][k]  (k = t*C + c is the packed (h,w,c) order); head_part_reduce_kernel
// sums the rows in order into the PyTorch-layout gradient.  grid (K/8/64, NS): 64 column units x 4 image lanes per workgroup.
template <typename T>
__global__ __launch_bounds__(256) void head_bwd_fused_kernel(const float* __restrict__ ds, const float* __restrict__ w,
                                                             const T* __restrict__ a4, int B, int K, int C,
                                                             T* __restrict__ g, float* __restrict__ grad, int Bmore = 0) {
  // Bmore: rows [B, B + Bmore) that only get their input gradient (the penalty group behind the loss groups of the batched D
  // pass): one launch for both; the rows < B meet the same lanes in the same order, so the partial sums keep their bits
  __shared__ float red[4][64][9];
  const int u = threadIdx.x & 63, ln = threadIdx.x >> 6;
  const int k = (blockIdx.x * 64 + u) * 8;
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (k < K) {
    float wv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) wv[j] = w[k + j];
    for (int n = blockIdx.y * 4 + ln; n < B + Bmore; n += gridDim.y * 4) {
      const float d = ds[n];
      if (grad && n < B) {
        float v[8];
        ld8(a4 + (long long)n * K + k, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) s[j] += d * v[j];
      }
      if (g) {
        float o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = d * wv[j];
        st8(g + (long long)n * K + k, o);
      }
    }
  }
  if (!grad) return;
#pragma unroll
  for (int j = 0; j < 8; ++j) red[ln][u][j] = s[j];
  __syncthreads();
  if (ln == 0 && k < K) {
    float o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (red[0][u][j] + red[1][u][j]) + (red[2][u][j] + red[3][u][j]);
    st8(grad + (long long)blockIdx.y * K + k, o);          // `grad` is the partial buffer [NS][K] here
  }
}

// ------------------------------------------------------------------------------------------------------
// CGAN pieces (model/CGAN.py:79-162): Linear layers as GEMM operands, label embedding, concat, dropout, GP gradient
// ------------------------------------------------------------------------------------------------------
// nn.Linear weight [N][K] fp32 -> wp[row][col] of type W:
//   transpose = 0: wp[n][k'] (forward operand, rows padded to NPad, K padded to KPad)
//   transpose = 1: wp[k'][n] (dgrad operand, rows padded to KRows, columns padded to NPadK)
// k' is the position in OUR activation order: the first hw*C columns of the reference are (c, hw) (NCHW flatten,
// model/CGAN.py:119-120), ours are (hw, c) (NHWC); columns >= hw*C (the label embedding) keep their place.
template <typename W>
__global__ void pack_linear_kernel(const float* __restrict__ w, int N, int K, int rows, int cols, int transpose, int permC,
                                   int permHW, W* __restrict__ wp) {
  const long long total = (long long)rows * cols;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int r = (int)(i / cols), c = (int)(i % cols);
    const int n = transpose ? c : r, kp = transpose ? r : c;
    float v = 0.f;
    if (n < N && kp < K) {
      int k = kp;
      if (permC > 0 && kp < permC * permHW) { const int hw = kp / permC, ch = kp % permC; k = ch * permHW + hw; }
      v = w[(long long)n * K + k];
    }
    stf(wp + i, v);
  }
}

// both layouts of one nn.Linear weight in ONE launch: blockIdx.y = 0 the forward operand wp0[rows0][cols0], 1 the dgrad operand
// wp1[rows1][cols1] (pack_linear_kernel with transpose = blockIdx.y)
template <typename W>
__global__ void pack_linear_pair_kernel(const float* __restrict__ w, int N, int K, int rows0, int cols0, W* __restrict__ wp0, int rows1,
                                        int cols1, W* __restrict__ wp1, int permC, int permHW) {
  const int transpose = blockIdx.y;
  const int rows = transpose ? rows1 : rows0, cols = transpose ? cols1 : cols0;
  W* wp = transpose ? wp1 : wp0;
  const long long total = (long long)rows * cols;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int r = (int)(i / cols), c = (int)(i % cols);
    const int n = transpose ? c : r, kp = transpose ? r : c;
    float v = 0.f;
    if (n < N && kp < K) {
      int k = kp;
      if (permC > 0 && kp < permC * permHW) { const int hw = kp / permC, ch = kp % permC; k = ch * permHW + hw; }
      v = w[(long long)n * K + k];
    }
    stf(wp + i, v);
  }
}

// grad[n][k] (+)= gp[n][k'] with the same column permutation (k' -> k) as pack_linear_kernel
static __global__ void unperm_linear_grad_kernel(const float* __restrict__ gp, int N, int K, int ldp, int permC, int permHW,
                                                 float* __restrict__ grad, int accumulate) {
  const long long total = (long long)N * K;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int n = (int)(i / K), k = (int)(i % K);
    int kp = k;
    if (permC > 0 && k < permC * permHW) { const int ch = k / permHW, hw = k % permHW; kp = hw * permC + ch; }
    const float v = gp[(long long)n * ldp + kp];
    grad[i] = accumulate ? grad[i] + v : v;
  }
}

// label embedding: e[b][j] = lrelu(sum_i W[j][i] * onehot[b][i] + bias[j])   (model/CGAN.py:83-84,111)
// labels: int64 one-hot [B][100] as the reference feeds them (preprocess/cgan_data_preprocessor.py:11-16)
template <typename T>
__global__ void label_embed_fwd_kernel(const long long* __restrict__ labels, const float* __restrict__ W,
                                       const float* __restrict__ bias, float slope, int B, int NI, int NO, T* __restrict__ cbuf,
                                       int ld, int col0, float* __restrict__ pre, int label_period = 0) {
  // one workgroup per image: the label row goes to LDS once; its zeros (99 of 100 for a one-hot row) are skipped - a
  // workgroup-uniform branch, and adding an exact 0 * W changes nothing
  extern __shared__ float lab[];                      // [NI]
  const int b = blockIdx.x;
  const int lb = label_period > 0 ? b % label_period : b;       // rows of several batches that share one label tensor
  for (int k = threadIdx.x; k < NI; k += blockDim.x) lab[k] = (float)labels[(long long)lb * NI + k];
  __syncthreads();
  for (int j = threadIdx.x; j < NO; j += blockDim.x) {
    float s = bias[j];
    for (int k = 0; k < NI; ++k) {
      const float l = lab[k];
      if (l != 0.f) s += W[j * NI + k] * l;
    }
    if (pre) pre[b * NO + j] = s;
    stf(cbuf + (long long)b * ld + col0 + j, s > 0.f ? s : slope * s);
  }
}
// dW[j][i] += sum_b ue[b][j]*act'(pre) * onehot[b][i];  db[j] += sum_b ...      ue taken from gc[b][col0 + j] (type T)
// One workgroup per label column i (threads over the output units j; workgroup NI sums the bias gradient): the label
// labels[b][i] is the same for the whole workgroup, so rows with a zero label - all but ~B/NI of them for one-hot labels -
// are skipped by a uniform branch, and the masked gradient row is read contiguously along j.  (One thread per (j, i)
// looping over b took 116 us at B = 256, one workgroup per j 32 us.)
template <typename T>
__global__ __launch_bounds__(256) void label_embed_bwd_kernel(const T* __restrict__ gc, int ld, int col0, const float* __restrict__ pre,
                                                              const long long* __restrict__ labels, float slope, int B, int NI,
                                                              int NO, float* __restrict__ dW, float* __restrict__ db, int label_period = 0) {
  extern __shared__ float lcol[];                     // [B]: this label column, fetched by all threads at once
  const int i = blockIdx.x;
  if (i >= NI) {
    // bias gradient: workgroups NI.. take 16 units each, 16 row lanes per unit with four rows in flight, LDS reduce in lane order
    // (every row contributes).  Round 2's 64 units x 4 lanes walked B / 4 rows one dependent load pair at a time: 37 us of the
    // kernel's 37 at 512 rows.
    __shared__ float red[16][16];
    const int jl = threadIdx.x & 15, ln = threadIdx.x >> 4, j = (i - NI) * 16 + jl;
    float s = 0.f;
    if (j < NO) {
      auto term = [&](int b) { return ldf(gc + (long long)b * ld + col0 + j) * (pre[b * NO + j] > 0.f ? 1.f : slope); };
      int b = ln;
      for (; b + 48 < B; b += 64) {
        const float v0 = term(b), v1 = term(b + 16), v2 = term(b + 32), v3 = term(b + 48);
        s += v0; s += v1; s += v2; s += v3;
      }
      for (; b < B; b += 16) s += term(b);
    }
    red[ln][jl] = s;
    __syncthreads();
    if (ln == 0 && j < NO) {
      float t = 0.f;
#pragma unroll
      for (int k = 0; k < 16; ++k) t += red[k][jl];
      db[j] += t;
    }
    return;
  }
  __shared__ int nnz;
  int* rows = reinterpret_cast<int*>(lcol + B);       // [B]: indices of the rows with a non-zero label, in order
  for (int b = threadIdx.x; b < B; b += blockDim.x) lcol[b] = (float)labels[(long long)(label_period > 0 ? b % label_period : b) * NI + i];
  if (threadIdx.x == 0) nnz = 0;
  __syncthreads();
  // ordered compaction (deterministic summation order) by wavefront ballots, 256 rows per round; a serial loop of one thread
  // over B LDS words was half of this kernel's 21 us
  __shared__ int wcnt[4];
  for (int b0 = 0; b0 < B; b0 += 256) {
    const int b = b0 + (int)threadIdx.x;
    const bool hit = b < B && lcol[b] != 0.f;
    const unsigned long long m = __ballot(hit);
    const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
    if (ln == 0) wcnt[wv] = __popcll(m);
    __syncthreads();
    int off = nnz;
    for (int w2 = 0; w2 < wv; ++w2) off += wcnt[w2];
    if (hit) rows[off + __popcll(m & ((1ull << ln) - 1ull))] = b;
    __syncthreads();
    if (threadIdx.x == 0) nnz += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    __syncthreads();
  }
  const int n = nnz;
  for (int j = threadIdx.x; j < NO; j += blockDim.x) {
    float s = 0.f;
#pragma unroll 4
    for (int k = 0; k < n; ++k) {                     // no branch: the loads of several rows are in flight together
      const int b = rows[k];
      s += lcol[b] * (ldf(gc + (long long)b * ld + col0 + j) * (pre[b * NO + j] > 0.f ? 1.f : slope));
    }
    dW[j * NI + i] += s;
  }
}

// cbuf[b][0..K0) = a4[b][0..K0)  (columns [K0, ld) are written by the label embedding / keep the zeros of the buffer's owner: jck_engine_bind
// for the engine's cbuf / cbuf2, infer_alloc for the scoring group's)
template <typename T>
__global__ void concat_rows_kernel(const T* __restrict__ a4, int K0, T* __restrict__ cbuf, int ld, long long total8) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total8; i += (long long)gridDim.x * blockDim.x) {
    const long long e = i * 8;
    const long long b = e / K0;
    const int k = (int)(e % K0);
    *reinterpret_cast<Raw8<T>*>(cbuf + b * ld + k) = *reinterpret_cast<const Raw8<T>*>(a4 + e);
  }
}
// the reverse: a4-shaped gradient out of the first K0 columns
template <typename T>
__global__ void split_rows_kernel(const T* __restrict__ gc, int ld, int K0, T* __restrict__ ga4, long long total8) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total8; i += (long long)gridDim.x * blockDim.x) {
    const long long e = i * 8;
    const long long b = e / K0;
    const int k = (int)(e % K0);
    *reinterpret_cast<Raw8<T>*>(ga4 + e) = *reinterpret_cast<const Raw8<T>*>(gc + b * ld + k);
  }
}

// y = x * mask * scale   (nn.Dropout(0.25) forward and backward: model/CGAN.py:105,122; mask in {0,1}, scale = 1/(1-p))
template <typename T>
__global__ void dropout_kernel(const T* __restrict__ x, const float* __restrict__ mask, float scale, T* __restrict__ y,
                               long long n) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    stf(y + i, ldf(x + i) * mask[i] * scale);
}

// column sums of a [B][N] matrix of T into fp32 (bias gradients): db[j] += sum_b g[b][j].  16 columns x 16 row lanes per
// workgroup, four rows in flight per thread, LDS reduce over the lanes in lane order (deterministic).  (Round 2: 64 columns x 4
// lanes, one row in flight - 128 dependent load round trips for the 512 rows of CGAN's batched head, 21 us.)
#define COLSUM_COLS 16
template <typename T>
__global__ __launch_bounds__(256) void colsum_kernel(const T* __restrict__ g, int B, int N, int ld, float* __restrict__ db) {
  __shared__ float red[16][COLSUM_COLS];
  const int jl = threadIdx.x & 15, ln = threadIdx.x >> 4, j = blockIdx.x * COLSUM_COLS + jl;
  float s = 0.f;
  if (j < N) {
    int b = ln;
    for (; b + 48 < B; b += 64) {
      const float v0 = ldf(g + (long long)b * ld + j), v1 = ldf(g + (long long)(b + 16) * ld + j);
      const float v2 = ldf(g + (long long)(b + 32) * ld + j), v3 = ldf(g + (long long)(b + 48) * ld + j);
      s += v0; s += v1; s += v2; s += v3;
    }
    for (; b < B; b += 16) s += ldf(g + (long long)b * ld + j);
  }
  red[ln][jl] = s;
  __syncthreads();
  if (ln == 0 && j < N) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += red[k][jl];
    db[j] += t;
  }
}

// u = coef * (norm - 1) / norm * g      gradient of  lambda * mean_n (||g_n|| - 1)^2  w.r.t. g  (coef = 2*lambda/B)
template <typename T>
__global__ void gp_grad_kernel(const T* __restrict__ g, const float* __restrict__ norms, float coef, int per_image,
                               T* __restrict__ u, long long total4) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total4; i += (long long)gridDim.x * blockDim.x) {
    const float nr = norms[(i * 4) / per_image];
    const float f = nr > 0.f ? coef * (nr - 1.f) / nr : 0.f;
    float v[4];
    ld4(g + i * 4, v);
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] *= f;
    st4(u + i * 4, v);
  }
}

// second-order head terms of the penalty (see tests/test_gp_double_backward_math.py):
//   uds[n] = <ughd[n,:], w2>;  rs[n] = uds * (1-2p) * p(1-p);  dw2[j] += sum_n ds[n] * ughd[n][j]     (ds = p(1-p))
// (the dw2 sum is formed afterwards by head_wgrad_kernel + head_part_reduce_kernel from pq[n] = ds[n]: no atomics)
template <typename T>
__global__ __launch_bounds__(256) void gp_head2_kernel(const T* __restrict__ ughd, const float* __restrict__ w2,
                                                       const float* __restrict__ prob, int B, int K, float* __restrict__ rs,
                                                       float* __restrict__ pq_out) {
  __shared__ float sm[4];
  const int n = blockIdx.x;
  float s = 0.f;
  for (int j = threadIdx.x; j < K; j += 256) s += ldf(ughd + (long long)n * K + j) * w2[j];
  s = block_sum256(s, sm);
  if (threadIdx.x == 0) {
    const float p = prob[n], pq = p * (1.f - p);
    rs[n] = s * (1.f - 2.f * p) * pq;
    pq_out[n] = pq;
  }
}

// DCGAN head step of the penalty's double backward (conv5 = one dot product per image, K = 16*C; tests/test_dcgan_gp_math.py):
//   rows:    rs[n] = <v4[n,:], w5> * (1-2p) * p(1-p),  sn[n] = p(1-p)          (one workgroup per row, as head_fwd_kernel)
//   columns: g_a4[n][k] = rs[n] * w5[k]  and  grad[c][t] += sum_n sn[n] v4[n][k] + rs[n] a4[n][k]   (k = t*C + c)
// The column launch reads v4[n][k] before it writes g_a4[n][k] from the same thread: g_a4 may BE v4 (the engine's reverse sweep
// starts in place from the v-chain's last buffer).
template <typename T>
__global__ __launch_bounds__(256) void dcgan_gp_head_rows_kernel(const T* __restrict__ v4, const float* __restrict__ w, int K,
                                                                 const float* __restrict__ prob, float* __restrict__ rs,
                                                                 float* __restrict__ sn) {
  __shared__ float sm[4];
  const T* x = v4 + (long long)blockIdx.x * K;
  float s = 0.f;
  for (int i = threadIdx.x * 8; i < K; i += 256 * 8) {
    float v[8];
    ld8(x + i, v);
    const f32x4 w0 = *reinterpret_cast<const f32x4*>(w + i), w1 = *reinterpret_cast<const f32x4*>(w + i + 4);
#pragma unroll
    for (int k = 0; k < 4; ++k) s += v[k] * w0[k] + v[4 + k] * w1[k];
  }
  s = block_sum256(s, sm);
  if (threadIdx.x == 0) {
    const float p = prob[blockIdx.x], pq = p * (1.f - p);
    rs[blockIdx.x] = s * (1.f - 2.f * p) * pq;
    sn[blockIdx.x] = pq;
  }
}

// grid (cdiv(K/8, GP_HEAD_CU)): GP_HEAD_CU column units of 8 columns x GP_HEAD_RL row lanes per workgroup; a workgroup owns its
// columns over ALL rows, so the weight term needs no cross-workgroup sum: the row lanes' partial sums are added in lane order
// (deterministic, no atomics).  grad == nullptr: g_a4 only.
#define GP_HEAD_CU 8
#define GP_HEAD_RL 32
template <typename T>
__global__ __launch_bounds__(256) void dcgan_gp_head_cols_kernel(const T* v4, const T* __restrict__ a4, const float* __restrict__ w,
                                                                 const float* __restrict__ rs, const float* __restrict__ sn, int B,
                                                                 int K, int C, T* g_a4, float* __restrict__ grad) {
  __shared__ float red[GP_HEAD_RL][GP_HEAD_CU * 8 + 1];
  const int u = threadIdx.x % GP_HEAD_CU, ln = threadIdx.x / GP_HEAD_CU;
  const int k = (blockIdx.x * GP_HEAD_CU + u) * 8;
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (k < K) {
    float wv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) wv[j] = w[k + j];
    for (int n = ln; n < B; n += GP_HEAD_RL) {
      const long long o = (long long)n * K + k;
      float v[8], a[8];
      ld8(v4 + o, v);
      ld8(a4 + o, a);
      const float r = rs[n], q = sn[n];
#pragma unroll
      for (int j = 0; j < 8; ++j) s[j] += q * v[j] + r * a[j];
      if (g_a4) {
        float g[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) g[j] = r * wv[j];
        st8(g_a4 + o, g);
      }
    }
  }
  if (!grad) return;
#pragma unroll
  for (int j = 0; j < 8; ++j) red[ln][u * 8 + j] = s[j];
  __syncthreads();
  if (threadIdx.x < GP_HEAD_CU * 8) {
    const int kk = blockIdx.x * GP_HEAD_CU * 8 + threadIdx.x;
    if (kk < K) {
      float t = 0.f;
      for (int l = 0; l < GP_HEAD_RL; ++l) t += red[l][threadIdx.x];
      const int tt = kk / C, c = kk - tt * C;
      grad[c * 16 + tt] += t;
    }
  }
}

// The same stretch of the penalty's double backward as ONE launch, one workgroup per row of 256 columns (thread = column):
// linear_finish_kernel (split-K sum of the v-chain's Linear product, Dropout) -> ughd, gp_head2_kernel (rs, pq), head_dgrad_kernel
// (g_hd = rs * w2) and the Dropout backward (g_h) - the arithmetic and the rounding points of the four launches.
template <typename T>
__global__ __launch_bounds__(256) void cg_gp_head_mid_kernel(const float* __restrict__ slab, int Z, long long zstride, const float* __restrict__ mask,
                                                             float scale, T* __restrict__ ughd, const float* __restrict__ w2,
                                                             const float* __restrict__ prob, float* __restrict__ rs, float* __restrict__ pq_out,
                                                             T* __restrict__ g_hd, T* __restrict__ g_h) {
  __shared__ float sm[4];
  __shared__ float srs;
  const int j = threadIdx.x, n = blockIdx.x;
  const long long i = (long long)n * 256 + j;
  float s = 0.f;
  for (int z = 0; z < Z; ++z) s += slab[(long long)z * zstride + i];
  T t;
  stf(&t, s * mask[i] * scale);
  ughd[i] = t;
  float d = 0.f;
  d += ldf(&t) * w2[j];
  d = block_sum256(d, sm);
  if (j == 0) {
    const float p = prob[n], pq = p * (1.f - p);
    const float r = d * (1.f - 2.f * p) * pq;
    rs[n] = r;
    pq_out[n] = pq;
    srs = r;
  }
  __syncthreads();
  T tg;
  stf(&tg, srs * w2[j]);
  g_hd[i] = tg;
  stf(g_h + i, ldf(&tg) * mask[i] * scale);
}

// h[b][j] = sum_z slab[z][b][j] + bias[j];  hd = h * mask * scale     (Linear(8392,256) finish + Dropout, model/CGAN.py:104-105,122)
template <typename T>
__global__ void linear_finish_kernel(const float* __restrict__ slab, int Z, long long zstride, const float* __restrict__ bias,
                                     const float* __restrict__ mask, float scale, T* __restrict__ h, T* __restrict__ hd, int B, int N) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * N) return;
  float s = bias ? bias[i % N] : 0.f;
  for (int z = 0; z < Z; ++z) s += slab[(long long)z * zstride + i];
  if (h) stf(h + i, s);
  if (hd) stf(hd + i, mask ? s * mask[i] * scale : s);
}

// The middle of CGAN's head as ONE launch, one workgroup per row of N = 256 columns (thread = column): linear_finish_kernel
// (split-K sum + bias, Dropout), head_fwd_kernel (Linear(256,1) + sigmoid + BCE, ds), head_dgrad_kernel (g_hd = ds * w2) and the
// Dropout backward (g_h = g_hd * mask * scale) - four launches at the launch floor on a serial chain.  Same arithmetic in the same
// order as the four (the dot product is formed by threads 0..31 over 8 columns each, then block_sum256, as head_fwd_kernel
// does it; every value is rounded to T where the separate launches stored it).
template <typename T>
__global__ __launch_bounds__(256) void cg_head_mid_kernel(const float* __restrict__ slab, int Z, long long zstride, const float* __restrict__ bias1,
                                                          const float* __restrict__ mask, float scale, T* __restrict__ h, T* __restrict__ hd,
                                                          const float* __restrict__ w2, const float* __restrict__ bias2, const HeadGroups hg,
                                                          float invB, float* __restrict__ prob, float* __restrict__ ds, float* __restrict__ scal,
                                                          int scal_ld, T* __restrict__ g_hd, T* __restrict__ g_h) {
  __shared__ float sm[4];
  __shared__ __attribute__((aligned(16))) float shd[256];
  __shared__ float sds;
  const int j = threadIdx.x;
  const long long i = (long long)blockIdx.x * 256 + j;
  float s = bias1 ? bias1[j] : 0.f;
  for (int z = 0; z < Z; ++z) s += slab[(long long)z * zstride + i];
  stf(h + i, s);
  T t;
  stf(&t, s * mask[i] * scale);
  hd[i] = t;
  shd[j] = ldf(&t);
  __syncthreads();
  float d = 0.f;
  if (j < 32) {
    const float* v = shd + j * 8;
    const f32x4 w0 = *reinterpret_cast<const f32x4*>(w2 + j * 8), w1 = *reinterpret_cast<const f32x4*>(w2 + j * 8 + 4);
#pragma unroll
    for (int k = 0; k < 4; ++k) d += v[k] * w0[k] + v[4 + k] * w1[k];
  }
  d = block_sum256(d, sm);
  if (j == 0) {
    const int grp = blockIdx.x / hg.rows_per_group, nrow = blockIdx.x - grp * hg.rows_per_group;
    const float target = hg.target[grp];
    const int mode = hg.mode[grp], slot_loss = hg.slot_loss[grp], slot_p = hg.slot_p[grp];
    if (bias2) d += bias2[0];
    const float p = 1.f / (1.f + expf(-d));
    prob[blockIdx.x] = p;
    const float pq = p * (1.f - p);
    float dsv;
    if (mode == 0) {
      const float lp = fmaxf(logf(p), -100.f), lq = fmaxf(logf(1.f - p), -100.f);
      const float loss = -(target * lp + (1.f - target) * lq);
      const float dp = (p - target) / fmaxf(pq, 1e-12f) * invB;
      dsv = dp * pq;
      if (slot_loss >= 0) scal[(long long)slot_loss * scal_ld + nrow] = loss;
    } else {
      dsv = pq;
    }
    ds[blockIdx.x] = dsv;
    sds = dsv;
    if (slot_p >= 0) scal[(long long)slot_p * scal_ld + nrow] = p;
  }
  __syncthreads();
  T tg;
  stf(&tg, sds * w2[j]);
  g_hd[i] = tg;
  stf(g_h + i, ldf(&tg) * mask[i] * scale);
}

// out[0] += sum_i x[i]   (bias gradient of a 1-output Linear)
static __global__ __launch_bounds__(256) void sum_vec_kernel(const float* __restrict__ x, int n, float* __restrict__ out) {
  __shared__ float sm[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) s += x[i];
  s = block_sum256(s, sm);
  if (threadIdx.x == 0) out[0] += s;
}
// G input of the conditional GAN: [z | one-hot label] -> [B][CiPad] T   (model/CGAN.py:154-155: cat([x, labels], 1), int64 -> float)
template <typename T>
__global__ void cgan_z_kernel(const float* __restrict__ z, const long long* __restrict__ labels, int B, int NZ, int NL, int CiPad,
                              T* __restrict__ out) {
  const long long total = (long long)B * CiPad;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % CiPad);
    const long long b = i / CiPad;
    float v = 0.f;
    if (c < NZ) v = z[b * NZ + c];
    else if (c < NZ + NL) v = (float)labels[b * NL + (c - NZ)];
    stf(out + i, v);
  }
}
