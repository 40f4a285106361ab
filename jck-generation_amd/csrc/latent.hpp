// Latent projection (fit z to given images through the frozen eval-mode generator): the image loss with its gradient at the pre-tanh
// product, and Adam on z fused with the split-K slab sum of the dz product.  Memory-bound, one launch each; the third piece - the
// backward of a folded BatchNorm + ReLU - is the Epi::ReluMask form of the gather-GEMM epilogue (igemm.hpp).
#pragma once
#include "common.hpp"

// One thread per (image, latent column k < zd): g = slab[0][b][k] + slab[1][b][k] + ... (fp32, in slab order) + prior * 2 z / zd, then
// torch.optim.Adam's update of (z, m, v) with the bias-corrected step - evaluated in fp64 from the fp32 state and rounded once, so the
// result does not depend on how a compiler contracts the fp32 chain - and z in the element type T into the first zd columns of the
// padded operand row (pitch zp; the columns behind them - a CGAN's one-hot half, the padding - are left alone).
// sum_only: z[b][k] = the slab sum, nothing else is read or written (jck_engine_latent_grad).
template <typename T>
__global__ void latent_adam_kernel(const float* __restrict__ slab, int Z, long long slab_stride, int ld, float* __restrict__ z,
                                   float* __restrict__ m, float* __restrict__ v, double step_size, double bc2_sqrt, double prior2,
                                   T* __restrict__ z_operand, int zp, int zd, int N, int sum_only) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * zd) return;
  const int b = i / zd, k = i - b * zd;
  const float* sp = slab + (long long)b * ld + k;
  float g = sp[0];
  for (int q = 1; q < Z; ++q) g += sp[q * slab_stride];
  if (sum_only) { z[i] = g; return; }
  const double zc = (double)z[i];
  const double gd = (double)g + prior2 * zc;
  const double mn = 0.9 * (double)m[i] + (1.0 - 0.9) * gd;
  const double vn = 0.999 * (double)v[i] + (1.0 - 0.999) * gd * gd;
  const float zn = (float)(zc - step_size * mn / (sqrt(vn) / bc2_sqrt + 1e-8));
  m[i] = (float)mn; v[i] = (float)vn; z[i] = zn;
  stf(z_operand + (long long)b * zp + k, zn);
}

// ---- the image loss (jck_latent_loss, jck_latent_loss_ex) and the critic's latent gradient: D(G(z)) differentiated with respect to z under model.eval() ----
// One workgroup per image.  x is the stored tanh output (NHWC4, type T), t the caller's NCHW fp32 target read in place, w a per-pixel
// weight [n][HW] (fp32, or null: 1), g_x an additive image gradient (NHWC4 of T, or null):
// L_b = sum_p w_p sum_c (x - t)^2 / (3 sum_p w_p), g_raw = (k w_p (x - t) + g_x) (1 - x^2) in T, k = 2 / (3 sum_p w_p), padding channel +0.
// Two passes, sum w and then the loss; thread i takes pixels i, i + 256, ... in that order and the workgroup's 256 partial sums are
// added in a fixed tree: the same bits on every run, and image b's loss does not depend on N.  sum w = 0: loss 0, no reconstruction
// gradient.  target null (g_x required): L_b = 0, g_raw = g_x (1 - x^2).  w null and g_x null - jck_latent_loss - is the plain mean:
// w d = d, sum w = HW, k = 2 / (3 HW), and neither the first pass nor a load of w or g_x runs.
// PLAIN: the launcher's promise that w and g_x are null and target is not - the same statements with those three tests decided by the
// compiler.  Tested at run time once per pixel instead, the plain projection measured 0.6-0.8 % slower.
template <typename T, bool PLAIN>
__global__ __launch_bounds__(256) void latent_loss_kernel(const T* __restrict__ x, const float* __restrict__ target, const float* __restrict__ w,
                                                          const T* __restrict__ g_x, T* __restrict__ g_raw, float* __restrict__ loss, int HW) {
  __shared__ float sm[4];
  if (PLAIN) { w = nullptr; g_x = nullptr; }
  const int b = blockIdx.x;
  const T* xb = x + (long long)b * HW * 4;
  T* gb = g_raw + (long long)b * HW * 4;
  const T* gxb = g_x ? g_x + (long long)b * HW * 4 : nullptr;
  if (!PLAIN && !target) {                             // critic only
    for (int p = threadIdx.x; p < HW; p += 256) {
      float v[4], c[4], g[4];
      ld4(xb + (long long)p * 4, v);
      ld4(gxb + (long long)p * 4, c);
#pragma unroll
      for (int k = 0; k < 3; ++k) g[k] = c[k] * (1.f - v[k] * v[k]);
      g[3] = 0.f;
      st4(gb + (long long)p * 4, g);
    }
    if (threadIdx.x == 0) loss[b] = 0.f;
    return;
  }
  const float* tb = target + (long long)b * 3 * HW;
  const float* wb = w ? w + (long long)b * HW : nullptr;
  float sw = (float)HW;
  if (wb) {
    float a = 0.f;
    for (int p = threadIdx.x; p < HW; p += 256) a += wb[p];
    sw = block_sum256(a, sm);
    __syncthreads();                                   // sm is reused by the second sum
  }
  const float k = sw > 0.f ? 2.0f / (3.0f * sw) : 0.f;
  float s = 0.f;
  for (int p = threadIdx.x; p < HW; p += 256) {
    float v[4], g[4], c[4] = {0.f, 0.f, 0.f, 0.f};
    ld4(xb + (long long)p * 4, v);
    if (gxb) ld4(gxb + (long long)p * 4, c);
    const float wp = wb ? wb[p] : 1.f;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float d = v[ch] - tb[(long long)ch * HW + p];
      const float wd = wb ? wp * d : d;
      s = fmaf(wd, d, s);
      if (gxb) g[ch] = (k * wd + c[ch]) * (1.f - v[ch] * v[ch]);
      else g[ch] = k * wd * (1.f - v[ch] * v[ch]);
    }
    g[3] = 0.f;
    st4(gb + (long long)p * 4, g);
  }
  s = block_sum256(s, sm);
  if (threadIdx.x == 0) loss[b] = sw > 0.f ? s / (3.0f * sw) : 0.f;
}

// The backward of a folded eval-mode stage a = leaky(scale[c] * y + shift[c]) on a gradient of its output, 8 channels per thread:
// g_y[r, c] = a[r, c] > 0 ? scale[c] g[r, c] : scale[c] g[r, c] slope (ATen's leaky_relu_backward: a = +-0 and NaN take the slope).
// g_y may be g.  C a power of two >= 8.
template <typename T>
__global__ void leaky_affine_bwd_kernel(const T* g, const T* __restrict__ a, const float* __restrict__ scale, float slope, T* g_y,
                                        long long total8, int C) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total8; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)((i * 8) & (C - 1));
    float v[8], av[8];
    ld8(g + i * 8, v);
    ld8(a + i * 8, av);
    const f32x4 s0 = *reinterpret_cast<const f32x4*>(scale + c), s1 = *reinterpret_cast<const f32x4*>(scale + c + 4);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float t = (j < 4 ? s0[j] : s1[j - 4]) * v[j];
      v[j] = av[j] > 0.f ? t : t * slope;
    }
    st8(g_y + i * 8, v);
  }
}

// Feature matching on a folded eval-mode stage a = leaky(scale[c] * y + shift[c]): the squared distance between the generated image's
// activation a and a fixed feature f of the same stage, its gradient and the stage's backward in one pass.  One workgroup per image
// (M elements, NHWC, a multiple of C; C a power of two >= 8), 8 channels per access; thread i takes groups i, i + 256, ... in that
// order and the 256 partial sums are added in the fixed tree: the same bits on every run, and image b does not depend on N.
// d = a - f, s += d^2, t = scale[c] * (kg * d) with kg = 2 weight / M, g = a > 0 ? t : t * slope (ATen's leaky_relu_backward on the
// generated image's own activation: a = +-0 and NaN take the slope); ACC: g_y = g_y + g (the old value read in T, the sum in fp32, one
// rounding), else g_y = g.  fterm[b] = (weight / M) * s.
template <typename T, bool ACC>
__global__ __launch_bounds__(256) void feat_match_kernel(const T* __restrict__ a, const T* __restrict__ f, const float* __restrict__ scale,
                                                         float slope, float weight, T* g_y, float* __restrict__ fterm, long long M, int C) {
  __shared__ float sm[4];
  const int b = blockIdx.x;
  const T* ab = a + (long long)b * M;
  const T* fb = f + (long long)b * M;
  T* gb = g_y + (long long)b * M;
  const float wm = weight / (float)M, kg = 2.0f * wm;
  float s = 0.f;
  for (long long i = threadIdx.x; i < M / 8; i += 256) {
    const int c = (int)((i * 8) & (C - 1));
    float av[8], fv[8], g[8];
    ld8(ab + i * 8, av);
    ld8(fb + i * 8, fv);
    if (ACC) ld8(gb + i * 8, g);
    const f32x4 s0 = *reinterpret_cast<const f32x4*>(scale + c), s1 = *reinterpret_cast<const f32x4*>(scale + c + 4);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float d = av[j] - fv[j];
      s = fmaf(d, d, s);
      const float t = (j < 4 ? s0[j] : s1[j - 4]) * (kg * d);
      const float v = av[j] > 0.f ? t : t * slope;
      g[j] = ACC ? g[j] + v : v;
    }
    st8(gb + i * 8, g);
  }
  s = block_sum256(s, sm);
  if (threadIdx.x == 0) fterm[b] = wm * s;
}

// The critic's objective on a logit, one thread per row: ds[b] = lambda c'(logit), term[b] = lambda c(logit).
// mode 1 (nsgan): c = softplus(-logit) = -log sigmoid(logit), the generator's own training loss, c' = -sigmoid(-logit), both from
// e = exp(-|logit|) <= 1 (no overflow at any logit).  mode 2 (logit): c = -logit, c' = -1.  A non-finite logit: NaN in both.
__global__ void critic_ds_kernel(const float* __restrict__ logit, int mode, float lambda, int B, float* __restrict__ ds, float* __restrict__ term) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const float l = logit[b];
  float c, dc;
  if (mode == 1) {
    const float e = expf(-fabsf(l));
    c = fmaxf(-l, 0.f) + log1pf(e);
    dc = l >= 0.f ? -e / (1.f + e) : -1.f / (1.f + e);
  } else {
    c = -l; dc = -1.f;
  }
  if (!(fabsf(l) <= 3.402823466e38f)) c = dc = __builtin_nanf("");
  ds[b] = lambda * dc;
  term[b] = lambda * c;
}
