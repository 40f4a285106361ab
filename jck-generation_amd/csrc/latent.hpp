// Latent projection (fit z to given images through the frozen eval-mode generator): the image loss with its gradient at the pre-tanh
// product, and Adam on z fused with the split-K slab sum of the dz product.  Memory-bound, one launch each; the third piece - the
// backward of a folded BatchNorm + ReLU - is the MASK option of the gather-GEMM epilogue (igemm.hpp).
#pragma once
#include "common.hpp"

// One workgroup per image: L_b = mean over the 3 * HW real elements of (x - t)^2, x the stored tanh output (NHWC4, type T), t the
// caller's NCHW fp32 target read in place; g_raw = 2 (x - t) / (3 HW) * (1 - x^2) in T, padding channel +0.  Thread i takes pixels
// i, i + 256, ... in that order and the workgroup's 256 partial sums are added in a fixed tree: the same bits on every run, and
// image b's loss does not depend on N.
template <typename T>
__global__ __launch_bounds__(256) void latent_loss_kernel(const T* __restrict__ x, const float* __restrict__ target, T* __restrict__ g_raw,
                                                          float* __restrict__ loss, int HW) {
  __shared__ float sm[4];
  const int b = blockIdx.x;
  const T* xb = x + (long long)b * HW * 4;
  T* gb = g_raw + (long long)b * HW * 4;
  const float* tb = target + (long long)b * 3 * HW;
  const float k = 2.0f / (3.0f * (float)HW);
  float s = 0.f;
  for (int p = threadIdx.x; p < HW; p += 256) {
    float v[4], g[4];
    ld4(xb + (long long)p * 4, v);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float d = v[c] - tb[(long long)c * HW + p];
      s = fmaf(d, d, s);
      g[c] = k * d * (1.f - v[c] * v[c]);
    }
    g[3] = 0.f;
    st4(gb + (long long)p * 4, g);
  }
  s = block_sum256(s, sm);
  if (threadIdx.x == 0) loss[b] = s / (3.0f * (float)HW);
}

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
