// Second-order BatchNorm terms of the back-propagated gradient penalty (CGAN, train/cgan_trainer.py:200-203).
// Notation (tests/test_gp_double_backward_math.py): first backward gy = (gamma/sigma) (gz - m1 - xhat*m2),
// gz = g_a*act'(z), m1 = mean gz, m2 = mean gz*xhat.  The adjoint sweep carries v = adj(gy) forward through D
// ("v-chain") and then the usual reverse sweep with two extra inputs per layer (xdir, sigexp).
// Generic per-channel reduction: NA accumulators per channel, per-workgroup partials [blk][NA][C] (no atomics).
// The per-element expressions, the slice sum and the slice streamer are bn.hpp's; launchers: ops_bn.hip.
#pragma once
#include "bn.hpp"

// MODE 1 (v-chain):  acc = { v, v*xhat, v*gy }             inputs a = v, b = y, c = gy
// MODE 2 (reverse):  acc = { uz, uz*xhat, xdir, xdir*xhat } inputs a = ua, b = y, c = xdir;  uz = ua*act'(z)
template <typename T, int MODE>
__global__ __launch_bounds__(256) void bn2_reduce_kernel(const T* __restrict__ a, const T* __restrict__ b, const T* __restrict__ c,
                                                         const float* __restrict__ aux, float slope, float* __restrict__ partial,
                                                         long long rows, int C) {
  constexpr int NA = MODE == 1 ? 3 : 4;
  extern __shared__ float lsum[];                         // [rstep][NA][C]
  const int upr = C >> 3;
  const int u = threadIdx.x % upr, r0 = threadIdx.x / upr, rstep = 256 / upr;
  const int ch = u * 8;
  const BnAux8 ax(aux, C, ch);
  float acc[NA][8];
#pragma unroll
  for (int k = 0; k < 8; ++k)
#pragma unroll
    for (int q = 0; q < NA; ++q) acc[q][k] = 0.f;
  // two rows of this thread's sequence in flight, accumulated in sequence order (same sums, bit for bit; see bn_bwd_reduce_kernel)
  constexpr int UNR = 2;
  const long long stride = (long long)gridDim.x * rstep;
  for (long long r = (long long)blockIdx.x * rstep + r0; r < rows; r += stride * UNR) {
    float va[UNR][8], vb[UNR][8], vc[UNR][8];
#pragma unroll
    for (int q = 0; q < UNR; ++q) {
      const long long rq = r + q * stride;
      if (rq < rows) { ld8(a + rq * C + ch, va[q]); ld8(b + rq * C + ch, vb[q]); ld8(c + rq * C + ch, vc[q]); }
    }
#pragma unroll
    for (int q = 0; q < UNR; ++q) {
      if (r + q * stride >= rows) break;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float xh = bn_xhat(vb[q][k], ax.mu[k], ax.is[k]);
        if (MODE == 1) {
          acc[0][k] += va[q][k]; acc[1][k] += va[q][k] * xh; acc[2][k] += va[q][k] * vc[q][k];
        } else {
          const float uz = bn_act_grad(bn_z(vb[q][k], ax.sc[k], ax.sh[k]), va[q][k], slope);
          acc[0][k] += uz; acc[1][k] += uz * xh; acc[2][k] += vc[q][k]; acc[NA - 1][k] += vc[q][k] * xh;
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < NA; ++q)
#pragma unroll
    for (int k = 0; k < 8; ++k) lsum[(r0 * NA + q) * C + ch + k] = acc[q][k];
  __syncthreads();
  for (int i = threadIdx.x; i < NA * C; i += 256) {
    float t = 0.f;
    for (int r = 0; r < rstep; ++r) t += lsum[r * NA * C + i];
    partial[(long long)blockIdx.x * NA * C + i] = t;
  }
}

// sums[i] = sum over workgroups of partial[blk][i], i < NA*C (a multiple of 4): one workgroup per 4 outputs, 256 lanes over
// the partials with 16-byte loads (one thread per output looping over 256 strided partials took 64 us for C = 64)
// mode 1 (v-chain): dgamma[c] += sum(v*gy)[c] / gamma[c] (the direct parameter gradient of the v-chain);  mode 2 (reverse sweep):
// dgamma[c] += sum uz*xhat, dbeta[c] += sum uz - by the thread that owns that sum, instead of a launch of their own
static __global__ __launch_bounds__(256) void bn2_sums_kernel(const float* __restrict__ partial, int nblk, int NA, int C,
                                                              float* __restrict__ sums, int mode = 0, const float* __restrict__ gamma = nullptr,
                                                              float* __restrict__ dgamma = nullptr, float* __restrict__ dbeta = nullptr) {
  __shared__ float sh[4][4];
  const int i0 = blockIdx.x * 4, n = NA * C;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  for (int k = threadIdx.x; k < nblk; k += 256) s += *reinterpret_cast<const f32x4*>(partial + (long long)k * n + i0);
#pragma unroll
  for (int j = 0; j < 4; ++j) s[j] = wave_sum(s[j]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) sh[threadIdx.x >> 6][j] = s[j];
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int i = i0 + threadIdx.x;
    const float t = sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
    sums[i] = t;
    if (mode == 1 && i >= 2 * C && i < 3 * C) dgamma[i - 2 * C] += t / gamma[i - 2 * C];
    if (mode == 2 && i < C) dbeta[i] += t;
    if (mode == 2 && i >= C && i < 2 * C) dgamma[i - C] += t;
  }
}

// v-chain apply:  u = act'(z) * (gamma/sigma) (v - mean v - xhat * mean(v xhat))                 (u may overwrite v)
//                 xdir = -(gamma/sigma) (v*m2 + gz * mean(v xhat)),  gz = gy*sigma/gamma + m1 + xhat*m2
// m1, m2 = means of the FIRST backward's sums (sum gz, sum gz*xhat), mv, mvx = means of {sum v, sum v*xhat}
// (channel k of the 8)
__device__ __forceinline__ void bn2_vchain_apply1(float v, float y, float gy, const BnAux8& a, int k, float m1, float m2, float mv, float mvx,
                                                  float slope, float& u, float& xdir) {
  const float sc = a.sc[k];                                  // gamma / sigma
  const float z = bn_z(y, sc, a.sh[k]);
  const float xh = bn_xhat(y, a.mu[k], a.is[k]);
  const float gz = gy / sc + m1 + xh * m2;
  xdir = -sc * (v * m2 + gz * mvx);
  u = bn_act_grad(z, sc * (v - mv - xh * mvx), slope);
}
// reverse-sweep apply with the penalty's extra inputs:
//   q = gamma*uz + xdir;  uy = (q - mean q - xhat*mean(q xhat)) / sigma  -  (sum(v*gy)/sigma) * xhat / n
// mq, mqx: bn2_mean_q of s4 = {sum uz, sum uz*xhat, sum xdir, sum xdir*xhat};  vgy = sum v*gy (from the v-chain)
__device__ __forceinline__ float bn2_mean_q(float g, float s_uz, float s_xdir, float inv_count) { return (g * s_uz + s_xdir) * inv_count; }
__device__ __forceinline__ float bn2_reverse_apply1(float ua, float y, float xdir, const BnAux8& a, int k, float g, float mq, float mqx, float vgy,
                                                    float slope, float inv_count) {
  const float is = a.is[k];
  const float z = bn_z(y, a.sc[k], a.sh[k]);
  const float xh = bn_xhat(y, a.mu[k], is);
  const float q = g * bn_act_grad(z, ua, slope) + xdir;
  return (q - mq - xh * mqx) * is - vgy * is * xh * inv_count;
}

// s1 = sums of the FIRST backward (sum gz, sum gz*xhat), s3 = {sum v, sum v*xhat, sum v*gy}
template <typename T>
__global__ void bn2_vchain_apply_kernel(const T* __restrict__ v, const T* __restrict__ y, const T* __restrict__ gy,
                                        const float* __restrict__ aux, const float* __restrict__ s1, const float* __restrict__ s3,
                                        float slope, float inv_count, T* __restrict__ u, T* __restrict__ xdir, long long total8, int C) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total8; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)((i * 8) & (C - 1));
    float vv[8], vy[8], vg[8], ou[8], ox[8];
    ld8(v + i * 8, vv);
    ld8(y + i * 8, vy);
    ld8(gy + i * 8, vg);
    const BnAux8 ax(aux, C, c);
#pragma unroll
    for (int k = 0; k < 8; ++k)
      bn2_vchain_apply1(vv[k], vy[k], vg[k], ax, k, s1[c + k] * inv_count, s1[C + c + k] * inv_count, s3[c + k] * inv_count,
                        s3[C + c + k] * inv_count, slope, ou[k], ox[k]);
    st8(u + i * 8, ou);
    st8(xdir + i * 8, ox);
  }
}
// s4 = {sum uz, sum uz*xhat, sum xdir, sum xdir*xhat}.  dgamma += sum uz*xhat, dbeta += sum uz: bn2_sums_kernel
template <typename T>
__global__ void bn2_reverse_apply_kernel(const T* __restrict__ ua, const T* __restrict__ y, const T* __restrict__ xdir,
                                         const float* __restrict__ aux, const float* __restrict__ gamma, const float* __restrict__ s4,
                                         const float* __restrict__ vgy, float slope, float inv_count, T* __restrict__ uy,
                                         long long total8, int C) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total8; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)((i * 8) & (C - 1));
    float va[8], vy[8], vx[8];
    ld8(ua + i * 8, va);
    ld8(y + i * 8, vy);
    ld8(xdir + i * 8, vx);
    const BnAux8 ax(aux, C, c);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float g = gamma[c + k];
      va[k] = bn2_reverse_apply1(va[k], vy[k], vx[k], ax, k, g, bn2_mean_q(g, s4[c + k], s4[2 * C + c + k], inv_count),
                                 bn2_mean_q(g, s4[C + c + k], s4[3 * C + c + k], inv_count), vgy[c + k], slope, inv_count);
    }
    st8(uy + i * 8, va);
  }
}

// The second-order chains as two launches instead of three (round 5; the backward twin bn_bwd_apply_fused_kernel): the apply
// kernel's workgroups own a 64-channel slice of a pixel range and sum the partial rows of bn2_reduce_kernel for THEIR channels
// themselves ([blk][NA][C] floats; bn_slice_sums) - bn2_sums_kernel, ~6 us on the main stream's chain eight times per CGAN step, is
// gone.  The first workgroup of a slice writes the sums (ws[q*C + c], as bn2_sums_kernel did: the reverse sweep reads the v-chain's)
// and the direct parameter gradients.
// -> LDS tot[q][j] = sum over the nblk rows of accumulator q, channel slice*64 + j   (q < NA)
template <int NA>
__device__ __forceinline__ void bn2_slice_totals(const float* __restrict__ partial, int nblk, int C, int slice, double (*part)[NA * 64], float (*tot)[64]) {
  const float t = (float)bn_slice_sums<NA, 8>(partial, nblk, (long long)NA * C, C, slice, part);
  if (threadIdx.x < NA * 64) tot[threadIdx.x >> 6][threadIdx.x & 63] = t;
  __syncthreads();
}

// v-chain apply (bn2_vchain_apply_kernel's arithmetic: bn2_vchain_apply1) with the sums of ITS slice formed in the prologue
template <typename T>
__global__ __launch_bounds__(BNF_THREADS) void bn2_vchain_apply_fused_kernel(const T* __restrict__ v, const T* __restrict__ y, const T* __restrict__ gy,
                                                                             const float* __restrict__ aux, const float* __restrict__ s1,
                                                                             const float* __restrict__ partial, int nblk, float* __restrict__ ws,
                                                                             const float* __restrict__ gamma, float* __restrict__ dgamma, float slope,
                                                                             float inv_count, T* __restrict__ u, T* __restrict__ xdir, long long rows, int C) {
  __shared__ double part[5][3 * 64];
  __shared__ float tot[3][64];
  __builtin_amdgcn_s_setprio(JCK_BN_PRIO);
  const int t = threadIdx.x, s = blockIdx.y;
  const BnSlice sl(s);
  const T* const in[3] = {v, y, gy};
  Raw8<T> raw[2][3];                                          // two rows of this thread in flight
  bn_slice_load(in, sl, sl.rfirst, rows, C, raw);
  bn2_slice_totals<3>(partial, nblk, C, s, part, tot);
  if (blockIdx.x == 0 && t < 64) {
    const int c = s * 64 + t;
    ws[c] = tot[0][t]; ws[C + c] = tot[1][t]; ws[2 * C + c] = tot[2][t];
    if (dgamma) dgamma[c] += tot[2][t] / gamma[c];
  }
  const BnAux8 ax(aux, C, sl.off);
  float m1[8], m2[8], mv[8], mvx[8];
  bn_means8(s1 + sl.off, inv_count, m1); bn_means8(s1 + C + sl.off, inv_count, m2);
  bn_means8(tot[0] + (t & 7) * 8, inv_count, mv); bn_means8(tot[1] + (t & 7) * 8, inv_count, mvx);
  bn_slice_stream(in, sl, rows, C, raw, [&](long long e, float (&r)[3][8]) {
    float ou[8], ox[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) bn2_vchain_apply1(r[0][k], r[1][k], r[2][k], ax, k, m1[k], m2[k], mv[k], mvx[k], slope, ou[k], ox[k]);
    st8(u + e, ou);
    st8(xdir + e, ox);
  });
}

// reverse-sweep apply (bn2_reverse_apply_kernel's arithmetic: bn2_reverse_apply1) with the sums of ITS slice formed in the prologue
template <typename T>
__global__ __launch_bounds__(BNF_THREADS) void bn2_reverse_apply_fused_kernel(const T* __restrict__ ua, const T* __restrict__ y, const T* __restrict__ xdir,
                                                                              const float* __restrict__ aux, const float* __restrict__ gamma,
                                                                              const float* __restrict__ partial, int nblk, float* __restrict__ ws,
                                                                              const float* __restrict__ vgy, float* __restrict__ dgamma,
                                                                              float* __restrict__ dbeta, float slope, float inv_count, T* __restrict__ uy,
                                                                              long long rows, int C) {
  __shared__ double part[4][4 * 64];
  __shared__ float tot[4][64];
  __builtin_amdgcn_s_setprio(JCK_BN_PRIO);
  const int t = threadIdx.x, s = blockIdx.y;
  const BnSlice sl(s);
  const T* const in[3] = {ua, y, xdir};
  Raw8<T> raw[2][3];                                          // two rows of this thread in flight
  bn_slice_load(in, sl, sl.rfirst, rows, C, raw);
  bn2_slice_totals<4>(partial, nblk, C, s, part, tot);
  if (blockIdx.x == 0 && t < 64) {
    const int c = s * 64 + t;
    ws[c] = tot[0][t]; ws[C + c] = tot[1][t]; ws[2 * C + c] = tot[2][t]; ws[3 * C + c] = tot[3][t];
    if (dbeta) dbeta[c] += tot[0][t];
    if (dgamma) dgamma[c] += tot[1][t];
  }
  const BnAux8 ax(aux, C, sl.off);
  float g[8], mq[8], mqx[8], kv[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int j = (t & 7) * 8 + k;
    g[k] = gamma[sl.off + k];
    mq[k] = bn2_mean_q(g[k], tot[0][j], tot[2][j], inv_count);
    mqx[k] = bn2_mean_q(g[k], tot[1][j], tot[3][j], inv_count);
    kv[k] = vgy[sl.off + k];
  }
  bn_slice_stream(in, sl, rows, C, raw, [&](long long e, float (&r)[3][8]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) r[0][k] = bn2_reverse_apply1(r[0][k], r[1][k], r[2][k], ax, k, g[k], mq[k], mqx[k], kv[k], slope, inv_count);
    st8(uy + e, r[0]);
  });
}
