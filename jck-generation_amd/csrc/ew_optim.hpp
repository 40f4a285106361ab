// Memory-bound kernels, optimiser side: Adam over a flat arena (with the step's small random draws) and weight packing (with the
// end-of-step job that rides in the repack launch).
#pragma once
#include "common.hpp"
#include "philox.hpp"

// ------------------------------------------------------------------------------------------------------
// Adam (torch.optim.Adam single-tensor algorithm, amsgrad=False, weight_decay=0) over a flat arena
// ------------------------------------------------------------------------------------------------------
// hp (optional): device float[2] = {step_size, bc2_sqrt} of THIS step, written by adam_hp_kernel before the step is enqueued
// - the whole-step engine passes its per-step scalars this way so that a captured hipGraph of the step carries no
// per-step kernel argument; the values are the same host-computed floats either way.
// hp[0..1] = Adam's per-step scalars; hp[2] = the generator EMA's weight 1 - decay of this step (0 when no EMA is configured; read
// by adam_kernel only when it is handed an EMA arena); hp[3] unused; hp[4..7] (as uint32) = {noise seed lo, hi, step, 0} for the in-kernel Philox noise.
// The same launch draws the step's SMALL random inputs when the caller hands over none (perf mode): z [nz] ~ N(0,1)
// (train/dcgan_trainer.py:168), alpha [nalpha] ~ U[0,1) (:111), CGAN's Dropout keep masks [nmask] in {0,1} with P(keep) = keep_p
// (model/CGAN.py:105) - Philox4x32-10, counter = (index/4, tensor id 8 / 9 / 10, step), key = seed.  No ATen launch is left
// in the step, and a captured step replays with fresh draws without any copy into static buffers.
struct StepRng { float* z; long long nz; float* alpha; long long nalpha; float* masks; long long nmask; float keep_p; float* zero; long long nzero;
                 float* zbig[2]; long long nzbig[2];
                 void* zpad; int zd, zp, zpad_f32; };     // zpad (optional): the same z as the rows [nz / zd][zp] of G.conv1's operand (bf16 | fp32)
// (zero / nzero: a small buffer the same launch clears - the engine's per-step accumulator rows, instead of a memset node;
// zbig: up to two large 16-byte aligned ranges, counts % 4 == 0 - D's gradient arena and CGAN's permuted Linear gradient, which
// D.zero_grad() (train/dcgan_trainer.py:155) would clear with a launch of its own a few microseconds later)
__device__ __forceinline__ float u01(unsigned x) { return ((float)(x >> 8) + 0.5f) * (1.0f / 16777216.0f); }
static __global__ void adam_hp_kernel(float* __restrict__ hp, float step_size, float bc2_sqrt, unsigned seed_lo, unsigned seed_hi,
                                      unsigned step, const StepRng r, float ema_w) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    hp[0] = step_size; hp[1] = bc2_sqrt; hp[2] = ema_w;
    unsigned* w = reinterpret_cast<unsigned*>(hp + 4);
    w[0] = seed_lo; w[1] = seed_hi; w[2] = step; w[3] = 0u;
  }
  const long long q0 = (r.nz + 3) / 4, q1 = (r.nalpha + 3) / 4, q2 = (r.nmask + 3) / 4;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < r.nzero; i += (long long)gridDim.x * blockDim.x) r.zero[i] = 0.f;
#pragma unroll
  for (int b = 0; b < 2; ++b)
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < (r.nzbig[b] >> 2); i += (long long)gridDim.x * blockDim.x)
      reinterpret_cast<f32x4*>(r.zbig[b])[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < q0 + q1 + q2; i += (long long)gridDim.x * blockDim.x) {
    unsigned o[4];
    if (i < q0) {                                                     // four normals: two Box-Muller pairs
      philox4x32_10((unsigned)i, (unsigned)(i >> 32), 8u, step, seed_lo, seed_hi, o);
      const float r0 = sqrtf(-2.0f * logf(u01(o[0]))), r1 = sqrtf(-2.0f * logf(u01(o[2])));
      float s0, c0, s1, c1;
      sincosf(6.283185307179586f * u01(o[1]), &s0, &c0);
      sincosf(6.283185307179586f * u01(o[3]), &s1, &c1);
      const float v[4] = {r0 * c0, r0 * s0, r1 * c1, r1 * s1};
      for (int k = 0; k < 4; ++k)
        if (i * 4 + k < r.nz) {
          r.z[i * 4 + k] = v[k];
          // ... and, in the same launch, into G.conv1's operand rows (what pad_rows_kernel would copy a launch later; the padding
          // columns [zd, zp) are never written by anybody: they keep the zeros jck_engine_bind cleared the workspace to)
          if (r.zpad) {
            const long long e = i * 4 + k, b = e / r.zd;
            const int c = (int)(e - b * r.zd);
            if (r.zpad_f32) reinterpret_cast<float*>(r.zpad)[b * r.zp + c] = v[k];
            else stf(reinterpret_cast<bf16_t*>(r.zpad) + b * r.zp + c, v[k]);
          }
        }
    } else if (i < q0 + q1) {
      const long long j = i - q0;
      philox4x32_10((unsigned)j, (unsigned)(j >> 32), 9u, step, seed_lo, seed_hi, o);
      for (int k = 0; k < 4; ++k)
        if (j * 4 + k < r.nalpha) r.alpha[j * 4 + k] = (float)(o[k] >> 8) * (1.0f / 16777216.0f);      // [0, 1)
    } else {
      const long long j = i - q0 - q1;
      philox4x32_10((unsigned)j, (unsigned)(j >> 32), 10u, step, seed_lo, seed_hi, o);
      for (int k = 0; k < 4; ++k)
        if (j * 4 + k < r.nmask) r.masks[j * 4 + k] = (float)(o[k] >> 8) * (1.0f / 16777216.0f) < r.keep_p ? 1.f : 0.f;
    }
  }
}
__device__ __forceinline__ void adam_one(float& pi, float gi_raw, float& mi_io, float& vi_io, float w1, float beta2, float omb2,
                                         float eps, float step_size, float bc2_sqrt, float grad_scale) {
  const float gi = gi_raw * grad_scale;
  // exp_avg.lerp_(grad, 1-beta1): weight 0.5 takes ATen's "end - (end-start)*(1-w)" branch when w >= 0.5
  const float mi = (w1 < 0.5f) ? mi_io + w1 * (gi - mi_io) : gi - (gi - mi_io) * (1.f - w1);
  const float vi = vi_io * beta2 + (omb2 * gi) * gi;
  mi_io = mi;
  vi_io = vi;
  const float denom = sqrtf(vi) / bc2_sqrt + eps;
  pi = pi - step_size * (mi / denom);
}
// Exponential moving average of the parameters, updated from the new parameter while it is still in a register: ATen's lerp
// (the same two branches adam_one takes for exp_avg), so w = 1 gives e = p exactly
__device__ __forceinline__ float ema_one(float e, float pn, float w) { return (w < 0.5f) ? e + w * (pn - e) : pn - (pn - e) * (1.f - w); }
// Adam's constants and the step's scalars as every element sees them
struct AdamScal { float w1 /*1-beta1*/, beta2, omb2 /*1-beta2*/, eps, step_size, bc2_sqrt, grad_scale, ema_w; };
// elements [4i, 4i + 4) of 16-byte aligned arenas; pn (optional): the four new parameters, for a caller that goes on with them
template <bool EMA>
__device__ __forceinline__ void adam_quad(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                          float* __restrict__ ema, long long i, const AdamScal& s, float* pn = nullptr) {
  f32x4 pv = reinterpret_cast<f32x4*>(p)[i], mv = reinterpret_cast<f32x4*>(m)[i], vv = reinterpret_cast<f32x4*>(v)[i];
  const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
  f32x4 ev;
  if (EMA) ev = reinterpret_cast<f32x4*>(ema)[i];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float pk = pv[k], mk = mv[k], vk = vv[k];
    adam_one(pk, gv[k], mk, vk, s.w1, s.beta2, s.omb2, s.eps, s.step_size, s.bc2_sqrt, s.grad_scale);
    pv[k] = pk; mv[k] = mk; vv[k] = vk;
    if (EMA) ev[k] = ema_one(ev[k], pk, s.ema_w);
    if (pn) pn[k] = pk;
  }
  reinterpret_cast<f32x4*>(p)[i] = pv; reinterpret_cast<f32x4*>(m)[i] = mv; reinterpret_cast<f32x4*>(v)[i] = vv;
  if (EMA) reinterpret_cast<f32x4*>(ema)[i] = ev;
}
template <bool EMA>
__device__ __forceinline__ void adam_single(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                            float* __restrict__ ema, long long i, const AdamScal& s) {
  adam_one(p[i], g[i], m[i], v[i], s.w1, s.beta2, s.omb2, s.eps, s.step_size, s.bc2_sqrt, s.grad_scale);
  if (EMA) ema[i] = ema_one(ema[i], p[i], s.ema_w);
}
// four elements per thread (16-byte loads and stores: the arenas are 16-byte aligned); the last n % 4 elements one by one
// EMA = true: `ema` is a fifth arena of n floats (16-byte aligned like the others when vec = 1), weight ema_w - or hp[2] when the
// per-step scalars come from device memory; EMA = false is the kernel without any of it
template <bool EMA>
static __global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                            float* __restrict__ v, long long n, float w1 /*1-beta1*/, float beta2, float omb2 /*1-beta2*/,
                            float eps, float step_size, float bc2_sqrt, float grad_scale, const float* __restrict__ hp = nullptr,
                            int vec = 1, float* __restrict__ zero = nullptr, long long nzero4 = 0,
                            const unsigned* __restrict__ skip_if = nullptr, float* __restrict__ ema = nullptr, float ema_w = 1.f) {
  if (hp) { step_size = hp[0]; bc2_sqrt = hp[1]; }
  if (EMA && hp) ema_w = hp[2];
  // skip_if (the engine's grid-barrier error word): a resident launch of this step went on with incomplete sums - the gradients
  // are invalid, so parameters and moments stay as they are (the host learns of it at jck_engine_check); the zero range below is
  // still cleared: the next pass accumulates into it
  const bool skip = skip_if && *skip_if != 0u;
  // zero (optional): a 16-byte aligned range of nzero4 float4 the same launch clears - the OTHER network's gradient arena, whose
  // zero_grad() (train/dcgan_trainer.py:182) is the next thing in the step
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < nzero4; i += (long long)gridDim.x * blockDim.x)
    reinterpret_cast<f32x4*>(zero)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (skip) return;
  const AdamScal s = {w1, beta2, omb2, eps, step_size, bc2_sqrt, grad_scale, ema_w};
  const long long n4 = vec ? (n >> 2) : 0;                 // vec = 0: a pointer is not 16-byte aligned -> element by element
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x)
    adam_quad<EMA>(p, g, m, v, ema, i, s);
  for (long long i = (n4 << 2) + blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    adam_single<EMA>(p, g, m, v, ema, i, s);
}

// ------------------------------------------------------------------------------------------------------
// weight packing (fp32 PyTorch layout [Cs][Cb][4][4] -> GEMM operand layouts in bf16 (fast) or fp32 (parity))
// ------------------------------------------------------------------------------------------------------
// down: wp[cs][ (kh*4+kw)*CbPad + cb ]   rows cs in [0, CsPad)
__device__ __forceinline__ float pack_down_val(const float* __restrict__ w, int Cs, int Cb, int logCbPad, long long i) {
  const long long K = 16ll << logCbPad;
  const int cs = (int)(i / K);
  const int k = (int)(i % K);
  const int t = k >> logCbPad, cb = k & ((1 << logCbPad) - 1);
  return (cs < Cs && cb < Cb) ? w[((long long)cs * Cb + cb) * 16 + t] : 0.f;
}
template <typename W>
__global__ void pack_down_kernel(const float* __restrict__ w, int Cs, int Cb, int CsPad, int logCbPad, W* __restrict__ wp) {
  const long long K = 16ll << logCbPad, total = (long long)CsPad * K;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x)
    stf(wp + i, pack_down_val(w, Cs, Cb, logCbPad, i));
}

// up: wp[phase][cb][ (th*2+tw)*Cs + cs ], rows cb in [0, CbPad); phase = ph*2+pw;
// output row 2q+ph takes input rows q + DY[ph][th] through kernel rows KH[ph][th]
static __device__ __constant__ int c_up_k[2][2] = {{1, 3}, {0, 2}};
__device__ __forceinline__ float pack_up_val(const float* __restrict__ w, int Cs, int Cb, int CbPad, long long i) {
  const long long K = 4ll * Cs, per = (long long)CbPad * K;
  const int phase = (int)(i / per);
  const long long r = i % per;
  const int cb = (int)(r / K);
  const int k = (int)(r % K);
  const int t = k / Cs, cs = k % Cs;
  const int kh = c_up_k[phase >> 1][t >> 1], kw = c_up_k[phase & 1][t & 1];
  return cb < Cb ? w[((long long)cs * Cb + cb) * 16 + kh * 4 + kw] : 0.f;
}
template <typename W>
__global__ void pack_up_kernel(const float* __restrict__ w, int Cs, int Cb, int CbPad, W* __restrict__ wp) {
  const long long total = 4ll * CbPad * 4 * Cs;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x)
    stf(wp + i, pack_up_val(w, Cs, Cb, CbPad, i));
}

// up, 3/4-channel output (G.conv5, dgrad of D.conv1): all four output parities in ONE 16-row operand,
// wp[phase*4 + c][ (dyi*3+dxi)*Cs + cs ] over the 9 input offsets dy,dx in {-1,0,1}; unused (phase, offset) pairs are 0
__device__ __forceinline__ float pack_up16_val(const float* __restrict__ w, int Cs, int Cb, long long i) {
  const long long K = 9ll * Cs;
  const int r = (int)(i / K), k = (int)(i % K);
  const int phase = r >> 2, c = r & 3, t9 = k / Cs, cs = k % Cs;
  const int dy = t9 / 3 - 1, dx = t9 % 3 - 1, ph = phase >> 1, pw = phase & 1;
  // output row 2q+ph reads input row q+dy through kernel row kh:  ph=0: (0 -> 1), (-1 -> 3);  ph=1: (+1 -> 0), (0 -> 2)
  const int kh = ph == 0 ? (dy == 0 ? 1 : (dy == -1 ? 3 : -1)) : (dy == 1 ? 0 : (dy == 0 ? 2 : -1));
  const int kw = pw == 0 ? (dx == 0 ? 1 : (dx == -1 ? 3 : -1)) : (dx == 1 ? 0 : (dx == 0 ? 2 : -1));
  return (c < Cb && kh >= 0 && kw >= 0) ? w[((long long)cs * Cb + c) * 16 + kh * 4 + kw] : 0.f;
}
template <typename W>
__global__ void pack_up16_kernel(const float* __restrict__ w, int Cs, int Cb, W* __restrict__ wp) {
  const long long total = 16 * 9ll * Cs;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x)
    stf(wp + i, pack_up16_val(w, Cs, Cb, i));
}

// G.conv1 (ConvTranspose on a 1x1 input): wp[(kh*4+kw)*Co + co][ci], ci in [0, CiPad)
__device__ __forceinline__ float pack_g1_val(const float* __restrict__ w, int Ci, int Co, int CiPad, long long i) {
  const int ci = (int)(i % CiPad);
  const long long r = i / CiPad;
  const int co = (int)(r % Co), t = (int)(r / Co);
  return ci < Ci ? w[((long long)ci * Co + co) * 16 + t] : 0.f;
}
template <typename W>
__global__ void pack_g1_kernel(const float* __restrict__ w, int Ci, int Co, int CiPad, W* __restrict__ wp) {
  const long long total = 16ll * Co * CiPad;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x)
    stf(wp + i, pack_g1_val(w, Ci, Co, CiPad, i));
}

// D.conv5 (a dot product per image): wp[(kh*4+kw)*C + c] fp32
static __global__ void pack_head_kernel(const float* __restrict__ w, int C, float* __restrict__ wp) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 16 * C) return;
  const int t = i / C, c = i % C;
  wp[i] = w[c * 16 + t];
}

// Every packed operand of one network in ONE launch (the optimiser step is followed by 9-10 repacks; as separate launches
// their ~4.5 us floor each left the GPU idle for ~45 us twice per step).  A thread owns one (output channel, input channel)
// pair of a conv weight: it reads the pair's 16 taps (64 contiguous bytes) once and writes the 16 operand elements, with
// the lane-fastest index chosen per layout so that every store instruction covers contiguous elements.  Padding rows and
// channels are never written: they stay zero from jck_engine_bind's clear of the workspace.  256 pairs per workgroup.
#define PACK_MAX_JOBS 12
#define PACK_CHUNK 256
struct PackJob { const float* w; void* wp; long long total; int kind, a, b, c; };   // kind: 0 down 1 up 2 up16 3 g1 4 head
struct PackJobs { PackJob j[PACK_MAX_JOBS]; int first_chunk[PACK_MAX_JOBS + 1]; int n; };
// the operand elements of one pair (x, y) of a conv weight [A][Bc][4][4] from its 16 taps v: x is the weight's outer channel index
// (Cs, G.conv1's Ci, the head's C), y the inner one (Cb, Co).  One copy for the repack kernels and for Adam's launch below
template <typename W>
__device__ __forceinline__ void pack_store_pair(const PackJob& J, int x, int y, const float* v) {
  W* wp = reinterpret_cast<W*>(J.wp);
  switch (J.kind) {
    case 0: {   // down: a = Cs, b = Cb, c = logCbPad; wp[cs][t*CbPad + cb]
      W* d = wp + (((long long)x * 16) << J.c) + y;
#pragma unroll
      for (int t = 0; t < 16; ++t) stf(d + ((long long)t << J.c), v[t]);
    } break;
    case 1: {   // up: a = Cs, b = Cb, c = CbPad; wp[phase][cb][t4*Cs + cs]
      const int Cs = J.a;
      const long long K = 4ll * Cs, per = (long long)J.c * K;
#pragma unroll
      for (int phase = 0; phase < 4; ++phase)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int kh = c_up_k[phase >> 1][t >> 1], kw = c_up_k[phase & 1][t & 1];
          stf(wp + phase * per + (long long)y * K + (long long)t * Cs + x, v[kh * 4 + kw]);
        }
    } break;
    case 2: {   // up16: a = Cs, b = Cb; wp[phase*4 + c][t9*Cs + cs], unused (phase, offset) pairs stay 0
      const int Cs = J.a;
      const long long K = 9ll * Cs;
#pragma unroll
      for (int phase = 0; phase < 4; ++phase)
#pragma unroll
        for (int t9 = 0; t9 < 9; ++t9) {
          const int dy = t9 / 3 - 1, dx = t9 % 3 - 1, ph = phase >> 1, pw = phase & 1;
          const int kh = ph == 0 ? (dy == 0 ? 1 : (dy == -1 ? 3 : -1)) : (dy == 1 ? 0 : (dy == 0 ? 2 : -1));
          const int kw = pw == 0 ? (dx == 0 ? 1 : (dx == -1 ? 3 : -1)) : (dx == 1 ? 0 : (dx == 0 ? 2 : -1));
          if (kh >= 0 && kw >= 0) stf(wp + (long long)(phase * 4 + y) * K + (long long)t9 * Cs + x, v[kh * 4 + kw]);
        }
    } break;
    case 3: {   // g1: a = Ci, b = Co, c = CiPad; wp[(t*Co + co)][ci]
#pragma unroll
      for (int t = 0; t < 16; ++t) stf(wp + ((long long)t * J.b + y) * J.c + x, v[t]);
    } break;
    default: {  // head: a = C; wp[t*C + c] fp32
#pragma unroll
      for (int t = 0; t < 16; ++t) reinterpret_cast<float*>(J.wp)[(long long)t * J.a + x] = v[t];
    } break;
  }
}
// the repack: thread u of a job owns one pair, the lane-fastest index chosen per layout (down: cb; up, up16: cs; g1: ci; head: c)
template <typename W>
__device__ __forceinline__ void pack_multi_block(const PackJobs& jobs, int bx) {
  int ji = 0;
  while (ji + 1 < jobs.n && bx >= jobs.first_chunk[ji + 1]) ++ji;
  const PackJob& J = jobs.j[ji];
  const long long u = (long long)(bx - jobs.first_chunk[ji]) * PACK_CHUNK + threadIdx.x;
  if (u >= J.total) return;
  int x, y, Bc = J.b;
  if (J.kind == 0) { x = (int)(u / J.b); y = (int)(u % J.b); }
  else if (J.kind == 4) { x = (int)u; y = 0; Bc = 1; }
  else { y = (int)(u / J.a); x = (int)(u % J.a); }
  const float* src = J.w + ((long long)x * Bc + y) * 16;
  float v[16];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(src + 4 * q);
    v[4 * q] = t[0]; v[4 * q + 1] = t[1]; v[4 * q + 2] = t[2]; v[4 * q + 3] = t[3];
  }
  pack_store_pair<W>(J, x, y, v);
}
template <typename W>
__global__ __launch_bounds__(256) void pack_multi_kernel(const PackJobs jobs) { pack_multi_block<W>(jobs, (int)blockIdx.x); }

template <typename T>
__global__ void cast_f32_kernel(const float* __restrict__ in, T* __restrict__ out, long long n) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    stf(out + i, in[i]);
}
template <typename T>
__global__ void cast_to_f32_kernel(const T* __restrict__ in, float* __restrict__ out, long long n) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    out[i] = ldf(in + i);
}

// z [B][Ci] fp32 -> [B][CiPad] T, zero padded (G.conv1 operand)
template <typename T>
__global__ void pad_rows_kernel(const float* __restrict__ in, int B, int Ci, int CiPad, T* __restrict__ out) {
  const long long total = (long long)B * CiPad;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % CiPad);
    const long long b = i / CiPad;
    stf(out + i, c < Ci ? in[b * Ci + c] : 0.f);
  }
}

// acc rows: 0 loss_real 1 loss_fake 2 loss_g 3 p(real) 4 p(fake) 5 p(g phase) 6 (||g||-1)^2, one entry per image
// out: loss_d, loss_g, D(x), D(G(z))_1, D(G(z))_2, gp, loss_real, loss_fake      (train/dcgan_trainer.py:179,192-193)
// End of a step in ONE launch: the deferred BatchNorm running-stat records of D's four layers (blockIdx.y = layer, same
// recurrence as sequential momentum updates) and the logged scalars (blockIdx.y = number of layers).
struct TailLayer { const float* rec; float* rm; float* rv; long long* nbt; int C; };
// acc is the per-image table [7][acc_ld] (head_fwd / gp_norm write one entry per image): each row is summed here in a fixed
// order (thread-strided partial sums, wavefront shuffles, 4 wave totals), so the logged scalars are bitwise reproducible.
struct TailJobs { TailLayer l[5]; int nl; int npass; float momentum; const float* acc; int acc_ld, B; float invB, lambda_gp; float* out; };
__device__ __forceinline__ void step_tail_block(const TailJobs& t, int bx, int by) {
  if (by == t.nl) {
    if (bx != 0) return;
    __shared__ float sm[4];
    float tot[7];
#pragma unroll
    for (int q = 0; q < 7; ++q) {
      float s = 0.f;
      for (int n = threadIdx.x; n < t.B; n += 256) s += t.acc[(long long)q * t.acc_ld + n];
      tot[q] = block_sum256(s, sm);
    }
    if (threadIdx.x == 0) {
      const float lr = tot[0] * t.invB, lf = tot[1] * t.invB, gp = tot[6] * t.invB;
      t.out[0] = (lr + lf) + t.lambda_gp * gp;
      t.out[1] = tot[2] * t.invB;
      t.out[2] = tot[3] * t.invB;
      t.out[3] = tot[4] * t.invB;
      t.out[4] = tot[5] * t.invB;
      t.out[5] = gp;
      t.out[6] = lr;
      t.out[7] = lf;
    }
    return;
  }
  const TailLayer& L = t.l[by];
  const int c = bx * blockDim.x + threadIdx.x;
  if (c == 0 && L.nbt) *L.nbt += t.npass;
  if (c >= L.C) return;
  float rm = L.rm[c], rv = L.rv[c];
  for (int p = 0; p < t.npass; ++p) {
    rm = (1.f - t.momentum) * rm + t.momentum * L.rec[(long long)p * 2 * L.C + c];
    rv = (1.f - t.momentum) * rv + t.momentum * L.rec[(long long)p * 2 * L.C + L.C + c];
  }
  L.rm[c] = rm;
  L.rv[c] = rv;
}
// G's repack and the end of the step in one launch (two independent jobs at the very end of the step, each near the launch
// floor): workgroups [0, pack_chunks) repack, the next tail_x * (nl + 1) are step_tail_block's grid (tail_x, nl + 1) row-major
template <typename W>
__global__ __launch_bounds__(256) void pack_tail_kernel(const PackJobs jobs, int pack_chunks, const TailJobs t, int tail_x) {
  if ((int)blockIdx.x < pack_chunks) { pack_multi_block<W>(jobs, (int)blockIdx.x); return; }
  const int q = (int)blockIdx.x - pack_chunks;
  step_tail_block(t, q % tail_x, q / tail_x);
}

// ------------------------------------------------------------------------------------------------------
// Adam and the repack of one network as ONE launch: the operands are written from the registers that hold the new weights
// ------------------------------------------------------------------------------------------------------
// The repack read, once per operand form, the fp32 weights Adam had written a launch earlier.  Here a conv weight [A][Bc][4][4] at
// arena offset `off` is a group of the jobs [j0, j0 + nj) that pack it, cut into tiles of 16 x 16 pairs, one workgroup each.  The
// update streams like adam_kernel: a wave takes one outer channel of the tile per turn, its 64 lanes the 64 consecutive quads of
// that row's 16 pairs (1 KB of each arena per instruction; a thread that owned a pair's 64 bytes would load 16 bytes at a stride of
// 64 and made the step 2.3 % slower than the two launches).  The new weights go to LDS, and every form is written from there with
// pack_store_pair by the thread that owns the pair: (tid >> 4, tid & 15) for `down`, whose inner channel is fastest, (tid & 15,
// tid >> 4) for the forms with the outer channel fastest - 16 lanes to a contiguous run either way.  LDS slots are 20 floats per
// pair, 17 slots per row: both readers' 16-byte reads fall on distinct banks.  Every arena range [fa, fb) between the conv weights
// (BatchNorm weights and biases, CGAN's embedding and Linear layers) goes four elements per thread as in adam_kernel, 1024 per
// workgroup.  Values are those of adam_kernel followed by pack_multi_kernel bit for bit: the same adam_one per element, the same
// stf per operand element.
#define ADAM_MAX_FLAT 8
struct AdamGroup { long long off; int A, Bc, j0, nj; };
struct AdamPlan {
  AdamGroup g[PACK_MAX_JOBS]; int first_blk[PACK_MAX_JOBS + 1]; int ng;
  long long fa[ADAM_MAX_FLAT], fb[ADAM_MAX_FLAT]; int first_fblk[ADAM_MAX_FLAT + 1]; int nf;
};
struct AdamArenas { float* p; const float* g; float *m, *v, *ema; const float* hp; float* zero; long long nzero4; const unsigned* skip_if; };
template <typename W, bool EMA>
__device__ __forceinline__ void adam_pair_block(const PackJobs& jobs, const AdamGroup& G, int tile, const AdamArenas& a, const AdamScal& s) {
  __shared__ __attribute__((aligned(16))) float sm[16 * 17 * 20];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int ty = (G.Bc + 15) >> 4, x0 = tile / ty * 16, y0 = tile % ty * 16;
  const int nq = min(64, (G.Bc - y0) * 4);                       // quads of a row inside the tile
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int xr = 4 * k + wv;
    if (x0 + xr < G.A && lane < nq) {
      float pn[4];
      adam_quad<EMA>(a.p, a.g, a.m, a.v, a.ema, (G.off >> 2) + ((long long)(x0 + xr) * G.Bc + y0) * 4 + lane, s, pn);
      *reinterpret_cast<f32x4*>(sm + (xr * 17 + (lane >> 2)) * 20 + (lane & 3) * 4) = f32x4{pn[0], pn[1], pn[2], pn[3]};
    }
  }
  __syncthreads();
  for (int f = G.j0; f < G.j0 + G.nj; ++f) {
    const PackJob& J = jobs.j[f];
    const int xl = J.kind == 0 ? tid >> 4 : tid & 15, yl = J.kind == 0 ? tid & 15 : tid >> 4;
    if (x0 + xl >= G.A || y0 + yl >= G.Bc) continue;
    float r[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(sm + (xl * 17 + yl) * 20 + 4 * q);
      r[4 * q] = t[0]; r[4 * q + 1] = t[1]; r[4 * q + 2] = t[2]; r[4 * q + 3] = t[3];
    }
    pack_store_pair<W>(J, x0 + xl, y0 + yl, r);
  }
}
// workgroups [0, pair_blks): tiles of the conv weights; the next flat_blks: the ranges between them; then (G's launch) the end-of-step
// job's tail_x * (nl + 1) as in pack_tail_kernel.  zero / skip_if / hp as in adam_kernel: a set error word leaves parameters,
// moments AND operands as they are - the operands come from registers here, and those would hold the weights Adam did not write
template <typename W, bool EMA>
__global__ __launch_bounds__(256) void adam_pack_kernel(const PackJobs jobs, const AdamPlan plan, const AdamArenas a, AdamScal s, int pair_blks,
                                                        int flat_blks, const TailJobs t, int tail_x) {
  const int bx = (int)blockIdx.x, nb = pair_blks + flat_blks;
  if (bx >= nb) { step_tail_block(t, (bx - nb) % tail_x, (bx - nb) / tail_x); return; }
  for (long long i = bx * 256ll + threadIdx.x; i < a.nzero4; i += nb * 256ll) reinterpret_cast<f32x4*>(a.zero)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (a.skip_if && *a.skip_if != 0u) return;
  if (a.hp) { s.step_size = a.hp[0]; s.bc2_sqrt = a.hp[1]; if (EMA) s.ema_w = a.hp[2]; }
  if (bx < pair_blks) {
    int gi = 0;
    while (gi + 1 < plan.ng && bx >= plan.first_blk[gi + 1]) ++gi;
    adam_pair_block<W, EMA>(jobs, plan.g[gi], bx - plan.first_blk[gi], a, s);
    return;
  }
  const int fx = bx - pair_blks;
  int fi = 0;
  while (fi + 1 < plan.nf && fx >= plan.first_fblk[fi + 1]) ++fi;
  // [fa, fb) = unaligned head | whole quads [a4, b4) | tail; the range's first workgroup takes head and tail one by one
  const long long fa = plan.fa[fi], fb = plan.fb[fi], a4 = min((fa + 3) & ~3ll, fb), b4 = max(fb & ~3ll, a4);
  const int k = fx - plan.first_fblk[fi];
  const long long i = (a4 >> 2) + k * 256ll + threadIdx.x;
  if (i < (b4 >> 2)) adam_quad<EMA>(a.p, a.g, a.m, a.v, a.ema, i, s);
  if (k == 0) {
    const int nh = (int)(a4 - fa), nt = (int)(fb - b4);
    if ((int)threadIdx.x < nh + nt) adam_single<EMA>(a.p, a.g, a.m, a.v, a.ema, (int)threadIdx.x < nh ? fa + threadIdx.x : b4 + (threadIdx.x - nh), s);
  }
}
