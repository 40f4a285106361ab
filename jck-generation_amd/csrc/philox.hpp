// Philox4x32-10 counter-based random numbers, shared by the image kernels' in-kernel noise and the per-step draws of the optimiser launch.
#pragma once
#include "common.hpp"

// ------------------------------------------------------------------------------------------------------
// In-kernel instance noise (perf mode): the reference draws 0.1 * N(0,1) for every pixel of the real and of the fake batch each
// step (train/dcgan_trainer.py:160,171).  Drawing it with ATen costs a 25 MB write plus two 12.6 MB reads per step; here each
// pixel's three normals come out of ONE Philox4x32-10 block (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3":
// counter = (pixel index, tensor id, optimiser step), key = seed) and a Box-Muller transform, inside the kernel that mixes them
// in.  rng: device uint32[4] = {seed lo, seed hi, step, 0}, written per step by jck_engine_set_step (so a captured graph of the
// step carries no per-step argument).  A different stream than torch's generator - parity runs upload their noise instead.
// ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                              unsigned (&o)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}
// three N(0,1) values for pixel `i` of tensor `tensor_id` at the step held in rng[2]
__device__ __forceinline__ void pixel_normals(const unsigned* __restrict__ rng, unsigned tensor_id, long long i, float (&nz)[3]) {
  unsigned o[4];
  philox4x32_10((unsigned)i, (unsigned)(i >> 32), tensor_id, rng[2], rng[0], rng[1], o);
  const float u0 = ((float)(o[0] >> 8) + 0.5f) * (1.0f / 16777216.0f), u1 = ((float)(o[1] >> 8) + 0.5f) * (1.0f / 16777216.0f);
  const float u2 = ((float)(o[2] >> 8) + 0.5f) * (1.0f / 16777216.0f), u3 = ((float)(o[3] >> 8) + 0.5f) * (1.0f / 16777216.0f);
  // Box-Muller on the hardware transcendentals (round 5): v_log_f32 is log2, v_sin_f32 / v_cos_f32 take their argument in
  // REVOLUTIONS - sin(2 pi u) is one instruction on u itself - and v_sqrt_f32 needs no fix-up here.  The library logf / sincosf (range
  // reduction, correctly rounded) made the two noise kernels of a step ALU-bound: ~150 instructions per pixel for three normals
  // whose last bits nobody can check (the reference's noise is torch.randn of another generator; parity tests hand the noise in).
  const float r0 = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u0));
  const float r1 = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u2));
  nz[0] = r0 * __builtin_amdgcn_cosf(u1); nz[1] = r0 * __builtin_amdgcn_sinf(u1); nz[2] = r1 * __builtin_amdgcn_cosf(u3);
}
