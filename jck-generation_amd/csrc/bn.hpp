// BatchNorm + activation, first order (training mode always - the reference never switches G/D to eval): statistics finalise,
// normalise + activation, backward reduce / sums / apply, and the fused forms whose workgroups sum the partial rows of their own
// 64-channel slice.  The building blocks every one of them shares stand first - the per-element expressions, the finalize
// arithmetic, the slice sum, the slice streamer; the second-order kernels (bn2.hpp) use them too.  Launchers: ops_bn.hip; the
// resident one-launch backward: bnres.hpp.  16-byte vectorised along the NHWC channel axis; per-channel reductions use registers
// -> LDS -> per-workgroup partial rows summed in a fixed order (no float atomics: two runs give bitwise identical results).
#pragma once
#include "common.hpp"

// The streaming BatchNorm kernels run at wave priority 3: in the backward passes they share the chip with the weight-gradient
// products of the second stream, whose waves otherwise win the issue arbitration by age (step 1.8535 -> 1.8466 ms, two A/B
// rounds on one box; -DJCK_BN_PRIO=0 to compare)
#ifndef JCK_BN_PRIO
#define JCK_BN_PRIO 3
#endif

// ------------------------------------------------------------------------------------------------------
// per-element expressions.  aux layout (floats): [0,C) scale = gamma*invstd   [C,2C) shift = beta - mean*scale
//                                                [2C,3C) mean                 [3C,4C) invstd
// ------------------------------------------------------------------------------------------------------
// the table's four entries for the 8 channels from c on
struct BnAux8 {
  float sc[8], sh[8], mu[8], is[8];
  __device__ __forceinline__ BnAux8(const float* __restrict__ aux, int C, int c) {
#pragma unroll
    for (int k = 0; k < 8; ++k) { sc[k] = aux[c + k]; sh[k] = aux[C + c + k]; mu[k] = aux[2 * C + c + k]; is[k] = aux[3 * C + c + k]; }
  }
};
// m[k] = p[k] * inv_count: a mean out of a sum, formed before it is used
__device__ __forceinline__ void bn_means8(const float* __restrict__ p, float inv_count, float (&m)[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) m[k] = p[k] * inv_count;
}
__device__ __forceinline__ float bn_z(float y, float sc, float sh) { return y * sc + sh; }
__device__ __forceinline__ float bn_xhat(float y, float mu, float is) { return (y - mu) * is; }
__device__ __forceinline__ float bn_act(float z, float slope) { return z > 0.f ? z : slope * z; }
__device__ __forceinline__ float bn_act_grad(float z, float g, float slope) { return z > 0.f ? g : slope * g; }      // act'(z) * g
// backward apply of channel k of the 8: g_y = scale * (g_z - m1 - xhat * m2),  g_z = g_a * act'(z),  m1 = s1/n,  m2 = s2/n
__device__ __forceinline__ float bn_bwd_apply1(float g, float y, const BnAux8& a, int k, float m1, float m2, float slope) {
  const float z = bn_z(y, a.sc[k], a.sh[k]);
  const float gz = bn_act_grad(z, g, slope);
  const float xh = bn_xhat(y, a.mu[k], a.is[k]);
  return a.sc[k] * (gz - m1 - xh * m2);
}

// ------------------------------------------------------------------------------------------------------
// finalize arithmetic: (sum, sum of squares) of a channel in double -> what the aux table, the deferred record and the running
// statistics hold
// ------------------------------------------------------------------------------------------------------
struct BnChannel { float sc, sh, mean, invstd, unbiased; };
__device__ __forceinline__ BnChannel bn_finalize_channel(double sd, double qd, float count, float eps, float gamma, float beta) {
  const double meand = sd / (double)count;
  double vard = qd / (double)count - meand * meand;
  if (vard < 0.0) vard = 0.0;
  const float mean = (float)meand, var = (float)vard;
  const float invstd = 1.0f / sqrtf(var + eps);
  const float sc = gamma * invstd;
  return BnChannel{sc, beta - mean * sc, mean, invstd, var * (count / fmaxf(count - 1.f, 1.f))};
}
__device__ __forceinline__ void bn_write_channel(const BnChannel& b, int c, int C, float* __restrict__ aux, float* __restrict__ stat_out,
                                                 float* __restrict__ running_mean, float* __restrict__ running_var, float momentum) {
  aux[c] = b.sc; aux[C + c] = b.sh; aux[2 * C + c] = b.mean; aux[3 * C + c] = b.invstd;
  if (stat_out) {             // deferred running-stat update (passes that run concurrently on different streams)
    stat_out[c] = b.mean;
    stat_out[C + c] = b.unbiased;
  }
  if (running_mean) {
    running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * b.mean;
    running_var[c] = (1.f - momentum) * running_var[c] + momentum * b.unbiased;
  }
}

// ------------------------------------------------------------------------------------------------------
// The fused kernels' workgroups (BNF_THREADS threads) own a 64-channel SLICE of a pixel range (128 contiguous bytes per row in
// bf16): they sum the partial rows of THEIR channels themselves and stream their pixels.
// ------------------------------------------------------------------------------------------------------
#define BNF_THREADS 256
// The slice sum: rows of NA planes of C floats, row_stride floats apart.  Thread = (row lane, plane, 4 channels): NCOL = NA*16 float4
// columns of a slice row, RL = 256/NCOL row lanes (8, 5, 4 for NA = 2, 3, 4), RU rows of a lane in flight - RU changes the loads in
// flight, not the order of the adds.  Double accumulation in an order fixed by the geometry, through part[RL][NA*64].  Thread
// t < NA*64 returns the total of (plane t >> 6, channel slice*64 + (t & 63)); column t of part[] is read by thread t alone, and the
// first barrier lets the previous call's reads finish: callable repeatedly.
template <int NA, int RU>
__device__ __forceinline__ double bn_slice_sums(const float* __restrict__ rows_ptr, int nrows, long long row_stride, int C, int slice,
                                                double (*part)[NA * 64]) {
  constexpr int NCOL = NA * 16, RL = BNF_THREADS / NCOL;
  const int t = threadIdx.x, q4 = t % NCOL, rl = t / NCOL;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  if (rl < RL) {
    const float* col = rows_ptr + (q4 >> 4) * C + slice * 64 + (q4 & 15) * 4;
    for (int r0 = rl; r0 < nrows; r0 += RL * RU) {
      f32x4 v[RU];
#pragma unroll
      for (int u = 0; u < RU; ++u)
        if (r0 + u * RL < nrows) v[u] = *reinterpret_cast<const f32x4*>(col + (long long)(r0 + u * RL) * row_stride);
#pragma unroll
      for (int u = 0; u < RU; ++u) {
        if (r0 + u * RL >= nrows) break;
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] += (double)v[u][i];
      }
    }
  }
  __syncthreads();
  if (rl < RL) {
#pragma unroll
    for (int i = 0; i < 4; ++i) part[rl][q4 * 4 + i] = acc[i];
  }
  __syncthreads();
  double sd = 0.0;
  if (t < NA * 64) {
#pragma unroll
    for (int k = 0; k < RL; ++k) sd += part[k][t];
  }
  return sd;
}

// The slice streamer: 8 threads per row slice (8 channels = 16 / 32 bytes each), 32 rows per pass, BU rows of a thread in flight
// (few workgroups - each paid for its own sums - so the bytes in flight come from the unroll).  The first BU rows are requested with
// bn_slice_load BEFORE the sums are formed - their latency hides under the row sums - and bn_slice_stream reloads on every trip but
// the first.  body(e, v): e = element offset of the thread's 8 channels in its row, v[i] = those of input i as floats; the body
// stores its outputs itself.
struct BnSlice {
  long long rfirst, rstep;      // this thread's first row, rows per pass of the launch
  int off;                      // first of its 8 channels
  __device__ __forceinline__ BnSlice(int slice) : rfirst((long long)blockIdx.x * 32 + (threadIdx.x >> 3)), rstep((long long)gridDim.x * 32),
                                                  off(slice * 64 + (threadIdx.x & 7) * 8) {}
};
template <typename T, int NIN, int BU>
__device__ __forceinline__ void bn_slice_load(const T* const (&in)[NIN], const BnSlice& sl, long long r0, long long rows, int C, Raw8<T> (&raw)[BU][NIN]) {
#pragma unroll
  for (int u = 0; u < BU; ++u)
    if (r0 + u * sl.rstep < rows) {
#pragma unroll
      for (int i = 0; i < NIN; ++i) ldraw(in[i] + (r0 + u * sl.rstep) * C + sl.off, raw[u][i]);
    }
}
template <typename T, int NIN, int BU, class F>
__device__ __forceinline__ void bn_slice_stream(const T* const (&in)[NIN], const BnSlice& sl, long long rows, int C, Raw8<T> (&raw)[BU][NIN], F&& body) {
  for (long long r0 = sl.rfirst; r0 < rows; r0 += sl.rstep * BU) {
    if (r0 != sl.rfirst) bn_slice_load(in, sl, r0, rows, C, raw);
#pragma unroll
    for (int u = 0; u < BU; ++u) {
      if (r0 + u * sl.rstep >= rows) break;
      float v[NIN][8];
#pragma unroll
      for (int i = 0; i < NIN; ++i) unraw(raw[u][i], v[i]);
      body((r0 + u * sl.rstep) * C + sl.off, v);
    }
  }
}

// ------------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------------
// stats: [slots][2][C] partial sums / sums of squares written by the GEMM epilogue (every slot complete).
// One workgroup per 4 channels: 256 slot-lanes, 16-byte loads, double accumulation, wavefront + LDS reduction.
static __global__ __launch_bounds__(256) void bn_finalize_kernel(const float* __restrict__ stats, int slots, float count,
                                                                 const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                 float* __restrict__ running_mean, float* __restrict__ running_var,
                                                                 long long* __restrict__ nbt, float momentum, float eps,
                                                                 float* __restrict__ aux, int C, float* __restrict__ stat_out = nullptr) {
  __shared__ double sh[4][8];
  const int c0 = blockIdx.x * 4;
  // grouped launch (gridDim.y > 1): group g owns slots [g*slots, (g+1)*slots), aux block g and record g (independent
  // BatchNorm batches that went through ONE conv launch - the D passes that share weights)
  stats += (long long)blockIdx.y * slots * 2 * C;
  aux += (long long)blockIdx.y * 4 * C;
  if (stat_out) stat_out += (long long)blockIdx.y * 2 * C;
  double s[4] = {0, 0, 0, 0}, q[4] = {0, 0, 0, 0};
  // eight rows of this thread's sequence in flight (the rows are 2C floats apart: every load is a line of its own, and a launch with
  // a thousand rows was four to sixteen DEPENDENT memory round trips long - 5-9 us for a kernel that moves a megabyte); the adds
  // stay in sequence order: the same sums, bit for bit
  constexpr int FU = 8;
  for (int k0 = threadIdx.x; k0 < slots; k0 += 256 * FU) {
    f32x4 a[FU], b[FU];
#pragma unroll
    for (int u = 0; u < FU; ++u) {
      const int k = k0 + u * 256;
      if (k < slots) {
        a[u] = *reinterpret_cast<const f32x4*>(stats + (long long)k * 2 * C + c0);
        b[u] = *reinterpret_cast<const f32x4*>(stats + (long long)k * 2 * C + C + c0);
      }
    }
#pragma unroll
    for (int u = 0; u < FU; ++u) {
      if (k0 + u * 256 >= slots) break;
#pragma unroll
      for (int i = 0; i < 4; ++i) { s[i] += (double)a[u][i]; q[i] += (double)b[u][i]; }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) { s[i] = wave_sum_d(s[i]); q[i] = wave_sum_d(q[i]); }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) { sh[threadIdx.x >> 6][i] = s[i]; sh[threadIdx.x >> 6][4 + i] = q[i]; }
  }
  __syncthreads();
  if (blockIdx.x == 0 && threadIdx.x == 0 && nbt) *nbt += 1;
  if (threadIdx.x >= 4) return;
  const int i = threadIdx.x, c = c0 + i;
  const double sd = sh[0][i] + sh[1][i] + sh[2][i] + sh[3][i], qd = sh[0][4 + i] + sh[1][4 + i] + sh[2][4 + i] + sh[3][4 + i];
  bn_write_channel(bn_finalize_channel(sd, qd, count, eps, gamma[c], beta[c]), c, C, aux, stat_out, running_mean, running_var, momentum);
}

// Eval-mode BatchNorm folded into the aux table above from the RUNNING statistics (aten::native_batch_norm, training = false:
// invstd = 1 / sqrt(var + eps), scale = gamma * invstd, shift = beta - mean * scale, each product and sum rounded once:
// contraction is off in the kernel).  Every BatchNorm layer of a network in one launch: a job per layer, a thread
// per channel, block b belongs to the job with first_block[j] <= b < first_block[j + 1].  Nothing but aux is written.
#define BN_EVAL_MAX_JOBS 8
struct BnEvalJob { const float *gamma, *beta, *mean, *var; float* aux; int C; };
struct BnEvalJobs { BnEvalJob j[BN_EVAL_MAX_JOBS]; int first_block[BN_EVAL_MAX_JOBS + 1]; int n; float eps; };
static __global__ __launch_bounds__(256) void bn_eval_aux_kernel(const BnEvalJobs jobs) {
#pragma clang fp contract(off)
  int k = 0;
  while (k + 1 < jobs.n && (int)blockIdx.x >= jobs.first_block[k + 1]) ++k;
  const BnEvalJob& q = jobs.j[k];
  const int c = ((int)blockIdx.x - jobs.first_block[k]) * 256 + (int)threadIdx.x;
  if (c >= q.C) return;
  const float mean = q.mean[c];
  const float invstd = 1.0f / sqrtf(q.var[c] + jobs.eps);
  const float sc = q.gamma[c] * invstd;
  q.aux[c] = sc;
  q.aux[q.C + c] = q.beta[c] - mean * sc;
  q.aux[2 * q.C + c] = mean;
  q.aux[3 * q.C + c] = invstd;
}

// a = act(scale[c]*y + shift[c]), act = x>0 ? x : slope*x, stored at element e of the output
// pitch > 0: the output rows of 2^log_row elements are written `pitch` elements apart - the last layer of CGAN's D lands in the
// concat buffer of the Linear head ([rows][8448], model/CGAN.py:119-121) without a copy
template <typename T>
__device__ __forceinline__ void bn_act_store8(T* __restrict__ a, long long e, int log_row, long long pitch, float (&v)[8], const float* sc,
                                              const float* sh, float slope) {
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = bn_act(bn_z(v[k], sc[k], sh[k]), slope);
  st8(a + (pitch ? (e >> log_row) * pitch + (e & ((1ll << log_row) - 1)) : e), v);
}
template <typename T>
__global__ void bn_act_fwd_kernel(const T* __restrict__ y, const float* __restrict__ aux, float slope,
                                  T* __restrict__ a, long long total8, int C, int log_row = 0, long long pitch = 0) {
  __builtin_amdgcn_s_setprio(JCK_BN_PRIO);
  const long long g0 = (long long)blockIdx.y * total8 * 8;      // first element of this group
  y += g0; aux += (long long)blockIdx.y * 4 * C;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total8; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)((i * 8) & (C - 1));
    float v[8];
    ld8(y + i * 8, v);
    bn_act_store8(a, g0 + i * 8, log_row, pitch, v, aux + c, aux + C + c, slope);
  }
}

// BatchNorm finalize + apply as ONE launch with no hand-over between workgroups (round 5): a workgroup owns a 64-channel slice of a
// pixel range, sums the statistics rows of ITS 64 channels itself - rows of 2 x 64 floats - forms scale / shift in LDS and streams
// its pixels.  What bn_finalize did for everybody in a launch of its own (4.2 us of the step each, measured by skipping them:
// DESIGN.md section 7.2) every workgroup does for itself in ~2 us that overlap its first loads; it pays while the rows are few (the
// gather-GEMMs write one per workgroup).  The workgroups with blockIdx.x == 0 also write the aux table the backward reads, the
// deferred running-statistics record / the running statistics themselves.  aux, stats, stat_out: as bn_finalize_kernel; a: as
// bn_act_fwd_kernel (pitched output included).
template <typename T>
__global__ __launch_bounds__(BNF_THREADS) void bn_fwd_fused_kernel(const T* __restrict__ y, const float* __restrict__ stats, int slots, float count,
                                                                   const float* __restrict__ gamma, const float* __restrict__ beta, float eps, float slope,
                                                                   T* __restrict__ a, float* __restrict__ aux, float* __restrict__ stat_out,
                                                                   float* __restrict__ running_mean, float* __restrict__ running_var,
                                                                   long long* __restrict__ nbt, float momentum, long long rows, int C,
                                                                   int log_row, long long pitch) {
  __shared__ double part[8][128];
  __shared__ float tab[2][64];
  __builtin_amdgcn_s_setprio(JCK_BN_PRIO);
  const int t = threadIdx.x, s = blockIdx.y, grp = blockIdx.z;
  stats += (long long)grp * slots * 2 * C;
  aux += (long long)grp * 4 * C;
  if (stat_out) stat_out += (long long)grp * 2 * C;
  const long long g0 = (long long)grp * rows * C;              // first element of this group
  const BnSlice sl(s);
  const T* const in[1] = {y + g0};
  Raw8<T> raw[4][1];                                          // four rows of this thread in flight
  bn_slice_load(in, sl, sl.rfirst, rows, C, raw);
  // 256 rows: two round trips.  The sum of squares goes over to the thread that holds the sum, through its own column of part[]
  const double tot = bn_slice_sums<2, 16>(stats, slots, 2 * C, C, s, part);
  if (t >= 64 && t < 128) part[0][t] = tot;
  __syncthreads();
  if (t < 64) {
    const int c = s * 64 + t;
    const BnChannel b = bn_finalize_channel(tot, part[0][64 + t], count, eps, gamma[c], beta[c]);
    tab[0][t] = b.sc; tab[1][t] = b.sh;
    if (blockIdx.x == 0) {
      bn_write_channel(b, c, C, aux, stat_out, running_mean, running_var, momentum);
      if (nbt && s == 0 && grp == 0 && t == 0) *nbt += 1;
    }
  }
  __syncthreads();
  float sc[8], sh[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) { sc[k] = tab[0][(t & 7) * 8 + k]; sh[k] = tab[1][(t & 7) * 8 + k]; }
  bn_slice_stream(in, sl, rows, C, raw, [&](long long e, float (&v)[1][8]) { bn_act_store8(a, g0 + e, log_row, pitch, v[0], sc, sh, slope); });
}

// ------------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------------
// stage 1: partial[blk][0..C) = sum g_z,  partial[blk][C..2C) = sum g_z * xhat over this workgroup's rows,
// g_z = g_a * act'(z).  Register accumulation per (row-lane, 8-channel unit), one LDS pass over the row-lanes; no atomics:
// the summation order per (thread, channel) is fixed by the launch geometry alone, so the result is bitwise reproducible.
// Geometry (measured in the step, round 2): <= 256 workgroups per group.  A variant with 1024 workgroups and 4 rows in flight per
// thread (8x the bytes in flight) was SLOWER in the step (29.3 vs 22.1 us average): the kernel runs beside the weight-gradient
// product of the previous layer on the second stream and both are bound by the same memory system.  Two rows in flight at the
// same 256 workgroups (UNR = 2, the default; same summation order, same bits) is the optimum: step 1.867 -> 1.837 ms, UNR 4: 1.853.
#define BN_BWD_MAX_BLOCKS 256
template <typename T, int UNR = 1>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const T* __restrict__ ga, const T* __restrict__ y,
                                                            const float* __restrict__ aux, float slope,
                                                            float* __restrict__ partial, long long rows, int C,
                                                            long long group_stride = 0) {
  extern __shared__ float lsum[];                         // [rstep][2][C]
  __builtin_amdgcn_s_setprio(JCK_BN_PRIO);
  ga += (long long)blockIdx.y * rows * C; y += (long long)blockIdx.y * rows * C;                    // group
  aux += (long long)blockIdx.y * 4 * C; partial += (long long)blockIdx.y * group_stride;
  const int upr = C >> 3;                                 // 8-channel units per row
  const int u = threadIdx.x % upr, r0 = threadIdx.x / upr, rstep = 256 / upr;
  const int c = u * 8;
  const BnAux8 ax(aux, C, c);
  float s1[8], s2[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) { s1[k] = 0.f; s2[k] = 0.f; }
  // UNR rows of this thread's sequence are loaded together and accumulated in sequence order: the same sums, bit for bit,
  // with UNR times the bytes in flight
  const long long stride = (long long)gridDim.x * rstep;
  for (long long r = (long long)blockIdx.x * rstep + r0; r < rows; r += stride * UNR) {
    float vg[UNR][8], vy[UNR][8];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const long long ru = r + u * stride;
      if (ru < rows) { ld8(ga + ru * C + c, vg[u]); ld8(y + ru * C + c, vy[u]); }
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      if (r + u * stride >= rows) break;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float gz = bn_act_grad(bn_z(vy[u][k], ax.sc[k], ax.sh[k]), vg[u][k], slope);
        s1[k] += gz;
        s2[k] += gz * bn_xhat(vy[u][k], ax.mu[k], ax.is[k]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) { lsum[(r0 * 2) * C + c + k] = s1[k]; lsum[(r0 * 2 + 1) * C + c + k] = s2[k]; }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * C; i += 256) {
    float t = 0.f;
    for (int rr = 0; rr < rstep; ++rr) t += lsum[rr * 2 * C + i];
    partial[(long long)blockIdx.x * 2 * C + i] = t;
  }
}

// stage 2: sums[g][0..2C) = sum over workgroups for every group g; dgamma += sum_{g < grad_groups} s2, dbeta likewise (when
// given) - the groups are walked in order inside the workgroup, so the gradient does not depend on any arrival order.
// One workgroup per 4 channels.
static __global__ __launch_bounds__(256) void bn_bwd_sums_kernel(const float* __restrict__ partial, int nblk, float* __restrict__ sums,
                                                                 float* __restrict__ dgamma, float* __restrict__ dbeta, int C,
                                                                 long long group_stride = 0, int groups = 1, int grad_groups = 1,
                                                                 long long partial_group_stride = -1) {
  // groups in chunks of four: the loads of a chunk's groups are in flight together and one barrier pair serves them (the
  // grouped D pass has 3: one memory round trip instead of three; same summation order per group - same bits)
  __shared__ float sh[4][4][8];
  const int c0 = blockIdx.x * 4;
  const long long pgs = partial_group_stride >= 0 ? partial_group_stride : group_stride;
  float dg = 0.f, db = 0.f;
  for (int g0 = 0; g0 < groups; g0 += 4) {
    float s[4][4], q[4][4];
#pragma unroll
    for (int gg = 0; gg < 4; ++gg)
#pragma unroll
      for (int i = 0; i < 4; ++i) { s[gg][i] = 0.f; q[gg][i] = 0.f; }
    for (int k = threadIdx.x; k < nblk; k += 256) {
#pragma unroll
      for (int gg = 0; gg < 4; ++gg) {
        if (g0 + gg >= groups) continue;
        const float* pp = partial + (long long)(g0 + gg) * pgs;
        const f32x4 a = *reinterpret_cast<const f32x4*>(pp + (long long)k * 2 * C + c0);
        const f32x4 b = *reinterpret_cast<const f32x4*>(pp + (long long)k * 2 * C + C + c0);
#pragma unroll
        for (int i = 0; i < 4; ++i) { s[gg][i] += a[i]; q[gg][i] += b[i]; }
      }
    }
#pragma unroll
    for (int gg = 0; gg < 4; ++gg) {
      if (g0 + gg >= groups) continue;
#pragma unroll
      for (int i = 0; i < 4; ++i) { s[gg][i] = wave_sum(s[gg][i]); q[gg][i] = wave_sum(q[gg][i]); }
    }
    __syncthreads();                                        // the previous chunk's sh[] has been read
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int gg = 0; gg < 4; ++gg) {
        if (g0 + gg >= groups) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) { sh[gg][threadIdx.x >> 6][i] = s[gg][i]; sh[gg][threadIdx.x >> 6][4 + i] = q[gg][i]; }
      }
    }
    __syncthreads();
    if (threadIdx.x < 4) {
      const int i = threadIdx.x, c = c0 + i;
      for (int gg = 0; gg < 4 && g0 + gg < groups; ++gg) {
        const int g = g0 + gg;
        const float s1 = sh[gg][0][i] + sh[gg][1][i] + sh[gg][2][i] + sh[gg][3][i];
        const float s2 = sh[gg][0][4 + i] + sh[gg][1][4 + i] + sh[gg][2][4 + i] + sh[gg][3][4 + i];
        sums[(long long)g * group_stride + c] = s1;
        sums[(long long)g * group_stride + C + c] = s2;
        if (g < grad_groups) { dg += s2; db += s1; }
      }
    }
  }
  if (threadIdx.x < 4) {
    const int c = c0 + threadIdx.x;
    if (dgamma) dgamma[c] += dg;
    if (dbeta) dbeta[c] += db;
  }
}

// stage 3: g_y = scale * (g_z - s1/n - xhat * s2/n)       (bn_bwd_apply1)
template <typename T>
__global__ void bn_bwd_apply_kernel(const T* __restrict__ ga, const T* __restrict__ y, const float* __restrict__ aux,
                                    const float* __restrict__ sums, float slope, float inv_count,
                                    T* __restrict__ gy, long long total8, int C, long long group_stride = 0) {
  __builtin_amdgcn_s_setprio(JCK_BN_PRIO);
  ga += (long long)blockIdx.y * total8 * 8; y += (long long)blockIdx.y * total8 * 8; gy += (long long)blockIdx.y * total8 * 8;   // group
  aux += (long long)blockIdx.y * 4 * C; sums += (long long)blockIdx.y * group_stride;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total8; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)((i * 8) & (C - 1));
    float vg[8], vy[8];
    ld8(ga + i * 8, vg);
    ld8(y + i * 8, vy);
    const BnAux8 ax(aux, C, c);
#pragma unroll
    for (int k = 0; k < 8; ++k) vg[k] = bn_bwd_apply1(vg[k], vy[k], ax, k, sums[c + k] * inv_count, sums[C + c + k] * inv_count, slope);
    st8(gy + i * 8, vg);
  }
}

// Backward sums + apply as ONE launch (round 5, the backward twin of bn_fwd_fused_kernel): the three-launch form's middle launch -
// bn_bwd_sums_kernel, 10-13 us on the main stream's chain between two streaming kernels - is done by every workgroup for itself.
// A workgroup owns a 64-channel slice of a pixel range of ONE group, sums the partial rows bn_bwd_reduce_kernel wrote for ITS 64
// channels ([blk][2][C] floats: <= 256 rows of 512 bytes, L2-resident), keeps s1/n, s2/n in LDS and streams its pixels
// (bn_bwd_apply_kernel's arithmetic: bn_bwd_apply1).  The workgroups with blockIdx.x == 0 write the group's sums (CGAN's v-chain
// reads them); those of group 0 also form the parameter gradients: dgamma += sum_{g < grad_groups} s2_g, dbeta likewise, the
// groups walked in order.
template <typename T>
__global__ __launch_bounds__(BNF_THREADS) void bn_bwd_apply_fused_kernel(const T* __restrict__ ga, const T* __restrict__ y, const float* __restrict__ aux,
                                                                         const float* __restrict__ partial, int nblk, float* __restrict__ sums,
                                                                         float* __restrict__ dgamma, float* __restrict__ dbeta, float slope,
                                                                         float inv_count, T* __restrict__ gy, long long rows, int C,
                                                                         long long group_stride, int grad_groups) {
  __shared__ double part[8][128];
  __shared__ float tab[2][64];
  __builtin_amdgcn_s_setprio(JCK_BN_PRIO);
  const int t = threadIdx.x, s = blockIdx.y, grp = blockIdx.z;
  const long long g0 = (long long)grp * rows * C;              // first element of this group
  const BnSlice sl(s);
  const T* const in[2] = {ga + g0, y + g0};
  Raw8<T> raw[2][2];                                          // two rows in flight
  bn_slice_load(in, sl, sl.rfirst, rows, C, raw);
  // thread t < 128: s1 (t < 64) or s2 of channel s*64 + (t & 63)
  const float tot = (float)bn_slice_sums<2, 16>(partial + (long long)grp * group_stride, nblk, 2 * C, C, s, part);
  if (t < 128) {
    tab[t >> 6][t & 63] = tot * inv_count;
    if (blockIdx.x == 0) sums[(long long)grp * group_stride + (t >> 6) * C + s * 64 + (t & 63)] = tot;
  }
  __syncthreads();
  const BnAux8 ax(aux + (long long)grp * 4 * C, C, sl.off);
  float m1[8], m2[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) { m1[k] = tab[0][(t & 7) * 8 + k]; m2[k] = tab[1][(t & 7) * 8 + k]; }
  bn_slice_stream(in, sl, rows, C, raw, [&](long long e, float (&v)[2][8]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) v[0][k] = bn_bwd_apply1(v[0][k], v[1][k], ax, k, m1[k], m2[k], slope);
    st8(gy + g0 + e, v[0]);
  });
  // ---- parameter gradients: the first workgroup of a slice in group 0 walks the gradient groups in order
  if (blockIdx.x == 0 && grp == 0 && (dgamma || dbeta) && grad_groups > 0) {      // (uniform per workgroup)
    float d = tot;
    for (int g = 1; g < grad_groups; ++g) d += (float)bn_slice_sums<2, 16>(partial + (long long)g * group_stride, nblk, 2 * C, C, s, part);
    float* grad = t < 64 ? dbeta : dgamma;
    if (t < 128 && grad) grad[s * 64 + (t & 63)] += d;
  }
}
