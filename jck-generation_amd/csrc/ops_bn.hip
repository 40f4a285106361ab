// C-ABI launchers of the BatchNorm entry points of include/jckgan.h (host side): first order (kernels: bn.hpp), the resident
// one-launch backward (bnres.hpp) and the second-order chains of the gradient penalty (bn2.hpp).  Error string, knobs, the kernel
// registry and the launch profiler: ops.hip.
#include "ops_internal.hpp"
#include "bn2.hpp"
#include "bnres.hpp"

#include <climits>

// the channel counts the streaming kernels take: a power of two (the channel of an element is a mask of its index), 8 per thread;
// the reductions' 256 threads hold a row of up to 2048 (max_c).  The entry points keep their own messages.
static bool bn_channels_ok(int C, int max_c = INT_MAX) { return is_pow2(C) && C >= 8 && C <= max_c; }

// workgroups of the fused BatchNorm launches (forward, and the backward applies): each re-reads its slice's partial rows
// (L2-resident), so more of them cost more than they hide
constexpr int BN_FUSE_WGS = 256;
// grid x of a fused launch: 32 rows per pass and workgroup, C / 64 slices and `groups` groups share BN_FUSE_WGS workgroups
static unsigned bn_slice_grid(long long rows, int C, int groups) {
  const long long per = std::max<long long>(1, BN_FUSE_WGS / ((long long)(C / 64) * groups));
  return (unsigned)std::max<long long>(1, std::min<long long>((rows + 31) / 32, per));
}
// The backward forms (first and second order) as two launches: every workgroup of the apply sums the partial rows of its
// 64-channel slice itself.  The fast path's form: the fp32 parity path keeps the three launches and with them the summation order
// its step tolerances were measured with (a free-running second step amplifies a last-bit change of the sums to 1e-3 of D(G(z)));
// bn_bwd_fuse = 2 takes it there too
static bool bn_two_launches(int prec, int C) { return g_bn_bwd_fuse && C >= 64 && C % 64 == 0 && (prec == JCK_PREC_BF16 || g_bn_bwd_fuse > 1); }

extern "C" int jck_bn_finalize(const float* stats, int slots, float count, const float* gamma, const float* beta,
                               float* running_mean, float* running_var, int64_t* nbt, float momentum, float eps, float* aux,
                               int C, void* stream) {
  if (slots < 1) JCK_FAIL(JCK_E_ARG, "bn_finalize: slots must be >= 1");
  if (C % 4) JCK_FAIL(JCK_E_ARG, "bn_finalize: C % 4 != 0");
  hipLaunchKernelGGL(bn_finalize_kernel, dim3(C / 4), dim3(256), 0, (hipStream_t)stream, stats, slots, count, gamma, beta,
                     running_mean, running_var, (long long*)nbt, momentum, eps, aux, C);
  HIPCHK(hipGetLastError());
  return JCK_OK;
}


extern "C" int jck_bn_eval_aux(int nlayers, const float* const* gamma, const float* const* beta, const float* const* running_mean,
                               const float* const* running_var, float* const* aux, const int* C, float eps, void* stream) {
  if (nlayers < 1 || nlayers > BN_EVAL_MAX_JOBS) JCK_FAIL(JCK_E_ARG, "bn_eval_aux: 1 to " + std::to_string(BN_EVAL_MAX_JOBS) + " layers per launch");
  if (!gamma || !beta || !running_mean || !running_var || !aux || !C) JCK_FAIL(JCK_E_ARG, "bn_eval_aux: null table");
  BnEvalJobs jobs = {};
  jobs.n = nlayers; jobs.eps = eps;
  int blocks = 0;
  for (int k = 0; k < nlayers; ++k) {
    if (C[k] < 1 || !gamma[k] || !beta[k] || !running_mean[k] || !running_var[k] || !aux[k]) JCK_FAIL(JCK_E_ARG, "bn_eval_aux: bad layer " + std::to_string(k));
    jobs.j[k] = BnEvalJob{gamma[k], beta[k], running_mean[k], running_var[k], aux[k], C[k]};
    jobs.first_block[k] = blocks;
    blocks += cdiv(C[k], 256);
  }
  jobs.first_block[nlayers] = blocks;
  hipLaunchKernelGGL(bn_eval_aux_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, jobs);
  HIPCHK(hipGetLastError());
  return JCK_OK;
}

extern "C" int jck_bn_act_fwd(int prec, const void* y, const float* aux, float slope, void* a, long long rows, int C,
                              void* stream) {
  if (!bn_channels_ok(C)) JCK_FAIL(JCK_E_ARG, "bn_act_fwd: C must be a power of two >= 8");
  const long long total8 = rows * C / 8;
  ProfScope prof(K_BN_ACT_FWD, 0.0, (hipStream_t)stream, 2.0 * rows * C * (prec_f32_storage(prec) ? 4 : 2));
  DISPATCH_T(prec, hipLaunchKernelGGL(bn_act_fwd_kernel<T>, dim3(ew_grid(total8)), dim3(256), 0, (hipStream_t)stream,
                                      (const T*)y, aux, slope, (T*)a, total8, C));
  HIPCHK(hipGetLastError());
  return JCK_OK;
}

// finalize + apply in one launch (bn.hpp: bn_fwd_fused_kernel).  Taken while the statistics rows are few (every workgroup sums the rows of
// its channel slice itself); *fused = false and nothing launched otherwise - the caller then issues jck_bn_finalize* + jck_bn_act_fwd*.
constexpr int BN_FUSE_MAX_ROWS = 320;   // statistics rows per group up to which re-reading them in every workgroup still pays
int bn_fwd_fused(int prec, const void* y, const float* stats, int slots_per_group, float count, const float* gamma, const float* beta,
                 float eps, float slope, void* a, float* aux, float* stat_out, float* running_mean, float* running_var, int64_t* nbt,
                 float momentum, long long rows_per_group, int C, int groups, long long out_row, long long out_pitch, hipStream_t stream,
                 bool* fused) {
  *fused = C >= 64 && C % 64 == 0 && is_pow2(C) && slots_per_group >= 1 && slots_per_group <= BN_FUSE_MAX_ROWS && groups >= 1 &&
           (!out_pitch || (out_row >= 8 && !(out_row & (out_row - 1)) && out_pitch >= out_row && out_pitch % 8 == 0));
  if (!*fused) return JCK_OK;
  ProfScope prof(K_BN_ACT_FWD, 0.0, stream, 2.0 * groups * rows_per_group * C * (prec_f32_storage(prec) ? 4 : 2));
  DISPATCH_T(prec, hipLaunchKernelGGL(bn_fwd_fused_kernel<T>, dim3(bn_slice_grid(rows_per_group, C, groups), C / 64, groups), dim3(BNF_THREADS), 0,
                                      stream, (const T*)y, stats, slots_per_group, count, gamma, beta, eps, slope, (T*)a, aux, stat_out,
                                      running_mean, running_var, (long long*)nbt, momentum, rows_per_group, C,
                                      out_pitch ? ilog2((int)out_row) : 0, out_pitch));
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
// C-ABI form: falls back to the two launches itself where the fused form does not apply
extern "C" int jck_bn_fwd(int prec, const void* y, const float* stats, int slots_per_group, float count, const float* gamma, const float* beta,
                          float eps, float slope, void* a, float* aux, float* stat_out, float* running_mean, float* running_var, int64_t* nbt,
                          float momentum, long long rows_per_group, int C, int groups, void* stream) {
  if ((running_mean || nbt) && groups != 1) JCK_FAIL(JCK_E_ARG, "bn_fwd: running statistics are updated in place for ONE group only");
  bool fused = false;
  JCK_TRY(bn_fwd_fused(prec, y, stats, slots_per_group, count, gamma, beta, eps, slope, a, aux, stat_out, running_mean, running_var, nbt, momentum,
                       rows_per_group, C, groups, 0, 0, (hipStream_t)stream, &fused));
  if (fused) return JCK_OK;
  if (slots_per_group < 1 || groups < 1 || C % 4) JCK_FAIL(JCK_E_ARG, "bn_fwd: slots and groups must be >= 1, C % 4 == 0");
  hipLaunchKernelGGL(bn_finalize_kernel, dim3(C / 4, groups), dim3(256), 0, (hipStream_t)stream, stats, slots_per_group, count, gamma, beta,
                     running_mean, running_var, (long long*)nbt, momentum, eps, aux, C, stat_out);
  HIPCHK(hipGetLastError());
  return bn_act_fwd_pitched(prec, y, aux, slope, a, rows_per_group, C, groups, 0, 0, (hipStream_t)stream);
}

extern "C" size_t jck_bn_bwd_ws_floats(int C) { return (size_t)(2 + 2 * BN_BWD_MAX_BLOCKS) * C; }
// workgroups of the backward reduction (see bn_bwd_reduce_kernel for the measurement behind the cap)
static int bn_bwd_blocks(long long rows, int rstep) {
  return (int)std::max<long long>(1, std::min<long long>((rows + rstep * 4 - 1) / (rstep * 4), BN_BWD_MAX_BLOCKS));
}

static int bn_act_bwd_grouped_ev(int prec, const void* g_a, const void* y, const float* aux, float slope, float* sums, void* g_y,
                                 float* dgamma, float* dbeta, long long rows_per_group, int C, int groups, int grad_groups, hipStream_t st,
                                 hipEvent_t done);
extern "C" int jck_bn_act_bwd(int prec, const void* g_a, const void* y, const float* aux, float slope, float* sums,
                              void* g_y, float* dgamma, float* dbeta, long long rows, int C, void* stream) {
  return bn_act_bwd_grouped_ev(prec, g_a, y, aux, slope, sums, g_y, dgamma, dbeta, rows, C, 1, 1, (hipStream_t)stream, nullptr);
}

// Grouped forms: `groups` independent BatchNorm batches stored back to back ([groups][rows][C] tensors, [groups][slots]
// statistics slots, [groups][4C] aux, [groups][jck_bn_bwd_ws_floats(C)] backward workspace).  They serve D passes that
// share weights and went through ONE conv launch (train/dcgan_trainer.py:162,173,118 run D on three batches with the
// same weights); each group is normalised with its own batch statistics exactly as the separate passes are.
extern "C" int jck_bn_finalize_grouped(const float* stats, int slots_per_group, float count, const float* gamma, const float* beta,
                                       float eps, float* aux, float* stat_out, int C, int groups, void* stream) {
  if (slots_per_group < 1 || groups < 1) JCK_FAIL(JCK_E_ARG, "bn_finalize_grouped: slots and groups must be >= 1");
  if (C % 4) JCK_FAIL(JCK_E_ARG, "bn_finalize_grouped: C % 4 != 0");
  hipLaunchKernelGGL(bn_finalize_kernel, dim3(C / 4, groups), dim3(256), 0, (hipStream_t)stream, stats, slots_per_group, count, gamma,
                     beta, (float*)nullptr, (float*)nullptr, (long long*)nullptr, 0.f, eps, aux, C, stat_out);
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
extern "C" int jck_bn_act_fwd_grouped(int prec, const void* y, const float* aux, float slope, void* a, long long rows_per_group,
                                      int C, int groups, void* stream) {
  return bn_act_fwd_pitched(prec, y, aux, slope, a, rows_per_group, C, groups, 0, 0, (hipStream_t)stream);
}
// out_pitch > 0: every out_row (a power of two, >= 8) elements of the output start out_pitch elements apart (bn.hpp: bn_act_store8)
int bn_act_fwd_pitched(int prec, const void* y, const float* aux, float slope, void* a, long long rows_per_group, int C, int groups,
                       long long out_row, long long out_pitch, hipStream_t stream) {
  if (!bn_channels_ok(C) || groups < 1) JCK_FAIL(JCK_E_ARG, "bn_act_fwd_grouped: C must be a power of two >= 8");
  if (out_pitch && (out_row < 8 || (out_row & (out_row - 1)) || out_pitch < out_row || out_pitch % 8))
    JCK_FAIL(JCK_E_ARG, "bn_act_fwd: a pitched output needs rows of a power of two >= 8 elements, pitch >= row, pitch % 8 == 0");
  const long long total8 = rows_per_group * C / 8;
  ProfScope prof(K_BN_ACT_FWD, 0.0, stream, 2.0 * groups * rows_per_group * C * (prec_f32_storage(prec) ? 4 : 2));
  DISPATCH_T(prec, hipLaunchKernelGGL(bn_act_fwd_kernel<T>, dim3(ew_grid(total8), groups), dim3(256), 0, stream,
                                      (const T*)y, aux, slope, (T*)a, total8, C, out_pitch ? ilog2((int)out_row) : 0, out_pitch));
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
extern "C" int jck_bn_act_bwd_grouped(int prec, const void* g_a, const void* y, const float* aux, float slope, float* sums,
                                      void* g_y, float* dgamma, float* dbeta, long long rows_per_group, int C, int groups,
                                      int grad_groups, void* stream) {
  return bn_act_bwd_grouped_ev(prec, g_a, y, aux, slope, sums, g_y, dgamma, dbeta, rows_per_group, C, groups, grad_groups, (hipStream_t)stream, nullptr);
}
// (`done`: completed by the launch that writes g_y)
static int bn_act_bwd_grouped_ev(int prec, const void* g_a, const void* y, const float* aux, float slope, float* sums, void* g_y,
                                 float* dgamma, float* dbeta, long long rows_per_group, int C, int groups, int grad_groups, hipStream_t stream,
                                 hipEvent_t done) {
  if (!bn_channels_ok(C, 2048) || groups < 1) JCK_FAIL(JCK_E_ARG, "bn_act_bwd_grouped: C must be a power of two in [8, 2048]");
  const long long rows = rows_per_group;
  const int rstep = 256 / (C / 8);
  // algorithmic bytes of the backward: read g_a and y once, write g_y (what the resident form moves; this form reads twice)
  ProfScope prof(K_BN_BWD_3L, 0.0, (hipStream_t)stream, 3.0 * groups * rows * C * (prec_f32_storage(prec) ? 4 : 2));
  const int blocks = bn_bwd_blocks(rows, rstep);
  const long long gstride = (long long)jck_bn_bwd_ws_floats(C);
  float* partial = sums + 2 * C;
  DISPATCH_T(prec, hipLaunchKernelGGL((bn_bwd_reduce_kernel<T, 2>), dim3(blocks, groups), dim3(256), 2 * C * rstep * sizeof(float),
                                      (hipStream_t)stream, (const T*)g_a, (const T*)y, aux, slope, partial, rows, C, gstride));
  HIPCHK(hipGetLastError());
  if (bn_two_launches(prec, C)) {       // bn.hpp: bn_bwd_apply_fused_kernel
    DISPATCH_T(prec, LAUNCH_EV(bn_bwd_apply_fused_kernel<T>, dim3(bn_slice_grid(rows, C, groups), C / 64, groups), dim3(BNF_THREADS), 0,
                               (hipStream_t)stream, done, (const T*)g_a, (const T*)y, (const float*)aux, (const float*)partial, blocks, sums,
                               dgamma, dbeta, slope, 1.0f / (float)rows, (T*)g_y, rows, C, gstride, grad_groups));
    HIPCHK(hipGetLastError());
    return JCK_OK;
  }
  hipLaunchKernelGGL(bn_bwd_sums_kernel, dim3(C / 4), dim3(256), 0, (hipStream_t)stream, partial, blocks, sums, dgamma, dbeta, C,
                     gstride, groups, grad_groups);
  HIPCHK(hipGetLastError());
  const long long total8 = rows * C / 8;
  DISPATCH_T(prec, LAUNCH_EV(bn_bwd_apply_kernel<T>, dim3(ew_grid(total8), groups), dim3(256), 0, (hipStream_t)stream, done,
                             (const T*)g_a, (const T*)y, (const float*)aux, (const float*)sums, slope, 1.0f / (float)rows, (T*)g_y, total8, C, gstride));
  HIPCHK(hipGetLastError());
  return JCK_OK;
}

// Resident form (bnres.hpp): one launch per layer, every tensor byte read once, the groups one after the other.  Falls back to
// the three-launch form above when the layer does not fit the register file of the chip (or is not bf16, or JCK_BN_RES=0).
static int bnres_cus() {
  static int cus = [] {
    int dev = 0; hipDeviceProp_t pr;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&pr, dev) != hipSuccess) return 0;
    return pr.multiProcessorCount;
  }();
  return cus;
}
extern "C" size_t jck_grid_sync_bytes(void) { return BNRES_SYNC_BYTES; }
// 1 if a grid barrier of a resident launch timed out since the state was last zeroed (synchronises the device)
const unsigned* jck_grid_sync_error_word(const void* sync_ws) { return sync_ws ? (const unsigned*)sync_ws + BNRES_W_ERR * 32 : nullptr; }
extern "C" int jck_grid_sync_error(const void* sync_ws) {
  unsigned err = 0;
  if (!sync_ws) return 0;
  if (hipMemcpy(&err, (const unsigned*)sync_ws + BNRES_W_ERR * 32, sizeof(err), hipMemcpyDeviceToHost) != hipSuccess) return 1;
  return err != 0;
}
// multi-group passes take the resident form above this many MB of (g_a, y): below it their second read comes out of the Infinity Cache
constexpr int BN_RES_MIN_MB = 120;
// nb workgroups (all co-resident), nsl channel slices, ng groups resident together, chunks per thread; 0 = does not fit
static int bnres_plan(int prec, long long rows, int C, int groups, int* nb_out, int* nsl_out, int* ng_out) {
  if (!g_bn_res || prec != JCK_PREC_BF16 || !is_pow2(C) || C < 64 || groups < 1 || rows < 1) return 0;
  // Several groups in one pass (the batched D pass): the three-launch form's second read of (g_a, y) comes out of the
  // Infinity Cache while all groups fit it, and then it is as fast or faster in the step (measured, DESIGN.md section 5.3:
  // D.conv2's layer at 3 x 256 images 60 vs 70 us alone, the step 1.744 vs 1.733 ms); the resident form wins where they do not
  // fit (D.conv1's layer: 3 x 2 x 33.5 MB, or 2 x 2 x 33.5 MB for its loss groups alone).  bn_res = 2 takes the resident form whenever it fits the registers.
  if (g_bn_res == 1 && groups > 1 && (long long)groups * rows * C * 4 <= ((long long)BN_RES_MIN_MB << 20)) return 0;
  const int nsl = C / 64;
  int nb = std::min(bnres_cus(), 256);
  nb -= nb % std::max(nsl, 8);
  if (nb < nsl || nb < 8) return 0;
  if ((long long)groups * rows * C * 2 >= (1ll << 40)) return 0;
  const long long per_iter = (long long)(nb / nsl) * BNRES_ROWS;
  const long long need = (rows + per_iter - 1) / per_iter;
  if (need > 16) return 0;
  const int nch = need <= 1 ? 1 : need <= 2 ? 2 : need <= 4 ? 4 : need <= 8 ? 8 : 16;
  *nb_out = nb; *nsl_out = nsl;
  // groups resident together (one barrier for all of them) while their chunks fit the register file
  *ng_out = (groups >= 3 && 3 * nch <= 16) ? 3 : (groups >= 2 && 2 * nch <= 16) ? 2 : 1;
  return nch;
}
// the plan of jck_bn_act_bwd_res for these arguments, given a barrier workspace: 1 and (chunks, resident groups, workgroups), or 0
// where that call takes the three-launch form.  Host only (the CU count is asked of the runtime once).
extern "C" int jck_bn_res_plan(int prec, long long rows_per_group, int C, int groups, int* nch, int* ng, int* nb) {
  int b = 0, sl = 0, g = 0;
  const int ch = bnres_plan(prec, rows_per_group, C, groups, &b, &sl, &g);
  if (!ch) return 0;
  if (nch) *nch = ch;
  if (ng) *ng = g;
  if (nb) *nb = b;
  return 1;
}
extern "C" int jck_bn_act_bwd_res(int prec, const void* g_a, const void* y, const float* aux, float slope, float* sums, void* g_y,
                                  float* dgamma, float* dbeta, long long rows_per_group, int C, int groups, int grad_groups,
                                  void* sync_ws, void* stream) {
  return bn_act_bwd_res_ev(prec, g_a, y, aux, slope, sums, g_y, dgamma, dbeta, rows_per_group, C, groups, grad_groups, sync_ws,
                           (hipStream_t)stream, nullptr);
}
int bn_act_bwd_res_ev(int prec, const void* g_a, const void* y, const float* aux, float slope, float* sums, void* g_y, float* dgamma,
                      float* dbeta, long long rows_per_group, int C, int groups, int grad_groups, void* sync_ws, hipStream_t stream,
                      hipEvent_t done) {
  int nb = 0, nsl = 0, ng = 0;
  const int nch = sync_ws ? bnres_plan(prec, rows_per_group, C, groups, &nb, &nsl, &ng) : 0;
  if (!nch) return bn_act_bwd_grouped_ev(prec, g_a, y, aux, slope, sums, g_y, dgamma, dbeta, rows_per_group, C, groups, grad_groups, stream, done);
  BnResParams p;
  p.ga = (const bf16_t*)g_a; p.y = (const bf16_t*)y; p.gy = (bf16_t*)g_y; p.aux = aux;
  p.sums = sums; p.sums_stride = (long long)jck_bn_bwd_ws_floats(C);
  p.dgamma = dgamma; p.dbeta = dbeta; p.sync = (unsigned*)sync_ws;
  p.rows = rows_per_group; p.C = C; p.groups = groups; p.grad_groups = grad_groups; p.nb = nb; p.nsl = nsl;
  p.slope = slope; p.inv_count = 1.0f / (float)rows_per_group;
  const dim3 grid(nb), block(BNRES_THREADS);
  ProfScope prof(K_BN_BWD_RES, 0.0, stream, 3.0 * groups * rows_per_group * C * 2);
#define BNRES_CASE(NCH_, NG_) case NCH_ * 4 + NG_: LAUNCH_EV((bn_bwd_res_kernel<NCH_, NG_>), grid, block, 0, stream, done, p); break
  switch (nch * 4 + ng) {
    BNRES_CASE(1, 1); BNRES_CASE(2, 1); BNRES_CASE(4, 1); BNRES_CASE(8, 1); BNRES_CASE(16, 1);
    BNRES_CASE(1, 2); BNRES_CASE(2, 2); BNRES_CASE(4, 2); BNRES_CASE(8, 2);
    BNRES_CASE(1, 3); BNRES_CASE(2, 3); BNRES_CASE(4, 3);
    default: JCK_FAIL(JCK_E_ARG, "bn_act_bwd_res: no kernel for this plan");
  }
#undef BNRES_CASE
  HIPCHK(hipGetLastError());
  return JCK_OK;
}

// ---------------------------------------------------------------------------------------------------------
// second order (bn2.hpp): reduce, then sums + apply, or the apply that sums its slice itself (bn_two_launches)
// ---------------------------------------------------------------------------------------------------------
// v-chain step of the penalty's double backward at one BatchNorm layer.  ws: jck_bn2_ws_floats(C) floats; on return
// ws[0..3C) = {sum v, sum v*xhat, sum v*gy} (keep it for jck_bn2_reverse).  u may alias v.
extern "C" size_t jck_bn2_ws_floats(int C) { return (size_t)(4 + 4 * BN_BWD_MAX_BLOCKS) * C; }
extern "C" int jck_bn2_vchain(int prec, const void* v, const void* y, const void* gy, const float* aux, const float* s1,
                              const float* gamma, float slope, float* ws, void* u, void* xdir, float* dgamma, long long rows, int C,
                              void* stream) {
  if (!bn_channels_ok(C, 2048)) JCK_FAIL(JCK_E_ARG, "bn2_vchain: C must be a power of two in [8, 2048]");
  const int rstep = 256 / (C / 8);
  const int blocks = bn_bwd_blocks(rows, rstep);
  float* partial = ws + 4 * C;
  DISPATCH_T(prec, hipLaunchKernelGGL((bn2_reduce_kernel<T, 1>), dim3(blocks), dim3(256), 3 * C * rstep * sizeof(float),
                                      (hipStream_t)stream, (const T*)v, (const T*)y, (const T*)gy, aux, slope, partial, rows, C));
  HIPCHK(hipGetLastError());
  if (bn_two_launches(prec, C)) {
    DISPATCH_T(prec, hipLaunchKernelGGL(bn2_vchain_apply_fused_kernel<T>, dim3(bn_slice_grid(rows, C, 1), C / 64), dim3(BNF_THREADS), 0,
                                        (hipStream_t)stream, (const T*)v, (const T*)y, (const T*)gy, aux, s1, (const float*)partial, blocks, ws,
                                        gamma, dgamma, slope, 1.0f / (float)rows, (T*)u, (T*)xdir, rows, C));
    HIPCHK(hipGetLastError());
    return JCK_OK;
  }
  hipLaunchKernelGGL(bn2_sums_kernel, dim3(3 * C / 4), dim3(256), 0, (hipStream_t)stream, partial, blocks, 3, C, ws, dgamma ? 1 : 0, gamma,
                     dgamma, (float*)nullptr);
  HIPCHK(hipGetLastError());
  const long long total8 = rows * C / 8;
  DISPATCH_T(prec, hipLaunchKernelGGL(bn2_vchain_apply_kernel<T>, dim3(ew_grid(total8)), dim3(256), 0, (hipStream_t)stream, (const T*)v,
                                      (const T*)y, (const T*)gy, aux, s1, ws, slope, 1.0f / (float)rows, (T*)u, (T*)xdir, total8, C));
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
// reverse-sweep BatchNorm backward with the penalty's extra inputs (xdir, sum v*gy from the v-chain at vsums[2C..3C)).
// The parameter gradients are formed when both dgamma and dbeta are given.
extern "C" int jck_bn2_reverse(int prec, const void* ua, const void* y, const void* xdir, const float* aux, const float* gamma,
                               const float* vsums, float slope, float* ws, void* uy, float* dgamma, float* dbeta, long long rows,
                               int C, void* stream) {
  if (!bn_channels_ok(C, 2048)) JCK_FAIL(JCK_E_ARG, "bn2_reverse: C must be a power of two in [8, 2048]");
  const int rstep = 256 / (C / 8);
  const int blocks = bn_bwd_blocks(rows, rstep);
  float* partial = ws + 4 * C;
  const bool grads = dgamma && dbeta;
  DISPATCH_T(prec, hipLaunchKernelGGL((bn2_reduce_kernel<T, 2>), dim3(blocks), dim3(256), 4 * C * rstep * sizeof(float),
                                      (hipStream_t)stream, (const T*)ua, (const T*)y, (const T*)xdir, aux, slope, partial, rows, C));
  HIPCHK(hipGetLastError());
  if (bn_two_launches(prec, C)) {
    DISPATCH_T(prec, hipLaunchKernelGGL(bn2_reverse_apply_fused_kernel<T>, dim3(bn_slice_grid(rows, C, 1), C / 64), dim3(BNF_THREADS), 0,
                                        (hipStream_t)stream, (const T*)ua, (const T*)y, (const T*)xdir, aux, gamma, (const float*)partial, blocks,
                                        ws, vsums + 2 * C, grads ? dgamma : nullptr, grads ? dbeta : nullptr, slope, 1.0f / (float)rows,
                                        (T*)uy, rows, C));
    HIPCHK(hipGetLastError());
    return JCK_OK;
  }
  hipLaunchKernelGGL(bn2_sums_kernel, dim3(4 * C / 4), dim3(256), 0, (hipStream_t)stream, partial, blocks, 4, C, ws, grads ? 2 : 0,
                     (const float*)nullptr, dgamma, dbeta);
  HIPCHK(hipGetLastError());
  const long long total8 = rows * C / 8;
  DISPATCH_T(prec, hipLaunchKernelGGL(bn2_reverse_apply_kernel<T>, dim3(ew_grid(total8)), dim3(256), 0, (hipStream_t)stream,
                                      (const T*)ua, (const T*)y, (const T*)xdir, aux, gamma, ws, vsums + 2 * C, slope,
                                      1.0f / (float)rows, (T*)uy, total8, C));
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
