// Host glue shared by the launcher units (ops.hip, ops_bn.hip, ops_gemm.hip) and the engine units (engine.hip, engine_infer.hip): error and launch
// macros, the kernel registry, the knobs and the prototypes of the functions that cross a unit.  No kernels: each unit includes the
// kernel headers it launches from.
#pragma once
#include <hip/hip_ext.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "../../include/jckgan.h"
#include "common.hpp"

void jck_set_error(const std::string& s);

// fp32 storage (HBM tensors, packed weights) and the f32 path's kernel choices: JCK_PREC_F32 and JCK_PREC_BF16X3, which differ
// only in the MFMA core of the register-staged GEMM kernels
static inline bool prec_f32_storage(int prec) { return prec == JCK_PREC_F32 || prec == JCK_PREC_BF16X3; }
static inline bool is_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
// workgroups of a grid-stride elementwise launch
static inline unsigned ew_grid(long long n, int per_block = 256) { return (unsigned)std::max<long long>(1, std::min<long long>((n + per_block - 1) / per_block, 8192)); }

#define JCK_FAIL(code, msg)                                   \
  do {                                                        \
    jck_set_error(std::string(__func__) + ": " + (msg));     \
    return (code);                                            \
  } while (0)

#define HIPCHK(expr)                                                                                     \
  do {                                                                                                   \
    hipError_t e_ = (expr);                                                                              \
    if (e_ != hipSuccess) {                                                                              \
      jck_set_error(std::string(__func__) + ": HIP error " + hipGetErrorString(e_) + " at " #expr);     \
      return JCK_E_HIP;                                                                                  \
    }                                                                                                    \
  } while (0)

#define JCK_TRY(expr)           \
  do {                          \
    int rc_ = (expr);           \
    if (rc_ != JCK_OK) return rc_; \
  } while (0)

// launch whose completion hands a tensor to another stream: `ev` (may be null) is completed by the dispatch packet itself
// (hipExtLaunchKernel's stop event) - what a hipEventRecord behind the launch would do with a marker packet of its own, which
// costs the launch stream ~6-7 us of idle time per record on this runtime.  Every kernel argument must be passed explicitly
// (the extended launch checks the count).
#define LAUNCH_EV(kernel, grid, block, shmem, stream, ev, ...)                                                      \
  do {                                                                                                              \
    if (ev) hipExtLaunchKernelGGL(kernel, grid, block, shmem, stream, (hipEvent_t) nullptr, (hipEvent_t)(ev), 0u, __VA_ARGS__); \
    else hipLaunchKernelGGL(kernel, grid, block, shmem, stream, __VA_ARGS__);                                       \
  } while (0)
#define DISPATCH_T(prec, CALL)                                  \
  do {                                                          \
    if ((prec) == JCK_PREC_BF16) { typedef bf16_t T; CALL; }    \
    else if (prec_f32_storage(prec)) { typedef float T; CALL; } \
    else JCK_FAIL(JCK_E_ARG, "bad prec");                       \
  } while (0)

// ---------------------------------------------------------------------------------------------------------
// kernel registry: one id per kernel the library reports on.  KERNELS[id] (ops.hip) holds the id's launch name - what
// jck_last_launch says after a call and jck_launch_name enumerates, one name per kernel; tests assert that a case still lands on the
// kernel it was written for - and its profiler label - what jck_prof_collect hands to bench.py, which merges the persistent and the
// non-persistent forms of a tile.  A read-only report: it selects nothing.  Launch sites name an id or compute one from their
// template parameters with the kid_* functions below; a new kernel is one entry of the table and one launch site.
// ---------------------------------------------------------------------------------------------------------
enum KernelId : int {
  K_PRECS = 3,                                    // bf16, f32, bf16x3
  K_IGEMM_TILES = 5,                              // 128x128, 128x64, 64x128 img, 64x128, 16x256
  K_DMA_TILES = 4,                                // 128x256, 128x128, 128x64, 64x128
  K_WGRAD_TILES = 4,                              // 128x128, 128x64, 64x64 img, 64x64
  K_IGEMM = 0,                                    // + K_IGEMM_TILES * precision + tile     (kid_igemm)
  K_IGEMM_PERSIST = K_IGEMM + K_PRECS * K_IGEMM_TILES,      // + tile                       (kid_igemm_dma)
  K_IGEMM_DMA = K_IGEMM_PERSIST + K_DMA_TILES,              // + tile                       (kid_igemm_dma)
  K_IMG_DOWN = K_IGEMM_DMA + K_DMA_TILES, K_IMG_UP,
  K_WGRAD_DMA_WS, K_WGRAD_DMA,
  K_WGRAD,                                        // + K_WGRAD_TILES * precision + tile     (kid_wgrad)
  K_BN_ACT_FWD = K_WGRAD + K_PRECS * K_WGRAD_TILES, K_BN_BWD_RES, K_BN_BWD_3L,      // profiler labels without a launch name
  K_LATENT_LOSS, K_LATENT_ADAM,                   // latent projection (latent.hpp): labels without a launch name as well
  // the critic's latent gradient: labels without a launch name.  K_CONV_UP_MASK names the leaky mask epilogue in the table only: its
  // launches are timed and reported under the id of the tile they run on, like every other epilogue option
  K_CONV_UP_MASK, K_LEAKY_AFFINE_BWD, K_CRITIC_DS, K_LATENT_LOSS_EX,
  K_FEAT_MATCH,                                   // feature matching on D's activations (latent.hpp): a label without a launch name
  K_IMG_PREP_ANY,                                 // any-size input pipeline (resize.hpp): a label without a launch name, like img_prep_u8_kernel beside it
  K_IMG_PREP_BOX,                                 // the same transform of a box of the source (resize.hpp), likewise a label only
  K_COUNT
};
template <class P> constexpr int kid_prec() { return P::SPLIT ? 2 : P::IS_F32 ? 1 : 0; }
// register-staged gather-GEMM (the fused-epilogue instantiations, enum Epi, report the id of their tile: it says which kernel form and tile ran, not which
// of the epilogue's options - statistics, bias, tanh, the inference affine - it applied)
template <class P, int BCH, int BPIX, int NSUB> constexpr KernelId kid_igemm() {
  static_assert(P::IS_F32 || !(BCH == 64 && NSUB == 1), "bf16 has no register-staged 64 x 128 tile (and no name for one)");
  return KernelId(K_IGEMM + K_IGEMM_TILES * kid_prec<P>() + (BCH == 128 ? (BPIX == 128 ? 0 : 1) : BCH == 64 ? (NSUB == 2 ? 2 : 3) : 4));
}
// LDS-DMA gather-GEMM: family = K_IGEMM_PERSIST or K_IGEMM_DMA
constexpr KernelId kid_igemm_dma(KernelId family, int BCH, int BPIX) { return KernelId(family + (BPIX == 256 ? 0 : BCH == 64 ? 3 : BPIX == 128 ? 1 : 2)); }
template <class P, int BG, int BS, int NSUB> constexpr KernelId kid_wgrad() {
  return KernelId(K_WGRAD + K_WGRAD_TILES * kid_prec<P>() + (BG == 128 ? (BS == 128 ? 0 : 1) : NSUB == 2 ? 2 : 3));
}
// records the id's launch name as the calling thread's last launch
void note_launch(KernelId k);

// optional per-launch timing with HIP events on the launch stream (bench.py's roofline leg; jck_prof_enable).  Off by default:
// zero cost in the timed region.  A launch is priced in algorithmic FLOPs (MFMA kernels) or algorithmic bytes (the streaming
// BatchNorm kernels: bytes > 0).
extern bool g_prof_on;
struct ProfRec { KernelId kernel; double flops, bytes; hipStream_t st; hipEvent_t e0, e1; };
struct ProfScope {
  ProfScope(KernelId k, double flops, hipStream_t st, double bytes = 0.0) : on(g_prof_on) { if (on) begin(k, flops, st, bytes); }
  ~ProfScope() { if (on) end(); }
 private:
  void begin(KernelId k, double flops, hipStream_t st, double bytes);
  void end();
  bool on; ProfRec r;
};
bool jck_prof_is_on();

// kernel-selection knobs (ops.hip: defaults, JCK_<KEY> presets, jck_tune)
extern int g_igemm_dma_ksplit, g_bn_bwd_fuse, g_bn_res, g_wgrad_wgs, g_wgrad_ws, g_wgrad_dma;

// ---------------------------------------------------------------------------------------------------------
// functions that cross a unit
// ---------------------------------------------------------------------------------------------------------
// Adam with {step_size, bc2_sqrt} in device memory (ops.hip): the engine's step has no per-step kernel argument
// ema_w: the generator EMA's weight of this step, written to hp[2] (0: no EMA configured)
int jck_adam_set_step(float* hp, double lr, double beta1, double beta2, int step, unsigned long long seed, float ema_w, hipStream_t st,
                      float* rz = nullptr, long long nz = 0, float* ralpha = nullptr, long long nalpha = 0, float* rmasks = nullptr,
                      long long nmask = 0, float keep_p = 0.75f, float* zero = nullptr, long long nzero = 0, float* zbig0 = nullptr,
                      long long nzbig0 = 0, float* zbig1 = nullptr, long long nzbig1 = 0, void* zpad = nullptr, int zd = 0, int zp = 0,
                      int zpad_f32 = 0);      // zpad: the drawn z also as rows [nz / zd][zp] of type T (G.conv1's operand; padding columns untouched)
int jck_adam_hp(float* p, const float* g, float* m, float* v, long long n, double beta1, double beta2, double eps,
                float grad_scale, const float* hp, hipStream_t st, float* zero = nullptr, long long nzero = 0,
                const unsigned* skip_if = nullptr,       // skip_if: device word; non-zero = leave p, m, v untouched (a grid barrier of the step timed out)
                float* ema = nullptr);                   // ema: moving average of p, advanced in the same launch with the weight in hp[2]
// jck_adam_hp on elements [first, first + count) of the arenas p, g, m, v (ema) AND the repack of every conv weight inside that range, one
// launch (ew_optim.hpp: adam_pack_kernel): `jobs` is the network's repack table (weights that lie outside the range are left out),
// tail (optional) the end-of-step job that rides along.  All arenas 16-byte aligned.
struct PackJobs;
struct TailJobs;
int jck_adam_pack_hp(int prec, float* p, const float* g, float* m, float* v, float* ema, long long first, long long count, const PackJobs& jobs,
                     double beta1, double beta2, double eps, float grad_scale, const float* hp, float step_size, float bc2_sqrt, float ema_w,
                     hipStream_t st, float* zero, long long nzero, const unsigned* skip_if, const TailJobs* tail, int tail_x);
const unsigned* jck_grid_sync_error_word(const void* sync_ws);      // (ops_bn.hip)
// BatchNorm finalize + apply as one launch where the statistics rows are few (ops_bn.hip); *fused = false: nothing was launched
int bn_fwd_fused(int prec, const void* y, const float* stats, int slots_per_group, float count, const float* gamma, const float* beta,
                 float eps, float slope, void* a, float* aux, float* stat_out, float* running_mean, float* running_var, int64_t* nbt,
                 float momentum, long long rows_per_group, int C, int groups, long long out_row, long long out_pitch, hipStream_t stream,
                 bool* fused);
// Internal forms of the two launches whose result another stream waits for: `done` (may be null) is completed by the launch
// that writes the result - the dispatch packet's own completion signal (hipExtLaunchKernel's stop event) instead of a
// hipEventRecord behind it, whose marker packet costs the launch stream ~6-7 us of idle time on this runtime.  The event is an
// explicit argument (round 3 handed it over through a thread-local "armed" slot that the next armable launch consumed).
// (bn_act_bwd_res_ev, bn_act_fwd_pitched: ops_bn.hip; the others: ops.hip)
int bn_act_bwd_res_ev(int prec, const void* g_a, const void* y, const float* aux, float slope, float* sums, void* g_y, float* dgamma,
                      float* dbeta, long long rows_per_group, int C, int groups, int grad_groups, void* sync_ws, hipStream_t stream,
                      hipEvent_t done);
int conv_up_tanh_bwd_ev(int prec, const void* small_in, const void* w, const void* tanh_y, float scale, void* out, int N, int Hs, int Ws,
                        int Cs, int Cb, hipStream_t stream, hipEvent_t done, bool* fused);
int head_bwd_conv2_ev(int prec, const float* ds, const float* wp, const void* a4, int B, int B_more, int C, void* g_a4, float* grad, float* ws,
                      hipStream_t stream, hipStream_t side, hipEvent_t handover);
int gp_head2_ev(int prec, const void* ughd, const float* w2, const float* prob, int B, int K, float* rs, float* dw2, float* ws,
                hipStream_t stream, hipStream_t side, hipEvent_t handover);
int pack_linear_pair(int prec, const float* w, int N, int K, int rows0, int cols0, void* wp0, int rows1, int cols1, void* wp1, int permC,
                     int permHW, hipStream_t stream);
int bn_act_fwd_pitched(int prec, const void* y, const float* aux, float slope, void* a, long long rows_per_group, int C, int groups,
                       long long out_row, long long out_pitch, hipStream_t stream);
int cg_head_mid(int prec, const float* slab, int ksplit, const float* bias1, const float* mask, float scale, void* h, void* hd, const float* w2,
                const float* bias2, int B, int G, const float* targets, const int* modes, float* prob, float* ds, float* scal,
                const int* slot_loss, const int* slot_p, int scal_ld, void* g_hd, void* g_h, hipStream_t stream);
int gp_head_mid_ev(int prec, const float* slab, int ksplit, const float* mask, float scale, void* ughd, const float* w2, const float* prob, int B,
                   float* rs, float* dw2, float* ws, void* g_hd, void* g_h, hipStream_t stream, hipStream_t side, hipEvent_t handover);
int head_fwd_grouped_ev(int prec, const void* a4, const float* wp, const float* bias, int B, int K, int G, const float* targets,
                        const int* modes, float* prob, float* ds, float* scal, const int* slot_loss, const int* slot_p, int scal_ld,
                        void* g_out, hipStream_t stream, hipEvent_t done);
int tanh_bwd_ev(int prec, const void* g, const void* y, float scale, void* out, long long numel, hipStream_t stream, hipEvent_t done);
