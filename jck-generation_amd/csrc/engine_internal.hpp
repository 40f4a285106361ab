// What the step engine (engine.hip) and the inference entry points beside it (engine_infer.hip) share: the engine object with its
// layout, channel plan and buffers, the name tables and constants, and the generator forward that both sides run.
#pragma once
#include <cstring>
#include <vector>

#include "ops_internal.hpp"
#include "ew_optim.hpp"      // pad_rows_kernel (launch_pad_rows)
#define JCK_INTERNAL __attribute__((visibility("hidden")))      /* shared by the two files, not exported from the library */
struct jck_engine;
#define TT (e->T)        /* the engine's channel plan; `e` is the engine in every function below (this inside its members) */

namespace jck_eng JCK_INTERNAL {

struct TensorInfo { const char* name; int kind; long long offset, numel; int shape[4]; };

struct NetLayout {
  std::vector<TensorInfo> t;
  long long n_params = 0, n_bn = 0;
};

// Channel plan.  S = 64 is the reference's topology (model/DCGAN.py:10-26, :42-58): NS = 4 stride-2 stages, 512 channels at
// the 4x4 end.  S = 128 (BASELINE.json configs[4]; no reference behaviour exists - SURVEY section 8d) adds ONE stage at the
// deep end, the usual way a DCGAN is grown: D 3 -> 64 -> 128 -> 256 -> 512 -> 1024 -> 1, G 100 -> 1024 -> ... -> 64 -> 3,
// so every layer keeps >= 64 channels on its wide side and the image-side layers stay 3 <-> 64.
#define JCK_MAX_STAGES 5
struct Topo {
  int S, NS, HW;                       // image size, stride-2 stages, S*S
  int D_CS[JCK_MAX_STAGES], D_CB[JCK_MAX_STAGES], D_HB[JCK_MAX_STAGES];
  int G_CS[JCK_MAX_STAGES], G_CB[JCK_MAX_STAGES], G_HS[JCK_MAX_STAGES];     // G.conv2 .. G.conv(NS+1)
  int G_C1, FEAT;                      // channels at the 4x4 end; D's flattened top features 16*G_C1
};
const int N_CLASS = 100, EMB = 200, L1_OUT = 256, L1_FEAT = 8192, L1_K = L1_FEAT + EMB, L1_KPAD = 8448;   // model/CGAN.py:83,104
// split-K of Linear(8392, 256): 132 k-steps of 64 over L1_KSPLIT workgroups per tile (a divisor of 132; hipgan/functional.py uses the same)
constexpr int L1_KSPLIT = 12;
inline int z_dim(int family) { return family == 1 ? 200 : 100; }      // model/CGAN.py:132: ConvTranspose2d(200, 512)
inline int z_pad(int family) { return family == 1 ? 256 : 128; }

static const char* const CWN[6] = {"conv1.weight", "conv2.weight", "conv3.weight", "conv4.weight", "conv5.weight", "conv6.weight"};
static const char* const NWN[5] = {"norm1.weight", "norm2.weight", "norm3.weight", "norm4.weight", "norm5.weight"};
static const char* const NBN[5] = {"norm1.bias", "norm2.bias", "norm3.bias", "norm4.bias", "norm5.bias"};
static const char* const RMN[5] = {"norm1.running_mean", "norm2.running_mean", "norm3.running_mean", "norm4.running_mean", "norm5.running_mean"};
static const char* const RVN[5] = {"norm1.running_var", "norm2.running_var", "norm3.running_var", "norm4.running_var", "norm5.running_var"};

inline const TensorInfo* find(const NetLayout& L, const char* name) {
  for (auto& t : L.t) if (!strcmp(t.name, name)) return &t;
  return nullptr;
}

struct Carver {
  size_t off = 0;
  unsigned char* base = nullptr;
  template <typename T> T* take(size_t count) {
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off = (off + count * sizeof(T) + 255) / 256 * 256;
    return p;
  }
};

struct BnBuf { float *stats, *sums, *aux; int slots; };      // G's BatchNorm buffers of one stage

// D's activations for `cap` batches of B images stored back to back (cap = 1: the set of one pass, 3: the batched schedule's
// [real | fake | penalty]), or a view of `groups` of them from group `g0` on.  Per stage: conv output y, activation a, gradient g,
// BatchNorm statistic slots / scale-shift table / backward sums.  Per set: probabilities and logit gradients, and - the penalty
// pass - the gradient w.r.t. its input image and that gradient's per-image norms.
struct DActs {
  void *y[JCK_MAX_STAGES], *a[JCK_MAX_STAGES], *g[JCK_MAX_STAGES], *gx;
  float *stats[JCK_MAX_STAGES], *aux[JCK_MAX_STAGES], *sums[JCK_MAX_STAGES], *prob, *ds, *norms;
  int cap, g0, groups;
  DActs group(const jck_engine* e, int first, int n) const;      // groups [first, first + n) of this set or view
};

}  // namespace jck_eng
using namespace jck_eng;

static const float BN_MOM = 0.1f, BN_EPS = 1e-5f, LRELU = 0.2f;

// What one phase call leaves behind for a later one - the state of the step in flight.  Everything else in jck_engine is
// configuration, buffers, streams or the per-call selection (parity, acc, scal_out, cur_labels) that every phase call makes anew.
struct StepState {
  bool gp_done = false;                 // the penalty's forward and first backward ran as group 2 of the batched pass (PHASE_D_LOSS / _B; consumed by PHASE_D_GP)
  bool gp_inflight = false;             // the penalty pass runs on sC, evGP behind it (per-pass PHASE_D_LOSS / PHASE_D_FAKE; joined by PHASE_D_GP)
  bool join_pending = false, mid_recorded = false;    // PHASE_LAZY_JOIN: evWdone (and evWmid) recorded on sA, not yet waited for
  long long real_fwd_step = -1;         // step whose D(real) forward already ran (PHASE_D_REAL_FWD), -1: none
  bool tail_on_side = false, pre_on_side = false;       // PHASE_D_LOSS_A's tail marker sits on sA; PHASE_D_REAL_FWD ran on sA (evReal)
  int head_row0 = 0;                    // CGAN: first row of the head state (h_drop, cbuf, pre_e) the pass in hand READS (2B: penalty group of a batched head)
  int head_wrow0 = 0;                   //       first row of the head buffers it WRITES (g_hd, g_h, gc)
  int acc_clean_step = -1;              // the step whose accumulator rows jck_engine_set_step has just cleared (consumed by its first D phase)
  // zero_grad() without a launch of its own: D's gradient arena (+ CGAN's permuted Linear gradient) is cleared by the set-step
  // launch of the step's first D phase, G's by D's Adam launch; the step whose arena is clean (consumed by the phase that would memset)
  int dg_clean_step = -1, gg_clean_step = -1;
  long long gz_step = -1;               // the step whose set-step launch wrote its own z into g_z (G.conv1's operand) as well
  // a phase that failed half way leaves no promise behind: the next D phase clears its arenas itself and joins the
  // weight-gradient stream before anything else (state armed before a failing call must not outlive it)
  void drop_promises() { acc_clean_step = dg_clean_step = gg_clean_step = -1; join_pending = mid_recorded = false; }
  // PHASE_GP_ONLY clears the accumulator rows and D's gradient arena itself and runs the penalty as a pass of its own on set 0
  void begin_gp_only() { acc_clean_step = dg_clean_step = -1; gp_done = gp_inflight = false; head_row0 = head_wrow0 = 0; }
};
struct jck_engine {
  int family, prec, B;
  Topo T;
  size_t esz;
  NetLayout LG, LD;
  size_t ws_bytes = 0;
  bool bound = false;
  // arenas
  float *gp = nullptr, *gg = nullptr, *gm = nullptr, *gv = nullptr, *gbn = nullptr;
  float *dp = nullptr, *dg = nullptr, *dm = nullptr, *dv = nullptr, *dbn = nullptr;
  int64_t *gnbt = nullptr, *dnbt = nullptr;
  // exponential moving average of G's parameters (jck_engine_bind_ema; null: none): advanced by Adam(G)'s launch with the weight
  // jck_engine_set_ema configures - 1 below ema_start (the average tracks the weights), 1 - decay from there on
  float* gema = nullptr;
  double ema_decay = 0.0; int ema_start = 0;
  float ema_w(int step) const { return !gema ? 0.f : (step < ema_start ? 1.f : (float)(1.0 - ema_decay)); }
  int graph_nodes = 0;                  // nodes of the graph jck_engine_capture_end instantiated last
  // packed weights
  void *d_down[JCK_MAX_STAGES], *d_up[JCK_MAX_STAGES];
  float *d_head_wp, *d_head_dwp;
  void *g1_w, *g_up[JCK_MAX_STAGES], *g_down[JCK_MAX_STAGES];
  // activations: three B-image D sets for the per-pass schedules (each pass that may run concurrently has its own)
  DActs dset[3] = {};                   // 0: D(fake) and the G-phase pass, 1: penalty pass, 2: D(real) (may overlap the previous step's G phase)
  // batched D passes: up to 3 batches that share D's weights go through ONE launch per layer, BatchNorm grouped.  The penalty
  // group's image gradient and norms go where the per-pass schedule leaves them: bset.gx / .norms are dset[0]'s
  DActs bset = {};
  int batched = 0;                      // 0: one D pass per batch (batch % 8 != 0, JCK_BATCHED=0), 3: [real | fake | penalty] as ONE 3B pass
  StepState ss;                         // what the phases of a step hand to one another
  float* d_rs[JCK_MAX_STAGES];                       // deferred BatchNorm running-stat records of D: [step parity][pass 0..3][2*C] per layer
  int parity = 0;                       // step & 1: selects the scalar accumulators and the BN records of the step in flight
  // side streams: A = weight gradients beside the dgrad chain, B = G forward beside D(real), C = penalty pass beside D(fake)
  hipStream_t sA = nullptr, sB = nullptr, sC = nullptr;
  hipEvent_t evW[JCK_MAX_STAGES] = {}, evWdone = nullptr, evWmid = nullptr, evHead = nullptr, evTail = nullptr, ev0 = nullptr, evF = nullptr, evReal = nullptr, evGP = nullptr;
  template <typename F> void for_each_side_stream(F f) { for (hipStream_t* p : {&sA, &sB, &sC}) f(*p); }
  template <typename F> void for_each_event(F f) {
    for (hipEvent_t* p : {&evWdone, &evWmid, &evHead, &evTail, &ev0, &evF, &evReal, &evGP}) f(*p);
    for (hipEvent_t& p : evW) f(p);
  }
  bool overlap = true, defer_join = true;
  bool wgrad_side = true;               // weight gradients beside the dgrad chain on sA (JCK_WGRAD_SIDE=0: on the main stream)
  bool head_side = true;                // the head's parameter gradients on sA as well (JCK_HEAD_SIDE=0: on the main stream)
  // cross-stream hand-overs of the backward: the producing launch completes the event itself (the `done` argument of
  // bn_act_bwd_res_ev / tanh_bwd_ev: hipExtLaunchKernel's stop event) instead of a
  // hipEventRecord behind it; JCK_EXT_EVENTS=0 restores the records
  bool ext_events = true;
  // resident one-launch BatchNorm backward (bnres.hpp): grid-barrier state (zeroed at bind); JCK_BN_RES=0 switches it off
  unsigned* gsync = nullptr; bool bn_res = true;
  bool cbuf_direct = true;              // CGAN: D's last BatchNorm+LeakyReLU writes straight into the head's concat buffer (JCK_CBUF_DIRECT=0: a copy)
  bool head_fuse = true;                // CGAN: Linear finish + Linear(256,1)/sigmoid/BCE + its input gradient + Dropout backward as one launch; DCGAN: conv5's
                                        // forward writes its input gradient too (JCK_HEAD_FUSE=0: separate launches)
  bool real_side = true;                // batched D pass: D(real)'s forward beside G's forward on the weight-gradient stream (JCK_REAL_SIDE=0: one 3B forward)
  bool fold_zero = true;                // zero_grad() of both networks inside neighbouring launches (JCK_FOLD_ZERO=0: memsets)
  bool fuse_tanh = true;                // G's loss pass: tanh backward in the epilogue of D.conv1's input gradient (JCK_FUSE_TANH=0: a launch of its own)
  bool adam_pack = true;                // an optimiser phase's Adam writes the packed operands itself, one launch per network (JCK_ADAM_PACK=0: Adam, then the repack)
  void *g_z, *g_y[JCK_MAX_STAGES], *g_a[JCK_MAX_STAGES], *g_gr[JCK_MAX_STAGES], *fake_raw, *fake, *g_raw;
  void *real_noisy, *xhat;
  // small buffers
  BnBuf g_bn[JCK_MAX_STAGES];
  float *acc, *scal_out;                // current-parity views into acc2 / scal2
  float *acc2, *scal2;                  // acc2: [2 parities][8 rows][acc_ld] per-image scalar table (summed by the step tail)
  int acc_ld = 0;
  float *head_ws, *gp2_ws;              // partial rows of the head weight gradients (deterministic two-stage sums)
  float* hp2;                           // [2 parities][8]: {step_size, bc2_sqrt, EMA weight, -, noise seed lo, hi, step, 0} of the step in flight (jck_engine_set_step)
  unsigned long long noise_seed = 0x6a636b67616e0001ull;      // in-kernel instance noise (jck_engine_set_noise_seed)
  float *rz[2] = {nullptr, nullptr}, *ralpha[2] = {nullptr, nullptr}, *rmask[2] = {nullptr, nullptr};
  int hp_step[2] = {0, 0};              // which step's scalars each parity holds (checked by the optimiser phases) ...
  float hp_lr[2] = {-1.f, -1.f};        // ... and at which learning rate they were computed (a scheduler may change it between steps)
  bool hp_holds(int step, float lr) const { return hp_step[step & 1] == step && hp_lr[step & 1] == lr; }
  bool capturing = false;
  bool gp_bwd = false;                  // DCGAN created with JCK_ENGINE_GP_BACKWARD: PHASE_D_GP back-propagates the penalty as CGAN's does
  float* g1_ws = nullptr; size_t g1_ws_bytes = 0;
  float* wg_ws; size_t wg_ws_bytes;
  // family 1 (CGAN): Linear head, label path, second-order penalty buffers
  void *l1_w, *l1_wT;                 // packed linear1: [256][8448] and transposed [8448][256]
  void *cbuf, *cbuf2;                 // [B][8448] concat(flatten(a4), e) ; [u4 | 0]
  void *h_pre, *h_drop, *g_h, *g_hd, *gh_b1, *ughd, *gc;    // [B][256] x6, [B][8448]
  float *pre_e, *l1_slab, *gw1p, *rs, *prob_gp;
  void *d_v[JCK_MAX_STAGES], *d_xdir[JCK_MAX_STAGES], *d_u0;
  float* bn2_ws[JCK_MAX_STAGES]; float* bn2_ws_rev;
  const int64_t* cur_labels = nullptr;
  // The four buffer groups of the inference side (engine_infer.hip): each is memory of its own, ONE allocation made by the first call
  // that needs the group (infer_alloc carves it) and freed with the engine (infer_free).
  // latent projection (jck_engine_latent_grad / jck_engine_project): G.conv1's weight as the dz product's operand [128][16 * G_C1], that
  // product's split-K slabs, a loss row
  struct LatentBufs {
    void* base = nullptr;
    void* w = nullptr; float *slab = nullptr, *loss = nullptr;
  } lat;
  // discriminator inference (jck_engine_score): the transformed input, a stage's activations and folded aux table each, one
  // pre-activation tensor that the stages share (bf16: see jck_engine_score), and CGAN's head rows (concat buffer, split-K slabs,
  // hidden row)
  struct ScoreBufs {
    void* base = nullptr;
    void *x = nullptr, *y = nullptr, *a[JCK_MAX_STAGES] = {}, *cbuf = nullptr, *h = nullptr;
    float *aux[JCK_MAX_STAGES] = {}, *slab = nullptr;
  } sc;
  // the critic's latent gradient (jck_engine_latent_grad_ex / jck_engine_project_ex with critic_mode != 0, or a feature term): the
  // gradient at every stage's pre-activation, the image gradient (NHWC4), the rows ds / term / logit, and CGAN's gradient rows at the
  // Linear(8392,256) output and at the concat buffer
  struct CriticBufs {
    void* base = nullptr;
    void *g[JCK_MAX_STAGES] = {}, *gx = nullptr, *g_h = nullptr, *gc = nullptr;
    float *ds = nullptr, *term = nullptr, *logit = nullptr;
  } cr;
  // the feature-matching term (jck_engine_latent_grad_fm / jck_engine_project_fm with a feature target): the target's activation at the
  // chosen stage, with room for the largest stage (stage 0), and a row for the term
  struct FeatBufs {
    void* base = nullptr;
    void* fa = nullptr; float* term = nullptr;
  } fm;
  bool d_packed = false;               // D's operands were derived from its parameters at least once (jck_engine_repack, a D step)

  void carve(unsigned char* base) {
    jck_engine* e = this;
    Carver c; c.base = base;
    auto bytes = [&](size_t n) { return n * esz; };
    for (int i = 0; i < TT.NS; ++i) {
      d_down[i] = c.take<unsigned char>(bytes((size_t)jck_pad_rows(TT.D_CS[i]) * 16 * jck_pad_chan(TT.D_CB[i])));
      d_up[i] = c.take<unsigned char>(bytes((size_t)4 * jck_pad_rows(TT.D_CB[i]) * 4 * TT.D_CS[i]));
    }
    d_head_wp = c.take<float>(TT.FEAT); d_head_dwp = c.take<float>(TT.FEAT);
    g1_w = c.take<unsigned char>(bytes((size_t)16 * TT.G_C1 * z_pad(family)));
    for (int i = 0; i < TT.NS; ++i) {
      g_up[i] = c.take<unsigned char>(bytes((size_t)4 * jck_pad_rows(TT.G_CB[i]) * 4 * TT.G_CS[i]));
      g_down[i] = c.take<unsigned char>(bytes((size_t)jck_pad_rows(TT.G_CS[i]) * 16 * jck_pad_chan(TT.G_CB[i])));
    }
    const size_t img = (size_t)B * TT.HW * 4;
    auto take_set = [&](DActs& D, int cap, bool penalty_out) {
      D.cap = D.groups = cap; D.g0 = 0;
      for (int i = 0; i < TT.NS; ++i) {
        const size_t n = (size_t)cap * B * (TT.D_HB[i] / 2) * (TT.D_HB[i] / 2) * TT.D_CS[i];
        D.y[i] = c.take<unsigned char>(bytes(n)); D.a[i] = c.take<unsigned char>(bytes(n)); D.g[i] = c.take<unsigned char>(bytes(n));
        D.sums[i] = c.take<float>(cap * jck_bn_bwd_ws_floats(TT.D_CS[i]));
        D.aux[i] = c.take<float>(cap * 4 * TT.D_CS[i]);
        D.stats[i] = c.take<float>(jck_stats_floats((long long)cap * B * (TT.D_HB[i] / 2) * (TT.D_HB[i] / 2), TT.D_CS[i], 1));
      }
      if (penalty_out) D.gx = c.take<unsigned char>(bytes(img));
      D.prob = c.take<float>((size_t)cap * B); D.ds = c.take<float>((size_t)cap * B);
      if (penalty_out) D.norms = c.take<float>(B);
    };
    for (DActs& D : dset) take_set(D, 1, true);
    for (int i = 0; i < TT.NS; ++i) d_rs[i] = c.take<float>(2 * 4 * 2 * TT.D_CS[i]);
    g_z = c.take<unsigned char>(bytes((size_t)B * z_pad(family)));
    // G layer i (0..3): output of conv(i+1) = [B, h, h, C] with (h, C) = (4,512), (8,256), (16,128), (32,64)
    for (int i = 0; i < TT.NS; ++i) {
      const int h = 4 << i, C = TT.G_C1 >> i;
      const size_t n = (size_t)B * h * h * C;
      g_y[i] = c.take<unsigned char>(bytes(n)); g_a[i] = c.take<unsigned char>(bytes(n)); g_gr[i] = c.take<unsigned char>(bytes(n));
    }
    fake_raw = c.take<unsigned char>(bytes(img)); g_raw = c.take<unsigned char>(bytes(img));
    // real_noisy | fake | xhat are consecutive (img bytes % 256 == 0): the batched D pass reads them as one 3B-image tensor
    real_noisy = c.take<unsigned char>(bytes(img)); fake = c.take<unsigned char>(bytes(img)); xhat = c.take<unsigned char>(bytes(img));
    if (batched) {
      take_set(bset, 3, false);
      bset.gx = dset[0].gx; bset.norms = dset[0].norms;
    }
    for (int i = 0; i < TT.NS; ++i) g_bn[i].sums = c.take<float>(jck_bn_bwd_ws_floats(TT.G_C1 >> i));
    for (int i = 0; i < TT.NS; ++i) {
      const int C = TT.G_C1 >> i, h = 4 << i;
      g_bn[i].aux = c.take<float>(4 * C);
      g_bn[i].stats = c.take<float>(jck_stats_floats((long long)B * h * h, C, i == 0 ? 16 : 1));
    }
    acc_ld = (B + 63) / 64 * 64;
    acc2 = c.take<float>((size_t)2 * 8 * acc_ld); scal2 = c.take<float>(16);
    acc = acc2; scal_out = scal2;
    hp2 = c.take<float>(16);
    // the step's small random inputs when the caller hands over none, per step parity (jck_engine_set_step draws them)
    for (int q = 0; q < 2; ++q) {
      rz[q] = c.take<float>((size_t)B * 100); ralpha[q] = c.take<float>((size_t)(B + 3) / 4 * 4);
      rmask[q] = family == 1 ? c.take<float>((size_t)4 * B * L1_OUT) : nullptr;
    }
    head_ws = c.take<float>(jck_head_bwd_ws_floats(TT.FEAT));
    gp2_ws = c.take<float>((size_t)acc_ld + jck_head_bwd_ws_floats(L1_OUT));
    gsync = c.take<unsigned>(jck_grid_sync_bytes() / sizeof(unsigned));
    size_t w = 0;
    for (int i = 0; i < TT.NS; ++i) {
      w = std::max(w, jck_conv_wgrad_ws_bytes(B, TT.D_HB[i], TT.D_HB[i], TT.D_CB[i], TT.D_CS[i]));
      w = std::max(w, jck_conv_wgrad_ws_bytes(2 * B, TT.D_HB[i], TT.D_HB[i], TT.D_CB[i], TT.D_CS[i]));
      w = std::max(w, jck_conv_wgrad_ws_bytes(B, TT.G_HS[i] * 2, TT.G_HS[i] * 2, TT.G_CB[i], TT.G_CS[i]));
    }
    w = std::max(w, jck_g1_wgrad_ws_bytes(B, z_pad(family), TT.G_C1));
    if (family == 1) w = std::max(std::max(w, jck_linear_wgrad_ws_bytes(B, L1_KPAD, L1_OUT)), jck_linear_wgrad_ws_bytes(2 * B, L1_KPAD, L1_OUT));
    wg_ws_bytes = w;
    wg_ws = c.take<float>(w / 4);
    // G.conv1's weight gradient runs on the MAIN stream at the very end of G's backward (it needs the last BatchNorm backward,
    // which is on that stream): its own split-K workspace, because the side stream may still be using wg_ws
    g1_ws_bytes = jck_g1_wgrad_ws_bytes(B, z_pad(family), TT.G_C1);
    g1_ws = c.take<float>(g1_ws_bytes / 4);
    if (family == 1) {
      l1_w = c.take<unsigned char>(bytes((size_t)L1_OUT * L1_KPAD)); l1_wT = c.take<unsigned char>(bytes((size_t)L1_KPAD * L1_OUT));
      // head buffers: HR batches of rows - the batched schedule runs the label / Linear / Dropout head of the real | fake |
      // penalty groups as ONE 3B-row pass (cg_head_batched)
      const size_t HR = batched ? 3 : 1;
      cbuf = c.take<unsigned char>(bytes(HR * B * L1_KPAD)); cbuf2 = c.take<unsigned char>(bytes((size_t)B * L1_KPAD));
      h_pre = c.take<unsigned char>(bytes(HR * B * L1_OUT)); h_drop = c.take<unsigned char>(bytes(HR * B * L1_OUT));
      g_h = c.take<unsigned char>(bytes(HR * B * L1_OUT)); g_hd = c.take<unsigned char>(bytes(HR * B * L1_OUT));
      gh_b1 = c.take<unsigned char>(bytes((size_t)B * L1_OUT)); ughd = c.take<unsigned char>(bytes((size_t)B * L1_OUT));
      gc = c.take<unsigned char>(bytes(HR * B * L1_KPAD));
      pre_e = c.take<float>(HR * B * EMB); l1_slab = c.take<float>((size_t)L1_KSPLIT * HR * B * L1_OUT);
      gw1p = c.take<float>((size_t)L1_OUT * L1_KPAD);
    }
    // second-order penalty buffers: CGAN, and DCGAN with JCK_ENGINE_GP_BACKWARD (a default DCGAN engine carves none of them)
    if (family == 1 || gp_bwd) {
      rs = c.take<float>(B); prob_gp = c.take<float>(B);
      for (int i = 0; i < TT.NS; ++i) {
        const size_t n = (size_t)B * (TT.D_HB[i] / 2) * (TT.D_HB[i] / 2) * TT.D_CS[i];
        d_v[i] = c.take<unsigned char>(bytes(n)); d_xdir[i] = c.take<unsigned char>(bytes(n));
        bn2_ws[i] = c.take<float>(jck_bn2_ws_floats(TT.D_CS[i]));
      }
      bn2_ws_rev = c.take<float>(jck_bn2_ws_floats(TT.G_C1));          // the widest D stage: 512, 1024 on the 128x128 plan
      d_u0 = c.take<unsigned char>(bytes(img));
    }
    ws_bytes = c.off;
  }

  float* P(const NetLayout& L, float* arena, const char* name) const { return arena + find(L, name)->offset; }
  const unsigned* rng() const { return reinterpret_cast<const unsigned*>(hp2 + 8 * parity + 4); }     // this step's Philox words
  // fake = 0.9 * G(z) + 0.1 * N(0,1) (:171): uploaded noise, or drawn in the kernel when the step carries none
  int mix_fake_noise(const jck_step_inputs* in, int B, hipStream_t st) {
    if (!in->noise_fake) return jck_axpy_noise_rng(prec, fake_raw, rng(), 1, 0.9f, 0.1f, fake, B, T.HW, st);
    return jck_axpy_noise(prec, fake_raw, in->noise_fake, 0.9f, 0.1f, fake, B, T.HW, st);
  }
  // ... and the penalty's interpolate (:111-113) in the same launch
  int mix_fake_noise_interp(const jck_step_inputs* in, int B, hipStream_t st) {
    return jck_mix_interp(prec, fake_raw, in->noise_fake, in->noise_fake ? nullptr : rng(), 1, 0.9f, 0.1f, fake, real_noisy, in->alpha, xhat,
                          B, T.HW, st);
  }
};

template <typename T>
static void launch_pad_rows(const float* z, int B, int zd, int zp, void* out, hipStream_t st) {
  const long long total = (long long)B * zp;
  hipLaunchKernelGGL(pad_rows_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, z, B, zd, zp, (T*)out);
}

// engine.hip: the eval-mode generator in two pieces, and the forward both sides run
JCK_INTERNAL int g_eval_fold(jck_engine* e, hipStream_t st);
JCK_INTERNAL int g_eval_products(jck_engine* e, int B, hipStream_t st);
JCK_INTERNAL int g_forward(jck_engine* e, const float* z, const int64_t* labels, int B, hipStream_t st, bool z_in_place = false, bool eval = false);
// engine_infer.hip: frees the inference side's buffer groups (jck_engine_destroy)
JCK_INTERNAL void infer_free(jck_engine* e);
