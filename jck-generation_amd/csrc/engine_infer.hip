// Inference beside the step engine: sampling, the latent projection, discriminator scoring and features, and the critic's latent gradient.
// None of it touches the step state except to note that the operand rows hold a caller's z.
#include "engine_internal.hpp"

extern "C" int jck_engine_sample_ex(jck_engine* e, const float* z, const int64_t* labels, int n, unsigned flags, float* out_nchw,
                                    unsigned char* out_u8_nhwc, void* stream) {
  if (!e || !e->bound) JCK_FAIL(JCK_E_ARG, "engine not bound");
  if (n < 1 || n > e->B) JCK_FAIL(JCK_E_ARG, "sample: n must be in [1, batch]");
  if (flags & ~JCK_SAMPLE_EVAL) JCK_FAIL(JCK_E_ARG, "sample: unknown flag");
  hipStream_t st = (hipStream_t)stream;
  JCK_TRY(g_forward(e, z, labels, n, st, false, (flags & JCK_SAMPLE_EVAL) != 0));
  if (out_nchw) JCK_TRY(jck_nhwc4_to_nchw(e->prec, e->fake_raw, out_nchw, n, TT.HW, st));
  if (out_u8_nhwc) JCK_TRY(jck_img_to_u8(e->prec, e->fake_raw, out_u8_nhwc, n, TT.HW, st));
  return JCK_OK;
}
extern "C" int jck_engine_sample(jck_engine* e, const float* z, const int64_t* labels, int n, float* out_nchw, void* stream) {
  return jck_engine_sample_ex(e, z, labels, n, 0, out_nchw, nullptr, stream);
}

// One of the engine's inference buffer groups (LatentBufs, ScoreBufs, CriticBufs, FeatBufs), allocated by the first call that needs it:
// `carve` takes the group's buffers from a Carver and runs twice - without memory for the size, then on the allocation.  Every group
// reads as zero from the start, as the workspace does after jck_engine_bind: the call clears it on `st` and waits for the clear
// (score_alloc says why) - once per group and engine, next to a hipMalloc that synchronises anyway.
template <typename Bufs, typename Carve>
static int infer_alloc(Bufs& group, Carve carve, hipStream_t st) {
  if (group.base) return JCK_OK;
  Carver c;
  Bufs b;
  carve(c, b);                                                       // sizes
  void* base = nullptr;
  HIPCHK(hipMalloc(&base, c.off));
  if (hipMemsetAsync(base, 0, c.off, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
    (void)hipFree(base);
    JCK_FAIL(JCK_E_HIP, "clearing an inference buffer group failed");
  }
  c = Carver{0, reinterpret_cast<unsigned char*>(base)};
  carve(c, b);
  b.base = base;
  group = b;
  return JCK_OK;
}
void infer_free(jck_engine* e) {
  for (void* base : {e->lat.base, e->sc.base, e->cr.base, e->fm.base}) if (base) (void)hipFree(base);
}

// ---------------------------------------------------------------------------------------------------------
// latent projection: dL/dz through the frozen generator under model.eval(), L_b = mean((G(z_b) - t_b)^2), and Adam on z.
// Beside the step: it uses only buffers that every step rewrites before reading (g_z, g_a, g_gr, g_raw, fake_raw, the stages' aux) -
// never real_noisy or D's activations, which a prefetched D(real) forward may own - and memory of its own.  Image b's numbers do not
// depend on n: no statistic, a per-image loss reduction, a split-K factor that is a constant.
// Here the head of a call and the backward; one evaluation and the entry points come behind the critic's buffers, which they may use.
// ---------------------------------------------------------------------------------------------------------
constexpr int LAT_KSPLIT = 16, LAT_LD = 128;          // 16 * G_C1 / 64 = 128 (64 x 64) or 256 (128 x 128) k-steps: 8 or 16 per slab
// operand rows from z (and the labels), the BatchNorm fold and the pack of G.conv1's weight for the dz product: once per call
static int latent_begin(jck_engine* e, const float* z, const int64_t* labels, int n, hipStream_t st) {
  const int K = 16 * TT.G_C1, zp = z_pad(e->family);
  JCK_TRY(infer_alloc(e->lat, [&](Carver& c, jck_engine::LatentBufs& b) {
    b.w = c.take<unsigned char>((size_t)LAT_LD * K * e->esz);
    b.slab = c.take<float>((size_t)LAT_KSPLIT * e->B * LAT_LD);
    b.loss = c.take<float>(e->B);
  }, st));
  if (e->family == 1) JCK_TRY(jck_cgan_z(e->prec, z, labels, n, 100, N_CLASS, zp, e->g_z, st));
  else {
    e->ss.gz_step = -1;                        // the operand rows now hold somebody else's z
    if (e->prec == JCK_PREC_BF16) launch_pad_rows<bf16_t>(z, n, 100, zp, e->g_z, st); else launch_pad_rows<float>(z, n, 100, zp, e->g_z, st);
    HIPCHK(hipGetLastError());
  }
  JCK_TRY(g_eval_fold(e, st));
  // conv1.weight [z_dim][G_C1][4][4]: its first 100 rows as a Linear weight [100][G_C1 * 16] whose columns go from (c, pos) to (pos, c)
  return jck_pack_linear(e->prec, e->P(e->LG, e->gp, CWN[0]), 100, K, LAT_LD, K, 0, TT.G_C1, 16, e->lat.w, st);
}
// from g_raw, the gradient at the pre-tanh product: the masked dgrads and the dz product's slabs
static int latent_backward(jck_engine* e, int n, hipStream_t st) {
  const void* gbig = e->g_raw;
  for (int i = TT.NS - 1; i >= 0; --i) {       // through conv(i+2) and the folded stage in front of it
    const int hs = TT.G_HS[i];
    JCK_TRY(jck_conv_down_mask(e->prec, gbig, e->g_down[i], e->g_a[i], e->g_bn[i].aux, e->g_gr[i], n, 2 * hs, 2 * hs, TT.G_CB[i], TT.G_CS[i], st));
    gbig = e->g_gr[i];
  }
  return jck_linear_fwd(e->prec, e->g_gr[0], e->lat.w, nullptr, e->lat.slab, n, 16 * TT.G_C1, 100, LAT_LD, LAT_KSPLIT, st);
}

// ---------------------------------------------------------------------------------------------------------
// discriminator inference: D as under model.eval() - every Conv2d + BatchNorm (running statistics) + LeakyReLU stage one launch
// (jck_conv_down_affine) in fp32 storage, two (the product, then the folded BatchNorm + LeakyReLU) in bf16 - score_stage_fused says
// why -, the head without loss, gradient or scalar slots.  Beside the step like the projection above, and stricter:
// D's training activations, real_noisy and the head's concat buffer may belong to a prefetched D(real) forward, so every buffer this
// writes is memory of its own; it reads fake_raw when no image is given.  Row b's numbers do not depend on n: no statistic, a
// per-row head reduction in a fixed order, a split-K factor that is a constant.
// ---------------------------------------------------------------------------------------------------------
// Which form a stage takes.  fp32 storage (f32, bf16x3): fused - jck_conv_down_affine runs the tile jck_conv_down would and saves the
// BatchNorm launch and its pass over the output.  bf16: jck_conv_down + jck_bn_act_fwd on the same folded aux table - there jck_conv_down
// has the image-side streaming kernel and the persistent gather-GEMMs with their 16-byte-store epilogue, which the fused form (shared
// epilogue only) gives up, and the whole call measured 4 % faster that way at batch 64 and 256 (tools/score_rate.py).
static bool score_stage_fused(int prec) { return prec_f32_storage(prec); }
static int score_alloc(jck_engine* e, hipStream_t st) {
  if (!e->sc.base && e->capturing) JCK_FAIL(JCK_E_ARG, "score: the first scoring call allocates and cannot run inside a graph capture");
  // the concat buffer's padding columns are a GEMM operand: they read as zero from the start - for a later call on ANY stream, so this
  // one call, which allocates anyway, waits for the clear
  return infer_alloc(e->sc, [&](Carver& c, jck_engine::ScoreBufs& b) {
    b.x = c.take<unsigned char>((size_t)e->B * TT.HW * 4 * e->esz);
    if (!score_stage_fused(e->prec)) b.y = c.take<unsigned char>((size_t)e->B * (TT.S / 2) * (TT.S / 2) * TT.D_CS[0] * e->esz);   // the largest stage's
    for (int i = 0; i < TT.NS; ++i) {
      b.a[i] = c.take<unsigned char>((size_t)e->B * (TT.D_HB[i] / 2) * (TT.D_HB[i] / 2) * TT.D_CS[i] * e->esz);
      b.aux[i] = c.take<float>(4 * TT.D_CS[i]);
    }
    if (e->family == 1) {
      b.cbuf = c.take<unsigned char>((size_t)e->B * L1_KPAD * e->esz);
      b.slab = c.take<float>((size_t)L1_KSPLIT * e->B * L1_OUT);
      b.h = c.take<unsigned char>((size_t)e->B * L1_OUT * e->esz);
    }
  }, st);
}
// the fold of D's BatchNorm layers (gamma, beta and the running statistics) into the stages' aux tables: one launch ...
static int score_fold(jck_engine* e, hipStream_t st) {
  const jck_engine::ScoreBufs& S = e->sc;
  const float *gamma[JCK_MAX_STAGES], *beta[JCK_MAX_STAGES], *rm[JCK_MAX_STAGES], *rv[JCK_MAX_STAGES];
  float* aux[JCK_MAX_STAGES];
  int Cs[JCK_MAX_STAGES];
  for (int i = 0; i < TT.NS; ++i) {
    gamma[i] = e->P(e->LD, e->dp, NWN[i]); beta[i] = e->P(e->LD, e->dp, NBN[i]);
    rm[i] = e->dbn + find(e->LD, RMN[i])->offset; rv[i] = e->dbn + find(e->LD, RVN[i])->offset;
    aux[i] = S.aux[i]; Cs[i] = TT.D_CS[i];
  }
  return jck_bn_eval_aux(TT.NS, gamma, beta, rm, rv, aux, Cs, BN_EPS, st);
}
// D's input and the fold, the head of jck_engine_score and jck_engine_features: the buffers, *in = the images (and their instance noise)
// transformed into S.x or - NULL images - the generator's last output, where it lies, then score_fold
static int score_input(jck_engine* e, const float* images_nchw, const float* noise_nchw, int n, const void** in, hipStream_t st) {
  JCK_TRY(score_alloc(e, st));
  *in = images_nchw ? e->sc.x : e->fake_raw;
  if (images_nchw) JCK_TRY(jck_img_prep(e->prec, images_nchw, noise_nchw, noise_nchw ? 0.9f : 1.0f, noise_nchw ? 0.1f : 0.0f, e->sc.x, n, TT.HW, st));
  return score_fold(e, st);
}
// ... and the stages on the NHWC4 images `in`, each leaving its activation in S.a[i]: jck_engine_score, jck_engine_features and the
// forward half of the critic's latent gradient, which reads the activations and aux tables afterwards.  `last`: the last stage to run
// (the feature term stops at its stage); -1: all of them
static int score_stages(jck_engine* e, const void* in, int n, hipStream_t st, int last = -1) {
  const jck_engine::ScoreBufs& S = e->sc;
  if (last < 0) last = TT.NS - 1;
  for (int i = 0; i <= last; ++i) {
    const int hb = TT.D_HB[i], cs = TT.D_CS[i];
    if (score_stage_fused(e->prec)) {
      JCK_TRY(jck_conv_down_affine(e->prec, in, e->d_down[i], S.aux[i], S.aux[i] + cs, LRELU, S.a[i], n, hb, hb, TT.D_CB[i], cs, st));
    } else {
      JCK_TRY(jck_conv_down(e->prec, in, e->d_down[i], S.y, nullptr, nullptr, n, hb, hb, TT.D_CB[i], cs, st));
      JCK_TRY(jck_bn_act_fwd(e->prec, S.y, S.aux[i], LRELU, S.a[i], (long long)n * (hb / 2) * (hb / 2), cs, st));
    }
    in = S.a[i];
  }
  return JCK_OK;
}
// the head on the deepest stage's activation
static int score_head(jck_engine* e, const int64_t* labels, int n, float* logit, float* prob, hipStream_t st) {
  const jck_engine::ScoreBufs& S = e->sc;
  const void* in = S.a[TT.NS - 1];
  if (e->family == 0) return jck_score_head(e->prec, in, e->d_head_wp, nullptr, n, TT.FEAT, logit, prob, st);
  JCK_TRY(jck_concat_rows(e->prec, in, TT.FEAT, S.cbuf, L1_KPAD, n, st));
  JCK_TRY(jck_label_embed_fwd(e->prec, labels, e->P(e->LD, e->dp, "label_embedding.weight"), e->P(e->LD, e->dp, "label_embedding.bias"), LRELU, n,
                              N_CLASS, EMB, S.cbuf, L1_KPAD, TT.FEAT, nullptr, st));
  JCK_TRY(jck_linear_fwd(e->prec, S.cbuf, e->l1_w, nullptr, S.slab, n, L1_KPAD, L1_OUT, L1_OUT, L1_KSPLIT, st));
  // Dropout is the identity under model.eval(): no mask
  JCK_TRY(jck_linear_finish(e->prec, S.slab, L1_KSPLIT, e->P(e->LD, e->dp, "linear1.bias"), nullptr, 1.0f, S.h, nullptr, n, L1_OUT, st));
  return jck_score_head(e->prec, S.h, e->P(e->LD, e->dp, "linear2.weight"), e->P(e->LD, e->dp, "linear2.bias"), n, L1_OUT, logit, prob, st);
}
static int score_stages_head(jck_engine* e, const void* in, const int64_t* labels, int n, float* logit, float* prob, hipStream_t st) {
  JCK_TRY(score_stages(e, in, n, st));
  return score_head(e, labels, n, logit, prob, st);
}
extern "C" int jck_engine_score(jck_engine* e, const float* images_nchw, const float* noise_nchw, const int64_t* labels, int n, float* logit,
                                float* prob, void* stream) {
  if (!e || !e->bound) JCK_FAIL(JCK_E_ARG, "score: engine not bound");
  if (n < 1 || n > e->B) JCK_FAIL(JCK_E_ARG, "score: n must be in [1, batch]");
  if (!logit) JCK_FAIL(JCK_E_ARG, "score: null logit");
  if (noise_nchw && !images_nchw) JCK_FAIL(JCK_E_ARG, "score: instance noise goes with images");
  if (e->family == 1 && !labels) JCK_FAIL(JCK_E_ARG, "score: CGAN discriminator needs labels");
  if (!e->d_packed) JCK_FAIL(JCK_E_ARG, "score: the discriminator's weights were never packed (load a discriminator state and repack net 1 first)");
  hipStream_t st = (hipStream_t)stream;
  const void* in;
  JCK_TRY(score_input(e, images_nchw, noise_nchw, n, &in, st));
  return score_stages_head(e, in, labels, n, logit, prob, st);
}

// ---------------------------------------------------------------------------------------------------------
// discriminator features: the stages of jck_engine_score, then each stage's activation pooled to a grid x grid raster (jck_grid_pool)
// into that stage's column block of the caller's rows, stage 0 first; no head, no labels.  The same buffers of its own, the same
// contract: rows independent, nothing of the training state read or written beyond D's weights and running statistics.
// ---------------------------------------------------------------------------------------------------------
static bool feature_grid_ok(int grid) { return grid == 1 || grid == 2 || grid == 4; }
extern "C" long long jck_engine_feature_dim(const jck_engine* e, int grid) {
  if (!e || !feature_grid_ok(grid)) return 0;
  long long c = 0;
  for (int i = 0; i < TT.NS; ++i) c += TT.D_CS[i];
  return c * grid * grid;
}
extern "C" int jck_engine_features(jck_engine* e, const float* images_nchw, int n, int grid, int mode, float* out, long long ld, void* stream) {
  if (!e || !e->bound) JCK_FAIL(JCK_E_ARG, "features: engine not bound");
  if (n < 1 || n > e->B) JCK_FAIL(JCK_E_ARG, "features: n must be in [1, batch]");
  if (!feature_grid_ok(grid)) JCK_FAIL(JCK_E_ARG, "features: grid must be 1, 2 or 4");
  if (mode != 0 && mode != 1) JCK_FAIL(JCK_E_ARG, "features: mode must be 0 (max) or 1 (mean)");
  if (!out || (uintptr_t)out % 16) JCK_FAIL(JCK_E_ARG, "features: out must be a 16-byte aligned device pointer");
  if (ld < jck_engine_feature_dim(e, grid) || ld % 4) JCK_FAIL(JCK_E_ARG, "features: ld must be a multiple of 4 and at least the feature dimension");
  if (!e->d_packed) JCK_FAIL(JCK_E_ARG, "features: the discriminator's weights were never packed (load a discriminator state and repack net 1 first)");
  hipStream_t st = (hipStream_t)stream;
  const void* in;
  JCK_TRY(score_input(e, images_nchw, nullptr, n, &in, st));
  JCK_TRY(score_stages(e, in, n, st));
  long long col0 = 0;
  for (int i = 0; i < TT.NS; ++i) {
    JCK_TRY(jck_grid_pool(e->prec, e->sc.a[i], n, TT.D_HB[i] / 2, TT.D_CS[i], grid, mode, out, ld, col0, st));
    col0 += (long long)grid * grid * TT.D_CS[i];
  }
  return JCK_OK;
}

// ---------------------------------------------------------------------------------------------------------
// the critic's latent gradient: the projection above with a per-pixel weight on the image loss and c(D(G(z))) as a second term -
// masked projection (semantic inpainting) and refinement of a latent along the discriminator's gradient.  D runs as jck_engine_score
// runs it, and its input gradient comes from the activations and folded aux tables that pass keeps in memory of its own: the head's
// input gradient, the leaky backward of the deepest stage, one masked ConvTranspose-direction product per stage (jck_conv_up_mask)
// and the plain one of stage 0 into an image gradient that jck_latent_loss_ex adds in front of the tanh.  Nothing of D's training
// buffers (DActs, real_noisy, the head's cbuf, any gradient arena) is read or written.
// ---------------------------------------------------------------------------------------------------------
static int critic_alloc(jck_engine* e, hipStream_t st) {
  return infer_alloc(e->cr, [&](Carver& c, jck_engine::CriticBufs& b) {
    for (int i = 0; i < TT.NS; ++i) b.g[i] = c.take<unsigned char>((size_t)e->B * (TT.D_HB[i] / 2) * (TT.D_HB[i] / 2) * TT.D_CS[i] * e->esz);
    b.gx = c.take<unsigned char>((size_t)e->B * TT.HW * 4 * e->esz);
    b.ds = c.take<float>(e->B); b.term = c.take<float>(e->B); b.logit = c.take<float>(e->B);
    if (e->family == 1) {
      b.g_h = c.take<unsigned char>((size_t)e->B * L1_OUT * e->esz);
      b.gc = c.take<unsigned char>((size_t)e->B * L1_KPAD * e->esz);
    }
  }, st);
}
// The objective of a latent call, as the six entry points build it: the image loss on `target` under the per-pixel `weight` (either may be
// null), the critic's term (mode 0: none) at weight cw, and
// feat_target / feat_stage / feat_weight: the feature-matching term F_b = feat_weight * mean((a_k(G(z_b)) - a_k(x_b))^2) on the LeakyReLU
// output of D's stage k (-1: the deepest); on iff there is a target and a positive weight
struct LatentEx {
  const int64_t* labels; const float* target; const float* weight; int mode; float cw;
  const float* feat_target; int feat_stage; float feat_weight;
  bool fm() const { return feat_target && feat_weight > 0.f; }
};
// What a call reports per image: rows [n] of one evaluation, or (project) histories [steps][n] of which row(s) is update s's; null: not wanted
struct LatentOut {
  float *loss, *term, *logit, *fterm;
  LatentOut row(int s, int n) const {
    auto at = [&](float* p) { return p ? p + (size_t)s * n : nullptr; };
    return {at(loss), at(term), at(logit), at(fterm)};
  }
};
struct LatentAdam { int steps; float lr, prior; float *m, *v; int t0; };      // project's schedule and the caller's Adam state
static int latent_check(jck_engine* e, const float* z, const LatentEx& o, int n, const std::string& w) {
  if (!e || !e->bound) JCK_FAIL(JCK_E_ARG, w + ": engine not bound");
  if (n < 1 || n > e->B) JCK_FAIL(JCK_E_ARG, w + ": n must be in [1, batch]");
  if (!z) JCK_FAIL(JCK_E_ARG, w + ": null z");
  if (o.mode < 0 || o.mode > 2) JCK_FAIL(JCK_E_ARG, w + ": critic_mode must be 0 (none), 1 (nsgan) or 2 (logit)");
  if (!(o.feat_weight >= 0.f) || !(o.feat_weight <= 3.402823466e38f)) JCK_FAIL(JCK_E_ARG, w + ": feat_weight must be finite and >= 0");
  if (o.feat_weight > 0.f && !o.feat_target) JCK_FAIL(JCK_E_ARG, w + ": feat_weight > 0 needs a feature target");
  if (o.feat_stage < -1 || o.feat_stage >= TT.NS) JCK_FAIL(JCK_E_ARG, w + ": feat_stage must be -1 (the deepest stage) or a stage of D");
  if (!o.target && !o.mode && !o.fm()) JCK_FAIL(JCK_E_ARG, w + ": without a target and without a feature term a critic is required");
  if (!(o.cw >= 0.f)) JCK_FAIL(JCK_E_ARG, w + ": critic_weight >= 0");
  if (e->family == 1 && !o.labels) JCK_FAIL(JCK_E_ARG, w + ": CGAN needs labels");
  if ((o.mode || o.fm()) && !e->d_packed)
    JCK_FAIL(JCK_E_ARG, w + ": the discriminator's weights were never packed (load a discriminator state and repack net 1 first)");
  if (e->capturing) JCK_FAIL(JCK_E_ARG, w + ": not inside a graph capture");
  return JCK_OK;
}
static int feat_stage_of(const jck_engine* e, const LatentEx& o) { return o.feat_stage < 0 ? TT.NS - 1 : o.feat_stage; }
static long long feat_elems(const jck_engine* e, int k) { return (long long)(TT.D_HB[k] / 2) * (TT.D_HB[k] / 2) * TT.D_CS[k]; }
// once per call, behind latent_begin: the critic's buffers and D's BatchNorm fold; with a feature term also its buffers (room for the
// largest stage, and a row for F), and the target's activation at stage k, which stays there for the call
static int latent_ex_begin(jck_engine* e, const LatentEx& o, int n, hipStream_t st) {
  if (!o.mode && !o.fm()) return JCK_OK;
  JCK_TRY(score_alloc(e, st));
  JCK_TRY(critic_alloc(e, st));
  if (o.fm()) JCK_TRY(infer_alloc(e->fm, [&](Carver& c, jck_engine::FeatBufs& b) {
    b.fa = c.take<unsigned char>((size_t)e->B * feat_elems(e, 0) * e->esz);
    b.term = c.take<float>(e->B);
  }, st));
  JCK_TRY(score_fold(e, st));
  if (!o.fm()) return JCK_OK;
  const int k = feat_stage_of(e, o);
  JCK_TRY(jck_img_prep(e->prec, o.feat_target, nullptr, 1.0f, 0.0f, e->sc.x, n, TT.HW, st));
  JCK_TRY(score_stages(e, e->sc.x, n, st, k));
  HIPCHK(hipMemcpyAsync(e->fm.fa, e->sc.a[k], (size_t)n * feat_elems(e, k) * e->esz, hipMemcpyDeviceToDevice, st));
  return JCK_OK;
}
// one evaluation: the eval forward's products, the critic's forward and input gradient if there is one, the loss and its gradient, the
// masked dgrads, the dz product's slabs.  Plain (no weight, no critic): the products, jck_latent_loss_ex, latent_backward.
// With a feature term jck_feat_match puts its gradient where C.g[k] holds (or would hold) the gradient at stage k's product: without a
// critic D runs up to stage k only and its backward starts there; with one it is added onto what came down from the head.
static int latent_eval(jck_engine* e, const LatentEx& o, int n, const LatentOut& out, hipStream_t st) {
  JCK_TRY(g_eval_products(e, n, st));
  const jck_engine::ScoreBufs& S = e->sc;
  const jck_engine::CriticBufs& C = e->cr;
  // a row the caller does not want goes to one of the engine's own
  float *loss = out.loss ? out.loss : e->lat.loss, *term = out.term ? out.term : C.term, *logit = out.logit ? out.logit : C.logit;
  const bool fm = o.fm();
  const int top = TT.NS - 1, k = feat_stage_of(e, o), from = o.mode ? top : k;
  auto feat_match = [&](int accumulate) {
    return jck_feat_match(e->prec, S.a[k], e->fm.fa, S.aux[k], LRELU, o.feat_weight, C.g[k], accumulate, out.fterm ? out.fterm : e->fm.term, n,
                          feat_elems(e, k), TT.D_CS[k], st);
  };
  if (o.mode) {
    JCK_TRY(score_stages_head(e, e->fake_raw, o.labels, n, logit, nullptr, st));
    JCK_TRY(jck_critic_ds(logit, o.mode, o.cw, n, C.ds, term, st));
    if (e->family == 0) {
      JCK_TRY(jck_head_bwd_conv(e->prec, C.ds, e->d_head_wp, S.a[top], n, TT.G_C1, C.g[top], nullptr, nullptr, st));
    } else {
      // Linear(8392,256) -> Dropout (the identity) -> Linear(256,1): no nonlinearity between the two products under model.eval()
      JCK_TRY(jck_head_bwd(e->prec, C.ds, e->P(e->LD, e->dp, "linear2.weight"), nullptr, n, L1_OUT, C.g_h, nullptr, 0, nullptr, st));
      JCK_TRY(jck_linear_fwd(e->prec, C.g_h, e->l1_wT, nullptr, C.gc, n, L1_OUT, L1_KPAD, L1_KPAD, 1, st));
      JCK_TRY(jck_split_rows(e->prec, C.gc, L1_KPAD, TT.FEAT, C.g[top], n, st));
    }
    JCK_TRY(jck_leaky_affine_bwd(e->prec, C.g[top], S.a[top], S.aux[top], LRELU, C.g[top], (long long)n * (TT.D_HB[top] / 2) * (TT.D_HB[top] / 2),
                                 TT.D_CS[top], st));
    if (fm && k == top) JCK_TRY(feat_match(1));
  } else if (fm) {
    JCK_TRY(score_stages(e, e->fake_raw, n, st, k));
    JCK_TRY(feat_match(0));
  }
  if (o.mode || fm) {
    for (int i = from; i >= 1; --i) {           // through conv(i+1) and the folded stage in front of it
      const int hs = TT.D_HB[i] / 2;
      JCK_TRY(jck_conv_up_mask(e->prec, C.g[i], e->d_up[i], S.a[i - 1], S.aux[i - 1], LRELU, C.g[i - 1], n, hs, hs, TT.D_CS[i], TT.D_CB[i], st));
      if (fm && i - 1 == k) JCK_TRY(feat_match(1));
    }
    JCK_TRY(jck_conv_up(e->prec, C.g[0], e->d_up[0], C.gx, nullptr, nullptr, 0, n, TT.D_HB[0] / 2, TT.D_HB[0] / 2, TT.D_CS[0], TT.D_CB[0], st));
  }
  JCK_TRY(jck_latent_loss_ex(e->prec, e->fake_raw, o.target, o.weight, o.mode || fm ? C.gx : nullptr, e->g_raw, loss, n, TT.HW, st));
  return latent_backward(e, n, st);
}
static int latent_grad(const std::string& who, jck_engine* e, const float* z, const LatentEx& o, int n, const LatentOut& out, float* dz,
                       void* stream) {
  JCK_TRY(latent_check(e, z, o, n, who));
  if (!out.loss || !dz) JCK_FAIL(JCK_E_ARG, who + ": null loss / dz");
  hipStream_t st = (hipStream_t)stream;
  JCK_TRY(latent_begin(e, z, o.labels, n, st));
  JCK_TRY(latent_ex_begin(e, o, n, st));
  JCK_TRY(latent_eval(e, o, n, out, st));
  return jck_latent_adam(e->prec, e->lat.slab, LAT_KSPLIT, LAT_LD, dz, nullptr, nullptr, 0.f, 0.f, 0, nullptr, 0, n, st);
}
// a.steps Adam updates of z [n][100] (in, out) on the stream, no host synchronisation: a.m, a.v [n][100] are the caller's (zero them for
// a fresh run), a.t0 the number of updates they have seen; hist's loss[s][n] / term[s][n] / fterm[s][n] (or null) are the loss, the
// critic's term and the feature term BEFORE update s.
static int project(const std::string& who, jck_engine* e, float* z, const LatentEx& o, int n, const LatentAdam& a, const LatentOut& hist,
                   void* stream) {
  JCK_TRY(latent_check(e, z, o, n, who));
  if (a.steps < 1 || a.t0 < 0 || !a.m || !a.v) JCK_FAIL(JCK_E_ARG, who + ": steps >= 1, t0 >= 0 and the Adam state m, v are required");
  if (!(a.lr > 0.f) || !(a.prior >= 0.f)) JCK_FAIL(JCK_E_ARG, who + ": lr > 0 and prior >= 0");
  hipStream_t st = (hipStream_t)stream;
  JCK_TRY(latent_begin(e, z, o.labels, n, st));
  JCK_TRY(latent_ex_begin(e, o, n, st));
  for (int s = 0; s < a.steps; ++s) {
    JCK_TRY(latent_eval(e, o, n, hist.row(s, n), st));
    JCK_TRY(jck_latent_adam(e->prec, e->lat.slab, LAT_KSPLIT, LAT_LD, z, a.m, a.v, a.lr, a.prior, a.t0 + s + 1, e->g_z, z_pad(e->family), n, st));
  }
  return JCK_OK;
}
// the six entry points: the plain ones are the _ex ones with no weight and no critic, the _ex ones the _fm ones with no feature term
extern "C" int jck_engine_latent_grad(jck_engine* e, const float* z, const int64_t* labels, const float* target_nchw, int n, float* loss,
                                      float* dz, void* stream) {
  return latent_grad("latent_grad", e, z, {labels, target_nchw, nullptr, 0, 0.f, nullptr, -1, 0.f}, n, {loss, nullptr, nullptr, nullptr}, dz, stream);
}
extern "C" int jck_engine_latent_grad_ex(jck_engine* e, const float* z, const int64_t* labels, const float* target_nchw, const float* weight,
                                         int critic_mode, float critic_weight, int n, float* loss, float* term, float* logit, float* dz,
                                         void* stream) {
  return latent_grad("latent_grad_ex", e, z, {labels, target_nchw, weight, critic_mode, critic_weight, nullptr, -1, 0.f}, n,
                     {loss, term, logit, nullptr}, dz, stream);
}
extern "C" int jck_engine_latent_grad_fm(jck_engine* e, const float* z, const int64_t* labels, const float* target_nchw, const float* weight,
                                         int critic_mode, float critic_weight, int n, float* loss, float* term, float* logit, float* dz,
                                         void* stream, const float* feat_target_nchw, int feat_stage, float feat_weight, float* fterm) {
  return latent_grad("latent_grad_fm", e, z, {labels, target_nchw, weight, critic_mode, critic_weight, feat_target_nchw, feat_stage, feat_weight},
                     n, {loss, term, logit, fterm}, dz, stream);
}
extern "C" int jck_engine_project(jck_engine* e, float* z, const int64_t* labels, const float* target_nchw, int n, int steps, float lr,
                                  float prior, float* m, float* v, int t0, float* loss_hist, void* stream) {
  return project("project", e, z, {labels, target_nchw, nullptr, 0, 0.f, nullptr, -1, 0.f}, n, {steps, lr, prior, m, v, t0},
                 {loss_hist, nullptr, nullptr, nullptr}, stream);
}
extern "C" int jck_engine_project_ex(jck_engine* e, float* z, const int64_t* labels, const float* target_nchw, int n, int steps, float lr,
                                     float prior, const float* weight, int critic_mode, float critic_weight, float* m, float* v, int t0,
                                     float* loss_hist, float* term_hist, void* stream) {
  return project("project_ex", e, z, {labels, target_nchw, weight, critic_mode, critic_weight, nullptr, -1, 0.f}, n, {steps, lr, prior, m, v, t0},
                 {loss_hist, term_hist, nullptr, nullptr}, stream);
}
extern "C" int jck_engine_project_fm(jck_engine* e, float* z, const int64_t* labels, const float* target_nchw, int n, int steps, float lr,
                                     float prior, const float* weight, int critic_mode, float critic_weight, float* m, float* v, int t0,
                                     float* loss_hist, float* term_hist, void* stream, const float* feat_target_nchw, int feat_stage,
                                     float feat_weight, float* fterm_hist) {
  return project("project_fm", e, z, {labels, target_nchw, weight, critic_mode, critic_weight, feat_target_nchw, feat_stage, feat_weight}, n,
                 {steps, lr, prior, m, v, t0}, {loss_hist, term_hist, nullptr, fterm_hist}, stream);
}
