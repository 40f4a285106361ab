// Whole-step engine: the reference's training iteration (train/dcgan_trainer.py:155-189) as one native
// schedule of kernel launches on a HIP stream.  The host makes one call per phase; nothing in here
// allocates, synchronises or reads back - scalars stay on the device until the trainer logs them.
#include <cstdlib>

#include "engine_internal.hpp"      // ew_optim.hpp with it: the kernels this file launches itself (pack_multi_kernel, pack_tail_kernel) and the repack table of adam_pack_kernel
#define JCK_BATCHED_DEFAULT 3

namespace {

constexpr long long ALIGN_F = 64;   // floats

void add_param(NetLayout& L, const char* name, int a, int b, int c, int d) {
  TensorInfo ti{name, 0, L.n_params, (long long)a * b * c * d, {a, b, c, d}};
  L.t.push_back(ti);
  L.n_params = (L.n_params + ti.numel + ALIGN_F - 1) / ALIGN_F * ALIGN_F;
}
void add_bn(NetLayout& L, const char* wn, const char* bn, const char* rm, const char* rv, int c) {
  add_param(L, wn, c, 1, 1, 1);
  add_param(L, bn, c, 1, 1, 1);
  TensorInfo m{rm, 1, L.n_bn, c, {c, 1, 1, 1}};
  L.t.push_back(m);
  L.n_bn += (c + ALIGN_F - 1) / ALIGN_F * ALIGN_F;
  TensorInfo v{rv, 2, L.n_bn, c, {c, 1, 1, 1}};
  L.t.push_back(v);
  L.n_bn += (c + ALIGN_F - 1) / ALIGN_F * ALIGN_F;
}

Topo make_topo(int S) {
  Topo T = {};
  T.S = S; T.NS = S == 128 ? 5 : 4; T.HW = S * S;
  T.G_C1 = 64 << (T.NS - 1);
  T.FEAT = 16 * T.G_C1;
  for (int i = 0; i < T.NS; ++i) {
    T.D_CS[i] = 64 << i; T.D_CB[i] = i == 0 ? 3 : 32 << i; T.D_HB[i] = S >> i;
    T.G_CS[i] = T.G_C1 >> i; T.G_CB[i] = i == T.NS - 1 ? 3 : T.G_C1 >> (i + 1); T.G_HS[i] = 4 << i;
  }
  return T;
}
NetLayout make_layout(int family, int net, int S = 64) {
  NetLayout L;
  const Topo T = make_topo(S);
  const char* const* CW = CWN; const char* const* NW = NWN; const char* const* NB = NBN; const char* const* RM = RMN; const char* const* RV = RVN;
  if (net == 0) {
    add_param(L, CW[0], z_dim(family), T.G_C1, 4, 4);
    add_bn(L, NW[0], NB[0], RM[0], RV[0], T.G_C1);
    for (int i = 0; i < T.NS; ++i) {
      add_param(L, CW[i + 1], T.G_CS[i], T.G_CB[i], 4, 4);
      if (i < T.NS - 1) add_bn(L, NW[i + 1], NB[i + 1], RM[i + 1], RV[i + 1], T.G_CB[i]);
    }
  } else {
    if (family == 1) {                                  // model/CGAN.py:83: registered first
      add_param(L, "label_embedding.weight", EMB, N_CLASS, 1, 1);
      add_param(L, "label_embedding.bias", EMB, 1, 1, 1);
    }
    for (int i = 0; i < T.NS; ++i) {
      add_param(L, CW[i], T.D_CS[i], T.D_CB[i], 4, 4);
      add_bn(L, NW[i], NB[i], RM[i], RV[i], T.D_CS[i]);
    }
    if (family == 0) {
      add_param(L, CW[T.NS], 1, T.G_C1, 4, 4);
    } else {                                            // model/CGAN.py:104,106
      add_param(L, "linear1.weight", L1_OUT, L1_K, 1, 1);
      add_param(L, "linear1.bias", L1_OUT, 1, 1, 1);
      add_param(L, "linear2.weight", 1, L1_OUT, 1, 1);
      add_param(L, "linear2.bias", 1, 1, 1, 1);
    }
  }
  return L;
}

}  // namespace

// the engine's events order kernels of ONE device across its streams: no system-scope fence (cache write-back for the host's sake)
// when they are recorded
static unsigned jck_event_flags() { return hipEventDisableTiming | hipEventDisableSystemFence; }

DActs DActs::group(const jck_engine* e, int first, int n) const {
  DActs v = *this;
  v.g0 = g0 + first; v.groups = n;
  const size_t B = (size_t)e->B;
  auto at = [&](void* p, size_t elems) { return (void*)((unsigned char*)p + elems * e->esz); };
  for (int i = 0; i < TT.NS; ++i) {
    const int cs = TT.D_CS[i];
    const size_t px = (size_t)(TT.D_HB[i] / 2) * (TT.D_HB[i] / 2), off = first * B * px * cs;
    v.y[i] = at(y[i], off); v.a[i] = at(a[i], off); v.g[i] = at(g[i], off);
    v.aux[i] = aux[i] + (size_t)first * 4 * cs;
    v.sums[i] = sums[i] + (size_t)first * jck_bn_bwd_ws_floats(cs);
    // statistic slots of a group start at its 1/cap point of the buffer (sized for cap * B images at one slot per 32 pixels)
    v.stats[i] = stats[i] + (size_t)first * (jck_stats_floats((long long)(cap * B * px), cs, 1) / cap / (2 * cs)) * (2 * cs);
  }
  v.prob = prob + first * B; v.ds = ds + first * B;
  return v;
}

// a schedule switch: on unless the variable is set to 0
static bool env_on(const char* name) {
  const char* v = getenv(name);
  return !(v && atoi(v) == 0);
}
// the side streams and events of an overlapping engine (at creation, and again after an aborted capture)
static int create_side_streams(jck_engine* e) {
  hipError_t rc = hipSuccess;
  e->for_each_side_stream([&](hipStream_t& s) { if (rc == hipSuccess) rc = hipStreamCreateWithFlags(&s, hipStreamNonBlocking); });      // queue priorities measured neutral (r1-r4)
  e->for_each_event([&](hipEvent_t& ev) { if (rc == hipSuccess) rc = hipEventCreateWithFlags(&ev, jck_event_flags()); });
  HIPCHK(rc);
  return JCK_OK;
}
static void destroy_side_streams(jck_engine* e, bool sync) {
  e->for_each_side_stream([&](hipStream_t& s) {
    if (s) { if (sync) (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
    s = nullptr;
  });
  e->for_each_event([](hipEvent_t& ev) { if (ev) (void)hipEventDestroy(ev); ev = nullptr; });
}

extern "C" int jck_engine_create(jck_engine** out, int family, int prec, int batch) {
  return jck_engine_create_sized(out, family, prec, batch, 64);
}
// image_size 64 = the reference's topology; 128 = one more stride-2 stage (DCGAN only; BASELINE.json configs[4])
extern "C" int jck_engine_create_sized(jck_engine** out, int family, int prec, int batch, int image_size) {
  return jck_engine_create_ex(out, family, prec, batch, image_size, 0);
}
// flags: JCK_ENGINE_GP_BACKWARD (include/jckgan.h)
extern "C" int jck_engine_create_ex(jck_engine** out, int family, int prec, int batch, int image_size, unsigned flags) {
  if (!out) JCK_FAIL(JCK_E_ARG, "null out");
  if (flags & ~JCK_ENGINE_GP_BACKWARD) JCK_FAIL(JCK_E_ARG, "unknown engine flags");
  if (image_size != 64 && image_size != 128) JCK_FAIL(JCK_E_ARG, "image_size must be 64 or 128");
  if (image_size != 64 && family != 0) JCK_FAIL(JCK_E_ARG, "the 128x128 topology exists for DCGAN only (CGAN's Linear(8392,256) fixes 64x64)");
  if (family != 0 && family != 1) JCK_FAIL(JCK_E_ARG, "family must be 0 (DCGAN) or 1 (CGAN)");
  if (prec != JCK_PREC_BF16 && !prec_f32_storage(prec)) JCK_FAIL(JCK_E_ARG, "bad prec");
  if (batch < 1 || batch > 8192) JCK_FAIL(JCK_E_ARG, "batch must be in [1, 8192]");
  jck_engine* e = new jck_engine();
  e->family = family; e->prec = prec; e->B = batch; e->esz = prec_f32_storage(prec) ? 4 : 2;
  e->T = make_topo(image_size);
  e->LG = make_layout(family, 0, image_size); e->LD = make_layout(family, 1, image_size);
  e->overlap = env_on("JCK_OVERLAP");
  // batched D passes need whole tiles per group: 16*B rows at the last layer, tiles of up to 128 rows
  e->batched = getenv("JCK_BATCHED") ? atoi(getenv("JCK_BATCHED")) : JCK_BATCHED_DEFAULT;
  if (!e->overlap || batch % 8 != 0 || e->batched != 3) e->batched = 0;
  e->gp_bwd = family == 0 && (flags & JCK_ENGINE_GP_BACKWARD);        // CGAN back-propagates its penalty anyway
  e->carve(nullptr);
  e->wgrad_side = env_on("JCK_WGRAD_SIDE");
  e->head_side = env_on("JCK_HEAD_SIDE");
  e->ext_events = env_on("JCK_EXT_EVENTS");
  e->bn_res = env_on("JCK_BN_RES");
  e->cbuf_direct = family == 1 && env_on("JCK_CBUF_DIRECT");
  e->head_fuse = env_on("JCK_HEAD_FUSE");
  e->real_side = env_on("JCK_REAL_SIDE");
  e->fold_zero = env_on("JCK_FOLD_ZERO");
  e->fuse_tanh = env_on("JCK_FUSE_TANH");
  e->adam_pack = env_on("JCK_ADAM_PACK");
  if (e->overlap) JCK_TRY(create_side_streams(e));
  *out = e;
  return JCK_OK;
}
extern "C" void jck_engine_destroy(jck_engine* e) {
  if (!e) return;
  if (e->overlap) destroy_side_streams(e, true);
  infer_free(e);
  delete e;
}
extern "C" int jck_engine_num_tensors(int family, int net) { return (int)make_layout(family, net).t.size(); }
static int tensor_info(const NetLayout& L, int idx, char* name, int name_cap, int* kind, long long* offset, long long* numel, int* shape4) {
  if (idx < 0 || idx >= (int)L.t.size()) JCK_FAIL(JCK_E_ARG, "index out of range");
  const TensorInfo& t = L.t[idx];
  if (name && name_cap > 0) { strncpy(name, t.name, name_cap - 1); name[name_cap - 1] = 0; }
  if (kind) *kind = t.kind;
  if (offset) *offset = t.offset;
  if (numel) *numel = t.numel;
  if (shape4) for (int q_ = 0; q_ < 4; ++q_) shape4[q_] = t.shape[q_];
  return JCK_OK;
}
static long long arena_numel(const NetLayout& L, int which) { return which == 0 ? L.n_params : L.n_bn; }
extern "C" int jck_engine_tensor_info(int family, int net, int idx, char* name, int name_cap, int* kind, long long* offset,
                                      long long* numel, int* shape4) {
  return tensor_info(make_layout(family, net), idx, name, name_cap, kind, offset, numel, shape4);
}
extern "C" long long jck_engine_arena_numel(int family, int net, int which) { return arena_numel(make_layout(family, net), which); }
// the same three queries for a created engine (its own image size)
extern "C" int jck_engine_num_tensors_of(const jck_engine* e, int net) { return e ? (int)(net == 0 ? e->LG : e->LD).t.size() : 0; }
extern "C" int jck_engine_tensor_info_of(const jck_engine* e, int net, int idx, char* name, int name_cap, int* kind, long long* offset,
                                         long long* numel, int* shape4) {
  if (!e) JCK_FAIL(JCK_E_ARG, "null engine");
  return tensor_info(net == 0 ? e->LG : e->LD, idx, name, name_cap, kind, offset, numel, shape4);
}
extern "C" long long jck_engine_arena_numel_of(const jck_engine* e, int net, int which) {
  return e ? arena_numel(net == 0 ? e->LG : e->LD, which) : 0;
}
extern "C" int jck_engine_image_size(const jck_engine* e) { return e ? e->T.S : 0; }
extern "C" size_t jck_engine_workspace_bytes(const jck_engine* e) { return e ? e->ws_bytes : 0; }

extern "C" int jck_engine_bind(jck_engine* e, void* workspace, size_t ws_bytes, float* g_params, float* g_grads, float* g_m,
                               float* g_v, float* g_bn, int64_t* g_nbt, float* d_params, float* d_grads, float* d_m,
                               float* d_v, float* d_bn, int64_t* d_nbt) {
  if (!e || !workspace) JCK_FAIL(JCK_E_ARG, "null engine / workspace");
  if (ws_bytes < e->ws_bytes) JCK_FAIL(JCK_E_WS, "workspace too small: need " + std::to_string(e->ws_bytes));
  if (((uintptr_t)workspace) % 256) JCK_FAIL(JCK_E_ARG, "workspace must be 256-byte aligned");
  e->carve(reinterpret_cast<unsigned char*>(workspace));
  // Bind owns the workspace's zero contract: whatever the caller's memory held, everything the engine carves reads as zero from
  // here on.  The kernels rely on it where they write only part of a buffer - the repack kernels write real (channel, channel)
  // pairs and leave the padding rows / channels of the packed operands alone, the set-step launch and the label embedding leave
  // the padding columns of g_z / cbuf / cbuf2 alone - and the grid-barrier words (gsync) start at generation 0 with no error.
  // One clear of all of it, once per bind, in no step - finished when bind returns, so that the first launch may come on any stream.
  HIPCHK(hipMemset(workspace, 0, e->ws_bytes));
  HIPCHK(hipStreamSynchronize(nullptr));
  // ... which also took the device copies of the step scalars and the packed operands of an engine that is bound again
  e->hp_step[0] = e->hp_step[1] = 0;
  e->hp_lr[0] = e->hp_lr[1] = -1.f;
  e->ss = StepState();
  e->d_packed = false;
  e->gp = g_params; e->gg = g_grads; e->gm = g_m; e->gv = g_v; e->gbn = g_bn; e->gnbt = g_nbt;
  e->dp = d_params; e->dg = d_grads; e->dm = d_m; e->dv = d_v; e->dbn = d_bn; e->dnbt = d_nbt;
  e->bound = true;
  return JCK_OK;
}

// the repack table of one network: a job per operand form, the forms of one weight next to each other, weights in arena order;
// returns the workgroups of pack_multi_kernel's grid
static int pack_jobs(const jck_engine* e, int net, PackJobs& jobs) {
  int n = 0, chunk = 0;
  auto add = [&](int kind, const float* w, void* wp, long long total, int a, int b, int c) {
    PackJob& J = jobs.j[n];
    J.w = w; J.wp = wp; J.total = total; J.kind = kind; J.a = a; J.b = b; J.c = c;
    jobs.first_chunk[n] = chunk;
    chunk += (int)((total + PACK_CHUNK - 1) / PACK_CHUNK);
    ++n;
  };
  // totals are (output channel, input channel) pairs: one thread each (ew_optim.hpp: pack_multi_kernel)
  auto add_down = [&](const float* w, int Cs, int Cb, void* wp) { add(0, w, wp, (long long)Cs * Cb, Cs, Cb, ilog2(jck_pad_chan(Cb))); };
  auto add_up = [&](const float* w, int Cs, int Cb, void* wp) {
    if (Cb <= 4) add(2, w, wp, (long long)Cs * Cb, Cs, Cb, 0);
    else add(1, w, wp, (long long)Cs * Cb, Cs, Cb, jck_pad_rows(Cb));
  };
  if (net == 1) {
    for (int i = 0; i < TT.NS; ++i) {
      const float* w = e->P(e->LD, e->dp, CWN[i]);
      add_down(w, TT.D_CS[i], TT.D_CB[i], e->d_down[i]);
      add_up(w, TT.D_CS[i], TT.D_CB[i], e->d_up[i]);
    }
    if (e->family == 0) add(4, e->P(e->LD, e->dp, CWN[TT.NS]), e->d_head_wp, TT.G_C1, TT.G_C1, 0, 0);
  } else {
    add(3, e->P(e->LG, e->gp, CWN[0]), e->g1_w, (long long)z_dim(e->family) * TT.G_C1, z_dim(e->family), TT.G_C1, z_pad(e->family));
    for (int i = 0; i < TT.NS; ++i) {
      const float* w = e->P(e->LG, e->gp, CWN[i + 1]);
      add_up(w, TT.G_CS[i], TT.G_CB[i], e->g_up[i]);
      add_down(w, TT.G_CS[i], TT.G_CB[i], e->g_down[i]);
    }
  }
  jobs.first_chunk[n] = chunk;
  jobs.n = n;
  return chunk;
}
// all conv operands of one network in one launch (ew_optim.hpp: pack_multi_kernel); the two Linear operands of CGAN's D follow
// tail (optional): the end-of-step job rides in the same launch (ew_optim.hpp: pack_tail_kernel)
static int repack_convs(jck_engine* e, int net, void* stream, const TailJobs* tail = nullptr, int tail_x = 0) {
  PackJobs jobs = {};
  const int chunk = pack_jobs(e, net, jobs);
  if (net == 1) e->d_packed = true;
  if (tail) {
    const int nblk = chunk + tail_x * (tail->nl + 1);
    if (e->prec == JCK_PREC_BF16) hipLaunchKernelGGL(pack_tail_kernel<bf16_t>, dim3(nblk), dim3(256), 0, (hipStream_t)stream, jobs, chunk, *tail, tail_x);
    else hipLaunchKernelGGL(pack_tail_kernel<float>, dim3(nblk), dim3(256), 0, (hipStream_t)stream, jobs, chunk, *tail, tail_x);
  } else if (e->prec == JCK_PREC_BF16) hipLaunchKernelGGL(pack_multi_kernel<bf16_t>, dim3(chunk), dim3(256), 0, (hipStream_t)stream, jobs);
  else hipLaunchKernelGGL(pack_multi_kernel<float>, dim3(chunk), dim3(256), 0, (hipStream_t)stream, jobs);
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
static int repack_linear(jck_engine* e, void* stream) {
  const float* w1 = e->P(e->LD, e->dp, "linear1.weight");
  return pack_linear_pair(e->prec, w1, L1_OUT, L1_K, L1_OUT, L1_KPAD, e->l1_w, L1_KPAD, L1_OUT, e->l1_wT, 512, 16, (hipStream_t)stream);
}
extern "C" int jck_engine_repack(jck_engine* e, int net, void* stream) {
  if (!e || !e->bound) JCK_FAIL(JCK_E_ARG, "engine not bound");
  JCK_TRY(repack_convs(e, net, stream));
  if (net == 1 && e->family == 1) JCK_TRY(repack_linear(e, stream));
  return JCK_OK;
}

// ---------------------------------------------------------------------------------------------------------
// building blocks
// ---------------------------------------------------------------------------------------------------------
static const double ADAM_B1 = 0.5, ADAM_B2 = 0.999, ADAM_EPS = 1e-8;      // both optimisers (train/dcgan_trainer.py:61-62)


// `ws` work enqueued after this starts behind everything on `st` so far: on `side` when there is one (the hand-over goes through
// evW[k]; record = false: the last launch on st completes that event itself), else on st
static int fork_side(jck_engine* e, int k, hipStream_t st, hipStream_t side, hipStream_t* ws, bool record = true) {
  *ws = st;
  if (!side) return JCK_OK;
  if (record) HIPCHK(hipEventRecord(e->evW[k], st));
  HIPCHK(hipStreamWaitEvent(side, e->evW[k], 0));
  *ws = side;
  return JCK_OK;
}

// conv stack of D for the groups of view `S` (x_in = first image of its first group): ONE launch per layer for all of them,
// BatchNorm statistics per group (= per batch, train/dcgan_trainer.py:162,173,118).  BatchNorm running statistics are NOT touched
// here: (mean, unbiased var) of group g go to the deferred record of pass `pass0 + g` (g counted in the set: 0 real, 1 fake,
// 2 penalty; 3 G phase) and are applied in that order at the end of the step, which keeps the result bitwise independent of how the
// passes overlap on streams.
// to_cbuf (CGAN): the last layer's activation goes to the groups' rows of the head's concat buffer instead of S.a (cg_head_forward
// then has nothing to copy)
static int d_convs_forward(jck_engine* e, const DActs& S, const void* x_in, int B, int pass0, hipStream_t st, bool to_cbuf = false) {
  const int n = S.groups;
  const void* in = x_in;
  for (int i = 0; i < TT.NS; ++i) {
    const int hb = TT.D_HB[i], cs = TT.D_CS[i];
    const long long rows = (long long)B * (hb / 2) * (hb / 2);
    float* rec = e->d_rs[i] + ((size_t)e->parity * 4 + pass0 + S.g0) * 2 * cs;
    int slots = 0;
    JCK_TRY(jck_conv_down_grouped(e->prec, in, e->d_down[i], S.y[i], S.stats[i], &slots, n * B, hb, hb, TT.D_CB[i], cs, B, st));
    if (slots % n) JCK_FAIL(JCK_E_ARG, "batched D pass: statistic slots do not split by group");
    const bool cb = to_cbuf && i == TT.NS - 1;
    void* out = cb ? (unsigned char*)e->cbuf + (size_t)S.g0 * B * L1_KPAD * e->esz : S.a[i];
    bool fused = false;                           // finalize + apply as one launch where the statistics rows are few (ops_bn.hip)
    JCK_TRY(bn_fwd_fused(e->prec, S.y[i], S.stats[i], slots / n, (float)rows, e->P(e->LD, e->dp, NWN[i]), e->P(e->LD, e->dp, NBN[i]), BN_EPS, LRELU, out,
                         S.aux[i], rec, nullptr, nullptr, nullptr, BN_MOM, rows, cs, n, cb ? TT.FEAT : 0, cb ? L1_KPAD : 0, st, &fused));
    if (!fused) {
      JCK_TRY(jck_bn_finalize_grouped(S.stats[i], slots / n, (float)rows, e->P(e->LD, e->dp, NWN[i]), e->P(e->LD, e->dp, NBN[i]), BN_EPS, S.aux[i], rec,
                                      cs, n, st));
      JCK_TRY(bn_act_fwd_pitched(e->prec, S.y[i], S.aux[i], LRELU, out, rows, cs, n, cb ? TT.FEAT : 0, cb ? L1_KPAD : 0, st));
    }
    in = S.a[i];
  }
  return JCK_OK;
}

// D forward up to (not including) the sigmoid head.  family 1: concat + Linear(8392,256) + Dropout (model/CGAN.py:117-122)
// CGAN head up to the dropped-out hidden layer from the conv features a4 [B][8192] (model/CGAN.py:111-121): concat with the
// label embedding, Linear(8392,256), Dropout.  Leaves cbuf, pre_e, h_pre, h_drop for the matching d_head_backward.
// rows: B, or 3B for the batched head (label_period = B: the three groups share the batch's labels; drop_mask = their three
// [B][256] masks back to back)
// finish = false: stops at the split-K slabs of Linear(8392,256); cg_head_mid (one launch) takes it from there
static int cg_head_forward(jck_engine* e, const void* a4, int rows, const float* drop_mask, hipStream_t st, int label_period = 0, bool finish = true) {
  if (!e->cur_labels || !drop_mask) JCK_FAIL(JCK_E_ARG, "CGAN pass needs labels and a dropout mask");
  if (a4) JCK_TRY(jck_concat_rows(e->prec, a4, TT.FEAT, e->cbuf, L1_KPAD, rows, st));      // null: the conv stack wrote the rows itself
  JCK_TRY(jck_label_embed_fwd_tiled(e->prec, e->cur_labels, e->P(e->LD, e->dp, "label_embedding.weight"),
                                    e->P(e->LD, e->dp, "label_embedding.bias"), LRELU, rows, N_CLASS, EMB, e->cbuf, L1_KPAD, TT.FEAT,
                                    e->pre_e, label_period, st));
  JCK_TRY(jck_linear_fwd(e->prec, e->cbuf, e->l1_w, nullptr, e->l1_slab, rows, L1_KPAD, L1_OUT, L1_OUT, L1_KSPLIT, st));
  if (!finish) return JCK_OK;
  return jck_linear_finish(e->prec, e->l1_slab, L1_KSPLIT, e->P(e->LD, e->dp, "linear1.bias"), drop_mask, 1.0f / 0.75f, e->h_pre,
                           e->h_drop, rows, L1_OUT, st);
}
// The head from the split-K slabs to the gradient at the Linear(8392,256) output, rows [0, G * B) of the head buffers: h_pre, h_drop,
// prob / ds / scalar slots per group, g_hd, g_h (ops.hip: cg_head_mid)
static int cg_head_middle(jck_engine* e, int B, int G, const float* targets, const int* modes, const int* slot_loss, const int* slot_p,
                          float* prob, float* ds, const float* drop_mask, hipStream_t st) {
  return cg_head_mid(e->prec, e->l1_slab, L1_KSPLIT, e->P(e->LD, e->dp, "linear1.bias"), drop_mask, 1.0f / 0.75f, e->h_pre, e->h_drop,
                     e->P(e->LD, e->dp, "linear2.weight"), e->P(e->LD, e->dp, "linear2.bias"), B, G, targets, modes, prob, ds, e->acc, slot_loss,
                     slot_p, e->acc_ld, e->g_hd, e->g_h, st);
}

static int d_forward(jck_engine* e, DActs& D, const void* x_in, int B, int pass, const float* drop_mask, hipStream_t st, bool head_finish = true) {
  const bool direct = e->family == 1 && e->cbuf_direct;
  JCK_TRY(d_convs_forward(e, D, x_in, B, pass, st, direct));
  if (e->family == 1) return cg_head_forward(e, direct ? nullptr : D.a[TT.NS - 1], B, drop_mask, st, 0, head_finish);
  return JCK_OK;
}

// sigmoid head + loss (mode 0) or + d(sum p)/dlogit (mode 1); fills D.prob / D.ds
// g_out (family 0, optional): conv5's input gradient ds[n] * w from the same launch
static int d_head(jck_engine* e, DActs& D, int B, float target, int mode, int slot_loss, int slot_p, hipStream_t st, void* g_out = nullptr) {
  if (e->family == 0)
    return head_fwd_grouped_ev(e->prec, D.a[TT.NS - 1], e->d_head_wp, nullptr, B, TT.FEAT, 1, &target, &mode, D.prob, D.ds, e->acc, &slot_loss,
                               &slot_p, e->acc_ld, g_out, st, nullptr);
  return jck_head_fwd(e->prec, e->h_drop, e->P(e->LD, e->dp, "linear2.weight"), e->P(e->LD, e->dp, "linear2.bias"), B, L1_OUT, target,
                      mode, D.prob, D.ds, e->acc, slot_loss, slot_p, e->acc_ld, st);
}

// head backward from ds (device float[B]) down to the gradient w.r.t. a4 in `ga4_out`.
// side (family 1, optional): the parameter gradients run there (see cg_head_backward_batched)
// mid_done: g_hd and g_h are in place (cg_head_middle)
static int d_head_backward(jck_engine* e, DActs& D, const float* ds, int B, bool want_wgrad, const float* drop_mask, void* ga4_out, hipStream_t st,
                           hipStream_t side = nullptr, bool mid_done = false) {
  if (e->family == 0)       // mid_done: the input gradient is in place (d_head with g_out)
    return jck_head_bwd_conv(e->prec, ds, e->d_head_wp, D.a[TT.NS - 1], B, TT.G_C1, mid_done ? nullptr : ga4_out,
                             want_wgrad ? e->P(e->LD, e->dg, CWN[TT.NS]) : nullptr, e->head_ws, st);
  // linear2 + sigmoid: g_hd = ds * w2, dW2 += sum ds * h_drop, db2 += sum ds.  Head buffers from row e->ss.head_row0 on (the
  // penalty group of a batched head sits at rows [2B, 3B))
  const size_t r0 = (size_t)e->ss.head_row0, w0 = (size_t)e->ss.head_wrow0;
  auto hb = [&](void* p, size_t row, size_t per_row) { return (void*)((unsigned char*)p + row * per_row * e->esz); };
  void *h_drop = hb(e->h_drop, r0, L1_OUT), *cbuf = hb(e->cbuf, r0, L1_KPAD);
  void *g_hd = hb(e->g_hd, w0, L1_OUT), *g_h = hb(e->g_h, w0, L1_OUT), *gc = hb(e->gc, w0, L1_KPAD);
  const float* pre_e = e->pre_e + r0 * EMB;
  hipStream_t ws = st;
  auto fork = [&](int k) { return fork_side(e, k, st, side, &ws); };
  const float* w2 = e->P(e->LD, e->dp, "linear2.weight");
  if (!mid_done) JCK_TRY(jck_head_bwd(e->prec, ds, w2, h_drop, B, L1_OUT, g_hd, nullptr, 1, e->head_ws, st));
  if (want_wgrad) {
    JCK_TRY(fork(0));
    JCK_TRY(jck_head_bwd(e->prec, ds, w2, h_drop, B, L1_OUT, nullptr, e->P(e->LD, e->dg, "linear2.weight"), 1, e->head_ws, ws));
    JCK_TRY(jck_sum_vec(ds, B, e->P(e->LD, e->dg, "linear2.bias"), ws));
  }
  if (!mid_done) JCK_TRY(jck_dropout(e->prec, g_hd, drop_mask, 1.0f / 0.75f, g_h, (long long)B * L1_OUT, st));
  if (want_wgrad) {
    JCK_TRY(fork(1));
    JCK_TRY(jck_linear_wgrad(e->prec, g_h, L1_OUT, cbuf, L1_KPAD, e->wg_ws, e->wg_ws_bytes, e->gw1p, 1, B, L1_OUT, ws));
    JCK_TRY(jck_colsum(e->prec, g_h, B, L1_OUT, L1_OUT, e->P(e->LD, e->dg, "linear1.bias"), ws));
  }
  JCK_TRY(jck_linear_fwd(e->prec, g_h, e->l1_wT, nullptr, gc, B, L1_OUT, L1_KPAD, L1_KPAD, 1, st));
  if (want_wgrad) {
    JCK_TRY(fork(2));
    JCK_TRY(jck_label_embed_bwd(e->prec, gc, L1_KPAD, TT.FEAT, pre_e, e->cur_labels, LRELU, B, N_CLASS, EMB,
                                e->P(e->LD, e->dg, "label_embedding.weight"), e->P(e->LD, e->dg, "label_embedding.bias"), ws));
  }
  return jck_split_rows(e->prec, gc, L1_KPAD, TT.FEAT, ga4_out, B, st);
}

// The head backward of the real | fake | penalty groups as ONE pass over 3B rows (forward: cg_head_forward(rows = 3B)): input
// gradients for all three, parameter gradients from the first two (the penalty's come from its double backward, PHASE_D_GP).
// 11 launches instead of 26; the penalty group's rows [2B, 3B) stay behind as gp_double_backward expects them.
// side (optional): the parameter gradients of the head (linear2, linear1, the label embedding: 8 launches, ~80 us that only the
// optimiser waits for) run on the weight-gradient stream - idle at this point of the step - beside the chain that carries the input
// gradient down to the conv stack; evHead marks their end on that stream (PHASE_D_GP's main-stream writers of the same gradients
// wait for it).
static int cg_head_backward_batched(jck_engine* e, const float* ds, int B, const float* drop_mask, void* ga4_out, hipStream_t st,
                                    hipStream_t side = nullptr, bool mid_done = false) {
  const int R3 = 3 * B, R2 = 2 * B;
  const float* w2 = e->P(e->LD, e->dp, "linear2.weight");
  hipStream_t ws = st;
  auto fork = [&](int k) { return fork_side(e, k, st, side, &ws); };
  if (!mid_done) JCK_TRY(jck_head_bwd(e->prec, ds, w2, e->h_drop, R3, L1_OUT, e->g_hd, nullptr, 1, e->head_ws, st));
  if (!mid_done) {        // (with the middle in one launch both forks start at the same point: one hand-over)
    JCK_TRY(fork(0));
    JCK_TRY(jck_head_bwd(e->prec, ds, w2, e->h_drop, R2, L1_OUT, nullptr, e->P(e->LD, e->dg, "linear2.weight"), 1, e->head_ws, ws));
    JCK_TRY(jck_sum_vec(ds, R2, e->P(e->LD, e->dg, "linear2.bias"), ws));
    JCK_TRY(jck_dropout(e->prec, e->g_hd, drop_mask, 1.0f / 0.75f, e->g_h, (long long)R3 * L1_OUT, st));
  }
  JCK_TRY(fork(1));
  if (mid_done) {
    JCK_TRY(jck_head_bwd(e->prec, ds, w2, e->h_drop, R2, L1_OUT, nullptr, e->P(e->LD, e->dg, "linear2.weight"), 1, e->head_ws, ws));
    JCK_TRY(jck_sum_vec(ds, R2, e->P(e->LD, e->dg, "linear2.bias"), ws));
  }
  JCK_TRY(jck_linear_wgrad(e->prec, e->g_h, L1_OUT, e->cbuf, L1_KPAD, e->wg_ws, e->wg_ws_bytes, e->gw1p, 1, R2, L1_OUT, ws));
  JCK_TRY(jck_colsum(e->prec, e->g_h, R2, L1_OUT, L1_OUT, e->P(e->LD, e->dg, "linear1.bias"), ws));
  JCK_TRY(jck_linear_fwd(e->prec, e->g_h, e->l1_wT, nullptr, e->gc, R3, L1_OUT, L1_KPAD, L1_KPAD, 1, st));
  JCK_TRY(fork(2));
  JCK_TRY(jck_label_embed_bwd_tiled(e->prec, e->gc, L1_KPAD, TT.FEAT, e->pre_e, e->cur_labels, LRELU, R2, N_CLASS, EMB,
                                    e->P(e->LD, e->dg, "label_embedding.weight"), e->P(e->LD, e->dg, "label_embedding.bias"), B, ws));
  if (side) HIPCHK(hipEventRecord(e->evHead, side));
  return jck_split_rows(e->prec, e->gc, L1_KPAD, TT.FEAT, ga4_out, R3, st);
}

// xe (G's loss pass): the input gradient is wanted only as the operand of the tanh + noise-mix backward of G's output - that
// product rides in the epilogue of the launch that computes it (conv_up_tanh_bwd_ev) when the layer runs on the image-side kernel
struct XgradEpi { const void* tanh_y; float scale; void* out; hipEvent_t done; bool fused; };
// What a backward pass through D's conv stack does beside the dgrad chain
struct DBackward {
  int gw = 1;                   // the first gw groups contribute weight gradients (0: no parameter gradient is wanted)
  hipStream_t side = nullptr;   // the weight-gradient products run on this stream beside the dgrad chain (both only READ gy_i and the
                                // saved activations)
  // join = false: the caller's NEXT backward with a side stream (or its own join) orders the main stream behind these weight
  // gradients - nothing on the main stream reads them before the optimiser step.  lazy_join (JCK_PHASE_LAZY_JOIN): the side stream
  // is marked, whoever comes next waits
  bool join = true, lazy_join = false;
  // part 0: the whole pass.  part 1 / 2 (data parallel, PHASE_D_LOSS_A / _B): up to and including the weight gradient of the LAST
  // layer (joined into `st`: the tail of D's gradient arena - conv4.weight, norm4.*, conv5.weight - is then final in `st` order and
  // its all-reduce can start) / everything after it
  int part = 0;
  // resident = false: the pass runs beside another pass of the step on a second stream.  Two resident BatchNorm launches in flight
  // at once would share the engine's barrier words and could each hold CUs the other's missing workgroups need: such a pass takes
  // the three-launch form
  bool resident = true;
  bool xgrad = false;           // the gradient w.r.t. the input image of the LAST group -> S.gx ...
  XgradEpi* xe = nullptr;       // ... or into the epilogue above
  bool gp_norm = false;         // ... and its per-image norms -> S.norms (the penalty pass)
};
// Backward of D's conv stack for the groups of `S` whose gradients w.r.t. the top activation are in S.g[NS - 1] (x_in = first image
// of the first group): BatchNorm backward grouped, ONE dgrad launch per layer over all groups, ONE weight-gradient launch per
// layer over the first o.gw groups.
static int d_convs_backward(jck_engine* e, const DActs& S, const void* x_in, int B, hipStream_t st, const DBackward& o) {
  const int G = S.groups, gw = o.gw;
  hipStream_t side = gw > 0 ? o.side : nullptr;
  for (int i = TT.NS - 1; i >= 0; --i) {
    const int hb = TT.D_HB[i], cs = TT.D_CS[i], cb = TT.D_CB[i];
    const long long rows = (long long)B * (hb / 2) * (hb / 2);
    const bool resume = o.part == 2 && i == TT.NS - 1;      // part 2 starts at this layer's dgrad
    // The bottom layer's weight gradient is the last product of the pass and nothing but the penalty's image gradient runs
    // beside it (37 us of the main stream waiting for it in round 3).  Its operand is the gradient of the LOSS groups only:
    // their BatchNorm backward goes first, the weight gradient starts behind it on the second stream, and the penalty
    // group's BatchNorm backward (a launch of its own - in the resident form the groups of this layer go one after the other
    // anyway) runs beside it.
    // (the split does not depend on the stream layout: a captured, one-stream step is the same arithmetic launch for launch)
    const bool split0 = !resume && i == 0 && e->bn_res && e->prec == JCK_PREC_BF16 && gw > 0 && gw < G;
    hipEvent_t done = side && e->ext_events && !resume ? e->evW[i] : nullptr;    // the launch that writes g_y completes evW[i] itself
    if (!resume)
      JCK_TRY(bn_act_bwd_res_ev(e->prec, S.g[i], S.y[i], S.aux[i], LRELU, S.sums[i], S.g[i], gw ? e->P(e->LD, e->dg, NWN[i]) : nullptr,
                                gw ? e->P(e->LD, e->dg, NBN[i]) : nullptr, rows, cs, split0 ? gw : G, gw,
                                e->bn_res && o.resident ? e->gsync : nullptr, st, done));
    if (!resume && gw) {
      hipStream_t ws;
      JCK_TRY(fork_side(e, i, st, side, &ws, !done));
      JCK_TRY(jck_conv_wgrad(e->prec, S.g[i], i == 0 ? x_in : S.a[i - 1], e->wg_ws, e->wg_ws_bytes, e->P(e->LD, e->dg, CWN[i]), 1, gw * B, hb, hb, cb,
                             cs, ws));
    }
    if (split0) {
      const DActs P = S.group(e, gw, G - gw);
      JCK_TRY(bn_act_bwd_res_ev(e->prec, P.g[i], P.y[i], P.aux[i], LRELU, P.sums[i], P.g[i], nullptr, nullptr, rows, cs, G - gw, 0, e->gsync, st, nullptr));
    }
    if (o.part == 1) {
      // evTail: the tail of D's gradient arena is final behind it (jck_engine_order_after_tail); lazy_join: st does not wait
      HIPCHK(hipEventRecord(e->evTail, side ? side : st));
      e->ss.tail_on_side = side != nullptr;
      if (side && !o.lazy_join) HIPCHK(hipStreamWaitEvent(st, e->evTail, 0));
      return JCK_OK;
    }
    if (i > 0)
      JCK_TRY(jck_conv_up(e->prec, S.g[i], e->d_up[i], S.g[i - 1], nullptr, nullptr, 0, G * B, hb / 2, hb / 2, cs, cb, st));
    else if (o.xgrad) {
      const void* g0 = S.group(e, G - 1, 1).g[0];
      if (o.xe) JCK_TRY(conv_up_tanh_bwd_ev(e->prec, g0, e->d_up[0], o.xe->tanh_y, o.xe->scale, o.xe->out, B, hb / 2, hb / 2, cs, cb, st, o.xe->done, &o.xe->fused));
      if (!o.xe || !o.xe->fused) JCK_TRY(jck_conv_up(e->prec, g0, e->d_up[0], S.gx, nullptr, nullptr, 0, B, hb / 2, hb / 2, cs, cb, st));
    }
  }
  // the penalty's norm does not need the weight gradients: it runs while the side stream finishes the last of them
  if (o.gp_norm) JCK_TRY(jck_gp_norm(e->prec, S.gx, B, TT.HW, e->acc, 6, e->acc_ld, S.norms, st));
  if (side && o.join) {
    HIPCHK(hipEventRecord(e->evWdone, side));
    if (o.lazy_join) { e->ss.join_pending = true; e->ss.mid_recorded = false; }
    else HIPCHK(hipStreamWaitEvent(st, e->evWdone, 0));
  }
  return JCK_OK;
}
// one pass's backward on its set `D`: the head from D.ds down to the gradient w.r.t. a4, then the conv stack
static int d_backward(jck_engine* e, DActs& D, const void* x_in, int B, const float* drop_mask, hipStream_t st, const DBackward& o,
                      bool head_mid_done = false) {
  JCK_TRY(d_head_backward(e, D, D.ds, B, o.gw > 0, drop_mask, D.g[TT.NS - 1], st, nullptr, head_mid_done));
  return d_convs_backward(e, D, x_in, B, st, o);
}

// DCGAN's heads and backward on the G batches stored back to back from `x_in` (real_noisy | fake | xhat are consecutive; the
// forward has filled every group: d_batched_forward): ONE launch per layer instead of G.  Groups
// [0, G-1) are loss passes (targets / accumulator slots given per group) and contribute weight gradients; the LAST group is the
// penalty pass (head mode 1, gradient w.r.t. its input image -> dset[0].gx, norms -> dset[0].norms).  Weight gradients run on `side`.
static int d_batched_pass(jck_engine* e, const void* x_in, int B, int G, const float* targets, const int* slot_loss, const int* slot_p,
                          hipStream_t st, hipStream_t side, int part = 0, bool lazy_tail = false) {
  const DActs S = e->bset.group(e, 0, G);
  const int gw = G - 1;
  DBackward bw;
  bw.gw = gw; bw.side = side; bw.xgrad = bw.gp_norm = true; bw.part = part; bw.lazy_join = part == 1 && lazy_tail;
  if (part == 2) return d_convs_backward(e, S, x_in, B, st, bw);
  {
    float tg[4] = {0.f, 0.f, 0.f, 0.f};
    int md[4] = {0, 0, 0, 0}, sl[4] = {-1, -1, -1, -1}, sp[4] = {-1, -1, -1, -1};
    for (int g = 0; g < G; ++g) {
      const bool pen = g == G - 1;
      tg[g] = pen ? 0.f : targets[g]; md[g] = pen ? 1 : 0; sl[g] = pen ? -1 : slot_loss[g]; sp[g] = pen ? -1 : slot_p[g];
    }
    // conv5's forward also writes the rows' input gradient and completes the hand-over event itself: the weight gradient (partial
    // rows + their ordered sum) is then all the weight-gradient stream's (JCK_HEAD_FUSE=0: head_bwd_fused_kernel does both on st)
    JCK_TRY(head_fwd_grouped_ev(e->prec, S.a[TT.NS - 1], e->d_head_wp, nullptr, B, TT.FEAT, G, tg, md, S.prob, S.ds, e->acc, sl, sp, e->acc_ld,
                                e->head_fuse ? S.g[TT.NS - 1] : nullptr, st, e->head_fuse && side && e->ext_events ? e->evHead : nullptr));
  }
  // loss groups (input + weight gradient) and the penalty group (input gradient only), one launch
  // (the ordered sum of conv5's weight-gradient rows is wanted by the optimiser only: weight-gradient stream, 10 us off the main one)
  const bool hs = side && e->ext_events && e->head_side;
  if (e->head_fuse) {
    const bool hf = side && e->ext_events;
    JCK_TRY(head_bwd_conv2_ev(e->prec, S.ds, e->d_head_wp, S.a[TT.NS - 1], gw * B, 0, TT.G_C1, nullptr, e->P(e->LD, e->dg, CWN[TT.NS]),
                              e->head_ws, st, hf ? side : nullptr, hf ? e->evHead : nullptr));
  } else
    JCK_TRY(head_bwd_conv2_ev(e->prec, S.ds, e->d_head_wp, S.a[TT.NS - 1], gw * B, B, TT.G_C1, S.g[TT.NS - 1], e->P(e->LD, e->dg, CWN[TT.NS]),
                              e->head_ws, st, hs ? side : nullptr, hs ? e->evHead : nullptr));
  return d_convs_backward(e, S, x_in, B, st, bw);
}

// The back-propagated gradient penalty (train/cgan_trainer.py:200-203; DCGAN with JCK_ENGINE_GP_BACKWARD).  Precondition: the GP forward and first backward
// have run (d_forward(xhat), d_head(mode 1), d_backward(gw = 0, xgrad)), so P.g[i] = gy_i, P.sums[i] = first-
// backward sums, g_h = gradient at the Linear(8392,256) output, P.gx = g_x, P.norms = ||g_x[n]||.  Accumulates
// lambda * dGP/dtheta into D's gradient arena.  Derivation + fp64 check: tests/test_gp_double_backward_math.py.
// `side` (optional): the weight-gradient products run there beside the v-chain / reverse sweep; they share the split-K
// workspace, so everything that uses it is ordered on that one stream, and the main stream joins it before the reverse sweep
// (which overwrites the v_i the v-chain products read and runs the Linear weight gradient on the main stream) and at the end.
// P: where the penalty pass left its forward / first-backward tensors, image gradient and norms - the set of a per-pass penalty
// pass (set 1: DCGAN's on its own stream), or the last group of the batched set
static int gp_double_backward(jck_engine* e, const DActs& P, const void* xhat, int B, float lambda, const float* drop_mask, hipStream_t st,
                              hipStream_t side = nullptr, bool lazy_join = false) {
  const size_t esz = e->esz;
  hipStream_t ws = st;
  auto fork = [&](int k) { return fork_side(e, k, st, side, &ws); };
  auto join = [&]() {
    if (!side) return;
    (void)hipEventRecord(e->evWdone, side);
    (void)hipStreamWaitEvent(st, e->evWdone, 0);
  };
  // the first backward's gradient at the Linear(8392,256) output and the penalty pass's probabilities: read in place after a
  // batched head (its penalty rows [2B, 3B) are not written again: the head backward below writes rows [0, B)), copied aside
  // otherwise (the per-pass head backward below overwrites g_h)
  // the head's parameter gradients of PHASE_D_LOSS may still be queued on the weight-gradient stream (cg_head_backward_batched, no
  // join in between under JCK_PHASE_LAZY_JOIN): this pass adds to the same tensors from the main stream
  const bool cg = e->family == 1;
  const void* gh1 = e->gh_b1;
  const float* prob1 = e->prob_gp;
  if (cg) {
    if (side) (void)hipStreamWaitEvent(st, e->evHead, 0);
    if (e->ss.head_row0 > 0) {
      gh1 = (const unsigned char*)e->g_h + (size_t)e->ss.head_row0 * L1_OUT * esz;
      prob1 = P.prob;
    } else {
      HIPCHK(hipMemcpyAsync(e->gh_b1, e->g_h, (size_t)B * L1_OUT * esz, hipMemcpyDeviceToDevice, st));
      HIPCHK(hipMemcpyAsync(e->prob_gp, P.prob, (size_t)B * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
  }
  JCK_TRY(jck_gp_grad(e->prec, P.gx, P.norms, 2.0f * lambda / (float)B, B, TT.HW, e->d_u0, st));
  // ---- v-chain: adjoint of the first backward, swept forward through D
  const void* u = e->d_u0;
  for (int i = 0; i < TT.NS; ++i) {
    const int hb = TT.D_HB[i], cs = TT.D_CS[i], cb = TT.D_CB[i];
    const long long rows = (long long)B * (hb / 2) * (hb / 2);
    // g_{a_{i-1}} = convT(gy_i; W_i):  dW_i += wgrad(gy_i, u_{i-1}),  v_i = conv(u_{i-1}; W_i)
    JCK_TRY(fork(i));
    JCK_TRY(jck_conv_wgrad(e->prec, P.g[i], u, e->wg_ws, e->wg_ws_bytes, e->P(e->LD, e->dg, CWN[i]), 1, B, hb, hb, cb, cs, ws));
    JCK_TRY(jck_conv_down(e->prec, u, e->d_down[i], e->d_v[i], nullptr, nullptr, B, hb, hb, cb, cs, st));
    JCK_TRY(jck_bn2_vchain(e->prec, e->d_v[i], P.y[i], P.g[i], P.aux[i], P.sums[i], e->P(e->LD, e->dp, NWN[i]),
                           LRELU, e->bn2_ws[i], e->d_v[i], e->d_xdir[i], e->P(e->LD, e->dg, NWN[i]), rows, cs, st));
    u = e->d_v[i];
  }
  if (!cg) {
    // DCGAN's head (conv5 + sigmoid) in one step (ops.hip: jck_gp_head2_conv): rs, conv5.weight's gradient and the reverse sweep's
    // input g_a4 = rs * w5 written over v4.  The v-chain's products on the weight-gradient stream read v_0 .. v_{NS-2}, which the
    // reverse sweep overwrites: it waits for the mark behind the last of them.
    if (side) (void)hipEventRecord(e->evGP, side);
    JCK_TRY(jck_gp_head2_conv(e->prec, e->d_v[TT.NS - 1], P.a[TT.NS - 1], e->d_head_wp, P.prob, B, TT.G_C1, e->rs, e->d_v[TT.NS - 1],
                              e->P(e->LD, e->dg, CWN[TT.NS]), e->gp2_ws, st));
    if (side) (void)hipStreamWaitEvent(st, e->evGP, 0);
  } else {
    // head: gc[:, :8192] = gh W1 -> adj(gh) = [u4 | 0] W1^T, dW1 += gh^T [u4 | 0]; gh = gh' * m/(1-p); gh' = ds w2; ds = p(1-p)
    JCK_TRY(jck_concat_rows(e->prec, e->d_v[TT.NS - 1], TT.FEAT, e->cbuf2, L1_KPAD, B, st));          // tail columns of cbuf2: the zeros of jck_engine_bind
    JCK_TRY(fork(0));
    JCK_TRY(jck_linear_wgrad(e->prec, gh1, L1_OUT, e->cbuf2, L1_KPAD, e->wg_ws, e->wg_ws_bytes, e->gw1p, 1, B, L1_OUT, ws));
    // What the reverse sweep must wait for are the v-chain's products (they read the v_i it overwrites): the weight-gradient stream is
    // marked HERE, behind the last of them - not after the head's parameter gradients, which are forked to it below and which nothing
    // on the main stream waits for before the optimiser
    if (side) (void)hipEventRecord(e->evGP, side);
    JCK_TRY(jck_linear_fwd(e->prec, e->cbuf2, e->l1_w, nullptr, e->l1_slab, B, L1_KPAD, L1_OUT, L1_OUT, L1_KSPLIT, st));
    const bool fuse = e->head_fuse && L1_OUT == 256;    // the next four launches as one (ops.hip: gp_head_mid_ev)
    if (!fuse) JCK_TRY(jck_linear_finish(e->prec, e->l1_slab, L1_KSPLIT, nullptr, drop_mask, 1.0f / 0.75f, nullptr, e->ughd, B, L1_OUT, st));
    // (the head's parameter gradients - the dw2 sum here, linear2 / linear1 / the label embedding in d_head_backward below: ~75 us of
    // launches that only the optimiser waits for - go to the weight-gradient stream; JCK_HEAD_SIDE=0 keeps them on the main one)
    hipStream_t hs = e->head_side && e->ext_events ? side : nullptr;
    if (fuse) {
      // g_hd / g_h rows [head_wrow0, + B): not the rows the v-chain's Linear weight gradient reads (the penalty group's, or the copy)
      const size_t w0 = (size_t)e->ss.head_wrow0 * L1_OUT * esz;
      JCK_TRY(gp_head_mid_ev(e->prec, e->l1_slab, L1_KSPLIT, drop_mask, 1.0f / 0.75f, e->ughd, e->P(e->LD, e->dp, "linear2.weight"), prob1, B, e->rs,
                             e->P(e->LD, e->dg, "linear2.weight"), e->gp2_ws, (unsigned char*)e->g_hd + w0, (unsigned char*)e->g_h + w0, st, hs,
                             hs ? e->evHead : nullptr));
    } else
      JCK_TRY(gp_head2_ev(e->prec, e->ughd, e->P(e->LD, e->dp, "linear2.weight"), prob1, B, L1_OUT, e->rs,
                          e->P(e->LD, e->dg, "linear2.weight"), e->gp2_ws, st, hs, hs ? e->evHead : nullptr));
    // ---- reverse sweep through the forward pass from the logit adjoint rs, with the extra BatchNorm inputs
    if (side) (void)hipStreamWaitEvent(st, e->evGP, 0); else join();
    JCK_TRY(d_head_backward(e, e->dset[0], e->rs, B, true, drop_mask, e->d_v[TT.NS - 1], st, hs, fuse));
    // the last sum into the permuted Linear gradient is enqueued: back to the reference's layout, on the stream that holds it
    JCK_TRY(jck_unperm_linear_grad(e->gw1p, L1_OUT, L1_K, L1_KPAD, 512, 16, e->P(e->LD, e->dg, "linear1.weight"), 1, hs ? hs : st));
  }
  for (int i = TT.NS - 1; i >= 0; --i) {
    const int hb = TT.D_HB[i], cs = TT.D_CS[i], cb = TT.D_CB[i];
    const long long rows = (long long)B * (hb / 2) * (hb / 2);
    JCK_TRY(jck_bn2_reverse(e->prec, e->d_v[i], P.y[i], e->d_xdir[i], P.aux[i], e->P(e->LD, e->dp, NWN[i]), e->bn2_ws[i],
                            LRELU, e->bn2_ws_rev, e->d_v[i], e->P(e->LD, e->dg, NWN[i]), e->P(e->LD, e->dg, NBN[i]), rows, cs, st));
    const void* big = i == 0 ? xhat : P.a[i - 1];
    JCK_TRY(fork(i));
    JCK_TRY(jck_conv_wgrad(e->prec, e->d_v[i], big, e->wg_ws, e->wg_ws_bytes, e->P(e->LD, e->dg, CWN[i]), 1, B, hb, hb, cb, cs, ws));
    // everything but the bottom conv weight's gradient is final on the side stream here (lazy join: the optimiser phase starts
    // behind this point and takes that one tensor last)
    if (side && lazy_join && i == 1) { (void)hipEventRecord(e->evWmid, side); e->ss.mid_recorded = true; }
    if (i > 0)
      JCK_TRY(jck_conv_up(e->prec, e->d_v[i], e->d_up[i], e->d_v[i - 1], nullptr, nullptr, 0, B, hb / 2, hb / 2, cs, cb, st));
  }
  if (side && lazy_join) { (void)hipEventRecord(e->evWdone, side); e->ss.join_pending = true; }
  else join();
  return JCK_OK;
}

// The eval-mode generator in two pieces (g_forward(eval) runs both; a latent projection folds once and runs the products per iteration).
// Fold: one launch writes every layer's scale / shift (gamma, beta and the running statistics) into the stage's aux table ...
int g_eval_fold(jck_engine* e, hipStream_t st) {
  const float *gamma[JCK_MAX_STAGES], *beta[JCK_MAX_STAGES], *rm[JCK_MAX_STAGES], *rv[JCK_MAX_STAGES];
  float* aux[JCK_MAX_STAGES];
  int Cs[JCK_MAX_STAGES];
  for (int i = 0; i < TT.NS; ++i) {
    gamma[i] = e->P(e->LG, e->gp, NWN[i]); beta[i] = e->P(e->LG, e->gp, NBN[i]);
    rm[i] = e->gbn + find(e->LG, RMN[i])->offset; rv[i] = e->gbn + find(e->LG, RVN[i])->offset;
    aux[i] = e->g_bn[i].aux; Cs[i] = TT.G_C1 >> i;
  }
  return jck_bn_eval_aux(TT.NS, gamma, beta, rm, rv, aux, Cs, BN_EPS, st);
}
// ... and the products apply them and the ReLU in their epilogues: g_z -> g_a[0..NS-1] -> fake_raw
int g_eval_products(jck_engine* e, int B, hipStream_t st) {
  const int zp = z_pad(e->family);
  auto scale = [&](int i) { return e->g_bn[i].aux; };
  auto shift = [&](int i) { return e->g_bn[i].aux + (TT.G_C1 >> i); };
  JCK_TRY(jck_g1_fwd_affine(e->prec, e->g_z, e->g1_w, scale(0), shift(0), e->g_a[0], B, zp, TT.G_C1, st));
  for (int i = 0; i < TT.NS; ++i) {
    const int h = 4 << i;
    if (i < TT.NS - 1)
      JCK_TRY(jck_conv_up_affine(e->prec, e->g_a[i], e->g_up[i], scale(i + 1), shift(i + 1), e->g_a[i + 1], B, h, h, TT.G_CS[i], TT.G_CB[i], st));
    else
      JCK_TRY(jck_conv_up(e->prec, e->g_a[i], e->g_up[i], e->fake_raw, nullptr, nullptr, 1, B, h, h, TT.G_CS[i], TT.G_CB[i], st));
  }
  return JCK_OK;
}

// eval: BatchNorm with the RUNNING statistics (model.eval()): one launch folds every layer's gamma, beta and running statistics into
// scale / shift (the stage's aux table, which every train-mode forward rewrites before its backward reads it), and each product
// applies them and the ReLU in its epilogue - one launch and one activation store per stage, images independent of each other,
// no statistics, running statistics and num_batches_tracked untouched.
int g_forward(jck_engine* e, const float* z, const int64_t* labels, int B, hipStream_t st, bool z_in_place, bool eval) {
  const int zp = z_pad(e->family);
  if (e->family == 1) {
    if (!labels) JCK_FAIL(JCK_E_ARG, "CGAN generator needs labels");
    JCK_TRY(jck_cgan_z(e->prec, z, labels, B, 100, N_CLASS, zp, e->g_z, st));            // model/CGAN.py:154-155
  } else if (!z_in_place) {                 // (z_in_place: the step's set-step launch drew this z and wrote the operand rows itself)
    e->ss.gz_step = -1;                        // the operand rows now hold somebody else's z
    if (e->prec == JCK_PREC_BF16) launch_pad_rows<bf16_t>(z, B, 100, zp, e->g_z, st); else launch_pad_rows<float>(z, B, 100, zp, e->g_z, st);
    HIPCHK(hipGetLastError());
  }
  if (eval) {
    JCK_TRY(g_eval_fold(e, st));
    return g_eval_products(e, B, st);
  }
  JCK_TRY(jck_g1_fwd(e->prec, e->g_z, e->g1_w, e->g_y[0], e->g_bn[0].stats, &e->g_bn[0].slots, B, zp, TT.G_C1, st));
  for (int i = 0; i < TT.NS; ++i) {
    const int h = 4 << i, C = TT.G_C1 >> i;
    const long long rows = (long long)B * h * h;
    bool fused = false;
    JCK_TRY(bn_fwd_fused(e->prec, e->g_y[i], e->g_bn[i].stats, e->g_bn[i].slots, (float)rows, e->P(e->LG, e->gp, NWN[i]), e->P(e->LG, e->gp, NBN[i]), BN_EPS,
                         0.f, e->g_a[i], e->g_bn[i].aux, nullptr, e->gbn + find(e->LG, RMN[i])->offset, e->gbn + find(e->LG, RVN[i])->offset,
                         (int64_t*)(e->gnbt + i), BN_MOM, rows, C, 1, 0, 0, st, &fused));
    if (!fused) {
    JCK_TRY(jck_bn_finalize(e->g_bn[i].stats, e->g_bn[i].slots, (float)rows, e->P(e->LG, e->gp, NWN[i]), e->P(e->LG, e->gp, NBN[i]),
                            e->gbn + find(e->LG, RMN[i])->offset, e->gbn + find(e->LG, RVN[i])->offset,
                            e->gnbt + i, BN_MOM, BN_EPS, e->g_bn[i].aux, C, st));
    JCK_TRY(jck_bn_act_fwd(e->prec, e->g_y[i], e->g_bn[i].aux, 0.f, e->g_a[i], rows, C, st));
    }
    if (i < TT.NS - 1)
      JCK_TRY(jck_conv_up_grouped(e->prec, e->g_a[i], e->g_up[i], e->g_y[i + 1], e->g_bn[i + 1].stats, &e->g_bn[i + 1].slots, B, h, h, TT.G_CS[i], TT.G_CB[i], B, st));
    else                                             // last ConvTranspose + tanh -> the image
      JCK_TRY(jck_conv_up(e->prec, e->g_a[i], e->g_up[i], e->fake_raw, nullptr, nullptr, 1, B, h, h, TT.G_CS[i], TT.G_CB[i], st));
  }
  return JCK_OK;
}

// g_fake = gradient w.r.t. the noisy fake image (NHWC4); fills G's grads arena (accumulating)
// raw_ready: g_raw was written by the launch that computed g_fake (XgradEpi), which also completed the first stage's event
static int g_backward(jck_engine* e, const void* g_fake, int B, hipStream_t st, hipStream_t side, bool raw_ready = false) {
  // every launch that writes a gradient the weight-gradient stream reads (tanh backward, then the BatchNorm backward of each
  // stage) completes that stage's event itself
  const bool ext = side && e->ext_events;
  if (!raw_ready)
    JCK_TRY(tanh_bwd_ev(e->prec, g_fake, e->fake_raw, 0.9f, e->g_raw, (long long)B * TT.HW * 4, st, ext ? e->evW[TT.NS - 1] : nullptr));
  const void* gbig = e->g_raw;       // gradient w.r.t. the output of conv(i+2)
  for (int i = TT.NS - 1; i >= 0; --i) {     // stage i: conv(i+2): small = g_a[i] (C = TT.G_CS[i]), big side has TT.G_CB[i] channels
    const int hs = TT.G_HS[i], cs = TT.G_CS[i], cb = TT.G_CB[i];
    hipStream_t ws = st;
    if (side) { if (!ext) HIPCHK(hipEventRecord(e->evW[i], st)); HIPCHK(hipStreamWaitEvent(side, e->evW[i], 0)); ws = side; }
    JCK_TRY(jck_conv_wgrad(e->prec, e->g_a[i], gbig, e->wg_ws, e->wg_ws_bytes, e->P(e->LG, e->gg, CWN[i + 1]), 1, B,
                           2 * hs, 2 * hs, cb, cs, ws));
    const long long rows = (long long)B * hs * hs;
    JCK_TRY(jck_conv_down(e->prec, gbig, e->g_down[i], e->g_gr[i], nullptr, nullptr, B, 2 * hs, 2 * hs, cb, cs, st));
    // g_gr[i] is what stage i - 1's weight gradient reads
    JCK_TRY(bn_act_bwd_res_ev(e->prec, e->g_gr[i], e->g_y[i], e->g_bn[i].aux, 0.f, e->g_bn[i].sums, e->g_gr[i],
                              e->P(e->LG, e->gg, NWN[i]), e->P(e->LG, e->gg, NBN[i]), rows, cs, 1, 1, e->bn_res ? e->gsync : nullptr, st,
                              ext && i > 0 ? e->evW[i - 1] : nullptr));
    gbig = e->g_gr[i];
  }
  // G.conv1's weight gradient depends on the last kernel of the main stream: it runs there, behind it, with its own
  // workspace (forking it to the side stream cost a ~12 us cross-stream hand-over at the very end of the step, twice)
  JCK_TRY(jck_g1_wgrad(e->prec, e->g_z, e->g_gr[0], e->g1_ws, e->g1_ws_bytes, e->P(e->LG, e->gg, CWN[0]), 1, B, z_dim(e->family),
                       z_pad(e->family), TT.G_C1, st));
  if (side) { HIPCHK(hipEventRecord(e->evWdone, side)); HIPCHK(hipStreamWaitEvent(st, e->evWdone, 0)); }
  return JCK_OK;
}

// the real batch -> NHWC4 with instance noise (:160): from an fp32 NCHW tensor, or gathered from the device-resident uint8
// dataset with the input transform applied on the fly
static int prep_real(jck_engine* e, const jck_step_inputs* in, int B, hipStream_t st) {
  if (in->real_u8 && in->real_box_h)     // a box of every image: real_taps is the box's table (the launcher refuses a missing one)
    return jck_img_prep_u8_box(e->prec, in->real_u8, in->real_idx, in->real_flip, in->real_origin, in->noise_real, in->noise_real ? nullptr : e->rng(),
                               0, 0.9f, 0.1f, e->real_noisy, nullptr, B, in->real_h, in->real_w, in->real_box_h, in->real_box_w, in->real_y0,
                               in->real_x0, TT.S, in->real_taps, st);
  if (in->real_u8 && in->real_taps)      // any source size, either engine size, optional mirror: Pillow's general bilinear taps
    return jck_img_prep_u8_any(e->prec, in->real_u8, in->real_idx, in->real_flip, in->noise_real, in->noise_real ? nullptr : e->rng(), 0,
                               0.9f, 0.1f, e->real_noisy, nullptr, B, in->real_h, in->real_w, TT.S, in->real_taps, st);
  if (in->real_u8) {
    if (TT.S != 64) JCK_FAIL(JCK_E_ARG, "the device-resident uint8 pipeline is the reference's Resize(64) of 32x32 images: 64x64 engines only");
    if (!in->noise_real)
      return jck_img_prep_u8_rng(e->prec, in->real_u8, in->real_idx, e->rng(), 0, 0.9f, 0.1f, e->real_noisy, B, 32, 32, st);
    return jck_img_prep_u8(e->prec, in->real_u8, in->real_idx, in->noise_real, 0.9f, 0.1f, e->real_noisy, nullptr, B, 32, 32, st);
  }
  if (!in->noise_real) return jck_img_prep_rng(e->prec, in->real_nchw, e->rng(), 0, 0.9f, 0.1f, e->real_noisy, B, TT.HW, st);
  return jck_img_prep(e->prec, in->real_nchw, in->noise_real, 0.9f, 0.1f, e->real_noisy, B, TT.HW, st);
}

// An optimiser phase called with another learning rate than the step's loss phases (separate G and D rates): only the Adam
// scalars of the step's slot are rewritten - NOT the accumulator rows (the step's losses are in them, the tail of G_STEP reads
// them) and not the step's random inputs (jck_engine_set_step here logged loss_d = loss_g = gp = 0).
static int refresh_adam_scalars(jck_engine* e, int step, float lr, hipStream_t st) {
  const int q = step & 1;
  JCK_TRY(jck_adam_set_step(e->hp2 + 8 * q, (double)lr, ADAM_B1, ADAM_B2, step, e->noise_seed, e->ema_w(step), st));
  e->hp_step[q] = step;
  e->hp_lr[q] = lr;
  return JCK_OK;
}
static int set_step_impl(jck_engine* e, int step, float lr, void* stream, bool zero_d);
// Adam (:180, :189) on elements [first, first + count) of a network's arenas (net 0: G, 1: D) with the step's scalars `hp`.
// zero_other: the other network's gradient arena, cleared by the same launch; ema: G's moving average, advanced by it
static int adam_net(jck_engine* e, int net, long long first, long long count, float grad_scale, const float* hp, hipStream_t st,
                    float* zero_other = nullptr, float* ema = nullptr) {
  float *p = net ? e->dp : e->gp, *g = net ? e->dg : e->gg, *m = net ? e->dm : e->gm, *v = net ? e->dv : e->gv;
  return jck_adam_hp(p + first, g + first, m + first, v + first, count, ADAM_B1, ADAM_B2, ADAM_EPS, grad_scale, hp, st, zero_other,
                     zero_other ? (net ? e->LG : e->LD).n_params : 0, jck_grid_sync_error_word(e->gsync), ema);
}
// adam_net and repack_convs for the conv weights inside the range as ONE launch (ew_optim.hpp: adam_pack_kernel), same values;
// JCK_ADAM_PACK=0, or an arena that is not 16-byte aligned: the two launches
static int adam_repack_net(jck_engine* e, int net, long long first, long long count, float grad_scale, const float* hp, hipStream_t st,
                           float* zero_other = nullptr, float* ema = nullptr, const TailJobs* tail = nullptr, int tail_x = 0) {
  float *p = net ? e->dp : e->gp, *g = net ? e->dg : e->gg, *m = net ? e->dm : e->gm, *v = net ? e->dv : e->gv;
  if (!e->adam_pack || (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) & 15)) {
    JCK_TRY(adam_net(e, net, first, count, grad_scale, hp, st, zero_other, ema));
    return repack_convs(e, net, st, tail, tail_x);
  }
  PackJobs jobs = {};
  pack_jobs(e, net, jobs);
  if (net == 1) e->d_packed = true;
  return jck_adam_pack_hp(e->prec, p, g, m, v, ema, first, count, jobs, ADAM_B1, ADAM_B2, ADAM_EPS, grad_scale, hp, 0.f, 1.f, 1.f, st, zero_other,
                          zero_other ? (net ? e->LG : e->LD).n_params : 0, jck_grid_sync_error_word(e->gsync), tail, tail_x);
}
// `p` (and `p2`) cleared by a neighbour launch for this step - `clean_step`, a promise that is consumed here - else by a memset
// (captured steps, a phase called twice)
static int clear_or_memset(jck_engine* e, int& clean_step, int step, hipStream_t st, void* p, size_t bytes, void* p2 = nullptr, size_t bytes2 = 0) {
  const bool clean = clean_step == step && !e->capturing;
  clean_step = -1;
  if (!clean) HIPCHK(hipMemsetAsync(p, 0, bytes, st));
  if (!clean && p2) HIPCHK(hipMemsetAsync(p2, 0, bytes2, st));
  return JCK_OK;
}
// D.zero_grad() (:155): cleared by the step's set-step launch when that has just run for this step (zero_d), else by a memset
static int zero_d_grads(jck_engine* e, int step, hipStream_t st) {
  return clear_or_memset(e, e->ss.dg_clean_step, step, st, e->dg, e->LD.n_params * sizeof(float), e->family == 1 ? e->gw1p : nullptr,
                         (size_t)L1_OUT * L1_KPAD * sizeof(float));
}
// the step's accumulator rows (losses, probabilities, penalty norms): cleared by the launch that wrote the step's scalars
// (jck_engine_set_step) when that has just run for this step, else - captured steps, a phase called twice - by a memset
static int clear_acc(jck_engine* e, int step, hipStream_t st) {
  return clear_or_memset(e, e->ss.acc_clean_step, step, st, e->acc, (size_t)8 * e->acc_ld * sizeof(float));
}

// ---------------------------------------------------------------------------------------------------------
// phases
// ---------------------------------------------------------------------------------------------------------
// What every phase of one jck_engine_phase call works with: made once by phase_impl, read-only from there on
struct PhaseCtx {
  hipStream_t st, sA;                   // the caller's stream; the weight-gradient stream, or null
  const jck_step_inputs* in;            // the caller's inputs with the engine's own draws in place of z / alpha / masks left NULL ...
  const jck_step_inputs* given;         // ... and as the caller handed them over
  int B, HW;
  bool cg, lazy, lazy_tail;             // CGAN; JCK_PHASE_LAZY_JOIN as CGAN's phases / DCGAN's PHASE_D_LOSS_A take it
  bool par, ov_g, ov_gp;                // side streams in use; per-pass schedule: G forward beside D(real), penalty pass beside D(fake)
  DActs &DR, &D0, &D1;
};

static int penalty_pass(jck_engine* e, const PhaseCtx& c, DActs& D, hipStream_t s) {                 // :110-127, 178
  JCK_TRY(jck_interp(e->prec, e->real_noisy, e->fake, c.in->alpha, e->xhat, c.B, c.HW, s));
  JCK_TRY(d_forward(e, D, e->xhat, c.B, 2, c.in->drop_mask[2], s));
  JCK_TRY(d_head(e, D, c.B, 0.f, 1, -1, -1, s));
  // DCGAN's per-pass schedule runs this pass on its own stream beside D(fake): three-launch BatchNorm backward (DBackward),
  // whatever the stream layout of this call (a captured one-stream step stays launch for launch the eager one)
  DBackward bw;
  bw.gw = 0; bw.resident = c.cg; bw.xgrad = bw.gp_norm = true;
  return d_backward(e, D, e->xhat, c.B, c.in->drop_mask[2], s, bw);
}
static int g_forward_step(jck_engine* e, const PhaseCtx& c, hipStream_t s) {                         // :168-169
  return g_forward(e, c.in->z, c.in->labels, c.B, s, c.in->z == e->rz[c.in->step & 1] && e->ss.gz_step == (long long)c.in->step);
}

// The forward half of a batched D pass, both families: real batch, G's forward, the fake batch and the penalty's interpolate, D's
// conv stack on all three.
// pre: D(real)'s forward of this step has run already (PHASE_D_REAL_FWD)
// split: D(real)'s conv stack by itself and [fake | penalty] as one 2B forward behind G's; else one 3B forward behind G's
// direct (CGAN): the last layer writes the head's concat buffer (d_convs_forward: to_cbuf)
static int d_batched_forward(jck_engine* e, const PhaseCtx& c, bool pre, bool split, bool direct) {
  const DActs& S = e->bset;
  // D(real)'s forward needs nothing of G, and G's forward is a chain of small launches that leaves most of the chip idle: the
  // real batch's input transform and conv stack run on the weight-gradient stream (idle at the start of a step) beside it,
  // [fake | penalty] follow as one 2B forward - the split PHASE_D_REAL_FWD makes across steps; the arithmetic of the 3B forward
  // (a batch's BatchNorm statistics may be split into partial sums differently: summation order only)
  // (1.632 -> 1.609 ms; JCK_REAL_SIDE=0: one 3B forward behind G's)
  // (the split does not depend on the stream layout: a captured, one-stream step is the same arithmetic launch for launch)
  const bool beside = !pre && e->real_side && c.sA;
  const bool pre_side = pre && e->ss.pre_on_side;    // PHASE_D_REAL_FWD ran on the weight-gradient stream: joined behind G's forward
  e->ss.pre_on_side = false;
  hipStream_t sr = beside ? c.sA : c.st;
  if (beside) { HIPCHK(hipEventRecord(e->ev0, c.st)); HIPCHK(hipStreamWaitEvent(c.sA, e->ev0, 0)); }
  if (!pre) JCK_TRY(prep_real(e, c.in, c.B, sr));                                               // :160
  if (!pre && split) JCK_TRY(d_convs_forward(e, S.group(e, 0, 1), e->real_noisy, c.B, 0, sr, direct));      // :162
  if (beside) HIPCHK(hipEventRecord(e->evReal, c.sA));
  JCK_TRY(g_forward_step(e, c, c.st));
  if (beside || pre_side) HIPCHK(hipStreamWaitEvent(c.st, e->evReal, 0));
  JCK_TRY(e->mix_fake_noise_interp(c.in, c.B, c.st));                                             // :171, :111-113
  if (split) return d_convs_forward(e, S.group(e, 1, 2), e->fake, c.B, 0, c.st, direct);          // :173, 118 as one 2B forward
  return d_convs_forward(e, S, e->real_noisy, c.B, 0, c.st, direct);
}

// CGAN: the real, fake and penalty passes (:181-203) share D's weights -> their conv stacks run as ONE 3B pass with
// grouped BatchNorm.  The label / Linear / Dropout head runs per batch, forward and backward back to back, so the
// head buffers serve all three; the penalty group goes last and leaves them as its double backward (PHASE_D_GP)
// expects them.
// This is the pass from the conv stack's output on: the heads of the three groups, then the backward of the 3B set.
// head3: the head runs once over 3B rows (direct: its concat buffer is filled already)
static int cg_batched_heads_backward(jck_engine* e, const PhaseCtx& c, bool head3, bool direct) {
  const DActs& S = e->bset;
  const float tg[2] = {0.9f, 0.1f};
  const float *w2 = e->P(e->LD, e->dp, "linear2.weight"), *b2 = e->P(e->LD, e->dp, "linear2.bias");
  e->ss.head_row0 = 0;
  if (head3) {
    const bool fuse = e->head_fuse;
    const float tg3[3] = {tg[0], tg[1], 0.f};
    const int md3[3] = {0, 0, 1}, sl3[3] = {0, 1, -1}, sp3[3] = {3, 4, -1};
    JCK_TRY(cg_head_forward(e, direct ? nullptr : S.a[TT.NS - 1], 3 * c.B, c.in->drop_mask[0], c.st, c.B, !fuse));
    if (fuse) JCK_TRY(cg_head_middle(e, c.B, 3, tg3, md3, sl3, sp3, S.prob, S.ds, c.in->drop_mask[0], c.st));
    else JCK_TRY(jck_head_fwd_grouped(e->prec, e->h_drop, w2, b2, c.B, L1_OUT, 3, tg3, md3, S.prob, S.ds, e->acc, sl3, sp3, e->acc_ld, c.st));
    JCK_TRY(cg_head_backward_batched(e, S.ds, c.B, c.in->drop_mask[0], S.g[TT.NS - 1], c.st, e->head_side ? c.sA : nullptr, fuse));
    e->ss.head_row0 = 2 * c.B;                        // where PHASE_D_GP finds the penalty group's head state
    e->ss.head_wrow0 = 0;
  } else
    for (int g = 0; g < 3; ++g) {
      const bool pen = g == 2;
      const DActs Sg = S.group(e, g, 1);
      JCK_TRY(cg_head_forward(e, Sg.a[TT.NS - 1], c.B, c.in->drop_mask[g], c.st));
      JCK_TRY(jck_head_fwd(e->prec, e->h_drop, w2, b2, c.B, L1_OUT, pen ? 0.f : tg[g], pen ? 1 : 0, Sg.prob, Sg.ds, e->acc, pen ? -1 : g,
                           pen ? -1 : 3 + g, e->acc_ld, c.st));
      JCK_TRY(d_head_backward(e, e->dset[0], Sg.ds, c.B, !pen, c.in->drop_mask[g], Sg.g[TT.NS - 1], c.st));
    }
  DBackward bw;
  bw.gw = 2; bw.side = c.sA; bw.xgrad = bw.gp_norm = true; bw.lazy_join = c.lazy;
  JCK_TRY(d_convs_backward(e, S, e->real_noisy, c.B, c.st, bw));
  e->ss.gp_done = true;
  return JCK_OK;
}

// PHASE_D_LOSS of the batched schedule, both families; PHASE_D_LOSS_A / _B, its two halves (DCGAN)
static int phase_d_loss_batched(jck_engine* e, const PhaseCtx& c, int phase) {
  if (phase != JCK_PHASE_D_LOSS && (c.cg || e->batched != 3 || e->capturing || e->gp_bwd))
    JCK_FAIL(JCK_E_ARG, "PHASE_D_LOSS_A / _B: only with the batched DCGAN schedule, outside a capture, without JCK_ENGINE_GP_BACKWARD "
                        "(D's gradients are final only after PHASE_D_GP then)");
  // DCGAN: [real | fake | penalty] as one 3B pass after G's forward
  const float tg[2] = {0.9f, 0.1f};
  const int sl[2] = {0, 1}, sp[2] = {3, 4};
  if (phase == JCK_PHASE_D_LOSS_B) {            // second half of a split pass (after the early all-reduce has started)
    JCK_TRY(d_batched_pass(e, e->real_noisy, c.B, 3, tg, sl, sp, c.st, c.sA, 2));
    e->ss.gp_done = true;
    return JCK_OK;
  }
  if ((!c.in->real_nchw && !c.in->real_u8) || !c.in->z || !c.in->alpha) JCK_FAIL(JCK_E_ARG, "PHASE_D_LOSS needs real_nchw (or real_u8), z and alpha");
  // D(real)'s forward of this step may already have run under the previous step's G all-reduce (PHASE_D_REAL_FWD)
  const bool pre = !c.cg && e->ss.real_fwd_step == (long long)c.in->step;
  if (!c.cg) e->ss.real_fwd_step = -1;
  JCK_TRY(clear_acc(e, c.in->step, c.st));
  JCK_TRY(zero_d_grads(e, c.in->step, c.st));                                                   // D.zero_grad()  :155
  // the three dropout masks back to back (hipgan/engine.py hands them over that way): the head runs once over 3B rows
  const bool head3 = c.cg && c.in->drop_mask[0] && c.in->drop_mask[1] == c.in->drop_mask[0] + (size_t)c.B * L1_OUT &&
                     c.in->drop_mask[2] == c.in->drop_mask[0] + (size_t)2 * c.B * L1_OUT;
  const bool direct = head3 && e->cbuf_direct;
  // D(real)'s conv stack beside G's forward, [fake | penalty] as a 2B forward behind it (d_batched_forward)
  JCK_TRY(d_batched_forward(e, c, pre, pre || e->real_side, direct));
  if (c.cg) return cg_batched_heads_backward(e, c, head3, direct);
  const int part = phase == JCK_PHASE_D_LOSS_A ? 1 : 0;
  JCK_TRY(d_batched_pass(e, e->real_noisy, c.B, 3, tg, sl, sp, c.st, c.sA, part, c.lazy_tail));      // :162-176, 178
  if (part == 0) e->ss.gp_done = true;
  return JCK_OK;
}

// the per-pass schedule: PHASE_D_LOSS, or its two halves PHASE_D_REAL and PHASE_D_FAKE
static int phase_d_per_pass(jck_engine* e, const PhaseCtx& c, int phase) {
  if (phase != JCK_PHASE_D_FAKE) {              // ---- D on the real batch (:155-165); independent of G
    if (!c.in->real_nchw && !c.in->real_u8) JCK_FAIL(JCK_E_ARG, "PHASE_D_REAL needs real_nchw (or real_u8)");
    JCK_TRY(clear_acc(e, c.in->step, c.st));
    JCK_TRY(zero_d_grads(e, c.in->step, c.st));                                                 // D.zero_grad()  :155
  }
  hipStream_t sG = c.st;
  if (phase == JCK_PHASE_D_LOSS || phase == JCK_PHASE_D_FAKE) {   // G forward: beside D(real) when both are in this call
    if (!c.in->z) JCK_FAIL(JCK_E_ARG, "G forward needs z");
    if (c.ov_gp && !c.in->alpha) JCK_FAIL(JCK_E_ARG, "alpha is needed here (the penalty pass starts inside this phase)");
    if (c.ov_g) { HIPCHK(hipEventRecord(e->ev0, c.st)); HIPCHK(hipStreamWaitEvent(e->sB, e->ev0, 0)); sG = e->sB; }
    JCK_TRY(g_forward_step(e, c, sG));
    JCK_TRY(e->mix_fake_noise(c.in, c.B, sG));   // :171
    if (c.ov_g) HIPCHK(hipEventRecord(e->evF, sG));
  }
  if (phase != JCK_PHASE_D_FAKE) {
    JCK_TRY(prep_real(e, c.in, c.B, c.st));   // :160
    if (c.ov_gp && phase == JCK_PHASE_D_LOSS) HIPCHK(hipEventRecord(e->evReal, c.st));           // penalty pass needs only this
    JCK_TRY(d_forward(e, c.DR, e->real_noisy, c.B, 0, c.in->drop_mask[0], c.st));                      // :162
    JCK_TRY(d_head(e, c.DR, c.B, 0.9f, 0, 0, 3, c.st));                                             // :163,165
    // D(real)'s weight gradients stay in flight on sA while D(fake) starts (own activation set); D(fake)'s backward
    // queues behind them on sA and joins.  PHASE_D_REAL alone (pipeline mode) and CGAN (shared set) join here.
    DBackward bw;
    bw.side = c.sA; bw.join = phase == JCK_PHASE_D_REAL || c.cg || !e->defer_join;
    JCK_TRY(d_backward(e, c.DR, e->real_noisy, c.B, c.in->drop_mask[0], c.st, bw));                   // :164 (cgan :203)
    if (phase == JCK_PHASE_D_REAL) return JCK_OK;
  }
  // ---- D on the fake batch (:170-176) with the penalty pass (:178) beside it
  if (c.ov_g) HIPCHK(hipStreamWaitEvent(c.st, e->evF, 0));
  if (c.ov_gp) {                                   // penalty pass on its own stream and activation set
    if (phase == JCK_PHASE_D_FAKE) HIPCHK(hipEventRecord(e->evReal, c.st));    // real_noisy came from an earlier call on st
    HIPCHK(hipStreamWaitEvent(e->sC, e->evF, 0));
    HIPCHK(hipStreamWaitEvent(e->sC, e->evReal, 0));
    JCK_TRY(penalty_pass(e, c, c.D1, e->sC));
    HIPCHK(hipEventRecord(e->evGP, e->sC));
    e->ss.gp_inflight = true;
  }
  JCK_TRY(d_forward(e, c.D0, e->fake, c.B, 1, c.in->drop_mask[1], c.st));                             // :173
  JCK_TRY(d_head(e, c.D0, c.B, 0.1f, 0, 1, 4, c.st));                                               // :174,176
  DBackward bw;
  bw.side = c.sA;
  return d_backward(e, c.D0, e->fake, c.B, c.in->drop_mask[1], c.st, bw);                             // :175
}

// forward half of D(real) of step in->step, ahead of its PHASE_D_LOSS: touches only real_noisy and group 0 of the batched
// set (activations, statistic slots, scale/shift table) and the BatchNorm record of (parity of in->step, pass 0) - nothing
// the G phase of the step before it reads or writes
static int phase_d_real_fwd(jck_engine* e, const PhaseCtx& c) {
  if (c.cg || e->batched != 3 || e->capturing) JCK_FAIL(JCK_E_ARG, "PHASE_D_REAL_FWD: only with the batched DCGAN schedule, outside a capture");
  if (!c.in->real_nchw && !c.in->real_u8) JCK_FAIL(JCK_E_ARG, "PHASE_D_REAL_FWD needs real_nchw (or real_u8)");
  // on the weight-gradient stream when there is one (idle here: G's backward has joined it): the caller's stream then only
  // carries the wait for G's all-reduce and Adam(G), and the rest of this forward runs beside the next step's G forward
  hipStream_t sr = (e->real_side && c.sA) ? c.sA : c.st;
  if (sr != c.st) { HIPCHK(hipEventRecord(e->ev0, c.st)); HIPCHK(hipStreamWaitEvent(sr, e->ev0, 0)); }
  JCK_TRY(prep_real(e, c.in, c.B, sr));                                                         // :160
  JCK_TRY(d_convs_forward(e, e->bset.group(e, 0, 1), e->real_noisy, c.B, 0, sr));             // :162
  if (sr != c.st) HIPCHK(hipEventRecord(e->evReal, sr));
  e->ss.pre_on_side = sr != c.st;
  e->ss.real_fwd_step = c.in->step;
  return JCK_OK;
}

// A PHASE_D_REAL_FWD already enqueued for the next step is abandoned: `st` waits for it where it ran on the weight-gradient stream
// (it may still be reading D's packed operands and writing real_noisy there), and the next D phase computes D(real) itself.
static int drop_prefetch(jck_engine* e, hipStream_t st) {
  if (e->ss.real_fwd_step >= 0 && e->ss.pre_on_side && e->evReal) HIPCHK(hipStreamWaitEvent(st, e->evReal, 0));
  e->ss.real_fwd_step = -1;
  e->ss.pre_on_side = false;
  return JCK_OK;
}

// The stand-alone gradient penalty of the module path (train/dcgan_trainer.py:110-127, train/cgan_trainer.py:114-131 called
// outside this engine's step): real_nchw = real_data, noise_real = fake_data - both [B,3,S,S] fp32, taken as they are -, alpha
// (CGAN: labels, drop_mask[2]).  Leaves the per-image gradient norms in "norms" (the caller forms mean((n - 1)^2)) and, CGAN
// and DCGAN with JCK_ENGINE_GP_BACKWARD, d(penalty)/d(theta_D) with lambda = 1 in D's gradient arena, which is cleared first: the
// double backward in closed form.
static int phase_gp_only(jck_engine* e, const PhaseCtx& c) {
  if (!c.in->real_nchw || !c.in->noise_real || !c.given->alpha) JCK_FAIL(JCK_E_ARG, "PHASE_GP_ONLY needs real_nchw (real), noise_real (fake) and alpha");
  if (e->capturing) JCK_FAIL(JCK_E_ARG, "PHASE_GP_ONLY: not inside a capture");
  if (c.cg && !c.given->drop_mask[2]) JCK_FAIL(JCK_E_ARG, "PHASE_GP_ONLY (CGAN) needs drop_mask[2]");
  // a D(real) forward enqueued ahead of the next step owns real_noisy (and may still be writing it on the weight-gradient stream):
  // it is abandoned before the first write here, and that step's D phase computes D(real) itself
  JCK_TRY(drop_prefetch(e, c.st));
  HIPCHK(hipMemsetAsync(e->acc, 0, (size_t)8 * e->acc_ld * sizeof(float), c.st));
  HIPCHK(hipMemsetAsync(e->dg, 0, e->LD.n_params * sizeof(float), c.st));
  if (c.cg) HIPCHK(hipMemsetAsync(e->gw1p, 0, (size_t)L1_OUT * L1_KPAD * sizeof(float), c.st));
  e->ss.begin_gp_only();
  JCK_TRY(jck_img_prep(e->prec, c.in->real_nchw, nullptr, 1.0f, 0.0f, e->real_noisy, c.B, c.HW, c.st));
  JCK_TRY(jck_img_prep(e->prec, c.in->noise_real, nullptr, 1.0f, 0.0f, e->fake, c.B, c.HW, c.st));
  JCK_TRY(penalty_pass(e, c, c.D0, c.st));
  if (c.cg || e->gp_bwd) JCK_TRY(gp_double_backward(e, c.D0, e->xhat, c.B, 1.0f, c.in->drop_mask[2], c.st, nullptr));
  return JCK_OK;
}

static int phase_d_gp(jck_engine* e, const PhaseCtx& c) {
  if (!c.in->alpha) JCK_FAIL(JCK_E_ARG, "PHASE_D_GP needs alpha");
  if (e->ss.gp_done && (c.cg || e->gp_bwd)) {          // forward and first backward ran as group 2 of the batched pass
    e->ss.gp_done = false;
    JCK_TRY(gp_double_backward(e, e->bset.group(e, 2, 1), e->xhat, c.B, 10.0f, c.in->drop_mask[2], c.st, c.sA, c.lazy));
    if (!(c.lazy && c.sA)) e->ss.join_pending = e->ss.mid_recorded = false;      // it joined the stream itself
    e->ss.head_row0 = 0;
    return JCK_OK;
  }
  if (e->ss.gp_done) { e->ss.gp_done = false; return JCK_OK; }    // computed inside the batched pass of PHASE_D_LOSS
  if (e->ss.gp_inflight) {                           // started in PHASE_D_LOSS: join (JCK_ENGINE_GP_BACKWARD: and back-propagate it)
    HIPCHK(hipStreamWaitEvent(c.st, e->evGP, 0));
    e->ss.gp_inflight = false;
    if (e->gp_bwd) JCK_TRY(gp_double_backward(e, c.D1, e->xhat, c.B, 10.0f, nullptr, c.st, c.sA));
    return JCK_OK;
  }
  JCK_TRY(penalty_pass(e, c, c.D0, c.st));
  // CGAN back-propagates the penalty (train/cgan_trainer.py:200-203); DCGAN when created with JCK_ENGINE_GP_BACKWARD
  if (c.cg || e->gp_bwd) JCK_TRY(gp_double_backward(e, c.D0, e->xhat, c.B, 10.0f, c.in->drop_mask[2], c.st, c.sA));
  return JCK_OK;
}

static int phase_d_step(jck_engine* e, const PhaseCtx& c) {                                       // :180
  if (e->ss.gp_inflight || (e->gp_bwd && e->ss.gp_done)) JCK_FAIL(JCK_E_ARG, "PHASE_D_GP must be called before PHASE_D_STEP");
  if (!e->hp_holds(c.in->step, c.in->lr) && !e->capturing) JCK_TRY(refresh_adam_scalars(e, c.in->step, c.in->lr, c.st));   // (eager callers)
  const float* hp = e->hp2 + 8 * e->parity;
  // G.zero_grad() (:182) rides on D's Adam launch: G's gradient arena is dead between G's optimiser step and PHASE_G_LOSS
  float* zg = (e->fold_zero && !e->capturing && e->LG.n_params % 4 == 0) ? e->gg : nullptr;
  if (zg) e->ss.gg_clean_step = c.in->step;
  if (e->ss.join_pending) {
    // the weight-gradient stream is still on its last products: Adam and the Linear repack for everything behind the bottom
    // conv weight in the arena now, [label embedding | conv1.weight] and the conv repack once that stream is through
    const TensorInfo* c1 = find(e->LD, CWN[0]);
    const long long cut = c1->offset + c1->numel;
    HIPCHK(hipStreamWaitEvent(c.st, e->ss.mid_recorded ? e->evWmid : e->evWdone, 0));
    if (e->adam_pack) JCK_TRY(adam_repack_net(e, 1, cut, e->LD.n_params - cut, c.in->grad_scale, hp, c.st, zg));      // each range packs what it updates
    else JCK_TRY(adam_net(e, 1, cut, e->LD.n_params - cut, c.in->grad_scale, hp, c.st, zg));
    JCK_TRY(repack_linear(e, c.st));
    if (e->ss.mid_recorded) HIPCHK(hipStreamWaitEvent(c.st, e->evWdone, 0));
    e->ss.join_pending = e->ss.mid_recorded = false;
    return adam_repack_net(e, 1, 0, cut, c.in->grad_scale, hp, c.st);
  }
  JCK_TRY(adam_repack_net(e, 1, 0, e->LD.n_params, c.in->grad_scale, hp, c.st, zg));
  return e->family == 1 ? repack_linear(e, c.st) : JCK_OK;
}

static int phase_g_loss(jck_engine* e, const PhaseCtx& c) {                                       // :182-188
  JCK_TRY(clear_or_memset(e, e->ss.gg_clean_step, c.in->step, c.st, e->gg, e->LG.n_params * sizeof(float)));
  const bool fuse = e->head_fuse;                 // CGAN: the middle of the head as one launch (cg_head_middle); DCGAN: conv5's forward
                                                  // writes its input gradient too
  JCK_TRY(d_forward(e, c.D0, e->fake, c.B, 3, c.in->drop_mask[3], c.st, !fuse));
  if (fuse && !c.cg) JCK_TRY(d_head(e, c.D0, c.B, 0.9f, 0, 2, 5, c.st, c.D0.g[TT.NS - 1]));
  else if (fuse) {
    const float tg1 = 0.9f;
    const int md1 = 0, sl1 = 2, sp1 = 5;
    JCK_TRY(cg_head_middle(e, c.B, 1, &tg1, &md1, &sl1, &sp1, c.D0.prob, c.D0.ds, c.in->drop_mask[3], c.st));
  } else JCK_TRY(d_head(e, c.D0, c.B, 0.9f, 0, 2, 5, c.st));
  // D's own weight gradients from this pass are dead (zeroed at :155 before they are read): skipped
  XgradEpi xe = {e->fake_raw, 0.9f, e->g_raw, (c.sA && e->ext_events) ? e->evW[TT.NS - 1] : nullptr, false};
  DBackward bw;
  bw.gw = 0; bw.xgrad = true; bw.xe = e->fuse_tanh ? &xe : nullptr;
  JCK_TRY(d_backward(e, c.D0, e->fake, c.B, c.in->drop_mask[3], c.st, bw, fuse));
  return g_backward(e, c.D0.gx, c.B, c.st, c.sA, xe.fused);
}

static int phase_g_step(jck_engine* e, const PhaseCtx& c) {                                       // :189
  if (!e->hp_holds(c.in->step, c.in->lr) && !e->capturing) JCK_TRY(refresh_adam_scalars(e, c.in->step, c.in->lr, c.st));
  // Adam(G) with the moving average of G's weights, when one is bound (its weight is hp[2] of the step), G's repack, the four D
  // passes' BatchNorm records in the reference's order and the logged scalars: one launch
  TailJobs t = {};
  for (int i = 0; i < TT.NS; ++i) {
    const int cs = TT.D_CS[i];
    t.l[i].rec = e->d_rs[i] + (size_t)e->parity * 4 * 2 * cs;
    t.l[i].rm = e->dbn + find(e->LD, RMN[i])->offset;
    t.l[i].rv = e->dbn + find(e->LD, RVN[i])->offset;
    t.l[i].nbt = (long long*)(e->dnbt + i);
    t.l[i].C = cs;
  }
  t.nl = TT.NS; t.npass = 4; t.momentum = BN_MOM; t.acc = e->acc; t.acc_ld = e->acc_ld; t.B = c.B; t.invB = 1.0f / (float)c.B; t.lambda_gp = 10.0f; t.out = e->scal_out;
  return adam_repack_net(e, 0, 0, e->LG.n_params, c.in->grad_scale, e->hp2 + 8 * e->parity, c.st, nullptr, e->gema, &t, cdiv(TT.G_C1, 256));
}

// What every phase call does first, in this order: the engine's own draws for inputs left NULL, the wait for a join left open,
// the labels, the step's parity and its scalars
static int phase_begin(jck_engine* e, int phase, jck_step_inputs& loc, hipStream_t st) {
  const bool cg = e->family == 1;
  // z, alpha and (CGAN) the Dropout keep masks left NULL: the engine's own draws for this step (jck_engine_set_step)
  const int q = loc.step & 1;
  if (!loc.z) loc.z = e->rz[q];
  if (!loc.alpha) loc.alpha = e->ralpha[q];
  if (cg && !loc.drop_mask[0] && !loc.drop_mask[1] && !loc.drop_mask[2] && !loc.drop_mask[3])
    for (int i = 0; i < 4; ++i) loc.drop_mask[i] = e->rmask[q] + (size_t)i * e->B * L1_OUT;
  // a join left open by the phase before (JCK_PHASE_LAZY_JOIN): the penalty's double backward keeps using the weight-gradient
  // stream in order and the optimiser phase closes it tensor by tensor; anything else waits here
  if (e->ss.join_pending && !(phase == JCK_PHASE_D_STEP || (phase == JCK_PHASE_D_GP && cg && e->ss.gp_done))) {
    HIPCHK(hipStreamWaitEvent(st, e->evWdone, 0));
    e->ss.join_pending = e->ss.mid_recorded = false;
  }
  if (cg) {
    if (!loc.labels) JCK_FAIL(JCK_E_ARG, "CGAN phases need labels");
    e->cur_labels = loc.labels;
  }
  e->parity = q;
  // eager callers that did not call jck_engine_set_step: the step's scalars / Philox words are written by its first phase
  // (a phase called with another learning rate than the step's earlier phases - separate G and D rates - rewrites the Adam
  // scalars only: the step's accumulator rows and random inputs are live)
  if (!e->capturing) {
    // (PHASE_D_REAL_FWD ahead of its step: D's gradients of the step before were consumed by its PHASE_D_STEP, and nothing writes
    // them until this step's D pass - the set-step launch clears them here as well, instead of a memset in front of that pass)
    const int ph = phase & 0xff;
    const bool zero_d = ph == JCK_PHASE_D_LOSS || ph == JCK_PHASE_D_LOSS_A || ph == JCK_PHASE_D_REAL || ph == JCK_PHASE_D_REAL_FWD;
    if (e->hp_step[q] != loc.step) JCK_TRY(set_step_impl(e, loc.step, loc.lr, st, zero_d));
    else if (e->hp_lr[q] != loc.lr) JCK_TRY(refresh_adam_scalars(e, loc.step, loc.lr, st));
  }
  e->acc = e->acc2 + (size_t)8 * e->acc_ld * e->parity;
  e->scal_out = e->scal2 + 8 * e->parity;
  return JCK_OK;
}
static int phase_impl(jck_engine* e, int phase, const jck_step_inputs* in_, void* stream) {
  if (!e || !e->bound || !in_) JCK_FAIL(JCK_E_ARG, "engine not bound / null inputs");
  hipStream_t st = (hipStream_t)stream;
  const bool cg = e->family == 1;
  const bool lazy = (phase & JCK_PHASE_LAZY_JOIN) && cg && !e->capturing;
  const bool lazy_tail = (phase & JCK_PHASE_LAZY_JOIN) && !cg && (phase & 0xff) == JCK_PHASE_D_LOSS_A;
  phase &= ~JCK_PHASE_LAZY_JOIN;
  jck_step_inputs loc = *in_;
  JCK_TRY(phase_begin(e, phase, loc, st));
  // stream overlap (DCGAN): A = wgrads, B = G forward beside D(real), C = penalty pass beside D(fake).  CGAN keeps the penalty
  // on the main stream (it produces gradients and shares the head buffers).
  // weight gradients beside the dgrad chain on a second stream: +8 % for DCGAN in round 1, +1.5 % now; CGAN +1.4 % (2.886 vs
  // 2.929 ms eager, round 3).  JCK_WGRAD_SIDE=0 keeps them on the main stream.  A captured step keeps everything on one stream
  // either way (below).
  // Under a stream capture everything stays on the capturing stream: a hipGraph with parallel branches makes the ROCm 7.2
  // runtime keep per-graph side streams, costs ~7 us of host time per node at launch, ran slower than the linear graph for
  // CGAN, and its hipGraphLaunch reads past the end of the graph's stream pool whenever two of those streams share the launch
  // stream's hardware queue (hip::Graph::UpdateStreams; cause and frame in DESIGN.md section 5.6; jck_engine_capture_end refuses
  // any non-linear graph).  Same kernels, same order per stream as the eager schedule - bitwise the same results.
  const bool par = e->overlap && !e->capturing;
  // D(real) (DR): own set so it may run beside the previous step's G phase
  const PhaseCtx c = {st, (par && e->wgrad_side) ? e->sA : nullptr, &loc, in_, e->B, TT.HW, cg, lazy, lazy_tail, par, par, par && !cg,
                      cg ? e->dset[0] : e->dset[2], e->dset[0], e->dset[1]};
  switch (phase) {
    case JCK_PHASE_D_LOSS_A: case JCK_PHASE_D_LOSS_B: return phase_d_loss_batched(e, c, phase);
    case JCK_PHASE_D_LOSS: return e->batched ? phase_d_loss_batched(e, c, phase) : phase_d_per_pass(e, c, phase);
    case JCK_PHASE_D_REAL: case JCK_PHASE_D_FAKE: return phase_d_per_pass(e, c, phase);
    case JCK_PHASE_D_REAL_FWD: return phase_d_real_fwd(e, c);
    case JCK_PHASE_GP_ONLY: return phase_gp_only(e, c);
    case JCK_PHASE_D_GP: return phase_d_gp(e, c);
    case JCK_PHASE_D_STEP: return phase_d_step(e, c);
    case JCK_PHASE_G_LOSS: return phase_g_loss(e, c);
    case JCK_PHASE_G_STEP: return phase_g_step(e, c);
  }
  JCK_FAIL(JCK_E_ARG, "unknown phase");
}
extern "C" int jck_engine_phase(jck_engine* e, int phase, const jck_step_inputs* in_, void* stream) {
  // JCK_PHASE_NO_RESIDENT: no grid-barrier launch in this call (a collective may be holding CUs: include/jckgan.h)
  const bool keep_res = e ? e->bn_res : false;
  if (e && (phase & JCK_PHASE_NO_RESIDENT)) e->bn_res = false;
  const int rc = phase_impl(e, phase & ~JCK_PHASE_NO_RESIDENT, in_, stream);
  if (e) e->bn_res = keep_res;
  if (rc != JCK_OK && e) {
    if (e->ss.join_pending && e->sA && stream && !e->capturing) (void)hipStreamWaitEvent((hipStream_t)stream, e->evWdone, 0);
    e->ss.drop_promises();
  }
  return rc;
}

// Per-step optimiser scalars (Adam bias corrections of step `step` at learning rate `lr`, computed on the host in double as
// torch.optim.Adam does) -> device memory of parity step & 1.  Call once per step BEFORE its phases when the phases are
// replayed from a captured graph (the graph bakes every kernel argument); eager callers may skip it - the optimiser phases
// then write the scalars themselves.
// zero_d: the caller is the step's first D-loss phase - the same launch clears D's gradient arena (D.zero_grad(), :155)
static int set_step_impl(jck_engine* e, int step, float lr, void* stream, bool zero_d) {
  if (!e || !e->bound) JCK_FAIL(JCK_E_ARG, "engine not bound");
  if (e->capturing) JCK_FAIL(JCK_E_ARG, "set_step inside a graph capture would bake one step's scalars into the graph");
  const int q = step & 1;
  zero_d = zero_d && e->fold_zero && e->LD.n_params % 4 == 0;
  JCK_TRY(jck_adam_set_step(e->hp2 + 8 * q, (double)lr, ADAM_B1, ADAM_B2, step, e->noise_seed, e->ema_w(step), (hipStream_t)stream, e->rz[q], (long long)e->B * 100,
                            e->ralpha[q], e->B, e->rmask[q], e->rmask[q] ? (long long)4 * e->B * L1_OUT : 0, 0.75f,
                            e->acc2 + (size_t)8 * e->acc_ld * q, (long long)8 * e->acc_ld,
                            zero_d ? e->dg : nullptr, e->LD.n_params, zero_d && e->family == 1 ? e->gw1p : nullptr, (long long)L1_OUT * L1_KPAD,
                            // DCGAN: the drawn z goes straight into G.conv1's operand rows too (no pad_rows launch in front of G's forward
                            // when the step uses the engine's own z)
                            e->family == 0 && e->fold_zero ? e->g_z : nullptr, 100, z_pad(e->family), prec_f32_storage(e->prec) ? 1 : 0));
  e->ss.gz_step = (e->family == 0 && e->fold_zero) ? step : -1;
  if (zero_d) e->ss.dg_clean_step = step;
  e->ss.acc_clean_step = step;
  e->hp_step[step & 1] = step;
  e->hp_lr[step & 1] = lr;
  return JCK_OK;
}
extern "C" int jck_engine_set_step(jck_engine* e, int step, float lr, void* stream) { return set_step_impl(e, step, lr, stream, false); }
// Exponential moving average of G's weights (the averaged generator a GAN trainer samples, scores and ships; the reference has
// none).  bind: `g_ema` = LG.n_params floats, 16-byte aligned, NULL detaches; PHASE_G_STEP's Adam launch then advances it.  set:
// the weight of step s is 1 for s < start_step and (float)(1 - decay) from there on; it travels in the step's hp block.
extern "C" int jck_engine_bind_ema(jck_engine* e, float* g_ema) {
  if (!e || !e->bound) JCK_FAIL(JCK_E_ARG, "engine not bound");
  if (e->capturing) JCK_FAIL(JCK_E_ARG, "bind_ema inside a graph capture");
  if ((uintptr_t)g_ema & 15) JCK_FAIL(JCK_E_ARG, "bind_ema: the EMA arena must be 16-byte aligned");
  e->gema = g_ema;
  e->hp_step[0] = e->hp_step[1] = 0;      // the next step rewrites the device copy of its scalars (the weight slot among them)
  e->hp_lr[0] = e->hp_lr[1] = -1.f;
  return JCK_OK;
}
extern "C" int jck_engine_set_ema(jck_engine* e, double decay, int start_step) {
  if (!e) JCK_FAIL(JCK_E_ARG, "null engine");
  if (!(decay >= 0.0 && decay <= 1.0)) JCK_FAIL(JCK_E_ARG, "set_ema: decay must lie in [0, 1]");
  e->ema_decay = decay; e->ema_start = start_step;
  e->hp_step[0] = e->hp_step[1] = 0;
  e->hp_lr[0] = e->hp_lr[1] = -1.f;
  return JCK_OK;
}
// Seed of the in-kernel instance noise (steps whose jck_step_inputs carry no noise tensors draw 0.1*N(0,1) inside the image
// kernels: Philox4x32-10 keyed by this seed, counter = pixel | tensor | optimiser step).  Data-parallel ranks pass seed + rank.
extern "C" int jck_engine_set_noise_seed(jck_engine* e, unsigned long long seed) {
  if (!e) JCK_FAIL(JCK_E_ARG, "null engine");
  e->noise_seed = seed;
  e->hp_step[0] = e->hp_step[1] = 0;      // the next step rewrites the device copy
  e->hp_lr[0] = e->hp_lr[1] = -1.f;
  return JCK_OK;
}

// hipGraph capture of phases: begin -> jck_engine_phase(...) x n on the same stream -> end gives an executable graph that
// replays exactly those launches (incl. the side-stream forks and joins, which become graph dependencies).  Everything a
// phase reads through jck_step_inputs pointers is baked: the caller keeps those buffers at fixed addresses, refreshes
// their contents before each launch, keeps one graph per step parity (scalar / BatchNorm-record buffers alternate) and
// calls jck_engine_set_step first.  `stream` must not be the legacy default stream.
extern "C" int jck_engine_capture_begin(jck_engine* e, void* stream) {
  if (!e || !e->bound) JCK_FAIL(JCK_E_ARG, "engine not bound");
  if (!stream) JCK_FAIL(JCK_E_ARG, "cannot capture on the default stream");
  if (jck_prof_is_on()) JCK_FAIL(JCK_E_ARG, "per-launch profiling (jck_prof_enable) records timing events: not capturable");
  // relaxed: a call that is "unsafe" during a capture (a free, a stream destroy from a garbage-collected object, ...) issued
  // by this thread must not invalidate the graph being captured
  HIPCHK(hipStreamBeginCapture((hipStream_t)stream, hipStreamCaptureModeRelaxed));
  e->capturing = true;
  return JCK_OK;
}
extern "C" int jck_engine_capture_end(jck_engine* e, void* stream, void** graph_exec) {
  if (!e || !graph_exec) JCK_FAIL(JCK_E_ARG, "null argument");
  e->capturing = false;
  hipGraph_t g = nullptr;
  HIPCHK(hipStreamEndCapture((hipStream_t)stream, &g));
  // Only LINEAR graphs are instantiated (every node at most one successor, one root).  ROCm 7.2's hip::GraphExec creates
  // max_streams_ internal streams for a graph with parallel branches and hip::Graph::UpdateStreams (called by every
  // hipGraphLaunch of such a graph) skips each of them that shares the launch stream's HARDWARE queue - with no bound on the
  // index: when two or more of the internal streams sit on the launch stream's queue (streams are dealt onto a small pool of
  // hardware queues, so this depends on every stream the process ever created) it reads past the end of the vector and
  // dereferences garbage - the SIGSEGV of round 2.  A graph whose width is 1 never enters that code.
  {
    size_t nn = 0, ne = 0;
    hipError_t q = hipGraphGetNodes(g, nullptr, &nn);
    if (q == hipSuccess) q = hipGraphGetEdges(g, nullptr, nullptr, &ne);
    bool linear = q == hipSuccess && nn > 0 && ne == nn - 1;
    e->graph_nodes = (int)nn;
    if (linear && ne > 0) {
      std::vector<hipGraphNode_t> from(ne), to(ne);
      q = hipGraphGetEdges(g, from.data(), to.data(), &ne);
      linear = q == hipSuccess;
      for (size_t i = 0; linear && i < ne; ++i)
        for (size_t k = i + 1; k < ne; ++k)
          if (from[i] == from[k] || to[i] == to[k]) { linear = false; break; }       // a fork or a join
    }
    if (!linear) {
      (void)hipGraphDestroy(g);
      JCK_FAIL(JCK_E_ARG, "captured graph has parallel branches (" + std::to_string(nn) + " nodes, " + std::to_string(ne) +
                              " edges): not instantiated on this runtime - see DESIGN.md section 5.6");
    }
  }
  hipGraphExec_t ge = nullptr;
  hipError_t rc = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (rc != hipSuccess) JCK_FAIL(JCK_E_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(rc));
  *graph_exec = ge;
  return JCK_OK;
}
// abandon a capture after a failed phase (the stream leaves capture mode; nothing was executed)
extern "C" int jck_engine_capture_abort(jck_engine* e, void* stream) {
  if (e) e->capturing = false;
  hipGraph_t g = nullptr;
  (void)hipStreamEndCapture((hipStream_t)stream, &g);
  if (g) (void)hipGraphDestroy(g);
  (void)hipGetLastError();
  // side streams that joined the broken capture may be left invalidated: replace them
  // ... and so may the events recorded inside it
  if (e && e->overlap) {
    destroy_side_streams(e, false);
    JCK_TRY(create_side_streams(e));
    e->ss.gp_inflight = false;
    e->ss.join_pending = e->ss.mid_recorded = false;
    (void)hipGetLastError();
  }
  return JCK_OK;
}
// nodes (kernel launches and memsets) of the graph the last jck_engine_capture_end of this engine instantiated: the launch count
// of the captured phases
extern "C" int jck_engine_graph_nodes(const jck_engine* e) { return e ? e->graph_nodes : 0; }
extern "C" int jck_graph_launch(void* graph_exec, void* stream) {
  if (!graph_exec) JCK_FAIL(JCK_E_ARG, "null graph");
  HIPCHK(hipGraphLaunch((hipGraphExec_t)graph_exec, (hipStream_t)stream));
  return JCK_OK;
}
extern "C" void jck_graph_destroy(void* graph_exec) {
  if (graph_exec) (void)hipGraphExecDestroy((hipGraphExec_t)graph_exec);
}

// Makes `stream` wait until the tail of D's gradient arena that PHASE_D_LOSS_A finalises is complete (its last writers: the
// BatchNorm backward of the top layer on the phase's stream, the top layer's weight gradient and conv5's on the weight-gradient
// stream).  For a caller that passed JCK_PHASE_LAZY_JOIN with PHASE_D_LOSS_A and starts the tail's all-reduce from `stream`.
extern "C" int jck_engine_order_after_tail(jck_engine* e, void* stream) {
  if (!e || !e->bound || !stream) JCK_FAIL(JCK_E_ARG, "engine not bound / null stream");
  if (!e->evTail) return JCK_OK;                    // no second stream: the tail is final in the phase's stream order
  if (e->ss.tail_on_side) HIPCHK(hipStreamWaitEvent((hipStream_t)stream, e->evW[e->T.NS - 1], 0));
  HIPCHK(hipStreamWaitEvent((hipStream_t)stream, e->evTail, 0));
  return JCK_OK;
}
// drop_prefetch for a caller whose weights are about to change (a re-broadcast of the replica guard, load_model, another engine's
// step on the same arenas): `stream`, the one the change is made on - NULL is the default stream, which waits like any other.
extern "C" int jck_engine_drop_prefetch(jck_engine* e, void* stream) {
  if (!e || !e->bound) JCK_FAIL(JCK_E_ARG, "engine not bound");
  return drop_prefetch(e, (hipStream_t)stream);
}
extern "C" long long jck_engine_grad_tail(const jck_engine* e, int net) {
  if (!e || !e->bound || net != 1 || e->family != 0 || e->batched != 3 || e->gp_bwd) return -1;
  return (long long)find(e->LD, CWN[e->T.NS - 1])->offset;
}

// Call after a device synchronisation (e.g. when the step scalars are read): a grid barrier of a resident launch that timed out -
// its workgroups were not all resident, which happens when another process or stream fills the same GPU - leaves invalid
// results; the error is reported here, the barrier state re-armed.
extern "C" int jck_engine_check(jck_engine* e) {
  if (!e || !e->bound || !e->gsync) return JCK_OK;
  if (!jck_grid_sync_error(e->gsync)) return JCK_OK;
  HIPCHK(hipMemset(e->gsync, 0, jck_grid_sync_bytes()));
  JCK_FAIL(JCK_E_HIP, "a grid barrier of the resident BatchNorm backward timed out: the launch needs every CU of the device to itself "
                      "(another process or stream on this GPU?); the step's results are invalid - set JCK_BN_RES=0 to use the three-launch form");
}
extern "C" const float* jck_engine_scalars(const jck_engine* e) { return e ? e->scal_out : nullptr; }
extern "C" const float* jck_engine_scalars_at(const jck_engine* e, int step) { return e ? e->scal2 + 8 * (step & 1) : nullptr; }

extern "C" const void* jck_engine_tensor(const jck_engine* e, const char* name, long long* numel) {
  if (!e || !e->bound || !name) return nullptr;
  const long long img = (long long)e->B * TT.HW * 4;
  const DActs& D = e->dset[0];
  struct { const char* n; const void* p; long long c; } tab[] = {
      {"fake", e->fake, img}, {"fake_raw", e->fake_raw, img}, {"real_noisy", e->real_noisy, img}, {"xhat", e->xhat, img},
      {"d_gx", D.gx, img}, {"prob", D.prob, e->B}, {"ds", D.ds, e->B}, {"norms", D.norms, e->B}, {"acc", e->acc, (long long)8 * e->acc_ld},
      {"d_y1", D.y[0], (long long)e->B * (TT.S / 2) * (TT.S / 2) * 64}, {"d_a4", D.a[TT.NS - 1], (long long)e->B * TT.FEAT},
      {"g_y1", e->g_y[0], (long long)e->B * TT.FEAT}, {"g_a4", e->g_a[TT.NS - 1], (long long)e->B * (TT.S / 2) * (TT.S / 2) * 64}};
  for (auto& t : tab)
    if (!strcmp(t.n, name)) { if (numel) *numel = t.c; return t.p; }
  // the packed GEMM operands, with the element counts carve() allocates (padding included): "d_down0", "g_up3", ...
  auto hit = [&](const void* p, long long c) { if (numel) *numel = c; return p; };
  for (int i = 0; i < TT.NS; ++i) {
    const long long d_dn = (long long)jck_pad_rows(TT.D_CS[i]) * 16 * jck_pad_chan(TT.D_CB[i]), d_up = 4ll * jck_pad_rows(TT.D_CB[i]) * 4 * TT.D_CS[i];
    const long long g_dn = (long long)jck_pad_rows(TT.G_CS[i]) * 16 * jck_pad_chan(TT.G_CB[i]), g_up = 4ll * jck_pad_rows(TT.G_CB[i]) * 4 * TT.G_CS[i];
    const struct { const char* pre; const void* p; long long c; } ops[] = {
        {"d_down", e->d_down[i], d_dn}, {"d_up", e->d_up[i], d_up}, {"g_up", e->g_up[i], g_up}, {"g_down", e->g_down[i], g_dn}};
    for (auto& o : ops) {
      const size_t l = strlen(o.pre);
      if (!strncmp(name, o.pre, l) && name[l] == (char)('0' + i) && name[l + 1] == '\0') return hit(o.p, o.c);
    }
  }
  if (!strcmp(name, "d_head_wp")) return hit(e->d_head_wp, TT.FEAT);
  if (!strcmp(name, "g1_w")) return hit(e->g1_w, 16ll * TT.G_C1 * z_pad(e->family));
  if (e->family == 1 && !strcmp(name, "l1_w")) return hit(e->l1_w, (long long)L1_OUT * L1_KPAD);
  if (e->family == 1 && !strcmp(name, "l1_wT")) return hit(e->l1_wT, (long long)L1_KPAD * L1_OUT);
  return nullptr;
}
