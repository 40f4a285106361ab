// C-ABI launchers for the per-op entry points of include/jckgan.h (host side; kernels in *.hpp): everything that is per thread or per
// process in the launcher layer (error string, knobs, the kernel registry's table, the launch profiler) and the launchers of the
// memory-bound kernels.  The gather-GEMM and weight-gradient launchers are ops_gemm.hip, the BatchNorm launchers ops_bn.hip.
#include "ops_internal.hpp"
#include "ew.hpp"
#include "ew_optim.hpp"
#include "latent.hpp"
#include "resize.hpp"

#include <cstdlib>
#include <cstring>
#include <string>

static thread_local std::string g_err;
void jck_set_error(const std::string& s) { g_err = s; }
extern "C" const char* jck_last_error(void) { return g_err.c_str(); }
// hash of csrc/ + include/jckgan.h at build time (hipgan/build.py passes it; the loader refuses a binary whose answer differs from
// the sources beside it); 100 for a hand-made build without the define
#ifndef JCK_BUILD_ID
#define JCK_BUILD_ID 100
#endif
extern "C" int jck_version(void) { return JCK_BUILD_ID; }

// ---------------------------------------------------------------------------------------------------------
// kernel registry (ops_internal.hpp: KernelId): {launch name, profiler label} per id, in the order of the ids.  A null launch name:
// a kernel that is not built (bf16's register-staged 64 x 128 tile, whose label the LDS-DMA kernels of that tile report) or launches
// that were never named (BatchNorm); the LDS-DMA kernels carry the label of the register-staged tile of their size.
// ---------------------------------------------------------------------------------------------------------
struct KernelInfo { const char* launch; const char* label; };
#define SAME(s) {s, s}
static constexpr KernelInfo KERNELS[] = {
    SAME("igemm<bf16,128,128>"),   SAME("igemm<bf16,128,64>"),   SAME("igemm<bf16,64,128,img>"),   {nullptr, "igemm<bf16,64,128>"}, SAME("igemm<bf16,16,256>"),
    SAME("igemm<f32,128,128>"),    SAME("igemm<f32,128,64>"),    SAME("igemm<f32,64,128,img>"),    SAME("igemm<f32,64,128>"),       SAME("igemm<f32,16,256>"),
    SAME("igemm<bf16x3,128,128>"), SAME("igemm<bf16x3,128,64>"), SAME("igemm<bf16x3,64,128,img>"), SAME("igemm<bf16x3,64,128>"),    SAME("igemm<bf16x3,16,256>"),
    {"igemm_dma_persist<128,256,8>", "igemm<bf16,128,256>"}, {"igemm_dma_persist<128,128,4>", "igemm<bf16,128,128>"},
    {"igemm_dma_persist<128,64,4>", "igemm<bf16,128,64>"},   {"igemm_dma_persist<64,128,4>", "igemm<bf16,64,128>"},
    {"igemm_dma<128,256,3,ws,8>", "igemm<bf16,128,256>"},    {"igemm_dma<128,128,2>", "igemm<bf16,128,128>"},
    {"igemm_dma<128,64,3,ws>", "igemm<bf16,128,64>"},        {"igemm_dma<64,128,2>", "igemm<bf16,64,128>"},
    {"img_down", "img_down<bf16>"}, {"img_up", "img_up<bf16>"},
    {"wgrad_dma<3,ws>", "wgrad<bf16,128,128>"}, {"wgrad_dma<2>", "wgrad<bf16,128,128>"},
    SAME("wgrad<bf16,128,128>"),   SAME("wgrad<bf16,128,64>"),   SAME("wgrad<bf16,64,64,img>"),   SAME("wgrad<bf16,64,64>"),
    SAME("wgrad<f32,128,128>"),    SAME("wgrad<f32,128,64>"),    SAME("wgrad<f32,64,64,img>"),    SAME("wgrad<f32,64,64>"),
    SAME("wgrad<bf16x3,128,128>"), SAME("wgrad<bf16x3,128,64>"), SAME("wgrad<bf16x3,64,64,img>"), SAME("wgrad<bf16x3,64,64>"),
    {nullptr, "bn_act_fwd"}, {nullptr, "bn_bwd_resident"}, {nullptr, "bn_bwd_3launch"},
    {nullptr, "latent_loss"}, {nullptr, "latent_adam"},
    {nullptr, "conv_up_mask"}, {nullptr, "leaky_affine_bwd"}, {nullptr, "critic_ds"}, {nullptr, "latent_loss_ex"},
    {nullptr, "feat_match"}, {nullptr, "img_prep_u8_any"}, {nullptr, "img_prep_u8_box"}};
#undef SAME
static_assert(sizeof(KERNELS) / sizeof(KERNELS[0]) == K_COUNT, "KERNELS and the KernelId offsets disagree");
// the id arithmetic against the table, row by row: what every launch site's id resolves to (the affine 16 x 256 form with 8..32 gathered
// channels, NSUB = 0, shares its tile's row)
constexpr bool same_str(const char* a, const char* b) { return *a == *b && (!*a || same_str(a + 1, b + 1)); }
constexpr bool row(KernelId id, const char* launch, const char* label) { return same_str(KERNELS[id].launch, launch) && same_str(KERNELS[id].label, label); }
static_assert(row(kid_igemm<PrecBf16, 128, 128, 1>(), "igemm<bf16,128,128>", "igemm<bf16,128,128>") && row(kid_igemm<PrecBf16, 128, 64, 1>(), "igemm<bf16,128,64>", "igemm<bf16,128,64>") && row(kid_igemm<PrecBf16, 64, 128, 2>(), "igemm<bf16,64,128,img>", "igemm<bf16,64,128,img>") && row(kid_igemm<PrecBf16, 16, 256, 1>(), "igemm<bf16,16,256>", "igemm<bf16,16,256>") &&
              row(kid_igemm<PrecF32, 128, 128, 1>(), "igemm<f32,128,128>", "igemm<f32,128,128>") && row(kid_igemm<PrecF32, 128, 64, 1>(), "igemm<f32,128,64>", "igemm<f32,128,64>") && row(kid_igemm<PrecF32, 64, 128, 2>(), "igemm<f32,64,128,img>", "igemm<f32,64,128,img>") && row(kid_igemm<PrecF32, 64, 128, 1>(), "igemm<f32,64,128>", "igemm<f32,64,128>") && row(kid_igemm<PrecF32, 16, 256, 1>(), "igemm<f32,16,256>", "igemm<f32,16,256>") &&
              row(kid_igemm<PrecBf16x3, 128, 128, 1>(), "igemm<bf16x3,128,128>", "igemm<bf16x3,128,128>") && row(kid_igemm<PrecBf16x3, 128, 64, 1>(), "igemm<bf16x3,128,64>", "igemm<bf16x3,128,64>") && row(kid_igemm<PrecBf16x3, 64, 128, 2>(), "igemm<bf16x3,64,128,img>", "igemm<bf16x3,64,128,img>") && row(kid_igemm<PrecBf16x3, 64, 128, 1>(), "igemm<bf16x3,64,128>", "igemm<bf16x3,64,128>") && row(kid_igemm<PrecBf16x3, 16, 256, 1>(), "igemm<bf16x3,16,256>", "igemm<bf16x3,16,256>") &&
              row(kid_igemm_dma(K_IGEMM_PERSIST, 128, 256), "igemm_dma_persist<128,256,8>", "igemm<bf16,128,256>") && row(kid_igemm_dma(K_IGEMM_PERSIST, 128, 128), "igemm_dma_persist<128,128,4>", "igemm<bf16,128,128>") && row(kid_igemm_dma(K_IGEMM_PERSIST, 128, 64), "igemm_dma_persist<128,64,4>", "igemm<bf16,128,64>") && row(kid_igemm_dma(K_IGEMM_PERSIST, 64, 128), "igemm_dma_persist<64,128,4>", "igemm<bf16,64,128>") &&
              row(kid_igemm_dma(K_IGEMM_DMA, 128, 256), "igemm_dma<128,256,3,ws,8>", "igemm<bf16,128,256>") && row(kid_igemm_dma(K_IGEMM_DMA, 128, 128), "igemm_dma<128,128,2>", "igemm<bf16,128,128>") && row(kid_igemm_dma(K_IGEMM_DMA, 128, 64), "igemm_dma<128,64,3,ws>", "igemm<bf16,128,64>") && row(kid_igemm_dma(K_IGEMM_DMA, 64, 128), "igemm_dma<64,128,2>", "igemm<bf16,64,128>") &&
              row(K_IMG_DOWN, "img_down", "img_down<bf16>") && row(K_IMG_UP, "img_up", "img_up<bf16>") && row(K_WGRAD_DMA_WS, "wgrad_dma<3,ws>", "wgrad<bf16,128,128>") && row(K_WGRAD_DMA, "wgrad_dma<2>", "wgrad<bf16,128,128>") &&
              row(kid_wgrad<PrecBf16, 128, 128, 1>(), "wgrad<bf16,128,128>", "wgrad<bf16,128,128>") && row(kid_wgrad<PrecBf16, 128, 64, 1>(), "wgrad<bf16,128,64>", "wgrad<bf16,128,64>") && row(kid_wgrad<PrecBf16, 64, 64, 2>(), "wgrad<bf16,64,64,img>", "wgrad<bf16,64,64,img>") && row(kid_wgrad<PrecBf16, 64, 64, 1>(), "wgrad<bf16,64,64>", "wgrad<bf16,64,64>") &&
              row(kid_wgrad<PrecF32, 128, 128, 1>(), "wgrad<f32,128,128>", "wgrad<f32,128,128>") && row(kid_wgrad<PrecF32, 128, 64, 1>(), "wgrad<f32,128,64>", "wgrad<f32,128,64>") && row(kid_wgrad<PrecF32, 64, 64, 2>(), "wgrad<f32,64,64,img>", "wgrad<f32,64,64,img>") && row(kid_wgrad<PrecF32, 64, 64, 1>(), "wgrad<f32,64,64>", "wgrad<f32,64,64>") &&
              row(kid_wgrad<PrecBf16x3, 128, 128, 1>(), "wgrad<bf16x3,128,128>", "wgrad<bf16x3,128,128>") && row(kid_wgrad<PrecBf16x3, 128, 64, 1>(), "wgrad<bf16x3,128,64>", "wgrad<bf16x3,128,64>") && row(kid_wgrad<PrecBf16x3, 64, 64, 2>(), "wgrad<bf16x3,64,64,img>", "wgrad<bf16x3,64,64,img>") && row(kid_wgrad<PrecBf16x3, 64, 64, 1>(), "wgrad<bf16x3,64,64>", "wgrad<bf16x3,64,64>") &&
              same_str(KERNELS[K_LATENT_LOSS].label, "latent_loss") && same_str(KERNELS[K_LATENT_ADAM].label, "latent_adam") &&
              same_str(KERNELS[K_CONV_UP_MASK].label, "conv_up_mask") && same_str(KERNELS[K_LEAKY_AFFINE_BWD].label, "leaky_affine_bwd") &&
              same_str(KERNELS[K_CRITIC_DS].label, "critic_ds") && same_str(KERNELS[K_LATENT_LOSS_EX].label, "latent_loss_ex") && same_str(KERNELS[K_FEAT_MATCH].label, "feat_match") && same_str(KERNELS[K_IMG_PREP_ANY].label, "img_prep_u8_any") && same_str(KERNELS[K_IMG_PREP_BOX].label, "img_prep_u8_box") &&
              same_str(KERNELS[K_BN_ACT_FWD].label, "bn_act_fwd") && same_str(KERNELS[K_BN_BWD_RES].label, "bn_bwd_resident") && same_str(KERNELS[K_BN_BWD_3L].label, "bn_bwd_3launch") &&
              kid_igemm<PrecBf16, 16, 256, 0>() == kid_igemm<PrecBf16, 16, 256, 1>() && !KERNELS[K_IGEMM + 3].launch,
              "KERNELS and the kid_* functions disagree");
static thread_local const char* g_last_launch = "";
void note_launch(KernelId k) { g_last_launch = KERNELS[k].launch ? KERNELS[k].launch : ""; }      // (a tile without a name: bf16's register-staged 64 x 128)
extern "C" const char* jck_last_launch(void) { return g_last_launch; }
extern "C" const char* jck_launch_name(int i) {       // the i-th launch name, in the order of the ids
  for (int k = 0; k < K_COUNT; ++k)
    if (KERNELS[k].launch && i-- == 0) return KERNELS[k].launch;
  return nullptr;
}
extern "C" int jck_pad_rows(int c) { return c <= 16 ? 16 : (c <= 64 ? 64 : (c + 127) / 128 * 128); }
extern "C" int jck_pad_chan(int c) { return c == 3 ? 4 : c; }

// ---------------------------------------------------------------------------------------------------------
// kernel-selection knobs: defaults are the measured-best choices; each can be preset with an environment variable of the
// same name (JCK_<KEY>) or changed at run time with jck_tune("<key>", value) - which is what lets a test force the other
// variant at a small shape.
// ---------------------------------------------------------------------------------------------------------
static int env_int(const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; }
int g_igemm_dma_ksplit = env_int("JCK_IGEMM_DMA_KSPLIT", 1);   // split-K plain GEMMs on the LDS-DMA gather-GEMM; 0: register-staged
int g_bn_bwd_fuse = env_int("JCK_BN_BWD_FUSE", 1);       // three-launch BatchNorm backward as two: the apply sums its slice's partial rows itself (bn_bwd_apply_fused_kernel); 2: fp32 too
int g_bn_res = env_int("JCK_BN_RES", 1);                  // resident one-launch BatchNorm backward (bnres.hpp); 0: reduce + sums + apply, 2: whenever it fits
int g_wgrad_wgs = env_int("JCK_WGRAD_WGS", 256);      // split-K target workgroups
int g_wgrad_ws = env_int("JCK_WGRAD_WS", 1);          // wave-specialised LDS-DMA weight gradient; 0: the 4-wave, 2-stage form
int g_wgrad_dma = env_int("JCK_WGRAD_DMA", 1);        // LDS-DMA weight gradient; 0: register-staged
extern "C" int jck_tune(const char* key, int value) {
  struct { const char* k; int* p; } tab[] = {{"bn_res", &g_bn_res}, {"igemm_dma_ksplit", &g_igemm_dma_ksplit}, {"bn_bwd_fuse", &g_bn_bwd_fuse},
                                              {"wgrad_wgs", &g_wgrad_wgs}, {"wgrad_ws", &g_wgrad_ws}, {"wgrad_dma", &g_wgrad_dma}};
  for (auto& t : tab)
    if (key && !strcmp(t.k, key)) { *t.p = value; return JCK_OK; }
  JCK_FAIL(JCK_E_ARG, std::string("jck_tune: unknown key ") + (key ? key : "(null)"));
}

#include <vector>
// ---------------------------------------------------------------------------------------------------------
// launch profiler (ops_internal.hpp: ProfScope)
// ---------------------------------------------------------------------------------------------------------
bool g_prof_on = false;
static std::vector<ProfRec> g_prof;
void ProfScope::begin(KernelId k, double flops, hipStream_t st, double bytes) {
  r.kernel = k; r.flops = flops; r.bytes = bytes; r.st = st;
  (void)hipEventCreate(&r.e0); (void)hipEventCreate(&r.e1);
  (void)hipEventRecord(r.e0, st);
}
void ProfScope::end() {
  (void)hipEventRecord(r.e1, r.st);
  g_prof.push_back(r);
}
bool jck_prof_is_on() { return g_prof_on; }
extern "C" int jck_prof_enable(int on) {
  g_prof_on = on != 0;
  return JCK_OK;
}
// Synchronises the recorded events, accumulates per (profiler label, HIP stream the launches ran on): count, total ms, total
// algorithmic FLOPs, total algorithmic bytes (streaming kernels).  A label launched on two streams comes back as two rows.
// Returns the number of rows written (<= cap).  name_out[i] points at a static string.
extern "C" int jck_prof_collect(int cap, const char** name_out, int* count_out, double* ms_out, double* flops_out, double* bytes_out,
                                void** stream_out) {
  struct Row { const char* label; hipStream_t st; int cnt; double ms, fl, by; };
  std::vector<Row> rows;
  for (auto& r : g_prof) {
    (void)hipEventSynchronize(r.e1);
    float t = 0.f;
    (void)hipEventElapsedTime(&t, r.e0, r.e1);
    const char* label = KERNELS[r.kernel].label;
    Row* q = nullptr;
    for (auto& x : rows) if (!strcmp(x.label, label) && x.st == r.st) { q = &x; break; }
    if (!q) { rows.push_back(Row{label, r.st, 0, 0.0, 0.0, 0.0}); q = &rows.back(); }
    q->cnt++; q->ms += t; q->fl += r.flops; q->by += r.bytes;
    (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1);
  }
  g_prof.clear();
  int n = 0;
  for (auto& x : rows) {
    if (n >= cap) break;
    name_out[n] = x.label; count_out[n] = x.cnt; ms_out[n] = x.ms; flops_out[n] = x.fl;
    if (bytes_out) bytes_out[n] = x.by;
    if (stream_out) stream_out[n] = (void*)x.st;
    ++n;
  }
  return n;
}

// rows of partial statistics a launch may write: one per (tile, wave) = at most one per 32 pixels, or - the persistent kernels'
// accumulated BatchNorm-backward rows - [<= 4 groups][<= 512 workgroups / channel tiles][<= 4 pixel waves] <= 4096
extern "C" size_t jck_stats_floats(long long pixels, int C, int nyrep) {
  return (size_t)std::max<long long>(pixels / 32 + 16, 4096) * (size_t)std::max(1, nyrep) * 2 * (size_t)C;
}
extern "C" size_t jck_packed_bytes(int prec, long long elems) { return (size_t)elems * (prec_f32_storage(prec) ? 4 : 2); }

// ---------------------------------------------------------------------------------------------------------
// packing
// ---------------------------------------------------------------------------------------------------------
extern "C" int jck_pack_down(int prec, const float* w, int Cs, int Cb, void* wp, void* stream) {
  const int cbp = jck_pad_chan(Cb), rows = jck_pad_rows(Cs);
  if (!is_pow2(cbp)) JCK_FAIL(JCK_E_ARG, "pack_down: Cb must be 3 or a power of two");
  const long long total = (long long)rows * 16 * cbp;
  DISPATCH_T(prec, hipLaunchKernelGGL(pack_down_kernel<T>, dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream, w, Cs, Cb,
                                      rows, ilog2(cbp), (T*)wp));
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
extern "C" int jck_pack_up(int prec, const float* w, int Cs, int Cb, void* wp, void* stream) {
  if (Cb <= 4) {     // thin outputs: four parities as rows of one operand (see jck_conv_up)
    if (Cs % 64) JCK_FAIL(JCK_E_ARG, "pack_up: Cs % 64 != 0 for a <=4-channel output");
    const long long total16 = 16ll * 9 * Cs;
    DISPATCH_T(prec, hipLaunchKernelGGL(pack_up16_kernel<T>, dim3(ew_grid(total16)), dim3(256), 0, (hipStream_t)stream, w, Cs, Cb,
                                        (T*)wp));
    HIPCHK(hipGetLastError());
    return JCK_OK;
  }
  const int rows = jck_pad_rows(Cb);
  const long long total = 4ll * rows * 4 * Cs;
  DISPATCH_T(prec, hipLaunchKernelGGL(pack_up_kernel<T>, dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream, w, Cs, Cb, rows,
                                      (T*)wp));
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
extern "C" int jck_pack_g1(int prec, const float* w, int Ci, int Co, int CiPad, void* wp, void* stream) {
  const long long total = 16ll * Co * CiPad;
  DISPATCH_T(prec, hipLaunchKernelGGL(pack_g1_kernel<T>, dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream, w, Ci, Co, CiPad,
                                      (T*)wp));
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
extern "C" int jck_pack_head(const float* w, int C, float* wp, void* stream) {
  hipLaunchKernelGGL(pack_head_kernel, dim3(cdiv(16 * C, 256)), dim3(256), 0, (hipStream_t)stream, w, C, wp);
  HIPCHK(hipGetLastError());
  return JCK_OK;
}

// ---------------------------------------------------------------------------------------------------------
// images, heads
// ---------------------------------------------------------------------------------------------------------
extern "C" int jck_resize_norm(const float* in, float* out, int N, int C, int H, int W, int OH, int OW, float pre_scale,
                               float pre_shift, const float* mean, const float* stdv, void* stream) {
  if (!in || !out || !mean || !stdv || N < 1 || C < 1 || H < 1 || W < 1 || OH < 1 || OW < 1) JCK_FAIL(JCK_E_ARG, "resize_norm: bad arguments");
  hipLaunchKernelGGL(resize_norm_kernel, dim3(ew_grid((long long)N * C * OH * OW)), dim3(256), 0, (hipStream_t)stream, in, out, N, C, H,
                     W, OH, OW, pre_scale, pre_shift, mean, stdv);
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
extern "C" int jck_img_prep_u8(int prec, const unsigned char* data, const int64_t* idx, const float* noise, float keep, float mix,
                               void* out_nhwc4, float* out_nchw, int B, int Hs, int Ws, void* stream) {
  if (!data || B < 1 || Hs < 1 || Ws < 1) JCK_FAIL(JCK_E_ARG, "img_prep_u8: bad arguments");
  if (!out_nhwc4 && !out_nchw) return JCK_OK;
  DISPATCH_T(prec, hipLaunchKernelGGL(img_prep_u8_kernel<T>, dim3(ew_grid((long long)B * 4 * Hs * Ws)), dim3(256), 0,
                                      (hipStream_t)stream, data, (const long long*)idx, noise, keep, mix, (T*)out_nhwc4, out_nchw, B,
                                      Hs, Ws));
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
// ---- any-size input pipeline (resize.hpp): the tap tables are made on the host, in Pillow's double arithmetic and order
// (ImagingResample's precompute_coeffs + normalize_coeffs_8bpc with the bilinear filter) ----
static int resize_geometry_ok(int Hs, int Ws, int S) {
  return (S == 64 || S == 128) && Hs >= 1 && Ws >= 1 && Hs <= JCK_RESIZE_MAX_SRC && Ws <= JCK_RESIZE_MAX_SRC;
}
static int resize_ksize(int L, int S) {
  const double scale = (double)L / (double)S, support = scale < 1.0 ? 1.0 : scale;
  return (int)std::ceil(support) * 2 + 1;
}
extern "C" long long jck_resize_taps_bytes(int Hs, int Ws, int S) {
  if (!resize_geometry_ok(Hs, Ws, S)) JCK_FAIL(JCK_E_ARG, "resize taps: S must be 64 or 128 and 1 <= Hs, Ws <= " + std::to_string(JCK_RESIZE_MAX_SRC));
  return 4ll * (RESIZE_HDR + (long long)S * (2 + resize_ksize(Ws, S)) + (long long)S * (2 + resize_ksize(Hs, S)));
}
// one axis: lo[S], cnt[S], k[K][S] (include/jckgan.h); every product, sum and quotient below is rounded on its own
static void resize_axis_taps(int L, int S, int K, int* lo_out, int* cnt_out, int* k_out) {
#pragma clang fp contract(off)
  const double scale = (double)L / (double)S;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 1.0 * filterscale;
  const double ss = 1.0 / filterscale;
  double w[2 * JCK_RESIZE_MAX_SRC / 64 + 3];                  // K <= 2 * ceil(1024 / 64) + 1
  for (int o = 0; o < S; ++o) {
    const double center = (o + 0.5) * scale;
    int lo = (int)(center - support + 0.5);
    if (lo < 0) lo = 0;
    int hi = (int)(center + support + 0.5);
    if (hi > L) hi = L;
    const int cnt = hi - lo;
    double ww = 0.0;
    for (int j = 0; j < cnt; ++j) {
      double a = (j + lo - center + 0.5) * ss;
      if (a < 0.0) a = -a;
      w[j] = a < 1.0 ? 1.0 - a : 0.0;
      ww += w[j];
    }
    for (int j = 0; j < K; ++j) {
      double v = 0.0;
      if (j < cnt) v = ww != 0.0 ? w[j] / ww : w[j];
      k_out[j * S + o] = j < cnt ? (int)(0.5 + v * (double)(1 << 22)) : 0;      // bilinear weights are never negative
    }
    lo_out[o] = lo;
    cnt_out[o] = cnt;
  }
}
extern "C" int jck_resize_taps_build(int Hs, int Ws, int S, void* host_buf) {
  if (!resize_geometry_ok(Hs, Ws, S)) JCK_FAIL(JCK_E_ARG, "resize taps: S must be 64 or 128 and 1 <= Hs, Ws <= " + std::to_string(JCK_RESIZE_MAX_SRC));
  if (!host_buf) JCK_FAIL(JCK_E_ARG, "resize taps: host_buf is NULL");
  const int KX = resize_ksize(Ws, S), KY = resize_ksize(Hs, S);
  int* t = (int*)host_buf;
  const int hdr[RESIZE_HDR] = {(int)JCK_RESIZE_TAPS_MAGIC, Hs, Ws, S, KX, KY, 0, 0};
  memcpy(t, hdr, sizeof(hdr));
  int* ax = t + RESIZE_HDR;
  resize_axis_taps(Ws, S, KX, ax, ax + S, ax + 2 * S);
  ax += (2 + KX) * S;
  resize_axis_taps(Hs, S, KY, ax, ax + S, ax + 2 * S);
  return JCK_OK;
}
// The band of output rows of one workgroup and the dynamic LDS it takes, for Hs source rows (of the image, or of the box): the source
// rows a band can touch are (band - 1) * scale + 2 * support + 1 <= band * Hs / S + 2 * ceil(Hs / S) + 2, each 3 * S bytes after the
// horizontal pass; the band is halved while that exceeds 64 KiB
static long long resize_band_lds(int Hs, int S, int* band_out, int* rows_out) {
  int band = RESIZE_BAND, rows = 0;
  for (;; band >>= 1) {
    rows = std::min(band * Hs / S + 2 * ((Hs + S - 1) / S) + 2, Hs);
    if ((long long)rows * 3 * S <= 65536 || band == 1) break;
  }
  *band_out = band, *rows_out = rows;
  return (long long)rows * 3 * S;
}
extern "C" long long jck_resize_lds_bytes(int Hs, int S, int* band, int* rows) {
  if (!resize_geometry_ok(Hs, 1, S)) JCK_FAIL(JCK_E_ARG, "resize_lds_bytes: S must be 64 or 128 and 1 <= Hs <= " + std::to_string(JCK_RESIZE_MAX_SRC));
  int b, r;
  const long long bytes = resize_band_lds(Hs, S, &b, &r);
  if (band) *band = b;
  if (rows) *rows = r;
  return bytes;
}
extern "C" int jck_img_prep_u8_any(int prec, const unsigned char* data, const int64_t* idx, const unsigned char* flip, const float* noise,
                                   const unsigned* rng, int tensor_id, float keep, float mix, void* out_nhwc4, float* out_nchw, int B,
                                   int Hs, int Ws, int S, const void* taps_dev, void* stream) {
  if (!data || !taps_dev || B < 1 || B > (1 << 24)) JCK_FAIL(JCK_E_ARG, "img_prep_u8_any: data and taps_dev must be set, 1 <= B <= 2^24");
  if (!resize_geometry_ok(Hs, Ws, S)) JCK_FAIL(JCK_E_ARG, "img_prep_u8_any: S must be 64 or 128 and 1 <= Hs, Ws <= " + std::to_string(JCK_RESIZE_MAX_SRC));
  if (prec != JCK_PREC_BF16 && !prec_f32_storage(prec)) JCK_FAIL(JCK_E_ARG, "bad prec");
  if ((uintptr_t)taps_dev % 4) JCK_FAIL(JCK_E_ARG, "img_prep_u8_any: taps_dev must be 4-byte aligned");
  if (!out_nhwc4 && !out_nchw) return JCK_OK;
  int band, rows;
  if (resize_band_lds(Hs, S, &band, &rows) > 65536) JCK_FAIL(JCK_E_ARG, "img_prep_u8_any: no band of output rows fits 64 KiB of LDS");
  const hipStream_t st = (hipStream_t)stream;
  ProfScope prof(K_IMG_PREP_ANY, 0.0, st, (double)B * (3.0 * Hs * Ws + (double)S * S * (out_nhwc4 ? (prec == JCK_PREC_BF16 ? 8 : 16) : 12)));
  DISPATCH_T(prec, hipLaunchKernelGGL(img_prep_u8_any_kernel<T>, dim3((unsigned)B * (S / band)), dim3(RESIZE_THREADS), (size_t)rows * 3 * S, st,
                                      data, (const long long*)idx, flip, noise, rng, (unsigned)tensor_id, keep, mix, (T*)out_nhwc4, out_nchw,
                                      Hs, Ws, S, resize_ksize(Ws, S), resize_ksize(Hs, S), band, rows, (unsigned)JCK_RESIZE_TAPS_MAGIC,
                                      (const int*)taps_dev));
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
// ---- the same transform of a box of the source (img_prep_u8_box_kernel): the table, the band and the LDS are those of a source of
// Hc x Wc; the kernel adds the box's corner to its addresses ----
extern "C" int jck_img_prep_u8_box(int prec, const unsigned char* data, const int64_t* idx, const unsigned char* flip, const int* origin,
                                   const float* noise, const unsigned* rng, int tensor_id, float keep, float mix, void* out_nhwc4,
                                   float* out_nchw, int B, int Hs, int Ws, int Hc, int Wc, int y0, int x0, int S, const void* taps_dev,
                                   void* stream) {
  if (!data || !taps_dev || B < 1 || B > (1 << 24)) JCK_FAIL(JCK_E_ARG, "img_prep_u8_box: data and taps_dev must be set, 1 <= B <= 2^24");
  if (!resize_geometry_ok(Hs, Ws, S)) JCK_FAIL(JCK_E_ARG, "img_prep_u8_box: S must be 64 or 128 and 1 <= Hs, Ws <= " + std::to_string(JCK_RESIZE_MAX_SRC));
  if (Hc < 1 || Wc < 1 || Hc > Hs || Wc > Ws)
    JCK_FAIL(JCK_E_ARG, "img_prep_u8_box: a box of " + std::to_string(Hc) + "x" + std::to_string(Wc) + " does not lie in a source of " + std::to_string(Hs) + "x" + std::to_string(Ws));
  if (!origin && (y0 < 0 || x0 < 0 || y0 > Hs - Hc || x0 > Ws - Wc))
    JCK_FAIL(JCK_E_ARG, "img_prep_u8_box: origin (" + std::to_string(y0) + ", " + std::to_string(x0) + ") puts the box outside the source");
  if (prec != JCK_PREC_BF16 && !prec_f32_storage(prec)) JCK_FAIL(JCK_E_ARG, "bad prec");
  if ((uintptr_t)taps_dev % 4 || (uintptr_t)origin % 4) JCK_FAIL(JCK_E_ARG, "img_prep_u8_box: taps_dev and origin must be 4-byte aligned");
  if (!out_nhwc4 && !out_nchw) return JCK_OK;
  int band, rows;
  const long long lds = resize_band_lds(Hc, S, &band, &rows);
  if (lds > 65536) JCK_FAIL(JCK_E_ARG, "img_prep_u8_box: no band of output rows fits 64 KiB of LDS");
  const hipStream_t st = (hipStream_t)stream;
  ProfScope prof(K_IMG_PREP_BOX, 0.0, st, (double)B * (3.0 * Hc * Wc + (double)S * S * (out_nhwc4 ? (prec == JCK_PREC_BF16 ? 8 : 16) : 12)));
  DISPATCH_T(prec, hipLaunchKernelGGL(img_prep_u8_box_kernel<T>, dim3((unsigned)B * (S / band)), dim3(RESIZE_THREADS), (size_t)lds, st, data,
                                      (const long long*)idx, flip, origin, noise, rng, (unsigned)tensor_id, keep, mix, (T*)out_nhwc4,
                                      out_nchw, Hs, Ws, Hc, Wc, y0, x0, S, resize_ksize(Wc, S), resize_ksize(Hc, S), band, rows,
                                      (unsigned)JCK_RESIZE_TAPS_MAGIC, (const int*)taps_dev));
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
// in-kernel Philox noise instead of an uploaded noise tensor (philox.hpp: pixel_normals); rng = device uint32[4]
extern "C" int jck_img_prep_rng(int prec, const float* img, const unsigned* rng, int tensor_id, float keep, float mix, void* out, int N,
                                int HW, void* stream) {
  if (!rng) JCK_FAIL(JCK_E_ARG, "img_prep_rng: rng is NULL");
  DISPATCH_T(prec, hipLaunchKernelGGL(img_prep_kernel<T>, dim3(ew_grid((long long)N * HW)), dim3(256), 0, (hipStream_t)stream, img,
                                      (const float*)nullptr, keep, mix, (T*)out, N, HW, rng, (unsigned)tensor_id));
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
extern "C" int jck_img_prep_u8_rng(int prec, const unsigned char* data, const int64_t* idx, const unsigned* rng, int tensor_id,
                                   float keep, float mix, void* out_nhwc4, int B, int Hs, int Ws, void* stream) {
  if (!data || !rng || !out_nhwc4 || B < 1) JCK_FAIL(JCK_E_ARG, "img_prep_u8_rng: bad arguments");
  DISPATCH_T(prec, hipLaunchKernelGGL(img_prep_u8_kernel<T>, dim3(ew_grid((long long)B * 4 * Hs * Ws)), dim3(256), 0, (hipStream_t)stream,
                                      data, (const long long*)idx, (const float*)nullptr, keep, mix, (T*)out_nhwc4, (float*)nullptr, B,
                                      Hs, Ws, rng, (unsigned)tensor_id));
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
extern "C" int jck_axpy_noise_rng(int prec, const void* x, const unsigned* rng, int tensor_id, float keep, float mix, void* out, int N,
                                  int HW, void* stream) {
  if (!rng) JCK_FAIL(JCK_E_ARG, "axpy_noise_rng: rng is NULL");
  DISPATCH_T(prec, hipLaunchKernelGGL(axpy_noise_kernel<T>, dim3(ew_grid((long long)N * HW)), dim3(256), 0, (hipStream_t)stream,
                                      (const T*)x, (const float*)nullptr, keep, mix, (T*)out, N, HW, rng, (unsigned)tensor_id));
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
extern "C" int jck_img_prep(int prec, const float* img, const float* noise, float keep, float mix, void* out, int N, int HW,
                            void* stream) {
  DISPATCH_T(prec, hipLaunchKernelGGL(img_prep_kernel<T>, dim3(ew_grid((long long)N * HW)), dim3(256), 0,
                                      (hipStream_t)stream, img, noise, keep, mix, (T*)out, N, HW));
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
extern "C" int jck_nhwc4_to_nchw(int prec, const void* in, float* out, int N, int HW, void* stream) {
  DISPATCH_T(prec, hipLaunchKernelGGL(nhwc4_to_nchw_kernel<T>, dim3(ew_grid((long long)N * HW)), dim3(256), 0,
                                      (hipStream_t)stream, (const T*)in, out, N, HW));
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
extern "C" int jck_img_to_u8(int prec, const void* in, unsigned char* out_u8_nhwc, int N, int HW, void* stream) {
  if (N < 1 || HW < 4 || HW % 4) JCK_FAIL(JCK_E_ARG, "img_to_u8: N >= 1 and HW a multiple of 4");
  if ((uintptr_t)in % 16 || (uintptr_t)out_u8_nhwc % 4) JCK_FAIL(JCK_E_ARG, "img_to_u8: the image must be 16-byte, the output 4-byte aligned");
  const long long total4 = (long long)N * HW / 4;
  DISPATCH_T(prec, hipLaunchKernelGGL(img_to_u8_kernel<T>, dim3(ew_grid(total4)), dim3(256), 0, (hipStream_t)stream, (const T*)in,
                                      out_u8_nhwc, total4));
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
extern "C" int jck_axpy_noise(int prec, const void* x, const float* noise, float keep, float mix, void* out, int N, int HW,
                              void* stream) {
  DISPATCH_T(prec, hipLaunchKernelGGL(axpy_noise_kernel<T>, dim3(ew_grid((long long)N * HW)), dim3(256), 0,
                                      (hipStream_t)stream, (const T*)x, noise, keep, mix, (T*)out, N, HW));
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
// jck_axpy_noise (noise given) / jck_axpy_noise_rng (rng given) followed by jck_interp(real, out, alpha) -> xhat as ONE launch
extern "C" int jck_mix_interp(int prec, const void* x, const float* noise, const unsigned* rng, int tensor_id, float keep, float mix,
                              void* out, const void* real, const float* alpha, void* xhat, int N, int HW, void* stream) {
  if (!real || !alpha || !xhat) JCK_FAIL(JCK_E_ARG, "mix_interp: real / alpha / xhat is NULL");
  if ((noise != nullptr) == (rng != nullptr)) JCK_FAIL(JCK_E_ARG, "mix_interp: exactly one of noise and rng");
  DISPATCH_T(prec, hipLaunchKernelGGL(axpy_noise_kernel<T>, dim3(ew_grid((long long)N * HW)), dim3(256), 0, (hipStream_t)stream,
                                      (const T*)x, noise, keep, mix, (T*)out, N, HW, rng, (unsigned)tensor_id, (const T*)real, alpha, (T*)xhat));
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
extern "C" int jck_interp(int prec, const void* a, const void* b, const float* alpha, void* out, int N, int HW, void* stream) {
  DISPATCH_T(prec, hipLaunchKernelGGL(interp_kernel<T>, dim3(ew_grid((long long)N * HW)), dim3(256), 0, (hipStream_t)stream,
                                      (const T*)a, (const T*)b, alpha, (T*)out, N, HW));
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
extern "C" int jck_gp_norm(int prec, const void* g, int N, int HW, float* scal, int slot, int scal_ld, float* norms, void* stream) {
  if (scal && slot >= 0 && scal_ld < N) JCK_FAIL(JCK_E_ARG, "gp_norm: scal_ld < N");
  DISPATCH_T(prec, hipLaunchKernelGGL(gp_norm_kernel<T>, dim3(N), dim3(256), 0, (hipStream_t)stream, (const T*)g, HW, scal,
                                      slot, scal_ld, norms));
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
extern "C" int jck_tanh_bwd(int prec, const void* g, const void* y, float scale, void* out, long long numel, void* stream) {
  return tanh_bwd_ev(prec, g, y, scale, out, numel, (hipStream_t)stream, nullptr);
}
int tanh_bwd_ev(int prec, const void* g, const void* y, float scale, void* out, long long numel, hipStream_t stream, hipEvent_t done) {
  if (numel % 4) JCK_FAIL(JCK_E_ARG, "tanh_bwd: numel % 4 != 0");
  DISPATCH_T(prec, LAUNCH_EV(tanh_bwd_kernel<T>, dim3(ew_grid(numel / 4)), dim3(256), 0, stream, done,
                             (const T*)g, (const T*)y, scale, (T*)out, numel / 4));
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
// the kernels' table of G (<= 4, checked by the caller) row groups; false: a group has a scalar slot and there is no table of >= B
// columns to write it to
static bool head_groups(HeadGroups& hg, int B, int G, const float* targets, const int* modes, const int* slot_loss, const int* slot_p,
                        const float* scal, int scal_ld) {
  hg = {};
  hg.rows_per_group = B;
  for (int g = 0; g < G; ++g) {
    hg.target[g] = targets[g]; hg.mode[g] = modes[g]; hg.slot_loss[g] = slot_loss[g]; hg.slot_p[g] = slot_p[g];
    if ((slot_loss[g] >= 0 || slot_p[g] >= 0) && (!scal || scal_ld < B)) return false;
  }
  return true;
}
// G (<= 4) batches of B rows stacked in a4 / prob / ds, each with its own target, mode and scalar slots - one launch
extern "C" int jck_head_fwd_grouped(int prec, const void* a4, const float* wp, const float* bias, int B, int K, int G,
                                    const float* targets, const int* modes, float* prob, float* ds, float* scal,
                                    const int* slot_loss, const int* slot_p, int scal_ld, void* stream) {
  return head_fwd_grouped_ev(prec, a4, wp, bias, B, K, G, targets, modes, prob, ds, scal, slot_loss, slot_p, scal_ld, nullptr,
                             (hipStream_t)stream, nullptr);
}
// g_out (optional): the rows' input gradient ds[n] * wp[k] from the same launch; done (optional): completed by the launch
int head_fwd_grouped_ev(int prec, const void* a4, const float* wp, const float* bias, int B, int K, int G, const float* targets,
                        const int* modes, float* prob, float* ds, float* scal, const int* slot_loss, const int* slot_p, int scal_ld,
                        void* g_out, hipStream_t stream, hipEvent_t done) {
  if (K % 8) JCK_FAIL(JCK_E_ARG, "head_fwd: K % 8 != 0");
  if (G < 1 || G > 4 || B < 1) JCK_FAIL(JCK_E_ARG, "head_fwd: 1..4 groups of >= 1 rows");
  HeadGroups hg;
  if (!head_groups(hg, B, G, targets, modes, slot_loss, slot_p, scal, scal_ld)) JCK_FAIL(JCK_E_ARG, "head_fwd: scalar slots need scal with scal_ld >= B");
  DISPATCH_T(prec, LAUNCH_EV(head_fwd_kernel<T>, dim3(G * B), dim3(256), 0, stream, done, (const T*)a4, wp, K, bias,
                             hg, 1.0f / (float)B, prob, ds, scal, scal_ld, (T*)g_out));
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
extern "C" int jck_head_fwd(int prec, const void* a4, const float* wp, const float* bias, int B, int K, float target, int mode,
                            float* prob, float* ds, float* scal, int slot_loss, int slot_p, int scal_ld, void* stream) {
  return jck_head_fwd_grouped(prec, a4, wp, bias, B, K, 1, &target, &mode, prob, ds, scal, &slot_loss, &slot_p, scal_ld, stream);
}
// the head at inference: logit and sigmoid alone (ew.hpp: score_head_kernel)
extern "C" int jck_score_head(int prec, const void* x, const float* w, const float* bias, int B, int K, float* logit, float* prob, void* stream) {
  if (!x || !w || !logit) JCK_FAIL(JCK_E_ARG, "score_head: null x / w / logit");
  if (B < 1 || K < 8 || K % 8) JCK_FAIL(JCK_E_ARG, "score_head: B >= 1 and K a multiple of 8");
  if ((uintptr_t)x % 16 || (uintptr_t)w % 16) JCK_FAIL(JCK_E_ARG, "score_head: x and w must be 16-byte aligned");
  DISPATCH_T(prec, hipLaunchKernelGGL(score_head_kernel<T>, dim3(B), dim3(256), 0, (hipStream_t)stream, (const T*)x, w, K, bias, logit, prob));
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
// an NHWC activation pooled to a grid x grid raster, as fp32 feature columns (ew.hpp: grid_pool_kernel)
extern "C" int jck_grid_pool(int prec, const void* a, int N, int H, int C, int grid, int mode, float* out, long long ld, long long col0, void* stream) {
  if (!a || !out) JCK_FAIL(JCK_E_ARG, "grid_pool: null a / out");
  if (N < 1 || H < 1 || C < 8 || C % 8) JCK_FAIL(JCK_E_ARG, "grid_pool: N >= 1, H >= 1 and C a multiple of 8");
  if (grid != 1 && grid != 2 && grid != 4) JCK_FAIL(JCK_E_ARG, "grid_pool: grid must be 1, 2 or 4");
  if (H % grid) JCK_FAIL(JCK_E_ARG, "grid_pool: H must be a multiple of grid");
  if (mode != 0 && mode != 1) JCK_FAIL(JCK_E_ARG, "grid_pool: mode must be 0 (max) or 1 (mean)");
  if (col0 < 0 || ld < col0 + (long long)grid * grid * C) JCK_FAIL(JCK_E_ARG, "grid_pool: the column block [col0, col0 + grid * grid * C) must lie inside a row of ld");
  if ((uintptr_t)a % 16 || ((uintptr_t)out + 4 * (uintptr_t)col0) % 16 || (N > 1 && ld % 4))
    JCK_FAIL(JCK_E_ARG, "grid_pool: a and every row's column block must be 16-byte aligned");
  DISPATCH_T(prec, {
    const long long total = (long long)N * grid * grid * (C / (16 / (int)sizeof(T)));
    hipLaunchKernelGGL(grid_pool_kernel<T>, dim3(ew_grid(total, 64)), dim3(64), 0, (hipStream_t)stream, (const T*)a, H, C, grid, mode, out, ld, col0, total);
  });
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
// jck_linear_finish + jck_head_fwd_grouped + the input-gradient half of jck_head_bwd + jck_dropout of CGAN's head in one launch
// (ew.hpp: cg_head_mid_kernel); N = 256 columns; rows = G * B; mask required
int cg_head_mid(int prec, const float* slab, int ksplit, const float* bias1, const float* mask, float scale, void* h, void* hd, const float* w2,
                const float* bias2, int B, int G, const float* targets, const int* modes, float* prob, float* ds, float* scal,
                const int* slot_loss, const int* slot_p, int scal_ld, void* g_hd, void* g_h, hipStream_t stream) {
  if (G < 1 || G > 4 || B < 1 || !mask || !slab || ksplit < 1) JCK_FAIL(JCK_E_ARG, "cg_head_mid: 1..4 groups of >= 1 rows, a dropout mask, split-K slabs");
  HeadGroups hg;
  if (!head_groups(hg, B, G, targets, modes, slot_loss, slot_p, scal, scal_ld)) JCK_FAIL(JCK_E_ARG, "cg_head_mid: scalar slots need scal with scal_ld >= B");
  const long long rows = (long long)G * B;
  DISPATCH_T(prec, hipLaunchKernelGGL(cg_head_mid_kernel<T>, dim3((unsigned)rows), dim3(256), 0, stream, slab, ksplit, rows * 256, bias1, mask, scale,
                                      (T*)h, (T*)hd, w2, bias2, hg, 1.0f / (float)B, prob, ds, scal, scal_ld, (T*)g_hd, (T*)g_h));
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
#define HEAD_NS 8          /* partial rows of jck_head_bwd */
#define HEAD_CONV_NS 16    /* partial rows of jck_head_bwd_conv */
extern "C" size_t jck_head_bwd_ws_floats(int K) { return (size_t)HEAD_CONV_NS * K; }
extern "C" int jck_head_bwd(int prec, const float* ds, const float* wp, const void* a4, int B, int K, void* g_a4, float* dwp,
                            int accumulate, float* ws, void* stream) {
  if (K % 8) JCK_FAIL(JCK_E_ARG, "head_bwd: K % 8 != 0");
  if (dwp && !ws) JCK_FAIL(JCK_E_ARG, "head_bwd: the weight gradient needs a workspace of jck_head_bwd_ws_floats(K) floats");
  if (g_a4) {
    const long long total8 = (long long)B * K / 8;
    DISPATCH_T(prec, hipLaunchKernelGGL(head_dgrad_kernel<T>, dim3(ew_grid(total8)), dim3(256), 0, (hipStream_t)stream, ds, wp,
                                        K, (T*)g_a4, total8));
    HIPCHK(hipGetLastError());
  }
  if (dwp) {
    DISPATCH_T(prec, hipLaunchKernelGGL(head_wgrad_kernel<T>, dim3(cdiv(K / 8, 64), HEAD_NS), dim3(256), 0, (hipStream_t)stream, ds,
                                        (const T*)a4, B, K, ws));
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(head_part_reduce_kernel, dim3(cdiv(K, 256)), dim3(256), 0, (hipStream_t)stream, ws, HEAD_NS, K, 0, dwp, accumulate);
    HIPCHK(hipGetLastError());
  }
  return JCK_OK;
}
extern "C" int jck_head_bwd_conv(int prec, const float* ds, const float* wp, const void* a4, int B, int C, void* g_a4,
                                 float* grad, float* ws, void* stream) {
  return jck_head_bwd_conv2(prec, ds, wp, a4, B, 0, C, g_a4, grad, ws, stream);
}
// jck_head_bwd_conv over B rows and, in the same launch, the input gradient alone for the B_more rows behind them (ds, a4, g_a4 hold
// B + B_more rows; the weight gradient sums the first B only) - the loss groups and the penalty group of the batched D pass
extern "C" int jck_head_bwd_conv2(int prec, const float* ds, const float* wp, const void* a4, int B, int B_more, int C, void* g_a4,
                                  float* grad, float* ws, void* stream) {
  return head_bwd_conv2_ev(prec, ds, wp, a4, B, B_more, C, g_a4, grad, ws, (hipStream_t)stream, nullptr, nullptr);
}
// side / handover (both or neither): the ordered sum of the weight-gradient partial rows - wanted by the optimiser only - runs on
// `side` behind `handover`, which the launch that writes the rows completes itself
int head_bwd_conv2_ev(int prec, const float* ds, const float* wp, const void* a4, int B, int B_more, int C, void* g_a4, float* grad, float* ws,
                      hipStream_t stream, hipStream_t side, hipEvent_t handover) {
  if (C % 8) JCK_FAIL(JCK_E_ARG, "head_bwd_conv: C % 8 != 0");
  if ((side != nullptr) != (handover != nullptr)) JCK_FAIL(JCK_E_ARG, "head_bwd_conv: side stream and hand-over event go together");
  if (B_more < 0 || (B_more > 0 && !g_a4)) JCK_FAIL(JCK_E_ARG, "head_bwd_conv2: the extra rows produce an input gradient only");
  if (!g_a4 && !grad) return JCK_OK;
  if (grad && !ws) JCK_FAIL(JCK_E_ARG, "head_bwd_conv: the weight gradient needs a workspace of jck_head_bwd_ws_floats(16*C) floats");
  const int K = 16 * C;
  if (!g_a4 && grad && side) {
    // only the weight gradient is wanted (the rows' input gradient came out of head_fwd_grouped_ev, which completed `handover`):
    // the partial rows and their sum both run on `side`
    HIPCHK(hipStreamWaitEvent(side, handover, 0));
    DISPATCH_T(prec, hipLaunchKernelGGL(head_bwd_fused_kernel<T>, dim3(cdiv(K / 8, 64), HEAD_CONV_NS), dim3(256), 0, side, ds, wp,
                                        (const T*)a4, B, K, C, (T*)nullptr, ws, 0));
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(head_part_reduce_kernel, dim3(cdiv(K, 256)), dim3(256), 0, side, ws, HEAD_CONV_NS, K, C, grad, 1);
    HIPCHK(hipGetLastError());
    return JCK_OK;
  }
  hipEvent_t ev = grad ? handover : nullptr;
  DISPATCH_T(prec, LAUNCH_EV(head_bwd_fused_kernel<T>, dim3(cdiv(K / 8, 64), HEAD_CONV_NS), dim3(256), 0, stream, ev, ds, wp,
                             (const T*)a4, B, K, C, (T*)g_a4, grad ? ws : nullptr, B_more));
  HIPCHK(hipGetLastError());
  if (grad) {
    hipStream_t rs = stream;
    if (ev) { HIPCHK(hipStreamWaitEvent(side, ev, 0)); rs = side; }
    hipLaunchKernelGGL(head_part_reduce_kernel, dim3(cdiv(K, 256)), dim3(256), 0, rs, ws, HEAD_CONV_NS, K, C, grad, 1);
    HIPCHK(hipGetLastError());
  }
  return JCK_OK;
}

extern "C" int jck_adam(float* p, const float* g, float* m, float* v, long long n, double lr, double beta1, double beta2,
                        double eps, int step, float grad_scale, void* stream) {
  if (step < 1) JCK_FAIL(JCK_E_ARG, "adam: step is 1-based");
  // scalar preparation in double exactly as torch.optim.Adam does it in Python, then one cast to float
  const double bc1 = 1.0 - std::pow(beta1, step), bc2 = 1.0 - std::pow(beta2, step);
  const float step_size = (float)(lr / bc1), bc2s = (float)std::sqrt(bc2);
  const int vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
  hipLaunchKernelGGL(adam_kernel<false>, dim3(ew_grid(vec ? (n + 3) / 4 : n)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, (float)(1.0 - beta1),
                     (float)beta2, (float)(1.0 - beta2), (float)eps, step_size, bc2s, grad_scale, (const float*)nullptr, vec);
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
// jck_adam that advances an exponential moving average of the parameters in the same launch (the averaged generator that GAN
// trainers sample and checkpoint): ema <- lerp(ema, p_new, ema_weight), ema_weight = 1 - decay; skip_if as in jck_adam_hp
extern "C" int jck_adam_ema(float* p, const float* g, float* m, float* v, float* ema, long long n, double lr, double beta1, double beta2,
                            double eps, int step, float grad_scale, float ema_weight, const unsigned* skip_if, void* stream) {
  if (step < 1) JCK_FAIL(JCK_E_ARG, "adam: step is 1-based");
  if (!ema) JCK_FAIL(JCK_E_ARG, "adam_ema: null EMA arena (jck_adam is the form without one)");
  if (!(ema_weight >= 0.f && ema_weight <= 1.f)) JCK_FAIL(JCK_E_ARG, "adam_ema: ema_weight = 1 - decay must lie in [0, 1]");
  const double bc1 = 1.0 - std::pow(beta1, step), bc2 = 1.0 - std::pow(beta2, step);
  const float step_size = (float)(lr / bc1), bc2s = (float)std::sqrt(bc2);
  const int vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) & 15) == 0;
  hipLaunchKernelGGL(adam_kernel<true>, dim3(ew_grid(vec ? (n + 3) / 4 : n)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, (float)(1.0 - beta1),
                     (float)beta2, (float)(1.0 - beta2), (float)eps, step_size, bc2s, grad_scale, (const float*)nullptr, vec, (float*)nullptr,
                     0ll, skip_if, ema, ema_weight);
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
// the same update with {step_size, bc2_sqrt} read from device memory: jck_adam_set_step writes them (same host arithmetic)
// ... and (rz / ralpha / rmasks, each optional) the step's small random inputs, drawn by the same launch (ew_optim.hpp: adam_hp_kernel)
int jck_adam_set_step(float* hp, double lr, double beta1, double beta2, int step, unsigned long long seed, float ema_w, hipStream_t st, float* rz,
                      long long nz, float* ralpha, long long nalpha, float* rmasks, long long nmask, float keep_p, float* zero,
                      long long nzero, float* zbig0, long long nzbig0, float* zbig1, long long nzbig1, void* zpad, int zd, int zp, int zpad_f32) {
  if (step < 1) JCK_FAIL(JCK_E_ARG, "adam: step is 1-based");
  if (((uintptr_t)zbig0 | (uintptr_t)zbig1) & 15 || (nzbig0 | nzbig1) & 3) JCK_FAIL(JCK_E_ARG, "set_step: large zero ranges must be 16-byte aligned, counts % 4 == 0");
  const double bc1 = 1.0 - std::pow(beta1, step), bc2 = 1.0 - std::pow(beta2, step);
  StepRng r = {rz, rz ? nz : 0, ralpha, ralpha ? nalpha : 0, rmasks, rmasks ? nmask : 0, keep_p, zero, zero ? nzero : 0,
               {zbig0, zbig1}, {zbig0 ? nzbig0 : 0, zbig1 ? nzbig1 : 0}, (rz && zd > 0 && zp >= zd) ? zpad : nullptr, zd, zp, zpad_f32};
  const long long quads = std::max((r.nz + 3) / 4 + (r.nalpha + 3) / 4 + (r.nmask + 3) / 4, std::max(r.nzbig[0], r.nzbig[1]) / 16);
  const unsigned blocks = (unsigned)std::max<long long>(1, std::min<long long>((quads + 255) / 256, 1024));
  hipLaunchKernelGGL(adam_hp_kernel, dim3(blocks), dim3(256), 0, st, hp, (float)(lr / bc1), (float)std::sqrt(bc2), (unsigned)seed,
                     (unsigned)(seed >> 32), (unsigned)step, r, ema_w);
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
// test / binding access to the per-step draws: fills z [nz] ~ N(0,1), alpha [nalpha] ~ U[0,1), masks [nmask] ~ Bernoulli(keep_p)
// exactly as jck_engine_set_step does for step `step` and noise seed `seed`; hp: device float[8] scratch
extern "C" int jck_step_rng(float* hp, int step, unsigned long long seed, float* z, long long nz, float* alpha, long long nalpha,
                            float* masks, long long nmask, float keep_p, void* stream) {
  if (!hp) JCK_FAIL(JCK_E_ARG, "step_rng: hp scratch (8 floats) is required");
  return jck_adam_set_step(hp, 2e-4, 0.5, 0.999, step, seed, 0.f, (hipStream_t)stream, z, nz, alpha, nalpha, masks, nmask, keep_p);
}
int jck_adam_hp(float* p, const float* g, float* m, float* v, long long n, double beta1, double beta2, double eps,
                float grad_scale, const float* hp, hipStream_t st, float* zero, long long nzero, const unsigned* skip_if, float* ema) {
  const int vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) & 15) == 0;
  if (zero && (((uintptr_t)zero & 15) || (nzero & 3))) JCK_FAIL(JCK_E_ARG, "adam: the zero range must be 16-byte aligned, count % 4 == 0");
  if (ema)
    hipLaunchKernelGGL(adam_kernel<true>, dim3(ew_grid(vec ? (n + 3) / 4 : n)), dim3(256), 0, st, p, g, m, v, n, (float)(1.0 - beta1), (float)beta2,
                       (float)(1.0 - beta2), (float)eps, 0.f, 1.f, grad_scale, hp, vec, zero, zero ? nzero / 4 : 0, skip_if, ema, 1.f);
  else
    hipLaunchKernelGGL(adam_kernel<false>, dim3(ew_grid(vec ? (n + 3) / 4 : n)), dim3(256), 0, st, p, g, m, v, n, (float)(1.0 - beta1), (float)beta2,
                     (float)(1.0 - beta2), (float)eps, 0.f, 1.f, grad_scale, hp, vec, zero, zero ? nzero / 4 : 0, skip_if);
  HIPCHK(hipGetLastError());
  return JCK_OK;
}

int jck_adam_pack_hp(int prec, float* p, const float* g, float* m, float* v, float* ema, long long first, long long count, const PackJobs& jobs,
                     double beta1, double beta2, double eps, float grad_scale, const float* hp, float step_size, float bc2_sqrt, float ema_w,
                     hipStream_t st, float* zero, long long nzero, const unsigned* skip_if, const TailJobs* tail, int tail_x) {
  if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) & 15) JCK_FAIL(JCK_E_ARG, "adam_pack: the arenas must be 16-byte aligned");
  if (zero && (((uintptr_t)zero & 15) || (nzero & 3))) JCK_FAIL(JCK_E_ARG, "adam: the zero range must be 16-byte aligned, count % 4 == 0");
  if (first < 0 || count < 0) JCK_FAIL(JCK_E_ARG, "adam_pack: bad range");
  // the jobs of the weights inside the range, grouped per weight (the forms of one weight are neighbours in the table) ...
  PackJobs sel = {};
  AdamPlan plan = {};
  int blk = 0;
  for (int i = 0; i < jobs.n; ++i) {
    const PackJob& J = jobs.j[i];
    const int A = J.a, Bc = J.kind == 4 ? 1 : J.b;
    const long long off = J.w - p, numel = 16ll * A * Bc;
    if (off + numel <= first || off >= first + count) continue;
    if (off < first || off + numel > first + count || (off & 3)) JCK_FAIL(JCK_E_ARG, "adam_pack: a conv weight straddles the range or is not 16-byte aligned");
    if (plan.ng && plan.g[plan.ng - 1].off == off) ++plan.g[plan.ng - 1].nj;
    else {
      if (plan.ng && off < plan.g[plan.ng - 1].off + 16ll * plan.g[plan.ng - 1].A * plan.g[plan.ng - 1].Bc) JCK_FAIL(JCK_E_ARG, "adam_pack: conv weights must come in arena order, without overlap");
      plan.g[plan.ng] = AdamGroup{off, A, Bc, sel.n, 1};
      plan.first_blk[plan.ng++] = blk;
      blk += cdiv(A, 16) * cdiv(Bc, 16);
    }
    sel.j[sel.n++] = J;
  }
  plan.first_blk[plan.ng] = blk;
  const int pair_blks = blk;
  // ... and what lies between them
  int fblk = 0;
  auto flat = [&](long long a, long long b) {
    if (a >= b) return true;
    if (plan.nf == ADAM_MAX_FLAT) return false;
    plan.fa[plan.nf] = a; plan.fb[plan.nf] = b;
    plan.first_fblk[plan.nf++] = fblk;
    const long long a4 = std::min((a + 3) & ~3ll, b), b4 = std::max(b & ~3ll, a4);
    fblk += (int)std::max<long long>(1, ((b4 - a4) / 4 + 255) / 256);
    return true;
  };
  long long at = first;
  bool fits = true;
  for (int i = 0; i < plan.ng; ++i) {
    fits = fits && flat(at, plan.g[i].off);
    at = plan.g[i].off + 16ll * plan.g[i].A * plan.g[i].Bc;
  }
  fits = fits && flat(at, first + count);
  if (!fits) JCK_FAIL(JCK_E_ARG, "adam_pack: more than ADAM_MAX_FLAT ranges between the conv weights");
  plan.first_fblk[plan.nf] = fblk;
  const int nb = pair_blks + fblk;
  const TailJobs no_tail = {};
  const int tail_blks = tail ? tail_x * (tail->nl + 1) : 0;
  if (nb + tail_blks == 0) return JCK_OK;
  const AdamArenas a = {p, g, m, v, ema, hp, zero, zero ? nzero / 4 : 0, skip_if};
  const AdamScal s = {(float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps, step_size, bc2_sqrt, grad_scale, ema_w};
#define ADAM_PACK_LAUNCH(W, EMA) \
  hipLaunchKernelGGL((adam_pack_kernel<W, EMA>), dim3(nb + tail_blks), dim3(256), 0, st, sel, plan, a, s, pair_blks, fblk, tail ? *tail : no_tail, tail ? tail_x : 1)
  if (prec == JCK_PREC_BF16) { if (ema) ADAM_PACK_LAUNCH(bf16_t, true); else ADAM_PACK_LAUNCH(bf16_t, false); }
  else if (ema) ADAM_PACK_LAUNCH(float, true);
  else ADAM_PACK_LAUNCH(float, false);
#undef ADAM_PACK_LAUNCH
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
extern "C" int jck_adam_pack(int prec, float* p, const float* g, float* m, float* v, float* ema, long long n, int njobs, const int* kind,
                             const long long* w_off, void* const* wp, const int* a, const int* b, double lr, double beta1, double beta2, double eps,
                             int step, float grad_scale, float ema_weight, const unsigned* skip_if, void* stream) {
  if (step < 1) JCK_FAIL(JCK_E_ARG, "adam: step is 1-based");
  if (njobs < 0 || njobs > PACK_MAX_JOBS || (njobs && (!kind || !w_off || !wp || !a || !b))) JCK_FAIL(JCK_E_ARG, "adam_pack: 0..12 jobs, every table given");
  if (prec != JCK_PREC_BF16 && !prec_f32_storage(prec)) JCK_FAIL(JCK_E_ARG, "bad prec");
  PackJobs jobs = {};
  for (int i = 0; i < njobs; ++i) {
    PackJob& J = jobs.j[i];
    if (kind[i] < 0 || kind[i] > 4 || a[i] < 1 || (kind[i] != 4 && b[i] < 1) || !wp[i]) JCK_FAIL(JCK_E_ARG, "adam_pack: bad job");
    J.w = p + w_off[i]; J.wp = wp[i]; J.kind = kind[i]; J.a = a[i]; J.b = kind[i] == 4 ? 0 : b[i];
    J.total = (long long)a[i] * (kind[i] == 4 ? 1 : b[i]);
    // the third size of each layout follows from the two channel counts, as in the engine's table
    J.c = kind[i] == 0 ? ilog2(jck_pad_chan(b[i])) : kind[i] == 1 ? jck_pad_rows(b[i]) : kind[i] == 3 ? (a[i] + 127) / 128 * 128 : 0;
    if (kind[i] == 0 && (1 << J.c) != jck_pad_chan(b[i])) JCK_FAIL(JCK_E_ARG, "adam_pack: down needs a power-of-two (padded) Cb");
    if (kind[i] == 2 && b[i] > 4) JCK_FAIL(JCK_E_ARG, "adam_pack: up16 packs at most 4 channels");
  }
  jobs.n = njobs;
  const double bc1 = 1.0 - std::pow(beta1, step), bc2 = 1.0 - std::pow(beta2, step);
  return jck_adam_pack_hp(prec, p, g, m, v, ema, 0, n, jobs, beta1, beta2, eps, grad_scale, nullptr, (float)(lr / bc1), (float)std::sqrt(bc2),
                          ema_weight, (hipStream_t)stream, nullptr, 0, skip_if, nullptr, 0);
}

// ---------------------------------------------------------------------------------------------------------
// latent projection (latent.hpp)
// ---------------------------------------------------------------------------------------------------------
// latent_loss_kernel for both entry points below: `id` is the caller's registry label, `bytes` its traffic estimate.  No weight and no
// image gradient: the PLAIN instantiation of the same body.
static int launch_latent_loss(KernelId id, double bytes, int prec, const void* x, const float* target, const float* weight, const void* g_x,
                              void* g_raw, float* loss, int N, int HW, hipStream_t st) {
  ProfScope prof(id, 0.0, st, bytes);
  if (target && !weight && !g_x) {
    DISPATCH_T(prec, hipLaunchKernelGGL((latent_loss_kernel<T, true>), dim3(N), dim3(256), 0, st, (const T*)x, target, nullptr, nullptr, (T*)g_raw,
                                        loss, HW));
  } else {
    DISPATCH_T(prec, hipLaunchKernelGGL((latent_loss_kernel<T, false>), dim3(N), dim3(256), 0, st, (const T*)x, target, weight, (const T*)g_x,
                                        (T*)g_raw, loss, HW));
  }
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
// loss_out[b] = mean((x_b - t_b)^2) over the 3 * HW real elements; g_raw_out = its gradient at the pre-tanh product (NHWC4, element
// type of prec, padding channel 0).  The target is the caller's NCHW fp32 tensor, read in place.
extern "C" int jck_latent_loss(int prec, const void* x_nhwc4, const float* target_nchw_f32, void* g_raw_out, float* loss_out, int N,
                               int HW, void* stream) {
  if (!x_nhwc4 || !target_nchw_f32 || !g_raw_out || !loss_out || N < 1 || HW < 1) JCK_FAIL(JCK_E_ARG, "latent_loss: bad arguments");
  if ((((uintptr_t)x_nhwc4 | (uintptr_t)g_raw_out) & 15) != 0) JCK_FAIL(JCK_E_ARG, "latent_loss: the image tensors must be 16-byte aligned");
  return launch_latent_loss(K_LATENT_LOSS, (double)N * HW * (12.0 + 8.0 * (prec_f32_storage(prec) ? 4 : 2)), prec, x_nhwc4, target_nchw_f32,
                            nullptr, nullptr, g_raw_out, loss_out, N, HW, (hipStream_t)stream);
}
// Sums the Z split-K slabs [Z][N][ld] of the dz product in order, adds the prior's gradient 2 * prior * z / 100 and applies
// torch.optim.Adam(betas = (0.9, 0.999), eps = 1e-8) update number t >= 1 to z, m, v [N][100]; z also goes, in the element type, to
// the first 100 columns of the operand rows z_operand [N][CiPad].  t = 0: sum only - z receives the summed gradient, m, v and
// z_operand are not touched (and may be null).
extern "C" int jck_latent_adam(int prec, const float* slab, int Z, int ld, float* z, float* m, float* v, float lr, float prior, int t,
                               void* z_operand, int CiPad, int N, void* stream) {
  const int zd = 100;
  if (!slab || !z || Z < 1 || ld < zd || N < 1 || t < 0) JCK_FAIL(JCK_E_ARG, "latent_adam: bad arguments");
  if (t > 0 && (!m || !v || !z_operand || CiPad < zd)) JCK_FAIL(JCK_E_ARG, "latent_adam: an update needs m, v and the operand rows");
  const double bc1 = 1.0 - std::pow(0.9, (double)t), bc2 = 1.0 - std::pow(0.999, (double)t);
  const double step_size = t > 0 ? (double)lr / bc1 : 0.0, bc2_sqrt = t > 0 ? std::sqrt(bc2) : 1.0;
  ProfScope prof(K_LATENT_ADAM, 0.0, (hipStream_t)stream, (double)N * zd * 4.0 * (Z + 6));
  DISPATCH_T(prec, hipLaunchKernelGGL(latent_adam_kernel<T>, dim3((unsigned)((N * zd + 255) / 256)), dim3(256), 0, (hipStream_t)stream, slab, Z,
                                      (long long)N * ld, ld, z, m, v, step_size, bc2_sqrt, 2.0 * (double)prior / zd, (T*)z_operand, CiPad, zd,
                                      N, t == 0 ? 1 : 0));
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
// jck_latent_loss with a per-pixel weight (fp32 [N][HW], or null: 1) and an additive image gradient g_x (NHWC4, element type, or null):
// loss_out[b] = sum_p w_p sum_c (x - t)^2 / (3 sum_p w_p), g_raw_out = (k w_p (x - t) + g_x) (1 - x^2) with k = 2 / (3 sum_p w_p).
// target null (g_x required): loss 0, g_raw_out = g_x (1 - x^2).  weight null and g_x null: jck_latent_loss (the same launch).
extern "C" int jck_latent_loss_ex(int prec, const void* x_nhwc4, const float* target_nchw_f32, const float* weight, const void* g_x,
                                  void* g_raw_out, float* loss_out, int N, int HW, void* stream) {
  if (!x_nhwc4 || !g_raw_out || !loss_out || N < 1 || HW < 1) JCK_FAIL(JCK_E_ARG, "latent_loss_ex: bad arguments");
  if (!target_nchw_f32 && !g_x) JCK_FAIL(JCK_E_ARG, "latent_loss_ex: without a target the image gradient g_x is required");
  if ((((uintptr_t)x_nhwc4 | (uintptr_t)g_raw_out | (uintptr_t)g_x) & 15) != 0) JCK_FAIL(JCK_E_ARG, "latent_loss_ex: the image tensors must be 16-byte aligned");
  return launch_latent_loss(K_LATENT_LOSS_EX, (double)N * HW * (16.0 + 12.0 * (prec_f32_storage(prec) ? 4 : 2)), prec, x_nhwc4, target_nchw_f32,
                            weight, g_x, g_raw_out, loss_out, N, HW, (hipStream_t)stream);
}
// g_y[r, c] = a[r, c] > 0 ? scale[c] g[r, c] : scale[c] g[r, c] slope over `rows` rows of C channels (a power of two >= 8); g_y may be g
extern "C" int jck_leaky_affine_bwd(int prec, const void* g, const void* a, const float* scale, float slope, void* g_y, long long rows, int C,
                                    void* stream) {
  if (!g || !a || !scale || !g_y || rows < 1) JCK_FAIL(JCK_E_ARG, "leaky_affine_bwd: null tensor or no rows");
  if (!is_pow2(C) || C < 8) JCK_FAIL(JCK_E_ARG, "leaky_affine_bwd: C must be a power of two >= 8");
  if ((((uintptr_t)g | (uintptr_t)a | (uintptr_t)g_y | (uintptr_t)scale) & 15) != 0) JCK_FAIL(JCK_E_ARG, "leaky_affine_bwd: tensors and scale must be 16-byte aligned");
  const long long total8 = rows * C / 8;
  ProfScope prof(K_LEAKY_AFFINE_BWD, 0.0, (hipStream_t)stream, (double)rows * C * 3.0 * (prec_f32_storage(prec) ? 4 : 2));
  DISPATCH_T(prec, hipLaunchKernelGGL(leaky_affine_bwd_kernel<T>, dim3(ew_grid(total8)), dim3(256), 0, (hipStream_t)stream, (const T*)g, (const T*)a,
                                      scale, slope, (T*)g_y, total8, C));
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
// fterm[b] = weight / M * sum (a_b - f_b)^2 over image b's M elements, and g = the gradient of that term through the folded stage
// a = leaky(scale[c] y + shift[c]): 2 weight / M * (a - f) * scale[c], times slope where a is not > 0; g_y = g, or g_y + g (accumulate)
extern "C" int jck_feat_match(int prec, const void* a, const void* f, const float* scale, float slope, float weight, void* g_y, int accumulate,
                              float* fterm, int N, long long M, int C, void* stream) {
  if (prec != JCK_PREC_BF16 && !prec_f32_storage(prec)) JCK_FAIL(JCK_E_ARG, "feat_match: bad prec");
  if (!a || !f || !scale || !g_y || !fterm || N < 1) JCK_FAIL(JCK_E_ARG, "feat_match: null tensor or no images");
  if (!is_pow2(C) || C < 8) JCK_FAIL(JCK_E_ARG, "feat_match: C must be a power of two >= 8");
  if (M < C || M % C) JCK_FAIL(JCK_E_ARG, "feat_match: M must be a positive multiple of C");
  if (!(weight >= 0.f) || !(weight <= 3.402823466e38f)) JCK_FAIL(JCK_E_ARG, "feat_match: weight must be finite and >= 0");
  if (accumulate != 0 && accumulate != 1) JCK_FAIL(JCK_E_ARG, "feat_match: accumulate must be 0 or 1");
  if ((((uintptr_t)a | (uintptr_t)f | (uintptr_t)g_y | (uintptr_t)scale) & 15) != 0) JCK_FAIL(JCK_E_ARG, "feat_match: tensors and scale must be 16-byte aligned");
  const hipStream_t st = (hipStream_t)stream;
  ProfScope prof(K_FEAT_MATCH, 0.0, st, (double)N * M * (accumulate ? 4.0 : 3.0) * (prec_f32_storage(prec) ? 4 : 2));
  if (accumulate) {
    DISPATCH_T(prec, hipLaunchKernelGGL((feat_match_kernel<T, true>), dim3(N), dim3(256), 0, st, (const T*)a, (const T*)f, scale, slope, weight,
                                        (T*)g_y, fterm, M, C));
  } else {
    DISPATCH_T(prec, hipLaunchKernelGGL((feat_match_kernel<T, false>), dim3(N), dim3(256), 0, st, (const T*)a, (const T*)f, scale, slope, weight,
                                        (T*)g_y, fterm, M, C));
  }
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
// ds[b] = weight c'(logit[b]), term[b] = weight c(logit[b]); mode 1 (nsgan): c = softplus(-logit); mode 2 (logit): c = -logit
extern "C" int jck_critic_ds(const float* logit, int mode, float weight, int B, float* ds, float* term, void* stream) {
  if (!logit || !ds || !term || B < 1) JCK_FAIL(JCK_E_ARG, "critic_ds: null logit / ds / term or no rows");
  if (mode != 1 && mode != 2) JCK_FAIL(JCK_E_ARG, "critic_ds: mode must be 1 (nsgan) or 2 (logit)");
  ProfScope prof(K_CRITIC_DS, 0.0, (hipStream_t)stream, (double)B * 12.0);
  hipLaunchKernelGGL(critic_ds_kernel, dim3(cdiv(B, 256)), dim3(256), 0, (hipStream_t)stream, logit, mode, weight, B, ds, term);
  HIPCHK(hipGetLastError());
  return JCK_OK;
}

// ---------------------------------------------------------------------------------------------------------
// CGAN: Linear operands and finish (the products: ops_gemm.hip), label embedding, concat, dropout, second-order terms of the gradient penalty
// ---------------------------------------------------------------------------------------------------------
extern "C" int jck_pack_linear(int prec, const float* w, int N, int K, int rows, int cols, int transpose, int permC, int permHW,
                               void* wp, void* stream) {
  const long long total = (long long)rows * cols;
  DISPATCH_T(prec, hipLaunchKernelGGL(pack_linear_kernel<T>, dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream, w, N, K, rows,
                                      cols, transpose, permC, permHW, (T*)wp));
  HIPCHK(hipGetLastError());
  return JCK_OK;
}

// jck_pack_linear(transpose = 0) into wp0[rows0][cols0] and jck_pack_linear(transpose = 1) into wp1[rows1][cols1], one launch
int pack_linear_pair(int prec, const float* w, int N, int K, int rows0, int cols0, void* wp0, int rows1, int cols1, void* wp1, int permC,
                     int permHW, hipStream_t stream) {
  const long long total = std::max((long long)rows0 * cols0, (long long)rows1 * cols1);
  DISPATCH_T(prec, hipLaunchKernelGGL(pack_linear_pair_kernel<T>, dim3(ew_grid(total), 2), dim3(256), 0, stream, w, N, K, rows0, cols0,
                                      (T*)wp0, rows1, cols1, (T*)wp1, permC, permHW));
  HIPCHK(hipGetLastError());
  return JCK_OK;
}

extern "C" int jck_unperm_linear_grad(const float* gp, int N, int K, int ldp, int permC, int permHW, float* grad, int accumulate,
                                      void* stream) {
  const long long total = (long long)N * K;
  hipLaunchKernelGGL(unperm_linear_grad_kernel, dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream, gp, N, K, ldp, permC,
                     permHW, grad, accumulate);
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
extern "C" int jck_linear_finish(int prec, const float* slab, int Z, const float* bias, const float* mask, float scale, void* h,
                                 void* hd, int B, int N, void* stream) {
  DISPATCH_T(prec, hipLaunchKernelGGL(linear_finish_kernel<T>, dim3(cdiv(B * N, 256)), dim3(256), 0, (hipStream_t)stream, slab, Z,
                                      (long long)B * N, bias, mask, scale, (T*)h, (T*)hd, B, N));
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
// `_tiled`: B rows that are `label_period`-row batches stacked on top of each other, all labelled by the same [label_period][NI]
// tensor (the real | fake | penalty groups of one CGAN step share the batch's labels, train/cgan_trainer.py:181-203)
extern "C" int jck_label_embed_fwd_tiled(int prec, const int64_t* labels, const float* W, const float* b, float slope, int B, int NI,
                                         int NO, void* cbuf, int ld, int col0, float* pre, int label_period, void* stream) {
  if (label_period < 0 || (label_period > 0 && B % label_period)) JCK_FAIL(JCK_E_ARG, "label_embed: rows are not a multiple of the label period");
  DISPATCH_T(prec, hipLaunchKernelGGL(label_embed_fwd_kernel<T>, dim3(B), dim3(256), (size_t)NI * sizeof(float), (hipStream_t)stream,
                                      (const long long*)labels, W, b, slope, B, NI, NO, (T*)cbuf, ld, col0, pre, label_period));
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
extern "C" int jck_label_embed_fwd(int prec, const int64_t* labels, const float* W, const float* b, float slope, int B, int NI,
                                   int NO, void* cbuf, int ld, int col0, float* pre, void* stream) {
  return jck_label_embed_fwd_tiled(prec, labels, W, b, slope, B, NI, NO, cbuf, ld, col0, pre, 0, stream);
}
extern "C" int jck_label_embed_bwd_tiled(int prec, const void* gc, int ld, int col0, const float* pre, const int64_t* labels, float slope,
                                         int B, int NI, int NO, float* dW, float* db, int label_period, void* stream) {
  if (label_period < 0 || (label_period > 0 && B % label_period)) JCK_FAIL(JCK_E_ARG, "label_embed: rows are not a multiple of the label period");
  DISPATCH_T(prec, hipLaunchKernelGGL(label_embed_bwd_kernel<T>, dim3(NI + cdiv(NO, 16)), dim3(256), (size_t)B * (sizeof(float) + sizeof(int)), (hipStream_t)stream,
                                      (const T*)gc, ld, col0, pre, (const long long*)labels, slope, B, NI, NO, dW, db, label_period));
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
extern "C" int jck_label_embed_bwd(int prec, const void* gc, int ld, int col0, const float* pre, const int64_t* labels, float slope,
                                   int B, int NI, int NO, float* dW, float* db, void* stream) {
  return jck_label_embed_bwd_tiled(prec, gc, ld, col0, pre, labels, slope, B, NI, NO, dW, db, 0, stream);
}
extern "C" int jck_concat_rows(int prec, const void* a4, int K0, void* cbuf, int ld, int B, void* stream) {
  if (K0 % 8 || ld % 8) JCK_FAIL(JCK_E_ARG, "concat_rows: K0 % 8 or ld % 8");
  const long long total8 = (long long)B * K0 / 8;
  DISPATCH_T(prec, hipLaunchKernelGGL(concat_rows_kernel<T>, dim3(ew_grid(total8)), dim3(256), 0, (hipStream_t)stream, (const T*)a4,
                                      K0, (T*)cbuf, ld, total8));
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
extern "C" int jck_split_rows(int prec, const void* gc, int ld, int K0, void* ga4, int B, void* stream) {
  if (K0 % 8 || ld % 8) JCK_FAIL(JCK_E_ARG, "split_rows: K0 % 8 or ld % 8");
  const long long total8 = (long long)B * K0 / 8;
  DISPATCH_T(prec, hipLaunchKernelGGL(split_rows_kernel<T>, dim3(ew_grid(total8)), dim3(256), 0, (hipStream_t)stream, (const T*)gc, ld,
                                      K0, (T*)ga4, total8));
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
extern "C" int jck_dropout(int prec, const void* x, const float* mask, float scale, void* y, long long n, void* stream) {
  DISPATCH_T(prec, hipLaunchKernelGGL(dropout_kernel<T>, dim3(ew_grid(n)), dim3(256), 0, (hipStream_t)stream, (const T*)x, mask, scale,
                                      (T*)y, n));
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
extern "C" int jck_colsum(int prec, const void* g, int B, int N, int ld, float* db, void* stream) {
  DISPATCH_T(prec, hipLaunchKernelGGL(colsum_kernel<T>, dim3(cdiv(N, COLSUM_COLS)), dim3(256), 0, (hipStream_t)stream, (const T*)g, B, N, ld, db));
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
extern "C" int jck_gp_grad(int prec, const void* g, const float* norms, float coef, int N, int HW, void* u, void* stream) {
  const long long total4 = (long long)N * HW;
  DISPATCH_T(prec, hipLaunchKernelGGL(gp_grad_kernel<T>, dim3(ew_grid(total4)), dim3(256), 0, (hipStream_t)stream, (const T*)g, norms,
                                      coef, HW * 4, (T*)u, total4));
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
// ws: float[B + jck_head_bwd_ws_floats(K)] (pq[n] = p(1-p), then the partial rows of the dw2 sum)
extern "C" int jck_gp_head2(int prec, const void* ughd, const float* w2, const float* prob, int B, int K, float* rs, float* dw2,
                            float* ws, void* stream) {
  return gp_head2_ev(prec, ughd, w2, prob, B, K, rs, dw2, ws, (hipStream_t)stream, nullptr, nullptr);
}
// side / handover (both or neither): the dw2 sum - wanted by the optimiser only - runs on `side` behind `handover`, which the
// launch that writes rs and pq completes itself
int gp_head2_ev(int prec, const void* ughd, const float* w2, const float* prob, int B, int K, float* rs, float* dw2, float* ws,
                hipStream_t stream, hipStream_t side, hipEvent_t handover) {
  if (K % 8 || !ws) JCK_FAIL(JCK_E_ARG, "gp_head2: K % 8 != 0 or no workspace");
  if ((side != nullptr) != (handover != nullptr)) JCK_FAIL(JCK_E_ARG, "gp_head2: side stream and hand-over event go together");
  DISPATCH_T(prec, LAUNCH_EV(gp_head2_kernel<T>, dim3(B), dim3(256), 0, stream, handover, (const T*)ughd, w2, prob, B, K, rs, ws));
  HIPCHK(hipGetLastError());
  hipStream_t gs = stream;
  if (side) { HIPCHK(hipStreamWaitEvent(side, handover, 0)); gs = side; }
  // dw2[j] += sum_n pq[n] * ughd[n][j]
  float* part = ws + (B + 63) / 64 * 64;
  DISPATCH_T(prec, hipLaunchKernelGGL(head_wgrad_kernel<T>, dim3(cdiv(K / 8, 64), HEAD_NS), dim3(256), 0, gs, ws, (const T*)ughd, B, K, part));
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(head_part_reduce_kernel, dim3(cdiv(K, 256)), dim3(256), 0, gs, part, HEAD_NS, K, 0, dw2, 1);
  HIPCHK(hipGetLastError());
  return JCK_OK;
}

// DCGAN head step of the penalty's double backward (ew.hpp: dcgan_gp_head_rows_kernel, dcgan_gp_head_cols_kernel): two launches
// where gp_head2_ev + jck_head_bwd_conv + jck_head_unpack_grad would take five.  ws: sn[n] = p(1-p) between the two.
extern "C" size_t jck_gp_head2_conv_ws_floats(int B) { return (size_t)(B + 63) / 64 * 64; }
extern "C" int jck_gp_head2_conv(int prec, const void* v4, const void* a4, const float* wp, const float* prob, int B, int C, float* rs,
                                 void* g_a4, float* grad, float* ws, void* stream) {
  if (B < 1 || C < 8 || C % 8) JCK_FAIL(JCK_E_ARG, "gp_head2_conv: B >= 1 and C % 8 == 0 required");
  if (!v4 || !a4 || !wp || !prob || !rs || !ws) JCK_FAIL(JCK_E_ARG, "gp_head2_conv: null operand or workspace");
  if (g_a4 && g_a4 == a4) JCK_FAIL(JCK_E_ARG, "gp_head2_conv: g_a4 may alias v4, not a4");
  const int K = 16 * C;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_T(prec, hipLaunchKernelGGL(dcgan_gp_head_rows_kernel<T>, dim3(B), dim3(256), 0, st, (const T*)v4, wp, K, prob, rs, ws));
  HIPCHK(hipGetLastError());
  if (!g_a4 && !grad) return JCK_OK;
  DISPATCH_T(prec, hipLaunchKernelGGL(dcgan_gp_head_cols_kernel<T>, dim3(cdiv(K / 8, GP_HEAD_CU)), dim3(256), 0, st, (const T*)v4,
                                      (const T*)a4, wp, rs, ws, B, K, C, (T*)g_a4, grad));
  HIPCHK(hipGetLastError());
  return JCK_OK;
}

// jck_linear_finish(bias = NULL, h = NULL) + gp_head2_ev + the input-gradient half of jck_head_bwd(ds = rs) + jck_dropout in one launch
// (ew.hpp: cg_gp_head_mid_kernel; 256 columns), then the dw2 sum as in gp_head2_ev (on `side` behind `handover` when given)
int gp_head_mid_ev(int prec, const float* slab, int ksplit, const float* mask, float scale, void* ughd, const float* w2, const float* prob, int B,
                   float* rs, float* dw2, float* ws, void* g_hd, void* g_h, hipStream_t stream, hipStream_t side, hipEvent_t handover) {
  if (!ws || !mask || !slab || ksplit < 1) JCK_FAIL(JCK_E_ARG, "gp_head_mid: workspace, dropout mask and split-K slabs are required");
  if ((side != nullptr) != (handover != nullptr)) JCK_FAIL(JCK_E_ARG, "gp_head_mid: side stream and hand-over event go together");
  const int K = 256;
  DISPATCH_T(prec, LAUNCH_EV(cg_gp_head_mid_kernel<T>, dim3(B), dim3(256), 0, stream, handover, slab, ksplit, (long long)B * K, mask, scale,
                             (T*)ughd, w2, prob, rs, ws, (T*)g_hd, (T*)g_h));
  HIPCHK(hipGetLastError());
  hipStream_t gs = stream;
  if (side) { HIPCHK(hipStreamWaitEvent(side, handover, 0)); gs = side; }
  float* part = ws + (B + 63) / 64 * 64;
  DISPATCH_T(prec, hipLaunchKernelGGL(head_wgrad_kernel<T>, dim3(cdiv(K / 8, 64), HEAD_NS), dim3(256), 0, gs, ws, (const T*)ughd, B, K, part));
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(head_part_reduce_kernel, dim3(cdiv(K, 256)), dim3(256), 0, gs, part, HEAD_NS, K, 0, dw2, 1);
  HIPCHK(hipGetLastError());
  return JCK_OK;
}

extern "C" int jck_sum_vec(const float* x, int n, float* out, void* stream) {
  hipLaunchKernelGGL(sum_vec_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, x, n, out);
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
extern "C" int jck_cgan_z(int prec, const float* z, const int64_t* labels, int B, int NZ, int NL, int CiPad, void* out, void* stream) {
  const long long total = (long long)B * CiPad;
  DISPATCH_T(prec, hipLaunchKernelGGL(cgan_z_kernel<T>, dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream, z,
                                      (const long long*)labels, B, NZ, NL, CiPad, (T*)out));
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
