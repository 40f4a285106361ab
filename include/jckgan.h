/* jckgan.h - C ABI of libjckgan_hip.so: the MI355X (gfx950) replacement for the DCGAN / CGAN
 * training hot path of hy-vision-learning/jck-generation.
 *
 * The reference has no FFI layer of its own: its hot path is torch.nn modules + autograd
 * (model/DCGAN.py, model/CGAN.py, train/dcgan_trainer.py, train/cgan_trainer.py).  Every entry
 * point below names the reference call site (file:line under the reference root) whose ATen work it
 * replaces.  The Python side (jck-generation_amd/hipgan) binds these symbols with ctypes; see
 * INTEGRATION.md for the stub a reference maintainer would add.
 *
 * Conventions
 *   - plain C: raw DEVICE pointers, explicit sizes, `void* stream` = hipStream_t (NULL = default)
 *   - every function returns 0 on success, a negative JCK_E_* code on error; jck_last_error()
 *     returns the message of the calling thread's last failure
 *   - no allocation, no ownership transfer: outputs and workspaces are caller-allocated
 *   - asynchronous with respect to the host; thread-compatible (one stream per caller thread)
 *   - `prec` selects storage / arithmetic:
 *       JCK_PREC_BF16  activations, gradients, GEMM operands bf16 in HBM; v_mfma_f32_16x16x32_bf16, fp32 accumulate (fast)
 *       JCK_PREC_F32   everything fp32 in HBM; v_mfma_f32_16x16x4_f32 = exact fp32 products + accumulation      (parity)
 *       JCK_PREC_BF16X3 storage and kernels of JCK_PREC_F32; the GEMM operands are split x = hi + lo (two bf16) and
 *                      each product is lo*hi + hi*lo + hi*hi on v_mfma_f32_16x16x32_bf16, fp32 accumulate   (tracking)
 *     "T" below means bf16 (2 bytes) or float (JCK_PREC_F32, JCK_PREC_BF16X3) according to `prec`
 *   - activations are NHWC; 3-channel images are stored with 4 channels (4th = 0)
 *   - a stride-2 stage is described by its BIG side [N,Hb,Wb,Cb] and SMALL side [N,Hb/2,Wb/2,Cs];
 *     Conv2d (D) maps big->small, ConvTranspose2d (G) maps small->big; both keep the weight as
 *     [Cs][Cb][4][4] fp32 (Conv2d.weight [Cout,Cin,4,4] / ConvTranspose2d.weight [Cin,Cout,4,4])
 */
#ifndef JCKGAN_H
#define JCKGAN_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define JCK_PREC_BF16 0
#define JCK_PREC_F32 1
#define JCK_PREC_BF16X3 2

#define JCK_OK 0
#define JCK_E_ARG (-1)      /* bad argument / unsupported shape */
#define JCK_E_HIP (-2)      /* HIP runtime error (see jck_last_error) */
#define JCK_E_WS (-3)       /* workspace too small */

const char* jck_last_error(void);
/* Name of the kernel that the calling thread's last gather-GEMM, weight-gradient or image-side launch ran on ("" before the
 * first), e.g. "igemm_dma_persist<128,256,8>", "wgrad_dma<3,ws>", "wgrad<bf16x3,128,64>", "img_up".  A report only: it selects
 * nothing.  jck_launch_name(i) enumerates every name the library can report, NULL past the end. */
const char* jck_last_launch(void);
const char* jck_launch_name(int i);
int jck_version(void);
/* rows of a packed weight matrix for `c` output channels (tile padding): 16, 64 or a multiple of 128 */
int jck_pad_rows(int c);
/* channels per pixel as stored in HBM: 3 -> 4, otherwise c (must be a power of two) */
int jck_pad_chan(int c);

/* ---- weight packing: fp32 parameter -> GEMM operand of element type T ---------------------------------------------
 * down : [pad_rows(Cs)][16*pad_chan(Cb)]      operand of Conv2d forward / ConvTranspose2d dgrad
 * up   : [4][pad_rows(Cb)][4*Cs]              operand of ConvTranspose2d forward / Conv2d dgrad
 * g1   : [16*Co][CiPad]                       G.conv1, ConvTranspose2d(k4,s1,p0) on a 1x1 input (model/DCGAN.py:42)
 * head : float[16*C]                          D.conv5, Conv2d(512,1,k4,s1,p0) as a dot product (model/DCGAN.py:26) */
size_t jck_packed_bytes(int prec, long long elems);
int jck_pack_down(int prec, const float* w, int Cs, int Cb, void* wp, void* stream);
int jck_pack_up(int prec, const float* w, int Cs, int Cb, void* wp, void* stream);
int jck_pack_g1(int prec, const float* w, int Ci, int Co, int CiPad, void* wp, void* stream);
int jck_pack_head(const float* w, int C, float* wp, void* stream);

/* ---- convolution-shaped products (replace aten::convolution / convolution_backward) -----------------------
 * stats (optional): partial per-channel sums for the BatchNorm that follows, float[slots][2][C] written without
 * atomics by the GEMM epilogue; *stats_slots receives the slot count to hand to jck_bn_finalize.  The buffer must
 * hold jck_stats_floats(output pixels, C, nyrep) floats (nyrep = 16 for jck_g1_fwd, else 1). */
size_t jck_stats_floats(long long pixels, int C, int nyrep);
/* small = Conv2d_k4s2p1(big)            model/DCGAN.py:10-22 forward; dgrad of model/DCGAN.py:46-58 */
int jck_conv_down(int prec, const void* big, const void* w, void* small_out, float* stats, int* stats_slots,
                  int N, int Hb, int Wb, int Cb, int Cs, void* stream);
/* big = ConvTranspose2d_k4s2p1(small)   model/DCGAN.py:46-58 forward; dgrad of model/DCGAN.py:10-22.  epi_tanh=1 fuses model/DCGAN.py:66 */
int jck_conv_up(int prec, const void* small_in, const void* w, void* big_out, float* stats, int* stats_slots,
                int epi_tanh, int N, int Hs, int Ws, int Cs, int Cb, void* stream);
/* grad[Cs][Cb][4][4] (+)= sum small (x) gather(big)     weight gradient of either layer kind */
size_t jck_conv_wgrad_ws_bytes(int N, int Hb, int Wb, int Cb, int Cs);
int jck_conv_wgrad(int prec, const void* small_side, const void* big_side, float* ws, size_t ws_bytes, float* grad,
                   int accumulate, int N, int Hb, int Wb, int Cb, int Cs, void* stream);
/* out[B][16*Co] = z[B][CiPad] x W   (NHWC [B,4,4,Co]); stats over Co channels   model/DCGAN.py:42,62 */
int jck_g1_fwd(int prec, const void* z, const void* w, void* out, float* stats, int* stats_slots, int B, int CiPad,
               int Co, void* stream);
/* Inference forms of the two products above (model/DCGAN.py:42-66 under model.eval()): the BatchNorm that follows runs on its
 * running statistics, so it is a per-channel affine, and it and the ReLU are applied to the fp32 accumulators in the product's
 * epilogue: out = relu(scale[c] * y + shift[c]), ONE rounding to the storage type, no statistics, no pre-activation tensor.
 * NaN passes as through torch.relu.  scale / shift: device float[Cb] (float[Co]; the channel of GEMM column (position, co) is co),
 * 16-byte aligned - the first two quarters of an aux table (jck_bn_eval_aux).  Cb a power of two >= 8, Cs >= 16; Co >= 4.
 * In bf16 the result is not bitwise jck_conv_up + jck_bn_act_fwd, which round y to bf16 between the two launches. */
int jck_conv_up_affine(int prec, const void* small_in, const void* w, const float* scale, const float* shift, void* big_out,
                       int N, int Hs, int Ws, int Cs, int Cb, void* stream);
int jck_g1_fwd_affine(int prec, const void* z, const void* w, const float* scale, const float* shift, void* out, int B,
                      int CiPad, int Co, void* stream);
/* Latent projection, per op.  jck_conv_down_mask: jck_conv_down (a ConvTranspose's input gradient) through a folded eval-mode stage
 * a = relu(scale[c] * y + shift[c]) in front of it: out = a_small[m, c] > 0 ? scale[c] * acc : +0 on the fp32 accumulators, ONE rounding
 * to the storage type; a NaN activation masks (torch.relu's backward).  a_small has small_out's layout [N, Hb/2, Wb/2, Cs]; scale:
 * device float[Cs], 16-byte aligned; Cs a power of two; Cb 3 / 4, 8..32 (with Cs = 64) or >= 64.  Never the persistent kernels or the
 * image-side streaming kernel: every launch ends in the gather-GEMM's shared epilogue. */
int jck_conv_down_mask(int prec, const void* big, const void* w, const void* a_small, const float* scale, void* small_out,
                       int N, int Hb, int Wb, int Cb, int Cs, void* stream);
/* Discriminator inference, per op.  jck_conv_down_affine: jck_conv_down (Conv2d k4 s2 p1, NHWC) with the eval-mode BatchNorm that
 * follows it (model/DCGAN.py:40-43 under model.eval(); scale / shift folded by jck_bn_eval_aux) and the LeakyReLU applied to the fp32
 * accumulators in the product's epilogue: t = fmaf(scale[c], acc, shift[c]), out = t > 0 ? t : t * slope (ATen's form: NaN passes,
 * -0 stays -0), ONE rounding to the storage type, no statistics, no pre-activation tensor.  scale / shift: device float[Cs], 16-byte
 * aligned - the first two quarters of an aux table.  Cb 3 or 4 with Cs = 64, or Cb a power of two >= 64; Cs a power of two >= 64;
 * anything else is JCK_E_ARG.  Never the persistent kernels or the image-side streaming kernel: every launch ends in the gather-GEMM's
 * shared epilogue (Cb = 4: the register-staged 64 x 128 tile in every precision), and jck_last_launch reports that tile's name.
 * In bf16 the result is not bitwise jck_conv_down + jck_bn_act_fwd, which round y to bf16 between the two launches. */
int jck_conv_down_affine(int prec, const void* big, const void* w, const float* scale, const float* shift, float slope,
                         void* small_out, int N, int Hb, int Wb, int Cb, int Cs, void* stream);
/* loss_out[b] = mean over the 3 * HW real elements of (x_b - t_b)^2 with x the stored tanh output (NHWC4, element type of prec) and t
 * the caller's NCHW fp32 target, read in place; g_raw_out (NHWC4, same type) = 2 (x - t) / (3 HW) * (1 - x^2), padding channel +0.
 * One launch, one workgroup per image, a fixed-order reduction: equal bits on every run and for every N.  It is jck_latent_loss_ex
 * below with weight = g_x = NULL: the same kernel, under a profiler label of its own. */
int jck_latent_loss(int prec, const void* x_nhwc4, const float* target_nchw_f32, void* g_raw_out, float* loss_out, int N, int HW,
                    void* stream);
/* g = slab[0] + slab[1] + ... (Z fp32 split-K slabs [Z][N][ld] of the dz product, summed in order) + 2 * prior * z / 100, then update
 * number t >= 1 of torch.optim.Adam(lr, betas = (0.9, 0.999), eps = 1e-8) on z, m, v (fp32 [N][100]); z is also written, in the element
 * type of prec, to the first 100 columns of the operand rows z_operand [N][CiPad] (the columns behind them are left alone).
 * t = 0: sum only - z receives the summed slabs; m, v and z_operand are not touched and may be NULL. */
int jck_latent_adam(int prec, const float* slab, int Z, int ld, float* z, float* m, float* v, float lr, float prior, int t,
                    void* z_operand, int CiPad, int N, void* stream);
/* The critic's latent gradient, per op (D(G(z)) differentiated with respect to z under model.eval(): jck_engine_latent_grad_ex).
 * jck_conv_up_mask: jck_conv_up (a Conv2d's input gradient, 4 output parities) through the folded eval-mode stage
 * a = leaky(scale[c] * y + shift[c]) in front of it: t = scale[c] * acc, out = a_big[m, c] > 0 ? t : t * slope on the fp32 accumulators,
 * ONE rounding to the storage type - ATen's leaky_relu_backward on the stored result: a = +-0 and a NaN activation take the slope.
 * a_big has big_out's layout [N, 2Hs, 2Ws, Cb]; scale: device float[Cb], 16-byte aligned; Cs and Cb powers of two >= 64, anything
 * else is JCK_E_ARG.  Never the persistent kernels; jck_last_launch reports the tile's name. */
int jck_conv_up_mask(int prec, const void* small_in, const void* w, const void* a_big, const float* scale, float slope, void* big_out,
                     int N, int Hs, int Ws, int Cs, int Cb, void* stream);
/* The same backward without a product (the deepest stage, whose gradient comes from the head): g_y[r, c] = a[r, c] > 0 ? scale[c] *
 * g[r, c] : scale[c] * g[r, c] * slope, 16 bytes per access along C (a power of two >= 8); g_y may be g. */
int jck_leaky_affine_bwd(int prec, const void* g, const void* a, const float* scale, float slope, void* g_y, long long rows, int C,
                         void* stream);
/* ds[b] = weight * c'(logit[b]), term[b] = weight * c(logit[b]).  mode 1 (nsgan): c = softplus(-logit) = -log D, the generator's
 * training loss, c' = -sigmoid(-logit), overflow-free at any logit; mode 2 (logit): c = -logit, c' = -1.  A non-finite logit gives
 * NaN in both. */
int jck_critic_ds(const float* logit, int mode, float weight, int B, float* ds, float* term, void* stream);
/* jck_latent_loss with a per-pixel weight (fp32 [N][HW], or NULL: 1) and an additive image gradient g_x (NHWC4, element type, or NULL):
 * loss_out[b] = sum_p w_p sum_c (x - t)^2 / (3 sum_p w_p), g_raw_out = (k w_p (x - t) + g_x) (1 - x^2), k = 2 / (3 sum_p w_p); two
 * fixed-order passes per image (sum w, then the loss); sum w = 0: loss 0 and no reconstruction gradient.  target NULL (g_x required):
 * loss 0, g_raw_out = g_x (1 - x^2).  weight NULL and g_x NULL is jck_latent_loss: no first pass, w and g_x never read; all-one
 * weights return the same bits. */
int jck_latent_loss_ex(int prec, const void* x_nhwc4, const float* target_nchw_f32, const float* weight, const void* g_x, void* g_raw_out,
                       float* loss_out, int N, int HW, void* stream);
/* Feature matching on a folded eval-mode stage a = leaky(scale[c] * y + shift[c]): fterm[b] = weight / M * sum over image b's M
 * elements of (a - f)^2, and that term's gradient at the stage's product y in the same pass: d = a - f, t = scale[c] * (2 weight / M * d),
 * g = a > 0 ? t : t * slope (ATen's leaky_relu_backward on a: a = +-0 and NaN take the slope), all in fp32.  accumulate 0: g_y = g;
 * accumulate 1: g_y = g_y + g, the old value read in the element type, the sum rounded once - onto a gradient that came down from
 * the head.  a, f, g_y: NHWC of the element type, M elements per image, M a multiple of C, C a power of two >= 8; scale: device
 * float[C]; all 16-byte aligned; weight finite and >= 0; anything else is JCK_E_ARG with nothing launched.  One launch, one workgroup
 * per image, 16 bytes per access, a fixed-order reduction: equal bits on every run, and image b does not depend on N. */
int jck_feat_match(int prec, const void* a, const void* f, const float* scale, float slope, float weight, void* g_y, int accumulate,
                   float* fterm, int N, long long M, int C, void* stream);
size_t jck_g1_wgrad_ws_bytes(int B, int CiPad, int Co);
int jck_g1_wgrad(int prec, const void* z, const void* dy, float* ws, size_t ws_bytes, float* grad, int accumulate, int B,
                 int Ci, int CiPad, int Co, void* stream);

/* ---- BatchNorm2d (training mode) + ReLU / LeakyReLU  (model/DCGAN.py:11-24,43-56; aten::native_batch_norm*) ----
 * aux: float[4*C] = scale(gamma*invstd) | shift | mean | invstd, produced by jck_bn_finalize */
int jck_bn_finalize(const float* stats, int slots, float count, const float* gamma, const float* beta,
                    float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum, float eps,
                    float* aux, int C, void* stream);
int jck_bn_act_fwd(int prec, const void* y, const float* aux, float slope, void* a, long long rows, int C, void* stream);
/* Eval-mode BatchNorm (model/DCGAN.py:43-56 under model.eval(); aten::native_batch_norm, training = false): the same aux table from
 * the RUNNING statistics, invstd = 1 / sqrtf(var + eps), scale = gamma * invstd, shift = beta - mean * scale in fp32, each operation
 * rounded once.  One launch for the nlayers <= 8 BatchNorm layers of a network: host arrays of nlayers device pointers / channel
 * counts; aux[k] receives 4 * C[k] floats.  Nothing else is written. */
int jck_bn_eval_aux(int nlayers, const float* const* gamma, const float* const* beta, const float* const* running_mean,
                    const float* const* running_var, float* const* aux, const int* C, float eps, void* stream);
/* sums: scratch of jck_bn_bwd_ws_floats(C) floats (first 2*C = final sum g_z, sum g_z*xhat; no zeroing needed);
 * g_y may alias g_a; dgamma/dbeta (optional) are accumulated into */
size_t jck_bn_bwd_ws_floats(int C);
int jck_bn_act_bwd(int prec, const void* g_a, const void* y, const float* aux, float slope, float* sums, void* g_y,
                   float* dgamma, float* dbeta, long long rows, int C, void* stream);
/* Grouped forms: `groups` independent BatchNorm batches stored back to back - [groups][rows][C] tensors, [groups][slots]
 * statistic slots, [groups][4C] aux, [groups][2C] (mean, unbiased var) records, [groups][jck_bn_bwd_ws_floats(C)] backward
 * workspace.  For the D passes that share weights and run as ONE conv launch (train/dcgan_trainer.py:162,173,118); every
 * group is normalised with its own batch statistics, exactly as in the separate passes.  Only groups < grad_groups add to
 * dgamma / dbeta. */
int jck_bn_finalize_grouped(const float* stats, int slots_per_group, float count, const float* gamma, const float* beta, float eps,
                            float* aux, float* stat_out, int C, int groups, void* stream);
/* jck_bn_finalize_grouped + jck_bn_act_fwd_grouped as ONE launch where the statistics rows are few (each workgroup owns a 64-channel
 * slice and sums that slice's rows itself; otherwise the two launches are issued): a = act(scale * y + shift) with the batch
 * statistics of each group, aux [groups][4C] and stat_out [groups][2C] (may be NULL) written as jck_bn_finalize_grouped writes
 * them; running_mean / running_var / nbt (may be NULL; groups == 1 only) updated as jck_bn_finalize updates them
 * (aten::native_batch_norm + the activation, model/DCGAN.py:30-33,62-65). */
int jck_bn_fwd(int prec, const void* y, const float* stats, int slots_per_group, float count, const float* gamma, const float* beta,
               float eps, float slope, void* a, float* aux, float* stat_out, float* running_mean, float* running_var, int64_t* nbt,
               float momentum, long long rows_per_group, int C, int groups, void* stream);
int jck_bn_act_fwd_grouped(int prec, const void* y, const float* aux, float slope, void* a, long long rows_per_group, int C,
                           int groups, void* stream);
int jck_bn_act_bwd_grouped(int prec, const void* g_a, const void* y, const float* aux, float slope, float* sums, void* g_y,
                           float* dgamma, float* dbeta, long long rows_per_group, int C, int groups, int grad_groups, void* stream);
/* Resident form of jck_bn_act_bwd_grouped (round 4; csrc/bnres.hpp): ONE launch; one workgroup per CU keeps its share of a
 * group's (g_a, y) in registers across a grid barrier, so every tensor byte is read once (HBM passes 5 -> 3, launches 3 -> 1).
 * Same arguments and results (summation order differs: fp32 rounding), plus sync_ws = jck_grid_sync_bytes() bytes of device
 * memory zeroed ONCE by the caller and used by no two launches at the same time (the launch occupies every CU: one stream).
 * Falls back to jck_bn_act_bwd_grouped when the layer does not fit the chip's register file, for fp32, for C < 64, with
 * sync_ws == NULL or JCK_BN_RES=0.  jck_grid_sync_error: 1 if a barrier timed out (results invalid; re-zero sync_ws). */
size_t jck_grid_sync_bytes(void);
int jck_grid_sync_error(const void* sync_ws);
int jck_bn_act_bwd_res(int prec, const void* g_a, const void* y, const float* aux, float slope, float* sums, void* g_y,
                       float* dgamma, float* dbeta, long long rows_per_group, int C, int groups, int grad_groups, void* sync_ws,
                       void* stream);
/* The plan jck_bn_act_bwd_res follows for these arguments when it is given a sync_ws (host only, no launch): returns 1 and fills
 * nch (16-byte chunks per thread and group: 1, 2, 4, 8 or 16), ng (groups resident together; groups > ng go through several
 * passes and barrier generations) and nb (workgroups; a pass covers nb / (C / 64) * 64 rows per chunk), each pointer optional; returns
 * 0 where that call falls back to jck_bn_act_bwd_grouped.  Follows jck_tune("bn_res", ...) / JCK_BN_RES. */
int jck_bn_res_plan(int prec, long long rows_per_group, int C, int groups, int* nch, int* ng, int* nb);
/* jck_conv_down / jck_conv_up with the forward statistics laid out per BatchNorm group of `group_images` images
 * (N % group_images == 0): *stats_slots rows, the first *stats_slots / (N / group_images) of them belong to group 0, and so
 * on - what jck_bn_finalize_grouped reads.  Large launches write one row per (workgroup, group) instead of one per (tile, wave). */
int jck_conv_down_grouped(int prec, const void* big, const void* w, void* small_out, float* stats, int* stats_slots, int N, int Hb,
                          int Wb, int Cb, int Cs, int group_images, void* stream);
int jck_conv_up_grouped(int prec, const void* small_in, const void* w, void* big_out, float* stats, int* stats_slots, int N, int Hs,
                        int Ws, int Cs, int Cb, int group_images, void* stream);
/* ---- images, noise, heads, loss ----------------------------------------------------------------------------- */
/* out NHWC4 T = keep*img + mix*noise (NCHW fp32 inputs; noise may be NULL)   train/dcgan_trainer.py:157-160 */
int jck_img_prep(int prec, const float* img_nchw, const float* noise_nchw, float keep, float mix, void* out, int N, int HW,
                 void* stream);
/* Device-resident input pipeline: gathers B images by index from a uint8 dataset [Ntot][3][Hs][Ws] kept in HBM (idx NULL:
 * the first B) and applies the reference's transform chain on the fly - Resize(2x) exactly as PIL's bilinear upscale
 * (horizontal then vertical pass, each rounded to uint8), ToTensor, Normalize(0.5,0.5)
 * (preprocess/dcgan_data_preprocessor.py:38-43) - then the instance-noise mix keep*x + mix*noise
 * (train/dcgan_trainer.py:160).  out_nhwc4 [B][2Hs][2Ws][4] (element type of prec) and/or out_nchw fp32 [B][3][2Hs][2Ws]
 * (the transformed image without noise); either may be NULL. */
int jck_img_prep_u8(int prec, const unsigned char* data, const int64_t* idx, const float* noise, float keep, float mix,
                    void* out_nhwc4, float* out_nchw, int B, int Hs, int Ws, void* stream);
/* The same pipeline for any source size: Resize((S, S)) of an Hs x Ws image exactly as PIL.Image.resize(BILINEAR) computes it
 * (what transforms.Resize does to a PIL image) - a horizontal and then a vertical pass of fixed-point taps, each rounded to uint8 -
 * then ToTensor, Normalize(0.5, 0.5) and the noise mix as above.  S = 64 or 128, 1 <= Hs, Ws <= JCK_RESIZE_MAX_SRC.
 *
 * The taps come from a table that the HOST builds (no device call, works without a GPU) and the caller copies to the device once
 * per geometry.  jck_resize_taps_bytes: its size in bytes, or JCK_E_ARG (negative) for an unsupported geometry.
 * jck_resize_taps_build fills host_buf (that many bytes) with int32 words:
 *   [0..7]   header: JCK_RESIZE_TAPS_MAGIC, Hs, Ws, S, KX, KY, 0, 0       (KX, KY: taps per output column / row, see below)
 *   x axis (source length L = Ws, K = KX), then y axis (L = Hs, K = KY), each (2 + K) * S words:
 *     lo[S]      first source index of output o
 *     cnt[S]     taps of output o, 1 <= cnt <= K, lo + cnt <= L
 *     k[K][S]    k[j][o] = weight of source index lo[o] + j in units of 2^-22 (0 for j >= cnt[o]); tap-major, so neighbouring
 *                outputs read neighbouring words
 *   with, in IEEE double and in this order, never contracted: scale = L / S, support = max(scale, 1), K = (int)ceil(support) * 2 + 1,
 *   center = (o + 0.5) * scale, lo = max((int)(center - support + 0.5), 0), cnt = min((int)(center + support + 0.5), L) - lo,
 *   w_j = max(1 - |(j + lo - center + 0.5) * (1 / support)|, 0) divided by their sum, k_j = (int)(0.5 + w_j * 2^22).
 *   out[o] = clip((2^21 + sum_j k_j * src[lo + j]) >> 22, 0, 255); an axis with L == S has the single weight 2^22.
 *
 * jck_img_prep_u8_any: data uint8 [Ntot][3][Hs][Ws]; idx int64 [B] or NULL (the first B); flip uint8 [B] or NULL, non-zero = the
 * image is mirrored left-right in the source (column x reads Ws-1-x) before the resize; noise fp32 [B][3][S][S] or NULL; rng device
 * uint32[4] or NULL (in-kernel Philox noise keyed on the output pixel, as jck_img_prep_u8_rng; noise wins when both are given);
 * out_nhwc4 [B][S][S][4] T and / or out_nchw fp32 [B][3][S][S] (the transformed image without noise), either may be NULL;
 * taps_dev: the table above in device memory.  A table built for another geometry leaves the outputs untouched.  One workgroup
 * per (image, band of output rows): horizontal pass of the band's source rows into LDS, vertical pass out of it; integer
 * arithmetic up to the uint8 result, no atomics.  At 32x32 -> 64 the result is jck_img_prep_u8's bit for bit. */
#define JCK_RESIZE_MAX_SRC 1024
#define JCK_RESIZE_TAPS_MAGIC 0x7a736572
long long jck_resize_taps_bytes(int Hs, int Ws, int S);
int jck_resize_taps_build(int Hs, int Ws, int S, void* host_buf);
int jck_img_prep_u8_any(int prec, const unsigned char* data, const int64_t* idx, const unsigned char* flip, const float* noise,
                        const unsigned* rng, int tensor_id, float keep, float mix, void* out_nhwc4, float* out_nchw, int B, int Hs,
                        int Ws, int S, const void* taps_dev, void* stream);
/* The same transform of a BOX of the source: PIL.Image.crop((x0, y0, x0 + Wc, y0 + Hc)).resize((S, S), BILINEAR) - the resize of
 * the cropped array, not Pillow's resize(box=...) - then ToTensor, Normalize and the noise mix as above.  The box is Hc x Wc source
 * pixels with its top-left corner at (y0, x0): 1 <= Hc <= Hs, 1 <= Wc <= Ws, 0 <= y0 <= Hs - Hc, 0 <= x0 <= Ws - Wc.  taps_dev is
 * the table of jck_resize_taps_build(Hc, Wc, S); a flip mirrors inside the box (box column x reads x0 + Wc - 1 - x).  origin:
 * device int32 [B][2] = (y0, x0) per image, or NULL for the scalar (y0, x0) of the call.  A scalar origin outside its range is
 * JCK_E_ARG; per-image origins cannot be checked without a sync, so the kernel clamps each to its range and no origin makes it read
 * outside its image.  Every other argument, refusal and the arithmetic are jck_img_prep_u8_any's: a whole-image box gives its bits.
 * The kernel is jck_img_prep_u8_any's with the corner added to its addresses.
 * jck_resize_lds_bytes: the dynamic LDS in bytes that either launch takes for Hs source rows (of the image, or of the box; never
 * more than 65536), and through the pointers that are not NULL the output rows per workgroup and the source rows they can touch;
 * host arithmetic only.  JCK_E_ARG (negative) for an unsupported geometry. */
long long jck_resize_lds_bytes(int Hs, int S, int* band, int* rows);
int jck_img_prep_u8_box(int prec, const unsigned char* data, const int64_t* idx, const unsigned char* flip,
                        const int* origin /* device int32 [B][2] = (y0, x0) per image, or NULL */, const float* noise,
                        const unsigned* rng, int tensor_id, float keep, float mix, void* out_nhwc4, float* out_nchw,
                        int B, int Hs, int Ws, int Hc, int Wc, int y0, int x0 /* used when origin is NULL */, int S,
                        const void* taps_dev /* table of (Hc, Wc, S) */, void* stream);
/* Evaluation branch (train/dcgan_trainer.py:202-206, train/cgan_trainer.py:227-231): out = (resize(pre_scale*in + pre_shift,
 * [OH,OW]) - mean[c]) / std[c], bilinear with align_corners = False exactly as aten::upsample_bilinear2d (what
 * torchvision.transforms.functional.resize does to a tensor; an upscale, so antialiasing is moot).  NCHW fp32 in / out;
 * mean / std: device float[C]. */
int jck_resize_norm(const float* in, float* out, int N, int C, int H, int W, int OH, int OW, float pre_scale, float pre_shift,
                    const float* mean, const float* stdv, void* stream);
int jck_nhwc4_to_nchw(int prec, const void* in, float* out_nchw, int N, int HW, void* stream);
/* NHWC4 image in [-1, 1] (the tanh of model/DCGAN.py:66) -> packed uint8 [N][HW][3]:
 * u8 = (unsigned char)(fminf(fmaxf(x * 127.5f + 127.5f, 0.f), 255.f) + 0.5f), product and sum rounded separately.  NaN gives 0: that
 * is what fmaxf returns for it.  HW % 4 == 0; `in` 16-byte, the output 4-byte aligned. */
int jck_img_to_u8(int prec, const void* in, unsigned char* out_u8_nhwc, int N, int HW, void* stream);
/* out = keep*x + mix*noise for an NHWC4 x                                      train/dcgan_trainer.py:171 */
int jck_axpy_noise(int prec, const void* x, const float* noise_nchw, float keep, float mix, void* out, int N, int HW,
                   void* stream);
/* x_hat = alpha*a + (1-alpha)*b                                                 train/dcgan_trainer.py:111-112 */
int jck_interp(int prec, const void* a, const void* b, const float* alpha, void* out, int N, int HW, void* stream);
/* jck_axpy_noise (noise_nchw given) or jck_axpy_noise_rng (rng given; exactly one of the two) followed by
 * jck_interp(real, out, alpha) -> xhat, as one launch with the same results bit for bit (train/dcgan_trainer.py:171 then :111-113). */
int jck_mix_interp(int prec, const void* x, const float* noise_nchw, const unsigned* rng, int tensor_id, float keep, float mix, void* out,
                   const void* real, const float* alpha, void* xhat, int N, int HW, void* stream);
/* scal[slot*scal_ld + n] = (||g[n]||_2 - 1)^2 (plain store per image; the caller sums the row in a fixed order - no float
 * atomics, so the logged penalty is bitwise reproducible); norms[n] optional     train/dcgan_trainer.py:125-126 */
int jck_gp_norm(int prec, const void* g, int N, int HW, float* scal, int slot, int scal_ld, float* norms, void* stream);
/* g_out = scale * g * (1 - y^2)                                                 tanh backward, model/DCGAN.py:66 */
int jck_tanh_bwd(int prec, const void* g, const void* y, float scale, void* out, long long numel, void* stream);
/* D head: logit = <a4[n], wp>, p = sigmoid (model/DCGAN.py:34), BCELoss with the -100 clamp (train/dcgan_trainer.py:64,163);
 * mode 0: ds = dLoss/dlogit for mean BCE against `target`; scal[slot_loss*scal_ld + n] = loss_n; mode 1: ds = p(1-p) (GP
 * pass).  scal[slot_p*scal_ld + n] = p_n.  slot < 0 disables.  `scal` is a per-image table [slots][scal_ld >= B]: plain
 * stores, summed in a fixed order by the step tail (no float atomics anywhere on the path). */
int jck_head_fwd(int prec, const void* a4, const float* wp, const float* bias /* device scalar or NULL */, int B, int K,
                 float target, int mode, float* prob, float* ds, float* scal, int slot_loss, int slot_p, int scal_ld, void* stream);
/* The head at inference: logit[n] = <x[n,:], w> (+ bias[0]), prob[n] = 1 / (1 + expf(-logit)) (prob may be NULL); x [B][K] of the
 * element type, w fp32 [K], both 16-byte aligned, K % 8 == 0.  One workgroup per row, a fixed-order reduction (the dot product of
 * jck_head_fwd), no loss, no gradient, no scalar slots: a row's numbers do not depend on B. */
int jck_score_head(int prec, const void* x, const float* w, const float* bias /* device scalar or NULL */, int B, int K,
                   float* logit, float* prob /* or NULL */, void* stream);
/* Discriminator features: a, NHWC [N,H,H,C] of the precision's storage type (bf16, or fp32 for f32 / bf16x3), pooled to a grid x grid
 * raster of w x w windows (w = H / grid).  For every image b, grid cell (gy,gx) and channel c
 *   out[b*ld + col0 + (gy*grid + gx)*C + c] = pool over the window of a[b, gy*w+dy, gx*w+dx, c],  as fp32
 * - cell-major, channel-minor: F.adaptive_max_pool2d(a_nchw, grid).permute(0, 2, 3, 1).flatten(1).
 * mode 0: max (a NaN in the window gives NaN, as torch's max_pool2d; an all -inf window gives -inf)
 * mode 1: mean = (fp32 sum in row-major window order) * (1 / w^2)
 * grid in {1,2,4}, H a multiple of grid, C a multiple of 8, a 16-byte aligned, out, col0 and ld such that every row's column block
 * is 16-byte aligned and lies inside the row; anything else: JCK_E_ARG with a message and no launch.  Columns outside
 * [col0, col0 + grid*grid*C) are not written.  One lane per (image, cell, 16 bytes of channels), 16-byte loads and stores, no LDS, no
 * atomics: row b does not depend on N. */
int jck_grid_pool(int prec, const void* a, int N, int H, int C, int grid, int mode, float* out, long long ld, long long col0,
                  void* stream);
/* G (<= 4) batches of B rows stacked in a4 / prob / ds (the real | fake | penalty groups of a batched D pass), each with its own
 * target, mode and scalar slots, in one launch; the scalar table is indexed by the row inside its group */
int jck_head_fwd_grouped(int prec, const void* a4, const float* wp, const float* bias, int B, int K, int G, const float* targets,
                         const int* modes, float* prob, float* ds, float* scal, const int* slot_loss, const int* slot_p,
                         int scal_ld, void* stream);
/* floats of workspace for the weight-gradient partial rows of jck_head_bwd / jck_head_bwd_conv (K = 16*C there) */
size_t jck_head_bwd_ws_floats(int K);
/* g_a4[n][k] = ds[n]*wp[k];  dwp[k] (+)= sum_n ds[n]*a4[n][k] through `ws` (partial rows summed in order: deterministic) */
int jck_head_bwd(int prec, const float* ds, const float* wp, const void* a4, int B, int K, void* g_a4, float* dwp,
                 int accumulate, float* ws, void* stream);
/* grad[1][C][4][4] (+)= dwp (packed (h,w,c) order) */
int jck_head_unpack_grad(const float* dwp, int C, float* grad, int accumulate, void* stream);
/* D.conv5 backward in one launch (DCGAN engine path): g_a4[n][k] = ds[n]*wp[k] (skipped when g_a4 is NULL) and
 * grad[c][t] += sum_n ds[n]*a4[n][t*C+c] into the PyTorch-layout gradient of conv5.weight [1][C][4][4] (skipped when grad
 * is NULL): 16 partial rows in `ws` (jck_head_bwd_ws_floats(16*C) floats), summed in order by a second small launch - no
 * float atomics.  Replaces aten::convolution_backward behind model/DCGAN.py:26 in train/dcgan_trainer.py:164,175,187. */
int jck_head_bwd_conv(int prec, const float* ds, const float* wp, const void* a4, int B, int C, void* g_a4, float* grad,
                      float* ws, void* stream);
/* the same over B rows plus, in the same launch, the input gradient alone of the B_more rows stored behind them (ds, a4 and g_a4
 * hold B + B_more rows; the weight gradient sums the first B only): the loss groups and the penalty group of one batched D pass. */
int jck_head_bwd_conv2(int prec, const float* ds, const float* wp, const void* a4, int B, int B_more, int C, void* g_a4, float* grad,
                       float* ws, void* stream);

/* ---- CGAN pieces (model/CGAN.py:79-162, train/cgan_trainer.py:173-213) ---------------------------------------------
 * Linear layers run on the gather-GEMM kernels as plain row-major products; our activation order is NHWC, so the
 * first permC*permHW weight columns (the flattened conv features, NCHW order in the reference, model/CGAN.py:119-120)
 * are permuted when packing and un-permuted when the gradient is written back. */
int jck_pack_linear(int prec, const float* w, int N, int K, int rows, int cols, int transpose, int permC, int permHW, void* wp,
                    void* stream);
/* out[B][NStore] = x[B][Kpad] * wp^T (+ bias); ksplit > 1: fp32 partial slabs [ksplit][B][NStore] for jck_linear_finish */
int jck_linear_fwd(int prec, const void* x, const void* wp, const float* bias, void* out, int B, int Kpad, int N, int NStore,
                   int ksplit, void* stream);
/* h = sum of slabs + bias; hd = h * mask * scale (nn.Dropout, model/CGAN.py:105); h or hd may be NULL */
int jck_linear_finish(int prec, const float* slab, int Z, const float* bias, const float* mask, float scale, void* h, void* hd,
                      int B, int N, void* stream);
size_t jck_linear_wgrad_ws_bytes(int B, int Kpad, int N);
int jck_linear_wgrad(int prec, const void* gy, int ldgy, const void* x, int Kpad, float* ws, size_t ws_bytes, float* gradp,
                     int accumulate, int B, int N, void* stream);
int jck_unperm_linear_grad(const float* gp, int N, int K, int ldp, int permC, int permHW, float* grad, int accumulate, void* stream);
/* label path: e = LeakyReLU(Linear(100,200)(onehot.float())) written into columns [col0, col0+NO) of cbuf (model/CGAN.py:111) */
int jck_label_embed_fwd(int prec, const int64_t* labels, const float* W, const float* b, float slope, int B, int NI, int NO,
                        void* cbuf, int ld, int col0, float* pre, void* stream);
int jck_label_embed_bwd(int prec, const void* gc, int ld, int col0, const float* pre, const int64_t* labels, float slope, int B,
                        int NI, int NO, float* dW, float* db, void* stream);
/* `_tiled`: the B rows are label_period-row batches stacked on top of each other that share one [label_period][NI] label
 * tensor - the real | fake | penalty groups of a CGAN step (train/cgan_trainer.py:181-203); label_period 0 = one label row per row */
int jck_label_embed_fwd_tiled(int prec, const int64_t* labels, const float* W, const float* b, float slope, int B, int NI, int NO,
                              void* cbuf, int ld, int col0, float* pre, int label_period, void* stream);
int jck_label_embed_bwd_tiled(int prec, const void* gc, int ld, int col0, const float* pre, const int64_t* labels, float slope,
                              int B, int NI, int NO, float* dW, float* db, int label_period, void* stream);
/* torch.cat([flatten(a4), e], 1) (model/CGAN.py:117-120) and its backward split */
int jck_concat_rows(int prec, const void* a4, int K0, void* cbuf, int ld, int B, void* stream);
int jck_split_rows(int prec, const void* gc, int ld, int K0, void* ga4, int B, void* stream);
int jck_dropout(int prec, const void* x, const float* mask, float scale, void* y, long long n, void* stream);
int jck_colsum(int prec, const void* g, int B, int N, int ld, float* db, void* stream);
int jck_sum_vec(const float* x, int n, float* out, void* stream);
/* G input [z | one-hot] (model/CGAN.py:154-155) */
int jck_cgan_z(int prec, const float* z, const int64_t* labels, int B, int NZ, int NL, int CiPad, void* out, void* stream);
/* back-propagated gradient penalty (train/cgan_trainer.py:200-203): u = dL/dg, second-order BatchNorm and head terms;
 * the closed form is derived and checked against autograd in tests/test_gp_double_backward_math.py */
int jck_gp_grad(int prec, const void* g, const float* norms, float coef, int N, int HW, void* u, void* stream);
/* ws: float[B + jck_head_bwd_ws_floats(K)] */
int jck_gp_head2(int prec, const void* ughd, const float* w2, const float* prob, int B, int K, float* rs, float* dw2, float* ws,
                 void* stream);
/* DCGAN's head step of the back-propagated penalty (conv5 = one dot product per image over K = 16*C, packed (h,w,c) order; the
 * closed form is checked in tests/test_dcgan_gp_math.py), with v4 the adjoint at a4 from the v-chain and prob the penalty pass's
 * probabilities:  rs[n] = <v4[n], wp> (1-2p) p(1-p);  g_a4[n][k] = rs[n] wp[k] in the storage type (skipped when NULL; may alias v4,
 * not a4);  grad[c][t] += sum_n p(1-p) v4[n][t*C+c] + rs[n] a4[n][t*C+c] into the PyTorch-layout gradient of conv5.weight
 * [1][C][4][4] (skipped when NULL; always accumulates; rows summed in a fixed order, no float atomics).  Two launches;
 * ws: jck_gp_head2_conv_ws_floats(B) floats. */
size_t jck_gp_head2_conv_ws_floats(int B);
int jck_gp_head2_conv(int prec, const void* v4, const void* a4, const float* wp, const float* prob, int B, int C, float* rs,
                      void* g_a4, float* grad, float* ws, void* stream);
/* Second-order BatchNorm steps of the back-propagated penalty at one layer (closed form: tests/bn_ref.py, held to fp64 autograd in
 * tests/test_bn2_math.py; aux, y as in the first backward, gy and s1 = {sum g_z, sum g_z*xhat} what jck_bn_act_bwd left).
 * jck_bn2_vchain: u (may alias v) and xdir from the adjoint v of gy; ws[0..3C) = {sum v, sum v*xhat, sum v*gy} on return (keep it
 * for jck_bn2_reverse); dgamma (optional) += sum v*gy / gamma.  g_z is reconstructed as gy / (gamma / sigma): gamma ≠ 0.
 * jck_bn2_reverse: uy from the adjoint ua of the activation, xdir and vsums = the v-chain's ws; ws[0..4C) = {sum uz, sum uz*xhat,
 * sum xdir, sum xdir*xhat}; dgamma += sum uz*xhat and dbeta += sum uz when BOTH are given (neither is written otherwise).
 * ws: jck_bn2_ws_floats(C) floats each, no zeroing needed; C a power of two in [8, 2048]. */
size_t jck_bn2_ws_floats(int C);
int jck_bn2_vchain(int prec, const void* v, const void* y, const void* gy, const float* aux, const float* s1, const float* gamma,
                   float slope, float* ws, void* u, void* xdir, float* dgamma, long long rows, int C, void* stream);
int jck_bn2_reverse(int prec, const void* ua, const void* y, const void* xdir, const float* aux, const float* gamma,
                    const float* vsums, float slope, float* ws, void* uy, float* dgamma, float* dbeta, long long rows, int C,
                    void* stream);

/* ---- optimiser (torch.optim.Adam as built at train/dcgan_trainer.py:61-62) over a flat fp32 arena ---------- */
int jck_adam(float* p, const float* g, float* m, float* v, long long n, double lr, double beta1, double beta2, double eps,
             int step, float grad_scale, void* stream);
/* The same update with an exponential moving average of the parameters advanced in the same launch.  The reference samples and
 * checkpoints the raw generator (train/dcgan_trainer.py:199-200,86-91); the averaged generator is the usual remedy for its
 * oscillation against D and an opt-in addition here.  ema [n]: e <- lerp(e, p_new, ema_weight) with ATen's two lerp branches
 * (ema_weight = 1 - decay in [0, 1]; 1 gives e = p_new exactly).  skip_if: device word or NULL; non-zero leaves p, m, v and ema
 * untouched.  p, m, v come out bitwise as jck_adam leaves them. */
int jck_adam_ema(float* p, const float* g, float* m, float* v, float* ema, long long n, double lr, double beta1, double beta2,
                 double eps, int step, float grad_scale, float ema_weight, const unsigned* skip_if, void* stream);
/* jck_adam (ema != NULL: jck_adam_ema) over the arena AND the packed operands of the conv weights inside it, written by the same
 * launch from the registers that hold the new weights: what the engine's optimiser phases run.  Job i packs the weight at element
 * w_off[i] (% 4 == 0; jobs in arena order, the forms of one weight next to each other) into wp[i], element type by prec:
 * kind 0 = jck_pack_down(Cs = a, Cb = b), 1 = jck_pack_up (Cb > 4), 2 = jck_pack_up (Cb <= 4), 3 = jck_pack_g1(Ci = a, Co = b,
 * CiPad = a rounded up to 128), 4 = jck_pack_head(C = a).  Padding rows and channels of the operands are not written.  All arenas
 * 16-byte aligned; at most 12 jobs.  skip_if non-zero leaves arenas and operands untouched.  Every value comes out bitwise as
 * jck_adam / jck_adam_ema followed by the jck_pack_* calls leave it. */
int jck_adam_pack(int prec, float* p, const float* g, float* m, float* v, float* ema, long long n, int njobs, const int* kind,
                  const long long* w_off, void* const* wp, const int* a, const int* b, double lr, double beta1, double beta2, double eps,
                  int step, float grad_scale, float ema_weight, const unsigned* skip_if, void* stream);

/* ---- whole-step engine (train/dcgan_trainer.py:155-189 as one native schedule) --------------------------- */
typedef struct jck_engine jck_engine;
/* family 0 = DCGAN, 1 = CGAN.  Layout queries let the host build flat parameter arenas with the reference's state-dict order. */
int jck_engine_create(jck_engine** out, int family, int prec, int batch);
/* image_size 64 = the reference's nets (model/DCGAN.py:10-27,42-59); 128 = one more stride-2 stage at the deep end (D 3-64-128-
 * 256-512-1024-1, G 100-1024-...-64-3; DCGAN only) for BASELINE.json configs[4] - no reference behaviour exists for it. */
int jck_engine_create_sized(jck_engine** out, int family, int prec, int batch, int image_size);
/* flags (OR-ed; 0 = jck_engine_create_sized):
 *   JCK_ENGINE_GP_BACKWARD - DCGAN: back-propagate the gradient penalty as CGAN does (the reference only logs it,
 *     train/dcgan_trainer.py:178-179): PHASE_D_GP adds 10 * d(penalty)/d(theta_D) to D's gradient arena and PHASE_GP_ONLY leaves
 *     d(penalty)/d(theta_D) there; D's gradients are final only after PHASE_D_GP (no PHASE_D_LOSS_A / _B split, grad_tail -1).
 *     The workspace grows by the second-order buffers.  CGAN ignores the flag. */
#define JCK_ENGINE_GP_BACKWARD 1u
int jck_engine_create_ex(jck_engine** out, int family, int prec, int batch, int image_size, unsigned flags);
int jck_engine_image_size(const jck_engine*);
/* layout queries of a created engine (its own image size); same meaning as the family-keyed ones below */
int jck_engine_num_tensors_of(const jck_engine*, int net);
int jck_engine_tensor_info_of(const jck_engine*, int net, int idx, char* name, int name_cap, int* kind, long long* offset,
                              long long* numel, int* shape4);
long long jck_engine_arena_numel_of(const jck_engine*, int net, int which);
void jck_engine_destroy(jck_engine*);
int jck_engine_num_tensors(int family, int net /*0=G,1=D*/);
/* kind: 0 = parameter, 1 = running_mean, 2 = running_var ; name buffer gets the state-dict key */
int jck_engine_tensor_info(int family, int net, int idx, char* name, int name_cap, int* kind, long long* offset,
                           long long* numel, int* shape4);
size_t jck_engine_workspace_bytes(const jck_engine*);
/* arenas: params/grads/m/v are flat fp32 of jck_engine_arena_numel(net, 0); bn = running stats arena (kind 1,2);
 * nbt = int64[4] per net */
long long jck_engine_arena_numel(int family, int net, int which /*0 params, 1 bn buffers*/);
/* workspace: jck_engine_workspace_bytes(e) bytes of device memory, 256-byte aligned.  The workspace's contents on entry do not
 * matter; bind clears it (all of it, synchronously, once per call - no step pays for it); between bind and destroy it belongs to
 * the engine: the kernels rely on the zeros bind left wherever they write only part of a buffer (padding rows / columns of the
 * packed operands, of G.conv1's operand rows and of CGAN's concat buffers, the grid-barrier words), so a caller reads it
 * (jck_engine_tensor, jck_engine_scalars) and never writes it.  Binding a bound engine again is allowed (no step in flight): the
 * workspace is cleared again - call jck_engine_repack for both networks afterwards -, the arenas are not touched. */
int jck_engine_bind(jck_engine*, void* workspace, size_t ws_bytes, float* g_params, float* g_grads, float* g_m, float* g_v,
                    float* g_bn, int64_t* g_nbt, float* d_params, float* d_grads, float* d_m, float* d_v, float* d_bn,
                    int64_t* d_nbt);
/* re-derive the bf16 GEMM operand planes from the fp32 parameters (after init / load_state_dict) */
int jck_engine_repack(jck_engine*, int net, void* stream);
/* phases of one step; between them the host may all-reduce the grads arenas (data parallel).
 *   PHASE_D_LOSS : zero D grads; D(real'), D(fake): forward+backward; G forward   (dcgan_trainer.py:155-176)
 *   PHASE_D_GP   : gradient-penalty pass (value only in DCGAN)                     (:178-179)
 *   PHASE_D_STEP : Adam on D, repack D                                             (:180)
 *   PHASE_G_LOSS : zero G grads; D(fake) with the new D; backward into G           (:182-188)
 *   PHASE_G_STEP : Adam on G, repack G, finalise the scalars                       (:189) */
#define JCK_PHASE_D_LOSS 0
#define JCK_PHASE_D_GP 1
#define JCK_PHASE_D_STEP 2
#define JCK_PHASE_G_LOSS 3
#define JCK_PHASE_G_STEP 4
/* PHASE_D_LOSS = PHASE_D_REAL (:155-165, needs no G) followed by PHASE_D_FAKE (:168-176 + start of the penalty pass).
 * Issued separately, D_REAL of step k+1 may run on another stream beside the G phase of step k: it uses its own
 * activation set, and scalar accumulators / BatchNorm records are double-buffered on the parity of `step`. */
#define JCK_PHASE_D_REAL 5
#define JCK_PHASE_D_FAKE 6
/* PHASE_D_REAL_FWD (DCGAN, batched schedule): the forward half of D(real) of step k+1 only - input transform, instance noise,
 * conv stack with its BatchNorm statistics (:160-162) - issued with the inputs of step k+1 between PHASE_G_LOSS and
 * PHASE_G_STEP of step k, i.e. while G's gradient all-reduce of step k is in flight (data parallel): it needs D's weights
 * (final since PHASE_D_STEP of step k) and nothing of G.  PHASE_D_LOSS of step k+1 then skips that part and runs
 * [fake | penalty] as one 2B forward behind it; everything else (heads, losses, the 3B backward) is unchanged, so results
 * are bitwise those of the plain order.  Returns JCK_E_ARG when the engine's schedule has no such split (CGAN, per-pass). */
#define JCK_PHASE_D_REAL_FWD 7
/* PHASE_D_LOSS = PHASE_D_LOSS_A + PHASE_D_LOSS_B (DCGAN, batched schedule; data parallel).  After _A the tail of D's gradient
 * arena [jck_engine_grad_tail() .. end) - conv4.weight, norm4.*, conv5.weight, 76 % of its bytes - is final in stream order:
 * the caller starts its all-reduce, issues _B (the remaining ~0.5 ms of the backward pass), then all-reduces the head of the
 * arena.  Same kernels in the same order on every tensor: bitwise the results of PHASE_D_LOSS. */
#define JCK_PHASE_D_LOSS_A 8
#define JCK_PHASE_D_LOSS_B 9
/* The gradient penalty alone, for a caller that keeps the reference's loop on the HIP modules (compute_gradient_penalty,
 * train/dcgan_trainer.py:110-127, train/cgan_trainer.py:114-131): real_nchw = real_data and noise_real = fake_data, both
 * [B,3,S,S] fp32 taken as they are, alpha [B] (CGAN: labels, drop_mask[2]).  Afterwards jck_engine_tensor("norms") holds the
 * per-image gradient norms - the penalty is mean((norm - 1)^2) - and, CGAN, D's gradient arena holds d(penalty)/d(theta_D)
 * (cleared first; lambda = 1): the double backward the reference obtains with create_graph=True, in closed form
 * (hipgan/functional.py: gradient_penalty).  It overwrites real_noisy: a PHASE_D_REAL_FWD enqueued ahead for the next step is
 * waited for and abandoned first (jck_engine_drop_prefetch), and that step's D phase computes D(real) itself. */
#define JCK_PHASE_GP_ONLY 10
/* OR-ed into PHASE_D_LOSS / PHASE_D_GP (CGAN): the caller reads nothing of D's gradient arena before PHASE_D_STEP (no
 * all-reduce in between), so the phase need not wait for the weight-gradient stream before it returns.  PHASE_D_STEP then
 * runs Adam over everything but the bottom conv weight - the last product of that stream - while it finishes, and that one
 * tensor behind it.  Any other phase that follows joins first.  Same kernels on the same values: bitwise the plain order. */
#define JCK_PHASE_LAZY_JOIN 0x100
/* OR-ed into any phase: the BatchNorm backward launches of THIS call take the three-launch form instead of the resident
 * (grid-barrier) one.  A resident launch needs every CU of the device: while a collective is in flight (data parallel, N > 1:
 * RCCL's kernel holds CUs until every peer has arrived) its missing workgroups could not be placed and the placed ones would
 * spin at the barrier until its time bound - hipgan/engine.py sets the flag on the phases it issues between the start of an
 * all-reduce and the wait for it (train/dcgan_trainer.py:180,189 are the exchange points).  Same sums in another order: held to
 * the oracle like the resident form. */
#define JCK_PHASE_NO_RESIDENT 0x200
typedef struct jck_step_inputs {
  const float* real_nchw; /* [B,3,64,64] fp32 */
  const float* noise_real; /* [B,3,64,64] N(0,1); NULL (with noise_fake NULL): drawn inside the kernels (jck_engine_set_noise_seed) */
  const float* z;          /* [B,100] N(0,1); NULL: the engine's own draw for this step (jck_engine_set_step, jck_step_rng) */
  const float* noise_fake; /* [B,3,64,64] N(0,1) */
  const float* alpha;      /* [B] U[0,1); NULL: the engine's own draw */
  float lr;
  float grad_scale;        /* 1/world_size when grads were SUM-all-reduced, else 1 */
  int step;                /* 1-based optimiser step (Adam bias correction) */
  /* family 1 (CGAN) only: */
  const int64_t* labels;   /* [B,100] one-hot int64 (preprocess/cgan_data_preprocessor.py:11-16) */
  const float* drop_mask[4]; /* [B,256] 0/1 keep masks of nn.Dropout(0.25) for the 4 D passes (real, fake, GP, G phase); all four
                              * NULL: the engine's own draws.  Masks 0..2 back to back in memory let the head run once over 3B rows */
  /* device-resident dataset (optional; used instead of real_nchw when real_u8 != NULL): uint8 [Ntot,3,32,32] + the batch's
   * indices int64 [B]; the step applies the input transform itself (jck_img_prep_u8) */
  const unsigned char* real_u8;
  const int64_t* real_idx;
  /* any-size dataset (optional; all zero = the 32x32 -> 64 path above): real_u8 is uint8 [Ntot,3,real_h,real_w], real_taps the
   * device copy of jck_resize_taps_build(real_h, real_w, S) for the engine's image size S, real_flip uint8 [B] (or NULL) mirrors
   * images left-right before the resize; the step then applies jck_img_prep_u8_any.  Caller's device memory: the step neither
   * allocates nor copies. */
  int real_h, real_w;
  const unsigned char* real_flip;
  const void* real_taps;
  /* a box of every image (optional; all zero = the whole image, as above): real_box_h x real_box_w source pixels at (real_y0,
   * real_x0), or at real_origin's int32 [B][2] = (y0, x0) per image when that is set; real_taps is then the table of
   * (real_box_h, real_box_w, S) and the step applies jck_img_prep_u8_box. */
  int real_box_h, real_box_w, real_y0, real_x0;
  const int* real_origin;
} jck_step_inputs;
int jck_engine_phase(jck_engine*, int phase, const jck_step_inputs* in, void* stream);
/* device pointer to float[8]: loss_d, loss_g, D(x), D(G(z))_1, D(G(z))_2, gp, loss_real, loss_fake (valid after PHASE_G_STEP) */
/* first element of the gradient-arena tail that PHASE_D_LOSS_A finalises (net 1 = D); -1 when the schedule has no such split */
long long jck_engine_grad_tail(const jck_engine*, int net);
/* PHASE_D_LOSS_A | JCK_PHASE_LAZY_JOIN (DCGAN, data parallel): the phase returns without making its stream wait for the weight-
 * gradient stream (the stall cost more than the early all-reduce hid); the caller starts the tail's all-reduce from ANOTHER stream
 * that it first passes here - it then waits for the tail's last writers on both engine streams. */
int jck_engine_order_after_tail(jck_engine*, void* stream);
/* abandons a PHASE_D_REAL_FWD enqueued ahead for the next step (D's weights are about to be overwritten from outside the step:
 * the replica guard's re-broadcast, load_model): `stream` waits for that forward, the next D phase recomputes it */
int jck_engine_drop_prefetch(jck_engine*, void* stream);
/* after a device synchronisation: JCK_E_HIP if a grid barrier of a resident launch (jck_bn_act_bwd_res) timed out since the last
 * call - that launch went on with incomplete sums, so the step's results are invalid; the engine's optimiser phases read the same
 * word on the device and leave parameters and Adam moments untouched while it is set.  The call re-arms the barrier state. */
int jck_engine_check(jck_engine*);
const float* jck_engine_scalars(const jck_engine*);
const float* jck_engine_scalars_at(const jck_engine*, int step);   /* buffer of the given (1-based) step's parity */
/* G forward only (train/dcgan_trainer.py:199-200, train-mode BN: running stats move); out NCHW fp32 [n,3,64,64].
 * jck_engine_sample_ex(flags = 0, out_u8_nhwc = NULL). */
int jck_engine_sample(jck_engine*, const float* z, const int64_t* labels /* family 1 */, int n, float* out_nchw, void* stream);
/* The same with options, and an optional second output.  flags == 0: train-mode BatchNorm as above.  JCK_SAMPLE_EVAL: the
 * generator as under model.eval() (model/DCGAN.py:42-66 with BatchNorm on its running statistics): one launch folds the layers' aux
 * tables, every ConvTranspose + BatchNorm + ReLU is one launch, each image depends on its own z alone, any 1 <= n <= batch, and
 * neither the running statistics nor num_batches_tracked are written.  out_nchw: fp32 [n,3,S,S] or NULL; out_u8_nhwc: uint8
 * [n,S,S,3] as from the image-to-uint8 kernel above, or NULL. */
#define JCK_SAMPLE_EVAL 1u   /* BatchNorm with the running statistics; no buffer moves */
int jck_engine_sample_ex(jck_engine*, const float* z, const int64_t* labels, int n, unsigned flags, float* out_nchw /* or NULL */,
                         unsigned char* out_u8_nhwc /* or NULL */, void* stream);
/* Latent projection through the frozen generator under model.eval(): for image b, L_b = mean((G(z_b) - t_b)^2) over the 3 S^2
 * real elements, target_nchw fp32 [n,3,S,S] in [-1, 1] on the device (read in place, never rounded), labels fixed (family 1).
 * latent_grad: loss [n] and dz = dL/dz [n,100].  project: `steps` updates of torch.optim.Adam(lr, (0.9, 0.999), 1e-8) on z [n,100]
 * (in, out) minimising L_b + prior * mean_k(z_bk^2), all on the stream without a host synchronisation; m, v [n,100] are the
 * caller's Adam state (zeros and t0 = 0 to begin, the returned state and the updates done so far to continue), loss_hist[s][n]
 * (or NULL) is L before update s.  1 <= n <= batch; row b of every output is bit for bit what a call with that row alone returns.
 * Neither the running statistics nor num_batches_tracked nor any parameter is written.  On a training engine both may be called
 * between two steps: they use buffers that every step rewrites before it reads them, and memory of their own that the first call
 * allocates (so: not inside a graph capture) and jck_engine_destroy frees.  Both forward to the _ex entry points below with
 * weight = NULL, critic_mode = 0, critic_weight = 0 and term = logit = term_hist = NULL: one implementation. */
int jck_engine_latent_grad(jck_engine*, const float* z, const int64_t* labels, const float* target_nchw, int n,
                           float* loss /* [n] */, float* dz /* [n,100] */, void* stream);
int jck_engine_project(jck_engine*, float* z /* in, out */, const int64_t* labels, const float* target_nchw, int n,
                       int steps, float lr, float prior, float* m, float* v /* [n,100], caller-owned */, int t0,
                       float* loss_hist /* [steps][n] or NULL */, void* stream);
/* The same with a per-pixel weight and the eval-mode discriminator as a critic: per image J_b = L_b + term_b + prior * mean_k(z_bk^2),
 * L_b = sum_p w_p sum_c (G(z_b) - t_b)^2 / (3 sum_p w_p) (weight: fp32 [n,S,S] on the device, or NULL for 1; target NULL: L_b = 0,
 * critic only) and term_b = critic_weight * c(D(G(z_b))), c = softplus(-logit) (critic_mode 1, nsgan) or -logit (2, logit); mode 0:
 * no critic.  latent_grad_ex: loss = L [n], term [n] (or NULL), logit [n] (or NULL) and dz = d(L + term)/dz.  project_ex:
 * jck_engine_project on that objective; term_hist[s][n] (or NULL) is term before update s.  With weight NULL and critic_mode 0 both
 * are the entry points above (the products, jck_latent_loss_ex, the projection's backward).  With a critic one evaluation is: the eval generator's products,
 * jck_engine_score's stages and head on its output, jck_critic_ds, the head's input gradient, jck_leaky_affine_bwd at the deepest stage,
 * jck_conv_up_mask per stage down to stage 1, jck_conv_up into an image gradient, jck_latent_loss_ex, then the projection's backward.
 * D's gradients, the image gradient and the critic's rows are ONE allocation that the first call with a critic makes (so: not inside
 * a graph capture) and jck_engine_destroy frees; D's training activations, real_noisy and the head's concat buffer are never used, and
 * nothing of the training state is written.  critic_mode != 0 needs D's packed operands (as jck_engine_score) and, family 1, labels;
 * critic_weight >= 0; target NULL requires a critic: JCK_E_ARG otherwise, nothing launched.  Rows are independent bit for bit. */
int jck_engine_latent_grad_ex(jck_engine*, const float* z, const int64_t* labels, const float* target_nchw /* or NULL */,
                              const float* weight /* or NULL */, int critic_mode, float critic_weight, int n, float* loss /* [n] */,
                              float* term /* [n] or NULL */, float* logit /* [n] or NULL */, float* dz /* [n,100] */, void* stream);
int jck_engine_project_ex(jck_engine*, float* z /* in, out */, const int64_t* labels, const float* target_nchw /* or NULL */, int n,
                          int steps, float lr, float prior, const float* weight /* or NULL */, int critic_mode, float critic_weight,
                          float* m, float* v, int t0, float* loss_hist /* [steps][n] or NULL */, float* term_hist /* [steps][n] or NULL */,
                          void* stream);
/* The same with a feature-matching term on the discriminator's activations: J_b = L_b + term_b + F_b + prior * mean_k(z_bk^2),
 * F_b = feat_weight / M_k * sum over stage k's elements of (a_k(G(z_b)) - a_k(x_b))^2, a_k the LeakyReLU output of D's conv stage k as
 * under model.eval() (what jck_engine_features pools), M_k its elements per image, x = feat_target_nchw (fp32 [n,3,S,S] in [-1, 1] on
 * the device), feat_stage 0 .. NS-1 or -1 for the deepest.  Labels play no part in F.  The term is on iff feat_target_nchw is not NULL
 * and feat_weight > 0; off, both are the _ex entry points bit for bit (which forward here with NULL, -1, 0, NULL: one implementation).
 * latent_grad_fm: fterm [n] (or NULL) = F, dz = d(L + term + F)/dz.  project_fm: fterm_hist[s][n] (or NULL) is F before update s.
 * Once per call the target's activation a_k(x) is computed (the input transform, the stages 0..k) and kept in a buffer of its own.
 * One evaluation without a critic: the eval generator's products, D's stages 0..k on its output, jck_feat_match into the gradient at
 * stage k's product, jck_conv_up_mask from stage k down to stage 1, jck_conv_up into the image gradient, jck_latent_loss_ex, the
 * projection's backward - the head and the stages above k do not run.  With a critic: the _ex chain from the head, and jck_feat_match
 * (accumulate 1) where the gradient at stage k's product has just been written.  The feature buffer (batch images of stage 0's size
 * and a row of floats) is ONE allocation made by the first call with a feature term (so: not inside a graph capture) and freed by
 * jck_engine_destroy; otherwise the contract of the _ex entry points.  JCK_E_ARG, nothing launched: feat_weight negative or not
 * finite, feat_weight > 0 without a feature target, feat_stage outside [-1, NS-1], a feature term without D's packed operands,
 * neither a target nor a critic nor a feature term, critic_mode outside 0..2. */
int jck_engine_latent_grad_fm(jck_engine*, const float* z, const int64_t* labels, const float* target_nchw /* or NULL */,
                              const float* weight /* or NULL */, int critic_mode, float critic_weight, int n, float* loss /* [n] */,
                              float* term /* [n] or NULL */, float* logit /* [n] or NULL */, float* dz /* [n,100] */, void* stream,
                              const float* feat_target_nchw /* or NULL */, int feat_stage, float feat_weight, float* fterm /* [n] or NULL */);
int jck_engine_project_fm(jck_engine*, float* z /* in, out */, const int64_t* labels, const float* target_nchw /* or NULL */, int n,
                          int steps, float lr, float prior, const float* weight /* or NULL */, int critic_mode, float critic_weight,
                          float* m, float* v, int t0, float* loss_hist /* [steps][n] or NULL */, float* term_hist /* [steps][n] or NULL */,
                          void* stream, const float* feat_target_nchw /* or NULL */, int feat_stage, float feat_weight,
                          float* fterm_hist /* [steps][n] or NULL */);
/* The discriminator as under model.eval() (model/DCGAN.py:28-50, model/CGAN.py:18-42 with BatchNorm on its running statistics and
 * Dropout the identity): logit[b] = D's pre-sigmoid output for image b, prob[b] (or NULL) its sigmoid.  images_nchw: fp32 [n,3,S,S]
 * in [-1, 1] on the device, or NULL to score the generator's current output where it lies (jck_engine_sample_ex just before: the images
 * never leave the device); noise_nchw (with images only, or NULL): the trainers' instance noise, D sees 0.9 * image + 0.1 * noise
 * (train/dcgan_trainer.py:160); labels: one-hot int64 [n,100], family 1.  One launch folds D's BatchNorm layers; every Conv2d +
 * BatchNorm + LeakyReLU stage is one launch (jck_conv_down_affine) in f32 / bf16x3 and jck_conv_down + jck_bn_act_fwd on the folded
 * table in bf16, where that form measured faster; the head computes no loss; no host synchronisation.
 * 1 <= n <= batch; row b of both outputs is bit for bit what a call with that row alone returns.  Nothing of the training state
 * is written: parameters, gradients, Adam moments, running statistics, num_batches_tracked, the step's scalars.  On a training engine
 * it may be called between two steps, also with the next batch's D(real) forward in flight: every buffer it writes is memory of its
 * own that the first call allocates, clears and waits for (so: the first call not inside a graph capture, and the only one that
 * synchronises with the host; later calls may use any stream) and jck_engine_destroy frees.  D's operands must
 * have been packed (jck_engine_repack(net 1) after loading its state, or a training step): JCK_E_ARG otherwise. */
int jck_engine_score(jck_engine*, const float* images_nchw /* fp32 [n,3,S,S] or NULL */, const float* noise_nchw /* or NULL */,
                     const int64_t* labels /* family 1 */, int n, float* logit /* [n] */, float* prob /* [n] or NULL */, void* stream);
/* The discriminator as a feature extractor (Radford et al. 2016, section 5.1): the conv stack of jck_engine_score - the same input
 * transform without instance noise, the same fold, the same stage launches - and then, instead of the head, one jck_grid_pool per
 * stage on that stage's LeakyReLU output: stage i's grid^2 * D_CS[i] columns at col0 = grid^2 * sum_{j<i} D_CS[j] of row b of `out`
 * (fp32 [n, ld], ld >= the feature dimension, ld % 4 == 0, out 16-byte aligned), stage 0 first.  mode 0: max, 1: mean.  No labels:
 * a CGAN's conv stack never sees them.  jck_engine_feature_dim: grid^2 * sum_i D_CS[i] (960 grid^2 at 64 x 64, 1984 grid^2 at
 * 128 x 128); 0 for a null engine or a grid outside {1,2,4}.  Guards, buffers and contract are jck_engine_score's: 1 <= n <= batch,
 * D's operands packed, the first allocating call not inside a graph capture, nothing of the training state written, D's training
 * activations, real_noisy and the head's concat buffer untouched, row b bit for bit what a call with that row alone returns. */
long long jck_engine_feature_dim(const jck_engine*, int grid);
int jck_engine_features(jck_engine*, const float* images_nchw /* fp32 [n,3,S,S] or NULL: the generator's last output where it lies */,
                        int n, int grid, int mode, float* out /* fp32 [n, ld] */, long long ld, void* stream);
/* debug / parity access to internal NHWC tensors: name in {"fake","real_noisy",...}; returns device ptr or NULL.  The packed GEMM
 * operands are in the table too, numel = their allocated element count (padding included): "d_down{i}", "d_up{i}", "g_up{i}",
 * "g_down{i}" (stage i, the engine's storage type), "g1_w", "d_head_wp" (always fp32), CGAN's "l1_w" and "l1_wT". */
const void* jck_engine_tensor(const jck_engine*, const char* name, long long* numel);

/* ---- evaluation branch: the metric network (reference metrics.py:46-51,80-94: torchvision inception_v3 with a
 * Linear(2048,100) head, eval mode) as a chain of NHWC fp32 kernels; jck-generation_amd/inception.py holds the topology and
 * the local-weights loader.  conv2d: out[n,oy,ox, out_coff + co] = act(scale[co] * sum_{kh,kw,ci} x[n, oy*SH-PH+kh, ox*SW-PW+kw, ci]
 * * w_kc[(kh*KW + kw)*Cin + ci][co] + shift[co]) - eval-mode BatchNorm folded into scale / shift (NULL: 1 / 0), exact-fp32
 * MFMA, the output written into a channel slice of a [.., out_cstride] tensor (Inception concatenations need no copy).
 * pool2d mode 0: max (aten::max_pool2d, no padding value enters), mode 1: average with count_include_pad = True
 * (F.avg_pool2d default).  mean_cov: column means and the unbiased covariance of x[N][D] in fp64 (np.mean / np.cov of
 * metrics.py:120-126 on the device). */
int jck_conv2d_nhwc_f32(const float* x, const float* w_kc, const float* scale, const float* shift, float* out, int N, int H, int W,
                        int Cin, int KH, int KW, int SH, int SW, int PH, int PW, int Cout, int out_cstride, int out_coff, int relu,
                        void* stream);
int jck_pool2d_nhwc_f32(const float* x, float* out, int N, int H, int W, int C, int k, int stride, int pad, int mode, int out_cstride,
                        int out_coff, void* stream);
int jck_global_avgpool_nhwc_f32(const float* x, float* out, int N, int HW, int C, void* stream);
int jck_nchw_to_nhwc_f32(const float* x, float* out, int N, int C, int H, int W, void* stream);
int jck_mean_cov_f64(const float* x, double* mean, double* cov, int N, int D, void* stream);

/* Pairwise statistics over feature matrices x[M][D], y[N][D] (row-major fp32, any D, any alignment) for KID and improved
 * precision / recall (jck-generation_amd/metrics.py): one Gram-tile core on the exact-fp32 MFMA, never an M x N matrix in
 * memory.  Squared distances are d2 = max(0, (|a|^2 + |b|^2) - 2 <a, b>) in fp32 with fmaf-chain norms. */
/* bytes of workspace jck_poly3_sum_f64 needs for M x N pairs (host only; grows with the launch grid, not with M * N; 0 for
 * sizes the entry points refuse) */
size_t jck_pairstat_ws_bytes(int M, int N);
/* out[0] = sum_{i,j} (gamma * <x_i, y_j> + coef0)^3, the polynomial in fp64; skip_diag != 0 leaves out the pairs i == j (by
 * index).  Partials per workgroup go to ws, a second launch adds them in a fixed order: deterministic, no atomics. */
int jck_poly3_sum_f64(const float* x, int M, const float* y, int N, int D, double gamma, double coef0, int skip_diag, double* out,
                      double* ws, void* stream);
/* r2[i] = the k-th smallest d2(x_i, x_j) over j != i (by index), 1 <= k <= 8, k < N; NaN for a row with a non-finite norm */
int jck_knn_radius2_f32(const float* x, int N, int D, int k, float* r2, void* stream);
/* hit[i] = 1 when d2(q_i, ref_j) <= r2[j] for some j (a tie is a hit), else 0; 255 for a query row with a non-finite norm.
 * A reference row whose radius is NaN never hits. */
int jck_manifold_hit_u8(const float* q, int M, const float* ref, const float* r2, int N, int D, unsigned char* hit, void* stream);

/* Nearest reference rows WITH their indices (memorisation checks: a sample beside its nearest training images).  For every
 * query row q_i the k (1..8) rows of ref[N][D] with the smallest squared Euclidean distance, ascending by (d2, index): equal
 * distances go to the lower index.  idx[i][t] = ref_base + j (or -1), d2[i][t] its distance.  Two stages on the device: the 8
 * smallest Gram distances max(0, (|a|^2 + |b|^2) - 2 G) per query pick the candidates (the tile core above; the walk over the
 * references is split over the grid, partial lists go to ws and merge in a fixed order - no atomics, two runs give the same
 * bits); each candidate's distance is then recomputed from differences, sum_c (q_c - ref_c)^2 in fp32 in a fixed order, so that
 * |d2 - exact| <= (D + 4) 2^-24 exact even for a near copy, where the Gram form has no correct digit left.
 *   exclude_self != 0   leaves out the pair with q_base + i == ref_base + j (by index: a duplicate row elsewhere stays a
 *                       neighbour at distance 0)
 *   merge != 0          idx / d2 come in holding earlier results (real distances, tail-padded as below) and are merged by
 *                       (d2, idx): a reference set fed in chunks with the right ref_base gives the one-call result
 *   fewer than k eligible references: the tail is idx -1 / d2 +inf.  A query row with a non-finite norm: idx -1 / d2 NaN in
 *   all k places.  A reference row with a non-finite norm is never a neighbour.
 * jck_knn_index_ws_bytes: bytes of ws for M queries against N references in one call (host only; 0 for sizes the entry point
 * refuses). */
size_t jck_knn_index_ws_bytes(int M, int N);
int jck_knn_index_f32(const float* q, int M, const float* ref, int N, int D, int k, long long q_base, long long ref_base,
                      int exclude_self, int merge, long long* idx, float* d2, void* ws, void* stream);

/* Per-cluster sums and means of feature rows (csrc/cluster.hip): the update half of a Lloyd iteration of k-means; the assignment
 * half is jck_knn_index_f32 with k = 1, whose idx[M][1] is `label` as it stands (int64).
 *   sum[c][j]    = the sum over the rows i of x[N][D] with label[i] == c of x[i][j]; count[c] = their number.  Both are always
 *                  written; an empty cluster gets zeros.  Rows with label[i] < 0 or >= K are skipped and counted nowhere
 *                  (jck_knn_index_f32 gives -1 to a non-finite row).
 *   centre[c][j] = __fdiv_rn(sum[c][j], (float)count[c]) for every c with count[c] > 0 (a correctly rounded division); rows of
 *                  empty clusters are not touched.  NULL: no centres.
 * Deterministic, and more: no floating-point atomics.  The row indices are grouped by label with a stable counting sort in ws,
 * every cluster's list is cut from its own start into pieces of R = jck_segment_chunk_rows() rows, a piece is summed row after row
 * from zero, and a cluster's pieces are added in ascending order: sum[c] = ((p_0 + p_1) + p_2) + ..., p_j = (((0 + r_jR) + r_jR+1)
 * + ...).  The bits of sum[c] therefore depend on the sequence of rows labelled c, in ascending row index, and on nothing else -
 * not on N, K, the other rows, the launch grid or the scheduling - and |sum - exact| <= gamma_(n_c - 1) sum |x_ij|.
 * Every element of x is read once.  16-byte loads when D % 4 == 0 and x, sum, centre and ws lie on 16-byte boundaries, scalar
 * loads otherwise, with the same results.  Limits: 1 <= K <= 1024, 1 <= N <= 2^30, 1 <= D <= 65535 * 256; these, or a NULL x, label,
 * sum, count or ws: JCK_E_ARG from the host, nothing launched.
 * jck_segment_ws_bytes: bytes of ws (host only; 0 for sizes the entry point refuses; grows with N).  jck_segment_chunk_rows: R
 * (host only). */
size_t jck_segment_ws_bytes(int N, int D, int K);
int jck_segment_chunk_rows(void);
int jck_segment_mean_f32(const float* x, int N, int D, const long long* label, int K, float* sum, int* count, float* centre, void* ws,
                         void* stream);

/* Structural similarity of pairs of uint8 NHWC pictures [n][S][S][3] (csrc/ssim.hip; the definition: DESIGN.md 5.16).  Pair p is
 * (a[ia[p]], b[ib[p]]); b may equal a; the index lists are device int64 [P].  11 <= S <= 128; L levels, L >= 1, S % 2^(L-1) == 0 and
 * S >> (L-1) >= 11 (so L <= 4).
 *   ssim[p]     the mean over the channels of the mean SSIM map at level 0 (11-tap Gaussian window, sigma 1.5, valid region)
 *   ms_ssim[p]  the mean over the channels of prod_{l<L-1} max(cs[c][l], 0)^w_l * max(ss[c][L-1], 0)^w_(L-1), w = the first L of
 *               (0.0448, 0.2856, 0.3001, 0.2363, 0.1333) over their sum; the next level is the 2 x 2 mean of both planes
 *   sq_err[p]   sum (a - b)^2 over the 3 S^2 bytes, an exact integer
 *   terms       [P][3][L][2] = (cs[c][l], ss[c][l]), the means of the two maps per channel and level; NULL: not written
 * A pair with an index outside 0 .. na-1 / 0 .. nb-1 gets NaN, NaN, -1 (and NaN terms); nothing else of it is touched.
 * One workgroup per pair: every byte of the two pictures is read once, at any byte alignment, and planes, filter passes and levels
 * stay in LDS and registers.  No floating-point atomics and no contraction in the map formulas: a map's mean is added in an order
 * fixed by S and the level, the bits of a pair's outputs depend on its two pictures, S and L alone (not on P, its place, the other
 * pairs or the grid), they are equal when the two pictures are swapped, and equal pictures give exactly 1.0f, 1.0f, 0.
 * NULL a, b, ia, ib, ssim, ms_ssim or sq_err, S or L outside the above, P < 1, P > 2^24, na or nb < 1: JCK_E_ARG from the host before
 * any HIP call.  jck_ssim_max_levels: the largest admissible L for S, 0 when S is out of range (host only). */
int jck_ssim_pairs_u8(const unsigned char* a, long long na, const unsigned char* b, long long nb, int S, const long long* ia,
                      const long long* ib, int P, int L, float* ssim, float* ms_ssim, long long* sq_err, float* terms, void* stream);
int jck_ssim_max_levels(int S);

/* Sliced Wasserstein distance on Laplacian-pyramid patches of uint8 NHWC pictures [n][S][S][3] (csrc/swd.hip; the definition:
 * DESIGN.md 5.17).  S is 32, 64 or 128; level l has side S >> l, 1 <= L <= jck_swd_max_levels(S) (the levels with side >= 16:
 * 2, 3, 4; 0 for another S; host only).  pos: device int32 [n][L][P][2], the (y, x) top-left corners of P 7 x 7 patches per picture
 * and level, each in [0, (S >> l) - 7].  A descriptor is the 147 Laplacian values of a patch in the order [c][dy][dx]; every one is
 * the fp64 value of the definition rounded once to fp32 (the pyramid is exact fixed point).
 *   jck_swd_patch_stats_u8   sum[l][c], sumsq[l][c] (fp64 [L][3]) of the descriptor components over the n P 49 of a level and
 *                            channel.  part: fp64 workspace [n][L][3][2], one row per picture (kept: a caller may inspect it).  fp64
 *                            accumulation in an order fixed by n and P: two calls give the same bits.
 *   jck_swd_project_u8       proj[(l D + d) ld + i P + p] = sum_j fmul(fsub(x_j, mean[l][c(j)]), rstd[l][c(j)]) dirs[d][j], dirs
 *                            fp32 [D][147], mean / rstd fp32 [L][3], ld >= n P the length of a row (a chunk of pictures passes proj +
 *                            its first column).  fp32, one fmaf per product, per channel from zero in ascending j, the three
 *                            channels added in ascending order: |proj - exact| <= 53 2^-24 sum_j |(x_j - mean) rstd dirs[d][j]|.
 * A picture with a corner out of range: its part[] row / its P entries of every proj row are NaN, nothing else of it is written.
 * One workgroup per picture; descriptors stay in LDS.
 *   jck_sort_rows_f32        out[r] = x[r] sorted ascending, rows of M >= 1 keys, by the sign-flip order of the bit patterns (total:
 *                            -0 < +0; NaNs at the two ends by their bits).  ws: jck_sort_rows_ws_bytes(Rows, M) bytes (0 when M <=
 *                            jck_sort_rows_tile(); may then be NULL); ws_bytes is what the caller has.  out may equal x.
 *   jck_swd_rows             w[r] = mean_j |sa[r][j] - sb[r][j]| in fp64, an order fixed by M.
 * NULL pointers, S, L, P, D, n, Rows, M out of range, ld < n P, a workspace that is too small: JCK_E_ARG from the host before any
 * HIP call.  jck_sort_rows_ws_bytes returns 0 for sizes the entry point refuses too. */
int jck_swd_max_levels(int S);
int jck_swd_patch_stats_u8(const unsigned char* images, int n, int S, int L, const int* pos, int P, double* part, double* sum,
                           double* sumsq, void* stream);
int jck_swd_project_u8(const unsigned char* images, int n, int S, int L, const int* pos, int P, const float* dirs, int D,
                       const float* mean, const float* rstd, float* proj, long long ld, void* stream);
size_t jck_sort_rows_ws_bytes(int Rows, long long M);
int jck_sort_rows_tile(void);
int jck_sort_rows_f32(const float* x, int Rows, long long M, float* out, void* ws, size_t ws_bytes, void* stream);
int jck_swd_rows(const float* sa, const float* sb, int Rows, long long M, double* w, void* stream);

/* Power spectra of uint8 NHWC pictures [n][S][S][3], S in 32, 64, 128 (csrc/spectrum.hip; the definition: DESIGN.md 5.18).  plane: 0, 1, 2
 * = a channel (Y = 256 * byte), 3 = luma (Y = 77 R + 150 G + 29 B).  Per picture T = sum Y, mean[i] = T / (256 S^2) (exact), the plane
 * c = S^2 Y - T converted to fp32 once, scaled by 1 / (256 S^2) and, with win (device fp32 [S], or NULL), multiplied by win[y] then win[x];
 * F its two-dimensional DFT (fp32, in LDS, twiddles rounded from fp64), P = |F|^2 / (S^2 win_power) in fp64.
 *   jck_spectrum_bins      R = 24 / 46 / 92 radial bins of S = 32 / 64 / 128 (bin r of (u, v): r^2 - r < fu^2 + fv^2 <= r^2 + r with fu =
 *                          min(u, S - u), fv likewise); JCK_E_ARG for another S.  Host only.
 *   jck_spectrum_grid      G, the workgroups of a launch that forms the mean plane (JCK_E_ARG for another S).  Host only.
 *   jck_spectrum_ws_bytes  bytes of the partial planes: min(n, G) S (S / 2 + 1) 8 with the mean plane, 0 without it or for sizes the
 *                          entry point refuses.  Host only.
 *   jck_spectrum_u8        prof[i][r] (device fp64 [n][R]) = the mean of P_i over bin r; mean (device fp64 [n]); mean2d (device fp64
 *                          [S][S], or NULL) = (1/n) sum_i P_i[u][v], (u, v) and (-u, -v) holding equal bits; ws / ws_bytes: what
 *                          jck_spectrum_ws_bytes(n, S, 1) asks for, 8-byte aligned (unused when mean2d is NULL).
 * A picture's prof row and mean depend on that picture alone (equal bits at n = 1 and inside any batch); every sum runs in an order
 * fixed by S, the mean plane's by S and n.  x may start at any byte address.  sum |P^ - P| <= B(S) sum P with B = 8.5e-6, 1.01e-5,
 * 1.16e-5 (derived in csrc/spectrum.hip).  n = 0: JCK_OK, nothing launched.  S, plane, n < 0, a win_power that is not finite and
 * positive, a NULL x / prof / mean, a workspace that is too small: JCK_E_ARG from the host before any HIP call. */
int jck_spectrum_bins(int S);
int jck_spectrum_grid(int S);
size_t jck_spectrum_ws_bytes(int n, int S, int want_mean2d);
int jck_spectrum_u8(const unsigned char* x, int n, int S, int plane, const float* win, double win_power, double* prof, double* mean,
                    double* mean2d, void* ws, size_t ws_bytes, void* stream);

/* Per-step optimiser scalars into device memory (so that a captured graph of the step has no per-step kernel argument), and
 * hipGraph capture of a sequence of jck_engine_phase calls: begin -> phases on `stream` (not the default stream) -> end
 * returns an executable graph; launch replays it.  The jck_step_inputs pointers are baked: keep the buffers in place,
 * refresh their contents, keep one graph per step parity, call jck_engine_set_step before every launch. */
int jck_engine_set_step(jck_engine*, int step, float lr, void* stream);
/* Moving average of G's weights inside the step (optimizer_g.step(), train/dcgan_trainer.py:189, train/cgan_trainer.py:212, is
 * where it advances; the reference keeps none).  bind_ema attaches an arena of jck_engine_arena_numel_of(e, 0, 0) floats, 16-byte
 * aligned, to a bound engine (NULL detaches): JCK_PHASE_G_STEP's Adam launch then updates it as jck_adam_ema does - no further
 * launch, workspace and every other launch unchanged; D has no average.  set_ema: the weight of optimiser step s is 1 for
 * s < start_step (the average tracks the weights during warm-up) and (float)(1.0 - decay) from there on (decay is a double so that this is the one rounding, as for jck_adam's scalars).  It reaches the launch
 * through the step's scalars in device memory (jck_engine_set_step), so a captured graph bakes no weight.  An engine bound with
 * the EMA arena AS its g_params samples the averaged generator through jck_engine_sample. */
int jck_engine_bind_ema(jck_engine*, float* g_ema);
int jck_engine_set_ema(jck_engine*, double decay, int start_step);
/* Instance noise drawn INSIDE the image kernels (steps whose jck_step_inputs.noise_real / noise_fake are NULL): Philox4x32-10
 * keyed by `seed`, counter = (pixel, tensor, optimiser step), Box-Muller normals - no 25 MB noise tensor per step.  The *_rng
 * entry points are the per-op forms (rng: device uint32[4] = {seed lo, seed hi, step, 0}; tensor_id separates real / fake). */
int jck_engine_set_noise_seed(jck_engine*, unsigned long long seed);
/* The step's small random inputs as jck_engine_set_step draws them when jck_step_inputs carries none (z, alpha, CGAN's
 * Dropout keep masks NULL): z [nz] ~ N(0,1) (train/dcgan_trainer.py:168), alpha [nalpha] ~ U[0,1) (:111), masks [nmask] in {0,1}
 * with P(1) = keep_p (model/CGAN.py:105); Philox4x32-10, counter = (index/4, tensor id, step), key = seed.  hp: 8 floats scratch. */
int jck_step_rng(float* hp, int step, unsigned long long seed, float* z, long long nz, float* alpha, long long nalpha,
                 float* masks, long long nmask, float keep_p, void* stream);
int jck_img_prep_rng(int prec, const float* img_nchw, const unsigned* rng, int tensor_id, float keep, float mix, void* out, int N, int HW,
                     void* stream);
int jck_img_prep_u8_rng(int prec, const unsigned char* data, const int64_t* idx, const unsigned* rng, int tensor_id, float keep,
                        float mix, void* out_nhwc4, int B, int Hs, int Ws, void* stream);
int jck_axpy_noise_rng(int prec, const void* x, const unsigned* rng, int tensor_id, float keep, float mix, void* out, int N, int HW,
                       void* stream);
int jck_engine_capture_begin(jck_engine*, void* stream);
int jck_engine_capture_end(jck_engine*, void* stream, void** graph_exec);
int jck_engine_capture_abort(jck_engine*, void* stream);
/* nodes (kernel launches, memsets) of the graph this engine's last jck_engine_capture_end instantiated: the launch count of the
 * captured phases (one optimizer step = train/dcgan_trainer.py:155-189 when all five phases are captured) */
int jck_engine_graph_nodes(const jck_engine*);
int jck_graph_launch(void* graph_exec, void* stream);
void jck_graph_destroy(void* graph_exec);

/* Kernel-selection knob (same names as the JCK_<KEY> environment presets, lower case): "bn_res", "bn_bwd_fuse",
 * "igemm_dma_ksplit", "wgrad_ws", "wgrad_dma", "wgrad_wgs".  Lets a test force a variant at a small shape.
 * Unknown key -> JCK_E_ARG. */
int jck_tune(const char* key, int value);
/* per-launch HIP-event timing of the MFMA kernels (bench.py roofline leg).  enable(1) ... run ... collect():
 * per (kernel variant, HIP stream the launches ran on): launches, total milliseconds, total algorithmic FLOPs, total algorithmic
 * bytes (streaming kernels), the stream.  A variant launched on two streams comes back as two rows.  Returns the number of rows. */
int jck_prof_enable(int on);
int jck_prof_collect(int cap, const char** name_out, int* count_out, double* ms_out, double* flops_out, double* bytes_out,
                     void** stream_out);

/* debug probe: lane l of one wave returns the 8 elements wgrad's transposed LDS read hands it from a
 * [32][ld] 16-bit tile: out[l*8+j] must equal in[(8*(l>>4)+j)*ld + (l&15)] */
int jck_debug_tr_read(const void* in, int ld, void* out, void* stream);

/* ---- RCCL gradient all-reduce {init, enqueue, wait} ------------------------------------------------------------------------
 * The reference's multi-GPU form is DistributedDataParallel around G and D: what optimizer_d.step() / optimizer_g.step() consume
 * (train/dcgan_trainer.py:180,189, train/cgan_trainer.py:204,212) are gradients averaged over the ranks.  A network's gradients
 * are one flat fp32 arena here, so the exchange is one SUM all-reduce per arena (or slice); the 1/world factor goes into jck_adam's
 * grad_scale.  The collective runs on the communicator's OWN stream: enqueue orders it behind everything `producer_stream` holds
 * at the time of the call, wait makes `consumer_stream` wait for it on the device; the host never blocks.  Up to 8 tickets in
 * flight.  librccl is resolved at the first call (a copy already in the process - PyTorch's - is preferred; JCK_RCCL_LIB names
 * another), so a single-GPU process never maps it.
 *   rank 0: jck_comm_unique_id(id); every rank receives the 128 bytes over any host channel; every rank: jck_comm_create (a
 *   collective call, with its device current). */
typedef struct jck_comm jck_comm;
#define JCK_COMM_ID_BYTES 128
int jck_comm_unique_id(unsigned char* id128);
int jck_comm_create(jck_comm** out, const unsigned char* id128, int world, int rank);
int jck_comm_world(const jck_comm*);
int jck_comm_allreduce_enqueue(jck_comm*, float* buf, size_t count, void* producer_stream, int* ticket);
int jck_comm_wait(jck_comm*, int ticket, void* consumer_stream);
int jck_comm_destroy(jck_comm*);

#ifdef __cplusplus
}
#endif
#endif
