// C-ABI launchers, gather-GEMM and weight gradient (host side; kernels in *.hpp).
#include "ops_internal.hpp"
#include "igemm.hpp"
#include "thin.hpp"
#include "wgrad.hpp"

// ---------------------------------------------------------------------------------------------------------
// gather-GEMM dispatch
// ---------------------------------------------------------------------------------------------------------
// precision -> P for the kernels that are instantiated per precision tag (common.hpp)
#define DISPATCH_P(prec, CALL)                                          \
  do {                                                                  \
    if ((prec) == JCK_PREC_BF16) { typedef PrecBf16 P; return CALL; }   \
    if ((prec) == JCK_PREC_F32) { typedef PrecF32 P; return CALL; }     \
    if ((prec) == JCK_PREC_BF16X3) { typedef PrecBf16x3 P; return CALL; } \
    JCK_FAIL(JCK_E_ARG, "bad prec");                                    \
  } while (0)

// launch of a kernel instantiation that needs more dynamic LDS than the default limit: its limit is raised once, on the first launch
// of that instantiation - to what it launches with, or to LDS_LIMIT where that is given
template <auto KERN, int LDS_LIMIT = 0, class Params>
static int launch_lds(dim3 grid, dim3 block, int lds, hipStream_t st, const Params& q) {
  static bool attr_done = false;
  if (!attr_done) {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_LIMIT ? LDS_LIMIT : lds));
    attr_done = true;
  }
  hipLaunchKernelGGL(KERN, grid, block, lds, st, q);
  HIPCHK(hipGetLastError());
  return JCK_OK;
}

// what the three gather-GEMM launchers share: the tile grid and the kernel's copy of the parameters, which carries it ...
static dim3 igemm_grid(const IgemmParams& p, int nch_pad, int phases, int BCH, int BPIX, IgemmParams& q) {
  const dim3 grid(cdiv(p.M, BPIX), nch_pad / BCH, phases);
  q = p;
  q.gx = grid.x; q.gy = grid.y; q.gz = grid.z;
  return grid;
}
// ... and, for statistics written per tile, the channel tiles per channel set and the slot count: `rows_per_tile` rows per tile
static void igemm_tile_stats(IgemmParams& q, const dim3& grid, int BCH, int rows_per_tile, int* slots) {
  q.ytiles_per_cset = std::max(1, q.cstat / BCH);
  if (slots) *slots = (int)(grid.x * grid.z * (grid.y / q.ytiles_per_cset) * rows_per_tile);
}

template <class P, int BCH, int BPIX, int NSUB, Epi E = Epi::Plain>
static int launch_igemm_t(const IgemmParams& p, int nch_pad, int phases, hipStream_t st, int* slots) {
  typedef IgemmCfg<P, BCH, BPIX> C;
  constexpr KernelId id = kid_igemm<P, BCH, BPIX, NSUB>();
  ProfScope prof(id, p.flops, st);
  note_launch(id);
  IgemmParams q;
  const dim3 grid = igemm_grid(p, nch_pad, phases, BCH, BPIX, q);
  if (q.stats) {
    if (q.cstat % BCH != 0 && BCH % q.cstat != 0) JCK_FAIL(JCK_E_ARG, "igemm: stats channel count incompatible with the tile");
    igemm_tile_stats(q, grid, BCH, C::WPIX, slots);
  }
  return launch_lds<igemm_kernel<P, BCH, BPIX, NSUB, 2, E>>(dim3(grid.x * grid.y * grid.z), dim3(256), C::LDS_BYTES, st, q);
}

template <int BCH, int BPIX, int NSTG, bool WS = false, int NCW = 4, Epi E = Epi::Plain>
static int launch_igemm_dma(const IgemmParams& p, int nch_pad, int phases, hipStream_t st, int* slots) {
  constexpr int LDSB = NSTG * (BCH + BPIX) * IG_BK * 2;
  ProfScope prof(kid_igemm_dma(K_IGEMM_DMA, BCH, BPIX), p.flops, st);
  note_launch(kid_igemm_dma(K_IGEMM_DMA, BCH, BPIX));
  IgemmParams q;
  const dim3 grid = igemm_grid(p, nch_pad, phases, BCH, BPIX, q);
  if (q.stats) igemm_tile_stats(q, grid, BCH, IgemmCfg<PrecBf16, BCH, BPIX, NCW>::WPIX, slots);
  return launch_lds<igemm_dma_kernel<BCH, BPIX, NSTG, WS, NCW, E>>(dim3(grid.x * grid.y * grid.z), dim3(WS ? (NCW + 4) * 64 : 256), LDSB, st, q);
}

// persistent wave-specialised form: at most `cap` workgroups (what the chip holds at this tile's LDS footprint) walk the tiles
template <int BCH, int BPIX, int NCW>
static int launch_igemm_dma_persist(const IgemmParams& p, int nch_pad, int phases, hipStream_t st, int* slots) {
  // three stages + the per-wave BatchNorm lane values and their arrival counters (igemm_wg_row)
  constexpr int LDSB = 3 * (BCH + BPIX) * IG_BK * 2 + NCW * (BCH >= 128 ? 2 : 1) * 256 + 64;
  ProfScope prof(kid_igemm_dma(K_IGEMM_PERSIST, BCH, BPIX), p.flops, st);
  note_launch(kid_igemm_dma(K_IGEMM_PERSIST, BCH, BPIX));
  IgemmParams q;
  const dim3 grid = igemm_grid(p, nch_pad, phases, BCH, BPIX, q);
  const int ntiles = (int)(grid.x * grid.y * grid.z);
  const int cap = 256 * (160 * 1024 / LDSB);                         // 256 CUs x workgroups that fit their LDS
  const int nwg = std::min(ntiles, cap);
  if (q.stats && q.stat_accum) {
    // accumulated rows need several tiles of ONE channel tile per workgroup and tiles inside one group (igemm.hpp)
    const int gyy = (int)grid.y;
    if (!(ntiles >= cap && ntiles % 8 == 0 && (ntiles / 8) % gyy == 0 && (cap / 8) % gyy == 0 && q.cstat == nch_pad &&
          (q.bn_group_rows == 0 || q.bn_group_rows % BPIX == 0)))
      q.stat_accum = 0;
  }
  if (q.stats && !q.stat_accum) igemm_tile_stats(q, grid, BCH, 1, slots);            // one row per tile (igemm_wg_row)
  if (q.stats && q.stat_accum) {    // accumulated forward statistics: rows [group][nwg / gy][2][cstat], one per workgroup (igemm.hpp)
    const int groups = q.bn_group_rows > 0 ? (q.M + q.bn_group_rows - 1) / q.bn_group_rows : 1;
    if (slots) *slots = groups * (nwg / (int)grid.y);
  }
  return launch_lds<igemm_dma_persist_kernel<BCH, BPIX, NCW>, 160 * 1024>(dim3(nwg), dim3((NCW + 4) * 64), LDSB, st, q);
}

// 128 x 256 tiles when there are at least this many: about one tile per CU (fewer leave most of the chip idle)
constexpr int IGEMM_256_MIN_TILES = 250;
// 128 x 128 tiles on the persistent kernel when there are at least this many: batch-256 layers with 8x8 outputs
// (D.conv3's forward at 3 x 256 images 60.6 -> 55.3 us against 128 x 256 tiles)
constexpr int IGEMM_128_MIN_TILES = 200;

// >= 128 channel rows on the register-staged kernel: keep >= ~256 workgroups in flight - halve the pixel tile for small pixel counts
template <class P, Epi E = Epi::Plain>
static int launch_igemm_t128(const IgemmParams& p, int nch_pad, int phases, hipStream_t st, int* slots) {
  const long long wgs = (long long)cdiv(p.M, 128) * (nch_pad / 128) * phases;
  if (wgs >= 256) return launch_igemm_t<P, 128, 128, 1, E>(p, nch_pad, phases, st, slots);
  return launch_igemm_t<P, 128, 64, 1, E>(p, nch_pad, phases, st, slots);
}

template <class P>
static int launch_igemm_p(const IgemmParams& p, int nch_pad, int phases, int nsub, hipStream_t st, int* slots) {
  // bf16 tiles with >= 128 channel rows run on the LDS-DMA kernels: 128x128 tiles with 2 LDS stages (64 KB -> 2-3 workgroups per
  // CU, which hide each other's load latency) while that still gives >= 512 workgroups, else wave-specialised 128x64 tiles.
  // Measured on MI355X at B=256 (tools/micro.py, us): down2 36.2 -> 29.7, down3 43.0 -> 30.3, down4 65.8 -> 40.3,
  // up2 47.2 -> 30.8, up3 34.5 -> 28.8 against the register-staged kernel.  Split-K plain GEMMs (CGAN's Linear(8392,256)) take
  // them too unless jck_tune("igemm_dma_ksplit", 0) sends them to the register-staged one.
  if (!P::IS_F32 && nsub == 1 && nch_pad % 128 == 0 && (p.ksplit <= 1 || (g_igemm_dma_ksplit && p.act_row_elems)) && !p.rows_are_phases) {
    const long long wgs = (long long)cdiv(p.M, 128) * (nch_pad / 128) * phases;
    const long long wgs256 = (long long)cdiv(p.M, 256) * (nch_pad / 128) * phases;
    // persistent kernels: plain bf16 conv / dgrad launches only (their epilogue has no bias, tanh, fp32 or split-K output)
    const bool persist = !(p.bias || p.epi || p.out_f32 || p.out_split_stride);
    // a tile must not straddle two BatchNorm groups: groups are multiples of 8 images (8 * OH*OW % 256 == 0)
    const bool groups_ok = !p.stats || p.logOHW >= 5;
    // ... and the 256 persistent workgroups are not left half idle in their last round: 384 tiles are 1.5 rounds, the same layer in
    // 128 x 128 tiles is 3 full ones
    const auto round_eff = [](long long t) { return (double)t / (double)(((t + 255) / 256) * 256); };
    const bool prefer128 = wgs >= IGEMM_128_MIN_TILES && round_eff(wgs256) < 0.85 && round_eff(wgs) > round_eff(wgs256) + 0.1;
    if (wgs256 >= IGEMM_256_MIN_TILES && !prefer128 && !p.act_row_elems && groups_ok && p.M % 256 == 0)
      return persist ? launch_igemm_dma_persist<128, 256, 8>(p, nch_pad, phases, st, slots)
                     : launch_igemm_dma<128, 256, 3, true, 8>(p, nch_pad, phases, st, slots);
    if (wgs >= IGEMM_128_MIN_TILES && persist && !p.act_row_elems && (!p.stats || p.logOHW >= 4) && p.M % 128 == 0)
      return launch_igemm_dma_persist<128, 128, 4>(p, nch_pad, phases, st, slots);
    if (wgs >= 512) return launch_igemm_dma<128, 128, 2>(p, nch_pad, phases, st, slots);
    if (persist && !p.act_row_elems) return launch_igemm_dma_persist<128, 64, 4>(p, nch_pad, phases, st, slots);
    return launch_igemm_dma<128, 64, 3, true>(p, nch_pad, phases, st, slots);
  }
  if (nch_pad % 128 == 0) {
    if (nsub != 1) JCK_FAIL(JCK_E_ARG, "igemm: 4-channel gather with >=128 output rows unsupported");
    return launch_igemm_t128<P>(p, nch_pad, phases, st, slots);
  }
  if (nch_pad == 64) {
    if (nsub == 2) return launch_igemm_t<P, 64, 128, 2>(p, nch_pad, phases, st, slots);
    if constexpr (!P::IS_F32) {
      // bf16: always the LDS-DMA kernels, so the register-staged 64 x 128 tile is not built for it.  (Split-K comes from
      // jck_linear_fwd alone, which needs a multiple of 128 rows, and rows-as-phases from the 16-row image layer alone: neither
      // gets here.)
      if (!p.act_row_elems && !p.bias && !p.epi && !p.out_f32 && !p.out_split_stride)
        return launch_igemm_dma_persist<64, 128, 4>(p, nch_pad, phases, st, slots);
      return launch_igemm_dma<64, 128, 2>(p, nch_pad, phases, st, slots);
    } else {
      return launch_igemm_t<P, 64, 128, 1>(p, nch_pad, phases, st, slots);
    }
  }
  if (nch_pad == 16) {
    if (nsub != 1) JCK_FAIL(JCK_E_ARG, "igemm: 4->4 channel product unsupported");
    return launch_igemm_t<P, 16, 256, 1>(p, nch_pad, phases, st, slots);
  }
  JCK_FAIL(JCK_E_ARG, "igemm: unsupported padded row count " + std::to_string(nch_pad));
}

// what launch_igemm_fused_p says when it refuses
constexpr const char* epi_built_for(Epi e) {
  return e == Epi::ReluAffine ? "igemm: the ReLU affine epilogue is built for 8..32 gathered channels, or >= 64 and 16, 64 or a multiple of 128 output rows"
       : e == Epi::LeakyAffine ? "igemm: the leaky affine epilogue is built for 4 gathered channels and 64 output rows, or >= 64 and 64 or a multiple of 128"
       : e == Epi::ReluMask ? "igemm: the ReLU mask epilogue is built for 4..32 gathered channels and 64 output rows, or >= 64 and 64 or a multiple of 128"
                            : "igemm: the leaky mask epilogue is built for >= 64 gathered channels and 64 or a multiple of 128 output rows";
}
// Fused-epilogue launches (E != Epi::Plain, igemm.hpp): the kernels that end in the shared epilogue, never the persistent ones, and no
// statistics.  First what E alone has or refuses, then the one tile ladder - launch_igemm_p's non-persistent choices, `phases`
// counted into the workgroups.  No tile is built for an epilogue that does not launch it.
template <class P, Epi E>
static int launch_igemm_fused_p(const IgemmParams& p, int nch_pad, int phases, int nsub, hipStream_t st) {
  static_assert(E != Epi::Plain, "the plain epilogue launches through launch_igemm_p");
  if constexpr (E == Epi::LeakyAffine || E == Epi::ReluMask) {         // nsub 2, the image-side layer: register-staged in every precision
    if (nsub == 2) {
      if (nch_pad != 64) JCK_FAIL(JCK_E_ARG, "igemm: a 4-channel gather is built for 64 output rows");
      return launch_igemm_t<P, 64, 128, 2, E>(p, nch_pad, phases, st, nullptr);
    }
  }
  if constexpr (E == Epi::ReluAffine) {                                // nsub 0, small generators: 16-row tiles whatever the row count
    if (nsub == 0 && nch_pad % 16 == 0) return launch_igemm_t<P, 16, 256, 0, E>(p, nch_pad, phases, st, nullptr);
    if (nsub == 1 && nch_pad == 16) return launch_igemm_t<P, 16, 256, 1, E>(p, nch_pad, phases, st, nullptr);
  }
  if constexpr (E == Epi::ReluMask) {                                  // nsub 0, small generators: 64 output rows alone
    if (nsub == 0 && nch_pad == 64) return launch_igemm_t<P, 64, 128, 0, E>(p, nch_pad, phases, st, nullptr);
  }
  if (nsub != 1 || (nch_pad != 64 && nch_pad % 128)) JCK_FAIL(JCK_E_ARG, std::string(epi_built_for(E)) + ", got " + std::to_string(nch_pad));
  // the ladder: >= 64 gathered channels, 64 or a multiple of 128 channel rows
  if (nch_pad == 64) {
    if constexpr (!P::IS_F32) return launch_igemm_dma<64, 128, 2, false, 4, E>(p, nch_pad, phases, st, nullptr);
    else return launch_igemm_t<P, 64, 128, 1, E>(p, nch_pad, phases, st, nullptr);
  }
  if constexpr (!P::IS_F32) {
    const long long wgs = (long long)cdiv(p.M, 128) * (nch_pad / 128) * phases;
    const long long wgs256 = (long long)cdiv(p.M, 256) * (nch_pad / 128) * phases;
    if (wgs256 >= IGEMM_256_MIN_TILES && p.M % 256 == 0) return launch_igemm_dma<128, 256, 3, true, 8, E>(p, nch_pad, phases, st, nullptr);
    if (wgs >= 512) return launch_igemm_dma<128, 128, 2, false, 4, E>(p, nch_pad, phases, st, nullptr);
    return launch_igemm_dma<128, 64, 3, true, 4, E>(p, nch_pad, phases, st, nullptr);
  } else {
    return launch_igemm_t128<P, E>(p, nch_pad, phases, st, nullptr);
  }
}

static int launch_wgrad_reduce(const float* ws, int Z, int CsRows, int ncols, int Cs, int Cb, int logCbPad, float* grad,
                               int accumulate, hipStream_t st);
// e: the epilogue (igemm.hpp); a fused one finds its operands in p0, where set_epilogue put them
static int launch_igemm(int prec, const IgemmParams& p0, int nch_pad, int phases, int nsub, hipStream_t st, int* slots, Epi e = Epi::Plain) {
  IgemmParams p = p0;
  for (int zz = 0; zz < 4; ++zz)
    for (int t = 0; t < 16; ++t) p.tap[zz][t] = ((int)p.dy[zz][t] << 16) | ((int)p.dx[zz][t] & 0xffff);
  const long long esz = prec_f32_storage(prec) ? 4 : 2;
  if (nsub == 0 && (p.logC < 3 || p.logC > 5 || e == Epi::Plain)) JCK_FAIL(JCK_E_ARG, "igemm: 8..32 gathered channels are built for the affine and mask epilogues alone");
  if (nsub == 1 && p.logC < 6 && !p.act_row_elems) JCK_FAIL(JCK_E_ARG, "igemm: the gathered tensor needs >= 64 channels (or exactly 4)");
  {
    // extent of the gathered tensor: rows (n, oy, ox) span N = M / (OH*OW) images of H x W x C
    const long long nimg = ((long long)p.M + (1ll << p.logOHW) - 1) >> p.logOHW;
    const long long ab = p.act_row_elems ? (long long)p.M * p.act_row_elems * esz : nimg * p.H * p.W * (1ll << p.logC) * esz;
    const long long wb = (long long)(p.ksplit > 1 ? 1 : phases) * (p.w_phase_stride ? p.w_phase_stride : (long long)nch_pad * p.K) * esz;
    if (ab >= (1ll << 31) || wb >= (1ll << 31)) JCK_FAIL(JCK_E_ARG, "igemm: operand exceeds 2 GiB (32-bit buffer offsets)");
    p.act_bytes = (unsigned)ab; p.w_bytes = (unsigned)wb;
  }
  if (p.K % IG_BK != 0) JCK_FAIL(JCK_E_ARG, "igemm: K must be a multiple of 64, got " + std::to_string(p.K));
  if (p.M <= 0) JCK_FAIL(JCK_E_ARG, "igemm: empty problem");
  if (p.stats && !slots) JCK_FAIL(JCK_E_ARG, "igemm: stats requested without a slot-count output");
  if (e != Epi::Plain) {
    // the two operands of the variant: scale and shift, or scale and the stored activation
    const void* a = epi_affine(e) ? (const void*)p.aff_scale : (const void*)p.mask_scale;
    const void* b = epi_affine(e) ? (const void*)p.aff_shift : p.mask_act;
    if (!a || !b || p.stats || p.bias || p.epi || p.ksplit > 1 || p.rows_are_phases || (e == Epi::ReluMask && phases != 1) ||
        !is_pow2(p.cstat) || p.cstat % 4 || ((uintptr_t)a | (uintptr_t)b) % 16)
      JCK_FAIL(JCK_E_ARG, std::string("igemm: the ") + (epi_affine(e) ? "affine epilogue takes 16-byte aligned scale and shift" :
               "mask epilogue takes a 16-byte aligned scale and activation") + ", a power-of-two channel count and no other option" +
               (e == Epi::ReluMask ? ", in one phase" : ""));
    switch (e) {
      case Epi::ReluAffine: DISPATCH_P(prec, (launch_igemm_fused_p<P, Epi::ReluAffine>(p, nch_pad, phases, nsub, st)));
      case Epi::LeakyAffine: DISPATCH_P(prec, (launch_igemm_fused_p<P, Epi::LeakyAffine>(p, nch_pad, phases, nsub, st)));
      case Epi::ReluMask: DISPATCH_P(prec, (launch_igemm_fused_p<P, Epi::ReluMask>(p, nch_pad, phases, nsub, st)));
      case Epi::LeakyMask: DISPATCH_P(prec, (launch_igemm_fused_p<P, Epi::LeakyMask>(p, nch_pad, phases, nsub, st)));
      case Epi::Plain: break;
    }
  }
  DISPATCH_P(prec, launch_igemm_p<P>(p, nch_pad, phases, nsub, st, slots));
}

// image-side layers on the streaming kernels of thin.hpp (bf16, 64 channels on the wide side, row length % 16 == 0)
#define IMG_GPW 8
static int launch_img_down(const void* x, const void* w, void* out, float* stats, int* slots, int N, int Hb, int Wb, double flops,
                           hipStream_t st) {
  ImgDownParams q = {};
  const int OH = Hb / 2, OW = Wb / 2;
  q.x = x; q.w = w; q.out = out; q.stats = stats;
  q.ngroups = N * OH * (OW / 16); q.H = Hb; q.W = Wb; q.logOH = ilog2(OH); q.logG = ilog2(OW / 16);
  q.x_bytes = (unsigned)((long long)N * Hb * Wb * 4 * 2);
  const int grid = cdiv(q.ngroups, 4 * IMG_GPW);       // 8 groups per wave: 2 / 4 / 16 measured 20.0 / 14.7 / 13.2 us against 13.6
  if (stats) {
    if (!slots) JCK_FAIL(JCK_E_ARG, "conv_down: stats requested without a slot-count output");
    *slots = grid;
  }
  ProfScope prof(K_IMG_DOWN, flops, st);
  note_launch(K_IMG_DOWN);
  hipLaunchKernelGGL(img_down_kernel<IMG_GPW>, dim3(grid), dim3(256), 0, st, q);
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
#define IMG_UP_R 8
static int launch_img_up(const void* a, const void* w, void* out, int epi_tanh, int N, int Hs, int Ws, double flops, hipStream_t st,
                         const void* mul_t = nullptr, float mul_scale = 1.f, hipEvent_t done = nullptr) {
  ImgUpParams q = {};
  q.a = a; q.w = w; q.out = out; q.epi_tanh = epi_tanh; q.mul_t = mul_t; q.mul_scale = mul_scale;
  q.nunits = N * (Hs / IMG_UP_R) * (Ws / 16); q.Hs = Hs; q.Ws = Ws; q.logYB = ilog2(Hs / IMG_UP_R); q.logG = ilog2(Ws / 16);
  q.a_bytes = (unsigned)((long long)N * Hs * Ws * 64 * 2);
  ProfScope prof(K_IMG_UP, flops, st);
  note_launch(K_IMG_UP);
  LAUNCH_EV(img_up_kernel<IMG_UP_R>, dim3(cdiv(q.nunits, 4)), dim3(256), 0, st, done, q);
  HIPCHK(hipGetLastError());
  return JCK_OK;
}

// The fused epilogue of an _impl call (enum Epi, igemm.hpp), filled in by name; a default-constructed one is the plain epilogue.
struct IgemmEpiArgs {
  Epi kind = Epi::Plain;
  const float* scale = nullptr;    // every fused kind
  const float* shift = nullptr;    // the affine kinds
  const void* act = nullptr;       // the mask kinds: the stored activation, in the output's layout and type
  float slope = 0.f;               // the leaky kinds
};
// ... and where IgemmParams keeps it: the leaky mask's slope travels in aff_slope
static void set_epilogue(IgemmParams& p, const IgemmEpiArgs& e) {
  if (epi_affine(e.kind)) { p.aff_scale = e.scale; p.aff_shift = e.shift; }
  if (epi_mask(e.kind)) { p.mask_scale = e.scale; p.mask_act = e.act; }
  if (epi_leaky(e.kind)) p.aff_slope = e.slope;
}

static int conv_down_impl(int prec, const void* big, const void* w, void* small_out, int N, int Hb, int Wb, int Cb, int Cs, void* stream,
                          const IgemmEpiArgs& e = {}, float* stats = nullptr, int* stats_slots = nullptr, int fwd_group_images = 0) {
  const int cbp = jck_pad_chan(Cb);
  if (!is_pow2(cbp) || !is_pow2(Hb) || !is_pow2(Wb) || Hb < 2 || Wb < 2 || Cs % 4 != 0)
    JCK_FAIL(JCK_E_ARG, "conv_down: shapes must be powers of two (Hb,Wb,Cb) and Cs % 4 == 0");
  if ((long long)N * Hb * Wb * cbp >= (1ll << 31)) JCK_FAIL(JCK_E_ARG, "conv_down: tensor exceeds 2^31 elements");
  IgemmParams p = {};
  p.act = big; p.w = w; p.out = small_out; p.stats = stats;
  const int OH = Hb / 2, OW = Wb / 2;
  p.M = N * OH * OW; p.NchStore = Cs; p.logC = ilog2(cbp); p.K = 16 << p.logC;
  p.H = Hb; p.W = Wb; p.logOW = ilog2(OW); p.logOHW = ilog2(OH * OW); p.sy = p.sx = 2; p.ntaps = 16;
  for (int t = 0; t < 16; ++t) { p.dy[0][t] = (signed char)(t / 4 - 1); p.dx[0][t] = (signed char)(t % 4 - 1); }
  p.osN = (long long)OH * OW * Cs; p.osY = OW * Cs; p.osX = Cs; p.obase[0] = 0;
  p.cstat = Cs; p.ytiles_per_cset = 1; p.epi = 0; p.w_phase_stride = 0;
  if (stats && !is_pow2(Cs)) JCK_FAIL(JCK_E_ARG, "conv_down: BN statistics need a power-of-two channel count");
  p.flops = 2.0 * p.M * Cs * 16.0 * Cb;
  if (stats && fwd_group_images > 0) { p.bn_group_rows = fwd_group_images * OH * OW; p.stat_accum = 1; }
  set_epilogue(p, e);
  if (e.kind == Epi::Plain && prec == JCK_PREC_BF16 && cbp == 4 && Cs == 64 && OW % 16 == 0 && is_pow2(OH))
    return launch_img_down(big, w, small_out, stats, stats_slots, N, Hb, Wb, p.flops, (hipStream_t)stream);
  const int nsub = cbp == 4 ? 2 : (e.kind == Epi::ReluMask && cbp < 64 ? 0 : 1);
  return launch_igemm(prec, p, jck_pad_rows(Cs), 1, nsub, (hipStream_t)stream, stats_slots, e.kind);
}
// Input gradient of a ConvTranspose2d whose INPUT is a folded eval-mode stage a = relu(scale[c] * y + shift[c]) (latent projection):
// jck_conv_down with v = a_small[m, c] > 0 ? scale[c] * acc : +0 applied to the fp32 accumulators before the one rounding of the store.
// Never the persistent kernels or the image-side streaming kernel: Cb = 4 runs on the register-staged 64 x 128 tile in every precision.
extern "C" int jck_conv_down_mask(int prec, const void* big, const void* w, const void* a_small, const float* scale, void* small_out,
                                  int N, int Hb, int Wb, int Cb, int Cs, void* stream) {
  if (!a_small || !scale) JCK_FAIL(JCK_E_ARG, "conv_down_mask: the activation and the scale are required");
  if (!is_pow2(Cs)) JCK_FAIL(JCK_E_ARG, "conv_down_mask: Cs must be a power of two");
  IgemmEpiArgs e;
  e.kind = Epi::ReluMask; e.act = a_small; e.scale = scale;
  return conv_down_impl(prec, big, w, small_out, N, Hb, Wb, Cb, Cs, stream, e);
}
// D's stage at inference: jck_conv_down with an eval-mode BatchNorm (folded by jck_bn_eval_aux) and the LeakyReLU applied to the fp32
// accumulators, t = fmaf(scale[c], acc, shift[c]), out = t > 0 ? t : t * slope, before the one rounding of the store.  Never the persistent
// kernels or the image-side streaming kernel: Cb = 4 runs on the register-staged 64 x 128 tile in every precision.
extern "C" int jck_conv_down_affine(int prec, const void* big, const void* w, const float* scale, const float* shift, float slope,
                                    void* small_out, int N, int Hb, int Wb, int Cb, int Cs, void* stream) {
  if (!big || !w || !small_out || !scale || !shift) JCK_FAIL(JCK_E_ARG, "conv_down_affine: null tensor, scale or shift");
  if (N < 1) JCK_FAIL(JCK_E_ARG, "conv_down_affine: N must be >= 1");
  if (!is_pow2(Cs) || Cs < 64) JCK_FAIL(JCK_E_ARG, "conv_down_affine: Cs must be a power of two >= 64");
  if (Cb == 3 || Cb == 4) {
    if (Cs != 64) JCK_FAIL(JCK_E_ARG, "conv_down_affine: a 3 / 4-channel input is built for Cs = 64");
  } else if (Cb < 64 || !is_pow2(Cb)) {
    JCK_FAIL(JCK_E_ARG, "conv_down_affine: Cb must be 3, 4 or a power of two >= 64");
  }
  IgemmEpiArgs e;
  e.kind = Epi::LeakyAffine; e.scale = scale; e.shift = shift; e.slope = slope;
  return conv_down_impl(prec, big, w, small_out, N, Hb, Wb, Cb, Cs, stream, e);
}
extern "C" int jck_conv_down(int prec, const void* big, const void* w, void* small_out, float* stats, int* stats_slots,
                             int N, int Hb, int Wb, int Cb, int Cs, void* stream) {
  return conv_down_impl(prec, big, w, small_out, N, Hb, Wb, Cb, Cs, stream, {}, stats, stats_slots);
}
// Forward statistics per BatchNorm group of `group_images` images (N % group_images == 0): *stats_slots rows, the first
// *stats_slots / (N / group_images) of them belong to group 0, and so on - the layout jck_bn_finalize_grouped reads.  Large
// launches on the persistent kernels write one row per (workgroup, group) instead of one per (tile, wave).
extern "C" int jck_conv_down_grouped(int prec, const void* big, const void* w, void* small_out, float* stats, int* stats_slots,
                                     int N, int Hb, int Wb, int Cb, int Cs, int group_images, void* stream) {
  if (group_images < 1 || N % group_images) JCK_FAIL(JCK_E_ARG, "conv_down_grouped: N must be a multiple of group_images >= 1");
  return conv_down_impl(prec, big, w, small_out, N, Hb, Wb, Cb, Cs, stream, {}, stats, stats_slots, group_images);
}
static int conv_up_impl(int prec, const void* small_in, const void* w, void* big_out, int epi_tanh, int N, int Hs, int Ws, int Cs, int Cb,
                        void* stream, const IgemmEpiArgs& e = {}, float* stats = nullptr, int* stats_slots = nullptr, int fwd_group_images = 0) {
  const int cbp = jck_pad_chan(Cb);
  // (<= 4 output channels run as rows-are-phases tiles or on the image-side kernel below, neither of which has the affine)
  if (epi_affine(e.kind) && (Cb < 8 || !is_pow2(Cb))) JCK_FAIL(JCK_E_ARG, "conv_up_affine: Cb must be a power of two >= 8");
  if (!is_pow2(Cs) || Cs < 16 || !is_pow2(Hs) || !is_pow2(Ws) || cbp % 4 != 0)
    JCK_FAIL(JCK_E_ARG, "conv_up: shapes must be powers of two (Hs,Ws,Cs>=16)");
  if ((long long)N * Hs * Ws * 4 * cbp >= (1ll << 31)) JCK_FAIL(JCK_E_ARG, "conv_up: tensor exceeds 2^31 elements");
  IgemmParams p = {};
  p.act = small_in; p.w = w; p.out = big_out; p.stats = stats;
  p.M = N * Hs * Ws; p.NchStore = cbp; p.logC = ilog2(Cs); p.K = 4 << p.logC;
  p.H = Hs; p.W = Ws; p.logOW = ilog2(Ws); p.logOHW = ilog2(Hs * Ws); p.sy = p.sx = 1; p.ntaps = 4;
  if (cbp == 4) {
    // 3/4-channel output: one launch, the four output parities are the 16 MFMA rows, 9 input offsets as taps; every
    // workgroup then writes whole contiguous output rows instead of interleaved 8-byte pixels
    if (Cs % 64) JCK_FAIL(JCK_E_ARG, "conv_up: Cs % 64 != 0 for a <=4-channel output");
    if (stats) JCK_FAIL(JCK_E_ARG, "conv_up: statistics are not provided for <=4-channel outputs");
    p.ntaps = 9; p.K = 9 * Cs; p.NchStore = 16; p.rows_are_phases = 1;
    for (int t = 0; t < 9; ++t) { p.dy[0][t] = (signed char)(t / 3 - 1); p.dx[0][t] = (signed char)(t % 3 - 1); }
    for (int ph = 0; ph < 2; ++ph)
      for (int pw = 0; pw < 2; ++pw) p.obase[ph * 2 + pw] = (ph * 2 * Ws + pw) * cbp;
    p.osN = (long long)4 * Hs * Ws * cbp; p.osY = 2 * 2 * Ws * cbp; p.osX = 2 * cbp;
    p.cstat = 4; p.ytiles_per_cset = 1; p.epi = epi_tanh ? 1 : 0; p.w_phase_stride = 0;
    p.flops = 2.0 * p.M * 4.0 * Cb * 4.0 * Cs;
    if (prec == JCK_PREC_BF16 && Cs == 64 && Ws % 16 == 0 && Hs % IMG_UP_R == 0)
      return launch_img_up(small_in, w, big_out, epi_tanh ? 1 : 0, N, Hs, Ws, p.flops, (hipStream_t)stream);
    return launch_igemm(prec, p, 16, 1, 1, (hipStream_t)stream, nullptr);
  }
  static const int DI[2][2] = {{0, -1}, {1, 0}};          // input offset of tap th for output parity ph
  for (int ph = 0; ph < 2; ++ph)
    for (int pw = 0; pw < 2; ++pw) {
      const int z = ph * 2 + pw;
      for (int t = 0; t < 4; ++t) { p.dy[z][t] = (signed char)DI[ph][t >> 1]; p.dx[z][t] = (signed char)DI[pw][t & 1]; }
      p.obase[z] = (ph * 2 * Ws + pw) * cbp;
    }
  p.osN = (long long)4 * Hs * Ws * cbp; p.osY = 2 * 2 * Ws * cbp; p.osX = 2 * cbp;
  p.cstat = cbp; p.ytiles_per_cset = 1; p.epi = epi_tanh ? 1 : 0;
  if (stats && !is_pow2(cbp)) JCK_FAIL(JCK_E_ARG, "conv_up: BN statistics need a power-of-two channel count");
  const int rows = jck_pad_rows(Cb);
  p.w_phase_stride = (long long)rows * p.K;
  if (p.K % 64 != 0) JCK_FAIL(JCK_E_ARG, "conv_up: 4*Cs must be a multiple of 64");
  p.flops = 2.0 * p.M * 4.0 * Cb * 4.0 * Cs;
  if (stats && fwd_group_images > 0) { p.bn_group_rows = fwd_group_images * Hs * Ws; p.stat_accum = 1; }
  set_epilogue(p, e);
  return launch_igemm(prec, p, rows, 4, e.kind == Epi::ReluAffine && Cs < 64 ? 0 : 1, (hipStream_t)stream, stats_slots, e.kind);
}
// D.conv1's input gradient with the tanh + instance-noise-mix backward of G's output in its epilogue (thin.hpp: ImgUpParams::mul_t):
// out = scale * bf16(convT(small_in)) * (1 - tanh_y^2), bit for bit jck_conv_up followed by tanh_bwd_ev.  *fused = false (and
// nothing launched) when the layer does not run on the image-side streaming kernel: the caller then issues the two launches.
int conv_up_tanh_bwd_ev(int prec, const void* small_in, const void* w, const void* tanh_y, float scale, void* out, int N, int Hs, int Ws,
                        int Cs, int Cb, hipStream_t stream, hipEvent_t done, bool* fused) {
  *fused = prec == JCK_PREC_BF16 && jck_pad_chan(Cb) == 4 && Cs == 64 && Ws % 16 == 0 && Hs % IMG_UP_R == 0 &&
           is_pow2(Hs) && is_pow2(Ws) && (long long)N * Hs * Ws * 16 < (1ll << 31);
  if (!*fused) return JCK_OK;
  return launch_img_up(small_in, w, out, 0, N, Hs, Ws, 2.0 * N * Hs * Ws * 4.0 * Cb * 4.0 * Cs, stream, tanh_y, scale, done);
}
extern "C" int jck_conv_up(int prec, const void* small_in, const void* w, void* big_out, float* stats, int* stats_slots,
                           int epi_tanh, int N, int Hs, int Ws, int Cs, int Cb, void* stream) {
  return conv_up_impl(prec, small_in, w, big_out, epi_tanh, N, Hs, Ws, Cs, Cb, stream, {}, stats, stats_slots);
}
// Input gradient of a Conv2d(k4, s2, p1) whose INPUT is a folded eval-mode stage a = leaky(scale[c] * y + shift[c]) (the critic's latent
// gradient): jck_conv_up with t = scale[c] * acc, v = a_big[m, c] > 0 ? t : t * slope applied to the fp32 accumulators before the one
// rounding of the store (ATen's leaky_relu_backward on the stored result: a = +-0 and a NaN activation take the slope).  Never the
// persistent kernels; Cs and Cb powers of two >= 64.
extern "C" int jck_conv_up_mask(int prec, const void* small_in, const void* w, const void* a_big, const float* scale, float slope,
                                void* big_out, int N, int Hs, int Ws, int Cs, int Cb, void* stream) {
  if (!small_in || !w || !a_big || !scale || !big_out) JCK_FAIL(JCK_E_ARG, "conv_up_mask: null tensor, activation or scale");
  if (N < 1) JCK_FAIL(JCK_E_ARG, "conv_up_mask: N must be >= 1");
  if (!is_pow2(Cs) || Cs < 64 || !is_pow2(Cb) || Cb < 64) JCK_FAIL(JCK_E_ARG, "conv_up_mask: Cs and Cb must be powers of two >= 64");
  if ((uintptr_t)scale % 16 || (uintptr_t)a_big % 16) JCK_FAIL(JCK_E_ARG, "conv_up_mask: the scale and the activation must be 16-byte aligned");
  IgemmEpiArgs e;
  e.kind = Epi::LeakyMask; e.act = a_big; e.scale = scale; e.slope = slope;
  return conv_up_impl(prec, small_in, w, big_out, 0, N, Hs, Ws, Cs, Cb, stream, e);
}
extern "C" int jck_conv_up_grouped(int prec, const void* small_in, const void* w, void* big_out, float* stats, int* stats_slots,
                                   int N, int Hs, int Ws, int Cs, int Cb, int group_images, void* stream) {
  if (group_images < 1 || N % group_images) JCK_FAIL(JCK_E_ARG, "conv_up_grouped: N must be a multiple of group_images >= 1");
  return conv_up_impl(prec, small_in, w, big_out, 0, N, Hs, Ws, Cs, Cb, stream, {}, stats, stats_slots, group_images);
}
static int g1_fwd_impl(int prec, const void* z, const void* w, void* out, int B, int CiPad, int Co, void* stream,
                       const IgemmEpiArgs& e = {}, float* stats = nullptr, int* stats_slots = nullptr) {
  if (!is_pow2(CiPad) || CiPad < 64 || !is_pow2(Co) || (16 * Co) % 128 != 0)
    JCK_FAIL(JCK_E_ARG, "g1_fwd: CiPad must be a power of two >= 64, Co a power of two");
  IgemmParams p = {};
  p.act = z; p.w = w; p.out = out; p.stats = stats;
  p.M = B; p.NchStore = 16 * Co; p.logC = ilog2(CiPad); p.K = CiPad;
  p.H = 1; p.W = 1; p.logOW = 0; p.logOHW = 0; p.sy = p.sx = 1; p.ntaps = 1;
  p.dy[0][0] = 0; p.dx[0][0] = 0;
  p.osN = (long long)16 * Co; p.osY = 0; p.osX = 0; p.obase[0] = 0;
  p.cstat = Co; p.ytiles_per_cset = 1; p.epi = 0; p.w_phase_stride = 0;
  if (Co < 128 && e.kind == Epi::Plain) JCK_FAIL(JCK_E_ARG, "g1_fwd: Co must be >= 128");      // (statistics: a channel set must fill a tile)
  p.flops = 2.0 * B * 16.0 * Co * CiPad;
  set_epilogue(p, e);
  return launch_igemm(prec, p, 16 * Co, 1, 1, (hipStream_t)stream, stats_slots, e.kind);
}
extern "C" int jck_g1_fwd(int prec, const void* z, const void* w, void* out, float* stats, int* stats_slots, int B,
                          int CiPad, int Co, void* stream) {
  return g1_fwd_impl(prec, z, w, out, B, CiPad, Co, stream, {}, stats, stats_slots);
}
// inference: the product with relu(scale[c] * y + shift[c]) - an eval-mode BatchNorm folded by jck_bn_eval_aux - in its epilogue
extern "C" int jck_conv_up_affine(int prec, const void* small_in, const void* w, const float* scale, const float* shift, void* big_out,
                                  int N, int Hs, int Ws, int Cs, int Cb, void* stream) {
  if (!scale || !shift) JCK_FAIL(JCK_E_ARG, "conv_up_affine: scale and shift are required");
  IgemmEpiArgs e;
  e.kind = Epi::ReluAffine; e.scale = scale; e.shift = shift;
  return conv_up_impl(prec, small_in, w, big_out, 0, N, Hs, Ws, Cs, Cb, stream, e);
}
extern "C" int jck_g1_fwd_affine(int prec, const void* z, const void* w, const float* scale, const float* shift, void* out, int B,
                                 int CiPad, int Co, void* stream) {
  if (!scale || !shift) JCK_FAIL(JCK_E_ARG, "g1_fwd_affine: scale and shift are required");
  if (Co < 4) JCK_FAIL(JCK_E_ARG, "g1_fwd_affine: Co must be >= 4");
  IgemmEpiArgs e;
  e.kind = Epi::ReluAffine; e.scale = scale; e.shift = shift;
  return g1_fwd_impl(prec, z, w, out, B, CiPad, Co, stream, e);
}

// ---------------------------------------------------------------------------------------------------------
// weight gradient
// ---------------------------------------------------------------------------------------------------------
struct WgradPlan { int BG, BS, gx, gy, Z, mchunk, CsRows, ncols; size_t ws; };

// split-K target workgroups of a plan with fewer than 4 tiles
constexpr int WGRAD_SMALL_WGS = 512;
static WgradPlan plan_wgrad(long long Mtot, int ncols, int Cs) {
  WgradPlan pl;
  pl.ncols = ncols;
  pl.BG = (ncols % 128 == 0) ? 128 : 64;
  pl.BS = (Cs >= 128) ? 128 : 64;
  pl.gx = cdiv(ncols, pl.BG);
  pl.gy = cdiv(Cs, pl.BS);
  pl.CsRows = pl.gy * pl.BS;
  const int tiles = pl.gx * pl.gy;
  long long Z = std::max(1, (tiles >= 4 ? g_wgrad_wgs : WGRAD_SMALL_WGS) / tiles);
  const long long maxZ = std::max(1ll, Mtot / (WG_BKP * 4));
  Z = std::min(Z, maxZ);
  long long mchunk = (Mtot + Z - 1) / Z;
  mchunk = (mchunk + 63) / 64 * 64;            // multiple of both k-step sizes (32 register-staged, 64 LDS-DMA)
  Z = (Mtot + mchunk - 1) / mchunk;
  pl.Z = (int)Z; pl.mchunk = (int)mchunk;
  pl.ws = (size_t)Z * pl.CsRows * ncols * sizeof(float);
  return pl;
}

template <class P, int BG, int BS, int NSUB>
static int launch_wgrad_t(const WgradParams& p, const WgradPlan& pl, hipStream_t st) {
  constexpr KernelId id = kid_wgrad<P, BG, BS, NSUB>();
  ProfScope prof(id, p.flops, st);
  note_launch(id);
  constexpr int LDSB = WgradCfg<P, BG, BS>::LDS_BYTES;
  return launch_lds<wgrad_kernel<P, BG, BS, NSUB>>(dim3(pl.gx, pl.gy, pl.Z), dim3(256), LDSB, st, p);
}

// LDS-DMA weight gradient: wave-specialised (4 loader + 4 software-pipelined consumer waves, 3 stages = 96 KB) by default;
// jck_tune("wgrad_ws", 0) selects the 4-wave, 2-stage form (48.4 vs 33.7 us at B=256 on the isolated product).
template <int NSTG, bool WS>
static int launch_wgrad_dma_t(const WgradParams& q, int grid, hipStream_t st) {
  constexpr int LDSB = NSTG * 2 * WGD_BKP * 256;
  ProfScope prof(WS ? K_WGRAD_DMA_WS : K_WGRAD_DMA, q.flops, st);
  note_launch(WS ? K_WGRAD_DMA_WS : K_WGRAD_DMA);
  return launch_lds<wgrad_dma_kernel<NSTG, 4, WS>>(dim3(grid), dim3(WS ? 8 * 64 : 256), LDSB, st, q);
}
static int launch_wgrad_dma(const WgradParams& p, const WgradPlan& pl, hipStream_t st) {
  WgradParams q = p;
  q.gx = pl.gx; q.gy = pl.gy; q.gz = pl.Z;
  const int grid = pl.gx * pl.gy * pl.Z;
  if (g_wgrad_ws) return launch_wgrad_dma_t<3, true>(q, grid, st);
  return launch_wgrad_dma_t<2, false>(q, grid, st);
}

template <class P>
static int launch_wgrad_p(const WgradParams& p, const WgradPlan& pl, int nsub, hipStream_t st) {
  if (g_wgrad_dma && p.big_bytes && p.s_bytes && !P::IS_F32 && pl.BG == 128 && pl.BS == 128 && nsub == 1 && !p.big_row_elems && p.logCb >= 6 && p.logCb < 30 &&
      pl.mchunk % WGD_BKP == 0 && p.logOW <= 6 &&
      ((1 << p.logOHW) <= WGD_BKP || p.H == p.sy * ((1 << p.logOHW) >> p.logOW)))     // constant 64-pixel address step (wgrad.hpp)
    return launch_wgrad_dma(p, pl, st);
  if (pl.BG == 128 && pl.BS == 128 && nsub == 1) return launch_wgrad_t<P, 128, 128, 1>(p, pl, st);
  if (pl.BG == 128 && pl.BS == 64 && nsub == 1) return launch_wgrad_t<P, 128, 64, 1>(p, pl, st);
  if (pl.BG == 64 && pl.BS == 64 && nsub == 2) return launch_wgrad_t<P, 64, 64, 2>(p, pl, st);
  if (pl.BG == 64 && pl.BS == 64 && nsub == 1) return launch_wgrad_t<P, 64, 64, 1>(p, pl, st);
  JCK_FAIL(JCK_E_ARG, "wgrad: unsupported tile plan");
}

static int run_wgrad(int prec, WgradParams& p, const WgradPlan& pl, int nsub, float* ws, size_t ws_bytes, hipStream_t st) {
  if (ws_bytes < pl.ws) JCK_FAIL(JCK_E_WS, "wgrad: workspace too small: need " + std::to_string(pl.ws));
  p.part = ws; p.CsRows = pl.CsRows; p.ncols = pl.ncols; p.mchunk = pl.mchunk;
  DISPATCH_P(prec, launch_wgrad_p<P>(p, pl, nsub, st));
}

static int launch_wgrad_reduce(const float* ws, int Z, int CsRows, int ncols, int Cs, int Cb, int logCbPad, float* grad,
                               int accumulate, hipStream_t st) {
  if (Cb % 64 == 0 && (1 << logCbPad) == Cb) {
    // few workgroups and many slabs (the tap-reuse plan): four slab groups per workgroup
    if (Z >= 16 && (long long)(Cb / 64) * Cs <= 1024)
      hipLaunchKernelGGL(wgrad_reduce16_kernel<4>, dim3(Cb / 64, Cs), dim3(1024), 0, st, ws, Z, CsRows, ncols, Cb, logCbPad, grad, accumulate);
    else
      hipLaunchKernelGGL(wgrad_reduce16_kernel<1>, dim3(Cb / 64, Cs), dim3(256), 0, st, ws, Z, CsRows, ncols, Cb, logCbPad, grad, accumulate);
  } else if (logCbPad == 2 && ncols == 64) {
    hipLaunchKernelGGL(wgrad_reduce_img_kernel, dim3(Cs), dim3(256), 0, st, ws, Z, CsRows, Cb, grad, accumulate);
  } else {
    const long long total = (long long)Cs * Cb * 16;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)std::min<long long>((total + 255) / 256, 4096)), dim3(256), 0, st, ws,
                       Z, CsRows, ncols, Cs, Cb, logCbPad, 16, grad, accumulate);
  }
  HIPCHK(hipGetLastError());
  return JCK_OK;
}

extern "C" size_t jck_conv_wgrad_ws_bytes(int N, int Hb, int Wb, int Cb, int Cs) {
  const long long M = (long long)N * (Hb / 2) * (Wb / 2);
  return plan_wgrad(M, 16 * jck_pad_chan(Cb), Cs).ws;
}

extern "C" int jck_conv_wgrad(int prec, const void* small_side, const void* big_side, float* ws, size_t ws_bytes,
                              float* grad, int accumulate, int N, int Hb, int Wb, int Cb, int Cs, void* stream) {
  const int cbp = jck_pad_chan(Cb);
  if (!is_pow2(cbp) || !is_pow2(Hb) || !is_pow2(Wb) || Cs % 8 != 0) JCK_FAIL(JCK_E_ARG, "conv_wgrad: bad shape");
  const int OH = Hb / 2, OW = Wb / 2;
  WgradParams p = {};
  p.sside = small_side; p.big = big_side; p.Mtot = N * OH * OW; p.CsStride = Cs; p.logCb = ilog2(cbp);
  p.H = Hb; p.W = Wb; p.logOW = ilog2(OW); p.logOHW = ilog2(OH * OW); p.sy = p.sx = 2; p.ntaps = 16;
  for (int t = 0; t < 16; ++t) { p.dy[t] = (signed char)(t / 4 - 1); p.dx[t] = (signed char)(t % 4 - 1); }
  p.flops = 2.0 * p.Mtot * Cs * 16.0 * Cb;
  {   // operand sizes for the buffer descriptors of the LDS-DMA kernels (32-bit byte offsets: < 2 GiB each)
    const long long esz = prec_f32_storage(prec) ? 4 : 2;
    const long long bb = (long long)N * Hb * Wb * cbp * esz, sbytes = (long long)p.Mtot * Cs * esz;
    if (bb < (1ll << 31) && sbytes < (1ll << 31)) { p.big_bytes = (unsigned)bb; p.s_bytes = (unsigned)sbytes; }
  }
  const WgradPlan pl = plan_wgrad(p.Mtot, 16 * cbp, Cs);
  JCK_TRY(run_wgrad(prec, p, pl, cbp == 4 ? 2 : 1, ws, ws_bytes, (hipStream_t)stream));
  JCK_TRY(launch_wgrad_reduce(ws, pl.Z, pl.CsRows, pl.ncols, Cs, Cb, p.logCb, grad, accumulate, (hipStream_t)stream));
  return JCK_OK;
}

extern "C" size_t jck_g1_wgrad_ws_bytes(int B, int CiPad, int Co) { return plan_wgrad(B, 16 * Co, CiPad).ws; }

extern "C" int jck_g1_wgrad(int prec, const void* z, const void* dy, float* ws, size_t ws_bytes, float* grad,
                            int accumulate, int B, int Ci, int CiPad, int Co, void* stream) {
  if (!is_pow2(Co) || CiPad % 64 != 0) JCK_FAIL(JCK_E_ARG, "g1_wgrad: bad shape");
  WgradParams p = {};
  p.sside = z; p.big = dy; p.Mtot = B; p.CsStride = CiPad; p.logCb = ilog2(Co);
  p.H = 4; p.W = 4; p.logOW = 0; p.logOHW = 0; p.sy = p.sx = 1; p.ntaps = 16;
  for (int t = 0; t < 16; ++t) { p.dy[t] = (signed char)(t / 4); p.dx[t] = (signed char)(t % 4); }
  const WgradPlan pl = plan_wgrad(B, 16 * Co, CiPad);
  p.flops = 2.0 * B * Ci * 16.0 * Co;
  {
    const long long esz = prec_f32_storage(prec) ? 4 : 2;
    p.big_bytes = (unsigned)((long long)B * 16 * Co * esz); p.s_bytes = (unsigned)((long long)B * CiPad * esz);
  }
  int rc = run_wgrad(prec, p, pl, 1, ws, ws_bytes, (hipStream_t)stream);
  if (rc) return rc;
  JCK_TRY(launch_wgrad_reduce(ws, pl.Z, pl.CsRows, pl.ncols, Ci, Co, p.logCb, grad, accumulate, (hipStream_t)stream));
  return JCK_OK;
}

// the head's packed weight gradient back in PyTorch's layout: the weight gradient's slab sum over one slab
extern "C" int jck_head_unpack_grad(const float* dwp, int C, float* grad, int accumulate, void* stream) {
  return launch_wgrad_reduce(dwp, 1, 1, 16 * C, 1, C, ilog2(C), grad, accumulate, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------------------
// CGAN's Linear layers: plain products on the same kernels
// ---------------------------------------------------------------------------------------------------------
// out[B][NStore] (T, or fp32 slabs [ksplit][B][NStore] when ksplit > 1) = x[B][Kpad] * wp[rows][Kpad]^T (+ bias)
extern "C" int jck_linear_fwd(int prec, const void* x, const void* wp, const float* bias, void* out, int B, int Kpad, int N,
                              int NStore, int ksplit, void* stream) {
  if (Kpad % 64 || NStore % 4) JCK_FAIL(JCK_E_ARG, "linear_fwd: Kpad % 64 or NStore % 4");
  const int rows = jck_pad_rows(N);
  if (rows % 128) JCK_FAIL(JCK_E_ARG, "linear_fwd: N must be >= 65");
  IgemmParams p = {};
  p.act = x; p.w = wp; p.out = out; p.stats = nullptr;
  p.M = B; p.NchStore = std::min(NStore, rows); p.K = Kpad; p.logC = 30; p.H = 1; p.W = 1; p.logOW = 0; p.logOHW = 0;
  p.sy = p.sx = 1; p.ntaps = 1; p.act_row_elems = Kpad; p.bias = ksplit > 1 ? nullptr : bias;
  p.osN = NStore; p.cstat = 4; p.ytiles_per_cset = 1;
  int phases = 1;
  if (ksplit > 1) {
    const int nk = Kpad / 64;
    if (nk % ksplit) JCK_FAIL(JCK_E_ARG, "linear_fwd: k-steps not divisible by ksplit");
    p.ksplit = ksplit; p.ksteps = nk / ksplit; p.out_split_stride = (long long)B * NStore; p.out_f32 = 1;
    phases = ksplit;
  }
  p.flops = 2.0 * B * N * (double)Kpad;
  return launch_igemm(prec, p, rows, phases, 1, (hipStream_t)stream, nullptr);
}

extern "C" size_t jck_linear_wgrad_ws_bytes(int B, int Kpad, int N) { return plan_wgrad(B, Kpad, N).ws; }
// gradp[N][Kpad] fp32 (+)= gy[B][N]^T * x[B][Kpad]     (our column order; see jck_unperm_linear_grad)
extern "C" int jck_linear_wgrad(int prec, const void* gy, int ldgy, const void* x, int Kpad, float* ws, size_t ws_bytes,
                                float* gradp, int accumulate, int B, int N, void* stream) {
  if (Kpad % 64 || ldgy % 8) JCK_FAIL(JCK_E_ARG, "linear_wgrad: bad leading dimensions");
  WgradParams p = {};
  p.sside = gy; p.big = x; p.Mtot = B; p.CsStride = ldgy; p.logCb = 30; p.H = 1; p.W = 1; p.logOW = 0; p.logOHW = 0;
  p.sy = p.sx = 1; p.ntaps = 1; p.dy[0] = 0; p.dx[0] = 0; p.big_row_elems = Kpad;
  const WgradPlan pl = plan_wgrad(B, Kpad, N);
  p.flops = 2.0 * B * N * (double)Kpad;
  int rc = run_wgrad(prec, p, pl, 1, ws, ws_bytes, (hipStream_t)stream);
  if (rc) return rc;
  const long long total = (long long)N * Kpad;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)std::min<long long>((total + 255) / 256, 4096)), dim3(256), 0,
                     (hipStream_t)stream, ws, pl.Z, pl.CsRows, pl.ncols, N, Kpad, 0, 1, gradp, accumulate);
  HIPCHK(hipGetLastError());
  return JCK_OK;
}

// ---------------------------------------------------------------------------------------------------------
// debug probe: what ds_read_b64_tr_b16 returns for the addressing wgrad.hpp uses (pins the hardware
// semantics the weight-gradient kernel relies on; exercised by tests/test_ops_gpu.py)
// ---------------------------------------------------------------------------------------------------------
__global__ void debug_tr_kernel(const bf16_t* __restrict__ in, int ld, bf16_t* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  bf16_t* t = reinterpret_cast<bf16_t*>(smem_raw);
  for (int i = threadIdx.x; i < 32 * ld; i += 64) t[i] = in[i];
  __syncthreads();
  const int lane = threadIdx.x;
  const int trow = (lane >> 4) * 8 + ((lane & 15) >> 2), tcol = (lane & 3) * 4;
  short4v a = lds_tr4(t + trow * ld + tcol), b = lds_tr4(t + (trow + 4) * ld + tcol);
  for (int j = 0; j < 4; ++j) { out[lane * 8 + j] = (bf16_t)a[j]; out[lane * 8 + 4 + j] = (bf16_t)b[j]; }
}
extern "C" int jck_debug_tr_read(const void* in, int ld, void* out, void* stream) {
  if (ld % 4 || ld < 16) JCK_FAIL(JCK_E_ARG, "ld must be a multiple of 4 and >= 16");
  hipLaunchKernelGGL(debug_tr_kernel, dim3(1), dim3(64), 32 * ld * 2, (hipStream_t)stream, (const bf16_t*)in, ld, (bf16_t*)out);
  HIPCHK(hipGetLastError());
  return JCK_OK;
}
