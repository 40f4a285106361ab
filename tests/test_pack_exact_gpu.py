"""Weight packing, bit for bit: the per-op jck_pack_down / up / g1 / head kernels and the engine's one-launch repack
(pack_multi_kernel after load_state / repack(), pack_tail_kernel at the end of a training step) against operand layouts built in torch
by indexing the fp32 parameter as the layout comments of csrc/ew_optim.hpp state them:

  down  wp[cs][t * CbPad + cb]                 rows cs < CsPad, t = kh * 4 + kw
  up    wp[phase][cb][t4 * Cs + cs]            rows cb < CbPad, phase = ph * 2 + pw, t4 = th * 2 + tw, kernel row {1,3},{0,2}[ph][th]
  up16  wp[phase * 4 + c][t9 * Cs + cs]        Cb <= 4: nine input offsets dy, dx in {-1,0,1}; ConvTranspose2d(k4, s2, p1) has output row
                                               2q + ph = 2 (q + dy) - 1 + kh, so kh = ph + 1 - 2 dy where that lies in 0..3, else the entry is 0
  g1    wp[t * Co + co][ci]                    ci < CiPad
  head  wp[t * C + c]                          fp32 always

bf16 storage rounds to nearest even; padding is +0.  Every weight of a layer is a distinct fp32 value (its index, scrambled, is the
mantissa), so one misplaced element shows; a second fill plants zeros, infinities, NaN, denormals and bf16 ties."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

UP_K = ((1, 3), (0, 2))


@pytest.fixture(scope="module")
def G():
    import gpu_util
    return gpu_util


# ---- weights ----------------------------------------------------------------------------------------------------------------------
def ramp(shape, salt=0):
    """fp32 tensor of `shape` (< 2^23 elements): element i has mantissa (i * odd) mod 2^23 - a bijection, so all values are distinct,
    and the seven mantissa bits bf16 keeps change from one element to the next -, exponent 2^-9 .. 2^-6 and sign from other bits of
    the scrambled index (the magnitude of a DCGAN initialisation: a training step on these weights stays finite)."""
    n = int(np.prod(shape))
    assert n <= 1 << 23
    i = np.arange(n, dtype=np.uint64) + np.uint64(salt)
    man = (i * np.uint64(0x9E3779B1)) & np.uint64(0x7FFFFF)
    h = (i * np.uint64(0x85EBCA6B)) >> np.uint64(9)
    bits = ((h & np.uint64(1)) << np.uint64(31)) | ((np.uint64(118) + ((h >> np.uint64(1)) & np.uint64(3))) << np.uint64(23)) | man
    return torch.from_numpy(bits.astype(np.uint32).view(np.float32).reshape(shape).copy())


# sixteen taps' worth of edge values, as fp32 bit patterns
EDGE_BITS = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000,        # +-0, +-inf
             0x00800000, 0x00100000, 0x80000001, 0x7FC00000,        # smallest normal, a denormal bf16 can hold (2^-129), the smallest denormal (-), NaN
             0x3F808000, 0x3F818000, 0xBF818000, 0x3F808001,        # bf16 ties: to even down, to even up, negative; just above a tie
             0x3F807FFF, 0x7F7FFFFF, 0x7F7F0000, 0x00008000]        # just below a tie, the largest fp32 (bf16: inf), the largest bf16, a denormal tie


def plant_edges(w):
    """the edge values as the 16 taps of the first, the last and a middle channel pair -> the pairs"""
    a, b = w.shape[0], w.shape[1]
    pairs = sorted({(0, 0), (a - 1, b - 1), (a // 2, b // 3)})
    e = torch.from_numpy(np.array(EDGE_BITS, dtype=np.uint32).view(np.float32).copy()).view(4, 4)
    for k, (i, j) in enumerate(pairs):
        w[i, j] = torch.roll(e.reshape(16), k).view(4, 4)
    return pairs


# ---- reference layouts (CPU, fp32) -------------------------------------------------------------------------------------------------
def pad_rows(c):
    return 16 if c <= 16 else (64 if c <= 64 else (c + 127) // 128 * 128)


def ref_down(w):
    cs, cb = w.shape[:2]
    cbp = 4 if cb == 3 else cb
    out = torch.zeros(pad_rows(cs), 16, cbp)
    out[:cs, :, :cb] = w.reshape(cs, cb, 16).permute(0, 2, 1)
    return out.reshape(-1)


def ref_up(w):
    cs, cb = w.shape[:2]
    if cb <= 4:
        out = torch.zeros(16, 9, cs)
        for phase in range(4):
            for t9 in range(9):
                kh, kw = (phase >> 1) + 1 - 2 * (t9 // 3 - 1), (phase & 1) + 1 - 2 * (t9 % 3 - 1)
                if 0 <= kh < 4 and 0 <= kw < 4:
                    out[phase * 4:phase * 4 + cb, t9, :] = w[:, :, kh, kw].t()
        return out.reshape(-1)
    out = torch.zeros(4, pad_rows(cb), 4, cs)
    for phase in range(4):
        for t in range(4):
            out[phase, :cb, t, :] = w[:, :, UP_K[phase >> 1][t >> 1], UP_K[phase & 1][t & 1]].t()
    return out.reshape(-1)


def ref_g1(w, cip):
    ci, co = w.shape[:2]
    out = torch.zeros(16, co, cip)
    out[:, :, :ci] = w.reshape(ci, co, 16).permute(2, 1, 0)
    return out.reshape(-1)


def ref_head(w):
    return w.reshape(-1, 16).t().reshape(-1)


def ref_linear1(w):
    """CGAN's Linear(8392, 256) as the forward operand [256][8448]: the first 16 * 512 columns move from (c, hw) to (hw, c) order"""
    out = torch.zeros(256, 8448)
    out[:, :8192] = w[:, :8192].reshape(256, 512, 16).permute(0, 2, 1).reshape(256, 8192)
    out[:, 8192:8392] = w[:, 8192:]
    return out


def stored_bits(ref, bf16, numel=None):
    """fp32 reference -> the bits the library stores (int64 numpy): fp32 as is, or bf16 by round-to-nearest-even on the bit pattern;
    zero-extended with +0 to `numel` elements.  -> (bits, isnan)"""
    b = ref.contiguous().numpy().reshape(-1).view(np.uint32).astype(np.int64)
    nan = np.isnan(ref.numpy().reshape(-1))
    if bf16:
        b = (b + 0x7FFF + ((b >> 16) & 1)) >> 16
    if numel is not None:
        assert numel >= b.size
        b, nan = np.concatenate([b, np.zeros(numel - b.size, np.int64)]), np.concatenate([nan, np.zeros(numel - nan.size, bool)])
    return b, nan


def got_bits(t):
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).numpy().view(np.uint16).astype(np.int64), torch.isnan(t).numpy()
    return t.view(torch.int32).numpy().view(np.uint32).astype(np.int64), torch.isnan(t).numpy()


def assert_bits(t, ref, what, numel=None):
    got, gnan = got_bits(t)
    want, wnan = stored_bits(ref, t.dtype == torch.bfloat16, numel)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(gnan, wnan), (what, "NaN positions")
    bad = (got != want) & ~wnan
    assert not bad.any(), (what, int(bad.sum()), int(np.argmax(bad)), hex(int(got[np.argmax(bad)])), hex(int(want[np.argmax(bad)])))


# ---- per-op entry points -----------------------------------------------------------------------------------------------------------
GUARD = 64
PRECS = [0, 1, 2]          # bf16, fp32, bf16x3 (fp32 storage)


def _buf(G, prec, n):
    """n + GUARD elements of the storage type, all set to a sentinel (1.5)"""
    return torch.full((n + GUARD,), 1.5, dtype=torch.bfloat16 if prec == 0 else torch.float32, device="cuda")


def _fills(shape):
    w0 = ramp(shape)
    w1 = ramp(shape, salt=977)
    plant_edges(w1)
    return (("ramp", w0), ("edges", w1))


def _check_op(G, prec, launch, ref, what):
    for fill, w, r in ref:
        n = r.numel()
        wp = _buf(G, prec, n)
        launch(w.cuda().contiguous(), wp)
        torch.cuda.synchronize()
        assert_bits(wp[:n], r, f"{what} {fill} prec {prec}")
        assert bool((wp[n:].float() == 1.5).all()), (what, "sentinel")


# (Cs, Cb): a 3-channel input (CbPad 4), a 3-row output (CsPad 16), a padded-to-128 case; the last has 1024 * 16 * 512 > 8192 * 256
# elements: the stride loop of the launch wraps
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("cs,cb", [(64, 3), (3, 64), (128, 64), (1024, 512)])
def test_pack_down(G, prec, cs, cb):
    assert (cs, cb) != (1024, 512) or pad_rows(cs) * 16 * cb > 8192 * 256
    _check_op(G, prec, lambda w, wp: G.lib.jck_pack_down(prec, w, cs, cb, wp, G.cur_stream()),
              [(f, w, ref_down(w)) for f, w in _fills((cs, cb, 4, 4))], f"down {cs}x{cb}")


# (64, 3) and (64, 4): the 16-row operand of a thin output, with and without the empty fourth row; (5, 64): Cs no multiple of anything;
# (512, 1024): 4 * 1024 * 4 * 512 > 8192 * 256 elements; (16384, 3): 144 * 16384 elements, past the cap in the thin kernel
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("cs,cb", [(64, 3), (64, 4), (128, 64), (5, 64), (512, 1024), (16384, 3)])
def test_pack_up(G, prec, cs, cb):
    if cb <= 4:
        assert cs < 16384 or 16 * 9 * cs > 8192 * 256
    else:
        assert cs < 512 or 16 * pad_rows(cb) * cs > 8192 * 256
    _check_op(G, prec, lambda w, wp: G.lib.jck_pack_up(prec, w, cs, cb, wp, G.cur_stream()),
              [(f, w, ref_up(w)) for f, w in _fills((cs, cb, 4, 4))], f"up {cs}x{cb}")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("ci,co,cip", [(100, 64, 128), (110, 32, 128), (200, 512, 256), (250, 1024, 256)])
def test_pack_g1(G, prec, ci, co, cip):
    assert co < 1024 or 16 * co * cip > 8192 * 256
    _check_op(G, prec, lambda w, wp: G.lib.jck_pack_g1(prec, w, ci, co, cip, wp, G.cur_stream()),
              [(f, w, ref_g1(w, cip)) for f, w in _fills((ci, co, 4, 4))], f"g1 {ci}x{co}")


@pytest.mark.parametrize("c", [512, 1000])
def test_pack_head(G, c):
    for fill, w in _fills((1, c, 4, 4)):
        wp = _buf(G, 1, 16 * c)
        G.lib.jck_pack_head(w.cuda(), c, wp, G.cur_stream())
        torch.cuda.synchronize()
        assert_bits(wp[:16 * c], ref_head(w), f"head {c} {fill}")
        assert bool((wp[16 * c:] == 1.5).all())


# ---- the engine's one-launch repack ------------------------------------------------------------------------------------------------
def _operands(eng):
    """name -> (reference builder, per-op launcher or None) for every packed operand of the engine, from its parameter shapes"""
    dv, gv = eng.named_views("d"), eng.named_views("g")
    ns = 5 if eng.size == 128 else 4
    ops = {}
    for i in range(ns):
        ops[f"d_down{i}"] = (dv[f"conv{i + 1}.weight"], ref_down, "down")
        ops[f"d_up{i}"] = (dv[f"conv{i + 1}.weight"], ref_up, "up")
        ops[f"g_up{i}"] = (gv[f"conv{i + 2}.weight"], ref_up, "up")
        ops[f"g_down{i}"] = (gv[f"conv{i + 2}.weight"], ref_down, "down")
    zp = 256 if eng.family == 1 else 128
    ops["g1_w"] = (gv["conv1.weight"], lambda w: ref_g1(w, zp), "g1")
    if eng.family == 0:
        ops["d_head_wp"] = (dv[f"conv{ns + 1}.weight"], ref_head, "head")
    else:
        ops["l1_w"] = (dv["linear1.weight"], lambda w: ref_linear1(w).reshape(-1), None)
        ops["l1_wT"] = (dv["linear1.weight"], lambda w: ref_linear1(w).t().reshape(-1), None)
    return ops


def _check_engine_operands(G, eng, what, single_ops):
    from hipgan import PREC_BF16
    torch.cuda.synchronize()
    zp = 256 if eng.family == 1 else 128
    for name, (view, ref, kind) in _operands(eng).items():
        w = view.detach().float().cpu()
        got = eng.tensor(name)
        assert_bits(got, ref(w), f"{what} {name}", numel=got.numel())
        if not single_ops or kind is None:
            continue
        # the per-op entry point on the same parameter, into a zeroed buffer of the operand's allocated size
        one = torch.zeros_like(got)
        a, b = w.shape[0], w.shape[1]
        prec, st = (0 if eng.prec == PREC_BF16 else 1), G.cur_stream()
        wd = view.detach().contiguous()
        if kind == "down":
            G.lib.jck_pack_down(prec, wd, a, b, one, st)
        elif kind == "up":
            G.lib.jck_pack_up(prec, wd, a, b, one, st)
        elif kind == "g1":
            G.lib.jck_pack_g1(prec, wd, a, b, zp, one, st)
        else:
            G.lib.jck_pack_head(wd, b, one, st)
        torch.cuda.synchronize()
        g1, n1 = got_bits(got)
        g2, n2 = got_bits(one)
        assert np.array_equal(n1, n2) and np.array_equal(g1[~n1], g2[~n2]), (what, name, "per-op entry point")


def _fill_convs(eng, g, d, edges):
    """state dicts whose conv (and linear1) weights are the distinct ramp, optionally with the edge values planted"""
    g, d = {k: v.clone() for k, v in g.items()}, {k: v.clone() for k, v in d.items()}
    for salt, sd in ((0, g), (12345, d)):
        for j, k in enumerate(sorted(sd)):
            if k.endswith(".weight") and (k.startswith("conv") or k == "linear1.weight"):
                sd[k] = ramp(tuple(sd[k].shape), salt + 1000 * j)
                if edges and sd[k].dim() == 4:
                    plant_edges(sd[k])
    return g, d


@pytest.mark.parametrize("family,size,prec,B", [("dcgan", 64, "bf16", 8), ("dcgan", 64, "f32", 2), ("dcgan", 128, "bf16", 8),
                                                ("dcgan", 128, "f32", 8), ("cgan", 64, "bf16", 8), ("cgan", 64, "f32", 4)])
def test_engine_repack_is_the_reference(G, family, size, prec, B):
    """load_state + repack() (pack_multi_kernel, one launch per network over the real layer list - every first_chunk boundary): each
    packed operand over its WHOLE allocation, padding included (the zeros of the bind-time memset), equals the reference and the
    per-op entry point bit for bit - with the edge-value fill, then with the plain one; then one training step (D's operands from
    pack_multi_kernel behind Adam(D), G's from pack_tail_kernel) and the same against references rebuilt from the updated fp32
    parameters.  A neighbour's first and last elements are inside its own whole-allocation comparison."""
    import bf16_error as be
    from hipgan.engine import CganEngine, DcganEngine
    from oracle.gan_oracle import build_params
    from util import synth_images
    torch.manual_seed(12345)
    g, d = build_params(family) if size == 64 else build_params(family, size)
    eng = (CganEngine if family == "cgan" else DcganEngine)(batch=B, prec=prec, **({"image_size": 128} if size == 128 else {}))
    eng.load_state(*_fill_convs(eng, g, d, edges=True))
    _check_engine_operands(G, eng, "edges", single_ops=True)
    eng.load_state(*_fill_convs(eng, g, d, edges=False))
    _check_engine_operands(G, eng, "ramp", single_ops=False)
    before = {k: v.clone() for k, v in eng.arenas.items() if k.endswith("_params")}
    imgs = synth_images(B)
    if size == 128:
        imgs = torch.nn.functional.interpolate(imgs, size=128, mode="bilinear", align_corners=False)
    lab = be.labels_for(B, 5) if family == "cgan" else None
    nz = be.noise_for(family, B, 40, lab, size=size)
    sc = eng.step(imgs.cuda().contiguous(), {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in nz.items()}, lr=2e-4)
    assert all(np.isfinite(v) for v in sc.values()), sc
    for k, v in before.items():                       # the step moved the weights, so the operands had to be written again
        assert not torch.equal(v, eng.arenas[k]), k
    _check_engine_operands(G, eng, "after a step", single_ops=True)
