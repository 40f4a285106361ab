"""Discriminator inference: the Conv2d product with the folded eval-mode BatchNorm + LeakyReLU in its epilogue (jck_conv_down_affine),
the inference head (jck_score_head), the engine's scoring (jck_engine_score; DcganEngine.score / score_latents) and the score-guided
sampling built on it (Sampler.images(select=...), generate.py --score).

Exact cases (the integer-data pattern of tests/test_sample_eval_gpu.py): activations 0..15 and weights in {-1, 0, 1} with equal
weight on both signs - every partial sum is an integer of magnitude below 15 * K <= 15 * 4096 < 2^24, exact in fp32 in any order and
exact as bf16 operands; scale[c] = 2^((c % 12) - 6) and an integer shift[c] in [-15, 15], so t = scale * y + shift is exact in fp64
(it spans at most 6 + 16 + 6 bits) and the fp32 value is its ONE rounding - what fmaf gives; slope = 0.25 scales by a power of two,
which commutes with that rounding.  The bf16 result is one more rounding.  A wrong channel, a ReLU in the LeakyReLU's place, a
rounding of y to bf16 before the affine or a second rounding of t all change bits.

Engine parity: the bound tests/test_modules_gpu.py puts on D's module forward, per element |a - b| <= 1e-6 + rtol * max(|b|, rms b)
with rtol 2e-4 (f32) and 1.2e-1 (bf16) - the _parity of tests/test_sample_eval_gpu.py - on the logits, and |prob - ref| below the
same two numbers.  The module returns the probability alone; its logit is torch.logit of that fp32 probability in fp64, which the
fp32 rounding of p leaves good to 6e-8 / (p (1 - p)) - far inside the bound for the |logit| < 8 that these networks give (asserted).

Measured on one MI355X (worst err / tol of the logits, worst |prob - ref|): see DESIGN.md section 5.10."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_sample_eval_gpu import _affine_exact, _expect_equal, _parity, _ref_affine, _up_exact_data

pytestmark = pytest.mark.gpu
PREC_NAME = {0: "bf16", 1: "f32", 2: "bf16x3"}
DT = {0: torch.bfloat16, 1: torch.float32, 2: torch.float32}
TAIL = 1024
SLOPE = 0.25


@pytest.fixture(scope="module")
def G():
    import gpu_util
    return gpu_util


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _nhwc4(x, prec):
    """CPU NCHW fp32 -> device NHWC of the element type, 3 channels zero-padded to 4"""
    n, c, h, w = x.shape
    cp = 4 if c == 3 else c
    t = torch.zeros(n, h, w, cp)
    t[..., :c] = x.permute(0, 2, 3, 1)
    return t.to(DT[prec]).cuda().contiguous()


def _pack_down(G, w, prec):
    cs, cb = w.shape[0], w.shape[1]
    wp = torch.empty(G.lib.jck_pad_rows(cs) * 16 * G.lib.jck_pad_chan(cb), dtype=DT[prec], device="cuda")
    G.lib.jck_pack_down(prec, w.cuda().contiguous(), cs, cb, wp, G.cur_stream())
    return wp


def _affine_down(c):
    k = torch.arange(c)
    return torch.pow(2.0, ((k % 12) - 6).double()).float(), (((k * 7) % 31) - 15).float()


def _t64(y64, scale, shift):
    return y64 * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)


def _leaky64(t, slope):
    return torch.where(t > 0, t, t * slope)


# (N, Hb, Cb, Cs): the image-side gather (NSUB = 2, a ragged last tile: M = 16, 192), the 128-row tiles at M below one tile, and - D.conv2's
# shape at 16x16 inputs with 256 / 257 images - the tiles the dispatch takes only at >= 250 / 512 / 256 workgroups: 128x256
# wave-specialised (bf16, M % 256 == 0), 128x128 LDS-DMA (bf16, 257 images: M % 256 != 0), 128x128 register-staged (f32, bf16x3)
BIG, BIG1 = (256, 16, 64, 512), (257, 16, 64, 512)
IMG = ("igemm<bf16,64,128,img>", "igemm<f32,64,128,img>", "igemm<bf16x3,64,128,img>")
SMALL = ("igemm_dma<128,64,3,ws>", "igemm<f32,128,64>", "igemm<bf16x3,128,64>")
DOWN_KERNEL = {(1, 8, 4, 64): IMG, (3, 16, 3, 64): IMG, (1, 8, 64, 128): SMALL, (3, 8, 128, 256): SMALL, (2, 8, 256, 512): SMALL,
               (1, 8, 64, 64): ("igemm_dma<64,128,2>", "igemm<f32,64,128>", "igemm<bf16x3,64,128>"),       # the 64-row tile at >= 64 gathered channels
               BIG: ("igemm_dma<128,256,3,ws,8>", "igemm<f32,128,128>", "igemm<bf16x3,128,128>"),
               BIG1: ("igemm_dma<128,128,2>", None, None)}
DOWN_EXACT = [pytest.param(s, p, id="x".join(map(str, s)) + "-" + PREC_NAME[p]) for s in DOWN_KERNEL for p in (0, 1, 2) if DOWN_KERNEL[s][p]]
_down_cache = {}


def _down_exact_data(shape):
    if shape not in _down_cache:
        n, hb, cb, cs = shape
        if shape == BIG:                        # the first 256 images of the 257-image case: one CPU reference for both
            x, w, y = _down_exact_data(BIG1)
            _down_cache[shape] = (x[:256], w, y[:256])
            return _down_cache[shape]
        x = torch.randint(0, 16, (n, cb, hb, hb), generator=_gen(31)).float()
        w = torch.randint(-1, 2, (cs, cb, 4, 4), generator=_gen(32)).float()
        assert 15 * 16 * cb < 2 ** 24                              # bounds every partial sum (16 taps x Cb terms of at most 15)
        y = F.conv2d(x, w, None, 2, 1).double()                    # integers below 2^24: the fp32 sums are exact in any order
        _down_cache[shape] = (x, w, y)
    return _down_cache[shape]


@pytest.mark.parametrize("shape,prec", DOWN_EXACT)
def test_conv_down_affine_exact(G, shape, prec):
    n, hb, cb, cs = shape
    x, w, y = _down_exact_data(shape)
    scale, shift = _affine_down(cs)
    t = _t64(y, scale, shift)
    neg = float((t < 0).double().mean())
    assert 0.2 < neg < 0.8, f"test data: {neg:.2f} of the pre-activations are negative"
    if 16 * cb >= 1024:                                            # a rounding of y to bf16 before the affine would show
        assert float((y.float().to(torch.bfloat16).double() != y).double().mean()) > 0.05
    ref = _leaky64(t, SLOPE)
    numel = n * (hb // 2) * (hb // 2) * cs
    out = torch.full((numel + TAIL,), 7.0, dtype=DT[prec], device="cuda")
    G.lib.jck_conv_down_affine(prec, _nhwc4(x, prec), _pack_down(G, w, prec), scale.cuda(), shift.cuda(), SLOPE, out, n, hb, hb, cb, cs,
                               G.cur_stream())
    torch.cuda.synchronize()
    what = f"conv_down_affine {shape} {PREC_NAME[prec]}"
    assert G.lib.jck_last_launch().decode() == DOWN_KERNEL[shape][prec], what
    assert bool((out[numel:] == 7.0).all()), f"{what}: wrote past the output"
    _expect_equal(out[:numel].view(n, hb // 2, hb // 2, cs), ref, prec, what)


@pytest.mark.parametrize("shape", [(3, 16, 3, 64), (3, 8, 128, 256)], ids=lambda s: "x".join(map(str, s)))
def test_conv_down_affine_slope_is_a_plain_fp32_multiply(G, shape):
    """slope = 0.2f: the negative side equals torch's fp32 product of the same t with the same fp32 slope, bit for bit (f32)"""
    n, hb, cb, cs = shape
    x, w, y = _down_exact_data(shape)
    scale, shift = _affine_down(cs)
    t32 = _t64(y, scale, shift).float()                            # the one rounding of the exact t: fmaf's result
    exp = torch.where(t32 > 0, t32, t32 * torch.tensor(0.2, dtype=torch.float32)).permute(0, 2, 3, 1).contiguous()
    out = torch.empty(n, hb // 2, hb // 2, cs, device="cuda")
    G.lib.jck_conv_down_affine(1, _nhwc4(x, 1), _pack_down(G, w, 1), scale.cuda(), shift.cuda(), 0.2, out, n, hb, hb, cb, cs, G.cur_stream())
    assert torch.equal(out.cpu(), exp)


@pytest.mark.parametrize("cb", [3, 64])
def test_conv_down_affine_nan_and_negative_zero(G, cb):
    """a NaN input pixel reaches exactly the outputs whose 4x4 window holds it (t > 0 ? t : t * slope passes NaN); a -0
    pre-activation stores -0"""
    n, hb, cs = 2, 8, 64 if cb == 3 else 128
    x = torch.zeros(n, cb, hb, hb)
    x[1, cb - 1, 3, 5] = float("nan")
    w = torch.ones(cs, cb, 4, 4)
    ref = F.conv2d(x, w, None, 2, 1) * 2.0 - 1.0
    ref = torch.where(ref > 0, ref, ref * SLOPE)
    assert int(torch.isnan(ref[:, 0]).sum()) == 4 and not bool(torch.isnan(ref[0]).any())
    for prec in (0, 1, 2):
        out = torch.empty(n, hb // 2, hb // 2, cs, dtype=DT[prec], device="cuda")
        wp = _pack_down(G, w, prec)
        G.lib.jck_conv_down_affine(prec, _nhwc4(x, prec), wp, torch.full((cs,), 2.0, device="cuda"), torch.full((cs,), -1.0, device="cuda"),
                                   SLOPE, out, n, hb, hb, cb, cs, G.cur_stream())
        got = out.float().cpu().permute(0, 3, 1, 2)
        assert torch.equal(torch.isnan(got), torch.isnan(ref)), PREC_NAME[prec]
        assert torch.equal(torch.nan_to_num(got), torch.nan_to_num(ref)), PREC_NAME[prec]
        # acc = +0, scale = -1, shift = -0: t = fmaf(-1, +0, -0) = -0, not > 0, and -0 * slope = -0
        G.lib.jck_conv_down_affine(prec, _nhwc4(torch.zeros(n, cb, hb, hb), prec), wp, torch.full((cs,), -1.0, device="cuda"),
                                   torch.full((cs,), -0.0, device="cuda"), SLOPE, out, n, hb, hb, cb, cs, G.cur_stream())
        z = out.float().cpu()
        assert bool((z == 0).all()) and bool(torch.signbit(z).all()), PREC_NAME[prec]


def test_conv_down_affine_refuses_what_it_was_not_built_for(G):
    from hipgan import JckError
    out = torch.zeros(1, 4, 4, 512, device="cuda")
    x, wp = torch.zeros(1, 8, 8, 256, device="cuda"), torch.zeros(512 * 16 * 256, device="cuda")
    aux = torch.ones(2 * 512 + 8, device="cuda")
    sc, sh = aux[:512], aux[512:1024]
    call = lambda cb, cs, s=sc, h=sh: G.lib.jck_conv_down_affine(1, x, wp, s, h, SLOPE, out, 1, 8, 8, cb, cs, G.cur_stream())
    for cb, cs in ((8, 64), (32, 64), (96, 128), (4, 128), (3, 256), (64, 32), (64, 96), (128, 16)):
        with pytest.raises(JckError, match="conv_down_affine"):
            call(cb, cs)
    with pytest.raises(JckError, match="16-byte aligned"):
        call(64, 128, aux[1:129], sh)
    with pytest.raises(JckError, match="16-byte aligned"):
        call(64, 128, sc, aux[513:641])
    with pytest.raises(JckError):
        call(64, 128, None, sh)
    with pytest.raises(JckError, match="bad prec"):
        G.lib.jck_conv_down_affine(7, x, wp, sc, sh, SLOPE, out, 1, 8, 8, 64, 128, G.cur_stream())
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0


@pytest.mark.parametrize("prec", [0, 1, 2], ids=PREC_NAME.get)
def test_relu_affine_is_untouched(G, prec):
    """the generator's Epi::ReluAffine instantiations keep t < 0 ? 0 : t: jck_conv_up_affine still equals the exact reference"""
    shape = (1, 4, 64, 32)
    n, hs, cs, cb = shape
    x, w, y = _up_exact_data(shape)
    scale, shift = _affine_exact(cb)
    ref = _ref_affine(y, scale, shift)
    out = torch.empty(n, 2 * hs, 2 * hs, cb, dtype=DT[prec], device="cuda")
    wp = torch.empty(4 * G.lib.jck_pad_rows(cb) * 4 * cs, dtype=DT[prec], device="cuda")
    G.lib.jck_pack_up(prec, w.cuda().contiguous(), cs, cb, wp, G.cur_stream())
    G.lib.jck_conv_up_affine(prec, x.permute(0, 2, 3, 1).contiguous().to(DT[prec]).cuda(), wp, scale.cuda(), shift.cuda(), out, n, hs, hs, cs, cb,
                             G.cur_stream())
    _expect_equal(out, ref, prec, f"conv_up_affine {PREC_NAME[prec]}")


@pytest.mark.parametrize("prec", [0, 1], ids=PREC_NAME.get)
@pytest.mark.parametrize("b,k", [(1, 256), (5, 8192), (3, 16384)])
def test_score_head(G, b, k, prec):
    """integers: x in -3..3, w in -2..2 - every partial sum an integer below 6 * K < 2^24, so the logit is exact in any order; the
    sigmoid is 1 / (1 + expf(-s)) within 4 ulp (2^-23 relative each) of the fp64 value: expf to an ulp, the sum and the correctly rounded
    quotient half an ulp each"""
    x = torch.randint(-3, 4, (b, k), generator=_gen(41)).float()
    w = torch.randint(-2, 3, (k,), generator=_gen(42)).float()
    bias = torch.tensor([3.0])
    ref = x.double() @ w.double() + 3.0
    logit = torch.full((b + 8,), 7.0, device="cuda")
    prob = torch.full((b + 8,), 7.0, device="cuda")
    G.lib.jck_score_head(prec, x.to(DT[prec]).cuda(), w.cuda(), bias.cuda(), b, k, logit, prob, G.cur_stream())
    assert torch.equal(logit[:b].cpu().double(), ref) and bool((logit[b:] == 7.0).all()) and bool((prob[b:] == 7.0).all())
    p64 = torch.sigmoid(ref)
    assert bool(((prob[:b].cpu().double() - p64).abs() <= 4 * 2.0 ** -23 * torch.clamp(p64, min=2.0 ** -126)).all())
    G.lib.jck_score_head(prec, x.to(DT[prec]).cuda(), w.cuda(), None, b, k, logit, None, G.cur_stream())
    assert torch.equal(logit[:b].cpu().double(), ref - 3.0) and bool((prob[b:] == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------------
# engine
# ---------------------------------------------------------------------------------------------------------------------
_engines = {}
ENGINES = [pytest.param(f, p, id=f"{f}-{p}") for f in ("dcgan", "cgan") for p in ("bf16", "f32")]
RTOL = {"f32": 2e-4, "bf16": 1.2e-1}


def _d_state(orc_d):
    """the oracle's discriminator with non-trivial running statistics: mean ~ N(0, 0.1), var ~ U(0.5, 1.5)"""
    g = _gen(777)
    d = {k: v.clone() for k, v in orc_d.items()}
    for k in sorted(d):
        if k.endswith("running_mean"):
            d[k] = torch.randn(d[k].shape, generator=g) * 0.1
        elif k.endswith("running_var"):
            d[k] = torch.rand(d[k].shape, generator=g) + 0.5
    return d


def _z(n, seed, family):
    g = _gen(seed)
    z = torch.randn(n, 100, generator=g)
    lab = F.one_hot(torch.randint(0, 100, (n,), generator=g), 100).to(torch.int64) if family == "cgan" else None
    return z, lab


def _engine(family, prec, batch=8, size=64):
    """one engine per configuration for the module: oracle weights, D's running statistics drawn, G's fitted by 30 train-mode batches"""
    key = (family, prec, batch, size)
    if key not in _engines:
        from hipgan.engine import CganEngine, DcganEngine
        from oracle.gan_oracle import GanOracle
        kw = {"image_size": size} if size != 64 else {}
        orc = GanOracle(family, lr=2e-4, seed=12345, **kw)
        eng = (CganEngine if family == "cgan" else DcganEngine)(batch=batch, prec=prec, **kw)
        eng.load_state(orc.g, _d_state(orc.d))
        for s in range(30):
            eng.sample(*_z(batch, 100 + s, family))
        _engines[key] = eng
    return _engines[key]


def _images(n, seed, size=64):
    return torch.rand(n, 3, size, size, generator=_gen(seed)) * 2 - 1


def _module_prob(eng, family, x, lab, size=64):
    from model import CGAN, DCGAN
    d = CGAN.Discriminator() if family == "cgan" else DCGAN.Discriminator(**({"image_size": size} if size != 64 else {}))
    d.load_state_dict(eng.state_dicts()[1])
    d = d.cuda().eval()
    d.prec = "f32"
    with torch.no_grad():
        p = d(x.cuda(), lab.cuda()) if family == "cgan" else d(x.cuda())
    return p.reshape(-1)


def _check_scores(logit, prob, ref_p, prec, what):
    ref_l = torch.logit(ref_p.double())
    assert float(ref_l.abs().max()) < 8.0, f"{what}: |logit| {float(ref_l.abs().max()):.2f}: the fp32 probability no longer pins it"
    assert logit.dtype == torch.float32 and prob.dtype == torch.float32 and logit.shape == prob.shape == ref_p.shape
    perr = float((prob.double().cpu() - ref_p.double().cpu()).abs().max())
    print(f"{what}: max |prob - ref| {perr:.3e}")
    _parity(logit, ref_l, prec, what + " logit")
    assert perr < RTOL[prec], f"{what}: |prob - ref| {perr:.3e}"
    assert torch.equal(prob, torch.sigmoid(logit)) or float((prob - torch.sigmoid(logit)).abs().max()) < 1e-6


def _arenas(eng):
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in eng.arenas.items()}


@pytest.mark.parametrize("family,prec", ENGINES)
def test_score_matches_the_module_in_eval_mode(family, prec):
    eng = _engine(family, prec)
    x, (_, lab) = _images(8, 1), _z(8, 2, family)
    before = _arenas(eng)
    logit, prob = eng.score(x, lab)
    _check_scores(logit, prob, _module_prob(eng, family, x, lab), prec, f"{family} {prec}")
    nz = torch.randn(8, 3, 64, 64, generator=_gen(3))
    logit_n, prob_n = eng.score(x, lab, noise=nz)
    assert not torch.equal(logit_n, logit)
    _check_scores(logit_n, prob_n, _module_prob(eng, family, 0.9 * x + 0.1 * nz, lab), prec, f"{family} {prec} with noise")
    # nothing was written: parameters, gradients, Adam moments, both networks' BatchNorm buffers and num_batches_tracked
    after = _arenas(eng)
    assert set(before) == set(after) and all(torch.equal(before[k], after[k]) for k in before)


@pytest.mark.parametrize("family,prec", ENGINES)
def test_score_uint8_and_rows(family, prec):
    """uint8 NHWC equals the float path on u8 / 127.5 - 1; n = 1, 5, 20 (three chunks of a batch-8 engine): every row is that of a
    single-row call; changing image 2 leaves logit 3 alone"""
    eng = _engine(family, prec)
    u8 = torch.randint(0, 256, (20, 64, 64, 3), generator=_gen(4), dtype=torch.uint8)
    _, lab = _z(20, 5, family)
    xf = (u8.float() / 127.5 - 1.0).permute(0, 3, 1, 2).contiguous()
    full = eng.score(u8, lab)
    assert full[0].shape == (20,) and all(torch.equal(a, b) for a, b in zip(full, eng.score(xf, lab)))
    sub = lambda lo, hi: (xf[lo:hi], None if lab is None else lab[lo:hi])
    for lo, hi in ((0, 1), (3, 8), (7, 8), (8, 16), (19, 20)):
        got = eng.score(*sub(lo, hi))
        assert torch.equal(got[0], full[0][lo:hi]) and torch.equal(got[1], full[1][lo:hi]), (lo, hi)
    for i in range(8):
        assert torch.equal(eng.score(*sub(i, i + 1))[0], full[0][i:i + 1]), i
    x2 = xf[:8].clone()
    x2[2] = -x2[2]
    other = eng.score(x2, None if lab is None else lab[:8])[0]
    assert torch.equal(other[3], full[0][3]) and not torch.equal(other[2], full[0][2])


@pytest.mark.parametrize("family,prec", ENGINES)
def test_score_latents(family, prec):
    """D(G(z)) with the images left on the device: bit for bit the score of the generator's current output, and the score of the
    fp32 copy of those images (the copy holds exactly the stored values, so the input transform rounds nothing)"""
    eng = _engine(family, prec)
    z, lab = _z(20, 6, family)
    before = _arenas(eng)
    logit, prob = eng.score_latents(z, lab)
    assert logit.shape == (20,) and bool(torch.isfinite(logit).all())
    img = eng.sample(z[8:16], None if lab is None else lab[8:16], bn="running")
    cur = eng.score_current(8, None if lab is None else lab[8:16])
    assert torch.equal(cur[0], logit[8:16]) and torch.equal(cur[1], prob[8:16])
    via = eng.score(img, None if lab is None else lab[8:16])
    assert torch.equal(via[0], logit[8:16])
    after = _arenas(eng)
    assert all(torch.equal(before[k], after[k]) for k in before)


def test_score_image_size_128():
    eng = _engine("dcgan", "f32", batch=2, size=128)
    x = _images(2, 7, 128)
    logit, prob = eng.score(x)
    _check_scores(logit, prob, _module_prob(eng, "dcgan", x, None, 128), "f32", "dcgan 128 f32")


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graph"])
def test_score_between_two_training_steps_changes_no_bit(graphs):
    """A training engine (DCGAN, B = 8, bf16) with score calls between every two steps: scalars and every arena equal those of the
    run without them, bit for bit.  eager: the next batch announced, so that its D(real) forward is in flight; graph: the steps
    replayed from captured graphs on the engine's own stream (the first runs eagerly), scoring on the caller's."""
    from hipgan.engine import DcganEngine
    from oracle.gan_oracle import build_params
    from util import synth_images
    B, steps = 8, 4 if graphs else 3
    imgs = synth_images(B * steps).cuda()
    x, z = _images(5, 8), _z(5, 9, "dcgan")[0]
    res = []
    for with_score in (False, True):
        torch.manual_seed(12345)
        g, d = build_params("dcgan")
        eng = DcganEngine(batch=B, prec="bf16", device="cuda:0")
        eng.graphs = graphs
        eng.load_state(g, d)
        eng.set_noise_seed(77)
        gen = torch.Generator(device="cuda").manual_seed(5)
        scal = []
        for s in range(steps):
            kw = dict(next_real=imgs[(s + 1) * B:(s + 2) * B]) if s + 1 < steps and not graphs else {}
            eng.step_async(imgs[s * B:(s + 1) * B], None, 2e-4, generator=gen, **kw)
            if kw:
                assert eng._prefetched_real is not None
            if with_score:
                logit, _ = eng.score(x)
                cur, _ = eng.score_current(5)                        # the step's own fake batch, where it lies
                assert bool(torch.isfinite(logit).all()) and bool(torch.isfinite(cur).all())
                if kw:
                    assert eng._prefetched_real is not None          # scoring did not drop the prefetched pass
            scal.append(eng.scalars())
        torch.cuda.synchronize()
        assert (len(eng._graph_cache) > 0) == graphs
        res.append((scal, {k: v.clone() for k, v in eng.arenas.items()}))
    assert res[0][0] == res[1][0], (res[0][0], res[1][0])
    for k, v in res[0][1].items():
        assert torch.equal(v, res[1][1][k]), k


def _ckpt(family="dcgan"):
    eng = _engine(family, "bf16")
    g, d = eng.state_dicts()
    return {"model_g": g, "model_d": d}


def test_sampler_without_discriminator_refuses():
    from hipgan import JckError
    from hipgan.sampler import Sampler
    s = Sampler.from_checkpoint(_ckpt(), "DCGAN", batch=8)
    with pytest.raises(JckError, match="discriminator"):
        s.score(torch.zeros(2, 64, 64, 3, dtype=torch.uint8))
    with pytest.raises(JckError, match="discriminator"):
        s.images(4, select="top", oversample=2)
    # the native entry point refuses an engine whose D operands were never packed
    from hipgan.engine import DcganEngine
    import gpu_util as G
    e = DcganEngine(batch=4, prec="bf16")
    out = torch.zeros(4, device="cuda")
    with pytest.raises(JckError, match="never packed"):
        G.lib.jck_engine_score(e._h, torch.zeros(4, 3, 64, 64, device="cuda"), None, None, 4, out, None, G.cur_stream())


def test_sampler_select():
    from hipgan.sampler import Sampler, latents
    s = Sampler.from_checkpoint(_ckpt(), "DCGAN", batch=8, with_d=True)
    z = latents(32, 11)
    logit = s.score_latents(z)[0].cpu()
    best = torch.sort(logit.double(), descending=True, stable=True).indices[:16]
    img, info = s.images(16, seed=11, select="top", oversample=2, return_info=True)
    assert img.shape == (16, 64, 64, 3) and img.dtype == torch.uint8 and info["drawn"] == 32
    assert torch.equal(info["z"], z[best]) and torch.equal(info["logit"], logit[best]) and info["prob"].shape == (16,)
    img2, l2, p2 = s.from_latents_scored(z[best])
    assert torch.equal(img2, img) and torch.equal(l2.cpu(), info["logit"]) and torch.equal(p2.cpu(), info["prob"])
    from hipgan import JckError
    with pytest.raises(JckError, match="oversample"):
        s.images(2, seed=1, select="drs", oversample=51)
    assert torch.equal(img, s.from_latents(z[best])) and torch.equal(img, s.images(16, seed=11, select="top", oversample=2))
    assert float(info["logit"].min()) >= float(np.sort(logit.numpy())[15])
    a, ia = s.images(16, seed=12, select="drs", oversample=2, return_info=True)
    b, ib = s.images(16, seed=12, select="drs", oversample=2, return_info=True)
    assert a.shape == (16, 64, 64, 3) and torch.equal(a, b) and torch.equal(ia["z"], ib["z"]) and ia["drawn"] == ib["drawn"]
    assert ia["drawn"] % 32 == 0 and 32 <= ia["drawn"] <= 50 * 16 and ia["z"].shape == (16, 100)
    # the kept logits are the scores of the kept latents
    assert torch.equal(s.score_latents(ia["z"])[0].cpu(), ia["logit"])
    assert torch.equal(a, s.from_latents(ia["z"]))


def test_generate_score_cli(tmp_path):
    import generate
    path = str(tmp_path / "ckpt.pt")
    torch.save(_ckpt(), path)
    out = tmp_path / "out"
    assert generate.main(["-m", "DCGAN", "--checkpoint", path, "--num", "12", "-b", "8", "--seed", "3", "--score", "--out", str(out)]) == 0
    f = np.load(os.path.join(str(out), "images.npz"))
    assert f["images"].shape == (12, 64, 64, 3) and f["logit"].shape == (12,) and f["prob"].shape == (12,)
    assert f["logit"].dtype == np.float32 and np.all((f["prob"] > 0) & (f["prob"] < 1))
    plain = tmp_path / "plain"
    assert generate.main(["-m", "DCGAN", "--checkpoint", path, "--num", "12", "-b", "8", "--seed", "3", "--out", str(plain)]) == 0
    p = np.load(os.path.join(str(plain), "images.npz"))
    assert sorted(p.files) == ["images", "z"] and p["images"].tobytes() == f["images"].tobytes()
    sc = tmp_path / "scored"
    assert generate.main(["-m", "DCGAN", "--checkpoint", path, "-b", "8", "--score_images", os.path.join(str(out), "images.npz"), "--out", str(sc)]) == 0
    g = np.load(os.path.join(str(sc), "scores.npz"))
    assert g["logit"].shape == (12,) and g["prob"].shape == (12,) and np.all(np.isfinite(g["logit"]))
    from hipgan.sampler import Sampler
    s = Sampler.from_checkpoint(path, "DCGAN", batch=8, with_d=True)
    assert np.array_equal(s.score(torch.from_numpy(f["images"]))[0].cpu().numpy(), g["logit"])
    top = tmp_path / "top"
    assert generate.main(["-m", "DCGAN", "--checkpoint", path, "--num", "8", "-b", "8", "--select", "top", "--oversample", "2", "--score",
                          "--out", str(top)]) == 0
    t = np.load(os.path.join(str(top), "images.npz"))
    assert t["images"].shape == (8, 64, 64, 3) and np.all(np.diff(t["logit"]) <= 0)
