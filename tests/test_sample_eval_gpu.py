"""Generator inference: the products with the folded eval-mode BatchNorm + ReLU in their epilogue (jck_conv_up_affine,
jck_g1_fwd_affine), jck_bn_eval_aux, jck_img_to_u8, and the engine's eval sampling (jck_engine_sample_ex, DcganEngine.sample with
bn="running").

Exact cases (the integer-data pattern of tests/test_exact_gpu.py): activations 0..15 and weights in {-1, 0, 1} - every partial sum
is an integer below 15 * K < 2^24, exact in fp32 in any order and exact as bf16 operands; scale[c] = 2^(c - C/2), all distinct, so
the product with the accumulator is exact; shift[c] = distinct integers in [-C/2, C/2).  The fp32 result is the one rounding of the
exact scale * y + shift (a fused or an unfused multiply-add give the same, the product being exact), the bf16 result one more.  The
reference is evaluated in fp64: exact where the terms span at most 53 bits, and where they span more (C = 128: 2^63 * y against
|shift| <= 64, or 2^-64 * y against a shift) the smaller term is below a quarter ulp of the fp32 result either way, so rounding
through fp64 first cannot move it.  A wrong channel or a missed clip changes bits, and so does a rounding of y to bf16 before the
affine: every case asserts that at least a fifth of its sums are not bf16 numbers (odd values above 256).

Real-valued cases: the form and bounds of tests/test_ops_gpu.py::test_conv_up / test_g1 - G.check, maximum error relative to the
reference's maximum, 3e-6 (f32, gpu_util.TOL) and 1.5e-2 (bf16); those tests hold f32 and bf16, so do these.

Engine parity: the bound tests/test_modules_gpu.py puts on the module forward, per element |a - b| <= 1e-6 + rtol * max(|b|, rms b)
with rtol 2e-4 (f32) and 1.2e-1 (bf16), here on every element instead of a sample."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
PREC_NAME = {0: "bf16", 1: "f32", 2: "bf16x3"}
DT = {0: torch.bfloat16, 1: torch.float32, 2: torch.float32}
TAIL = 1024


@pytest.fixture(scope="module")
def G():
    import gpu_util
    return gpu_util


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=_gen(seed)).float()


def _biased_w(shape, seed):
    """{-1, 0, 1} with P(+1) = 0.6, P(-1) = 0.2: sums of several hundred against activations 0..3"""
    u = torch.rand(shape, generator=_gen(seed))
    return (u < 0.6).float() - (u > 0.8).float()


def _affine_exact(c):
    k = torch.arange(c)
    return torch.pow(2.0, (k - c // 2).double()).float(), (((k * 7) % c) - c // 2).float()


def _nhwc(x, prec):
    return x.permute(0, 2, 3, 1).contiguous().to(DT[prec]).cuda()


def _out(numel, prec):
    return torch.full((numel + TAIL,), 7.0, dtype=DT[prec], device="cuda")


def _tail_ok(buf, numel, what):
    assert bool((buf[numel:] == 7.0).all()), f"{what}: wrote past the output"


def _ref_affine(y64, scale, shift):
    return torch.relu(y64 * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1))


def _expect_equal(got, ref64, prec, what):
    exp = ref64.permute(0, 2, 3, 1).contiguous().float().to(DT[prec]).cuda()
    assert got.shape == exp.shape
    if not torch.equal(got, exp):
        bad = torch.nonzero(got != exp)
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {bad.shape[0]} of {exp.numel()} elements differ, first at (n, y, x, c) = {i}: "
                             f"got {float(got[i]):.10g} exact {float(exp[i]):.10g}")


UP_SHAPES = [(1, 4, 64, 32), (3, 4, 128, 64), (2, 8, 32, 16)]
# batch-256 shapes (G.conv3 of the 64x64 net): the tiles the dispatch takes only at >= 250 / 512 / 256 workgroups - 128x256
# wave-specialised (bf16, M % 256 == 0), 128x128 LDS-DMA (bf16, 257 images: M % 256 != 0), 128x128 register-staged (f32, bf16x3)
BIG, BIG1 = (256, 8, 256, 128), (257, 8, 256, 128)
UP_KERNEL = {(1, 4, 64, 32): ("igemm_dma<64,128,2>", "igemm<f32,64,128>", "igemm<bf16x3,64,128>"),
             (3, 4, 128, 64): ("igemm_dma<64,128,2>", "igemm<f32,64,128>", "igemm<bf16x3,64,128>"),
             (2, 8, 32, 16): ("igemm<bf16,16,256>", "igemm<f32,16,256>", "igemm<bf16x3,16,256>"),
             BIG: ("igemm_dma<128,256,3,ws,8>", "igemm<f32,128,128>", "igemm<bf16x3,128,128>"),
             BIG1: ("igemm_dma<128,128,2>", None, None)}
UP_EXACT = [pytest.param(s, p, id="x".join(map(str, s)) + "-" + PREC_NAME[p]) for s in UP_SHAPES + [BIG1, BIG] for p in (0, 1, 2)
            if UP_KERNEL[s][p]]
_up_cache = {}


def _up_exact_data(shape):
    if shape not in _up_cache:
        n, hs, cs, cb = shape
        if shape == BIG:                        # the first 256 images of the 257-image case: one CPU reference for both
            x, w, y = _up_exact_data(BIG1)
            _up_cache[shape] = (x[:256], w, y[:256])
            return _up_cache[shape]
        x, w = _ints((n, cs, hs, hs), 0, 15, 11), _biased_w((cs, cb, 4, 4), 12)
        assert 15 * 4 * cs < 2 ** 24                               # bounds every partial sum (4 taps x Cs terms of at most 15)
        y = F.conv_transpose2d(x, w, None, 2, 1).double()          # integers below 2^24: the fp32 sums are exact in any order
        _not_bf16(y, f"conv_up {shape}")
        _up_cache[shape] = (x, w, y)
    return _up_cache[shape]


def _not_bf16(y, what):
    f = float((y.float().to(torch.bfloat16).double() != y).double().mean())
    assert f > 0.2, f"test data, {what}: only {f:.2f} of the sums would change if rounded to bf16"


@pytest.mark.parametrize("shape,prec", UP_EXACT)
def test_conv_up_affine_exact(G, shape, prec):
    n, hs, cs, cb = shape
    x, w, y = _up_exact_data(shape)
    scale, shift = _affine_exact(cb)
    ref = _ref_affine(y, scale, shift)
    assert float((ref == 0).double().mean()) > 0.01, "test data: the ReLU never clips"
    numel = n * 4 * hs * hs * cb
    out = _out(numel, prec)
    wp = torch.empty(4 * G.lib.jck_pad_rows(cb) * 4 * cs, dtype=DT[prec], device="cuda")
    G.lib.jck_pack_up(prec, w.cuda().contiguous(), cs, cb, wp, G.cur_stream())
    G.lib.jck_conv_up_affine(prec, _nhwc(x, prec), wp, scale.cuda(), shift.cuda(), out, n, hs, hs, cs, cb, G.cur_stream())
    torch.cuda.synchronize()
    what = f"conv_up_affine {shape} {PREC_NAME[prec]}"
    assert G.lib.jck_last_launch().decode() == UP_KERNEL[shape][prec], what
    _tail_ok(out, numel, what)
    _expect_equal(out[:numel].view(n, 2 * hs, 2 * hs, cb), ref, prec, what)


_g1_cache = {}


def _g1_exact_data(b, ci, co):
    if b not in _g1_cache:
        z, w = _ints((b, ci, 1, 1), 0, 15, 21), _biased_w((ci, co, 4, 4), 22)
        _g1_cache[b] = (z, w, F.conv_transpose2d(z.double(), w.double(), None, 1, 0))
        _not_bf16(_g1_cache[b][2], f"g1 B={b}")
    return _g1_cache[b]


@pytest.mark.parametrize("prec", [0, 1, 2], ids=PREC_NAME.get)
@pytest.mark.parametrize("b", [1, 3, 8])
def test_g1_fwd_affine_exact(G, b, prec):
    ci, cip, co = 100, 128, 64
    z, w, y = _g1_exact_data(b, ci, co)
    scale, shift = _affine_exact(co)
    ref = _ref_affine(y, scale, shift)
    assert float((ref == 0).double().mean()) > 0.01
    zp = torch.zeros(b, cip)
    zp[:, :ci] = z.view(b, ci)
    wp = torch.empty(16 * co * cip, dtype=DT[prec], device="cuda")
    G.lib.jck_pack_g1(prec, w.cuda().contiguous(), ci, co, cip, wp, G.cur_stream())
    numel = b * 16 * co
    out = _out(numel, prec)
    G.lib.jck_g1_fwd_affine(prec, zp.to(DT[prec]).cuda(), wp, scale.cuda(), shift.cuda(), out, b, cip, co, G.cur_stream())
    torch.cuda.synchronize()
    what = f"g1_fwd_affine B={b} {PREC_NAME[prec]}"
    assert G.lib.jck_last_launch().decode() == ("igemm_dma<128,64,3,ws>", "igemm<f32,128,64>", "igemm<bf16x3,128,64>")[prec], what
    _tail_ok(out, numel, what)
    _expect_equal(out[:numel].view(b, 4, 4, co), ref, prec, what)


def test_affine_epilogue_passes_nan(G):
    """relu(NaN) is NaN in torch; a max(v, 0) would return 0"""
    n, hs, cs, cb = 1, 4, 64, 32
    x = torch.zeros(n, cs, hs, hs)
    x[0, 0, 1, 1] = float("nan")
    w = torch.ones(cs, cb, 4, 4)
    ref = torch.relu(F.conv_transpose2d(x, w, None, 2, 1) * 2.0 - 1.0)
    assert bool(torch.isnan(ref).any()) and not bool(torch.isnan(ref).all())
    for prec in (0, 1, 2):
        out = torch.empty(n, 2 * hs, 2 * hs, cb, dtype=DT[prec], device="cuda")
        G.lib.jck_conv_up_affine(prec, _nhwc(x, prec), _pack_up(G, w, prec), torch.full((cb,), 2.0, device="cuda"),
                                 torch.full((cb,), -1.0, device="cuda"), out, n, hs, hs, cs, cb, G.cur_stream())
        got = out.float().cpu().permute(0, 3, 1, 2)
        assert torch.equal(torch.isnan(got), torch.isnan(ref)), PREC_NAME[prec]
        assert torch.equal(torch.nan_to_num(got), torch.nan_to_num(ref)), PREC_NAME[prec]


def test_conv_up_affine_refuses_thin_outputs(G):
    """<= 4 output channels run on kernels that have no affine epilogue: an error, not the plain product"""
    from hipgan import JckError
    n, hs, cs = 1, 4, 64
    for cb in (3, 4):
        x, out = torch.zeros(n, hs, hs, cs, device="cuda"), torch.zeros(n, 2 * hs, 2 * hs, 4, device="cuda")
        wp = torch.zeros(16 * 9 * cs, device="cuda")
        sc = torch.ones(4, device="cuda")
        with pytest.raises(JckError, match="Cb must be a power of two >= 8"):
            G.lib.jck_conv_up_affine(1, x, wp, sc, sc, out, n, hs, hs, cs, cb, G.cur_stream())
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0


def _pack_up(G, w, prec):
    cs, cb = w.shape[0], w.shape[1]
    wp = torch.empty(4 * G.lib.jck_pad_rows(cb) * 4 * cs, dtype=DT[prec], device="cuda")
    G.lib.jck_pack_up(prec, w.cuda().contiguous(), cs, cb, wp, G.cur_stream())
    return wp


def _bn_for(scale, shift):
    """BatchNorm parameters whose eval-mode affine is (scale, shift) up to rounding: running_var + eps = 1, mean 0"""
    c = scale.numel()
    return scale.clone(), shift.clone(), torch.zeros(c), torch.full((c,), 1.0 - 1e-5)


def _eval_aux(G, layers, eps=1e-5):
    """jck_bn_eval_aux over [(gamma, beta, mean, var)] of device tensors -> list of aux [4C]"""
    n = len(layers)
    aux = [torch.full((4 * l[0].numel(),), float("nan"), device="cuda") for l in layers]
    arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
    G.lib.jck_bn_eval_aux(n, arr([l[0] for l in layers]), arr([l[1] for l in layers]), arr([l[2] for l in layers]),
                          arr([l[3] for l in layers]), arr(aux), (ctypes.c_int * n)(*[l[0].numel() for l in layers]), eps, G.cur_stream())
    torch.cuda.synchronize()
    return aux


def test_bn_eval_aux(G):
    """the three-line fp32 formula (IEEE arithmetic, one rounding per operation), bit for bit; several layers - C below, at and above
    one block of 256 - in one launch"""
    g = _gen(5)
    host = []
    for c in (8, 64, 256, 520):
        host.append((torch.randn(c, generator=g), torch.randn(c, generator=g), torch.randn(c, generator=g), torch.rand(c, generator=g) * 3 + 1e-3))
    layers = [tuple(t.cuda() for t in l) for l in host]
    before = [tuple(t.clone() for t in l) for l in layers]
    aux = _eval_aux(G, layers)
    eps = torch.tensor(1e-5, dtype=torch.float32)
    rn = lambda t: t.float().double()                      # one rounding to fp32 of an fp64 result
    for (gamma, beta, mean, var), a, l, b in zip(host, aux, layers, before):
        # the three lines in fp32, every operation rounded once: fp64 holds an fp32 product or sum exactly, and a square root or a
        # quotient of fp32 operands rounded to fp64 and then to fp32 is the correctly rounded fp32 result (53 >= 2 * 24 + 2) - torch's
        # own vectorised fp32 sqrt / reciprocal on the CPU are not correctly rounded for every operand
        invstd = rn(1.0 / rn(torch.sqrt(rn(var.double() + eps.double()))))
        scale = rn(gamma.double() * invstd)
        shift = rn(beta.double() - rn(mean.double() * scale)).float()
        invstd, scale = invstd.float(), scale.float()
        got, exp = a.cpu(), torch.cat([scale, shift, mean, invstd])
        if not torch.equal(got, exp):
            i = int(torch.nonzero(got != exp)[0])
            c = gamma.numel()
            raise AssertionError(f"C = {c}: {int((got != exp).sum())} of {4 * c} differ, first in {('scale', 'shift', 'mean', 'invstd')[i // c]}[{i % c}]: "
                                 f"got {got[i].item().hex()} exp {exp[i].item().hex()} (var {var[i % c].item().hex()} gamma {gamma[i % c].item().hex()})")
        assert all(torch.equal(x, y) for x, y in zip(l, b)), "inputs were written"


@pytest.mark.parametrize("prec", [1, 0], ids=PREC_NAME.get)
@pytest.mark.parametrize("shape", UP_SHAPES + [(2, 8, 256, 128)], ids=lambda s: "x".join(map(str, s)))
def test_conv_up_affine_real(G, shape, prec):
    """against fp32 CPU F.batch_norm(training=False) + relu; bound: G.TOL (3e-6 f32, 1.5e-2 bf16) relative to the reference's maximum"""
    n, hs, cs, cb = shape
    g = _gen(2)
    x = G.rnd(torch.randn(n, cs, hs, hs, generator=g), prec)
    w = torch.randn(cs, cb, 4, 4, generator=g) * 0.05
    scale, shift = torch.rand(cb, generator=g) * 1.5 + 0.5, torch.rand(cb, generator=g) * 2 - 1
    gamma, beta, mean, var = _bn_for(scale, shift)
    ref = torch.relu(F.batch_norm(F.conv_transpose2d(x, G.rnd(w, prec), None, 2, 1), mean, var, gamma, beta, False, 0.1, 1e-5))
    aux = _eval_aux(G, [(gamma.cuda(), beta.cuda(), mean.cuda(), var.cuda())])[0]
    out = torch.full((n, 2 * hs, 2 * hs, cb), 7.0, dtype=DT[prec], device="cuda")
    G.lib.jck_conv_up_affine(prec, _nhwc(x, prec), _pack_up(G, w, prec), aux[:cb], aux[cb:2 * cb], out, n, hs, hs, cs, cb, G.cur_stream())
    torch.cuda.synchronize()
    G.check(G.from_nhwc(out), ref, G.TOL[prec], f"conv_up_affine {shape}")


@pytest.mark.parametrize("prec", [1, 0], ids=PREC_NAME.get)
@pytest.mark.parametrize("cfg", [(8, 100, 128, 512), (5, 200, 256, 512), (3, 100, 128, 64)])
def test_g1_fwd_affine_real(G, cfg, prec):
    """as test_ops_gpu.py::test_g1, bound G.TOL relative to the reference's maximum"""
    b, ci, cip, co = cfg
    g = _gen(4)
    z = G.rnd(torch.randn(b, ci, 1, 1, generator=g), prec)
    w = torch.randn(ci, co, 4, 4, generator=g) * 0.05
    scale, shift = torch.rand(co, generator=g) * 1.5 + 0.5, torch.rand(co, generator=g) * 2 - 1
    gamma, beta, mean, var = _bn_for(scale, shift)
    ref = torch.relu(F.batch_norm(F.conv_transpose2d(z, G.rnd(w, prec), None, 1, 0), mean, var, gamma, beta, False, 0.1, 1e-5))
    aux = _eval_aux(G, [(gamma.cuda(), beta.cuda(), mean.cuda(), var.cuda())])[0]
    zp = torch.zeros(b, cip)
    zp[:, :ci] = z.view(b, ci)
    wp = torch.empty(16 * co * cip, dtype=DT[prec], device="cuda")
    G.lib.jck_pack_g1(prec, w.cuda(), ci, co, cip, wp, G.cur_stream())
    out = torch.empty(b, 4, 4, co, dtype=DT[prec], device="cuda")
    G.lib.jck_g1_fwd_affine(prec, zp.to(DT[prec]).cuda(), wp, aux[:co], aux[co:2 * co], out, b, cip, co, G.cur_stream())
    torch.cuda.synchronize()
    G.check(G.from_nhwc(out), ref, G.TOL[prec], f"g1_fwd_affine {cfg}")


@pytest.mark.parametrize("prec", [1, 0], ids=PREC_NAME.get)
def test_img_to_u8(G, prec):
    """the stated formula in torch fp32, bit for bit: the ends, values on both sides of every x.5 step, out of range, NaN, inf"""
    k = torch.arange(0, 256, dtype=torch.float32)
    steps = (k + 0.5 - 127.5) / 127.5                      # x * 127.5 + 127.5 ~ k + 0.5
    special = torch.tensor([-1.0, 1.0, 0.0, -0.0, -1.5, 1.5, 3.0, -3.0, float("nan"), float("inf"), -float("inf"), 1e-8, 0.999999, -0.999999])
    vals = torch.cat([special, steps, torch.nextafter(steps, torch.tensor(9.0)), torch.nextafter(steps, torch.tensor(-9.0)),
                      torch.rand(3000, generator=_gen(3)) * 2.2 - 1.1])
    n, hw = 3, 20 * 20                                     # (HW is not a multiple of the 1024 pixels of a workgroup)
    x = vals[torch.randint(0, vals.numel(), (n, hw, 4), generator=_gen(6))]
    x.view(-1)[:vals.numel()] = vals
    xd = x.to(DT[prec]).cuda()
    xf = xd.float().cpu()[..., :3]
    exp = (torch.clamp(torch.nan_to_num(xf * 127.5 + 127.5, nan=0.0, posinf=255.0, neginf=0.0), 0.0, 255.0) + 0.5).to(torch.uint8)
    # torch's own fmax / fmin state the formula literally (fmax(NaN, 0) = 0)
    lit = (torch.fmin(torch.fmax(xf * 127.5 + 127.5, torch.tensor(0.0)), torch.tensor(255.0)) + 0.5).to(torch.uint8)
    assert torch.equal(exp, lit)
    out = torch.full((n * hw * 3 + TAIL,), 77, dtype=torch.uint8, device="cuda")
    G.lib.jck_img_to_u8(prec, xd, out, n, hw, G.cur_stream())
    torch.cuda.synchronize()
    assert bool((out[n * hw * 3:] == 77).all())
    assert torch.equal(out[:n * hw * 3].view(n, hw, 3).cpu(), lit)


# ---------------------------------------------------------------------------------------------------------------------
# engine
# ---------------------------------------------------------------------------------------------------------------------
_engines = {}


def _engine(family, prec, batch=8, size=64):
    """one engine per configuration for the module: oracle weights, running statistics fitted to them by 30 train-mode batches
    (0.9^30 = 0.04 of the initial (0, 1) is left; with the initial statistics a fresh generator's eval output is a flat grey)"""
    key = (family, prec, batch, size)
    if key not in _engines:
        from hipgan.engine import CganEngine, DcganEngine
        from oracle.gan_oracle import GanOracle
        orc = GanOracle(family, lr=2e-4, seed=12345, **({"image_size": size} if size != 64 else {}))
        eng = (CganEngine if family == "cgan" else DcganEngine)(batch=batch, prec=prec, **({"image_size": size} if size != 64 else {}))
        eng.load_state(orc.g, orc.d)
        for s in range(30):
            z, lab = _z(batch, 100 + s, family)
            eng.sample(z, lab)
        _engines[key] = eng
    return _engines[key]


def _z(n, seed, family):
    g = _gen(seed)
    z = torch.randn(n, 100, generator=g)
    lab = F.one_hot(torch.randint(0, 100, (n,), generator=g), 100).to(torch.int64) if family == "cgan" else None
    return z, lab


def _bn_state(eng):
    torch.cuda.synchronize()
    return eng.arenas["g_bn"].clone(), eng.arenas["g_nbt"].clone()


ENGINES = [pytest.param(f, p, id=f"{f}-{p}") for f in ("dcgan", "cgan") for p in ("bf16", "f32")]


@pytest.mark.parametrize("family,prec", ENGINES)
def test_eval_images_are_independent(family, prec):
    """row 3 depends on z[3] alone with bn="running"; with bn="batch" it depends on the whole batch - why the mode exists"""
    eng = _engine(family, prec)
    z0, lab = _z(8, 1, family)
    z1, _ = _z(8, 2, family)
    z1[3] = z0[3]
    a, b = eng.sample(z0, lab, bn="running"), eng.sample(z1, lab, bn="running")
    assert torch.equal(a[3], b[3]) and not torch.equal(a[2], b[2])
    a, b = eng.sample(z0, lab), eng.sample(z1, lab)
    assert not torch.equal(a[3], b[3])


@pytest.mark.parametrize("family,prec", ENGINES)
def test_eval_leaves_the_buffers(family, prec):
    eng = _engine(family, prec)
    z, lab = _z(8, 3, family)
    bn0, nbt0 = _bn_state(eng)
    eng.sample(z, lab, bn="running")
    eng.sample(z[:5], None if lab is None else lab[:5], bn="running", out="uint8")
    bn1, nbt1 = _bn_state(eng)
    assert torch.equal(bn0, bn1) and torch.equal(nbt0, nbt1)
    eng.sample(z, lab)
    bn2, nbt2 = _bn_state(eng)
    assert not torch.equal(bn1, bn2) and not torch.equal(nbt1, nbt2)


def _module_eval(eng, family, z, lab, size=64):
    from model import CGAN, DCGAN
    g = CGAN.Generator() if family == "cgan" else DCGAN.Generator(**({"image_size": size} if size != 64 else {}))
    g.load_state_dict(eng.state_dicts()[0])
    g = g.cuda().eval()
    g.prec = "f32"
    with torch.no_grad():
        zz = z.cuda().view(-1, 100, 1, 1)
        return g(zz, lab.cuda()) if family == "cgan" else g(zz)


def _parity(got, ref, prec, what):
    rtol = {"f32": 2e-4, "bf16": 1.2e-1}[prec]
    got, ref = got.double().cpu(), ref.double().cpu()
    tol = 1e-6 + rtol * torch.maximum(ref.abs(), ref.pow(2).mean().sqrt())
    err = (got - ref).abs()
    print(f"{what}: max |err| {float(err.max()):.3e}, max err / tol {float((err / tol).max()):.3f}")
    assert bool((err <= tol).all()), f"{what}: {int((err > tol).sum())} elements outside the bound, worst {float((err / tol).max()):.2f} x"


@pytest.mark.parametrize("family,prec", ENGINES)
def test_eval_matches_the_module_in_eval_mode(family, prec):
    eng = _engine(family, prec)
    z, lab = _z(8, 4, family)
    got = eng.sample(z, lab, bn="running")
    assert got.shape == (8, 3, 64, 64) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    _parity(got, _module_eval(eng, family, z, lab), prec, f"{family} {prec}")


@pytest.mark.parametrize("family,prec", ENGINES)
def test_eval_sizes_and_chunks(family, prec):
    """n = 1, n = 5 and n = 20 (three chunks of a batch-8 engine): rows equal those of single-chunk calls, float and uint8"""
    eng = _engine(family, prec)
    z, lab = _z(20, 5, family)
    sub = lambda lo, hi: (z[lo:hi], None if lab is None else lab[lo:hi])
    full = eng.sample(z, lab, bn="running")
    assert full.shape == (20, 3, 64, 64)
    for lo, hi in ((0, 8), (8, 16), (16, 20), (7, 8), (3, 8)):
        assert torch.equal(eng.sample(*sub(lo, hi), bn="running"), full[lo:hi]), (lo, hi)
    u8 = eng.sample(z, lab, bn="running", out="uint8")
    assert u8.shape == (20, 64, 64, 3) and u8.dtype == torch.uint8
    # the float image is fp32 of the stored (bf16 / fp32) tanh output, so the stated formula on it gives the same bytes
    x = full.permute(0, 2, 3, 1)
    assert torch.equal(u8, (torch.clamp(x * 127.5 + 127.5, 0.0, 255.0) + 0.5).to(torch.uint8))
    with pytest.raises(Exception):
        eng.sample(z, lab)                      # train-mode BatchNorm still refuses to split a batch


@pytest.mark.parametrize("family,prec", ENGINES)
def test_default_sample_is_unchanged(family, prec):
    """sample(z) with the defaults is jck_engine_sample, bit for bit, before and after an eval call, and flags = 0 of the extended
    entry point runs the same"""
    import gpu_util as G
    eng = _engine(family, prec)
    z, lab = _z(8, 6, family)
    bn0, nbt0 = _bn_state(eng)

    def restore():
        eng.arenas["g_bn"].copy_(bn0)
        eng.arenas["g_nbt"].copy_(nbt0)

    def raw(ex):
        out = torch.empty(8, 3, 64, 64, device="cuda")
        zc, lc = z.cuda().contiguous(), None if lab is None else lab.cuda().contiguous()
        if ex:
            G.lib.jck_engine_sample_ex(eng._h, zc, lc, 8, 0, out, None, G.cur_stream())
        else:
            G.lib.jck_engine_sample(eng._h, zc, lc, 8, out, G.cur_stream())
        torch.cuda.synchronize()
        return out
    ref = raw(False)
    bn_ref = _bn_state(eng)
    for step in ("before", "after"):
        restore()
        assert torch.equal(eng.sample(z, lab), ref), step
        assert all(torch.equal(a, b) for a, b in zip(_bn_state(eng), bn_ref)), step
        restore()
        assert torch.equal(raw(True), ref), step
        eng.sample(z, lab, bn="running")


@pytest.mark.parametrize("prec", ["bf16", "f32"])
def test_sampling_engine_of_the_average_takes_both_options(prec):
    """a sampling engine (ema=True) with bn="running" and out="uint8": right after load_state the average is the live generator and
    its BatchNorm buffers are copies of the live ones, so the two engines give the same images; the average's buffers do not move"""
    from hipgan.engine import DcganEngine
    from oracle.gan_oracle import GanOracle
    orc = GanOracle("dcgan", lr=2e-4, seed=12345)
    live = DcganEngine(batch=8, prec=prec, ema_decay=0.999)
    live.load_state(orc.g, orc.d)
    for s in range(30):
        live.sample(_z(8, 200 + s, "dcgan")[0])
    live.reset_ema()                                  # the average's buffers := the fitted live ones
    avg = DcganEngine(batch=8, prec=prec, share=live, ema=True)
    z, _ = _z(20, 8, "dcgan")
    torch.cuda.synchronize()
    bn0, nbt0 = live.arenas["g_ema_bn"].clone(), live.arenas["g_ema_nbt"].clone()
    a = avg.sample(z, bn="running")
    assert a.shape == (20, 3, 64, 64) and float(a.std()) > 0.01
    assert torch.equal(a, live.sample(z, bn="running"))
    u8 = avg.sample(z, bn="running", out="uint8")
    assert torch.equal(u8, live.sample(z, bn="running", out="uint8")) and u8.shape == (20, 64, 64, 3)
    torch.cuda.synchronize()
    assert torch.equal(bn0, live.arenas["g_ema_bn"]) and torch.equal(nbt0, live.arenas["g_ema_nbt"])
    avg.sample(z[:8])                                 # train mode moves the average's buffers, not the live ones
    torch.cuda.synchronize()
    assert not torch.equal(bn0, live.arenas["g_ema_bn"])


def test_eval_image_size_128():
    eng = _engine("dcgan", "bf16", batch=4, size=128)
    z, _ = _z(4, 7, "dcgan")
    bn0, nbt0 = _bn_state(eng)
    got = eng.sample(z, bn="running")
    assert got.shape == (4, 3, 128, 128)
    assert all(torch.equal(a, b) for a, b in zip(_bn_state(eng), (bn0, nbt0)))
    assert torch.equal(eng.sample(z[1:3], bn="running"), got[1:3])
    _parity(got, _module_eval(eng, "dcgan", z, None, 128), "bf16", "dcgan 128 bf16")
