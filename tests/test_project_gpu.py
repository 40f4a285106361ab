"""Latent projection: jck_conv_down_mask, jck_latent_loss, jck_latent_adam, the dz product, jck_engine_latent_grad / _project,
DcganEngine.latent_grad / .project and Sampler.project.

Per op, exact (the integer-data pattern of tests/test_exact_gpu.py and tests/test_sample_eval_gpu.py): gradients 0..15 and weights
in {-1, 0, 1} - every partial sum is an integer below 2^24, exact in fp32 in any order and exact as bf16 operands - and
scale[c] = 2^(c - Cs/2) (Cs > 128: the exponents -64 .. 63 repeat every 128 channels, so that no product leaves the normal range of
fp32), so scale * sum is exact and the stored value is its ONE rounding to the element type, which fp64 -> fp32
-> bf16 reproduces (the fp32 step is exact: the sums have at most 14 significant bits).  Masked elements must be +0 bit for bit.

Per op, real valued: fp64 references from the same (rounded) inputs, bounds gpu_util.TOL relative to the reference (3e-6 f32,
1.5e-2 bf16); the Adam update within 4 ulp of the rounded fp64 formula.

Engine: the reference is a functional fp64 generator on the CPU (F.conv_transpose2d, F.batch_norm(training=False), relu, tanh)
built from eng.state_dicts()[0], autograd for dz and torch.optim.Adam for the updates.  latent_grad is compared from identical
state (teacher forced, as tests/test_step_gpu.py compares steps); the free-running projection is NOT compared by trajectory - Adam
divides by |g| and elements with |g| ~ 1e-7 flip sign under rounding - but on a planted optimum: t = G(z*), z0 = z* + 0.3 eps,
the loss must fall monotonically and its end / start ratio must match the fp64 run's."""
import numpy as np
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


def _out(numel, prec, dtype=None):
    return torch.full((numel + TAIL,), 7.0, dtype=dtype or DT[prec], device="cuda")


def _tail_ok(buf, numel, what):
    assert bool((buf[numel:] == 7.0).all()), f"{what}: wrote past the output"


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ---------------------------------------------------------------------------------------------------------------------
# jck_conv_down_mask, exact
# ---------------------------------------------------------------------------------------------------------------------
# (N, Hb, Cb, Cs).  (1, 8, 64, 64): the 64-row tile at >= 64 gathered channels.  BIG / BIG1 - 256 / 257 images of 16 x 16 x 64 into 512
# channels - reach the tiles the dispatch takes only at >= 250 / 512 / 256 workgroups: 128x256 wave-specialised (bf16, M % 256 == 0),
# 128x128 LDS-DMA (bf16, 257 images: M % 256 != 0), 128x128 register-staged (f32, bf16x3); None: not run
BIG, BIG1 = (256, 16, 64, 512), (257, 16, 64, 512)
MASK_KERNEL = {(1, 8, 32, 64): ("", "igemm<f32,64,128>", "igemm<bf16x3,64,128>"),    # (bf16's register-staged 64 x 128 tile has no name)
               (3, 8, 64, 128): ("igemm_dma<128,64,3,ws>", "igemm<f32,128,64>", "igemm<bf16x3,128,64>"),
               (2, 16, 4, 64): ("igemm<bf16,64,128,img>", "igemm<f32,64,128,img>", "igemm<bf16x3,64,128,img>"),
               (1, 8, 64, 64): ("igemm_dma<64,128,2>", "igemm<f32,64,128>", "igemm<bf16x3,64,128>"),
               BIG: ("igemm_dma<128,256,3,ws,8>", "igemm<f32,128,128>", "igemm<bf16x3,128,128>"),
               BIG1: ("igemm_dma<128,128,2>", None, None)}
MASK_EXACT = [pytest.param(s, p, id="x".join(map(str, s)) + "-" + PREC_NAME[p]) for s in MASK_KERNEL for p in (0, 1, 2)
              if MASK_KERNEL[s][p] is not None]
_mask_cache = {}


def _mask_data(shape):
    if shape not in _mask_cache:
        n, hb, cb, cs = shape
        if shape == BIG:                        # the first 256 images of the 257-image case: one CPU reference for both
            g, w, a, scale, ref = _mask_data(BIG1)
            _mask_cache[shape] = (g[:256], w, a[:256], scale, ref[:256])
            return _mask_cache[shape]
        g = torch.randint(0, 16, (n, cb, hb, hb), generator=_gen(31)).float()
        u = torch.rand((cs, cb, 4, 4), generator=_gen(32))
        w = (u < 0.6).float() - (u > 0.8).float()
        assert 15 * 16 * cb < 2 ** 24
        y = F.conv2d(g, w, None, 2, 1).double()                     # the ConvTranspose's input gradient: integers, exact in any order
        assert float((y.float().to(torch.bfloat16).double() != y).double().mean()) > 0.2 or cb <= 4, "sums would survive a bf16 rounding"
        a = torch.randn(n, cs, hb // 2, hb // 2, generator=_gen(33))
        flat = a.view(-1)
        idx = torch.randperm(flat.numel(), generator=_gen(34))
        k = flat.numel() // 10
        flat[idx[:k]] = 0.0                                          # exact zeros: masked (torch.relu's convention at 0)
        flat[idx[k:2 * k]] = -0.0
        flat[idx[2 * k:3 * k]] = float("nan")                       # NaN activations mask as well
        # exponents -64 .. 63 at the most: |scale * sum| stays between 2^-64 and 2^77, a normal number in fp32 and bf16
        scale = torch.pow(2.0, (torch.arange(cs) % 128 - min(cs, 128) // 2).double())
        ref = torch.where(a.double() > 0, y * scale.view(1, -1, 1, 1), torch.zeros_like(y))
        assert float((a > 0).double().mean()) > 0.2 and float((a < 0).double().mean()) > 0.2
        _mask_cache[shape] = (g, w, a, scale.float(), ref)
    return _mask_cache[shape]


@pytest.mark.parametrize("shape,prec", MASK_EXACT)
def test_conv_down_mask_exact(G, shape, prec):
    n, hb, cb, cs = shape
    g, w, a, scale, ref = _mask_data(shape)
    nhwc = lambda x: x.permute(0, 2, 3, 1).contiguous().to(DT[prec]).cuda()
    wp = torch.empty(G.lib.jck_pad_rows(cs) * 16 * G.lib.jck_pad_chan(cb), dtype=DT[prec], device="cuda")
    G.lib.jck_pack_down(prec, w.cuda().contiguous(), cs, cb, wp, G.cur_stream())
    numel = n * (hb // 2) ** 2 * cs
    out = _out(numel, prec)
    G.lib.jck_conv_down_mask(prec, nhwc(g), wp, nhwc(a), scale.cuda(), out, n, hb, hb, cb, cs, G.cur_stream())
    torch.cuda.synchronize()
    what = f"conv_down_mask {shape} {PREC_NAME[prec]}"
    assert (G.lib.jck_last_launch() or b"").decode() == MASK_KERNEL[shape][prec], what
    _tail_ok(out, numel, what)
    exp = ref.permute(0, 2, 3, 1).contiguous().float().to(DT[prec]).cuda()          # fp64 -> fp32 exact, -> bf16 the one rounding
    got = out[:numel].view(exp.shape)
    if not torch.equal(_bits(got), _bits(exp)):
        bad = torch.nonzero(_bits(got) != _bits(exp))
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {bad.shape[0]} of {exp.numel()} elements differ, first at (n, y, x, c) = {i}: "
                             f"got {float(got[i]):.10g} exact {float(exp[i]):.10g}")
    masked = ~(a > 0).permute(0, 2, 3, 1).cuda()
    assert bool((_bits(got)[masked] == 0).all()), f"{what}: a masked element is not +0"


def test_conv_down_mask_refuses_bad_arguments(G):
    from hipgan import JckError
    x, wp = torch.zeros(1, 8, 8, 64, device="cuda"), torch.zeros(128 * 16 * 64, device="cuda")
    out = torch.zeros(1, 4, 4, 128, device="cuda")
    with pytest.raises(JckError):
        G.lib.jck_conv_down_mask(1, x, wp, None, torch.ones(128, device="cuda"), out, 1, 8, 8, 64, 128, G.cur_stream())
    with pytest.raises(JckError):
        G.lib.jck_conv_down_mask(1, x, wp, out, None, out, 1, 8, 8, 64, 128, G.cur_stream())


# ---------------------------------------------------------------------------------------------------------------------
# the dz product + jck_latent_adam in sum-only mode, exact
# ---------------------------------------------------------------------------------------------------------------------
_dz_cache = {}


def _dz_data():
    if not _dz_cache:
        c1 = 512
        g = torch.randint(0, 16, (8, c1, 4, 4), generator=_gen(41)).float()
        u = torch.rand((100, c1, 4, 4), generator=_gen(42))
        w = (u < 0.6).float() - (u > 0.8).float()
        assert 15 * 16 * c1 < 2 ** 24
        _dz_cache["d"] = (g, w, torch.einsum("bcp,kcp->bk", g.view(8, c1, 16).double(), w.view(100, c1, 16).double()))
    return _dz_cache["d"]


@pytest.mark.parametrize("prec", [0, 1, 2], ids=PREC_NAME.get)
@pytest.mark.parametrize("b", [1, 5, 8])
def test_dz_product_and_slab_sum_exact(G, b, prec):
    """dz[b, k] = sum_{pos, co} g[b, pos, co] * W1[k, co, pos]: jck_pack_linear's (co, pos) -> (pos, co) column permutation, the
    split-K plain GEMM with 16 slabs, and their sum in jck_latent_adam(t = 0)"""
    g, w, ref = _dz_data()
    c1, K, Z, ld = 512, 16 * 512, 16, 128
    wp = torch.empty(ld * K, dtype=DT[prec], device="cuda")
    G.lib.jck_pack_linear(prec, w.cuda().contiguous(), 100, K, ld, K, 0, c1, 16, wp, G.cur_stream())
    gd = g[:b].permute(0, 2, 3, 1).contiguous().to(DT[prec]).cuda()                  # [b, 4, 4, C1]: (pos, co) columns
    slab = _out(Z * b * ld, prec, torch.float32)
    G.lib.jck_linear_fwd(prec, gd, wp, None, slab, b, K, 100, ld, Z, G.cur_stream())
    dz = _out(b * 100, prec, torch.float32)
    G.lib.jck_latent_adam(prec, slab, Z, ld, dz, None, None, 0.0, 0.0, 0, None, 0, b, G.cur_stream())
    torch.cuda.synchronize()
    what = f"dz product B={b} {PREC_NAME[prec]}"
    _tail_ok(slab, Z * b * ld, what), _tail_ok(dz, b * 100, what)
    assert torch.equal(dz[:b * 100].view(b, 100).cpu().double(), ref[:b]), what


# ---------------------------------------------------------------------------------------------------------------------
# jck_latent_loss
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [1, 0], ids=PREC_NAME.get)
@pytest.mark.parametrize("n,hw", [(1, 64 * 64), (5, 64 * 64), (1, 8 * 8), (5, 8 * 8)])
def test_latent_loss(G, n, hw, prec):
    g = _gen(51)
    x5 = torch.tanh(torch.randn(5, hw, 4, generator=g)).to(DT[prec])                # (the padding channel holds values too: it is not read)
    t5 = (torch.rand(5, 3, hw, generator=g) * 2 - 1)
    x, t = x5[:n].contiguous(), t5[:n].contiguous()
    xd = x.double()[..., :3].permute(0, 2, 1)                                        # [n, 3, hw]
    d = xd - t.double()
    ref_loss = d.pow(2).mean(dim=(1, 2))
    ref_g = (2.0 * d / (3 * hw) * (1.0 - xd * xd)).permute(0, 2, 1)                  # [n, hw, 3]

    def run(xx, tt, k):
        graw, loss = _out(k * hw * 4, prec), _out(k, prec, torch.float32)
        G.lib.jck_latent_loss(prec, xx.cuda(), tt.cuda(), graw, loss, k, hw, G.cur_stream())
        torch.cuda.synchronize()
        _tail_ok(graw, k * hw * 4, "latent_loss g_raw"), _tail_ok(loss, k, "latent_loss loss")
        return graw[:k * hw * 4].view(k, hw, 4).clone(), loss[:k].clone()
    (g0, l0), (g1, l1) = run(x, t, n), run(x, t, n)
    assert torch.equal(_bits(g0), _bits(g1)) and torch.equal(_bits(l0), _bits(l1)), "two runs differ"
    rel = ((l0.cpu().double() - ref_loss).abs() / ref_loss).max().item()
    print(f"latent_loss n={n} hw={hw} {PREC_NAME[prec]}: loss rel err {rel:.3e}")
    assert rel <= G.TOL[prec]
    G.check(g0[..., :3].cpu(), ref_g, G.TOL[prec], "latent_loss gradient")
    assert bool((_bits(g0[..., 3]) == 0).all()), "padding channel is not +0"
    g5, l5 = run(x5, t5, 5)                                                          # image b's numbers do not depend on N
    assert torch.equal(_bits(l5[:n]), _bits(l0)) and torch.equal(_bits(g5[:n]), _bits(g0))


# ---------------------------------------------------------------------------------------------------------------------
# jck_latent_adam
# ---------------------------------------------------------------------------------------------------------------------
def _ulps(got, ref64):
    """|got - fp32(ref64)| in units of the spacing of fp32 numbers at fp32(ref64)"""
    r = ref64.float()
    ulp = (torch.nextafter(r.abs(), torch.tensor(float("inf"))) - r.abs()).double()
    return ((got.double() - r.double()).abs() / ulp).max().item()


@pytest.mark.parametrize("prec", [1, 0], ids=PREC_NAME.get)
@pytest.mark.parametrize("prior", [0.0, 0.1])
@pytest.mark.parametrize("t", [1, 7])
def test_latent_adam(G, t, prior, prec):
    n, Z, ld, zp = 5, 3, 128, 256 if prior else 128
    g = _gen(61 + t)
    slab = torch.randn(Z, n, ld, generator=g) * 1e-3
    z, m, v = torch.randn(n, 100, generator=g), torch.randn(n, 100, generator=g) * 1e-3, torch.rand(n, 100, generator=g) * 1e-6
    lr = 0.05
    gsum = slab[0, :, :100].clone()
    for q in range(1, Z):
        gsum = gsum + slab[q, :, :100]                              # fp32, in slab order: IEEE adds, the kernel's bits
    lr32, prior32 = float(np.float32(lr)), float(np.float32(prior))
    gd = gsum.double() + (2.0 * prior32 / 100) * z.double()
    m64 = 0.9 * m.double() + (1.0 - 0.9) * gd
    v64 = 0.999 * v.double() + (1.0 - 0.999) * gd * gd
    step = lr32 / (1.0 - 0.9 ** t)
    z64 = z.double() - step * m64 / (v64.sqrt() / (1.0 - 0.999 ** t) ** 0.5 + 1e-8)
    zd, md, vd = z.cuda(), m.cuda(), v.cuda()
    op = _out(n * zp, prec)
    G.lib.jck_latent_adam(prec, slab.cuda(), Z, ld, zd, md, vd, lr, prior, t, op, zp, n, G.cur_stream())
    torch.cuda.synchronize()
    what = f"latent_adam t={t} prior={prior} {PREC_NAME[prec]}"
    _tail_ok(op, n * zp, what)
    uz, um, uv = _ulps(zd.cpu(), z64), _ulps(md.cpu(), m64), _ulps(vd.cpu(), v64)
    print(f"{what}: ulps z {uz:.2f} m {um:.2f} v {uv:.2f}")
    assert uz <= 4 and um <= 4 and uv <= 4, what
    rows = op[:n * zp].view(n, zp)
    assert torch.equal(_bits(rows[:, :100]), _bits(zd.to(DT[prec]))), what + ": operand rows"
    assert bool((rows[:, 100:] == 7.0).all()), what + ": columns >= 100 were written"
    # sum only: nothing but z is touched
    dz, m2, v2 = _out(n * 100, prec, torch.float32), md.clone(), vd.clone()
    G.lib.jck_latent_adam(prec, slab.cuda(), Z, ld, dz, m2, v2, lr, prior, 0, op, zp, n, G.cur_stream())
    torch.cuda.synchronize()
    assert torch.equal(dz[:n * 100].view(n, 100).cpu(), gsum) and torch.equal(m2, md) and torch.equal(v2, vd)
    assert torch.equal(_bits(op[:n * zp].view(n, zp)), _bits(rows))


# ---------------------------------------------------------------------------------------------------------------------
# engine
# ---------------------------------------------------------------------------------------------------------------------
_engines = {}


def _z(n, seed, family):
    g = _gen(seed)
    z = torch.randn(n, 100, generator=g)
    lab = F.one_hot(torch.randint(0, 100, (n,), generator=g), 100).to(torch.int64) if family == "cgan" else None
    return z, lab


def _engine(family, prec, batch=8, size=64):
    """as tests/test_sample_eval_gpu.py::_engine: oracle weights, running statistics fitted by 30 train-mode batches"""
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
        torch.cuda.synchronize()
        _engines[key] = eng
    return _engines[key]


def _ref_generator(eng):
    """fp64 functional generator under model.eval() from the engine's own state: (z [n,100], labels or None) -> [n,3,S,S]"""
    sd = {k: v.detach().cpu().double() for k, v in eng.state_dicts()[0].items()}
    nconv = sum(1 for k in sd if k.startswith("conv") and k.endswith(".weight"))

    def gen(z, lab=None):
        x = z.view(-1, 100, 1, 1)
        if lab is not None:
            x = torch.cat([x, lab.double().view(-1, 100, 1, 1)], 1)
        x = F.conv_transpose2d(x, sd["conv1.weight"], None, 1, 0)
        for i in range(1, nconv):
            x = F.batch_norm(x, sd[f"norm{i}.running_mean"], sd[f"norm{i}.running_var"], sd[f"norm{i}.weight"], sd[f"norm{i}.bias"],
                             False, 0.1, 1e-5)
            x = F.conv_transpose2d(torch.relu(x), sd[f"conv{i + 1}.weight"], None, 2, 1)
        return torch.tanh(x)
    return gen


def _ref_loss(gen, z, lab, t):
    return (gen(z, lab) - t.double()).pow(2).mean(dim=(1, 2, 3))


_case_cache = {}


def _grad_case(family, prec, n, size=64, batch=8):
    """(engine, z, labels, target, fp64 loss [n], fp64 dz [n,100]); one reference per engine: the running statistics each engine
    fitted in its own precision are part of the function"""
    eng = _engine(family, prec, batch, size)
    key = (family, prec, n, size)
    if key not in _case_cache:
        gen = _ref_generator(eng)
        z, lab = _z(n, 7, family)
        with torch.no_grad():
            t = gen(_z(n, 8, family)[0].double(), lab).float()      # pictures the generator can make, of other latents
        zz = z.double().requires_grad_(True)
        loss = _ref_loss(gen, zz, lab, t)
        dz, = torch.autograd.grad(loss.sum(), zz)
        _case_cache[key] = (z, lab, t, loss.detach(), dz)
    return (eng,) + _case_cache[key]


ENGINES = [pytest.param(f, p, id=f"{f}-{p}") for f in ("dcgan", "cgan") for p in ("bf16", "f32")]
LOSS_TOL = {"f32": 1e-3, "bf16": 3e-2}                 # the project's step-scalar bounds
DZ_TOL = {"f32": 5e-3, "bf16": 0.11}                  # the project's f32 gradient bound; the tighter of its two bf16 gradient bounds


def _check_grad(eng, z, lab, t, ref_loss, ref_dz, prec, what):
    loss, dz = eng.latent_grad(z, t, lab)
    assert loss.shape == ref_loss.shape and dz.shape == ref_dz.shape and bool(torch.isfinite(dz).all())
    el = ((loss.cpu().double() - ref_loss).abs() / ref_loss).max().item()
    ed = ((dz.cpu().double() - ref_dz).norm(dim=1) / ref_dz.norm(dim=1)).max().item()
    print(f"{what}: loss rel err {el:.3e} (bound {LOSS_TOL[prec]}), dz rel L2 per image, worst {ed:.3e} (bound {DZ_TOL[prec]})")
    assert el < LOSS_TOL[prec] and ed < DZ_TOL[prec], what


@pytest.mark.parametrize("family,prec", ENGINES)
def test_latent_grad_matches_fp64_autograd(family, prec):
    """n = 5 (ragged on a batch-8 engine) and n = 1.  Bounds: loss relative error 1e-3 (f32) / 3e-2 (bf16); dz relative L2 per image
    5e-3 (f32) / 0.11 (bf16).  Measured on an MI355X (worst image, n = 5): dcgan f32 loss 1.4e-7 dz 6.3e-7, dcgan bf16 loss
    5.2e-4 dz 3.8e-2, cgan f32 loss 1.2e-7 dz 6.9e-7, cgan bf16 loss 8.7e-4 dz 3.9e-2 (n = 1: the same or below)."""
    eng, z, lab, t, rl, rd = _grad_case(family, prec, 5)
    _check_grad(eng, z, lab, t, rl, rd, prec, f"latent_grad {family} {prec} n=5")
    one = lambda x: None if x is None else x[2:3]
    _check_grad(eng, z[2:3], one(lab), t[2:3], rl[2:3], rd[2:3], prec, f"latent_grad {family} {prec} n=1")


def test_latent_grad_128():
    """the 128 x 128 plan (five stride-2 stages, 1024 channels at the 4 x 4 end, 256 k-steps in the dz product), n = 2, f32.
    Measured on an MI355X: loss rel err 4.4e-8, dz rel L2 6.8e-7 (worst image)."""
    eng, z, lab, t, rl, rd = _grad_case("dcgan", "f32", 2, size=128, batch=4)
    _check_grad(eng, z, lab, t, rl, rd, "f32", "latent_grad dcgan f32 128x128 n=2")


_planted = {}


def _planted_case(family, prec, eng):
    """t = G(z*), z0 = z* + 0.3 eps, and the fp64 run: 12 updates of torch.optim.Adam(lr = 0.05) -> loss history [12, 4]"""
    if (family, prec) not in _planted:
        gen = _ref_generator(eng)
        zs, lab = _z(4, 21, family)
        with torch.no_grad():
            t = gen(zs.double(), lab).float()
        z0 = zs + 0.3 * torch.randn(4, 100, generator=_gen(22))
        zz = z0.double().clone().requires_grad_(True)
        opt = torch.optim.Adam([zz], lr=0.05, betas=(0.9, 0.999), eps=1e-8)
        hist = []
        for _ in range(12):
            opt.zero_grad()
            loss = _ref_loss(gen, zz, lab, t)
            hist.append(loss.detach().clone())
            loss.sum().backward()
            opt.step()
        _planted[(family, prec)] = (z0, lab, t, torch.stack(hist))
    return _planted[(family, prec)]


@pytest.mark.parametrize("family,prec", ENGINES)
def test_project_descends_to_a_planted_optimum(family, prec):
    """loss_hist non-increasing; end / start ratio per image within 1e-3 (f32) / 6e-2 (bf16) relative of the fp64 run's.
    Measured on an MI355X (worst image): dcgan f32 6.6e-7, dcgan bf16 1.8e-2, cgan f32 4.3e-7, cgan bf16 1.4e-2; the ratios
    themselves are 0.066 - 0.091, and every history fell monotonically."""
    eng = _engine(family, prec)
    z0, lab, t, ref = _planted_case(family, prec, eng)
    z, hist = eng.project(t, lab, steps=12, lr=0.05, z0=z0)
    hist = hist.cpu().double()
    assert z.shape == (4, 100) and hist.shape == (12, 4) and bool(torch.isfinite(hist).all())
    ratio, rref = hist[-1] / hist[0], ref[-1] / ref[0]
    dev = ((ratio - rref).abs() / rref).max().item()
    print(f"project {family} {prec}: loss end / start {ratio.tolist()} (fp64 {rref.tolist()}), worst relative deviation {dev:.3e}")
    assert bool((hist[1:] <= hist[:-1]).all()), f"loss history is not non-increasing: {hist.tolist()}"
    assert dev < {"f32": 1e-3, "bf16": 6e-2}[prec]


@pytest.mark.parametrize("family,prec", ENGINES)
def test_rows_are_independent_and_chunked(family, prec):
    """n = 20 on a batch-8 engine (chunks of 8, 8, 4) equals three separate calls, and a row alone, bit for bit"""
    eng = _engine(family, prec)
    z0, lab = _z(20, 31, family)
    t = (torch.rand(20, 3, 64, 64, generator=_gen(32)) * 2 - 1)
    sub = lambda x, lo, hi: None if x is None else x[lo:hi]
    z, hist = eng.project(t, lab, steps=3, lr=0.05, z0=z0)
    assert z.shape == (20, 100) and hist.shape == (3, 20)
    for lo, hi in ((0, 8), (8, 16), (16, 20), (5, 6)):
        zs, hs = eng.project(t[lo:hi], sub(lab, lo, hi), steps=3, lr=0.05, z0=z0[lo:hi])
        assert torch.equal(zs, z[lo:hi]) and torch.equal(hs, hist[:, lo:hi]), (lo, hi)
    loss, dz = eng.latent_grad(z0, t, lab)
    l1, d1 = eng.latent_grad(z0[9:10], t[9:10], sub(lab, 9, 10))
    assert torch.equal(loss[9:10], l1) and torch.equal(dz[9:10], d1) and torch.equal(loss, hist[0])


@pytest.mark.parametrize("family,prec", ENGINES)
def test_project_writes_no_parameter_or_buffer(family, prec):
    eng = _engine(family, prec)
    torch.cuda.synchronize()
    before = {k: v.clone() for k, v in eng.arenas.items()}
    z0, lab = _z(5, 41, family)
    t = (torch.rand(5, 3, 64, 64, generator=_gen(42)) * 2 - 1)
    eng.project(t, lab, steps=3, z0=z0)
    eng.latent_grad(z0, t, lab)
    torch.cuda.synchronize()
    for k, v in before.items():                         # g_bn, g_nbt, every parameter, gradient and Adam arena of both networks
        assert torch.equal(v, eng.arenas[k]), k


@pytest.mark.parametrize("family,prec", [pytest.param("dcgan", "bf16", id="dcgan-bf16"), pytest.param("cgan", "f32", id="cgan-f32")])
def test_project_continues(family, prec):
    """6 + 6 updates with the returned Adam state equal 12, bit for bit; the prior changes the result"""
    eng = _engine(family, prec)
    z0, lab = _z(5, 51, family)
    t = (torch.rand(5, 3, 64, 64, generator=_gen(52)) * 2 - 1)
    z12, h12 = eng.project(t, lab, steps=12, lr=0.05, prior=0.01, z0=z0)
    assert eng.project_state["t"] == 12
    za, ha = eng.project(t, lab, steps=6, lr=0.05, prior=0.01, z0=z0)
    st = eng.project_state
    zb, hb = eng.project(t, lab, steps=6, lr=0.05, prior=0.01, z0=za, state=st)
    assert torch.equal(zb, z12) and torch.equal(torch.cat([ha, hb]), h12)
    assert not torch.equal(eng.project(t, lab, steps=12, lr=0.05, prior=0.0, z0=z0)[0], z12)


def test_project_between_two_training_steps_changes_no_bit():
    """A training engine (DCGAN, B = 8, bf16, the next batch announced so that its D(real) forward is in flight) with a projection
    and a latent_grad between every two steps: scalars and every arena equal those of the run without them, bit for bit."""
    from hipgan.engine import DcganEngine
    from oracle.gan_oracle import build_params
    from util import synth_images
    B, steps = 8, 3
    imgs = synth_images(B * steps).cuda()
    t = (torch.rand(5, 3, 64, 64, generator=_gen(62)) * 2 - 1)
    z0 = _z(5, 61, "dcgan")[0]
    res = []
    for with_project in (False, True):
        torch.manual_seed(12345)
        g, d = build_params("dcgan")
        eng = DcganEngine(batch=B, prec="bf16", device="cuda:0")
        eng.graphs = False
        eng.load_state(g, d)
        eng.set_noise_seed(77)
        gen = torch.Generator(device="cuda").manual_seed(5)
        scal = []
        for s in range(steps):
            kw = dict(next_real=imgs[(s + 1) * B:(s + 2) * B]) if s + 1 < steps else {}
            eng.step_async(imgs[s * B:(s + 1) * B], None, 2e-4, generator=gen, **kw)
            if s + 1 < steps:
                assert eng._prefetched_real is not None
            if with_project:
                _, hist = eng.project(t, steps=3, z0=z0)
                eng.latent_grad(z0, t)
                assert bool(torch.isfinite(hist).all())
                if s + 1 < steps:
                    assert eng._prefetched_real is not None          # the projection did not drop the prefetched pass
            scal.append(eng.scalars())
        torch.cuda.synchronize()
        res.append((scal, {k: v.clone() for k, v in eng.arenas.items()}))
    assert res[0][0] == res[1][0], (res[0][0], res[1][0])
    for k, v in res[0][1].items():
        assert torch.equal(v, res[1][1][k]), k


@pytest.mark.parametrize("family", ["dcgan", "cgan"])
def test_sampler_project_round_trip(family):
    """images the sampler drew itself, as uint8: 30 updates end below the loss at z0 for every image; restarts keep the best start"""
    from hipgan.sampler import Sampler, images_to_target, latents
    s = Sampler(_engine(family, "bf16"), "live")
    cls = [3, 17, 42, 3, 99, 0] if family == "cgan" else None
    u8 = s.images(6, seed=1, labels=cls)
    assert u8.shape == (6, 64, 64, 3) and u8.dtype == torch.uint8
    z, loss = s.project(u8, cls, steps=30, lr=0.05, seed=9)
    lab = s._labels(cls, 6)
    start, _ = s.engine.latent_grad(latents(6, 9), images_to_target(u8.cpu()), lab)
    print(f"Sampler.project {family}: loss at z0 {start.tolist()} -> {loss.tolist()}")
    assert z.shape == (6, 100) and loss.shape == (6,) and bool((loss < start).all())
    z2, loss2 = s.project(u8, cls, steps=30, lr=0.05, seed=9, restarts=2)
    assert z2.shape == (6, 100) and bool((loss2 <= loss).all())         # seed 9 is one of the two starts, and rows are independent
    with pytest.raises(Exception):
        s.project(u8[:, :32], cls)


def test_argument_errors_launch_nothing(G):
    from hipgan import JckError
    eng, ceng = _engine("dcgan", "f32"), _engine("cgan", "f32")
    f = lambda *s: torch.full(s, 7.0, device="cuda")
    z, m, v, hist, t = f(9, 100), f(9, 100), f(9, 100), f(2, 9), f(9, 3, 64, 64)
    loss, dz = f(9), f(9, 100)
    st = G.cur_stream()
    with pytest.raises(JckError, match="n must be in"):
        G.lib.jck_engine_project(eng._h, z, None, t, 9, 2, 0.05, 0.0, m, v, 0, hist, st)              # n > batch
    with pytest.raises(JckError, match="n must be in"):
        G.lib.jck_engine_latent_grad(eng._h, z, None, t, 9, loss, dz, st)
    with pytest.raises(JckError, match="steps"):
        G.lib.jck_engine_project(eng._h, z, None, t, 8, 0, 0.05, 0.0, m, v, 0, hist, st)
    with pytest.raises(JckError, match="labels"):
        G.lib.jck_engine_project(ceng._h, z, None, t, 8, 2, 0.05, 0.0, m, v, 0, hist, st)
    with pytest.raises(JckError, match="labels"):
        G.lib.jck_engine_latent_grad(ceng._h, z, None, t, 8, loss, dz, st)
    torch.cuda.synchronize()
    for x in (z, m, v, hist, loss, dz):
        assert bool((x == 7.0).all()), "a refused call wrote an output"
    tt = torch.zeros(4, 3, 64, 64)
    with pytest.raises(JckError, match="labels"):
        ceng.project(tt)
    with pytest.raises(JckError, match="labels"):
        ceng.latent_grad(torch.zeros(4, 100), tt)
    with pytest.raises(JckError, match="target must be"):
        eng.project(torch.zeros(4, 3, 32, 32))
    with pytest.raises(JckError, match="target must be"):
        eng.latent_grad(torch.zeros(4, 100), torch.zeros(3, 3, 64, 64))
    with pytest.raises(JckError, match="steps"):
        eng.project(tt, steps=0)
    with pytest.raises(JckError, match="z0"):
        eng.project(tt, z0=torch.zeros(3, 100))


def test_generate_cli_projects_its_own_images(tmp_path):
    """generate.py in this process: images.npz from one run is the --project input of the next; projected.npz holds z, the loss of
    each reconstruction and the reconstructions, projected.png the sheet"""
    import generate
    eng = _engine("dcgan", "bf16")
    g, d = eng.state_dicts()
    ckpt = str(tmp_path / "g.pt")
    torch.save({"model_g": {k: v.detach().cpu().clone() for k, v in g.items()}, "model_d": {}}, ckpt)
    base = ["-m", "DCGAN", "--checkpoint", ckpt, "-b", "8"]
    assert generate.main(base + ["--num", "5", "--seed", "3", "--out", str(tmp_path / "s")]) == 0
    src = np.load(str(tmp_path / "s" / "images.npz"))["images"]
    assert generate.main(base + ["--project", str(tmp_path / "s" / "images.npz"), "--project_steps", "30", "--seed", "4",
                                 "--out", str(tmp_path / "p")]) == 0
    f = np.load(str(tmp_path / "p" / "projected.npz"))
    assert sorted(f.files) == ["images", "loss", "z"]
    assert f["z"].shape == (5, 100) and f["z"].dtype == np.float32 and f["loss"].shape == (5,) and f["images"].shape == src.shape
    assert f["images"].dtype == np.uint8 and bool(np.isfinite(f["loss"]).all())
    # the stored loss is the mean squared error of the stored reconstruction, up to its rounding to bytes (half a step of 1 / 127.5)
    mse = ((f["images"].astype(np.float64) - src.astype(np.float64)) / 127.5) ** 2
    assert np.all(np.abs(np.sqrt(mse.mean(axis=(1, 2, 3))) - np.sqrt(f["loss"])) < 1.0 / 127.5)
    from hipgan.sampler import Sampler, latents
    start, _ = Sampler(eng, "live").engine.latent_grad(latents(5, 4), torch.from_numpy(src).float().div(127.5).sub(1.0).permute(0, 3, 1, 2))
    assert np.all(f["loss"] < start.cpu().numpy())                         # 30 updates from the seed-4 start went down for every image
    png = open(str(tmp_path / "p" / "projected.png"), "rb").read()
    assert png[:8] == b"\x89PNG\r\n\x1a\n" and len(png) > 1000
