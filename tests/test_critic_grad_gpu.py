"""The critic's latent gradient: jck_conv_up_mask, jck_leaky_affine_bwd, jck_critic_ds, jck_latent_loss_ex, jck_engine_latent_grad_ex /
_project_ex, DcganEngine.critic_grad / .latent_grad / .project with weight and critic / .refine, Sampler.inpaint / .refine and the CLI.

Per op, exact (the integer-data pattern of tests/test_project_gpu.py): gradients 0..15 and weights in {-1, 0, 1} - every partial sum
is an integer below 2^24 -, scale[c] = 2^(c mod 16 - 8) and slope 0.25, so scale * sum * slope is exact and the stored value is its ONE
rounding to the element type, which fp64 -> fp32 -> bf16 reproduces.

Engine: the reference is a functional fp64 generator AND discriminator on the CPU built from eng.state_dicts() (F.conv2d,
F.batch_norm(training=False), leaky_relu(0.2), the head), autograd for dz and torch.optim.Adam for the updates.  Bounds: loss
relative LOSS_TOL (1e-3 f32, 3e-2 bf16); logit and term the _parity bound of tests/test_sample_eval_gpu.py (term is a 1-Lipschitz
function of the logit times its weight); dz relative L2 per image 5e-3 in f32, where only fp32 sums are reordered.  In bf16 the
chain is twice as deep as the projection's and had no bound.  Measured on an MI355X over the cases of this file (worst image,
test_latent_grad_ex_matches_fp64_autograd): 0.134.  Twice that is 0.268, above the 0.25 beyond which the direction no longer
reliably descends and a value counts as a defect, not as a tolerance: DZ_TOL["bf16"] is the smaller of the two, 0.25."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_project_gpu import _ref_generator
from test_sample_eval_gpu import _parity
from test_score_gpu import _arenas, _ckpt, _engine, _z

pytestmark = pytest.mark.gpu
PREC_NAME = {0: "bf16", 1: "f32", 2: "bf16x3"}
DT = {0: torch.bfloat16, 1: torch.float32, 2: torch.float32}
TAIL = 1024
SLOPE = 0.25
ENGINES = [pytest.param(f, p, id=f"{f}-{p}") for f in ("dcgan", "cgan") for p in ("bf16", "f32")]
LOSS_TOL = {"f32": 1e-3, "bf16": 3e-2}                 # the project's step-scalar bounds
DZ_TOL = {"f32": 5e-3, "bf16": min(2 * 0.134, 0.25)}  # f32: the project's gradient bound; bf16: 2 x the worst measured value, at most 0.25 (docstring)
CW = 0.003


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


def _nhwc(x, prec):
    return x.permute(0, 2, 3, 1).contiguous().to(DT[prec]).cuda()


# ---------------------------------------------------------------------------------------------------------------------
# jck_conv_up_mask, exact.  Tile branches of launch_igemm_fused_p<P, Epi::LeakyMask> (rows = Cb, M = N * Hs^2 pixel rows, 4 phases):
#   Cb = 64                                              -> 64 x 128      (1, 4, 128, 64): 16 rows, far below one tile
#   Cb % 128 == 0, few workgroups                        -> 128 x 64      (3, 4, 128, 128): M = 48, ragged
#   ceil(M / 128) * Cb / 128 * 4 >= 256 (f32) / 512 (bf16) -> 128 x 128   (31, 8, 128, 1024): M = 1984 = 15.5 tiles, 512 workgroups
#   bf16, ceil(M / 256) * Cb / 128 * 4 >= 250, M % 256 == 0 -> 128 x 256  (32, 8, 128, 1024): 256 workgroups
# ---------------------------------------------------------------------------------------------------------------------
T64 = ("igemm_dma<64,128,2>", "igemm<f32,64,128>", "igemm<bf16x3,64,128>")
T12864 = ("igemm_dma<128,64,3,ws>", "igemm<f32,128,64>", "igemm<bf16x3,128,64>")
T128 = ("igemm_dma<128,128,2>", "igemm<f32,128,128>", "igemm<bf16x3,128,128>")
UP_KERNEL = {(1, 4, 128, 64): T64, (3, 4, 128, 128): T12864, (31, 8, 128, 1024): T128,       # (N, Hs, Cs, Cb)
             (32, 8, 128, 1024): ("igemm_dma<128,256,3,ws,8>", None, None)}
UP_CASES = [pytest.param(s, p, id="x".join(map(str, s)) + "-" + PREC_NAME[p]) for s in UP_KERNEL for p in (0, 1, 2) if UP_KERNEL[s][p]]
_up_cache = {}


def _up_data(shape):
    if shape not in _up_cache:
        _up_cache.clear()                                                    # one shape's tensors at a time: the large ones are 30 MB each
        n, hs, cs, cb = shape
        g = torch.randint(0, 16, (n, cs, hs, hs), generator=_gen(31)).float()
        u = torch.rand((cs, cb, 4, 4), generator=_gen(32))
        w = (u < 0.6).float() - (u > 0.8).float()
        assert 15 * 4 * cs < 2 ** 24
        y = F.conv_transpose2d(g, w, None, 2, 1).double()                   # the Conv2d's input gradient: integers, exact in any order
        a = torch.randn(n, cb, 2 * hs, 2 * hs, generator=_gen(33))
        flat = a.view(-1)
        idx = torch.randperm(flat.numel(), generator=_gen(34))
        k = flat.numel() // 10
        flat[idx[:k]] = 0.0
        flat[idx[k:2 * k]] = -0.0
        flat[idx[2 * k:3 * k]] = float("nan")
        scale = torch.pow(2.0, (torch.arange(cb) % 16 - 8).double())
        t = y * scale.view(1, -1, 1, 1)
        ref = torch.where(a.double() > 0, t, t * SLOPE)
        _up_cache[shape] = (g, w, a, scale.float(), ref, t * SLOPE)
    return _up_cache[shape]


@pytest.mark.parametrize("shape,prec", UP_CASES)
def test_conv_up_mask_exact(G, shape, prec):
    n, hs, cs, cb = shape
    g, w, a, scale, ref, slope_branch = _up_data(shape)
    wp = torch.empty(4 * G.lib.jck_pad_rows(cb) * 4 * cs, dtype=DT[prec], device="cuda")
    G.lib.jck_pack_up(prec, w.cuda().contiguous(), cs, cb, wp, G.cur_stream())
    numel = n * 4 * hs * hs * cb
    out = _out(numel, prec)
    G.lib.jck_conv_up_mask(prec, _nhwc(g, prec), wp, _nhwc(a, prec), scale.cuda(), SLOPE, out, n, hs, hs, cs, cb, G.cur_stream())
    torch.cuda.synchronize()
    what = f"conv_up_mask {shape} {PREC_NAME[prec]}"
    assert (G.lib.jck_last_launch() or b"").decode() == UP_KERNEL[shape][prec], what
    _tail_ok(out, numel, what)
    exp = _nhwc(ref.float(), prec)                                           # fp64 -> fp32 exact, -> bf16 the one rounding
    got = out[:numel].view(exp.shape)
    if not torch.equal(_bits(got), _bits(exp)):
        bad = torch.nonzero(_bits(got) != _bits(exp))
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {bad.shape[0]} of {exp.numel()} elements differ, first at (n, y, x, c) = {i}: "
                             f"got {float(got[i]):.10g} exact {float(exp[i]):.10g}")
    slope_bits = _bits(_nhwc(slope_branch.float(), prec))                    # +0, -0 and NaN activations: the slope branch, each
    for name, pick in (("+0", (a == 0) & ~torch.signbit(a)), ("-0", (a == 0) & torch.signbit(a)), ("NaN", torch.isnan(a))):
        pick = pick.permute(0, 2, 3, 1).cuda()
        assert int(pick.sum()) >= a.numel() // 10, (what, name)
        assert torch.equal(_bits(got)[pick], slope_bits[pick]), f"{what}: an activation of {name} did not take the slope branch"


def test_conv_up_mask_refuses_bad_arguments(G):
    from hipgan import JckError
    f = lambda *s: torch.full(s, 7.0, device="cuda")
    g, wp, a, out, sc = f(1, 4, 4, 128), f(4 * 128 * 4 * 128), f(1, 8, 8, 128), f(1, 8, 8, 128), torch.ones(132, device="cuda")
    st = G.cur_stream()
    bad = [lambda: G.lib.jck_conv_up_mask(1, g, wp, None, sc, SLOPE, out, 1, 4, 4, 128, 128, st),              # no activation
           lambda: G.lib.jck_conv_up_mask(1, g, wp, a, None, SLOPE, out, 1, 4, 4, 128, 128, st),               # no scale
           lambda: G.lib.jck_conv_up_mask(1, g, wp, a, sc[1:], SLOPE, out, 1, 4, 4, 128, 128, st),             # scale not 16-byte aligned
           lambda: G.lib.jck_conv_up_mask(1, g, wp, a.view(-1)[1:], sc, SLOPE, out, 1, 4, 4, 128, 128, st),    # activation not aligned
           lambda: G.lib.jck_conv_up_mask(1, g, wp, a, sc, SLOPE, out, 1, 4, 4, 128, 32, st),                  # Cb < 64
           lambda: G.lib.jck_conv_up_mask(1, g, wp, a, sc, SLOPE, out, 1, 4, 4, 128, 96, st),                  # Cb no power of two
           lambda: G.lib.jck_conv_up_mask(1, g, wp, a, sc, SLOPE, out, 1, 4, 4, 32, 128, st),                  # Cs < 64
           lambda: G.lib.jck_conv_up_mask(1, g, wp, a, sc, SLOPE, out, 0, 4, 4, 128, 128, st)]                 # N < 1
    for call in bad:
        with pytest.raises(JckError):
            call()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused call wrote the output"


def test_relu_mask_is_untouched(G):
    """jck_conv_down_mask on one fixed case, bf16 and f32: the bits of the fp64 formula (a > 0 ? scale * sum : +0), as before the
    leaky form joined the epilogue"""
    n, hb, cb, cs = 2, 8, 64, 128
    g = torch.randint(0, 16, (n, cb, hb, hb), generator=_gen(71)).float()
    u = torch.rand((cs, cb, 4, 4), generator=_gen(72))
    w = (u < 0.6).float() - (u > 0.8).float()
    y = F.conv2d(g, w, None, 2, 1).double()
    a = torch.randn(n, cs, hb // 2, hb // 2, generator=_gen(73))
    a.view(-1)[::7] = 0.0
    a.view(-1)[3::11] = float("nan")
    scale = torch.pow(2.0, (torch.arange(cs) % 16 - 8).double())
    ref = torch.where(a.double() > 0, y * scale.view(1, -1, 1, 1), torch.zeros_like(y))
    for prec in (0, 1):
        numel = n * (hb // 2) ** 2 * cs
        out = _out(numel, prec)
        G.lib.jck_conv_down_mask(prec, _nhwc(g, prec), G.pack_down(w, prec), _nhwc(a, prec), scale.float().cuda(), out, n, hb, hb, cb, cs,
                                 G.cur_stream())
        torch.cuda.synchronize()
        _tail_ok(out, numel, "conv_down_mask")
        exp = _nhwc(ref.float(), prec)
        assert torch.equal(_bits(out[:numel].view(exp.shape)), _bits(exp)), PREC_NAME[prec]
        assert bool((_bits(out[:numel].view(exp.shape))[~(a > 0).permute(0, 2, 3, 1).cuda()] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# jck_latent_loss_ex
# ---------------------------------------------------------------------------------------------------------------------
def _loss_inputs(n, hw, prec, seed=51):
    g = _gen(seed)
    x = torch.tanh(torch.randn(n, hw, 4, generator=g)).to(DT[prec])
    t = torch.rand(n, 3, hw, generator=g) * 2 - 1
    gx = (torch.randn(n, hw, 4, generator=g) * 1e-3).to(DT[prec])
    w = torch.randint(0, 3, (n, hw), generator=g).float()
    return x, t, gx, w


def _loss_ex(G, prec, x, t, w, gx, n, hw):
    graw, loss = _out(n * hw * 4, prec), _out(n, prec, torch.float32)
    dev = lambda v: None if v is None else v.cuda()
    G.lib.jck_latent_loss_ex(prec, x.cuda(), dev(t), dev(w), dev(gx), graw, loss, n, hw, G.cur_stream())
    torch.cuda.synchronize()
    _tail_ok(graw, n * hw * 4, "latent_loss_ex g_raw"), _tail_ok(loss, n, "latent_loss_ex loss")
    return graw[:n * hw * 4].view(n, hw, 4).clone(), loss[:n].clone()


@pytest.mark.parametrize("prec", [1, 0], ids=PREC_NAME.get)
@pytest.mark.parametrize("n,hw", [(1, 64), (5, 4096)])
def test_latent_loss_ex_is_latent_loss_without_weight_and_gradient(G, n, hw, prec):
    x, t, _, _ = _loss_inputs(n, hw, prec)
    graw, loss = _out(n * hw * 4, prec), _out(n, prec, torch.float32)
    G.lib.jck_latent_loss(prec, x.cuda(), t.cuda(), graw, loss, n, hw, G.cur_stream())
    torch.cuda.synchronize()
    for w in (torch.ones(n, hw), None):
        g1, l1 = _loss_ex(G, prec, x, t, w, None, n, hw)
        assert torch.equal(_bits(g1), _bits(graw[:n * hw * 4].view(n, hw, 4))) and torch.equal(_bits(l1), _bits(loss[:n])), w is None


@pytest.mark.parametrize("prec", [1, 0], ids=PREC_NAME.get)
@pytest.mark.parametrize("n,hw", [(1, 64), (5, 4096)])
def test_latent_loss_ex_weighted(G, n, hw, prec):
    """integer weights in {0, 1, 2} and a real image gradient against fp64; an all-zero weight row: loss 0, the critic part alone;
    target NULL: loss 0, g_raw = g_x (1 - x^2)"""
    x, t, gx, w = _loss_inputs(n, hw, prec)
    w[n - 1] = 0.0 if n > 1 else w[n - 1]
    xd = x.double()[..., :3]                                                         # [n, hw, 3]
    d = xd - t.double().permute(0, 2, 1)
    sw = w.double().sum(1)
    k = torch.where(sw > 0, 2.0 / (3.0 * sw.clamp_min(1)), torch.zeros_like(sw))
    ref_loss = torch.where(sw > 0, (w.double().unsqueeze(-1) * d * d).sum(dim=(1, 2)) / (3.0 * sw.clamp_min(1)), torch.zeros_like(sw))
    crit = gx.double()[..., :3] * (1.0 - xd * xd)
    ref_g = k.view(-1, 1, 1) * w.double().unsqueeze(-1) * d * (1.0 - xd * xd) + crit
    g0, l0 = _loss_ex(G, prec, x, t, w, gx, n, hw)
    g1, l1 = _loss_ex(G, prec, x, t, w, gx, n, hw)
    assert torch.equal(_bits(g0), _bits(g1)) and torch.equal(_bits(l0), _bits(l1)), "two runs differ"
    rel = ((l0.cpu().double() - ref_loss).abs() / ref_loss.clamp_min(1e-30)).max().item()
    print(f"latent_loss_ex n={n} hw={hw} {PREC_NAME[prec]}: loss rel err {rel:.3e}")
    assert rel <= G.TOL[prec]
    G.check(g0[..., :3].cpu(), ref_g, G.TOL[prec], "latent_loss_ex gradient")
    assert bool((_bits(g0[..., 3]) == 0).all()), "padding channel is not +0"
    if n > 1:
        assert float(l0[n - 1]) == 0.0
        G.check(g0[n - 1, :, :3].cpu(), crit[n - 1], G.TOL[prec], "all-zero weights: the critic part alone")
    gn, ln = _loss_ex(G, prec, x, None, None, gx, n, hw)
    assert bool((ln == 0).all())
    G.check(gn[..., :3].cpu(), crit, G.TOL[prec], "target NULL")
    from hipgan import JckError
    with pytest.raises(JckError):
        G.lib.jck_latent_loss_ex(prec, x.cuda(), None, None, None, _out(n * hw * 4, prec), _out(n, prec, torch.float32), n, hw, G.cur_stream())


# ---------------------------------------------------------------------------------------------------------------------
# jck_leaky_affine_bwd, jck_critic_ds
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [1, 0], ids=PREC_NAME.get)
@pytest.mark.parametrize("rows,c", [(3, 8), (37, 64), (1030, 512)])
def test_leaky_affine_bwd(G, rows, c, prec):
    gen = _gen(81)
    a = torch.randn(rows, c, generator=gen)
    a.view(-1)[::5] = 0.0
    a.view(-1)[1::7] = -0.0
    a.view(-1)[2::9] = float("nan")
    scale = torch.pow(2.0, (torch.arange(c) % 16 - 8).double())
    for exact in (True, False):
        g = torch.randint(-15, 16, (rows, c), generator=gen).float() if exact else torch.randn(rows, c, generator=gen).to(DT[prec]).float()
        sc = scale if exact else scale * (1.0 + torch.rand(c, generator=gen).double())
        t = g.double() * sc.float().double()
        ref = torch.where(a.double() > 0, t, t * (SLOPE if exact else float(np.float32(0.2))))
        out = _out(rows * c, prec)
        G.lib.jck_leaky_affine_bwd(prec, g.to(DT[prec]).cuda(), a.to(DT[prec]).cuda(), sc.float().cuda(), SLOPE if exact else 0.2, out, rows, c,
                                   G.cur_stream())
        torch.cuda.synchronize()
        _tail_ok(out, rows * c, "leaky_affine_bwd")
        got = out[:rows * c].view(rows, c)
        if exact:
            assert torch.equal(_bits(got), _bits(ref.float().to(DT[prec]).cuda())), (rows, c, PREC_NAME[prec])
            buf = g.to(DT[prec]).cuda()                                              # in place
            G.lib.jck_leaky_affine_bwd(prec, buf, a.to(DT[prec]).cuda(), sc.float().cuda(), SLOPE, buf, rows, c, G.cur_stream())
            assert torch.equal(_bits(buf), _bits(got))
        else:
            G.check(got.cpu(), ref, G.TOL[prec], "leaky_affine_bwd")


def test_critic_ds(G):
    from hipgan import JckError
    gen = _gen(91)
    l = torch.cat([torch.randn(300, generator=gen) * 4, torch.tensor([0.0, -0.0, 80.0, -80.0, 1e-8, 30.0, -30.0])])
    n = l.numel()
    ld = l.double()
    for mode, lam in ((1, 0.003), (1, 1.0), (2, 0.5), (2, 1.0)):
        lam32 = float(np.float32(lam))
        c, dc = (F.softplus(-ld), -torch.sigmoid(-ld)) if mode == 1 else (-ld, -torch.ones_like(ld))
        ds, term = _out(n, 1), _out(n, 1)
        G.lib.jck_critic_ds(l.cuda(), mode, lam, n, ds, term, G.cur_stream())
        torch.cuda.synchronize()
        _tail_ok(ds, n, "critic_ds"), _tail_ok(term, n, "critic_ds")
        assert bool(torch.isfinite(ds[:n]).all()) and bool(torch.isfinite(term[:n]).all()), "logits +-80 must stay finite"
        if mode == 2:                                                                # exact: a product of two fp32 numbers
            assert torch.equal(term[:n].cpu().double(), (lam32 * c).float().double()) and torch.equal(ds[:n].cpu().double(), (lam32 * dc).float().double())
        G.check(term[:n].cpu(), lam32 * c, G.TOL[1], f"critic_ds term mode {mode}")
        G.check(ds[:n].cpu(), lam32 * dc, G.TOL[1], f"critic_ds ds mode {mode}")
        rel = ((ds[:n].cpu().double() - lam32 * dc).abs() / (lam32 * dc).abs().clamp_min(1e-300)).max().item()
        assert rel < 1e-5, f"critic_ds ds mode {mode}: element-wise relative error {rel:.2e} (the small tail of the sigmoid)"
    bad = torch.tensor([float("nan"), float("inf"), -float("inf"), 1.0])
    for mode in (1, 2):
        ds, term = _out(4, 1), _out(4, 1)
        G.lib.jck_critic_ds(bad.cuda(), mode, 1.0, 4, ds, term, G.cur_stream())
        torch.cuda.synchronize()
        assert bool(torch.isnan(ds[:3]).all()) and bool(torch.isnan(term[:3]).all()) and bool(torch.isfinite(ds[3:4]).all())
    with pytest.raises(JckError):
        G.lib.jck_critic_ds(bad.cuda(), 0, 1.0, 4, ds, term, G.cur_stream())


# ---------------------------------------------------------------------------------------------------------------------
# engine
# ---------------------------------------------------------------------------------------------------------------------
def _ref_discriminator(eng):
    """fp64 functional discriminator under model.eval() from the engine's own state: (x [n,3,S,S], labels or None) -> logit [n]"""
    sd = {k: v.detach().cpu().double() for k, v in eng.state_dicts()[1].items()}
    ns = sum(1 for k in sd if k.startswith("norm") and k.endswith(".weight"))

    def dis(x, lab=None):
        for i in range(1, ns + 1):
            x = F.conv2d(x, sd[f"conv{i}.weight"], None, 2, 1)
            x = F.batch_norm(x, sd[f"norm{i}.running_mean"], sd[f"norm{i}.running_var"], sd[f"norm{i}.weight"], sd[f"norm{i}.bias"], False, 0.1, 1e-5)
            x = F.leaky_relu(x, 0.2)
        if lab is None:
            return F.conv2d(x, sd[f"conv{ns + 1}.weight"]).reshape(-1)
        e = F.leaky_relu(F.linear(lab.double(), sd["label_embedding.weight"], sd["label_embedding.bias"]), 0.2)
        h = F.linear(torch.cat([x.flatten(1), e], 1), sd["linear1.weight"], sd["linear1.bias"])          # Dropout: the identity
        return F.linear(h, sd["linear2.weight"], sd["linear2.bias"]).reshape(-1)
    return dis


_nets = {}


def _refs(family, prec, batch=8, size=64):
    eng = _engine(family, prec, batch, size)
    key = (family, prec, batch, size)
    if key not in _nets:
        _nets[key] = (_ref_generator(eng), _ref_discriminator(eng))
    return (eng,) + _nets[key]


def _critic(logit, mode):
    return F.softplus(-logit) if mode == "nsgan" else -logit


def _wloss(x, t, w):
    """sum_p w_p sum_c (x - t)^2 / (3 sum_p w_p) per image; w [n,S,S] fp64"""
    return (w.unsqueeze(1) * (x - t) ** 2).sum(dim=(1, 2, 3)) / (3.0 * w.sum(dim=(1, 2)))


def _centre_weight(size, n, window=7):
    from hipgan.inpaint import importance_weights, parse_mask
    return importance_weights(parse_mask(f"center:{size // 2}", size), window).unsqueeze(0).expand(n, -1, -1).contiguous()


_cases = {}


def _case(family, prec, n, size=64, batch=8):
    """(engine, z, labels, target, weight, fp64 references): critic_grad in both modes and latent_grad with a centre-hole importance
    weight and critic_weight 0.003; one reference per engine"""
    eng, gen, dis = _refs(family, prec, batch, size)
    key = (family, prec, n, size)
    if key not in _cases:
        z, lab = _z(n, 7, family)
        with torch.no_grad():
            t = gen(_z(n, 8, family)[0].double(), lab).float()
        w = _centre_weight(size, n)
        ref = {}
        for mode in ("nsgan", "logit"):
            zz = z.double().requires_grad_(True)
            logit = dis(gen(zz, lab), lab)
            term = _critic(logit, mode)
            ref[mode] = (logit.detach(), term.detach(), torch.autograd.grad(term.sum(), zz)[0])
        zz = z.double().requires_grad_(True)
        x = gen(zz, lab)
        loss, logit = _wloss(x, t.double(), w.double()), dis(x, lab)
        term = float(np.float32(CW)) * _critic(logit, "nsgan")
        ref["inpaint"] = (loss.detach(), term.detach(), logit.detach(), torch.autograd.grad((loss + term).sum(), zz)[0])
        _cases[key] = (z, lab, t, w, ref)
    return (eng,) + _cases[key]


def _dz_err(dz, ref):
    return ((dz.cpu().double() - ref).norm(dim=1) / ref.norm(dim=1)).max().item()


def _check_case(eng, z, lab, t, w, ref, prec, what):
    worst = 0.0
    for mode in ("nsgan", "logit"):
        logit, term, dz = eng.critic_grad(z, lab, mode=mode)
        rl, rt, rd = ref[mode]
        assert logit.shape == rl.shape and dz.shape == rd.shape and bool(torch.isfinite(dz).all())
        ed = _dz_err(dz, rd)
        print(f"{what} critic_grad {mode}: dz rel L2 per image, worst {ed:.3e} (bound {DZ_TOL[prec]})")
        _parity(logit, rl, prec, f"{what} critic_grad {mode} logit")
        _parity(term, rt, prec, f"{what} critic_grad {mode} term")
        worst = max(worst, ed)
    loss, term, logit, dz = eng.latent_grad(z, t, lab, weight=w, critic="nsgan", critic_weight=CW)
    rl, rt, rg, rd = ref["inpaint"]
    el = ((loss.cpu().double() - rl).abs() / rl).max().item()
    ed = _dz_err(dz, rd)
    print(f"{what} latent_grad weight + critic: loss rel err {el:.3e} (bound {LOSS_TOL[prec]}), dz rel L2 per image, worst {ed:.3e} "
          f"(bound {DZ_TOL[prec]})")
    _parity(logit, rg, prec, f"{what} latent_grad logit")
    _parity(term, rt, prec, f"{what} latent_grad term")
    worst = max(worst, ed)
    assert el < LOSS_TOL[prec], what
    assert worst < DZ_TOL[prec], f"{what}: dz rel L2 {worst:.3e}"


@pytest.mark.parametrize("family,prec", ENGINES)
def test_latent_grad_ex_matches_fp64_autograd(family, prec):
    """critic_grad in both modes and latent_grad with a centre-hole importance weight and critic_weight 0.003, n = 5 (ragged on a
    batch-8 engine) and n = 1, against fp64 autograd through the functional generator and discriminator.
    Measured on an MI355X, dz relative L2 of the worst image (critic_grad nsgan / critic_grad logit / weight + critic), n = 5:
    dcgan f32 1.7e-6 / 1.7e-6 / 1.2e-6, cgan f32 1.8e-6 / 1.7e-6 / 1.3e-6; dcgan bf16 0.133 / 0.134 / 0.085, cgan bf16 0.126 / 0.125 / 0.080
    (n = 1: dcgan bf16 0.132 / 0.131 / 0.082, cgan bf16 0.077 / 0.077 / 0.040); loss relative error 7.4e-4 (dcgan bf16), 1.4e-3
    (cgan bf16).  D here is the oracle's untrained discriminator (|logit| ~ 0.05): its gradient is a sum of many terms of either
    sign, which is why the bf16 chain loses three times what the projection's loses (0.038)."""
    eng, z, lab, t, w, ref = _case(family, prec, 5)
    _check_case(eng, z, lab, t, w, ref, prec, f"{family} {prec} n=5")
    one = lambda x: None if x is None else x[2:3]
    ref1 = {k: tuple(v[2:3] for v in vals) for k, vals in ref.items()}
    _check_case(eng, z[2:3], one(lab), t[2:3], w[2:3], ref1, prec, f"{family} {prec} n=1")


def test_latent_grad_ex_128():
    """the 128 x 128 plan (five stages each way), f32, n = 2 on a batch-4 engine"""
    eng, z, lab, t, w, ref = _case("dcgan", "f32", 2, size=128, batch=4)
    _check_case(eng, z, lab, t, w, ref, "f32", "dcgan f32 128x128 n=2")


# ---------------------------------------------------------------------------------------------------------------------
# equalities, bitwise
# ---------------------------------------------------------------------------------------------------------------------
def _targets(n, seed):
    return torch.rand(n, 3, 64, 64, generator=_gen(seed)) * 2 - 1


@pytest.mark.parametrize("family,prec", ENGINES)
def test_plain_calls_are_the_projection(G, family, prec):
    """project(...) without the new keywords, jck_engine_project called directly and jck_engine_project_ex with no weight and no
    critic: the same bits; likewise latent_grad"""
    eng = _engine(family, prec)
    z0, lab = _z(5, 101, family)
    t = _targets(5, 102)
    z, hist = eng.project(t, lab, steps=3, lr=0.05, prior=0.01, z0=z0)
    dev = lambda x: None if x is None else x.cuda()
    res = []
    for ex in (False, True):
        zz, m, v, h = z0.cuda().clone(), torch.zeros(5, 100, device="cuda"), torch.zeros(5, 100, device="cuda"), torch.empty(3, 5, device="cuda")
        if ex:
            G.lib.jck_engine_project_ex(eng._h, zz, dev(lab), t.cuda(), 5, 3, 0.05, 0.01, None, 0, 0.0, m, v, 0, h, None, G.cur_stream())
        else:
            G.lib.jck_engine_project(eng._h, zz, dev(lab), t.cuda(), 5, 3, 0.05, 0.01, m, v, 0, h, G.cur_stream())
        torch.cuda.synchronize()
        res.append((zz, h, m, v))
    for zz, h, m, v in res:
        assert torch.equal(zz, z) and torch.equal(h, hist) and torch.equal(m, eng.project_state["m"]) and torch.equal(v, eng.project_state["v"])
    loss, dz = eng.latent_grad(z0, t, lab)
    l2, d2 = torch.empty(5, device="cuda"), torch.empty(5, 100, device="cuda")
    G.lib.jck_engine_latent_grad_ex(eng._h, z0.cuda(), dev(lab), t.cuda(), None, 0, 0.0, 5, l2, None, None, d2, G.cur_stream())
    assert torch.equal(l2, loss) and torch.equal(d2, dz)


@pytest.mark.parametrize("family,prec", ENGINES)
def test_project_ex_continues_steps_and_rows(G, family, prec):
    """with a weight and a critic: 6 + 6 updates equal 12 through project_state; a 1-step project_ex from a given (m, v, t0) equals
    latent_grad_ex followed by jck_latent_adam on the same state; n = 11 on a batch-8 engine equals its rows computed alone; two
    runs give the same bits"""
    eng = _engine(family, prec)
    z0, lab = _z(11, 111, family)
    t, w = _targets(11, 112), _centre_weight(64, 11)
    kw = dict(lr=0.05, prior=0.01, weight=w, critic="nsgan", critic_weight=CW)
    sub = lambda x, lo, hi: None if x is None else x[lo:hi]
    z12, h12 = eng.project(t, lab, steps=12, z0=z0, **kw)
    t12 = eng.project_term.clone()
    assert eng.project_state["t"] == 12 and h12.shape == (12, 11) and bool(torch.isfinite(h12).all()) and bool((t12 > 0).all())
    again = eng.project(t, lab, steps=12, z0=z0, **kw)
    assert torch.equal(again[0], z12) and torch.equal(again[1], h12) and torch.equal(eng.project_term, t12)
    za, ha = eng.project(t, lab, steps=6, z0=z0, **kw)
    st, ta = eng.project_state, eng.project_term.clone()
    zb, hb = eng.project(t, lab, steps=6, z0=za, state=st, **kw)
    assert torch.equal(zb, z12) and torch.equal(torch.cat([ha, hb]), h12) and torch.equal(torch.cat([ta, eng.project_term]), t12)
    for lo, hi in ((0, 8), (8, 11), (9, 10), (3, 4)):
        zs, hs = eng.project(t[lo:hi], sub(lab, lo, hi), steps=12, z0=z0[lo:hi], **{**kw, "weight": w[lo:hi]})
        assert torch.equal(zs, z12[lo:hi]) and torch.equal(hs, h12[:, lo:hi]) and torch.equal(eng.project_term, t12[:, lo:hi]), (lo, hi)
    full = eng.latent_grad(z0, t, lab, weight=w, critic="nsgan", critic_weight=CW)
    row = eng.latent_grad(z0[9:10], t[9:10], sub(lab, 9, 10), weight=w[9:10], critic="nsgan", critic_weight=CW)
    assert all(torch.equal(a[9:10], b) for a, b in zip(full, row)) and torch.equal(full[0], h12[0]) and torch.equal(full[1], t12[0])
    lg, tg, dg = eng.critic_grad(z0, lab, "logit")
    l1, t1, d1 = eng.critic_grad(z0[10:11], sub(lab, 10, 11), "logit")
    assert torch.equal(lg[10:11], l1) and torch.equal(tg[10:11], t1) and torch.equal(dg[10:11], d1) and torch.equal(tg, -lg)
    # one step from a given state
    n, prec_id = 5, 0 if prec == "bf16" else 1
    gen = _gen(113)
    m0, v0, t0 = torch.randn(n, 100, generator=gen) * 1e-3, torch.rand(n, 100, generator=gen) * 1e-6, 4
    dev = lambda x: None if x is None else x[:n].cuda().contiguous()
    zz, m, v, h, th = dev(z0), m0.cuda(), v0.cuda(), torch.empty(1, n, device="cuda"), torch.empty(1, n, device="cuda")
    G.lib.jck_engine_project_ex(eng._h, zz, dev(lab), dev(t), n, 1, 0.05, 0.01, dev(w), 1, CW, m, v, t0, h, th, G.cur_stream())
    loss, term, dz = torch.empty(n, device="cuda"), torch.empty(n, device="cuda"), torch.empty(n, 100, device="cuda")
    G.lib.jck_engine_latent_grad_ex(eng._h, dev(z0), dev(lab), dev(t), dev(w), 1, CW, n, loss, term, None, dz, G.cur_stream())
    z2, m2, v2, op = dev(z0), m0.cuda(), v0.cuda(), torch.zeros(n, 128, dtype=DT[prec_id], device="cuda")
    G.lib.jck_latent_adam(prec_id, dz, 1, 100, z2, m2, v2, 0.05, 0.01, t0 + 1, op, 128, n, G.cur_stream())
    torch.cuda.synchronize()
    assert torch.equal(zz, z2) and torch.equal(m, m2) and torch.equal(v, v2) and torch.equal(h[0], loss) and torch.equal(th[0], term)


# ---------------------------------------------------------------------------------------------------------------------
# behaviour, asserted on the fp64 reference first
# ---------------------------------------------------------------------------------------------------------------------
_planted = {}


def _planted_inpainting(family, prec):
    """t = G(z*), the centre 32 x 32 unknown, every known pixel weight 1, no critic, z0 = z* + 0.3 eps; the fp64 run: 12 updates of
    torch.optim.Adam(lr = 0.05) -> (loss history [12, 4], hidden-pixel RMSE to t at z0 and at the end)"""
    eng, gen, _ = _refs(family, prec)
    if (family, prec) not in _planted:
        from hipgan.inpaint import importance_weights, parse_mask
        known = parse_mask("center:32", 64)
        w = importance_weights(known, 0).unsqueeze(0).expand(4, -1, -1).contiguous()
        zs, lab = _z(4, 21, family)
        with torch.no_grad():
            t = gen(zs.double(), lab).float()
        z0 = zs + 0.3 * torch.randn(4, 100, generator=_gen(22))
        zz = z0.double().clone().requires_grad_(True)
        opt = torch.optim.Adam([zz], lr=0.05, betas=(0.9, 0.999), eps=1e-8)
        hist = []
        for _ in range(12):
            opt.zero_grad()
            loss = _wloss(gen(zz, lab), t.double(), w.double())
            hist.append(loss.detach().clone())
            loss.sum().backward()
            opt.step()
        _planted[(family, prec)] = (z0, lab, t, w, known, torch.stack(hist))
    return (eng, gen) + _planted[(family, prec)]


def _hidden_rmse(x, t, known):
    h = (~known).double().view(1, 1, *known.shape)
    return ((h * (x.double() - t.double()) ** 2).sum(dim=(1, 2, 3)) / (3.0 * h.sum())).sqrt()


@pytest.mark.parametrize("family,prec", ENGINES)
def test_planted_inpainting_descends(family, prec):
    """the fp64 history falls monotonically (asserted first); the device history then falls monotonically too, its end / start ratio
    is within the planted-optimum bounds (1e-3 f32, 6e-2 bf16) of the fp64 run's, and the completed picture's RMSE to t over the
    HIDDEN pixels is smaller at the end than at z0"""
    eng, gen, z0, lab, t, w, known, ref = _planted_inpainting(family, prec)
    assert bool((ref[1:] < ref[:-1]).all()), f"the fp64 history does not fall monotonically: {ref.tolist()}"
    z, hist = eng.project(t, lab, steps=12, lr=0.05, z0=z0, weight=w)
    hist = hist.cpu().double()
    assert z.shape == (4, 100) and hist.shape == (12, 4) and bool(torch.isfinite(hist).all())
    ratio, rref = hist[-1] / hist[0], ref[-1] / ref[0]
    dev = ((ratio - rref).abs() / rref).max().item()
    print(f"planted inpainting {family} {prec}: loss end / start {ratio.tolist()} (fp64 {rref.tolist()}), worst relative deviation {dev:.3e}")
    assert bool((hist[1:] <= hist[:-1]).all()), f"loss history is not non-increasing: {hist.tolist()}"
    assert dev < {"f32": 1e-3, "bf16": 6e-2}[prec]
    x0, x1 = eng.sample(z0, lab, bn="running").cpu(), eng.sample(z, lab, bn="running").cpu()
    k = known.view(1, 1, 64, 64)
    r0, r1 = _hidden_rmse(torch.where(k, t, x0), t, known), _hidden_rmse(torch.where(k, t, x1), t, known)
    print(f"planted inpainting {family} {prec}: hidden-pixel RMSE {r0.tolist()} -> {r1.tolist()}")
    assert bool((r1 < r0).all())


@pytest.mark.parametrize("family,prec", ENGINES)
def test_refine_raises_the_logit(family, prec):
    """refine(z, steps=10, lr=0.02, mode="logit"), n = 4: the fp64 run (Adam on -logit) raises every row's logit (asserted first); the
    device run's mean gain is at least half the reference's, and logit_after is score_latents(z') bit for bit"""
    eng, gen, dis = _refs(family, prec)
    z0, lab = _z(4, 121, family)
    zz = z0.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([zz], lr=0.02, betas=(0.9, 0.999), eps=1e-8)
    with torch.no_grad():
        before = dis(gen(zz, lab), lab).clone()
    for _ in range(10):
        opt.zero_grad()
        (-dis(gen(zz, lab), lab)).sum().backward()
        opt.step()
    with torch.no_grad():
        after = dis(gen(zz, lab), lab)
    assert bool((after > before).all()), f"the fp64 run does not raise every logit: {before.tolist()} -> {after.tolist()}"
    z, lb, la = eng.refine(z0, lab, steps=10, lr=0.02, mode="logit")
    gain, rgain = float((la - lb).double().mean()), float((after - before).mean())
    print(f"refine {family} {prec}: logit {lb.tolist()} -> {la.tolist()}; mean gain {gain:.4f} (fp64 {rgain:.4f})")
    assert z.shape == (4, 100) and gain >= 0.5 * rgain
    assert torch.equal(la, eng.score_latents(z, lab)[0]) and torch.equal(lb, eng.score_latents(z0, lab)[0])
    assert torch.equal(eng.project_term[0], -lb)                            # the term before the first update is -logit(z0)


# ---------------------------------------------------------------------------------------------------------------------
# state and pipeline
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,prec", ENGINES)
def test_writes_no_parameter_or_buffer(family, prec):
    eng = _engine(family, prec)
    z0, lab = _z(5, 131, family)
    t, w = _targets(5, 132), _centre_weight(64, 5)
    before = _arenas(eng)
    eng.project(t, lab, steps=2, z0=z0, weight=w, critic="nsgan", critic_weight=CW)
    eng.latent_grad(z0, t, lab, weight=w, critic="logit", critic_weight=CW)
    eng.critic_grad(z0, lab)
    eng.refine(z0, lab, steps=2)
    after = _arenas(eng)
    assert set(before) == set(after) and all(torch.equal(before[k], after[k]) for k in before)


def test_between_two_training_steps_changes_no_bit():
    """A training engine (DCGAN, B = 8, bf16, the next batch announced so that its D(real) forward is in flight) with a masked
    projection with critic, a critic_grad and a refinement between every two steps: scalars and every arena equal those of the run
    without them, bit for bit."""
    from hipgan.engine import DcganEngine
    from oracle.gan_oracle import build_params
    from util import synth_images
    B, steps = 8, 3
    imgs = synth_images(B * steps).cuda()
    t, w, z0 = _targets(5, 142), _centre_weight(64, 5), _z(5, 141, "dcgan")[0]
    res = []
    for with_calls in (False, True):
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
            if kw:
                assert eng._prefetched_real is not None
            if with_calls:
                _, hist = eng.project(t, steps=2, z0=z0, weight=w, critic="nsgan", critic_weight=CW)
                logit, _, dz = eng.critic_grad(z0)
                z1, _, la = eng.refine(z0, steps=2)
                assert bool(torch.isfinite(hist).all()) and bool(torch.isfinite(dz).all()) and bool(torch.isfinite(la).all())
                if kw:
                    assert eng._prefetched_real is not None          # the calls did not drop the prefetched pass
            scal.append(eng.scalars())
        torch.cuda.synchronize()
        res.append((scal, {k: v.clone() for k, v in eng.arenas.items()}))
    assert res[0][0] == res[1][0], (res[0][0], res[1][0])
    for k, v in res[0][1].items():
        assert torch.equal(v, res[1][1][k]), k


def test_argument_errors_launch_nothing(G):
    from hipgan import JckError
    from hipgan.engine import DcganEngine
    eng, ceng = _engine("dcgan", "f32"), _engine("cgan", "f32")
    f = lambda *s: torch.full(s, 7.0, device="cuda")
    z, m, v, hist, th, t, w = f(9, 100), f(9, 100), f(9, 100), f(2, 9), f(2, 9), f(9, 3, 64, 64), f(9, 64, 64)
    loss, term, logit, dz = f(9), f(9), f(9), f(9, 100)
    st = G.cur_stream()
    grad = lambda e, lab, tt, mode, cw, n: G.lib.jck_engine_latent_grad_ex(e._h, z, lab, tt, w, mode, cw, n, loss, term, logit, dz, st)
    proj = lambda e, lab, tt, mode, cw, n, steps=2: G.lib.jck_engine_project_ex(e._h, z, lab, tt, n, steps, 0.05, 0.0, w, mode, cw, m, v, 0, hist, th, st)
    for call in (grad, proj):
        with pytest.raises(JckError, match="n must be in"):
            call(eng, None, t, 1, CW, 9)
        with pytest.raises(JckError, match="critic_mode"):
            call(eng, None, t, 3, CW, 8)
        with pytest.raises(JckError, match="critic_weight"):
            call(eng, None, t, 1, -1.0, 8)
        with pytest.raises(JckError, match="critic is required"):
            call(eng, None, None, 0, 0.0, 8)
        with pytest.raises(JckError, match="labels"):
            call(ceng, None, t, 1, CW, 8)
    with pytest.raises(JckError, match="steps"):
        proj(eng, None, t, 1, CW, 8, 0)
    fresh = DcganEngine(batch=8, prec="f32")                                       # D never loaded: its operands were never packed
    with pytest.raises(JckError, match="never packed"):
        grad(fresh, None, t, 1, CW, 8)
    torch.cuda.synchronize()
    for x in (z, m, v, hist, th, loss, term, logit, dz):
        assert bool((x == 7.0).all()), "a refused call wrote an output"
    tt, zz = torch.zeros(4, 3, 64, 64), torch.zeros(4, 100)
    with pytest.raises(JckError, match="critic must be"):
        eng.project(tt, critic="hinge")
    with pytest.raises(JckError, match="critic_weight"):
        eng.latent_grad(zz, tt, critic="nsgan", critic_weight=-1.0)
    with pytest.raises(JckError, match="weight must be"):
        eng.project(tt, weight=torch.ones(32, 32))
    with pytest.raises(JckError, match="all zero"):
        eng.project(tt, weight=torch.zeros(64, 64))
    with pytest.raises(JckError, match="mode"):
        eng.critic_grad(zz, mode="hinge")
    with pytest.raises(JckError, match="labels"):
        ceng.critic_grad(zz)
    with pytest.raises(JckError, match="never loaded"):
        fresh.critic_grad(zz)
    with pytest.raises(JckError, match="never loaded"):
        fresh.refine(zz)


def test_sampler_inpaint_and_refine_round_trip():
    """pictures the sampler drew itself with the centre hidden: 30 updates end below the weighted loss at z0 for every image, the
    completed picture keeps the known pixels; refine and images(select="refine") agree; without a discriminator all of it is refused"""
    from hipgan import JckError
    from hipgan.inpaint import importance_weights, parse_mask
    from hipgan.sampler import Sampler, images_to_target, latents
    s = Sampler.from_checkpoint(_ckpt(), "DCGAN", batch=8, with_d=True)
    u8 = s.images(6, seed=1)
    known = parse_mask("center:32", 64)
    r = s.inpaint(u8, known, steps=30, lr=0.05, critic_weight=CW, seed=9)
    assert sorted(r) == ["completed", "generated", "loss", "term", "z"]
    assert r["z"].shape == (6, 100) and r["loss"].shape == (6,) and r["term"].shape == (6,) and bool((r["term"] > 0).all())
    assert r["generated"].shape == u8.shape and r["generated"].dtype == torch.uint8 and r["completed"].dtype == torch.uint8
    k = known.cuda().view(1, 64, 64, 1).expand_as(u8)
    assert torch.equal(r["completed"][k], u8[k]) and torch.equal(r["completed"][~k], r["generated"][~k])
    assert torch.equal(r["generated"], s.from_latents(r["z"]))
    w = importance_weights(known, 7).unsqueeze(0).expand(6, -1, -1).contiguous()
    start = s.engine.latent_grad(latents(6, 9), images_to_target(u8.cpu()), weight=w)[0]
    print(f"Sampler.inpaint: weighted loss at z0 {start.tolist()} -> {r['loss'].tolist()}")
    assert bool((r["loss"] < start).all())
    r2 = s.inpaint(u8, known, steps=30, lr=0.05, critic_weight=CW, seed=9, restarts=2)
    assert bool((r2["loss"] + r2["term"] <= r["loss"] + r["term"]).all())       # seed 9 is one of the two starts, and rows are independent
    r0 = s.inpaint(u8, known, steps=5, critic_weight=0.0, seed=9)
    assert bool((r0["term"] == 0).all())
    z0 = latents(6, 3)
    z, lb, la = s.refine(z0, steps=5)
    img, info = s.images(6, seed=3, select="refine", refine_steps=5, return_info=True)
    assert torch.equal(info["z"], z.cpu()) and torch.equal(info["logit_after"], la.cpu()) and torch.equal(info["logit_before"], lb.cpu())
    assert torch.equal(img, s.from_latents(z)) and float((la - lb).mean()) > 0
    with pytest.raises(JckError, match="no pixel known"):
        s.inpaint(u8, torch.zeros(64, 64, dtype=torch.bool))
    plain = Sampler.from_checkpoint(_ckpt(), "DCGAN", batch=8)
    for call in (lambda: plain.inpaint(u8, known, steps=2), lambda: plain.refine(z0), lambda: plain.images(2, select="refine")):
        with pytest.raises(JckError, match="with_d=True"):
            call()
    assert plain.inpaint(u8, known, steps=2, critic_weight=0.0)["z"].shape == (6, 100)      # no critic: no discriminator needed


def test_generate_cli_inpaints_and_refines(tmp_path):
    import generate
    path = str(tmp_path / "ckpt.pt")
    torch.save(_ckpt(), path)
    base = ["-m", "DCGAN", "--checkpoint", path, "-b", "8"]
    assert generate.main(base + ["--num", "5", "--seed", "3", "--out", str(tmp_path / "s")]) == 0
    src = np.load(str(tmp_path / "s" / "images.npz"))
    assert sorted(src.files) == ["images", "z"]                                  # without the new flags: what the tool wrote before
    from hipgan.sampler import Sampler, latents
    s = Sampler.from_checkpoint(path, "DCGAN", batch=8)
    assert np.array_equal(src["images"], s.from_latents(latents(5, 3)).cpu().numpy()) and np.array_equal(src["z"], latents(5, 3).numpy())
    assert generate.main(base + ["--inpaint", str(tmp_path / "s" / "images.npz"), "--mask", "half:left", "--project_steps", "20", "--seed", "4",
                                 "--out", str(tmp_path / "i")]) == 0
    f = np.load(str(tmp_path / "i" / "inpainted.npz"))
    assert sorted(f.files) == ["completed", "images", "known", "loss", "term", "z"]
    assert f["z"].shape == (5, 100) and f["loss"].shape == (5,) and f["images"].shape == src["images"].shape and f["known"].shape == (64, 64)
    assert np.array_equal(f["completed"][:, :, 32:], src["images"][:, :, 32:]) and np.array_equal(f["completed"][:, :, :32], f["images"][:, :, :32])
    assert bool(np.isfinite(f["loss"]).all()) and bool((f["term"] > 0).all())
    png = open(str(tmp_path / "i" / "inpainted.png"), "rb").read()
    assert png[:8] == b"\x89PNG\r\n\x1a\n" and len(png) > 1000
    assert generate.main(base + ["--num", "5", "--seed", "3", "--refine", "4", "--out", str(tmp_path / "r")]) == 0
    r = np.load(str(tmp_path / "r" / "images.npz"))
    assert sorted(r.files) == ["images", "logit_after", "logit_before", "z"] and r["logit_after"].shape == (5,)
    assert float((r["logit_after"] - r["logit_before"]).mean()) > 0 and not np.array_equal(r["z"], src["z"])
    sd = Sampler.from_checkpoint(path, "DCGAN", batch=8, with_d=True)
    assert np.array_equal(r["images"], sd.from_latents(torch.from_numpy(r["z"])).cpu().numpy())
    assert np.array_equal(sd.score_latents(torch.from_numpy(r["z"]))[0].cpu().numpy(), r["logit_after"])
