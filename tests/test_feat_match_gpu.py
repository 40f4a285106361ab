"""Feature matching on the discriminator's activations: jck_feat_match, jck_engine_latent_grad_fm / _project_fm, DcganEngine.latent_grad /
.project with feature_target, Sampler.anomaly and generate.py --anomaly.

Per op, exact (the integer-data pattern of tests/test_critic_grad_gpu.py): a and f integers in [-8, 7], weight 2^-3, M a power of two,
scale[c] = 2^(c mod 16 - 8), slope 0.25: 225 M < 2^24, so fterm is exact in any summation order and g is the one rounding of an exact
value, which fp64 -> fp32 -> T reproduces.

Engine: the reference is the fp64 functional generator of tests/test_project_gpu.py and an fp64 discriminator truncated at stage k,
built from eng.state_dicts()[1] (F.conv2d, F.batch_norm(training=False), leaky_relu(0.2)), autograd for dz and torch.optim.Adam for
the updates.  The feature targets are uniform images, not generator outputs (on those a - f cancels).  Bounds: fterm and loss relative
LOSS_TOL (1e-3 f32, 3e-2 bf16), logit and term the _parity bound, dz relative L2 per image 5e-3 in f32.  bf16 dz, the rule of
tests/test_critic_grad_gpu.py: DZ_TOL["bf16"] = min(2 x the worst image measured, 0.25); the measured values are in the docstring of
test_latent_grad_fm_matches_fp64_autograd."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_critic_grad_gpu import _centre_weight, _critic, _ref_discriminator, _wloss
from test_project_gpu import _ref_generator
from test_sample_eval_gpu import _parity
from test_score_gpu import _arenas, _ckpt, _engine, _images, _z

pytestmark = pytest.mark.gpu
PREC_NAME = {0: "bf16", 1: "f32", 2: "bf16x3"}
DT = {0: torch.bfloat16, 1: torch.float32, 2: torch.float32}
TAIL = 1024
SLOPE = 0.25
WEIGHT = 2.0 ** -3
ENGINES = [pytest.param(f, p, id=f"{f}-{p}") for f in ("dcgan", "cgan") for p in ("bf16", "f32")]
LOSS_TOL = {"f32": 1e-3, "bf16": 3e-2}                 # the project's step-scalar bounds
DZ_WORST_BF16 = 0.101                                  # the worst image measured on an MI355X (test_latent_grad_fm_matches_fp64_autograd)
DZ_TOL = {"f32": 5e-3, "bf16": min(2 * DZ_WORST_BF16, 0.25)}      # f32: the project's gradient bound; bf16: 2 x the worst measured value, at most 0.25
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


# ---------------------------------------------------------------------------------------------------------------------
# jck_feat_match, exact
# ---------------------------------------------------------------------------------------------------------------------
FM_SHAPES = [(1, 2, 8), (1, 4, 512), (3, 32, 64), (2, 4, 1024)]          # (N, H, C): M = H^2 C = 32, 8192, 65536, 16384
_fm_cache = {}


def _fm_data(shape):
    """(a, f, old [N, M] fp32 integers / multiples of the scale, scale [C], fp64 references {acc: (g, fterm)}, slope-branch g)"""
    if shape not in _fm_cache:
        n, h, c = shape
        m = h * h * c
        assert m & (m - 1) == 0 and 225 * m < 2 ** 24
        gen = _gen(41)
        a = torch.randint(-8, 8, (n, m), generator=gen).float()
        f = torch.randint(-8, 8, (n, m), generator=gen).float()
        flat = a.view(-1)
        idx = torch.randperm(flat.numel(), generator=gen)
        k = flat.numel() // 10
        flat[idx[:k]] = 0.0
        flat[idx[k:2 * k]] = -0.0
        scale = torch.pow(2.0, (torch.arange(c) % 16 - 8).double())
        sc = scale.repeat(m // c).view(1, m)
        kg = 2.0 * WEIGHT / m
        old = torch.randint(0, 16, (n, m), generator=gen).double() * sc * kg          # the same power-of-two scale: the sum stays exact
        d = a.double() - f.double()
        t = sc * (kg * d)
        g = torch.where(a.double() > 0, t, t * SLOPE)
        fterm = (WEIGHT / m) * (d * d).sum(1)
        _fm_cache[shape] = (a, f, old.float(), scale.float(), {0: (g, fterm), 1: (old + g, fterm)}, t * SLOPE)
    return _fm_cache[shape]


def _fm_run(G, prec, a, f, scale, acc, old, n, m, c, weight=WEIGHT):
    gy, ft = _out(n * m, prec), _out(n, prec, torch.float32)
    if acc:
        gy[:n * m] = old.to(DT[prec]).cuda().view(-1)
    G.lib.jck_feat_match(prec, a.to(DT[prec]).cuda(), f.to(DT[prec]).cuda(), scale.cuda(), SLOPE, weight, gy, acc, ft, n, m, c, G.cur_stream())
    torch.cuda.synchronize()
    _tail_ok(gy, n * m, "feat_match g_y"), _tail_ok(ft, n, "feat_match fterm")
    return gy[:n * m].view(n, m).clone(), ft[:n].clone()


@pytest.mark.parametrize("prec", [0, 1, 2], ids=PREC_NAME.get)
@pytest.mark.parametrize("shape", FM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_feat_match_exact(G, shape, prec):
    n, h, c = shape
    m = h * h * c
    a, f, old, scale, ref, slope_branch = _fm_data(shape)
    for acc in (0, 1):
        what = f"feat_match {shape} {PREC_NAME[prec]} accumulate {acc}"
        g, ft = _fm_run(G, prec, a, f, scale, acc, old, n, m, c)
        exp = ref[acc][0].float().to(DT[prec]).cuda()                         # fp64 -> fp32 exact, -> T the one rounding
        if not torch.equal(_bits(g), _bits(exp)):
            bad = torch.nonzero(_bits(g) != _bits(exp))
            i = tuple(bad[0].tolist())
            raise AssertionError(f"{what}: {bad.shape[0]} of {exp.numel()} elements differ, first at {i}: got {float(g[i]):.10g} "
                                 f"exact {float(exp[i]):.10g}")
        assert torch.equal(_bits(ft), _bits(ref[acc][1].float().cuda())), f"{what}: fterm {ft.tolist()} exact {ref[acc][1].tolist()}"
        g2, ft2 = _fm_run(G, prec, a, f, scale, acc, old, n, m, c)
        assert torch.equal(_bits(g), _bits(g2)) and torch.equal(_bits(ft), _bits(ft2)), f"{what}: two runs differ"
        if acc == 0:                                                          # +0 and -0 activations: the slope branch, each
            sb = _bits(slope_branch.float().to(DT[prec]).cuda())
            for name, pick in (("+0", (a == 0) & ~torch.signbit(a)), ("-0", (a == 0) & torch.signbit(a))):
                assert int(pick.sum()) >= a.numel() // 10, (what, name)
                assert torch.equal(_bits(g)[pick.cuda()], sb[pick.cuda()]), f"{what}: an activation of {name} did not take the slope branch"
        if n > 1:                                                             # row b does not depend on N
            for b in range(n):
                gb, fb = _fm_run(G, prec, a[b:b + 1], f[b:b + 1], scale, acc, old[b:b + 1], 1, m, c)
                assert torch.equal(_bits(gb), _bits(g[b:b + 1])) and torch.equal(_bits(fb), _bits(ft[b:b + 1])), (what, b)


@pytest.mark.parametrize("prec", [0, 1, 2], ids=PREC_NAME.get)
def test_feat_match_nan_stays_in_its_cell(G, prec):
    shape = (3, 32, 64)
    n, h, c = shape
    m = h * h * c
    a, f, old, scale, ref, slope_branch = _fm_data(shape)
    cell = 12345
    an = a.clone()
    an[1, cell] = float("nan")
    for acc in (0, 1):
        g0, ft0 = _fm_run(G, prec, a, f, scale, acc, old, n, m, c)
        g, ft = _fm_run(G, prec, an, f, scale, acc, old, n, m, c)
        assert bool(torch.isnan(ft[1])) and bool(torch.isnan(g[1, cell]))
        assert torch.equal(_bits(ft[[0, 2]]), _bits(ft0[[0, 2]])) and torch.equal(_bits(g[[0, 2]]), _bits(g0[[0, 2]]))
        keep = torch.ones(m, dtype=torch.bool, device="cuda")
        keep[cell] = False
        assert torch.equal(_bits(g[1])[keep], _bits(g0[1])[keep]) and not bool(torch.isnan(g[1][keep]).any())


def test_feat_match_refuses_bad_arguments(G):
    from hipgan import JckError
    n, m, c = 2, 512, 64
    f32 = lambda *s: torch.full(s, 7.0, device="cuda")
    a, f, gy, ft, sc = f32(n * m + 4), f32(n * m + 4), f32(n * m + 4), f32(n + 4), f32(c + 4)
    st = G.cur_stream()
    call = lambda prec=1, a=a, f=f, sc=sc, w=WEIGHT, gy=gy, ft=ft, n=n, m=m, c=c: G.lib.jck_feat_match(prec, a, f, sc, SLOPE, w, gy, 0, ft, n, m, c, st)
    bad = [lambda: call(a=None), lambda: call(f=None), lambda: call(sc=None), lambda: call(gy=None), lambda: call(ft=None),      # a null pointer
           lambda: call(n=0),                                                                                                    # N < 1
           lambda: call(c=4, m=512), lambda: call(c=48, m=480), lambda: call(c=0),                                              # C
           lambda: call(m=96), lambda: call(m=0),                                                                                # M no multiple of C
           lambda: call(w=-1.0), lambda: call(w=float("inf")), lambda: call(w=float("nan")),                                     # weight
           lambda: call(a=a[1:]), lambda: call(f=f[1:]), lambda: call(gy=gy[1:]), lambda: call(sc=sc[1:]),                       # alignment
           lambda: call(prec=3), lambda: call(prec=-1)]                                                                          # prec
    for fn in bad:
        with pytest.raises(JckError):
            fn()
    torch.cuda.synchronize()
    assert bool((gy == 7.0).all()) and bool((ft == 7.0).all()), "a refused call wrote an output"


# ---------------------------------------------------------------------------------------------------------------------
# engine against fp64 autograd
# ---------------------------------------------------------------------------------------------------------------------
def _ref_features(eng):
    """fp64 functional discriminator under model.eval(), truncated: (x [n,3,S,S], k) -> the LeakyReLU output of conv stage k"""
    sd = {k: v.detach().cpu().double() for k, v in eng.state_dicts()[1].items()}
    ns = sum(1 for k in sd if k.startswith("norm") and k.endswith(".weight"))

    def feat(x, k):
        for i in range(1, k + 2):
            x = F.conv2d(x, sd[f"conv{i}.weight"], None, 2, 1)
            x = F.batch_norm(x, sd[f"norm{i}.running_mean"], sd[f"norm{i}.running_var"], sd[f"norm{i}.weight"], sd[f"norm{i}.bias"], False, 0.1, 1e-5)
            x = F.leaky_relu(x, 0.2)
        return x
    return feat, ns


_nets = {}


def _refs(family, prec, batch=8, size=64):
    eng = _engine(family, prec, batch, size)
    key = (family, prec, batch, size)
    if key not in _nets:
        _nets[key] = (_ref_generator(eng), _ref_discriminator(eng)) + _ref_features(eng)
    return (eng,) + _nets[key]


def _fterm(feat, x, ft, k, fw):
    with torch.no_grad():
        target = feat(ft.double(), k)
    return fw * (feat(x, k) - target).pow(2).mean(dim=(1, 2, 3))


_cases = {}


def _case(family, prec, n, size=64, batch=8, only=None):
    """(engine, z, labels, pixel target, weight, feature target, {name: (keywords, fp64 loss, term, logit, fterm, dz)})"""
    eng, gen, dis, feat, ns = _refs(family, prec, batch, size)
    key = (family, prec, n, size, only)
    if key not in _cases:
        top = ns - 1
        z, lab = _z(n, 7, family)
        with torch.no_grad():
            t = gen(_z(n, 8, family)[0].double(), lab).float()
        w = _centre_weight(size, n)
        ft = _images(n, 9, size)
        plan = {"feature top": (False, False, top, 1.0), "feature 0": (False, False, 0, 1.0), "pixel + feature 1": (True, False, 1, 100.0),
                "weight + critic + feature top": (True, True, top, 100.0), "weight + critic + feature 1": (True, True, 1, 100.0)}
        if only:
            plan = {only: (True, False, top, 100.0)}
        ref = {}
        for name, (pixel, critic, k, fw) in plan.items():
            zz = z.double().requires_grad_(True)
            x = gen(zz, lab)
            zero = torch.zeros(n, dtype=torch.float64)
            loss = zero if not pixel else _wloss(x, t.double(), w.double()) if critic else (x - t.double()).pow(2).mean(dim=(1, 2, 3))
            logit = dis(x, lab) if critic else None
            term = float(np.float32(CW)) * _critic(logit, "nsgan") if critic else zero
            fterm = _fterm(feat, x, ft, k, fw)
            dz = torch.autograd.grad((loss + term + fterm).sum(), zz)[0]
            kw = dict(feature_target=ft, feature_weight=fw, feature_stage=k)
            if critic:
                kw.update(weight=w, critic="nsgan", critic_weight=CW)
            det = lambda v: None if v is None else v.detach()
            ref[name] = (pixel, kw, det(loss), det(term), det(logit), det(fterm), dz)
        _cases[key] = (z, lab, t, ft, ref)
    return (eng,) + _cases[key]


def _dz_err(dz, ref):
    return ((dz.cpu().double() - ref).norm(dim=1) / ref.norm(dim=1)).max().item()


def _check_case(eng, z, lab, t, ref, prec, what, rows=slice(None)):
    sub = lambda v: None if v is None else v[rows]
    worst = 0.0
    for name, (pixel, kw, rl, rt, rg, rf, rd) in ref.items():
        kw = {k: (sub(v) if torch.is_tensor(v) else v) for k, v in kw.items()}
        r = eng.latent_grad(z[rows], t[rows] if pixel else None, sub(lab), **kw)
        assert sorted(r) == ["dz", "fterm", "logit", "loss", "term"] and r["dz"].shape == rd[rows].shape and bool(torch.isfinite(r["dz"]).all())
        ef = ((r["fterm"].cpu().double() - rf[rows]).abs() / rf[rows]).max().item()
        el = ((r["loss"].cpu().double() - rl[rows]).abs() / rl[rows]).max().item() if pixel else float(r["loss"].abs().max())
        ed = _dz_err(r["dz"], rd[rows])
        print(f"{what} {name}: fterm {rf[rows].tolist()} rel err {ef:.3e}, loss rel err {el:.3e} (bound {LOSS_TOL[prec]}), dz rel L2 per image, "
              f"worst {ed:.3e} (bound {DZ_TOL[prec]})")
        assert ef < LOSS_TOL[prec], f"{what} {name}: fterm rel err {ef:.3e}"
        assert el < LOSS_TOL[prec] if pixel else el == 0.0, f"{what} {name}: loss {el:.3e}"
        if rg is not None:
            _parity(r["logit"], rg[rows], prec, f"{what} {name} logit")
            _parity(r["term"], rt[rows], prec, f"{what} {name} term")
        else:
            assert bool((r["term"] == 0).all()) and bool(torch.isnan(r["logit"]).all())
        worst = max(worst, ed)
    assert worst < DZ_TOL[prec], f"{what}: dz rel L2 {worst:.3e}"


@pytest.mark.parametrize("family,prec", ENGINES)
def test_latent_grad_fm_matches_fp64_autograd(family, prec):
    """feature only at the deepest stage and at stage 0 (feature_weight 1), pixel + feature at stage 1 (feature_weight 100), per-pixel
    weight + nsgan critic (0.003) + feature at the deepest stage and at stage 1 (both injection points), n = 5 (ragged on a batch-8
    engine) and n = 1, against fp64 autograd through the functional generator and the truncated discriminator.
    Measured on an MI355X, dz relative L2 of the worst image (feature top / feature 0 / pixel + feature 1 / weight + critic + feature
    top / weight + critic + feature 1): dcgan bf16 n = 5 0.101 / 0.076 / 0.046 / 0.082 / 0.079, n = 1 0.094 / 0.076 / 0.038 / 0.082 /
    0.079; cgan bf16 n = 5 0.089 / 0.073 / 0.045 / 0.075 / 0.070, n = 1 0.056 / 0.041 / 0.021 / 0.038 / 0.037; f32 at most 6.9e-6.
    fterm relative error: bf16 at most 1.4e-3, f32 at most 5.4e-7.  The worst, 0.101, gives DZ_TOL["bf16"] = 0.202."""
    eng, z, lab, t, ft, ref = _case(family, prec, 5)
    _check_case(eng, z, lab, t, ref, prec, f"{family} {prec} n=5")
    _check_case(eng, z, lab, t, ref, prec, f"{family} {prec} n=1", slice(2, 3))


def test_latent_grad_fm_128():
    """the 128 x 128 plan (NS = 5), f32, n = 2 on a batch-4 engine: pixel + feature at the deepest stage"""
    eng, z, lab, t, ft, ref = _case("dcgan", "f32", 2, size=128, batch=4, only="pixel + feature top")
    _check_case(eng, z, lab, t, ref, "f32", "dcgan f32 128x128 n=2")


# ---------------------------------------------------------------------------------------------------------------------
# equalities, bitwise
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,prec", ENGINES)
def test_fm_without_a_feature_term_is_ex(G, family, prec):
    """_fm with feat_target NULL, or with a feature target and weight 0, equals _ex bit for bit, with and without a critic"""
    eng = _engine(family, prec)
    z0, lab = _z(5, 101, family)
    t, w, ft = _images(5, 102), _centre_weight(64, 5), _images(5, 103).cuda()
    dev = lambda x: None if x is None else x.cuda()
    st = G.cur_stream()
    new = lambda *s: torch.empty(*s, device="cuda")
    for mode, ww in ((0, None), (1, w)):
        runs = []
        for feat in (None, (None, -1, 0.0), (ft, 1, 0.0), (None, 2, 0.0)):
            zz, m, v, h, th, fh = z0.cuda().clone(), torch.zeros(5, 100, device="cuda"), torch.zeros(5, 100, device="cuda"), new(3, 5), new(3, 5), new(3, 5)
            loss, term, logit, dz, fterm = new(5), new(5), new(5), new(5, 100), new(5)
            a1 = (eng._h, zz, dev(lab), t.cuda(), 5, 3, 0.05, 0.01, dev(ww), mode, CW, m, v, 0, h, th if mode else None, st)
            a2 = (eng._h, z0.cuda(), dev(lab), t.cuda(), dev(ww), mode, CW, 5, loss, term if mode else None, logit if mode else None, dz, st)
            if feat is None:
                G.lib.jck_engine_project_ex(*a1)
                G.lib.jck_engine_latent_grad_ex(*a2)
            else:
                G.lib.jck_engine_project_fm(*a1, feat[0], feat[1], feat[2], fh)
                G.lib.jck_engine_latent_grad_fm(*a2, feat[0], feat[1], feat[2], fterm)
            torch.cuda.synchronize()
            runs.append((zz, m, v, h, loss, dz) + ((th, term, logit) if mode else ()))
        for r in runs[1:]:
            assert all(torch.equal(a, b) for a, b in zip(runs[0], r)), (family, prec, mode)
    z, hist = eng.project(t, lab, steps=3, lr=0.05, prior=0.01, z0=z0)          # and the Python keywords at their defaults
    assert eng.project_fterm is None
    z2, hist2 = eng.project(t, lab, steps=3, lr=0.05, prior=0.01, z0=z0, feature_target=ft, feature_weight=0.0)
    assert torch.equal(z, z2) and torch.equal(hist, hist2) and eng.project_fterm is None


@pytest.mark.parametrize("family,prec", ENGINES)
def test_project_fm_continues_steps_and_rows(G, family, prec):
    """with a weight, a critic and a feature term at stage 1: 6 + 6 updates equal 12 through project_state, project_fterm included; n =
    11 on a batch-8 engine equals its rows computed alone; two runs give the same bits; a 1-step project_fm from a given (m, v, t0)
    equals latent_grad_fm followed by jck_latent_adam on the same state"""
    eng = _engine(family, prec)
    z0, lab = _z(11, 111, family)
    t, w, ft = _images(11, 112), _centre_weight(64, 11), _images(11, 114)
    kw = dict(lr=0.05, prior=0.01, weight=w, critic="nsgan", critic_weight=CW, feature_target=ft, feature_weight=100.0, feature_stage=1)
    sub = lambda x, lo, hi: None if x is None else x[lo:hi]
    z12, h12 = eng.project(t, lab, steps=12, z0=z0, **kw)
    t12, f12 = eng.project_term.clone(), eng.project_fterm.clone()
    assert eng.project_state["t"] == 12 and f12.shape == (12, 11) and bool(torch.isfinite(f12).all()) and bool((f12 > 0).all())
    again = eng.project(t, lab, steps=12, z0=z0, **kw)
    assert torch.equal(again[0], z12) and torch.equal(again[1], h12) and torch.equal(eng.project_term, t12) and torch.equal(eng.project_fterm, f12)
    za, ha = eng.project(t, lab, steps=6, z0=z0, **kw)
    st, ta, fa = eng.project_state, eng.project_term.clone(), eng.project_fterm.clone()
    zb, hb = eng.project(t, lab, steps=6, z0=za, state=st, **kw)
    assert torch.equal(zb, z12) and torch.equal(torch.cat([ha, hb]), h12) and torch.equal(torch.cat([ta, eng.project_term]), t12)
    assert torch.equal(torch.cat([fa, eng.project_fterm]), f12)
    for lo, hi in ((0, 8), (8, 11), (9, 10), (3, 4)):
        zs, hs = eng.project(t[lo:hi], sub(lab, lo, hi), steps=12, z0=z0[lo:hi], **{**kw, "weight": w[lo:hi], "feature_target": ft[lo:hi]})
        assert torch.equal(zs, z12[lo:hi]) and torch.equal(hs, h12[:, lo:hi]) and torch.equal(eng.project_fterm, f12[:, lo:hi]), (lo, hi)
    gkw = {k: v for k, v in kw.items() if k not in ("lr", "prior")}
    full = eng.latent_grad(z0, t, lab, **gkw)
    row = eng.latent_grad(z0[9:10], t[9:10], sub(lab, 9, 10), **{**gkw, "weight": w[9:10], "feature_target": ft[9:10]})
    assert all(torch.equal(full[k][9:10], row[k]) for k in full) and torch.equal(full["fterm"], f12[0]) and torch.equal(full["loss"], h12[0])
    only = eng.latent_grad(z0, None, lab, feature_target=ft, feature_weight=1.0, feature_stage=0)          # feature only, three chunks
    for lo, hi in ((0, 8), (10, 11)):
        r = eng.latent_grad(z0[lo:hi], None, sub(lab, lo, hi), feature_target=ft[lo:hi], feature_weight=1.0, feature_stage=0)
        assert all(torch.equal(only[k][lo:hi], r[k]) or k == "logit" for k in only), (lo, hi)
    # one step from a given state
    n, prec_id = 5, 0 if prec == "bf16" else 1
    gen = _gen(113)
    m0, v0, t0 = torch.randn(n, 100, generator=gen) * 1e-3, torch.rand(n, 100, generator=gen) * 1e-6, 4
    dev = lambda x: None if x is None else x[:n].cuda().contiguous()
    new = lambda *s: torch.empty(*s, device="cuda")
    zz, m, v, h, th, fh = dev(z0), m0.cuda(), v0.cuda(), new(1, n), new(1, n), new(1, n)
    G.lib.jck_engine_project_fm(eng._h, zz, dev(lab), dev(t), n, 1, 0.05, 0.01, dev(w), 1, CW, m, v, t0, h, th, G.cur_stream(), dev(ft), 1, 100.0, fh)
    loss, term, fterm, dz = new(n), new(n), new(n), new(n, 100)
    G.lib.jck_engine_latent_grad_fm(eng._h, dev(z0), dev(lab), dev(t), dev(w), 1, CW, n, loss, term, None, dz, G.cur_stream(), dev(ft), 1, 100.0, fterm)
    z2, m2, v2, op = dev(z0), m0.cuda(), v0.cuda(), torch.zeros(n, 128, dtype=DT[prec_id], device="cuda")
    G.lib.jck_latent_adam(prec_id, dz, 1, 100, z2, m2, v2, 0.05, 0.01, t0 + 1, op, 128, n, G.cur_stream())
    torch.cuda.synchronize()
    assert torch.equal(zz, z2) and torch.equal(m, m2) and torch.equal(v, v2)
    assert torch.equal(h[0], loss) and torch.equal(th[0], term) and torch.equal(fh[0], fterm)


# ---------------------------------------------------------------------------------------------------------------------
# state and pipeline
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,prec", ENGINES)
def test_fm_writes_no_parameter_or_buffer(family, prec):
    eng = _engine(family, prec)
    z0, lab = _z(5, 131, family)
    t, w, ft = _images(5, 132), _centre_weight(64, 5), _images(5, 133)
    before = _arenas(eng)
    eng.project(t, lab, steps=2, z0=z0, weight=w, critic="nsgan", critic_weight=CW, feature_target=ft, feature_weight=10.0, feature_stage=2)
    eng.project(None, lab, steps=2, z0=z0, feature_target=ft, feature_weight=1.0)
    eng.latent_grad(z0, t, lab, feature_target=ft, feature_weight=1.0, feature_stage=0)
    after = _arenas(eng)
    assert set(before) == set(after) and all(torch.equal(before[k], after[k]) for k in before)


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graph"])
def test_fm_between_two_training_steps_changes_no_bit(graphs):
    """A training engine (DCGAN, B = 8, bf16) with a feature-only projection, a pixel + critic + feature projection and a latent_grad
    with a feature term between every two steps: scalars and every arena (parameters, Adam moments, running statistics) equal those
    of the run without them, bit for bit, and so do the following steps' results.  eager: the next batch announced, so that its
    D(real) forward is in flight; graph: the steps replayed from captured graphs."""
    from hipgan.engine import DcganEngine
    from oracle.gan_oracle import build_params
    from util import synth_images
    B, steps = 8, 4 if graphs else 3
    imgs = synth_images(B * steps).cuda()
    t, w, ft, z0 = _images(5, 142), _centre_weight(64, 5), _images(5, 143), _z(5, 141, "dcgan")[0]
    res = []
    for with_calls in (False, True):
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
            if with_calls:
                _, h1 = eng.project(None, steps=2, z0=z0, feature_target=ft, feature_weight=1.0)
                f1 = eng.project_fterm
                _, h2 = eng.project(t, steps=2, z0=z0, weight=w, critic="nsgan", critic_weight=CW, feature_target=ft, feature_weight=10.0, feature_stage=1)
                r = eng.latent_grad(z0, t, feature_target=ft, feature_weight=1.0, feature_stage=0)
                assert all(bool(torch.isfinite(x).all()) for x in (h1, f1, h2, eng.project_fterm, r["fterm"], r["dz"]))
                if kw:
                    assert eng._prefetched_real is not None          # the calls did not drop the prefetched pass
            scal.append(eng.scalars())
        torch.cuda.synchronize()
        assert (len(eng._graph_cache) > 0) == graphs
        res.append((scal, {k: v.clone() for k, v in eng.arenas.items()}))
    assert res[0][0] == res[1][0], (res[0][0], res[1][0])
    for k, v in res[0][1].items():
        assert torch.equal(v, res[1][1][k]), k


def test_fm_argument_errors_launch_nothing(G):
    from hipgan import JckError
    from hipgan.engine import DcganEngine
    eng, ceng = _engine("dcgan", "f32"), _engine("cgan", "f32")
    f = lambda *s: torch.full(s, 7.0, device="cuda")
    z, m, v, hist, th, fh, t, w, ft = f(9, 100), f(9, 100), f(9, 100), f(2, 9), f(2, 9), f(2, 9), f(9, 3, 64, 64), f(9, 64, 64), f(9, 3, 64, 64)
    loss, term, logit, dz, fterm = f(9), f(9), f(9), f(9, 100), f(9)
    st = G.cur_stream()

    def grad(e, lab, tt, mode, cw, n, fx, fk, fw):
        return G.lib.jck_engine_latent_grad_fm(e._h, z, lab, tt, w, mode, cw, n, loss, term, logit, dz, st, fx, fk, fw, fterm)

    def proj(e, lab, tt, mode, cw, n, fx, fk, fw, steps=2):
        return G.lib.jck_engine_project_fm(e._h, z, lab, tt, n, steps, 0.05, 0.0, w, mode, cw, m, v, 0, hist, th, st, fx, fk, fw, fh)
    for call in (grad, proj):
        with pytest.raises(JckError, match="n must be in"):
            call(eng, None, t, 0, 0.0, 9, ft, -1, 1.0)
        with pytest.raises(JckError, match="critic_mode"):
            call(eng, None, t, 3, CW, 8, ft, -1, 1.0)
        for bad in (-1.0, float("inf"), float("nan")):
            with pytest.raises(JckError, match="feat_weight"):
                call(eng, None, t, 0, 0.0, 8, ft, -1, bad)
        with pytest.raises(JckError, match="feature target"):
            call(eng, None, t, 0, 0.0, 8, None, -1, 1.0)
        for bad in (-2, 4, 7):
            with pytest.raises(JckError, match="feat_stage"):
                call(eng, None, t, 0, 0.0, 8, ft, bad, 1.0)
        with pytest.raises(JckError, match="without a target and without a feature term a critic is required"):
            call(eng, None, None, 0, 0.0, 8, None, -1, 0.0)
        with pytest.raises(JckError, match="without a target and without a feature term a critic is required"):
            call(eng, None, None, 0, 0.0, 8, ft, -1, 0.0)
        with pytest.raises(JckError, match="labels"):
            call(ceng, None, t, 0, 0.0, 8, ft, -1, 1.0)
    with pytest.raises(JckError, match="steps"):
        proj(eng, None, t, 0, 0.0, 8, ft, -1, 1.0, 0)
    fresh = DcganEngine(batch=8, prec="f32")                                       # D never loaded: its operands were never packed
    for call in (grad, proj):
        with pytest.raises(JckError, match="never packed"):
            call(fresh, None, t, 0, 0.0, 8, ft, -1, 1.0)
    torch.cuda.synchronize()
    for x in (z, m, v, hist, th, fh, loss, term, logit, dz, fterm):
        assert bool((x == 7.0).all()), "a refused call wrote an output"
    tt, zz = torch.zeros(4, 3, 64, 64), torch.zeros(4, 100)
    for call in (lambda **kw: eng.latent_grad(zz, tt, **kw), lambda **kw: eng.project(tt, steps=1, **kw)):
        with pytest.raises(JckError, match="feature_weight"):
            call(feature_target=tt, feature_weight=-1.0)
        with pytest.raises(JckError, match="feature_weight"):
            call(feature_target=tt, feature_weight=float("nan"))
        with pytest.raises(JckError, match="needs a feature_target"):
            call(feature_weight=1.0)
        with pytest.raises(JckError, match="feature_stage"):
            call(feature_target=tt, feature_weight=1.0, feature_stage=4)
        with pytest.raises(JckError, match="feature_target must be"):
            call(feature_target=tt[:3], feature_weight=1.0)
        with pytest.raises(JckError, match="feature_target must be"):
            call(feature_target=torch.zeros(4, 3, 128, 128), feature_weight=1.0)
    with pytest.raises(JckError, match="never loaded"):
        fresh.latent_grad(zz, tt, feature_target=tt, feature_weight=1.0)
    u8 = torch.randint(0, 256, (4, 64, 64, 3), generator=_gen(5), dtype=torch.uint8)          # uint8 NHWC is u8 / 127.5 - 1
    a = eng.latent_grad(zz, tt, feature_target=u8, feature_weight=1.0)
    b = eng.latent_grad(zz, tt, feature_target=(u8.float() / 127.5 - 1.0).permute(0, 3, 1, 2), feature_weight=1.0)
    assert all(torch.equal(a[k], b[k]) or k == "logit" for k in a)


# ---------------------------------------------------------------------------------------------------------------------
# Sampler.anomaly, asserted on the fp64 reference first
# ---------------------------------------------------------------------------------------------------------------------
_anomaly_ref = {}


def _anomaly_reference(steps=60, lr=0.05, lam=0.1, seed=7):
    """four of the generator's own images (z from seed 8) and four uniform images (seed 9); the fp64 run of Sampler.anomaly's
    objective with torch.optim.Adam -> (images, residual, feature, score)"""
    if not _anomaly_ref:
        from hipgan.sampler import latents
        eng, gen, dis, feat, ns = _refs("dcgan", "bf16")                   # the engine _ckpt() is taken from
        with torch.no_grad():
            own = gen(_z(4, 8, "dcgan")[0].double()).float()
        images = torch.cat([own, _images(4, 9)])
        fw, k = lam / (1.0 - lam), ns - 1
        with torch.no_grad():
            target = feat(images.double(), k)
        zz = latents(8, seed).double().clone().requires_grad_(True)
        opt = torch.optim.Adam([zz], lr=lr, betas=(0.9, 0.999), eps=1e-8)

        def terms():
            x = gen(zz)
            return (x - images.double()).pow(2).mean(dim=(1, 2, 3)), (feat(x, k) - target).pow(2).mean(dim=(1, 2, 3))
        for _ in range(steps):
            opt.zero_grad()
            res, fe = terms()
            (res + fw * fe).sum().backward()
            opt.step()
        with torch.no_grad():
            res, fe = terms()
        _anomaly_ref["r"] = (images, res, fe, (1.0 - lam) * res + lam * fe)
    return _anomaly_ref["r"]


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_sampler_anomaly_separates_own_images_from_noise(prec):
    """steps = 60, lr = 0.05, lam = 0.1, seed = 7, the deepest stage: every own-image score below 0.05 x the smallest uniform-image
    score, on the fp64 reference first and then on the engine; f32 residuals of the uniform images within 5 % of the reference's;
    AUROC 1.  Measured on an MI355X (largest own score / smallest uniform score): fp64 2.31e-4 / 0.2978, f32 2.31e-4 / 0.2978,
    bf16 2.27e-4 / 0.2978 - a ratio below 1e-3 against the required 0.05."""
    from hipgan.anomaly import auroc
    from hipgan.sampler import Sampler
    images, rres, rfe, rscore = _anomaly_reference()
    print(f"fp64 anomaly scores: own {rscore[:4].tolist()}, uniform {rscore[4:].tolist()}")
    assert float(rscore[:4].max()) < 0.05 * float(rscore[4:].min()), "the fp64 reference does not separate the two groups"
    s = Sampler.from_checkpoint(_ckpt(), "DCGAN", prec=prec, batch=8, with_d=True)
    r = s.anomaly(images, steps=60, lr=0.05, lam=0.1, seed=7)
    assert sorted(r) == ["feature", "generated", "residual", "score", "z"]
    assert r["z"].shape == (8, 100) and r["residual"].shape == r["feature"].shape == r["score"].shape == (8,)
    assert r["score"].dtype == torch.float64 and r["generated"].shape == (8, 64, 64, 3) and r["generated"].dtype == torch.uint8
    score = r["score"].cpu()
    print(f"{prec} anomaly scores: own {score[:4].tolist()}, uniform {score[4:].tolist()}; residual {r['residual'].tolist()} "
          f"(fp64 {rres.tolist()}), feature {r['feature'].tolist()} (fp64 {rfe.tolist()})")
    assert float(score[:4].max()) < 0.05 * float(score[4:].min())
    assert torch.equal(score, 0.9 * r["residual"].cpu().double() + 0.1 * r["feature"].cpu().double())
    if prec == "f32":
        rel = ((r["residual"][4:].cpu().double() - rres[4:]).abs() / rres[4:]).max().item()
        assert rel < 0.05, f"residual of the uniform images: {rel:.3e} from the fp64 run's"
    assert auroc(score, [0, 0, 0, 0, 1, 1, 1, 1]) == 1.0
    assert torch.equal(r["generated"], s.from_latents(r["z"]))


def test_generate_cli_anomaly(tmp_path):
    import generate
    path = str(tmp_path / "ckpt.pt")
    torch.save(_ckpt(), path)
    u8 = torch.randint(0, 256, (6, 64, 64, 3), generator=_gen(6), dtype=torch.uint8).numpy()
    flags = np.array([0, 1, 0, 1, 1, 0], dtype=bool)
    np.savez(str(tmp_path / "q.npz"), images=u8, anomalous=flags)
    base = ["-m", "DCGAN", "--checkpoint", path, "-b", "8"]
    out = tmp_path / "a"
    assert generate.main(base + ["--anomaly", str(tmp_path / "q.npz"), "--project_steps", "5", "--anomaly_lam", "0.2", "--anomaly_stage", "2",
                                 "--out", str(out)]) == 0
    f = np.load(str(out / "anomaly.npz"))
    assert sorted(f.files) == ["feature", "generated", "order", "residual", "score", "z"]
    assert f["z"].shape == (6, 100) and f["residual"].shape == f["feature"].shape == f["score"].shape == f["order"].shape == (6,)
    assert f["generated"].shape == u8.shape and f["generated"].dtype == np.uint8 and f["score"].dtype == np.float64
    assert sorted(f["order"].tolist()) == list(range(6)) and bool((np.diff(f["score"][f["order"]]) <= 0).all())
    assert np.allclose(f["score"], 0.8 * f["residual"].astype(np.float64) + 0.2 * f["feature"].astype(np.float64), rtol=1e-12, atol=0)
    png = open(str(out / "anomaly.png"), "rb").read()
    assert png[:8] == b"\x89PNG\r\n\x1a\n" and len(png) > 1000
    js = json.load(open(str(out / "anomaly.json")))
    from hipgan.anomaly import auroc
    assert js["auroc"] == auroc(f["score"], flags) and js["n"] == 6 and js["anomalous"] == 3 and js["lam"] == 0.2 and js["stage"] == 2
    np.savez(str(tmp_path / "plain.npz"), images=u8)                                # without flags: no json
    out2 = tmp_path / "b"
    assert generate.main(base + ["--anomaly", str(tmp_path / "plain.npz"), "--project_steps", "2", "--out", str(out2)]) == 0
    assert not (out2 / "anomaly.json").exists() and (out2 / "anomaly.npz").exists()
    out3 = tmp_path / "p"                                                           # perceptual projection through the CLI
    assert generate.main(base + ["--project", str(tmp_path / "plain.npz"), "--project_steps", "3", "--project_feature_weight", "10",
                                 "--out", str(out3)]) == 0
    assert np.load(str(out3 / "projected.npz"))["z"].shape == (6, 100)
