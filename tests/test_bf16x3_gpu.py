"""The bf16x3 precision (JCK_PREC_BF16X3, prec="bf16x3"): fp32 storage and every kernel choice of the f32 path, with the GEMM
operands split into two bf16 halves (hi = bf16(x), lo = bf16(x - hi)) and every product formed as lo*hi + hi*lo + hi*hi on
v_mfma_f32_16x16x32_bf16 with fp32 accumulation.

  * per op against float64 torch on the CPU: <= 3e-5 of the output's largest element, and >= 100x closer than the bf16 op
  * a GEMM whose three precisions give three different exact answers (the mode is the split product, not the f32 kernel)
  * whole DCGAN / CGAN steps against the CPU oracle: the north star's 1e-3 per step on every scalar
  * determinism, graph replay and the per-pass schedule; the module path, EngineAdam and JCKGAN_PREC in the trainer"""
import argparse
import copy

import pytest
import torch
import torch.nn.functional as F

import test_cgan_gpu as CG
from test_step_gpu import _rel
from test_step_gpu import _run as _dcgan_run

pytestmark = pytest.mark.gpu

BF16, F32, X3 = 0, 1, 2
SCALARS = ("loss_d", "loss_g", "gp", "loss_real", "loss_fake", "d_x", "d_gz1", "d_gz2")
LR = 2e-4


def _dt(prec):
    return torch.bfloat16 if prec == BF16 else torch.float32


def _lib():
    from hipgan import lib
    from hipgan._lib import cur_stream
    return lib, cur_stream()


def _nhwc(x, prec):
    n, c, h, w = x.shape
    t = torch.zeros(n, h, w, 4 if c == 3 else c)
    t[..., :c] = x.permute(0, 2, 3, 1)
    return t.to(_dt(prec)).cuda().contiguous()


def _nchw(t, c):
    return t.double().cpu()[..., :c].permute(0, 3, 1, 2).contiguous()


def _err(got, ref):
    """max |got - ref| relative to max |ref| (float64)"""
    return ((got.double() - ref).abs().max() / ref.abs().max()).item()


# ---- the ops; each takes fp32 CPU data, runs the library in `prec` and returns the result as float64 NCHW ----------------------
def _conv_down(prec, x, w):
    lib, st = _lib()
    n, cb, hb, _ = x.shape
    cs = w.shape[0]
    wp = torch.empty(lib.jck_pad_rows(cs) * 16 * lib.jck_pad_chan(cb), dtype=_dt(prec), device="cuda")
    lib.jck_pack_down(prec, w.cuda(), cs, cb, wp, st)
    out = torch.empty(n, hb // 2, hb // 2, cs, dtype=_dt(prec), device="cuda")
    lib.jck_conv_down(prec, _nhwc(x, prec), wp, out, None, None, n, hb, hb, cb, cs, st)
    torch.cuda.synchronize()
    return _nchw(out, cs)


def _conv_up(prec, x, w):
    lib, st = _lib()
    n, cs, hs, _ = x.shape
    cb = w.shape[1]
    wp = torch.empty(4 * lib.jck_pad_rows(cb) * 4 * cs, dtype=_dt(prec), device="cuda")
    lib.jck_pack_up(prec, w.cuda(), cs, cb, wp, st)
    out = torch.empty(n, 2 * hs, 2 * hs, lib.jck_pad_chan(cb), dtype=_dt(prec), device="cuda")
    lib.jck_conv_up(prec, _nhwc(x, prec), wp, out, None, None, 1 if cb == 3 else 0, n, hs, hs, cs, cb, st)
    torch.cuda.synchronize()
    return _nchw(out, cb)


def _g1_operands(prec, z, w, cip):
    lib, st = _lib()
    b, ci = z.shape[0], z.shape[1]
    co = w.shape[1]
    zp = torch.zeros(b, cip)
    zp[:, :ci] = z.view(b, ci)
    wp = torch.empty(16 * co * cip, dtype=_dt(prec), device="cuda")
    lib.jck_pack_g1(prec, w.cuda(), ci, co, cip, wp, st)
    return zp.to(_dt(prec)).cuda(), wp


def _g1_fwd(prec, z, w, cip):
    lib, st = _lib()
    b, co = z.shape[0], w.shape[1]
    zp, wp = _g1_operands(prec, z, w, cip)
    out = torch.empty(b, 4, 4, co, dtype=_dt(prec), device="cuda")
    lib.jck_g1_fwd(prec, zp, wp, out, None, None, b, cip, co, st)
    torch.cuda.synchronize()
    return _nchw(out, co)


def _conv_wgrad(prec, small, big):
    lib, st = _lib()
    n, cb, hb, _ = big.shape
    cs = small.shape[1]
    nb = lib.jck_conv_wgrad_ws_bytes(n, hb, hb, cb, cs)
    ws = torch.empty(nb // 4, device="cuda")
    grad = torch.full((cs, cb, 4, 4), float("nan"), device="cuda")
    lib.jck_conv_wgrad(prec, _nhwc(small, prec), _nhwc(big, prec), ws, nb, grad, 0, n, hb, hb, cb, cs, st)
    torch.cuda.synchronize()
    return grad.double().cpu()


def _g1_wgrad(prec, z, dy, cip):
    lib, st = _lib()
    b, ci, co = z.shape[0], z.shape[1], dy.shape[1]
    zp = torch.zeros(b, cip)
    zp[:, :ci] = z.view(b, ci)
    nb = lib.jck_g1_wgrad_ws_bytes(b, cip, co)
    ws = torch.empty(nb // 4, device="cuda")
    grad = torch.full((ci, co, 4, 4), float("nan"), device="cuda")
    lib.jck_g1_wgrad(prec, zp.to(_dt(prec)).cuda(), _nhwc(dy, prec), ws, nb, grad, 0, b, ci, cip, co, st)
    torch.cuda.synchronize()
    return grad.double().cpu()


L1 = (256, 8392, 8448, 12)      # CGAN's Linear(8392, 256): N, K, padded K, split-K layers (engine.hip)


def _linear(prec, x, w, ksplit=L1[3]):
    lib, st = _lib()
    B, K = x.shape
    N, KP = w.shape[0], (K + 63) // 64 * 64
    xp = torch.zeros(B, KP)
    xp[:, :K] = x
    wp = torch.empty(N * KP, dtype=_dt(prec), device="cuda")
    lib.jck_pack_linear(prec, w.cuda(), N, K, N, KP, 0, 0, 0, wp, st)
    slab = torch.full((ksplit, B, N), float("nan"), device="cuda")
    lib.jck_linear_fwd(prec, xp.to(_dt(prec)).cuda(), wp, None, slab, B, KP, N, N, ksplit, st)
    torch.cuda.synchronize()
    return slab.double().cpu().sum(0)


def _wgrad_ref(fwd, w_shape, args, upstream):
    w = torch.zeros(w_shape, dtype=torch.float64, requires_grad=True)
    (fwd(*[a.double() for a in args], w) * upstream.double()).sum().backward()
    return w.grad


def _cases():
    """(name, run(prec) -> float64 result, float64 reference) at the shapes of tests/test_ops_gpu.py; between them they take
    every tile variant of the register-staged gather-GEMM and weight gradient"""
    g = torch.Generator().manual_seed(11)
    out = []
    for n, hb, cb, cs in [(2, 8, 64, 128), (3, 64, 3, 64), (2, 16, 128, 256), (4, 8, 256, 512)]:
        x, w = torch.randn(n, cb, hb, hb, generator=g), torch.randn(cs, cb, 4, 4, generator=g) * 0.05
        out.append((f"conv_down{(n, hb, cb, cs)}", lambda p, x=x, w=w: _conv_down(p, x, w),
                    F.conv2d(x.double(), w.double(), None, 2, 1)))
    for n, hs, cs, cb in [(2, 4, 512, 256), (2, 8, 256, 128), (3, 16, 128, 64), (2, 32, 64, 3)]:
        x, w = torch.randn(n, cs, hs, hs, generator=g), torch.randn(cs, cb, 4, 4, generator=g) * 0.05
        ref = F.conv_transpose2d(x.double(), w.double(), None, 2, 1)
        out.append((f"conv_up{(n, hs, cs, cb)}", lambda p, x=x, w=w: _conv_up(p, x, w), torch.tanh(ref) if cb == 3 else ref))
    for b, ci, cip, co in [(8, 100, 128, 512), (256, 100, 128, 512)]:
        z, w = torch.randn(b, ci, 1, 1, generator=g), torch.randn(ci, co, 4, 4, generator=g) * 0.05
        out.append((f"g1_fwd{(b, ci, cip, co)}", lambda p, z=z, w=w, cip=cip: _g1_fwd(p, z, w, cip),
                    F.conv_transpose2d(z.double(), w.double(), None, 1, 0)))
        dy = torch.randn(b, co, 4, 4, generator=g)
        out.append((f"g1_wgrad{(b, ci, cip, co)}", lambda p, z=z, dy=dy, cip=cip: _g1_wgrad(p, z, dy, cip),
                    _wgrad_ref(lambda z_, w_: F.conv_transpose2d(z_, w_, None, 1, 0), (ci, co, 4, 4), [z], dy)))
    for n, hb, cb, cs in [(2, 8, 64, 128), (3, 64, 3, 64), (2, 16, 128, 256), (4, 8, 256, 512), (16, 32, 64, 128), (3, 16, 128, 64)]:
        big, small = torch.randn(n, cb, hb, hb, generator=g), torch.randn(n, cs, hb // 2, hb // 2, generator=g)
        out.append((f"conv_wgrad{(n, hb, cb, cs)}", lambda p, s=small, b_=big: _conv_wgrad(p, s, b_),
                    _wgrad_ref(lambda x_, w_: F.conv2d(x_, w_, None, 2, 1), (cs, cb, 4, 4), [big], small)))
    N, K = L1[0], L1[1]
    for B in (16, 300):
        x, w = torch.randn(B, K, generator=g) * 0.5, torch.randn(N, K, generator=g) * 0.02
        out.append((f"linear_splitk(B={B})", lambda p, x=x, w=w: _linear(p, x, w), x.double() @ w.double().t()))
    return out


def test_ops_against_float64():
    """Every GEMM-shaped op within 3e-5 of its output's largest element of float64 torch on the same fp32 data, and at least
    100x closer to it than the bf16 op on the same data."""
    bad, rows = [], []
    for name, run, ref in _cases():
        e3, e16 = _err(run(X3), ref), _err(run(BF16), ref)
        rows.append(f"{name}: bf16x3 {e3:.2e} bf16 {e16:.2e} ratio {e16 / max(e3, 1e-30):.0f}")
        if not (e3 <= 3e-5 and 100.0 * e3 <= e16):
            bad.append(rows[-1])
    print("\n".join(rows))
    assert not bad, "\n".join(bad)


def test_split_product_is_exact_and_distinct():
    """K = 64 with 16 terms (1 + 2^-10) * (1 + 2^-10) and the rest zero: hi = 1, lo = 2^-10 exactly, and each precision has ONE
    answer whatever the summation order - f32 16 + 2^-5 + 2^-16, bf16x3 16 + 2^-5 (lo*lo dropped), bf16 16.  Non-finite
    operands give non-finite outputs, never finite ones."""
    b, ci, cip, co = 4, 16, 64, 128
    v = 1.0 + 2.0 ** -10
    z = torch.full((b, ci, 1, 1), v)
    w = torch.full((ci, co, 4, 4), v)
    want = {F32: 16.0 + 2.0 ** -5 + 2.0 ** -16, X3: 16.0 + 2.0 ** -5, BF16: 16.0}
    for prec, val in want.items():
        out = _g1_fwd(prec, z, w, cip)
        assert torch.equal(out, torch.full_like(out, val)), (prec, out.unique().tolist(), val)
    z2, w2 = z.clone(), w.clone()
    z2[1, 0] = float("inf")
    z2[2, 3] = float("nan")
    w2[5, 2, 0, 0] = float("inf")
    w2[7, 6, 1, 2] = -float("inf")
    out = _g1_fwd(X3, z2, w2, cip)
    bad = torch.zeros_like(out, dtype=torch.bool)
    bad[1] = bad[2] = True
    bad[:, 2, 0, 0] = bad[:, 6, 1, 2] = True
    assert not torch.isfinite(out[bad]).any(), "a non-finite operand gave a finite output"
    assert torch.equal(out[~bad], torch.full_like(out[~bad], want[X3]))
    x = torch.zeros(8, 64)
    x[:, :16] = v
    x[3, 5] = float("inf")
    wl = torch.zeros(128, 64)
    wl[:, :16] = v
    o = _linear(X3, x, wl, ksplit=1)
    assert not torch.isfinite(o[3]).any()
    assert torch.equal(o[torch.arange(8) != 3], torch.full((7, 128), want[X3], dtype=torch.float64))


def _tensor_errs(views, refs):
    """per tensor: (max error / max |ref|, relative L2)"""
    out = {}
    for k, r in refs.items():
        g = views[k].detach().float().cpu().view(r.shape)
        out[k] = (((g - r).abs().max() / (r.abs().max() + 1e-30)).item(), ((g - r).norm() / (r.norm() + 1e-30)).item())
    return out


def _state_errs(views, refs):
    """weights after Adam, per tensor: (max |difference| in units of lr, fraction of elements more than lr/4 apart).  Adam moves an
    element by ~lr * sign(g) on the first step: an element whose gradient is within rounding of 0 may move the other way (2 lr)."""
    out = {}
    for k, r in refs.items():
        if r.dtype != torch.float32:
            continue
        d = (views[k].detach().float().cpu().view(r.shape) - r).abs()
        out[k] = (d.max().item() / LR, (d > 0.25 * LR).float().mean().item())
    return out


def _bn(k):
    return k.startswith("norm")


def _scalars_ok(got, ref):
    """the north star's 1e-3 relative per step.  D(x) / D(G(z)) are means of sigmoids: where D saturates (a mean below 1e-3) the
    relative error of the probability is the absolute error of a logit of -7 or less, so there it is compared as log(p)."""
    import math
    worst, bad = 0.0, []
    for k in SCALARS:
        g, r = got[k], ref[k]
        if k.startswith("d_") and 0.0 < r < 1e-3 and g > 0.0:
            g, r = math.log(g), math.log(r)
        e = _rel(g, r)
        worst = max(worst, e)
        if not e < 1e-3:
            bad.append((k, got[k], ref[k], e))
    return worst, bad


def _step_report(what, eng, orc_d, orc_g, dgr, ggr):
    """{group: worst (max-rel, l2)} of D's / G's gradients (BatchNorm affine parameters apart) and of the weights after Adam"""
    d_errs, g_errs = _tensor_errs(eng.named_views("d", "grads"), dgr), _tensor_errs(eng.named_views("g", "grads"), ggr)
    groups = {"d": {k: v for k, v in d_errs.items() if not _bn(k)}, "d_bn": {k: v for k, v in d_errs.items() if _bn(k)}, "g": g_errs}
    if orc_d is not None:
        groups["d_state"], groups["g_state"] = _state_errs(eng.named_views("d"), orc_d), _state_errs(eng.named_views("g"), orc_g)
    rep = {gk: (max(e[0] for e in v.values()), max(e[1] for e in v.values())) for gk, v in groups.items()}
    print(what, {gk: (f"{a:.3e}", f"{b:.3e}") for gk, (a, b) in rep.items()})
    return rep, groups


def _check(rep, groups, bounds, what):
    bad = {}
    for gk, lim in bounds.items():
        for k, e in groups[gk].items():
            if e[0] > lim[0] or e[1] > lim[1]:
                bad[f"{gk}.{k}"] = (round(e[0], 5), round(e[1], 5), lim)
    assert not bad, f"{what}: {bad}"


# Bounds per batch, each 4x what was measured on an MI355X (printed by this file under `pytest -s`), as (max-rel,
# relative L2) for gradients and (max |difference| / lr, fraction of elements more than lr/4 apart) for the weights after Adam.
#   d    D's conv / Linear weight gradients: from identical weights; the 5e-3 relative L2 of the f32 path's tests
#   d_bn D's BatchNorm affine gradients: per-channel sums with heavy cancellation (the BatchNorm backward that follows removes
#        their mean), which amplifies the ~4e-6 relative error of every split-bf16 product - measured up to 6.4e-3 at batch 64
#   g    G's gradients come through the D that Adam has just stepped: an element of D whose gradient is within rounding of 0
#        moves the other way (2 lr), so they are looser than D's
#   *_state: at most one Adam flip per element (2 lr; 2.5 lr held), the fraction of flipped elements 4x the measurement
# Measured (max-rel, L2) / (max in lr, fraction):   d                 d_bn              g                 d_state        g_state
#   B = 8 (step 2)                                  8.6e-3, 2.0e-3    7.4e-3, 2.7e-3    1.7e-1, 1.6e-2    0.42, 7.6e-6   2.0, 3.9e-3
#   B = 64                                          2.2e-2, 4.7e-3    1.7e-2, 6.4e-3    5.7e-2, 3.9e-2    2.0, 2.3e-2    2.0, 2.3e-2
#   B = 256                                         1.4e-2, 3.2e-3    5.4e-3, 4.4e-3    3.3e-2, 3.4e-2    2.0, 1.6e-2    2.0, 1.1e-2
DCGAN_BOUNDS = {
    8: {"d": (1.0, 5e-3), "d_bn": (1.0, 1.1e-2), "g": (0.68, 6.4e-2), "d_state": (2.5, 3.1e-5), "g_state": (2.5, 1.6e-2)},
    64: {"d": (1.0, 5e-3), "d_bn": (1.0, 2.6e-2), "g": (0.23, 0.16), "d_state": (2.5, 9.4e-2), "g_state": (2.5, 9.4e-2)},
    256: {"d": (1.0, 5e-3), "d_bn": (1.0, 1.8e-2), "g": (0.14, 0.14), "d_state": (2.5, 6.3e-2), "g_state": (2.5, 4.4e-2)},
}


@pytest.mark.parametrize("B,steps", [(8, 2), (64, 1), (256, 1)])
def test_dcgan_step_parity(B, steps):
    """Teacher-forced steps against the oracle: every step scalar within 1e-3 (the north star's criterion), gradients and the
    post-Adam weights within DCGAN_BOUNDS.  At batch 256 every gradient tensor is also at least 3x inside the bf16 path's limits of
    tests/test_step_gpu.py::test_full_size_step_batch256 (relative L2 0.11 for D, 0.21 for G)."""
    orc, eng, out = _dcgan_run(B, steps, "bf16x3")
    worst, bad = 0.0, []
    for s, (ref, got, dgr, ggr) in enumerate(out):
        w, b = _scalars_ok(got, ref)
        worst, bad = max(worst, w), bad + [(s,) + x for x in b]
    print(f"dcgan B={B}: worst scalar {worst:.3e}")
    ref, got, dgr, ggr = out[-1]
    rep, groups = _step_report(f"dcgan B={B}", eng, orc.d, orc.g, dgr, ggr)
    assert not bad, bad
    _check(rep, groups, DCGAN_BOUNDS[B], f"dcgan B={B}")
    if B == 256:
        assert max(rep["d"][1], rep["d_bn"][1]) <= 0.11 / 3 and rep["g"][1] <= 0.21 / 3, rep


# measured relative L2: B = 8 (worst of two steps) d 4.0e-3, d_bn 3.9e-3, g 4.2e-2; B = 256 d 1.9e-3, d_bn 9.2e-4, g 2.9e-2
CGAN_BOUNDS = {8: {"d": (1.0, 5e-3), "d_bn": (1.0, 1.6e-2), "g": (1.0, 0.17)},
               256: {"d": (1.0, 5e-3), "d_bn": (1.0, 3.7e-3), "g": (1.0, 0.12)}}


@pytest.mark.parametrize("B,steps", [(8, 2), (256, 1)])
def test_cgan_step_parity(B, steps):
    """CGAN (back-propagated penalty) with 10-class labels, teacher-forced: scalars within 1e-3 per step, gradients within
    CGAN_BOUNDS (as DCGAN_BOUNDS; G's relative L2 4x the measurement)."""
    from hipgan.engine import CganEngine
    from oracle.gan_oracle import GanOracle
    from util import synth_images
    orc = GanOracle("cgan", lr=LR, seed=12345)
    eng = CganEngine(batch=B, prec="bf16x3")
    eng.load_state(orc.g, orc.d)
    imgs = synth_images(B * steps)
    g = torch.Generator().manual_seed(77)
    worst, bad, fails = 0.0, [], []
    for s in range(steps):
        lab = F.one_hot(torch.randint(0, 10, (B,), generator=g), 100).to(torch.int64)
        nz = CG._noise(B, 900 + s, lab)
        if s > 0:
            eng.load_state(orc.g, orc.d)
            for tag, opt in (("g", orc.opt_g), ("d", orc.opt_d)):
                for what, src in (("m", opt.m), ("v", opt.v)):
                    v = eng.named_views(tag, what)
                    for k, t in src.items():
                        v[k].copy_(t.view(v[k].shape))
            eng.t = orc.opt_d.t
        with CG._oracle_threads(CG.ORACLE_THREADS):
            ref = orc.step(imgs[s * B:(s + 1) * B], lab, nz)
        got = eng.step(imgs[s * B:(s + 1) * B].cuda(), {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in nz.items()}, lr=LR)
        w, b = _scalars_ok(got, ref)
        worst, bad = max(worst, w), bad + [(s,) + x for x in b]
        rep, groups = _step_report(f"cgan B={B} s{s}", eng, None, None, orc.d_grads, orc.g_grads)
        try:
            _check(rep, groups, CGAN_BOUNDS[B], f"cgan B={B} s{s}")
        except AssertionError as e:
            fails.append(str(e))
    print(f"cgan B={B}: worst scalar {worst:.3e}")
    assert not bad, bad
    assert not fails, "\n".join(fails)


def test_step_128():
    """The 128x128 topology at batch 16: one step against GanOracle(image_size=128), scalars within 1e-3."""
    import bf16_error as be
    from hipgan.engine import DcganEngine
    from oracle.gan_oracle import GanOracle
    from util import synth_images
    B = 16
    orc = GanOracle("dcgan", lr=LR, seed=12345, image_size=128)
    eng = DcganEngine(batch=B, prec="bf16x3", image_size=128)
    be._force_engine(eng, orc)
    real = F.interpolate(synth_images(B), size=128, mode="bilinear", align_corners=False)
    nz = be.noise_for("dcgan", B, 100, size=128)
    ref = orc.step(real, None, nz)
    got = eng.step(real.cuda(), {k: v.cuda() for k, v in nz.items()}, lr=LR)
    worst, bad = _scalars_ok(got, ref)
    print(f"dcgan 128 B={B}: worst scalar {worst:.3e}", {k: (got[k], ref[k]) for k in SCALARS})
    assert not bad, bad


def _eager_or_graph(family, B, graphs):
    from test_graph_gpu import _run
    return _run(family, "bf16x3", B, 3, graphs)


@pytest.mark.parametrize("family", ["dcgan", "cgan"])
def test_deterministic_and_graph_replay(family):
    """Two eager runs are bitwise equal, and the hipGraph replay is the eager step bit for bit."""
    s1, a1, _, _ = _eager_or_graph(family, 16, False)
    s2, a2, _, _ = _eager_or_graph(family, 16, False)
    s3, a3, n3, _ = _eager_or_graph(family, 16, True)
    assert n3 > 0 and s1 == s2 == s3
    for k in a1:
        assert torch.equal(a1[k], a2[k]) and torch.equal(a1[k], a3[k]), k


def test_per_pass_schedule(monkeypatch):
    """JCK_BATCHED=0 (separate real / fake passes): the first step's scalars of D's phase within 1e-5 of the batched schedule's.
    loss_g and D(G(z)) are evaluated by the D that Adam has just stepped, where an element whose gradient is within summation-order
    distance of 0 moves the other way (2 lr), and so is every later step: those are held to the north star's 1e-3."""
    s_b, _, _, _ = _eager_or_graph("dcgan", 16, False)
    monkeypatch.setenv("JCK_BATCHED", "0")
    s_p, _, _, _ = _eager_or_graph("dcgan", 16, False)
    err = {k: _rel(s_p[0][k], s_b[0][k]) for k in SCALARS}
    print("per-pass vs batched, step 0:", {k: f"{v:.2e}" for k, v in err.items()})
    for k, v in err.items():
        assert v < (1e-3 if k in ("loss_g", "d_gz2") else 1e-5), (k, v)


def test_modules_and_gradient_penalty():
    """Generator / Discriminator (train and eval mode), the CGAN modules and hipgan.functional.gradient_penalty with
    prec="bf16x3" against the CPU oracle: the forward within the f32 path's 2e-4, the penalty within 1e-3, gradients in relative L2
    within 4x the measurement."""
    from hipgan import functional as HF
    from model import CGAN, DCGAN
    from oracle import gan_oracle as go
    from test_modules_gpu import _inputs, _oracle_grads, _rel_l2
    from util import synth_images, synth_onehot
    torch.manual_seed(12345)
    z, x, rg, rd = _inputs(4)
    for fam, mod in (("dcgan", DCGAN), ("cgan", CGAN)):
        g, d = mod.Generator(), mod.Discriminator()
        g.apply(mod.weights_init)
        d.apply(mod.weights_init)
        oh, _ = synth_onehot(4, seed=5)
        kw = {"labels": oh, "mask": torch.full((4, 256), 0.75)} if fam == "cgan" else {}
        og, od, ox = _oracle_grads(fam, g.state_dict(), d.state_dict(), z, x, rg, rd, **kw)
        g, d = g.cuda(), d.cuda()
        g.prec = d.prec = "bf16x3"
        xg = x.cuda().requires_grad_(True)
        if fam == "cgan":
            fake = g(z.cuda(), oh.cuda())
            dout = HF.cgan_discriminator(d, xg, oh.cuda(), "bf16x3", mask=torch.full((4, 256), 0.75, device="cuda")).view(-1)
        else:
            fake, dout = g(z.cuda()), d(xg).view(-1)
        assert fake.dtype == torch.float32
        (fake * rg.cuda()).sum().backward()
        (dout * rd.cuda()).sum().backward()
        errs = {f"{fam}.g.{k}": _rel_l2(p.grad, og[k]) for k, p in g.named_parameters()}
        errs.update({f"{fam}.d.{k}": _rel_l2(p.grad, od[k]) for k, p in d.named_parameters()})
        errs[f"{fam}.x"] = _rel_l2(xg.grad, ox)
        print(f"{fam} modules: worst gradient rel-l2 {max(errs.values()):.3e}")
        # 4x the measurement (G's BatchNorm affine gradients at batch 4, 5.1e-3: sums with heavy cancellation, see DCGAN_BOUNDS)
        bad = {k: v for k, v in errs.items() if v > 2e-2}
        assert not bad, bad
        if fam == "dcgan":          # eval(): running statistics, against the same nn layers run by ATen on the CPU
            gc = copy.deepcopy(g).cpu().eval()
            g.eval()
            with torch.no_grad():
                e = g(z.cuda()).cpu()
                n, h = sum(1 for k, _ in gc.named_children() if k.startswith("norm")), z
                for i in range(1, n + 1):
                    h = getattr(gc, f"relu{i}")(getattr(gc, f"norm{i}")(getattr(gc, f"conv{i}")(h)))
                r = torch.tanh(getattr(gc, f"conv{n + 1}")(h))
            assert (e - r).abs().max().item() < 2e-4
    # the penalty as one differentiable Function (the engine's double backward) on the CGAN discriminator
    orc = go.GanOracle("cgan", lr=LR, seed=12345)
    d = CGAN.Discriminator().cuda()
    d.prec = "bf16x3"
    d.load_state_dict({k: v.clone() for k, v in orc.d.items()})
    gen = torch.Generator().manual_seed(5)
    B = 8
    real, fake = synth_images(B), torch.tanh(torch.randn(B, 3, 64, 64, generator=gen))
    labels = synth_onehot(B)[0]
    alpha, mask = torch.rand(B, 1, 1, 1, generator=gen), (torch.rand(B, 256, generator=gen) >= 0.25).float()
    dp = {k: v.clone().requires_grad_(go.is_param(k)) for k, v in orc.d.items()}
    ref = go.gradient_penalty(dp, real, fake, alpha, labels, mask)
    names = [k for k in dp if go.is_param(k)]
    ref_grads = dict(zip(names, torch.autograd.grad(ref, [dp[k] for k in names], allow_unused=True)))
    gp = HF.gradient_penalty(d, real.cuda(), fake.cuda(), labels=labels.cuda(), alpha=alpha.cuda(), drop_mask=mask.cuda())
    assert abs(gp.item() - ref.item()) <= 1e-3 * abs(ref.item()), (gp.item(), ref.item())
    (10.0 * gp).backward()
    for k, p in d.named_parameters():
        r = ref_grads[k]
        if r is None:
            continue
        l2 = ((p.grad.float().cpu() - 10.0 * r).norm() / (10.0 * r.norm() + 1e-30)).item()
        assert l2 < 5e-3, (k, l2)


def test_module_loop_with_engine_adam():
    """The reference's loop statements (tests/test_module_loop_gpu.py) on the HIP modules with prec="bf16x3" and EngineAdam: one
    step's losses within 1e-3 of the oracle, G's gradients within 0.12 relative L2 (4x the measurement: they come through the D that
    Adam has just stepped, see DCGAN_BOUNDS), the weights within one Adam flip."""
    from torch import nn
    from hipgan.engine import DcganEngine
    from hipgan.optim import EngineAdam
    from model import DCGAN
    from oracle.gan_oracle import GanOracle
    from test_module_loop_gpu import _noise
    from util import synth_images
    B = 8
    orc = GanOracle("dcgan", lr=LR, seed=12345)
    model_g, model_d = DCGAN.Generator().cuda(), DCGAN.Discriminator().cuda()
    model_g.prec = model_d.prec = "bf16x3"
    eng = DcganEngine(batch=B, prec="bf16x3")
    eng.adopt_modules(model_g, model_d)
    eng.load_state(orc.g, orc.d)
    opt_g = EngineAdam(eng, "g", model_g.named_parameters(), LR, betas=[0.5, 0.999])
    opt_d = EngineAdam(eng, "d", model_d.named_parameters(), LR, betas=[0.5, 0.999])
    criterion = nn.BCELoss()
    real_cpu, nz = synth_images(B), _noise(B, 300)
    ref = orc.step(real_cpu, None, nz)
    n1, z, n2, alpha = (nz[k].cuda() for k in ("n1", "z", "n2", "alpha"))
    model_d.zero_grad()
    real = 0.9 * real_cpu.cuda() + 0.1 * n1
    label = torch.full((B,), 0.9, dtype=torch.float, device="cuda")
    output = model_d(real).view(-1)
    error_real = criterion(output, label)
    error_real.backward()
    fake = 0.9 * model_g(z) + 0.1 * n2
    label.fill_(0.1)
    output = model_d(fake.detach()).view(-1)
    error_fake = criterion(output, label)
    error_fake.backward()
    inter = (alpha * real + (1 - alpha) * fake.detach()).requires_grad_(True)
    d_inter = model_d(inter)
    grads = torch.autograd.grad(outputs=d_inter, inputs=inter, grad_outputs=torch.ones_like(d_inter))[0]
    gp = ((grads.view(B, -1).norm(2, dim=1) - 1) ** 2).mean()
    error_d = error_real + error_fake + 10 * gp
    opt_d.step()
    model_g.zero_grad()
    label.fill_(0.9)
    error_g = criterion(model_d(fake).view(-1), label)
    error_g.backward()
    opt_g.step()
    for k, v in (("loss_d", error_d.item()), ("loss_g", error_g.item()), ("gp", gp.item()), ("loss_real", error_real.item()),
                 ("loss_fake", error_fake.item())):
        assert _rel(v, ref[k]) < 1e-3, (k, v, ref[k])
    l2 = {k: ((p.grad.float().cpu() - orc.g_grads[k]).norm() / (orc.g_grads[k].norm() + 1e-30)).item() for k, p in model_g.named_parameters()}
    print(f"module loop: worst G gradient rel-l2 {max(l2.values()):.3e}")
    assert max(l2.values()) < 0.12, l2
    for tag, mod, refp in (("g", model_g, orc.g), ("d", model_d, orc.d)):
        for k, p in mod.named_parameters():
            assert (p.detach().cpu() - refp[k]).abs().max().item() <= 2.5 * LR, (tag, k)


def test_trainer_through_the_environment(tmp_path, monkeypatch):
    """JCKGAN_PREC=bf16x3 selects the mode for the trainer, its modules and its engine: the first step of
    DCGANTrainer.train() against the fixture recorded from the reference's own trainer, within 1e-3."""
    from model import DCGAN
    from test_trainer_gpu import SynthPre, _fresh_logger
    from train.dcgan_trainer import DCGANTrainer
    from util import load_golden, rel, synth_images
    from hipgan._lib import PREC_BF16X3
    gold = load_golden("dcgan_steps")["B64"]
    B = gold["B"]
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("JCKGAN_PREC", "bf16x3")
    _fresh_logger()
    batches = [(synth_images(B * gold["steps"])[:B],)]
    args = argparse.Namespace(epoch=1, max_learning_rate=gold["lr"], model_path="golden", log_file=0,
                              save_path=str(tmp_path / "save" / "dcgan" / "golden"), batch_size=B, num_worker=0)
    torch.manual_seed(12345)
    tr = DCGANTrainer(args, DCGAN.Generator(), DCGAN.Discriminator(), SynthPre(batches), host_rng=True)
    assert tr.prec == "bf16x3" and tr.engine.prec == PREC_BF16X3
    losses_d, losses_g = tr.train()
    assert rel(losses_d[0], gold["losses_d"][0]) < 1e-3, (losses_d, gold["losses_d"])
    assert rel(losses_g[0], gold["losses_g"][0]) < 1e-3, (losses_g, gold["losses_g"])
    _fresh_logger()
