"""Adam and the weight repack as one launch per network (csrc/ew_optim.hpp adam_pack_kernel, JCK_ADAM_PACK): the launch must leave
parameters, moments, the moving average and every packed operand exactly as jck_adam followed by the repack leaves them - the same
adam_one per element and the same store per operand element, only from registers instead of a second read of the weights.

Op level: jck_adam_pack against jck_adam / jck_adam_ema + the per-op jck_pack_* entry points on a layer list with every job kind.
Step level: engines created with JCK_ADAM_PACK=1 and =0 run the same steps; arenas, operands and logged scalars bit for bit."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64


@pytest.fixture(scope="module")
def G():
    import gpu_util
    return gpu_util


# ---- op level -------------------------------------------------------------------------------------------------------------------------
# the arena: (name, numel, forms); a form = (job kind, a, b).  Every job kind and every padding case at its smallest size: a down / up
# pair (CsPad = 64, CbPad = 128), the 3 -> 64 layer (down with 4-channel padding + the 16-row up16 form), G.conv1 with Ci = 100 (ragged
# against the 16 x 16 tile, padded to 128), the head, BatchNorm vectors between them and one of 67 elements last: n % 4 = 3
ARENA = [("pair", 64 * 128 * 16, [(0, 64, 128), (1, 64, 128)]), ("bn0", 64, []),
         ("img", 64 * 3 * 16, [(0, 64, 3), (2, 64, 3)]), ("bn1", 128, []),
         ("g1", 100 * 64 * 16, [(3, 100, 64)]), ("head", 64 * 16, [(4, 64, 0)]), ("bn2", 67, [])]


def _operand_numel(lib, kind, a, b):
    if kind == 0:
        return lib.jck_pad_rows(a) * 16 * lib.jck_pad_chan(b)
    if kind == 1:
        return 4 * lib.jck_pad_rows(b) * 4 * a
    if kind == 2:
        return 16 * 9 * a
    if kind == 3:
        return 16 * b * 128
    return 16 * a


def _guarded(n, dtype, fill):
    t = torch.full((n + GUARD,), fill, dtype=dtype, device="cuda")
    t[n:] = 1.5
    return t


def _pack_plain(G, prec, kind, w, a, b, wp):
    st = G.cur_stream()
    if kind == 0:
        G.lib.jck_pack_down(prec, w, a, b, wp, st)
    elif kind in (1, 2):
        G.lib.jck_pack_up(prec, w, a, b, wp, st)
    elif kind == 3:
        G.lib.jck_pack_g1(prec, w, a, b, 128, wp, st)
    else:
        G.lib.jck_pack_head(w, a, wp, st)


@pytest.mark.parametrize("ema", [False, True])
@pytest.mark.parametrize("prec", [0, 1, 2])
def test_adam_pack_is_adam_then_the_repack(G, prec, ema):
    n = sum(x[1] for x in ARENA)
    assert n % 4 == 3
    gen = torch.Generator().manual_seed(31 + prec)
    src = {"p": torch.randn(n, generator=gen) * 0.05, "g": torch.randn(n, generator=gen) * 0.01, "m": torch.randn(n, generator=gen) * 0.01,
           "v": torch.rand(n, generator=gen) * 1e-4, "e": torch.randn(n, generator=gen) * 0.05}

    def arenas():
        out = {}
        for k, t in src.items():
            out[k] = _guarded(n, torch.float32, 0.0)
            out[k][:n] = t.cuda()
        return out

    jobs, off = [], 0
    for _, numel, forms in ARENA:
        jobs += [(kind, off, a, b) for kind, a, b in forms]
        off += numel
    dt = lambda kind: torch.float32 if (kind == 4 or prec != 0) else torch.bfloat16
    hyper = (2e-4, 0.5, 0.999, 1e-8, 3, 0.5)                   # lr, betas, eps, step, grad_scale
    ema_w = 0.25

    def fused(skip, fill):
        a = arenas()
        wps = [_guarded(_operand_numel(G.lib, k, x, y), dt(k), fill) for k, _, x, y in jobs]
        nj = len(jobs)
        G.lib.jck_adam_pack(prec, a["p"], a["g"], a["m"], a["v"], a["e"] if ema else None, n, nj, (C.c_int * nj)(*[j[0] for j in jobs]),
                            (C.c_longlong * nj)(*[j[1] for j in jobs]), (C.c_void_p * nj)(*[w.data_ptr() for w in wps]),
                            (C.c_int * nj)(*[j[2] for j in jobs]), (C.c_int * nj)(*[j[3] for j in jobs]), *hyper, ema_w, skip, G.cur_stream())
        torch.cuda.synchronize()
        return a, wps

    # the two launches on copies; the per-op pack kernels write the padding zeros themselves (over a 7.0 fill)
    ref = arenas()
    if ema:
        G.lib.jck_adam_ema(ref["p"], ref["g"], ref["m"], ref["v"], ref["e"], n, *hyper, ema_w, None, G.cur_stream())
    else:
        G.lib.jck_adam(ref["p"], ref["g"], ref["m"], ref["v"], n, *hyper, G.cur_stream())
    ref_wps = []
    for kind, o, a, b in jobs:
        wp = _guarded(_operand_numel(G.lib, kind, a, b), dt(kind), 7.0)
        _pack_plain(G, prec, kind, ref["p"][o:o + 16 * a * max(b, 1)], a, b, wp)
        ref_wps.append(wp)
    torch.cuda.synchronize()

    got, wps = fused(None, 0.0)
    assert not torch.equal(got["p"][:n], src["p"].cuda())
    for k in "pgmve":
        assert torch.equal(got[k], ref[k]), k                  # guard elements included; g and (without ema) e unchanged
    for j, w, r in zip(jobs, wps, ref_wps):
        assert torch.equal(w.view(torch.int16 if w.dtype == torch.bfloat16 else torch.int32),
                           r.view(torch.int16 if r.dtype == torch.bfloat16 else torch.int32)), j

    # the error word set: nothing moves, the operands (3.0 everywhere) included
    word = torch.ones(1, dtype=torch.int32, device="cuda")
    got, wps = fused(word, 3.0)
    for k in "pgmve":
        assert torch.equal(got[k][:n], src[k].cuda()) and bool((got[k][n:] == 1.5).all()), k
    for j, w in zip(jobs, wps):
        assert bool((w[:-GUARD].float() == 3.0).all()) and bool((w[-GUARD:].float() == 1.5).all()), j


# ---- step level -----------------------------------------------------------------------------------------------------------------------
def _operand_names(eng):
    ns = 5 if eng.size == 128 else 4
    names = [f"{p}{i}" for i in range(ns) for p in ("d_down", "d_up", "g_up", "g_down")] + ["g1_w"]
    return names + (["d_head_wp"] if eng.family == 0 else ["l1_w", "l1_wT"])


def _steps(monkeypatch, fused, family="dcgan", B=8, prec="bf16", size=64, ema=False, lr_g=None, graphs=False, reducers=False, env=(), steps=2):
    """`steps` training steps from the same state and seed -> per step (scalars, arenas, operands)"""
    import bf16_error as be
    from hipgan.engine import CganEngine, DcganEngine
    from oracle.gan_oracle import build_params
    from util import synth_images
    monkeypatch.setenv("JCK_ADAM_PACK", "1" if fused else "0")
    for k, v in env:
        monkeypatch.setenv(k, v)
    torch.manual_seed(12345)
    g, d = build_params(family) if size == 64 else build_params(family, size)
    kw = {"image_size": 128} if size == 128 else {}
    if ema:
        kw.update(ema_decay=0.9, ema_start=2)                  # step 1: the average tracks the weights (weight 1); step 2: 1 - decay
    eng = (CganEngine if family == "cgan" else DcganEngine)(batch=B, prec=prec, **kw)
    eng.graphs = graphs
    eng.load_state(g, d)
    eng.set_noise_seed(4242)
    imgs = synth_images(B * steps)
    if size == 128:
        imgs = torch.nn.functional.interpolate(imgs, size=128, mode="bilinear", align_corners=False)
    red = (lambda flat, **k: (lambda: None)) if reducers else None
    out = []
    for s in range(steps):
        lab = be.labels_for(B, 5 + s) if family == "cgan" else None
        nz = be.noise_for(family, B, 40 + s, lab, size=size)
        nz = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in nz.items()}
        eng.step_async(imgs[s * B:(s + 1) * B].cuda().contiguous(), nz, 2e-4, reduce_d=red, reduce_g=red, **({"lr_g": lr_g} if lr_g else {}))
        sc = eng.scalars()
        torch.cuda.synchronize()
        out.append((sc, {k: v.clone() for k, v in eng.arenas.items()}, {k: eng.tensor(k).clone() for k in _operand_names(eng)}))
    if graphs:
        assert len(eng._graph_cache) > 0
    return out


def _same(a, b):
    assert len(a) == len(b)
    for s, ((s0, a0, o0), (s1, a1, o1)) in enumerate(zip(a, b)):
        assert len(s0) == 8 and s0 == s1, (s, s0, s1)
        for k in a0:
            assert torch.equal(a0[k], a1[k]), (s, k)
        for k in o0:
            x, y = o0[k], o1[k]
            it = torch.int16 if x.dtype == torch.bfloat16 else torch.int32
            assert torch.equal(x.view(it), y.view(it)), (s, k)


# batch 24: three groups of 8, ragged against the GEMM tile sizes
@pytest.mark.parametrize("B,prec", [(8, "bf16"), (24, "bf16"), (8, "f32"), (24, "f32")])
def test_step_is_bit_identical_with_and_without_the_fused_launch(monkeypatch, B, prec):
    fused = _steps(monkeypatch, True, B=B, prec=prec)
    assert not torch.equal(fused[0][1]["g_params"], fused[1][1]["g_params"])
    _same(fused, _steps(monkeypatch, False, B=B, prec=prec))


@pytest.mark.parametrize("what", ["ema", "lr_g", "graph"])
def test_step_variants_are_bit_identical(monkeypatch, what):
    """the moving average inside G's launch (weight 1, then 1 - decay), G's own learning rate (only the Adam scalars are rewritten), and
    the fused launch replayed from a captured graph against the eager two-launch step"""
    if what == "ema":
        a, b = _steps(monkeypatch, True, ema=True), _steps(monkeypatch, False, ema=True)
        assert "g_ema" in a[0][1] and not torch.equal(a[1][1]["g_ema"], a[1][1]["g_params"])
    elif what == "lr_g":
        a, b = _steps(monkeypatch, True, lr_g=5e-4), _steps(monkeypatch, False, lr_g=5e-4)
    else:
        a, b = _steps(monkeypatch, True, graphs=True, steps=3), _steps(monkeypatch, False, steps=3)
    _same(a, b)


@pytest.mark.parametrize("family", ["dcgan", "cgan"])
def test_two_range_optimiser_phase_packs_what_each_range_updates(monkeypatch, family):
    """PHASE_D_STEP behind a lazy join runs Adam over [behind conv1.weight, end) first and [.., conv1.weight] once the weight-gradient
    stream is through: DCGAN with one-rank reducers (D's arena reduced in two pieces under its own backward), CGAN's plain eager step.
    Against the unsplit call (no reducers / JCK_LAZY_JOIN=0) and against the two-launch form of the same split."""
    if family == "dcgan":
        split = dict(reducers=True, env=(("JCK_DDP_SPLIT", "1"),))
        whole = dict(reducers=False)
    else:
        split = dict(env=(("JCK_LAZY_JOIN", "1"),))
        whole = dict(env=(("JCK_LAZY_JOIN", "0"),))
    a = _steps(monkeypatch, True, family=family, steps=1, **split)
    _same(a, _steps(monkeypatch, True, family=family, steps=1, **whole))
    _same(a, _steps(monkeypatch, False, family=family, steps=1, **split))


@pytest.mark.parametrize("family,size", [("cgan", 64), ("dcgan", 128)])
def test_cgan_and_the_sixth_stage_are_bit_identical(monkeypatch, family, size):
    """CGAN: the label embedding and the Linear layers go through the flat ranges, the Linear repack stays a launch of its own;
    128 x 128: one more conv stage in both networks"""
    _same(_steps(monkeypatch, True, family=family, size=size, steps=1), _steps(monkeypatch, False, family=family, size=size, steps=1))
