"""The DCGAN gradient penalty back-propagated on the GPU (opt-in: DcganEngine(gp_backward=True), jck_engine_create_ex with
JCK_ENGINE_GP_BACKWARD, `main.py --gp_backward 1`; the closed form is checked in fp64 in tests/test_dcgan_gp_math.py):
the head-step kernel against float64 torch, the module path's penalty against the oracle's autograd double backward, the opt-in
step against a teacher-forced oracle whose D descends on error_real + error_fake + 10 * gp, its schedules, and that default
engines are untouched.

Tolerances as tests/test_step_gpu.py: f32 / bf16x3 scalars 1e-3, D's gradients 5e-3 relative L2 per tensor (3e-2 max-norm), G's
as there (f32 5e-3; bf16x3 the 6.4e-2 of tests/test_bf16x3_gpu.py); bf16 against the fp32 oracle (oracle/bf16_emu.py's DCGAN
restatement is not twice differentiable) within about 4x the error measured on the MI355X, noted beside each bound."""
import argparse
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

PREC = {"bf16": 0, "f32": 1, "bf16x3": 2}
SCAL = ("loss_d", "loss_g", "gp", "loss_real", "loss_fake", "d_x", "d_gz1", "d_gz2")
SENT = -3.25


def _l2(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


# ---- 1. the head-step kernel ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [0, 1, 2])
@pytest.mark.parametrize("C", [512, 1024])
@pytest.mark.parametrize("B", [1, 7, 64, 256])
def test_gp_head2_conv_against_float64(prec, C, B):
    """rs = <v4, w5>(1-2p)p(1-p), g_a4 = rs w5 (storage type), conv5.weight's gradient += sum_n p(1-p) v4 + rs a4 in PyTorch layout,
    against float64 torch built from the operands as stored.  Outputs start as NaN (the gradient from non-zero values: it
    accumulates), what lies behind them holds a sentinel; the in-place form (g_a4 over v4) gives the same bits."""
    from hipgan import lib
    from hipgan._lib import cur_stream
    K = 16 * C
    dt = torch.bfloat16 if prec == 0 else torch.float32
    g = torch.Generator().manual_seed(7000 + 13 * B + C + prec)
    v4 = (torch.randn(B, K, generator=g) * 0.05).to(dt)
    a4 = torch.nn.functional.leaky_relu(torch.randn(B, K, generator=g), 0.2).to(dt)
    wp = torch.randn(K, generator=g) * 0.02
    prob = torch.rand(B, generator=g) * 0.9 + 0.05
    grad0 = torch.randn(16 * C, generator=g) * 0.1
    v, a, w, p = v4.double(), a4.double(), wp.double(), prob.double()
    sn = p * (1 - p)
    rs_r = (v @ w) * (1 - 2 * p) * sn
    ga_r = rs_r[:, None] * w[None, :]
    dw_r = (sn[:, None] * v + rs_r[:, None] * a).sum(0).view(16, C).t().reshape(-1)     # packed k = t*C + c -> [c][t]
    rs = torch.full((B + 8,), float("nan"), device="cuda")
    rs[B:] = SENT
    ga = torch.full((B + 1, K), float("nan"), dtype=dt, device="cuda")
    ga[B:] = SENT
    grad = torch.cat([grad0, torch.full((8,), SENT)]).cuda()
    ws = torch.full((lib.jck_gp_head2_conv_ws_floats(B),), float("nan"), device="cuda")
    v4d, a4d = v4.cuda(), a4.cuda()
    lib.jck_gp_head2_conv(prec, v4d, a4d, wp.cuda(), prob.cuda(), B, C, rs, ga, grad, ws, cur_stream())
    # in place: g_a4 written over v4
    vin, grad2, rs2 = v4d.clone(), grad0.cuda(), torch.empty(B, device="cuda")
    lib.jck_gp_head2_conv(prec, vin, a4d, wp.cuda(), prob.cuda(), B, C, rs2, vin, grad2, ws, cur_stream())
    torch.cuda.synchronize()
    rs, ga, grad = rs.cpu(), ga.float().cpu(), grad.cpu()
    assert bool((rs[B:] == SENT).all()) and bool((ga[B:] == SENT).all()) and bool((grad[16 * C:] == SENT).all()), "wrote past the end"
    assert bool(torch.isfinite(rs[:B]).all()) and bool(torch.isfinite(ga[:B]).all()) and bool(torch.isfinite(grad[:16 * C]).all())
    err = lambda x, r: ((x.double() - r).abs().max() / (r.abs().max() + 1e-30)).item()
    assert err(rs[:B], rs_r) < 2e-5, err(rs[:B], rs_r)
    assert err(ga[:B], ga_r) < (8e-3 if prec == 0 else 2e-5), err(ga[:B], ga_r)
    assert err(grad[:16 * C] - grad0, dw_r) < 2e-5, err(grad[:16 * C] - grad0, dw_r)
    assert torch.equal(rs2.cpu(), rs[:B]) and torch.equal(grad2.cpu(), grad[:16 * C]) and torch.equal(vin.float().cpu(), ga[:B])


# ---- 2. the module path ---------------------------------------------------------------------------------------------------
# Relative L2 per tensor against the fp64 double backward.  f32: 5e-3 (measured <= 1.4e-5).  bf16x3 at 64: 5e-3 (measured 9.5e-4).
# bf16x3 at 128 and bf16: about 4x the maximum measured on the MI355X (noted).  What sets them is LeakyReLU's kink, not the penalty's
# arithmetic: a pre-activation within rounding distance of 0 takes the other branch, which moves a handful of gradient elements by
# 0.8 g - in these 8-image cases a per-tensor error of ~1e-2 from one flip; the first-order gradient of the same module path shows
# the same (bf16x3: 1.5e-2 at 64, 6.4e-3 at 128, measured alongside).
MOD_LIM = {(64, "f32"): 5e-3, (128, "f32"): 5e-3, (64, "bf16x3"): 5e-3,
           (128, "bf16x3"): 5.6e-2,      # 1.39e-2 (norm2.bias)
           (64, "bf16"): 0.45,           # 0.108 (norm1.bias)
           (128, "bf16"): 0.55}          # 0.137 (conv1.weight)


def _module_case(size, prec, B=8):
    from model import DCGAN
    from oracle import gan_oracle as go
    torch.manual_seed(12345)
    _, dstate = go.build_params("dcgan", size)
    d = DCGAN.Discriminator(image_size=size).cuda()
    d.prec = prec
    d.load_state_dict({k: v.clone() for k, v in dstate.items()})
    g = torch.Generator().manual_seed(5)
    real = torch.rand(B, 3, size, size, generator=g) * 2 - 1
    fake = torch.tanh(torch.randn(B, 3, size, size, generator=g))
    alpha = torch.rand(B, 1, 1, 1, generator=g)
    return go, dstate, d, real, fake, alpha


@pytest.mark.parametrize("size", [64, 128])
@pytest.mark.parametrize("prec", ["f32", "bf16x3", "bf16"])
def test_module_penalty_is_back_propagated(size, prec):
    """HF.gradient_penalty(DCGAN.Discriminator) + (10 * gp).backward() - the WGAN-GP loop that raised JckError before: the value
    against the fp32 oracle (1e-3), every parameter's gradient against the fp64 autograd double backward."""
    from hipgan import functional as HF
    go, dstate, d, real, fake, alpha = _module_case(size, prec)
    ref32 = go.gradient_penalty({k: v.clone() for k, v in dstate.items()}, real, fake, alpha)
    dp = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in dstate.items()}
    for k in dp:
        if go.is_param(k):
            dp[k].requires_grad_(True)
    ref = go.gradient_penalty(dp, real.double(), fake.double(), alpha.double())
    names = [k for k in dp if go.is_param(k)]
    ref_grads = dict(zip(names, torch.autograd.grad(10.0 * ref, [dp[k] for k in names])))
    gp = HF.gradient_penalty(d, real.cuda(), fake.cuda(), alpha=alpha.cuda())
    print(f"module penalty {size} {prec}: value {gp.item():.6g} vs {ref32.item():.6g}")
    vtol = 1e-3 if prec != "bf16" else 6.5e-2          # bf16: 3.8e-3 measured at 64, 1.6e-2 at 128
    assert abs(gp.item() - ref32.item()) <= vtol * abs(ref32.item()), (gp.item(), ref32.item())
    (10.0 * gp).backward()
    worst = max(_l2(p.grad, ref_grads[k]) for k, p in d.named_parameters())
    print(f"module penalty {size} {prec}: worst rel-L2 {worst:.3e}")
    lim = MOD_LIM[(size, prec)]
    for k, p in d.named_parameters():
        assert _l2(p.grad, ref_grads[k]) < lim, (k, _l2(p.grad, ref_grads[k]))


def test_value_only_call_is_todays_pass():
    """Without gradients (no_grad, or no parameter requiring grad) the call is the value-only pass of a default engine: the same
    value bit for bit, no parameter gradient, the gradient engine's arena untouched, and backward raises."""
    from hipgan import JckError, functional as HF
    from hipgan.engine import DcganEngine
    go, dstate, d, real, fake, alpha = _module_case(64, "f32")
    r, f, al = real.cuda(), fake.cuda(), alpha.cuda()
    gp_back = HF.gradient_penalty(d, r, f, alpha=al)                 # creates (and caches) the gradient engine
    back_eng = [e for k, e in d._jck_gp_engines.items() if k[-1]][0]
    torch.cuda.synchronize()
    arena = back_eng.arenas["d_grads"].clone()
    with torch.no_grad():
        gp_nograd = HF.gradient_penalty(d, r, f, alpha=al)
    plain = DcganEngine(batch=8, prec="f32")
    with torch.no_grad():
        gp_plain = HF.gradient_penalty(d, r, f, alpha=al, engine=plain)
    torch.cuda.synchronize()
    assert gp_nograd.item() == gp_plain.item() == gp_back.item(), (gp_nograd.item(), gp_plain.item(), gp_back.item())
    assert torch.equal(back_eng.arenas["d_grads"], arena)
    assert all(p.grad is None for p in d.parameters())
    gp_plain2 = HF.gradient_penalty(d, r, f, alpha=al, engine=plain)   # formed on a default engine: no gradient path
    with pytest.raises(JckError):
        gp_plain2.backward()


# ---- 3. the step ----------------------------------------------------------------------------------------------------------
def _gp_oracle(lr=2e-4, seed=12345):
    from oracle import gan_oracle as go

    class GpOracle(go.GanOracle):
        """The oracle's DCGAN step with the penalty back-propagated: D descends on grad(e_real + e_fake + 10 gp), the penalty's
        fake detached (its path to G is discarded by the reference's model_g.zero_grad())."""

        def phase_d(self, real, labels=None, noise=None):
            nz = noise
            self._req(self.dp_params)
            self._req(self.gp_params)
            dnames = list(self.dp_params)
            real = go.NOISE_KEEP * real + go.NOISE_MIX * nz["n1"]
            out_real = go.discriminator(self.d, real).view(-1)
            e_real = go.bce(out_real, go.LABEL_REAL)
            fake = go.NOISE_KEEP * go.generator(self.g, nz["z"]) + go.NOISE_MIX * nz["n2"]
            out_fake = go.discriminator(self.d, fake.detach()).view(-1)
            e_fake = go.bce(out_fake, go.LABEL_FAKE)
            gp = go.gradient_penalty(self.d, real.detach(), fake.detach(), nz["alpha"])
            dg = torch.autograd.grad(e_real + e_fake + go.LAMBDA_GP * gp, [self.dp_params[k] for k in dnames])
            gp = gp.detach()
            self.d_grads = dict(zip(dnames, dg))
            return {"d_grads": self.d_grads, "fake": fake, "labels": None, "m4": None,
                    "loss_d": float((e_real + e_fake).detach() + go.LAMBDA_GP * gp), "gp": float(gp),
                    "loss_real": float(e_real.detach()), "loss_fake": float(e_fake.detach()),
                    "out_real": out_real.detach(), "out_fake": out_fake.detach(), "real_noisy": real.detach()}
    return GpOracle("dcgan", lr=lr, seed=seed)


def _noise(B, seed):
    g = torch.Generator().manual_seed(seed)
    return {"n1": torch.randn(B, 3, 64, 64, generator=g), "z": torch.randn(B, 100, 1, 1, generator=g),
            "n2": torch.randn(B, 3, 64, 64, generator=g), "alpha": torch.rand(B, 1, 1, 1, generator=g)}


def _step_vs_oracle(B, prec):
    """One step from identical state: -> (engine scalars, oracle scalars, engine, oracle D grads, oracle G grads).  The oracle's G
    phase runs on the ENGINE's post-Adam D weights: a first Adam step moves every weight by lr * sign(g), so the few dozen D weights
    whose gradient is within rounding of 0 move the other way, and G's gradient through them differs by up to 3 % whichever engine
    runs (measured on these cases: default engine 2.9 % at B = 24) - that is Adam's, not the penalty's."""
    from hipgan.engine import DcganEngine
    from util import synth_images
    orc = _gp_oracle()
    eng = DcganEngine(batch=B, prec=prec, gp_backward=True)
    eng.load_state(orc.g, orc.d)
    real, nz = synth_images(B), _noise(B, 100)
    got = eng.step(real.cuda(), {k: v.cuda() for k, v in nz.items()}, lr=2e-4)
    ctx = orc.phase_d(real, None, nz)
    orc.apply_d(ctx["d_grads"])
    with torch.no_grad():
        for k, v in eng.named_views("d").items():
            if k in orc.dp_params:
                orc.dp_params[k].copy_(v.float().cpu().view_as(orc.dp_params[k]))
    orc.phase_g(ctx)
    orc.apply_g(ctx["g_grads"])
    return got, orc.finish(ctx), eng, orc.d_grads, orc.g_grads


def _check_step(got, ref, eng, dgr, ggr, what, dlim=5e-3, glim=5e-3, slim=1e-3, dmax=3e-2):
    for k in SCAL:
        assert abs(got[k] - ref[k]) <= slim * max(abs(ref[k]), 1e-12), (what, k, got[k], ref[k])
    for tag, refs, lim in (("d", dgr, dlim), ("g", ggr, glim)):
        views = eng.named_views(tag, "grads")
        for k, r in refs.items():
            g = views[k].detach().float().cpu().view(r.shape)
            assert _l2(g, r) < lim, (what, tag, k, _l2(g, r))
            if tag == "d" and dmax is not None:
                assert (g - r).abs().max().item() <= dmax * (r.abs().max().item() + 1e-30), (what, k)


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
@pytest.mark.parametrize("B", [8, 24, 64, 106, 256])
def test_step_parity_with_the_penalty_back_propagated(B, prec):
    """B = 8, 24 (batched, not a power of two), 64, 256: the batched 3B schedule; 106: the per-pass schedule, penalty pass on its
    own stream, joined and back-propagated by PHASE_D_GP."""
    got, ref, eng, dgr, ggr = _step_vs_oracle(B, prec)
    # G's gradients of bf16x3 at tests/test_bf16x3_gpu.py's tightest bound (6.4e-2; its G phase stores the fake batch's gradient
    # chain in fp32 but takes LeakyReLU / ReLU branches from split-bf16 GEMM outputs); measured here <= 1.4e-2
    _check_step(got, ref, eng, dgr, ggr, (B, prec), glim=5e-3 if prec == "f32" else 6.4e-2)


# bf16 at B = 256 against the fp32 gradient oracle (measured on the MI355X beside each bound; about 4x that)
STEP_BF16 = {"scalars": 2.5e-2,       # 8.9e-4 (gp)
             "d": 0.3,                # 8.0e-2
             "g": 0.6}                # 0.16


def test_step_bf16_batch256():
    got, ref, eng, dgr, ggr = _step_vs_oracle(256, "bf16")
    worst = {t: max(_l2(eng.named_views(t, "grads")[k].float().cpu().view(r.shape), r) for k, r in refs.items())
             for t, refs in (("d", dgr), ("g", ggr))}
    print(f"bf16 B=256 step: worst rel-L2 {worst}, scalars " + ", ".join(f"{k} {abs(got[k] - ref[k]) / abs(ref[k]):.2e}" for k in SCAL))
    _check_step(got, ref, eng, dgr, ggr, "bf16", STEP_BF16["d"], STEP_BF16["g"], STEP_BF16["scalars"], None)


@pytest.mark.parametrize("env", [{"JCK_BATCHED": "0"}, {"JCK_OVERLAP": "0"}])
def test_alternative_schedules(env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got, ref, eng, dgr, ggr = _step_vs_oracle(16, "f32")
    _check_step(got, ref, eng, dgr, ggr, env, glim=2e-2)


def _run(B, prec, steps, graphs=False, gp_backward=True, reduce=None):
    import bf16_error as be
    from hipgan.engine import DcganEngine
    from oracle.gan_oracle import build_params
    from util import synth_images
    torch.manual_seed(12345)
    g, d = build_params("dcgan")
    eng = DcganEngine(batch=B, prec=prec, gp_backward=gp_backward)
    eng.graphs = graphs
    eng.load_state(g, d)
    imgs = synth_images(B * steps)
    sc = []
    for s in range(steps):
        nz = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in be.noise_for("dcgan", B, 40 + s, None).items()}
        eng.step_async(imgs[s * B:(s + 1) * B].cuda(), nz, 2e-4 * (1 + s), reduce_d=reduce)
        sc.append(eng.scalars())
    torch.cuda.synchronize()
    return sc, {k: v.clone() for k, v in eng.arenas.items()}, eng


@pytest.mark.parametrize("prec,B", [("bf16", 16), ("f32", 4)])
def test_graph_replay_and_reruns_are_bit_for_bit(prec, B):
    """Graph replay (B = 16 batched, B = 4 per-pass) is the eager step bit for bit, and two eager runs are identical."""
    s_e, a_e, _ = _run(B, prec, 4)
    s_g, a_g, eng = _run(B, prec, 4, graphs=True)
    s_2, a_2, _ = _run(B, prec, 4)
    assert len(eng._graph_cache) == 2
    assert s_e == s_g == s_2
    for k in a_e:
        assert torch.equal(a_e[k], a_g[k]) and torch.equal(a_e[k], a_2[k]), k


def test_default_engines_are_untouched():
    """No flag: the workspace is today's (create_sized == create_ex(flags=0)); the flag adds the second-order buffers to DCGAN
    engines only; CGAN ignores it; an unknown flag is refused."""
    import ctypes as C
    from hipgan._lib import load_library
    dll = load_library()

    def ws(fn, *a):
        h = C.c_void_p()
        assert fn(C.byref(h), *a) == 0, dll.jck_last_error()
        n = dll.jck_engine_workspace_bytes(h)
        dll.jck_engine_destroy(h)
        return n
    for fam, size in ((0, 64), (0, 128), (1, 64)):
        base = ws(dll.jck_engine_create_sized, fam, 0, 64, size)
        assert ws(dll.jck_engine_create_ex, fam, 0, 64, size, 0) == base
        flagged = ws(dll.jck_engine_create_ex, fam, 0, 64, size, 1)
        assert (flagged > base) if fam == 0 else (flagged == base), (fam, size, base, flagged)
    h = C.c_void_p()
    assert dll.jck_engine_create_ex(C.byref(h), 0, 0, 64, 64, 2) != 0


def test_reducer_sees_the_penalty_in_ds_arena():
    """Data parallel: reduce_d is handed D's arena with the penalty term already in it - the pre-Adam gradient of the same step run
    without a reducer - and the engine offers no early tail split."""
    from hipgan._lib import lib
    seen = []
    _, _, eng = _run(16, "f32", 1, reduce=lambda flat: seen.append(flat.clone()) or None)
    assert len(seen) == 1 and lib.jck_engine_grad_tail(eng._h, 1) == -1
    _, a_plain, _ = _run(16, "f32", 1)
    _, a_nogp, _ = _run(16, "f32", 1, gp_backward=False)
    assert torch.equal(seen[0], a_plain["d_grads"])
    assert _l2(seen[0], a_nogp["d_grads"]) > 1e-2


# ---- 4. trainer -----------------------------------------------------------------------------------------------------------
class _Pre:
    def __init__(self, batches):
        self.batches = batches

    def get_data_loader(self):
        return self.batches, None


def _trainer(tmp_path, name, gpb, B=16, steps=3):
    import logging
    from logger.main_logger import MainLogger
    from model import DCGAN
    from train.dcgan_trainer import DCGANTrainer
    from util import synth_images
    logging.getLogger("main").handlers.clear()
    MainLogger._instance, MainLogger._initialized = None, False
    imgs = synth_images(B * steps)
    args = argparse.Namespace(epoch=1, max_learning_rate=2e-4, model_path=name, log_file=0, batch_size=B, num_worker=0,
                              save_path=str(tmp_path / "save" / "dcgan" / name), gp_backward=gpb)
    torch.manual_seed(12345)
    return DCGANTrainer(args, DCGAN.Generator(), DCGAN.Discriminator(), _Pre([(imgs[i * B:(i + 1) * B],) for i in range(steps)]),
                        prec="f32", host_rng=True)


def test_trainer_gp_backward(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    runs = {}
    for gpb in (0, 1):
        tr = _trainer(tmp_path, f"gpb{gpb}", gpb)
        assert tr.engine.gp_backward == bool(gpb)
        tr.train()
        torch.cuda.synchronize()
        runs[gpb] = (tr, {k: v.detach().cpu().clone() for k, v in tr.model_d.state_dict().items()})
    d0, d1 = runs[0][1], runs[1][1]
    assert _l2(d1["conv1.weight"], d0["conv1.weight"]) > 1e-4
    pts = {gpb: sorted(str(p) for p in (tmp_path / "save" / "dcgan" / f"gpb{gpb}").rglob("*.pt")) for gpb in (0, 1)}
    assert pts[0] and pts[1]
    runs[0][0].load_model(pts[1][0])            # the checkpoint format is the same either way
    runs[1][0].load_model(pts[0][0])
    for k, v in runs[0][0].model_d.state_dict().items():
        assert torch.equal(v.cpu(), torch.load(pts[1][0], weights_only=False)["model_d"][k].cpu()), k
