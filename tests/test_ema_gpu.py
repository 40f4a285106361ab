"""Exponential moving average of the generator's weights: fused into Adam(G)'s launch (csrc/ew_optim.hpp adam_kernel<true>), sampled
through an engine bound to the average, checkpointed by the trainers.  The reference has no average and neither has the
oracle, so every numeric case carries the recurrence itself, in float64:

    e <- e + w * (p_k - e)        p_k: the fp32 weights read back after step k, w = float32(1 - decay) promoted to double

Tolerance after k averaging steps, per element: 4 * k * 2^-24 * M with M the largest |p| (and |e_0|) seen.  One update rounds
at most: the difference (|.| <= 2M, so <= 2M * 2^-24 - but it is then scaled by w or 1 - w), the product, 1 - w on the second
lerp branch, and the result (<= M * 2^-24).  That is <= 2 * 2^-24 * M on the first branch (w < 0.5) and <= 3.4 * 2^-24 * M on
the second with w = 0.6; the error obeys err <- (1 - w) * err + delta, so it grows at most linearly in k.  No measured number."""
import argparse
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24


def _w(decay):
    return float(torch.tensor(1.0 - decay, dtype=torch.float64).to(torch.float32))


def _check_recurrence(got, e_ref, k, M, what=""):
    err = (got.double().cpu() - e_ref).abs().max().item()
    tol = 4 * k * EPS * M
    print(f"{what}: k={k} M={M:.4g} max err {err:.4g} tol {tol:.4g}")
    assert err <= tol, (what, k, err, tol)


# ---- 1. the per-op form ------------------------------------------------------------------------------------------------
def _op_inputs(n, off, seed=7):
    """p, g, m, v, ema as views `off` floats into their allocations (off = 1: no pointer is 16-byte aligned)."""
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen) * 0.05
    t = {"p": p, "g": torch.randn(n, generator=gen) * 0.01, "m": torch.randn(n, generator=gen) * 0.01,
         "v": torch.rand(n, generator=gen) * 1e-4, "ema": torch.roll(p, 1)}        # |e_0| <= max |p_0|
    out = {}
    for k, x in t.items():
        buf = torch.zeros(n + off + 8, device="cuda")
        buf[off:off + n].copy_(x)
        out[k] = buf[off:off + n]
        assert (out[k].data_ptr() % 16 == 0) == (off == 0)
    return out


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("decay", [0.999, 0.4])
def test_adam_ema_op_against_the_recurrence(off, decay):
    """n = 4099: vector body + 3-element tail (off = 0) / the element-by-element path (off = 1); two consecutive steps;
    decay 0.999 takes lerp's first branch, 0.4 the second.  p, m, v bitwise as jck_adam leaves them."""
    from hipgan import lib
    from hipgan._lib import cur_stream
    n = 4099
    a, b = _op_inputs(n, off), _op_inputs(n, off)
    w = _w(decay)
    e_ref = a["ema"].double().cpu()
    M = max(a["p"].abs().max().item(), a["ema"].abs().max().item())
    for step in (1, 2):
        lib.jck_adam_ema(a["p"], a["g"], a["m"], a["v"], a["ema"], n, 2e-4, 0.5, 0.999, 1e-8, step, 0.5, w, None, cur_stream())
        lib.jck_adam(b["p"], b["g"], b["m"], b["v"], n, 2e-4, 0.5, 0.999, 1e-8, step, 0.5, cur_stream())
        for k in ("p", "m", "v"):
            assert torch.equal(a[k], b[k]), (k, step)
        p = a["p"].double().cpu()
        M = max(M, p.abs().max().item())
        e_ref = e_ref + w * (p - e_ref)
        _check_recurrence(a["ema"], e_ref, step, M, f"op off={off} decay={decay}")


@pytest.mark.parametrize("off", [0, 1])
def test_adam_ema_op_past_the_grid_cap(off):
    """One step whose launch passes the cap of 8192 workgroups of 256 threads: n = 8192 * 256 + 5 element by element (off = 1),
    n = 4 * 8192 * 256 + 7 on the vector path (off = 0: one quad of the second sweep and the 3-element tail).  decay 0.4; the
    average against the recurrence, p, m, v bitwise as jck_adam leaves them."""
    from hipgan import lib
    from hipgan._lib import cur_stream
    n = 8192 * 256 + 5 if off else 4 * 8192 * 256 + 7
    a, b = _op_inputs(n, off), _op_inputs(n, off)
    w = _w(0.4)
    e0 = a["ema"].double().cpu()
    M = max(a["p"].abs().max().item(), a["ema"].abs().max().item())
    lib.jck_adam_ema(a["p"], a["g"], a["m"], a["v"], a["ema"], n, 2e-4, 0.5, 0.999, 1e-8, 1, 0.5, w, None, cur_stream())
    lib.jck_adam(b["p"], b["g"], b["m"], b["v"], n, 2e-4, 0.5, 0.999, 1e-8, 1, 0.5, cur_stream())
    for k in ("p", "m", "v"):
        assert torch.equal(a[k], b[k]), k
    p = a["p"].double().cpu()
    _check_recurrence(a["ema"], e0 + w * (p - e0), 1, max(M, p.abs().max().item()), f"op past the grid cap off={off}")


@pytest.mark.parametrize("off", [0, 1])
def test_adam_ema_op_weight_one_and_skip(off):
    from hipgan import lib
    from hipgan._lib import cur_stream
    n = 4099
    a = _op_inputs(n, off)
    lib.jck_adam_ema(a["p"], a["g"], a["m"], a["v"], a["ema"], n, 2e-4, 0.5, 0.999, 1e-8, 1, 1.0, 1.0, None, cur_stream())
    assert torch.equal(a["ema"], a["p"])                          # w = 1: the average IS the new parameter
    before = {k: v.clone() for k, v in a.items()}
    flag = torch.ones(1, dtype=torch.int32, device="cuda")
    lib.jck_adam_ema(a["p"], a["g"], a["m"], a["v"], a["ema"], n, 2e-4, 0.5, 0.999, 1e-8, 2, 1.0, 0.25, flag, cur_stream())
    for k in a:
        assert torch.equal(a[k], before[k]), k                    # skip_if -> 1: nothing moves
    flag.zero_()
    lib.jck_adam_ema(a["p"], a["g"], a["m"], a["v"], a["ema"], n, 2e-4, 0.5, 0.999, 1e-8, 2, 1.0, 0.25, flag, cur_stream())
    assert not torch.equal(a["p"], before["p"]) and not torch.equal(a["ema"], before["ema"])


# ---- engines -------------------------------------------------------------------------------------------------------------
def _engine(family, B, prec, state=None, **kw):
    from hipgan.engine import CganEngine, DcganEngine
    from oracle.gan_oracle import build_params
    if state is None:
        torch.manual_seed(12345)
        state = build_params(family, kw.get("image_size", 64))
    eng = (CganEngine if family == "cgan" else DcganEngine)(batch=B, prec=prec, **kw)
    eng.load_state(*state)
    eng.set_noise_seed(4242)
    return eng


def _step(eng, family, s, imgs=None, lr=2e-4):
    """one step with the engine's own draws (as the trainers and bench.py run), batch s of the synthetic images."""
    import bf16_error as be
    from util import synth_images
    B = eng.batch
    imgs = synth_images(64) if imgs is None else imgs
    lab = be.labels_for(B, 5 + s).cuda() if family == "cgan" else None
    eng.step_async(imgs[(s * 8) % 56:(s * 8) % 56 + B].cuda().contiguous(), None, lr, labels=lab)


@pytest.fixture(autouse=True)
def _no_env_ema(monkeypatch):
    monkeypatch.delenv("JCKGAN_EMA_DECAY", raising=False)


@pytest.mark.parametrize("family,prec", [("dcgan", "f32"), ("dcgan", "bf16"), ("cgan", "bf16")])
def test_ema_does_not_perturb_training(family, prec):
    runs = []
    for decay in (None, 0.999):
        eng = _engine(family, 8, prec, ema_decay=decay)
        sc = []
        for s in range(3):
            _step(eng, family, s)
            sc.append(eng.scalars())
        torch.cuda.synchronize()
        runs.append((sc, {k: v.clone() for k, v in eng.arenas.items()}))
    (s0, a0), (s1, a1) = runs
    assert "g_ema" not in a0 and "g_ema" in a1
    assert s0 == s1, (s0, s1)                                      # the eight step scalars of every step
    assert len(a0) == 12
    for k in a0:                                                  # parameters, gradients, moments, BN buffers of both networks
        assert torch.equal(a0[k], a1[k]), k
    assert not torch.equal(a1["g_ema"], a1["g_params"])


def _run_recurrence(engines, family, steps, decay, start):
    """engines: the engine that takes step s (1-based) is engines[(s - 1) % len(engines)]; all share one state."""
    a = engines[0].arenas
    w = _w(decay)
    e_ref, k, M = None, 0, 0.0
    for s in range(1, steps + 1):
        eng = engines[(s - 1) % len(engines)]
        _step(eng, family, s)
        eng.join()
        torch.cuda.synchronize()
        p = a["g_params"].double().cpu()
        if s < start:
            assert torch.equal(a["g_ema"], a["g_params"]), s          # warm-up: the average IS the weights
            e_ref, M = p, p.abs().max().item()
        else:
            k += 1
            M = max(M, p.abs().max().item())
            e_ref = e_ref + w * (p - e_ref)
            _check_recurrence(a["g_ema"], e_ref, k, M, f"step {s}")
            assert not torch.equal(a["g_ema"], a["g_params"])


@pytest.mark.parametrize("family,prec", [("dcgan", "bf16"), ("dcgan", "f32"), ("cgan", "bf16")])
def test_recurrence_in_the_step(family, prec):
    eng = _engine(family, 8, prec, ema_decay=0.9, ema_start=3)
    _run_recurrence([eng], family, 4, 0.9, 3)


def test_recurrence_with_a_shared_ragged_engine():
    """batch 8 and a share= engine at batch 6 (the per-pass schedule) take alternate steps: ONE average advanced by both."""
    from hipgan.engine import DcganEngine
    eng = _engine("dcgan", 8, "bf16", ema_decay=0.9, ema_start=3)
    tail = DcganEngine(batch=6, share=eng)
    tail.set_noise_seed(4242)
    assert tail.ema_decay == 0.9 and tail.ema_start == 3 and tail.arenas is eng.arenas
    _run_recurrence([eng, tail], "dcgan", 4, 0.9, 3)


def test_recurrence_on_the_128_topology():
    from util import synth_images
    eng = _engine("dcgan", 8, "bf16", ema_decay=0.9, image_size=128)
    a = eng.arenas
    assert torch.equal(a["g_ema"], a["g_params"]) and a["g_ema"].abs().max().item() > 0       # load_state: average = parameters
    e0 = a["g_ema"].double().cpu()
    imgs = torch.nn.functional.interpolate(synth_images(8), size=128, mode="bilinear", align_corners=False)
    eng.step_async(imgs.cuda().contiguous(), None, 2e-4)
    eng.join()
    torch.cuda.synchronize()
    p = a["g_params"].double().cpu()
    _check_recurrence(a["g_ema"], e0 + _w(0.9) * (p - e0), 1, max(p.abs().max().item(), e0.abs().max().item()), "128")


# ---- 4. / 5. launch count and graph replay -----------------------------------------------------------------------------
def test_no_new_launch(monkeypatch):
    """The step captured as one graph (all five phases) has as many nodes - kernel launches and memsets - with the average
    as without: PHASE_G_STEP issues the same single Adam launch either way."""
    from hipgan import lib
    monkeypatch.setenv("JCK_GRAPH", "1")
    nodes = []
    for decay in (None, 0.999):
        eng = _engine("dcgan", 8, "bf16", ema_decay=decay)
        assert eng.graphs
        for s in range(2):                                        # the first step of an engine is eager, the second is captured
            _step(eng, "dcgan", s)
        torch.cuda.synchronize()
        assert len(eng._graph_cache) == 1
        nodes.append(lib.jck_engine_graph_nodes(eng._h))
    assert nodes[0] == nodes[1] and nodes[0] > 20, nodes


@pytest.mark.parametrize("start", [2, 4])
def test_graph_replay_advances_the_same_average(start, monkeypatch):
    """One eager step and four replayed ones.  start = 2: every replayed step averages; start = 4: both graphs (one per step
    parity) are CAPTURED at weight 1 and replayed at 1 - decay - a weight baked into the graph would show."""
    runs = []
    for graphs in ("0", "1"):
        monkeypatch.setenv("JCK_GRAPH", graphs)
        eng = _engine("dcgan", 8, "bf16", ema_decay=0.999, ema_start=start)
        for s in range(5):
            _step(eng, "dcgan", s)
        eng.join()
        torch.cuda.synchronize()
        assert len(eng._graph_cache) == (2 if graphs == "1" else 0)
        runs.append({k: v.clone() for k, v in eng.arenas.items()})
    assert torch.equal(runs[0]["g_params"], runs[1]["g_params"])
    assert torch.equal(runs[0]["g_ema"], runs[1]["g_ema"])
    assert not torch.equal(runs[1]["g_ema"], runs[1]["g_params"])


# ---- 6. module path ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", [0, 5])
def test_engine_adam_step_advances_the_average_as_the_engine_does(start):
    """EngineAdam.step() (jck_adam_ema) from the state and gradients of an engine step = PHASE_G_STEP's result, bit for bit.
    (The learning rate is a power of two: the engine's step takes it as a float, the optimiser as a double.)"""
    from hipgan.optim import EngineAdam
    lr = 2.0 ** -12
    a_eng = _engine("dcgan", 8, "bf16", ema_decay=0.9, ema_start=start)
    b_eng = _engine("dcgan", 8, "bf16", ema_decay=0.9, ema_start=start)
    _step(a_eng, "dcgan", 0, lr=lr)                               # so that moments and average are no longer trivial
    a_eng.join()
    torch.cuda.synchronize()
    pre = {k: a_eng.arenas[k].clone() for k in ("g_params", "g_m", "g_v", "g_ema")}
    _step(a_eng, "dcgan", 1, lr=lr)
    a_eng.join()
    torch.cuda.synchronize()
    for k, v in pre.items():
        b_eng.arenas[k].copy_(v)
    b_eng.arenas["g_grads"].copy_(a_eng.arenas["g_grads"])        # G's gradients of step 2 (cleared by the NEXT step's D phase)
    b_eng.t = 1
    opt = EngineAdam(b_eng, "g", [], lr, betas=[0.5, 0.999])    # no module parameters to gather: the arena is the state
    opt.step()
    torch.cuda.synchronize()
    for k in ("g_params", "g_m", "g_v", "g_ema"):
        assert torch.equal(a_eng.arenas[k], b_eng.arenas[k]), k
    assert torch.equal(b_eng.arenas["g_ema"], b_eng.arenas["g_params"]) == (start == 5)


# ---- 7. sampling -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,prec", [("dcgan", "f32"), ("dcgan", "bf16"), ("cgan", "bf16")])
def test_sampling_engine(family, prec):
    import bf16_error as be
    from hipgan import JckError
    from hipgan.engine import CganEngine, DcganEngine
    from util import synth_images
    cls = CganEngine if family == "cgan" else DcganEngine
    eng = _engine(family, 8, prec, ema_decay=0.9)
    for s in range(2):
        _step(eng, family, s)
    eng.join()
    z = torch.randn(8, 100, 1, 1, generator=torch.Generator().manual_seed(3)).cuda()
    lab = be.labels_for(8, 11).cuda() if family == "cgan" else None
    smp = cls(batch=8, share=eng, ema=True)
    live = {k: eng.arenas[k].clone() for k in ("g_bn", "g_nbt", "g_params")}
    s1 = smp.sample(z, lab).clone()
    torch.cuda.synchronize()
    for k, v in live.items():                                    # running_mean / running_var / num_batches_tracked of the live G
        assert torch.equal(eng.arenas[k], v), k
    ema_sd = eng.ema_state_dict()
    g_sd, d_sd = eng.state_dicts()
    assert list(ema_sd.keys()) == list(g_sd.keys()) and all(ema_sd[k].shape == g_sd[k].shape for k in g_sd)
    assert int(ema_sd["norm1.num_batches_tracked"]) == int(g_sd["norm1.num_batches_tracked"]) + 1      # the sampler's own buffers moved
    plain = cls(batch=8, prec=prec)
    plain.load_state(ema_sd, d_sd)
    assert torch.equal(plain.sample(z, lab), s1)
    assert not torch.equal(eng.sample(z, lab), s1)               # the live generator is another one
    _step(eng, family, 2)
    s2 = smp.sample(z, lab)
    assert not torch.equal(s2, s1)                               # the sampler re-derived its operands from the moved average
    plain.load_state(eng.ema_state_dict(), d_sd)
    assert torch.equal(plain.sample(z, lab), s2)
    with pytest.raises(JckError):
        smp.step_async(synth_images(8).cuda(), None, 2e-4, labels=lab)
    with pytest.raises(JckError):
        cls(batch=8, share=plain, ema=True)                      # no average to sample


# ---- 8. trainers -----------------------------------------------------------------------------------------------------------
class SynthPre:
    idx_to_labels = {i: str(i) for i in range(100)}

    def __init__(self, batches):
        self.batches = batches

    def get_data_loader(self):
        return self.batches, None


def _fresh_logger():
    import logging
    from logger.main_logger import MainLogger
    logging.getLogger("main").handlers.clear()
    MainLogger._instance, MainLogger._initialized = None, False


def _train(tmp_path, name, family="dcgan", **flags):
    """batches of 8, 8, 5 (ragged tail engine); evaluations at iteration 0 and at the last one -> (trainer, checkpoint path)."""
    from util import synth_images, synth_onehot
    _fresh_logger()
    imgs, (oh, _) = synth_images(21), synth_onehot(21)
    cuts = [(0, 8), (8, 16), (16, 21)]
    batches = [((imgs[a:b],) if family == "dcgan" else (imgs[a:b], oh[a:b])) for a, b in cuts]
    args = argparse.Namespace(epoch=1, max_learning_rate=2e-4, model_path=name, log_file=0,
                              save_path=str(tmp_path / "save" / family / name), batch_size=8, num_worker=0, **flags)
    torch.manual_seed(12345)
    if family == "dcgan":
        from model import DCGAN
        from train.dcgan_trainer import DCGANTrainer
        tr = DCGANTrainer(args, DCGAN.Generator(), DCGAN.Discriminator(), SynthPre(batches))
    else:
        from model import CGAN
        from train.cgan_trainer import CGANTrainer
        tr = CGANTrainer(args, CGAN.Generator(), CGAN.Discriminator(), SynthPre(batches))
    return tr, args


def _checkpoint(tmp_path, family, name):
    root = tmp_path / "save" / family / name / "latest"
    pts = [f for f in os.listdir(root) if f.endswith(".pt")]
    assert len(pts) == 1 and pts[0].startswith("2_"), pts          # the evaluation of the last iteration
    return str(root / pts[0])


FOUR = ["model_d", "model_g", "optimizer_d", "optimizer_g"]


def test_dcgan_trainer_checkpoints_and_resumes_the_average(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    tr, _ = _train(tmp_path, "ema", ema_decay=0.999)
    tr.train()
    assert sorted(tr._tail_engines) == [5] and sorted(tr._ema_samplers) == [64]
    path = _checkpoint(tmp_path, "dcgan", "ema")
    ck = torch.load(path, weights_only=False)
    assert sorted(ck.keys()) == sorted(FOUR + ["model_g_ema"])
    assert list(ck["model_g_ema"].keys()) == list(ck["model_g"].keys())
    assert all(ck["model_g_ema"][k].shape == v.shape for k, v in ck["model_g"].items())
    assert not torch.equal(ck["model_g_ema"]["conv3.weight"], ck["model_g"]["conv3.weight"])
    # evaluation sampled the average: the live generator's BatchNorm counters saw the three steps only; the sampling engine's
    # were seeded from the live ones at its creation (after step 1) and moved with its two samplings
    assert int(ck["model_g"]["norm1.num_batches_tracked"]) == 3 and int(ck["model_g_ema"]["norm1.num_batches_tracked"]) == 1 + 2
    # resume
    tr2, _ = _train(tmp_path, "ema2", ema_decay=0.999)
    tr2.load_model(path)
    torch.cuda.synchronize()
    views = tr2.engine.named_views("g", "ema")
    for k, v in ck["model_g_ema"].items():
        assert torch.equal(views[k].cpu(), v), k
    assert torch.equal(tr2.engine.arenas["g_params"].cpu(), tr.engine.arenas["g_params"].cpu())
    assert not torch.equal(tr2.engine.arenas["g_ema"], tr2.engine.arenas["g_params"])
    # a checkpoint written without the flag: the average starts at its weights
    four = str(tmp_path / "four.pt")
    torch.save({k: ck[k] for k in FOUR}, four)
    tr2.load_model(four)
    torch.cuda.synchronize()
    assert torch.equal(tr2.engine.arenas["g_ema"], tr2.engine.arenas["g_params"])
    _fresh_logger()


def test_dcgan_trainer_without_the_flag_is_the_reference_checkpoint(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    tr, _ = _train(tmp_path, "plain")
    tr.train()
    ck = torch.load(_checkpoint(tmp_path, "dcgan", "plain"), weights_only=False)
    assert sorted(ck.keys()) == FOUR
    assert not any("ema" in k for k in tr.engine.arenas) and tr.engine.ema_decay is None and not tr._ema_samplers
    assert int(ck["model_g"]["norm1.num_batches_tracked"]) == 3 + 2          # the reference samples the live generator
    _fresh_logger()


def test_cgan_trainer_writes_the_average(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    tr, _ = _train(tmp_path, "ema", family="cgan", ema_decay=0.999)
    tr.train()
    ck = torch.load(_checkpoint(tmp_path, "cgan", "ema"), weights_only=False)
    assert sorted(ck.keys()) == sorted(FOUR + ["model_g_ema"])
    assert list(ck["model_g_ema"].keys()) == list(ck["model_g"].keys())
    assert not torch.equal(ck["model_g_ema"]["conv3.weight"], ck["model_g"]["conv3.weight"])
    _fresh_logger()


def test_main_declares_the_flags():
    import main
    a = main.get_arg_parse(["-m", "DCGAN"])
    assert not hasattr(a, "ema_decay") and not hasattr(a, "ema_start")        # the reference's namespace unless given
    a = main.get_arg_parse(["-m", "DCGAN", "--ema_decay", "0.999", "--ema_start", "100"])
    assert a.ema_decay == 0.999 and a.ema_start == 100


def test_environment_default(monkeypatch):
    """JCKGAN_EMA_DECAY is the constructor's default, as JCKGAN_PREC is the trainers': an unmodified bench.py times the feature."""
    from hipgan.engine import DcganEngine
    monkeypatch.setenv("JCKGAN_EMA_DECAY", "0.999")
    assert DcganEngine(batch=8).ema_decay == 0.999
    assert DcganEngine(batch=8, ema_decay=0).ema_decay is None
    monkeypatch.setenv("JCKGAN_EMA_DECAY", "0")
    eng = DcganEngine(batch=8)
    assert eng.ema_decay is None and "g_ema" not in eng.arenas


# ---- 9. replica guard (host logic) ---------------------------------------------------------------------------------------
def test_replica_guard_broadcasts_the_average(monkeypatch):
    import torch.distributed as dist
    from hipgan.dist import ReplicaGuard
    sent = []
    monkeypatch.setattr(dist, "broadcast", lambda t, src=0, group=None: sent.append(t.data_ptr()))
    for decay, expect in ((0.999, True), (None, False)):
        eng = _engine("dcgan", 8, "bf16", ema_decay=decay)
        guard = ReplicaGuard(eng, world=2)
        monkeypatch.setattr(guard, "in_sync", lambda: False)
        del sent[:]
        assert guard.check() is False
        assert (eng.arenas.get("g_ema") is not None and eng.arenas["g_ema"].data_ptr() in sent) == expect
        assert eng.arenas["g_params"].data_ptr() in sent and len(sent) == (9 if expect else 8)
