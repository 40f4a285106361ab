"""The step engine's results do not depend on what its workspace held.

jck_engine_bind takes caller memory and clears all of it (include/jckgan.h); the kernels rely on those zeros wherever they write only
part of a buffer.  hipgan/engine.py allocates the workspace with torch.zeros, so every other test runs on memory where a read before
the first write returns 0.0 anyway.  Here the workspace is filled with a byte pattern and bound again (DcganEngine._bind, the
constructor's own call - binding again is ordinary use of the ABI), and the engine is held, bit for bit, to a twin that never saw the
pattern:
  part 1  poison BEFORE bind: three steps (hp2, scal2, acc2 and the rz / ralpha / rmask draws alternate on step parity, so step 2 meets
          step 0's leftovers) and the inference calls - guards bind's contract;
  part 3  poison of the twelve activation tensors jck_engine_tensor names AFTER step k: step k + 1 must not read step k's data in any
          of them ("every step rewrites before reading", csrc/engine_infer.hip) - which bind's zeros can no longer show.
Two bytes: 0xFF (bf16 0xFFFF and fp32 0xFFFFFFFF are NaNs, integers -1: survives arithmetic, swallowed by comparisons and masks) and
0x3F (bf16 0x3F3F = 0.74609375, fp32 0x3F3F3F3F ~ 0.747: finite, passes every comparison, shows a wrong finite sum).  No tolerance
anywhere: raw bits, torch.equal.  The twin's scalars must be finite (two identical NaN runs do not pass), and one case compares two
clean engines the same way - the project's run-to-run determinism (no float atomics, tests/test_bf16_envelope.py) is what makes a
difference attributable to the pattern.

Regions of the workspace (jck_engine::carve, csrc/engine_internal.hpp) whose contents are used as anything other than floating-point
data - an index, a count, an address, a barrier word - read off the code before the poisoned engine ran for the first time.  A pattern
in such a region could fault or hang a device instead of failing a test, so each has to be written or cleared before its first read
whatever the workspace held:

  region   what it holds                                              written / cleared before its first read by
  gsync    the grid barrier of the resident BatchNorm backward        jck_engine_bind's clear of the workspace (csrc/engine.hip), before any
           (csrc/bnres.hpp): arrival counters (words 0..8 * 32), the  launch; the counters are reset by their last arriver and the generation is
           generation word, the error word that every Adam launch     monotonic, so no launch needs another clear; jck_engine_check re-arms it
           reads (jck_grid_sync_error_word) and jck_engine_check       after a timeout.  Every spin on it is bounded by a clock (0.3 s).
  hp2      [2 parities][8]: words 4..7 are the Philox key and the      adam_hp_kernel (csrc/ew_optim.hpp), launched by set_step_impl: by
           step (uint32) that the image kernels and the draws read    jck_engine_set_step, or by the first phase of a step whose parity slot
           through jck_engine::rng(); words 0..2 Adam's scalars       does not hold that step (phase_begin: hp_step[q] != step).  Bind and
           (floats)                                                   jck_engine_set_noise_seed reset hp_step, so the first phase after either
                                                                      writes the slot before any kernel of the step reads it.
Nothing else: the barrier counters of the gather-GEMMs (csrc/igemm.hpp) live in LDS; BatchNorm's statistic slot counts, the split-K
factors and the tile plans are host integers; labels, dataset indices, flips and crop origins are the caller's tensors; the
num_batches_tracked counters live in the arenas.  Every other region - packed operands, activations, gradients, statistic rows, aux
tables, BatchNorm records (d_rs), accumulator rows (acc2), scalars (scal2), the draws (rz, ralpha, rmask), split-K slabs (wg_ws, g1_ws,
l1_slab, head_ws, gp2_ws), the head rows and the second-order buffers - is bf16 / fp32 data that only ever enters arithmetic,
comparisons with constants (ReLU / LeakyReLU masks) or stores.  Nothing is poisoned after bind except the twelve tensors of part 3,
all of that kind.

Part 3 keeps all twelve tensors: on the plain step() path none of them carries state from one step into the next.
"""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

B = 8                   # the smallest batch at which the batched schedule exists (batch % 8 == 0, csrc/engine.hip)
STEPS = 3
POISONS = [0xFF, 0x3F]
# jck_engine_tensor's names of plain floating-point activations; `acc` (cleared by promise for the coming step) and the packed
# operands (state) are left out
STEP_SCRATCH = ("fake", "fake_raw", "real_noisy", "xhat", "d_gx", "prob", "ds", "norms", "d_y1", "d_a4", "g_y1", "g_a4")


@functools.lru_cache(maxsize=None)
def _params(family, size=64):
    from oracle.gan_oracle import build_params
    torch.manual_seed(12345)
    return build_params(family, size) if size != 64 else build_params(family)


@functools.lru_cache(maxsize=None)
def _images(n, size=64):
    from util import synth_images
    x = synth_images(n)
    return x if size == 64 else torch.nn.functional.interpolate(x, size=size, mode="bilinear", align_corners=False)


def _bits(t):
    """a device or host tensor as raw bits on the host"""
    t = t.detach().contiguous()
    if t.dtype == torch.float32:
        t = t.view(torch.int32)
    elif t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return t.cpu().clone()


def _poison(eng, byte):
    """fills the engine's workspace with `byte` and binds it again, as the constructor bound it; the constructor's noise seed again"""
    eng.join()
    torch.cuda.synchronize()
    eng.workspace.fill_(byte)
    torch.cuda.synchronize()
    eng._bind()
    eng.set_noise_seed(int(torch.initial_seed()) + 0x6a636b67)


def _engine(family, poison, **kw):
    from hipgan.engine import CganEngine, DcganEngine
    eng = (CganEngine if family == "cgan" else DcganEngine)(**kw)
    if poison is not None:
        _poison(eng, poison)
    return eng


def _step(eng, family, s, caller_noise, graph=False, batch=B, first=0):
    """step s of a run (images [first, first + batch) of the run's set) -> the eight scalars as bits, after the host has seen them finite or not"""
    import bf16_error as be
    size = eng.size
    real = _images(B * STEPS, size)[first:first + batch].cuda()
    lab = be.labels_for(batch, 5 + s).cuda() if family == "cgan" else None
    if caller_noise:
        nz = be.noise_for(family, batch, 40 + s, lab, size)
        eng.step_async(real, {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in nz.items()}, 2e-4, graph=graph)
    else:
        eng.step_async(real, None, 2e-4, labels=lab, graph=graph)
    eng.scalars()                                   # joins, synchronises, raises on a barrier time-out
    return _bits(eng.scalars_view())


def _state(eng, out):
    torch.cuda.synchronize()
    for k, v in eng.arenas.items():
        out[f"arena.{k}"] = _bits(v)
    out["fake"] = _bits(eng.tensor("fake"))


def _inference(eng, family, out, tag="infer"):
    """sample (train-mode and eval-mode BatchNorm, n = 3 < B), score, features, one latent_grad with a critic and a feature target"""
    import bf16_error as be
    n = 3
    g = torch.Generator().manual_seed(7)
    z = torch.randn(n, 100, generator=g).cuda()
    x, ft = _images(B * STEPS)[:n].cuda(), _images(B * STEPS)[n:2 * n].cuda()
    lab = be.labels_for(n, 3).cuda() if family == "cgan" else None
    out[f"{tag}.sample_batch"] = _bits(eng.sample(z, lab, bn="batch"))
    out[f"{tag}.sample_running"] = _bits(eng.sample(z, lab, bn="running"))
    logit, prob = eng.score(x, lab)
    out[f"{tag}.score_logit"], out[f"{tag}.score_prob"] = _bits(logit), _bits(prob)
    out[f"{tag}.features"] = _bits(eng.features(x))
    r = eng.latent_grad(z, x, lab, critic="nsgan", critic_weight=0.1, feature_target=ft, feature_weight=1.0)
    for k in ("loss", "term", "logit", "fterm", "dz"):
        out[f"{tag}.latent_{k}"] = _bits(r[k])


def _run(family, poison, prec="bf16", caller_noise=False, size=64, graph=False, infer=False, **ekw):
    """Three steps from the oracle's initial weights on a fresh engine (poisoned and bound again, or not) -> {name: bits} in the order
    things are produced: the scalars of every step, then every arena and tensor("fake"), then (infer) the inference calls."""
    torch.manual_seed(12345)
    eng = _engine(family, poison, batch=B, prec=prec, image_size=size, **ekw)
    eng.load_state(*_params(family, size))
    out = {}
    for s in range(STEPS):
        out[f"scalars.{s}"] = _step(eng, family, s, caller_noise, graph=graph and s >= 1, first=s * B)
    _state(eng, out)
    if infer:
        _inference(eng, family, out)
    return out


@functools.lru_cache(maxsize=1)
def _clean(family, env, **kw_items):
    """the clean twin of a configuration, run once for both poison bytes, which follow each other (env: the switches in force, part of
    the key only)"""
    return _run(family, None, **kw_items)


def _finite(out):
    for k, v in out.items():
        if k.startswith("scalars."):
            assert bool(torch.isfinite(v.view(torch.float32)).all()), f"the clean twin's {k} are not finite: {v.view(torch.float32).tolist()}"


def _same(got, ref, what):
    """every quantity of the two runs, in order; the first that differs is named"""
    assert list(got) == list(ref), (list(got), list(ref))
    for k in ref:
        if not torch.equal(got[k], ref[k]):
            a, b = got[k].reshape(-1), ref[k].reshape(-1)
            i = int(torch.nonzero(a != b)[0])
            ndiff = int((a != b).sum())
            show = (lambda t: t.view(torch.float32) if t.dtype == torch.int32 else t.view(torch.bfloat16) if t.dtype == torch.int16 else t)
            raise AssertionError(f"{what}: first differing quantity {k}: {ndiff}/{a.numel()} elements, first at {i}: "
                                 f"{show(a)[i].item()} vs the clean twin's {show(b)[i].item()}")


def _twins(family, poison, monkeypatch=None, env=None, **kw):
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    ref = _clean(family, tuple(sorted((env or {}).items())), **kw)
    _finite(ref)
    _same(_run(family, poison, **kw), ref, f"{family} {kw} {env or ''} poison {poison:#x}")


# ---- part 1: poison before bind ------------------------------------------------------------------------------------------------------
def test_two_clean_engines_agree_bit_for_bit():
    """The control: what the poisoned cases compare - scalars of three steps, every arena, the last fake batch, the inference calls -
    is reproducible between two untouched engines."""
    ref = _run("dcgan", None, infer=True)
    _finite(ref)
    _same(_run("dcgan", None, infer=True), ref, "clean vs clean")


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("kw", [dict(prec="bf16"),                                   # the engine draws z: g_z's padding columns
                                dict(prec="bf16", caller_noise=True),                # n1, z, n2, alpha from the caller
                                dict(prec="f32"), dict(prec="bf16x3"),
                                dict(prec="bf16", gp_backward=True),                 # the second-order buffers d_v, d_xdir, bn2_ws*, d_u0
                                dict(prec="bf16", size=128),
                                dict(prec="bf16", graph=True)],                      # captured from the second step on: memset nodes for the promises
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_dcgan_steps_do_not_see_the_poison(kw, poison):
    _twins("dcgan", poison, **kw)


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("switch", ["JCK_BATCHED", "JCK_OVERLAP", "JCK_BN_RES", "JCK_ADAM_PACK", "JCK_FOLD_ZERO", "JCK_FUSE_TANH"])
def test_dcgan_alternative_schedules_do_not_see_the_poison(switch, poison, monkeypatch):
    """each switch changes which launch first writes some buffer (read when the engine is created)"""
    _twins("dcgan", poison, monkeypatch, {switch: "0"}, prec="bf16")


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("kw,env", [(dict(prec="bf16"), {}), (dict(prec="f32"), {}),       # engine-drawn masks (labels=)
                                    (dict(prec="bf16", caller_noise=True), {}),           # the caller's m1..m4
                                    (dict(prec="bf16"), {"JCK_CBUF_DIRECT": "0"}), (dict(prec="bf16"), {"JCK_HEAD_FUSE": "0"})],
                         ids=["bf16", "f32", "bf16-caller-masks", "bf16-cbuf-copy", "bf16-head-unfused"])
def test_cgan_steps_do_not_see_the_poison(kw, env, poison, monkeypatch):
    """cbuf's padding columns [8392, 8448) and cbuf2's [8192, 8448) - 200 of which are the label-embedding columns of the penalty's
    second-order product: finite garbage there is a wrong finite linear1 gradient, not a NaN"""
    _twins("cgan", poison, monkeypatch, env, **kw)


def _ragged(poison):
    """two steps on a batch-8 engine, one on a batch-5 engine bound to the same arenas (its own workspace: the per-pass schedule)"""
    from hipgan.engine import DcganEngine
    torch.manual_seed(12345)
    eng = _engine("dcgan", poison, batch=B, prec="bf16")
    tail = DcganEngine(batch=5, share=eng)
    if poison is not None:
        _poison(tail, poison)
    eng.load_state(*_params("dcgan"))
    out = {}
    for s in range(2):
        out[f"scalars.{s}"] = _step(eng, "dcgan", s, False, first=s * B)
    out["scalars.2"] = _step(tail, "dcgan", 2, False, batch=5, first=2 * B)
    _state(eng, out)
    out["tail.fake"] = _bits(tail.tensor("fake"))
    return out


@pytest.mark.parametrize("poison", POISONS)
def test_ragged_batch_on_shared_arenas_does_not_see_the_poison(poison):
    ref = _ragged(None)
    _finite(ref)
    _same(_ragged(poison), ref, f"ragged, poison {poison:#x}")


def _ema(poison):
    """three steps with the generator's moving average kept, then the sampling engine (ema=True: a workspace of its own) samples it"""
    from hipgan.engine import DcganEngine
    torch.manual_seed(12345)
    eng = _engine("dcgan", poison, batch=B, prec="bf16", ema_decay=0.999)
    eng.load_state(*_params("dcgan"))
    smp = DcganEngine(batch=B, share=eng, ema=True)
    if poison is not None:
        _poison(smp, poison)
    out = {}
    for s in range(STEPS):
        out[f"scalars.{s}"] = _step(eng, "dcgan", s, False, first=s * B)
    z = torch.randn(3, 100, generator=torch.Generator().manual_seed(7)).cuda()
    out["ema.sample_batch"] = _bits(smp.sample(z))
    out["ema.sample_running"] = _bits(smp.sample(z, bn="running"))
    _state(eng, out)
    assert "arena.g_ema" in out and "arena.g_ema_bn" in out
    return out


@pytest.mark.parametrize("poison", POISONS)
def test_moving_average_and_its_sampler_do_not_see_the_poison(poison):
    ref = _ema(None)
    _finite(ref)
    _same(_ema(poison), ref, f"ema, poison {poison:#x}")


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("family", ["dcgan", "cgan"])
def test_inference_after_the_steps_does_not_see_the_poison(family, poison):
    _twins(family, poison, prec="bf16", infer=True)


def _fresh_sample(family, poison):
    import bf16_error as be
    torch.manual_seed(12345)
    eng = _engine(family, poison, batch=B, prec="bf16")
    eng.load_state(*_params(family))
    z = torch.randn(3, 100, generator=torch.Generator().manual_seed(7)).cuda()
    lab = be.labels_for(3, 3).cuda() if family == "cgan" else None
    x = eng.sample(z, lab)
    assert bool(torch.isfinite(x).all())
    return {"sample": _bits(x), "arena.g_bn": _bits(eng.arenas["g_bn"])}


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("family", ["dcgan", "cgan"])
def test_sample_as_the_first_call_does_not_see_the_poison(family, poison):
    """no step before it: nothing but this call has written g_z"""
    _same(_fresh_sample(family, poison), _fresh_sample(family, None), f"{family} first sample, poison {poison:#x}")


# ---- part 3: poison of the step's scratch between two steps ----------------------------------------------------------------------------
def _region(eng, name):
    """the bytes of one of jck_engine_tensor's tensors inside the bound workspace"""
    from hipgan._lib import PREC_BF16, load_library
    n = C.c_longlong()
    p = load_library().jck_engine_tensor(eng._h, name.encode(), C.byref(n))
    assert p, name
    wide = name in ("prob", "ds", "norms") or eng.prec != PREC_BF16
    return eng._ws_view(p, n.value * (4 if wide else 2), torch.uint8)


def _two_steps(family, prec, k, poison):
    """steps 0 .. k + 1; poison (if any) goes into the scratch tensors after step k has been joined -> step k + 1's scalars and the state"""
    torch.manual_seed(12345)
    eng = _engine(family, None, batch=B, prec=prec)
    eng.load_state(*_params(family))
    out = {}
    for s in range(k + 2):
        if s == k + 1 and poison is not None:
            eng.join()
            torch.cuda.synchronize()
            for name in STEP_SCRATCH:
                _region(eng, name).fill_(poison)
            torch.cuda.synchronize()
        out[f"scalars.{s}"] = _step(eng, family, s, False, first=s * B)
    _state(eng, out)
    return out


@functools.lru_cache(maxsize=1)
def _two_steps_clean(family, prec, k):
    return _two_steps(family, prec, k, None)


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("k", [0, 1])
@pytest.mark.parametrize("family,prec", [("dcgan", "bf16"), ("dcgan", "f32"), ("cgan", "bf16")])
def test_a_step_reads_none_of_the_scratch_the_step_before_left(family, prec, k, poison):
    ref = _two_steps_clean(family, prec, k)
    _finite(ref)
    _same(_two_steps(family, prec, k, poison), ref, f"{family} {prec}: scratch poisoned with {poison:#x} after step {k}")
