"""The refusals of jck_engine_phase: every call below is an argument error that host code returns before the phase enqueues any
work, with the words a caller sees, and a refused call costs nothing - the engine then finishes a normal step whose scalars and
arenas equal, bit for bit, those of a second engine that started from the same state, got the same inputs and never saw the
refused call.  Engines are 64x64 at batch 8 (batched schedule) or 12 (12 % 8 != 0: the per-pass schedule)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

ARENAS = ("g_params", "d_params", "g_grads", "d_grads")
ONLY_BATCHED = "only with the batched DCGAN schedule"
REAL_FWD = "PHASE_D_REAL_FWD: only with the batched"


def _null(*fields):
    def f(si):
        for name in fields:
            if name.startswith("drop_mask"):
                si.drop_mask[int(name[-1])] = None
            else:
                setattr(si, name, None)
    return f


def _pair(family, B):
    """Two engines of one family and batch in the same initial state, and one step's inputs for both."""
    from hipgan.engine import CganEngine, DcganEngine
    from oracle.gan_oracle import build_params
    from util import synth_images, synth_onehot
    torch.manual_seed(12345)
    g, d = build_params(family)
    engs = []
    for _ in range(2):
        eng = (CganEngine if family == "cgan" else DcganEngine)(batch=B)
        eng.graphs = False
        eng.load_state(g, d)
        engs.append(eng)
    real = synth_images(B).cuda()
    labels = synth_onehot(B)[0].cuda() if family == "cgan" else None
    noise = engs[0].draw_noise(generator=torch.Generator(device="cuda").manual_seed(5), labels=labels)
    return engs[0], engs[1], real, noise


def _refuse(eng, phase, si, words):
    from hipgan import JckError
    from hipgan._lib import lib
    with pytest.raises(JckError) as err:
        lib.jck_engine_phase(eng._h, phase, C.byref(si), torch.cuda.current_stream().cuda_stream)
    assert words in str(err.value), (phase, str(err.value))


def _same_step(eng, ref):
    a, b = eng.scalars(), ref.scalars()
    assert list(a.values()) == list(b.values()) and all(v == v for v in a.values()), (a, b)      # no NaN hides a difference
    for k in ARENAS:
        assert torch.equal(eng.arenas[k], ref.arenas[k]), k


def _cases():
    from hipgan.engine import (PHASE_D_LOSS, PHASE_D_LOSS_A, PHASE_D_LOSS_B, PHASE_D_REAL_FWD, PHASE_GP_ONLY)
    real = True
    return {
        # 1: the two halves of the split D pass exist for DCGAN only
        "cgan_loss_a_b": ("cgan", 8, [(PHASE_D_LOSS_A, real, None, ONLY_BATCHED), (PHASE_D_LOSS_B, real, None, ONLY_BATCHED)]),
        # 2: ... and only with the batched schedule; the same for the announced-ahead D(real) forward
        "dcgan_per_pass_loss_a_real_fwd": ("dcgan", 12, [(PHASE_D_LOSS_A, real, None, ONLY_BATCHED), (PHASE_D_REAL_FWD, real, None, REAL_FWD)]),
        # 3
        "cgan_real_fwd": ("cgan", 8, [(PHASE_D_REAL_FWD, real, None, REAL_FWD)]),
        # 4: no real batch at all
        "dcgan_no_real": ("dcgan", 8, [(PHASE_D_LOSS, not real, None, "needs real_nchw"), (PHASE_D_REAL_FWD, not real, None, "needs real_nchw")]),
        # 5
        "cgan_no_labels": ("cgan", 8, [(PHASE_D_LOSS, real, _null("labels"), "CGAN phases need labels")]),
        # 6: the stand-alone penalty
        "dcgan_gp_only_no_alpha": ("dcgan", 8, [(PHASE_GP_ONLY, real, _null("alpha"), "PHASE_GP_ONLY needs")]),
        "cgan_gp_only_no_mask": ("cgan", 8, [(PHASE_GP_ONLY, real, _null("drop_mask2"), "needs drop_mask[2]")]),
        # 7
        "unknown_phase": ("dcgan", 8, [(99, real, None, "unknown phase")]),
    }


@pytest.mark.parametrize("case", ["cgan_loss_a_b", "dcgan_per_pass_loss_a_real_fwd", "cgan_real_fwd", "dcgan_no_real", "cgan_no_labels",
                                  "dcgan_gp_only_no_alpha", "cgan_gp_only_no_mask", "unknown_phase"])
def test_refused_phase_says_why_and_costs_nothing(case):
    family, B, calls = _cases()[case]
    eng, ref, real, noise = _pair(family, B)
    keep = []
    for phase, with_real, edit, words in calls:
        si, k = eng._inputs(real if with_real else None, noise, 2e-4, 1.0)
        keep.append(k)
        if edit:
            edit(si)
        _refuse(eng, phase, si, words)
    for e in (eng, ref):
        e.step_async(real, noise, 2e-4)
    _same_step(eng, ref)


def test_d_step_before_the_penalty_is_joined_is_refused_and_costs_nothing():
    """Per-pass DCGAN schedule: PHASE_D_LOSS starts the penalty pass on its own stream and PHASE_D_GP joins it; the optimiser
    phase in between is refused, and the step then goes on phase by phase to the result of an undisturbed step."""
    from hipgan._lib import lib
    from hipgan.engine import PHASE_D_GP, PHASE_D_LOSS, PHASE_D_STEP, PHASE_G_LOSS, PHASE_G_STEP
    eng, ref, real, noise = _pair("dcgan", 12)
    si, keep = eng._inputs(real, noise, 2e-4, 1.0)
    st = torch.cuda.current_stream().cuda_stream
    lib.jck_engine_phase(eng._h, PHASE_D_LOSS, C.byref(si), st)
    _refuse(eng, PHASE_D_STEP, si, "PHASE_D_GP must be called before PHASE_D_STEP")
    for phase in (PHASE_D_GP, PHASE_D_STEP, PHASE_G_LOSS, PHASE_G_STEP):
        lib.jck_engine_phase(eng._h, phase, C.byref(si), st)
    eng.t += 1                                   # what step_async notes behind its last phase
    eng._shared["last_step"] = eng.t
    eng._shared["version"] += 1
    eng._packed_version = eng._shared["version"]
    ref.step_async(real, noise, 2e-4)
    _same_step(eng, ref)
