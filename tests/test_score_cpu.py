"""Host side of discriminator scoring (no GPU): the selection helpers (select_top, drs_accept), the checkpoint's discriminator,
generate.py's argument validation for --score / --select / --score_images, and the new entry points' place in the C ABI."""
import ctypes as C
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def _closed_form(l, M, gamma, eps=1e-8):
    """Azadi et al. 2019, eq. 8, with plain fp64 arithmetic on one logit"""
    d = min(l - M, 0.0)
    F = d - math.log(1.0 - math.exp(d - eps)) - gamma
    return 1.0 / (1.0 + math.exp(-F))


def test_drs_accept_closed_form():
    from hipgan.sampler import drs_accept, drs_f
    M, gamma = 2.0, 1.5
    logits = [2.0, 3.5, 1.999, 1.0, 0.0, -4.0, -30.0, NAN]           # l = M, l > M (clamped to M), just below, ..., NaN
    p = [_closed_form(l, M, gamma) for l in logits[:-1]]
    assert p[0] == p[1] > 0.999 and all(a >= b for a, b in zip(p[1:], p[2:])) and p[-1] < 1e-12
    f = drs_f(logits, M, gamma)
    assert f.dtype == torch.float64 and math.isnan(float(f[-1]))
    for got, l in zip(f[:-1].tolist(), logits[:-1]):
        d = min(l - M, 0.0)
        assert got == pytest.approx(d - math.log(1.0 - math.exp(d - 1e-8)) - gamma, rel=1e-12, abs=1e-12)
    for shift in (-1e-9, 1e-9):                                       # u just below the acceptance probability accepts, just above rejects
        u = [min(max(q * (1.0 + shift) + shift * 1e-300, 0.0), 1.0) for q in p] + [0.0]
        acc = drs_accept(logits, M, gamma, u)
        assert acc.dtype == torch.bool and acc[:-1].tolist() == [shift < 0 and q > 0 for q in p] and not bool(acc[-1])
    assert drs_accept(logits, M, gamma, [0.0] * 8).tolist() == [True] * 7 + [False]      # a NaN logit is rejected even at u = 0
    with pytest.raises(Exception):
        drs_accept(logits, M, gamma, [0.5] * 3)


def test_drs_accept_monotone_and_limits():
    from hipgan.sampler import drs_accept
    g = torch.Generator().manual_seed(1)
    logits = torch.sort(torch.randn(200, generator=g, dtype=torch.float64) * 3).values
    M = float(logits.max())
    for u in (0.01, 0.3, 0.9):
        acc = drs_accept(logits, M, 0.0, torch.full((200,), u, dtype=torch.float64)).int()
        assert bool((acc[1:] >= acc[:-1]).all()), u                  # fixed u: once a logit is accepted every larger one is
    u = torch.rand(200, generator=g, dtype=torch.float64) * 0.999
    assert bool(drs_accept(logits, M, -1e300, u).all())               # gamma -> -inf accepts everything finite
    assert bool(drs_accept(logits, M, -INF, u).all())
    assert not bool(drs_accept(logits, M, 1e300, u + 1e-300).any())  # gamma -> +inf rejects
    more = drs_accept(logits, M, -2.0, u).sum()
    assert more >= drs_accept(logits, M, 2.0, u).sum()
    assert bool(drs_accept(torch.tensor([-INF]), M, -1e300, [0.5]).item()) is False      # sigmoid(-inf - gamma): F = -inf + 1e300 = -inf


def test_select_top():
    from hipgan import JckError
    from hipgan.sampler import select_top
    l = torch.tensor([0.5, 2.0, NAN, 2.0, -1.0, 7.0, NAN, 0.5])
    assert select_top(l, 3).tolist() == [5, 1, 3]                     # ties go to the lower index
    assert select_top(l, 6).tolist() == [5, 1, 3, 0, 7, 4]            # NaN is never selected
    assert select_top(l, 0).tolist() == [] and select_top(l, 1).dtype == torch.int64
    with pytest.raises(JckError, match="only 6 of 8"):
        select_top(l, 7)
    with pytest.raises(JckError):
        select_top(torch.tensor([NAN, NAN]), 1)
    assert select_top(torch.tensor([1.0, -INF, NAN, INF]), 3).tolist() == [3, 0, 1]
    assert select_top(torch.tensor([3.0, 3.0, 3.0], dtype=torch.bfloat16), 2).tolist() == [0, 1]
    big = torch.randn(1000, generator=torch.Generator().manual_seed(2))
    assert select_top(big, 10).tolist() == torch.topk(big, 10).indices.tolist()


def test_latents_continue_one_stream():
    """the pieces Sampler.images(select=...) draws are successive pieces of latents(n, seed): one helper, one arithmetic"""
    from hipgan.sampler import latents
    for t in (None, 0.7):
        g = torch.Generator().manual_seed(5)
        a, b = latents(6, 5, t, generator=g), latents(4, 5, t, generator=g)
        assert torch.equal(a, latents(6, 5, t)) and not torch.equal(b, latents(4, 5, t))


def test_pick_discriminator_state():
    from hipgan import JckError
    from hipgan.sampler import pick_discriminator_state
    d = {"conv1.weight": torch.zeros(1)}
    assert pick_discriminator_state({"model_g": {}, "model_d": d}) is d
    for bad in ({"model_g": {}}, {"model_g": {}, "model_d": {}}, {"model_g": {}, "model_d": None}, [1, 2], None):
        with pytest.raises(JckError, match="model_d"):
            pick_discriminator_state(bad)


def test_cli_validation():
    import generate
    from hipgan import JckError
    base = ["--checkpoint", "c.pt", "--out", "o"]
    a = generate.get_arg_parse(base)
    assert a.score is False and a.select is None and a.oversample is None and a.score_images is None
    assert not generate.needs_discriminator(a)
    generate.check_checkpoint(a, {"model_g": {}})                     # no new flag: the checkpoint needs no discriminator
    a = generate.get_arg_parse(base + ["--select", "top", "--oversample", "4", "--score", "--num", "8"])
    assert a.select == "top" and a.oversample == 4 and a.score and generate.needs_discriminator(a)
    assert generate.get_arg_parse(base + ["--select", "drs", "--oversample", "1"]).num == 64
    assert generate.get_arg_parse(base + ["-m", "CGAN", "--select", "top", "--oversample", "2", "--classes", "17"]).classes == [17]
    for bad in (["--select", "top"], ["--select", "top", "--oversample", "0"], ["--select", "best", "--oversample", "2"], ["--oversample", "2"],
                ["--select", "drs", "--oversample", "2", "--interpolate", "2:5"], ["-m", "CGAN", "--select", "top", "--oversample", "2", "--classes", "3,17"], ["--select", "top", "--oversample", "2", "--bn", "batch"],
                ["--score", "--bn", "batch"], ["--score_images", "x.npz", "--num", "4"], ["--score_images", "x.npz", "--score"],
                ["--score_images", "x.npz", "--select", "top", "--oversample", "2"]):
        with pytest.raises(SystemExit):
            generate.get_arg_parse(base + bad)
    # --select / --score / --score_images on a checkpoint without model_d: a clear error before any engine exists
    for flags in (["--select", "top", "--oversample", "2"], ["--score"], ["--score_images", "x.npz"]):
        a = generate.get_arg_parse(base + flags)
        with pytest.raises(JckError, match="model_d"):
            generate.check_checkpoint(a, {"model_g": {"conv1.weight": torch.zeros(1)}})
        generate.check_checkpoint(a, {"model_g": {}, "model_d": {"conv1.weight": torch.zeros(1)}})


def test_sampler_with_d_needs_a_gpu_or_a_discriminator(monkeypatch):
    from hipgan import JckError
    from hipgan.sampler import Sampler
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(JckError, match="GPU"):
        Sampler.from_checkpoint({"model_g": {}, "model_d": {}}, "DCGAN", with_d=True)


def test_abi_declares_and_exports_the_entry_points():
    from hipgan import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    dll = _lib.load_library()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jckgan.h")).read(), flags=re.S)
    for name, nargs in (("jck_conv_down_affine", 13), ("jck_engine_score", 8), ("jck_score_head", 9)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", src)
        assert m, f"{name} is not declared in include/jckgan.h"
        assert len(m.group(1).split(",")) == nargs == len(_lib.PROTOS[name][1]), name
        assert hasattr(dll, name), f"{name} is not exported"


def test_entry_points_fail_on_the_host_without_a_device():
    """argument errors come back as JCK_E_ARG with a message before any device call"""
    from hipgan import _lib
    dll = _lib.load_library()
    buf = (C.c_float * 256)()
    p = C.cast(buf, C.c_void_p)
    assert dll.jck_engine_score(None, p, None, None, 1, p, p, None) == -1 and b"not bound" in dll.jck_last_error()
    args = lambda scale, shift, cb, cs: (1, p, p, scale, shift, 0.2, p, 1, 8, 8, cb, cs, None)
    assert dll.jck_conv_down_affine(*args(None, p, 64, 128)) == -1 and b"scale" in dll.jck_last_error()
    assert dll.jck_conv_down_affine(*args(p, None, 64, 128)) == -1
    for cb, cs in ((8, 64), (32, 64), (4, 128), (64, 32), (64, 96), (96, 128)):
        assert dll.jck_conv_down_affine(*args(p, p, cb, cs)) == -1, (cb, cs)
        assert b"conv_down_affine" in dll.jck_last_error()
    assert dll.jck_conv_down_affine(1, None, p, p, p, 0.2, p, 1, 8, 8, 64, 128, None) == -1
    assert dll.jck_conv_down_affine(1, p, p, p, p, 0.2, p, 0, 8, 8, 64, 128, None) == -1
    assert dll.jck_conv_down_affine(1, p, p, p, p, 0.2, p, 1, 12, 12, 64, 128, None) == -1       # not a power of two
    assert dll.jck_score_head(1, None, p, None, 1, 256, p, p, None) == -1
    assert dll.jck_score_head(1, p, p, None, 1, 100, p, p, None) == -1 and b"multiple of 8" in dll.jck_last_error()
    assert dll.jck_score_head(1, p, p, None, 0, 256, p, p, None) == -1


def test_score_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        return                                  # (tests/test_score_gpu.py is this file's other half)
    from hipgan import JckError, lib
    with pytest.raises(JckError):
        lib.jck_conv_down_affine(1, torch.zeros(4), torch.zeros(4), torch.zeros(4), torch.zeros(4), 0.2, torch.zeros(4), 1, 8, 8, 64, 128, None)
    from hipgan.engine import DcganEngine
    with pytest.raises(JckError, match="GPU"):
        DcganEngine(batch=4).score(torch.zeros(1, 3, 64, 64))
