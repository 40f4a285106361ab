"""Host side of feature matching and anomaly scoring (no GPU): hipgan.anomaly's score and AUROC, Sampler.anomaly / .project's refusals
without a discriminator, generate.py's --anomaly / --project_feature_weight arguments, and the C ABI of jck_feat_match and the _fm
entry points, whose argument errors come back before any device call.  tests/test_feat_match_gpu.py is this file's other half."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_anomaly_score():
    from hipgan import JckError
    from hipgan.anomaly import anomaly_score
    r, f = torch.tensor([0.5, 0.25, 0.0], dtype=torch.float32), torch.tensor([2.0, 4.0, 8.0], dtype=torch.float32)
    s = anomaly_score(r, f, 0.25)
    assert s.dtype == torch.float64 and s.tolist() == [0.875, 1.1875, 2.0]
    assert anomaly_score(r, f, 0.0).tolist() == [0.5, 0.25, 0.0]
    third = anomaly_score(torch.tensor([1.0 / 3.0], dtype=torch.float32), torch.tensor([0.0]), 0.5)      # fp64 arithmetic on the fp32 value
    assert float(third) == 0.5 * float(torch.tensor(1.0 / 3.0, dtype=torch.float32))
    assert anomaly_score([1.0, 2.0], [3.0, 4.0], 0.5).tolist() == [2.0, 3.0]
    for bad in (1.0, 1.5, -0.1, float("nan")):
        with pytest.raises(JckError, match="lam"):
            anomaly_score(r, f, bad)
    with pytest.raises(JckError, match="shape"):
        anomaly_score(r, f[:2], 0.1)


def test_auroc_hand_cases():
    from hipgan import JckError
    from hipgan.anomaly import auroc
    flags = [0, 0, 0, 0, 1, 1, 1, 1]
    assert auroc([0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8], flags) == 1.0                     # perfect
    assert auroc([0.5, 0.6, 0.7, 0.8, 0.1, 0.2, 0.3, 0.4], flags) == 0.0                     # inverted
    assert auroc([3.0] * 8, flags) == 0.5                                                     # all tied
    assert auroc([1.0, 2.0, 2.0, 3.0], [False, False, True, True]) == (1 + 0.5 + 1 + 1) / 4   # one tie pair
    assert auroc([1.0, 3.0, 2.0], [False, False, True]) == 0.5                                # one of two pairs in order
    assert auroc(torch.tensor([1.0, 2.0]), torch.tensor([False, True])) == 1.0
    assert auroc(torch.tensor([-float("inf"), float("inf")]), [0, 1]) == 1.0
    for scores, fl, match in (([1.0, 2.0], [1, 1], "both classes"), ([1.0, 2.0], [0, 0], "both classes"),
                              ([1.0, float("nan")], [0, 1], "NaN"), ([1.0, 2.0, 3.0], [0, 1], "flags"), ([1.0, 2.0], [0, 2], "bool")):
        with pytest.raises(JckError, match=match):
            auroc(scores, fl)


def test_sampler_refuses_without_a_discriminator():
    from hipgan import JckError
    from hipgan.sampler import Sampler

    class Eng:                                                                  # a sampler's view of an engine without a discriminator
        family, size, batch, device, _shared = 0, 64, 8, "cpu", {}
    s = Sampler(Eng(), "live")
    u8 = torch.zeros(2, 64, 64, 3, dtype=torch.uint8)
    with pytest.raises(JckError, match="with_d=True"):
        s.anomaly(u8)
    with pytest.raises(JckError, match="with_d=True"):
        s.project(u8, feature_weight=1.0)
    with pytest.raises(JckError, match="lam"):
        s.anomaly(u8, lam=1.0)
    with pytest.raises(JckError, match="restarts"):
        s.anomaly(u8, restarts=0)
    with pytest.raises(JckError, match="feature_weight"):
        s.project(u8, feature_weight=-1.0)


def test_generate_arguments(tmp_path):
    import generate
    base = ["--checkpoint", "x.pt", "--out", str(tmp_path / "o")]
    a = generate.get_arg_parse(base)
    assert a.anomaly is None and a.anomaly_lam is None and a.anomaly_stage is None and a.project_feature_weight is None
    assert not generate.needs_discriminator(a)
    a = generate.get_arg_parse(base + ["--anomaly", "q.npz"])
    assert a.anomaly_lam == 0.1 and a.anomaly_stage is None and a.project_steps == 200 and generate.needs_discriminator(a)
    a = generate.get_arg_parse(base + ["--anomaly", "q.npz", "--anomaly_lam", "0", "--anomaly_stage", "1", "--project_steps", "50", "--project_lr", "0.1"])
    assert a.anomaly_lam == 0.0 and a.anomaly_stage == 1 and a.project_steps == 50 and a.project_lr == 0.1
    a = generate.get_arg_parse(base + ["--project", "g.npz", "--project_feature_weight", "10"])
    assert a.project_feature_weight == 10.0 and generate.needs_discriminator(a)
    assert not generate.needs_discriminator(generate.get_arg_parse(base + ["--project", "g.npz", "--project_feature_weight", "0"]))
    assert not generate.needs_discriminator(generate.get_arg_parse(base + ["--project", "g.npz"]))
    for bad in (["--anomaly", "q.npz", "--anomaly_lam", "1.0"], ["--anomaly", "q.npz", "--anomaly_lam", "-0.1"], ["--anomaly_lam", "0.1"],
                ["--anomaly_stage", "1"], ["--anomaly", "q.npz", "--anomaly_stage", "9"], ["--anomaly", "q.npz", "--project", "g.npz"],
                ["--anomaly", "q.npz", "--inpaint", "f.npz", "--mask", "center:32"], ["--anomaly", "q.npz", "--num", "4"],
                ["--anomaly", "q.npz", "--score"], ["--anomaly", "q.npz", "--score_images", "x.npz"], ["--anomaly", "q.npz", "--refine", "3"],
                ["--anomaly", "q.npz", "--features", "x.npz"], ["--anomaly", "q.npz", "--interpolate", "2:5"],
                ["--anomaly", "q.npz", "--select", "top", "--oversample", "2"], ["--project_feature_weight", "1"],
                ["--project", "g.npz", "--project_feature_weight", "-1"], ["--anomaly", "q.npz", "--project_feature_weight", "1"]):
        with pytest.raises(SystemExit):
            generate.get_arg_parse(base + bad)
    from hipgan import JckError
    for flags in (["--anomaly", "q.npz"], ["--project", "g.npz", "--project_feature_weight", "1"]):      # a checkpoint without model_d
        with pytest.raises(JckError, match="model_d"):
            generate.check_checkpoint(generate.get_arg_parse(base + flags), {"model_g": {"conv1.weight": torch.zeros(1)}})


def test_abi_declares_and_exports_the_entry_points():
    from hipgan import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    dll = _lib.load_library()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jckgan.h")).read(), flags=re.S)
    for name, nargs in (("jck_feat_match", 13), ("jck_engine_latent_grad_fm", 17), ("jck_engine_project_fm", 21)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", src)
        assert m, f"{name} is not declared in include/jckgan.h"
        assert len(m.group(1).split(",")) == nargs == len(_lib.PROTOS[name][1]), name
        assert hasattr(dll, name), f"{name} is not exported"
    names = []
    while dll.jck_launch_name(len(names)):
        names.append(dll.jck_launch_name(len(names)))
    assert len(names) == 38 and not any(b"feat" in n for n in names)          # nothing new is enumerated


def test_entry_points_fail_on_the_host_without_a_device():
    """argument errors come back as JCK_E_ARG with a message before any device call"""
    from hipgan import _lib
    dll = _lib.load_library()
    buf = (C.c_float * 256)()
    p = C.cast(buf, C.c_void_p)
    odd = C.c_void_p(p.value + 4)
    fm = lambda a=p, f=p, sc=p, w=0.125, gy=p, acc=0, ft=p, n=1, m=64, c=8, prec=1: dll.jck_feat_match(prec, a, f, sc, 0.2, w, gy, acc, ft, n, m, c, None)
    for kw in (dict(a=None), dict(f=None), dict(sc=None), dict(gy=None), dict(ft=None), dict(n=0)):
        assert fm(**kw) == -1 and b"feat_match" in dll.jck_last_error(), kw
    for kw in (dict(c=12, m=48), dict(c=4, m=64), dict(c=0)):
        assert fm(**kw) == -1 and b"power of two" in dll.jck_last_error(), kw
    for kw in (dict(m=68), dict(m=0), dict(m=4)):
        assert fm(**kw) == -1 and b"multiple of C" in dll.jck_last_error(), kw
    for w in (-1.0, float("inf"), float("nan")):
        assert fm(w=w) == -1 and b"weight" in dll.jck_last_error(), w
    for kw in (dict(a=odd), dict(f=odd), dict(gy=odd), dict(sc=odd)):
        assert fm(**kw) == -1 and b"aligned" in dll.jck_last_error(), kw
    assert fm(acc=2) == -1 and b"accumulate" in dll.jck_last_error()
    for prec in (3, -1):
        assert fm(prec=prec) == -1 and b"prec" in dll.jck_last_error(), prec
    assert dll.jck_engine_latent_grad_fm(None, p, None, p, None, 0, 0.0, 1, p, p, p, p, None, p, -1, 1.0, p) == -1 and b"not bound" in dll.jck_last_error()
    assert b"latent_grad_fm" in dll.jck_last_error()
    assert dll.jck_engine_project_fm(None, p, None, p, 1, 1, 0.05, 0.0, None, 0, 0.0, p, p, 0, p, p, None, p, -1, 1.0, p) == -1
    assert b"not bound" in dll.jck_last_error() and b"project_fm" in dll.jck_last_error()
