"""Host side of semantic inpainting and latent refinement (no GPU): hipgan.inpaint's masks, importance weights and blend,
generate.py's --inpaint / --refine arguments and their errors before any engine exists, and the C entry points' argument errors,
which come back before any device call.  tests/test_critic_grad_gpu.py is this file's other half."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parse_mask_specs(tmp_path):
    from hipgan.inpaint import parse_mask
    k = parse_mask("center:32", 64)
    assert k.dtype == torch.bool and k.shape == (64, 64) and int((~k).sum()) == 32 * 32
    assert not bool(k[16:48, 16:48].any()) and bool(k[:16].all()) and bool(k[48:].all()) and bool(k[:, :16].all()) and bool(k[:, 48:].all())
    k = parse_mask("center:5", 64)                                            # an odd hole: rows 29..33
    assert int((~k).sum()) == 25 and not bool(k[29:34, 29:34].any()) and bool(k[28].all()) and bool(k[34].all())
    assert int((~parse_mask("center:1", 128)).sum()) == 1 and int(parse_mask("center:63", 64).sum()) == 64 * 64 - 63 * 63
    for side, hole in (("left", (slice(None), slice(0, 32))), ("right", (slice(None), slice(32, 64))), ("top", (slice(0, 32), slice(None))),
                       ("bottom", (slice(32, 64), slice(None)))):
        k = parse_mask(f"half:{side}", 64)
        assert int(k.sum()) == 32 * 64 and not bool(k[hole].any()), side
    m = np.zeros((64, 64), np.uint8)
    m[::2] = 3                                                                  # non-zero = known
    np.save(str(tmp_path / "m.npy"), m)
    np.savez(str(tmp_path / "m.npz"), mask=np.stack([m, 1 - (m > 0)]).astype(bool))
    k = parse_mask(str(tmp_path / "m.npy"), 64)
    assert k.dtype == torch.bool and torch.equal(k, torch.from_numpy(m > 0))
    k = parse_mask(str(tmp_path / "m.npz"), 64)
    assert k.shape == (2, 64, 64) and torch.equal(k[0], torch.from_numpy(m > 0)) and torch.equal(k[1], ~torch.from_numpy(m > 0))


def test_parse_mask_errors(tmp_path):
    from hipgan import JckError
    from hipgan.inpaint import parse_mask
    np.savez(str(tmp_path / "nomask.npz"), known=np.ones((64, 64), bool))
    np.save(str(tmp_path / "small.npy"), np.ones((32, 32), bool))
    np.save(str(tmp_path / "none.npy"), np.zeros((64, 64), bool))               # all unknown
    np.save(str(tmp_path / "one_none.npy"), np.stack([np.ones((64, 64), bool), np.zeros((64, 64), bool)]))
    for spec, match in (("center:0", "side"), ("center:64", "side"), ("center:x", "integer"), ("center:", "integer"), ("half:middle", "half"),
                        ("half:", "half"), ("ring:3", "neither"), ("", "non-empty"), (None, "non-empty"), (3, "non-empty"),
                        (str(tmp_path / "absent.npz"), "no such file"), (str(tmp_path / "nomask.npz"), "no 'mask'"),
                        (str(tmp_path / "small.npy"), "must be"), (str(tmp_path / "none.npy"), "no pixel known"),
                        (str(tmp_path / "one_none.npy"), "no pixel known")):
        with pytest.raises(JckError, match=match):
            parse_mask(spec, 64)
    with pytest.raises(JckError, match="size"):
        parse_mask("center:1", 1)


def _weights_loop(known, window):
    """w_p = known_p * (unknown pixels in the window around p) / window^2, the picture's outside counted as known"""
    s, r = known.shape[0], window // 2
    w = np.zeros((s, s), np.float64)
    for y in range(s):
        for x in range(s):
            if not known[y, x]:
                continue
            cnt = 0
            for dy in range(-r, r + 1):
                for dx in range(-r, r + 1):
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < s and 0 <= xx < s and not known[yy, xx]:
                        cnt += 1
            w[y, x] = cnt / float(window * window)
    return w


def test_importance_weights_against_a_loop():
    from hipgan import JckError
    from hipgan.inpaint import importance_weights, parse_mask
    rnd = torch.rand(24, 24, generator=torch.Generator().manual_seed(5)) < 0.6
    corner = torch.ones(24, 24, dtype=torch.bool)
    corner[:6, :9] = False                                                      # a hole that touches the border
    for known in (parse_mask("center:12", 24), parse_mask("half:top", 24), rnd, corner):
        for window in (1, 3, 7):
            w = importance_weights(known, window)
            assert w.dtype == torch.float32 and w.shape == known.shape
            np.testing.assert_allclose(w.double().numpy(), _weights_loop(known.numpy(), window), rtol=0, atol=1e-6)
            assert bool((w[~known] == 0).all())
        w0 = importance_weights(known, 0)
        assert w0.dtype == torch.float32 and torch.equal(w0, known.float())
    assert float(importance_weights(parse_mask("center:12", 24), 1).sum()) == 0.0      # window 1: a known pixel has no unknown share
    both = torch.stack([rnd, corner])
    wb = importance_weights(both, 3)                                            # batched masks: image by image
    assert wb.shape == (2, 24, 24) and torch.equal(wb[0], importance_weights(rnd, 3)) and torch.equal(wb[1], importance_weights(corner, 3))
    for bad in (2, -1, 4):
        with pytest.raises(JckError, match="window"):
            importance_weights(rnd, bad)
    with pytest.raises(JckError, match="mask must be"):
        importance_weights(torch.ones(4, 5, dtype=torch.bool))


def test_blend():
    from hipgan import JckError
    from hipgan.inpaint import blend, parse_mask
    g = torch.Generator().manual_seed(7)
    t = torch.randint(0, 256, (3, 64, 64, 3), generator=g, dtype=torch.uint8)
    x = torch.randint(0, 256, (3, 64, 64, 3), generator=g, dtype=torch.uint8)
    known = parse_mask("half:left", 64)
    out = blend(t, x, known)
    assert out.dtype == torch.uint8 and torch.equal(out[:, :, 32:], t[:, :, 32:]) and torch.equal(out[:, :, :32], x[:, :, :32])
    per = torch.stack([known, ~known, parse_mask("center:8", 64)])
    out = blend(t, x, per)
    assert torch.equal(out[1, :, :32], t[1, :, :32]) and torch.equal(out[1, :, 32:], x[1, :, 32:]) and torch.equal(out[0], blend(t, x, known)[0])
    assert torch.equal(out[2, 28:36, 28:36], x[2, 28:36, 28:36]) and torch.equal(out[2, :28], t[2, :28])
    with pytest.raises(JckError, match="uint8"):
        blend(t.float(), x, known)
    with pytest.raises(JckError, match="uint8"):
        blend(t, x[:2], known)
    with pytest.raises(JckError, match="masks for"):
        blend(t, x, per[:2])
    with pytest.raises(JckError, match="no pixel known"):
        blend(t, x, torch.zeros(64, 64, dtype=torch.bool))


def test_generate_arguments_and_errors_before_any_engine(tmp_path, monkeypatch):
    import generate
    from hipgan import JckError
    base = ["--checkpoint", "x.pt", "--out", str(tmp_path / "o")]
    a = generate.get_arg_parse(base)
    assert a.inpaint is None and a.mask is None and a.critic_weight is None and a.refine is None and a.refine_lr is None
    assert not generate.needs_discriminator(a)
    a = generate.get_arg_parse(base + ["--inpaint", "f.npz", "--mask", "center:32"])
    assert a.critic_weight == 0.003 and a.project_steps == 200 and generate.needs_discriminator(a)
    a = generate.get_arg_parse(base + ["--inpaint", "f.npz", "--mask", "center:32", "--critic_weight", "0", "--project_steps", "50", "--project_lr", "0.1"])
    assert a.critic_weight == 0.0 and a.project_steps == 50 and a.project_lr == 0.1 and not generate.needs_discriminator(a)
    a = generate.get_arg_parse(base + ["--refine", "10", "--num", "8"])
    assert a.refine == 10 and a.refine_lr == 0.02 and generate.needs_discriminator(a)
    assert generate.get_arg_parse(base + ["--refine", "3", "--refine_lr", "0.1", "--score"]).refine_lr == 0.1
    for bad in (["--inpaint", "f.npz"], ["--mask", "center:32"], ["--inpaint", "f.npz", "--mask", "center:32", "--num", "4"],
                ["--inpaint", "f.npz", "--mask", "center:32", "--project", "g.npz"], ["--inpaint", "f.npz", "--mask", "center:32", "--score"],
                ["--inpaint", "f.npz", "--mask", "center:32", "--refine", "3"], ["--inpaint", "f.npz", "--mask", "center:32", "--critic_weight", "-1"],
                ["--inpaint", "f.npz", "--mask", "center:32", "--select", "top", "--oversample", "2"], ["--critic_weight", "0.1"],
                ["--refine", "0"], ["--refine_lr", "0.1"], ["--refine", "3", "--refine_lr", "0"], ["--refine", "3", "--bn", "batch"],
                ["--refine", "3", "--project", "g.npz"], ["--refine", "3", "--interpolate", "2:5"],
                ["--refine", "3", "--select", "top", "--oversample", "2"], ["--refine", "3", "--score_images", "x.npz"]):
        with pytest.raises(SystemExit):
            generate.get_arg_parse(base + bad)
    # a checkpoint without model_d: refused before any engine exists
    for flags in (["--refine", "3"], ["--inpaint", "f.npz", "--mask", "center:32"]):
        a = generate.get_arg_parse(base + flags)
        with pytest.raises(JckError, match="model_d"):
            generate.check_checkpoint(a, {"model_g": {"conv1.weight": torch.zeros(1)}})
    generate.check_checkpoint(generate.get_arg_parse(base + ["--inpaint", "f.npz", "--mask", "center:32", "--critic_weight", "0"]), {"model_g": {}})
    # ... and so are a bad picture file, a bad mask and an all-unknown mask: main() gets to no Sampler
    from hipgan import sampler
    monkeypatch.setattr(sampler.Sampler, "from_checkpoint", classmethod(lambda *a, **k: pytest.fail("an engine was created")))
    pics = str(tmp_path / "pics.npz")
    np.savez(pics, images=np.zeros((3, 64, 64, 3), np.uint8))
    np.save(str(tmp_path / "none.npy"), np.zeros((64, 64), bool))
    np.save(str(tmp_path / "two.npy"), np.ones((2, 64, 64), bool))
    for flags, match in ((["--inpaint", str(tmp_path / "absent.npz"), "--mask", "center:32"], None),
                         (["--inpaint", pics, "--mask", "center:64"], "side"), (["--inpaint", pics, "--mask", "disc:3"], "neither"),
                         (["--inpaint", pics, "--mask", str(tmp_path / "none.npy")], "no pixel known"),
                         (["--inpaint", pics, "--mask", str(tmp_path / "two.npy")], "masks for"),
                         (["-m", "CGAN", "--inpaint", pics, "--mask", "center:32"], "labels")):
        with pytest.raises(JckError if match else Exception, match=match):
            generate.main(base + flags)
    ckpt = str(tmp_path / "g_only.pt")
    torch.save({"model_g": {"conv1.weight": torch.zeros(1)}, "model_d": {}}, ckpt)
    for flags in (["--refine", "3"], ["--inpaint", pics, "--mask", "center:32"]):
        with pytest.raises(JckError, match="model_d"):
            generate.main(["--checkpoint", ckpt, "--out", str(tmp_path / "o")] + flags)
    u8, known, cls = generate.plan_inpaint(generate.get_arg_parse(base + ["--inpaint", pics, "--mask", "half:top"]))
    assert u8.shape == (3, 64, 64, 3) and known.shape == (64, 64) and cls is None and not bool(known[:32].any())


def test_engine_and_sampler_refuse_on_the_host(monkeypatch):
    """what the Python layer checks before it touches a device"""
    from hipgan import JckError
    from hipgan.engine import CRITIC_MODES, chunk_plan
    assert CRITIC_MODES == {None: 0, "nsgan": 1, "logit": 2}
    assert chunk_plan(11, 8) == [(0, 8), (8, 11)]
    from hipgan.sampler import Sampler

    class Eng:                                                                  # a sampler's view of an engine without a discriminator
        family, size, batch, device, _shared = 0, 64, 8, "cpu", {}
    s = Sampler(Eng(), "live")
    u8 = torch.zeros(2, 64, 64, 3, dtype=torch.uint8)
    known = torch.ones(64, 64, dtype=torch.bool)
    known[10:20, 10:20] = False
    with pytest.raises(JckError, match="with_d=True"):
        s.inpaint(u8, known)
    with pytest.raises(JckError, match="with_d=True"):
        s.refine(torch.zeros(2, 100))
    with pytest.raises(JckError, match="with_d=True"):
        s.images(2, select="refine")
    with pytest.raises(JckError, match="no pixel known"):
        s.inpaint(u8, torch.zeros(64, 64, dtype=torch.bool), critic_weight=0.0)
    with pytest.raises(JckError, match="uint8"):
        s.inpaint(u8.float(), known, critic_weight=0.0)
    with pytest.raises(JckError, match="restarts"):
        s.inpaint(u8, known, critic_weight=0.0, restarts=0)
    with pytest.raises(JckError, match="critic_weight"):
        s.inpaint(u8, known, critic_weight=-1.0)
    with pytest.raises(JckError, match="masks for"):
        s.inpaint(u8, known.unsqueeze(0).expand(3, -1, -1), critic_weight=0.0)
    with pytest.raises(JckError, match="all zero"):                            # window 1: no known pixel has an unknown share
        s.inpaint(u8, known, critic_weight=0.0, window=1)
    with pytest.raises(JckError, match="select must be"):
        s.images(2, select="best")


def test_restart_rows_and_the_pick_of_the_best_start():
    """restarts run as extra rows: row r * n + i is image i from seed + r, and the pick per image is the lowest score, ties to the lowest seed"""
    from hipgan.sampler import latents, pick_best, restart_rows
    n, R, seed = 2, 3, 7
    t = torch.arange(n * 3.0).view(n, 3, 1, 1)
    lab = torch.tensor([[1, 0], [0, 1]])
    z0, tt, none, ll = restart_rows(n, R, seed, t, None, lab)
    assert z0.shape == (R * n, 100) and tt.shape == (R * n, 3, 1, 1) and ll.shape == (R * n, 2) and none is None
    for r in range(R):
        zr = latents(n, seed + r)
        for i in range(n):
            assert torch.equal(z0[r * n + i], zr[i]) and torch.equal(tt[r * n + i], t[i]) and torch.equal(ll[r * n + i], lab[i])
    z1, t1, l1 = restart_rows(n, 1, seed, t, lab)                               # one start: the rows as they are
    assert torch.equal(z1, latents(n, seed)) and t1 is t and l1 is lab
    # image 0: seeds 7 and 8 tie at the minimum -> seed 7 (row 0); image 1: seed 9 is the lowest (row 5)
    score = torch.tensor([1.0, 5.0, 1.0, 4.0, 2.0, 3.0])
    rows = torch.arange(R * n)
    z, s = pick_best(score, n, rows, score)
    assert z.tolist() == [0, 5] and s.tolist() == [1.0, 3.0]
    score = torch.tensor([2.0, 3.0, 1.0, 3.0, 1.0, 3.0])                        # image 0: seeds 8 and 9 tie; image 1: all three tie
    assert pick_best(score, n, rows)[0].tolist() == [2, 1]
    assert pick_best(score[:n], n, rows[:n])[0] is not None and pick_best(score[:n], n, rows[:n])[0].tolist() == [0, 1]


def test_abi_declares_and_exports_the_entry_points():
    from hipgan import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    dll = _lib.load_library()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jckgan.h")).read(), flags=re.S)
    for name, nargs in (("jck_conv_up_mask", 13), ("jck_leaky_affine_bwd", 9), ("jck_critic_ds", 7), ("jck_latent_loss_ex", 10),
                        ("jck_engine_latent_grad_ex", 13), ("jck_engine_project_ex", 17)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", src)
        assert m, f"{name} is not declared in include/jckgan.h"
        assert len(m.group(1).split(",")) == nargs == len(_lib.PROTOS[name][1]), name
        assert hasattr(dll, name), f"{name} is not exported"
    names = []
    while dll.jck_launch_name(len(names)):
        names.append(dll.jck_launch_name(len(names)))
    assert len(names) == 38 and not any(b"mask" in n or b"critic" in n or b"leaky" in n for n in names)      # nothing new is enumerated


def test_entry_points_fail_on_the_host_without_a_device():
    """argument errors come back as JCK_E_ARG with a message before any device call"""
    from hipgan import _lib
    dll = _lib.load_library()
    buf = (C.c_float * 256)()
    p = C.cast(buf, C.c_void_p)
    odd = C.c_void_p(p.value + 4)
    up = lambda a, scale, cs, cb, n=1: dll.jck_conv_up_mask(1, p, p, a, scale, 0.2, p, n, 4, 4, cs, cb, None)
    assert up(None, p, 128, 128) == -1 and b"conv_up_mask" in dll.jck_last_error()
    assert up(p, None, 128, 128) == -1
    assert up(p, odd, 128, 128) == -1 and b"aligned" in dll.jck_last_error()
    assert up(odd, p, 128, 128) == -1 and b"aligned" in dll.jck_last_error()
    for cs, cb in ((128, 32), (128, 96), (32, 128), (128, 4), (96, 128)):
        assert up(p, p, cs, cb) == -1 and b"powers of two" in dll.jck_last_error(), (cs, cb)
    assert up(p, p, 128, 128, 0) == -1
    assert dll.jck_leaky_affine_bwd(1, p, p, p, 0.2, p, 4, 12, None) == -1 and b"power of two" in dll.jck_last_error()
    assert dll.jck_leaky_affine_bwd(1, p, p, p, 0.2, p, 4, 4, None) == -1
    assert dll.jck_leaky_affine_bwd(1, p, None, p, 0.2, p, 4, 64, None) == -1
    assert dll.jck_leaky_affine_bwd(1, p, p, odd, 0.2, p, 4, 64, None) == -1 and b"aligned" in dll.jck_last_error()
    assert dll.jck_leaky_affine_bwd(1, p, p, p, 0.2, p, 0, 64, None) == -1
    assert dll.jck_critic_ds(p, 0, 1.0, 4, p, p, None) == -1 and b"mode" in dll.jck_last_error()
    assert dll.jck_critic_ds(p, 3, 1.0, 4, p, p, None) == -1
    assert dll.jck_critic_ds(None, 1, 1.0, 4, p, p, None) == -1 and dll.jck_critic_ds(p, 1, 1.0, 0, p, p, None) == -1
    assert dll.jck_latent_loss_ex(1, p, None, None, None, p, p, 1, 64, None) == -1 and b"g_x" in dll.jck_last_error()
    assert dll.jck_latent_loss_ex(1, p, p, None, odd, p, p, 1, 64, None) == -1 and b"aligned" in dll.jck_last_error()
    assert dll.jck_latent_loss_ex(1, None, p, None, None, p, p, 1, 64, None) == -1
    assert dll.jck_engine_latent_grad_ex(None, p, None, p, None, 1, 0.003, 1, p, p, p, p, None) == -1 and b"not bound" in dll.jck_last_error()
    assert dll.jck_engine_project_ex(None, p, None, p, 1, 1, 0.05, 0.0, None, 1, 0.003, p, p, 0, p, p, None) == -1 and b"not bound" in dll.jck_last_error()
