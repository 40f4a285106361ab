"""Discriminator features, host side (no GPU): the column layout, the k-NN vote, the block normalisation, generate.py's argument
checks for --features / --probe / --space, and the C ABI of jck_grid_pool, jck_engine_feature_dim and jck_engine_features (declared,
exported, not enumerated by jck_launch_name, argument errors before any device call)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from hipgan import JckError
from hipgan.probe import feature_layout, knn_vote, load_images, normalise_blocks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("size,chans,heights", [(64, (64, 128, 256, 512), (32, 16, 8, 4)), (128, (64, 128, 256, 512, 1024), (64, 32, 16, 8, 4))])
@pytest.mark.parametrize("grid", [1, 2, 4])
def test_feature_layout(size, chans, heights, grid):
    layout, F = feature_layout(size, grid)
    assert [b[0] for b in layout] == list(range(len(chans)))
    assert tuple(b[2] for b in layout) == chans and tuple(b[3] for b in layout) == heights
    col0 = 0
    for (_, c0, c, h) in layout:
        assert c0 == col0 and h % grid == 0 and c0 % 4 == 0
        col0 += grid * grid * c
    assert F == col0 == grid * grid * sum(chans)
    assert F == {64: 960, 128: 1984}[size] * grid * grid


def test_feature_layout_numbers_and_refusals():
    assert feature_layout(64, 4)[1] == 15360 and feature_layout(64, 1)[1] == 960 and feature_layout(128, 4)[1] == 31744
    assert feature_layout(64, 4)[0] == [(0, 0, 64, 32), (1, 1024, 128, 16), (2, 3072, 256, 8), (3, 7168, 512, 4)]
    for size, grid in ((64, 3), (64, 0), (64, 8), (32, 4), (96, 2)):
        with pytest.raises(JckError):
            feature_layout(size, grid)


def test_knn_vote():
    labels = np.array([0, 0, 1, 1, 2, 2, 2])
    idx = np.array([[2, 0, 1],        # 1, 0, 0: a plain majority, not the nearest neighbour's class
                    [2, 0, 4],        # 1, 0, 2: a three-way tie goes to the nearest
                    [0, 2, 3],        # 0, 1, 1
                    [4, 0, 1],        # 2, 0, 0
                    [5, -1, -1],      # one neighbour
                    [-1, -1, -1],     # none
                    [0, 3, -1]])      # 0, 1: a tie between two, the missing entry ignored
    assert knn_vote(idx, labels, 3).tolist() == [0, 1, 1, 0, 2, -1, 0]
    # a tie between two classes of two members each goes to the one whose FIRST member is nearest, wherever its second one lies
    assert knn_vote(np.array([[2, 0, 1, 3], [0, 2, 3, 1], [4, 2, 3, 5]]), labels, 3).tolist() == [1, 0, 2]
    # -1 entries between valid ones are ignored too, and do not count for class 0
    assert knn_vote(np.array([[-1, 2, -1, 3, 0]]), labels, 3).tolist() == [1]
    assert knn_vote(np.zeros((0, 3), np.int64), labels, 3).shape == (0,)
    assert knn_vote(idx, labels, 3).dtype == np.int64
    with pytest.raises(JckError):
        knn_vote(idx, labels, 2)


def test_normalise_blocks():
    layout, F = feature_layout(64, 1)
    g = torch.Generator().manual_seed(3)
    f = torch.randn(5, F, generator=g) * torch.tensor([1.0, 10.0, 0.01, 3.0, 1.0]).view(5, 1)
    f[1, 64:192] = 0.0                       # a zero block
    f[2, 100] = float("nan")                 # a NaN in row 2's second block
    f[3, 300] = float("inf")                 # an inf in row 3's third block
    keep = f.clone()
    out = normalise_blocks(f, layout)
    assert torch.equal(torch.nan_to_num(f), torch.nan_to_num(keep)) and out.shape == f.shape and out.dtype == torch.float32
    for r in range(5):
        for (_, c0, c, _) in layout:
            b, src = out[r, c0:c0 + c], keep[r, c0:c0 + c]
            if (r, c0) == (1, 64):
                assert bool((b == 0).all())
            elif (r, c0) in ((2, 64), (3, 192)):
                assert not bool(torch.isfinite(b).all())
            else:
                assert abs(float(b.double().norm()) - 1.0) < 1e-6
                assert torch.allclose(b, src / torch.linalg.vector_norm(src), rtol=1e-6, atol=0)
    # the same at grid 2: the blocks are four times as wide
    layout2, F2 = feature_layout(64, 2)
    out2 = normalise_blocks(torch.ones(2, F2), layout2)
    for (_, c0, c, _) in layout2:
        assert torch.allclose(out2[:, c0:c0 + 4 * c].norm(dim=1), torch.ones(2), atol=1e-6)
    with pytest.raises(JckError):
        normalise_blocks(torch.ones(2, 961), layout)


def _npz(path, n=4, size=32, labels=True):
    arrays = {"images": np.zeros((n, size, size, 3), np.uint8)}
    if labels:
        arrays["labels"] = np.arange(n, dtype=np.int64)
    np.savez(path, **arrays)
    return str(path)


def test_cli_validation(tmp_path, capsys):
    import generate
    base = ["-m", "DCGAN", "--checkpoint", str(tmp_path / "none.pt"), "--out", str(tmp_path / "out")]
    a = generate.get_arg_parse(base)
    assert (a.k, a.space, a.feature_grid, a.feature_pool, a.features, a.probe) == (4, "pixel", 4, "max", None, None)
    assert not generate.needs_discriminator(a)
    for extra, word in ((["--space", "d"], "--neighbours"), (["--probe", "a.npz"], "--probe_test"), (["--probe_test", "a.npz"], "--probe"),
                        (["--feature_grid", "2"], "--feature_grid"), (["--features", "a.npz", "--feature_grid", "3"], "--feature_grid"),
                        (["--features", "a.npz", "--num", "4"], "--features"), (["--features", "a.npz", "--probe", "a.npz", "--probe_test", "b.npz"], "separate"),
                        (["--probe", "a.npz", "--probe_test", "b.npz", "--k", "9"], "--k")):
        with pytest.raises(SystemExit):
            generate.get_arg_parse(base + extra)
        assert word in capsys.readouterr().err, extra
    a = generate.get_arg_parse(base + ["--probe", "a.npz", "--probe_test", "b.npz"])
    assert a.k == 5 and generate.needs_discriminator(a)
    a = generate.get_arg_parse(base + ["--neighbours", "r.npz", "--space", "d", "--feature_pool", "mean"])
    assert a.k == 4 and a.space == "d" and a.feature_pool == "mean" and generate.needs_discriminator(a)
    assert not generate.needs_discriminator(generate.get_arg_parse(base + ["--neighbours", "r.npz"]))
    assert generate.needs_discriminator(generate.get_arg_parse(base + ["--features", "a.npz"]))
    # a probe file without labels ends the run before a checkpoint is read or an engine exists
    good, bad = _npz(tmp_path / "good.npz"), _npz(tmp_path / "bad.npz", labels=False)
    for train, test in ((good, bad), (bad, good)):
        with pytest.raises(JckError, match="labels"):
            generate.main(base + ["--probe", train, "--probe_test", test])
    np.savez(tmp_path / "short.npz", images=np.zeros((4, 32, 32, 3), np.uint8), labels=np.arange(3))
    with pytest.raises(JckError, match="3 labels for 4 images"):
        generate.main(base + ["--probe", good, "--probe_test", str(tmp_path / "short.npz")])
    np.savez(tmp_path / "noimg.npz", labels=np.arange(3))
    with pytest.raises(JckError, match="images"):
        generate.main(base + ["--features", str(tmp_path / "noimg.npz")])
    u8, lab = load_images(good, need_labels=True)
    assert u8.shape == (4, 32, 32, 3) and lab.tolist() == [0, 1, 2, 3] and load_images(bad)[1] is None


def test_small_pictures_are_upscaled_as_the_trainers_do():
    from hipgan.probe import _to_size
    from preprocess.dcgan_data_preprocessor import resize2x_pil_u8
    x = torch.randint(0, 256, (3, 32, 32, 3), generator=torch.Generator().manual_seed(5), dtype=torch.uint8)
    y = _to_size(x, 64, "images")
    assert y.shape == (3, 64, 64, 3) and y.dtype == torch.uint8
    assert torch.equal(y.permute(0, 3, 1, 2), resize2x_pil_u8(x.permute(0, 3, 1, 2)))
    assert _to_size(y, 64, "images") is y or torch.equal(_to_size(y, 64, "images"), y)
    assert _to_size(x, 128, "images").shape == (3, 128, 128, 3)
    with pytest.raises(JckError, match="not reachable"):
        _to_size(torch.zeros(1, 48, 48, 3, dtype=torch.uint8), 64, "images")


def _dll():
    from hipgan import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib, _lib.load_library()


def test_abi_declares_and_exports_the_entry_points():
    _lib, dll = _dll()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jckgan.h")).read(), flags=re.S)
    for name, ret, nargs in (("jck_grid_pool", "int", 11), ("jck_engine_feature_dim", r"long\s+long", 2), ("jck_engine_features", "int", 8)):
        m = re.search(r"\b" + ret + r"\s+" + name + r"\s*\(([^;]*)\)\s*;", src)
        assert m, f"{name} is not declared in include/jckgan.h"
        assert len(m.group(1).split(",")) == nargs == len(_lib.PROTOS[name][1]), name
        assert hasattr(dll, name), f"{name} is not exported"
    assert _lib.PROTOS["jck_engine_feature_dim"][0] is C.c_longlong
    names = []
    while dll.jck_launch_name(len(names)):
        names.append(dll.jck_launch_name(len(names)))
    assert len(names) == 38 and not any(b"pool" in n for n in names)          # the new kernel is not enumerated


def test_entry_points_fail_on_the_host_without_a_device():
    """argument errors come back as JCK_E_ARG with a message before any device call"""
    _, dll = _dll()
    buf = (C.c_float * 4096)()
    base = C.cast(buf, C.c_void_p).value
    p = C.c_void_p((base + 15) // 16 * 16)
    odd = C.c_void_p(p.value + 4)
    pool = lambda a=p, n=1, h=8, c=64, grid=4, mode=0, out=p, ld=1024 + 24, col0=8, prec=1: dll.jck_grid_pool(prec, a, n, h, c, grid, mode, out, ld, col0, None)
    for kw, word in ((dict(grid=3), b"grid"), (dict(grid=8), b"grid"), (dict(grid=0), b"grid"), (dict(h=6), b"multiple of grid"), (dict(c=12), b"multiple of 8"),
                     (dict(c=0), b"multiple of 8"), (dict(a=None), b"null"), (dict(out=None), b"null"), (dict(a=odd), b"aligned"), (dict(out=odd), b"aligned"),
                     (dict(col0=6), b"aligned"), (dict(n=2, ld=1024 + 26), b"aligned"), (dict(col0=-4), b"column block"), (dict(ld=1024), b"column block"),
                     (dict(mode=2), b"mode"), (dict(n=0), b"N >= 1"), (dict(prec=7), b"bad prec")):
        assert pool(**kw) == -1, kw
        err = dll.jck_last_error()
        assert b"grid_pool" in err and word in err, (kw, err)
    assert dll.jck_engine_feature_dim(None, 4) == 0
    assert dll.jck_engine_features(None, p, 1, 4, 0, p, 15360, None) == -1 and b"not bound" in dll.jck_last_error()
