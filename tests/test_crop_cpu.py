"""Centre and random crops in front of the resize, host side: the host statement and the tap tables of the box against what Pillow
returns for crop().resize() (tests/golden/crop_resize_u8.json), the centre formula, the command-line flags, the host preprocessor, the
loader's draws, the launcher's refusals and the LDS sizing.  No GPU."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest
import torch

from crop_ref import CASES, CENTRED, case_inputs, case_name, gold, host_crop_resize, ids, reference
from resize_any_ref import apply_taps, check, normalized, split_table, taps_table

E_ARG = -1


@pytest.mark.parametrize("case", CASES, ids=ids())
def test_host_statement_and_tap_tables_reproduce_pillow(case):
    hs, ws, hc, wc, y0, x0, s, n = case
    x, _ = reference(*case)                                                  # resize_pil_u8 of the slice, checked against the fixture inside
    t = taps_table(hc, wc, s)                                                # the unchanged table builder, for the BOX's geometry
    assert tuple(int(v) for v in t[1:4]) == (hc, wc, s)
    check(apply_taps(np.ascontiguousarray(x[:, :, y0:y0 + hc, x0:x0 + wc]), t, s), gold()["cases"][case_name(*case[:7])])


def test_fixture_is_complete():
    g = gold()
    assert g["pillow"].startswith("12.2") and list(g["cases"]) == ids() and len(CASES) == 10
    for *c, n in CASES:
        rec = g["cases"][case_name(*c)]
        assert rec["n"] == n == (2 if c[0] == 512 else 4) and len(rec["samples"]) == 60
    assert sorted(k for k, v in g["cases"].items() if "full_zlib_b64" in v) == sorted(case_name(*c) for c in ((5, 7, 1, 1, 4, 6, 64), (5, 7, 3, 2, 1, 5, 64)))
    assert case_inputs(48, 48, 41, 41, 7, 7, 64, 4).shape == (4, 3, 48, 48) and 7 + 41 == 48      # the box that ends on the last byte


def test_center_formula():
    from preprocess.dcgan_data_preprocessor import center_origin
    assert center_origin(125, 107, 100, 100) == (12, 4) and center_origin(140, 100, 100, 100) == (20, 0)     # differences 25, 7, 40, 0
    assert center_origin(50, 40, 37, 37) == (6, 2) and center_origin(38, 42, 37, 37) == (0, 2)                # 13 -> 6, 3 -> 2, 1 -> 0, 5 -> 2
    for hs, ws, hc, wc, y0, x0, s in CENTRED:                                                      # the fixture's centred cases
        assert center_origin(hs, ws, hc, wc) == (y0, x0)


# ---- command line ----------------------------------------------------------------------------------------------------------
def test_new_flags_add_only_their_own_key(capsys):
    import main
    today = {"test": 0, "model_path": "", "log_file": 1, "model": main.ModelEnum.DCGAN, "num_worker": 0, "batch_size": 128,
             "epoch": 100, "max_learning_rate": 0.1, "min_learning_rate": 1e-4, "weight_decay": 5e-4, "nesterov": 1}
    assert vars(main.get_arg_parse([])) == today
    assert vars(main.get_arg_parse(["--crop", "center"])) == {**today, "crop": "center"}
    assert vars(main.get_arg_parse(["--crop", "random", "--crop_size", "28"])) == {**today, "crop": "random", "crop_size": 28}
    for bad in (["--crop_size", "28"], ["--crop", "diagonal"]):
        with pytest.raises(SystemExit):
            main.get_arg_parse(bad)
    assert "--crop" in capsys.readouterr().err
    cg = vars(main.get_arg_parse(["-m", "CGAN", "--crop", "random", "--crop_size", "28"]))
    assert cg["crop"] == "random" and cg["crop_size"] == 28


# ---- the host preprocessor --------------------------------------------------------------------------------------------------
def _args(**kw):
    return argparse.Namespace(batch_size=3, num_worker=0, log_file=0, save_path=".", **kw)


def _npz(path, x, labels=None):
    arrays = {"images": np.ascontiguousarray(x.transpose(0, 2, 3, 1))}
    if labels is not None:
        arrays["labels"] = np.asarray(labels)
    np.savez(path, **arrays)
    return str(path)


@pytest.mark.parametrize("model", ["dcgan", "cgan"])
def test_host_preprocessor_center(model, tmp_path, monkeypatch):
    from preprocess.cgan_data_preprocessor import CGANDataPreprocessor
    from preprocess.dcgan_data_preprocessor import DCGANDataPreprocessor
    monkeypatch.setenv("JCKGAN_DEVICE_DATA", "0")
    case = (100, 75, 75, 75, 12, 0, 64, 4)
    x, y = reference(*case)
    labels = [7, 0, 99, 7]
    path = _npz(tmp_path / "d.npz", x, labels if model == "cgan" else None)
    cls = CGANDataPreprocessor if model == "cgan" else DCGANDataPreprocessor
    pre = cls(_args(data=path, crop="center"))
    assert pre.crop_size == 75                                                        # K defaults to min(Hs, Ws)
    loader, metric_src = pre.get_data_loader()
    assert metric_src.images.dtype == torch.uint8 and tuple(metric_src.images.shape) == (4, 3, 75, 75)
    assert torch.equal(metric_src.images, torch.from_numpy(x[:, :, 12:87, 0:75].copy()))
    want = normalized(y)
    seen = torch.zeros(4, dtype=torch.bool)
    for batch in loader:
        assert batch[0].shape[1:] == (3, 64, 64) and batch[0].dtype == torch.float32
        for b in range(batch[0].shape[0]):
            which = [i for i in range(4) if torch.equal(batch[0][b], want[i])]
            assert which, "a batch image is none of the fixture's transformed images"
            seen[which] = True
    assert bool(seen.all())
    # the real-feature cache carries the crop: not the uncropped name, and another name for another size
    plain, k75, k40 = cls(_args(data=path)).metric_cache, pre.metric_cache, cls(_args(data=path, crop="center", crop_size=40)).metric_cache
    assert len({plain, k75, k40}) == 3 and "crop75" in os.path.basename(k75) and "crop40" in os.path.basename(k40)
    assert cls(_args(data=path, crop="random", crop_size=40)).metric_cache == k40      # evaluation reads the centre box in both modes


def test_host_preprocessor_refusals(tmp_path, monkeypatch):
    from preprocess.dcgan_data_preprocessor import DCGANDataPreprocessor
    monkeypatch.setenv("JCKGAN_DEVICE_DATA", "0")
    path = _npz(tmp_path / "d.npz", case_inputs(100, 75, 75, 75, 12, 0, 64, 4))
    pre = DCGANDataPreprocessor(_args(data=path, crop="random", crop_size=40))
    with pytest.raises(ValueError, match="crop.*device-resident"):
        pre.transform_data()
    for k in (76, 0, -3):
        with pytest.raises(ValueError, match="crop_size"):
            DCGANDataPreprocessor(_args(data=path, crop="center", crop_size=k))
    with pytest.raises(ValueError):
        DCGANDataPreprocessor(_args(data=path, crop_size=40))
    with pytest.raises(ValueError):
        DCGANDataPreprocessor(_args(data=path, crop="diagonal"))
    small = DCGANDataPreprocessor(_args(data=path, crop="center", crop_size=1))
    small.transform_data()
    assert tuple(small._metric.images.shape) == (4, 3, 1, 1) and tuple(small._train.shape) == (4, 3, 64, 64)


def test_cifar_sized_data_takes_a_crop_too(monkeypatch):
    """--crop center --crop_size 28 on 32x32 images (the synthetic stand-in for CIFAR), 64 and 128: the fixture's geometry is (3, 1);
    the centred one is (2, 2), so compare with the host statement on that slice"""
    from preprocess.dcgan_data_preprocessor import DCGANDataPreprocessor
    monkeypatch.setenv("JCKGAN_DEVICE_DATA", "0")
    for size in (64, 128):
        pre = DCGANDataPreprocessor(_args(crop="center", crop_size=28, **({"image_size": 128} if size == 128 else {})), synthetic_size=6)
        pre.transform_data()
        assert os.path.basename(pre.metric_cache) == "metric_data_crop28.pikl"
        want = normalized(host_crop_resize(pre.images.numpy(), 28, 28, 2, 2, size))
        assert torch.equal(pre._train, want) and tuple(pre._metric.images.shape) == (6, 3, 28, 28)


# ---- the loader's draws -----------------------------------------------------------------------------------------------------
def _loader(n=41, world=1, rank=0, **kw):
    from preprocess.dcgan_data_preprocessor import DeviceLoader
    ld = DeviceLoader(torch.zeros(n, 3, 48, 56, dtype=torch.uint8), 16, seed=7, **kw)
    ld.rank, ld.world, ld.n_local = rank, world, (n + world - 1) // world
    return ld


def test_device_loader_draws():
    plain, mirror, crop = _loader(), _loader(mirror=True), _loader(mirror=True, crop="random", crop_size=40)
    assert (plain.crop_size, crop.crop_size, _loader(crop="center").crop_size) == (None, 40, 48)
    epochs = []
    for _ in range(2):
        (p0, f0, o0), (p1, f1, o1), (p2, f2, o2) = plain.draw_epoch(), mirror.draw_epoch(), crop.draw_epoch()
        assert torch.equal(p0, p1) and torch.equal(p1, p2) and torch.equal(f1, f2)          # the same order and flips with and without
        assert f0 is None and o0 is None and o1 is None
        assert o2.dtype == torch.int32 and tuple(o2.shape) == (41, 2)
        assert 0 <= int(o2[:, 0].min()) and int(o2[:, 0].max()) <= 48 - 40 and 0 <= int(o2[:, 1].min()) and int(o2[:, 1].max()) <= 56 - 40
        epochs.append((p2, o2))
    assert len(set(epochs[0][1][:, 0].tolist())) > 1 and len(set(epochs[0][1][:, 1].tolist())) > 1
    a, b = (o[torch.argsort(p)] for p, o in epochs)
    assert not torch.equal(a, b)                                                             # an image's origin differs between epochs
    again = _loader(mirror=True, crop="random", crop_size=40)                                # reproducible for a seed
    for p, o in epochs:
        p3, _, o3 = again.draw_epoch()
        assert torch.equal(p, p3) and torch.equal(o, o3)
    full = _loader(crop="random", crop_size=48).draw_epoch()[2]                              # no room on y: every y0 is 0
    assert int(full[:, 0].abs().max()) == 0 and int(full[:, 1].max()) <= 8
    for bad in (dict(crop="random", crop_size=49), dict(crop="center", crop_size=0), dict(crop_size=40), dict(crop="diagonal")):
        with pytest.raises(ValueError):
            _loader(**bad)


def test_device_loader_shares_of_two_ranks_are_the_strided_ones():
    kw = dict(mirror=True, crop="random", crop_size=40)
    p, f, o = _loader(**kw).draw_epoch()
    total = 42                                                                               # 41 images padded by wrap-around
    for rank in (0, 1):
        pr, fr, orr = _loader(world=2, rank=rank, **kw).draw_epoch()
        for got, whole in ((pr, p), (fr, f), (orr, o)):
            assert torch.equal(got, torch.cat([whole, whole[:total - 41]])[rank:total:2])
        assert pr.numel() == 21 and tuple(orr.shape) == (21, 2)


# ---- the launcher without a device ----------------------------------------------------------------------------------------
def test_box_launcher_refuses_on_the_host():
    from hipgan import _lib
    dll = _lib.load_library()
    buf = (C.c_int * 64)()                      # stands for device memory: a refusal comes before any device call
    p = C.addressof(buf)

    def call(data=p, taps=p, origin=None, b=4, hs=48, ws=48, hc=48, wc=48, y0=0, x0=0, s=64, prec=1):
        return dll.jck_img_prep_u8_box(prec, data, None, None, origin, None, None, 0, 1.0, 0.0, None, p, b, hs, ws, hc, wc, y0, x0, s, taps, None)
    for kw in (dict(data=None), dict(taps=None), dict(s=96), dict(b=0), dict(hc=49), dict(wc=49), dict(hc=0), dict(y0=1), dict(x0=1),
               dict(hc=40, y0=9), dict(wc=40, x0=-1), dict(hs=2000, hc=40), dict(ws=2000), dict(prec=7), dict(taps=p + 1), dict(origin=p + 2)):
        assert call(**kw) == E_ARG and dll.jck_last_error(), kw
    assert b"box" in dll.jck_last_error()


def test_one_band_always_fits_the_lds():
    """The launchers' sizing for every box height up to 1024 and both output sizes: the band's rows after the horizontal pass stay
    within 64 KiB, the band divides the output, and the rows cover what the band's vertical taps touch."""
    from hipgan import _lib
    dll = _lib.load_library()
    band, rows = C.c_int(), C.c_int()
    for s in (64, 128):
        for hc in range(1, 1025):
            nbytes = dll.jck_resize_lds_bytes(hc, s, C.byref(band), C.byref(rows))
            assert 0 < nbytes <= 65536 and nbytes == rows.value * 3 * s, (hc, s, nbytes)
            assert band.value in (1, 2, 4, 8, 16) and 1 <= rows.value <= hc
            if hc % 37 == 1 or hc in (2, 63, 64, 65, 127, 128, 129, 1023, 1024):
                (_, _, _), (ylo, ycnt, _) = split_table(taps_table(hc, 1, s), s)
                b = band.value
                need = max(int(ylo[y + b - 1] + ycnt[y + b - 1] - ylo[y]) for y in range(0, s, b))
                assert need <= rows.value, (hc, s, b, need, rows.value)
    assert dll.jck_resize_lds_bytes(0, 64, None, None) == E_ARG and dll.jck_resize_lds_bytes(1025, 64, None, None) == E_ARG
    assert dll.jck_resize_lds_bytes(4, 96, None, None) == E_ARG and dll.jck_last_error()
    assert dll.jck_resize_lds_bytes(178, 64, None, None) == (16 * 178 // 64 + 2 * 3 + 2) * 3 * 64
