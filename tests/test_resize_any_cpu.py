"""Any-size input pipeline, host side: the tap tables of jck_resize_taps_build and the host statement resize_pil_u8 against what
Pillow returns (tests/golden/resize_any_u8.json), the new command-line flags, the --data loader and its refusals.  No GPU."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest
import torch

from resize_any_ref import CASES, apply_taps, case_inputs, case_name, check, gold, normalized, reference, taps_table

E_ARG, LIMIT = -1, 1024


@pytest.mark.parametrize("h,w,s,n", CASES, ids=[case_name(*c[:3]) for c in CASES])
def test_tap_tables_reproduce_pillow(h, w, s, n):
    """jck_resize_taps_build (pure host), applied in numpy as two rounded passes, gives Pillow's bytes"""
    t = taps_table(h, w, s)
    assert tuple(int(v) for v in t[1:4]) == (h, w, s)
    check(apply_taps(case_inputs(h, w, s, n), t, s), gold()["cases"][case_name(h, w, s)])


def test_tap_entry_points_refuse_unsupported_geometries():
    from hipgan import _lib
    dll = _lib.load_library()
    buf = (C.c_int * 65536)()
    for hs, ws, s in ((32, 32, 96), (0, 32, 64), (32, 0, 64), (LIMIT + 1, 32, 64), (32, LIMIT + 1, 128)):
        assert dll.jck_resize_taps_bytes(hs, ws, s) == E_ARG and dll.jck_last_error(), (hs, ws, s)
        assert dll.jck_resize_taps_build(hs, ws, s, buf) == E_ARG and dll.jck_last_error(), (hs, ws, s)
        assert not any(buf[:64])                                        # nothing written
    assert dll.jck_resize_taps_build(32, 32, 64, None) == E_ARG
    # the limit itself is served, and the size is the documented one: header + per axis (2 + K) * S words, K = 2 * ceil(L / S) + 1
    assert dll.jck_resize_taps_bytes(LIMIT, LIMIT, 64) == 4 * (8 + 2 * 64 * (2 + 33))
    assert dll.jck_resize_taps_bytes(32, 32, 64) == 4 * (8 + 2 * 64 * (2 + 3))
    assert dll.jck_resize_taps_bytes(1, LIMIT, 128) == 4 * (8 + 128 * (2 + 17) + 128 * (2 + 3))
    from hipgan import JckError
    from hipgan.engine import resize_taps_host
    with pytest.raises(JckError):
        resize_taps_host(32, 32, 96)


@pytest.mark.parametrize("h,w,s,n", CASES, ids=[case_name(*c[:3]) for c in CASES])
def test_host_resize_matches_pillow(h, w, s, n):
    reference(h, w, s, n)                       # resize_pil_u8 on the case's inputs, checked against the fixture inside


def test_host_resize_matches_live_pillow_on_random_geometries():
    try:
        from make_golden_resize_any import pil_resize
        import PIL  # noqa: F401
    except Exception:
        pytest.skip("Pillow not installed")
    from preprocess.dcgan_data_preprocessor import resize_pil_u8
    rs = np.random.RandomState(20)
    for _ in range(20):
        h, w, s = int(rs.randint(1, 301)), int(rs.randint(1, 301)), int(rs.choice([64, 128]))
        x = rs.randint(0, 256, size=(2, 3, h, w)).astype(np.uint8)
        want = np.stack([pil_resize(img, s) for img in x])
        assert np.array_equal(resize_pil_u8(torch.from_numpy(x), s).numpy(), want), (h, w, s)
        assert np.array_equal(apply_taps(x, taps_table(h, w, s), s), want), (h, w, s)


def test_host_resize_at_2x_is_the_existing_one():
    from preprocess.dcgan_data_preprocessor import resize2x_pil_u8, resize_pil_u8
    x = torch.from_numpy(case_inputs(32, 32, 64, 4))
    assert torch.equal(resize_pil_u8(x, 64), resize2x_pil_u8(x))
    r = torch.randint(0, 256, (5, 3, 32, 32), generator=torch.Generator().manual_seed(3), dtype=torch.uint8)
    assert torch.equal(resize_pil_u8(r, 64), resize2x_pil_u8(r))


# ---- command line ----------------------------------------------------------------------------------------------------------
def test_new_flags_add_only_their_own_key():
    import main
    today = {"test": 0, "model_path": "", "log_file": 1, "model": main.ModelEnum.DCGAN, "num_worker": 0, "batch_size": 128,
             "epoch": 100, "max_learning_rate": 0.1, "min_learning_rate": 1e-4, "weight_decay": 5e-4, "nesterov": 1}
    assert vars(main.get_arg_parse([])) == today
    assert vars(main.get_arg_parse(["--data", "faces.npz"])) == {**today, "data": "faces.npz"}
    assert vars(main.get_arg_parse(["--image_size", "128"])) == {**today, "image_size": 128}
    assert vars(main.get_arg_parse(["--image_size", "64"])) == {**today, "image_size": 64}
    assert vars(main.get_arg_parse(["--mirror", "1"])) == {**today, "mirror": 1}
    for bad in (["--image_size", "96"], ["--mirror", "2"]):
        with pytest.raises(SystemExit):
            main.get_arg_parse(bad)


def test_cgan_refuses_image_size_128_at_parse_time(capsys):
    import main
    with pytest.raises(SystemExit):
        main.get_arg_parse(["-m", "CGAN", "--image_size", "128"])
    assert "DCGAN only" in capsys.readouterr().err
    assert main.get_arg_parse(["-m", "CGAN", "--image_size", "64"]).image_size == 64


# ---- --data: loader, host path ---------------------------------------------------------------------------------------------
def _args(**kw):
    return argparse.Namespace(batch_size=3, num_worker=0, log_file=0, save_path=".", **kw)


def _npz(path, h, w, s, n, labels=None):
    x = case_inputs(h, w, s, n)
    arrays = {"images": np.ascontiguousarray(x.transpose(0, 2, 3, 1))}
    if labels is not None:
        arrays["labels"] = np.asarray(labels)
    np.savez(path, **arrays)
    return str(path)


@pytest.mark.parametrize("model,h,w,s", [("dcgan", 100, 75, 64), ("dcgan", 37, 50, 128), ("cgan", 5, 7, 64)])
def test_preprocessor_feeds_the_fixture_transform_from_an_npz(model, h, w, s, tmp_path, monkeypatch):
    from preprocess.cgan_data_preprocessor import CGANDataPreprocessor
    from preprocess.dcgan_data_preprocessor import DCGANDataPreprocessor
    monkeypatch.setenv("JCKGAN_DEVICE_DATA", "0")
    n = 4
    labels = [7, 0, 99, 7]
    path = _npz(tmp_path / "d.npz", h, w, s, n, labels if model == "cgan" else None)
    size = {"image_size": s} if s != 64 else {}
    pre = (CGANDataPreprocessor if model == "cgan" else DCGANDataPreprocessor)(_args(data=path, **size))
    assert tuple(pre.images.shape) == (n, 3, h, w) and pre.images.dtype == torch.uint8       # planar, as the CIFAR data is kept
    assert os.path.basename(pre.metric_cache) != "metric_data.pikl" and "d_" in os.path.basename(pre.metric_cache)
    loader, metric_src = pre.get_data_loader()
    assert len(metric_src) == n and list(metric_src.targets) == (labels if model == "cgan" else [0] * n)
    want = normalized(reference(h, w, s, n)[1])
    seen = torch.zeros(n, dtype=torch.bool)
    for batch in loader:
        assert batch[0].shape[1:] == (3, s, s) and batch[0].dtype == torch.float32
        for b in range(batch[0].shape[0]):
            which = [i for i in range(n) if torch.equal(batch[0][b], want[i])]
            assert which, "a batch image is none of the fixture's transformed images"
            seen[which] = True
            if model == "cgan":
                assert batch[1].dtype == torch.int64 and int(batch[1][b].argmax()) in [labels[i] for i in which] and int(batch[1][b].sum()) == 1
    assert bool(seen.all())


def test_malformed_data_files_are_refused(tmp_path, monkeypatch):
    from preprocess.cgan_data_preprocessor import CGANDataPreprocessor
    from preprocess.dcgan_data_preprocessor import DCGANDataPreprocessor, load_npz_dataset
    monkeypatch.setenv("JCKGAN_DEVICE_DATA", "0")
    img = np.zeros((4, 8, 8, 3), np.uint8)
    bad = {"no_images": {"pictures": img}, "float": {"images": img.astype(np.float32)}, "planar": {"images": img.transpose(0, 3, 1, 2)},
           "rank": {"images": img[0]}, "empty": {"images": img[:0]}, "too_large": {"images": np.zeros((1, 2, 1025, 3), np.uint8)},
           "label_shape": {"images": img, "labels": np.zeros(3, np.int64)}, "label_dtype": {"images": img, "labels": np.zeros(4, np.float32)},
           "label_rank": {"images": img, "labels": np.zeros((4, 1), np.int64)}}
    for name, arrays in bad.items():
        path = str(tmp_path / f"{name}.npz")
        np.savez(path, **arrays)
        with pytest.raises(ValueError):
            load_npz_dataset(path)
        with pytest.raises(ValueError):
            DCGANDataPreprocessor(_args(data=path))
    ok = str(tmp_path / "ok.npz")
    np.savez(ok, images=img)
    assert load_npz_dataset(ok)[1] is None and tuple(load_npz_dataset(ok)[0].shape) == (4, 3, 8, 8)
    with pytest.raises(ValueError):                                     # the conditional model needs labels ...
        CGANDataPreprocessor(_args(data=ok))
    for labels in ([0, 1, 2, 100], [-1, 1, 2, 3]):                      # ... all of them classes it has
        path = str(tmp_path / "range.npz")
        np.savez(path, images=img, labels=np.asarray(labels))
        with pytest.raises(ValueError):
            CGANDataPreprocessor(_args(data=path))
        assert load_npz_dataset(path)[1] == labels                      # DCGAN takes them as they are
    with pytest.raises(FileNotFoundError):
        DCGANDataPreprocessor(_args(data=str(tmp_path / "missing.npz")))
    with pytest.raises(ValueError):
        DCGANDataPreprocessor(_args(data=ok, image_size=96))


def test_mirror_on_the_host_path_is_refused(tmp_path, monkeypatch):
    from preprocess.dcgan_data_preprocessor import DCGANDataPreprocessor
    monkeypatch.setenv("JCKGAN_DEVICE_DATA", "0")
    path = _npz(tmp_path / "d.npz", 5, 7, 64, 4)
    pre = DCGANDataPreprocessor(_args(data=path, mirror=1))
    with pytest.raises(ValueError, match="mirror"):
        pre.transform_data()
    DCGANDataPreprocessor(_args(data=path, mirror=0)).transform_data()
