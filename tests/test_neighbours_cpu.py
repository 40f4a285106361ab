"""Host side of the nearest-neighbour feature (no GPU): the numpy path of metrics.nearest against the brute-force reference, the
workspace size, the generate CLI's --neighbours arguments, the row layout of its picture and the errors of its reference file."""
import os
import sys

import numpy as np
import pytest
import torch

from neighbours_ref import knn_ref, merge_ref
from pairstats_ref import int_features, recipe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "jck-generation_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(np.asarray(got[1], np.float64), want[1], equal_nan=True)


def test_numpy_path_matches_brute_force_with_ties_and_edges():
    import metrics
    g = np.random.default_rng(1)
    pats = g.integers(-3, 4, size=(4, 20)).astype(np.float32)
    ref = np.concatenate([pats[g.integers(0, 4, size=200)], int_features(133, 20, seed=2)])        # exact ties, the lower index wins
    q = np.concatenate([pats, int_features(61, 20, seed=3)])
    for k in (1, 3, 8):
        got = metrics.nearest(q, ref, k)
        assert got[0].dtype == np.int64 and got[0].shape == (65, k) and same(got, knn_ref(q, ref, k))
        assert same(metrics.nearest(torch.as_tensor(q), ref, k), knn_ref(q, ref, k))                # a host tensor takes the numpy path too
        assert same(metrics.nearest(ref, ref, k, exclude_self=True), knn_ref(ref, ref, k, exclude_self=True))
    got = metrics.nearest(q, ref[:3], 8)                                                              # a -1 / +inf tail
    assert same(got, knn_ref(q, ref[:3], 8)) and (got[0][:, 3:] == -1).all() and np.isposinf(got[1][:, 3:]).all()
    got = metrics.nearest(q[:1], q[:1], 2, exclude_self=True)
    assert (got[0] == -1).all() and np.isposinf(got[1]).all()
    for bad in (np.nan, np.inf):
        qb, rb = q.copy(), ref.copy()
        qb[5, 3] = bad
        first = int(knn_ref(q, ref, 1)[0][9, 0])
        rb[first, 0] = bad
        got = metrics.nearest(qb, rb, 3)
        assert same(got, knn_ref(qb, rb, 3)) and (got[0][5] == -1).all() and np.isnan(got[1][5]).all() and not (got[0] == first).any()
    with pytest.raises(ValueError):
        metrics.nearest(q, ref, 9)
    with pytest.raises(ValueError):
        metrics.nearest(q, ref[:, :5], 3)


def test_numpy_path_on_real_valued_features_and_near_copies():
    import metrics
    real, fake = recipe(20)
    want = knn_ref(fake, real, 8)
    got = metrics.nearest(fake, real, 8)
    assert np.array_equal(got[0], want[0]) and np.allclose(got[1], want[1], rtol=1e-12, atol=0)
    g = np.random.default_rng(4)
    ref = g.integers(0, 256, size=(40, 3072)) / 127.5 - 1
    q = ref[[7, 21]] + 1e-3 * g.standard_normal((2, 3072))                  # d2 about 3e-3 beside norms of about 1000
    got = metrics.nearest(q, ref, 2)
    want = knn_ref(q, ref, 2)
    assert got[0][:, 0].tolist() == [7, 21] and np.array_equal(got[0], want[0]) and np.allclose(got[1], want[1], rtol=1e-12, atol=0)
    assert same(merge_ref([knn_ref(q, ref[:15], 2), knn_ref(q, ref[15:], 2, ref_base=15)], 2), want)


def test_workspace_size_is_host_only_and_refuses_bad_sizes():
    from hipgan import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    dll = _lib.load_library()
    assert dll.jck_knn_index_ws_bytes(0, 10) == 0 and dll.jck_knn_index_ws_bytes(10, 0) == 0 and dll.jck_knn_index_ws_bytes((1 << 30) + 1, 10) == 0
    strips = lambda m, n: (dll.jck_knn_index_ws_bytes(m, n) // (4 * m) - 1) // 16
    assert strips(1, 1) == 1 and strips(65, 5000) > 1
    assert strips(64, 50000) >= 256                                           # 64 queries against the training set: a workgroup per CU at least
    assert strips(10000, 50000) * ((10000 + 63) // 64) >= 256 and strips(10000, 50000) <= 8


def test_cli_arguments():
    import generate
    a = generate.get_arg_parse(["--checkpoint", "x.pt", "--out", "o"])
    assert a.neighbours is None and a.k == 4
    a = generate.get_arg_parse(["--checkpoint", "x.pt", "--out", "o", "--neighbours", "train.npz", "--k", "2", "--num", "5"])
    assert a.neighbours == "train.npz" and a.k == 2 and a.num == 5
    a = generate.get_arg_parse(["--checkpoint", "x.pt", "--out", "o", "--neighbours", "train.npz", "--score_images", "im.npz"])
    assert a.neighbours == "train.npz" and a.score_images == "im.npz"
    for bad in (["--neighbours", "t.npz", "--k", "0"], ["--neighbours", "t.npz", "--k", "9"], ["--neighbours", "t.npz", "--project", "im.npz"]):
        with pytest.raises(SystemExit):
            generate.get_arg_parse(["--checkpoint", "x.pt", "--out", "o"] + bad)


def test_picture_rows_are_the_sample_then_its_neighbours():
    import generate
    from hipgan.neighbours import neighbour_rows
    g = np.random.default_rng(5)
    q = g.integers(0, 256, size=(3, 8, 8, 3), dtype=np.uint8)
    ref = g.integers(0, 256, size=(10, 8, 8, 3), dtype=np.uint8)
    idx = np.array([[4, 9], [0, -1], [9, 4]])
    rows = neighbour_rows(q, ref, idx)
    assert rows.shape == (9, 8, 8, 3) and rows.dtype == np.uint8
    for i in range(3):
        assert np.array_equal(rows[3 * i], q[i])
        for t in range(2):
            assert np.array_equal(rows[3 * i + 1 + t], ref[idx[i, t]] if idx[i, t] >= 0 else np.zeros((8, 8, 3), np.uint8))
    sheet = generate.grid_u8(rows, 3)
    assert sheet.shape == (3 * 10 + 2, 3 * 10 + 2, 3)                        # one row per sample, 1 + k pictures wide, padding 2
    assert np.array_equal(sheet[2:10, 2:10], q[0]) and np.array_equal(sheet[12:20, 22:30], np.zeros((8, 8, 3), np.uint8))
    assert np.array_equal(sheet[22:30, 12:20], ref[9])
    # a 4x4 reference goes through the training transform's 2x upscale before it is shown
    from preprocess.dcgan_data_preprocessor import resize2x_pil_u8
    small = g.integers(0, 256, size=(10, 4, 4, 3), dtype=np.uint8)
    up = resize2x_pil_u8(torch.as_tensor(small).permute(0, 3, 1, 2)).permute(0, 2, 3, 1).numpy()
    assert np.array_equal(neighbour_rows(q, small, idx, steps=1), neighbour_rows(q, up, idx))


def test_reference_file_errors_name_the_file(tmp_path):
    from hipgan._lib import JckError
    from hipgan.neighbours import load_reference_images, nearest_images, upscale_steps
    ok = np.zeros((2, 32, 32, 3), np.uint8)
    cases = {"none.npz": {"pictures": ok}, "dtype.npz": {"images": ok.astype(np.float32)}, "shape.npz": {"images": ok[..., :2]},
             "rect.npz": {"images": np.zeros((2, 32, 16, 3), np.uint8)}, "empty.npz": {"images": ok[:0]}}
    for name, arrays in cases.items():
        path = str(tmp_path / name)
        np.savez(path, **arrays)
        with pytest.raises(JckError, match=name):
            load_reference_images(path)
    path = str(tmp_path / "good.npz")
    np.savez(path, images=ok)
    assert load_reference_images(path).shape == (2, 32, 32, 3)
    assert upscale_steps(32, 64) == 1 and upscale_steps(32, 128) == 2 and upscale_steps(64, 64) == 0
    for ref_size, size in ((48, 64), (128, 64), (24, 64)):
        with pytest.raises(JckError, match="train.npz"):
            upscale_steps(ref_size, size, what="train.npz")
    if not torch.cuda.is_available():
        with pytest.raises(JckError):
            nearest_images(np.zeros((1, 64, 64, 3), np.uint8), ok)


def test_bad_reference_ends_generate_before_an_engine_exists(tmp_path, monkeypatch):
    import generate
    from hipgan import sampler
    from hipgan._lib import JckError
    monkeypatch.setattr(sampler.Sampler, "from_checkpoint", classmethod(lambda *a, **k: pytest.fail("the sampler was built")))
    path = str(tmp_path / "bad.npz")
    np.savez(path, images=np.zeros((2, 32, 32), np.uint8))
    with pytest.raises(JckError, match="bad.npz"):
        generate.main(["--checkpoint", "x.pt", "--out", str(tmp_path / "o"), "--neighbours", path])
