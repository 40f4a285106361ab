"""The sliced Wasserstein distance without a GPU: the numpy path of metrics.swd against the restatement in tests/swd_ref.py, its exact
properties, the pyramid's identities, hipgan.swd's host helpers, the argument checks of metrics.swd and of the jck_swd_* / jck_sort_rows_*
entry points (which return before any HIP call), and the swd.py command line."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import swd_ref as R

JCK_E_ARG = -1


def both(S, n=5, P=3, D=4, reps=2, seed=3, L=None):
    import metrics
    from hipgan import swd as H
    a, b = R.pictures(n, S, 10 + S), R.pictures(n, S, 20 + S)[::-1].copy()
    L = R.levels_of(S) if L is None else L
    got = metrics.swd(a, b, levels=L, patches=P, dirs=D, repeats=reps, seed=seed)
    pos, dirs = H.draw(n, S, L, P, D, reps, seed)
    return got, R.swd(a, b, pos, dirs, L), (a, b)


@pytest.mark.parametrize("S", (32, 64))
def test_numpy_path_matches_the_restatement(S):
    got, ref, _ = both(S)
    L = R.levels_of(S)
    assert got["per_repeat"].shape == (2, L) and got["swd"].shape == (L,) and got["swd"].dtype == np.float64
    assert got["sides"] == [S >> l for l in range(L)] and got["sides"][-1] == 16
    assert (ref > 0).all()
    assert np.abs(got["per_repeat"] - ref).max() <= 1e-10 * np.abs(ref).max()
    assert np.abs(got["swd"] - ref.mean(axis=0)).max() <= 1e-10 * np.abs(ref).max() and abs(got["mean"] - ref.mean()) <= 1e-10 * np.abs(ref).max()
    fewer = both(S, L=L - 1)
    assert fewer[0]["sides"] == [S >> l for l in range(L - 1)] and np.abs(fewer[0]["per_repeat"] - fewer[1]).max() <= 1e-10 * np.abs(ref).max()


def test_exact_properties_of_the_numpy_path():
    import metrics
    a, b = R.pictures(6, 32, 1), R.pictures(6, 32, 2)[::-1].copy()
    kw = dict(patches=4, dirs=5, repeats=2, seed=9)
    same = metrics.swd(a, a.copy(), **kw)
    assert (same["swd"] == 0).all() and same["mean"] == 0.0 and (same["per_repeat"] == 0).all()
    ab, ba = metrics.swd(a, b, **kw), metrics.swd(b, a, **kw)
    assert ab["per_repeat"].tobytes() == ba["per_repeat"].tobytes() and ab["swd"].tobytes() == ba["swd"].tobytes() and ab["mean"] == ba["mean"]
    again = metrics.swd(torch.from_numpy(a), b, **kw)                               # host tensors take the numpy path too
    assert again["per_repeat"].tobytes() == ab["per_repeat"].tobytes()
    other = metrics.swd(a, b, **{**kw, "seed": 10})
    assert not np.array_equal(other["per_repeat"], ab["per_repeat"])
    dark = np.minimum(a, 245)
    shifted = metrics.swd(dark, dark + 10, **kw)                                    # brightness: identical dyadic band-pass descriptors
    assert (shifted["swd"][:-1] == 0).all() and 0 <= shifted["swd"][-1] < 1e-9
    flat = np.full((3, 32, 32, 3), 77, np.uint8)                                    # no deviation anywhere: rstd = 0, not NaN
    r = metrics.swd(flat, R.pictures(3, 32, 5), **kw)
    assert np.isfinite(r["per_repeat"]).all() and (r["swd"] > 0).all()
    assert (metrics.swd(flat, flat + 1, **kw)["swd"] == 0).all()


@pytest.mark.parametrize("S", (32, 64, 128))
def test_pyramid_identities(S):
    from hipgan import swd as H
    L = H.max_levels(S)
    assert L == R.levels_of(S) == {32: 2, 64: 3, 128: 4}[S]
    x = R.pictures(5, S, S)
    x[4] = 201
    g, lap = H.pyramid(x, L)
    gr, lapr = R.pyramid(x, L)
    for l in range(L):
        assert g[l].shape == (5, 3, S >> l, S >> l) and np.array_equal(g[l], gr[l]) and np.array_equal(lap[l], lapr[l])
    for l in range(L - 1):
        assert np.array_equal(lap[l] + H.up(g[l + 1]), g[l])                        # dyadic weights: exact in fp64
        assert (lap[l][4] == 0).all() and (lap[l][1] == 0).all()                    # a constant picture has no band-pass content
    assert (lap[L - 1][4] == 201).all() and np.array_equal(lap[L - 1], g[L - 1])
    # mirror borders, the edge sample not repeated: a ramp's first down-sampled value, by hand
    ramp = np.arange(S, dtype=np.float64)[None, :].repeat(S, 0)
    assert H.down(ramp)[0, 0] == (2 + 4 * 1 + 0 + 4 * 1 + 2) / 16.0 and H.down(ramp)[0, 1] == 2.0
    one = np.zeros((4, 4))
    one[0, 0] = 8.0
    assert H.up(one)[0, :3].tolist() == [8 * 36 / 64.0, 8 * 24 / 64.0, 8 * 6 / 64.0]


def test_draw_and_helpers():
    from hipgan import swd as H
    from hipgan._lib import JckError
    pos, d = H.draw(4, 64, 3, patches=6, dirs=5, repeats=2, seed=11)
    assert pos.shape == (4, 3, 6, 2) and pos.dtype == np.int32 and d.shape == (2, 5, 147) and d.dtype == np.float32
    for l in range(3):
        assert pos[:, l].min() >= 0 and pos[:, l].max() <= (64 >> l) - 7
    assert np.abs(np.sqrt((d.astype(np.float64) ** 2).sum(axis=2)) - 1).max() <= 1e-7
    p2, d2 = H.draw(4, 64, 3, patches=6, dirs=5, repeats=2, seed=11)
    assert np.array_equal(pos, p2) and np.array_equal(d, d2) and not np.array_equal(H.draw(4, 64, 3, 6, 5, 2, 12)[0], pos)
    g = np.random.default_rng(11)                                                   # the definition, written out
    want = np.stack([g.integers(0, (64 >> l) - 6, size=(4, 6, 2)) for l in range(3)], axis=1)
    dd = g.standard_normal((2, 5, 147))
    assert np.array_equal(pos, want) and np.array_equal(d, (dd / np.sqrt((dd * dd).sum(axis=2, keepdims=True))).astype(np.float32))
    assert [H.max_levels(S) for S in (16, 32, 48, 64, 128, 256)] == [0, 2, 0, 3, 4, 0]
    assert H.level_names(64, 3) == ["64x64", "32x32", "16x16"] and H.sides(128, 4) == [128, 64, 32, 16]
    for bad in (dict(n=0), dict(L=4), dict(L=0), dict(patches=0), dict(dirs=0), dict(repeats=0), dict(S=48)):
        kw = {**dict(n=2, S=64, L=3, patches=2, dirs=2, repeats=1), **bad}
        with pytest.raises(JckError):
            H.draw(**kw)
    plane = np.arange(2 * 3 * 16 * 16, dtype=np.float64).reshape(2, 3, 16, 16)
    corners = np.array([[[0, 0], [9, 9], [2, 5]], [[9, 0], [0, 9], [4, 4]]])
    got = H.descriptors(plane, corners)
    assert got.shape == (6, 3, 49) and np.array_equal(got.reshape(2, 3, 147), R.descriptors(plane, corners))
    m, r = H.moments(got)
    m2, r2 = H.moments_from_sums(got.sum(axis=(0, 2)), (got * got).sum(axis=(0, 2)), 6 * 49)
    assert np.abs(m - m2).max() <= 1e-9 and np.abs(r - r2).max() <= 1e-9 * r.max()
    assert H.moments(np.full((4, 3, 49), 5.0))[1].tolist() == [0, 0, 0] and H.moments_from_sums(np.full(3, 20.0), np.full(3, 100.0), 4)[1].tolist() == [0, 0, 0]
    rep = H.report([[1.0, 2.0, 6.0], [3.0, 4.0, 8.0]], 64, {"n": 7})
    assert rep["swd"].tolist() == [2.0, 3.0, 7.0] and rep["mean"] == 4.0 and rep["sides"] == [64, 32, 16] and rep["n"] == 7
    assert H.format_report(rep) == "64x64 2.00 | 32x32 3.00 | 16x16 7.00 | mean 4.00"
    js = H.to_json(rep)
    assert json.loads(json.dumps(js)) == js and js["levels"] == ["64x64", "32x32", "16x16"] and "per_repeat" not in js and len(js["reads_as"]) == 3


def test_metrics_swd_refuses_malformed_arguments():
    import metrics
    ok = R.pictures(2, 32, 1)
    bad_sets = (
        (ok[0], ok), (ok[:, :, :, :2], ok[:, :, :, :2]), (ok[:, :16], ok[:, :16]), (R.pictures(2, 64, 1), ok), (ok[:1], ok), (ok.astype(np.float32), ok),
        (np.zeros((2, 48, 48, 3), np.uint8),) * 2, (np.zeros((2, 16, 16, 3), np.uint8),) * 2, (np.zeros((0, 32, 32, 3), np.uint8),) * 2)
    for a, b in bad_sets:
        with pytest.raises(ValueError) as e:
            metrics.swd(a, b)
        assert "swd:" in str(e.value) and str(tuple(np.asarray(a).shape)) in str(e.value)        # the shape is in the message
    for kw in (dict(levels=0), dict(levels=3), dict(patches=0), dict(dirs=0), dict(repeats=0), dict(chunk=0)):
        with pytest.raises(ValueError):
            metrics.swd(ok, ok, **kw)


def test_swd_entry_points_check_their_arguments_on_the_host():
    """JCK_E_ARG with a message before any HIP call (no GPU here); the pattern of test_abi's comm test"""
    from hipgan import _lib
    from hipgan import swd as H
    dll = _lib.load_library()
    for S in (0, 16, 31, 32, 33, 48, 64, 96, 128, 129, 256):
        assert dll.jck_swd_max_levels(S) == H.max_levels(S), S
    T = dll.jck_sort_rows_tile()
    assert T >= 256 and T & (T - 1) == 0
    assert dll.jck_sort_rows_ws_bytes(3, T) == 0 and dll.jck_sort_rows_ws_bytes(3, T + 1) == 3 * (T + 1) * 4
    assert dll.jck_sort_rows_ws_bytes(0, 5) == 0 and dll.jck_sort_rows_ws_bytes(1, 0) == 0
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    err = lambda: dll.jck_last_error()
    # (never passed whole: every call below has one bad argument)
    stats = [p, 2, 64, 3, p, 4, p, p, p, None]                    # images, n, S, L, pos, P, part, sum, sumsq, stream
    for hole in (0, 4, 6, 7, 8):
        args = list(stats)
        args[hole] = None
        assert dll.jck_swd_patch_stats_u8(*args) == JCK_E_ARG and b"swd_patch_stats" in err() and b"null" in err(), hole
    proj = [p, 2, 64, 3, p, 4, p, 5, p, p, p, 8, None]            # images, n, S, L, pos, P, dirs, D, mean, rstd, proj, ld, stream
    for hole in (0, 4, 6, 8, 9, 10):
        args = list(proj)
        args[hole] = None
        assert dll.jck_swd_project_u8(*args) == JCK_E_ARG and b"swd_project" in err() and b"null" in err(), hole
    for fn, good in ((dll.jck_swd_patch_stats_u8, stats), (dll.jck_swd_project_u8, proj)):
        for at, value, word in ((2, 48, b"S must"), (2, 16, b"S must"), (2, 256, b"S must"), (3, 0, b"L must"), (3, 4, b"L must"), (5, 0, b"P must"),
                                (5, -3, b"P must"), (1, 0, b"n must")):
            args = list(good)
            args[at] = value
            assert fn(*args) == JCK_E_ARG and word in err(), (at, value)
    for at, value, word in ((7, 0, b"D must"), (7, -1, b"D must"), (11, 7, b"ld must")):
        args = list(proj)
        args[at] = value
        assert dll.jck_swd_project_u8(*args) == JCK_E_ARG and word in err(), (at, value)
    args32 = list(proj)
    args32[2], args32[3] = 32, 3
    assert dll.jck_swd_project_u8(*args32) == JCK_E_ARG and b"L must" in err()
    sort = [p, 3, T + 1, p, p, 3 * (T + 1) * 4, None]             # x, Rows, M, out, ws, ws_bytes, stream
    for at, value, word in ((0, None, b"null"), (3, None, b"null"), (1, 0, b"Rows and M"), (2, 0, b"Rows and M"), (2, -5, b"Rows and M"),
                            (5, 3 * (T + 1) * 4 - 1, b"workspace"), (4, None, b"workspace"), (1, 1 << 30, b"below 2^31")):
        args = list(sort)
        args[at] = value
        if at == 1 and value == 1 << 30:
            args[5] = 1 << 62
        assert dll.jck_sort_rows_f32(*args) == JCK_E_ARG and b"sort_rows" in err() and word in err(), (at, value)
    rows = [p, p, 3, 10, p, None]                                 # sa, sb, Rows, M, w, stream
    for at, value, word in ((0, None, b"null"), (1, None, b"null"), (4, None, b"null"), (2, 0, b"Rows and M"), (3, 0, b"Rows and M")):
        args = list(rows)
        args[at] = value
        assert dll.jck_swd_rows(*args) == JCK_E_ARG and b"swd_rows" in err() and word in err(), (at, value)


def test_swd_parser_defaults_refusals_and_help(capsys):
    import swd
    base = ["--checkpoint", "c.pt", "--train", "t.npz", "--out", "o"]
    a = swd.get_arg_parse(base)
    assert (a.model, a.num, a.patches, a.dirs, a.repeats, a.seed, a.which, a.batch_size, a.prec) == ("DCGAN", 8192, 128, 128, 4, 0, "auto", 64, "bf16")
    assert a.levels is None and a.classes is None and a.compare is None and a.truncation is None
    a = swd.get_arg_parse(base + ["-m", "CGAN", "--classes", "3,17,42", "--num", "200", "--patches", "16", "--dirs", "8", "--repeats", "2", "--seed", "5",
                                  "--which", "ema", "--levels", "2"])
    assert (a.model, a.classes, a.num, a.patches, a.dirs, a.repeats, a.seed, a.which, a.levels) == ("CGAN", [3, 17, 42], 200, 16, 8, 2, 5, "ema", 2)
    assert swd.settings_of(a) == {"patches": 16, "dirs": 8, "repeats": 2}
    a = swd.get_arg_parse(["--compare", "a.npz:recon", "dir.x/b.npz", "--out", "o"])
    assert a.compare == [("a.npz", "recon"), ("dir.x/b.npz", "images")]
    for bad in (["--num", "0"], ["-b", "0"], ["--levels", "0"], ["--levels", "5"], ["--truncation", "0"], ["--patches", "0"], ["--dirs", "0"], ["--repeats", "0"],
                ["--classes", "3"], ["-m", "CGAN", "--classes", "100"], ["-m", "CGAN", "--classes", "a,b"], ["--compare", "a.npz", "b.npz"], ["--which", "x"]):
        with pytest.raises(SystemExit):
            swd.get_arg_parse(base + bad)
    for argv in (["--out", "o"], ["--checkpoint", "c.pt", "--train", "t.npz"], ["--checkpoint", "c.pt", "--out", "o"], ["--compare", "a.npz", "--out", "o"],
                 ["--compare", "a.npz", "b.npz", "--out", "o", "--train", "t.npz"]):
        with pytest.raises(SystemExit):
            swd.get_arg_parse(argv)
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        swd.get_arg_parse(["--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    assert "--compare" in text and "swd.json" in text and "texture" in text and "layout" in text and "--repeats" in text


def test_compare_run_end_to_end(tmp_path):
    """--compare needs no checkpoint, and without a GPU no device: the files' keys and shapes, the numbers against metrics.swd's numpy
    path (where there is a GPU the run goes through the kernels: within swd_ref.device_error_bound)"""
    import metrics
    import swd
    from hipgan import swd as H
    from hipgan._lib import JckError
    a, b = R.pictures(6, 32, 41), R.pictures(6, 32, 42)[::-1].copy()
    np.savez(str(tmp_path / "a.npz"), images=a, other=b)
    argv = ["--patches", "5", "--dirs", "4", "--repeats", "3", "--seed", "2"]
    assert swd.main(["--compare", str(tmp_path / "a.npz"), str(tmp_path / "a.npz"), "--out", str(tmp_path / "same")] + argv) == 0
    rec = json.load(open(str(tmp_path / "same" / "swd.json")))
    assert rec["swd"] == [0.0, 0.0] and rec["mean"] == 0.0
    assert swd.main(["--compare", str(tmp_path / "a.npz"), str(tmp_path / "a.npz") + ":other", "--out", str(tmp_path / "cmp")] + argv) == 0
    rec = json.load(open(str(tmp_path / "cmp" / "swd.json")))
    f = np.load(str(tmp_path / "cmp" / "swd.npz"))
    assert set(rec) == {"swd", "mean", "sides", "levels", "reads_as", "n", "seed", "settings"}
    assert rec["sides"] == [32, 16] and rec["levels"] == ["32x32", "16x16"] and rec["n"] == 6 and rec["seed"] == 2
    assert rec["settings"] == {"patches": 5, "dirs": 4, "repeats": 3}
    assert f.files == ["per_repeat"] and f["per_repeat"].shape == (3, 2) and f["per_repeat"].dtype == np.float64
    want = metrics.swd(a, b, patches=5, dirs=4, repeats=3, seed=2)
    tol = np.full(2, 1e-10 * want["per_repeat"].max())
    if torch.cuda.is_available():
        tol = 2e3 * R.device_error_bound(a, b, *H.draw(6, 32, 2, 5, 4, 3, 2), 2)
    assert (np.abs(f["per_repeat"] - want["per_repeat"]) <= tol[None, :]).all() and (np.abs(np.array(rec["swd"]) - want["swd"]) <= tol).all()
    assert abs(rec["mean"] - np.mean(rec["swd"])) <= 1e-12 * rec["mean"]
    np.savez(str(tmp_path / "c.npz"), images=R.pictures(6, 64, 1))
    np.savez(str(tmp_path / "d.npz"), images=np.zeros((6, 48, 48, 3), np.uint8))
    for other in ("c.npz", "d.npz", "a.npz:nothing"):
        with pytest.raises(JckError):
            swd.main(["--compare", str(tmp_path / "a.npz"), str(tmp_path / other), "--out", str(tmp_path / "bad")])
