"""Power spectra without a GPU: the numpy path of metrics.spectrum against the restatement in tests/spectrum_ref.py, the bin rule and
its counts, the exact properties (constants, checkerboard, Parseval), the report's properties, the argument checks of metrics.spectrum and
of the jck_spectrum_* entry points (which return before any HIP call), and the spectrum.py --compare command line."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import spectrum_ref as R

JCK_E_ARG = -1
PLANES = ("r", "g", "b", "luma")


@pytest.mark.parametrize("S", (32, 64))
def test_numpy_path_matches_the_restatement(S):
    import metrics
    x = R.pictures(7, S, 100 + S)
    for p, plane in enumerate(PLANES):
        for window in (None, "hann"):
            got = metrics.spectrum(x, plane=plane, window=window, mean2d=True, chunk=3)
            P, mean = R.power(x, plane, window)
            prof, count = R.profile(P)
            scale = np.abs(prof).max()
            assert got["profile"].shape == prof.shape and got["profile"].dtype == np.float64
            assert np.abs(got["profile"] - prof).max() <= 1e-10 * scale, (plane, window)
            assert np.abs(got["mean2d"] - P.mean(axis=0)).max() <= 1e-10 * P.mean(axis=0).max(), (plane, window)
            assert np.array_equal(got["mean"], mean) and np.array_equal(got["count"], count)
            assert np.array_equal(got["radius"], np.arange(prof.shape[1])) and (got["S"], got["plane"], got["window"]) == (S, plane, window)
            again = metrics.spectrum(torch.from_numpy(x), plane=p, window=window)       # host tensors and plane numbers take the same path
            assert np.abs(again["profile"] - prof).max() <= 1e-10 * scale and again["mean2d"] is None


@pytest.mark.parametrize("S,bins", ((32, 24), (64, 46), (128, 92)))
def test_bins_counts_and_the_integer_rule(S, bins):
    from hipgan import spectrum as H
    b = H.bin_map(S)
    assert H.bins(S) == bins and int(b.max()) + 1 == bins
    c = H.counts(S)
    assert c.shape == (bins,) and int(c.sum()) == S * S and c.min() >= 1 and c[0] == 1 and c[bins - 1] >= 1
    f = np.minimum(np.arange(S), S - np.arange(S))
    d2 = f[:, None] ** 2 + f[None, :] ** 2
    assert np.array_equal(b, np.floor(np.sqrt(d2.astype(np.float64)) + 0.5).astype(np.int64))       # the whole plane
    assert np.array_equal(b, R.bin_map(S))
    assert ((b * b - b < d2) & (d2 <= b * b + b) | (d2 == 0)).all() and b[0, 0] == 0
    assert b[S // 2, S // 2] == bins - 1 and np.array_equal(b, b.T) and np.array_equal(b[1:, 1:], b[1:, 1:][::-1, ::-1])


def test_bounds_of_the_restatement():
    got = [R.bound(S) for S in (32, 64, 128)]
    assert got[0] < got[1] < got[2] <= 2e-5
    for have, plain in zip(got, (7.9e-6, 9.5e-6, 1.11e-5)):              # the plain radix-2 figure plus the input, split and fp64 terms
        assert plain < have < plain + 6e-7


@pytest.mark.parametrize("S", (32, 64))
def test_constant_checkerboard_and_parseval(S):
    import metrics
    x = R.pictures(7, S, 200 + S)
    for plane in PLANES:
        r = metrics.spectrum(x, plane=plane)
        prof, count = r["profile"], r["count"]
        assert (prof[1] == 0).all() and (prof[2] == 0).all() and r["mean"][1] == 0.0 and r["mean"][2] == 255.0
        Y = R.plane_int(x, plane).astype(np.float64) / 256.0
        var = Y.reshape(7, -1).var(axis=1)
        assert np.abs((prof * count[None, :]).sum(axis=1) / (S * S) - var).max() <= 1e-10 * var.max()          # Parseval
    last = r["count"].shape[0] - 1
    board = metrics.spectrum(x[3:4], plane="g")
    energy = board["profile"][0] * board["count"]
    assert abs(energy[last] - S * S * 127.5 ** 2) <= 1e-9 * S * S * 127.5 ** 2
    assert (np.abs(energy[:last]) < 1e-9 * energy[last]).all()
    hann = metrics.spectrum(x[1:3], window="hann", mean2d=True)
    assert (hann["profile"] == 0).all() and (hann["mean2d"] == 0).all()


def test_window_table_and_helpers():
    from hipgan import spectrum as H
    w, W = H.window_table(64, "hann")
    assert w.dtype == np.float32 and w.shape == (64,) and w[0] == 0 and w[32] == 1 and np.array_equal(w, R.hann32(64))
    assert abs(W - 0.375 ** 2) < 1e-7 and H.window_table(64, None) == (None, 1.0)
    assert [H.plane_index(p) for p in ("r", "g", "b", "luma", 0, 3)] == [0, 1, 2, 3, 0, 3]
    assert len(H.lattice_points(64)) == 15 and (32, 32) in H.lattice_points(64) and (0, 0) not in H.lattice_points(64)
    plane = np.full((32, 32), 2.0)
    plane[16, 16] = 200.0
    assert abs(H.peak_db(plane, 16, 16) - 20.0) < 1e-12 and H.peak_db(plane, 8, 8) == 0.0
    img = H.render(plane)
    assert img.shape == (32, 32, 3) and img.dtype == np.uint8 and img[0, 0, 0] == img[0, 0, 2]
    lo, hi = H.RENDER_DB
    assert img[0, 0, 0] == int(np.rint((10 * np.log10(200.0) - lo) * 255 / (hi - lo)))            # fft-shifted: (16, 16) is at the corner
    assert img[5, 5, 0] == int(np.rint((10 * np.log10(2.0) - lo) * 255 / (hi - lo)))
    diff = H.render_diff(plane, plane)
    assert diff.shape == (32, 32, 3) and (diff == 128).all()


def test_report_properties():
    import metrics
    S = 32
    a = np.concatenate([R.pictures(7, S, s)[[0, 5, 6]] for s in range(4)])                        # 12 pictures without constant ones
    b = np.concatenate([R.pictures(7, S, 50 + s)[[0, 5, 6]] for s in range(3)])                   # 9 others
    sa, sb = metrics.spectrum(a, mean2d=True), metrics.spectrum(b, mean2d=True)
    same = metrics.spectrum_report(sa, metrics.spectrum(a.copy(), mean2d=True))
    assert (same["gap_db"] == 0).all() and (same["z"] == 0).all() and same["separability"] == 0.5
    assert same["rms_gap_db"] == 0 and same["high_gap_db"] == 0 and same["checkerboard_db"] == 0 and len(same["peaks"]) == 15
    ab, ba = metrics.spectrum_report(sa, sb), metrics.spectrum_report(sb, sa)
    assert np.array_equal(ab["gap_db"], -ba["gap_db"]) and np.array_equal(ab["z"], -ba["z"]) and ab["high_gap_db"] == -ba["high_gap_db"]
    assert ab["n_a"] == 12 and ab["n_b"] == 9 and ab["gap_db"].shape == (24,) and ab["worst"]["bin"] == int(np.argmax(np.abs(ab["gap_db"])))
    assert abs(ab["rms_gap_db"] - np.sqrt((ab["gap_db"][1:] ** 2).mean())) < 1e-12 and abs(ab["high_gap_db"] - ab["gap_db"][9:].mean()) < 1e-12
    db = 10 * np.log10(np.maximum(sa["profile"], 1e-6))
    assert np.allclose(ab["mean_db_a"], db.mean(axis=0), rtol=0, atol=1e-12) and np.allclose(ab["std_db_a"], db.std(axis=0, ddof=1), rtol=0, atol=1e-12)
    assert abs(ab["separability"] - ba["separability"]) < 1e-12 and 0.0 <= ab["separability"] <= 1.0   # the rule and the flags swap together
    one = metrics.spectrum_report(metrics.spectrum(a[:1]), metrics.spectrum(b[:3]))              # n = 1: std 0; below 4 pictures: no separability
    assert (one["std_db_a"] == 0).all() and one["separability"] is None and one["peaks"] is None and one["checkerboard_db"] is None
    # a planted checkerboard of amplitude 2 levels on smooth pictures
    smooth = np.concatenate([R.pictures(7, S, 90 + s)[[6]] for s in range(8)])
    yy, xx = np.mgrid[0:S, 0:S]
    planted = (smooth.astype(np.int64) + (2 * (((yy + xx) & 1) * 2 - 1))[None, :, :, None]).clip(0, 255).astype(np.uint8)
    r = metrics.spectrum_report(metrics.spectrum(planted, mean2d=True), metrics.spectrum(smooth, mean2d=True))
    assert r["checkerboard_db"] > 20 and r["gap_db"][23] > 10 and r["worst"]["bin"] == 23 and r["separability"] == 1.0
    pk = {(p["u"], p["v"]): p for p in r["peaks"]}
    assert pk[(16, 16)]["diff_db"] == r["checkerboard_db"] and abs(pk[(8, 8)]["diff_db"]) < 3
    with pytest.raises(ValueError):
        metrics.spectrum_report(sa, metrics.spectrum(b, plane="r"))
    from hipgan.spectrum import format_report, to_json
    js = to_json(r)
    assert json.loads(json.dumps(js)) == js and "checkerboard" in format_report(r) and len(js["peaks"]) == 15


def test_metrics_spectrum_refuses_malformed_arguments():
    import metrics
    ok = R.pictures(2, 32, 1)
    for x in (ok[0], ok[:, :, :, :2], ok[:, :16], ok.astype(np.float32), np.zeros((2, 48, 48, 3), np.uint8), np.zeros((2, 16, 16, 3), np.uint8)):
        with pytest.raises(ValueError) as e:
            metrics.spectrum(x)
        assert "spectrum:" in str(e.value) and str(tuple(np.asarray(x).shape)) in str(e.value)
    for kw in (dict(plane="y"), dict(plane=4), dict(plane=-1), dict(plane=1.5), dict(window="hamming"), dict(chunk=0)):
        with pytest.raises(ValueError):
            metrics.spectrum(ok, **kw)
    empty = metrics.spectrum(np.zeros((0, 64, 64, 3), np.uint8), mean2d=True)
    assert empty["profile"].shape == (0, 46) and empty["mean"].shape == (0,) and empty["mean2d"].shape == (64, 64)


def test_spectrum_entry_points_check_their_arguments_on_the_host():
    """JCK_E_ARG with a message before any HIP call (no GPU here), as test_swd_cpu does it"""
    from hipgan import _lib
    from hipgan import spectrum as H
    dll = _lib.load_library()
    for S, bins in ((32, 24), (64, 46), (128, 92)):
        assert dll.jck_spectrum_bins(S) == bins == H.bins(S)
        G = dll.jck_spectrum_grid(S)
        assert G >= 1
        plane_bytes = S * (S // 2 + 1) * 8
        assert dll.jck_spectrum_ws_bytes(5, S, 0) == 0 and dll.jck_spectrum_ws_bytes(0, S, 1) == 0
        assert dll.jck_spectrum_ws_bytes(1, S, 1) == plane_bytes and dll.jck_spectrum_ws_bytes(G, S, 1) == G * plane_bytes
        assert dll.jck_spectrum_ws_bytes(G + 1, S, 1) == G * plane_bytes and dll.jck_spectrum_ws_bytes(1 << 30, S, 1) == G * plane_bytes
    for S in (0, 16, 31, 33, 48, 96, 129, 256, -64):
        assert dll.jck_spectrum_bins(S) == JCK_E_ARG and b"S must" in dll.jck_last_error()
        assert dll.jck_spectrum_grid(S) == JCK_E_ARG and dll.jck_spectrum_ws_bytes(4, S, 1) == 0
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    err = lambda: dll.jck_last_error()
    need = dll.jck_spectrum_ws_bytes(3, 64, 1)
    # (never passed whole: every call below has one bad argument)
    good = [p, 3, 64, 3, p, 0.14, p, p, p, p, need, None]          # x, n, S, plane, win, win_power, prof, mean, mean2d, ws, ws_bytes, stream
    for hole in (0, 6, 7):
        args = list(good)
        args[hole] = None
        assert dll.jck_spectrum_u8(*args) == JCK_E_ARG and b"spectrum" in err() and b"null" in err(), hole
    for at, value, word in ((2, 48, b"S must"), (2, 16, b"S must"), (2, 256, b"S must"), (3, 4, b"plane must"), (3, -1, b"plane must"), (1, -1, b"n must"),
                            (5, 0.0, b"win_power"), (5, -1.0, b"win_power"), (5, float("inf"), b"win_power"), (5, float("nan"), b"win_power"),
                            (9, None, b"workspace"), (10, need - 1, b"workspace"), (10, 0, b"workspace")):
        args = list(good)
        args[at] = value
        assert dll.jck_spectrum_u8(*args) == JCK_E_ARG and word in err(), (at, value)
    nothing = list(good)
    nothing[1] = 0                                                   # n = 0: success, nothing launched
    assert dll.jck_spectrum_u8(*nothing) == 0
    nothing[2] = 48
    assert dll.jck_spectrum_u8(*nothing) == JCK_E_ARG and b"S must" in err()


def test_spectrum_parser_defaults_refusals_and_help(capsys):
    import spectrum
    base = ["--checkpoint", "c.pt", "--train", "t.npz", "--out", "o"]
    a = spectrum.get_arg_parse(base)
    assert (a.model, a.num, a.plane, a.window, a.seed, a.which, a.batch_size, a.prec) == ("DCGAN", 8192, "luma", None, 0, "auto", 64, "bf16")
    a = spectrum.get_arg_parse(base + ["-m", "CGAN", "--classes", "3,17", "--num", "200", "--plane", "g", "--window", "hann", "--seed", "5", "--which", "ema"])
    assert (a.model, a.classes, a.num, a.plane, a.window, a.seed, a.which) == ("CGAN", [3, 17], 200, "g", "hann", 5, "ema")
    assert spectrum.settings_of(a) == {"plane": "g", "window": "hann"}
    a = spectrum.get_arg_parse(["--compare", "a.npz:recon", "dir.x/b.npz", "--out", "o"])
    assert a.compare == [("a.npz", "recon"), ("dir.x/b.npz", "images")]
    for bad in (["--num", "0"], ["-b", "0"], ["--plane", "y"], ["--window", "hamming"], ["--truncation", "0"], ["--classes", "3"],
                ["-m", "CGAN", "--classes", "100"], ["--compare", "a.npz", "b.npz"]):
        with pytest.raises(SystemExit):
            spectrum.get_arg_parse(base + bad)
    for argv in (["--out", "o"], ["--checkpoint", "c.pt", "--train", "t.npz"], ["--compare", "a.npz", "--out", "o"]):
        with pytest.raises(SystemExit):
            spectrum.get_arg_parse(argv)
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        spectrum.get_arg_parse(["--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    assert "--compare" in text and "spectrum.json" in text and "checkerboard" in text and "--window" in text


def test_compare_run_end_to_end(tmp_path):
    """--compare needs no checkpoint and, without a GPU, no device: the three files, their keys and shapes, the numbers against
    metrics.spectrum's numpy path (where there is a GPU the run goes through the kernel: within the dB equivalent of the derived bound)"""
    import metrics
    import spectrum
    from hipgan._lib import JckError
    S = 32
    a = np.concatenate([R.pictures(1, S, 300 + s) for s in range(6)])                             # random bytes (white spectra): the derived dB
    b = np.concatenate([R.pictures(1, S, 400 + s) for s in range(8)])                             # tolerance of the device path is finite there
    np.savez(str(tmp_path / "a.npz"), images=a, other=b)
    out = tmp_path / "cmp"
    assert spectrum.main(["--compare", str(tmp_path / "a.npz"), str(tmp_path / "a.npz") + ":other", "--out", str(out), "--plane", "g", "--window", "hann"]) == 0
    rec = json.load(open(str(out / "spectrum.json")))
    f = np.load(str(out / "spectrum.npz"))
    assert set(rec) == {"S", "plane", "window", "n_a", "n_b", "bins", "rms_gap_db", "high_gap_db", "worst", "separability", "checkerboard_db", "peaks"}
    assert (rec["S"], rec["plane"], rec["window"], rec["n_a"], rec["n_b"], rec["bins"]) == (32, "g", "hann", 6, 8, 24)
    assert len(rec["peaks"]) == 15 and set(rec["peaks"][0]) == {"u", "v", "a_db", "b_db", "diff_db"} and set(rec["worst"]) == {"bin", "gap_db", "z"}
    assert 0.0 <= rec["separability"] <= 1.0
    assert sorted(f.files) == sorted(["radius", "count", "mean_db_a", "std_db_a", "mean_db_b", "std_db_b", "gap_db", "z", "mean2d_a", "mean2d_b"])
    assert f["gap_db"].shape == (24,) and f["mean2d_a"].shape == (32, 32) and f["mean2d_a"].dtype == np.float64 and int(f["count"].sum()) == 1024
    png = open(str(out / "spectrum.png"), "rb").read()
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    sa, sb = metrics.spectrum(a, plane="g", window="hann", mean2d=True), metrics.spectrum(b, plane="g", window="hann", mean2d=True)
    want = metrics.spectrum_report(sa, sb)
    tol = np.full(24, 1e-9)
    if torch.cuda.is_available():
        # a picture's bin is within B E of count[r] prof[r]: |d dB| <= (10 / ln 10) rel / (1 - rel) with rel = B E / (count prof); a set's
        # mean_db moves by at most the mean of that over its pictures, the gap by both sets' (a bin with rel >= 0.5 is not compared)
        tol = np.zeros(24)
        for s in (sa, sb):
            rel = R.bound(S) * (s["profile"] * s["count"]).sum(axis=1, keepdims=True) / (s["count"] * np.maximum(s["profile"], 1e-6))
            with np.errstate(divide="ignore", invalid="ignore"):
                tol += np.where(rel < 0.5, (10 / np.log(10)) * rel / (1 - rel), np.inf).mean(axis=0)
        assert set(np.nonzero(~np.isfinite(tol))[0].tolist()) <= {0, 23}                           # the one-point bins (a property of the reference alone)
    assert (np.abs(f["gap_db"] - want["gap_db"]) <= tol).all()
    if np.isfinite(tol).all():
        assert abs(rec["rms_gap_db"] - want["rms_gap_db"]) <= tol.max()
    same = tmp_path / "same"
    assert spectrum.main(["--compare", str(tmp_path / "a.npz"), str(tmp_path / "a.npz"), "--out", str(same)]) == 0
    rec = json.load(open(str(same / "spectrum.json")))
    assert rec["rms_gap_db"] == 0 and rec["checkerboard_db"] == 0 and rec["separability"] == 0.5
    np.savez(str(tmp_path / "c.npz"), images=R.pictures(6, 64, 1))
    np.savez(str(tmp_path / "d.npz"), images=np.zeros((6, 48, 48, 3), np.uint8))
    for other in ("c.npz", "d.npz", "a.npz:nothing"):
        with pytest.raises(JckError):
            spectrum.main(["--compare", str(tmp_path / "a.npz"), str(tmp_path / other), "--out", str(tmp_path / "bad")])
