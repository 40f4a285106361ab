"""The structural-similarity layer without a GPU: the reference (tests/ssim_ref.py) against an independent torch fp64 statement, the
numpy twin of metrics.ssim_pairs, closed forms, hipgan.diversity's host helpers, the host side of the jck_ssim_* entry points and the
diversity.py command line."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import ssim_ref as R

JCK_E_ARG = -1
GEOMETRIES = ((11, 1), (16, 1), (22, 2), (32, 2), (48, 3), (64, 3))


def torch_terms(a, b, L):
    """terms [3,L,2] of one pair with F.conv2d (the outer-product window) and F.avg_pool2d in fp64"""
    F = torch.nn.functional
    g = torch.as_tensor(R.window())
    k = torch.outer(g, g).view(1, 1, 11, 11)
    x, y = (torch.as_tensor(v.astype(np.float64)).permute(2, 0, 1).unsqueeze(1) for v in (a, b))      # [3,1,S,S]
    out = torch.empty(3, L, 2, dtype=torch.float64)
    for l in range(L):
        mx, my = F.conv2d(x, k), F.conv2d(y, k)
        vx, vy, vxy = F.conv2d(x * x, k) - mx * mx, F.conv2d(y * y, k) - my * my, F.conv2d(x * y, k) - mx * my
        cs = (2 * vxy + R.C2) / (vx + vy + R.C2)
        ss = (2 * mx * my + R.C1) / (mx * mx + my * my + R.C1) * cs
        out[:, l, 0], out[:, l, 1] = cs.mean(dim=(1, 2, 3)), ss.mean(dim=(1, 2, 3))
        x, y = F.avg_pool2d(x, 2), F.avg_pool2d(y, 2)
    return out.numpy()


@pytest.mark.parametrize("S,L", GEOMETRIES)
def test_reference_equals_an_independent_torch_statement(S, L):
    x, ia, ib, _ = R.case_set(S, seed=S)
    ref = R.pairs_ref(x, x, ia, ib, L)
    for p, (i, j) in enumerate(zip(ia, ib)):
        t = torch_terms(x[i], x[j], L)
        assert np.abs(t - ref["terms"][p]).max() <= 1e-12, (p, np.abs(t - ref["terms"][p]).max())
        w = R.weights(L)
        ms = np.mean([np.prod([max(t[c, l, 1 if l == L - 1 else 0], 0.0) ** w[l] for l in range(L)]) for c in range(3)])
        assert abs(t[:, 0, 1].mean() - ref["ssim"][p]) <= 1e-12 and abs(ms - ref["ms_ssim"][p]) <= 1e-12


@pytest.mark.parametrize("S,L", GEOMETRIES)
def test_numpy_twin_equals_the_reference(S, L):
    import metrics
    x, ia, ib, _ = R.case_set(S, seed=100 + S)
    y = R.noise(3, S, seed=5)
    ref = R.pairs_ref(x, x, ia, ib, L)
    got = metrics.ssim_pairs(x, x, ia, ib, levels=L, terms=True)
    assert got["terms"].shape == (ia.shape[0], 3, L, 2) and got["sq_err"].dtype == np.int64
    assert np.abs(got["terms"] - ref["terms"]).max() <= 1e-12
    assert np.abs(got["ssim"] - ref["ssim"]).max() <= 1e-12 and np.abs(got["ms_ssim"] - ref["ms_ssim"]).max() <= 1e-12
    assert np.array_equal(got["sq_err"], ref["sq_err"])
    assert np.abs(metrics.ms_ssim_from_terms(ref["terms"]) - ref["ms_ssim"]).max() <= 1e-12
    # two arrays, torch host tensors, an index outside either array: NaN / NaN / -1 for that pair alone
    two = metrics.ssim_pairs(torch.from_numpy(x), y, np.array([0, x.shape[0], 1, -1, 2]), torch.tensor([0, 0, 3, 0, 2]), levels=L, terms=True)
    want = R.pairs_ref(x, y, [0, 2], [0, 2], L)
    assert np.abs(two["ssim"][[0, 4]] - want["ssim"]).max() <= 1e-12 and np.array_equal(two["sq_err"][[0, 4]], want["sq_err"])
    assert np.isnan(two["ssim"][1:4]).all() and np.isnan(two["ms_ssim"][1:4]).all() and (two["sq_err"][1:4] == -1).all() and np.isnan(two["terms"][1:4]).all()
    assert "terms" not in metrics.ssim_pairs(x, x, ia, ib, levels=L)


def test_closed_forms():
    import metrics
    for S, L in ((11, 1), (32, 2), (64, 3), (128, 4)):
        x = np.concatenate([R.extremes(S), R.noise(1, S, 3), np.full((1, S, S, 3), 100, np.uint8), np.full((1, S, S, 3), 37, np.uint8)])
        r = metrics.ssim_pairs(x, x, np.array([2, 0, 3]), np.array([2, 1, 4]), levels=L, terms=True)
        assert r["ssim"][0] == 1.0 and r["ms_ssim"][0] == 1.0 and r["sq_err"][0] == 0                   # a picture against itself
        lum = R.C1 / (255.0 ** 2 + R.C1)                                                                   # 255 against 0: every map is constant
        assert np.abs(r["terms"][1, :, :, 0] - 1.0).max() <= 1e-12 and np.abs(r["terms"][1, :, :, 1] - lum).max() <= 1e-12
        assert abs(r["ssim"][1] - lum) <= 1e-12 and r["sq_err"][1] == 255 ** 2 * 3 * S * S
        w = R.weights(L)
        assert abs(r["ms_ssim"][1] - lum ** w[L - 1]) <= 1e-12
        pq = (2 * 100 * 37 + R.C1) / (100 ** 2 + 37 ** 2 + R.C1)                                         # constants p, q: at every level
        assert np.abs(r["terms"][2, :, :, 1] - pq).max() <= 1e-12 and abs(r["ssim"][2] - pq) <= 1e-12
        ref = R.pairs_ref(x, x, [0, 3], [1, 4], L)
        assert np.abs(ref["terms"][0, :, :, 1] - lum).max() <= 1e-12 and np.abs(ref["terms"][1, :, :, 1] - pq).max() <= 1e-12
    assert R.pairs_ref(R.extremes(128), R.extremes(128), [0], [1], 1)["sq_err"][0] == 255 ** 2 * 3 * 128 * 128 > 2 ** 31
    p = metrics.psnr(np.array([0, 255 ** 2 * 3 * 64 * 64, 3 * 64 * 64, -1]), 64)
    assert p[0] == np.inf and p[1] == 0.0 and abs(p[2] - 20 * math.log10(255.0)) <= 1e-12 and np.isnan(p[3])
    for bad in (dict(levels=3), dict(levels=0)):
        with pytest.raises(ValueError):
            metrics.ssim_pairs(R.noise(2, 32, 1), R.noise(2, 32, 1), [0], [1], **bad)
    with pytest.raises(ValueError):
        metrics.ssim_pairs(R.noise(2, 10, 1), R.noise(2, 10, 1), [0], [1])
    with pytest.raises(ValueError):
        metrics.ssim_pairs(R.noise(2, 32, 1), R.noise(2, 16, 1), [0], [1])
    with pytest.raises(ValueError):
        metrics.ssim_pairs(R.noise(2, 32, 1).astype(np.float32), R.noise(2, 32, 1), [0], [1])
    with pytest.raises(ValueError):
        metrics.ssim_pairs(R.noise(2, 32, 1), R.noise(2, 32, 1), [0, 1], [1])


def test_default_and_max_levels():
    from hipgan.diversity import default_levels, max_levels
    assert [default_levels(S) for S in (11, 16, 22, 32, 48, 64, 128)] == [1, 1, 1, 2, 2, 3, 4]
    assert [max_levels(S) for S in (10, 11, 16, 22, 32, 33, 48, 64, 128, 129)] == [0, 1, 1, 2, 2, 1, 3, 3, 4, 0]


def test_draw_pairs():
    from hipgan._lib import JckError
    from hipgan.diversity import draw_pairs
    a, b = draw_pairs(50, 200, 7), draw_pairs(50, 200, 7)
    assert np.array_equal(a["i"], b["i"]) and np.array_equal(a["j"], b["j"]) and a["group"] is None and a["dropped"] == []
    assert a["i"].dtype == np.int64 and a["i"].shape == (200,) and (a["i"] != a["j"]).all()
    assert min(a["i"].min(), a["j"].min()) >= 0 and max(a["i"].max(), a["j"].max()) < 50
    g = np.random.default_rng(7)                                                  # the definition, written out
    i = g.integers(0, 50, 200)
    j = g.integers(0, 49, 200)
    j += j >= i
    assert np.array_equal(a["i"], i) and np.array_equal(a["j"], j)
    assert not np.array_equal(draw_pairs(50, 200, 8)["i"], a["i"])
    for p in (10, 11, 1000):                                                      # p >= n (n - 1) / 2: every pair once, in order
        e = draw_pairs(5, p, 3)
        assert list(zip(e["i"], e["j"])) == [(i, j) for i in range(5) for j in range(i + 1, 5)]
    assert draw_pairs(5, 9, 3)["i"].shape == (9,)
    groups = np.array([4, 2, 4, 9, 2, 4, 2, 4, 7, 2, 2, 2])                       # 2: six members, 4: four, 7 and 9: one each
    r = draw_pairs(12, 8, 1, groups)
    assert r["dropped"] == [7, 9] and r["group"].tolist() == [2] * 8 + [4] * 6    # class 4 has 6 pairs in all: every one of them
    assert (groups[r["i"]] == r["group"]).all() and (groups[r["j"]] == r["group"]).all() and (r["i"] != r["j"]).all()
    members = np.flatnonzero(groups == 4)
    assert list(zip(r["i"][8:], r["j"][8:])) == [(members[i], members[j]) for i in range(4) for j in range(i + 1, 4)]
    g = np.random.default_rng(1)                                                  # class 2 takes the first draws of the one generator
    i = g.integers(0, 6, 8)
    j = g.integers(0, 5, 8)
    j += j >= i
    assert np.array_equal(r["i"][:8], np.flatnonzero(groups == 2)[i]) and np.array_equal(r["j"][:8], np.flatnonzero(groups == 2)[j])
    for bad in (lambda: draw_pairs(1, 5, 0), lambda: draw_pairs(5, 0, 0), lambda: draw_pairs(3, 5, 0, [1, 2, 3]), lambda: draw_pairs(3, 5, 0, [1, 1])):
        with pytest.raises(JckError):
            bad()


def test_summarise_and_compare_on_numbers_worked_out_by_hand():
    from hipgan.diversity import compare, summarise, top_pairs
    s = summarise([0.2, 0.4, 0.6, 0.8, 0.5], [1, 1, 3, 3, 5])
    assert s["n"] == 5 and abs(s["mean"] - 0.5) <= 1e-15 and abs(s["sem"] - math.sqrt(0.05 / 5)) <= 1e-15        # var (ddof 1) = 0.2 / 4
    assert set(s["per_class"]) == {1, 3, 5}
    assert abs(s["per_class"][1]["mean"] - 0.3) <= 1e-15 and abs(s["per_class"][1]["sem"] - 0.1) <= 1e-15 and s["per_class"][1]["n"] == 2
    assert abs(s["per_class"][3]["mean"] - 0.7) <= 1e-15 and s["per_class"][5]["n"] == 1 and math.isnan(s["per_class"][5]["sem"])
    assert summarise(torch.tensor([0.25, 0.75]))["per_class"] == {} and summarise(torch.tensor([0.25, 0.75]))["mean"] == 0.5
    t = summarise([0.4, 0.2, 0.9, 0.9, 0.1], [1, 1, 3, 3, 4])                                             # class 1 as in s, 3: 0.9; 4 has no samples
    c = compare(s, t)
    assert set(c["per_class"]) == {1, 3} and c["per_class"][1]["less_diverse"] is False and c["per_class"][3]["less_diverse"] is False
    assert c["flagged"] == [] and c["share_less_diverse"] == 0.0 and c["overall"] is False                 # an equal mean is not less diverse
    c = compare(t, s)
    assert c["flagged"] == [3] and c["share_less_diverse"] == 0.5 and c["per_class"][3] == {"sample": 0.9, "train": s["per_class"][3]["mean"], "less_diverse": True}
    assert math.isnan(compare(summarise([0.5, 0.6]), summarise([0.1, 0.2]))["share_less_diverse"])
    assert top_pairs([0.1, 0.9, 0.5, 0.9, float("nan"), 0.2], 3).tolist() == [1, 3, 2] and top_pairs([0.1, 0.2], 5).tolist() == [1, 0]
    assert top_pairs([0.1, 0.2], 0).shape == (0,)


def test_ssim_entry_points_check_their_arguments_on_the_host():
    """JCK_E_ARG with a message before any HIP call (no GPU here); the pattern of test_abi's comm test"""
    from hipgan import _lib
    from hipgan.diversity import max_levels
    dll = _lib.load_library()
    for S in (0, 10, 11, 12, 16, 21, 22, 23, 32, 33, 44, 48, 64, 88, 96, 127, 128, 129, 256):
        assert dll.jck_ssim_max_levels(S) == max_levels(S), S
    assert [dll.jck_ssim_max_levels(S) for S in (10, 11, 22, 32, 48, 64, 128, 129)] == [0, 1, 2, 2, 3, 3, 4, 0]
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    good = [p, 4, p, 4, 32, p, p, 1, 2, p, p, p, None, None]      # (never passed whole: every call below has one bad argument)
    for hole in (0, 2, 5, 6, 9, 10, 11):
        args = list(good)
        args[hole] = None
        assert dll.jck_ssim_pairs_u8(*args) == JCK_E_ARG, hole
        assert b"ssim_pairs" in dll.jck_last_error() and b"null" in dll.jck_last_error()
    for S, L, word in ((10, 1, b"S must"), (129, 1, b"S must"), (32, 3, b"L must"), (33, 2, b"L must"), (32, 0, b"L must"), (128, 5, b"L must")):
        args = list(good)
        args[4], args[8] = S, L
        assert dll.jck_ssim_pairs_u8(*args) == JCK_E_ARG, (S, L)
        assert word in dll.jck_last_error()
    for P in (0, -1, (1 << 24) + 1):
        args = list(good)
        args[7] = P
        assert dll.jck_ssim_pairs_u8(*args) == JCK_E_ARG and b"P must" in dll.jck_last_error()
    for na, nb in ((0, 4), (4, 0), (-1, 4)):
        args = list(good)
        args[1], args[3] = na, nb
        assert dll.jck_ssim_pairs_u8(*args) == JCK_E_ARG and b"na and nb" in dll.jck_last_error()


def test_diversity_parser_defaults_refusals_and_help(capsys):
    import diversity
    base = ["--checkpoint", "c.pt", "--out", "o"]
    a = diversity.get_arg_parse(base)
    assert (a.model, a.num, a.pairs, a.top, a.seed, a.which, a.batch_size, a.prec) == ("DCGAN", 2000, 1000, 16, 0, "auto", 64, "bf16")
    assert a.levels is None and a.train is None and a.classes is None and a.compare is None and a.truncation is None
    a = diversity.get_arg_parse(base + ["-m", "CGAN", "--classes", "3,17,42", "--num", "200", "--pairs", "50", "--train", "t.npz", "--levels", "2"])
    assert (a.model, a.classes, a.num, a.pairs, a.train, a.levels) == ("CGAN", [3, 17, 42], 200, 50, "t.npz", 2)
    a = diversity.get_arg_parse(["--compare", "a.npz:recon", "dir.x/b.npz", "--out", "o"])
    assert a.compare == [("a.npz", "recon"), ("dir.x/b.npz", "images")]
    assert diversity.split_key("C:/x/a.npz") == ("C:/x/a.npz", "images") and diversity.split_key("a.npz:z") == ("a.npz", "z")
    for bad in (["--num", "1"], ["--pairs", "0"], ["--top", "-1"], ["-b", "0"], ["--levels", "0"], ["--levels", "5"], ["--truncation", "0"],
                ["--classes", "3"], ["-m", "CGAN"], ["-m", "CGAN", "--classes", "100"], ["-m", "CGAN", "--classes", "a,b"], ["-m", "CGAN", "--classes", "-1"],
                ["--compare", "a.npz", "b.npz"], ["--which", "x"]):
        with pytest.raises(SystemExit):
            diversity.get_arg_parse(base + bad)
    for argv in (["--out", "o"], ["--checkpoint", "c.pt"], ["--compare", "a.npz", "--out", "o"], ["--compare", "a.npz", "b.npz", "--out", "o", "--train", "t.npz"]):
        with pytest.raises(SystemExit):
            diversity.get_arg_parse(argv)
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        diversity.get_arg_parse(["--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    assert "--compare" in text and "diversity.json" in text and "share_less_diverse" in text


def test_compare_run_on_the_host(tmp_path):
    """--compare needs no checkpoint, and without a GPU no device: a file against itself is inf / 1 / 1 / 0"""
    import json
    tol = R.TOL if torch.cuda.is_available() else 1e-12              # (where there is a GPU the run goes through the kernel)
    import diversity
    x = R.smooth(3, 32, seed=4)
    np.savez(str(tmp_path / "a.npz"), images=x, other=R.jitter(x, 5))
    assert diversity.main(["--compare", str(tmp_path / "a.npz"), str(tmp_path / "a.npz"), "--out", str(tmp_path / "same")]) == 0
    f = np.load(str(tmp_path / "same" / "compare.npz"))
    assert sorted(f.files) == ["ms_ssim", "psnr", "sq_err", "ssim"]
    assert (f["psnr"] == np.inf).all() and (f["ssim"] == 1).all() and (f["ms_ssim"] == 1).all() and (f["sq_err"] == 0).all()
    assert diversity.main(["--compare", str(tmp_path / "a.npz"), str(tmp_path / "a.npz") + ":other", "--out", str(tmp_path / "cmp")]) == 0
    f = np.load(str(tmp_path / "cmp" / "compare.npz"))
    rec = json.load(open(str(tmp_path / "cmp" / "compare.json")))
    ref = R.pairs_ref(x, R.jitter(x, 5), range(3), range(3), 2)
    assert np.abs(f["ssim"] - ref["ssim"]).max() <= tol and np.array_equal(f["sq_err"], ref["sq_err"])
    assert set(rec) == {"n", "size", "psnr", "ssim", "ms_ssim", "sq_err"} and abs(rec["ssim"] - ref["ssim"].mean()) <= tol
    assert abs(rec["psnr"] - np.mean(10 * np.log10(255.0 ** 2 * 3 * 32 * 32 / ref["sq_err"]))) <= 1e-9
