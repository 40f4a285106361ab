"""The SSIM / MS-SSIM pair kernel (csrc/ssim.hip) and the layers above it, on the GPU.  The reference is tests/ssim_ref.py (fp64).  The
geometries (S, L) are the smallest at which something can go wrong: (11, 1) a 1 x 1 map and 3 S^2 odd, (16, 1), (22, 2) a last level of
11 with a 1 x 1 map, (32, 2), (48, 3) a last level of 12, (64, 1) and (64, 3) one column per lane at its limit, (128, 4) two columns per
lane, the LDS limit and a squared error beyond 2^31.

Tolerance of the floats: 5e-5 absolute (ssim_ref.TOL).  It comes from the reference side: an fp32 emulation of the definition differs
from fp64 by at most 9.0e-6 on these input kinds (worst: the flat picture with one changed pixel); 5x that allows for the device's order
of addition.  The MI355X run showed at most 2.8e-7 (terms, at S = 11) with the planes centred as DESIGN 5.16 describes, and 8.2e-5 on
the flat pair at S = 11 before that; the first test prints its worst figures per geometry."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import ssim_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "jck-generation_amd")
GEOMETRIES = ((11, 1), (16, 1), (22, 2), (32, 2), (48, 3), (64, 1), (64, 3), (128, 4))
SENT_F, SENT_I = -77.25, -55


def dev_u8(x, offset=0):
    """the pictures on the device; offset: as a view that starts `offset` bytes into its allocation"""
    x = np.ascontiguousarray(x)
    buf = torch.empty(x.size + offset, dtype=torch.uint8, device="cuda")
    view = buf[offset:].view(x.shape)
    view.copy_(torch.from_numpy(x))
    assert view.data_ptr() % 16 == (buf.data_ptr() + offset) % 16
    return view


def run(a, b, ia, ib, S, L, with_terms=True):
    """jck_ssim_pairs_u8 into sentinel-filled outputs with a guard row each -> host dict; the guard rows are compared here"""
    from hipgan._lib import cur_stream, lib
    P = len(ia)
    idx = lambda v: torch.as_tensor(np.asarray(v, dtype=np.int64)).cuda()
    ssim = torch.full((P + 1,), SENT_F, dtype=torch.float32, device="cuda")
    ms = torch.full((P + 1,), SENT_F, dtype=torch.float32, device="cuda")
    sq = torch.full((P + 1,), SENT_I, dtype=torch.int64, device="cuda")
    terms = torch.full((P + 1, 3, L, 2), SENT_F, dtype=torch.float32, device="cuda")
    lib.jck_ssim_pairs_u8(a, a.shape[0], b, b.shape[0], S, idx(ia), idx(ib), P, L, ssim, ms, sq, terms if with_terms else None, cur_stream())
    ssim, ms, sq, terms = ssim.cpu().numpy(), ms.cpu().numpy(), sq.cpu().numpy(), terms.cpu().numpy()
    assert ssim[P] == SENT_F and ms[P] == SENT_F and sq[P] == SENT_I and (terms[P] == SENT_F).all()          # nothing past [P]
    if not with_terms:
        assert (terms == SENT_F).all()
    return {"ssim": ssim[:P], "ms_ssim": ms[:P], "sq_err": sq[:P], "terms": terms[:P]}


def same_bits(r, p, q, rq=None):
    rq = r if rq is None else rq
    return all(r[k][p].tobytes() == rq[k][q].tobytes() for k in ("ssim", "ms_ssim", "sq_err", "terms"))


@pytest.fixture(scope="module")
def cases():
    """per geometry: the pictures, the 46 pairs, their reference (computed once) and a list of 67 pairs made of them and their swaps"""
    out = {}
    for S, L in GEOMETRIES:
        x, ia, ib, like = R.case_set(S, seed=1000 + S)
        ref = R.pairs_ref(x, x, ia, ib, L)
        g = np.random.default_rng(S + L)
        pick = np.concatenate([np.arange(46), g.integers(0, 46, size=21)])          # every pair, then 21 of them once more ...
        swap = np.arange(67) >= 46                                                   # ... the other way round (the reference is symmetric)
        out[S, L] = {"x": x, "ia": ia, "ib": ib, "like": like, "ref": ref, "pick": pick,
                     "ia67": np.where(swap, ib[pick], ia[pick]), "ib67": np.where(swap, ia[pick], ib[pick])}
    return out


@pytest.mark.parametrize("S,L", GEOMETRIES)
def test_outputs_against_the_reference(cases, S, L):
    """P = 1, 5, 67; a and b the same buffer, two buffers, and views one byte into their allocations: terms, ssim and sq_err of every
    pair against the reference; ms_ssim tightly against the reference's combine step on the kernel's own terms, and against the full
    reference where no reference term lies within 1e-3 of zero (max(t, 0)^w has no bounded slope there)"""
    c = cases[S, L]
    ref, pick = c["ref"], c["pick"]
    bufs = {"same": (dev_u8(c["x"]),) * 2, "two": (dev_u8(c["x"]), dev_u8(c["x"])), "offset": (dev_u8(c["x"], 1), dev_u8(c["x"], 1))}
    worst = {"terms": 0.0, "ssim": 0.0, "ms_own": 0.0, "ms_ref": 0.0}
    far = (np.abs(ref["terms"]) > 1e-3).all(axis=(1, 2, 3))
    left_out = int((~far[c["like"]]).sum())
    for name, (a, b) in bufs.items():
        for P in (1, 5, 67):
            first = 0 if P == 67 else 40 - P // 2                                   # P = 5: smooth pairs and the special ones
            sel = pick[first:first + P]
            r = run(a, b, c["ia67"][first:first + P], c["ib67"][first:first + P], S, L)
            assert np.array_equal(r["sq_err"], ref["sq_err"][sel]), (name, P)
            own = np.array([R.combine(t)[1] for t in r["terms"].astype(np.float64)])
            keep = far[sel]
            worst["terms"] = max(worst["terms"], float(np.abs(r["terms"] - ref["terms"][sel]).max()))
            worst["ssim"] = max(worst["ssim"], float(np.abs(r["ssim"] - ref["ssim"][sel]).max()))
            worst["ms_own"] = max(worst["ms_own"], float(np.abs(r["ms_ssim"] - own).max()))
            if keep.any():
                worst["ms_ref"] = max(worst["ms_ref"], float(np.abs(r["ms_ssim"] - ref["ms_ssim"][sel])[keep].max()))
    print(f"S={S} L={L}: worst |terms - ref| {worst['terms']:.3e}, |ssim - ref| {worst['ssim']:.3e}, |ms - combine(own terms)| {worst['ms_own']:.3e}, "
          f"|ms - ref| {worst['ms_ref']:.3e}; {left_out} of 40 smooth pairs left out of the last")
    assert worst["terms"] <= R.TOL and worst["ssim"] <= R.TOL and worst["ms_own"] <= 1e-5 and worst["ms_ref"] <= R.TOL
    assert left_out <= 4                                                            # at most 10 % of the smooth / blend pairs
    if (S, L) == (128, 4):
        assert ref["sq_err"][43] == 255 ** 2 * 3 * 128 * 128 > 2 ** 31              # the extremes: beyond 32 bits


@pytest.mark.parametrize("S,L", GEOMETRIES)
def test_exact_properties(cases, S, L):
    c = cases[S, L]
    a, copy = dev_u8(c["x"]), dev_u8(c["x"], 1)
    n = c["x"].shape[0]
    # equal pictures, through the same pointer and through a copy (at another alignment): exactly 1.0f, 1.0f, 0
    every = np.arange(n)
    for b in (a, copy):
        r = run(a, b, every, every, S, L)
        assert (r["ssim"] == 1.0).all() and (r["ms_ssim"] == 1.0).all() and (r["sq_err"] == 0).all() and (r["terms"] == 1.0).all()
    # swapped pairs: equal bits in every output
    fwd, bwd = run(a, a, c["ia"], c["ib"], S, L), run(a, copy, c["ib"], c["ia"], S, L)
    assert all(same_bits(fwd, p, p, bwd) for p in range(46))
    # a pair's bits do not depend on the list: the list of 67, that list reversed, and the pair alone
    r67 = run(a, a, c["ia67"], c["ib67"], S, L)
    rev = run(a, a, c["ia67"][::-1].copy(), c["ib67"][::-1].copy(), S, L)
    assert all(same_bits(r67, p, 66 - p, rev) for p in range(67))
    assert all(same_bits(r67, p, int(c["pick"][p]), fwd) for p in range(67))        # (46..66 are swaps of pairs of fwd)
    for p in (0, 41, 43, 66):
        alone = run(a, a, c["ia67"][p:p + 1], c["ib67"][p:p + 1], S, L)
        assert same_bits(r67, p, 0, alone), p
    none = run(a, a, c["ia67"], c["ib67"], S, L, with_terms=False)                  # no terms buffer: the same three outputs
    assert all(none[k].tobytes() == r67[k].tobytes() for k in ("ssim", "ms_ssim", "sq_err"))
    # an index outside its array: NaN / NaN / -1 for that pair, every other pair unchanged
    for which, bad in (("ia", n), ("ib", n), ("ia", -1), ("ib", 1 << 40)):
        ia, ib = c["ia67"].copy(), c["ib67"].copy()
        (ia if which == "ia" else ib)[[3, 66]] = bad
        r = run(a, a, ia, ib, S, L)
        for p in range(67):
            if p in (3, 66):
                assert np.isnan(r["ssim"][p]) and np.isnan(r["ms_ssim"][p]) and r["sq_err"][p] == -1 and np.isnan(r["terms"][p]).all()
            else:
                assert same_bits(r, p, p, r67), (which, bad, p)
        r = run(a, a, ia, ib, S, L, with_terms=False)
        assert np.isnan(r["ssim"][[3, 66]]).all() and (r["sq_err"][[3, 66]] == -1).all()


def test_bad_arguments_are_refused_before_any_launch():
    from hipgan._lib import JckError, cur_stream, lib
    a = dev_u8(R.noise(3, 32, 1))
    idx = torch.zeros(2, dtype=torch.int64, device="cuda")
    f = torch.full((2,), SENT_F, dtype=torch.float32, device="cuda")
    q = torch.full((2,), SENT_I, dtype=torch.int64, device="cuda")
    good = [a, 3, a, 3, 32, idx, idx, 2, 2, f, f, q, None]
    for hole, value in ((0, None), (2, None), (5, None), (6, None), (9, None), (10, None), (11, None), (1, 0), (3, 0), (4, 10), (4, 129), (7, 0),
                        (7, (1 << 24) + 1), (8, 0), (8, 3)):
        args = list(good)
        args[hole] = value
        with pytest.raises(JckError):
            lib.jck_ssim_pairs_u8(*args, cur_stream())
    torch.cuda.synchronize()
    assert (f == SENT_F).all() and (q == SENT_I).all()


def test_device_path_of_the_twin_equals_the_raw_call(cases):
    import metrics
    for S, L in ((32, 2), (64, 3)):
        c = cases[S, L]
        a = dev_u8(c["x"])
        raw = run(a, a, c["ia67"], c["ib67"], S, L)
        got = metrics.ssim_pairs(a, a, c["ia67"], torch.as_tensor(c["ib67"]), levels=L, terms=True)
        assert all(got[k].is_cuda for k in got) and got["sq_err"].dtype == torch.int64 and got["terms"].shape == (67, 3, L, 2)
        assert all(got[k].cpu().numpy().tobytes() == raw[k].tobytes() for k in raw)
        mixed = metrics.ssim_pairs(c["x"], a, c["ia67"], c["ib67"])                  # a host array beside a device one, the default levels
        assert "terms" not in mixed and all(mixed[k].cpu().numpy().tobytes() == raw[k].tobytes() for k in mixed)
        p = metrics.psnr(got["sq_err"], S)
        assert p.shape == (67,) and (p[raw["sq_err"] == 0] == np.inf).all() and np.isfinite(p[raw["sq_err"] > 0]).all()


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """a tiny seeded checkpoint (as test_cluster_gpu builds it) and a training file of uniform random pictures"""
    from hipgan.engine import DcganEngine
    from hipgan.sampler import Sampler
    from oracle.gan_oracle import GanOracle
    d = tmp_path_factory.mktemp("diversity")
    orc = GanOracle("dcgan", lr=2e-4, seed=12345)
    eng = DcganEngine(batch=8, prec="bf16")
    eng.load_state(orc.g, orc.d)
    gen = torch.Generator().manual_seed(9)
    for _ in range(30):          # running statistics that belong to the weights
        eng.sample(torch.randn(8, 100, generator=gen))
    gs, ds = eng.state_dicts()
    ckpt = str(d / "plain.pt")
    torch.save({"model_g": gs, "model_d": ds}, ckpt)
    train = np.random.default_rng(91).integers(0, 256, size=(24, 64, 64, 3), dtype=np.uint8)
    np.savez(str(d / "train.npz"), images=train)
    return {"dir": d, "ckpt": ckpt, "sampler": Sampler.from_checkpoint(ckpt, "DCGAN", batch=8), "train": train}


def test_sampler_diversity(trained, monkeypatch):
    import metrics
    from hipgan import sampler as sampler_mod
    from hipgan._lib import JckError
    s, train = trained["sampler"], trained["train"]
    r = s.diversity(32, pairs=40, seed=3, train_u8=train, top=5)
    again = s.diversity(32, pairs=40, seed=3, train_u8=train, top=5)
    assert r["levels"] == 3 and r["images"].shape == (32, 64, 64, 3) and r["images"].is_cuda and r["z"].shape == (32, 100)
    assert r["ssim"].shape == (40,) and r["pairs"]["group"].tolist() == [0] * 40 and r["dropped"] == [] and r["top"].shape == (5,)
    for key in ("ssim", "ms_ssim", "sq_err"):                                        # reproducible bit for bit
        assert r[key].tobytes() == again[key].tobytes() and r["train"][key].tobytes() == again["train"][key].tobytes()
    assert torch.equal(r["images"], again["images"]) and np.array_equal(r["top"], again["top"])
    host = metrics.ssim_pairs(r["images"].cpu().numpy(), r["images"].cpu().numpy(), r["pairs"]["i"], r["pairs"]["j"], levels=3)
    assert np.abs(r["ssim"] - host["ssim"]).max() <= R.TOL and np.array_equal(r["sq_err"], host["sq_err"])
    far = np.abs(metrics.ssim_pairs(r["images"].cpu().numpy(), r["images"].cpu().numpy(), r["pairs"]["i"], r["pairs"]["j"], levels=3,
                                    terms=True)["terms"]).reshape(40, -1).min(axis=1) > 1e-3
    assert not far.any() or np.abs(r["ms_ssim"] - host["ms_ssim"])[far].max() <= R.TOL
    ms = r["summary"]["ms_ssim"]
    assert ms["n"] == 40 and abs(ms["mean"] - r["ms_ssim"].astype(np.float64).mean()) <= 1e-12 and ms["per_class"][0]["n"] == 40
    assert r["top"].tolist() == np.argsort(-r["ms_ssim"].astype(np.float64), kind="stable")[:5].tolist()
    t = r["train"]
    assert t["ssim"].shape == (40,) and max(t["pairs"]["i"].max(), t["pairs"]["j"].max()) < 24 and set(r["comparison"]["per_class"]) == {0}
    assert r["comparison"]["per_class"][0]["less_diverse"] == (ms["mean"] > t["summary"]["ms_ssim"]["mean"])
    assert "train" not in s.diversity(8, pairs=5) and s.diversity(8, pairs=5, levels=1)["levels"] == 1
    with pytest.raises(JckError):
        s.diversity(1)
    # every latent the same: every sample the same picture, mean exactly 1, the one class flagged against any training set with variety
    plain = sampler_mod.latents
    monkeypatch.setattr(sampler_mod, "latents", lambda n, seed, truncation=None, generator=None: plain(1, seed, truncation).expand(n, -1).contiguous())
    flat = s.diversity(32, pairs=40, seed=3, train_u8=train)
    assert (flat["ms_ssim"] == 1.0).all() and (flat["ssim"] == 1.0).all() and (flat["sq_err"] == 0).all()
    assert flat["summary"]["ms_ssim"]["mean"] == 1.0 and flat["summary"]["ssim"]["per_class"][0]["mean"] == 1.0
    assert flat["comparison"]["flagged"] == [0] and flat["comparison"]["share_less_diverse"] == 1.0 and flat["comparison"]["overall"] is True


def test_diversity_cli_and_compare(trained):
    d = trained["dir"]
    out = d / "out"
    r = subprocess.run([sys.executable, "diversity.py", "-m", "DCGAN", "--checkpoint", trained["ckpt"], "--train", str(d / "train.npz"), "--num", "32",
                        "--pairs", "40", "--top", "6", "-b", "8", "--out", str(out)], cwd=PKG, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    rec = json.load(open(str(out / "diversity.json")))
    assert set(rec) == {"levels", "n", "pairs", "samples", "train", "share_less_diverse", "flagged", "dropped"}
    assert rec["levels"] == 3 and rec["n"] == 32 and rec["pairs"] == 40 and rec["dropped"] == [] and rec["share_less_diverse"] in (0.0, 1.0)
    for side in ("samples", "train"):
        assert set(rec[side]) == {"ms_ssim", "ssim"} and set(rec[side]["ms_ssim"]) == {"mean", "sem", "n", "per_class"}
        assert rec[side]["ms_ssim"]["n"] == 40 and set(rec[side]["ssim"]["per_class"]) == {"0"}
    f = np.load(str(out / "diversity.npz"))
    assert sorted(f.files) == sorted(["i", "j", "group", "ssim", "ms_ssim", "sq_err", "top", "train_i", "train_j", "train_group", "train_ssim",
                                      "train_ms_ssim", "train_sq_err"])
    assert f["i"].shape == (40,) and f["ms_ssim"].dtype == np.float32 and f["sq_err"].dtype == np.int64 and f["top"].shape == (6,)
    assert abs(rec["samples"]["ms_ssim"]["mean"] - f["ms_ssim"].astype(np.float64).mean()) <= 1e-12
    same = trained["sampler"].diversity(32, pairs=40, seed=0, train_u8=trained["train"], top=6)      # the script is the method
    assert f["ms_ssim"].tobytes() == same["ms_ssim"].tobytes() and f["train_ssim"].tobytes() == same["train"]["ssim"].tobytes()
    png = open(str(out / "diversity.png"), "rb").read()
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    w, h = int.from_bytes(png[16:20], "big"), int.from_bytes(png[20:24], "big")
    assert (w, h) == (8 * 66 + 2, 2 * 66 + 2)                                       # 6 pairs, four a row, padding 2
    line = [l for l in r.stdout.splitlines() if l.startswith("diversity: ")]
    assert len(line) == 1
    m = re.match(r"diversity: MS-SSIM ([0-9.]+) \+- ([0-9.]+) over 40 pairs \(train ([0-9.]+)\), ([01]) of 1 classes less diverse", line[0])
    assert m and abs(float(m.group(1)) - rec["samples"]["ms_ssim"]["mean"]) <= 5e-5 and int(m.group(4)) == len(rec["flagged"])
    # --compare: a file against itself is inf / 1 / 1 / 0; against another key the reference's numbers
    x = R.smooth(5, 64, seed=4)
    np.savez(str(d / "a.npz"), images=x, other=R.jitter(x, 5))
    cmp_ = d / "cmp"
    r = subprocess.run([sys.executable, "diversity.py", "--compare", str(d / "a.npz"), str(d / "a.npz"), "--out", str(cmp_)], cwd=PKG,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    f = np.load(str(cmp_ / "compare.npz"))
    assert sorted(f.files) == ["ms_ssim", "psnr", "sq_err", "ssim"] and f["psnr"].shape == (5,)
    assert (f["psnr"] == np.inf).all() and (f["ssim"] == 1).all() and (f["ms_ssim"] == 1).all() and (f["sq_err"] == 0).all()
    rec = json.load(open(str(cmp_ / "compare.json")))
    assert set(rec) == {"n", "size", "psnr", "ssim", "ms_ssim", "sq_err"} and rec["n"] == 5 and rec["size"] == 64 and rec["ssim"] == 1.0
    import diversity
    assert diversity.main(["--compare", str(d / "a.npz"), str(d / "a.npz") + ":other", "--out", str(d / "cmp2")]) == 0
    f = np.load(str(d / "cmp2" / "compare.npz"))
    ref = R.pairs_ref(x, R.jitter(x, 5), range(5), range(5), 3)
    assert np.abs(f["ssim"] - ref["ssim"]).max() <= R.TOL and np.abs(f["ms_ssim"] - ref["ms_ssim"]).max() <= R.TOL
    assert np.array_equal(f["sq_err"], ref["sq_err"]) and np.abs(f["psnr"] - 10 * np.log10(255.0 ** 2 * 3 * 64 * 64 / ref["sq_err"])).max() <= 1e-9
