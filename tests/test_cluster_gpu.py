"""The per-cluster sum kernels (csrc/cluster.hip) and the layers above them, on the GPU.  On integer-valued data (|x| <= 3, at most a few
thousand rows) every sum is below 2^24, so any order is exact and sum, count and centre must EQUAL the fp64 reference; on real-valued
data the bits of a cluster's sum must depend on that cluster's rows alone, and every entry lies within the bound of a recursive sum in
any order.  The reference arithmetic is tests/cluster_ref.py.  A piece is R = jck_segment_chunk_rows() rows: R - 1 / R / R + 1 / 2R + 1
straddle it; 63 / 64 / 65 / 257 straddle the wave and the strip of the counting sort."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from cluster_ref import U32, blobs, kmeans_ref, segment_ref
from pairstats_ref import int_features
from test_neighbours_gpu import dev, dev_offset

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "jck-generation_amd")
SENT_F, SENT_I = -77.25, -55


def chunk_rows():
    from hipgan._lib import load_library
    return load_library().jck_segment_chunk_rows()


def seg(x, labels, k, with_centre=True):
    """jck_segment_mean_f32 into sentinel-filled outputs with a guard row each -> host (sum [k,D], count [k], centre [k,D]); the guard
    rows are compared here"""
    from hipgan._lib import cur_stream, lib, load_library
    n, d = x.shape
    lab = torch.as_tensor(np.asarray(labels, dtype=np.int64)).cuda()
    total = torch.full((k + 1, d), SENT_F, dtype=torch.float32, device="cuda")
    count = torch.full((k + 1,), SENT_I, dtype=torch.int32, device="cuda")
    centre = torch.full((k + 1, d), SENT_F, dtype=torch.float32, device="cuda")
    nbytes = load_library().jck_segment_ws_bytes(n, d, k)
    assert nbytes > 0
    ws = torch.empty(nbytes // 4 + 1, dtype=torch.float32, device="cuda")
    lib.jck_segment_mean_f32(x, n, d, lab, k, total, count, centre if with_centre else None, ws, cur_stream())
    total, count, centre = total.cpu().numpy(), count.cpu().numpy(), centre.cpu().numpy()
    assert (total[k] == SENT_F).all() and count[k] == SENT_I and (centre[k] == SENT_F).all()      # nothing past [K][D]
    if not with_centre:
        assert (centre == SENT_F).all()
    return total[:k], count[:k], centre[:k]


def check_exact(xh, xd, labels, k):
    """sum, count and centre equal the reference; empty clusters: zeros and an untouched centre row; skipped rows counted nowhere"""
    labels = np.asarray(labels)
    total, count, centre = seg(xd, labels, k)
    rt, rc, rcen = segment_ref(xh, labels, k, np.full((k, xh.shape[1]), SENT_F, np.float32))
    assert np.array_equal(count, rc)
    assert np.array_equal(total.astype(np.float64), rt)
    assert np.array_equal(centre, rcen)
    empty = rc == 0
    assert (total[empty] == 0).all() and (count[empty] == 0).all() and (centre[empty] == SENT_F).all()
    assert count.sum() == ((labels >= 0) & (labels < k)).sum()


@pytest.mark.parametrize("D,offset", [(1, False), (5, False), (64, False), (260, False), (64, True)])
def test_sums_are_bit_exact_on_integer_features_at_every_edge(D, offset):
    """N over the wave, piece and strip edges, K from 1 to the limit (K > N: most clusters empty), the scalar path (D = 1, 5, or a base
    one float off a 16-byte boundary) and the 16-byte path (D = 64; D = 260: a second workgroup of columns)"""
    xh = int_features(1000, D, seed=11)
    xd = (dev_offset if offset else dev)(xh)
    g = np.random.default_rng(12)
    for n in (1, 63, 64, 65, 257, 1000):
        for k in (1, 2, 100, 1024):
            check_exact(xh[:n], xd[:n], g.integers(0, k, size=n), k)


@pytest.mark.parametrize("D", [5, 64])
def test_label_patterns_around_the_piece_size(D):
    R = chunk_rows()
    assert R >= 1
    xh = int_features(6 * R + 40, D, seed=21)
    xd = dev(xh)
    n = xh.shape[0]
    g = np.random.default_rng(22)
    check_exact(xh, xd, np.zeros(n, np.int64), 1)                            # all one cluster
    check_exact(xh, xd, np.full(n, 37), 100)                                 # ... which is not the first
    for rows in (R - 1, R, R + 1, 2 * R + 1):                                # one cluster of exactly `rows` among others
        for k in (2, 100):
            labels = g.integers(0, k - 1, size=n)
            labels[labels >= 1] += 1                                         # 0, 2 .. k-1: cluster 1 is kept free (k = 2: all others in cluster 0)
            labels[g.permutation(n)[:rows]] = 1
            assert (labels == 1).sum() == rows
            check_exact(xh, xd, labels, k)
    # labels -1 and K are skipped, in a strip of their own and among the others; every row skipped: all zeros
    labels = g.integers(0, 7, size=n)
    labels[:70] = -1
    labels[g.permutation(n)[:50]] = 7
    labels[g.permutation(n)[:50]] = -1
    check_exact(xh, xd, labels, 7)
    check_exact(xh, xd, np.full(n, -1), 3)
    check_exact(xh, xd, np.full(n, 1 << 40), 3)                              # an int64 label beyond 32 bits is out of range, not cluster 0
    total, count, centre = seg(xd, labels, 7, with_centre=False)             # no centre: sums and counts alone
    rt, rc, _ = segment_ref(xh, labels, 7)
    assert np.array_equal(total.astype(np.float64), rt) and np.array_equal(count, rc)


def test_bad_arguments_are_refused_before_any_launch():
    from hipgan._lib import JckError, cur_stream, lib
    xd = dev(int_features(65, 8, seed=31))
    lab = torch.zeros(65, dtype=torch.int64, device="cuda")
    total = torch.full((3, 8), SENT_F, dtype=torch.float32, device="cuda")
    count = torch.full((3,), SENT_I, dtype=torch.int32, device="cuda")
    ws = torch.empty(1 << 16, dtype=torch.float32, device="cuda")
    for args in ((None, 65, 8, lab, 3, total, count, None, ws), (xd, 65, 8, None, 3, total, count, None, ws), (xd, 65, 8, lab, 3, None, count, None, ws),
                 (xd, 65, 8, lab, 3, total, None, None, ws), (xd, 65, 8, lab, 3, total, count, None, None), (xd, 0, 8, lab, 3, total, count, None, ws),
                 (xd, 65, 0, lab, 3, total, count, None, ws), (xd, 65, 8, lab, 0, total, count, None, ws), (xd, 65, 8, lab, 1025, total, count, None, ws)):
        with pytest.raises(JckError):
            lib.jck_segment_mean_f32(*args, cur_stream())
    torch.cuda.synchronize()
    assert (total == SENT_F).all() and (count == SENT_I).all()


@pytest.fixture(scope="module")
def real_case():
    """1000 standard normal rows in 7 clusters (about 143 rows each: three pieces), D = 260 on the 16-byte path and D = 5 on the scalar one"""
    g = np.random.default_rng(41)
    out = {}
    for D in (260, 5):
        xh = g.standard_normal((1000, D)).astype(np.float32)
        labels = g.integers(0, 7, size=1000)
        out[D] = (xh, dev(xh), labels, seg(dev(xh), labels, 7))
    return out


@pytest.mark.parametrize("D", [260, 5])
def test_a_clusters_sum_depends_on_its_own_rows_only(real_case, D):
    xh, xd, labels, (total, count, centre) = real_case[D]
    again = seg(xd, labels, 7)
    assert all(a.tobytes() == b.tobytes() for a, b in zip((total, count, centre), again))        # two identical calls
    g = np.random.default_rng(42)
    for c in (0, 3, 6):
        rows = np.flatnonzero(labels == c)
        assert rows.size > chunk_rows()
        alone = seg(dev(xh[rows]), np.zeros(rows.size, np.int64), 1)                              # N = n_c, K = 1
        assert alone[0][0].tobytes() == total[c].tobytes() and alone[1][0] == count[c] and alone[2][0].tobytes() == centre[c].tobytes()
        other = labels.copy()                                                                     # the other rows' labels permuted, K larger
        rest = np.flatnonzero(labels != c)
        other[rest] = g.permutation(np.where(labels[rest] > c, labels[rest] + 20, labels[rest]))
        mixed = seg(xd, other, 40)
        assert mixed[0][c].tobytes() == total[c].tobytes() and mixed[2][c].tobytes() == centre[c].tobytes()


@pytest.mark.parametrize("D", [260, 5])
def test_real_valued_sums_lie_within_the_bound_of_a_recursive_sum(real_case, D):
    """|sum - exact| <= gamma_(n_c - 1) sum_i |x_ij| with gamma_m = m u / (1 - m u), u = 2^-24: the bound of n_c - 1 rounded additions
    in ANY order (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2).  Every (c, j) is compared; exact: the fp64 sum."""
    xh, xd, labels, (total, count, centre) = real_case[D]
    x64 = xh.astype(np.float64)
    worst = 0.0
    for c in range(7):
        rows = labels == c
        m = int(rows.sum()) - 1
        gamma = m * U32 / (1.0 - m * U32)
        exact, mass = x64[rows].sum(0), np.abs(x64[rows]).sum(0)
        err = np.abs(total[c].astype(np.float64) - exact)
        worst = max(worst, float((err / (gamma * mass)).max()))
        assert (err <= gamma * mass).all(), c
        assert np.array_equal(centre[c], total[c] / np.float32(count[c]))                          # the correctly rounded quotient
    print(f"D={D}: worst error over its bound {worst:.3e}")


def same_result(a, b):
    host = lambda v: v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
    return all(np.array_equal(host(a[key]), host(b[key])) for key in ("labels", "count", "centres")) and a["iters"] == b["iters"]


def test_kmeans_on_the_device_equals_kmeans_on_the_host():
    """blobs of integers separated by 16: the seeding distances are exact integers in both paths and no assignment is near a tie, so
    the twins return EQUAL labels, counts, iterations and centres - every row compared"""
    from hipgan.cluster import kmeans
    for seed in (0, 1):
        x, blob = blobs(seed=3 + seed)
        host = kmeans(x, 6, seed=seed)
        on_dev = kmeans(dev(x), 6, seed=seed)
        assert on_dev["centres"].is_cuda and on_dev["labels"].dtype == torch.int64 and on_dev["count"].dtype == torch.int64
        assert same_result(on_dev, host) and same_result(on_dev, kmeans_ref(x, 6, 50, seed))
        # the first inertia is a sum of exact integers in both; later ones are distances to fp32 quotients, which the device rounds in
        # fp32: within metrics.nearest's (D + 4) 2^-24 relative of the host's fp64
        assert on_dev["history"][0] == host["history"][0] and len(on_dev["history"]) == len(host["history"])
        assert all(abs(a - b) <= 12 * U32 * b for a, b in zip(on_dev["history"], host["history"]))
        assert (on_dev["count"] == 40).all() and on_dev["iters"] < 50
        for chunk in (1, 4, 100):                                                                 # the centres walked in chunks
            assert same_result(kmeans(dev(x), 6, seed=seed, chunk=chunk), host), chunk
    x, _ = blobs(seed=5)
    for k, rows in ((1, x), (9, x[:9]), (4, np.repeat(x[:2], 4, axis=0))):                        # k = 1, k = N, duplicates (total 0 while seeding)
        assert same_result(kmeans(dev(rows), k, seed=2), kmeans(rows, k, seed=2)), k
    from hipgan._lib import JckError
    bad = x.copy()
    bad[5, 1] = np.nan
    with pytest.raises(JckError):
        kmeans(dev(bad), 3)
    import metrics
    labels = np.random.default_rng(51).integers(-1, 7, size=240)
    got = metrics.segment_mean(dev(x), labels, 6, centre=np.full((6, 8), 2.5, np.float32))         # the twins of segment_mean itself
    want = metrics.segment_mean(x, labels, 6, centre=np.full((6, 8), 2.5, np.float32))
    assert got[0].is_cuda and got[1].dtype == torch.int32 and all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(got, want))


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """a tiny seeded checkpoint (as test_generate_cli_neighbours builds it) and a training file: 48 of the sampler's own pictures and
    48 uniform random ones"""
    from hipgan.engine import DcganEngine
    from hipgan.sampler import Sampler, latents
    from oracle.gan_oracle import GanOracle
    d = tmp_path_factory.mktemp("modes")
    orc = GanOracle("dcgan", lr=2e-4, seed=12345)
    eng = DcganEngine(batch=8, prec="bf16")
    eng.load_state(orc.g, orc.d)
    gen = torch.Generator().manual_seed(9)
    for _ in range(30):          # running statistics that belong to the weights
        eng.sample(torch.randn(8, 100, generator=gen))
    gs, ds = eng.state_dicts()
    ckpt = str(d / "plain.pt")
    torch.save({"model_g": gs, "model_d": ds}, ckpt)
    s = Sampler.from_checkpoint(ckpt, "DCGAN", batch=8, with_d=True)
    own = s.from_latents(latents(48, 77)).cpu().numpy()
    rnd = np.random.default_rng(91).integers(0, 256, size=(48, 64, 64, 3), dtype=np.uint8)
    order = np.random.default_rng(92).permutation(96)
    train = np.concatenate([own, rnd])[order]
    np.savez(str(d / "train.npz"), images=train)
    return {"dir": d, "ckpt": ckpt, "sampler": s, "train": train, "is_own": order < 48}


def test_sampler_modes_end_to_end(trained):
    from hipgan._lib import JckError
    from hipgan.cluster import coverage
    from hipgan.probe import feature_layout
    from hipgan.sampler import Sampler
    s, train, is_own = trained["sampler"], trained["train"], trained["is_own"]
    r = s.modes(train, n=64, k=8, seed=0, space="pixel")
    assert r["k"] == 8 and r["hist_fake"].sum() == 64 and r["hist_real"].sum() == 96
    assert r["sample_cluster"].shape == (64,) and r["sample_cluster"].dtype == np.int64 and r["sample_d2"].shape == (64,)
    assert r["train_labels"].shape == (96,) and r["train_labels"].dtype == np.int64 and r["centres"].shape == (8, 12288)
    own_clusters = set(r["train_labels"][is_own].tolist())                    # every sample lands beside the generator's own pictures
    assert set(r["sample_cluster"].tolist()) <= own_clusters
    assert np.array_equal(np.bincount(r["train_labels"], minlength=8), r["hist_real"])
    c = coverage(r["hist_real"], r["sample_cluster"])
    assert (r["covered"], r["kl"]) == (c["covered"], c["kl"]) and r["missing"].tolist() == c["missing"].tolist()
    assert r["expected_covered"] == c["expected_covered"] and 1 <= r["covered"] <= r["k_real"] <= 8
    cl = s.cluster(train, 8, space="pixel")                                   # the same clustering handed in; deterministic for a seed
    assert np.array_equal(cl["labels"].cpu().numpy(), r["train_labels"])
    again = s.modes(train, n=64, seed=0, space="pixel", clusters=cl)
    assert np.array_equal(again["sample_cluster"], r["sample_cluster"]) and again["kl"] == r["kl"]
    d = s.modes(train, n=64, k=8, space="d", grid=2)
    assert d["centres"].shape == (8, feature_layout(64, 2)[1]) and d["hist_fake"].sum() == 64 - (d["hist_real"][d["sample_cluster"]] == 0).sum()
    plain = Sampler.from_checkpoint(trained["ckpt"], "DCGAN", batch=8)
    with pytest.raises(JckError):
        plain.cluster(train, 8, space="d")
    with pytest.raises(JckError):
        plain.modes(train, n=8, k=4, space="d")
    with pytest.raises(JckError):
        s.cluster(train, 8, space="z")


def run_cli(trained, out, labels_out):
    return subprocess.run([sys.executable, "modes.py", "-m", "DCGAN", "--checkpoint", trained["ckpt"], "--train", str(trained["dir"] / "train.npz"),
                           "--num", "64", "--k", "8", "-b", "8", "--out", str(out), "--labels_out", str(labels_out)], cwd=PKG, capture_output=True,
                          text=True, timeout=240)


def test_modes_cli(trained):
    from hipgan.probe import feature_layout
    out, pseudo = trained["dir"] / "out", trained["dir"] / "pseudo.npz"
    r = run_cli(trained, out, pseudo)
    assert r.returncode == 0, r.stdout + r.stderr
    rec = json.load(open(str(out / "modes.json")))
    assert set(rec) == {"k", "k_real", "covered", "expected_covered", "kl", "inertia", "iters", "n", "space", "missing"}
    assert rec["k"] == 8 and rec["n"] == 64 and rec["space"] == "d" and rec["covered"] <= rec["k_real"] <= 8 and len(rec["missing"]) <= 32
    f = np.load(str(out / "modes.npz"))
    assert sorted(f.files) == ["centres", "hist_fake", "hist_real", "sample_cluster", "sample_d2", "train_labels"]
    assert f["centres"].shape == (8, feature_layout(64, 4)[1]) and f["centres"].dtype == np.float32
    assert f["train_labels"].shape == (96,) and f["train_labels"].dtype == np.int64
    assert f["hist_real"].shape == (8,) and f["hist_fake"].shape == (8,) and f["hist_real"].dtype == np.int64 and f["hist_fake"].dtype == np.int64
    assert f["sample_cluster"].shape == (64,) and f["sample_cluster"].dtype == np.int64 and f["sample_d2"].shape == (64,) and f["sample_d2"].dtype == np.float32
    assert f["hist_real"].sum() == 96 and rec["covered"] == int((f["hist_fake"][f["hist_real"] > 0] >= 1).sum())
    png = open(str(out / "modes.png"), "rb").read()
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    w, h = int.from_bytes(png[16:20], "big"), int.from_bytes(png[20:24], "big")
    assert (w, h) == (16 * 66 + 2, min(16, rec["k_real"]) * 66 + 2)             # 8 training pictures and 8 samples a row, padding 2
    line = [l for l in r.stdout.splitlines() if l.startswith("modes: ")]
    assert len(line) == 1
    m = re.match(r"modes: (\d+) of (\d+) clusters covered \(expected ([0-9.]+) at n = (\d+)\), KL\(samples \|\| train\) ([0-9.]+|nan)", line[0])
    assert m and (int(m.group(1)), int(m.group(2)), int(m.group(4))) == (rec["covered"], rec["k_real"], 64)
    assert abs(float(m.group(3)) - rec["expected_covered"]) <= 0.05 and abs(float(m.group(5)) - rec["kl"]) <= 5e-5
    p = np.load(str(pseudo))
    assert np.array_equal(p["images"], trained["train"]) and np.array_equal(p["labels"], f["train_labels"])
    assert p["labels"].min() >= 0 and p["labels"].max() <= 7
    from preprocess.dcgan_data_preprocessor import load_npz_dataset
    assert load_npz_dataset(str(pseudo), need_labels=True)[1] == f["train_labels"].tolist()
    out2 = trained["dir"] / "out2"
    r2 = run_cli(trained, out2, trained["dir"] / "pseudo2.npz")                  # the same seed: the same bytes
    assert r2.returncode == 0, r2.stdout + r2.stderr
    f2 = np.load(str(out2 / "modes.npz"))
    assert all(f[key].tobytes() == f2[key].tobytes() for key in f.files)
    assert np.array_equal(np.load(str(trained["dir"] / "pseudo2.npz"))["labels"], p["labels"])
