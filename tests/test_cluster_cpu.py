"""The clustering layer without a GPU: the numpy twin of metrics.segment_mean, the host side of the jck_segment_* entry points,
hipgan.cluster.kmeans and coverage on host arrays, and the modes.py command line.  The reference arithmetic is tests/cluster_ref.py."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from cluster_ref import blobs, coverage_ref, kmeans_ref, seed_ref, segment_ref
from pairstats_ref import int_features

JCK_E_ARG = -1


def test_numpy_segment_mean_equals_the_reference_on_integer_features():
    import metrics
    x = int_features(300, 20, seed=1)
    g = np.random.default_rng(2)
    for k in (1, 7, 40):
        labels = g.integers(0, k, size=300)
        labels[g.integers(0, 300, size=20)] = -1                  # skipped rows: below the range ...
        labels[g.integers(0, 300, size=20)] = k                   # ... and above it
        if k == 40:
            labels[labels == 5] = 6                               # an empty cluster
        sent = np.full((k, 20), 7.5, np.float32)
        total, count, centre = metrics.segment_mean(x, labels, k, centre=sent)
        rt, rc, rcen = segment_ref(x, labels, k, sent)
        assert total.dtype == np.float32 and count.dtype == np.int32 and centre.dtype == np.float32
        assert np.array_equal(total.astype(np.float64), rt) and np.array_equal(count, rc) and np.array_equal(centre, rcen)
        assert count.sum() == ((labels >= 0) & (labels < k)).sum()
        assert (sent == 7.5).all()                                # the argument is not written to
        if k == 40:
            assert count[5] == 0 and (total[5] == 0).all() and (centre[5] == 7.5).all()
        none = metrics.segment_mean(x, labels.reshape(-1, 1), k)  # nearest's idx[:, 0:1] as it is; no centre: zeros at an empty cluster
        assert np.array_equal(none[0], total) and np.array_equal(none[2][count > 0], centre[count > 0]) and (none[2][count == 0] == 0).all()
    for bad in (dict(k=0), dict(k=1025)):
        with pytest.raises(ValueError):
            metrics.segment_mean(x, np.zeros(300, np.int64), **bad)
    with pytest.raises(ValueError):
        metrics.segment_mean(x, np.zeros(299, np.int64), 3)
    with pytest.raises(ValueError):
        metrics.segment_mean(x, np.zeros(300, np.int64), 3, centre=np.zeros((3, 19), np.float32))


def test_segment_entry_points_check_their_arguments_on_the_host():
    from hipgan import _lib
    dll = _lib.load_library()
    ws_bytes = dll.jck_segment_ws_bytes
    for bad in ((0, 8, 4), (-1, 8, 4), (100, 0, 4), (100, 8, 0), (100, 8, 1025), ((1 << 30) + 1, 8, 4)):
        assert ws_bytes(*bad) == 0, bad
    sizes = [ws_bytes(n, 64, 100) for n in (1, 2, 63, 64, 65, 255, 256, 257, 1000, 50000, 262144, 262145, 300000, 1 << 20)]
    assert all(s > 0 for s in sizes) and all(b >= a for a, b in zip(sizes, sizes[1:]))
    assert ws_bytes(1000, 64, 1) > 0 and ws_bytes(1000, 64, 1024) > ws_bytes(1000, 64, 1) and ws_bytes(1, 1, 1) > 0
    assert ws_bytes(50000, 15360, 1000) < 1 << 28                  # the partial sums of the probe's case stay a small share of its 3 GB
    R = dll.jck_segment_chunk_rows()
    assert R >= 1
    # null pointers and a bad K come back as JCK_E_ARG before any HIP call (no GPU here)
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    good = [p, 4, 4, p, 2, p, p, p, p, None]                      # (never passed whole: every call below has one bad argument)
    for hole in (0, 3, 5, 6, 8):
        args = list(good)
        args[hole] = None
        assert dll.jck_segment_mean_f32(*args) == JCK_E_ARG, hole
        assert b"segment_mean" in dll.jck_last_error()
    for k in (0, -3, 1025):
        args = list(good)
        args[4] = k
        assert dll.jck_segment_mean_f32(*args) == JCK_E_ARG, k
    for n, d in ((0, 4), (4, 0), ((1 << 30) + 1, 4)):
        args = list(good)
        args[1], args[2] = n, d
        assert dll.jck_segment_mean_f32(*args) == JCK_E_ARG, (n, d)


def test_kmeans_on_host_arrays_finds_the_blobs():
    from hipgan.cluster import kmeans
    x, blob = blobs(seed=3)
    r = kmeans(x, 6, iters=50, seed=0)
    assert set(r) >= {"centres", "labels", "count", "inertia", "iters", "history"}
    assert r["centres"].dtype == np.float32 and r["centres"].shape == (6, 8) and r["labels"].dtype == np.int64 and r["count"].dtype == np.int64
    assert (r["count"] == 40).all()
    for b in range(6):                                            # every blob is one cluster
        assert len(set(r["labels"][blob == b].tolist())) == 1
    assert len(set(r["labels"].tolist())) == 6
    assert all(b <= a for a, b in zip(r["history"], r["history"][1:])) and r["inertia"] == r["history"][-1]
    assert 1 <= r["iters"] < 50 and len(r["history"]) == r["iters"] + 1
    again = kmeans(x, 6, iters=50, seed=0)
    assert all(np.array_equal(r[key], again[key]) for key in ("centres", "labels", "count")) and again["history"] == r["history"]
    ref = kmeans_ref(x, 6, 50, 0)                                 # the fp64 restatement: on these integers nothing rounds before the division
    assert np.array_equal(r["labels"], ref["labels"]) and np.array_equal(r["centres"], ref["centres"]) and np.array_equal(r["count"], ref["count"])
    assert r["iters"] == ref["iters"] and r["history"] == ref["history"]
    for key in ("labels", "count"):                               # a host tensor takes the same path
        assert np.array_equal(kmeans(torch.as_tensor(x), 6, seed=0)[key], r[key])
    # labels, count and inertia belong to the centres returned, also where the updates ran out
    cut = kmeans(x, 6, iters=1, seed=0)
    assert cut["iters"] == 1 and len(cut["history"]) == 2
    d2 = ((x[:, None, :].astype(np.float64) - cut["centres"][None].astype(np.float64)) ** 2).sum(2)
    assert np.array_equal(cut["labels"], d2.argmin(1)) and cut["inertia"] == float(d2.min(1).sum())
    zero = kmeans(x, 6, iters=0, seed=0)
    assert zero["iters"] == 0 and np.array_equal(zero["centres"], x[seed_ref(x, 6, 0)])


def test_kmeans_edges_on_host_arrays():
    from hipgan._lib import JckError
    from hipgan.cluster import kmeans
    x, _ = blobs(seed=4)
    one = kmeans(x, 1)
    assert one["count"].tolist() == [240] and (one["labels"] == 0).all() and one["iters"] == 1
    assert np.array_equal(one["centres"][0], x.astype(np.float64).sum(0).astype(np.float32) / np.float32(240))
    small = x[:9]
    every = kmeans(small, 9, seed=5)                              # k = N: every row its own centre
    assert sorted(every["labels"].tolist()) == list(range(9)) and (every["count"] == 1).all() and every["inertia"] == 0.0
    assert np.array_equal(every["centres"][every["labels"]], small)
    dup = np.repeat(x[:2], 4, axis=0)                             # 8 rows, 2 distinct: after two centres every distance is 0
    r = kmeans(dup, 4, seed=6)
    assert np.array_equal(r["labels"], kmeans_ref(dup, 4, 50, 6)["labels"]) and r["inertia"] == 0.0 and r["count"].sum() == 8
    assert sorted(seed_ref(dup, 4, 6)) == sorted(set(seed_ref(dup, 4, 6)))          # the total-0 branch picks rows not picked before
    assert np.array_equal(r["centres"][r["labels"]], dup) and (r["count"] == 0).sum() == 2     # ties go to the lower centre: two stay empty
    for bad in (np.nan, np.inf):
        y = x.copy()
        y[17, 3] = bad
        for k in (1, 3):
            with pytest.raises(JckError):
                kmeans(y, k)
    for k in (0, 241, 1025):
        with pytest.raises(JckError):
            kmeans(x, k)


def test_coverage_against_values_worked_out_by_hand():
    from hipgan.cluster import coverage
    # five clusters of 40, 30, 20, 10 and 0 training pictures; 8 samples: 4 in cluster 0, 3 in 1, 1 in 3, none in 2
    real = [40, 30, 20, 10, 0]
    fake = [0, 0, 0, 0, 1, 1, 1, 3]
    c = coverage(real, fake)
    assert (c["k"], c["k_real"], c["covered"]) == (5, 4, 3)
    assert c["hist_real"].tolist() == real and c["hist_fake"].tolist() == [4, 3, 0, 1, 0] and c["hist_fake"].dtype == np.int64
    assert c["missing"].tolist() == [2]
    kl = 0.5 * math.log(0.5 / 0.4) + 0.375 * math.log(0.375 / 0.3) + 0.125 * math.log(0.125 / 0.1)
    assert abs(c["kl"] - kl) <= 1e-15
    expected = 4 - (0.6 ** 8 + 0.7 ** 8 + 0.8 ** 8 + 0.9 ** 8)
    assert abs(c["expected_covered"] - expected) <= 1e-14
    two = coverage(real, fake, min_count=2)                       # cluster 3 holds one sample only
    assert two["covered"] == 2 and two["missing"].tolist() == [2, 3] and two["kl"] == c["kl"] and two["expected_covered"] == c["expected_covered"]
    # a sample in the cluster without training pictures is dropped with it: n is 8 again; so are labels outside the range
    more = coverage(np.asarray(real), torch.as_tensor(fake + [4, 4, -1, 5]))
    assert more["hist_fake"].tolist() == [4, 3, 0, 1, 0] and more["kl"] == c["kl"] and more["k_real"] == 4 and more["covered"] == 3
    # missing: the largest real share first, the lower id among equals
    m = coverage([5, 9, 9, 2, 30], [4, 4, 4])
    assert m["missing"].tolist() == [1, 2, 0, 3] and m["covered"] == 1 and abs(m["kl"] - math.log(55 / 30)) <= 1e-15
    same = coverage(real, [0] * 4 + [1] * 3 + [2] * 2 + [3])      # the real proportions exactly: no divergence, all covered
    assert same["kl"] == 0.0 and same["covered"] == 4 and same["missing"].size == 0
    g = np.random.default_rng(7)
    rr, ff = g.integers(0, 50, size=30), g.integers(-1, 31, size=500)
    got, want = coverage(rr, ff, 3), coverage_ref(rr, ff, 3)
    assert all(got[key] == want[key] for key in ("k", "k_real", "covered")) and got["missing"].tolist() == want["missing"]
    assert got["hist_fake"].tolist() == want["hist_fake"] and abs(got["kl"] - want["kl"]) <= 1e-13
    assert abs(got["expected_covered"] - want["expected_covered"]) <= 1e-12


def test_modes_parser_defaults_refusals_and_help(capsys, tmp_path, monkeypatch):
    import evalcli
    import modes
    from hipgan._lib import JckError
    base = ["--checkpoint", "c.pt", "--train", "t.npz", "--out", "o"]
    a = modes.get_arg_parse(base)
    assert (a.model, a.k, a.num, a.space, a.grid, a.pool, a.seed, a.iters, a.which, a.batch_size) == ("DCGAN", 100, 10000, "d", 4, "max", 0, 50, "auto", 64)
    assert a.truncation is None and a.min_count == 1 and a.labels_out is None and a.prec == "bf16"
    a = modes.get_arg_parse(base + ["-m", "CGAN", "--k", "100", "--num", "0", "--labels_out", "p.npz", "--space", "pixel", "-b", "8"])
    assert (a.model, a.num, a.labels_out, a.space, a.batch_size) == ("CGAN", 0, "p.npz", "pixel", 8)
    for bad in (["--k", "101", "--labels_out", "p.npz"], ["--k", "0"], ["--k", "1025"], ["--num", "0"], ["--num", "-1"], ["--grid", "3"], ["--space", "x"],
                ["--truncation", "0"], ["--min_count", "0"], ["--iters", "-1"]):
        with pytest.raises(SystemExit):
            modes.get_arg_parse(base + bad)
    capsys.readouterr()
    for argv in (["--out", "o", "--train", "t.npz"], ["--checkpoint", "c.pt", "--out", "o"]):
        with pytest.raises(SystemExit):
            modes.get_arg_parse(argv)
    with pytest.raises(SystemExit) as e:
        modes.get_arg_parse(["--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    assert "--labels_out" in text and "modes.json" in text and "KL(samples || train)" in text
    # the discriminator's feature space needs the checkpoint's discriminator; pixel space does not: the run opener refuses the checkpoint
    # before any engine exists (Sampler.from_checkpoint is stood in for: it needs a GPU)
    from hipgan.sampler import Sampler
    monkeypatch.setattr(Sampler, "from_checkpoint", classmethod(lambda cls, ckpt, model, with_d=False, **kw: ("sampler", with_d)))
    np.savez(str(tmp_path / "t.npz"), images=np.zeros((4, 32, 32, 3), np.uint8))
    g_only = {"model_g": {"conv1.weight": torch.zeros(1)}}

    def open_with(ckpt, extra=()):
        torch.save(ckpt, str(tmp_path / "c.pt"))
        a = modes.get_arg_parse(["--checkpoint", str(tmp_path / "c.pt"), "--train", str(tmp_path / "t.npz"), "--out", "o", "--k", "2"] + list(extra))
        return evalcli.open_run(a, a.space == "d")[0]
    with pytest.raises(JckError):
        open_with(g_only)
    with pytest.raises(JckError):
        open_with({**g_only, "model_d": {}})
    assert open_with(g_only, ["--space", "pixel"]) == ("sampler", False)
    assert open_with({**g_only, "model_d": {"conv1.weight": torch.zeros(1)}}) == ("sampler", True)


def test_labels_file_loads_as_a_conditional_training_set(tmp_path):
    import modes
    from preprocess.dcgan_data_preprocessor import load_npz_dataset
    g = np.random.default_rng(8)
    images = g.integers(0, 256, size=(12, 32, 32, 3), dtype=np.uint8)
    labels = g.integers(0, 100, size=12)
    path = modes.write_labels(str(tmp_path / "sub" / "pseudo"), images, torch.as_tensor(labels))
    assert path.endswith("pseudo.npz") and os.path.exists(path)
    img, lab = load_npz_dataset(path, need_labels=True)
    assert lab == labels.tolist() and img.dtype == torch.uint8 and np.array_equal(img.permute(0, 2, 3, 1).numpy(), images)
    from hipgan.probe import load_images
    u8, l2 = load_images(path, need_labels=True)
    assert np.array_equal(u8.numpy(), images) and l2.dtype == np.int64 and l2.tolist() == labels.tolist()


def test_least_covered_rows_of_the_sheet():
    import modes
    r = {"hist_real": np.array([10, 0, 30, 20, 40]), "hist_fake": np.array([5, 0, 0, 10, 5])}
    # hist_fake / (n p_c): 2.5, -, 0, 2.5, 0.625 -> cluster 2, then 4, then the tie 0 before 3; the empty cluster 1 is left out
    assert modes.least_covered(r).tolist() == [2, 4, 0, 3] and modes.least_covered(r, 2).tolist() == [2, 4]
    of, d2 = np.array([1, 0, 1, 1, 2, 1]), np.array([0.5, 0.1, 0.2, 0.2, 0.0, 0.9], np.float32)
    assert modes.nearest_members(of, d2, 1).tolist() == [2, 3, 0, 5] and modes.nearest_members(of, d2, 1, 2).tolist() == [2, 3]
    assert modes.nearest_members(of, d2, 7).size == 0
