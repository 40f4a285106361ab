"""The pairwise-statistics kernels (csrc/pairstat.hip) and what metrics.py / the trainers build on them, on the GPU: bit-exact
on integer-valued data (every dot product, polynomial and partial sum is then exactly representable, so the result must EQUAL
the fp64 / integer reference whatever the summation order), within derived bounds on real-valued data.  The fp64 reference
arithmetic is tests/pairstats_ref.py.  The tile is 64 x 64: sizes 63 / 64 / 65 / 129 straddle it."""
import argparse
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from pairstats_ref import (MARGIN, d2_ref, hits_ref, int_features, kid_ref, kid_tol, margins, poly3_ref, pr_ref, radii_bound, radii_ref,
                           recipe)

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def dev_offset(a):
    """the same rows, starting one float past a 16-byte boundary"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    out = buf[1:].view(a.shape)
    out.copy_(torch.as_tensor(a))
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


def poly3(x, y, gamma, coef0, skip_diag):
    from hipgan._lib import cur_stream, lib, load_library
    out = torch.full((1,), -1.0, dtype=torch.float64, device="cuda")
    ws = torch.empty(load_library().jck_pairstat_ws_bytes(x.shape[0], y.shape[0]) // 8, dtype=torch.float64, device="cuda")
    lib.jck_poly3_sum_f64(x, x.shape[0], y, y.shape[0], x.shape[1], gamma, coef0, int(skip_diag), out, ws, cur_stream())
    return out


def knn(x, k):
    from hipgan._lib import cur_stream, lib
    r2 = torch.full((x.shape[0],), -1.0, dtype=torch.float32, device="cuda")
    lib.jck_knn_radius2_f32(x, x.shape[0], x.shape[1], k, r2, cur_stream())
    return r2


def hits(q, ref, r2):
    from hipgan._lib import cur_stream, lib
    hit = torch.full((q.shape[0],), 7, dtype=torch.uint8, device="cuda")
    lib.jck_manifold_hit_u8(q, q.shape[0], ref, r2, ref.shape[0], q.shape[1], hit, cur_stream())
    return hit


def int_sets():
    real, fake = int_features(333, seed=1), int_features(131, seed=2)
    real[17] = real[5]                   # two identical rows: the pair (5, 17) counts, the pairs (5, 5) and (17, 17) do not
    fake[3] = real[3]                    # ... and a row shared by both sets at the same index
    return real, fake


def d2_int(a, b):
    a, b = a.astype(np.int64), b.astype(np.int64)
    return ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :]) - 2 * (a @ b.T)


def radii_int(x, k):
    d2 = d2_int(x, x).astype(np.float64)
    d2[np.arange(len(x)), np.arange(len(x))] = np.inf
    return np.sort(d2, axis=1)[:, k - 1].astype(np.float32)


def test_poly3_sum_is_bit_exact_on_integer_features():
    real, fake = int_sets()
    r, f = dev(real), dev(fake)
    for x, y, hx, hy in ((f, r, fake, real), (r, r, real, real), (r, f, real, fake)):
        for skip in (0, 1):
            got = poly3(x, y, 1.0 / 64, 1.0, skip).item()
            assert got == poly3_ref(hx, hy, bool(skip), 1.0 / 64, 1.0), (x.shape, y.shape, skip)
    assert poly3(r, r, 1.0 / 64, 1.0, 0).item() - poly3(r, r, 1.0 / 64, 1.0, 1).item() == \
        float(sum(Fraction(int((row.astype(np.int64) ** 2).sum()) + 64, 64) ** 3 for row in real))


def test_poly3_sum_counts_more_than_2_to_31_pairs():
    """M = N = 50 000 (the workload's own real x real term; 2.5e9 pairs), D = 64, rows drawn from 4 patterns with entries in
    {-1, 0, 1}: |gamma G + 1| <= 2, every value a multiple of 2^-18, every partial sum below 2^53 of them - the closed form
    sum_{a,b} n_a n_b k(a,b) - [skip_diag] sum_a n_a k(a,a) in exact rationals must come back bit for bit."""
    g = np.random.default_rng(3)
    pats = g.integers(-1, 2, size=(4, 64))
    which = g.integers(0, 4, size=50000)
    x = dev(pats[which])
    cnt = np.bincount(which, minlength=4)
    k = [[(Fraction(int(pats[a] @ pats[b]), 64) + 1) ** 3 for b in range(4)] for a in range(4)]
    full = sum(int(cnt[a]) * int(cnt[b]) * k[a][b] for a in range(4) for b in range(4))
    diag = sum(int(cnt[a]) * k[a][a] for a in range(4))
    assert float(full) == full and float(full - diag) == full - diag          # representable: the comparison below is exact
    assert poly3(x, x, 1.0 / 64, 1.0, 0).item() == float(full)
    assert poly3(x, x, 1.0 / 64, 1.0, 1).item() == float(full - diag)


@pytest.mark.parametrize("D,offset", [(100, False), (37, True), (100, True)])
def test_kid_on_real_valued_features_within_the_fp32_dot_product_bound(D, offset):
    """the dot product is a D-term fp32 fmaf chain, the polynomial fp64: tolerance derived in pairstats_ref.kid_tol"""
    import metrics
    real, fake = recipe(D)
    want, tol = kid_ref(real, fake), kid_tol(real, fake)
    got = metrics.kid_from_features(dev(real), dev_offset(fake) if offset else dev(fake))
    print(f"D={D} offset={offset} kid={got!r} ref={want!r} diff={abs(got - want):.3e} tol={tol:.3e}")
    assert abs(got - want) <= tol
    if D == 100:
        assert 0.2 < got < 0.4               # 0.30 on these inputs


def test_knn_radii_are_bit_exact_on_integer_features():
    base = int_features(333, seed=4)
    base[1] = base[0]
    for n in (9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 333):
        x = base[:n]
        for k in (1, 3, 8):
            got = knn(dev(x), k).cpu().numpy()
            assert np.array_equal(got, radii_int(x, k)), (n, k)
            if k == 1:
                assert got[0] == 0.0 and got[1] == 0.0            # duplicate rows: excluded by index, not by value
    assert np.array_equal(knn(dev(base[:9]), 8).cpu().numpy(), radii_int(base[:9], 8))      # k = N - 1


def test_manifold_hits_are_bit_exact_on_integer_features_with_ties():
    ref = int_features(333, seed=5)
    r2 = radii_int(ref, 3)
    g = np.random.default_rng(6)
    q_all = ref[g.integers(0, 333, size=131)].copy()
    q_all[np.arange(131), g.integers(0, 64, size=131)] += 2          # near a reference row
    q_all[::3] = int_features(131, seed=7)[::3]                       # ... or nowhere near one
    for m in (1, 17, 131):
        q = q_all[:m]
        d2 = d2_int(q, ref)
        got = hits(dev(q), dev(ref), dev(r2)).cpu().numpy()
        assert np.array_equal(got, (d2 <= r2[None, :].astype(np.int64)).any(1).astype(np.uint8)), m
        # radii at which EVERY hit is a tie: r2[j] = the smallest distance any query has to ref_j
        tie = d2.min(axis=0).astype(np.float32)
        got = hits(dev(q), dev(ref), dev(tie)).cpu().numpy()
        assert np.array_equal(got, (d2 == d2.min(axis=0)[None, :]).any(1).astype(np.uint8)) and got.any(), m
        assert not hits(dev(q), dev(ref), dev(tie - 1)).cpu().numpy().any()
    d2 = d2_int(q_all, ref)
    assert 0 < (d2 <= r2[None, :].astype(np.int64)).any(1).sum() < 131 and (d2 == r2[None, :].astype(np.int64)).any()


@pytest.mark.parametrize("D,offset", [(5, False), (20, False), (64, True)])
def test_all_three_are_bit_exact_at_ragged_depth_and_off_alignment(D, offset):
    """the exact tests above stage with 16-byte loads only (D = 64, aligned).  D = 5 is scalar staging inside one 16-column step,
    D = 20 is 16-byte staging with a partly filled second step, D = 64 one float off the boundary is scalar staging over whole steps.
    Entries in -3..3 at D <= 64 keep every product, norm and partial sum exact."""
    put = dev_offset if offset else dev
    base, other = int_features(129, D, seed=11), int_features(65, D, seed=12)
    base[1] = base[0]
    g = np.random.default_rng(13)
    q = base[g.integers(0, 63, size=65)].copy()
    q[np.arange(65), g.integers(0, D, size=65)] += 2                 # near a reference row
    q[::3] = int_features(65, D, seed=14)[::3]                        # ... or nowhere near one
    for n in (63, 64, 65, 129):
        x = base[:n]
        xd, od, qd = put(x), put(other), put(q)
        for skip in (0, 1):
            assert poly3(xd, xd, 1.0 / 64, 1.0, skip).item() == poly3_ref(x, x, bool(skip), 1.0 / 64, 1.0), (n, skip)
            assert poly3(xd, od, 1.0 / 64, 1.0, skip).item() == poly3_ref(x, other, bool(skip), 1.0 / 64, 1.0), (n, skip)
            assert poly3(od, xd, 1.0 / 64, 1.0, skip).item() == poly3_ref(other, x, bool(skip), 1.0 / 64, 1.0), (n, skip)
        d2 = d2_int(q, x)
        for k in (1, 3, 8):
            r2 = radii_int(x, k)
            got = knn(xd, k)
            assert np.array_equal(got.cpu().numpy(), r2), (n, k)
            want = (d2 <= r2[None, :].astype(np.int64)).any(1).astype(np.uint8)
            assert np.array_equal(hits(qd, xd, got).cpu().numpy(), want), (n, k)
            assert np.array_equal(hits(xd, xd, got).cpu().numpy(), np.ones(n, np.uint8)), (n, k)      # d2 = 0 to itself


def _check_side(q, ref, k, name):
    """one side of precision / recall by the margin rule: queries whose fp64 decision margin is below MARGIN are set aside (at
    most 2 %), the others' hits must be identical, the device radii within the same bound"""
    r2_ref = radii_ref(ref, k)
    r2_dev = knn(dev(ref), k)
    err = np.abs(r2_dev.cpu().numpy().astype(np.float64) - r2_ref)
    assert (err <= radii_bound(ref)).all(), (name, float((err / radii_bound(ref)).max()))
    got = hits(dev(q), dev(ref), r2_dev).cpu().numpy()
    sure = margins(q, ref, r2_ref) >= MARGIN
    share = 1.0 - sure.mean()
    print(f"{name}: D={q.shape[1]} set aside {share:.4f}, hit rate {got.mean():.4f}, worst radius error / bound {float((err / radii_bound(ref)).max()):.3e}")
    assert share <= 0.02
    assert np.array_equal(got[sure], hits_ref(q, ref, r2_ref)[sure].astype(np.uint8))
    return got


@pytest.mark.parametrize("D", [20, 100])
def test_precision_recall_on_real_valued_features(D):
    import metrics
    real, fake = recipe(D)
    hp = _check_side(fake, real, 3, "precision")
    hr = _check_side(real, fake, 3, "recall")
    p, r = metrics.precision_recall_from_features(dev(real), dev(fake), k=3)
    assert (p, r) == (float(hp.mean()), float(hr.mean()))
    if D == 20:
        assert (p, r) == pr_ref(real, fake, 3) and abs(p - 0.931) < 1e-3 and abs(r - 0.279) < 1e-3      # no query inside the margin


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_features(bad):
    import metrics
    real, fake = recipe(20)
    f = fake.copy()
    f[5, 3] = bad
    r, fd, fc = dev(real), dev(f), dev(fake)
    assert np.isnan(metrics.kid_from_features(r, fd)) and np.isnan(metrics.kid_from_features(fd, r))
    rad = knn(fd, 3).cpu().numpy()
    assert np.isnan(rad[5]) and np.isfinite(np.delete(rad, 5)).all()
    want = metrics.knn_radius2(f, 3)                                   # host path: the bad row is nobody's neighbour
    assert (np.abs(np.delete(rad, 5) - np.delete(want, 5)) <= np.delete(radii_bound(fake), 5)).all()
    r2 = knn(r, 3)
    h_bad, h_clean = hits(fd, r, r2).cpu().numpy(), hits(fc, r, r2).cpu().numpy()
    assert h_bad[5] == 255 and np.array_equal(np.delete(h_bad, 5), np.delete(h_clean, 5))     # the other queries are untouched
    assert torch.equal(knn(r, 3), r2)
    h_ref_bad = hits(r, fd, knn(fd, 3)).cpu().numpy()                  # a reference row with a NaN radius never hits
    assert set(np.unique(h_ref_bad)) <= {0, 1}
    for a, b in ((r, fd), (fd, r)):
        assert all(np.isnan(v) for v in metrics.precision_recall_from_features(a, b))


def test_two_runs_give_identical_bytes():
    real, fake = recipe(100)
    r, f = dev(real), dev(fake)
    for fn in (lambda: poly3(f, r, 0.01, 1.0, 0), lambda: poly3(r, r, 0.01, 1.0, 1), lambda: knn(r, 3), lambda: hits(f, r, knn(r, 3)),
               lambda: hits(r, f, knn(f, 3))):
        a, b = fn(), fn()
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_metrics_object_agrees_with_the_host_path_and_caches_the_real_side(monkeypatch):
    import metrics
    g = np.random.default_rng(8)
    w = g.standard_normal((8, 100)) / np.sqrt(8)           # features near an 8-d subspace: isotropic noise in 100-d has no near neighbours
    real = (g.standard_normal((600, 8)) @ w + 0.05 * g.standard_normal((600, 100))).astype(np.float32)
    fake = ((0.8 * g.standard_normal((1000, 8)) + 0.3) @ w + 0.05 * g.standard_normal((1000, 100))).astype(np.float32)
    targets = [i % 100 for i in range(600)]
    m = metrics.Metrics(argparse.Namespace(targets=targets), real_features=real)
    logits = dev(fake)
    calls = []
    orig = metrics.knn_radius2
    # counts the device calls only: the numpy reference path below goes through the same function
    monkeypatch.setattr(metrics, "knn_radius2",
                        lambda x, k: (calls.append(int(x.shape[0])) if torch.is_tensor(x) and x.is_cuda else None, orig(x, k))[1])
    kid = m.kid([logits])
    assert abs(kid - metrics.kid_from_features(real, fake)) <= kid_tol(real, fake)
    rr = m._real_pair_stats(None, True)["rr"]
    assert m.kid([logits]) == kid and m._real_pair_stats(None, True)["rr"] is rr and rr.is_cuda
    want, tol = [], []
    for s in range(20):
        rs, fs = real[m.real_superclass_idx[s]], fake[m.fake_superclass_idx[s]]
        want.append(metrics.kid_from_features(rs, fs))
        tol.append(kid_tol(rs, fs))
    assert abs(m.intra_kid(logits) - float(np.mean(want))) <= float(np.mean(tol))
    # precision / recall by the margin rule: the two paths may differ only on queries inside the margin, at most 2 % of them
    p_ref, r_ref = metrics.precision_recall_from_features(real, fake, k=3)
    p, r = m.precision_recall([logits], k=3)
    assert (p, r) == m.precision_recall([logits], k=3)
    assert calls.count(600) == 1 and calls.count(1000) == 2            # real's radii once, fake's every time
    for got, ref_v, q, rf in ((p, p_ref, fake, real), (r, r_ref, real, fake)):
        aside = int((margins(q, rf, radii_ref(rf, 3)) < MARGIN).sum())
        assert aside <= 0.02 * len(q) and abs(got - ref_v) * len(q) <= aside + 1e-6
    # the split the trainers use gives the same numbers
    stats = {k_: v.cpu() for k_, v in m.fake_pair_stats_device(logits, intra=True).items()}
    assert stats["kid_rr"].dtype == torch.float64 and stats["hit_fake"].dtype == torch.uint8 and len(stats["hit_real"]) == 600
    extra = m.extra_scores_from_stats(stats, intra=True)
    assert set(extra) == {"kid", "precision", "recall", "intra_kid"}
    assert extra["kid"] == kid and (extra["precision"], extra["recall"]) == (p, r)
    assert abs(extra["intra_kid"] - float(np.mean(want))) <= float(np.mean(tol))
    assert calls.count(600) == 1


class TinyExtractor:
    """a seeded random projection of a 10 x 10 sampling of the 299 x 299 input to 100 features: the evaluation branch needs a
    metric network, this test is about what happens to its features"""

    def __init__(self):
        self.w = (torch.randn(300, 100, generator=torch.Generator().manual_seed(0)) / 17).cuda()

    def __call__(self, x):
        return x[:, :, ::30, ::30].reshape(x.shape[0], -1).float() @ self.w


class SynthPre:
    idx_to_labels = [str(i) for i in range(100)]

    def __init__(self, batches):
        self.batches = batches

    def get_data_loader(self):
        return self.batches, None


def _fresh_logger():
    import logging
    from logger.main_logger import MainLogger
    logging.getLogger("main").handlers.clear()
    MainLogger._instance, MainLogger._initialized = None, False


@pytest.mark.parametrize("flag", [None, 1])
def test_dcgan_trainer_reports_the_extra_scores_only_when_asked(flag, tmp_path, monkeypatch, caplog):
    import logging
    from metrics import Metrics
    from model import DCGAN
    from train.dcgan_trainer import DCGANTrainer
    from util import synth_images
    monkeypatch.chdir(tmp_path)
    _fresh_logger()
    B, steps = 8, 2
    imgs = synth_images(B * steps)
    batches = [(imgs[i * B:(i + 1) * B],) for i in range(steps)]
    root = tmp_path / "save" / "dcgan" / "ev"
    args = argparse.Namespace(epoch=1, max_learning_rate=2e-4, model_path="ev", log_file=0, save_path=str(root), batch_size=B, num_worker=0)
    if flag is not None:
        args.extra_metrics = flag
    real = torch.randn(300, 100, generator=torch.Generator().manual_seed(1)).numpy()
    monkeypatch.setattr(DCGANTrainer, "_make_metrics", lambda self, loader: Metrics(None, extractor=TinyExtractor(), real_features=real))
    torch.manual_seed(12345)
    caplog.set_level(logging.DEBUG, logger="main")
    tr = DCGANTrainer(args, DCGAN.Generator(), DCGAN.Discriminator(), SynthPre(batches), prec="f32")
    tr.train()
    msgs = [r.getMessage() for r in caplog.records if r.name == "main"]
    scores = [m for m in msgs if m.startswith("inception score: ")]
    extra = [m for m in msgs if m.startswith("kid: ")]
    assert len(scores) == 2 and all(len(m.split("\t")) == 2 and m.split("\t")[1].startswith("fid: ") for m in scores)
    if flag is None:
        assert not extra and "kid" not in os.listdir(root)
        assert {m.split(" ", 1)[1] for m in msgs if " lowest " in m or " highest " in m} <= {"lowest fid", "highest is"}
    else:
        assert len(extra) == 2 and all(msgs[msgs.index(s) + 1].startswith("kid: ") for s in scores)      # right after the existing line
        for m in extra:
            parts = m.split("\t")
            assert [p.split(": ")[0] for p in parts] == ["kid", "precision", "recall"]
            vals = [float(p.split(": ")[1]) for p in parts]
            assert all(np.isfinite(vals)) and 0.0 <= vals[1] <= 1.0 and 0.0 <= vals[2] <= 1.0
        pts = [f for f in os.listdir(root / "kid") if f.endswith(".pt")]
        assert len(pts) == 1 and any(f.endswith("_fake_image.png") for f in os.listdir(root / "kid"))
        ck = torch.load(root / "kid" / pts[0], weights_only=False)
        assert sorted(ck) == ["model_d", "model_g", "optimizer_d", "optimizer_g"]
        best_kid = min(float(m.split("\t")[0].split(": ")[1]) for m in extra)
        assert pts[0].split("_")[1] == f"{best_kid:.04f}.pt"
    _fresh_logger()


def test_cgan_evaluation_reports_intra_kid(tmp_path, monkeypatch, caplog):
    import logging
    from metrics import Metrics
    from model import CGAN
    from train.async_eval import AsyncEval
    from train.cgan_trainer import CGANTrainer
    from util import synth_images, synth_onehot
    monkeypatch.chdir(tmp_path)
    _fresh_logger()
    B = 8
    imgs, (oh, _) = synth_images(B), synth_onehot(B)
    root = tmp_path / "save" / "cgan" / "ev"
    args = argparse.Namespace(epoch=1, max_learning_rate=2e-4, model_path="ev", log_file=0, save_path=str(root), batch_size=B, num_worker=0,
                              extra_metrics=1)
    real = torch.randn(400, 100, generator=torch.Generator().manual_seed(1)).numpy()
    real_set = argparse.Namespace(targets=[i % 100 for i in range(400)])
    monkeypatch.setattr(CGANTrainer, "_make_metrics", lambda self, loader: Metrics(real_set, extractor=TinyExtractor(), real_features=real))
    monkeypatch.setattr(CGANTrainer, "save_image", lambda self, path, iters, images: None)       # the class grid is not what is tested
    torch.manual_seed(12345)
    caplog.set_level(logging.DEBUG, logger="main")
    tr = CGANTrainer(args, CGAN.Generator(), CGAN.Discriminator(), SynthPre([(imgs, oh)]), prec="f32")
    tr._eval = AsyncEval(tr)
    noise = torch.randn(1000, 100, 1, 1, device=tr.device)
    labels = torch.nn.functional.one_hot(torch.arange(100).repeat_interleave(10), 100).to(torch.int64).to(tr.device)
    best = {"fid": 1e10, "intra": 1e10, "is": 0}
    tr._evaluate(noise, labels, 0, best, str(root / "img"))
    tr._finish_eval(best, wait=True)
    msgs = [r.getMessage() for r in caplog.records if r.name == "main"]
    i = next(n for n, m in enumerate(msgs) if m.startswith("inception score: "))
    parts = msgs[i + 1].split("\t")
    assert [p.split(": ")[0] for p in parts] == ["kid", "precision", "recall", "intra kid"]
    vals = [float(p.split(": ")[1]) for p in parts]
    assert all(np.isfinite(vals)) and best["kid"] == vals[0] and best["intra_kid"] == vals[3]
    for typ in ("kid", "intra_kid"):
        assert len([f for f in os.listdir(root / typ) if f.endswith(".pt")]) == 1
    _fresh_logger()
