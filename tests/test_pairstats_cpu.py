"""KID and improved precision / recall without a GPU: the numpy paths of metrics.py against the fp64 restatement of
tests/pairstats_ref.py, the host-only entry point, the argument checks of the new C ABI, and the trainers with the flag off."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from pairstats_ref import kid_ref, poly3_ref, pr_ref, radii_ref, hits_ref, recipe

E_ARG = -1


def test_host_paths_match_the_brute_force_formulas(monkeypatch):
    import metrics
    real, fake = recipe(20)
    want = kid_ref(real, fake)
    assert metrics.kid_from_features(real, fake) == pytest.approx(want, rel=1e-10, abs=1e-12)
    assert metrics.kid_from_features(torch.as_tensor(real), torch.as_tensor(fake)) == pytest.approx(want, rel=1e-10, abs=1e-12)
    np.testing.assert_allclose(metrics.knn_radius2(real, 3), radii_ref(real, 3), rtol=1e-10)
    np.testing.assert_allclose(metrics.knn_radius2(fake, 1), radii_ref(fake, 1), rtol=1e-10)
    r2 = radii_ref(real, 3)
    assert np.array_equal(metrics.manifold_hit(fake, real, r2), hits_ref(fake, real, r2).astype(np.uint8))
    p, r = metrics.precision_recall_from_features(real, fake, k=3)
    assert (p, r) == pr_ref(real, fake, 3)
    assert 0.9 < p < 0.96 and 0.25 < r < 0.31           # 0.931 / 0.279 on these inputs
    # the Gram products are blocked: the same numbers with blocks smaller than either set
    monkeypatch.setattr(metrics, "_HOST_BLOCK", 50)
    assert metrics.kid_from_features(real, fake) == pytest.approx(want, rel=1e-10, abs=1e-12)
    assert metrics.precision_recall_from_features(real, fake, k=3) == (p, r)


def test_host_paths_non_finite_and_duplicates():
    import metrics
    real, fake = recipe(20)
    for bad in (np.nan, np.inf):
        f = fake.copy()
        f[5, 3] = bad
        assert np.isnan(metrics.kid_from_features(real, f))
        assert all(np.isnan(v) for v in metrics.precision_recall_from_features(real, f))
        assert all(np.isnan(v) for v in metrics.precision_recall_from_features(f, real))
        assert np.isnan(metrics.knn_radius2(f, 3)[5]) and metrics.manifold_hit(f, real, radii_ref(real, 3))[5] == 255
    dup = real.copy()
    dup[17] = dup[5]                                    # excluded by index, not by value
    assert metrics.knn_radius2(dup, 1)[5] == 0.0 and metrics.knn_radius2(dup, 1)[17] == 0.0
    assert metrics.poly3_sum(dup, dup, True) == pytest.approx(poly3_ref(dup, dup, True), rel=1e-12)
    with pytest.raises(ValueError):
        metrics.knn_radius2(real[:3], 3)


def test_workspace_query_is_small_and_monotone():
    from hipgan import _lib
    dll = _lib.load_library()
    big = dll.jck_pairstat_ws_bytes(50000, 50000)
    assert 0 < big <= 16 * 2 ** 20
    sizes = [(1, 1), (64, 64), (65, 64), (131, 333), (1000, 1000), (1000, 50000), (50000, 1000), (50000, 50000)]
    got = {s: dll.jck_pairstat_ws_bytes(*s) for s in sizes}
    assert all(v > 0 and v % 8 == 0 for v in got.values())
    by_pairs = sorted(sizes, key=lambda s: s[0] * s[1])
    grow_both = [(1, 1), (64, 64), (1000, 1000), (50000, 50000)]
    assert [got[s] for s in grow_both] == sorted(got[s] for s in grow_both) and got[by_pairs[0]] <= got[by_pairs[-1]]
    assert got[(50000, 50000)] < 50000 * 50000 // 512           # the grid, never M * N
    assert dll.jck_pairstat_ws_bytes(0, 5) == 0 and dll.jck_pairstat_ws_bytes(5, -1) == 0


def test_entry_points_validate_their_arguments_on_the_host():
    """every argument error comes back as JCK_E_ARG with a message before any device call (no GPU here)"""
    from hipgan import _lib
    dll = _lib.load_library()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    for k in (0, 9):
        assert dll.jck_knn_radius2_f32(p, 16, 4, k, p, None) == E_ARG and b"k must be 1..8" in dll.jck_last_error()
    assert dll.jck_knn_radius2_f32(p, 3, 4, 3, p, None) == E_ARG and b"smaller than" in dll.jck_last_error()          # k == N
    assert dll.jck_knn_radius2_f32(p, 3, 4, 8, p, None) == E_ARG                                                      # k > N
    assert dll.jck_knn_radius2_f32(None, 16, 4, 3, p, None) == E_ARG and dll.jck_knn_radius2_f32(p, 16, 4, 3, None, None) == E_ARG
    assert dll.jck_knn_radius2_f32(p, 0, 4, 1, p, None) == E_ARG and dll.jck_knn_radius2_f32(p, 16, 0, 3, p, None) == E_ARG
    ok = [p, 4, p, 4, 4, 0.25, 1.0, 0, p, p, None]
    for i, bad in ((0, None), (2, None), (8, None), (9, None), (1, 0), (3, 0), (4, 0), (1, -2)):
        a = list(ok)
        a[i] = bad
        assert dll.jck_poly3_sum_f64(*a) == E_ARG and b"poly3_sum" in dll.jck_last_error(), i
    ok = [p, 4, p, p, 4, 4, p, None]
    for i, bad in ((0, None), (2, None), (3, None), (6, None), (1, 0), (4, 0), (5, 0)):
        a = list(ok)
        a[i] = bad
        assert dll.jck_manifold_hit_u8(*a) == E_ARG and b"manifold_hit" in dll.jck_last_error(), i


def test_without_the_flag_nothing_is_added(monkeypatch):
    """--extra_metrics absent: the argument namespace has today's keys, and the evaluation's device part of both trainers
    returns today's tensors (the trainers' own closures, driven with stand-ins for the engine and the metric network)."""
    import main
    base = {"test", "model_path", "log_file", "model", "num_worker", "batch_size", "epoch", "max_learning_rate", "min_learning_rate",
            "weight_decay", "nesterov"}
    assert set(vars(main.get_arg_parse([]))) == base
    assert set(vars(main.get_arg_parse(["--extra_metrics", "1"]))) == base | {"extra_metrics"}
    assert main.get_arg_parse(["--extra_metrics", "1"]).extra_metrics == 1
    with pytest.raises(SystemExit):
        main.get_arg_parse(["--extra_metrics", "2"])

    from train import cgan_trainer, dcgan_trainer

    class Logits:
        is_cuda = True

    class Metric:
        def logits(self, x):
            return Logits()

        def fake_stats_device(self, logits, intra=False):
            return {"mu": 0, "cov": 0, **({f"{n}_s{s}": 0 for s in range(20) for n in ("mu", "cov")} if intra else {})}

        def fake_pair_stats_device(self, logits, intra=False):
            return {"kid_rr": 0, "kid_ff": 0, "kid_rf": 0, "hit_fake": 0, "hit_real": 0,
                    **({f"kid_{n}_s{s}": 0 for s in range(20) for n in ("rr", "ff", "rf")} if intra else {})}

    class Eval:
        def launch(self, iters, sample, device_part):
            self.keys = set(device_part(torch.zeros(10, 3, 4, 4)))

    monkeypatch.setattr(dcgan_trainer, "inception_input", lambda fake: fake)
    monkeypatch.setattr(cgan_trainer, "inception_input", lambda fake: fake)
    today_d = {"images", "logits", "mu", "cov"}
    today_c = {"denorm", "logits", "mu", "cov"} | {f"{n}_s{s}" for s in range(20) for n in ("mu", "cov")}
    for flag in (False, True):
        stub = types.SimpleNamespace(metric=Metric(), extra_metrics=flag, _eval=Eval(), _finish_eval=lambda best, wait: None,
                                     _sampler_for=lambda n: None)
        dcgan_trainer.DCGANTrainer._evaluate(stub, torch.zeros(4, 100, 1, 1), 0, {})
        extra = stub._eval.keys - today_d
        assert (extra == {"kid_rr", "kid_ff", "kid_rf", "hit_fake", "hit_real"}) if flag else (stub._eval.keys == today_d)
        cgan_trainer.CGANTrainer._evaluate(stub, torch.zeros(4, 100, 1, 1), None, 0, {}, "img")
        assert (len(stub._eval.keys - today_c) == 65) if flag else (stub._eval.keys == today_c)
