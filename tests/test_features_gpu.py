"""Discriminator features: the pooling kernel (jck_grid_pool), the engine path (jck_engine_features; DcganEngine.features /
features_latents) and what is built on it (hipgan.probe.knn_probe, Sampler.neighbours(space="d"), generate.py --features / --probe /
--space d).

Pool, exact: max never rounds, so on any data the result equals torch's max pool with `==` (seeded normals; bf16 on bf16-representable ones); the
mean is taken on integers 0..15 - a window sum is at most 15 * 1024 < 2^24 and 1 / w^2 is a power of two, so sum and product are exact in
any order.  The sign of a zero is not asserted.

Engine against the module: model.DCGAN / model.CGAN .Discriminator().eval() in fp32 on the oracle's weights with running statistics
drawn as tests/test_score_gpu.py draws them, forward hooks on the LeakyReLU outputs of the conv stack.  The modules' own forward hands
the whole stack to the HIP kernels and never calls its child layers, so the reference drives those children - the torch.nn layers
that hold the weights, conv_i -> norm_i -> relu_i on the CPU - and the hooks see what they return.  Bound: the project's _parity
(tests/test_sample_eval_gpu.py: |a - b| <= 1e-6 + rtol * max(|b|, rms b), rtol 2e-4 for f32 and bf16x3, 1.2e-1 for bf16) per stage
block; pooling is 1-Lipschitz in the sup norm, so what bounds D's activations bounds their pools.

Measured on one MI355X (worst err / tol per precision): see DESIGN.md section 5.13."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_sample_eval_gpu import _parity
from test_score_gpu import _arenas, _ckpt, _engine, _gen, _images, _z

pytestmark = pytest.mark.gpu
DT = {0: torch.bfloat16, 1: torch.float32}
PREC_NAME = {0: "bf16", 1: "f32"}
SENTINEL = -777.0
POOL = {"max": 0, "mean": 1}
# (N, H, C, grid): window 1; a C that is no multiple of 64; grid 2; grid 1; window 8; the smallest C with the largest window
SHAPES = [(1, 4, 64, 4), (3, 8, 72, 4), (2, 8, 128, 2), (1, 16, 64, 1), (2, 32, 64, 4), (1, 64, 8, 2)]


@pytest.fixture(scope="module")
def G():
    import gpu_util
    return gpu_util


def _torch_pool(a_nhwc, grid, pool):
    """the torch counterpart on the CPU: fp32 [N, grid * grid * C], cell-major and channel-minor"""
    x = a_nhwc.float().permute(0, 3, 1, 2)
    p = F.adaptive_max_pool2d(x, grid) if pool == "max" else F.adaptive_avg_pool2d(x, grid)
    return p.permute(0, 2, 3, 1).flatten(1)


def _run_pool(G, a, grid, pool, prec, pad=True):
    """jck_grid_pool on a CPU NHWC tensor -> (the block [N, grid^2 C], the whole output [N, ld]) on the CPU"""
    n, h, _, c = a.shape
    Fb = grid * grid * c
    ld, col0 = (Fb + 24, 8) if pad else (Fb, 0)
    out = torch.full((n, ld), SENTINEL, device="cuda")
    G.lib.jck_grid_pool(prec, a.to(DT[prec]).cuda().contiguous(), n, h, c, grid, POOL[pool], out, ld, col0, G.cur_stream())
    out = out.cpu()
    return out[:, col0:col0 + Fb], out, col0, Fb


@pytest.mark.parametrize("prec", [0, 1], ids=PREC_NAME.get)
@pytest.mark.parametrize("pool", ["max", "mean"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_grid_pool_exact(G, shape, pool, prec):
    n, h, c, grid = shape
    if pool == "max":
        a = torch.randn(n, h, h, c, generator=_gen(51))
        if prec == 0:
            a = a.to(torch.bfloat16).float()                         # bf16 storage: on values it can hold
    else:
        a = torch.randint(0, 16, (n, h, h, c), generator=_gen(52)).float()
        assert 15 * (h // grid) ** 2 < 2 ** 24
    ref = _torch_pool(a, grid, pool)
    got, out, col0, Fb = _run_pool(G, a, grid, pool, prec)
    assert got.shape == ref.shape and bool((got == ref).all()), f"{shape} {pool} {PREC_NAME[prec]}: {int((got != ref).sum())} of {ref.numel()} differ"
    assert bool((out[:, :col0] == SENTINEL).all()) and bool((out[:, col0 + Fb:] == SENTINEL).all()), "wrote outside its column block"


@pytest.mark.parametrize("prec", [0, 1], ids=PREC_NAME.get)
def test_grid_pool_non_finite(G, prec):
    n, h, c, grid = 2, 8, 72, 4
    a = torch.randn(n, h, h, c, generator=_gen(53)).to(torch.bfloat16).float()
    a[1, 5, 2, 70] = float("nan")                      # cell (2, 1), channel 70 of image 1
    a[0, 0:2, 6:8, 3] = float("-inf")                  # the whole window of cell (0, 3), channel 3 of image 0
    a[0, 7, 0, 9] = float("inf")                       # cell (3, 0), channel 9 of image 0
    a[1, 4, 2, 70] = float("inf")                      # beside the NaN: the NaN still wins
    got = _run_pool(G, a, grid, "max", prec)[0].view(n, grid, grid, c)
    nan = torch.isnan(got)
    assert int(nan.sum()) == 1 and bool(nan[1, 2, 1, 70])
    assert float(got[0, 0, 3, 3]) == float("-inf") and int(torch.isinf(got).sum()) == 2
    assert float(got[0, 3, 0, 9]) == float("inf")
    ref = _torch_pool(a, grid, "max").view(n, grid, grid, c)
    assert torch.equal(torch.isnan(ref), nan) and bool((got[~nan] == ref[~nan]).all())
    # the mean passes them on as a sum does
    gm = _run_pool(G, a, grid, "mean", prec)[0].view(n, grid, grid, c)
    assert bool(torch.isnan(gm[1, 2, 1, 70])) and float(gm[0, 0, 3, 3]) == float("-inf") and float(gm[0, 3, 0, 9]) == float("inf")
    assert int((~torch.isfinite(gm)).sum()) == 3


def test_grid_pool_refusals(G):
    from hipgan import JckError
    buf = torch.zeros(2 * 8 * 8 * 64 + 8, device="cuda")
    a = buf[:2 * 8 * 8 * 64]
    out = torch.full((2, 1024 + 24), SENTINEL, device="cuda")
    call = lambda a_=a, n=2, h=8, c=64, grid=4, col0=8, prec=1, ld=1048: G.lib.jck_grid_pool(prec, a_, n, h, c, grid, 0, out, ld, col0, G.cur_stream())
    for kw, word in ((dict(grid=3), "grid must be"), (dict(h=6), "multiple of grid"), (dict(c=12), "multiple of 8"), (dict(a_=None), "null"),
                     (dict(a_=buf[1:1 + 2 * 8 * 8 * 64]), "16-byte aligned"), (dict(col0=6), "16-byte aligned"), (dict(n=2, ld=1050), "16-byte aligned"),
                     (dict(col0=32), "column block"), (dict(prec=7), "bad prec")):
        with pytest.raises(JckError, match=word):
            call(**kw)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    call()
    assert bool((out[:, 8:1032] == 0).all()) and bool((out[:, :8] == SENTINEL).all()) and bool((out[:, 1032:] == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------------
# engine
# ---------------------------------------------------------------------------------------------------------------------
_refs = {}


def _module_activations(family, size, x):
    """the LeakyReLU outputs of the module's conv stack in eval mode, fp32 on the CPU: [NCHW tensors], stage 0 first"""
    from model import CGAN, DCGAN
    kw = {"image_size": size} if size != 64 else {}
    d = CGAN.Discriminator() if family == "cgan" else DCGAN.Discriminator(**kw)
    # the oracle's weights and the drawn running statistics, as every engine of _engine(family, ...) holds them in fp32
    d.load_state_dict({k: v.cpu() for k, v in _engine(family, "f32", batch=2 if size == 128 else 8, size=size).state_dicts()[1].items()})
    d = d.eval()
    acts, hooks, i = [], [], 1
    while hasattr(d, f"norm{i}"):
        hooks.append(getattr(d, f"relu{i}").register_forward_hook(lambda m, inp, out: acts.append(out.detach().clone())))
        i += 1
    with torch.no_grad():
        h = x
        for j in range(1, i):
            h = getattr(d, f"relu{j}")(getattr(d, f"norm{j}")(getattr(d, f"conv{j}")(h)))
    for hk in hooks:
        hk.remove()
    assert len(acts) == i - 1
    return acts


def _reference(family, size, n, seed):
    key = (family, size, n, seed)
    if key not in _refs:
        x = _images(n, seed, size)
        _refs[key] = (x, _module_activations(family, size, x))
    return _refs[key]


def _check_blocks(f, acts, size, grid, pool, prec, what):
    from hipgan.probe import feature_layout
    layout, Fdim = feature_layout(size, grid)
    assert f.shape == (acts[0].shape[0], Fdim) and f.dtype == torch.float32 and len(layout) == len(acts)
    for (stage, col0, c, h), a in zip(layout, acts):
        assert a.shape[1:] == (c, h, h)
        p = F.adaptive_max_pool2d(a, grid) if pool == "max" else F.adaptive_avg_pool2d(a, grid)
        _parity(f[:, col0:col0 + grid * grid * c], p.permute(0, 2, 3, 1).flatten(1), "bf16" if prec == "bf16" else "f32",
                f"{what} grid {grid} {pool} stage {stage}")


@pytest.mark.parametrize("prec", ["bf16", "f32", "bf16x3"])
@pytest.mark.parametrize("family", ["dcgan", "cgan"])
def test_features_match_the_module(family, prec):
    eng = _engine(family, prec)
    x, acts = _reference(family, 64, 3, 61)
    before = _arenas(eng)
    for grid, pool in ((4, "max"), (1, "max"), (4, "mean"), (1, "mean")):
        _check_blocks(eng.features(x, grid=grid, pool=pool), acts, 64, grid, pool, prec, f"{family} {prec}")
    after = _arenas(eng)
    assert set(before) == set(after) and all(torch.equal(before[k], after[k]) for k in before)


def test_features_image_size_128():
    eng = _engine("dcgan", "f32", batch=2, size=128)
    x, acts = _reference("dcgan", 128, 2, 62)
    for grid, pool in ((4, "max"), (1, "max"), (4, "mean"), (1, "mean")):
        _check_blocks(eng.features(x, grid=grid, pool=pool), acts, 128, grid, pool, "f32", "dcgan 128 f32")


def test_feature_dim_and_layout(G):
    from hipgan import JckError
    from hipgan.probe import feature_layout
    eng = _engine("dcgan", "f32")
    for grid in (1, 2, 4):
        assert G.lib.jck_engine_feature_dim(eng._h, grid) == feature_layout(64, grid)[1]
    assert G.lib.jck_engine_feature_dim(eng._h, 4) == 15360 and G.lib.jck_engine_feature_dim(eng._h, 3) == 0
    e128 = _engine("dcgan", "f32", batch=2, size=128)
    assert G.lib.jck_engine_feature_dim(e128._h, 4) == feature_layout(128, 4)[1] == 31744
    # the window of the deepest stage is one element at grid 4: its block is the activation itself, and every coarser raster is torch's
    # max pool of the finer one, bit for bit (a maximum rounds nothing)
    x = _images(3, 63)
    f4, f2, f1 = (eng.features(x, grid=g).cpu() for g in (4, 2, 1))
    for (stage, c4, c, h), (_, c2, _, _), (_, c1, _, _) in zip(*(feature_layout(64, g)[0] for g in (4, 2, 1))):
        b4 = f4[:, c4:c4 + 16 * c].view(3, 4, 4, c).permute(0, 3, 1, 2)
        b2 = F.max_pool2d(b4, 2)
        assert torch.equal(b2.permute(0, 2, 3, 1).flatten(1), f2[:, c2:c2 + 4 * c]), stage
        assert torch.equal(F.max_pool2d(b2, 2).flatten(1), f1[:, c1:c1 + c]), stage
    # the engine's guards
    out = torch.zeros(9, 15360 + 4, device="cuda")
    xd = x.cuda()
    for args, word in (((xd, 0, 4, 0, out, 15360), "n must be"), ((xd, 9, 4, 0, out, 15360), "n must be"), ((xd, 3, 3, 0, out, 15360), "grid"),
                       ((xd, 3, 4, 2, out, 15360), "mode"), ((xd, 3, 4, 0, None, 15360), "out"), ((xd, 3, 4, 0, out, 15356), "ld"),
                       ((xd, 3, 4, 0, out, 15362), "ld"), ((xd, 3, 4, 0, out.view(-1)[1:], 15360), "aligned")):
        with pytest.raises(JckError, match=word):
            G.lib.jck_engine_features(eng._h, *args, G.cur_stream())
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0
    G.lib.jck_engine_features(eng._h, xd, 3, 4, 0, out, 15364, G.cur_stream())          # a wider row: the tail columns stay
    assert torch.equal(out[:3, :15360].cpu(), f4) and float(out[:, 15360:].abs().max()) == 0.0 and float(out[3:].abs().max()) == 0.0
    with pytest.raises(JckError, match="pool"):
        eng.features(x, pool="min")
    with pytest.raises(JckError, match="64x64"):
        eng.features(_images(1, 1, 128))
    from hipgan.engine import DcganEngine
    fresh = DcganEngine(batch=4, prec="bf16")                      # its discriminator was never loaded: nothing is packed
    with pytest.raises(JckError, match="never packed"):
        G.lib.jck_engine_features(fresh._h, xd, 3, 4, 0, out, 15360, G.cur_stream())


@pytest.mark.parametrize("prec", ["bf16", "f32"])
@pytest.mark.parametrize("family", ["dcgan", "cgan"])
def test_feature_rows_are_independent(family, prec):
    """features(x)[i] is features(x[i:i+1]); n = batch + 3 is the per-chunk calls; uint8 NHWC is the float path on u8 / 127.5 - 1;
    changing image 2 leaves row 3 alone"""
    eng = _engine(family, prec)
    u8 = torch.randint(0, 256, (11, 64, 64, 3), generator=_gen(64), dtype=torch.uint8)
    xf = (u8.float() / 127.5 - 1.0).permute(0, 3, 1, 2).contiguous()
    full = eng.features(u8)
    assert full.shape == (11, 15360) and torch.equal(full, eng.features(xf)) and bool(torch.isfinite(full).all())
    assert torch.equal(torch.cat([eng.features(xf[:8]), eng.features(xf[8:])]), full)
    for i in (0, 3, 7, 8, 10):
        assert torch.equal(eng.features(xf[i:i + 1]), full[i:i + 1]), i
    x2 = xf[:8].clone()
    x2[2] = -x2[2]
    other = eng.features(x2)
    assert torch.equal(other[3], full[3]) and not torch.equal(other[2], full[2])


@pytest.mark.parametrize("prec", ["bf16", "f32", "bf16x3"])
@pytest.mark.parametrize("family", ["dcgan", "cgan"])
def test_features_latents(family, prec):
    """the features of G(z) with the images left on the device: bit for bit those of the fp32 copy of the same images (an image
    already rounded to the storage type survives the round trip through fp32)"""
    eng = _engine(family, prec)
    z, lab = _z(11, 65, family)
    before = _arenas(eng)
    for grid, pool in ((4, "max"), (2, "mean")):
        got = eng.features_latents(z, lab, grid=grid, pool=pool)
        assert torch.equal(got, eng.features(eng.sample(z, lab, bn="running"), grid=grid, pool=pool)), (grid, pool)
    after = _arenas(eng)
    assert all(torch.equal(before[k], after[k]) for k in before)


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graph"])
def test_features_between_two_training_steps_change_no_bit(graphs):
    """The protocol of tests/test_score_gpu.py: a training engine (DCGAN, B = 8, bf16) with features calls between every two steps -
    scalars and every arena equal those of the run without them, bit for bit.  eager: the next batch announced, so that its D(real)
    forward is in flight; graph: the steps replayed from captured graphs on the engine's own stream."""
    from hipgan.engine import DcganEngine
    from oracle.gan_oracle import build_params
    from util import synth_images
    B, steps = 8, 4 if graphs else 3
    imgs = synth_images(B * steps).cuda()
    x, z = _images(5, 66), _z(5, 67, "dcgan")[0]
    res = []
    for with_features in (False, True):
        torch.manual_seed(12345)
        g, d = build_params("dcgan")
        eng = DcganEngine(batch=B, prec="bf16", device="cuda:0")
        eng.graphs = graphs
        eng.load_state(g, d)
        eng.set_noise_seed(77)
        gen = torch.Generator(device="cuda").manual_seed(5)
        scal = []
        for s in range(steps):
            kw = dict(next_real=imgs[(s + 1) * B:(s + 2) * B]) if s + 1 < steps and not graphs else {}
            eng.step_async(imgs[s * B:(s + 1) * B], None, 2e-4, generator=gen, **kw)
            if kw:
                assert eng._prefetched_real is not None
            if with_features:
                f = eng.features(x, grid=4 if s % 2 == 0 else 2, pool="max" if s % 2 == 0 else "mean")
                assert bool(torch.isfinite(f).all())
                if kw:
                    assert eng._prefetched_real is not None          # the call did not drop the prefetched pass
            scal.append(eng.scalars())
        torch.cuda.synchronize()
        assert (len(eng._graph_cache) > 0) == graphs
        res.append((scal, {k: v.clone() for k, v in eng.arenas.items()}))
    assert res[0][0] == res[1][0], (res[0][0], res[1][0])
    for k, v in res[0][1].items():
        assert torch.equal(v, res[1][1][k]), k


def _patterns(n, seed):
    """n pictures, each a random 8 x 8 uint8 pattern repeated to 64 x 64"""
    p = torch.randint(0, 256, (n, 8, 8, 3), generator=_gen(seed), dtype=torch.uint8)
    return p.repeat(1, 8, 8, 1)


def test_probe_plumbing():
    from hipgan.probe import knn_probe
    eng = _engine("dcgan", "bf16")
    train = _patterns(24, 68)
    labels = torch.arange(24) % 5
    perm = torch.randperm(24, generator=_gen(69))
    r = knn_probe(eng, train, labels, train[perm], labels[perm], k=1, chunk=7)
    assert r["idx"].shape == (24, 1) and np.array_equal(r["idx"][:, 0], perm.numpy())
    assert r["d2"].dtype == np.float32 and bool((r["d2"] == 0).all())
    assert r["accuracy"] == 1.0 and np.array_equal(r["pred"], labels[perm].numpy())
    assert r["per_class"] == {c: 1.0 for c in range(5)}
    # wrong labels for the test set are counted as wrong
    r2 = knn_probe(eng, train, labels, train[perm], (labels[perm] + (torch.arange(24) < 6)) % 5, k=1, chunk=24, normalise="none")
    assert r2["accuracy"] == 18 / 24 and np.array_equal(r2["pred"], r["pred"])
    from hipgan import JckError
    with pytest.raises(JckError, match="k ="):
        knn_probe(eng, train, labels, train, labels, k=9)
    with pytest.raises(JckError, match="labels"):
        knn_probe(eng, train, labels[:5], train, labels)


def test_sampler_features_and_feature_space_neighbours():
    from hipgan import JckError
    from hipgan.probe import feature_layout, normalise_blocks
    from hipgan.sampler import Sampler
    from metrics import nearest
    q = torch.randint(0, 256, (5, 64, 64, 3), generator=_gen(70), dtype=torch.uint8)
    ref = torch.randint(0, 256, (12, 64, 64, 3), generator=_gen(71), dtype=torch.uint8)
    ref[7] = q[2]                                                     # a copy: found at distance 0 and flagged
    plain = Sampler.from_checkpoint(_ckpt(), "DCGAN", batch=8)
    for call in (lambda: plain.features(q), lambda: plain.neighbours(q, ref, k=3, space="d"), lambda: plain.knn_probe(ref, torch.arange(12), q, torch.arange(5))):
        with pytest.raises(JckError, match="discriminator"):
            call()
    s = Sampler.from_checkpoint(_ckpt(), "DCGAN", batch=8, with_d=True)
    layout = feature_layout(64, 4)[0]
    fq, fr = s.features(q), s.features(ref)
    assert fq.shape == (5, 15360) and torch.equal(fq, s.engine.features(q))
    idx, d2 = nearest(normalise_blocks(fq, layout), normalise_blocks(fr, layout), 3)
    r = s.neighbours(q, ref, k=3, space="d")
    assert sorted(r) == ["copy", "d2", "idx", "ref_nn_d2"]
    assert np.array_equal(r["idx"], idx.cpu().numpy()) and np.array_equal(r["d2"], d2.cpu().numpy())
    assert r["idx"][2, 0] == 7 and r["d2"][2, 0] == 0.0 and bool(r["copy"][2]) and np.array_equal(r["copy"], r["d2"][:, 0] < r["ref_nn_d2"])
    # the leave-one-out distance of the matched reference rows: the kernel's own bound on a distance, (D + 4) 2^-24 relative, both ways
    li, ld = nearest(normalise_blocks(fr, layout), normalise_blocks(fr, layout), 1, exclude_self=True)
    assert np.allclose(r["ref_nn_d2"], ld.cpu().numpy()[r["idx"][:, 0], 0], rtol=2 * (15360 + 4) * 2.0 ** -24, atol=0)
    with pytest.raises(JckError, match="space"):
        s.neighbours(q, ref, k=3, space="z")
    a, b = s.neighbours(q, ref, k=3, space="pixel"), s.neighbours(q, ref, k=3)
    assert sorted(a) == sorted(b) == ["copy", "d2", "idx", "ref_nn_d2", "rmse"] and all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


def test_generate_features_cli(tmp_path):
    import generate
    from hipgan.probe import feature_layout
    from hipgan.sampler import Sampler
    path = str(tmp_path / "ckpt.pt")
    torch.save(_ckpt(), path)
    train, labels = _patterns(24, 72), np.arange(24) % 5
    perm = torch.randperm(24, generator=_gen(73))
    np.savez(tmp_path / "train.npz", images=train.numpy(), labels=labels)
    np.savez(tmp_path / "test.npz", images=train[perm].numpy(), labels=labels[perm.numpy()])
    base = ["-m", "DCGAN", "--checkpoint", path, "-b", "8"]
    out = str(tmp_path / "feats")
    assert generate.main(base + ["--features", str(tmp_path / "train.npz"), "--feature_grid", "2", "--out", out]) == 0
    f = np.load(os.path.join(out, "features.npz"))
    assert f["features"].shape == (24, 3840) and f["features"].dtype == np.float32 and np.array_equal(f["labels"], labels)
    assert f["layout"].tolist() == [list(b) for b in feature_layout(64, 2)[0]] and int(f["grid"]) == 2 and str(f["pool"]) == "max"
    s = Sampler.from_checkpoint(path, "DCGAN", batch=8, with_d=True)
    assert np.array_equal(s.features(train, grid=2).cpu().numpy(), f["features"])
    out = str(tmp_path / "probe")
    assert generate.main(base + ["--probe", str(tmp_path / "train.npz"), "--probe_test", str(tmp_path / "test.npz"), "--k", "1", "--out", out]) == 0
    p = json.load(open(os.path.join(out, "probe.json")))
    assert p["accuracy"] == 1.0 and p["k"] == 1 and (p["train"], p["test"], p["F"], p["grid"], p["pool"]) == (24, 24, 15360, 4, "max")
    assert p["per_class"] == {str(c): 1.0 for c in range(5)}
    out = str(tmp_path / "nb")
    assert generate.main(base + ["--num", "6", "--seed", "3", "--neighbours", str(tmp_path / "train.npz"), "--space", "d", "--k", "2", "--out", out]) == 0
    nb = np.load(os.path.join(out, "neighbours.npz"))
    assert sorted(nb.files) == ["copy", "d2", "idx", "ref_nn_d2"] and nb["idx"].shape == (6, 2) and os.path.exists(os.path.join(out, "neighbours.png"))
    img = np.load(os.path.join(out, "images.npz"))["images"]
    want = s.neighbours(torch.from_numpy(img), train, k=2, space="d")
    assert np.array_equal(nb["idx"], want["idx"]) and np.array_equal(nb["d2"], want["d2"])
    # without the new flags the sampling output is what it was: the same bytes as the run above minus the neighbour files
    plain = str(tmp_path / "plain")
    assert generate.main(base + ["--num", "6", "--seed", "3", "--out", plain]) == 0
    assert np.load(os.path.join(plain, "images.npz"))["images"].tobytes() == img.tobytes() and not os.path.exists(os.path.join(plain, "neighbours.npz"))
