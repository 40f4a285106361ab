"""Centre and random crops in front of the resize, on the device: jck_img_prep_u8_box against what Pillow returns for crop().resize()
(tests/golden/crop_resize_u8.json) with a scalar origin and with one origin per image; a whole-image box against jck_img_prep_u8_any
bit for bit; flips inside the box; clamped origins; an unaligned dataset; refusals; which kernel a DeviceBatch with a box runs; engine
steps, eager and replayed, fed by indices against steps fed the transformed tensor; the loader's origins; a trainer run with --crop."""
import ctypes
import logging
import os

import numpy as np
import pytest
import torch

from crop_ref import CASES, case_inputs, host_crop_resize, ids, reference
from resize_any_ref import case_inputs as whole_inputs, normalized

pytestmark = pytest.mark.gpu
E_ARG = -1
LABEL = "img_prep_u8_box"              # the kernel's profiler label; like its two neighbours it has no launch name


@pytest.fixture(scope="module")
def G():
    import gpu_util
    return gpu_util


def _taps(h, w, s):
    from hipgan.engine import resize_taps
    return resize_taps(h, w, s, "cuda")


def _box(G, prec, data, idx, flip, origin, noise, rng, keep, mix, out4, out_nchw, b, hc, wc, y0, x0, s, taps=None):
    hs, ws = data.shape[2:]
    G.lib.jck_img_prep_u8_box(prec, data, idx, flip, origin, noise, rng, 0, keep, mix, out4, out_nchw, b, hs, ws, hc, wc, y0, x0, s,
                              taps if taps is not None else _taps(hc, wc, s), G.cur_stream())


def _origins(hs, ws, hc, wc, y0, x0, n):
    """n different origins where the geometry has room for them: the case's own, both extreme corners, one in between"""
    my, mx = hs - hc, ws - wc
    return [(y0, x0), (0, 0), (my, mx), (my // 2, mx // 3), (0, mx), (my, 0)][:n]


@pytest.mark.parametrize("case", CASES, ids=ids())
def test_transformed_box_is_pillows(G, case):
    hs, ws, hc, wc, y0, x0, s, n = case
    x, y = reference(*case)
    data = torch.from_numpy(np.array(x)).cuda()
    order = [n - 1, 0, n - 1, 1, 0, n - 1]                              # repeats, out of order
    idx = torch.tensor(order, dtype=torch.int64, device="cuda")
    out = torch.full((len(order), 3, s, s), 9.0, device="cuda")
    _box(G, G.PREC_F32, data, idx, None, None, None, None, 1.0, 0.0, None, out, len(order), hc, wc, y0, x0, s)
    # one origin per image; the expected images are the host statement on each slice (its taps are those of (hc, wc, s), which the
    # scalar run above has just held against Pillow's bytes)
    org = _origins(hs, ws, hc, wc, y0, x0, len(order))
    vec = torch.full((len(order), 3, s, s), 9.0, device="cuda")
    _box(G, G.PREC_F32, data, idx, None, torch.tensor(org, dtype=torch.int32, device="cuda"), None, None, 1.0, 0.0, None, vec, len(order),
         hc, wc, 0, 0, s)
    first = torch.full((n, 3, s, s), 9.0, device="cuda")
    _box(G, G.PREC_F32, data, None, None, None, None, None, 1.0, 0.0, None, first, n, hc, wc, y0, x0, s)      # idx = NULL: the first n
    torch.cuda.synchronize()
    want = normalized(y)
    assert torch.equal(out.cpu(), want[order])
    assert torch.equal(first.cpu(), want)
    want_vec = torch.stack([normalized(host_crop_resize(x[i], hc, wc, oy, ox, s)) for i, (oy, ox) in zip(order, org)])
    assert torch.equal(vec.cpu(), want_vec)
    if (hs - hc, ws - wc) != (0, 0) and hc * wc > 1:
        assert len({tuple(o) for o in org}) > 1 and not torch.equal(vec.cpu(), want[order])


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("h,w,s", [(32, 32, 64), (100, 75, 64), (37, 50, 128)])
def test_whole_image_box_is_the_any_size_kernel_bit_for_bit(G, h, w, s, prec):
    """origin 0, Hc = Hs, Wc = Ws: NHWC4 outputs with a noise tensor and with the in-kernel generator, under a mixed flip vector"""
    p = G.PREC_F32 if prec == "f32" else G.PREC_BF16
    data = torch.from_numpy(whole_inputs(h, w, s, 4)).cuda()
    idx = torch.tensor([3, 0, 2, 2, 1, 0], dtype=torch.int64, device="cuda")
    flip = torch.tensor([1, 0, 0, 1, 1, 0], dtype=torch.uint8, device="cuda")
    b, numel, guard = 6, 6 * s * s * 4, 4096
    noise = torch.randn(b, 3, s, s, generator=torch.Generator().manual_seed(3)).cuda()
    rng = torch.tensor([12345, 77, 7, 0], dtype=torch.int32).cuda()
    bits = torch.int32 if prec == "f32" else torch.int16
    taps, st = _taps(h, w, s), G.cur_stream()

    def buf():
        return torch.full((numel + guard,), 7.0, dtype=G.DT[p], device="cuda")
    any_n, box_n, any_r, box_r = buf(), buf(), buf(), buf()
    nchw_any, nchw_box = torch.empty(b, 3, s, s, device="cuda"), torch.empty(b, 3, s, s, device="cuda")
    G.lib.jck_img_prep_u8_any(p, data, idx, flip, noise, None, 0, 0.9, 0.1, any_n, nchw_any, b, h, w, s, taps, st)
    _box(G, p, data, idx, flip, None, noise, None, 0.9, 0.1, box_n, nchw_box, b, h, w, 0, 0, s)
    G.lib.jck_img_prep_u8_any(p, data, idx, flip, None, rng, 0, 0.9, 0.1, any_r, None, b, h, w, s, taps, st)
    _box(G, p, data, idx, flip, None, None, rng, 0.9, 0.1, box_r, None, b, h, w, 0, 0, s)
    torch.cuda.synchronize()
    for old, new in ((any_n, box_n), (any_r, box_r)):
        assert torch.equal(old.view(bits), new.view(bits))
        assert float(new[:numel].view(b, s, s, 4)[..., 3].float().abs().max()) == 0.0                # pad channel
        assert bool((new[numel:].float() == 7.0).all())                                             # canary behind the buffer
    assert torch.equal(nchw_any.view(torch.int32), nchw_box.view(torch.int32))
    assert not torch.equal(box_n.view(bits), box_r.view(bits))                                      # (two different noises)


@pytest.mark.parametrize("case", [CASES[1], CASES[2], CASES[8]], ids=[ids()[1], ids()[2], ids()[8]])
def test_flip_mirrors_inside_the_box(G, case):
    hs, ws, hc, wc, y0, x0, s, n = case
    x, y = reference(*case)
    data = torch.from_numpy(np.array(x)).cuda()
    order = [2, 3, 1, 1, 0, 3]
    idx = torch.tensor(order, dtype=torch.int64, device="cuda")
    flip = torch.tensor([1, 0, 7, 0, 255, 0], dtype=torch.uint8, device="cuda")          # any non-zero value mirrors
    got = torch.empty(len(order), 3, s, s, device="cuda")
    _box(G, G.PREC_F32, data, idx, flip, None, None, None, 1.0, 0.0, None, got, len(order), hc, wc, y0, x0, s)
    torch.cuda.synchronize()
    crop = np.ascontiguousarray(x[:, :, y0:y0 + hc, x0:x0 + wc])
    mirrored = normalized(host_crop_resize(np.ascontiguousarray(crop[..., ::-1]), hc, wc, 0, 0, s))     # the transform of the mirrored crop
    plain = normalized(y)
    want = torch.stack([mirrored[i] if f else plain[i] for i, f in zip(order, flip.tolist())])
    assert torch.equal(got.cpu(), want) and not torch.equal(got.cpu(), plain[order])


def test_origins_outside_the_image_are_clamped(G):
    hs, ws, hc, wc, s = 48, 56, 40, 33, 64
    data = torch.randint(0, 256, (3, 3, hs, ws), generator=torch.Generator().manual_seed(9), dtype=torch.uint8).cuda()
    wild = torch.tensor([[-5, 9999], [9999, -5], [-2 ** 31, 2 ** 31 - 1]], dtype=torch.int32, device="cuda")
    tame = torch.tensor([[0, ws - wc], [hs - hc, 0], [0, ws - wc]], dtype=torch.int32, device="cuda")
    guard, n3, n4 = 8192, 3 * 3 * s * s, 3 * s * s * 4

    def run(origin):
        a, b = torch.full((n3 + 2 * guard,), 7.0, device="cuda"), torch.full((n4 + 2 * guard,), 7.0, device="cuda")
        _box(G, G.PREC_F32, data, None, None, origin, None, None, 0.9, 0.0, b[guard:guard + n4], a[guard:guard + n3], 3, hc, wc, 0, 0, s)
        return a, b
    (wa, wb), (ta, tb) = run(wild), run(tame)
    torch.cuda.synchronize()
    assert torch.equal(wa, ta) and torch.equal(wb, tb)
    for t, n in ((wa, n3), (wb, n4)):
        assert bool((t[:guard] == 7.0).all()) and bool((t[guard + n:] == 7.0).all())              # the guards before and after
    want = torch.stack([normalized(host_crop_resize(data[i].cpu().numpy(), hc, wc, oy, ox, s)) for i, (oy, ox) in enumerate(tame.tolist())])
    assert torch.equal(wa[guard:guard + n3].view(3, 3, s, s).cpu(), want)


@pytest.mark.parametrize("case", [CASES[0], CASES[3], CASES[7]], ids=[ids()[0], ids()[3], ids()[7]])
def test_unaligned_dataset_gives_the_same_images(G, case):
    """the dataset's bytes one byte into a larger buffer: no load of the kernel may rely on the dataset's alignment"""
    hs, ws, hc, wc, y0, x0, s, n = case
    x, y = reference(*case)
    data = torch.from_numpy(np.array(x)).cuda()
    big = torch.zeros(data.numel() + 64, dtype=torch.uint8, device="cuda")
    off = 1 + (-big.data_ptr()) % 4                                     # one byte past a dword boundary
    shifted = big[off:off + data.numel()].view_as(data).copy_(data)
    assert shifted.data_ptr() % 4 == 1 and data.data_ptr() % 4 == 0 and shifted.is_contiguous()
    flip = torch.tensor([0, 1, 0, 1][:n], dtype=torch.uint8, device="cuda")
    a, b = torch.empty(n, 3, s, s, device="cuda"), torch.empty(n, 3, s, s, device="cuda")
    _box(G, G.PREC_F32, data, None, flip, None, None, None, 1.0, 0.0, None, a, n, hc, wc, y0, x0, s)
    _box(G, G.PREC_F32, shifted, None, flip, None, None, None, 1.0, 0.0, None, b, n, hc, wc, y0, x0, s)
    plain = torch.empty(n, 3, s, s, device="cuda")
    _box(G, G.PREC_F32, shifted, None, None, None, None, None, 1.0, 0.0, None, plain, n, hc, wc, y0, x0, s)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(plain.cpu(), normalized(y))


def _collect(G):
    cap = 16
    names, cnt, ms, fl = (ctypes.c_char_p * cap)(), (ctypes.c_int * cap)(), (ctypes.c_double * cap)(), (ctypes.c_double * cap)()
    by, sv = (ctypes.c_double * cap)(), (ctypes.c_void_p * cap)()
    n = G.lib.jck_prof_collect(cap, names, cnt, ms, fl, by, sv)
    return [(names[i].decode(), cnt[i]) for i in range(n)]


def test_refusals_launch_nothing(G):
    from hipgan._lib import load_library
    dll = load_library()
    data = torch.from_numpy(whole_inputs(48, 48, 64, 4)).cuda()
    out = torch.full((4, 3, 64, 64), 9.0, device="cuda")
    taps, st = _taps(40, 40, 64).data_ptr(), G.cur_stream()
    origin = torch.zeros(4, 2, dtype=torch.int32, device="cuda")

    def call(d=data.data_ptr(), t=taps, org=None, b=4, hs=48, ws=48, hc=40, wc=40, y0=0, x0=0, s=64, prec=G.PREC_F32):
        return dll.jck_img_prep_u8_box(prec, d, None, None, org, None, None, 0, 1.0, 0.0, None, out.data_ptr(), b, hs, ws, hc, wc, y0, x0, s, t, st)
    before = dll.jck_last_launch()
    _collect(G)
    G.lib.jck_prof_enable(1)
    try:
        for kw in (dict(d=None), dict(t=None), dict(s=96), dict(s=32), dict(b=0), dict(b=-1), dict(hc=49), dict(wc=49), dict(hc=0), dict(y0=9),
                   dict(x0=9), dict(y0=-1), dict(hs=2000), dict(prec=7), dict(org=origin.data_ptr() + 2)):
            assert call(**kw) == E_ARG and dll.jck_last_error(), kw
    finally:
        G.lib.jck_prof_enable(0)
    torch.cuda.synchronize()
    assert _collect(G) == [] and dll.jck_last_launch() == before
    assert bool((out == 9.0).all())
    # a table built for another geometry - the whole image's, a box of another size - is recognised on the device: nothing is written
    for other in (_taps(48, 48, 64), _taps(40, 41, 64), _taps(40, 40, 128)):
        assert call(t=other.data_ptr()) == 0
    torch.cuda.synchronize()
    assert bool((out == 9.0).all())
    assert call(y0=8, x0=8) == 0 and call(org=origin.data_ptr()) == 0                 # (the accepted forms of the same call do write)
    torch.cuda.synchronize()
    assert not bool((out == 9.0).any())


def test_which_kernel_a_device_batch_with_a_box_runs(G):
    from hipgan import JckError
    from hipgan.engine import DeviceBatch
    hs, ws, hc, wc, y0, x0, s, n = CASES[3]
    x, y = reference(*CASES[3])
    data = torch.from_numpy(np.array(x)).cuda()
    idx = torch.tensor([1, 3, 0], dtype=torch.int64)
    org = torch.tensor([[7, 7], [0, 3], [2, 0]], dtype=torch.int32)
    before = G.lib.jck_last_launch()
    got = {}
    for name, batch in (("scalar", DeviceBatch(data, idx, 64, None, (hc, wc, (y0, x0)))), ("vector", DeviceBatch(data, idx, box=(hc, wc, org))),
                        ("whole", DeviceBatch(data, idx, box=(hs, ws, (0, 0)))), ("none", DeviceBatch(data, idx))):
        _collect(G)
        G.lib.jck_prof_enable(1)
        try:
            t = batch.materialize()
        finally:
            G.lib.jck_prof_enable(0)
        torch.cuda.synchronize()
        got[name] = (_collect(G), t.cpu())
        assert batch.size(0) == 3 and tuple(t.shape) == (3, 3, 64, 64)
    assert G.lib.jck_last_launch() == before
    assert got["scalar"][0] == got["vector"][0] == got["whole"][0] == [(LABEL, 1)] and got["none"][0] == [("img_prep_u8_any", 1)]
    assert torch.equal(got["scalar"][1], normalized(y)[idx])
    assert torch.equal(got["vector"][1], torch.stack([normalized(host_crop_resize(x[i], hc, wc, oy, ox, 64)) for i, (oy, ox) in zip(idx.tolist(), org.tolist())]))
    assert torch.equal(got["whole"][1], got["none"][1])
    for bad in ((hc, wc, org.long()), (hc, wc, org[:2]), (hc, wc, org.flatten()), (49, wc, (0, 0)), (hc, 0, (0, 0)), (hc, wc, (8, 0)), (hc, wc, (0, -1)),
                (hc, wc), (hc, wc, (0, 0, 0))):
        with pytest.raises(JckError):
            DeviceBatch(data, idx, 64, None, bad)


# ---- engine steps ------------------------------------------------------------------------------------------------------------
def _steps(family, h, w, k, s, feed, graphs, steps):
    """`steps` f32 engine steps at B = 8 from a seeded h x w dataset, a k x k box at per-image origins under a mixed flip vector
    -> (scalars per step, arenas, captured graphs)"""
    from hipgan.engine import CganEngine, DcganEngine, DeviceBatch
    from oracle.gan_oracle import build_params
    B = 8
    torch.manual_seed(12345)
    g, d = build_params(family, s) if s != 64 else build_params(family)
    eng = CganEngine(batch=B, prec="f32") if family == "cgan" else DcganEngine(batch=B, prec="f32", **({"image_size": s} if s != 64 else {}))
    eng.graphs = graphs
    eng.load_state(g, d)
    data = torch.randint(0, 256, (20, 3, h, w), generator=torch.Generator().manual_seed(h + w), dtype=torch.uint8).cuda()
    gen = torch.Generator(device="cuda").manual_seed(5)
    sc, seen = [], []
    for t in range(steps):
        hg = torch.Generator().manual_seed(100 + t)
        idx, flip = torch.randperm(20, generator=hg)[:B], torch.randint(0, 2, (B,), generator=hg, dtype=torch.uint8)
        org = torch.stack([torch.randint(0, h - k + 1, (B,), generator=hg, dtype=torch.int32), torch.randint(0, w - k + 1, (B,), generator=hg, dtype=torch.int32)], 1)
        seen.append(org)
        batch = DeviceBatch(data, idx, s, flip, (k, k, org))
        labels = torch.nn.functional.one_hot(torch.randint(0, 100, (B,), generator=hg), 100).cuda() if family == "cgan" else None
        eng.step_async(batch.materialize() if feed == "tensor" else batch, eng.draw_noise(gen, labels=labels), 2e-4)
        sc.append(eng.scalars())
    torch.cuda.synchronize()
    assert all(not torch.equal(seen[0], o) for o in seen[1:])
    return sc, {k_: v.clone() for k_, v in eng.arenas.items()}, len(eng._graph_cache)


def _same(a, b):
    assert a[0] == b[0], (a[0], b[0])
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k


@pytest.mark.parametrize("family,h,w,k,s", [("dcgan", 48, 56, 40, 64), ("dcgan", 37, 50, 33, 128), ("cgan", 48, 56, 40, 64)])
def test_steps_from_a_box_equal_steps_from_the_tensor(family, h, w, k, s):
    """the transform is bit-exact and the step has no float atomics: scalars and every weight agree bit for bit"""
    _same(_steps(family, h, w, k, s, "tensor", False, 2), _steps(family, h, w, k, s, "indices", False, 2))


def test_replayed_steps_from_a_box_equal_the_eager_ones():
    """JCK_GRAPH=1: idx, the flip vector and the origin vector travel through fixed-address buffers.  The first step of an engine is
    eager and each step parity captures its graph once, so steps 4..6 are replays whose origin vectors all differ."""
    eager, replay = _steps("dcgan", 48, 56, 40, 64, "indices", False, 6), _steps("dcgan", 48, 56, 40, 64, "indices", True, 6)
    assert eager[2] == 0 and replay[2] == 2, (eager[2], replay[2])
    _same(eager, replay)


# ---- loader, trainer ---------------------------------------------------------------------------------------------------------
def test_device_loader_crops():
    from preprocess.dcgan_data_preprocessor import DeviceLoader, center_origin
    n, h, w, k = 20, 48, 56, 40
    host = torch.randint(0, 256, (n, 3, h, w), generator=torch.Generator().manual_seed(2), dtype=torch.uint8)
    data = host.cuda()
    seen = []
    rand = DeviceLoader(data, 8, seed=1, mirror=True, crop="random", crop_size=k)
    for _ in range(2):
        for (img,) in rand:
            assert img.box == (k, k) and img.origin.dtype == torch.int32 and tuple(img.origin.shape) == (img.size(0), 2)
            want = []
            for i, f, (oy, ox) in zip(img.idx.tolist(), img.flip.tolist(), img.origin.tolist()):
                crop = host[i, :, oy:oy + k, ox:ox + k].numpy()
                want.append(normalized(host_crop_resize(np.ascontiguousarray(crop[..., ::-1] if f else crop), k, k, 0, 0, 64)))
            assert torch.equal(img.materialize().cpu(), torch.stack(want))
            seen.append(img.origin.cpu())
    assert len({tuple(o) for o in torch.cat(seen).tolist()}) > 8
    oy, ox = center_origin(h, w, k, k)
    for (img,) in DeviceLoader(data, 8, seed=1, crop="center", crop_size=k):
        assert img.origin is None and img.corner == (oy, ox) == (4, 8) and img.flip is None
        want = normalized(host_crop_resize(host[img.idx.cpu()].numpy(), k, k, oy, ox, 64))
        assert torch.equal(img.materialize().cpu(), want)


def _fresh_logger():
    from logger.main_logger import MainLogger
    logging.getLogger("main").handlers.clear()
    MainLogger._instance, MainLogger._initialized = None, False


def test_trainer_runs_with_a_random_crop(tmp_path, monkeypatch):
    """main.py's wiring on 40 images of 48x56 with --crop random --crop_size 40 --mirror 1: two identical runs, a checkpoint, and a
    real-feature cache whose name carries the crop"""
    import main
    import metrics
    from model import DCGAN
    from preprocess.dcgan_data_preprocessor import DCGANDataPreprocessor
    from train.dcgan_trainer import DCGANTrainer
    monkeypatch.chdir(tmp_path)
    rs = np.random.RandomState(4)
    np.savez(tmp_path / "tiles.npz", images=rs.randint(0, 256, size=(40, 48, 56, 3)).astype(np.uint8))
    # a stand-in for the metric network (its weights are not available offline), so that the real-feature cache is written ...
    monkeypatch.setattr(metrics, "default_extractor", lambda device: (lambda x: x.flatten(1)[:, :100].float()))
    made = []
    real_make = DCGANTrainer._make_metrics

    def make_metrics(self, loader):
        made.append((real_make(self, loader), loader))
        return None                                 # ... and no evaluation: the run checkpoints `latest`
    monkeypatch.setattr(DCGANTrainer, "_make_metrics", make_metrics)
    runs = []
    for run in ("a", "b"):
        _fresh_logger()
        torch.manual_seed(12345)
        args = main.get_arg_parse(["-m", "DCGAN", "-b", "16", "-e", "2", "-mlr", "0.0002", "-pm", run, "-lf", "0",
                                   "--data", str(tmp_path / "tiles.npz"), "--mirror", "1", "--crop", "random", "--crop_size", "40"])
        args.save_path = str(tmp_path / "save" / "dcgan" / run)
        pre = DCGANDataPreprocessor(args)
        pre.transform_data()
        tr = DCGANTrainer(args, DCGAN.Generator(), DCGAN.Discriminator(), pre, prec="f32")
        ld = tr.train_loader
        assert ld.mirror and (ld.crop, ld.crop_size) == ("random", 40) and tuple(ld.data.shape) == (40, 3, 48, 56)
        runs.append(tr.train())
        pts = [f for r, _, fs in os.walk(tmp_path / "save" / "dcgan" / run) for f in fs if f.endswith(".pt")]
        assert pts, "no checkpoint"
    assert len(runs[0][0]) == 6 and runs[0] == runs[1] and all(v == v for v in runs[0][0] + runs[0][1])
    caches = os.listdir(tmp_path / "data")
    assert made[0][0] is not None and len(caches) == 1 and caches[0].startswith("metric_tiles_") and caches[0].endswith("_crop40.pikl")
    assert tuple(made[0][1].images.shape) == (40, 3, 40, 40) and made[0][1].images.dtype == torch.uint8       # evaluation reads the centre box
    _fresh_logger()
