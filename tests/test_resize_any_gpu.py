"""Any-size input pipeline on the device: jck_img_prep_u8_any against what Pillow returns (tests/golden/resize_any_u8.json) and, at
32x32 -> 64, against the existing 2x kernel bit for bit; flips; refusals; which kernel a DeviceBatch runs; engine steps, eager and
replayed, fed by indices against steps fed the transformed tensor; the loader's flips; a trainer run from --data."""
import ctypes
import logging
import os

import numpy as np
import pytest
import torch

from resize_any_ref import CASES, case_inputs, case_name, normalized, reference

pytestmark = pytest.mark.gpu
E_ARG = -1
LABEL = "img_prep_u8_any"              # the new kernel's profiler label; like the 2x kernel beside it, it has no launch name


@pytest.fixture(scope="module")
def G():
    import gpu_util
    return gpu_util


def _taps(h, w, s):
    from hipgan.engine import resize_taps
    return resize_taps(h, w, s, "cuda")


def _any(G, prec, data, idx, flip, noise, rng, keep, mix, out4, out_nchw, b, s):
    h, w = data.shape[2:]
    G.lib.jck_img_prep_u8_any(prec, data, idx, flip, noise, rng, 0, keep, mix, out4, out_nchw, b, h, w, s, _taps(h, w, s), G.cur_stream())


@pytest.mark.parametrize("h,w,s,n", CASES, ids=[case_name(*c[:3]) for c in CASES])
def test_transformed_image_is_pillows(G, h, w, s, n):
    x, y = reference(h, w, s, n)
    want = normalized(y)
    data = torch.from_numpy(np.array(x)).cuda()
    order = [n - 1, 0, n - 1, 1, 0, n - 1]                              # repeats, out of order
    idx = torch.tensor(order, dtype=torch.int64, device="cuda")
    out = torch.full((len(order), 3, s, s), 9.0, device="cuda")
    _any(G, G.PREC_F32, data, idx, None, None, None, 1.0, 0.0, None, out, len(order), s)
    first = torch.full((n, 3, s, s), 9.0, device="cuda")
    _any(G, G.PREC_F32, data, None, None, None, None, 1.0, 0.0, None, first, n, s)       # idx = NULL: the first n
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), want[order])
    assert torch.equal(first.cpu(), want)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_at_2x_the_existing_kernel_bit_for_bit(G, prec):
    """32x32 -> 64: NHWC4 outputs with a noise tensor and with the in-kernel generator equal jck_img_prep_u8 / _rng bit for bit"""
    p = G.PREC_F32 if prec == "f32" else G.PREC_BF16
    data = torch.from_numpy(case_inputs(32, 32, 64, 4)).cuda()
    idx = torch.tensor([3, 0, 2, 2, 1, 0], dtype=torch.int64, device="cuda")
    b, numel, guard = 6, 6 * 64 * 64 * 4, 4096
    noise = torch.randn(b, 3, 64, 64, generator=torch.Generator().manual_seed(3)).cuda()
    rng = torch.tensor([12345, 77, 7, 0], dtype=torch.int32).cuda()
    bits = torch.int32 if prec == "f32" else torch.int16

    def buf():
        return torch.full((numel + guard,), 7.0, dtype=G.DT[p], device="cuda")
    old_n, new_n, old_r, new_r = buf(), buf(), buf(), buf()
    G.lib.jck_img_prep_u8(p, data, idx, noise, 0.9, 0.1, old_n, None, b, 32, 32, G.cur_stream())
    _any(G, p, data, idx, None, noise, None, 0.9, 0.1, new_n, None, b, 64)
    G.lib.jck_img_prep_u8_rng(p, data, idx, rng, 0, 0.9, 0.1, old_r, b, 32, 32, G.cur_stream())
    _any(G, p, data, idx, None, None, rng, 0.9, 0.1, new_r, None, b, 64)
    torch.cuda.synchronize()
    for old, new in ((old_n, new_n), (old_r, new_r)):
        assert torch.equal(old.view(bits), new.view(bits))
        assert float(new[:numel].view(b, 64, 64, 4)[..., 3].float().abs().max()) == 0.0            # pad channel
        assert bool((new[numel:].float() == 7.0).all())                                             # canary behind the buffer
    assert not torch.equal(new_n.view(bits), new_r.view(bits))                                      # (two different noises)


@pytest.mark.parametrize("h,w,s", [(100, 75, 64), (37, 50, 128)])
def test_flip_is_the_transform_of_the_mirrored_dataset(G, h, w, s):
    data = torch.from_numpy(case_inputs(h, w, s, 4)).cuda()
    idx = torch.tensor([2, 3, 1, 1, 0, 3], dtype=torch.int64, device="cuda")
    flip = torch.tensor([1, 0, 7, 0, 255, 0], dtype=torch.uint8, device="cuda")          # any non-zero value mirrors
    b = idx.numel()
    got, plain, mirrored = (torch.empty(b, 3, s, s, device="cuda") for _ in range(3))
    _any(G, G.PREC_F32, data, idx, flip, None, None, 1.0, 0.0, None, got, b, s)
    _any(G, G.PREC_F32, data, idx, None, None, None, 1.0, 0.0, None, plain, b, s)
    _any(G, G.PREC_F32, torch.flip(data, [-1]).contiguous(), idx, None, None, None, 1.0, 0.0, None, mirrored, b, s)
    torch.cuda.synchronize()
    f = flip.bool().view(b, 1, 1, 1)
    assert torch.equal(got, torch.where(f, mirrored, plain))
    assert not torch.equal(got, plain)


def _collect(G):
    cap = 16
    names, cnt, ms, fl = (ctypes.c_char_p * cap)(), (ctypes.c_int * cap)(), (ctypes.c_double * cap)(), (ctypes.c_double * cap)()
    by, sv = (ctypes.c_double * cap)(), (ctypes.c_void_p * cap)()
    n = G.lib.jck_prof_collect(cap, names, cnt, ms, fl, by, sv)
    return [(names[i].decode(), cnt[i]) for i in range(n)]


def test_refusals_launch_nothing(G):
    from hipgan._lib import load_library
    dll = load_library()
    data = torch.from_numpy(case_inputs(48, 48, 64, 4)).cuda()
    out = torch.full((4, 3, 64, 64), 9.0, device="cuda")
    taps, st = _taps(48, 48, 64).data_ptr(), G.cur_stream()
    before = dll.jck_last_launch()
    _collect(G)
    G.lib.jck_prof_enable(1)
    try:
        for b, s, t in ((4, 64, None), (4, 96, taps), (4, 32, taps), (0, 64, taps), (-1, 64, taps)):
            rc = dll.jck_img_prep_u8_any(G.PREC_F32, data.data_ptr(), None, None, None, None, 0, 1.0, 0.0, None, out.data_ptr(), b, 48, 48, s, t, st)
            assert rc == E_ARG and dll.jck_last_error(), (b, s, t)
        assert dll.jck_img_prep_u8_any(G.PREC_F32, None, None, None, None, None, 0, 1.0, 0.0, None, out.data_ptr(), 4, 48, 48, 64, taps, st) == E_ARG
        assert dll.jck_img_prep_u8_any(7, data.data_ptr(), None, None, None, None, 0, 1.0, 0.0, None, out.data_ptr(), 4, 48, 48, 64, taps, st) == E_ARG
        assert dll.jck_img_prep_u8_any(G.PREC_F32, data.data_ptr(), None, None, None, None, 0, 1.0, 0.0, None, out.data_ptr(), 4, 2000, 48, 64, taps, st) == E_ARG
    finally:
        G.lib.jck_prof_enable(0)
    torch.cuda.synchronize()
    assert _collect(G) == [] and dll.jck_last_launch() == before
    assert bool((out == 9.0).all())
    # a table built for another geometry is recognised on the device: the launch writes nothing
    G.lib.jck_img_prep_u8_any(G.PREC_F32, data, None, None, None, None, 0, 1.0, 0.0, None, out, 4, 48, 48, 64, _taps(96, 96, 64), st)
    torch.cuda.synchronize()
    assert bool((out == 9.0).all())


def test_which_kernel_a_device_batch_runs(G):
    """[N,3,32,32] without flips keeps the 2x kernel, everything else takes the new one.  Neither kernel has a launch name (the
    registry gives them profiler labels only), so jck_last_launch stays what it was and the profiler's records tell them apart."""
    from hipgan.engine import DeviceBatch
    from oracle.preprocess_oracle import transform
    idx = torch.tensor([1, 3, 0], dtype=torch.int64)
    x32, x48 = case_inputs(32, 32, 64, 4), case_inputs(48, 48, 64, 4)
    d32, d48 = torch.from_numpy(x32).cuda(), torch.from_numpy(x48).cuda()
    flip = torch.tensor([0, 1, 0], dtype=torch.uint8)
    before = G.lib.jck_last_launch()
    got = {}
    for name, batch in (("old", DeviceBatch(d32, idx)), ("new", DeviceBatch(d48, idx)), ("flip32", DeviceBatch(d32, idx, 64, flip)),
                        ("to128", DeviceBatch(d32, idx, size=128))):
        _collect(G)
        G.lib.jck_prof_enable(1)
        try:
            t = batch.materialize()
        finally:
            G.lib.jck_prof_enable(0)
        torch.cuda.synchronize()
        got[name] = (_collect(G), t.cpu())
        assert batch.size(0) == 3 and batch.size(2) == t.shape[2] == t.shape[3] == (128 if name == "to128" else 64)
    assert G.lib.jck_last_launch() == before
    assert got["old"][0] == [] and got["new"][0] == got["flip32"][0] == got["to128"][0] == [(LABEL, 1)]
    assert torch.equal(got["old"][1], torch.from_numpy(transform(x32))[idx])
    assert torch.equal(got["new"][1], normalized(reference(48, 48, 64, 4)[1])[idx])
    want = got["old"][1].clone()
    want[1] = torch.from_numpy(transform(x32[:, :, :, ::-1].copy()))[3]                 # idx[1] = 3 is the mirrored one
    assert torch.equal(got["flip32"][1], want)
    from hipgan import JckError
    for bad in (lambda: DeviceBatch(d48, idx, size=96), lambda: DeviceBatch(d48[:, :2].contiguous(), idx),
                lambda: DeviceBatch(d48, idx, 64, flip[:2]), lambda: DeviceBatch(d48.float(), idx)):
        with pytest.raises(JckError):
            bad()


# ---- engine steps ------------------------------------------------------------------------------------------------------------
def _steps(h, w, s, feed, graphs, steps):
    """`steps` f32 engine steps at B = 8 from a seeded h x w dataset with a mixed flip vector -> (scalars per step, arenas)"""
    from hipgan.engine import DcganEngine, DeviceBatch
    from oracle.gan_oracle import build_params
    B = 8
    torch.manual_seed(12345)
    g, d = build_params("dcgan", s)
    eng = DcganEngine(batch=B, prec="f32", **({"image_size": s} if s != 64 else {}))
    eng.graphs = graphs
    eng.load_state(g, d)
    data = torch.randint(0, 256, (20, 3, h, w), generator=torch.Generator().manual_seed(h + w), dtype=torch.uint8).cuda()
    gen = torch.Generator(device="cuda").manual_seed(5)
    sc = []
    for t in range(steps):
        hg = torch.Generator().manual_seed(100 + t)
        batch = DeviceBatch(data, torch.randperm(20, generator=hg)[:B], s, torch.randint(0, 2, (B,), generator=hg, dtype=torch.uint8))
        assert batch.taps is not None
        eng.step_async(batch.materialize() if feed == "tensor" else batch, eng.draw_noise(gen), 2e-4)
        sc.append(eng.scalars())
    torch.cuda.synchronize()
    return sc, {k: v.clone() for k, v in eng.arenas.items()}, len(eng._graph_cache)


def _same(a, b):
    assert a[0] == b[0], (a[0], b[0])
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k


@pytest.mark.parametrize("h,w,s", [(48, 48, 64), (37, 50, 128)])
def test_steps_from_indices_equal_steps_from_the_tensor(h, w, s):
    """the transform is bit-exact and the step has no float atomics: scalars and every weight agree bit for bit"""
    _same(_steps(h, w, s, "tensor", False, 2), _steps(h, w, s, "indices", False, 2))


def test_replayed_steps_from_indices_equal_the_eager_ones():
    """JCK_GRAPH=1: idx and the flip vector travel through fixed-address buffers; geometry, table and 'has flips' key the graph"""
    eager, replay = _steps(48, 48, 64, "indices", False, 4), _steps(48, 48, 64, "indices", True, 4)
    assert eager[2] == 0 and replay[2] == 2, (eager[2], replay[2])               # one graph per step parity
    _same(eager, replay)


# ---- loader, trainer ---------------------------------------------------------------------------------------------------------
def test_device_loader_mirror():
    from preprocess.dcgan_data_preprocessor import DeviceLoader
    n = 40
    # image i is constant i in its left half and 200 in its right half: the left-most output pixel says which image and whether mirrored
    data = torch.full((n, 3, 48, 48), 200, dtype=torch.uint8)
    data[:, :, :, :24] = torch.arange(n, dtype=torch.uint8).view(n, 1, 1, 1)
    data = data.cuda()
    onehot = torch.nn.functional.one_hot(torch.arange(n) % 100, 100).cuda()
    plain, mirror = DeviceLoader(data, 16, onehot=onehot, seed=1), DeviceLoader(data, 16, onehot=onehot, seed=1, mirror=True)
    epochs = []
    for _ in range(2):
        a, b = list(plain), list(mirror)
        assert [x[0].size(0) for x in b] == [16, 16, 8]
        assert all(torch.equal(x[0].idx, y[0].idx) for x, y in zip(a, b))                     # the same index order with and without
        assert all(x[0].flip is None and y[0].flip is not None and y[0].flip.dtype == torch.uint8 for x, y in zip(a, b))
        for img, lab in b:
            t = img.materialize()
            assert t.shape == (img.size(0), 3, 64, 64)
            px = lambda col: ((t[:, 0, 0, col] * 0.5 + 0.5) * 255).round().long()
            flipped = px(0) == 200
            assert torch.equal(flipped, img.flip.bool())
            ids = torch.where(flipped, px(63), px(0))
            assert torch.equal(ids, img.idx) and torch.equal(lab.argmax(1), ids % 100)        # labels stay with their images
        epochs.append((torch.cat([x[0].idx for x in b]).cpu(), torch.cat([x[0].flip for x in b]).cpu()))
    (i0, f0), (i1, f1) = epochs
    assert sorted(i0.tolist()) == list(range(n)) and 0 < int(f0.sum()) < n
    order0, order1 = torch.argsort(i0), torch.argsort(i1)
    assert not torch.equal(f0[order0], f1[order1])                                            # an image's flip differs between epochs


def _fresh_logger():
    from logger.main_logger import MainLogger
    logging.getLogger("main").handlers.clear()
    MainLogger._instance, MainLogger._initialized = None, False


def test_trainer_runs_from_a_data_file(tmp_path, monkeypatch):
    """main.py's wiring on 40 images of 48x48 with --mirror 1: two identical runs, a checkpoint, and a real-feature cache of its own"""
    import main
    import metrics
    from model import DCGAN
    from preprocess.dcgan_data_preprocessor import DCGANDataPreprocessor
    from train.dcgan_trainer import DCGANTrainer
    monkeypatch.chdir(tmp_path)
    rs = np.random.RandomState(4)
    np.savez(tmp_path / "tiles.npz", images=rs.randint(0, 256, size=(40, 48, 48, 3)).astype(np.uint8))
    # a stand-in for the metric network (its weights are not available offline), so that the real-feature cache is written ...
    monkeypatch.setattr(metrics, "default_extractor", lambda device: (lambda x: x.flatten(1)[:, :100].float()))
    made = []
    real_make = DCGANTrainer._make_metrics

    def make_metrics(self, loader):
        made.append(real_make(self, loader))
        return None                                 # ... and no evaluation: the run checkpoints `latest`
    monkeypatch.setattr(DCGANTrainer, "_make_metrics", make_metrics)
    runs = []
    for run in ("a", "b"):
        _fresh_logger()
        torch.manual_seed(12345)
        args = main.get_arg_parse(["-m", "DCGAN", "-b", "16", "-e", "2", "-mlr", "0.0002", "-pm", run, "-lf", "0",
                                   "--data", str(tmp_path / "tiles.npz"), "--mirror", "1"])
        args.save_path = str(tmp_path / "save" / "dcgan" / run)
        pre = DCGANDataPreprocessor(args)
        pre.transform_data()
        tr = DCGANTrainer(args, DCGAN.Generator(), DCGAN.Discriminator(), pre, prec="f32")
        assert tr.train_loader.mirror and tuple(tr.train_loader.data.shape) == (40, 3, 48, 48)
        runs.append(tr.train())
        pts = [f for r, _, fs in os.walk(tmp_path / "save" / "dcgan" / run) for f in fs if f.endswith(".pt")]
        assert pts, "no checkpoint"
    assert len(runs[0][0]) == 6 and runs[0] == runs[1] and all(v == v for v in runs[0][0] + runs[0][1])
    caches = os.listdir(tmp_path / "data")
    assert made[0] is not None and len(caches) == 1 and caches[0].startswith("metric_tiles_") and caches[0] != "metric_data.pikl"
    _fresh_logger()
