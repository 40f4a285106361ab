"""The nearest-neighbour index kernels (csrc/knnindex.hip) and the layers above them, on the GPU.  On integer-valued data every norm,
dot product and difference sum is exact in fp32, so idx and d2 must EQUAL a stable int64 sort by (d2, idx); on real-valued data
the indices of decidable queries must be the fp64 reference's and every distance within (D + 4) 2^-24 relative of the fp64 distance
of the pair it names.  The reference arithmetic is tests/neighbours_ref.py.  The tile is 64 x 64: sizes 63 / 64 / 65 / 129 straddle
it."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from neighbours_ref import decidable, knn_ref, merge_ref, pair_d2
from pairstats_ref import EPS32, int_features, recipe

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "jck-generation_amd")
SENT_I, SENT_D = -77, -5.0


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


def strips_of(m, n):
    """strips of reference tiles the candidate walk of an m x n call is split into, from the workspace size:
    4 * m * (1 + 16 * strips) bytes (query norms, then 8 distances and 8 indices per query and strip)"""
    from hipgan._lib import load_library
    nbytes = load_library().jck_knn_index_ws_bytes(m, n)
    assert nbytes > 0 and nbytes % (4 * m) == 0 and (nbytes // (4 * m) - 1) % 16 == 0
    return (nbytes // (4 * m) - 1) // 16


def knn_into(q, ref, k, idx, d2, q_base=0, ref_base=0, exclude_self=False, merge=False):
    from hipgan._lib import cur_stream, lib, load_library
    ws = torch.empty(load_library().jck_knn_index_ws_bytes(q.shape[0], ref.shape[0]) // 4, dtype=torch.float32, device="cuda")
    lib.jck_knn_index_f32(q, q.shape[0], ref, ref.shape[0], q.shape[1], k, q_base, ref_base, int(exclude_self), int(merge), idx, d2, ws, cur_stream())


def knn(q, ref, k, **kw):
    idx = torch.full((q.shape[0], k), SENT_I, dtype=torch.int64, device="cuda")
    d2 = torch.full((q.shape[0], k), SENT_D, dtype=torch.float32, device="cuda")
    knn_into(q, ref, k, idx, d2, **kw)
    return idx.cpu().numpy(), d2.cpu().numpy()


def same(got, want):
    """bit-exact: indices equal, distances equal as numbers (the reference is fp64 of exactly representable values), NaN where NaN"""
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1].astype(np.float64), want[1], equal_nan=True)


SIZES = (1, 63, 64, 65, 129, 333)


@pytest.mark.parametrize("D,offset", [(5, False), (20, False), (64, False), (64, True)])
def test_index_is_bit_exact_on_integer_features_at_every_tile_edge(D, offset):
    """M and N over the tile edges, scalar (D = 5, or a base off a 16-byte boundary) and vector staging, k = 1, 3, 8.  Entries in
    -3..3 give many equal distances at small D: the lower index must win."""
    qh, rh = int_features(333, D, seed=11), int_features(333, D, seed=12)
    rh[7] = qh[2]                                             # an exact copy: distance 0
    up = dev_offset if offset else dev
    qd, rd = up(qh), up(rh)
    for n in SIZES:
        want8 = knn_ref(qh, rh[:n], 8)                        # prefixes of the k = 8 answer are the answers for smaller k
        for m in SIZES:
            for k in (1, 3, 8):
                got = knn(qd[:m], rd[:n], k)
                assert same(got, (want8[0][:m, :k], want8[1][:m, :k])), (m, n, D, k)


def test_ties_go_to_the_lowest_indices_across_the_candidate_cut():
    """333 references drawn from 4 patterns: every query has at most 4 distinct distances, each shared by about 80 rows, so the 8
    kept are the 8 LOWEST indices of the nearest pattern(s), whichever lane, wave, strip or chunk met them"""
    g = np.random.default_rng(21)
    pats = g.integers(-3, 4, size=(4, 20)).astype(np.float32)
    ref = pats[g.integers(0, 4, size=333)]
    q = np.concatenate([pats, int_features(61, 20, seed=22)])
    rd, qd = dev(ref), dev(q)
    for k in (1, 3, 8):
        want = knn_ref(q, ref, k)
        assert same(knn(qd, rd, k), want), k
        if k == 8:
            assert (want[1][:4, 7] == 0).all() and (np.diff(want[0][:4], axis=1) > 0).all()         # 8 exact copies each, ascending index


def test_split_walk_chunks_and_determinism():
    """N = 5000 against M = 65: the walk is split into more than one strip of reference tiles whose lists merge in the second
    launch.  The same references as three chunks (64, 65, the rest) through ref_base / merge give the same arrays; so do two runs."""
    assert strips_of(65, 5000) > 1
    q, ref = int_features(65, 16, seed=31), int_features(5000, 16, seed=32)
    qd, rd = dev(q), dev(ref)
    for k in (3, 8):
        want = knn_ref(q, ref, k)
        got = knn(qd, rd, k)
        assert same(got, want), k
        again = knn(qd, rd, k)
        assert got[0].tobytes() == again[0].tobytes() and got[1].tobytes() == again[1].tobytes()
        idx = torch.full((65, k), SENT_I, dtype=torch.int64, device="cuda")
        d2 = torch.full((65, k), SENT_D, dtype=torch.float32, device="cuda")
        for lo, hi in ((0, 64), (64, 129), (129, 5000)):
            knn_into(qd, rd[lo:hi], k, idx, d2, ref_base=lo, merge=lo > 0)
        assert idx.cpu().numpy().tobytes() == got[0].tobytes() and d2.cpu().numpy().tobytes() == got[1].tobytes(), k
    # chunks that each hold fewer than k rows: padding entries merge as padding
    small = knn(qd, rd[:5], 8)
    idx = torch.full((65, 8), SENT_I, dtype=torch.int64, device="cuda")
    d2 = torch.full((65, 8), SENT_D, dtype=torch.float32, device="cuda")
    for lo, hi in ((0, 2), (2, 3), (3, 5)):
        knn_into(qd, rd[lo:hi], 8, idx, d2, ref_base=lo, merge=lo > 0)
    assert same((idx.cpu().numpy(), d2.cpu().numpy()), knn_ref(q, ref[:5], 8)) and same(small, knn_ref(q, ref[:5], 8))
    assert same(merge_ref([knn_ref(q, ref[:64], 3), knn_ref(q, ref[64:], 3, ref_base=64)], 3), knn_ref(q, ref, 3))      # the reference's own merge


def test_exclude_self_is_by_global_index():
    ref = int_features(333, 64, seed=41)
    ref[200] = ref[120]                                       # a duplicate at another index stays a neighbour at distance 0
    q = ref[100:165]
    for k in (1, 8):
        want = knn_ref(q, ref, k, q_base=100, exclude_self=True)
        got = knn(dev(q), dev(ref), k, q_base=100, exclude_self=True)
        assert same(got, want), k
        assert not (got[0] == 100 + np.arange(65)[:, None]).any()
        assert got[0][20, 0] == 200 and got[1][20, 0] == 0.0
    assert same(knn(dev(q), dev(ref), 1, q_base=100), (np.arange(100, 165, dtype=np.int64)[:, None], np.zeros((65, 1))))       # without: itself
    # chunked, the excluded pair lies in the second chunk for some queries and in none for the others
    idx = torch.full((65, 8), SENT_I, dtype=torch.int64, device="cuda")
    d2 = torch.full((65, 8), SENT_D, dtype=torch.float32, device="cuda")
    for lo, hi in ((0, 130), (130, 333)):
        knn_into(dev(q), dev(ref[lo:hi]), 8, idx, d2, q_base=100, ref_base=lo, exclude_self=True, merge=lo > 0)
    assert same((idx.cpu().numpy(), d2.cpu().numpy()), knn_ref(q, ref, 8, q_base=100, exclude_self=True))


def test_edges_and_bad_arguments():
    from hipgan._lib import JckError
    q, ref = int_features(65, 20, seed=51), int_features(129, 20, seed=52)
    got = knn(dev(q), dev(ref[:3]), 8)                         # fewer than k references: a -1 / +inf tail
    assert same(got, knn_ref(q, ref[:3], 8)) and (got[0][:, 3:] == -1).all() and np.isposinf(got[1][:, 3:]).all() and (got[0][:, :3] >= 0).all()
    got = knn(dev(q[:1]), dev(q[:1]), 8, exclude_self=True)    # N = 1 and that one excluded
    assert (got[0] == -1).all() and np.isposinf(got[1]).all()
    for bad in (np.nan, np.inf):
        qb = q.copy()
        qb[5, 3] = bad
        got = knn(dev(qb), dev(ref), 3)
        want = knn_ref(q, ref, 3)
        assert (got[0][5] == -1).all() and np.isnan(got[1][5]).all()
        assert same((np.delete(got[0], 5, 0), np.delete(got[1], 5, 0)), (np.delete(want[0], 5, 0), np.delete(want[1], 5, 0)))
        rb = ref.copy()
        rb[want[0][0, 0], 7] = bad                             # query 0's nearest reference row: never returned now
        got = knn(dev(q), dev(rb), 8)
        assert not (got[0] == want[0][0, 0]).any() and same(got, knn_ref(q, rb, 8))
    qd, rd = dev(q), dev(ref)
    ws = torch.empty(strips_of(65, 129) * 16 * 65 + 65, dtype=torch.float32, device="cuda")
    from hipgan._lib import cur_stream, lib, load_library
    assert load_library().jck_knn_index_ws_bytes(0, 5) == 0 and load_library().jck_knn_index_ws_bytes(5, -1) == 0
    idx = torch.full((65, 8), SENT_I, dtype=torch.int64, device="cuda")
    d2 = torch.full((65, 8), SENT_D, dtype=torch.float32, device="cuda")
    for args in ((qd, 65, rd, 129, 20, 0), (qd, 65, rd, 129, 20, 9), (qd, 0, rd, 129, 20, 3), (qd, 65, rd, 0, 20, 3), (qd, 65, rd, 129, 0, 3),
                 (None, 65, rd, 129, 20, 3), (qd, 65, None, 129, 20, 3), (qd, (1 << 30) + 1, rd, 129, 20, 3)):
        with pytest.raises(JckError):
            lib.jck_knn_index_f32(*args, 0, 0, 0, 0, idx, d2, ws, cur_stream())
    for out in ((None, d2, ws), (idx, None, ws), (idx, d2, None)):
        with pytest.raises(JckError):
            lib.jck_knn_index_f32(qd, 65, rd, 129, 20, 3, 0, 0, 0, 0, *out, cur_stream())
    torch.cuda.synchronize()
    assert (idx == SENT_I).all() and (d2 == SENT_D).all()      # refused before any launch


@pytest.mark.parametrize("D", [5, 20, 100, 128])
def test_real_valued_features_match_fp64_where_decidable(D):
    """fake -> real and real -> real without itself.  Decidable queries (neighbours_ref.decidable: gaps above twice the fp32 error
    bounds of the two stages) must return exactly the reference's indices; EVERY returned distance is within (D + 4) 2^-24
    relative of the fp64 distance of the pair it names, and every row ascends."""
    real, fake = recipe(D)
    for name, q, excl in (("fake->real", fake, False), ("real->real", real, True)):
        sure = decidable(q, real, exclude_self=excl)
        share = 1.0 - sure.mean()
        print(f"D={D} {name}: undecidable {share:.4f}")
        assert share <= 0.05
        want = knn_ref(q, real, 8, exclude_self=excl)
        got = knn(dev(q), dev(real), 8, exclude_self=excl)
        assert np.array_equal(got[0][sure], want[0][sure])
        assert (got[0] >= 0).all()
        exact = pair_d2(q, real, got[0])
        rel = np.abs(got[1].astype(np.float64) - exact) / exact
        print(f"D={D} {name}: worst relative distance error {rel.max():.3e}, bound {(D + 4) * EPS32:.3e}")
        assert (np.abs(got[1].astype(np.float64) - exact) <= (D + 4) * EPS32 * exact).all()
        assert (np.diff(got[1], axis=1) >= 0).all()
        ties = np.diff(got[1], axis=1) == 0
        assert (np.diff(got[0], axis=1)[ties] > 0).all()
        k3 = knn(dev(q), dev(real), 3, exclude_self=excl)
        assert np.array_equal(k3[0], got[0][:, :3]) and np.array_equal(k3[1], got[1][:, :3])


def test_near_copies_at_pixel_width_keep_their_digits():
    """300 references uniform on the uint8 grid of [-1, 1], D = 12 288; 40 queries are a reference plus 1e-3 noise (d2 about 1e-2
    beside |a|^2 + |b|^2 of about 8000, where a Gram-only distance has no correct digit), 25 are fresh draws.  The planted queries
    find their reference with d2 within the bound of fp64.  The copy flag (d2 to the nearest reference below that reference's
    leave-one-out nearest-neighbour distance, from one exclude_self call) is set for every planted query and agrees with fp64 for
    every query whose two distances differ by more than their fp32 bounds.  It is NOT false for every fresh draw: an independent draw
    from the references' own distribution is closer to its nearest reference than that reference's nearest neighbour about every
    other time by symmetry (4 of these 25 in fp64), which is what the flag says and not a copy; only the planted queries sit orders
    of magnitude below, and that is asserted."""
    from neighbours_ref import gram_d2
    g = np.random.default_rng(61)
    D = 12288
    ref = (g.integers(0, 256, size=(300, D)).astype(np.float32) / np.float32(127.5) - np.float32(1)).astype(np.float32)
    p = g.permutation(300)[:40]
    q = np.concatenate([ref[p] + np.float32(1e-3) * g.standard_normal((40, D)).astype(np.float32),
                        g.integers(0, 256, size=(25, D)).astype(np.float32) / np.float32(127.5) - np.float32(1)]).astype(np.float32)
    rd = dev(ref)
    idx, d2 = knn(dev(q), rd, 4)
    bound = (D + 4) * EPS32
    assert np.array_equal(idx[:40, 0], p)
    exact = pair_d2(q, ref, idx)
    assert (np.abs(d2.astype(np.float64) - exact) <= bound * exact).all()
    assert (0.005 < d2[:40, 0]).all() and (d2[:40, 0] < 0.02).all() and (d2[:40, 1] > 7000).all()
    assert (np.diff(d2, axis=1) >= 0).all()
    all_d2 = gram_d2(q, ref)                                     # the fresh draws' nearest references, where the gap decides
    s = np.sort(all_d2, axis=1)
    sure = (s[:, 1] - s[:, 0]) > 2 * 3 * (D + 2) * EPS32 * ((q.astype(np.float64) ** 2).sum(1) + (ref.astype(np.float64) ** 2).sum(1).max())
    assert sure[:40].all() and np.array_equal(idx[sure, 0], all_d2.argmin(1)[sure])
    # the flag
    nn_idx, nn_d2 = knn(rd, rd, 1, exclude_self=True)
    copy = d2[:, 0] < nn_d2[idx[:, 0], 0]
    rr = gram_d2(ref, ref)
    rr[np.arange(300), np.arange(300)] = np.inf
    loo = rr.min(axis=1)
    assert (np.abs(nn_d2[:, 0].astype(np.float64) - loo) <= bound * loo + 1e-9).all()
    dq, dn = exact[:, 0], loo[idx[:, 0]]
    clear = np.abs(dq - dn) > bound * (dq + dn)
    print(f"near copies: planted d2 {d2[:40, 0].min():.5f}..{d2[:40, 0].max():.5f}, worst relative error {(np.abs(d2 - exact) / exact).max():.3e} "
          f"(bound {bound:.3e}); fresh draws flagged {int(copy[40:].sum())} of 25, comparable {int(clear.sum())} of 65")
    assert copy[:40].all() and clear[:40].all()
    assert np.array_equal(copy[clear], (dq < dn)[clear])


def test_metrics_nearest_device_path_matches_the_numpy_path():
    import metrics
    ref, q = int_features(333, 64, seed=71), int_features(131, 64, seed=72)
    ref[40] = q[3]
    want = metrics.nearest(q, ref, 5)
    assert np.array_equal(want[0], knn_ref(q, ref, 5)[0])
    for chunk in (None, 100, 64, 1000):
        idx, d2 = metrics.nearest(dev(q), ref, 5, chunk=chunk)             # one CUDA argument is enough
        assert idx.is_cuda and idx.dtype == torch.int64 and d2.dtype == torch.float32 and idx.shape == (131, 5)
        assert np.array_equal(idx.cpu().numpy(), want[0]) and np.array_equal(d2.cpu().numpy().astype(np.float64), want[1]), chunk
    wx = metrics.nearest(ref, ref, 8, exclude_self=True)
    for chunk in (None, 129):
        idx, d2 = metrics.nearest(dev(ref), dev(ref), 8, exclude_self=True, chunk=chunk)
        assert np.array_equal(idx.cpu().numpy(), wx[0]) and np.array_equal(d2.cpu().numpy().astype(np.float64), wx[1]), chunk
    with pytest.raises(ValueError):
        metrics.nearest(dev(q), ref, 0)


class TinyExtractor:
    """a seeded random projection of a 10 x 10 sampling of the 299 x 299 input to 100 features (as in test_pairstats_gpu.py)"""

    def __init__(self):
        self.w = (torch.randn(300, 100, generator=torch.Generator().manual_seed(0)) / 17).cuda()

    def __call__(self, x):
        return x[:, :, ::30, ::30].reshape(x.shape[0], -1).float() @ self.w


def test_metrics_object_finds_the_nearest_real_features():
    import argparse
    import metrics
    g = torch.Generator().manual_seed(5)
    ex = TinyExtractor()
    real_img = torch.randn(300, 3, 299, 299, generator=g)
    real = ex(real_img.cuda()).cpu().numpy()
    m = metrics.Metrics(argparse.Namespace(targets=[i % 100 for i in range(300)]), extractor=ex, real_features=real)
    gen = torch.cat([real_img[[17, 250]], torch.randn(18, 3, 299, 299, generator=g)])       # two real images among the generated ones
    batches = [gen[:12], gen[12:]]
    idx, d2 = m.nearest_real(batches, k=3)
    assert idx.is_cuda and idx.shape == (20, 3) and d2.shape == (20, 3)
    feats = m._extract(batches, keep_on_device=True)
    widx, wd2 = metrics.nearest(feats, real, 3)
    assert torch.equal(idx, widx) and torch.equal(d2, wd2)
    # the two real images: their features were made in another batch shape, so equal up to the extractor's own rounding
    assert idx[:2, 0].tolist() == [17, 250] and float(d2[:2, 0].max()) < 1e-6 and float(d2[:2, 1].min()) > 1.0
    hidx, hd2 = metrics.nearest(feats.cpu().numpy(), real, 3)              # the numpy path on the same features
    sure = decidable(feats.cpu().numpy(), real)
    sure[:2] = False                                                       # (a distance of rounding size has no relative accuracy)
    assert sure.sum() >= 10 and np.array_equal(idx.cpu().numpy()[sure], hidx[sure])
    assert np.allclose(d2.cpu().numpy()[sure], hd2[sure], rtol=104 * EPS32, atol=0)


def test_nearest_images_in_pixel_space():
    from hipgan.neighbours import nearest_images
    from preprocess.dcgan_data_preprocessor import resize2x_pil_u8
    g = np.random.default_rng(81)
    small = g.integers(0, 256, size=(50, 32, 32, 3), dtype=np.uint8)
    up = resize2x_pil_u8(torch.as_tensor(small).permute(0, 3, 1, 2)).permute(0, 2, 3, 1).contiguous().numpy()
    q = np.concatenate([up[[3, 10]], g.integers(0, 256, size=(5, 64, 64, 3), dtype=np.uint8)])
    q[1, 5, 5, 0] ^= 0x80                                                    # one channel of one pixel off by 128
    a = nearest_images(q, up, k=3)
    assert set(a) == {"idx", "d2", "rmse", "ref_nn_d2", "copy"}
    assert a["idx"].dtype == np.int64 and a["idx"].shape == (7, 3) and a["d2"].dtype == np.float32 and a["copy"].dtype == np.bool_
    assert a["idx"][:2, 0].tolist() == [3, 10] and a["d2"][0, 0] == 0.0
    assert abs(a["d2"][1, 0] - (128 / 127.5) ** 2) <= 1e-6 and a["copy"][:2].all()
    assert np.array_equal(a["rmse"], np.sqrt(a["d2"] / 12288))
    want = knn_ref(q.reshape(7, -1) / 127.5 - 1, up.reshape(50, -1) / 127.5 - 1, 3)
    assert np.allclose(a["d2"], want[1], rtol=1e-4, atol=1e-6)              # the distances of the true neighbours, rank by rank ...
    assert np.allclose(a["d2"], pair_d2(q.reshape(7, -1) / 127.5 - 1, up.reshape(50, -1) / 127.5 - 1, a["idx"]), rtol=1e-4, atol=1e-6)      # ... and of the images named
    loo = knn_ref(up.reshape(50, -1) / 127.5 - 1, up.reshape(50, -1) / 127.5 - 1, 1, exclude_self=True)[1][:, 0]
    assert np.allclose(a["ref_nn_d2"], loo[a["idx"][:, 0]], rtol=1e-4)
    assert np.array_equal(a["copy"], a["d2"][:, 0] < a["ref_nn_d2"])
    for other in (nearest_images(q, small, k=3), nearest_images(torch.as_tensor(q), torch.as_tensor(up), k=3, chunk=16)):
        assert all(np.array_equal(a[key], other[key]) for key in a)          # the 32 x 32 set through the exact upscale; chunks
    dup = up.copy()
    dup[40] = dup[3]                                                         # the matched image has a twin: its nearest other image is at 0
    b = nearest_images(q[:1], dup, k=2)
    assert b["idx"][0].tolist() == [3, 40] and b["ref_nn_d2"][0] == 0.0 and not b["copy"][0]
    assert set(nearest_images(q, up, k=1, flag=False)) == {"idx", "d2", "rmse"}
    from hipgan._lib import JckError
    for bad_q, bad_r in ((q.astype(np.float32), up), (q, up[:, :48, :48]), (q, up[..., :2]), (q[:, :32, :32], up)):
        with pytest.raises(JckError):
            nearest_images(bad_q, bad_r)


def test_generate_cli_neighbours(tmp_path):
    """a tiny seeded checkpoint; the reference file holds three of the run's own outputs among random pictures: they come back at
    distance 0 and flagged"""
    from hipgan.engine import DcganEngine
    from hipgan.sampler import Sampler, latents
    from oracle.gan_oracle import GanOracle
    orc = GanOracle("dcgan", lr=2e-4, seed=12345)
    eng = DcganEngine(batch=8, prec="bf16")
    eng.load_state(orc.g, orc.d)
    gen = torch.Generator().manual_seed(9)
    for _ in range(30):          # running statistics that belong to the weights
        eng.sample(torch.randn(8, 100, generator=gen))
    gs, ds = eng.state_dicts()
    ckpt = str(tmp_path / "plain.pt")
    torch.save({"model_g": gs, "model_d": ds}, ckpt)
    own = Sampler.from_checkpoint(ckpt, "DCGAN", batch=8).from_latents(latents(6, 3)).cpu().numpy()
    rnd = np.random.default_rng(91).integers(0, 256, size=(10, 64, 64, 3), dtype=np.uint8)
    ref = np.concatenate([rnd[:4], own[[0, 2, 4]], rnd[4:]])
    np.savez(str(tmp_path / "train.npz"), images=ref)
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, "generate.py", "-m", "DCGAN", "--checkpoint", ckpt, "--num", "6", "-b", "8", "--seed", "3", "--out", str(out),
                        "--neighbours", str(tmp_path / "train.npz"), "--k", "2"], cwd=PKG, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(np.load(str(out / "images.npz"))["images"], own)
    f = np.load(str(out / "neighbours.npz"))
    assert sorted(f.files) == ["copy", "d2", "idx", "ref_nn_d2", "rmse"]
    assert f["idx"].shape == (6, 2) and f["idx"].dtype == np.int64 and f["copy"].dtype == np.bool_ and f["copy"].shape == (6,)
    assert f["idx"][[0, 2, 4], 0].tolist() == [4, 5, 6] and (f["d2"][[0, 2, 4], 0] == 0).all() and (f["rmse"][[0, 2, 4], 0] == 0).all()
    assert f["copy"][[0, 2, 4]].all() and (f["ref_nn_d2"][[0, 2, 4]] > 0).all()
    png = open(str(out / "neighbours.png"), "rb").read()
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    w, h = int.from_bytes(png[16:20], "big"), int.from_bytes(png[20:24], "big")
    assert (w, h) == (3 * 66 + 2, 6 * 66 + 2)                                # 1 + k pictures a row, a row per sample, padding 2
    line = [l for l in r.stdout.splitlines() if l.startswith("neighbours: ")]
    assert len(line) == 1 and f"{int(f['copy'].sum())} of 6 samples flagged" in line[0] and "min 0.00000" in line[0]
