"""The sliced-Wasserstein kernels (csrc/swd.hip) and the layers above them, on the GPU.  The reference is tests/swd_ref.py (fp64).

Shapes are the smallest at which each kernel can go wrong: S = 32 / 64 / 128 are the three LDS size classes with 2 / 3 / 4 levels, n = 3
pictures and P = 5 patches whose first four corners are the four extreme ones (every mirror border), D = 147 (two direction tiles, the
second ragged), 5 and 128; the sort's sizes straddle 64, the tile T and several merge passes (3T + 5: two passes with a ragged last run,
8T + 1: four passes, the last merging a run of one key).

Bounds.  Descriptors: the kernel keeps the pyramid in fixed point and rounds every Laplacian value once, so EVERY level is the fp64
reference rounded to fp32, bit for bit (csrc/swd.hip's header); the weaker statement of an fp32 separable pyramid - level 0 and the coarsest exact, the middle
ones within 2^-13 - is asserted beside it.  Statistics: fp64 sums of N = n P 49 fp32 values in any order are within N 2^-53 sum |v| of the
exact sum, asserted at n P 49 2^-52 relative to sum |v| (for the squares: to the sum itself) against the exact sums (math.fsum) of the
reference's fp32-rounded descriptors.  Projections: 150 2^-24 sum_i |(x_i - mean) rstd d_i| + e_l max_c rstd_c sum_i |d_i| per element,
e_l = the largest rounding of a descriptor of that level (0 where 24 bits suffice); the centred value stands where one might write x_i
because the kernel rounds x_i - mean before it scales (53 roundings in all, header).  End to end: swd_ref.device_error_bound."""
import json
import math

import numpy as np
import pytest
import torch

import swd_ref as R

pytestmark = pytest.mark.gpu
SENT = -77.25
N, P = 3, 5


def dev_u8(x, offset=0):
    """the pictures on the device; offset: as a view that starts `offset` bytes into its allocation"""
    x = np.ascontiguousarray(x)
    buf = torch.empty(x.size + offset, dtype=torch.uint8, device="cuda")
    view = buf[offset:].view(x.shape)
    view.copy_(torch.from_numpy(x))
    assert view.data_ptr() % 16 == (buf.data_ptr() + offset) % 16
    return view


def cuda(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype=dtype))).cuda()


def project(x_dev, S, L, pos, dirs, mean, rstd, pad=0):
    """jck_swd_project_u8 into a sentinel-filled [L * D + 1][n P + pad] buffer -> host [L][D][n P]; the guard row and columns are checked"""
    from hipgan._lib import cur_stream, lib
    n, D, Pn = x_dev.shape[0], dirs.shape[0], pos.shape[2]
    ld = n * Pn + pad
    out = torch.full((L * D + 1, ld), SENT, dtype=torch.float32, device="cuda")
    lib.jck_swd_project_u8(x_dev, n, S, L, cuda(pos, np.int32), Pn, cuda(dirs, np.float32), D, cuda(mean, np.float32), cuda(rstd, np.float32), out, ld,
                           cur_stream())
    host = out.cpu().numpy()
    assert (host[L * D] == SENT).all() and (host[:, n * Pn:] == SENT).all()
    return host[:L * D, :n * Pn].reshape(L, D, n * Pn)


def stats(x_dev, S, L, pos):
    from hipgan._lib import cur_stream, lib
    n, Pn = x_dev.shape[0], pos.shape[2]
    part = torch.full((n + 1, L, 3, 2), SENT, dtype=torch.float64, device="cuda")
    s1, s2 = torch.full((L, 3), SENT, dtype=torch.float64, device="cuda"), torch.full((L, 3), SENT, dtype=torch.float64, device="cuda")
    lib.jck_swd_patch_stats_u8(x_dev, n, S, L, cuda(pos, np.int32), Pn, part, s1, s2, cur_stream())
    part = part.cpu().numpy()
    assert (part[n] == SENT).all()
    return s1.cpu().numpy(), s2.cpu().numpy(), part[:n]


@pytest.fixture(scope="module")
def cases():
    """per size two sets of three pictures (random bytes, all 0, all 255 | one-pixel checkerboard, smooth, smooth), their corners and the
    reference descriptors, computed once"""
    out = {}
    for S in (32, 64, 128):
        L = R.levels_of(S)
        eight = R.pictures(8, S, 500 + S)
        sets = [eight[[0, 1, 2]], eight[[3, 4, 5]]]
        pos = R.corners(N, S, L, P, 600 + S)
        desc = [[R.descriptors(lap_l, pos[:, l]) for l, lap_l in enumerate(R.pyramid(x, L)[1])] for x in sets]
        out[S] = {"L": L, "sets": sets, "pos": pos, "desc": desc}
    assert out[64]["L"] == 3 and (out[64]["pos"][:, 2, :4] == [[0, 0], [9, 9], [0, 9], [9, 0]]).all()
    return out


@pytest.mark.parametrize("S", (32, 64, 128))
def test_descriptors_through_the_identity_projection(cases, S):
    c = cases[S]
    L = c["L"]
    eye, zero, one = np.eye(147, dtype=np.float32), np.zeros((L, 3), np.float32), np.ones((L, 3), np.float32)
    worst = np.zeros(L)
    for k, (x, desc) in enumerate(zip(c["sets"], c["desc"])):
        got = project(dev_u8(x, offset=k), S, L, c["pos"], eye, zero, one, pad=k)      # the second set one byte into its allocation
        for l in range(L):
            mine = got[l].reshape(147, N, P).transpose(1, 2, 0)                         # [n][P][147]
            want = desc[l].astype(np.float32)
            worst[l] = max(worst[l], float(np.abs(mine.astype(np.float64) - desc[l]).max()))
            assert np.abs(mine.astype(np.float64) - desc[l]).max() <= (0 if l in (0,) else 2.0 ** -13), (k, l)
            assert mine.tobytes() == want.tobytes(), (k, l)                             # the reference rounded to fp32, at every level
    print(f"S={S}: worst |descriptor - fp64| per level {worst}")
    assert worst[0] == 0 and (L < 4 and worst[L - 1] == 0 or L == 4)                    # 8, 22 and 24 bits are exact; 32 bits (S = 128) are rounded


@pytest.mark.parametrize("S", (32, 64, 128))
def test_patch_statistics(cases, S):
    c = cases[S]
    L, cnt = c["L"], N * P * 49
    for x, desc in zip(c["sets"], c["desc"]):
        xd = dev_u8(x)
        s1, s2, part = stats(xd, S, L, c["pos"])
        again = stats(xd, S, L, c["pos"])
        assert s1.tobytes() == again[0].tobytes() and s2.tobytes() == again[1].tobytes() and part.tobytes() == again[2].tobytes()
        for l in range(L):
            v = desc[l].astype(np.float32).astype(np.float64).reshape(N, P, 3, 49)
            for ch in range(3):
                flat = v[:, :, ch].reshape(-1)
                want, want_sq, mag = math.fsum(flat), math.fsum(flat * flat), math.fsum(np.abs(flat))
                assert abs(s1[l, ch] - want) <= cnt * 2.0 ** -52 * mag and abs(s2[l, ch] - want_sq) <= cnt * 2.0 ** -52 * want_sq, (l, ch)
                for i in range(N):
                    assert abs(part[i, l, ch, 0] - math.fsum(v[i, :, ch].reshape(-1))) <= cnt * 2.0 ** -52 * mag
            if l == 0:                                                                   # multiples of 2^-14 below 2^18: exact in any order
                assert np.array_equal(s1[l], v.sum(axis=(0, 1, 3)))
            _, _, mean, rstd = R.stats(desc[l])
            from hipgan.swd import moments_from_sums
            m, r = moments_from_sums(s1[l], s2[l], cnt)
            assert np.abs(m - mean).max() <= 1e-6 * (1 + np.abs(mean).max()) and np.abs(r - rstd).max() <= 1e-5 * rstd.max()
            assert (r[rstd == 0] == 0).all()
    bad = c["pos"].copy()
    bad[1, L - 1, 2] = (0, (S >> (L - 1)) - 6)
    s1, s2, part = stats(dev_u8(c["sets"][0]), S, L, bad)
    good = stats(dev_u8(c["sets"][0]), S, L, c["pos"])[2]
    assert np.isnan(part[1]).all() and np.isnan(s1).all() and np.isnan(s2).all() and part[[0, 2]].tobytes() == good[[0, 2]].tobytes()


@pytest.mark.parametrize("S", (32, 64, 128))
def test_projection_within_the_bound_of_every_element(cases, S):
    c = cases[S]
    L = c["L"]
    worst = 0.0
    for D in (5, 128):
        dirs = R.unit_dirs(1, D, 700 + D)[0]
        ad = np.abs(dirs.astype(np.float64))
        for x, desc in zip(c["sets"], c["desc"]):
            mean = np.stack([R.stats(d)[2] for d in desc]).astype(np.float32)
            rstd = np.stack([R.stats(d)[3] for d in desc]).astype(np.float32)
            xd = dev_u8(x)
            got = project(xd, S, L, c["pos"], dirs, mean, rstd)
            assert got.tobytes() == project(xd, S, L, c["pos"], dirs, mean, rstd, pad=2).tobytes()              # two calls, another row length
            for l in range(L):
                xn = R.normalise(desc[l], mean[l].astype(np.float64), rstd[l].astype(np.float64))
                want = R.project(xn, dirs)
                e_l = float(np.abs(desc[l].astype(np.float32).astype(np.float64) - desc[l]).max())
                bound = 150 * 2.0 ** -24 * np.einsum("ipk,dk->dip", np.abs(xn), ad).reshape(D, -1) + e_l * float(rstd[l].max()) * ad.sum(axis=1)[:, None]
                err = np.abs(got[l].astype(np.float64) - want)
                assert (err <= bound).all(), (D, l, float((err - bound).max()))
                worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    print(f"S={S}: worst error / bound {worst:.3f}")
    # a corner out of range: NaN for that picture's P entries of every row, the other pictures as before
    dirs = R.unit_dirs(1, 5, 705)[0]
    mean, rstd = np.zeros((L, 3), np.float32), np.ones((L, 3), np.float32)
    good = project(dev_u8(c["sets"][0]), S, L, c["pos"], dirs, mean, rstd)
    for where, corner in (((1, 0, 4), (S - 6, 0)), ((1, L - 1, 0), (-1, 3))):
        bad = c["pos"].copy()
        bad[where] = corner
        got = project(dev_u8(c["sets"][0]), S, L, bad, dirs, mean, rstd).reshape(L, 5, N, P)
        assert np.isnan(got[:, :, 1]).all() and got[:, :, [0, 2]].tobytes() == good.reshape(L, 5, N, P)[:, :, [0, 2]].tobytes()


def sort_sizes():
    from hipgan._lib import load_library
    T = load_library().jck_sort_rows_tile()
    return T, (1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5, 8 * T + 1)


def contents(kind, rows, M, g):
    if kind == "normal":
        x = g.standard_normal((rows, M))
    elif kind == "ascending":
        x = np.sort(g.standard_normal((rows, M)), axis=1)
    elif kind == "descending":
        x = -np.sort(g.standard_normal((rows, M)), axis=1)
    elif kind == "equal":
        x = np.repeat(g.standard_normal((rows, 1)), M, axis=1)
    elif kind == "duplicates":
        x = g.standard_normal(8)[g.integers(0, 8, size=(rows, M))]
    else:
        fmax, tiny = np.finfo(np.float32).max, np.float32(1e-45)
        special = np.array([0.0, -0.0, np.inf, -np.inf, tiny, -tiny, 3 * tiny, np.float32(1e-39), -np.float32(1e-39), fmax, -fmax, 1.0, -1.0], dtype=np.float32)
        x = np.where(g.random((rows, M)) < 0.7, special[g.integers(0, special.shape[0], size=(rows, M))], g.standard_normal((rows, M)).astype(np.float32))
    return np.ascontiguousarray(x, dtype=np.float32)


def sort_rows(x, in_place=False):
    """jck_sort_rows_f32 of host rows [Rows][M] with 64 guard floats behind the last row of the input and of the output -> host rows"""
    from hipgan._lib import cur_stream, lib, load_library
    rows, M = x.shape
    src = torch.full((rows * M + 64,), SENT, dtype=torch.float32, device="cuda")
    src[:rows * M] = torch.from_numpy(x.reshape(-1))
    dst = src if in_place else torch.full((rows * M + 64,), SENT, dtype=torch.float32, device="cuda")
    nbytes = load_library().jck_sort_rows_ws_bytes(rows, M)
    ws = torch.full((nbytes // 4 + 64,), SENT, dtype=torch.float32, device="cuda")
    lib.jck_sort_rows_f32(src, rows, M, dst, ws, nbytes, cur_stream())
    out = dst.cpu().numpy()
    assert (out[rows * M:] == SENT).all() and (ws.cpu().numpy()[nbytes // 4:] == SENT).all()
    if not in_place:
        assert src.cpu().numpy()[:rows * M].tobytes() == x.tobytes()                # the input is only read
    return out[:rows * M].reshape(rows, M)


@pytest.mark.parametrize("kind", ("normal", "ascending", "descending", "equal", "duplicates", "special"))
def test_row_sort(kind):
    T, sizes = sort_sizes()
    g = np.random.default_rng(len(kind))
    for M in sizes:
        for rows in (1, 3):
            x = contents(kind, rows, M, g)
            for in_place in ((False, True) if M in (65, 3 * T + 5, 8 * T + 1) else (False,)):
                got = sort_rows(x, in_place)
                for r in range(rows):
                    assert np.array_equal(got[r], np.sort(x[r])), (M, rows, r, in_place)                    # as values
                    assert np.array_equal(np.sort(got[r].view(np.uint32)), np.sort(x[r].view(np.uint32)))   # the multiset of bit patterns
                    zeros = got[r].view(np.uint32)[got[r] == 0]
                    assert (np.diff((zeros == 0).astype(np.int8)) >= 0).all()                               # every -0 before every +0


def test_row_sort_honours_the_workspace_query():
    from hipgan._lib import JckError, cur_stream, lib, load_library
    T, _ = sort_sizes()
    x = torch.zeros(3 * (T + 1), dtype=torch.float32, device="cuda")
    need = load_library().jck_sort_rows_ws_bytes(3, T + 1)
    assert need == 3 * (T + 1) * 4 and load_library().jck_sort_rows_ws_bytes(3, T) == 0
    ws = torch.zeros(need // 4, dtype=torch.float32, device="cuda")
    with pytest.raises(JckError):
        lib.jck_sort_rows_f32(x, 3, T + 1, x, ws, need - 1, cur_stream())
    with pytest.raises(JckError):
        lib.jck_sort_rows_f32(x, 3, T + 1, x, None, need, cur_stream())
    lib.jck_sort_rows_f32(x, 3, T, x, None, 0, cur_stream())                       # one tile a row: no workspace
    lib.jck_sort_rows_f32(x, 3, T + 1, x, ws, need, cur_stream())
    assert (x == 0).all()


def test_row_distance():
    from hipgan._lib import cur_stream, lib
    T, sizes = sort_sizes()
    g = np.random.default_rng(77)
    for M in sizes:
        a, b = sort_rows(contents("normal", 3, M, g)), sort_rows((3 * contents("normal", 3, M, g) + 1).astype(np.float32))
        w = torch.full((4,), SENT, dtype=torch.float64, device="cuda")
        lib.jck_swd_rows(cuda(a), cuda(b), 3, M, w, cur_stream())
        w = w.cpu().numpy()
        assert w[3] == SENT
        for r in range(3):
            want = math.fsum(np.abs(a[r].astype(np.float64) - b[r].astype(np.float64))) / M
            assert abs(w[r] - want) <= M * 2.0 ** -53 * want, (M, r)
        lib.jck_swd_rows(cuda(a), cuda(a), 3, M, (w2 := torch.full((3,), SENT, dtype=torch.float64, device="cuda")), cur_stream())
        assert (w2.cpu().numpy() == 0).all()


def test_metrics_swd_on_the_device_against_the_numpy_path():
    import metrics
    from hipgan import swd as H
    kw = dict(patches=16, dirs=8, repeats=2, seed=4)
    for n, chunk in ((6, None), (7, 4)):                                            # 7 pictures in chunks of 4: rows written at the chunk's offset
        a, b = R.pictures(n, 64, 31), R.pictures(n + 4, 64, 32)[4:][::-1].copy()
        a[1:4] = R.pictures(8, 64, 33)[5:8]                                         # (keep the flat pictures out: they are in the kernel tests)
        host = metrics.swd(a, b, **kw)
        tol = 2e3 * R.device_error_bound(a, b, *H.draw(n, 64, 3, 16, 8, 2, 4), 3)
        ad, bd = cuda(a), cuda(b)
        dev = metrics.swd(ad, bd, chunk=chunk, **kw)
        print(f"n={n}: device {dev['swd']}, numpy {host['swd']}, |difference| {np.abs(dev['per_repeat'] - host['per_repeat']).max(axis=0)}, tolerance {tol}")
        assert dev["sides"] == [64, 32, 16] and dev["per_repeat"].shape == (2, 3) and dev["swd"].dtype == np.float64
        assert (np.abs(dev["per_repeat"] - host["per_repeat"]) <= tol[None, :]).all() and (tol < 0.05 * host["swd"]).all()
        assert dev["per_repeat"].tobytes() == metrics.swd(ad, b, chunk=chunk, **kw)["per_repeat"].tobytes()       # a host array beside a device one
        same = metrics.swd(ad, cuda(a), chunk=chunk, **kw)
        assert (same["per_repeat"] == 0).all() and same["mean"] == 0.0 and (metrics.swd(ad, ad, **kw)["swd"] == 0).all()
        assert metrics.swd(bd, ad, chunk=chunk, **kw)["per_repeat"].tobytes() == dev["per_repeat"].tobytes()
        two = metrics.swd(ad, bd, levels=2, **kw)
        assert two["sides"] == [64, 32] and (np.abs(two["per_repeat"] - metrics.swd(a, b, levels=2, **kw)["per_repeat"]) <= tol[None, :2]).all()
    flat = np.full((3, 32, 32, 3), 200, np.uint8)                                   # no deviation: rstd = 0, finite numbers
    r = metrics.swd(cuda(flat), cuda(R.pictures(3, 32, 5)), patches=4, dirs=3, repeats=1)
    assert np.isfinite(r["per_repeat"]).all() and (metrics.swd(cuda(flat), cuda(flat + 1), patches=4, dirs=3, repeats=1)["swd"] == 0).all()


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """a tiny seeded checkpoint (as test_ssim_gpu builds it) and a training file of uniform random pictures"""
    from hipgan.engine import DcganEngine
    from hipgan.sampler import Sampler
    from oracle.gan_oracle import GanOracle
    d = tmp_path_factory.mktemp("swd")
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


def test_sampler_swd_and_the_command_line(trained):
    import metrics
    import swd
    from hipgan._lib import JckError
    from hipgan.sampler import latents
    s, train = trained["sampler"], trained["train"]
    kw = dict(patches=8, dirs=8, repeats=2)
    r = s.swd(train, n=16, seed=3, **kw)
    assert set(r) == {"swd", "mean", "sides", "per_repeat", "n", "n_train", "seed"} and (r["n"], r["n_train"], r["seed"]) == (16, 24, 3)
    assert r["sides"] == [64, 32, 16] and r["per_repeat"].shape == (2, 3) and np.isfinite(r["per_repeat"]).all() and (r["swd"] > 0).all()
    assert np.isfinite(r["mean"]) and r["per_repeat"].tobytes() == s.swd(train, n=16, seed=3, **kw)["per_repeat"].tobytes()
    pick = np.random.default_rng(3).permutation(24)[:16]                            # the definition, written out
    own = metrics.swd(s.from_latents(latents(16, 3)), cuda(train[pick]), seed=3, **kw)
    assert own["per_repeat"].tobytes() == r["per_repeat"].tobytes()
    assert s.swd(train, n=8, levels=1, **kw)["sides"] == [64]
    with pytest.raises(JckError):
        s.swd(train, n=25)
    out = trained["dir"] / "out"
    assert swd.main(["-m", "DCGAN", "--checkpoint", trained["ckpt"], "--train", str(trained["dir"] / "train.npz"), "--num", "16", "--seed", "3", "-b", "8",
                     "--patches", "8", "--dirs", "8", "--repeats", "2", "--out", str(out)]) == 0
    rec = json.load(open(str(out / "swd.json")))
    assert set(rec) == {"swd", "mean", "sides", "levels", "reads_as", "n", "n_train", "seed", "settings"} and rec["n"] == 16 and rec["n_train"] == 24
    assert rec["swd"] == [float(v) for v in r["swd"]] and np.load(str(out / "swd.npz"))["per_repeat"].tobytes() == r["per_repeat"].tobytes()


def test_sampler_swd_per_class_of_a_cgan():
    """classes: one report per class id, from the samples and the training pictures of that class, as many of each as the smaller side"""
    from hipgan.engine import CganEngine
    from hipgan.sampler import Sampler
    from hipgan._lib import JckError
    from oracle.gan_oracle import GanOracle
    orc = GanOracle("cgan", lr=2e-4, seed=12345)
    eng = CganEngine(batch=8, prec="bf16")
    eng.load_state(orc.g, orc.d)
    gs, ds = eng.state_dicts()
    s = Sampler.from_checkpoint({"model_g": gs, "model_d": ds}, "CGAN", batch=8)
    train = np.random.default_rng(92).integers(0, 256, size=(24, 64, 64, 3), dtype=np.uint8)
    train_labels = np.array([3, 17, 42] * 8)
    ids = torch.tensor([3, 17] * 6)                                                 # six samples of each of two classes, eight training pictures
    r = s.swd(train, n=12, seed=1, labels=ids, train_labels=train_labels, classes=[3, 17], patches=4, dirs=4, repeats=1)
    assert set(r) == {"swd", "mean", "sides", "per_repeat", "n", "n_train", "seed", "per_class"} and set(r["per_class"]) == {3, 17}
    for c in (3, 17):
        pc = r["per_class"][c]
        assert pc["n"] == 6 and pc["sides"] == [64, 32, 16] and pc["per_repeat"].shape == (1, 3) and np.isfinite(pc["per_repeat"]).all()
    assert np.isfinite(r["per_repeat"]).all() and r["n"] == 12
    with pytest.raises(JckError):
        s.swd(train, n=12, labels=ids, classes=[3])                                 # no train_labels
    with pytest.raises(JckError):
        s.swd(train, n=12, labels=ids, train_labels=train_labels, classes=[5], patches=4, dirs=4, repeats=1)      # a class nobody has
