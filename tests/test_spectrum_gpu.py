"""The power-spectrum kernel (csrc/spectrum.hip) and the layers above it, on the GPU.  The reference is tests/spectrum_ref.py (fp64, DFT
matrices); the bound is its bound(S), derived in the kernel's header, never measured: with E the sum of the reference's P of a picture,
sum |P^ - P| <= B E over the plane and sum_r count[r] |prof^[r] - prof[r]| <= B E over the bins.

Shapes: S = 32 / 64 / 128 are the three LDS size classes; the n = 7 pictures of spectrum_ref.pictures (random bytes, all 0, all 255, a
one-pixel checkerboard, one bright pixel, a quantised cosine, smooth plus noise), every plane and both windows.  The mean plane is run at
n = 1, G, G + 1 and 2 G + 3 pictures (G workgroups, read from jck_spectrum_grid: one, exactly one each, one wrap, two wraps and a ragged
tail).  Measured worst error / bound (S = 32, 64, 128), printed by test_bounds: DESIGN.md 5.18."""
import numpy as np
import pytest
import torch

import spectrum_ref as R

pytestmark = pytest.mark.gpu
SENT = -77.25
N = 7
PLANES = ("r", "g", "b", "luma")
WINDOWS = (None, "hann")


def dev_u8(x, offset=0):
    """the pictures on the device; offset: as a view that starts `offset` bytes into its allocation"""
    x = np.ascontiguousarray(x)
    buf = torch.empty(x.size + offset, dtype=torch.uint8, device="cuda")
    view = buf[offset:].view(x.shape)
    view.copy_(torch.from_numpy(x))
    assert view.data_ptr() % 16 == (buf.data_ptr() + offset) % 16
    return view


def to_db(profile):
    return 10.0 * np.log10(np.maximum(profile, 1e-6))


def db_tolerance(B, prof, count):
    """[n][R]: -10 log10(1 - ratio) with ratio = B E / (count[r] prof[r]) of the reference profile; inf where the ratio is >= 1.  (The
    clamp at 1e-6 only brings two values closer in the logarithm.)"""
    E = (prof * count).sum(axis=1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(prof > 0, B * E / (count * prof), np.inf)
        return np.where(ratio < 1, -10.0 * np.log10(1.0 - np.where(ratio < 1, ratio, 0.0)), np.inf)


def run(x_dev, plane, window, mean2d=False):
    """jck_spectrum_u8 into sentinel-filled buffers with one guard row each -> (prof [n][R], mean [n], mean2d [S][S] or None); the guards
    behind prof, mean, mean2d and the workspace are checked"""
    from hipgan import spectrum as H
    from hipgan._lib import cur_stream, lib, load_library
    n, S = int(x_dev.shape[0]), int(x_dev.shape[1])
    Rb = load_library().jck_spectrum_bins(S)
    w, W = H.window_table(S, window)
    w_t = None if w is None else torch.from_numpy(w).cuda()
    prof = torch.full((n + 1, Rb), SENT, dtype=torch.float64, device="cuda")
    mean = torch.full((n + 1,), SENT, dtype=torch.float64, device="cuda")
    plane_t = ws = None
    ws_bytes = 0
    if mean2d:
        ws_bytes = load_library().jck_spectrum_ws_bytes(n, S, 1)
        assert ws_bytes % 8 == 0 and ws_bytes > 0
        ws = torch.full((ws_bytes // 8 + S,), SENT, dtype=torch.float64, device="cuda")
        plane_t = torch.full((S + 1, S), SENT, dtype=torch.float64, device="cuda")
    lib.jck_spectrum_u8(x_dev, n, S, H.plane_index(plane), w_t, float(W), prof, mean, plane_t, ws, ws_bytes, cur_stream())
    prof, mean = prof.cpu().numpy(), mean.cpu().numpy()
    assert (prof[n] == SENT).all() and mean[n] == SENT
    out2d = None
    if mean2d:
        out2d = plane_t.cpu().numpy()
        assert (out2d[S] == SENT).all() and (ws.cpu().numpy()[ws_bytes // 8:] == SENT).all()
        out2d = out2d[:S]
    return prof[:n], mean[:n], out2d


@pytest.fixture(scope="module")
def cases():
    """per size the seven pictures and, per plane and window, the reference planes, profiles and energies - computed once"""
    out = {}
    for S in (32, 64, 128):
        x = R.pictures(N, S, 700 + S)
        ref = {}
        for plane in PLANES:
            for window in WINDOWS:
                P, mean = R.power(x, plane, window)
                prof, count = R.profile(P)
                ref[(plane, window)] = {"P": P, "mean": mean, "prof": prof, "E": P.reshape(N, -1).sum(axis=1)}
        out[S] = {"x": x, "dev": dev_u8(x), "ref": ref, "count": count, "B": R.bound(S)}
    return out


@pytest.mark.parametrize("S", (32, 64, 128))
def test_bounds_constants_checkerboard_and_mean(cases, S):
    c = cases[S]
    B, count = c["B"], c["count"].astype(np.float64)
    last = count.shape[0] - 1
    worst = 0.0
    for plane in PLANES:
        Y = R.plane_int(c["x"], plane)
        for window in WINDOWS:
            ref = c["ref"][(plane, window)]
            prof, mean, _ = run(c["dev"], plane, window)
            assert np.array_equal(mean, Y.reshape(N, -1).sum(axis=1) / (256.0 * S * S)) and np.array_equal(mean, ref["mean"])      # T / (256 S^2), exactly
            err = (count[None, :] * np.abs(prof - ref["prof"])).sum(axis=1)
            print(f"S={S} {plane} {window}: profile error / (B E) per picture {np.where(ref['E'] > 0, err / np.maximum(B * ref['E'], 1e-300), 0)}")
            assert (err <= B * ref["E"]).all(), (plane, window)
            worst = max(worst, float(np.max(err[ref["E"] > 0] / (B * ref["E"][ref["E"] > 0]))))
            assert (prof[1] == 0).all() and (prof[2] == 0).all() and mean[1] == 0.0 and mean[2] == 255.0                # constants: exactly 0
            if window is None:                                                # checkerboard: all but B E of the energy in bin R - 1 (a window spreads it)
                energy = prof[3] * count
                assert energy[:last].sum() <= B * ref["E"][3] and abs(energy[last] - ref["E"][3]) <= B * ref["E"][3]
                assert abs(energy[last] - S * S * 127.5 ** 2) <= B * S * S * 127.5 ** 2
            for i in range(N):                                                                                        # the plane, at n = 1
                p1, m1, plane2d = run(c["dev"][i:i + 1], plane, window, mean2d=True)
                e2 = np.abs(plane2d - ref["P"][i]).sum()
                assert e2 <= B * ref["E"][i], (plane, window, i)
                if ref["E"][i] > 0:
                    worst = max(worst, float(e2 / (B * ref["E"][i])))
                assert p1.tobytes() == prof[i:i + 1].tobytes() and m1[0] == mean[i]                                   # alone = inside the batch
                assert np.array_equal(plane2d, np.roll(plane2d[::-1, ::-1], (1, 1), axis=(0, 1)))                     # (u, v) <-> (-u, -v): equal bits
                if i in (1, 2):
                    assert (plane2d == 0).all()
    print(f"S={S}: worst error / bound {worst:.4f}")
    assert worst > 0


@pytest.mark.parametrize("S", (32, 64, 128))
def test_repeatable_independent_unaligned_and_chunked(cases, S):
    import metrics
    c = cases[S]
    for plane, window in (("luma", None), ("b", "hann")):
        prof, mean, plane2d = run(c["dev"], plane, window, mean2d=True)
        again = run(c["dev"], plane, window, mean2d=True)
        assert prof.tobytes() == again[0].tobytes() and mean.tobytes() == again[1].tobytes() and plane2d.tobytes() == again[2].tobytes()
        assert run(c["dev"], plane, window)[0].tobytes() == prof.tobytes()                           # with or without the mean plane
        for off in (1, 2, 3):                                                                        # x at any byte address
            moved = run(dev_u8(c["x"], offset=off), plane, window, mean2d=True)
            assert moved[0].tobytes() == prof.tobytes() and moved[1].tobytes() == mean.tobytes() and moved[2].tobytes() == plane2d.tobytes()
        rev = run(dev_u8(c["x"][::-1]), plane, window)                                               # a row depends on its picture alone
        assert rev[0][::-1].tobytes() == prof.tobytes() and rev[1][::-1].tobytes() == mean.tobytes()
        whole = metrics.spectrum(c["dev"], plane=plane, window=window, mean2d=True)
        parts = metrics.spectrum(c["dev"], plane=plane, window=window, mean2d=True, chunk=4)
        assert whole["profile"].tobytes() == prof.tobytes() and parts["profile"].tobytes() == prof.tobytes() and parts["mean"].tobytes() == mean.tobytes()
        assert whole["mean2d"].tobytes() == plane2d.tobytes()
        Ebar = c["ref"][(plane, window)]["E"].mean()
        assert np.abs(parts["mean2d"] - c["ref"][(plane, window)]["P"].mean(axis=0)).sum() <= c["B"] * Ebar


@pytest.mark.parametrize("S", (32, 64, 128))
def test_mean_plane_over_the_grid(cases, S):
    from hipgan._lib import load_library
    c = cases[S]
    dll = load_library()
    G = dll.jck_spectrum_grid(S)
    assert G >= 1 and dll.jck_spectrum_ws_bytes(10 * G, S, 1) == G * S * (S // 2 + 1) * 8
    plane, window = "luma", "hann"
    ref = c["ref"][(plane, window)]
    for n in (1, G, G + 1, 2 * G + 3):
        idx = (np.arange(n) * 3 + 5) % N                                                             # which of the seven each picture is
        x = dev_u8(c["x"][idx])
        prof, mean, plane2d = run(x, plane, window, mean2d=True)
        weight = np.bincount(idx, minlength=N).astype(np.float64)
        want = np.tensordot(weight, ref["P"], axes=1) / n                                            # the fp64 mean of the per-picture planes
        Ebar = float((weight * ref["E"]).sum() / n)
        assert np.abs(plane2d - want).sum() <= c["B"] * Ebar, n
        assert np.array_equal(plane2d, np.roll(plane2d[::-1, ::-1], (1, 1), axis=(0, 1))), n
        assert run(x, plane, window, mean2d=True)[2].tobytes() == plane2d.tobytes()                  # equal n: equal bits
        first = run(c["dev"], plane, window)[0]
        assert prof.tobytes() == first[idx].tobytes()                                                # rows do not depend on the grid


def test_short_workspace_and_bad_arguments_leave_the_outputs_alone(cases):
    from hipgan import spectrum as H
    from hipgan._lib import JckError, cur_stream, lib, load_library
    S = 64
    x = cases[S]["dev"]
    need = load_library().jck_spectrum_ws_bytes(N, S, 1)
    prof = torch.full((N, 46), SENT, dtype=torch.float64, device="cuda")
    mean = torch.full((N,), SENT, dtype=torch.float64, device="cuda")
    plane2d = torch.full((S, S), SENT, dtype=torch.float64, device="cuda")
    ws = torch.full((need // 8,), SENT, dtype=torch.float64, device="cuda")
    for args in ((x, N, S, 3, None, 1.0, prof, mean, plane2d, ws, need - 1, cur_stream()),
                 (x, N, S, 4, None, 1.0, prof, mean, plane2d, ws, need, cur_stream()),
                 (x, N, S, 3, None, 0.0, prof, mean, plane2d, ws, need, cur_stream()),
                 (x, N, 48, 3, None, 1.0, prof, mean, plane2d, ws, need, cur_stream())):
        with pytest.raises(JckError):
            lib.jck_spectrum_u8(*args)
    torch.cuda.synchronize()
    for t in (prof, mean, plane2d, ws):
        assert (t.cpu().numpy() == SENT).all()
    lib.jck_spectrum_u8(x, 0, S, 3, None, 1.0, prof, mean, plane2d, ws, need, cur_stream())          # n = 0: success, nothing written
    torch.cuda.synchronize()
    assert (prof.cpu().numpy() == SENT).all() and (plane2d.cpu().numpy() == SENT).all()
    assert H.bins(S) == 46


@pytest.mark.parametrize("S", (32, 64, 128))
def test_metrics_device_path_against_the_numpy_path(cases, S):
    """End to end: profiles through the bound, dB values and the report's gap_db within the bound's dB equivalent per bin.

    A picture's bin is within B E of count[r] prof[r], so with ratio = B E / (count[r] prof[r]) < 1 its dB value moves by at most
    -10 log10(1 - ratio), and a set's mean_db (hence gap_db) by at most the mean of that over its pictures.  The ratio is a property of
    the reference and of B alone.  Evaluated on the CPU for this file's pictures it exceeds 1e-3 in 3 to 51 bins of even the white
    pictures (it is about B S^2 / count[r] there, and the first bins have as few points as the last ones; bin 0 of a centred plane is
    exactly 0), and it is >= 1 in nearly every bin of the checkerboard, the cosine and the smooth picture, whose energy sits in one or
    two bins: no kernel can make 'at most the last two bins exceed 1e-3' true.  So this test compares MORE than that rule would: every
    picture's every bin with ratio < 1 against its own derived tolerance, and gap_db on sets of white pictures (random bytes, the bright
    pixel), where only the one-point bins 0 and R - 1 may be skipped - which is asserted."""
    import metrics
    c = cases[S]
    B = c["B"]
    live = np.concatenate([c["x"][[0, 4]], R.pictures(1, S, 800 + S), R.pictures(1, S, 900 + S)])    # white spectra: random bytes, one bright pixel
    for n, plane, window in ((6, "luma", None), (7, "g", "hann")):
        x = c["x"][:n]
        host = metrics.spectrum(x, plane=plane, window=window, mean2d=True, chunk=4)
        dev = metrics.spectrum(torch.from_numpy(x).cuda(), plane=plane, window=window, mean2d=True, chunk=4)
        assert dev["profile"].shape == host["profile"].shape and np.array_equal(dev["mean"], host["mean"]) and np.array_equal(dev["count"], host["count"])
        count = host["count"].astype(np.float64)
        E = (host["profile"] * count).sum(axis=1)
        assert ((count * np.abs(dev["profile"] - host["profile"])).sum(axis=1) <= B * E * (1 + 1e-9)).all()
        assert np.abs(dev["mean2d"] - host["mean2d"]).sum() <= B * E.mean() * (1 + 1e-9)
        db_tol = lambda s: db_tolerance(B, s["profile"], count)
        t = db_tol(host)
        assert (np.abs(to_db(dev["profile"]) - to_db(host["profile"]))[np.isfinite(t)] <= t[np.isfinite(t)]).all() and np.isfinite(t).sum() >= count.shape[0]
        # the report on white pictures: set A on the device, set B on the host, against both on the host
        ha = metrics.spectrum(live, plane=plane, window=window, mean2d=True)
        da = metrics.spectrum(torch.from_numpy(live).cuda(), plane=plane, window=window, mean2d=True, chunk=3)
        hb = metrics.spectrum(live[::-1][:3].copy(), plane=plane, window=window, mean2d=True)
        want, got = metrics.spectrum_report(ha, hb), metrics.spectrum_report(da, hb)
        tol = db_tol(ha).mean(axis=0)
        skipped = np.nonzero(~np.isfinite(tol))[0]
        print(f"S={S} {plane} {window}: bins skipped {skipped.tolist()}, largest tolerance {tol[np.isfinite(tol)].max():.3g} dB")
        assert set(skipped.tolist()) <= {0, count.shape[0] - 1}
        keep = np.isfinite(tol)
        assert (np.abs(got["gap_db"] - want["gap_db"])[keep] <= tol[keep]).all()
        assert set(got) == set(want) and len(got["peaks"]) == 15 and np.isfinite(got["checkerboard_db"])


def test_sampler_spectrum_on_fresh_engines():
    from hipgan._lib import JckError
    from hipgan.engine import CganEngine, DcganEngine
    from hipgan.sampler import Sampler
    from oracle.gan_oracle import GanOracle
    keys = {"S", "plane", "window", "n_a", "n_b", "radius", "count", "mean_db_a", "std_db_a", "mean_db_b", "std_db_b", "gap_db", "z", "rms_gap_db",
            "high_gap_db", "worst", "separability", "peaks", "checkerboard_db", "mean2d_a", "mean2d_b", "n", "n_train", "seed"}
    train = np.random.default_rng(93).integers(0, 256, size=(24, 64, 64, 3), dtype=np.uint8)
    orc = GanOracle("dcgan", lr=2e-4, seed=12345)
    eng = DcganEngine(batch=8, prec="bf16")
    eng.load_state(orc.g, orc.d)
    gs, ds = eng.state_dicts()
    s = Sampler.from_checkpoint({"model_g": gs, "model_d": ds}, "DCGAN", batch=8)
    r = s.spectrum(train[:16], n=16, seed=3, window="hann")
    assert set(r) == keys and (r["n"], r["n_train"], r["seed"], r["S"], r["plane"], r["window"], r["n_a"], r["n_b"]) == (16, 16, 3, 64, "luma", "hann", 16, 16)
    for k in ("mean_db_a", "std_db_a", "mean_db_b", "std_db_b", "gap_db", "z"):
        assert r[k].shape == (46,) and np.isfinite(r[k]).all(), k
    assert r["mean2d_a"].shape == (64, 64) and np.isfinite(r["mean2d_a"]).all() and (r["mean2d_b"] > 0).all()
    assert len(r["peaks"]) == 15 and np.isfinite(r["checkerboard_db"]) and np.isfinite(r["rms_gap_db"]) and 0.0 <= r["separability"] <= 1.0
    with pytest.raises(JckError):
        s.spectrum(train, n=25)
    orc = GanOracle("cgan", lr=2e-4, seed=12345)
    eng = CganEngine(batch=8, prec="bf16")
    eng.load_state(orc.g, orc.d)
    gs, ds = eng.state_dicts()
    s = Sampler.from_checkpoint({"model_g": gs, "model_d": ds}, "CGAN", batch=8)
    train_labels = np.array([3, 17, 42] * 8)
    ids = torch.tensor([3, 17] * 6)
    r = s.spectrum(train, n=12, seed=1, labels=ids, train_labels=train_labels, classes=[3, 17], plane="g")
    assert set(r) == keys | {"per_class"} and set(r["per_class"]) == {3, 17} and r["plane"] == "g"
    for cid in (3, 17):
        pc = r["per_class"][cid]
        assert pc["n"] == 6 and pc["n_a"] == 6 and pc["n_b"] == 6 and pc["gap_db"].shape == (46,) and np.isfinite(pc["gap_db"]).all()
    with pytest.raises(JckError):
        s.spectrum(train, n=12, labels=ids, classes=[3])                                             # no train_labels
